"""Golden spectra of the reference's point-cloud eigenmap (IsoMap_LE/LE.py laplaEigen).

    python tools/gen_le_points_golden.py REFERENCE_ROOT

Runs only where the reference tree is at hand; the tests read the .npz files it writes into
tests/golden/ and never this script.  LE.py is imported as it is, with three shims on this side:
np.math (gone from numpy 2), np.mat (likewise) and a matplotlib backend that opens no window.
No reference file is touched.

Each fixture holds: x float32 [n][d] (the points; the reference is run on their float64 widening,
so both sides read the same numbers), k, t, and `eigenvalues`: the real parts of laplaEigen's n
eigenvalues, ascending, with `max_imag` the largest imaginary part seen (0 for both inputs) and
`asymmetry`, the number of entries where W's pattern differs from its transpose's (0 for both:
these are inputs whose k-NN graph the reference itself leaves symmetric, so the project's
symmetrised W is the same matrix).
"""
import importlib.util
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_reference(ref_root):
    os.environ.setdefault("MPLBACKEND", "Agg")
    if not hasattr(np, "math"):
        np.math = math
    if not hasattr(np, "mat"):
        np.mat = np.asmatrix
    spec = importlib.util.spec_from_file_location("ref_LE", os.path.join(ref_root, "IsoMap_LE", "LE.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def circle():
    a = 2.0 * np.pi * np.arange(12) / 12.0
    return np.stack([np.cos(a), np.sin(a)], axis=1), 3, 0.5


def lattice():
    a = 2.0 * np.pi * np.arange(8) / 8.0
    b = 2.0 * np.pi * np.arange(6) / 6.0
    A, B = np.meshgrid(a, b, indexing="ij")
    A, B = A.reshape(-1), B.reshape(-1)
    return np.stack([np.cos(A), np.sin(A), 1.5 * np.cos(B), 1.5 * np.sin(B)], axis=1), 5, 2.0


def main(ref_root):
    LE = load_reference(ref_root)
    for name, make in (("le_points_circle12.npz", circle), ("le_points_lattice8x6.npz", lattice)):
        pts, k, t = make()
        x = pts.astype(np.float32)
        wide = x.astype(np.float64)
        lam, _ = LE.laplaEigen(wide, k, t)
        lam = np.asarray(lam).reshape(-1)
        # the pattern the reference used, for the record: self first in every row, and symmetric
        pat = np.zeros((len(x), len(x)), bool)
        for i in range(len(x)):
            idx = np.asarray(LE.knn(wide[i, :], wide, k)).reshape(-1)
            assert idx[0] == i, (name, i, idx)
            pat[i, idx] = True
        out = os.path.join(ROOT, "tests", "golden", name)
        np.savez(out, x=x, k=np.int64(k), t=np.float64(t), eigenvalues=np.sort(lam.real),
                 max_imag=np.float64(np.abs(lam.imag).max()), asymmetry=np.int64((pat != pat.T).sum()))
        print(f"{out}: n {len(x)}, k {k}, t {t}, lambda in [{lam.real.min():.3e}, {lam.real.max():.6f}], "
              f"max |imag| {np.abs(lam.imag).max():.1e}, asymmetry {(pat != pat.T).sum()}")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
