"""CPU: points -> neighbour graph -> Laplacian eigenmap on the host (gw_nng -> gw_le with self_loops, device = -1):
the reference's own spectra (tests/golden/le_points_*.npz, written by tools/gen_le_points_golden.py from
IsoMap_LE/LE.py laplaEigen), the self_loops rule of gw_le against dense numpy, the swiss roll, the command line.
"""
import ctypes

import numpy as np
import pytest

from conftest import load_golden

FIXTURES = ["le_points_circle12.npz", "le_points_lattice8x6.npz"]


def _E():
    from gwamd import _lib as C
    from gwamd import eigenmaps
    C.lib()
    return eigenmaps


def golden_case(name):
    """(points, k, t, the reference's eigenvalues above 1e-5 ascending, how many it has at or below)."""
    g = load_golden(name)
    assert g["max_imag"] == 0.0 and g["asymmetry"] == 0
    ref = g["eigenvalues"]
    return g["x"], int(g["k"]), float(g["t"]), ref[ref > 1e-5], int((ref <= 1e-5).sum())


def roll():
    """The issue's swiss roll: n = 600, RandomState(1), height 20, as float32 points with the roll parameter."""
    from gwamd import pointgraph
    X, t = pointgraph.make_swiss_roll(600, seed=1, height=20.0)
    return X.astype(np.float32), t


def spearman(a, b):
    ra, rb = np.argsort(np.argsort(a)).astype(np.float64), np.argsort(np.argsort(b)).astype(np.float64)
    return float(np.corrcoef(ra, rb)[0, 1])


# ---- 1: the reference's spectra -----------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_golden_spectrum_through_laplaEigen(name):
    """Every eigenvalue of LE.py's D^-1 L above min_eigenvalue, within 1e-10.  S is symmetric, so a Ritz value lies
    within its residual (<= tol = 1e-12) of an eigenvalue; the rest is the ulp-level difference between the project's
    exp and libm's and np.linalg.eig's own rounding.  Measured: 3.1e-14 (circle), 4.0e-15 (lattice)."""
    E = _E()
    x, k, t, ref, zeros = golden_case(name)
    n = len(x)
    lam, f = E.laplaEigen(x, k, t, dim=len(ref), device=-1, block=n, tol=1e-12)
    err = np.abs(lam - ref).max()
    print(f"{name}: n {n}, {len(ref)} eigenvalues compared, {zeros} skipped, max |difference| {err:.2e}")
    assert lam.shape == (len(ref),) and f.shape == (n, len(ref))
    assert err <= 1e-10
    emb = E.eigenmaps_of_points(x, k, t, dim=len(ref), device=-1, block=n, tol=1e-12)
    assert emb.stats.state == 0 and emb.stats.skipped == zeros and emb.stats.isolated == 0
    assert np.array_equal(emb.eigenvalues, lam)
    # the pairs are D^-1 L's: (D - W) f = lambda D f on the symmetric W the reference built
    from gwamd import pointgraph
    ids, w = pointgraph.knn_graph(x, k, t, device=-1)
    W = np.zeros((n, n))
    for i in range(n):
        W[i, ids[i]] = w[i]
    assert np.array_equal(W, W.T) and (np.diag(W) == 1.0).all()
    D = np.diag(W.sum(1))
    assert np.abs((D - W) @ f - (D @ f) * lam).max() <= 1e-11


# ---- 2: self_loops in gw_le -------------------------------------------------------------------------------
def loop_rows(n=40, topk=6, seed=2):
    """Random symmetric weights with a diagonal, as rows: every row lists itself and some others; row 5 lists itself
    alone; row 9 lists nothing (isolated)."""
    rng = np.random.default_rng(seed)
    A = np.triu(rng.uniform(0.05, 1.0, (n, n)) * (rng.random((n, n)) < 0.12), 1)
    A = A + A.T + np.diag(rng.uniform(0.1, 1.0, n))
    A[5, :] = A[:, 5] = 0.0
    A[5, 5] = 0.7
    A[9, :] = A[:, 9] = 0.0
    width = int((A > 0).sum(1).max())
    ids = np.full((n, width), -1, np.int32)
    sc = np.zeros((n, width))
    for i in range(n):
        nz = np.nonzero(A[i])[0][::-1]          # any order within a row
        ids[i, :len(nz)] = nz
        sc[i, :len(nz)] = A[i, nz]
    return A, ids, sc


def test_self_loops_against_dense_eig():
    E = _E()
    A, ids, sc = loop_rows()
    n = len(A)
    alive = A.sum(1) > 0
    d = A.sum(1)[alive]
    M = np.diag(1.0 / d) @ (np.diag(d) - A[np.ix_(alive, alive)])        # D^-1 (D - W), W with its diagonal
    ref = np.sort(np.linalg.eigvals(M).real)
    # row 5 is a component of its own (its self-loop alone: S_55 = 1, lambda = 0), so two eigenvalues are ~0
    assert (ref <= 1e-5).sum() >= 2
    want = ref[ref > 1e-5]
    m = E.Eigenmaps(n, device=-1, dim=len(want), block=n, tol=1e-12, self_loops=1)
    m.set_rows(ids, sc)
    st = m.solve()
    lam, vec, res = m.export()
    assert st.state == 0 and st.isolated == 1 and st.skipped == (ref <= 1e-5).sum()
    assert np.abs(lam - want).max() <= 1e-10
    assert (vec[9] == 0).all()
    S = m.apply(np.eye(n))
    m.free()
    dd = A.sum(1)
    s = np.where(dd > 0, 1.0 / np.sqrt(np.where(dd > 0, dd, 1.0)), 0.0)
    assert np.abs(S - A * s[:, None] * s[None, :]).max() <= 4e-16 and abs(S[5, 5] - 1.0) <= 4e-16
    assert np.abs(np.linalg.eigvalsh(S)).max() <= 1.0 + 1e-15                # the spectrum stays within [-1, 1]


@pytest.mark.parametrize("sym", ["mean", "max"])
def test_self_loops_off_equals_the_rows_without_their_self_entries(sym):
    E = _E()
    A, ids, sc = loop_rows()
    n = len(A)
    stripped_ids, stripped_sc = np.full_like(ids, -1), np.zeros_like(sc)
    for i in range(n):
        keep = [e for e in range(ids.shape[1]) if ids[i, e] >= 0 and ids[i, e] != i]
        stripped_ids[i, :len(keep)] = ids[i, keep]
        stripped_sc[i, :len(keep)] = sc[i, keep]
    out = []
    for a, b, kw in ((ids, sc, dict(self_loops=0)), (ids, sc, dict()), (stripped_ids, stripped_sc, dict(self_loops=0)),
                     (stripped_ids, stripped_sc, dict(self_loops=1))):
        m = E.Eigenmaps(n, device=-1, dim=4, block=12, symmetrize=sym, seed=3, **kw)
        m.set_rows(a, b)
        st = m.solve()
        out.append(tuple(x.tobytes() for x in m.export()) + (m.vectors_numpy().tobytes(), st.iters, st.applies, st.isolated))
        m.free()
    assert out[0] == out[1] == out[2] == out[3]
    assert out[0][-1] == 2                                                   # rows 5 and 9 are isolated without loops


def test_struct_size_before_self_loops_keeps_todays_law():
    from gwamd import _lib as C
    E = _E()
    A, ids, sc = loop_rows()
    n = len(A)
    L = C.lib()
    p = C.LeParams(dim=4, block=12, seed=3, self_loops=1)
    assert C.LeParams.self_loops.offset == 48 and ctypes.sizeof(C.LeParams) == 56
    p.struct_size = 48                       # the struct as it was before the field
    h = ctypes.c_void_p()
    assert L.gw_le_create(-1, n, ctypes.byref(p), ctypes.byref(h)) == C.GW_OK
    assert L.gw_le_set_rows(h, C.ptr(ids), C.ptr(sc), ids.shape[1]) == C.GW_OK
    st = C.LeStats()
    assert L.gw_le_solve(h, ctypes.byref(st), None) == C.GW_OK
    lam = np.empty(4)
    assert L.gw_le_export(h, C.ptr(lam), None, None) == C.GW_OK
    L.gw_le_free(h)
    m = E.Eigenmaps(n, device=-1, dim=4, block=12, seed=3)
    m.set_rows(ids, sc)
    m.solve()
    assert np.array_equal(lam, m.export()[0]) and st.isolated == 2
    m.free()
    for bad in (2, -1):
        p = C.LeParams(dim=4, block=12, self_loops=bad)
        assert L.gw_le_create(-1, n, ctypes.byref(p), ctypes.byref(h)) == C.GW_ERR_INVALID


# ---- 3: the swiss roll ---------------------------------------------------------------------------------------
def test_swiss_roll_unrolls():
    """n = 600, RandomState(1), height 20, k = 10, t = 15, dim = 2: the first eigenvector follows the roll
    parameter (a dense scipy eigh of the same symmetrised matrix gives |rho| = 0.999, lambda 8.9e-4 and 3.5e-3)."""
    E = _E()
    x, t = roll()
    emb = E.eigenmaps_of_points(x, 10, 15.0, dim=2, device=-1)
    rho = abs(spearman(emb.vectors64[:, 0], t))
    print(f"swiss roll: {emb.stats.iters} iterations, lambda {emb.eigenvalues}, |Spearman rho| {rho:.4f}")
    assert emb.stats.state == 0                       # converged
    assert emb.stats.skipped == 1
    assert rho >= 0.99
    lam, f = E.laplaEigen(x, 10, 15.0, device=-1)
    assert np.array_equal(lam, emb.eigenvalues) and np.array_equal(f, emb.vectors64)


# ---- 4: the command line ---------------------------------------------------------------------------------------
def test_cli_with_points(tmp_path, capsys):
    from gwamd import classify
    E = _E()
    x, t = roll()
    x = x[:200]
    np.save(tmp_path / "x.npy", x)
    out = str(tmp_path / "x.emb")
    assert E.cli(["--points", str(tmp_path / "x.npy"), "--knn", "8", "--heat", "15.0", "--output", out, "--dimensions", "3",
                  "--device", "-1"]) == 0
    err = capsys.readouterr().err
    assert "200 x 3 eigenmap" in err and "converged" in err
    labels, X = classify.read_embedding(out)
    emb = E.eigenmaps_of_points(x, 8, 15.0, dim=3, device=-1)
    assert labels == [str(i) for i in range(200)] and np.array_equal(np.asarray(X, np.float32), emb.vectors)
    assert E.cli(["--points", str(tmp_path / "x.npy"), "--knn", "8", "--heat", "15.0", "--no-self", "--output", out,
                  "--dimensions", "3", "--device", "-1"]) == 0
    capsys.readouterr()
    _, X2 = classify.read_embedding(out)
    noself = E.eigenmaps_of_points(x, 8, 15.0, dim=3, device=-1, include_self=False)
    assert np.array_equal(np.asarray(X2, np.float32), noself.vectors) and not np.array_equal(X2, X)
    with pytest.raises(SystemExit):
        E.cli(["--points", str(tmp_path / "x.npy"), "--input", "e.txt", "--output", out])
    capsys.readouterr()
