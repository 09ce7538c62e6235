"""Laplacian eigenmaps (dim 128) on one MI355X, beside the dense recipe on the same GPU and ARPACK on the host.

    timeout -k 10 1100 python tools/bench_le.py [--out profiles/le/bench.json] [--skip-rmat] [--repeats 5]

Two shapes:

  blog    BlogCatalog's own adjacency (tests/golden/data/blog.txt, 10,313 rows), solved to tol 1e-8;
  rmat    gw_graph_rmat at scale 20 (646,323 rows with an edge), nothing skipped (its small components give more
          zero eigenvalues than a block holds), at most --rmat-max-iters Rayleigh-Ritz steps: the record says
          whether it converged.

Per shape: one warm-up gw_le_solve, then --repeats timed ones (host clock around the call, which synchronises
its stream): median, min, max, with iterations and operator applications.  Then, on the solver's own buffers and
with device events, the mean of --kernel-reps launches of

  apply     k_le_apply with the Chebyshev combine: achieved bytes/s against its algorithmic bytes
            nnz * m * 8 + 3 * n * m * 8 per application;
  gram      k_le_gram + k_le_gram_reduce: n * m * (m + 1) / 2 fma (the upper triangle);
  rotate    k_le_rotate: n * m * m fma;

the fma rates beside gw_knn_fma_rate measured in the same run.

Baselines (blog only): torch.linalg.eigh in fp64 of the dense I - S on the same GPU (what the reference's dense
recipe costs there; its eigenvalues check ours) and scipy.sparse.linalg.eigsh on the host where scipy is installed.

Prints one JSON line (and writes it to --out).
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graph-embedding_amd"))


def dense_s(csr, n):
    """S = D^-1/2 W D^-1/2 of an unweighted symmetric CSR as (scipy-free) COO arrays and the degrees."""
    off, nb = csr["offsets"], csr["nbrs"]
    rows = np.repeat(np.arange(n), np.diff(off))
    keep = rows != nb
    rows, cols = rows[keep], nb[keep]
    d = np.bincount(rows, minlength=n).astype(np.float64)
    with np.errstate(divide="ignore"):
        s = np.where(d > 0, 1 / np.sqrt(d), 0.0)
    return rows, cols, s[rows] * s[cols], d


def solve_shape(E, name, g, a, **kw):
    import torch
    csr = g.export_csr()
    n = len(csr["offsets"]) - 1
    m = E.Eigenmaps(n, device=0, dim=a.dim, **kw)
    m.set_csr(csr["offsets"], csr["nbrs"])
    st = m.solve()  # warm-up
    t = []
    for _ in range(a.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        st = m.solve()
        torch.cuda.synchronize()
        t.append(time.perf_counter() - t0)
    lam, _, res = m.export()
    mb = st.block_used
    nnz = int(m_nnz(csr))
    out = {"n": n, "isolated": int(st.isolated), "nnz_offered": nnz, "dim": a.dim, "block": mb,
           "solve": {"median_s": round(statistics.median(t), 4), "min_s": round(min(t), 4), "max_s": round(max(t), 4),
                     "repeats": a.repeats},
           "state": E.STATES[st.state], "iters": st.iters, "applies": int(st.applies), "skipped": st.skipped,
           "max_residual": st.max_residual, "eigenvalues_first_4": [float(x) for x in lam[:4]]}
    print(name, out, file=sys.stderr, flush=True)
    ms = {k: m.time_kernel(k, a.kernel_reps) for k in ("apply", "gram", "rotate")}
    bytes_apply = nnz * mb * 8 + 3 * n * mb * 8
    out["kernels"] = {
        "apply": {"ms": ms["apply"], "algorithmic_bytes": bytes_apply, "bytes_per_s": bytes_apply / (ms["apply"] * 1e-3)},
        "gram": {"ms": ms["gram"], "fma": n * mb * (mb + 1) // 2,
                 "fma_per_s": n * mb * (mb + 1) / 2 / (ms["gram"] * 1e-3)},
        "rotate": {"ms": ms["rotate"], "fma": n * mb * mb, "fma_per_s": n * mb * mb / (ms["rotate"] * 1e-3)}}
    for k in ("gram", "rotate"):
        out["kernels"][k]["share_of_fma_rate"] = round(out["kernels"][k]["fma_per_s"] / a.fma_rate, 4)
    print(name, out["kernels"], file=sys.stderr, flush=True)
    m.free()
    return out, csr, lam


def m_nnz(csr):
    off, nb = csr["offsets"], csr["nbrs"]
    rows = np.repeat(np.arange(len(off) - 1), np.diff(off))
    return (rows != nb).sum()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--kernel-reps", type=int, default=10)
    ap.add_argument("--rmat-scale", type=int, default=20)
    ap.add_argument("--rmat-max-iters", type=int, default=12)
    ap.add_argument("--skip-rmat", action="store_true")
    ap.add_argument("--skip-dense", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    from gwamd import GWGraph, eigenmaps as E, neighbors as N
    if not torch.cuda.is_available():
        raise SystemExit("bench_le.py needs a GPU (there is no CPU fallback for a rate)")
    k = N.Neighbors(4, device=0, dim=128, topk=20)
    a.fma_rate = statistics.median(k.fma_rate() for _ in range(3))
    k.free()
    probe = E.Eigenmaps(4, device=0, dim=1, block=2)
    res = {"fma_rate_per_s": a.fma_rate, "tiles": probe.tiles(), "kernel_attrs": probe.kernel_attrs()}
    probe.free()
    g = GWGraph.from_edgelist(os.path.join(ROOT, "tests", "golden", "data", "blog.txt"), ",")
    res["blog"], csr, lam = solve_shape(E, "blog", g, a)
    n = len(csr["offsets"]) - 1
    rows, cols, vals, d = dense_s(csr, n)
    skipped = res["blog"]["skipped"]
    if not a.skip_dense:
        def dense():
            S = torch.zeros((n, n), dtype=torch.float64, device="cuda:0")
            S[torch.as_tensor(rows, device="cuda:0"), torch.as_tensor(cols, device="cuda:0")] = \
                torch.as_tensor(vals, device="cuda:0")
            return torch.linalg.eigh(torch.eye(n, dtype=torch.float64, device="cuda:0") - S)[0]
        dense()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ref = dense()
        torch.cuda.synchronize()
        ref = ref.cpu().numpy()
        ref = ref[int((d == 0).sum()):]  # an isolated row of the dense matrix is an eigenvalue 1; blog has none
        res["blog"]["torch_eigh_fp64"] = {"s": round(time.perf_counter() - t0, 4),
                                          "max_eigenvalue_difference": float(np.abs(ref[skipped:skipped + a.dim] - lam).max())}
        res["blog"]["torch_eigh_over_solve"] = round(res["blog"]["torch_eigh_fp64"]["s"] / res["blog"]["solve"]["median_s"], 2)
        print("blog torch", res["blog"]["torch_eigh_fp64"], file=sys.stderr, flush=True)
    try:
        import scipy.sparse as sp
        from scipy.sparse.linalg import eigsh
        S = sp.csr_matrix((vals, (rows, cols)), shape=(n, n))
        t0 = time.perf_counter()
        w = eigsh(S, k=a.dim + skipped, which="LA", tol=1e-8, return_eigenvectors=True)[0]
        res["blog"]["scipy_eigsh_host"] = {"s": round(time.perf_counter() - t0, 4),
                                           "max_eigenvalue_difference":
                                               float(np.abs(np.sort(1 - w)[skipped:skipped + a.dim] - lam).max())}
        print("blog scipy", res["blog"]["scipy_eigsh_host"], file=sys.stderr, flush=True)
    except ImportError:
        res["blog"]["scipy_eigsh_host"] = "scipy is not installed"
    if not a.skip_rmat:
        g = GWGraph.rmat(a.rmat_scale)
        res["rmat"], _, _ = solve_shape(E, "rmat", g, a, min_eigenvalue=-1.0, max_iters=a.rmat_max_iters)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
