"""Euclidean k-NN graphs with heat weights on one MI355X, beside torch and beside the fp64 fma rate of the GPU.

    timeout -k 10 1100 python tools/bench_nng.py [--out profiles/nng/bench.json] [--skip-rmat] [--repeats 5]

Three shapes:

  roll    LE.py's swiss roll (pointgraph.make_swiss_roll, height 100), 100,000 x 3, k = 10, t = 15, all sources;
  blog    BlogCatalog's shape (10,313 x 128), standard-normal fp32 rows from --seed, k = 20, all sources;
  rmat    the R-MAT-20 corpus' shape (646,323 x 128), likewise, a seeded sample of 65,536 sources, k = 20.

For each shape, on the same GPU:

  nng       gw_nng_query (fused squared distances, selection and weights; include_self), host clock around the
            call, which synchronises its stream; one warm-up call, then --repeats timed calls: median, min, max;
  torch     the same rows by a chunked torch.cdist in fp64 followed by torch.topk(k, largest=False) (the source
            itself among them, as include_self has it), chunks of --chunk sources; warm-up and repeats alike.
            torch.cdist takes the |a|^2 + |b|^2 - 2 a.b form through a matrix product at these sizes;
  fma       gw_knn_fma_rate: 16 independent fp64 fma chains per lane on every CU.

The record states one fused multiply-add per pair and column (sources x n x dim) per second and that as a share
of the calibrated fma rate; the subtract that precedes each fma is extra work per pair and column which the count
leaves out, so the share understates the arithmetic the kernel issues by up to a factor of two.  The neighbour
ids of the first 256 sources are compared with torch's as sets per row (a rate for wrong rows is no rate; the two
forms of the distance may order near-ties differently).

The first two shapes also time the whole eigenmaps_of_points call (neighbour graph, host assembly of S, solver,
export): --le-dim eigenpairs, min_eigenvalue 1e-9 (at 100,000 points the roll's first eigenvalues lie below the
default 1e-5); one warm-up, --le-repeats calls.

Not measured: per-kernel counters, other k, other dim.

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


def timed(fn, repeats):
    import torch
    fn()  # warm-up
    t = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append(time.perf_counter() - t0)
    return {"median_s": round(statistics.median(t), 5), "min_s": round(min(t), 5), "max_s": round(max(t), 5),
            "repeats": repeats}


def torch_topk(x, src, k, chunk):
    """ids [nsrc][k] by fp64 cdist + topk of the smallest, the source itself among them."""
    import torch
    xd = x.double()
    out = torch.empty((len(src), k), dtype=torch.int64, device=x.device)
    for b in range(0, len(src), chunk):
        d = torch.cdist(xd[src[b:b + chunk]], xd)
        out[b:b + chunk] = torch.topk(d, k, dim=1, largest=False).indices
    return out


def shape(P, name, x, nsrc, k, t, a):
    import torch
    from gwamd import _lib as C
    n, d = x.shape
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(a.seed + 1)
    if nsrc < n:
        src = torch.randperm(n, device="cuda:0", generator=gen)[:nsrc].to(torch.int32)
    else:
        src = torch.arange(n, device="cuda:0", dtype=torch.int32)
    m = P.PointGraph(n, device=0, dim=d, topk=k, include_self=True, heat_t=t)
    m.set_vectors(x)
    ids = torch.empty((nsrc, k), dtype=torch.int32, device="cuda:0")
    w = torch.empty((nsrc, k), dtype=torch.float64, device="cuda:0")

    def nng():
        C.check(C.lib().gw_nng_query(m.handle, C.ptr(src), nsrc, C.ptr(ids), C.ptr(w), None, None), nng=m.handle)

    res = {"n": n, "dim": d, "sources": nsrc, "k": k, "heat_t": t, "fma": float(nsrc) * n * d}
    res["nng"] = timed(nng, a.repeats)
    print(name, "nng", res["nng"], file=sys.stderr, flush=True)
    src64 = src.long()
    res["torch_cdist_fp64"] = timed(lambda: torch_topk(x, src64, k, a.chunk), a.repeats)
    print(name, "torch", res["torch_cdist_fp64"], file=sys.stderr, flush=True)
    ref = torch_topk(x, src64[:256], k, a.chunk).sort(dim=1).values
    res["id_sets_equal_torch_first_256"] = bool((ref == ids[:256].long().sort(dim=1).values).all().item())
    rate = res["fma"] / res["nng"]["median_s"]
    res["fma_per_s"] = rate
    res["share_of_fma_rate"] = round(rate / a.fma_rate, 4)
    res["torch_over_nng"] = round(res["torch_cdist_fp64"]["median_s"] / res["nng"]["median_s"], 3)
    m.free()
    return res


def whole(E, x, k, t, a):
    """The whole eigenmaps_of_points call; a failure (a state, a capacity error) is recorded, not raised."""
    last = {}

    def call():
        emb = E.eigenmaps_of_points(x, k, t, dim=a.le_dim, device=0, min_eigenvalue=1e-9)
        st = emb.stats
        last.update(state=E.STATES[st.state], iters=st.iters, applies=int(st.applies), skipped=st.skipped,
                    isolated=int(st.isolated), max_residual=st.max_residual, first_eigenvalues=[float(v) for v in
                                                                                                 emb.eigenvalues[:2]])
        emb.model.free()
    try:
        res = timed(call, a.le_repeats)
    except Exception as e:  # noqa: BLE001 - recorded
        return {"error": type(e).__name__ + ": " + str(e)}
    return dict(res, dim=a.le_dim, **last)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=2048, help="sources per torch.cdist")
    ap.add_argument("--roll-n", type=int, default=100000)
    ap.add_argument("--rmat-n", type=int, default=646323)
    ap.add_argument("--rmat-sources", type=int, default=65536)
    ap.add_argument("--skip-rmat", action="store_true")
    ap.add_argument("--skip-le", action="store_true")
    ap.add_argument("--le-dim", type=int, default=2)
    ap.add_argument("--le-repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    from gwamd import eigenmaps as E
    from gwamd import neighbors as N
    from gwamd import pointgraph as P
    if not torch.cuda.is_available():
        raise SystemExit("bench_nng.py needs a GPU (there is no CPU fallback for a rate)")
    m = N.Neighbors(4, device=0, dim=128, topk=20)
    rates = [m.fma_rate() for _ in range(a.repeats)]
    m.free()
    g = P.PointGraph(4, device=0, dim=128, topk=20)
    res = {"fma_rate": {"median_per_s": statistics.median(rates), "min_per_s": min(rates), "max_per_s": max(rates)},
           "tiles": g.tiles(), "kernel_attrs": g.kernel_attrs()}
    g.free()
    a.fma_rate = res["fma_rate"]["median_per_s"]
    print("fma rate", res["fma_rate"], file=sys.stderr, flush=True)
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(a.seed)
    roll = torch.as_tensor(P.make_swiss_roll(a.roll_n, seed=a.seed)[0].astype(np.float32), device="cuda:0")
    res["roll"] = shape(P, "roll", roll, a.roll_n, 10, 15.0, a)
    blog = torch.randn((10313, 128), device="cuda:0", generator=gen)
    res["blog"] = shape(P, "blog", blog, 10313, 20, 2.0 * 128, a)
    if not a.skip_le:
        res["roll"]["eigenmaps_of_points"] = whole(E, roll, 10, 15.0, a)
        print("roll eigenmaps", res["roll"]["eigenmaps_of_points"], file=sys.stderr, flush=True)
        res["blog"]["eigenmaps_of_points"] = whole(E, blog, 20, 2.0 * 128, a)
        print("blog eigenmaps", res["blog"]["eigenmaps_of_points"], file=sys.stderr, flush=True)
    if not a.skip_rmat:
        x = torch.randn((a.rmat_n, 128), device="cuda:0", generator=gen)
        res["rmat"] = shape(P, "rmat", x, a.rmat_sources, 20, 2.0 * 128, a)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
