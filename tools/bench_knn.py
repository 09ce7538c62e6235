"""All-pairs top-20 cosine neighbours on one MI355X, beside torch and beside the fp64 fma rate of the GPU.

    timeout -k 10 1100 python tools/bench_knn.py [--out profiles/knn/bench.json] [--skip-rmat] [--repeats 5]

Two shapes, both standard-normal fp32 rows generated on the GPU from --seed:

  blog    BlogCatalog's shape (10,313 x 128), all sources;
  rmat    the R-MAT-20 corpus' shape (646,323 x 128), a seeded sample of 65,536 sources.

For each shape, on the same GPU:

  knn       gw_knn_query (norms + fused scores and selection), host clock around the call, which
            synchronises its stream; one warm-up call, then --repeats timed calls: median, min, max;
  torch     the same rows by a chunked torch.matmul in fp64 followed by torch.topk(k + 1) (the source
            itself still among them), chunks of --chunk sources; warm-up and repeats alike;
  fma       gw_knn_fma_rate: 16 independent fp64 fma chains per lane on every CU, the ceiling of the
            main loop's arithmetic.

The record states the fused multiply-adds of the algorithm (sources x n x dim) per second, that as a
share of the calibrated fma rate, and the ratio to the torch baseline.  The neighbour ids of the first
256 sources are compared with torch's (a rate for wrong rows is no rate).

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
    """ids [nsrc][k] by fp64 matmul + topk, the source dropped from its own row."""
    import torch
    xd = x.double()
    xn = xd / xd.norm(dim=1, keepdim=True)
    out = torch.empty((len(src), k), dtype=torch.int64, device=x.device)
    for b in range(0, len(src), chunk):
        s = src[b:b + chunk]
        sc = xn[s] @ xn.T
        sc[torch.arange(len(s), device=x.device), s] = -float("inf")
        out[b:b + chunk] = torch.topk(sc, k, dim=1).indices
    return out


def shape(N, name, n, d, nsrc, a):
    import torch
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(a.seed)
    x = torch.randn((n, d), device="cuda:0", generator=gen)
    if nsrc < n:
        src = torch.randperm(n, device="cuda:0", generator=gen)[:nsrc].to(torch.int32)
    else:
        src = torch.arange(n, device="cuda:0", dtype=torch.int32)
    m = N.Neighbors(n, device=0, dim=d, topk=a.topk)
    m.set_vectors(x)
    ids = torch.empty((nsrc, a.topk), dtype=torch.int32, device="cuda:0")
    sc = torch.empty((nsrc, a.topk), dtype=torch.float64, device="cuda:0")
    from gwamd import _lib as C

    def knn():
        C.check(C.lib().gw_knn_query(m.handle, C.ptr(src), nsrc, C.ptr(ids), C.ptr(sc), None), knn=m.handle)

    res = {"n": n, "dim": d, "sources": nsrc, "topk": a.topk, "fma": float(nsrc) * n * d}
    res["knn"] = timed(knn, a.repeats)
    print(name, "knn", res["knn"], file=sys.stderr, flush=True)
    src64 = src.long()
    res["torch_fp64"] = timed(lambda: torch_topk(x, src64, a.topk, a.chunk), a.repeats)
    print(name, "torch", res["torch_fp64"], file=sys.stderr, flush=True)
    ref = torch_topk(x, src64[:256], a.topk, a.chunk)
    res["ids_equal_torch_first_256"] = bool((ref == ids[:256].long()).all().item())
    rate = res["fma"] / res["knn"]["median_s"]
    res["fma_per_s"] = rate
    res["share_of_fma_rate"] = round(rate / a.fma_rate, 4)
    res["torch_over_knn"] = round(res["torch_fp64"]["median_s"] / res["knn"]["median_s"], 3)
    m.free()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--topk", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=2048, help="sources per torch.matmul")
    ap.add_argument("--rmat-n", type=int, default=646323)
    ap.add_argument("--rmat-sources", type=int, default=65536)
    ap.add_argument("--skip-rmat", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    from gwamd import neighbors as N
    if not torch.cuda.is_available():
        raise SystemExit("bench_knn.py needs a GPU (there is no CPU fallback for a rate)")
    m = N.Neighbors(4, device=0, dim=128, topk=a.topk)
    rates = [m.fma_rate() for _ in range(a.repeats)]
    res = {"fma_rate": {"median_per_s": statistics.median(rates), "min_per_s": min(rates), "max_per_s": max(rates)},
           "tiles": m.tiles(), "kernel_attrs": m.kernel_attrs()}
    m.free()
    a.fma_rate = res["fma_rate"]["median_per_s"]
    print("fma rate", res["fma_rate"], file=sys.stderr, flush=True)
    res["blog"] = shape(N, "blog", 10313, 128, 10313, a)
    if not a.skip_rmat:
        res["rmat"] = shape(N, "rmat", a.rmat_n, 128, a.rmat_sources, a)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
