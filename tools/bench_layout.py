"""Spring layout at two shapes: writes profiles/layout/bench.json.

    python tools/bench_layout.py [--out profiles/layout/bench.json] [--reps 5] [--nx-iterations 2]

  blog        BlogCatalog's shape: the 10,312 vertices and the edges of tests/golden/data/blog.txt, 50 iterations
  swiss_100k  the 10-nearest-neighbour graph of a 100,000-point swiss roll (values 1), 50 iterations

Each device run is timed with stream events around gw_layout_run (threshold 0: all 50 iterations are computed), the
median of `reps` after one warm-up.  Beside it at blog's shape: the same law in eager torch fp64 on the same GPU (dense
n x n temporaries; a few iterations timed, scaled to 50) and networkx's spring_layout on the host (`nx-iterations`
iterations timed, scaled to 50 and marked extrapolated; above 500 vertices networkx runs its float32 row loop).  Pair
evaluations per second stand beside the fp64 fma rate gw_knn_fma_rate measures in the same process.
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


def device_runs(m, pos, reps, iterations=50):
    import torch
    ts = []
    for r in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        p = torch.as_tensor(pos, device="cuda:0")
        a.record()
        done = m.run(p, iterations=iterations, threshold=0.0)
        b.record()
        b.synchronize()
        assert done == iterations
        if r:
            ts.append(a.elapsed_time(b) * 1e-3)
    return statistics.median(ts), ts


def torch_law(pos, off, nb, val, k, iterations):
    """The same law in eager torch fp64 (dense all-pairs temporaries, the attraction by index_add): seconds per
    iteration by stream events, after one untimed iteration."""
    import torch
    dev = "cuda:0"
    pos = torch.as_tensor(pos, device=dev)
    n = len(pos)
    rows = torch.repeat_interleave(torch.arange(n, device=dev), torch.as_tensor(np.diff(off), device=dev))
    cols = torch.as_tensor(nb.astype(np.int64), device=dev)
    a = torch.as_tensor(val, device=dev)
    t = 0.1 * float(max(pos[:, 0].max() - pos[:, 0].min(), pos[:, 1].max() - pos[:, 1].min()))
    dt = t / 51

    def one(pos, t):
        delta = pos[:, None, :] - pos[None, :, :]
        d2 = (delta * delta).sum(-1).clamp_(min=1e-4)
        disp = (delta * (k * k / d2)[:, :, None]).sum(1)
        de = pos[rows] - pos[cols]
        w = a * de.norm(dim=1).clamp_(min=0.01) / k
        disp.index_add_(0, rows, -de * w[:, None])
        length = disp.norm(dim=1)
        length = torch.where(length < 0.01, torch.full_like(length, 0.1), length)
        return pos + disp * (t / length)[:, None]

    pos = one(pos, t)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iterations):
        t -= dt
        pos = one(pos, t)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / iterations


def blog(reps, nx_iterations):
    from gwamd import layout
    from gwamd.graph import GWGraph
    G = GWGraph.from_edgelist(os.path.join(ROOT, "tests", "golden", "data", "blog.txt"), ",", "nx")
    nodes, off, nb, val = layout.graph_csr(G)
    n = len(nodes)
    pos = np.random.RandomState(0).rand(n, 2)
    m = layout.SpringLayout(n, device=0)
    m.set_csr(off, nb, val)
    med, ts = device_runs(m, pos, reps)
    r = {"n": n, "entries": int(off[-1]), "max_row": int(np.diff(off).max()), "iterations": 50, "dim": 2,
         "run_s_median": med, "run_s_all": ts, "pairs_per_s": 50.0 * n * n / med, "tiles": m.tiles(),
         "kernel_attrs": m.kernel_attrs()}
    h = layout.SpringLayout(n, device=-1)
    h.set_csr(off, nb, val)
    t = time.perf_counter()
    h.run(pos, iterations=5, threshold=0.0)
    r["host_openmp_s_extrapolated_from_5_iterations"] = (time.perf_counter() - t) * 10
    r["host_openmp_threads"] = int(os.environ.get("OMP_NUM_THREADS", "0")) or os.cpu_count()
    m.run(pos, iterations=5, threshold=0.0)
    r["bitwise_equal_to_host_after_5_iterations"] = bool(np.array_equal(m.positions_numpy().view(np.int64),
                                                                        h.positions_numpy().view(np.int64)))
    m.free()
    h.free()
    per = torch_law(pos, off, nb, val, float(np.sqrt(1.0 / n)), 5)
    r["eager_torch_fp64_s_extrapolated_from_5_iterations"] = per * 50
    r["speedup_over_eager_torch"] = per * 50 / med
    try:
        import networkx as nx
        import scipy  # noqa: F401 - networkx's path above 500 vertices needs it
        Gn = nx.Graph()
        Gn.add_nodes_from(nodes)
        rows = np.repeat(np.arange(n), np.diff(off))
        Gn.add_edges_from((nodes[i], nodes[j]) for i, j in zip(rows, nb) if i < j)
        t = time.perf_counter()
        nx.spring_layout(Gn, seed=0, iterations=nx_iterations, threshold=0.0)
        dt = time.perf_counter() - t
        r["networkx_s_extrapolated"] = dt * 50 / nx_iterations
        r["networkx_iterations_timed"] = nx_iterations
        r["networkx_version"] = nx.__version__
        r["speedup_over_networkx_extrapolated"] = r["networkx_s_extrapolated"] / med
    except ImportError as e:
        r["networkx_s_extrapolated"] = None
        r["networkx_missing"] = str(e)
    return r


def swiss(n, reps):
    from gwamd import layout, pointgraph
    X = pointgraph.make_swiss_roll(n, seed=0)[0].astype(np.float32)
    ids = pointgraph.knn_graph(X, 10, 0.0, device=0, d2=True)[0]
    pos = np.random.RandomState(0).rand(n, 2)
    m = layout.SpringLayout(n, device=0)
    m.set_rows(ids, np.ones(ids.shape))
    med, ts = device_runs(m, pos, reps)
    m.free()
    return {"n": n, "k": 10, "iterations": 50, "dim": 2, "run_s_median": med, "run_s_all": ts,
            "pairs_per_s": 50.0 * n * n / med}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "layout", "bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--nx-iterations", type=int, default=2)
    ap.add_argument("--swiss", type=int, default=100000)
    a = ap.parse_args()
    from gwamd import neighbors
    res = {"blog": blog(a.reps, a.nx_iterations), "swiss_100k": swiss(a.swiss, a.reps)}
    nb = neighbors.Neighbors(4, device=0, dim=128, topk=20)
    res["fp64_fma_per_s"] = nb.fma_rate()
    nb.free()
    for s in ("blog", "swiss_100k"):
        res[s]["pairs_per_s_over_fma_per_s"] = res[s]["pairs_per_s"] / res["fp64_fma_per_s"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
