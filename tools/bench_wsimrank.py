"""Weighted SimRank on blog's and moreno's adjacency: writes profiles/wsimrank/bench.json.

    python tools/bench_wsimrank.py [--out profiles/wsimrank/bench.json] [--reps 5] [--rounds 3] [--graphs blog,moreno]

Each graph's lines get a deterministic positive weight per pair, 1 + ((min * 31 + max * 17) % 7) / 4, and are loaded
once as a WGraph and once as a Graph (same adjacency).  In one process, per graph: the median over `reps` calls (after
one warm-up that builds the layout and workspace) of gw_simrank_weighted and of gw_simrank_naive at `rounds` rounds,
timed with stream events; their ratio (the derived check: at most 3, the ratio of streamed bytes per entry, 12 B
against 4 B); gathers per second (n * nnz per pass 1, half of it per pass 2); gw_simrank_weighted_ref on 16 host
threads at one round; the largest relative deviation of the kernel from that host evaluation; the kernel attributes.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graph-embedding_amd"))
DATA = os.path.join(ROOT, "tests", "golden", "data")
GRAPHS = {"blog": ("blog.txt", 10313, ","), "moreno": ("moreno_crime_crime.txt", 1380, "\t")}


def weight(u, v):
    return 1 + ((min(u, v) * 31 + max(u, v) * 17) % 7) / 4


def timed(fn, h, C, rounds, sim, sp, reps):
    import torch
    from gwamd import _lib as L
    st = torch.cuda.current_stream()
    ts = []
    for r in range(reps + 1):       # the first call warms (layout, workspace)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        L.check(fn(h, C, rounds, L.ptr(sim), sp), h)
        e1.record(st)
        torch.cuda.synchronize()
        if r:
            ts.append(e0.elapsed_time(e1))
    return statistics.median(ts), ts


def bench(name, reps, rounds, tmp):
    import torch
    from gwamd import _lib as L
    from gwamd import topsim
    f, V, sep = GRAPHS[name]
    pairs = [tuple(int(x) for x in l.split(sep)[:2]) for l in open(os.path.join(DATA, f)).read().split("\n") if l]
    path = os.path.join(tmp, name + "_weighted.txt")
    with open(path, "w") as out:
        out.writelines(f"{u}{sep}{v}{sep}{weight(u, v)!r}\n" for u, v in pairs)
    wg = topsim.WGraph(path, V, separator=sep)
    g = topsim.Graph(path, V, separator=sep)
    wg._ensure_device()
    g._ensure_device()
    assert np.array_equal(wg._offs, g._offs) and np.array_equal(wg._nbrs, g._nbrs)
    deg = np.diff(wg._offs)
    nnz, m = int(deg.sum()), int(np.count_nonzero(deg))
    sim = torch.empty((V, V), dtype=torch.float64, device="cuda")
    sp = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    wmed, wall = timed(L.lib().gw_simrank_weighted, wg._g.handle, 0.6, rounds, sim, sp, reps)
    wres = sim.cpu().numpy()
    umed, uall = timed(L.lib().gw_simrank_naive, g._g.handle, 0.6, rounds, sim, sp, reps)
    gathers = 1.5 * m * nnz * rounds
    r = {"graph": name, "V": V, "live_vertices": m, "adjacency_entries": nnz, "rounds": rounds, "reps": reps,
         "weighted_ms_per_round_median": wmed / rounds, "weighted_ms_all": wall,
         "unweighted_ms_per_round_median": umed / rounds, "unweighted_ms_all": uall,
         "ratio_weighted_over_unweighted": wmed / umed, "ratio_bound": 3.0,
         "weighted_gathers_per_s": gathers / (wmed / 1e3), "unweighted_gathers_per_s": gathers / (umed / 1e3),
         "weighted_stream_bytes": int(((deg + 7) // 8 * 8).sum()) * 12,
         "unweighted_stream_bytes": int(((deg + 15) // 16 * 16).sum()) * 4,
         "kernel_attrs": topsim.WeightedSimRank(wg).kernel_attrs()}
    host = np.empty((V, V))
    t = time.perf_counter()
    L.check(L.lib().gw_simrank_weighted_ref(wg._g.handle, 0.6, 1, 16, L.ptr(host)), wg._g.handle)
    r["host_ref_16_threads_ms_per_round"] = (time.perf_counter() - t) * 1e3
    r["speedup_over_host_ref_16_threads"] = r["host_ref_16_threads_ms_per_round"] / (wmed / rounds)
    if rounds != 1:
        L.check(L.lib().gw_simrank_weighted_ref(wg._g.handle, 0.6, rounds, 16, L.ptr(host)), wg._g.handle)
    nz = host != 0
    r["max_rel_deviation_from_host_ref"] = float(np.max(np.abs(wres[nz] - host[nz]) / np.abs(host[nz])))
    return r


def main():
    import tempfile
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wsimrank", "bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--graphs", default="blog,moreno")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        res = {name: bench(name, a.reps, a.rounds, tmp) for name in a.graphs.split(",")}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
