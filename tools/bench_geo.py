"""Geodesics and Isomap on the swiss roll: writes profiles/geo/bench.json.

    python tools/bench_geo.py [--out profiles/geo/bench.json] [--reps 5] [--scipy-sources 64]

Two shapes at k = 10: 10,000 x 3 with every point a source (classical Isomap) and 100,000 x 3 with 1,024 landmarks.
Each device query is timed as the median of `reps` calls after one warm-up (the call synchronises its stream), beside
scipy.sparse.csgraph.dijkstra on the host, single-threaded, on the first `scipy-sources` of the same sources and
scaled to all of them (marked extrapolated).  Per query: entries relaxed per source / graph entries, rounds,
fallbacks.  A sweep of the bucket width (multiples of the mean edge length) on the landmark shape, and the whole
isomap() call at both shapes.
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


def timed(f, reps):
    f()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t)
    return statistics.median(ts), ts


def shape(n, nsrc, reps, scipy_sources, sweep):
    import torch
    from gwamd import geodesics, isomap, pointgraph
    X = pointgraph.make_swiss_roll(n, seed=0)[0].astype(np.float32)
    ids, _, d2 = pointgraph.knn_graph(X, 10, 0.0, device=0, d2=True)
    src = None if nsrc is None else np.sort(np.random.RandomState(0).permutation(n)[:nsrc]).astype(np.int32)
    ns = n if src is None else len(src)
    g = geodesics.Geodesics(n, device=0, squared=True)
    g.set_rows(ids, d2)
    out = torch.empty((ns, n), dtype=torch.float64, device="cuda:0")
    med, ts = timed(lambda: g.query(src, as_torch=True, out=out), reps)
    st = g.stats()
    r = {"n": n, "k": 10, "sources": ns, "entries": st.entries, "components": st.components,
         "query_s_median": med, "query_s_all": ts, "sources_per_s": ns / med,
         "relaxed_per_source_over_entries": st.relaxations / (ns * st.entries), "rounds_max": st.rounds_max,
         "fallbacks": st.fallbacks, "tiles": g.tiles(), "kernel_attrs": g.kernel_attrs(),
         "mode": "lds" if n <= g.tiles()["lds_rows"] else "global"}
    # the host library's own Dijkstra on the box's threads, same sources
    h = geodesics.Geodesics(n, device=-1, squared=True)
    h.set_rows(ids, d2)
    sub = (np.arange(n, dtype=np.int32) if src is None else src)[:max(scipy_sources, 256)]
    t = time.perf_counter()
    hd = h.query(sub)
    r["host_openmp_s_extrapolated"] = (time.perf_counter() - t) * ns / len(sub)
    r["host_openmp_threads"] = int(os.environ.get("OMP_NUM_THREADS", "0")) or os.cpu_count()
    r["bitwise_equal_to_host_on_subset"] = bool(np.array_equal(out[:len(sub)].cpu().numpy().view(np.int64),
                                                               hd.view(np.int64)))
    try:
        import scipy.sparse as sp
        from scipy.sparse.csgraph import dijkstra
        off, col, ln = h_csr(ids, d2, n)
        M = sp.csr_matrix((ln, col, off), shape=(n, n))
        s2 = sub[:scipy_sources]
        t = time.perf_counter()
        dijkstra(M, directed=True, indices=s2)
        dt = time.perf_counter() - t
        r["scipy_dijkstra_s_extrapolated"] = dt * ns / len(s2)
        r["scipy_sources_timed"] = len(s2)
        r["speedup_over_scipy_single_thread"] = r["scipy_dijkstra_s_extrapolated"] / med
        r["speedup_over_scipy_on_16_cpus_assuming_perfect_scaling"] = r["scipy_dijkstra_s_extrapolated"] / 16 / med
    except ImportError:
        r["scipy_dijkstra_s_extrapolated"] = None
    if sweep:
        mean = float(np.sqrt(d2[ids >= 0][d2[ids >= 0] > 0]).mean())
        r["delta_sweep"] = []
        for mult in (1, 2, 4, 8, 16):
            gs = geodesics.Geodesics(n, device=0, squared=True, delta=mult * mean)
            gs.set_rows(ids, d2)
            m2, _ = timed(lambda: gs.query(src, as_torch=True, out=out), 3)
            s2 = gs.stats()
            r["delta_sweep"].append({"delta_over_mean_listed_length": mult, "query_s_median_of_3": m2,
                                     "relaxed_per_source_over_entries": s2.relaxations / (ns * s2.entries),
                                     "rounds_max": s2.rounds_max})
            gs.free()
    g.free()
    h.free()
    del out
    xt = torch.as_tensor(X, device="cuda:0")
    med, ts = timed(lambda: isomap.isomap(xt, k=10, dim=2, landmarks=nsrc, device=0), min(reps, 3))
    r["isomap_call_s_median"] = med
    r["isomap_call_s_all"] = ts
    return r


def h_csr(ids, d2, n):
    """The union-symmetrised CSR for scipy, from the rows."""
    r = np.repeat(np.arange(n), ids.shape[1])
    c = ids.ravel()
    keep = (c >= 0) & (c != r)
    r, c, l = r[keep], c[keep], np.sqrt(d2.ravel()[keep])
    rr, cc, ll = np.concatenate([r, c]), np.concatenate([c, r]), np.concatenate([l, l])
    order = np.lexsort((ll, cc, rr))
    rr, cc, ll = rr[order], cc[order], ll[order]
    first = np.ones(len(rr), bool)
    first[1:] = (rr[1:] != rr[:-1]) | (cc[1:] != cc[:-1])
    rr, cc, ll = rr[first], cc[first], ll[first]
    off = np.zeros(n + 1, np.int64)
    np.add.at(off, rr + 1, 1)
    return np.cumsum(off), cc.astype(np.int32), ll


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "geo", "bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scipy-sources", type=int, default=64)
    a = ap.parse_args()
    res = {"full_10k": shape(10000, None, a.reps, a.scipy_sources, False),
           "landmark_100k": shape(100000, 1024, a.reps, a.scipy_sources, True)}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
