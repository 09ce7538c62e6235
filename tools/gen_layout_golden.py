"""Golden spring layouts from networkx's own spring_layout, so that the check also runs where networkx is absent.

    python tools/gen_layout_golden.py

Needs networkx (the fixture was written with 3.4.2); the tests read tests/golden/layout_nx.npz and never this script.
Cases: karate (tests/golden/data/karate.edgelist) at seeds 0 and 7, the path of 40 at seed 1; each with scale=None and
with scale=1, center=(2, 3); 50 iterations, float64.  Per case `<name>_edges` int64 [m][2] (labels; G is the graph
built from them in this order), `<name>_nodes` int64 [n] (G's node order),
`<name>_raw` and `<name>_scaled` float64 [n][2] (rows in node order), `<name>_seed`.
"""
import os

import networkx as nx
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def cases():
    karate = np.loadtxt(os.path.join(ROOT, "tests", "golden", "data", "karate.edgelist"), dtype=np.int64)
    path = np.stack([np.arange(39), np.arange(1, 40)], axis=1)
    return [("karate_s0", karate, 0), ("karate_s7", karate, 7), ("path40_s1", path, 1)]


def main():
    out = {}
    for name, edges, seed in cases():
        G = nx.Graph()
        G.add_edges_from(edges.tolist())
        raw = nx.spring_layout(G, seed=seed, scale=None)
        scaled = nx.spring_layout(G, seed=seed, scale=1, center=(2, 3))
        out[name + "_edges"] = edges
        out[name + "_nodes"] = np.asarray(list(G), np.int64)
        out[name + "_seed"] = np.int64(seed)
        out[name + "_raw"] = np.stack([raw[u] for u in G]).astype(np.float64)
        out[name + "_scaled"] = np.stack([scaled[u] for u in G]).astype(np.float64)
    path = os.path.join(ROOT, "tests", "golden", "layout_nx.npz")
    np.savez(path, **out)
    print(f"{path}: {', '.join(n for n, _, _ in cases())} (networkx {nx.__version__})")


if __name__ == "__main__":
    main()
