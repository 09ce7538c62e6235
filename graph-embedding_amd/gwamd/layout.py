"""Spring layout of a graph on the GPU: networkx's spring_layout (Fruchterman-Reingold), the layout under the picture
IsoMap_LE/simRank.py:show draws of a vertex and its top-k SimRank neighbours.

The force simulation runs in HIP (gw_layout_* in include/graphwalk.h, the law in csrc/gw_layout_law.h): a fused
all-pairs repulsion kernel that keeps nothing of size n x n, a CSR gather for the attraction, the iterations back to back
on the stream.  device=-1 evaluates the same law on the host, bit for bit.  Drawing is not done here: the functions
return coordinates.

    python -m gwamd.layout --input edges.txt --output x.pos [--delimiter D] [--weighted] [--dimensions 2|3]
        [--iterations 50] [--threshold 1e-4] [--k K] [--seed 0] [--scale 1] [--init x.emb]
        [--simrank x.sim.txt --vertex V --topk 10] [--device N]
"""
import argparse
import ctypes

import numpy as np

from . import _lib as C

try:
    import torch
except Exception:  # pragma: no cover - torch is optional for the host path
    torch = None


class SpringLayout:
    """Owning handle over a gw_layout; it keeps the positions (a torch CUDA tensor on a device handle, a numpy array on
    the host) that run() and rescale() update in place."""

    def __init__(self, n, dim=2, device=0):
        self.params = C.LayoutParams()
        self.n, self.dim, self.device = int(n), int(dim), int(device)
        h = ctypes.c_void_p()
        C.check(C.lib().gw_layout_create(self.device, self.n, self.dim, ctypes.byref(self.params), ctypes.byref(h)),
                layout=True)
        self._h = h
        self._pos = None

    @property
    def handle(self):
        return self._h

    def set_csr(self, offsets, nbrs, values=None):
        offsets = np.ascontiguousarray(offsets, np.int64)
        nbrs = np.ascontiguousarray(nbrs, np.int32)
        v = None if values is None else np.ascontiguousarray(values, np.float64)
        if len(offsets) != self.n + 1 or len(nbrs) < offsets[-1] or (v is not None and len(v) < offsets[-1]):
            raise ValueError(f"offsets must be [{self.n + 1}] and cover nbrs and values")
        C.check(C.lib().gw_layout_set_csr(self._h, C.ptr(offsets), C.ptr(nbrs), C.ptr(v)), layout=self._h)

    def set_rows(self, ids, values):
        """ids int32 [n][topk], values float64 [n][topk] in gw_topsim's layout (numpy arrays or torch tensors)."""
        ids, values = (a.cpu().numpy() if hasattr(a, "cpu") else a for a in (ids, values))
        ids = np.ascontiguousarray(ids, np.int32)
        values = np.ascontiguousarray(values, np.float64)
        if ids.ndim != 2 or ids.shape != values.shape or ids.shape[0] != self.n:
            raise ValueError(f"ids and values must both be [{self.n}][topk]")
        C.check(C.lib().gw_layout_set_rows(self._h, C.ptr(ids), C.ptr(values), ids.shape[1]), layout=self._h)

    def set_fixed(self, ids=None):
        ids = np.ascontiguousarray([] if ids is None else ids, np.int32).reshape(-1)
        C.check(C.lib().gw_layout_set_fixed(self._h, C.ptr(ids) if len(ids) else None, len(ids)), layout=self._h)

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream) if self.device >= 0 else None

    def _own(self, pos):
        """A float64 [n][dim] copy of pos where the handle computes."""
        if self.device < 0:
            a = np.array(pos.cpu().numpy() if hasattr(pos, "cpu") else pos, np.float64, order="C")
        else:
            a = torch.as_tensor(pos).to(device=f"cuda:{self.device}", dtype=torch.float64, copy=True).contiguous()
        if tuple(a.shape) != (self.n, self.dim):
            raise ValueError(f"positions must be [{self.n}][{self.dim}]")
        return a

    def run(self, pos=None, k=0.0, iterations=50, threshold=1e-4):
        """Runs the simulation from pos (None: the positions the handle holds) and returns iterations_done; the result
        is positions_numpy() / positions_torch().  k = 0: sqrt(1 / n)."""
        if pos is not None:
            self._pos = self._own(pos)
        if self._pos is None:
            raise ValueError("no positions: pass pos")
        done = ctypes.c_int32()
        C.check(C.lib().gw_layout_run(self._h, C.ptr(self._pos), float(k), int(iterations), float(threshold),
                                      self._stream(), ctypes.byref(done)), layout=self._h)
        return done.value

    def step(self, pos, k=0.0, t=0.1, as_torch=False):
        """One iteration at temperature t from pos: (disp, pos_out), float64 [n][dim] each.  The handle's own positions
        are left alone."""
        p = self._own(pos)
        if self.device < 0:
            disp, out = np.empty_like(p), np.empty_like(p)
        else:
            disp, out = torch.empty_like(p), torch.empty_like(p)
        C.check(C.lib().gw_layout_step(self._h, C.ptr(p), float(k), float(t), C.ptr(disp), C.ptr(out), self._stream()),
                layout=self._h)
        if self.device < 0 or as_torch:
            return disp, out
        return disp.cpu().numpy(), out.cpu().numpy()

    def rescale(self, scale=1.0, center=None, pos=None):
        """networkx's rescale_layout(pos, scale) + center on the handle's positions (or on pos, which it then holds)."""
        if pos is not None:
            self._pos = self._own(pos)
        if self._pos is None:
            raise ValueError("no positions: pass pos")
        c = None if center is None else np.ascontiguousarray(center, np.float64).reshape(-1)
        if c is not None and len(c) != self.dim:
            raise ValueError("length of center coordinates must match dimension of layout")
        C.check(C.lib().gw_layout_rescale(self._h, C.ptr(self._pos), float(scale), C.ptr(c), self._stream()),
                layout=self._h)

    def positions_torch(self):
        """The positions as a torch tensor: the handle's own CUDA tensor on a device handle."""
        if self._pos is None:
            raise ValueError("no positions yet")
        return self._pos if self.device >= 0 else torch.from_numpy(self._pos)

    def positions_numpy(self):
        if self._pos is None:
            raise ValueError("no positions yet")
        return self._pos.cpu().numpy() if self.device >= 0 else self._pos.copy()

    def tiles(self):
        """{'rows', 'chunk', 'strands', 'block'}: rows of a k_layout_pairs workgroup (0 on the host) and the law's
        constants."""
        v = [ctypes.c_int32() for _ in range(4)]
        C.check(C.lib().gw_layout_tiles(self._h, *[ctypes.byref(t) for t in v]), layout=self._h)
        return dict(zip(("rows", "chunk", "strands", "block"), (t.value for t in v)))

    def kernel_attrs(self):
        """{kernel name: {'vgprs', 'scratch_bytes', 'lds_bytes'}} (hipFuncGetAttributes)."""
        cap = 16
        names = (ctypes.c_char_p * cap)()
        v, s, l = ((ctypes.c_int32 * cap)() for _ in range(3))
        n = ctypes.c_int32()
        C.check(C.lib().gw_layout_kernel_attrs(self._h, cap, names, v, s, l, ctypes.byref(n)), layout=self._h)
        return {names[i].decode(): {"vgprs": v[i], "scratch_bytes": s[i], "lds_bytes": l[i]}
                for i in range(min(n.value, cap))}

    def free(self):
        if getattr(self, "_h", None):
            C.lib().gw_layout_free(self._h)
            self._h = None
        self._pos = None

    def __del__(self):
        try:
            self.free()
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass


def _is_handle(G):
    return hasattr(G, "export_csr")


def graph_csr(G, weight="weight"):
    """(nodes, offsets, nbrs, values): nodes in G's node order (a networkx graph's, or a gwamd handle's node_order
    with its labels), row i the adjacency of nodes[i] over positions in that order, columns ascending.  Both kinds
    of graph of one edge list give the same arrays.  Values as nx.to_numpy_array's: the `weight` attribute (1 where it
    is missing or weight is None), parallel edges added."""
    if _is_handle(G):
        csr = G.export_csr()
        order = np.asarray(csr["node_order"], np.int64)
        where = np.empty(len(order), np.int64)
        where[order] = np.arange(len(order))
        nodes = [int(x) for x in np.asarray(csr["labels"])[order]]
        offs, nb = np.asarray(csr["offsets"]), np.asarray(csr["nbrs"])
        w = np.ones(len(nb)) if weight is None or csr.get("weights") is None else np.asarray(csr["weights"], np.float64)
        rows = [(where[nb[offs[d]:offs[d + 1]]], w[offs[d]:offs[d + 1]]) for d in order]
    else:
        nodes = list(G)
        index = {u: i for i, u in enumerate(nodes)}
        multi = G.is_multigraph()
        rows = []
        for u in nodes:
            cols, vals = [], []
            for v, d in G.adj[u].items():
                for a in (d.values() if multi else (d,)):
                    cols.append(index[v])
                    vals.append(1.0 if weight is None else a.get(weight, 1))
            rows.append((np.asarray(cols, np.int64), np.asarray(vals, np.float64)))
    offsets = np.zeros(len(nodes) + 1, np.int64)
    nbrs, values = [], []
    for i, (cols, vals) in enumerate(rows):
        o = np.argsort(cols, kind="stable")
        nbrs.append(cols[o])
        values.append(vals[o])
        offsets[i + 1] = offsets[i] + len(cols)
    cat = (lambda parts, t: np.concatenate(parts).astype(t) if parts else np.zeros(0, t))
    return nodes, offsets, cat(nbrs, np.int32), cat(values, np.float64)


def _layout_csr(nodes, offsets, nbrs, values, k, pos, fixed, iterations, threshold, scale, center, dim, seed, device):
    """spring_layout over a CSR whose rows follow `nodes`."""
    center = np.zeros(dim) if center is None else np.asarray(center, np.float64)
    if len(center) != dim:
        raise ValueError("length of center coordinates must match dimension of layout")
    index = {u: i for i, u in enumerate(nodes)}
    rng = seed if isinstance(seed, np.random.RandomState) else np.random.RandomState(seed)
    fixed_ix = None
    if fixed is not None:
        if pos is None:
            raise ValueError("nodes are fixed without positions given")
        for node in fixed:
            if node not in pos:
                raise ValueError("nodes are fixed without positions given")
        fixed_ix = np.asarray([index[node] for node in fixed if node in index], np.int32)
    if pos is not None:
        dom_size = max(coord for tup in pos.values() for coord in tup)
        if dom_size == 0:
            dom_size = 1
        pos_arr = rng.rand(len(nodes), dim) * dom_size + center
        for i, u in enumerate(nodes):
            if u in pos:
                pos_arr[i] = np.asarray(pos[u])
    else:
        pos_arr = None
        dom_size = 1
    if len(nodes) == 0:
        return {}
    if len(nodes) == 1:
        return {nodes[0]: center}
    if k is None and fixed is not None:
        k = dom_size / np.sqrt(len(nodes))
    if pos_arr is None:
        pos_arr = rng.rand(len(nodes), dim)
    m = SpringLayout(len(nodes), dim=dim, device=device)
    try:
        m.set_csr(offsets, nbrs, values)
        if fixed_ix is not None:
            m.set_fixed(fixed_ix)
        m.run(pos_arr, k=0.0 if k is None else k, iterations=iterations, threshold=threshold)
        if fixed is None and scale is not None:
            m.rescale(scale, center)
        out = m.positions_numpy()
    finally:
        m.free()
    return dict(zip(nodes, out))


def spring_layout(G, k=None, pos=None, fixed=None, iterations=50, threshold=1e-4, weight="weight", scale=1,
                  center=None, dim=2, seed=None, device=0):
    """networkx.spring_layout's signature and return value ({node: float64 array [dim]} in G's node order), computed by
    gw_layout_*.  G: a networkx graph or a gwamd graph handle (GWGraph; its labels are the keys).  device=-1: the host
    evaluation.  A k of exactly 0 means the default, as None does.  Anything that is not a graph is read as a
    collection of nodes without edges, as networkx reads it.  A 2-D result of eigenmaps or isomap, as a {node: row}
    dict, warm-starts the layout through pos=."""
    if not _is_handle(G) and not hasattr(G, "adj"):
        nodes = list(G)
        args = (nodes, np.zeros(len(nodes) + 1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float64))
    else:
        args = graph_csr(G, weight)
    return _layout_csr(*args, k, pos, fixed, iterations, threshold, scale, center, dim, seed, device)


def _edges_of(graph):
    """(nodes, [(u, v, w)]): every undirected edge once, as labels, u's position in the node order <= v's."""
    nodes, offsets, nbrs, values = graph_csr(graph)
    edges = []
    for i in range(len(nodes)):
        for e in range(offsets[i], offsets[i + 1]):
            if i <= nbrs[e]:
                edges.append((nodes[i], nodes[nbrs[e]], values[e]))
    return nodes, edges


def show_selection(rows, vertex, topk=10):
    """simRank.py:show's choice for `vertex`: (the vertex set [vertex] + [j : W[vertex][j] != 0, j != vertex] in id
    order, colours [m]: 0.7 the vertex, 0.9 its neighbours, 0.1 the rest), m = len(rows).  rows: (ids, values) arrays
    [m][>= topk] (-1 padded) or read_simrank's list of rows of (id, value) strings; W[i][id] = value for a row's first
    topk entries, a later entry of the same id replacing an earlier one, as the reference fills its matrix."""
    if isinstance(rows, (tuple, list)) and len(rows) == 2 and hasattr(rows[0], "shape"):
        ids, values = np.asarray(rows[0]), np.asarray(rows[1])
        m = len(ids)
        row = [(int(i), float(v)) for i, v in zip(ids[vertex][:topk], values[vertex][:topk]) if i >= 0]
    else:
        m = len(rows)
        row = [(int(i), float(v)) for i, v in rows[vertex][:topk]]
    W = {}
    for j, v in row:
        W[j] = v
    chosen = [vertex] + [j for j in range(m) if j != vertex and W.get(j, 0) != 0]
    colours = [0.7 if j == vertex else 0.1 if W.get(j, 0) == 0 else 0.9 for j in range(m)]
    return chosen, colours


def show(rows, graph, vertex, topk=10, **kw):
    """simRank.py:show without the drawing: (pos, colours, kept_edges) for `vertex` (a label of graph, and the index of
    its row).  kept_edges: the graph's edges with an end in {vertex} or its top-k SimRank neighbours, [(u, v)] sorted;
    pos: spring_layout of the graph with every other edge removed (all vertices stay, as in the reference); kw goes to
    the layout (seed, device, iterations, ...)."""
    chosen, colours = show_selection(rows, vertex, topk)
    chosen = set(chosen)
    nodes, edges = _edges_of(graph)
    kept = [(u, v, w) for u, v, w in edges if u in chosen or v in chosen]
    index = {u: i for i, u in enumerate(nodes)}
    adj = [[] for _ in nodes]
    for u, v, w in kept:
        adj[index[u]].append((index[v], w))
        if u != v:
            adj[index[v]].append((index[u], w))
    offsets = np.zeros(len(nodes) + 1, np.int64)
    nbrs, values = [], []
    for i, r in enumerate(adj):
        r.sort(key=lambda x: x[0])
        nbrs += [c for c, _ in r]
        values += [w for _, w in r]
        offsets[i + 1] = len(nbrs)
    lay = dict(k=None, pos=None, fixed=None, iterations=50, threshold=1e-4, scale=1, center=None, dim=2, seed=None,
               device=0)
    lay.update(kw)
    pos = _layout_csr(nodes, offsets, np.asarray(nbrs, np.int32), np.asarray(values, np.float64), **lay)
    return pos, colours, sorted((min(u, v), max(u, v)) for u, v, _ in kept)


def main(argv=None):
    from . import classify, deepsim, eigenmaps
    from .graph import GWGraph
    ap = argparse.ArgumentParser(prog="python -m gwamd.layout", description=__doc__.split("\n\n")[0])
    ap.add_argument("--input", required=True, help="edge list: `u v` or, with --weighted, `u v w` per line")
    ap.add_argument("--output", required=True, help="positions in save_embeddings' text: `<n> <dim>`, then `<label> x y`")
    ap.add_argument("--delimiter", default=None)
    ap.add_argument("--weighted", action="store_true")
    ap.add_argument("--dimensions", type=int, default=2, choices=(2, 3))
    ap.add_argument("--iterations", type=int, default=50)
    ap.add_argument("--threshold", type=float, default=1e-4)
    ap.add_argument("--k", type=float, default=None)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--init", default=None, help="an embedding file whose first --dimensions columns start the layout")
    ap.add_argument("--simrank", default=None, help="a .sim.txt: lay out --vertex's SimRank picture (show)")
    ap.add_argument("--vertex", type=int, default=0)
    ap.add_argument("--topk", type=int, default=10)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    G = GWGraph.from_edgelist(a.input, a.delimiter, "nx", False, a.weighted)
    kw = dict(k=a.k, iterations=a.iterations, threshold=a.threshold, scale=a.scale, dim=a.dimensions, seed=a.seed,
              device=a.device)
    if a.init:
        labels, X = classify.read_embedding(a.init)
        kw["pos"] = {int(u): X[i, :a.dimensions].astype(np.float64) for i, u in enumerate(labels)}
    if a.simrank:
        rows = eigenmaps.read_rows(a.simrank)
        pos, _, kept = show(rows, G, a.vertex, a.topk, **kw)
        print(f"vertex {a.vertex}: {len(kept)} edges kept")
    else:
        pos = spring_layout(G, **kw)
    # save_embeddings writes rows 0 .. n-1 with the row index as the label: rows in label order
    labels = sorted(pos)
    if labels != list(range(len(labels))):
        raise ValueError("the output format takes vertex labels 0 .. n-1")
    deepsim.save_embeddings(a.output, np.stack([pos[u] for u in labels]))
    print(f"{len(labels)} positions -> {a.output}")


if __name__ == "__main__":
    main()
