"""Laplacian eigenmaps of top-k rows on the GPU.

IsoMap_LE/simRank.py:95-123 builds W from the SimRank top-k rows as a dense
matrix and takes np.linalg.eig(D^-1 L); LE.py:35-51 is the general form.  Here
W is sparse and symmetrised, and the eigenpairs above `min_eigenvalue` come
from Chebyshev-filtered block subspace iteration in fp64 (gw_le_* in
include/graphwalk.h, the law in csrc/gw_le_law.h); device=-1 evaluates the same
law on the host, bit for bit.  The rows gw_topsim and gw_knn_query write (ids
int32, scores float64, -1 padded) are the input as they are, and the result is
an embedding classify.scoring and neighbors.most_similar read in place.

Points rather than a graph (LE.py's own input) go through gwamd.pointgraph first: their k
Euclidean nearest neighbours with heat-kernel weights, fused on the GPU (gw_nng_*), then this
solver with self_loops = 1, which keeps LE.py's W[i][i] = 1 (eigenmaps_of_points, laplaEigen).

    python -m gwamd.eigenmaps --simrank x.sim.txt | --input edges.txt [--delimiter D] |
        --points X.npy --knn 10 --heat 15.0 [--no-self]
        --output x.emb --dimensions 128 [--topk 10] [--symmetrize mean|max] [--min-eigenvalue 1e-5]
        [--block B] [--groups g.csv] [--neighbors x.nn] [--device N]
"""
import argparse
import ctypes
import sys

import numpy as np

from . import _lib as C

try:
    import torch
except Exception:  # pragma: no cover - torch is optional for the host path
    torch = None

SYMMETRIZE = {"mean": C.LE_SYM_MEAN, "max": C.LE_SYM_MAX}
STATES = {C.LE_CONVERGED: "converged", C.LE_NOT_CONVERGED: "not-converged"}


class Eigenmaps:
    """Owning handle over a gw_le."""

    def __init__(self, n, device=0, dim=128, symmetrize="mean", **params):
        self.params = C.LeParams(dim=int(dim), symmetrize=SYMMETRIZE.get(symmetrize, symmetrize), **params)
        self.n, self.device = int(n), int(device)
        h = ctypes.c_void_p()
        C.check(C.lib().gw_le_create(self.device, self.n, ctypes.byref(self.params), ctypes.byref(h)), le=True)
        self._h = h
        self.stats = None

    @property
    def handle(self):
        return self._h

    def set_rows(self, ids, scores):
        """ids int32 [n][topk], scores float64 [n][topk] in gw_topsim's layout (numpy arrays or torch tensors; the
        operator is assembled on the host)."""
        ids, scores = (a.cpu().numpy() if hasattr(a, "cpu") else a for a in (ids, scores))
        ids = np.ascontiguousarray(ids, np.int32)
        scores = np.ascontiguousarray(scores, np.float64)
        if ids.ndim != 2 or ids.shape != scores.shape or ids.shape[0] != self.n:
            raise ValueError(f"ids and scores must both be [{self.n}][topk]")
        C.check(C.lib().gw_le_set_rows(self._h, C.ptr(ids), C.ptr(scores), ids.shape[1]), le=self._h)

    def set_csr(self, offsets, nbrs, weights=None):
        offsets = np.ascontiguousarray(offsets, np.int64)
        nbrs = np.ascontiguousarray(nbrs, np.int32)
        w = None if weights is None else np.ascontiguousarray(weights, np.float64)
        if len(offsets) != self.n + 1 or len(nbrs) < offsets[-1] or (w is not None and len(w) < offsets[-1]):
            raise ValueError(f"offsets must be [{self.n + 1}] and cover nbrs and weights")
        C.check(C.lib().gw_le_set_csr(self._h, C.ptr(offsets), C.ptr(nbrs), C.ptr(w)), le=self._h)

    def solve(self, stream=None):
        """Runs the solver; returns (and keeps as .stats) the gw_le_stats_t."""
        st = C.LeStats()
        if stream is None and self.device >= 0 and torch is not None:
            stream = ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        C.check(C.lib().gw_le_solve(self._h, ctypes.byref(st), stream), le=self._h)
        self.stats = st
        return st

    def export(self):
        """(eigenvalues float64 [dim] ascending, vectors float64 [n][dim], residuals float64 [dim])."""
        dim = self.params.dim
        lam, vec, res = np.empty(dim), np.empty((self.n, dim)), np.empty(dim)
        C.check(C.lib().gw_le_export(self._h, C.ptr(lam), C.ptr(vec), C.ptr(res)), le=self._h)
        return lam, vec, res

    def vectors_dev(self):
        """(address of the float32 vectors where they lie, pitch in floats)."""
        p = ctypes.c_void_p()
        pitch = ctypes.c_int64()
        C.check(C.lib().gw_le_vectors_dev(self._h, ctypes.byref(p), ctypes.byref(pitch)), le=self._h)
        return p.value, pitch.value

    def vectors_numpy(self):
        """A float32 copy [n][dim] of the vectors."""
        p, pitch = self.vectors_dev()
        if self.device >= 0:
            return self.vectors_torch().cpu().numpy()
        return np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_float)), (self.n, pitch)).copy()

    def vectors_torch(self):
        """The float32 vectors as a torch view [n][dim] of the solver's own HBM (no copy); valid while this handle
        lives and until its next solve."""
        if self.device < 0:
            raise ValueError("host evaluation keeps its vectors in host memory (use vectors_numpy())")
        p, pitch = self.vectors_dev()

        class _View:  # the CUDA array interface torch.as_tensor reads
            __cuda_array_interface__ = {"shape": (self.n, pitch), "typestr": "<f4", "data": (p, False),
                                        "version": 2, "strides": None}
        return torch.as_tensor(_View(), device=f"cuda:{self.device}")[:, :self.params.dim]

    def apply(self, x):
        """S x for a float64 block [n][cols]: a torch CUDA tensor (device >= 0) or a numpy array (device = -1)."""
        if self.device < 0:
            x = np.ascontiguousarray(x, np.float64)
            y = np.empty_like(x)
        else:
            x = x.contiguous()
            torch.cuda.synchronize(self.device)
            y = torch.empty_like(x)
        if x.ndim != 2 or x.shape[0] != self.n:
            raise ValueError(f"x must be [{self.n}][cols]")
        C.check(C.lib().gw_le_apply(self._h, C.ptr(x), C.ptr(y), x.shape[1]), le=self._h)
        return y

    def tiles(self):
        """{'rows_per_wg', 'chunk', 'cols_per_pass'}: k_le_apply's geometry and the law's row chunk."""
        v = [ctypes.c_int32() for _ in range(3)]
        C.check(C.lib().gw_le_tiles(self._h, *[ctypes.byref(t) for t in v]), le=self._h)
        return dict(zip(("rows_per_wg", "chunk", "cols_per_pass"), (t.value for t in v)))

    def kernel_attrs(self):
        """{kernel name: {'vgprs', 'scratch_bytes', 'lds_bytes'}} (hipFuncGetAttributes)."""
        cap = 16
        names = (ctypes.c_char_p * cap)()
        v, s, l = ((ctypes.c_int32 * cap)() for _ in range(3))
        n = ctypes.c_int32()
        C.check(C.lib().gw_le_kernel_attrs(self._h, cap, names, v, s, l, ctypes.byref(n)), le=self._h)
        return {names[i].decode(): {"vgprs": v[i], "scratch_bytes": s[i], "lds_bytes": l[i]}
                for i in range(min(n.value, cap))}

    def time_kernel(self, which, reps=10):
        """Mean milliseconds of one launch of 'apply', 'gram' or 'rotate' on the solver's own blocks (after solve;
        the blocks are overwritten, so export first)."""
        ms = ctypes.c_double()
        C.check(C.lib().gw_le_time_kernel(self._h, ("apply", "gram", "rotate").index(which), int(reps),
                                          ctypes.byref(ms)), le=self._h)
        return ms.value

    def free(self):
        if getattr(self, "_h", None):
            C.lib().gw_le_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass


class EigenEmbedding:
    """What eigenmaps() returns: the part of gwamd.embed.Embedding its consumers read (vectors, labels, model with
    vectors_torch()), plus the spectrum.  classify.scoring and neighbors.most_similar take it as it is and, on a GPU,
    read the vectors where the solver left them."""

    def __init__(self, model, labels, eigenvalues, vectors64, residuals):
        self.model = model
        self.labels = labels
        self.eigenvalues = eigenvalues
        self.vectors64 = vectors64
        self.residuals = residuals
        self.vectors = model.vectors_numpy()  # [n][dim] float32, row = vertex
        self.stats = model.stats

    def save(self, path):
        """`<rows> <dim>` then `<label> v ... v` (deepsim.save_embeddings' text; classify.read_embedding reads it)."""
        from . import deepsim
        deepsim.save_embeddings(path, self.vectors)


def eigenmaps(rows_or_graph, dim=128, device=0, labels=None, **params):
    """The Laplacian eigenmap of top-k rows `(ids, scores)` (gw_topsim's layout, row r = vertex r) or of a graph's
    own adjacency (a GWGraph, or a dict with 'offsets', 'nbrs' and optionally 'weights').  params: block,
    cheb_degree, max_iters, tol, min_eigenvalue, symmetrize ('mean' | 'max'), seed.  Returns an EigenEmbedding."""
    if isinstance(rows_or_graph, (tuple, list)):
        ids, scores = rows_or_graph
        m = Eigenmaps(len(ids), device=device, dim=dim, **params)
        m.set_rows(ids, scores)
    else:
        csr = rows_or_graph.export_csr() if hasattr(rows_or_graph, "export_csr") else rows_or_graph
        m = Eigenmaps(len(csr["offsets"]) - 1, device=device, dim=dim, **params)
        m.set_csr(csr["offsets"], csr["nbrs"], csr.get("weights"))
        if labels is None and csr.get("labels") is not None:
            labels = [str(l) for l in csr["labels"]]
    st = m.solve()
    if st.state != C.LE_CONVERGED:
        print(f"warning: eigenmaps stopped at max_iters with residual {st.max_residual:.3g}", file=sys.stderr)
    lam, vec, res = m.export()
    return EigenEmbedding(m, [str(i) for i in range(m.n)] if labels is None else list(labels), lam, vec, res)


def eigenmaps_of_points(x, k, t, dim=2, device=0, include_self=True, labels=None, **params):
    """The Laplacian eigenmap of a point cloud: pointgraph.knn_graph(x, k, t, include_self) -> eigenmaps().  `x` is
    what knn_graph takes (a torch CUDA tensor is read in place and decides the device); k counts the point itself
    when include_self.  self_loops follows include_self unless given; the other params are eigenmaps()'s.  Returns
    an EigenEmbedding."""
    from . import pointgraph
    from .neighbors import _vectors_of
    x, device = _vectors_of(x, device)
    ids, w = pointgraph.knn_graph(x, k, t, include_self=include_self, device=device)
    params.setdefault("self_loops", int(bool(include_self)))
    return eigenmaps((ids, w), dim=dim, device=device, labels=labels, **params)


def laplaEigen(dataMat, k, t, dim=2, device=0, **params):
    """IsoMap_LE/LE.py:35-51 by name and argument order: (lamda float64 [dim], f float64 [n][dim]), column c of f the
    eigenvector of D^-1 (D - W) for lamda[c], W[i][j] = exp(-|x_i - x_j|^2 / t) over the k nearest neighbours of i,
    i itself among them.  Departures from the reference:
      - only the `dim` smallest eigenvalues above min_eigenvalue (default 1e-5, LE.py:74) and their vectors are
        returned, ascending, not all n in np.linalg.eig's order; the leading eigenvalue 0 is skipped;
      - W is symmetrised ((W + W') / 2, or symmetrize='max'); the reference uses the k-NN matrix as it is, so the
        two agree where that matrix is already symmetric;
      - the points are read as float32; f's columns have unit 2-norm and their largest entry positive;
      - a point at distance > sqrt(700 t) has weight +0 and is no edge."""
    x = np.ascontiguousarray(np.asarray(dataMat), np.float32)
    emb = eigenmaps_of_points(x, k, t, dim=dim, device=device, include_self=True, **params)
    return emb.eigenvalues, emb.vectors64


def read_rows(path, topk=None):
    """(ids, scores) of a `.sim.txt`: the project's `v,id:score,...` through io.read_simrank, or the reference's
    space-separated form (IsoMap_LE/simRank.py:76-93); line r is vertex r.  topk: keep the first topk of a row."""
    from . import deepsim, io
    with open(path) as f:
        comma = "," in f.readline()
    if comma:
        rows = io.read_simrank(path)
    else:
        with open(path) as f:
            rows = [[tuple(t.split(":")) for t in line.split()[1:]] for line in f if line.strip()]
    if topk:
        rows = [r[:topk] for r in rows]
    return deepsim.table_from_simrank(rows, len(rows))


def cli(argv=None):
    ap = argparse.ArgumentParser(description="Laplacian eigenmaps of SimRank top-k rows, of a graph or of points on MI355X.")
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--simrank", default=None, help="a .sim.txt: W from its top-k rows")
    src.add_argument("--input", default=None, help="an edge list: W is the graph's own adjacency")
    src.add_argument("--points", default=None, help="a .npy matrix [n][d]: W from the rows' --knn nearest neighbours")
    ap.add_argument("--knn", type=int, default=10, help="--points: neighbours per point, itself included (LE.py: 10)")
    ap.add_argument("--heat", type=float, default=15.0, help="--points: t of exp(-d2 / t) (LE.py: 15.0); 0: weight 1")
    ap.add_argument("--no-self", action="store_true", help="--points: a point is not its own neighbour, no self-loops")
    ap.add_argument("--delimiter", default=None)
    ap.add_argument("--output", required=True, help="embeddings (classify.read_embedding reads them)")
    ap.add_argument("--dimensions", type=int, default=128)
    ap.add_argument("--topk", type=int, default=10, help="entries read of a .sim.txt row")
    ap.add_argument("--symmetrize", choices=sorted(SYMMETRIZE), default="mean")
    ap.add_argument("--min-eigenvalue", type=float, default=1e-5, help="simRank.py:137 uses 1e-2")
    ap.add_argument("--block", type=int, default=0)
    ap.add_argument("--groups", default=None, help="lines `node,label`: print classify.scoring's table")
    ap.add_argument("--neighbors", default=None, help="write the top-20 cosine neighbours there")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args(argv)
    kw = dict(dim=args.dimensions, device=args.device, symmetrize=args.symmetrize, min_eigenvalue=args.min_eigenvalue,
              block=args.block)
    if args.simrank:
        emb = eigenmaps(read_rows(args.simrank, args.topk), **kw)
    elif args.points:
        pts = np.load(args.points, allow_pickle=False)
        if pts.ndim != 2:
            ap.error("--points must hold a matrix [n][d]")
        kw.pop("dim")
        emb = eigenmaps_of_points(pts, args.knn, args.heat, dim=args.dimensions, include_self=not args.no_self, **kw)
    else:
        from .graph import GWGraph
        emb = eigenmaps(GWGraph.from_edgelist(args.input, args.delimiter), **kw)
    emb.save(args.output)
    st = emb.stats
    print(f"{emb.model.n} x {args.dimensions} eigenmap -> {args.output}: {STATES[st.state]}, {st.iters} iterations, "
          f"{st.applies} applications, {st.skipped} skipped, {st.isolated} isolated, residual {st.max_residual:.3g}",
          file=sys.stderr)
    if args.groups:
        from . import classify
        classify.scoring(emb, classify.read_groups(args.groups), device=args.device)
    if args.neighbors:
        from . import neighbors
        neighbors.neighbors_of(emb, args.neighbors, emb.labels, device=args.device)
    return 0


if __name__ == "__main__":
    sys.exit(cli())
