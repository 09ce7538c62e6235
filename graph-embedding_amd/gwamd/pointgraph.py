"""The neighbour graph of a point cloud on the GPU.

IsoMap_LE/LE.py:35-60 (laplaEigen) goes from points to their k Euclidean nearest
neighbours (knn, the point itself first) and to heat-kernel weights
exp(-|x_i - x_j|^2 / t).  Here the all-pairs squared distances and the selection
of the k smallest run fused in HIP (gw_nng_* in include/graphwalk.h, the law in
csrc/gw_nng_law.h) on the matrix where it already lies in HBM; device=-1
evaluates the same law on the host, bit for bit.  Rows come back in gw_topsim's
layout (ids int32, weights float64, -1 padded), so eigenmaps.Eigenmaps.set_rows
and neighbors.write_neighbors take them as they are.
"""
import ctypes

import numpy as np

from . import _lib as C
from .neighbors import _PairsHandle, _vectors_of

try:
    import torch
except Exception:  # pragma: no cover - torch is optional for the host path
    torch = None


class PointGraph(_PairsHandle):
    """Owning handle over a gw_nng."""

    _prefix = "nng"

    def __init__(self, n, device=0, dim=3, topk=10, include_self=True, heat_t=0.0):
        self._create(n, device, C.NngParams(dim=int(dim), topk=int(topk), include_self=int(include_self),
                                            heat_t=float(heat_t)))

    def query(self, sources=None, d2=False, stream=None):
        """(ids int32 [nsrc][topk], weights float64 [nsrc][topk]) as numpy arrays, and with d2=True the squared
        distances float64 [nsrc][topk] as a third; sources None: every row."""
        topk = self.params.topk
        if sources is not None:
            sources = np.ascontiguousarray(sources, np.int32).reshape(-1)
        nsrc = self.n if sources is None else len(sources)
        if self.device < 0:
            ids = np.empty((nsrc, topk), np.int32)
            w = np.empty((nsrc, topk), np.float64)
            dd = np.empty((nsrc, topk), np.float64) if d2 else None
            self._call("query", C.ptr(sources), nsrc, C.ptr(ids), C.ptr(w), C.ptr(dd), None)
            return (ids, w, dd) if d2 else (ids, w)
        dev = f"cuda:{self.device}"
        src = None if sources is None else torch.as_tensor(sources, device=dev)
        ids = torch.empty((nsrc, topk), dtype=torch.int32, device=dev)
        w = torch.empty((nsrc, topk), dtype=torch.float64, device=dev)
        dd = torch.empty((nsrc, topk), dtype=torch.float64, device=dev) if d2 else None
        if stream is None:
            stream = ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        self._call("query", C.ptr(src), nsrc, C.ptr(ids), C.ptr(w), C.ptr(dd), stream)
        out = (ids.cpu().numpy(), w.cpu().numpy())
        return out + (dd.cpu().numpy(),) if d2 else out


def knn_graph(x, k, t=0.0, include_self=True, sources=None, device=0, d2=False):
    """For every source row (None: all) of the points `x` its `k` nearest rows by Euclidean distance, the row
    itself first when include_self (LE.py's knn), weighted exp(-d2 / t) (t = 0: weight 1): (ids int32 [nsrc][k],
    weights float64 [nsrc][k]), and the squared distances as a third with d2=True; distance ascending then id
    ascending, -1 / 0.0 padded.  `x`: a torch CUDA float32 tensor (used in place, pitch from its stride), a numpy
    array, an embedding or a live trainer (as neighbors.most_similar)."""
    x, device = _vectors_of(x, device)
    m = PointGraph(x.shape[0], device=device, dim=x.shape[1], topk=k, include_self=include_self, heat_t=t)
    try:
        m.set_vectors(x)
        return m.query(sources, d2=d2)
    finally:
        m.free()


def make_swiss_roll(n_samples=100, noise=0.0, seed=None, height=100.0):
    """LE.py:19-33's swiss roll, with its draws in its order from np.random.RandomState(seed): t = 1.5 pi (1 + 2 u),
    points (t cos t, height * u', t sin t) + noise * N(0, 1).  Returns (X float64 [n_samples][3], t [n_samples])."""
    rng = np.random.RandomState(seed)
    angle = 1.5 * np.pi * (1.0 + 2.0 * rng.rand(n_samples))
    across = height * rng.rand(n_samples)
    pts = np.stack([angle * np.cos(angle), across, angle * np.sin(angle)], axis=1)
    if noise:
        pts += noise * rng.randn(3, n_samples).T
    return pts, angle
