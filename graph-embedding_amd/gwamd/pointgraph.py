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
from .neighbors import _vectors_of

try:
    import torch
except Exception:  # pragma: no cover - torch is optional for the host path
    torch = None


class PointGraph:
    """Owning handle over a gw_nng."""

    def __init__(self, n, device=0, dim=3, topk=10, include_self=True, heat_t=0.0):
        self.params = C.NngParams(dim=int(dim), topk=int(topk), include_self=int(include_self), heat_t=float(heat_t))
        self.n, self.device = int(n), int(device)
        h = ctypes.c_void_p()
        C.check(C.lib().gw_nng_create(self.device, self.n, ctypes.byref(self.params), ctypes.byref(h)), nng=True)
        self._h = h
        self._keep = []

    @property
    def handle(self):
        return self._h

    def set_rows(self, n):
        """Another row count for the next set_vectors."""
        C.check(C.lib().gw_nng_set_rows(self._h, int(n)), nng=self._h)
        self.n = int(n)
        self._keep = []

    def set_vectors(self, x, pitch=None):
        """x: float32 [n][>= dim], rows contiguous: a torch CUDA tensor (device >= 0; read where it is), a numpy
        array (device = -1; uploaded when device >= 0) or a raw address with `pitch` in floats."""
        if isinstance(x, int):
            p = ctypes.c_void_p(x)
        else:
            if isinstance(x, np.ndarray):
                if x.dtype != np.float32 or x.ndim != 2 or x.strides[1] != 4 or x.strides[0] % 4:
                    x = np.ascontiguousarray(x, np.float32)
                if self.device >= 0:
                    x = torch.as_tensor(np.ascontiguousarray(x), device=f"cuda:{self.device}")
            elif x.dtype != torch.float32 or x.dim() != 2 or x.stride(1) != 1:
                raise ValueError("vectors tensor must be float32 [n][dim] with contiguous rows")
            if x.shape[0] != self.n or x.shape[1] < self.params.dim:
                raise ValueError(f"vectors must be [{self.n}][>= {self.params.dim}]")
            pitch = x.stride(0) if hasattr(x, "stride") else x.strides[0] // 4
            p = C.ptr(x)
            self._keep = [x]
        C.check(C.lib().gw_nng_set_vectors(self._h, p, int(pitch)), nng=self._h)

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
            C.check(C.lib().gw_nng_query(self._h, C.ptr(sources), nsrc, C.ptr(ids), C.ptr(w), C.ptr(dd), None),
                    nng=self._h)
            return (ids, w, dd) if d2 else (ids, w)
        dev = f"cuda:{self.device}"
        src = None if sources is None else torch.as_tensor(sources, device=dev)
        ids = torch.empty((nsrc, topk), dtype=torch.int32, device=dev)
        w = torch.empty((nsrc, topk), dtype=torch.float64, device=dev)
        dd = torch.empty((nsrc, topk), dtype=torch.float64, device=dev) if d2 else None
        if stream is None:
            stream = ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        C.check(C.lib().gw_nng_query(self._h, C.ptr(src), nsrc, C.ptr(ids), C.ptr(w), C.ptr(dd), stream), nng=self._h)
        out = (ids.cpu().numpy(), w.cpu().numpy())
        return out + (dd.cpu().numpy(),) if d2 else out

    def tiles(self):
        """{'tq', 'tc', 'kc', 'buf'}: the main kernel's launch geometry and the per-row buffer length."""
        v = [ctypes.c_int32() for _ in range(4)]
        C.check(C.lib().gw_nng_tiles(self._h, *[ctypes.byref(t) for t in v]), nng=self._h)
        return dict(zip(("tq", "tc", "kc", "buf"), (t.value for t in v)))

    def kernel_attrs(self):
        """{kernel name: {'vgprs', 'scratch_bytes', 'lds_bytes'}} (hipFuncGetAttributes)."""
        cap = 16
        names = (ctypes.c_char_p * cap)()
        v, s, l = ((ctypes.c_int32 * cap)() for _ in range(3))
        n = ctypes.c_int32()
        C.check(C.lib().gw_nng_kernel_attrs(self._h, cap, names, v, s, l, ctypes.byref(n)), nng=self._h)
        return {names[i].decode(): {"vgprs": v[i], "scratch_bytes": s[i], "lds_bytes": l[i]}
                for i in range(min(n.value, cap))}

    def free(self):
        if getattr(self, "_h", None):
            C.lib().gw_nng_free(self._h)
            self._h = None
            self._keep = []

    def __del__(self):
        try:
            self.free()
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass


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
