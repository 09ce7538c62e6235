"""Geodesic (shortest-path) distances on a sparse graph on the GPU.

Isomap's second step: from the k-NN graph of a point cloud to the graph distances from many sources, every vertex for
classical Isomap or L landmarks for landmark Isomap.  The relaxation runs in HIP (gw_geo_* in include/graphwalk.h, the
law in csrc/gw_geo_law.h): one workgroup per source, near-far rounds over a bitmap, 64-bit integer atomic minima on the
bit patterns of the distances; device=-1 evaluates the same law on the host (binary-heap Dijkstra), bit for bit.  The
rows pointgraph.knn_graph(..., d2=True) returns are the input as they are (squared=True).
"""
import ctypes

import numpy as np

from . import _lib as C

try:
    import torch
except Exception:  # pragma: no cover - torch is optional for the host path
    torch = None

SYMMETRIZE = {"union": C.GEO_SYM_UNION, "directed": C.GEO_DIRECTED}


class Geodesics:
    """Owning handle over a gw_geo."""

    def __init__(self, n, device=0, symmetrize="union", squared=False, delta=0.0, round_cap=0):
        """delta: the device schedule's bucket width (0: chosen from the mean edge length); round_cap: a measurement
        aid (c > 0: the device schedule falls back to Bellman-Ford after c - 1 rounds).  Neither changes a result."""
        self.params = C.GeoParams(symmetrize=SYMMETRIZE.get(symmetrize, symmetrize), squared=int(bool(squared)),
                                  delta=float(delta), round_cap=int(round_cap))
        self.n, self.device = int(n), int(device)
        h = ctypes.c_void_p()
        C.check(C.lib().gw_geo_create(self.device, self.n, ctypes.byref(self.params), ctypes.byref(h)), geo=True)
        self._h = h

    @property
    def handle(self):
        return self._h

    def set_rows(self, ids, values):
        """ids int32 [n][topk], values float64 [n][topk] in gw_topsim's layout (numpy arrays or torch tensors; the
        graph is assembled on the host)."""
        ids, values = (a.cpu().numpy() if hasattr(a, "cpu") else a for a in (ids, values))
        ids = np.ascontiguousarray(ids, np.int32)
        values = np.ascontiguousarray(values, np.float64)
        if ids.ndim != 2 or ids.shape != values.shape or ids.shape[0] != self.n:
            raise ValueError(f"ids and values must both be [{self.n}][topk]")
        C.check(C.lib().gw_geo_set_rows(self._h, C.ptr(ids), C.ptr(values), ids.shape[1]), geo=self._h)

    def set_csr(self, offsets, nbrs, values=None):
        offsets = np.ascontiguousarray(offsets, np.int64)
        nbrs = np.ascontiguousarray(nbrs, np.int32)
        v = None if values is None else np.ascontiguousarray(values, np.float64)
        if len(offsets) != self.n + 1 or len(nbrs) < offsets[-1] or (v is not None and len(v) < offsets[-1]):
            raise ValueError(f"offsets must be [{self.n + 1}] and cover nbrs and values")
        C.check(C.lib().gw_geo_set_csr(self._h, C.ptr(offsets), C.ptr(nbrs), C.ptr(v)), geo=self._h)

    def components(self):
        """(component_of int32 [n], main_component): a component's id is its lowest vertex; the main component is
        the largest, the lowest id winning ties."""
        comp = np.empty(self.n, np.int32)
        main = ctypes.c_int32()
        C.check(C.lib().gw_geo_components(self._h, C.ptr(comp), ctypes.byref(main)), geo=self._h)
        return comp, main.value

    def query(self, sources=None, as_torch=False, pitch=None, out=None, stream=None):
        """Distances float64 [nsrc][n] from `sources` (None: every vertex): a numpy array, or on a device handle with
        as_torch a torch CUDA tensor.  `out` (numpy for device=-1, a torch CUDA float64 tensor otherwise) is written
        in place with row pitch `pitch` >= n and returned whole."""
        if sources is not None:
            sources = np.ascontiguousarray(sources, np.int32).reshape(-1)
        nsrc = self.n if sources is None else len(sources)
        pitch = self.n if pitch is None else int(pitch)
        if self.device < 0:
            if as_torch:
                raise ValueError("host evaluation returns numpy arrays")
            if out is None:
                out = np.empty((nsrc, pitch), np.float64)
            C.check(C.lib().gw_geo_query(self._h, C.ptr(sources), nsrc, C.ptr(out), pitch, None), geo=self._h)
            return out
        dev = f"cuda:{self.device}"
        src = None if sources is None else torch.as_tensor(sources, device=dev)
        if out is None:
            out = torch.empty((nsrc, pitch), dtype=torch.float64, device=dev)
        if stream is None:
            stream = ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        C.check(C.lib().gw_geo_query(self._h, C.ptr(src), nsrc, C.ptr(out), pitch, stream), geo=self._h)
        return out if as_torch else out.cpu().numpy()

    def stats(self):
        """The gw_geo_stats_t: the graph's entries and components, and the last query's rounds_max, relaxations and
        fallbacks."""
        st = C.GeoStats()
        C.check(C.lib().gw_geo_stats(self._h, ctypes.byref(st)), geo=self._h)
        return st

    def tiles(self):
        """{'lanes', 'lds_rows', 'sources_per_launch'}: k_geo_main's geometry."""
        v = [ctypes.c_int32() for _ in range(3)]
        C.check(C.lib().gw_geo_tiles(self._h, *[ctypes.byref(t) for t in v]), geo=self._h)
        return dict(zip(("lanes", "lds_rows", "sources_per_launch"), (t.value for t in v)))

    def kernel_attrs(self):
        """{kernel name: {'vgprs', 'scratch_bytes', 'lds_bytes'}} (hipFuncGetAttributes)."""
        cap = 16
        names = (ctypes.c_char_p * cap)()
        v, s, l = ((ctypes.c_int32 * cap)() for _ in range(3))
        n = ctypes.c_int32()
        C.check(C.lib().gw_geo_kernel_attrs(self._h, cap, names, v, s, l, ctypes.byref(n)), geo=self._h)
        return {names[i].decode(): {"vgprs": v[i], "scratch_bytes": s[i], "lds_bytes": l[i]}
                for i in range(min(n.value, cap))}

    def free(self):
        if getattr(self, "_h", None):
            C.lib().gw_geo_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass


def geodesic_distances(rows_or_graph, sources=None, device=0, **kw):
    """Distances float64 [nsrc][n] over top-k rows `(ids, values)` or a graph (a GWGraph, or a dict with 'offsets',
    'nbrs' and optionally 'weights', read as lengths).  kw: symmetrize, squared, delta."""
    if isinstance(rows_or_graph, (tuple, list)):
        ids, values = rows_or_graph
        m = Geodesics(len(ids), device=device, **kw)
        m.set_rows(ids, values)
    else:
        csr = rows_or_graph.export_csr() if hasattr(rows_or_graph, "export_csr") else rows_or_graph
        m = Geodesics(len(csr["offsets"]) - 1, device=device, **kw)
        m.set_csr(csr["offsets"], csr["nbrs"], csr.get("weights"))
    try:
        return m.query(sources)
    finally:
        m.free()
