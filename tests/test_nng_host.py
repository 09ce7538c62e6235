"""CPU: the neighbour graph of points on the host (gw_nng_*, device = -1) - exact on an integer grid, against a
numpy fp64 restatement on Gaussian rows, include_self, duplicates, the heat weights at their ends, padding, NaN and
inf rows, the error paths, struct_size versioning, determinism, and the stand-alone check under sanitizers.

The law (csrc/gw_nng_law.h): d2(i,j) is a chain of e = x_i[k] - x_j[k], fma(e, e, acc) over k ascending in fp64 on
the widened fp32 features; a row lists candidates j != v with a finite d2 by d2 ascending, then id ascending; with
include_self the source itself is entry 0 at d2 0, weight 1; w = exp(-(d2 / t)) (t = 0: 1); (-1, 0.0) padding.
"""
import ctypes
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG, ROOT


def _C():
    from gwamd import _lib as C
    C.lib()
    return C


def _P():
    from gwamd import pointgraph
    _C()
    return pointgraph


def numpy_rows(x, topk, t, include_self, sources=None):
    """The law restated in numpy fp64: (ids, weights, d2).  Sums are numpy's, not the fma chain."""
    x = np.asarray(x, np.float64)
    n = len(x)
    src = np.arange(n) if sources is None else np.asarray(sources)
    ids = np.full((len(src), topk), -1, np.int32)
    w = np.zeros((len(src), topk))
    dd = np.zeros((len(src), topk))
    for r, v in enumerate(src):
        with np.errstate(invalid="ignore", over="ignore"):
            d2 = ((x[v] - x) ** 2).sum(1)
        d2[v] = np.nan
        cand = np.nonzero(np.isfinite(d2))[0]
        o = cand[np.argsort(d2[cand], kind="stable")][:topk - include_self]
        if include_self:
            ids[r, 0], w[r, 0] = v, 1.0
        s = slice(include_self, include_self + len(o))
        ids[r, s] = o
        dd[r, s] = d2[o]
        w[r, s] = np.exp(-(d2[o] / t)) if t > 0 else 1.0
    return ids, w, dd


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.int64), np.asarray(b, np.float64).view(np.int64))


def grid(seed=3):
    """Integer coordinates: every e, e * e and partial sum is a small integer, so any order gives the same bits."""
    rng = np.random.default_rng(seed)
    x = rng.integers(-4, 5, (300, 5)).astype(np.float32)
    x[17] = x[5]
    x[123] = x[5]
    x[299] = x[200]
    return x


# ---- 1: integer grid, exact ------------------------------------------------------------------
@pytest.mark.parametrize("include_self", [True, False])
@pytest.mark.parametrize("topk", [8, 301])
def test_integer_grid_is_exact(topk, include_self):
    P = _P()
    x = grid()
    ids, w, d2 = P.knn_graph(x, topk, 15.0, include_self=include_self, device=-1, d2=True)
    rid, rw, rd2 = numpy_rows(x, topk, 15.0, int(include_self))
    assert np.array_equal(ids, rid)
    assert same_bits(d2, rd2)                                   # exact
    assert np.abs(w - rw).max() <= 4 * 2.0 ** -53               # the project's exp against libm's: a few ulp below 1
    listed = (ids >= 0).sum(1)
    assert (listed == min(topk, 299 + include_self)).all()
    assert (w[ids < 0] == 0.0).all() and (d2[ids < 0] == 0.0).all()
    if include_self:
        assert np.array_equal(ids[:, 0], np.arange(300)) and (w[:, 0] == 1.0).all() and (d2[:, 0] == 0.0).all()
    else:
        assert not (ids == np.arange(300)[:, None]).any()


# ---- 2: Gaussian rows against numpy fp64 ----------------------------------------------------------
@pytest.mark.parametrize("V,d,topk,seed", [(500, 3, 10, 0), (400, 130, 20, 1), (300, 17, 8, 2)])
def test_gaussian_against_numpy_fp64(V, d, topk, seed):
    """Both sides subtract exactly (fp32 features in fp64) and add `d` non-negative terms, each rounded once or
    twice to 2^-53: the two d2 differ by at most d * 2^-52 * d2.  Ids may differ only inside such a near-tie."""
    P = _P()
    x = np.random.default_rng(seed).standard_normal((V, d)).astype(np.float32)
    ids, w, d2 = P.knn_graph(x, topk, 2.0 * d, include_self=False, device=-1, d2=True)
    rid, rw, rd2 = numpy_rows(x, topk, 2.0 * d, 0)
    bound = d * 2.0 ** -52
    differ = 0
    for r in range(V):
        for t in range(topk):
            if ids[r, t] != rid[r, t]:
                differ += 1
                alt = ((x[r].astype(np.float64) - x[ids[r, t]].astype(np.float64)) ** 2).sum()
                assert abs(alt - rd2[r, t]) <= bound * rd2[r, t], (r, t)
            assert abs(d2[r, t] - rd2[r, t]) <= bound * max(rd2[r, t], d2[r, t]), (r, t)
    print(f"({V}, {d}): {differ} entries differ inside near-ties; max relative d2 difference "
          f"{(np.abs(d2 - rd2) / rd2).max():.2e} (bound {bound:.2e})")
    assert np.allclose(w, np.exp(-d2 / (2.0 * d)), rtol=1e-15, atol=0)   # gw_ovr_exp and libm: a few 2^-53 apart


# ---- 3: include_self, duplicates ----------------------------------------------------------------------
def test_include_self_shifts_the_row_by_one():
    P = _P()
    x = np.random.default_rng(4).standard_normal((80, 6)).astype(np.float32)
    a = P.knn_graph(x, 7, 3.0, include_self=True, device=-1, d2=True)
    b = P.knn_graph(x, 6, 3.0, include_self=False, device=-1, d2=True)
    assert np.array_equal(a[0][:, 1:], b[0]) and same_bits(a[1][:, 1:], b[1]) and same_bits(a[2][:, 1:], b[2])
    assert np.array_equal(a[0][:, 0], np.arange(80)) and (a[1][:, 0] == 1.0).all() and (a[2][:, 0] == 0.0).all()
    one = P.knn_graph(x, 1, 3.0, include_self=True, device=-1)      # topk = 1: the point alone
    assert np.array_equal(one[0][:, 0], np.arange(80)) and (one[1] == 1.0).all()


def test_duplicates_are_at_zero_by_ascending_id_with_weight_one():
    P = _P()
    x = np.random.default_rng(5).standard_normal((50, 4)).astype(np.float32)
    for v in (3, 31, 49, 12):
        x[v] = x[20]
    ids, w, d2 = P.knn_graph(x, 6, 0.25, include_self=True, device=-1, d2=True)
    assert list(ids[20][:5]) == [20, 3, 12, 31, 49]
    assert (d2[20][:5] == 0.0).all() and not np.signbit(d2[20][:5]).any() and (w[20][:5] == 1.0).all()
    assert list(ids[31][:5]) == [31, 3, 12, 20, 49]
    ids, w, d2 = P.knn_graph(x, 4, 0.25, include_self=False, device=-1, d2=True)
    assert list(ids[3]) == [12, 20, 31, 49] and (w[3] == 1.0).all()
    # d2(i, j) and d2(j, i) have the same bits
    ids, w, d2 = P.knn_graph(x, 50, 1.0, include_self=False, device=-1, d2=True)
    D = np.zeros((50, 50))
    for v in range(50):
        D[v, ids[v, :49]] = d2[v, :49]
    assert same_bits(D, D.T)


# ---- 4: the weights at their ends ------------------------------------------------------------------------
def test_heat_zero_is_unit_weights_and_a_tiny_heat_is_plus_zero():
    P = _P()
    x = np.random.default_rng(6).standard_normal((40, 3)).astype(np.float32)
    x[7] = x[8]
    ids, w, d2 = P.knn_graph(x, 5, 0.0, include_self=True, device=-1, d2=True)
    assert (w == 1.0).all() and (d2[:, 1:] >= 0).all()
    ids3, w3 = P.knn_graph(x, 5, float("inf"), include_self=True, device=-1)     # d2 / inf = 0: exp(-0) is exactly 1
    assert np.array_equal(ids3, ids) and (w3 == 1.0).all()
    ids2, w2, d22 = P.knn_graph(x, 5, 1e-9, include_self=True, device=-1, d2=True)
    assert np.array_equal(ids, ids2) and same_bits(d2, d22)          # listed all the same
    far = d22 / 1e-9 > 700
    assert far.any() and (w2[far] == 0.0).all() and not np.signbit(w2[far]).any()
    assert w2[7, 1] == 1.0 and ids2[7, 1] == 8 and (w2[:, 0] == 1.0).all()
    # such a weight is no edge for gw_le: every row but 7 and 8 keeps its self-loop alone
    from gwamd.eigenmaps import Eigenmaps
    m = Eigenmaps(40, device=-1, dim=1, block=2, self_loops=1)
    m.set_rows(ids2, w2)
    y = m.apply(np.ones((40, 1)))
    assert np.allclose(y, 1.0, rtol=1e-15)                           # S = I off the pair, [[.5, .5], [.5, .5]] on it
    m.free()


def test_topk_beyond_n_pads():
    P = _P()
    x = np.random.default_rng(7).standard_normal((5, 2)).astype(np.float32)
    for self_, listed in ((True, 5), (False, 4)):
        ids, w, d2 = P.knn_graph(x, 9, 1.0, include_self=self_, device=-1, d2=True)
        assert ((ids >= 0).sum(1) == listed).all()
        assert (ids[:, listed:] == -1).all() and (w[:, listed:] == 0.0).all() and (d2[:, listed:] == 0.0).all()
    ids, w = P.knn_graph(x[:1], 3, 1.0, include_self=True, device=-1)      # n = 1
    assert list(ids[0]) == [0, -1, -1] and list(w[0]) == [1.0, 0.0, 0.0]
    ids, w = P.knn_graph(x[:1], 3, 1.0, include_self=False, device=-1)
    assert list(ids[0]) == [-1, -1, -1]


def test_nan_and_inf_rows_are_nobodys_neighbours():
    P = _P()
    x = np.random.default_rng(8).standard_normal((30, 3)).astype(np.float32)
    x[4, 1] = np.nan
    x[9, 0] = np.inf
    x[10] = 3e38                                 # the largest fp32 magnitudes: d2 near 1e77 stays finite in fp64
    ids, w, d2 = P.knn_graph(x, 30, 1.0, include_self=True, device=-1, d2=True)
    rid, rw, rd2 = numpy_rows(x, 30, 1.0, 1)
    assert np.array_equal(ids, rid)
    for v in (4, 9):
        assert list(ids[v]) == [v] + [-1] * 29 and w[v, 0] == 1.0      # the row lists itself alone
        assert not (ids[np.arange(30) != v] == v).any()
    assert ((ids >= 0).sum(1)[[0, 1, 10, 29]] == 28).all() and np.isfinite(d2).all()
    assert ids[0, 27] == 10 and d2[0, 27] > 1e76 and w[0, 27] == 0.0


# ---- 5: sources, pitch --------------------------------------------------------------------------------------
def test_sources_repeat_unordered_and_pitch():
    P = _P()
    x = np.random.default_rng(9).standard_normal((60, 7)).astype(np.float32)
    wide = np.full((60, 10), np.nan, np.float32)
    wide[:, :7] = x
    src = np.array([59, 3, 3, 0, 41, 59], np.int32)
    full = P.knn_graph(x, 5, 2.0, device=-1, d2=True)
    a = P.knn_graph(x, 5, 2.0, sources=src, device=-1, d2=True)
    assert np.array_equal(a[0], full[0][src]) and same_bits(a[1], full[1][src]) and same_bits(a[2], full[2][src])
    m = P.PointGraph(60, device=-1, dim=7, topk=5, heat_t=2.0)
    m.set_vectors(wide[:, :7])       # pitch 10: the NaN pads are never read
    b = m.query(src)
    assert np.array_equal(a[0], b[0]) and same_bits(a[1], b[1])
    flat = np.full(60 * 10 - 3, np.nan, np.float32)   # the last row allocated without its pad
    flat[:] = wide.reshape(-1)[:597]
    m.set_vectors(flat.ctypes.data, pitch=10)
    c = m.query(src)
    assert np.array_equal(a[0], c[0]) and same_bits(a[1], c[1])
    m.free()


# ---- 6: error paths ---------------------------------------------------------------------------------------------
def test_errors():
    C, P = _C(), _P()
    L = C.lib()
    x = np.random.default_rng(10).standard_normal((30, 4)).astype(np.float32)
    m = P.PointGraph(30, device=-1, dim=4, topk=3, heat_t=1.0)
    with pytest.raises(C.StateError):
        m.query()
    m.set_vectors(x)
    ids = np.full((3, 3), 77, np.int32)
    w = np.full((3, 3), 77.0)
    dd = np.full((3, 3), 77.0)
    for v in (30, -1):
        src = np.array([1, v, 2], np.int32)
        assert L.gw_nng_query(m.handle, C.ptr(src), 3, C.ptr(ids), C.ptr(w), C.ptr(dd), None) == C.GW_ERR_RANGE
        assert (ids == 77).all() and (w == 77.0).all() and (dd == 77.0).all()     # checked before anything is written
        with pytest.raises(IndexError):
            m.query(src)
    src = np.array([1, 2, 3], np.int32)
    assert L.gw_nng_query(m.handle, C.ptr(src), 0, None, None, None, None) == C.GW_OK        # nsrc = 0: a no-op
    assert L.gw_nng_query(m.handle, C.ptr(src), 0, C.ptr(ids), C.ptr(w), None, None) == C.GW_OK and (ids == 77).all()
    assert L.gw_nng_query(m.handle, C.ptr(src), -1, C.ptr(ids), C.ptr(w), None, None) == C.GW_ERR_INVALID
    assert L.gw_nng_query(m.handle, C.ptr(src), 3, None, C.ptr(w), None, None) == C.GW_ERR_INVALID
    assert L.gw_nng_query(m.handle, C.ptr(src), 3, C.ptr(ids), C.ptr(w), None, None) == C.GW_OK   # out_d2 is optional
    assert L.gw_nng_set_vectors(m.handle, C.ptr(x), 3) == C.GW_ERR_INVALID             # pitch below dim
    assert L.gw_nng_set_vectors(m.handle, None, 4) == C.GW_ERR_INVALID
    with pytest.raises(C.StateError):
        m.tiles()
    with pytest.raises(C.StateError):
        m.kernel_attrs()
    m.set_rows(20)                                           # another row count: the vectors must be set again
    with pytest.raises(C.StateError):
        m.query()
    m.set_vectors(x[:20])
    assert np.array_equal(m.query()[0], P.knn_graph(x[:20], 3, 1.0, device=-1)[0])
    m.free()
    h = ctypes.c_void_p()
    for kw in (dict(dim=0), dict(topk=0), dict(dim=-3), dict(include_self=2), dict(include_self=-1),
               dict(heat_t=-1.0), dict(heat_t=float("nan")), dict(heat_t=-0.5e-300)):
        p = C.NngParams(**kw)
        assert L.gw_nng_create(-1, 10, ctypes.byref(p), ctypes.byref(h)) == C.GW_ERR_INVALID, kw
    p = C.NngParams()
    p.struct_size = 3
    assert L.gw_nng_create(-1, 10, ctypes.byref(p), ctypes.byref(h)) == C.GW_ERR_INVALID
    assert b"struct_size" in L.gw_nng_last_error(None)
    p = C.NngParams()
    assert L.gw_nng_create(-1, 0, ctypes.byref(p), ctypes.byref(h)) == C.GW_ERR_INVALID
    assert L.gw_nng_create(-2, 10, ctypes.byref(p), ctypes.byref(h)) == C.GW_ERR_INVALID
    # the device limits are checked before any device is touched; the host path takes any size
    for kw, n in ((dict(dim=1025), 10), (dict(topk=129), 10), (dict(), 1 << 31)):
        p = C.NngParams(**kw)
        assert L.gw_nng_create(0, n, ctypes.byref(p), ctypes.byref(h)) == C.GW_ERR_UNSUPPORTED
        assert L.gw_nng_create(-1, n, ctypes.byref(p), ctypes.byref(h)) == C.GW_OK
        L.gw_nng_free(h)


def test_struct_size_shorter_than_the_librarys():
    """Only struct_size bytes are read: what lies past them keeps the defaults (include_self 1, heat_t 0)."""
    C, P = _C(), _P()
    L = C.lib()
    p = C.NngParams(dim=4, topk=6, include_self=0, heat_t=-3.0)
    p.struct_size = 12      # struct_size, dim, topk
    h = ctypes.c_void_p()
    assert L.gw_nng_create(-1, 40, ctypes.byref(p), ctypes.byref(h)) == C.GW_OK
    x = np.random.default_rng(11).standard_normal((40, 4)).astype(np.float32)
    ids, w = np.empty((40, 6), np.int32), np.empty((40, 6))
    assert L.gw_nng_set_vectors(h, C.ptr(x), 4) == 0
    assert L.gw_nng_query(h, None, 0, C.ptr(ids), C.ptr(w), None, None) == 0
    L.gw_nng_free(h)
    ref = P.knn_graph(x, 6, 0.0, include_self=True, device=-1)
    assert np.array_equal(ids, ref[0]) and same_bits(w, ref[1])
    assert ctypes.sizeof(C.NngParams) == 24 and C.NngParams.heat_t.offset == 16


# ---- 7: determinism ------------------------------------------------------------------------------------------------
def _digest():
    x = np.random.default_rng(12).standard_normal((700, 9)).astype(np.float32)
    x[100:110] = x[5]
    out = _P().knn_graph(x, 12, 4.0, device=-1, d2=True)
    return hashlib.sha256(b"".join(a.tobytes() for a in out)).hexdigest()


CHILD = """
import sys
sys.path[:0] = [{root!r}, {pkg!r}, {tests!r}]
import test_nng_host as T
print(T._digest())
"""


def test_same_bits_for_any_thread_count():
    first = _digest()
    assert _digest() == first
    code = CHILD.format(root=ROOT, pkg=PKG, tests=os.path.join(ROOT, "tests"))
    for threads in ("1", "4"):
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True,
                           env=dict(os.environ, OMP_NUM_THREADS=threads))
        assert r.returncode == 0, r.stderr
        assert r.stdout.split()[-1] == first, threads


# ---- 8: the writers take the rows as they are -------------------------------------------------------------------------
def test_round_trip_through_the_sim_text_writer(tmp_path):
    from gwamd import neighbors
    P = _P()
    x = np.random.default_rng(13).standard_normal((30, 3)).astype(np.float32)
    ids, w = P.knn_graph(x, 4, 2.0, device=-1)
    path = str(tmp_path / "x.nng")
    neighbors.write_neighbors(path, ids, w)
    first = open(path + ".sim.txt", newline="").read().split("\r\n")[0].split(",")
    assert first[0] == "0" and first[1] == "0:1.000000" and first[2] == f"{ids[0, 1]}:{w[0, 1]:.6f}"


def test_make_swiss_roll():
    P = _P()
    X, t = P.make_swiss_roll(50, seed=3, height=20.0)
    rng = np.random.RandomState(3)
    tt = 1.5 * np.pi * (1 + 2 * rng.rand(1, 50))
    yy = 20.0 * rng.rand(1, 50)
    assert X.shape == (50, 3) and np.array_equal(t, tt[0]) and np.array_equal(X[:, 1], yy[0])
    assert np.array_equal(X[:, 0], (tt * np.cos(tt))[0]) and np.array_equal(X[:, 2], (tt * np.sin(tt))[0])
    Xn, _ = P.make_swiss_roll(50, noise=0.1, seed=3)
    assert np.abs(Xn[:, 0] - X[:, 0]).max() > 0 and np.abs(Xn[:, 0] - X[:, 0]).max() < 1.0
    assert np.allclose(P.make_swiss_roll(50, seed=3)[0][:, 1], 5.0 * X[:, 1], rtol=1e-15, atol=0)   # the reference's height 100


# ---- 9: sanitizers ----------------------------------------------------------------------------------------
def test_host_check_under_sanitizers(tmp_path):
    """gw_nng_host.cpp + host/nng_host_check.cpp (its own main) under ASan + UBSan, run as a plain program."""
    exe = str(tmp_path / "nng_host_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-static-libasan", "-static-libubsan",
           "-ffp-contract=off", "-DGW_NNG_HOST_ONLY", f"-I{os.path.join(ROOT, 'include')}",
           os.path.join(PKG, "csrc", "gw_nng_host.cpp"), os.path.join(PKG, "host", "nng_host_check.cpp"),
           "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "nng host check ok" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr
