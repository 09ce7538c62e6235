"""GPU: the neighbour-graph kernels (gw_nng.hip) against the host evaluation of the law (device = -1), bit for bit:
ids array_equal, squared distances and weights as int64 views.  The shapes sit on the edges of the launch geometry
gw_nng_tiles reports (tq source rows per workgroup, tc candidates per tile, kc columns per LDS chunk, buf entries
of a row's candidate buffer).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _P():
    from gwamd import _lib as C
    from gwamd import pointgraph
    C.lib()
    return pointgraph


_tiles = {}


def tiles(topk=20):
    if topk not in _tiles:
        m = _P().PointGraph(4, device=0, dim=4, topk=topk)
        _tiles[topk] = m.tiles()
        m.free()
    return _tiles[topk]


def padded(x, pad=3, lead=0):
    """x on the GPU with pitch dim + pad, the pad columns NaN, the last row allocated without its pad, after `lead`
    floats (lead = 1: the base address is 4 B past a 16 B boundary): (tensor that owns the memory, address, pitch)."""
    import torch
    n, d = x.shape
    flat = np.full(lead + n * (d + pad) - pad, np.nan, np.float32)
    for v in range(n):
        flat[lead + v * (d + pad):lead + v * (d + pad) + d] = x[v]
    t = torch.as_tensor(flat, device="cuda:0")
    return t, t.data_ptr() + 4 * lead, d + pad


def both(x, topk, heat=15.0, include_self=True, sources=None, pad=3, lead=0):
    """(device ids, weights, d2), (host ids, weights, d2) of the same query; the device reads a padded matrix."""
    P = _P()
    n, d = x.shape
    t, addr, pitch = padded(x, pad, lead)
    dev = P.PointGraph(n, device=0, dim=d, topk=topk, include_self=include_self, heat_t=heat)
    dev.set_vectors(addr, pitch=pitch)
    got = dev.query(sources, d2=True)
    dev.free()
    del t
    host = P.PointGraph(n, device=-1, dim=d, topk=topk, include_self=include_self, heat_t=heat)
    host.set_vectors(np.ascontiguousarray(x))
    want = host.query(sources, d2=True)
    host.free()
    return got, want


def assert_same(got, want):
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1].view(np.int64), want[1].view(np.int64))
    assert np.array_equal(got[2].view(np.int64), want[2].view(np.int64))


def test_geometry():
    t = tiles(20)
    print("gw_nng_tiles:", t, tiles(128))
    assert t["tq"] >= 2 and t["tc"] >= 2 and t["kc"] >= 2 and t["buf"] >= 20 and tiles(128)["buf"] >= 128


def edge_cases():
    """(n, sources, dim, topk, include_self, pad, lead) in terms of the geometry (tq 32, tc 128, kc 32 today): every
    n of {1, 2, tq-1, tq, tq+1, tc-1, tc, tc+1, 2tc+1}, all rows and repeated unordered subsets of 1, tq and tq+1
    sources, every dim of {1, 3, 4, kc-1, kc, kc+1, 2kc+1}, every topk of {1, 2, 64, 65, 128} and topk > n, both
    include_self values, 16 B-aligned rows (pad 0 with dim % 4 == 0: the float4 path) and unaligned ones (odd pitch or
    a base 4 B off: the scalar path), pruned to a dozen."""
    t = tiles()
    tq, tc, kc = t["tq"], t["tc"], t["kc"]
    return [(1, None, 1, 1, True, 3, 0), (1, None, 3, 2, False, 0, 1), (2, None, 4, 2, True, 0, 0),
            (tq - 1, 1, kc - 1, 64, False, 3, 0), (tq, None, kc, 65, True, 0, 0), (tq + 1, tq + 1, kc + 1, 128, True, 3, 1),
            (tc - 1, tq, 3, 128, False, 1, 0), (tc, None, 4, 1, False, 0, 1), (tc + 1, tq + 1, 2 * kc + 1, 64, True, 2, 0),
            (2 * tc + 1, None, kc, 128, False, 4, 0), (2 * tc + 1, tq, 1, 65, True, 3, 0),
            (2 * tc + 1, 1, 2 * kc + 1, 2, False, 0, 1), (tc + 1, None, kc + 1, 2, True, 0, 0)]


@pytest.mark.parametrize("case", range(13))
def test_edge_shapes(case):
    n, ns, d, topk, self_, pad, lead = edge_cases()[case]
    rng = np.random.default_rng(100 + case)
    x = rng.standard_normal((n, d)).astype(np.float32)
    src = None if ns is None else rng.integers(0, n, ns).astype(np.int32)     # unordered, may repeat
    if ns is not None and ns > 1:
        src[-1] = src[0]                                                     # and does repeat
    got, want = both(x, topk, 2.0 * d, self_, src, pad, lead)
    assert_same(got, want)
    assert (got[0] >= 0).sum(1).max() == min(topk, n - 1 + self_)


@pytest.mark.parametrize("order", ["closer", "farther"])
@pytest.mark.parametrize("topk", [1, 20, 128])
def test_selection_at_its_worst_and_the_mirror(order, topk):
    """Points on a line.  'closer': seen from row 0's side the ids run towards the sources, so every tile brings
    candidates nearer than all before and every pass appends and compacts; 'farther' is the mirror, where after the
    first tile nothing passes the bound."""
    tc = tiles()["tc"]
    n = 5 * tc + 7
    pos = np.arange(n, dtype=np.float64)
    coord = (n - pos) if order == "closer" else pos
    x = np.stack([coord, np.zeros(n)], axis=1).astype(np.float32)
    src = np.array([n - 1, n - 2, 0, 1, n // 2], np.int32) if order == "closer" else np.array([0, 1, n - 1, n // 2], np.int32)
    got, want = both(x, topk, 50.0, False, src)
    assert_same(got, want)
    want_first = {"closer": n - 2, "farther": 1}[order]
    assert got[0][0, 0] == want_first and got[2][0, 0] == 1.0


def test_all_rows_identical():
    """Every distance is 0: the order is the ids' alone, and the buffers fill with ties."""
    tc = tiles()["tc"]
    n = 2 * tc + 5
    x = np.tile(np.array([[0.5, -1.25, 3.0]], np.float32), (n, 1))
    for self_ in (True, False):
        got, want = both(x, 70, 1.0, self_)
        assert_same(got, want)
        assert (got[2] == 0.0).all() and (got[1] == 1.0).all()
        row = list(got[0][n - 1])
        assert row == ([n - 1] + list(range(69)) if self_ else list(range(70)))


def test_integer_grid_against_numpy():
    from test_nng_host import grid, numpy_rows
    x = grid()
    P = _P()
    ids, w, d2 = P.knn_graph(x, 24, 15.0, include_self=True, device=0, d2=True)
    rid, rw, rd2 = numpy_rows(x, 24, 15.0, 1)
    assert np.array_equal(ids, rid) and np.array_equal(d2, rd2)
    assert np.abs(w - rw).max() <= 4 * 2.0 ** -53


@pytest.mark.parametrize("heat", [0.0, 1e-9, 15.0])
def test_heat(heat):
    x = np.random.default_rng(7).standard_normal((200, 3)).astype(np.float32)
    x[50] = x[51]
    got, want = both(x, 10, heat, True)
    assert_same(got, want)
    if heat == 0.0:
        assert (got[1] == 1.0).all()
    if heat == 1e-9:
        assert got[1][50, 1] == 1.0 and (got[1][0, 1:] == 0.0).all() and (got[0][0] >= 0).all()


def test_a_nan_row():
    tc = tiles()["tc"]
    x = np.random.default_rng(8).standard_normal((tc + 9, 5)).astype(np.float32)
    x[3, 4] = np.nan
    x[tc + 2, 0] = np.inf
    got, want = both(x, 12, 4.0, True)
    assert_same(got, want)
    assert list(got[0][3]) == [3] + [-1] * 11 and not (got[0][np.arange(len(x)) != 3] == 3).any()
    assert not (got[0][np.arange(len(x)) != tc + 2] == tc + 2).any() and np.isfinite(got[2]).all()


def test_a_source_out_of_range_leaves_the_outputs_untouched():
    import torch
    from gwamd import _lib as C
    P = _P()
    x = torch.as_tensor(np.random.default_rng(9).standard_normal((40, 4)).astype(np.float32), device="cuda:0")
    m = P.PointGraph(40, device=0, dim=4, topk=3, heat_t=1.0)
    m.set_vectors(x)
    ids = torch.full((3, 3), 77, dtype=torch.int32, device="cuda:0")
    w = torch.full((3, 3), 77.0, dtype=torch.float64, device="cuda:0")
    d2 = torch.full((3, 3), 77.0, dtype=torch.float64, device="cuda:0")
    for v in (40, -1):
        src = torch.as_tensor(np.array([1, v, 2], np.int32), device="cuda:0")
        rc = C.lib().gw_nng_query(m.handle, C.ptr(src), 3, C.ptr(ids), C.ptr(w), C.ptr(d2), None)
        torch.cuda.synchronize()
        assert rc == C.GW_ERR_RANGE
        assert (ids == 77).all().item() and (w == 77.0).all().item() and (d2 == 77.0).all().item()
        with pytest.raises(IndexError):
            m.query(np.array([1, v, 2], np.int32))
    assert C.lib().gw_nng_query(m.handle, C.ptr(ids), 0, None, None, None, None) == C.GW_OK     # nsrc = 0
    ok = m.query(np.array([1, 39, 2], np.int32))                                               # out_d2 = NULL
    assert np.array_equal(ok[0][:, 0], [1, 39, 2])
    m.free()


def test_kernel_attrs():
    m = _P().PointGraph(300, device=0, dim=128, topk=128)
    a = m.kernel_attrs()
    m.free()
    print("gw_nng kernels:", a)
    assert sorted(a) == ["k_nng_check", "k_nng_main"]
    for name, k in a.items():
        assert k["scratch_bytes"] == 0, name
        assert 0 < k["vgprs"] <= 128, name           # two workgroups of 256 lanes per CU keep their registers
    assert a["k_nng_main"]["lds_bytes"] <= 160 * 1024
