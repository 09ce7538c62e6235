"""GPU: the geodesic kernels (gw_geo.hip) against the host evaluation of the law (device = -1, binary-heap Dijkstra),
bit for bit on int64 views.  The graphs are synthetic CSRs through set_csr: v <-> v+1 plus 3 seeded random partners per
vertex, lengths uniform in [0.5, 1.5), unless said otherwise.  The shapes sit on the edges of the geometry
gw_geo_tiles reports: LANES threads scan 64 vertices each per trip, LDS_ROWS is the last n kept in LDS, SPL the grid's
bound (test_tiles holds the constants below to it)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LANES, LDS_ROWS, SPL = 256, 7936, 1024


def G():
    from gwamd import _lib as C
    from gwamd import geodesics
    C.lib()
    return geodesics


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def graph(n, seed=0, partners=3, length=None):
    """(offsets, nbrs, lengths) of the chain v -> v+1 plus `partners` random partners per vertex (union makes every
    edge two-way); length: a constant instead of uniform [0.5, 1.5)."""
    rng = np.random.RandomState(seed)
    r = np.concatenate([np.arange(n - 1), np.repeat(np.arange(n), partners if n > 1 else 0)])
    c = np.concatenate([np.arange(1, n), rng.randint(0, n, len(r) - (n - 1))])
    l = 0.5 + rng.rand(len(r)) if length is None else np.full(len(r), float(length))
    return csr(n, r, c, l)


def csr(n, r, c, l):
    order = np.argsort(r, kind="stable")
    off = np.zeros(n + 1, np.int64)
    np.add.at(off, np.asarray(r, np.int64) + 1, 1)
    return np.cumsum(off), np.asarray(c, np.int32)[order], np.asarray(l, np.float64)[order]


def both(n, g, sources, **kw):
    """(device distances, host distances, device stats) of the same graph and sources."""
    geo = G()
    out = []
    for device in (0, -1):
        m = geo.Geodesics(n, device=device, **(kw if device == 0 else
                                               {k: v for k, v in kw.items() if k in ("symmetrize", "squared")}))
        m.set_csr(*g)
        out.append(m.query(sources))
        if device == 0:
            st = m.stats()
        m.free()
    return out[0], out[1], st


def same(n, g, sources, **kw):
    d, h, st = both(n, g, sources, **kw)
    assert d.shape == h.shape and np.array_equal(bits(d), bits(h))
    return d, st


def test_tiles():
    m = G().Geodesics(4, device=0)
    assert m.tiles() == {"lanes": LANES, "lds_rows": LDS_ROWS, "sources_per_launch": SPL}
    m.free()


@pytest.mark.parametrize("n", [1, 2, LANES - 1, LANES, LANES + 1, 64 * LANES + 1])
def test_rows_at_the_scan_edges(n):
    same(n, graph(n, seed=n), sorted({0, n // 2, n - 1}))


@pytest.mark.parametrize("n", [LDS_ROWS - 1, LDS_ROWS, LDS_ROWS + 1])
def test_both_sides_of_the_lds_switch(n):
    same(n, graph(n, seed=n), [0, n // 3, n - 1])


@pytest.fixture(scope="module")
def g300():
    geo = G()
    g = graph(300, seed=7)
    m = geo.Geodesics(300, device=-1)
    m.set_csr(*g)
    return g, m.query()


@pytest.mark.parametrize("nsrc", [1, SPL - 1, SPL, SPL + 1, 2 * SPL + 1])
def test_sources_past_the_grid(g300, nsrc):
    g, H = g300
    src = np.random.RandomState(nsrc).randint(0, 300, nsrc)  # repeated and unordered
    m = G().Geodesics(300, device=0)
    m.set_csr(*g)
    assert np.array_equal(bits(m.query(src)), bits(H[src]))
    m.free()


def test_every_vertex_as_source(g300):
    g, H = g300
    m = G().Geodesics(300, device=0)
    m.set_csr(*g)
    assert np.array_equal(bits(m.query()), bits(H))
    t = m.query(as_torch=True)
    assert t.is_cuda and np.array_equal(bits(t.cpu().numpy()), bits(H))
    m.free()


def chain(n):
    rng = np.random.RandomState(11)
    return csr(n, np.arange(n - 1), np.arange(1, n), 0.5 + rng.rand(n - 1))


def test_the_round_bound_on_a_chain():
    """Hop diameter n - 1: pure Bellman-Ford (a huge delta) and one advance per vertex (delta 1e-9) give the same bits,
    and neither reaches the cap."""
    n = 3000
    a, sa = same(n, chain(n), [0, n - 1, n // 2], delta=1e300)
    b, sb = same(n, chain(n), [0, n - 1, n // 2], delta=1e-9)
    print(f"chain n={n}: rounds_max {sa.rounds_max} (delta 1e300), {sb.rounds_max} (delta 1e-9); relaxations "
          f"{sa.relaxations}, {sb.relaxations}; fallbacks {sa.fallbacks}, {sb.fallbacks}")
    assert np.array_equal(bits(a), bits(b))
    assert sa.fallbacks == 0 and sa.rounds_max <= n + 1


def test_the_fallback():
    """round_cap = 1 puts the cap at 0: every source runs as Bellman-Ford from its first round, within n rounds."""
    n = 3000
    d, st = same(n, chain(n), [0, n - 1], round_cap=1)
    print(f"fallback: rounds_max {st.rounds_max}, fallbacks {st.fallbacks}")
    assert st.fallbacks == 2 and st.rounds_max <= n
    same(300, graph(300, seed=7), [3, 299], round_cap=1, delta=1e-9)
    same(1, graph(1), [0], round_cap=1)


def test_a_star():
    n = 5000
    g = csr(n, np.zeros(n - 1, np.int64), np.arange(1, n), 0.5 + np.random.RandomState(5).rand(n - 1))
    same(n, g, [0, 1, n - 1])


def test_law_edge_cases():
    n = 300
    off, nb, l = graph(n, seed=3)
    z = l.copy()
    z[::3] = 0.0  # zero-length edges, as duplicate points give
    same(n, (off, nb, z), [0, 150, 299])
    same(n, graph(n, seed=3, length=1.0), [0, 150, 299])  # every path of equal hops ties
    w = l.copy()
    w[0::4], w[1::4], w[2::4] = 1e-310, 1e-300, 1e300
    same(n, (off, nb, w), [0, 150, 299])
    big = np.full(len(l), 1.5e308)  # two hops overflow: unreachable
    d, _ = same(n, (off, nb, big), [0])
    assert np.isinf(d).any()


def test_two_components_and_an_isolated_source():
    n = 401  # 0 .. 199, 200 .. 399, and 400 alone
    o1, n1, l1 = graph(200, seed=1)
    o2, n2, l2 = graph(200, seed=2)
    off = np.concatenate([o1, o1[-1] + o2[1:], [o1[-1] + o2[-1]]])
    g = (off, np.concatenate([n1, n2 + 200]).astype(np.int32), np.concatenate([l1, l2]))
    d, _ = same(n, g, [0, 399, 400])
    assert np.isinf(d[0, 200:]).all() and np.isfinite(d[0, :200]).all()
    assert d[2, 400] == 0.0 and np.isinf(d[2, :400]).all()
    geo = G()
    hd, hh = geo.Geodesics(n, device=0), geo.Geodesics(n, device=-1)
    for m in (hd, hh):
        m.set_csr(*g)
    assert np.array_equal(hd.components()[0], hh.components()[0]) and hd.components()[1] == 0
    hd.free()


@pytest.mark.parametrize("delta", [0.0, 1e-300, 1e300])
def test_delta_never_changes_a_result(g300, delta):
    g, H = g300
    m = G().Geodesics(300, device=0, delta=delta)
    m.set_csr(*g)
    assert np.array_equal(bits(m.query([0, 17, 299])), bits(H[[0, 17, 299]]))
    m.free()


def test_pitch_and_errors(g300):
    import torch
    from gwamd import _lib as C
    g, H = g300
    m = G().Geodesics(300, device=0)
    with pytest.raises(C.StateError):
        m.query([0])
    m.set_csr(*g)
    out = torch.full((4, 303), float("nan"), dtype=torch.float64, device="cuda:0")
    got = m.query([5, 5, 0, 299], out=out, pitch=303)
    assert np.array_equal(bits(got[:, :300]), bits(H[[5, 5, 0, 299]])) and np.isnan(got[:, 300:]).all()
    out = torch.full((2, 300), -3.0, dtype=torch.float64, device="cuda:0")
    for bad in ([0, 300], [-1, 0]):
        with pytest.raises(IndexError):
            m.query(bad, out=out)
        assert bool((out == -3.0).all())
    src = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    assert C.lib().gw_geo_query(m.handle, C.ptr(src), 0, C.ptr(out), 300, None) == 0
    assert bool((out == -3.0).all())
    m.free()


def test_kernel_attrs():
    m = G().Geodesics(300, device=0)
    attrs = m.kernel_attrs()
    print(attrs)
    assert set(attrs) == {"k_geo_check", "k_geo_main_lds", "k_geo_main_global"}
    assert attrs["k_geo_main_lds"]["lds_bytes"] <= 65536
    m.free()
