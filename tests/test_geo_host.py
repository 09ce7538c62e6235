"""CPU: geodesics on a sparse graph, the host evaluation (gw_geo_*, device = -1): the law against two independent
statements of it, every input rule on a hand-made graph, and the API's contract."""

import numpy as np
import pytest

INF = np.inf


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


@pytest.fixture(scope="module")
def geo(gw):
    from gwamd import geodesics
    return geodesics


def rows(n, topk, entries):
    """ids / values [n][topk] from {row: [(id, value), ...]}, -1 / 0.0 padded."""
    ids = np.full((n, topk), -1, np.int32)
    val = np.zeros((n, topk), np.float64)
    for r, es in entries.items():
        for t, (i, v) in enumerate(es):
            ids[r, t], val[r, t] = i, v
    return ids, val


def dist(geo, n, topk, entries, sources=None, **kw):
    m = geo.Geodesics(n, device=-1, **kw)
    m.set_rows(*rows(n, topk, entries))
    return m.query(sources)


# ---- the law against an independent statement ----------------------------------------
def jacobi_bellman_ford(n, r, c, l):
    """All sources at once: D[s][v] = min(D[s][v], min over the entries (u, v) of D[s][u] + l(u, v)), every entry from
    the previous sweep's values, until nothing changes.  Every vertex must be some entry's target."""
    order = np.argsort(c, kind="stable")
    r, c, l = r[order], c[order], l[order]
    starts = np.searchsorted(c, np.arange(n))
    assert np.array_equal(c[starts], np.arange(n))
    D = np.full((n, n), INF)
    D[np.arange(n), np.arange(n)] = 0.0
    sweeps = 0
    while True:
        new = np.minimum(D, np.minimum.reduceat(D[:, r] + l[None, :], starts, axis=1))
        sweeps += 1
        if np.array_equal(new, D):
            return D, sweeps
        D = new


def test_law_matches_bellman_ford_and_scipy(geo):
    from gwamd import pointgraph
    n, k = 600, 6
    X = pointgraph.make_swiss_roll(n, seed=0)[0].astype(np.float32)
    ids, _, d2 = pointgraph.knn_graph(X, k, 0.0, include_self=False, device=-1, d2=True)
    m = geo.Geodesics(n, device=-1, squared=True, symmetrize="union")
    m.set_rows(ids, d2)
    comp, main = m.components()
    assert main == 0 and np.all(comp == 0) and m.stats().components == 1  # connected
    D = m.query()
    # the symmetrised graph, built here from the rows: l_ij = min of the listed a_ij and a_ji
    A = np.full((n, n), INF)
    ln = np.sqrt(d2)
    for i in range(n):
        for t in range(k):
            j = ids[i, t]
            A[i, j] = A[j, i] = min(A[i, j], ln[i, t])
    r, c = np.nonzero(np.isfinite(A))
    assert len(r) == m.stats().entries
    bf, sweeps = jacobi_bellman_ford(n, r, c, A[r, c])
    print(f"{len(r)} entries, {sweeps} Jacobi sweeps")
    assert np.array_equal(bits(bf), bits(D))
    sp = pytest.importorskip("scipy.sparse")
    from scipy.sparse.csgraph import dijkstra
    S = dijkstra(sp.csr_matrix((A[r, c], (r, c)), shape=(n, n)), directed=True)
    assert np.array_equal(bits(S), bits(D))


# ---- the input rules -------------------------------------------------------------------
def test_terminator_ends_a_row(geo):
    D = dist(geo, 3, 3, {0: [(1, 1.0), (-1, 0.0), (2, 1.0)]})
    assert D[0].tolist() == [0.0, 1.0, INF]


def test_dropped_entries(geo):
    D = dist(geo, 6, 5, {0: [(0, 0.25), (1, np.nan), (2, -1.0), (3, INF), (4, 2.0)]})
    assert D[0].tolist() == [0.0, INF, INF, INF, 2.0, INF]
    assert D[0, 0] == 0.0 and not np.signbit(D[0, 0])


def test_negative_zero_counts_as_zero(geo):
    D = dist(geo, 2, 1, {0: [(1, -0.0)]})
    assert bits(D).tolist() == [[0, 0], [0, 0]]  # +0.0 both ways, never -0.0


def test_repeated_id_keeps_the_smallest(geo):
    D = dist(geo, 2, 3, {0: [(1, 3.0), (1, 2.0), (1, 5.0)], 1: [(0, 2.5)]})
    assert D[0, 1] == 2.0 and D[1, 0] == 2.0


def test_union_and_directed_differ_on_a_one_way_edge(geo):
    e = {0: [(1, 1.0)], 1: [(2, 1.0)]}
    U = dist(geo, 3, 1, e, symmetrize="union")
    Dd = dist(geo, 3, 1, e, symmetrize="directed")
    assert U.tolist() == [[0, 1, 2], [1, 0, 1], [2, 1, 0]]
    assert Dd.tolist() == [[0, 1, 2], [INF, 0, 1], [INF, INF, 0]]


def test_squared_takes_the_root_of_the_values(geo):
    rng = np.random.RandomState(3)
    e = {i: [((i + 1) % 8, rng.rand() * 7), ((i + 3) % 8, rng.rand() * 7)] for i in range(8)}
    ids, val = rows(8, 2, e)
    a = geo.Geodesics(8, device=-1, squared=True)
    a.set_rows(ids, val)
    b = geo.Geodesics(8, device=-1, squared=False)
    b.set_rows(ids, np.sqrt(val))
    assert np.array_equal(bits(a.query()), bits(b.query()))


def test_zero_length_edges(geo):
    # duplicate points: 0, 1 and 2 coincide
    D = dist(geo, 4, 2, {0: [(1, 0.0), (2, 0.0)], 2: [(3, 1.5)]})
    assert bits(D[:3, :3]).tolist() == [[0] * 3] * 3
    assert D[:, 3].tolist() == [1.5, 1.5, 1.5, 0.0]


def test_two_components_and_the_tie(geo):
    # {0, 3} and {1, 2} tie at size 2: the lowest id wins; 4 is alone
    m = geo.Geodesics(5, device=-1)
    m.set_rows(*rows(5, 1, {0: [(3, 1.0)], 1: [(2, 2.0)]}))
    comp, main = m.components()
    assert comp.tolist() == [0, 1, 1, 0, 4] and main == 0
    st = m.stats()
    assert (st.components, st.main_component_size, st.entries) == (3, 2, 4)
    D = m.query()
    assert D[0].tolist() == [0, INF, INF, 1, INF] and D[1].tolist() == [INF, 0, 2, INF, INF]
    assert D[4].tolist() == [INF, INF, INF, INF, 0]
    # the larger component wins whatever its id
    m.set_rows(*rows(5, 1, {0: [(3, 1.0)], 1: [(2, 2.0)], 2: [(4, 1.0)]}))
    assert m.components()[1] == 1


def test_lengths_across_the_range(geo):
    sub, tiny, big = 1e-310, 1e-300, 1e300
    D = dist(geo, 5, 1, {0: [(1, sub)], 1: [(2, tiny)], 2: [(3, 1.0)], 3: [(4, big)]}, sources=[0])
    want = [0.0, sub, sub + tiny, (sub + tiny) + 1.0, ((sub + tiny) + 1.0) + big]
    assert bits(D[0]).tolist() == bits(np.array(want)).tolist()


def test_overflowing_sum_is_unreachable(geo):
    D = dist(geo, 3, 1, {0: [(1, 1.5e308)], 1: [(2, 1.5e308)]})
    assert D[0].tolist() == [0.0, 1.5e308, INF] and D[2].tolist() == [INF, 1.5e308, 0.0]


def test_id_out_of_range(geo):
    m = geo.Geodesics(3, device=-1)
    for bad in (3, -2):
        with pytest.raises(IndexError):
            m.set_rows(*rows(3, 1, {0: [(bad, 1.0)]}))
    with pytest.raises(Exception) as e:  # the failed set_rows left no graph
        m.query()
    assert type(e.value).__name__ == "StateError"


def test_csr_input(geo):
    m = geo.Geodesics(3, device=-1, symmetrize="directed")
    m.set_csr([0, 2, 3, 3], [2, 1, 2], [5.0, 1.0, 1.0])
    assert m.query().tolist() == [[0, 1, 2], [INF, 0, 1], [INF, INF, 0]]
    m.set_csr([0, 1, 1, 1], [1])  # no values: every length 1
    assert m.query([0]).tolist() == [[0, 1, INF]]


# ---- the API ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ring(geo):
    m = geo.Geodesics(7, device=-1)
    m.set_rows(*rows(7, 1, {i: [((i + 1) % 7, 1.0 + i)] for i in range(7)}))
    return m, m.query()


def test_repeated_and_unordered_sources(ring):
    m, D = ring
    src = [5, 0, 5, 3, 0]
    assert np.array_equal(bits(m.query(src)), bits(D[src]))


def test_no_sources_is_a_no_op(gw, ring):
    m, _ = ring
    out = np.full((2, 7), 7.5)
    src = np.zeros(1, np.int32)
    assert gw.lib().gw_geo_query(m.handle, gw._lib.ptr(src), 0, gw._lib.ptr(out), 7, None) == 0
    assert np.all(out == 7.5)


def test_pitch_leaves_the_pad(ring):
    m, D = ring
    out = np.full((7, 10), -3.0)
    got = m.query(out=out, pitch=10)
    assert np.array_equal(bits(got[:, :7]), bits(D)) and np.all(got[:, 7:] == -3.0)
    with pytest.raises(ValueError):
        m.query(out=out, pitch=6)


def test_range_error_writes_nothing(ring):
    m, _ = ring
    for bad in ([0, 7], [-1, 2]):
        out = np.full((2, 7), -3.0)
        with pytest.raises(IndexError):
            m.query(bad, out=out)
        assert np.all(out == -3.0)


def test_state_error_before_set(gw, geo):
    m = geo.Geodesics(4, device=-1)
    for call in (m.query, m.components, m.stats):
        with pytest.raises(gw._lib.StateError):
            call()


def test_create_checks(geo):
    for kw in (dict(n=0), dict(n=3, delta=-1.0), dict(n=3, delta=float("nan")), dict(n=3, symmetrize=7)):
        with pytest.raises(ValueError):
            geo.Geodesics(device=-1, **kw)


def test_convenience(geo):
    ids, val = rows(3, 1, {0: [(1, 1.0)], 1: [(2, 4.0)]})
    assert geo.geodesic_distances((ids, val), device=-1, squared=True).tolist() == [[0, 1, 3], [1, 0, 2], [3, 2, 0]]
    csr = {"offsets": np.array([0, 1, 2, 2]), "nbrs": np.array([1, 2], np.int32), "weights": np.array([1.0, 4.0])}
    assert geo.geodesic_distances(csr, sources=[2], device=-1).tolist() == [[5, 4, 0]]
