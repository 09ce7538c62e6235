"""gw_simrank_weighted (gw_wsimrank.hip, k_wsr_gather) on the GPU, against the
long-double restatement of WeightedSimRank.java in tests/test_wsimrank_host.py
(reference, tolerance and its derivation are stated there).

The weighted layout has 8 entries per lane and 512 per wave trip (the
unweighted one 16 and 1024), so the long-row graph of
tests/test_simrank_edges_gpu.py (rows of 15 .. 2049 entries and a hub above
4096) still reaches the lane sum, every scan step, the chunk carry and all 16
wave slices; no graph is larger than moreno's 1,380 vertices."""
import os

import numpy as np
import pytest

from test_simrank_edges_gpu import LD, LONG_CLASSES, LONG_M, long_row_lines
from test_wsimrank_host import (GW_ERR_INVALID, GW_ERR_STATE, GW_ERR_UNSUPPORTED, HAND_LIVE, ZERO_EDGES, Replay,
                                assert_matches, data_edges, hand_edges, next_round, reference,
                                reference_nt)

WSR_K, WSR_CHUNK, SR_WAVES = 8, 512, 16    # gw_wsimrank.hip: entries per lane, per wave trip; waves per workgroup


def lines_text(edges, sep=","):
    """One line per edge; a weight of None writes a 2-field line."""
    return "".join(f"{u}{sep}{v}\n" if w is None else f"{u}{sep}{v}{sep}{w!r}\n" for u, v, w in edges)


def wgraph(path, edges, V, sep=","):
    from gwamd import topsim
    path.write_text(lines_text(edges, sep))
    return topsim.WGraph(str(path), V, separator=sep)


def _gpu(wg, C, iters, hbm_row=0, window=0):
    from gwamd import topsim
    wg._g.options(simrank_hbm_row=hbm_row, simrank_window=window)
    sr = topsim.WeightedSimRank(wg, C_=C, step=iters)
    sr.compute()
    wg._g.options(simrank_hbm_row=0, simrank_window=0)
    return sr.getResult()


def _check(sim, ref, deg):
    assert_matches(sim, ref)
    assert np.array_equal(sim, sim.T, equal_nan=True)
    assert np.all(np.diag(sim) == 0.0)
    iso = np.flatnonzero(np.asarray(deg) == 0)
    assert np.all(sim[iso] == 0.0) and np.all(sim[:, iso] == 0.0)


def padded_entries(deg):
    deg = np.asarray(deg)
    return int(((deg[deg > 0] + WSR_K - 1) // WSR_K * WSR_K).sum())


# ---- the hand graph: compaction with m < n at the end, the middle and the start -------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("ids", [(0, 1, 2, 3, 4), (1, 2, 4, 5, 6)])
def test_hand_graph(gw, tmp_path, ids):
    """8 ids of which 5..7, then 0, 3 and 7, are isolated; duplicates with
    changing weights, a self-loop, one negative weight."""
    edges = hand_edges(ids)
    rp = Replay(edges, 8)
    wg = wgraph(tmp_path / "h.txt", edges, 8)
    deg = [len(a) for a in rp.adjs]
    assert sum(d > 0 for d in deg) == HAND_LIVE and sorted(set(range(8)) - set(ids)) == [v for v in range(8) if not deg[v]]
    for iters in (0, 1, 2, 5):
        ref, cond = reference(rp, 0.6, iters, want_cond=True)
        assert cond < 100, cond
        sim = _gpu(wg, 0.6, iters)
        _check(sim, ref, deg)
        assert np.array_equal(sim, _gpu(wg, 0.6, iters, hbm_row=1))
        assert np.all(sim == 0) if iters == 0 else np.count_nonzero(sim) >= 12


# ---- long rows ------------------------------------------------------------------------------------------------------
def long_weight(u, v):
    return 0.25 + ((min(u, v) * 13 + max(u, v) * 7) % 11) / 8


class _Long:
    """The long-row graph with a weight per pair, loaded once per module, its
    references computed once per (C, rounds) and handed out read-only."""

    def __init__(self, path):
        edges = [(u, v, long_weight(u, v)) for u, v in long_row_lines()]
        self.rp = Replay(edges, LONG_M)
        self.wg = wgraph(path, edges, LONG_M)
        self.deg = np.array([len(a) for a in self.rp.adjs])
        have = set(int(d) for d in self.deg)
        assert all(c in have for c in LONG_CLASSES) and self.deg.max() > 4096 and np.all(self.deg > 0)
        assert padded_entries(self.deg) > SR_WAVES * WSR_CHUNK, "no wave would run a second trip of the pos loop"
        self._refs = {}

    def ref(self, C, iters):
        if (C, iters) not in self._refs:
            r = reference(self.rp, C, iters)
            r.setflags(write=False)
            self._refs[(C, iters)] = r
        return self._refs[(C, iters)]


@pytest.fixture(scope="module")
def long_graph(tmp_path_factory):
    return _Long(tmp_path_factory.mktemp("wsr") / "long.txt")


@pytest.mark.gpu
@pytest.mark.parametrize("iters", [1, 3])
def test_long_rows(gw, long_graph, iters):
    """Rows of 15..17, 255..257, 511..513, 1008..1041, 2047..2049 entries and a
    hub above 4096: the 8-term lane sum, every scan step, the chunk carry, all
    16 wave slices.  The HBM-row variant gives the same bits."""
    L = long_graph
    sim = _gpu(L.wg, 0.6, iters)
    _check(sim, L.ref(0.6, iters), L.deg)
    assert np.array_equal(sim, _gpu(L.wg, 0.6, iters, hbm_row=1))


@pytest.mark.gpu
@pytest.mark.parametrize("window", [1, 7, 0])
def test_windows(gw, long_graph, window):
    """simrank_window = 1, 7 and automatic: multi-window passes, windows with
    fewer rows than waves."""
    L = long_graph
    _check(_gpu(L.wg, 0.6, 3, window=window), L.ref(0.6, 3), L.deg)
    _check(_gpu(L.wg, 0.6, 3, hbm_row=1, window=window), L.ref(0.6, 3), L.deg)


@pytest.mark.gpu
def test_small_stream(gw, tmp_path):
    """17 rows of 2 to 8 entries: the padded stream is shorter than 16 wave
    trips, so most wave slices are empty or a row or two."""
    rng = np.random.default_rng(17)
    pairs = [(int(rng.integers(v)), v) for v in range(1, 17)] + [tuple(int(x) for x in rng.integers(17, size=2))
                                                                 for _ in range(24)]
    edges = [(u, v, long_weight(u, v)) for u, v in pairs]
    rp = Replay(edges, 17)
    deg = [len(a) for a in rp.adjs]
    assert all(deg) and padded_entries(deg) < SR_WAVES * WSR_CHUNK
    wg = wgraph(tmp_path / "s.txt", edges, 17)
    for iters in (1, 4):
        sim = _gpu(wg, 0.6, iters)
        _check(sim, reference(rp, 0.6, iters), deg)
        assert np.array_equal(sim, _gpu(wg, 0.6, iters, hbm_row=1))


# ---- data graphs ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def moreno(tmp_path_factory):
    edges, V = data_edges("moreno")
    rp = Replay(edges, V)
    return rp, wgraph(tmp_path_factory.mktemp("wsr") / "moreno.txt", edges, V, sep="\t"), [len(a) for a in rp.adjs]


@pytest.mark.gpu
@pytest.mark.parametrize("C,iters", [(0.6, 3), (0.8, 7)])
def test_moreno(gw, moreno, C, iters):
    rp, wg, deg = moreno
    sim = _gpu(wg, C, iters)
    _check(sim, reference(rp, C, iters), deg)
    assert np.array_equal(sim, _gpu(wg, C, iters, hbm_row=1))       # LDS row and HBM row: the same bits


@pytest.mark.gpu
def test_unit_weights_equal_naive(gw, tmp_path):
    """All weights 1.0, no duplicate lines: T is the degree, so the scores are
    gw_simrank_naive's on the JAVA_MULTI handle of the same lines."""
    from gwamd import topsim
    edges, V = data_edges("g333", weight=lambda u, v: 1.0, dedup=True)
    wg = wgraph(tmp_path / "u.txt", edges, V)
    g = topsim.Graph(str(tmp_path / "u.txt"), V, separator=",")      # ignores the third column
    assert np.array_equal(g._offs, wg._offs) and np.array_equal(g._nbrs, wg._nbrs)
    sr = topsim.SimRank(g, C_=0.6, step=3)
    sr.compute()
    assert_matches(_gpu(wg, 0.6, 3), sr.getResult().astype(LD))


@pytest.mark.gpu
@pytest.mark.parametrize("iters", [1, 2, 4])
def test_zero_total_component(gw, tmp_path, iters):
    """A component of 2-field lines (totals 0) beside a weighted one: NaN where
    the reference has NaN, the finite remainder within tolerance."""
    edges = [(u, v, None if w == 0.0 else w) for u, v, w in ZERO_EDGES]
    rp = Replay(ZERO_EDGES, 9)
    wg = wgraph(tmp_path / "z.txt", edges, 9)
    assert np.all(wg._totals[5:8] == 0.0) and wg._totals[8] == 0.0 and wg.degree(8) == 0
    ref = reference(rp, 0.6, iters)
    assert np.isnan(np.asarray(ref, np.float64)).sum() == 2 * (3 * 5) + 6
    for hbm_row in (0, 1):
        sim = _gpu(wg, 0.6, iters, hbm_row=hbm_row)
        assert_matches(sim, ref)
        assert np.all(sim[8] == 0) and np.all(sim[:, 8] == 0) and np.all(np.diag(sim) == 0)


def _host_call(gw, g, C, iters):
    n = g.n
    sim = np.full((n, n), -7.0)
    rc = gw.lib().gw_simrank_weighted_host(g.handle, C, iters, gw._lib.ptr(sim))
    return rc, sim


@pytest.mark.gpu
def test_weighted_nx_simple_handle(gw):
    """A 3-column file loaded as a weighted undirected NX_SIMPLE graph: entry
    weights and row sums as networkx merges them (main.py:76-89)."""
    import networkx as nx
    from conftest import DATA
    from gwamd.graph import GWGraph
    path = os.path.join(DATA, "weighted_quirks.edgelist")
    G = nx.read_edgelist(path, nodetype=int, data=(("weight", float),), create_using=nx.DiGraph()).to_undirected()
    labels = sorted(G.nodes())
    rank = {x: i for i, x in enumerate(labels)}
    n = len(labels)
    N = np.zeros((n, n), LD)
    for u, v, d in G.edges(data=True):
        N[rank[u], rank[v]] = N[rank[v], rank[u]] = LD(d["weight"])
    P = N != 0
    assert P.sum() == sum(2 - (u == v) for u, v in G.edges()) and np.any(np.diag(P))
    g = GWGraph.from_edgelist(path, semantics="nx", weighted=True).to_device(0)
    assert np.array_equal(g.export_csr()["labels"], labels)
    np.testing.assert_allclose(g.export_weight_totals(), N.sum(1).astype(np.float64), rtol=1e-15)
    for iters in (1, 5):
        rc, sim = _host_call(gw, g, 0.6, iters)
        assert rc == 0
        _check(sim, reference_nt(N, P, N.sum(1), P.sum(1), 0.6, iters), P.sum(1))


# ---- a WGRAPH handle in the other families --------------------------------------------------------------------------
@pytest.mark.gpu
def test_other_families_see_the_multigraph(gw, tmp_path):
    """gw_simrank_naive and gw_topsim on a WGRAPH handle against the JAVA_MULTI
    handle of the same lines (the weights are out of their way).  Naive
    SimRank: bit for bit.  TopSim (SAMPLE 1000, STEP 3, 64 sources, one seed):
    the same top-k ids and the same walk counters exactly; the scores within
    rtol 1e-12, not bit for bit, because gw_topsim sums a row's pair updates
    with fp64 atomics whose order differs from launch to launch.  Measured on
    these shapes: one JAVA_MULTI handle run twice differs from itself in 301 of
    1280 scores by up to 6.3e-16 relative, two JAVA_MULTI handles in 242 by up
    to 5.2e-16, the WGRAPH handle against a JAVA_MULTI handle in 257 by up to
    5.4e-16, ids equal every time.  1e-12 is the bound the TopSim tests hold
    the kernel to against the oracle."""
    from gwamd import topsim
    edges, V = data_edges("g333")
    wg = wgraph(tmp_path / "w.txt", edges, V)
    g = topsim.Graph(str(tmp_path / "w.txt"), V, separator=",")
    assert wg._g.info().weighted == 1 and g._g.info().weighted == 0
    a, b = topsim.SimRank(wg, step=3), topsim.SimRank(g, step=3)
    a.compute()
    b.compute()
    assert np.array_equal(a.getResult(), b.getResult()) and np.count_nonzero(a.getResult()) > V
    src = np.arange(64, dtype=np.int32)
    ta, tb = topsim.TopSim_singleSample(wg, 1000, 3, seed=5), topsim.TopSim_singleSample(g, 1000, 3, seed=5)
    (ia, sa), (ib, sb) = ta.topK(20, sources=src), tb.topK(20, sources=src)
    d = np.abs(sa - sb)
    print(f"topsim scores: {int((d != 0).sum())} of {d.size} differ, max relative {float((d[sb != 0] / sb[sb != 0]).max()):.3e}")
    assert np.array_equal(ia, ib) and ta.stats == tb.stats and ta.stats["walkers"] > 0 and np.any(sb > 0)
    np.testing.assert_allclose(sa, sb, rtol=1e-12, atol=0)


# ---- refusals -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals(gw, tmp_path):
    from conftest import DATA
    from gwamd import topsim
    from gwamd.graph import GWGraph
    edges = hand_edges(range(5))
    wg = wgraph(tmp_path / "h.txt", edges, 8)
    rc, _ = _host_call(gw, wg._g, 0.6, 1)
    assert rc == GW_ERR_STATE                                        # not on a device
    sim = np.zeros((8, 8))
    assert gw.lib().gw_simrank_weighted(wg._g.handle, 0.6, 1, gw._lib.ptr(sim), None) == GW_ERR_STATE
    wg._ensure_device()
    assert _host_call(gw, wg._g, 0.6, -1)[0] == GW_ERR_INVALID
    with pytest.raises(ValueError):
        topsim.WeightedSimRank(wg, step=-1).compute()
    g = topsim.Graph(str(tmp_path / "h.txt"), 8, separator=",")     # unweighted handle
    g._ensure_device()
    assert _host_call(gw, g._g, 0.6, 1)[0] == GW_ERR_UNSUPPORTED
    assert b"gw_simrank_naive" in gw.lib().gw_last_error(g._g.handle)
    d = GWGraph.from_edgelist(os.path.join(DATA, "weighted_quirks.edgelist"), semantics="nx", weighted=True,
                              directed=True).to_device(0)
    assert _host_call(gw, d, 0.6, 1)[0] == GW_ERR_UNSUPPORTED
    assert _host_call(gw, wg._g, 0.6, 1)[0] == 0                     # the handle still works afterwards


@pytest.mark.gpu
def test_kernel_attrs_no_scratch(gw, tmp_path):
    """All four weighted instantiations run without scratch at 1024 threads
    (128 VGPRs per lane)."""
    from gwamd import topsim
    attrs = topsim.WeightedSimRank(wgraph(tmp_path / "h.txt", hand_edges(range(5)), 8)).kernel_attrs()
    assert len(attrs) == 4
    for name, a in attrs.items():
        assert a["scratch_bytes"] == 0 and 0 < a["vgprs"] <= 128, (name, a)


# ---- mirrors --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_cpp_and_python_write_the_same_bytes(gw, tmp_path):
    """simrank_variants --algo wsimrank and printByOrder(WeightedSimRank) on the
    weighted 0_333_5038 graph: the same .sim.txt and id files."""
    import subprocess
    from conftest import ROOT
    from gwamd import topsim
    edges, V = data_edges("g333")
    wg = wgraph(tmp_path / "w.txt", edges, V)
    out = str(tmp_path / "cpp")
    subprocess.run([os.path.join(ROOT, "graph-embedding_amd", "bin", "simrank_variants"), "--graph",
                    str(tmp_path / "w.txt"), "--V", str(V), "--sep", ",", "--algo", "wsimrank", "--step", "5",
                    "--out", out], check=True, timeout=300)
    sr = topsim.WeightedSimRank(wg, step=5)
    sr.compute()
    topsim.printByOrder(sr, str(tmp_path / "py"), 20)
    for suffix in ("", ".sim.txt"):
        a = open(out + suffix, "rb").read()
        assert a == open(str(tmp_path / "py") + suffix, "rb").read() and a.count(b"\r\n") == V
    assert b":0." in open(out + ".sim.txt", "rb").read()


@pytest.mark.gpu
def test_sim_is_one_more_round(gw, tmp_path):
    from gwamd import topsim
    edges = hand_edges((1, 2, 4, 5, 6))
    rp = Replay(edges, 8)
    wg = wgraph(tmp_path / "h.txt", edges, 8)
    sr = topsim.WeightedSimRank(wg, step=3)
    assert sr.sim(1, 1) == 1.0 and sr.sim(0, 1) == 0.0
    np.testing.assert_allclose(sr.sim(1, 2), float(next_round(rp, 0.6, np.eye(8), 1, 2)), rtol=1e-12)
    sr.compute()                 # sim() now reads the matrix as postProcess left it (zero diagonal), as in Java
    for v, w in ((1, 2), (6, 4)):
        exp = float(next_round(rp, 0.6, sr.getResult(), v, w))
        np.testing.assert_allclose(sr.sim(v, w), exp, rtol=1e-12)
        assert exp != 0
