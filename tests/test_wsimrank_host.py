"""WGraph handles (GW_SEM_JAVA_WGRAPH) and gw_simrank_weighted_ref on the CPU,
against a restatement of the two Java classes written here.

The replay: structures.WGraph (WGraph.java:35-67) as lists plus dicts, built
from the same text lines with Java's rules (readLine strips "\\n" / "\\r\\n",
split drops trailing empty fields, 2 fields -> weight 0.0, the last put of an
unordered pair wins both ways).

The reference: simrank.weighted.WeightedSimRank (WeightedSimRank.java:40-93)
as S' = C * N S N^T / (T T^T) in np.longdouble, N[v][a] = the summed weights
of v's list entries that point at a (accumulated over the structural nonzeros,
so a 0.0 weight still meets a NaN), T[v] = the sum of v's map values, zero for
vertices without a list entry, diagonal 1 between rounds and 0 at the end.

Tolerance: rtol 1e-12 / atol 1e-15, the figure of the unweighted gather
(tests/test_simrank_edges_gpu.py): a row total passes a lane sum, at most 6
scan steps and the chunk carries, about 30 roundings per pass, plus one
multiply per term here, 7e-15 relative per round and 5e-14 at 7 rounds.  That
holds for positive weights; where signs mix it holds while sum|terms| /
|sum terms| (numerators and totals) stays below 100, which the tests assert."""
import ctypes
import os

import numpy as np
import pytest

from test_simrank_edges_gpu import ATOL, LD, RTOL
from test_simrank_edges_gpu import reference as unweighted_reference

GW_ERR_IO, GW_ERR_PARSE, GW_ERR_STATE, GW_ERR_UNSUPPORTED, GW_ERR_RANGE, GW_ERR_INVALID = -2, -3, -6, -7, -8, -1
SEM_WGRAPH = 2


# ---- the replay of WGraph ----------------------------------------------------------------------------------------
def java_double(s):
    """Double.valueOf on the decimal forms the tests use."""
    s = s.strip()
    if s[-1:] in "dDfF" and s[-3:] != "NaN":
        s = s[:-1]
    return float({"NaN": "nan", "Infinity": "inf", "-Infinity": "-inf", "+Infinity": "inf"}.get(s, s))


def parse_lines(text, sep):
    """The (src, dst, weight) of every line as the WGraph constructor reads them."""
    out = []
    lines = text.split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    for line in lines:
        f = line[:-1].split(sep) if line.endswith("\r") else line.split(sep)
        while f and f[-1] == "":
            f.pop()
        assert len(f) in (2, 3), line
        out.append((int(f[0]), int(f[1]), java_double(f[2]) if len(f) == 3 else 0.0))
    return out


class Replay:
    def __init__(self, edges, V):
        self.V = V
        self.adjs = [[] for _ in range(V)]
        self.edges = [dict() for _ in range(V)]
        self.eCount = 0
        for s, d, w in edges:                 # addEdge (WGraph.java:61-67)
            self.adjs[s].append(d)
            self.adjs[d].append(s)
            self.edges[s][d] = w
            self.edges[d][s] = w
            self.eCount += 1

    def offsets(self):
        return np.concatenate([[0], np.cumsum([len(a) for a in self.adjs])]).astype(np.int64)

    def nbrs(self):
        return np.array([x for a in self.adjs for x in a], np.int32)

    def entry_weights(self):
        return np.array([self.edges[v][x] for v, a in enumerate(self.adjs) for x in a], np.float64)

    def totals64(self):
        """fp64, ascending neighbour id: the order the library documents."""
        t = np.zeros(self.V)
        for v, m in enumerate(self.edges):
            s = 0.0
            for a in sorted(m):
                s += m[a]
            t[v] = s
        return t


# ---- the reference ------------------------------------------------------------------------------------------------
def _nsnt(r, c, w, S):
    """N S N^T in long double over N's structural nonzeros (r ascending)."""
    rows, starts = np.unique(r, return_index=True)

    def left(X):
        out = np.zeros_like(X)
        if len(r):
            out[rows] = np.add.reduceat(w[:, None] * X[c], starts, axis=0)
        return out
    return left(left(S).T).T


def reference_nt(N, P, T, deg, C, iters, want_cond=False):
    """N: n x n summed entry weights, P: structural pattern (bool), T: totals,
    deg: list lengths.  With want_cond also the largest sum|terms| / |sum terms|
    over the numerators of every round and over the totals."""
    n = len(N)
    N = np.asarray(N, LD)
    T = np.asarray(T, LD)
    r, c = np.nonzero(P)
    w = N[r, c]
    live = np.outer(deg > 0, deg > 0) & ~np.eye(n, dtype=bool)
    S = np.eye(n, dtype=LD)
    cond = 1.0
    with np.errstate(all="ignore"):
        TT = np.outer(T, T)
        for _ in range(iters):
            num = _nsnt(r, c, w, S)
            if want_cond:
                nabs = _nsnt(r, c, np.abs(w), np.abs(S))
                nz = live & np.isfinite(num) & (num != 0)
                if nz.any():
                    cond = max(cond, float((nabs[nz] / np.abs(num[nz])).max()))
            S = LD(C) * num / TT
            S[~live] = 0
            np.fill_diagonal(S, 1)
    np.fill_diagonal(S, 0)
    return (S, cond) if want_cond else S


def replay_matrices(rp):
    n = rp.V
    N = np.zeros((n, n), LD)
    P = np.zeros((n, n), bool)
    for v, a in enumerate(rp.adjs):
        for x in a:
            N[v, x] += LD(rp.edges[v][x])
            P[v, x] = True
    T = np.array([sum((LD(m[a]) for a in sorted(m)), LD(0)) for m in rp.edges], LD)
    deg = np.array([len(a) for a in rp.adjs])
    return N, P, T, deg


def totals_cond(rp):
    worst = 1.0
    for m in rp.edges:
        v = np.array(list(m.values()), LD)
        if len(v) and np.all(np.isfinite(v)) and v.sum() != 0:
            worst = max(worst, float(np.abs(v).sum() / abs(v.sum())))
    return worst


def reference(rp, C, iters, want_cond=False):
    N, P, T, deg = replay_matrices(rp)
    out = reference_nt(N, P, T, deg, C, iters, want_cond)
    if want_cond:
        return out[0], max(out[1], totals_cond(rp))
    return out


def next_round(rp, C, S, v, w):
    """WeightedSimRank.sim(v, w) for v != w of nonzero degree, in long double."""
    N, _, T, _ = replay_matrices(rp)
    return LD(C) * (N[v] @ np.asarray(S, LD) @ N[w]) / (T[v] * T[w])


def assert_matches(sim, ref):
    """NaN where the reference has NaN, the rest within tolerance (Inf equal)."""
    assert np.array_equal(np.isnan(sim), np.isnan(np.asarray(ref, np.float64)))
    ok = ~np.isnan(sim)
    np.testing.assert_allclose(sim[ok].astype(LD), ref[ok], rtol=RTOL, atol=ATOL)


# ---- graphs -------------------------------------------------------------------------------------------------------
# every loader rule of the issue; V = 10 (id 9 has no line)
LOADER_LINES = [
    "1,2,",            # trailing empty dropped: 2 fields, weight 0.0; the pair is set again below
    "1,2,3",
    "2,1,5",           # the pair reversed: both directions end at 5
    "0,1,1e-3",
    "0,1,2.5",         # a duplicate line with another weight
    "3,3,-2.5",        # a self-loop: listed twice, totalled once
    "0,4",             # 2 fields: weight 0.0
    "4,5",             # first seen with 2 fields ...
    "5,4, 4 ",         # ... later with 3, whitespace round the weight
    "5,6,7d",
    "6,7,NaN",
    "7,8,Infinity",
    "8,0,2.5e-1F",
]
LOADER_V = 10


def loader_text(sep, crlf):
    lines = [l.replace(",", sep) for l in LOADER_LINES]
    # "\r\n" on every other line when crlf is "mixed", no newline after the last line
    ends = ["\r\n" if (crlf == "all" or (crlf == "mixed" and i % 2 == 0)) else "\n" for i in range(len(lines))]
    ends[-1] = ""
    return "".join(l + e for l, e in zip(lines, ends))


# 8 ids; a duplicate pair with changing weights, a self-loop, one negative weight
HAND_EDGES = [(0, 1, 2.0), (1, 2, 0.5), (1, 0, 3.0), (2, 3, 1.25), (3, 4, 4.0), (4, 0, 0.75), (2, 2, 1.5),
              (0, 3, -0.5), (1, 4, 2.5), (3, 4, 1.0), (0, 2, 1.0)]
HAND_LIVE = 5


def hand_edges(ids):
    """HAND_EDGES over the given 5 ids of 8: the other three are isolated."""
    return [(ids[u], ids[v], w) for u, v, w in HAND_EDGES]


def g333_weight(u, v):
    return 1 + ((min(u, v) * 31 + max(u, v) * 17) % 7) / 4


def data_edges(name, weight=g333_weight, dedup=False):
    from conftest import DATA
    f, V, sep = {"moreno": ("moreno_crime_crime.txt", 1380, "\t"), "g333": ("0_333_5038.txt", 333, " ")}[name]
    pairs = [tuple(int(x) for x in l.split(sep)[:2]) for l in open(os.path.join(DATA, f)).read().split("\n") if l]
    if dedup:
        seen, out = set(), []
        for u, v in pairs:
            if (min(u, v), max(u, v)) not in seen:
                seen.add((min(u, v), max(u, v)))
                out.append((u, v))
        pairs = out
    return [(u, v, float(weight(u, v))) for u, v in pairs], V


def write_wgraph_file(path, edges, sep=","):
    path.write_text("".join(f"{u}{sep}{v}{sep}{w!r}\n" for u, v, w in edges))
    return str(path)


# ---- handles ------------------------------------------------------------------------------------------------------
def load(gw, path, sep, V, sem=SEM_WGRAPH, directed=0, weighted=1):
    h = ctypes.c_void_p()
    rc = gw.lib().gw_graph_load_edgelist(str(path).encode(), sep.encode(), sem, directed, weighted, V, ctypes.byref(h))
    return rc, h


def from_edges(gw, edges, V, with_weights=True, sem="wgraph"):
    from gwamd.graph import GWGraph
    src = np.array([e[0] for e in edges], np.int64)
    dst = np.array([e[1] for e in edges], np.int64)
    w = np.array([e[2] for e in edges], np.float64) if with_weights else None
    return GWGraph.from_edges(src, dst, w, semantics=sem, vcount=V)


def ref_host(gw, g, C, iters, nthreads=4):
    n = g.n
    sim = np.full((n, n), -7.0)
    gw._lib.check(gw.lib().gw_simrank_weighted_ref(g.handle, C, iters, nthreads, gw._lib.ptr(sim)), g.handle)
    return sim


def check_handle(gw, g, rp):
    inf = g.info()
    assert (inf.semantics, inf.weighted, inf.directed, inf.n) == (SEM_WGRAPH, 1, 0, rp.V)
    csr = g.export_csr()
    assert np.array_equal(csr["offsets"], rp.offsets())
    assert np.array_equal(csr["nbrs"], rp.nbrs())
    assert np.array_equal(csr["weights"], rp.entry_weights(), equal_nan=True)
    assert np.array_equal(g.export_weight_totals(), rp.totals64(), equal_nan=True)
    assert inf.nnz // 2 == rp.eCount


# ---- loader -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sep,crlf", [(",", "none"), (",", "all"), (",", "mixed"), ("\t", "mixed")])
def test_loader_replays_wgraph(gw, tmp_path, sep, crlf):
    from gwamd.graph import GWGraph
    text = loader_text(sep, crlf)
    p = tmp_path / "w.txt"
    p.write_bytes(text.encode())
    edges = parse_lines(text, sep)
    assert [e[2] for e in edges[:3]] == [0.0, 3.0, 5.0] and edges[8][2] == 4.0 and edges[9][2] == 7.0
    rp = Replay(edges, LOADER_V)
    assert rp.edges[1][2] == rp.edges[2][1] == 5.0 and rp.edges[0][1] == 2.5          # last put wins, both ways
    assert rp.adjs[3] == [3, 3] and rp.totals64()[3] == -2.5                          # listed twice, totalled once
    assert rp.edges[0][4] == 0.0 and rp.edges[4][5] == 4.0 and rp.adjs[1].count(2) == 3
    assert np.isnan(rp.totals64()[6]) and rp.totals64()[8] == np.inf and rp.edges[8][0] == 0.25
    g = GWGraph.from_edgelist(p, delimiter=sep, semantics="wgraph", weighted=True, vcount=LOADER_V)
    check_handle(gw, g, rp)
    check_handle(gw, from_edges(gw, edges, LOADER_V), rp)


def test_default_separator_is_comma(gw, tmp_path):
    p = tmp_path / "w.txt"
    p.write_text("0,1,2\n")
    rc, h = load(gw, p, "", 2)
    assert rc == 0
    w = np.zeros(2)
    assert gw.lib().gw_graph_export_csr(h, None, None, gw._lib.ptr(w), None, None) == 0 and list(w) == [2.0, 2.0]
    gw.lib().gw_graph_free(h)


def test_from_edges_without_weights_is_all_zero(gw):
    edges = parse_lines(loader_text(",", "none"), ",")
    rp = Replay([(u, v, 0.0) for u, v, _ in edges], LOADER_V)
    g = from_edges(gw, edges, LOADER_V, with_weights=False)
    check_handle(gw, g, rp)
    assert np.all(g.export_csr()["weights"] == 0.0) and np.all(g.export_weight_totals() == 0.0)


def test_python_wgraph_mirror(gw, tmp_path):
    from gwamd import topsim
    text = loader_text(",", "none")
    p = tmp_path / "w.txt"
    p.write_text(text)
    rp = Replay(parse_lines(text, ","), LOADER_V)
    wg = topsim.WGraph(str(p), LOADER_V)
    assert wg.getVCount() == LOADER_V and wg.getECount() == rp.eCount == len(LOADER_LINES)
    for v in range(LOADER_V):
        assert wg.degree(v) == len(rp.adjs[v]) and wg.neighbors(v) == rp.adjs[v]
        a, b = wg.getAllEdgeWeight(v), rp.edges[v]
        assert a.keys() == b.keys() and wg.edges(v).keys() == b.keys()
        assert all(a[k] == b[k] or (np.isnan(a[k]) and np.isnan(b[k])) for k in b)


@pytest.mark.parametrize("text,directed,code", [
    ("0,1,2\n3\n", 0, GW_ERR_IO),              # 1 field
    ("0,1,2\n0,1,2,3\n", 0, GW_ERR_IO),        # 4 fields
    ("0,1,x\n", 0, GW_ERR_PARSE),              # not a number
    ("0,1,0x1p3\n", 0, GW_ERR_PARSE),          # hexadecimal floats are refused (graphwalk.h)
    ("0,1,inf\n", 0, GW_ERR_PARSE),            # Double.valueOf knows "Infinity" only
    ("0,4,1\n", 0, GW_ERR_RANGE),              # an id equal to V
    ("0,1,2\n", 1, GW_ERR_UNSUPPORTED),        # directed
])
def test_loader_errors(gw, tmp_path, text, directed, code):
    p = tmp_path / "bad.txt"
    p.write_text(text)
    rc, h = load(gw, p, ",", 4, directed=directed)
    assert rc == code and not h.value
    if code == GW_ERR_IO:
        assert b"invalid edge file" in gw.lib().gw_last_error(None)


def test_java_multi_still_ignores_a_third_column(gw, tmp_path):
    """No existing behaviour changes: semantics 1 with a third column loads the
    unweighted multigraph, and has no totals."""
    p = tmp_path / "w.txt"
    p.write_text(loader_text(",", "none"))
    rc, h = load(gw, p, ",", LOADER_V, sem=1, weighted=0)
    assert rc == 0
    inf = gw._lib.GraphInfo()
    assert gw.lib().gw_graph_info(h, ctypes.byref(inf)) == 0 and (inf.semantics, inf.weighted) == (1, 0)
    t = np.zeros(LOADER_V)
    assert gw.lib().gw_graph_export_weight_totals(h, gw._lib.ptr(t)) == GW_ERR_STATE
    sim = np.zeros((LOADER_V, LOADER_V))
    assert gw.lib().gw_simrank_weighted_ref(h, 0.6, 1, 1, gw._lib.ptr(sim)) == GW_ERR_UNSUPPORTED
    assert b"gw_simrank_naive" in gw.lib().gw_last_error(h)
    gw.lib().gw_graph_free(h)
    rc, h = load(gw, p, ",", LOADER_V, sem=1, weighted=1)
    assert rc == GW_ERR_UNSUPPORTED


def test_weight_totals_of_a_weighted_nx_handle(gw):
    from conftest import DATA
    from gwamd.graph import GWGraph
    g = GWGraph.from_edgelist(os.path.join(DATA, "weighted_quirks.edgelist"), semantics="nx", weighted=True)
    csr = g.export_csr()
    exp = [csr["weights"][b:e].sum() for b, e in zip(csr["offsets"][:-1], csr["offsets"][1:])]
    np.testing.assert_allclose(g.export_weight_totals(), exp, rtol=1e-15)


# ---- gw_simrank_weighted_ref --------------------------------------------------------------------------------------
@pytest.mark.parametrize("ids", [(0, 1, 2, 3, 4), (1, 2, 4, 5, 6)])
@pytest.mark.parametrize("iters", [0, 1, 2, 5])
def test_ref_hand_graph(gw, ids, iters):
    edges = hand_edges(ids)
    rp = Replay(edges, 8)
    ref, cond = reference(rp, 0.6, iters, want_cond=True)
    assert cond < 100, cond
    sim = ref_host(gw, from_edges(gw, edges, 8), 0.6, iters)
    assert_matches(sim, ref)
    assert np.array_equal(sim, sim.T) and np.all(np.diag(sim) == 0)
    iso = [v for v in range(8) if v not in ids]
    assert np.all(sim[iso] == 0) and np.all(sim[:, iso] == 0)
    if iters == 0:
        assert np.all(sim == 0)
    else:
        assert np.count_nonzero(sim) >= 12


def test_ref_refusals(gw):
    g = from_edges(gw, hand_edges(range(5)), 8)
    sim = np.zeros((8, 8))
    assert gw.lib().gw_simrank_weighted_ref(g.handle, 0.6, -1, 1, gw._lib.ptr(sim)) == GW_ERR_INVALID


@pytest.mark.parametrize("C,iters", [(0.6, 3), (0.8, 7)])
def test_ref_g333(gw, C, iters):
    edges, V = data_edges("g333")
    ref = reference(Replay(edges, V), C, iters)
    assert_matches(ref_host(gw, from_edges(gw, edges, V), C, iters, nthreads=8), ref)


def test_ref_unit_weights_equal_unweighted(gw):
    """All weights 1.0 and no duplicate lines: T is the degree and the
    recurrence is SimRank.java's."""
    edges, V = data_edges("g333", weight=lambda u, v: 1.0, dedup=True)
    g = from_edges(gw, edges, V)
    csr = g.export_csr()
    assert np.array_equal(g.export_weight_totals(), np.diff(csr["offsets"]).astype(np.float64))
    ref = unweighted_reference(csr["offsets"], csr["nbrs"], 0.6, 3)
    assert_matches(ref_host(gw, g, 0.6, 3), ref)


# a component of 2-field lines only (ids 5, 6, 7: totals 0) beside a weighted one (ids 0..4)
ZERO_EDGES = [(0, 1, 2.0), (1, 2, 0.5), (2, 3, 1.25), (3, 4, 4.0), (4, 0, 0.75), (1, 3, 1.5), (5, 6, 0.0), (6, 7, 0.0),
              (7, 5, 0.0)]


@pytest.mark.parametrize("iters", [1, 2, 4])
def test_ref_zero_total_component(gw, iters):
    rp = Replay(ZERO_EDGES, 9)
    ref = reference(rp, 0.6, iters)
    nan = np.isnan(np.asarray(ref, np.float64))
    assert nan[5, 6] and nan[5, 0] and not nan[0, 1] and not nan[8].any() and ref[0, 2] > 0
    assert_matches(ref_host(gw, from_edges(gw, ZERO_EDGES, 9), 0.6, iters), ref)
