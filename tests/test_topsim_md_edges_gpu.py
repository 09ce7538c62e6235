"""TopSim_M (gw_topsim_m.hip) and the double-walk variants (gw_topsim_d.hip) at
their edges: every k_topsim_m<1..8> and k_topsim_levels<1..8>, FixedCacheMap
capacities 1..3 (4- and 8-slot key index, eviction on ties) and 4095/4096,
k_levels_syrk on both sides of its 64-tile and 16-deep k edges with a NaN
pre-filled output, several source batches of gw_topsim_dev, and the
DoubleRandomWalk first-meeting filter, dead-end key and bucket/block edges.

Graphs are the disjoint unions of test_topsim_dispatch_gpu (vertex 0 isolated
and kept as a source / row everywhere), so every reference is evaluated per
component and cross-component entries must be exact zeros.  The references are
written here and share nothing with oracle.c:

  R1  level rows: the literal Java-queue port _py_double_sample_levels
      (test_oracle_golden.py), deterministic regime (SAMPLE = 3^STEP: every
      queued mass >= its degree, the port asserts it);
  R2  getSim: sim[i][j] = sum_s C^s sum_x P_i[x][s] P_j[x][s] in np.longdouble
      from R1's rows, mirrored, zero diagonal;
  R3  TopSim_singleSample_M.java:62-239 in the deterministic regime
      (SAMPLE = maxdeg^(2 STEP)): the LinkedList queue over 2 STEP levels, every
      qualifying path at length 2i put as float32 into oracle.PyFixedCacheMap
      (the port pinned to FixedCacheMap.main), then drained.  Keys, float bits,
      sizes, drain order and the counters must be identical to the kernel's;
  R4  DoubleRandomWalk closed forms at C = 0.5 (star K_{1,3}, path-3, doubled
      edge): sim[leaf][leaf'] = 0.5 bitwise for every STEP and SAMPLE, 0 else;
  R5  the oracle in the random regime, at the two existing files' bars
      (bit-exact for _M, test_topsim_double_gpu._close for the double variants).

Tolerance facts.  _close is rtol 1e-12, atol 1e-12 x max|ref|, identical
support.  Against R2 it is derivable: every term is positive and at most
STEP x 11 <= 88 are nonzero per entry, so reassociation costs below
88 x 2^-53 ~ 1e-14 relative.  test_r2_equals_oracle_double_sample measures the
oracle against R2 on the tile-edge unions (max |oracle - R2| / max|R2|, V 65,
129, 193, STEP 1, 3, 5, 8): 0 at STEP 1, 1.2e-16 at STEP 3, 1.9e-16 at STEP 5
and 1.3e-16 at STEP 8, the same at every V -- well under 1e-12.

Case 6 note: at SAMPLE 50 no level can exceed 256 entries (the mass of a level
sums to SAMPLE and a walker carries >= 1/2), so the multi-trip scan of
k_topsim_levels is reached by the added SAMPLE 700 (the 600-wheel's hub then
enumerates 599 children of mass < 3: 1198 walkers) and by STEP 8 on K4 in
case 5 (6561 entries).

Capacity 4095/4096: a wheel's hub reaches only its k - 1 rim vertices, so more
than 4096 distinct targets need k >= 4098; at k = 4098 and STEP 2 the smallest
SAMPLE for which oracle.topsim reports all 4097 (seed 11) is WHEEL_SAMPLE.
"""
import math

import numpy as np
import pytest

from test_oracle_golden import _py_double_sample_levels
from test_topsim_dispatch_gpu import _Union, _component_union, _edges
from test_topsim_double_gpu import _close

C_DECAY = 0.6
SEED_M, SEED_D, SEED_DEV, SEED_DRW = 11, 4, 8, 2
CAPACITIES = (1, 2, 3, 5, 64)
DET_M = [(2, s) for s in range(1, 7)] + [(3, s) for s in range(1, 5)]
TILE_V = (1, 2, 63, 64, 65, 127, 128, 129, 193)
TILE_STEPS = (1, 3, 5, 8)
DEG3_FIRST = (("star", 4), ("k4", 4), ("loop", 3))
WHEEL_K, WHEEL_SAMPLE = 4098, 12291


# ---------------------------------------------------------------------------
# graphs
# ---------------------------------------------------------------------------
class _EdgeUnion(_Union):
    """_Union with adjacency lists in the loader's order and without its
    max-degree assertion (the V 1 and V 2 unions have no edge)."""

    def __init__(self, gw, V, max_deg, first=()):
        s, d, self.comps = _component_union(V, max_deg, first)
        self.G = gw.GWGraph.from_edges(s, d, semantics="java", vcount=V)
        c = self.G.export_csr()
        self.offs, self.nbrs, self.V = c["offsets"], c["nbrs"], V
        assert len(self.offs) == V + 1 and int(self.offs[-1]) == 2 * len(s)
        self.deg = [int(x) for x in np.diff(self.offs)]
        assert max(self.deg) <= max([max_deg] + [k - 1 for _, k in first])
        self.adj = [self.nbrs[self.offs[v]:self.offs[v + 1]].tolist() for v in range(V)]
        self._dev = False
        self._ref = {}

    def kind_sources(self, ncomp):
        """Vertex 0, then a middle vertex of each of the first ncomp components
        and, where it differs in degree (paths, stars), the first one."""
        out = [0]
        for c in self.comps[:ncomp]:
            out.append(int(c[len(c) // 2]))
            if self.deg[int(c[0])] != self.deg[out[-1]]:
                out.append(int(c[0]))
        return np.asarray(out, np.int32)


_UNIONS = {}


def _union(gw, V, max_deg, first=()):
    key = (V, max_deg, tuple(first))
    if key not in _UNIONS:
        _UNIONS[key] = _EdgeUnion(gw, V, max_deg, first)
    return _UNIONS[key]


def _tile_union(gw, V):
    return _union(gw, V, 3, DEG3_FIRST if V >= 12 else ())


# ---------------------------------------------------------------------------
# R1 + R2: level rows and getSim
# ---------------------------------------------------------------------------
def _r2(g, step, sample):
    """(sim float64 [V, V], same-component mask); computed once and shared."""
    key = ("r2", step, sample)
    if key not in g._ref:
        cache = [np.longdouble(C_DECAY ** s) for s in range(step + 1)]  # Math.pow, a double
        sim = np.zeros((g.V, g.V))
        mask = np.zeros((g.V, g.V), bool)
        for comp in g.comps:
            k, b = len(comp), int(comp[0])
            P = np.zeros((step + 1, k, k), np.longdouble)
            for i, v in enumerate(comp):
                rows = _py_double_sample_levels(g.adj, int(v), sample, step) if g.adj[int(v)] else {}
                for (x, s), m in rows.items():
                    assert b <= x < b + k
                    P[s, i, x - b] = m
            S = sum(cache[s] * (P[s] @ P[s].T) for s in range(1, step + 1))
            np.fill_diagonal(S, 0)
            sim[np.ix_(comp, comp)] = S.astype(np.float64)
            mask[np.ix_(comp, comp)] = True
        sim.setflags(write=False)
        mask.setflags(write=False)
        g._ref[key] = (sim, mask)
    return g._ref[key]


# ---------------------------------------------------------------------------
# R3: TopSim_singleSample_M, deterministic regime
# ---------------------------------------------------------------------------
def _py_topsim_m_walk(adj, src, SAMPLE, STEP):
    """Literal Python port of TopSim_singleSample_M.walk / computePathSim /
    isFirstMeet (TopSim_singleSample_M.java:62-258) for the deterministic
    regime: the put() sequence [(target, float32)], the number of queue.add
    calls and the largest queue a round started with."""
    from collections import deque
    maxStep = 2 * STEP
    cache = [0.0] + [C_DECAY ** i for i in range(1, STEP + 1)]
    queue = deque([[(src, float(SAMPLE))]])
    puts, stats = [], dict(ext=0, frontier=0)

    def isFirstMeet(path, srcIndex, dstIndex):
        internal = (dstIndex - srcIndex) // 2 + srcIndex
        for i in range(srcIndex, internal):
            if path[i][0] == path[dstIndex - i + srcIndex][0]:
                return False
        return True

    def computePathSim(pathLen, start):
        for path in queue:
            source = path[0][0]
            i = start
            while i <= STEP and 2 * i <= pathLen:
                interNode, target = path[i][0], path[2 * i][0]
                if target != source and isFirstMeet(path, 0, 2 * i):
                    incre = path[2 * i][1] * cache[i] * len(adj[interNode]) / len(adj[target]) / SAMPLE
                    puts.append((target, np.float32(incre)))
                i += 1

    pathLen, TopSim = 0, 1
    while pathLen < maxStep:
        if pathLen // 2 == TopSim:
            computePathSim(pathLen, TopSim)
            TopSim += 1
        stats["frontier"] = max(stats["frontier"], len(queue))
        for _ in range(len(queue)):
            path = queue[0]
            cur, sample = path[pathLen]
            degree = len(adj[cur])
            if degree != 0:  # (degree 0: randNeighbor returns -1, no child)
                assert sample >= degree, "deterministic regime only"
                newSample = sample / degree
                for j in range(degree):
                    queue.append(path + [(adj[cur][j], newSample)])
                    stats["ext"] += 1
            queue.popleft()
        pathLen += 1
    computePathSim(pathLen, TopSim)
    return puts, stats["ext"], stats["frontier"]


def _r3(oracle, g, sources, step, capacity):
    """(keys, float32 values, sizes, stats) of R3; walks and drains cached."""
    sample = max(g.deg) ** (2 * step)
    keys = np.full((len(sources), capacity), -1, np.int32)
    vals = np.zeros((len(sources), capacity), np.float32)
    size = np.zeros(len(sources), np.int32)
    st = dict(extensions=0, pair_updates=0, max_frontier=0, walkers=0)
    for r, v in enumerate(sources):
        wk = ("r3walk", int(v), step)
        if wk not in g._ref:
            g._ref[wk] = _py_topsim_m_walk(g.adj, int(v), sample, step)
        puts, ext, frontier = g._ref[wk]
        dk = ("r3drain", int(v), step, capacity)
        if dk not in g._ref:
            m = oracle.PyFixedCacheMap(capacity)
            for k, x in puts:
                m.put(k, x)
            g._ref[dk] = m.drain()
        d = g._ref[dk]
        size[r] = len(d)
        keys[r, :len(d)] = [k for k, _ in d]
        vals[r, :len(d)] = [x for _, x in d]
        st["extensions"] += ext
        st["pair_updates"] += len(puts)
        st["max_frontier"] = max(st["max_frontier"], frontier)
    return keys, vals, size, st


def _det_m(gw, max_deg):
    g = _union(gw, 130, max_deg)
    base = g.kind_sources(17 if max_deg == 2 else 20)
    return g, np.concatenate([base, base[3:4]])  # one source twice: identical rows


def _m_equal(got, ref, variant=0):
    (k, v, sz, st), (rk, rv, rsz, rst) = got, ref
    assert np.array_equal(sz, rsz)
    assert np.array_equal(k, rk)
    assert np.array_equal(v.view(np.uint32), rv.view(np.uint32))
    assert st["pair_updates"] == rst["pair_updates"] and st["extensions"] == rst["extensions"]
    if variant == 0:
        assert st["walkers"] == rst["walkers"] and st["max_frontier"] == rst["max_frontier"]


# ---------------------------------------------------------------------------
# R4: DoubleRandomWalk closed forms
# ---------------------------------------------------------------------------
R4_KINDS = (("star", 4), ("path", 3), ("double", 2))


def _r4(gw, C):
    """The union of R4_KINDS behind vertex 0 and its exact matrix: the leaves
    of a star or a path-3 sit on their only neighbour at step 0, so every walk
    pair of two leaves meets there first (C each, / SAMPLE^2: C); a leaf and
    its neighbour are never co-located (parity), nor the ends of a doubled
    edge."""
    g = _union(gw, 1 + sum(k for _, k in R4_KINDS), 3, R4_KINDS)
    exp = np.zeros((g.V, g.V))
    for (kind, k), comp in zip(R4_KINDS, g.comps):
        ends = [v for e in _edges(kind, k) for v in e]
        leaves = [int(comp[v]) for v in range(k) if ends.count(v) == 1]
        assert len({tuple(g.adj[v]) for v in leaves}) <= 1  # one shared neighbour
        for a in leaves:
            for b in leaves:
                if a != b:
                    exp[a, b] = C
    assert exp.sum() == (6 + 2) * C
    return g, exp


# ---------------------------------------------------------------------------
# CPU: the references against the oracle
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("capacity", CAPACITIES)
@pytest.mark.parametrize("max_deg,step", DET_M)
def test_r3_equals_oracle_topsim_m(gw, oracle, max_deg, step, capacity):
    g, sources = _det_m(gw, max_deg)
    ref = oracle.topsim_m(g.offs, g.nbrs, 0, max_deg ** (2 * step), step, capacity, C=C_DECAY, seed=SEED_M,
                          sources=sources, nthreads=8)
    _m_equal(ref, _r3(oracle, g, sources, step, capacity))
    assert ref[3]["walkers"] == 0


@pytest.mark.parametrize("step", TILE_STEPS)
@pytest.mark.parametrize("V", (65, 129, 193))
def test_r2_equals_oracle_double_sample(gw, oracle, V, step):
    g = _tile_union(gw, V)
    ref, mask = _r2(g, step, 3 ** step)
    sim = oracle.topsim_double_sample(g.offs, g.nbrs, 3 ** step, step, C=C_DECAY, seed=SEED_D, nthreads=8)
    print(f"V={V} STEP={step} max|oracle - R2| / max|R2| = {np.abs(sim - ref).max() / np.abs(ref).max():.3g}")
    _close(sim, ref)
    assert not sim[~mask].any()


@pytest.mark.parametrize("step", (1, 2, 5, 8))
@pytest.mark.parametrize("sample", (1, 7, 64, 257))
def test_r4_equals_oracle_double_random_walk(gw, oracle, sample, step):
    g, exp = _r4(gw, 0.5)
    sim = oracle.double_random_walk(g.offs, g.nbrs, sample, step, C=0.5, seed=SEED_DRW, nthreads=8)
    assert np.array_equal(sim, exp)


def test_java_int_square(oracle):
    """DoubleRandomWalk's divisor SAMPLE * SAMPLE as the Java int it is."""
    assert oracle.java_int_square(46340) == 2147395600
    assert oracle.java_int_square(46341) == -2147479015
    assert oracle.java_int_square(65536) == 0


def _dev_sample(sample_total, step, topK, singleStep):
    """TopSim_Dev.java:36."""
    return int(((step - singleStep) * sample_total * 2.0) / (float(step) * (topK + 1.0)))


def _sample_total_for(target, step, topK, singleStep):
    st = math.floor(target * step * (topK + 1.0) / (2.0 * (step - singleStep)))
    while _dev_sample(st, step, topK, singleStep) < target:
        st += 1
    assert _dev_sample(st, step, topK, singleStep) == target
    return st


def _cands(g, topK):
    """int32 [V][topK]: the other vertices of the row's component, then the
    next component's, then -1; vertex 0 all -1."""
    cand = np.full((g.V, topK), -1, np.int32)
    for ci, comp in enumerate(g.comps):
        nxt = g.comps[(ci + 1) % len(g.comps)]
        for v in comp:
            row = [int(u) for u in comp if u != v] + [int(u) for u in nxt]
            assert len(row) < topK and int(v) not in row
            cand[v, :len(row)] = row
    return cand


def _cand_mask(cand):
    mask = np.zeros((cand.shape[0], cand.shape[0]), bool)
    for i in range(cand.shape[0]):
        mask[i, cand[i][cand[i] >= 0]] = True
    return mask


# ---------------------------------------------------------------------------
# GPU call helpers (the C ABI on the handle; outputs pre-filled)
# ---------------------------------------------------------------------------
def _gpu_m(g, variant, capacity, sample, step, sources):
    import torch
    from gwamd import _lib as Cl
    assert Cl.TOPSIM_SINGLE_SAMPLE == 0 and Cl.TOPSIM_SINGLE_RW == 2
    h = g.handle
    src = torch.as_tensor(np.asarray(sources, np.int32), device="cuda")
    keys = torch.full((len(src), capacity), -7, dtype=torch.int32, device="cuda")
    vals = torch.full((len(src), capacity), float("nan"), dtype=torch.float32, device="cuda")
    size = torch.full((len(src),), -7, dtype=torch.int32, device="cuda")
    st = torch.zeros(4, dtype=torch.int64, device="cuda")
    Cl.check(Cl.lib().gw_topsim_m(h, variant, capacity, sample, step, C_DECAY, SEED_M, Cl.ptr(src), len(src),
                                  Cl.ptr(keys), Cl.ptr(vals), Cl.ptr(size), Cl.ptr(st), None), h)
    s = st.cpu().numpy()
    return keys.cpu().numpy(), vals.cpu().numpy(), size.cpu().numpy(), \
        dict(extensions=int(s[0]), pair_updates=int(s[1]), max_frontier=int(s[2]), walkers=int(s[3]))


def _gpu_sim(g, name, *args):
    """gw_topsim_double / gw_topsim_dev / gw_double_random_walk into a NaN-filled sim_dev."""
    import torch
    from gwamd import _lib as Cl
    h = g.handle
    sim = torch.full((g.V, g.V), float("nan"), dtype=torch.float64, device="cuda")
    keep = [torch.as_tensor(a, device="cuda") if isinstance(a, np.ndarray) else a for a in args]
    Cl.check(getattr(Cl.lib(), name)(h, *[Cl.ptr(a) if isinstance(a, torch.Tensor) else a for a in keep],
                                     Cl.ptr(sim), None), h)
    return sim.cpu().numpy()


def _full_symmetric(sim, mask):
    assert not np.isnan(sim).any()  # every entry of sim_dev written
    assert np.array_equal(sim, sim.T) and not np.diag(sim).any()
    assert not sim[~mask].any()  # exact zeros across components


# ---------------------------------------------------------------------------
# k_topsim_m
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("capacity", CAPACITIES)
@pytest.mark.parametrize("max_deg,step", DET_M)
def test_m_deterministic_equals_java_port(gw, oracle, max_deg, step, capacity):
    """Case 1.  On a cycle every update is a dyadic tie, so capacities 1..3
    evict at value == min and wrap the 4- or 8-slot key index."""
    g, sources = _det_m(gw, max_deg)
    got = _gpu_m(g, 0, capacity, max_deg ** (2 * step), step, sources)
    _m_equal(got, _r3(oracle, g, sources, step, capacity))
    assert got[3]["walkers"] == 0 and got[2][0] == 0  # the isolated source: an empty map
    assert np.array_equal(got[0][-1], got[0][3]) and np.array_equal(got[1][-1].view(np.uint32),
                                                                    got[1][3].view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("sample", (1, 255, 256, 257))
@pytest.mark.parametrize("variant,step", [(0, 7), (0, 8)] + [(2, s) for s in (1, 2, 4, 6, 7, 8)])
def test_m_every_template_equals_oracle(gw, oracle, variant, step, sample):
    """Case 2.  SingleRandomWalk_M writes UK[w * STEP + i - 1]: SAMPLE 1 and 257
    are its partial-block edges."""
    g = _union(gw, 430, 3, (("wheel", 300),))
    hub = int(g.comps[0][0])
    assert g.deg[hub] == 299
    sources = np.concatenate([[hub, hub + 1, hub + 150], g.kind_sources(21)]).astype(np.int32)
    capacity = 16
    got = _gpu_m(g, variant, capacity, sample, step, sources)
    ref = oracle.topsim_m(g.offs, g.nbrs, variant, sample, step, capacity, C=C_DECAY, seed=SEED_M, sources=sources,
                          nthreads=8)
    _m_equal(got, ref, variant)
    assert ref[3]["pair_updates"] > 0
    if variant == 0:
        assert ref[3]["walkers"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("capacity", (4095, 4096))
def test_m_capacity_4095_4096(gw, oracle, capacity):
    """Case 3: the hub of a 4098-wheel has 4097 distinct targets at STEP 2, so
    both capacities evict."""
    g = _union(gw, 1 + WHEEL_K + 7, 3, (("wheel", WHEEL_K),))
    hub = int(g.comps[0][0])
    assert g.deg[hub] == WHEEL_K - 1
    for smp, full in ((WHEEL_SAMPLE, True), (WHEEL_SAMPLE - 1, False)):
        rows, _ = oracle.topsim(g.offs, g.nbrs, 0, smp, 2, C=C_DECAY, seed=SEED_M, sources=np.array([hub], np.int32))
        assert (int((rows[0] > 0).sum()) > 4096) == full
    sources = np.array([hub, hub + 1, 0, hub + 2049, int(g.comps[1][0])], np.int32)
    got = _gpu_m(g, 0, capacity, WHEEL_SAMPLE, 2, sources)
    ref = oracle.topsim_m(g.offs, g.nbrs, 0, WHEEL_SAMPLE, 2, capacity, C=C_DECAY, seed=SEED_M, sources=sources,
                          nthreads=8)
    _m_equal(got, ref)
    assert got[2][0] == capacity


@pytest.mark.gpu
def test_m_capacity_4097_unsupported(gw):
    """Case 4."""
    from gwamd import _lib as Cl
    g = _tile_union(gw, 65)
    with pytest.raises(Cl.UnsupportedError, match="capacity"):
        _gpu_m(g, 0, 4097, 100, 2, np.arange(4, dtype=np.int32))


# ---------------------------------------------------------------------------
# k_topsim_levels + k_levels_syrk
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("step", TILE_STEPS)
@pytest.mark.parametrize("V", TILE_V)
def test_double_sample_tile_edges(gw, V, step):
    """Case 5: n on both sides of the 64-tiles; K = STEP n is a multiple of 16
    only at V 64 and 128 (and V 2 at STEP 8)."""
    g = _tile_union(gw, V)
    sim = _gpu_sim(g, "gw_topsim_double", 3 ** step, step, C_DECAY, SEED_D)
    ref, mask = _r2(g, step, 3 ** step)
    _full_symmetric(sim, mask)
    _close(sim, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("sample", (50, 700))
@pytest.mark.parametrize("step", (1, 5, 6, 7, 8))
def test_double_sample_random_equals_oracle(gw, oracle, step, sample):
    """Case 6: the 600-wheel's hub draws walkers at level 0 at SAMPLE 50; at
    SAMPLE 700 its 599 children spawn 1198 walkers (several scan trips)."""
    g = _union(gw, 680, 3, (("wheel", 600),))
    assert g.deg[int(g.comps[0][0])] == 599
    sim = _gpu_sim(g, "gw_topsim_double", sample, step, C_DECAY, SEED_D)
    ref = oracle.topsim_double_sample(g.offs, g.nbrs, sample, step, C=C_DECAY, seed=SEED_D, nthreads=8)
    assert not np.isnan(sim).any()
    assert np.array_equal(sim, sim.T) and not np.diag(sim).any()
    _close(sim, ref)


@pytest.mark.gpu
def test_double_sample_zero_sample(gw):
    """Case 7."""
    g = _tile_union(gw, 65)
    sim = _gpu_sim(g, "gw_topsim_double", 0, 3, C_DECAY, SEED_D)
    assert np.array_equal(sim, np.zeros((65, 65)))


# ---------------------------------------------------------------------------
# gw_topsim_dev + k_levels_dot
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("step", TILE_STEPS)
@pytest.mark.parametrize("V", (65, 129))
def test_dev_deterministic_equals_r2(gw, V, step):
    """Case 8."""
    g = _tile_union(gw, V)
    topK = 24
    cand = _cands(g, topK)
    total = _sample_total_for(3 ** step, step, topK, 0)
    sim = _gpu_sim(g, "gw_topsim_dev", total, step, topK, 0, C_DECAY, SEED_DEV, cand)
    ref, _ = _r2(g, step, 3 ** step)
    assert not np.isnan(sim).any()
    _close(sim, np.where(_cand_mask(cand), ref, 0.0))  # support included: exact zeros everywhere else


@pytest.mark.gpu
def test_dev_several_batches_equals_oracle(gw, oracle):
    """Case 9: the source loop of gw_dev_topsim_dev takes five trips; the
    Philox call id 1 + i topK + r is global, the row indices batch-relative."""
    n, step, topK = 1500, 8, 31
    g = _union(gw, n, 3)
    bsrc = max(1, min(n, (1 << 30) // (step * n * 8 * (1 + topK))))
    assert bsrc < n / 3
    cand = _cands(g, topK)
    total = _sample_total_for(50, step, topK, 1)
    sim = _gpu_sim(g, "gw_topsim_dev", total, step, topK, 1, C_DECAY, SEED_DEV, cand)
    ref = oracle.topsim_dev(g.offs, g.nbrs, 50, step, cand, C=C_DECAY, seed=SEED_DEV, nthreads=8)
    assert not np.isnan(sim).any()
    _close(sim, ref)
    assert not sim[~_cand_mask(cand)].any()
    assert np.count_nonzero(ref[n - bsrc // 2:]) > 0  # the last batch has entries


@pytest.mark.gpu
@pytest.mark.parametrize("total,topK,single", [(1000, 0, 0), (1, 24, 0), (1000, 24, 3)])
def test_dev_topk_zero_and_sample_zero(gw, total, topK, single):
    """Case 10."""
    g = _tile_union(gw, 65)
    assert topK == 0 or _dev_sample(total, 3, topK, single) == 0
    args = (_cands(g, topK),) if topK else (None,)
    sim = _gpu_sim(g, "gw_topsim_dev", total, 3, topK, single, C_DECAY, SEED_DEV, *args)
    assert np.array_equal(sim, np.zeros((65, 65)))


# ---------------------------------------------------------------------------
# DoubleRandomWalk
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("step", (1, 2, 5, 8))
@pytest.mark.parametrize("sample", (1, 7, 64, 257))
def test_double_random_walk_closed_forms(gw, sample, step):
    """Case 11: bitwise 0.5 / 0 (every partial sum k * 0.5 and the division by
    SAMPLE^2 are exact).  V = 10: n SAMPLE is never a multiple of 256, and at
    SAMPLE 257 the hub's bucket of 771 walks spans four thread blocks."""
    g, exp = _r4(gw, 0.5)
    assert (g.V * sample) % 256 != 0
    sim = _gpu_sim(g, "gw_double_random_walk", sample, step, 0.5, SEED_DRW)
    assert np.array_equal(sim, exp)


@pytest.mark.gpu
@pytest.mark.parametrize("step", (1, 2, 6, 7, 8))
def test_double_random_walk_random_equals_oracle(gw, oracle, step):
    """Case 12: about a third of the 299 x 9 rim walks sit on the hub at step
    0, a bucket of several thread blocks."""
    g = _union(gw, 430, 3, (("wheel", 300),))
    assert (g.V * 9) % 256 != 0
    sim = _gpu_sim(g, "gw_double_random_walk", 9, step, C_DECAY, SEED_DRW)
    ref = oracle.double_random_walk(g.offs, g.nbrs, 9, step, C=C_DECAY, seed=SEED_DRW, nthreads=8)
    assert not np.isnan(sim).any()
    assert np.array_equal(sim, sim.T) and not np.diag(sim).any() and not sim[0].any()
    _close(sim, ref)
