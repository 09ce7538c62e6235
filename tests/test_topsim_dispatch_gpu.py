"""TopSim dispatch matrix: every kernel family, STEP 1..8, the three variants
and the three output forms, on both sides of every switch-over of
gw_dev_topsim_prepare (V 9216/9217 and 12288/12289, SAMPLE 2048/2049, the
1792-entry LDS offset arrays), each case asserting the kernel it ran.

Graphs are disjoint unions of tiny components (cycles, paths, doubled edges;
with max_deg 3 also stars, K4 and a self-loop), so V alone picks the kernel
family and the reference is independent of the oracle: in the deterministic
regime (every path's mass >= its degree) TopSim / SAMPLE is naive SimRank after
STEP sweeps, a dense numpy iteration per component (_naive_block), with exact
zeros across components.

Tolerance facts.  test_oracle_equals_numpy_on_component_unions measures the
oracle against _naive_block on these graphs (max |rows / SAMPLE - numpy|,
variants 0 and 1, walkers == 0 everywhere):
  max_deg 2, V 12305, STEP 5, SAMPLE 2^10:  9.7e-16
  max_deg 2, V 12305, STEP 7, SAMPLE 2^14:  1.3e-14
  max_deg 2, V 12305, STEP 8, SAMPLE 2^16:  7.3e-14
  max_deg 3, V 402,   STEP 5, SAMPLE 3^10:  1.5e-14
all under the naive-SimRank KAT's atol = 1e-13 on rows / SAMPLE
(test_topsim_gpu.test_topsim_kat_naive_simrank), which every deterministic
case here uses.  (The deviation is the summation's: the oracle, like the
kernels, adds up to 2^16 equal path terms one by one, numpy a handful per
entry; the kernels measured the same figures on the MI355X.)  max_deg 3 stops
at STEP 5: at STEP 6 the oracle itself is at 5.5e-14 and at STEP 8 at
2.8e-12.  The random-regime cases compare with the
oracle at the suite's TopSim tolerances (rtol 1e-12, atol 1e-12 * SAMPLE,
identical support, exact extension / pair-update / walker counts).

The pipelined hash kernel cannot be reached deterministically at SAMPLE 3^10
(above kPipeMaxSample with no walkers the host replay declines it), so its
max_deg 3 case runs STEP 3 at SAMPLE 3^6.
"""
import numpy as np
import pytest

from test_topsim_gpu import _topk_match

C_DECAY = 0.6
KAT_ATOL = 1e-13

# family -> (V, kernel name); V alone selects the accumulator / kernel family
K_2WG0 = "k_topsim_2wg<{s}, 0>"
K_ROW = "k_topsim_pipe_row<{s}>"
K_PLAIN = "k_topsim<{s}, 0>"
K_PIPE = "k_topsim_pipe<{s}>"
K_2WG2 = "k_topsim_2wg<{s}, 2>"


# ---------------------------------------------------------------------------
# generator and independent reference
# ---------------------------------------------------------------------------
def _edges(kind, k):
    if kind == "cycle":
        return [(i, (i + 1) % k) for i in range(k)]
    if kind == "path":
        return [(i, i + 1) for i in range(k - 1)]
    if kind == "double":
        return [(0, 1), (0, 1)]
    if kind == "star":
        return [(0, 1), (0, 2), (0, 3)]
    if kind == "k4":
        return [(a, b) for a in range(4) for b in range(a + 1, 4)]
    if kind == "loop":  # one duplicate edge and one self-loop (degrees 2, 3, 3)
        return [(0, 1), (0, 1), (1, 2), (2, 2)]
    if kind == "wheel":  # hub 0, rim 1..k-1: hub-rim spokes and the rim cycle
        m = k - 1
        return [(0, 1 + i) for i in range(m)] + [(1 + i, 1 + (i + 1) % m) for i in range(m)]
    raise ValueError(kind)


def _kinds(max_deg):
    kinds = [("cycle", k) for k in range(3, 12)] + [("path", k) for k in range(2, 9)] + [("double", 2)]
    if max_deg == 3:
        kinds += [("star", 4), ("k4", 4), ("loop", 3)]
    return kinds


def _component_union(v_target, max_deg, first=()):
    """Edge list (src, dst) and the components (arrays of vertex ids) of a
    disjoint union with exactly v_target vertices: vertex 0 isolated, the
    components of `first`, then the kinds of _kinds(max_deg) in turn, padded
    with a path."""
    src, dst, comps = [], [], []
    nxt, i = 1, 0
    kinds = _kinds(max_deg)
    pending = list(first)
    while nxt < v_target:
        if pending:
            kind, k = pending.pop(0)
            assert nxt + k <= v_target
        else:
            kind, k = kinds[i % len(kinds)]
            i += 1
            if nxt + k > v_target:
                kind, k = "path", v_target - nxt
        for a, b in _edges(kind, k):
            src.append(nxt + a)
            dst.append(nxt + b)
        comps.append(np.arange(nxt, nxt + k, dtype=np.int64))
        nxt += k
    assert nxt == v_target
    return np.asarray(src, np.int64), np.asarray(dst, np.int64), comps


def _naive_block(offs, nbrs, comp, C, iters):
    """Naive SimRank over one component in dense numpy: P[i, j] = multiplicity
    / deg, S <- C P S P^T with the diagonal reset to 1 each round, diagonal
    zeroed at the end (as sim[i][i] = 0)."""
    idx = {int(v): i for i, v in enumerate(comp)}
    k = len(comp)
    P = np.zeros((k, k))
    for i, v in enumerate(comp):
        nb = nbrs[offs[v]:offs[v + 1]]
        for u in nb:
            P[i, idx[int(u)]] += 1.0  # KeyError: the component is not closed
        if len(nb):
            P[i] /= len(nb)
    S = np.eye(k)
    for _ in range(iters):
        S = C * (P @ S @ P.T)
        np.fill_diagonal(S, 1.0)
    np.fill_diagonal(S, 0.0)
    return S


class _Union:
    def __init__(self, gw, V, max_deg, first=()):
        s, d, self.comps = _component_union(V, max_deg, first)
        self.G = gw.GWGraph.from_edges(s, d, semantics="java", vcount=V)
        c = self.G.export_csr()  # the loader's multigraph counts, not the test's
        self.offs, self.nbrs, self.V = c["offsets"], c["nbrs"], V
        assert len(self.offs) == V + 1 and int(self.offs[-1]) == 2 * len(s)
        assert int(np.diff(self.offs).max()) == max(max_deg, max([k - 1 for _, k in first], default=0))
        self._dev = False
        self._ref = {}

    @property
    def handle(self):
        if not self._dev:
            self.G.to_device(0)
            self._dev = True
        return self.G.handle

    def std_sources(self, ncomp=60):
        """Vertex 0 plus the first and last vertex of ~ncomp components: one of
        every kind (the first round) and a stride over the rest, the padding
        path included."""
        nk = min(20, len(self.comps))
        pick = list(range(nk)) + np.linspace(nk, len(self.comps) - 1, ncomp - nk).astype(int).tolist()
        out = [0]
        for ci in dict.fromkeys(pick):
            c = self.comps[ci]
            out += [int(c[0]), int(c[-1])] if len(c) > 1 else [int(c[0])]
        return np.asarray(out, np.int32)

    def comp_of(self, v):
        starts = np.asarray([c[0] for c in self.comps])
        return self.comps[int(np.searchsorted(starts, v, side="right")) - 1] if v > 0 else np.zeros(0, np.int64)

    def naive_rows(self, sources, step):
        """(expected rows / SAMPLE, own-component mask) from _naive_block; computed
        once per (sources, step) and shared."""
        key = (sources.tobytes(), step)
        if key not in self._ref:
            exp = np.zeros((len(sources), self.V))
            mask = np.zeros((len(sources), self.V), bool)
            for r, v in enumerate(sources):
                comp = self.comp_of(int(v))
                if len(comp):
                    S = _naive_block(self.offs, self.nbrs, comp, C_DECAY, step)
                    exp[r, comp] = S[int(v) - int(comp[0])]
                    mask[r, comp] = True
            exp.setflags(write=False)
            mask.setflags(write=False)
            self._ref[key] = (exp, mask)
        return self._ref[key]


_UNIONS = {}


def _union(gw, V, max_deg, first=()):
    key = (V, max_deg, tuple(first))
    if key not in _UNIONS:
        _UNIONS[key] = _Union(gw, V, max_deg, first)
    return _UNIONS[key]


# ---------------------------------------------------------------------------
# 2. CPU anchor: the oracle against numpy on these shapes
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("V,max_deg,step", [(402, 3, s) for s in range(1, 6)] + [(12305, 2, s) for s in range(1, 9)])
def test_oracle_equals_numpy_on_component_unions(gw, oracle, V, max_deg, step):
    g = _union(gw, V, max_deg)
    sample = max_deg ** (2 * step)
    sources = g.std_sources(40)
    exp, mask = g.naive_rows(sources, step)
    for variant in (0, 1):
        rows, st = oracle.topsim(g.offs, g.nbrs, variant, sample, step, C=C_DECAY, seed=11, sources=sources,
                                 nthreads=8)
        assert st["walkers"] == 0
        print(f"V={V} STEP={step} variant={variant} max|rows/SAMPLE - numpy| = {np.abs(rows / sample - exp).max():.3g}")
        np.testing.assert_allclose(rows / sample, exp, rtol=0, atol=KAT_ATOL)
        assert not rows[~mask].any()  # exact zeros outside the source's component


# ---------------------------------------------------------------------------
# GPU call helpers: each returns the kernel the call ran
# ---------------------------------------------------------------------------
def _kernel(h):
    from gwamd import _lib as Cl
    assert Cl.lib().gw_topsim_last_launches(h) == 1
    return Cl.lib().gw_topsim_kernel(h).decode()


def _dense(g, variant, sample, step, sources, seed=11):
    import torch
    from gwamd import _lib as Cl
    h = g.handle
    src = torch.as_tensor(np.asarray(sources, np.int32), device="cuda")
    rows = torch.empty((len(src), g.V), dtype=torch.float64, device="cuda")
    st = torch.zeros(4, dtype=torch.int64, device="cuda")
    Cl.check(Cl.lib().gw_topsim_dense(h, variant, sample, step, C_DECAY, seed, Cl.ptr(src), len(src), Cl.ptr(rows),
                                      Cl.ptr(st), None), h)
    return rows.cpu().numpy(), st.cpu().numpy(), _kernel(h)


def _topk(g, variant, sample, step, sources, K, seed=11):
    import torch
    from gwamd import _lib as Cl
    h = g.handle
    src = torch.as_tensor(np.asarray(sources, np.int32), device="cuda")
    ids = torch.full((len(src), K), -7, dtype=torch.int32, device="cuda")
    sc = torch.full((len(src), K), -7.0, dtype=torch.float64, device="cuda")
    st = torch.zeros(4, dtype=torch.int64, device="cuda")
    Cl.check(Cl.lib().gw_topsim(h, variant, sample, step, C_DECAY, seed, Cl.ptr(src), len(src), K, Cl.ptr(ids),
                                Cl.ptr(sc), Cl.ptr(st), None), h)
    return ids.cpu().numpy(), sc.cpu().numpy(), st.cpu().numpy(), _kernel(h)


def _sparse(g, variant, sample, step, sources, capacity, seed=11):
    import torch
    from gwamd import _lib as Cl
    h = g.handle
    src = torch.as_tensor(np.asarray(sources, np.int32), device="cuda")
    b = torch.empty(len(src), dtype=torch.int64, device="cuda")
    ln = torch.empty(len(src), dtype=torch.int32, device="cuda")
    ids = torch.empty(max(capacity, 1), dtype=torch.int32, device="cuda")
    sc = torch.empty(max(capacity, 1), dtype=torch.float64, device="cuda")
    used = torch.full((1,), 123, dtype=torch.int64, device="cuda")
    st = torch.zeros(4, dtype=torch.int64, device="cuda")
    rc = Cl.lib().gw_topsim_sparse(h, variant, sample, step, C_DECAY, seed, Cl.ptr(src), len(src), capacity,
                                   Cl.ptr(b), Cl.ptr(ln), Cl.ptr(ids), Cl.ptr(sc), Cl.ptr(used), Cl.ptr(st), None)
    return rc, b.cpu().numpy(), ln.cpu().numpy(), ids.cpu().numpy(), sc.cpu().numpy(), int(used.cpu()[0]), \
        st.cpu().numpy(), _kernel(h)


def _same_counters(st, rst):
    assert int(st[0]) == rst["extensions"] and int(st[1]) == rst["pair_updates"] and int(st[3]) == rst["walkers"]


def _same_row(a, b):
    """Two runs of one source: the same support, values equal up to the order
    of the atomic adds."""
    assert np.array_equal(a > 0, b > 0)
    np.testing.assert_allclose(a, b, rtol=1e-12, atol=0)


def _rows_equal_oracle(rows, ref, variant, sample):
    # SingleRandomWalk rows are divided by SAMPLE already (entries <= 1)
    np.testing.assert_allclose(rows, ref, rtol=1e-12, atol=1e-12 * (1 if variant == 2 else sample))
    assert np.array_equal(rows > 0, ref > 0)


# ---------------------------------------------------------------------------
# 3. deterministic matrix against numpy
# ---------------------------------------------------------------------------
def _det_cases():
    out = []
    for V, variant, name, steps in [(9216, 0, K_2WG0, range(1, 9)), (9217, 0, K_ROW, range(1, 9)),
                                    (12288, 0, K_ROW, range(1, 9)), (12289, 0, K_PIPE, range(1, 6)),
                                    (12289, 0, K_2WG2, range(6, 9)),  # SAMPLE > 2048, replay: W = 0
                                    (9217, 1, K_PLAIN, range(1, 9)), (12289, 1, K_2WG2, range(1, 9))]:
        out += [(V, 2, variant, s, 2 ** (2 * s), name.format(s=s)) for s in steps]
    out += [(9216, 3, 0, 5, 3 ** 10, K_2WG0.format(s=5)), (9217, 3, 0, 5, 3 ** 10, K_ROW.format(s=5)),
            (9217, 3, 1, 5, 3 ** 10, K_PLAIN.format(s=5)), (12289, 3, 0, 5, 3 ** 10, K_2WG2.format(s=5)),
            (12289, 3, 0, 3, 3 ** 6, K_PIPE.format(s=3))]
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("V,max_deg,variant,step,sample,kernel", _det_cases())
def test_deterministic_cell_equals_numpy(gw, V, max_deg, variant, step, sample, kernel):
    g = _union(gw, V, max_deg)
    sources = g.std_sources(60)
    assert len(sources) <= 130
    rows, st, ran = _dense(g, variant, sample, step, sources)
    assert ran == kernel
    assert st[3] == 0  # no walkers: the deterministic regime
    exp, mask = g.naive_rows(sources, step)
    print(f"{ran} V={V} max|rows/SAMPLE - numpy| = {np.abs(rows / sample - exp).max():.3g}")
    np.testing.assert_allclose(rows / sample, exp, rtol=0, atol=KAT_ATOL)
    assert not rows[~mask].any()


# ---------------------------------------------------------------------------
# 4. random regime against the oracle
# ---------------------------------------------------------------------------
def _rand_cases():
    out = []
    for s in range(1, 9):
        out += [(9216, 0, 37, s, K_2WG0), (9217, 0, 37, s, K_ROW), (12288, 0, 37, s, K_ROW), (12289, 0, 37, s, K_PIPE),
                # SingleRandomWalk off the small-row path
                (9216, 2, 37, s, K_2WG0), (9217, 2, 37, s, K_PLAIN), (12289, 2, 37, s, K_2WG2),
                # variant 0 above kPipeMaxSample: the replay's W/E ~ max(0, 2 STEP - 11) < 16
                (12289, 0, 2049, s, K_2WG2)]
    out += [(12289, 0, 2048, s, K_PIPE) for s in (6, 7, 8)]
    return [(V, v, smp, s, k.format(s=s)) for V, v, smp, s, k in out]


@pytest.mark.gpu
@pytest.mark.parametrize("V,variant,sample,step,kernel", _rand_cases())
def test_random_cell_equals_oracle(gw, oracle, V, variant, sample, step, kernel):
    g = _union(gw, V, 2)
    sources = g.std_sources(60)
    rows, st, ran = _dense(g, variant, sample, step, sources)
    assert ran == kernel
    ref, rst = oracle.topsim(g.offs, g.nbrs, variant, sample, step, C=C_DECAY, seed=11, sources=sources, nthreads=8)
    _rows_equal_oracle(rows, ref, variant, sample)
    _same_counters(st, rst)
    # a degree-2 vertex at level 2 STEP - 1 carries mass SAMPLE / 2^(2 STEP - 1): below 2 it spawns walkers
    # (SAMPLE 37 from STEP 3, both sides of the kPipeMaxSample pair from STEP 6)
    if variant == 2 or sample < 2 ** (2 * step):
        assert rst["walkers"] > 0


# one case per family with more sources than the 1,024 persistent workgroups:
# workgroups run several sources in a row (top-k: the pipelined kernels'
# deferred ordering)
FAMILIES = [(9216, 0, 37, K_2WG0), (9217, 0, 37, K_ROW), (9217, 2, 37, K_PLAIN), (12289, 0, 37, K_PIPE),
            (12289, 2, 37, K_2WG2)]
FAMILY_IDS = ["2wg_row", "pipe_row", "plain_row", "pipe_hash", "2wg_hash"]


@pytest.mark.gpu
@pytest.mark.parametrize("V,variant,sample,kernel", FAMILIES, ids=FAMILY_IDS)
def test_many_sources_per_workgroup(gw, oracle, V, variant, sample, kernel):
    g = _union(gw, V, 2)
    step, K = 3, 20
    sources = np.arange(0, V, 8, dtype=np.int32)
    assert len(sources) >= 1100
    ids, sc, st, ran = _topk(g, variant, sample, step, sources, K)
    assert ran == kernel.format(s=step)
    oi, osc, ost = oracle.topsim_topk(g.offs, g.nbrs, variant, sample, step, K, C=C_DECAY, seed=11, sources=sources,
                                      nthreads=8)
    _same_counters(st, ost)
    assert ost["walkers"] > 0
    _topk_match(ids, sc, oi, osc)
    m = (oi >= 0).sum(axis=1)
    for r in range(len(sources)):
        assert np.all(ids[r, m[r]:] == -1) and np.all(sc[r, m[r]:] == 0.0)


@pytest.mark.gpu
@pytest.mark.parametrize("step", [2, 7])
@pytest.mark.parametrize("V,variant,sample,kernel", FAMILIES, ids=FAMILY_IDS)
def test_output_forms(gw, oracle, V, variant, sample, kernel, step):
    """Top-k (K 1, 20, 256), sparse rows with the capacity protocol, and dense
    rows of one family, against the oracle's rows of the same call."""
    from gwamd import _lib as Cl
    g = _union(gw, V, 2)
    kernel = kernel.format(s=step)
    sample = 7  # below 2^(2 STEP) at both STEP values: walkers run
    base = g.std_sources(60)
    sources = np.concatenate([base, base[5:6]])  # a duplicated vertex: identical rows
    ref, rst = oracle.topsim(g.offs, g.nbrs, variant, sample, step, C=C_DECAY, seed=11, sources=sources, nthreads=8)
    # dense
    rows, st, ran = _dense(g, variant, sample, step, sources)
    assert ran == kernel
    _rows_equal_oracle(rows, ref, variant, sample)
    _same_counters(st, rst)
    assert rst["walkers"] > 0
    _same_row(rows[-1], rows[5])
    assert not rows[0].any()
    # top-k: every row has fewer than 20 nonzeros (components of <= 11 vertices)
    assert 0 < (ref > 0).sum(axis=1).max() < 20
    for K in (1, 20, 256):
        oi, osc, ost = oracle.topsim_topk(g.offs, g.nbrs, variant, sample, step, K, C=C_DECAY, seed=11,
                                          sources=sources, nthreads=8)
        ids, sc, st, ran = _topk(g, variant, sample, step, sources, K)
        assert ran == kernel
        _same_counters(st, ost)
        _topk_match(ids, sc, oi, osc)
        m = (oi >= 0).sum(axis=1)
        for r in range(len(sources)):
            assert np.all(ids[r, m[r]:] == -1) and np.all(sc[r, m[r]:] == 0.0)  # tail past the row's nonzeros
            assert np.all(ids[r, :m[r]] >= 0) and np.all(sc[r, :m[r]] > 0.0)
        assert m[0] == 0  # the isolated source: all -1
        _topk_match(ids[-1:], sc[-1:], ids[5:6], sc[5:6])
        if K == 20:  # nsrc = 1
            i1, s1, st1, ran = _topk(g, variant, sample, step, sources[7:8], K)
            assert ran == kernel
            _topk_match(i1, s1, oi[7:8], osc[7:8])
            assert np.all(i1[0, m[7]:] == -1) and np.all(s1[0, m[7]:] == 0.0)
    # sparse rows: too small -> GW_ERR_CAPACITY, *used = room needed, rows that did not fit marked -1
    need = int((ref > 0).sum())
    rc, b, ln, ids, sc, used, st, ran = _sparse(g, variant, sample, step, sources, need // 3)
    assert ran == kernel
    assert rc == Cl.GW_ERR_CAPACITY and used == need
    assert np.all((ln == -1) == (b == -1)) and (ln == -1).any() and int(ln[ln >= 0].sum()) <= need // 3
    rc, b, ln, ids, sc, used, st, ran = _sparse(g, variant, sample, step, sources, need)
    assert ran == kernel
    assert rc == 0 and used == need and int(ln.sum()) == need and np.all(ln >= 0)
    _same_counters(st, rst)
    got = np.zeros_like(ref)
    for r in range(len(sources)):
        row_ids = ids[b[r]:b[r] + ln[r]]
        assert len(np.unique(row_ids)) == ln[r]
        got[r, row_ids] = sc[b[r]:b[r] + ln[r]]
    np.testing.assert_allclose(got, ref, rtol=1e-12, atol=0)
    assert np.array_equal(got > 0, ref > 0)


# ---------------------------------------------------------------------------
# 5. the 1792-entry LDS offset arrays (TS_CO_LDS)
# ---------------------------------------------------------------------------
WHEELS = (1790, 1791, 1792, 1793)


def _wheel_union(gw, V):
    return _union(gw, V, 2, first=tuple(("wheel", m + 1) for m in WHEELS))


@pytest.mark.gpu
@pytest.mark.parametrize("step", [2, 3])
@pytest.mark.parametrize("V,kernel", [(9216, K_2WG0), (12288, K_ROW), (12289, K_PIPE)],
                         ids=["2wg_row", "pipe_row", "pipe_hash"])
def test_offset_arrays_at_1792_entries(gw, oracle, V, kernel, step):
    """A wheel's hub with m rim vertices at SAMPLE = m enumerates one level of
    m nodes of mass 1 and degree 3: m level entries and m spawners, so both
    sz + 1 <= 1792 and ns + 1 <= 1792 flip between m = 1791 and 1792."""
    g = _wheel_union(gw, V)
    sizes = []
    for ci, m in enumerate(WHEELS):
        comp = g.comps[ci]
        hub = int(comp[0])
        assert len(comp) == m + 1 and g.offs[hub + 1] - g.offs[hub] == m
        assert np.all(np.diff(g.offs)[comp[1:]] == 3)
        _, hst = oracle.topsim(g.offs, g.nbrs, 0, m, step, C=C_DECAY, seed=11, sources=np.array([hub], np.int32))
        assert hst["max_frontier"] == m and hst["walkers"] == m
        sizes.append(hst["max_frontier"] + 1)
        sources = np.array([hub, hub + 1, hub + 1 + m // 2, 0, int(g.comps[len(WHEELS)][0])], np.int32)
        rows, st, ran = _dense(g, 0, m, step, sources)
        assert ran == kernel.format(s=step)
        ref, rst = oracle.topsim(g.offs, g.nbrs, 0, m, step, C=C_DECAY, seed=11, sources=sources, nthreads=8)
        _rows_equal_oracle(rows, ref, 0, m)
        _same_counters(st, rst)
    assert sizes[1] == 1792 and sizes[2] == 1793  # the four cases straddle the 1792-entry arrays
