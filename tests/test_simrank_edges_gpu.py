"""Naive SimRank (gw_simrank.hip, k_sr_gather) at its structural edges, against
a long-double evaluation of the recurrence.

The gather kernel sums a row of the padded adjacency stream as 16-entry lane
sums, a DPP segmented scan over a wave's 64 lanes and a carry from one
1024-entry chunk to the next; rows are dealt to 16 wave slices per output
window, isolated vertices are compacted away, and deg(v)*deg(w) is Java's
`int` product (SimRank.java:76, wrap-around kept).  The loader keeps repeated
edge lines (Java multigraph), so a few dozen vertices reach every row length,
start lane, window count and degree product that matters.

Reference: S' = C * (A S A^T) / dd in np.longdouble over the integer count
matrix A, dd = the degree product reduced to a signed 32-bit value, diagonal
kept at 1 between rounds and zeroed at the end.  The oracle's fp64 Java-order
loop is NOT the reference on long rows: adding one repeated term millions of
times in sequence rounds with a bias (test_oracle_drifts_on_long_rows).

Tolerance: rtol 1e-12 / atol 1e-15.  Outside the wrap graphs all terms are
non-negative; a row total passes a 16-term lane sum, at most 6 scan steps and
d/1024 carries: about 30 roundings per pass, 7e-15 relative per round,
5e-14 at 7 rounds, a margin of 20.  On the wrap graphs the bound holds while
sum|terms| / |sum terms| stays below 100, which the tests assert."""
import functools

import numpy as np
import pytest

RTOL, ATOL = 1e-12, 1e-15
SR_K, SR_CHUNK, SR_WAVES = 16, 1024, 16   # gw_simrank.hip: entries per lane, per wave trip, waves per workgroup
LD = np.longdouble


# ---- the reference -----------------------------------------------------------------------------------------------
def java_int(x):
    """A Python int / int64 array reduced to Java's signed 32-bit `int`."""
    return (x + (1 << 31)) % (1 << 32) - (1 << 31)


def count_matrix(offs, nbrs):
    n = len(offs) - 1
    A = np.zeros((n, n), np.int64)
    np.add.at(A, (np.repeat(np.arange(n), np.diff(offs)), np.asarray(nbrs, np.int64)), 1)
    assert np.array_equal(A, A.T), "the graph is undirected: the count matrix is symmetric"
    return A


def _asat(A, S):
    """A S A^T in long double over A's nonzero counts only (long double has no
    BLAS, and the data graphs' count matrices are sparse)."""
    r, c = np.nonzero(A)                        # row-major: r ascending
    rows, starts = np.unique(r, return_index=True)
    w = A[r, c].astype(LD)[:, None]

    def left(X):                                # A @ X
        out = np.zeros_like(X)
        if len(r):
            out[rows] = np.add.reduceat(w * X[c], starts, axis=0)
        return out
    return left(left(S).T).T


def reference(offs, nbrs, C, iters, want_cond=False):
    """SimRank.java:36-77 in long double.  With want_cond also the largest
    sum|terms| / |sum terms| over the nonzero pairs of every round."""
    A = count_matrix(offs, nbrs)
    n = len(A)
    deg = np.diff(offs).astype(np.int64)
    assert np.array_equal(A.sum(1), deg)
    live = np.outer(deg > 0, deg > 0) & ~np.eye(n, dtype=bool)   # sim(v, v) is 1 without a division
    dd = java_int(np.outer(deg, deg))
    assert np.all(dd[live] != 0), "a degree product congruent to 0 mod 2^32 divides by zero"
    ddl = np.where(live, dd, 1).astype(LD)
    S = np.eye(n, dtype=LD)
    cond = 1.0
    for _ in range(iters):
        T = _asat(A, S)
        if want_cond:
            Tabs = _asat(A, np.abs(S))
            nz = live & (T != 0)
            if nz.any():
                cond = max(cond, float((Tabs[nz] / np.abs(T[nz])).max()))
        S = LD(C) * T / ddl
        S[~live] = 0
        np.fill_diagonal(S, 1)
    np.fill_diagonal(S, 0)
    return (S, cond) if want_cond else S


def next_round(offs, nbrs, C, S, v, w):
    """SimRank.sim(v, w) (:67-77), v != w of nonzero degree: one more round for
    that pair over the matrix S as it stands, in long double."""
    A = count_matrix(offs, nbrs).astype(LD)
    deg = np.diff(offs)
    return LD(C) * (A[v] @ np.asarray(S, LD) @ A[w]) / LD(int(java_int(int(deg[v]) * int(deg[w]))))


def ulps(x, ref):
    """|x - ref| in units of the fp64 spacing at ref (long double ref)."""
    r64 = np.asarray(ref, np.float64)
    return float(np.max(np.abs(np.asarray(x, LD) - ref) / np.spacing(np.maximum(np.abs(r64), np.finfo(np.float64).tiny))))


# ---- graphs ------------------------------------------------------------------------------------------------------
def write_graph(path, lines, V):
    from gwamd import topsim
    path.write_text("".join(f"{u},{v}\n" for u, v in lines))
    return topsim.Graph(str(path), V, separator=",")


LONG_M = 48
LONG_CLASSES = (15, 16, 17, 255, 256, 257, 511, 512, 513, 1008, 1009, 1023, 1024, 1025, 1040, 1041, 2047, 2048, 2049)


@functools.lru_cache(maxsize=None)
def long_row_lines():
    """(a) 48 live vertices: a random tree + 3m extra edges + an edge from every
    vertex to the hub, then multiplicities raised on those edges until one
    vertex has each degree of LONG_CLASSES; the hub takes what is left over
    (far above 4096).  Lines shuffled, so neighbours mix inside a lane's 16."""
    m = LONG_M
    rng = np.random.default_rng(20240611)
    mult = {}
    for v in range(1, m):
        mult[(int(rng.integers(v)), v)] = 1
    while len(mult) < (m - 1) + 3 * m:
        u, v = (int(x) for x in rng.integers(m, size=2))
        if u != v:
            mult.setdefault((min(u, v), max(u, v)), 1)
    deg = np.zeros(m, np.int64)
    for (u, v), c in mult.items():
        deg[u] += c
        deg[v] += c
    hub = int(np.argmax(deg))
    for v in range(m):
        if v != hub:
            mult.setdefault((min(v, hub), max(v, hub)), 1)
    deg[:] = 0
    for (u, v), c in mult.items():
        deg[u] += c
        deg[v] += c
    small = [v for v in range(m) if v != hub and deg[v] <= 14]
    assert len(small) > len(LONG_CLASSES), "skeleton too dense for the short-row classes"
    chosen = [int(v) for v in rng.permutation(small)[:len(LONG_CLASSES)]]
    target = {v: t for v, t in zip(chosen, LONG_CLASSES)}
    nbr = {v: [] for v in range(m)}
    for (u, v) in mult:
        nbr[u].append(v)
        nbr[v].append(u)
    for v in sorted(chosen, key=lambda x: target[x]):       # ascending: finished rows are never touched again
        need = int(target[v] - deg[v])
        assert need >= 0
        for u in nbr[v]:
            if u != hub and target.get(u, 0) > target[v]:
                give = int(min(rng.integers(0, need // 4 + 1), (target[u] - deg[u]) // 2, need))
                mult[(min(u, v), max(u, v))] += give
                deg[u] += give
                deg[v] += give
                need -= give
        mult[(min(v, hub), max(v, hub))] += need
        deg[v] += need
        deg[hub] += need
    lines = [e for e, c in mult.items() for _ in range(c)]
    return tuple(lines[i] for i in rng.permutation(len(lines)))


def assert_long_row_classes(g, ids=None):
    deg = np.diff(g._offs)
    if ids is not None:
        deg = deg[ids]
    have = set(int(d) for d in deg)
    assert all(c in have for c in LONG_CLASSES), sorted(set(LONG_CLASSES) - have)
    assert np.any((deg > 0) & (deg <= 14)) and np.any(deg > 4096) and np.all(deg > 0) and len(deg) == LONG_M
    padded = int(((deg + SR_K - 1) // SR_K * SR_K).sum())
    assert padded > SR_WAVES * SR_CHUNK, "no wave would run a second trip of the pos loop"


def padded_offsets(g):
    """sr_build_layout's row starts in the padded stream, over the live rows."""
    deg = np.diff(g._offs)
    deg = deg[deg > 0]
    return np.concatenate([[0], np.cumsum((deg + 15) // 16 * 16)]).astype(np.int64)


def wave_slices(poff, j0, j1):
    """k_sr_gather's 16 row-aligned slices [ra, rb) of the window [j0, j1)."""
    e_lo, tot = int(poff[j0]), int(poff[j1] - poff[j0])
    first = lambda e: j0 + int(np.searchsorted(poff[j0:j1 + 1], e, side="left"))
    out = []
    for w in range(SR_WAVES):
        t0, t1 = e_lo + tot * w // SR_WAVES, e_lo + tot * (w + 1) // SR_WAVES
        out.append((j0 if w == 0 else min(first(t0), j1), j1 if w == SR_WAVES - 1 else min(first(t1), j1)))
    return out


# (f) edge multiplicities.  46341^2 = 2^31 + 4633 wraps to -2147479015, 2 * 46341^2 lands on 9266 past 2^32,
# 65537^2 = 2^32 + 131073 lands on 131073.
#
# WRAP_SPECS are the graphs the CPU oracle (or_simrank_naive) is compared on as well, at 1 and 2 rounds.  Its
# sequential fp64 sum is exact only while the term it repeats is exactly representable, so these are stars:
# bipartite, every sum repeats S[2][2] = 1 or a 0.  The products the oracle is checked on with a nonzero numerator
# are the two (0,1) pairs: one wrapped negative, one past 2^32.
#   neg        0 and 1 each tied 46 341 times to 2: (0,1) -> -2147479015 under the numerator 46341^2, score
#              -0.6000026; (0,2), (1,2) -> 9266 (past 2^32), but under a zero numerator in every round
#   star65537  0 and 1 each tied 65 537 times to 2: (0,1) -> 131073 (past 2^32) under 65537^2, score 19661.25;
#              (0,2), (1,2) -> 262146 under a zero numerator
# HEAVY_SPECS run on the GPU only, against the long-double reference: 0 and 1 tied to each other, each with
# self-loops (a self-loop is two entries of its row), so the second round repeats an inexact term 10^9 times,
# where the oracle is off by 1.7e-8 relative on neg_loops.  neg_loops mixes signs in round 2 (sum|terms| /
# |sum terms| = 1.86); pos_loops has positive terms only (1.0).
#   neg_loops  deg 46341, 46341, 6: (0,1) -> -2147479015, score -0.2999625
#   pos_loops  deg 65537, 65537, 6: (0,1) -> 131073, score 9829.725
# or_simrank_round_rows is checked on row 0 of neg_loops at 1 round (integer numerators).
WRAP_SPECS = {
    "neg": (3, (((0, 2), 46341), ((1, 2), 46341))),
    "star65537": (3, (((0, 2), 65537), ((1, 2), 65537))),
}
HEAVY_SPECS = {
    "neg_loops": (3, (((0, 0), 11585), ((1, 1), 11585), ((0, 1), 23168), ((0, 2), 3), ((1, 2), 3))),
    "pos_loops": (3, (((0, 0), 16384), ((1, 1), 16384), ((0, 1), 32766), ((0, 2), 3), ((1, 2), 3))),
}
# name -> (degrees, java_int(deg 0 * deg 1), 1-round score of (0, 1) at C = 0.6 to 7 digits)
WRAP_EXPECT = {
    "neg": ((46341, 46341, 92682), -2147479015, -0.6000026),
    "star65537": ((65537, 65537, 131074), 131073, 19661.25),
    "neg_loops": ((46341, 46341, 6), -2147479015, -0.2999625),
    "pos_loops": ((65537, 65537, 6), 131073, 9829.725),
}


def wrap_graph(name, tmp_path):
    V, spec = (WRAP_SPECS.get(name) or HEAVY_SPECS[name])
    return write_graph(tmp_path / f"wrap_{name}.txt", [e for e, c in spec for _ in range(c)], V)


def assert_wrap_properties(g, name):
    """Each wrap graph has what it is there for (asserted, so an edit to the
    tables cannot silently lose it): its degrees, the wrapped product and score
    of the pair (0, 1), no product that is 0 mod 2^32, rows long enough for 45
    carries in a row, and a second round with sum|terms| / |sum terms| < 100."""
    degs, dd01, s01 = WRAP_EXPECT[name]
    deg = np.diff(g._offs).astype(np.int64)
    assert tuple(deg) == degs
    full = np.outer(deg, deg)
    assert np.all(full[~np.eye(len(deg), dtype=bool)] % (1 << 32) != 0)
    assert java_int(full)[0, 1] == dd01 and full[0, 1] >= 1 << 31
    s1 = reference(g._offs, g._nbrs, 0.6, 1)
    assert s01 != 0 and abs(float(s1[0, 1]) - s01) <= 1e-6 * abs(s01)    # a nonzero numerator over the wrapped product
    if name == "neg":
        assert full[0, 2] > 1 << 32 and java_int(full)[0, 2] == 9266
    assert deg.max() > 45 * SR_CHUNK
    _, cond = reference(g._offs, g._nbrs, 0.6, 2, want_cond=True)
    assert cond < 100, cond


# ---- CPU: the reference and the oracle ---------------------------------------------------------------------------
def _data_graph(name):
    import os
    from conftest import DATA
    from gwamd import topsim
    f, V, sep = {"moreno": ("moreno_crime_crime.txt", 1380, "\t"), "g333": ("0_333_5038.txt", 333, " ")}[name]
    return topsim.Graph(os.path.join(DATA, f), V, separator=sep)


@pytest.mark.parametrize("name,C,iters", [("g333", 0.8, 30), ("g333", 0.6, 3), ("moreno", 0.6, 3)])
def test_reference_equals_pinned_oracle(gw, oracle, name, C, iters):
    """The oracle is pinned to the reference implementation's committed output;
    at these degrees (max 154) its summation error is far below the tolerance."""
    g = _data_graph(name)
    ref = reference(g._offs, g._nbrs, C, iters)
    orc = oracle.simrank_naive(g._offs, g._nbrs, C, iters, nthreads=8)
    np.testing.assert_allclose(orc.astype(LD), ref, rtol=RTOL, atol=ATOL)


def test_reference_iters0_and_isolated(gw, tmp_path):
    g = write_graph(tmp_path / "g.txt", [(1, 2), (2, 3), (3, 1), (3, 5), (5, 5)], 7)
    assert np.all(reference(g._offs, g._nbrs, 0.6, 0) == 0)
    s = reference(g._offs, g._nbrs, 0.6, 3)
    for v in (0, 4, 6):
        assert np.all(s[v] == 0) and np.all(s[:, v] == 0)
    assert np.all(np.diag(s) == 0) and s[1, 2] > 0


@pytest.mark.slow
@pytest.mark.parametrize("name", sorted(WRAP_SPECS))
def test_oracle_wraps_like_java(gw, oracle, tmp_path, name):
    """or_simrank_naive divides by Java's int product: equal to the reference
    on the wrap graphs (2 ulp at 1 round: the numerators are exact integers).
    The pair (0, 1) has a nonzero score over a product wrapped negative (neg)
    and over one past 2^32 (star65537).  The double loop walks 6.4e9 and
    1.3e10 neighbour pairs per round, one thread per row: 8 s and 17 s each."""
    g = wrap_graph(name, tmp_path)
    assert_wrap_properties(g, name)
    one = oracle.simrank_naive(g._offs, g._nbrs, 0.6, 1, nthreads=8)
    assert one[0, 1] != 0 and ulps(one, reference(g._offs, g._nbrs, 0.6, 1)) <= 2
    two = oracle.simrank_naive(g._offs, g._nbrs, 0.6, 2, nthreads=8)
    np.testing.assert_allclose(two.astype(LD), reference(g._offs, g._nbrs, 0.6, 2), rtol=RTOL, atol=ATOL)


@pytest.mark.slow
def test_oracle_round_rows_wraps_like_java(gw, oracle, tmp_path):
    """or_simrank_round_rows (bench.py's CPU baseline) divides by the same Java
    int product: row 0 of neg_loops, one sweep from the identity, where (0, 1)
    is -0.2999625 over -2147479015.  Integer numerators: 2 ulp.  2.1e9 pairs."""
    g = wrap_graph("neg_loops", tmp_path)
    assert_wrap_properties(g, "neg_loops")
    rows, pairs = oracle.simrank_round_rows(g._offs, g._nbrs, 0.6, np.eye(3), 0, 1, nthreads=1)
    assert pairs == 46341 * 46341 + 46341 * 6
    ref = reference(g._offs, g._nbrs, 0.6, 1)
    assert rows[0, 1] < 0 and ulps(rows[0, 1:], ref[0, 1:]) <= 2


def test_oracle_drifts_on_long_rows(gw, oracle, tmp_path):
    """Why the oracle is not the reference for graph (a): its sequential fp64
    sums of up to 10^8 terms leave the long-double value by more than the
    tolerance (DESIGN.md section 4 records the figure)."""
    g = write_graph(tmp_path / "a.txt", long_row_lines(), LONG_M)
    assert_long_row_classes(g)
    ref = reference(g._offs, g._nbrs, 0.6, 3)
    orc = oracle.simrank_naive(g._offs, g._nbrs, 0.6, 3, nthreads=8).astype(LD)
    nz = ref != 0
    dev = float(np.max(np.abs(orc[nz] - ref[nz]) / np.abs(ref[nz])))
    print(f"oracle vs long double, graph (a), 3 rounds: max relative deviation {dev:.3e}")
    assert dev > 1e-12


# ---- GPU ---------------------------------------------------------------------------------------------------------
def _gpu(g, C, iters, hbm_row=0, window=0):
    from gwamd import topsim
    g._g.options(simrank_hbm_row=hbm_row, simrank_window=window)
    sr = topsim.SimRank(g, C_=C, step=iters)
    sr.compute()
    return sr.getResult()


def _check(sim, ref, g):
    np.testing.assert_allclose(sim.astype(LD), ref, rtol=RTOL, atol=ATOL)
    assert np.array_equal(sim, sim.T)
    assert np.all(np.diag(sim) == 0.0)
    iso = np.flatnonzero(np.diff(g._offs) == 0)
    assert np.all(sim[iso] == 0.0) and np.all(sim[:, iso] == 0.0)


class _Long:
    """Graph (a), loaded once per module, with its references computed once
    per (C, rounds) from g._offs / g._nbrs and handed out read-only."""

    def __init__(self, path):
        self.g = write_graph(path, long_row_lines(), LONG_M)
        assert_long_row_classes(self.g)
        self._refs = {}

    def ref(self, C, iters):
        if (C, iters) not in self._refs:
            r = reference(self.g._offs, self.g._nbrs, C, iters)
            r.setflags(write=False)
            self._refs[(C, iters)] = r
        return self._refs[(C, iters)]


@pytest.fixture(scope="module")
def long_graph(tmp_path_factory):
    return _Long(tmp_path_factory.mktemp("sr") / "a.txt")


@pytest.mark.gpu
@pytest.mark.parametrize("iters,C", [(1, 0.6), (3, 0.6), (7, 0.8)])
def test_row_length_edges(gw, long_graph, iters, C):
    """(a) rows of 15..17, 255..257, 511..513, 1008..1041, 2047..2049 entries
    and one far above 4096: lane sum, every scan step, both broadcasts and one
    to many chunk carries; some wave runs several trips of the pos loop."""
    g, ref = long_graph.g, long_graph.ref(C, iters)
    lds = _gpu(g, C, iters)
    _check(lds, ref, g)
    hbm = _gpu(g, C, iters, hbm_row=1)
    _check(hbm, ref, g)
    assert np.array_equal(lds, hbm)


def _align_graph(tmp_path, s, k, tail):
    """(b) id 0: a row of padded length 16 s; id 1: the hub, degree 1024 + 16 k;
    ids 2..5 its leaves (tied among themselves so that nothing is bipartite);
    ids 6, 7: a pair tied `tail` times, which moves the slice boundaries."""
    dp, D = 16 * s - 5, 1024 + 16 * k
    rest = D - (dp - 3)
    assert dp >= 4 and rest >= 8
    parts = [rest // 2, rest // 4, rest // 8]
    parts.append(rest - sum(parts))
    spec = [((0, 1), dp - 3), ((0, 2), 3), ((2, 3), 7), ((4, 5), 5), ((2, 6), 2), ((6, 7), tail)]
    spec += [((1, 2 + i), c) for i, c in enumerate(parts)]
    rng = np.random.default_rng(s * 1000 + k)
    lines = [e for e, c in spec for _ in range(c)]
    g = write_graph(tmp_path / f"b_{s}_{k}_{tail}.txt", [lines[i] for i in rng.permutation(len(lines))], 8)
    deg = np.diff(g._offs)
    assert deg[1] == D and (deg[0] + 15) // 16 * 16 == 16 * s
    return g


def _hub_place(g, row=1):
    """Where the kernel meets `row` in a single-window pass: (wave, chunk of
    that wave's slice, lane, nominal slice boundaries strictly inside the row)."""
    poff = padded_offsets(g)
    m = len(poff) - 1
    tot = int(poff[m])
    sl = wave_slices(poff, 0, m)
    wave = [w for w, (ra, rb) in enumerate(sl) if ra <= row < rb]
    assert len(wave) == 1                                   # the slices partition the rows
    ra = sl[wave[0]][0]
    rel = int(poff[row] - poff[ra]) // SR_K
    inside = [w for w in range(1, SR_WAVES) if poff[row] < tot * w // SR_WAVES < poff[row + 1]]
    return wave[0], rel // 64, rel % 64, inside


# (s, k, tail) -> (wave, chunk of its slice, lane, a nominal slice boundary falls inside the hub)
ALIGN_CASES = {
    (1, 0, 1): (0, 0, 1, True),          # lane 1; the hub swallows the shares of waves 1..7, which get empty slices
    (2, 5, 24000): (0, 0, 2, False),     # lane 2, the hub wholly inside wave 0's share
    (63, 1, 8000): (0, 0, 63, True),     # last lane of a chunk: the whole hub but 16 entries rides on the carry
    (64, 3, 8000): (0, 1, 0, True),      # lane 0 of wave 0's second chunk: the row before it closes from the carry
    (64, 0, 1): (7, 0, 0, True),         # first row of a later wave's slice, exactly one chunk long
    (65, 5, 16000): (0, 1, 1, True),     # lane 1 of the second chunk
}


@pytest.mark.gpu
@pytest.mark.parametrize("s,k,tail", sorted(ALIGN_CASES))
def test_row_start_alignment(gw, tmp_path, s, k, tail):
    """(b) a hub of 1024 + 16 k entries that starts at a chosen lane of a chunk:
    the row before it has padded length 16 s.  Which wave meets the hub, and at
    which lane, follows from the slice boundaries e_lo + tot * wave / 16 of the
    kernel (tot = the window's padded entries), which move with every degree in
    the graph: _hub_place restates them and the case asserts what it expects."""
    g = _align_graph(tmp_path, s, k, tail)
    wave, chunk, lane, inside = _hub_place(g)
    assert (wave, chunk, lane, bool(inside)) == ALIGN_CASES[(s, k, tail)]
    assert lane == s % 64 or wave > 0
    for iters in (1, 3):
        ref = reference(g._offs, g._nbrs, 0.6, iters)
        assert np.count_nonzero(ref[1]) >= 5            # the hub's row total matters
        sim = _gpu(g, 0.6, iters)
        _check(sim, ref, g)
        assert np.array_equal(sim, _gpu(g, 0.6, iters, hbm_row=1))


# window -> passes of the window loop in pass 1 (pass 2 of row i starts at i + 1 and runs fewer)
WINDOWS = {1: 48, 2: 24, 3: 16, 7: 7, 16: 3, LONG_M - 1: 2, LONG_M: 1, LONG_M + 5: 1}


@pytest.mark.gpu
@pytest.mark.parametrize("hbm_row", [0, 1])
def test_windows(gw, long_graph, hbm_row):
    """(c) simrank_window on graph (a): windows that start at i + 1 in pass 2,
    windows with fewer rows than waves (empty slices), the hub alone in a
    window; m and m + 5 (clamped) are the automatic window bit for bit."""
    g, ref = long_graph.g, long_graph.ref(0.6, 3)
    m = int(np.count_nonzero(np.diff(g._offs)))
    poff = padded_offsets(g)
    hub = int(np.argmax(np.diff(g._offs)))
    auto = _gpu(g, 0.6, 3, hbm_row=hbm_row)
    _check(auto, ref, g)
    for win, count in WINDOWS.items():
        assert -(-m // min(win, m)) == count
        if win < SR_WAVES:
            assert any(ra == rb for ra, rb in wave_slices(poff, hub // win * win, min(m, hub // win * win + win)))
        sim = _gpu(g, 0.6, 3, hbm_row=hbm_row, window=win)
        _check(sim, ref, g)
        if win >= m:
            assert np.array_equal(sim, auto)
    assert g._g.options(simrank_window=0)["simrank_window"] == 0


def _few_rows(name, tmp_path):
    if name == "loop":
        return write_graph(tmp_path / "m1.txt", [(0, 0)], 1), 1
    if name == "pair":
        return write_graph(tmp_path / "m2.txt", [(0, 1)] * 3 + [(1, 1)], 2), 2
    if name == "star":
        return write_graph(tmp_path / "m3.txt", [(1, 0), (0, 2)] * 2500 + [(1, 2)], 3), 3
    rng = np.random.default_rng(17)
    lines = [(int(rng.integers(v)), v) for v in range(1, 17)] + [tuple(int(x) for x in rng.integers(17, size=2))
                                                                  for _ in range(40)]
    return write_graph(tmp_path / "m17.txt", lines, 17), 17


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["loop", "pair", "star", "m17"])
def test_few_rows(gw, tmp_path, name):
    """(d) fewer rows than waves (m = 1, 2, 3) and one more than waves (17):
    most slices are empty; the star's centre (degree 5000) is one wave's whole
    window.  Rounds 0, 1, 2."""
    g, m = _few_rows(name, tmp_path)
    deg = np.diff(g._offs)
    assert np.count_nonzero(deg) == m == len(deg)
    if name == "star":
        assert deg[0] == 5000
        assert sum(ra == rb for ra, rb in wave_slices(padded_offsets(g), 0, m)) >= SR_WAVES - 3
    for iters in (0, 1, 2):
        ref = reference(g._offs, g._nbrs, 0.6, iters)
        sim = _gpu(g, 0.6, iters)
        _check(sim, ref, g)
        assert np.array_equal(sim, _gpu(g, 0.6, iters, hbm_row=1))
        if iters == 0:
            assert np.all(sim == 0)


@pytest.mark.gpu
def test_isolated_ids_interleaved(gw, long_graph, tmp_path):
    """(e) graph (a) relabelled so that id 0, every fifth id and id V - 1 are
    unused: the compact problem is the same, so the scores are graph (a)'s bit
    for bit, scattered through the rank map by k_sr_expand."""
    V = 62
    ids = np.array([i for i in range(V - 1) if i % 5], np.int64)
    assert len(ids) == LONG_M
    g = write_graph(tmp_path / "e.txt", [(int(ids[u]), int(ids[v])) for u, v in long_row_lines()], V)
    deg = np.diff(g._offs)
    iso = np.flatnonzero(deg == 0)
    assert set(iso) == set(range(0, V, 5)) | {V - 1} and np.array_equal(deg[ids], np.diff(long_graph.g._offs))
    assert_long_row_classes(g, ids)
    for hbm_row in (0, 1):
        base = _gpu(long_graph.g, 0.6, 3, hbm_row=hbm_row)
        sim = _gpu(g, 0.6, 3, hbm_row=hbm_row)
        _check(sim, reference(g._offs, g._nbrs, 0.6, 3), g)
        exp = np.zeros((V, V))
        exp[np.ix_(ids, ids)] = base
        assert np.array_equal(sim, exp)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(WRAP_SPECS) + sorted(HEAVY_SPECS))
def test_java_int_wrap(gw, tmp_path, name):
    """(f) deg(v) * deg(w) is a Java int: products past 2^31 divide by a
    negative number, products past 2^32 by a small one.  1 round: exact integer
    numerators, 2 ulp.  2 rounds (mixed signs on neg_loops): rtol 1e-12
    while the reference's sum|terms| / |sum terms| < 100 (asserted).  Rows of
    46 000+ entries: 45 and more carries in a row in one wave."""
    g = wrap_graph(name, tmp_path)
    assert_wrap_properties(g, name)
    for hbm_row in (0, 1):
        one = _gpu(g, 0.6, 1, hbm_row=hbm_row)
        ref1 = reference(g._offs, g._nbrs, 0.6, 1)
        _check(one, ref1, g)
        assert ulps(one, ref1) <= 2
        _check(_gpu(g, 0.6, 2, hbm_row=hbm_row), reference(g._offs, g._nbrs, 0.6, 2), g)
