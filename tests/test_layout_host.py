"""CPU: the spring-layout law (csrc/gw_layout_law.h) through the host evaluation (device = -1).

The numeric reference is `fr`, a restatement of networkx 3.4.2's dense _fruchterman_reingold in numpy.  The one-step
tests run it in np.longdouble and bound the difference by the conditioning of the sums, which the restatement computes;
the whole runs are compared with networkx itself and with tests/golden/layout_nx.npz (its own output, written by
tools/gen_layout_golden.py), only for graphs of at most 40 vertices: the dynamics amplify rounding differences, and
above a few dozen vertices two correct implementations that sum in different orders part ways."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import DATA, PKG, load_golden

U = 2.0 ** -53
CHUNK, STRANDS, BLOCK = 1024, 4, 64


def L():
    from gwamd import _lib as C
    from gwamd import layout
    C.lib()
    return layout


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


# ---- the restatement ---------------------------------------------------------------------------------------------
def fr(A, k, pos, fixed=None, iterations=50, threshold=1e-4, dtype=np.float64, order=None):
    """networkx's dense loop.  order: None = its einsum; 'asc' / 'desc' = the sum over columns as an explicit loop in
    that order.  Returns (positions, iterations done)."""
    A = np.asarray(A, dtype)
    pos = np.array(pos, dtype)
    n = len(pos)
    k = dtype(np.sqrt(1.0 / n) if k is None else k)
    t = max(max(pos.T[0]) - min(pos.T[0]), max(pos.T[1]) - min(pos.T[1])) * dtype(0.1)
    dt = t / dtype(iterations + 1)
    done = 0
    for _ in range(iterations):
        delta = pos[:, np.newaxis, :] - pos[np.newaxis, :, :]
        distance = np.sqrt((delta ** 2).sum(axis=-1))
        np.clip(distance, dtype(0.01), None, out=distance)
        coef = k * k / distance ** 2 - A * distance / k
        if order is None:
            displacement = np.einsum("ijk,ij->ik", delta, coef)
        else:
            displacement = np.zeros_like(pos)
            for j in (range(n) if order == "asc" else range(n - 1, -1, -1)):
                displacement += delta[:, j, :] * coef[:, j, None]
        length = np.sqrt((displacement ** 2).sum(axis=-1))
        length = np.where(length < 0.01, dtype(0.1), length)
        delta_pos = displacement * (t / length)[:, None]
        if fixed is not None:
            delta_pos[fixed] = 0.0
        pos += delta_pos
        t -= dt
        done += 1
        if np.sqrt((delta_pos ** 2).sum()) / n < threshold:
            break
    return pos, done


def one_step(A, k, pos, t):
    """(pos_out, disp, kappa) of one iteration at temperature t in np.longdouble.  kappa [n] = (sum_j |repulsion
    term_j| + sum_j |attraction term_j|) / |disp| in Euclidean norms: the conditioning of disp = R - T as the law forms
    it, R and T apart."""
    ld = np.longdouble
    A = np.asarray(A, ld)
    pos = np.asarray(pos, ld)
    k = ld(k)
    delta = pos[:, np.newaxis, :] - pos[np.newaxis, :, :]
    distance = np.sqrt((delta ** 2).sum(axis=-1))
    np.clip(distance, ld(0.01), None, out=distance)
    rep, att = k * k / distance ** 2, A * distance / k
    disp = (delta * (rep - att)[:, :, None]).sum(axis=1)
    length = np.sqrt((disp ** 2).sum(axis=-1))
    mass = np.sqrt((delta ** 2).sum(-1)) * (np.abs(rep) + np.abs(att))
    kappa = mass.sum(axis=1) / length
    length = np.where(length < 0.01, ld(0.1), length)
    return pos + disp * (ld(t) / length)[:, None], disp, kappa


# ---- graphs ------------------------------------------------------------------------------------------------------
def csr_of(n, r, c, v):
    order = np.argsort(r, kind="stable")
    off = np.zeros(n + 1, np.int64)
    np.add.at(off, np.asarray(r, np.int64) + 1, 1)
    return np.cumsum(off), np.asarray(c, np.int32)[order], np.asarray(v, np.float64)[order]


def dense_of(n, g):
    """What nx.to_numpy_array would hold: repeated entries added, the diagonal as listed (the law drops it; so does the
    force, whose delta is 0 there)."""
    off, nb, v = g
    A = np.zeros((n, n))
    for i in range(n):
        for e in range(off[i], off[i + 1]):
            A[i, nb[e]] += v[e]
    return A


def karate_edges():
    e = np.loadtxt(os.path.join(DATA, "karate.edgelist"), dtype=np.int64)
    return e - e.min()


def sym(n, edges, w=None):
    e = np.asarray(edges, np.int64)
    w = np.ones(len(e)) if w is None else np.asarray(w, np.float64)
    return csr_of(n, np.concatenate([e[:, 0], e[:, 1]]), np.concatenate([e[:, 1], e[:, 0]]), np.concatenate([w, w]))


def gnm(n, m, seed, weighted=True, keep_isolated=0):
    """m random edges among the first n - keep_isolated vertices (the rest have no edge), weights in [0.5, 1.5)."""
    rng = np.random.RandomState(seed)
    e = rng.randint(0, n - keep_isolated, (m, 2))
    e = e[e[:, 0] != e[:, 1]]
    return sym(n, e, 0.5 + rng.rand(len(e)) if weighted else None)


def graphs():
    rng = np.random.RandomState(5)
    out = {"karate": (34, sym(34, karate_edges())),
           "path40": (40, sym(40, np.stack([np.arange(39), np.arange(1, 40)], 1))),
           "g120_200_isolated": (120, gnm(120, 200, 2, keep_isolated=7))}
    r, c = rng.randint(0, 50, 150), rng.randint(0, 50, 150)
    keep = r != c
    out["directed"] = (50, csr_of(50, r[keep], c[keep], 0.5 + rng.rand(keep.sum())))
    e = rng.randint(0, 36, (60, 2))
    e = e[e[:, 0] != e[:, 1]]
    rep = np.concatenate([e, e[:20], e[:5]])  # 20 edges listed twice, 5 of them three times
    out["repeated"] = (36, sym(36, rep, 0.5 + rng.rand(len(rep))))
    off, nb, v = gnm(36, 70, 9)
    rows = np.repeat(np.arange(36), np.diff(off))
    out["diagonal"] = (36, csr_of(36, np.concatenate([rows, [3, 3, 17]]), np.concatenate([nb, [3, 3, 17]]),
                                   np.concatenate([v, [2.5, 1.0, 4.0]])))
    off, nb, v = gnm(36, 70, 10)
    v = v.copy()
    v[::7] = -v[::7]
    out["negative"] = (36, (off, nb, v))
    return out


GRAPHS = graphs()


def handle(n, g, dim=2, device=-1):
    m = L().SpringLayout(n, dim=dim, device=device)
    m.set_csr(*g)
    return m


# ---- 1. one step -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_one_step_against_the_restatement(name, dim):
    """|pos_out - reference| <= 8 n 2^-53 kappa t per vertex.  Why: disp_i is a sum of at most 2n terms of which each
    carries a few roundings, so its error is at most about n u M_i (M_i = sum of the terms' norms, first order in
    u = 2^-53); the step has length exactly t along disp_i, so that error moves pos_out by at most t n u M_i / |disp_i|
    = t n u kappa_i, once through the direction and once more through the length.  8 covers both and the terms' own
    roundings.  kappa is formed on R and T apart, as the law adds them; kappa <= 1e4 keeps the bound far below t."""
    n, g = GRAPHS[name]
    pos = np.random.RandomState(0).rand(n, dim)
    k, t = np.sqrt(1.0 / n), 0.1
    m = handle(n, g, dim)
    disp, out = m.step(pos, k=0.0, t=t)
    m.free()
    ref, rdisp, kappa = one_step(dense_of(n, g), k, pos, t)
    print(f"{name} dim {dim}: kappa max {float(kappa.max()):.1f}, "
          f"max |pos diff| {float(np.abs(out - ref).max()):.2e}, bound min {8 * n * U * float(kappa.min()) * t:.2e}")
    assert kappa.max() <= 1e4
    bound = (8 * n * U * kappa * t).astype(np.float64)
    assert (np.abs(out - ref).max(axis=1) <= bound).all()
    length = np.sqrt((rdisp ** 2).sum(-1))
    assert (np.abs(disp - rdisp).max(axis=1) <= (8 * n * U * kappa * length).astype(np.float64)).all()


def law_in_numpy(n, g, pos, k, t):
    """The law's own order of summation, vectorised over rows: (disp, pos_out) to compare bit for bit."""
    off, nb, v = g
    dim = pos.shape[1]
    kk = k * k
    R = np.zeros_like(pos)
    for c0 in range(0, n, CHUNK):
        acc = np.zeros((STRANDS,) + pos.shape)
        for j in range(c0, min(c0 + CHUNK, n)):
            d = pos - pos[j]
            d2 = d[:, 0] * d[:, 0]
            for c in range(1, dim):
                d2 = d2 + d[:, c] * d[:, c]
            f = kk / np.where(d2 < 1e-4, 1e-4, d2)
            acc[(j - c0) % STRANDS] += d * f[:, None]
        s = np.zeros_like(pos)
        for a in range(STRANDS):
            s = s + acc[a]
        R = R + s
    T = np.zeros_like(pos)
    for i in range(n):
        for e in range(off[i], off[i + 1]):
            if nb[e] == i:
                continue
            d = pos[i] - pos[nb[e]]
            d2 = d[0] * d[0]
            for c in range(1, dim):
                d2 = d2 + d[c] * d[c]
            dist = np.sqrt(d2)
            T[i] = T[i] + d * ((v[e] * (0.01 if dist < 0.01 else dist)) / k)
    disp = R - T
    l2 = disp[:, 0] * disp[:, 0]
    for c in range(1, dim):
        l2 = l2 + disp[:, c] * disp[:, c]
    length = np.sqrt(l2)
    length = np.where(length < 0.01, 0.1, length)
    return disp, pos + disp * (t / length)[:, None]


@pytest.mark.parametrize("dim", [2, 3])
def test_host_sums_in_the_laws_order(dim):
    """Past one chunk and not a multiple of the strands: the C++ host evaluation and the same order in numpy."""
    n = CHUNK + 71
    g = gnm(n, 3 * n, 4)
    pos = np.random.RandomState(1).rand(n, dim)
    m = handle(n, g, dim)
    disp, out = m.step(pos, k=0.05, t=0.07)
    m.free()
    rdisp, rout = law_in_numpy(n, g, pos, 0.05, 0.07)
    assert np.array_equal(bits(disp), bits(rdisp)) and np.array_equal(bits(out), bits(rout))


def test_tiles_on_the_host():
    m = L().SpringLayout(5, device=-1)
    assert m.tiles() == {"rows": 0, "chunk": CHUNK, "strands": STRANDS, "block": BLOCK}
    m.free()


# ---- 2. the branches ---------------------------------------------------------------------------------------------
def branch_inputs():
    """name -> (n, csr, pos, fixed): shared with the GPU tests."""
    none3 = (np.zeros(4, np.int64), np.zeros(0, np.int32), np.zeros(0))
    rng = np.random.RandomState(3)
    coincident = rng.rand(6, 2)
    coincident[4] = coincident[1]          # d2 = 0 < 1e-4: the clip
    coincident[5] = coincident[2] + 1e-3   # 0 < d2 < 1e-4 as well
    return {"coincident": (6, sym(6, [(0, 1), (1, 4), (2, 5), (3, 0)]), coincident, None),
            "collinear": (3, none3, np.array([[0.25, 0.5], [0.5, 0.5], [0.75, 0.5]]), None),
            "fixed": (34, sym(34, karate_edges()), np.random.RandomState(2).rand(34, 2), [0, 33, 7])}


def test_coincident_points_take_the_clip():
    n, g, pos, _ = branch_inputs()["coincident"]
    m = handle(n, g)
    disp, out = m.step(pos, k=0.0, t=0.1)
    m.free()
    ref, rdisp, kappa = one_step(dense_of(n, g), np.sqrt(1.0 / n), pos, 0.1)
    assert np.isfinite(disp).all() and np.isfinite(out).all()
    assert (np.abs(out - ref).max(axis=1) <= (8 * n * U * kappa * 0.1).astype(np.float64)).all()
    # the coincident pair feels no force from each other: only the clip keeps 0 / 0 out
    assert np.abs(out[1] - out[4]).max() > 0  # their other edges differ, so they part


def test_the_middle_of_three_collinear_points_stays():
    n, g, pos, _ = branch_inputs()["collinear"]
    m = handle(n, g)
    disp, out = m.step(pos, k=0.0, t=0.1)
    assert np.array_equal(bits(disp[1]), bits([0.0, 0.0])) and np.array_equal(bits(out[1]), bits(pos[1]))
    assert out[0, 0] < pos[0, 0] and out[2, 0] > pos[2, 0] and out[0, 1] == 0.5 and out[2, 1] == 0.5
    assert m.run(pos, iterations=5) == 5 and np.array_equal(bits(m.positions_numpy()[1]), bits(pos[1]))
    m.free()


def test_a_fixed_vertex_does_not_move():
    n, g, pos, fixed = branch_inputs()["fixed"]
    m = handle(n, g)
    m.set_fixed(fixed)
    disp, out = m.step(pos, k=0.0, t=0.1)
    assert np.array_equal(bits(out[fixed]), bits(pos[fixed])) and np.abs(disp[fixed]).min() > 0
    m.run(pos)
    end = m.positions_numpy()
    assert np.array_equal(bits(end[fixed]), bits(pos[fixed]))
    free = np.setdiff1d(np.arange(n), fixed)
    assert (np.abs(end[free] - pos[free]).max(axis=1) > 0).all()
    ref, _ = fr(dense_of(n, g), None, pos, fixed=fixed)
    assert np.abs(end - ref).max() < 1e-6
    m.set_fixed(None)
    m.run(pos)
    assert np.abs(m.positions_numpy()[fixed] - pos[fixed]).min() > 0
    m.free()


def stop_threshold(pos, after, iterations=50):
    """Every vertex of a graph in general position steps by exactly t, so the stop norm of iteration i (from 1) is
    t_i / sqrt(n) with t_i = t0 - (i - 1) dt: a threshold half a dt above t_after / sqrt(n) is first undercut by iteration
    `after`."""
    n = len(pos)
    t0 = 0.1 * max(np.ptp(pos[:, 0]), np.ptp(pos[:, 1]))
    dt = t0 / (iterations + 1)
    return (t0 - (after - 1.5) * dt) / np.sqrt(n)


@pytest.mark.parametrize("after", [1, 2])
def test_early_stop_counts_its_iterations(after):
    n, g = GRAPHS["karate"]
    pos = np.random.RandomState(0).rand(n, 2)
    m = handle(n, g)
    assert m.run(pos, threshold=stop_threshold(pos, after)) == after
    ref, done = fr(dense_of(n, g), None, pos, threshold=stop_threshold(pos, after))
    assert done == after and np.abs(m.positions_numpy() - ref).max() < 1e-12
    m.free()


def test_zero_iterations_leave_the_positions():
    n, g = GRAPHS["karate"]
    pos = np.random.RandomState(0).rand(n, 2)
    m = handle(n, g)
    assert m.run(pos, iterations=0) == 0 and np.array_equal(bits(m.positions_numpy()), bits(pos))
    m.free()


def test_set_rows_and_set_csr_of_one_matrix_agree():
    n, (off, nb, v) = GRAPHS["g120_200_isolated"]
    topk = int(np.diff(off).max()) + 1
    ids = np.full((n, topk), -1, np.int32)
    val = np.full((n, topk), np.nan)  # never read behind the -1
    for i in range(n):
        ids[i, :off[i + 1] - off[i]] = nb[off[i]:off[i + 1]]
        val[i, :off[i + 1] - off[i]] = v[off[i]:off[i + 1]]
    pos = np.random.RandomState(0).rand(n, 2)
    a, b = L().SpringLayout(n, device=-1), L().SpringLayout(n, device=-1)
    a.set_csr(off, nb, v)
    b.set_rows(ids, val)
    assert a.run(pos) == b.run(pos) and np.array_equal(bits(a.positions_numpy()), bits(b.positions_numpy()))
    a.free()
    b.free()


def test_rescale_is_networkx_rescale_layout():
    rng = np.random.RandomState(4)
    for dim in (2, 3):
        pos = rng.rand(200, dim) * 3 - 1
        m = L().SpringLayout(200, dim=dim, device=-1)
        c = np.arange(dim) + 2.0
        m.rescale(0.5, c, pos=pos)
        ref = pos - pos.mean(axis=0)
        ref = ref * (0.5 / np.abs(ref).max()) + c
        assert np.abs(m.positions_numpy() - ref).max() < 1e-14
        m.rescale(2.0, None, pos=np.zeros((200, dim)))  # max |pos| = 0: only the shift
        assert not m.positions_numpy().any()
        m.free()


# ---- 3. whole runs against networkx ------------------------------------------------------------------------------
CASES = ["karate_s0", "karate_s7", "path40_s1"]


def golden_graph(gold, name):
    from gwamd.graph import GWGraph
    e = gold[name + "_edges"]
    return GWGraph.from_edges(e[:, 0], e[:, 1], semantics="nx")


@pytest.mark.parametrize("name", CASES)
def test_whole_runs_against_the_golden(name):
    """atol 1e-6 against networkx's own output.  The yardstick is the reference's own reassociation noise: the
    restatement summed over ascending and over descending columns, asserted below 1e-8 (measured on these three
    cases: <= 5.7e-11); the orders of margin are there because the growth of a perturbation was sampled, not
    bounded."""
    gold = load_golden("layout_nx.npz")
    G = golden_graph(gold, name)
    seed = int(gold[name + "_seed"])
    nodes = [int(u) for u in gold[name + "_nodes"]]
    raw = L().spring_layout(G, seed=seed, scale=None, device=-1)
    scaled = L().spring_layout(G, seed=seed, scale=1, center=(2, 3), device=-1)
    assert list(raw) == nodes and list(scaled) == nodes
    assert np.abs(np.stack([raw[u] for u in nodes]) - gold[name + "_raw"]).max() < 1e-6
    assert np.abs(np.stack([scaled[u] for u in nodes]) - gold[name + "_scaled"]).max() < 1e-6
    nodes_, off, nb, v = L().graph_csr(G)
    A = dense_of(len(nodes), (off, nb, v))
    pos0 = np.random.RandomState(seed).rand(len(nodes), 2)
    asc, _ = fr(A, None, pos0, order="asc")
    desc, _ = fr(A, None, pos0, order="desc")
    noise = np.abs(asc - desc).max()
    print(f"{name}: reassociation noise {noise:.2e}, ours - networkx "
          f"{np.abs(np.stack([raw[u] for u in nodes]) - gold[name + '_raw']).max():.2e}")
    assert noise < 1e-8
    assert np.abs(asc - gold[name + "_raw"]).max() < 1e-6  # the restatement is networkx's loop


@pytest.mark.parametrize("name", CASES)
def test_whole_runs_against_networkx(name):
    nx = pytest.importorskip("networkx")
    gold = load_golden("layout_nx.npz")
    G = nx.Graph()
    G.add_edges_from(gold[name + "_edges"].tolist())
    seed = int(gold[name + "_seed"])
    for kw in (dict(scale=None), dict(scale=1, center=(2, 3))):
        ref = nx.spring_layout(G, seed=seed, **kw)
        got = L().spring_layout(G, seed=seed, device=-1, **kw)
        assert list(got) == list(ref)
        assert max(np.abs(got[u] - ref[u]).max() for u in G) < 1e-6
    assert np.abs(np.stack([ref[u] for u in G]) - gold[name + "_scaled"]).max() < 1e-6  # the golden is networkx's


# ---- 4. the Python surface ---------------------------------------------------------------------------------------
def test_return_type_and_vertex_order():
    nx = pytest.importorskip("networkx")
    G = nx.Graph()
    G.add_edges_from([("c", "a"), ("a", "b"), ("z", "c")])
    G.add_node("lonely")
    got = L().spring_layout(G, seed=1, device=-1)
    assert isinstance(got, dict) and list(got) == ["c", "a", "b", "z", "lonely"]
    assert all(isinstance(p, np.ndarray) and p.shape == (2,) and p.dtype == np.float64 for p in got.values())
    assert L().spring_layout(G, seed=1, dim=3, device=-1)["a"].shape == (3,)
    assert L().spring_layout(nx.Graph(), device=-1) == {}
    one = L().spring_layout(nx.path_graph(1), center=(4, 5), device=-1)
    assert list(one) == [0] and np.array_equal(one[0], [4, 5])
    ref = nx.spring_layout(G, seed=1)
    assert max(np.abs(got[u] - ref[u]).max() for u in G) < 1e-9  # 5 vertices: no room for amplification
    listed = L().spring_layout(["p", "q", "r"], seed=2, device=-1)  # not a graph: nodes without edges
    ref = nx.spring_layout(["p", "q", "r"], seed=2)
    assert list(listed) == ["p", "q", "r"] and max(np.abs(listed[u] - ref[u]).max() for u in ref) < 1e-9


def test_pos_and_fixed_follow_the_dom_size_rule():
    """The warm start: missing vertices are drawn in [0, dom_size) + center, and with fixed vertices k becomes
    dom_size / sqrt(n).  The check that pins the rule is the one after a single iteration, where nothing is amplified
    yet: 1e-12.  The 50-iteration comparison only catches gross errors: its bound is the whole-run yardstick applied
    to this start, 1000 times the restatement's own reassociation noise (ascending against descending columns) from
    the same start, k and fixed set, never below 1e-6; from a start 3 units wide that noise reaches 4e-5 (printed), so
    the bound is as wide as 4e-2 on coordinates of order 3."""
    nx = pytest.importorskip("networkx")
    G = nx.read_edgelist(os.path.join(DATA, "karate.edgelist"), nodetype=int)
    nodes = list(G)
    A = nx.to_numpy_array(G)
    p0 = {1: (0.0, 0.0), 5: (3.0, 1.0), 34: (1.0, 2.5)}
    for kw in (dict(pos=p0, fixed=[1, 34]), dict(pos=p0), dict(pos=p0, fixed=[5], k=0.3),
               dict(pos=p0, center=(1, 1), fixed=[1])):
        ref = nx.spring_layout(G, seed=3, iterations=1, **kw)
        got = L().spring_layout(G, seed=3, iterations=1, device=-1, **kw)
        assert max(np.abs(got[u] - ref[u]).max() for u in G) < 1e-12
        # networkx's start, restated, for the noise of its own loop
        start = np.random.RandomState(3).rand(len(nodes), 2) * 3.0 + np.asarray(kw.get("center", (0, 0)))
        for u, p in p0.items():
            start[nodes.index(u)] = p
        fixed = [nodes.index(u) for u in kw["fixed"]] if "fixed" in kw else None
        k = kw.get("k", 3.0 / np.sqrt(len(nodes)) if fixed else None)
        asc, _ = fr(A, k, start, fixed=fixed, order="asc")
        desc, _ = fr(A, k, start, fixed=fixed, order="desc")
        noise = np.abs(asc - desc).max()
        ref = nx.spring_layout(G, seed=3, scale=None, **kw)
        got = L().spring_layout(G, seed=3, scale=None, device=-1, **kw)
        diff = max(np.abs(got[u] - ref[u]).max() for u in G)
        print(sorted(kw), f"noise {noise:.2e}, ours - networkx {diff:.2e}")
        assert np.abs(asc - np.stack([ref[u] for u in G])).max() <= max(1e-6, 1e3 * noise)  # the start is networkx's
        assert diff <= max(1e-6, 1e3 * noise)
        for u in kw.get("fixed", []):
            assert np.array_equal(got[u], np.asarray(p0[u], np.float64))


def test_error_cases():
    from gwamd import _lib as C
    lay = L()
    with pytest.raises(ValueError):
        lay.SpringLayout(5, dim=4, device=-1)
    with pytest.raises(ValueError):
        lay.SpringLayout(5, dim=1, device=-1)
    with pytest.raises(ValueError):
        lay.SpringLayout(0, device=-1)
    m = lay.SpringLayout(4, device=-1)
    pos = np.random.RandomState(0).rand(4, 2)
    with pytest.raises(C.StateError):
        m.run(pos)
    with pytest.raises(C.StateError):
        m.step(pos)
    off = np.array([0, 1, 2, 2, 2], np.int64)
    with pytest.raises(IndexError):
        m.set_csr(off, np.array([1, 4], np.int32))
    with pytest.raises(IndexError):
        m.set_csr(off, np.array([1, -2], np.int32))
    with pytest.raises(C.StateError):  # a refused matrix leaves none behind
        m.run(pos)
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError):
            m.set_csr(off, np.array([1, 0], np.int32), np.array([1.0, bad]))
    with pytest.raises(IndexError):
        m.set_rows(np.array([[1], [0], [7], [-1]], np.int32), np.ones((4, 1)))
    m.set_csr(off, np.array([1, 0], np.int32))
    for kw in (dict(k=-1.0), dict(k=np.nan), dict(threshold=np.nan), dict(iterations=-1)):
        with pytest.raises(ValueError):
            m.run(pos, **kw)
    with pytest.raises(IndexError):
        m.set_fixed([4])
    with pytest.raises(IndexError):
        m.set_fixed([-1])
    with pytest.raises(ValueError):
        m.run(np.zeros((4, 3)))
    assert m.run(pos) == 50  # and the handle still works
    m.free()
    nx = pytest.importorskip("networkx")
    G = nx.path_graph(4)
    with pytest.raises(ValueError):
        lay.spring_layout(G, fixed=[0], device=-1)
    with pytest.raises(ValueError):
        lay.spring_layout(G, pos={1: (0, 0)}, fixed=[0], device=-1)
    with pytest.raises(ValueError):
        lay.spring_layout(G, center=(1, 2, 3), device=-1)


def test_a_handle_and_the_networkx_graph_of_one_edge_list_give_the_same_bits():
    nx = pytest.importorskip("networkx")
    from gwamd.graph import GWGraph
    path = os.path.join(DATA, "karate.edgelist")
    H = GWGraph.from_edgelist(path, " ", "nx")
    G = nx.read_edgelist(path, nodetype=int)
    a = L().spring_layout(H, seed=0, device=-1)
    b = L().spring_layout(G, seed=0, device=-1)
    assert list(a) == list(b) == list(G)
    assert all(np.array_equal(bits(a[u]), bits(b[u])) for u in G)


def fixture333():
    from gwamd import eigenmaps
    from gwamd.graph import GWGraph
    rows = eigenmaps.read_rows(os.path.join(DATA, "0_333_5038_simrank_navie_top10.txt.sim.txt"))
    return rows, GWGraph.from_edgelist(os.path.join(DATA, "0_333_5038.txt"), " ", "nx")


def expected_selection(vertex, topk=10):
    """The rule show has to follow on the 333-vertex fixture, written out with sets: the chosen vertices are `vertex`
    and the ids of its row's first topk entries whose value is not 0; an edge is kept when an end is chosen; a vertex is
    coloured 0.7 when it is `vertex`, 0.9 when chosen, 0.1 otherwise.  Line r of the .sim.txt is vertex r."""
    with open(os.path.join(DATA, "0_333_5038_simrank_navie_top10.txt.sim.txt")) as f:
        table = [[t.split(":") for t in line.split()[1:]] for line in f]
    chosen = {vertex} | {int(i) for i, v in table[vertex][:topk] if float(v) != 0}
    e = np.loadtxt(os.path.join(DATA, "0_333_5038.txt"), dtype=np.int64)
    kept = sorted({(int(min(u, v)), int(max(u, v))) for u, v in e if u in chosen or v in chosen})
    colours = [0.7 if j == vertex else 0.9 if j in chosen else 0.1 for j in range(len(table))]
    return colours, kept


@pytest.mark.parametrize("vertex", [0, 200])
def test_show_selects_the_vertex_its_neighbours_and_their_edges(vertex):
    rows, G = fixture333()
    pos, colours, kept = L().show(rows, G, vertex, topk=10, seed=0, device=-1, iterations=3)
    color, edges = expected_selection(vertex)
    assert colours == color and kept == edges
    assert colours.count(0.7) == 1 and 0 < colours.count(0.9) <= 10 and 0 < len(kept) < 5038
    assert len(pos) == G.n and all(np.isfinite(p).all() and p.shape == (2,) for p in pos.values())


def test_cli_writes_a_file_read_embedding_reads(tmp_path):
    from gwamd import classify
    edges = tmp_path / "karate0.txt"
    np.savetxt(edges, karate_edges(), fmt="%d")
    out = tmp_path / "karate.pos"
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "gwamd.layout", "--input", str(edges), "--output", str(out),
                        "--device", "-1", "--seed", "0", "--iterations", "20"], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    labels, X = classify.read_embedding(out)
    assert labels == [str(i) for i in range(34)] and X.shape == (34, 2)
    from gwamd.graph import GWGraph
    want = L().spring_layout(GWGraph.from_edgelist(str(edges), None, "nx"), seed=0, iterations=20, scale=1.0, device=-1)
    assert np.array_equal(X, np.stack([want[i] for i in range(34)]).astype(np.float32))
    # a warm start from the file just written, in 3 dimensions' worth of arguments
    out2 = tmp_path / "karate2.pos"
    r = subprocess.run([sys.executable, "-m", "gwamd.layout", "--input", str(edges), "--output", str(out2),
                        "--device", "-1", "--init", str(out), "--iterations", "5", "--k", "0.2"], env=env,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert classify.read_embedding(out2)[1].shape == (34, 2)


def test_cli_simrank_picture_weights_and_three_dimensions(tmp_path):
    """The argument plumbing of --simrank / --vertex / --topk, --dimensions 3 and --weighted: each file equals what
    the library call under it returns, as float32."""
    from gwamd import classify
    from gwamd.graph import GWGraph
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    sim = os.path.join(DATA, "0_333_5038_simrank_navie_top10.txt.sim.txt")
    edges = os.path.join(DATA, "0_333_5038.txt")
    out = tmp_path / "show.pos"
    r = subprocess.run([sys.executable, "-m", "gwamd.layout", "--input", edges, "--output", str(out), "--device", "-1",
                        "--simrank", sim, "--vertex", "200", "--topk", "4", "--dimensions", "3", "--iterations", "3",
                        "--seed", "2"], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    labels, X = classify.read_embedding(out)
    rows, G = fixture333()
    want, _, kept = L().show(rows, G, 200, topk=4, seed=2, device=-1, iterations=3, dim=3, scale=1.0)
    assert labels == [str(i) for i in range(G.n)] and X.shape == (G.n, 3)
    assert np.array_equal(X, np.stack([want[i] for i in range(G.n)]).astype(np.float32))
    assert f"{len(kept)} edges kept" in r.stdout and len(kept) == len(expected_selection(200, 4)[1])
    wfile = tmp_path / "karate_w.txt"
    e = karate_edges()
    w = 0.5 + np.random.RandomState(0).rand(len(e))
    with open(wfile, "w") as f:
        f.writelines(f"{u} {v} {x!r}\n" for (u, v), x in zip(e.tolist(), w.tolist()))
    o = tmp_path / "w.pos"
    r = subprocess.run([sys.executable, "-m", "gwamd.layout", "--input", str(wfile), "--output", str(o), "--device",
                        "-1", "--iterations", "10", "--weighted"], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = classify.read_embedding(o)[1]
    want = L().spring_layout(GWGraph.from_edgelist(str(wfile), None, "nx", False, True), seed=0, iterations=10,
                             scale=1.0, device=-1)
    assert np.array_equal(got, np.stack([want[i] for i in range(34)]).astype(np.float32))
    plain = L().spring_layout(GWGraph.from_edges(e[:, 0], e[:, 1], semantics="nx"), seed=0, iterations=10, scale=1.0,
                              device=-1)
    assert not np.array_equal(got, np.stack([plain[i] for i in range(34)]).astype(np.float32))  # the weights were read
