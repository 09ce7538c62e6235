"""k_walk_bitset's per-lane region loads (the membership word and the directory
pairs of a region select) are issued at one point per loop iteration, beside
the cooperative entry loads, and consumed after the exchange.  These tests run
the kernel where lanes of one wave sit in different phases in the same
iteration — fetching an entry, reading a membership word, guessing and
correcting a directory block (in the region and in the entry), fetching a
region block — and compare walks, lengths and both counters bitwise with
oracle.walks_bitset."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 7000
BIG = list(range(0, 6))        # degree 6,999 > 4,096: 14 directory blocks, kept in the region
MED = [6, 7, 8]                # degree 513..4,096: directory kept in the entry
CL = np.concatenate([np.arange(9, 209), np.arange(6800, 7000)])  # the dense cluster
SEED = 20


def _edgelist(path):
    """6 hubs adjacent to every vertex; three hubs of degree ~2,900 / ~1,400 /
    ~600; a 400-vertex cluster (pairs linked with probability 0.3) whose ids
    sit at both ends of the id range, so the common positions of a slot
    (cluster vertex -> big hub) fall into the first and the last directory
    blocks and the interpolated guess is corrected downwards for low ranks and
    upwards for high ones; a fringe of ~3 random links per vertex (list, dual
    and, towards the cluster, inline and Elias-Fano entries).  Vertices appear
    in id order, so without the start shuffle walk w starts at vertex w % N."""
    rng = np.random.default_rng(SEED)
    E = set()
    for h in BIG:
        E |= {(h, v) for v in range(h + 1, N)}
    E |= {(6, int(v)) for v in CL} | {(6, v) for v in range(209, 2700)}
    E |= {(7, int(v)) for v in CL} | {(7, int(v)) for v in rng.choice(np.arange(209, 6800), 1000, replace=False)}
    E |= {(8, int(v)) for v in CL[::4]} | {(8, int(v)) for v in rng.choice(np.arange(209, 6800), 500, replace=False)}
    m = rng.random((len(CL), len(CL))) < 0.3
    for a in range(len(CL)):
        for b in np.nonzero(m[a, a + 1:])[0]:
            E.add((int(CL[a]), int(CL[a + 1 + b])))
    for u in range(209, 6800):
        for v in rng.integers(209, 6800, 3):
            if int(v) != u:
                E.add((min(u, int(v)), max(u, int(v))))
    with open(path, "w") as f:
        for a, b in sorted(E):
            f.write(f"{a} {b}\n")


def _is_region(c, d):
    """bs_mode(c, d) == BS_REGION for d < 65536 (gw_internal.h: 352 payload bits)."""
    if c <= 22 or d <= 352:
        return False
    l = int(d // c).bit_length() - 1
    return c * l + c + ((d - 1) >> l) + 1 > 352


_REGION = {}


def _coverage(csr, walks, lens):
    """Steps (prev -> cur -> nxt) whose incoming entry (prev -> cur) is in
    region mode, split by where cur's directory lives, and those at a big hub
    whose successor is a common neighbour of prev."""
    off, nb = csr["offsets"], csr["nbrs"]
    deg = np.diff(off)
    n = len(deg)
    src = np.repeat(np.arange(n), deg)
    keys = np.sort(src.astype(np.int64) * n + nb)
    region = _REGION  # hub -> bool per vertex u: slot (u -> hub) is in region mode (one graph: computed once)
    for h in np.nonzero(deg > 512)[0] if not region else []:
        mask = np.zeros(n, bool)
        mask[nb[off[h]:off[h + 1]]] = True
        c = np.zeros(n, np.int64)
        nz = deg > 0
        c[nz] = np.add.reduceat(mask[nb].astype(np.int64), off[:-1][nz])
        region[int(h)] = np.array([mask[u] and _is_region(int(c[u]), int(deg[h])) for u in range(n)])
    in_region = in_entry = common_at_big = guess_high = guess_low = 0
    T = walks.shape[1]
    for s in range(1, T - 1):
        ok = lens > s + 1
        prev, cur, nxt = walks[ok, s - 1], walks[ok, s], walks[ok, s + 1]
        for h, reg in region.items():
            sel = (cur == h) & reg[prev]
            if deg[h] > 4096:
                in_region += int(sel.sum())
                k = nxt[sel].astype(np.int64) * n + prev[sel]
                com = np.isin(k, keys) & (nxt[sel] != prev[sel])
                common_at_big += int(com.sum())
                # the select's first guess of the directory block (the kernel's
                # interpolation j * ndir / c) against the block that holds the
                # successor: too high is corrected downwards, too low upwards
                row = nb[off[h]:off[h + 1]]
                ndir = (len(row) + 511) // 512
                for u, x in zip(prev[sel][com], nxt[sel][com]):
                    adj = np.zeros(n, bool)
                    adj[nb[off[u]:off[u + 1]]] = True
                    bits = adj[row] & (row != u)
                    pos = int(np.searchsorted(row, x))
                    j, c = int(bits[:pos].sum()), int(bits.sum())
                    g = min(int(np.float32(j) * np.float32(ndir) * (np.float32(1) / np.float32(c))), ndir - 1)
                    guess_high += g > pos // 512
                    guess_low += g < pos // 512
            else:
                in_entry += int(sel.sum())
    return dict(in_region=in_region, in_entry=in_entry, common_at_big=common_at_big,
                guess_high=int(guess_high), guess_low=int(guess_low))


@pytest.fixture(scope="module")
def hub_csr(gw, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("bsloads") / "phases.edgelist")
    _edgelist(path)
    G = gw.GWGraph.from_edgelist(path, " ", "nx")
    csr = G.export_csr()
    G.free()
    deg = np.diff(csr["offsets"])
    assert len(deg) == N and (csr["node_order"] == np.arange(N)).all()
    assert deg.max() > 4096 and ((deg > 512) & (deg <= 4096)).sum() == 3
    return path, csr


_REFS = {}


def _ref(oracle, csr, p, q, seed, L, begin, count, shuffle):
    key = (p, q, seed, L, begin, count, shuffle)
    if key not in _REFS:
        out = oracle.walks_bitset(csr, p, q, seed, L, begin, count, shuffle=bool(shuffle), nthreads=8)
        for a in out:
            a.setflags(write=False)
        _REFS[key] = out
    return _REFS[key]


def _device_graph(gw, path, p, q):
    from gwamd import _lib as C
    G = gw.GWGraph.from_edgelist(path, " ", "nx").to_device(0)
    C.check(C.lib().gw_n2v_prepare(G.handle, float(p), float(q), C.N2V_BITSET), G.handle)
    return G


def _launch_and_compare(G, oracle, csr, p, q, seed, L, begin, count, shuffle, with_outputs):
    import torch
    from gwamd import _lib as C
    out = torch.full((count, L), -7, dtype=torch.int32, device="cuda")
    lens = torch.empty(count, dtype=torch.int32, device="cuda") if with_outputs else None
    cnt = torch.zeros(2, dtype=torch.int64, device="cuda") if with_outputs else None
    C.check(C.lib().gw_n2v_walks(G.handle, L, seed, begin, count, int(shuffle), C.ptr(out),
                                 C.ptr(lens) if with_outputs else None, C.ptr(cnt) if with_outputs else None, None),
            G.handle)
    torch.cuda.synchronize()
    ref, rl, rc = _ref(oracle, csr, p, q, seed, L, begin, count, shuffle)
    msg = f"p={p} q={q} L={L} begin={begin} count={count} shuffle={shuffle} outputs={with_outputs}"
    np.testing.assert_array_equal(out.cpu().numpy(), ref, err_msg=msg)
    if with_outputs:
        np.testing.assert_array_equal(lens.cpu().numpy(), rl, err_msg=msg)
        assert int(cnt[0]) == int(rc[0]) and int(cnt[1]) == int(rc[1]), msg


def test_graph_reaches_every_region_path(oracle, hub_csr):
    """The oracle's walks of the main launch shape at the headline p, q pass
    >= 64 times through a region-mode entry of each directory kind, and >= 64
    times from a big hub on to a common neighbour (a region select through
    the directory words).  The cluster's ids lie in the first and the last
    directory block, the interpolated guess spreads over all 14: of any 64 such
    selects about half guess too high and half too low, so at least a quarter
    of 64 each way is asked."""
    _, csr = hub_csr
    ref, rl, _ = _ref(oracle, csr, 0.25, 4.0, 11, 80, 777, 4000, 1)
    cov = _coverage(csr, ref, rl)
    print(cov)
    assert cov["in_region"] >= 64 and cov["in_entry"] >= 64 and cov["common_at_big"] >= 64, cov
    assert cov["guess_high"] >= 16 and cov["guess_low"] >= 16, cov  # corrections walk g down and up


@pytest.mark.parametrize("p,q", [(0.25, 4.0), (4.0, 0.25)])
def test_launch_shapes_equal_oracle(gw, oracle, hub_csr, p, q):
    """L = 80 (vector flush), 33 (scalar flush, one full stage), 7 (shorter
    than a stage) x 4000, 63, 65 walks, walk_begin never a multiple of 64,
    with lens and counters and with neither."""
    path, csr = hub_csr
    G = _device_graph(gw, path, p, q)
    assert G.info().max_degree > 4096
    for L in (80, 33, 7):
        for count in (4000, 63, 65):
            begin = 777 if count == 4000 else 7 * count + L + 1
            assert begin % 64 != 0
            for with_outputs in (True, False):
                _launch_and_compare(G, oracle, csr, p, q, 11, L, begin, count, 1, with_outputs)
    G.free()


@pytest.mark.parametrize("p,q", [(0.25, 4.0), (0.25, 64.0)])
def test_one_wave_from_the_cluster_keeps_directory_words(gw, oracle, hub_csr, p, q):
    """64 walks — one wave — that all start in the dense cluster, unshuffled:
    big hubs are common neighbours of every cluster pair, so the walkers keep
    arriving at them over region entries and, above all at q = 64, select a
    common neighbour there: several lanes verify or correct directory words
    while others fetch their block or step on.  A lane that loads no
    directory words in an iteration must keep the pair it holds."""
    path, csr = hub_csr
    begin = 3 * N + 12  # walk w starts at vertex w % N: 12..75, all in the cluster
    ref, rl, _ = _ref(oracle, csr, p, q, 5, 80, begin, 64, 0)
    assert np.isin(ref[:, 0], CL).all()
    cov = _coverage(csr, ref, rl)
    print(cov)
    if q == 64.0:
        assert cov["common_at_big"] >= 64 and cov["in_entry"] >= 64, cov
    G = _device_graph(gw, path, p, q)
    for with_outputs in (True, False):
        _launch_and_compare(G, oracle, csr, p, q, 5, 80, begin, 64, 0, with_outputs)
    G.free()
