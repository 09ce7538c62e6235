"""CPU checks of tests/bitset_tables.py, the reference and decoder behind
test_bitset_tables_gpu.py: the common sets against the O(d^2) definition, the
mode thresholds of gw_internal.h, the Elias-Fano decoder and the draw-filter
set against a plain encoder and brute force, and the coverage every graph of
the GPU test is meant to have (so those tests cannot pass vacuously)."""
import numpy as np
import pytest

import bitset_tables as T


# ---- common sets ---------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_common_sets_equal_brute_force(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(5, 40))
    m = rng.random((n, n)) < rng.choice([0.15, 0.4, 0.8])
    e = np.argwhere(np.triu(m))  # the diagonal too: self-loops
    assert (e[:, 0] == e[:, 1]).any()
    csr = T.csr_from_edges(e, n)
    ref = T.Reference(csr, chunk=64)  # several chunks
    want = T.brute_common(csr)
    assert len(want) == ref.nnz
    for s in range(ref.nnz):
        assert ref.common(s).tolist() == want[s], s
        assert ref.c[s] == len(want[s])
        assert csr["nbrs"][ref.off[ref.x[s]] + ref.kp[s]] == ref.u[s]
        assert ref.u[ref.rev[s]] == ref.x[s] and ref.x[ref.rev[s]] == ref.u[s]
        assert ref.c_rev[s] == len(want[ref.rev[s]])
    loops = np.nonzero(ref.u == ref.x)[0]
    assert (ref.c[loops] == ref.d[loops] - 1).all() and not ref.dual[loops].any()


# ---- modes ---------------------------------------------------------------------
def _runs(d):
    """[(first c, mode letter), ...] over c = 0 .. min(d - 1, 400)."""
    c = np.arange(0, min(d - 1, 400) + 1)
    m = T.mode_of(c, np.full_like(c, d))
    out = []
    for ci, mi in zip(c, m):
        if not out or out[-1][1] != "LIER"[mi]:
            out.append((int(ci), "LIER"[mi]))
    return out


def test_mode_thresholds():
    assert _runs(352) == [(0, "L"), (23, "I")]
    assert _runs(353) == [(0, "L"), (23, "E"), (88, "R")]
    assert _runs(4096) == [(0, "L"), (23, "E"), (42, "R")]
    assert _runs(4097) == [(0, "L"), (23, "E"), (42, "R")]
    assert _runs(65535) == [(0, "L"), (23, "E"), (27, "R")]
    assert _runs(65536) == [(0, "R"), (1, "E"), (25, "R")]


def test_mode_matches_scalar_predicates():
    """mode_of against the predicates of gw_internal.h restated with Python integers."""
    rng = np.random.default_rng(7)
    d = np.concatenate([rng.integers(1, 1000, 3000), rng.integers(1000, 200000, 3000),
                        [352, 353, 65535, 65536, 65537] * 40])
    c = np.minimum((rng.random(len(d)) ** 3 * d).astype(np.int64), d - 1)
    got = T.mode_of(c, d)
    for ci, di, g in zip(c.tolist(), d.tolist(), got.tolist()):
        bits = 352 if di < 65536 else 320
        if ci <= 22 and di < 65536:
            want = T.LIST
        elif di <= bits:
            want = T.INLINE
        else:
            want = T.REGION
            if ci > 0:
                l = (di // ci).bit_length() - 1
                if ci * l + ci + ((di - 1) >> l) + 1 <= bits:
                    want = T.EF
        assert g == want, (ci, di)


def test_region_sizes():
    # bits padded to a block; the directory joins the region (padded) only when d > 4096
    assert T.region_words(353) == 16 and T.region_words(512) == 16 and T.region_words(513) == 32
    assert T.region_words(4096) == 128 and T.region_words(4097) == 16 + 144
    assert T.region_words(70000) == T._round_blk(137) + T._round_blk(2188)
    assert [int(v) for v in T.filter_shape(np.array([400, 513, 4096, 4097, 65535, 65536]))[1]] == \
        [320, 192, 192, 320, 320, 288]
    assert [int(v) for v in T.filter_shape(np.array([400, 513, 4097]))[0]] == [1, 5, 1]


# ---- Elias-Fano ------------------------------------------------------------------
def _ef_cases():
    rng = np.random.default_rng(11)
    cases = [(T.ef_positions(23, 353), 353), (T.ef_positions(87, 353), 353), (T.ef_positions(41, 4096), 4096),
             ([65535], 65536), (T.ef_positions(24, 65536), 65536), ([0], 70000),
             (list(range(64 * 3 + 1, 64 * 3 + 44)), 3046)]  # one bucket of 43: > 32 ones in a row
    for _ in range(300):
        d = int(rng.choice([353, 400, 1000, 4096, 4097, 30000, 65535, 65536, 70000, 1 << 20]))
        c = int(rng.integers(1, 90))
        if T.mode_of(c, d) != T.EF:
            continue
        if rng.random() < 0.3:  # a dense run somewhere
            s = int(rng.integers(0, d - c))
            pos = list(range(s, s + c))
        else:
            pos = sorted(rng.choice(d, c, replace=False).tolist())
        cases.append((pos, d))
    return cases


def test_elias_fano_decoder_inverts_the_plain_encoder():
    cases = _ef_cases()
    assert len(cases) > 100
    for nw_sel in (11, 10):
        sub = [(p, d) for p, d in cases if int(T.pw(d)) == nw_sel]
        assert sub
        W = np.stack([T.ef_encode(p, d, nw_sel) for p, d in sub])
        c = np.array([len(p) for p, _ in sub])
        d = np.array([d for _, d in sub])
        l = T.ef_l(c, d)
        U = T.ef_U(c, d, l)
        row, pos, cnt, tail = T.ef_decode(W, c, l, U)
        assert (cnt == c).all() and tail.all()
        assert pos.tolist() == [k for p, _ in sub for k in p]
        # a stray bit behind the code is reported, and a changed low bit changes a position
        W2 = W.copy()
        W2[0, nw_sel - 1] |= 1 << 31
        assert not T.ef_decode(W2, c, l, U)[3][0]


def test_elias_fano_small_d_brute_force():
    """Every c-subset of a small row survives encode -> decode (a 64-bit code space, brute force)."""
    from itertools import combinations
    for d, c in ((9, 2), (12, 3), (16, 4)):
        l = int(T.ef_l(c, d))
        U = int(T.ef_U(c, d, l))
        subs = list(combinations(range(d), c))
        W = np.stack([T.ef_encode(p, d, 11) for p in subs])
        n = len(subs)
        row, pos, cnt, tail = T.ef_decode(W, np.full(n, c), np.full(n, l), np.full(n, U))
        assert (cnt == c).all() and tail.all()
        assert pos.reshape(n, c).tolist() == [list(p) for p in subs]


# ---- draw filter -----------------------------------------------------------------
@pytest.mark.parametrize("W", [5, 7])
def test_draw_range_equals_brute_force_over_all_draws(W):
    """The closed form for {y : some z draws position k} against every (y, z)
    of a W-bit word pair, for every d up to 2^W (degrees are < 2^32 at W = 32)."""
    for d in range(1, (1 << W) + 1, 1 if W == 5 else 3):
        hit = {}
        for y in range(1 << W):
            for z in range(1 << W):
                hit.setdefault(T.gw_index(y, z, d, W), set()).add(y)
        assert sorted(hit) == list(range(d))
        for k in range(d):
            lo, hi = T.draw_range(k, d, W)
            assert hit[k] == set(range(int(lo), int(hi) + 1)), (k, d)


def test_draw_range_ends_at_32_bits():
    """At W = 32 the index is monotone in (y, z): the ends of the closed form against gw_index itself."""
    rng = np.random.default_rng(3)
    M = (1 << 32) - 1
    for d in [353, 354, 4096, 4097, 65535, 65536, 70000, (1 << 27) - 1] + rng.integers(353, 1 << 27, 300).tolist():
        for k in {0, d - 1, int(rng.integers(0, d)), int(rng.integers(0, d))}:
            lo, hi = (int(v) for v in T.draw_range(k, d))
            assert T.gw_index(lo, 0, d) <= k <= T.gw_index(lo, M, d)
            assert T.gw_index(hi, 0, d) <= k <= T.gw_index(hi, M, d)
            assert lo == 0 or T.gw_index(lo - 1, M, d) < k
            assert hi == M or T.gw_index(hi + 1, 0, d) > k


def test_filter_set_equals_brute_force_small_words():
    """Bucket set by definition (every draw of a small word pair) == first/last bucket of the closed form."""
    W = 7
    for d, F in ((40, 12), (100, 20), (128, 32), (77, 77)):
        for pos in ([0], [d - 1], [3, 4, 5], list(range(0, d, 7))):
            want = set()
            for y in range(1 << W):
                if any(T.gw_index(y, z, d, W) in pos for z in range(1 << W)):
                    want.add((y * F) >> W)
            got = set()
            for k in pos:
                b0, b1 = T.filter_buckets(k, d, F, W)
                got |= set(range(int(b0), int(b1) + 1))
            assert got == want, (d, F, pos)


# ---- a plain encoder of the whole table, to drive the checker on the CPU ------------
def encode_tables(ref, lists_only=False):
    """Entries and pool written slot by slot from the layout in bitset_tables' docstring (loops, no vector code)."""
    E = np.zeros((ref.nnz, 16), np.uint32)
    sizes = [int(T.region_words(ref.d[s])) if ref.mode[s] == T.REGION and not lists_only else 0
             for s in range(ref.nnz)]
    pool = np.zeros(max(1, sum(sizes)), np.uint32)
    at = 0
    for s in range(ref.nnz):
        d, c, pos = int(ref.d[s]), int(ref.c[s]), ref.common(s).tolist()
        E[s, 0:4] = (ref.x[s], d, ref.offx[s], ref.meta[s])
        if d < T.PACK_D:
            E[s, 4] = int(ref.kp[s]) | c << 16
            w = E[s, 5:16]
        else:
            E[s, 4], E[s, 5] = ref.kp[s], c
            w = E[s, 6:16]
        h = w.view(np.uint16)
        if ref.dual[s]:
            h[:12] = 0xFFFF
            h[:c] = pos
            rp = ref.common(ref.rev[s])
            h[6:6 + len(rp)] = rp
        elif ref.mode[s] == T.LIST:
            h[:22] = 0xFFFF
            h[:c] = pos
        elif ref.mode[s] == T.INLINE:
            for k in pos:
                w[k >> 5] |= np.uint32(1 << (k & 31))
        elif ref.mode[s] == T.EF:
            w[:] = T.ef_encode(pos, d, len(w))
        elif lists_only:
            w[:10] = T.filter_words(pos, d, 320, 10)
        else:
            nd = int(T.ndir_of(d))
            w[0] = at // 16
            w0, F = (int(v) for v in T.filter_shape(d))
            w[w0:] = T.filter_words(pos, d, F, len(w) - w0)
            counts = [sum(1 for k in pos if k < 512 * g) for g in range(nd)]
            boff = 0
            if 0 < nd <= 8:
                w[1:5].view(np.uint16)[:nd] = counts
            elif nd > 8:
                pool[at:at + nd] = counts
                boff = (nd + 15) // 16 * 16
            for k in pos:
                pool[at + boff + (k >> 5)] |= np.uint32(1 << (k & 31))
            at += sizes[s]
    return E, pool


def _small_graph():
    """A few gadgets small enough for the loop encoder, every mode and directory placement among them."""
    E, base = [], 0
    for c, d, kind, loop in [(6, 40, "ef", False), (6, 40, "ef", True), (23, 352, "ef", False), (23, 353, "ef", False),
                             (88, 353, "region", False), (100, 513, "region", False), (42, 4097, "region", False)]:
        e, base, _ = T.gadget(base, c, d, T._positions(c, d, kind), loop)
        E.append(e)
    return T.csr_from_edges(np.concatenate(E))


@pytest.fixture(scope="module")
def small_ref():
    ref = T.Reference(_small_graph())
    cov = ref.coverage()
    for k in ("list", "inline", "ef", "region", "dual", "entry_dir", "region_dir", "selfloop"):
        assert cov[k] > 0, k
    return ref


@pytest.mark.parametrize("lists_only", [False, True])
def test_checker_accepts_the_plain_encoding(small_ref, lists_only):
    E, pool = encode_tables(small_ref, lists_only)
    assert len(pool) == small_ref.pool_words(lists_only)
    assert T.check_tables(small_ref, E, pool, lists_only) == small_ref.nnz


def test_checker_names_single_field_mutations(small_ref):
    ref = small_ref
    E, pool = encode_tables(ref)
    for name, (E2, pool2, slot) in T.mutations(ref, E, pool).items():
        with pytest.raises(T.TableMismatch) as ei:
            T.check_tables(ref, E2, pool2)
        assert ei.value.field == T.MUTATION_FIELD[name] and ei.value.slot == slot, (name, str(ei.value))
    # header fields and the other payloads
    reg = int(np.nonzero(ref.mode == T.REGION)[0][0])
    for col, field in ((0, "x"), (1, "d"), (2, "off"), (3, "meta"), (4, "kp")):
        E2 = E.copy()
        E2[reg, col] += 1
        with pytest.raises(T.TableMismatch) as ei:
            T.check_tables(ref, E2, pool)
        assert ei.value.field == field and ei.value.slot == reg
    for mode, field, word in ((T.INLINE, "inline_bits", 15), (T.EF, "ef_tail", 15)):
        s = int(np.nonzero(ref.mode == mode)[0][0])
        E2 = E.copy()
        E2[s, word] ^= 1 << 31
        with pytest.raises(T.TableMismatch) as ei:
            T.check_tables(ref, E2, pool)
        assert ei.value.field == field and ei.value.slot == s
    s = int(np.nonzero(ref.dual & (ref.c_rev > 0))[0][0])
    E2 = E.copy()
    E2[s, 5 + 3] ^= 1  # halfword 6: the first position of the reverse slot's list
    with pytest.raises(T.TableMismatch) as ei:
        T.check_tables(ref, E2, pool)
    assert ei.value.field == "dual_rev" and ei.value.slot == s


# ---- coverage of the GPU test's graphs ----------------------------------------------
def _csr(name, gw, tmp_path):
    kind, make = T.graphs()[name]
    if kind == "edges":
        return T.csr_from_edges(make())
    if kind == "rmat":
        G = gw.GWGraph.rmat(*make[0], **make[1])
    else:
        path = make if kind == "file" else str(tmp_path / f"{name}.edgelist")
        if kind == "writer":
            make(path)
        G = gw.GWGraph.from_edgelist(path, " ", "nx")
    csr = G.export_csr()
    G.free()
    return csr


@pytest.mark.parametrize("name", sorted(T.EXPECTED_COVERAGE))
def test_gpu_graphs_have_their_coverage(name, gw, tmp_path):
    ref = T.Reference(_csr(name, gw, tmp_path))
    cov = ref.coverage()
    for k in T.EXPECTED_COVERAGE[name]:
        assert cov[k] > 0, (name, k, cov)
    if name in ("thresholds", "wide"):
        _, gadgets = (T.threshold_graph if name == "thresholds" else T.wide_graph)()
        for c, d, ids in gadgets:
            s = T.gadget_slot(ref, ids["u"], ids["x"])
            assert (ref.c[s], ref.d[s], ref.kp[s]) == (c, d, ids["kp"])
