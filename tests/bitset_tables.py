"""Reference and decoder for the tables gw_dev_bitset_build writes (the 64 B
entries and the region pool that k_walk_bitset / k_walk_listed read), in plain
numpy from the CSR alone.

`Reference(csr)` computes, for every adjacency slot e = (u -> x), the common
positions C = {k : N(x)[k] != u and N(x)[k] in N(u)} (self-loops included by
that formula), kp, d, offsets[x], c = |C|, the reverse slot and its count, the
payload mode (gw_internal.h: gw_bs_is_list / gw_bs_is_inline / gw_bs_is_ef /
gw_bs_ef_l / gw_bs_pw) and the dual rule.  `check_tables(ref, entries, region,
lists_only)` then decodes the exported bytes (gw_n2v_export_bitset) field by
field and raises TableMismatch for the first field that differs, naming the
slot, u, x, c, d, mode and field.

Layout restated (gw_internal.h, gw_n2v_bitset.hip header comment):
  entry  = u32 x, d, off, meta, r[12]
  d < 65536: r[0] = kp | c << 16, payload w = r[1..11] (pw = 11 words)
  else       r[0] = kp, r[1] = c, payload w = r[2..11] (pw = 10 words)
  meta   = mode | l << 2 | U << 7 | (directory blocks before the bits) << 16,
           or kMetaDual | c_rev << 2 for a dual entry (mode LIST)
  LIST   c ascending u16 positions, 0xFFFF up to halfword 2 pw
  dual   halfwords 0..5 own list, 6..11 the reverse slot's list (positions in
         N(u)), both 0xFFFF padded; words 6.. zero.  A slot is dual when
         c <= 6, c_rev <= 6, both degrees < 65536 and u != x (a self-loop
         slot is its own reverse: nothing to elide, the builder keeps a list)
  INLINE bit k of w set <=> k in C (d <= 352)
  EF     U = c + ((d-1) >> l) + 1 unary high bits (bit (k >> l) + rank set),
         then c x l low bits; l = floor(log2(d / c))
  REGION w[0] = 64 B block index of the region; 512 < d <= 4096: w[1..4] =
         u16 common counts before each 512-bit block, filter of 192 buckets
         in w[5..10]; else the filter fills w[1..] (320 buckets, 288 when
         d >= 65536).  Region = [u32 directory padded to a block, d > 4096
         only][bits padded to a block].
  lists-only build (listed rejection sampler): REGION slots have no region;
         the payload is a 320-bucket filter in w[0..9], further words zero;
         the pool is one placeholder word.
  filter bucket b of F is set <=> some 64-bit draw (y:z) with
         gw_index(y, z, d) in C has floor(y F / 2^32) = b.
"""
import numpy as np

PACK_D = 65536
LIST, INLINE, EF, REGION = 0, 1, 2, 3
MODE_NAMES = {LIST: "LIST", INLINE: "INLINE", EF: "EF", REGION: "REGION"}
META_DUAL = 0x40000000
DUAL_C = 6
BLK = 16          # u32 words per 64 B block
DIR_BITS = 512    # bits per directory block
PDIR = 8          # directories of up to 8 blocks live in the entry


class TableMismatch(AssertionError):
    def __init__(self, field, slot, ref, got, want, extra=""):
        self.field, self.slot = field, int(slot)
        s = int(slot)
        dual = bool(ref.dual[s])
        msg = (f"slot {s} ({int(ref.u[s])}->{int(ref.x[s])}) c={int(ref.c[s])} d={int(ref.d[s])} "
               f"mode={MODE_NAMES[int(ref.mode[s])]}{'/dual' if dual else ''}: {field} is {got}, expected {want}")
        super().__init__(msg + (f" ({extra})" if extra else ""))


# ---- predicates of gw_internal.h (vectorised; scalars work too) -------------
def pw(d):
    return np.where(np.asarray(d) < PACK_D, 11, 10)


def payload_bits(d):
    return 32 * pw(d)


def _floor_log2(v):
    # exact for 1 <= v < 2^53: v = m 2^e with m in [0.5, 1)
    return np.frexp(np.asarray(v, np.float64))[1].astype(np.int64) - 1


def ef_l(c, d):
    c, d = np.asarray(c, np.int64), np.asarray(d, np.int64)
    return _floor_log2(np.maximum(d // np.maximum(c, 1), 1))


def ef_U(c, d, l):
    return np.asarray(c, np.int64) + ((np.asarray(d, np.int64) - 1) >> l) + 1


def mode_of(c, d):
    c, d = np.asarray(c, np.int64), np.asarray(d, np.int64)
    is_list = (c <= 22) & (d < PACK_D)
    is_inline = d <= payload_bits(d)
    l = ef_l(c, d)
    fits = c * l + ef_U(c, d, l) <= payload_bits(d)
    is_ef = ~is_list & ~is_inline & (c > 0) & fits
    return np.where(is_list, LIST, np.where(is_inline, INLINE, np.where(is_ef, EF, REGION)))


def ndir_of(d):
    d = np.asarray(d, np.int64)
    return np.where(d > DIR_BITS, (d + DIR_BITS - 1) // DIR_BITS, 0)


def _round_blk(w):
    return (w + BLK - 1) // BLK * BLK


def bits_offset(d):
    """Word offset of the bits inside a region: an in-region directory (d > 4096) padded to a block."""
    nd = ndir_of(d)
    return np.where(nd > PDIR, _round_blk(nd), 0)


def region_words(d):
    d = np.asarray(d, np.int64)
    return bits_offset(d) + _round_blk((d + 31) // 32)


def filter_shape(d, lists_only=False):
    """(first payload word, bucket count) of a REGION entry's draw filter."""
    d = np.asarray(d, np.int64)
    if lists_only:
        return np.zeros_like(d), np.full_like(d, 320)
    nd = ndir_of(d)
    w0 = np.where((nd > 0) & (nd <= PDIR), 5, 1)
    return w0, 32 * (pw(d) - w0)


# ---- draw index and filter -----------------------------------------------------
def gw_index(y, z, d, W=32):
    """floor((y 2^W + z) d / 2^2W) in exact integers (gw_philox.h, W = 32)."""
    return ((int(y) << W) + int(z)) * int(d) >> (2 * W)


def draw_range(k, d, W=32):
    """Closed form of {y : some z has gw_index(y, z, d) == k} = [ylo, yhi].
    The index is monotone in (y, z); y qualifies iff index(y, 0) <= k <=
    index(y, 2^W - 1).  index(y, 0) = floor(y d / 2^W) <= k  <=>  y <=
    ceil((k + 1) 2^W / d) - 1, and index(y, 2^W - 1) >= k  <=>  y >=
    floor(k 2^W / d) (the remainder of k 2^W / d is < d <= 2^W)."""
    k, d = np.asarray(k, np.int64), np.asarray(d, np.int64)
    ylo = (k << W) // d
    yhi = (((k + 1) << W) + d - 1) // d - 1
    return ylo, yhi


def filter_buckets(k, d, F, W=32):
    """First and last bucket of position k (at most two buckets when d >= F)."""
    ylo, yhi = draw_range(k, d, W)
    F = np.asarray(F, np.int64)
    return (ylo * F) >> W, (yhi * F) >> W


def filter_words(pos, d, F, nwords):
    """The filter of one slot as u32 words (plain loop; the checker's vectorised twin is _filters)."""
    w = np.zeros(nwords, np.uint32)
    for k in pos:
        b0, b1 = filter_buckets(int(k), int(d), int(F))
        for b in range(int(b0), int(b1) + 1):
            w[b >> 5] |= np.uint32(1 << (b & 31))
    return w


# ---- Elias-Fano ------------------------------------------------------------------
def ef_encode(pos, d, nwords):
    """Plain encoder from the header comment: bit (k >> l) + rank of the unary
    part, then l low bits per position from bit U on."""
    c = len(pos)
    l = int(ef_l(c, d))
    U = int(ef_U(c, d, l))
    v = 0
    for i, k in enumerate(pos):
        v |= 1 << ((int(k) >> l) + i)
        v |= (int(k) & ((1 << l) - 1)) << (U + i * l)
    assert v < 1 << (32 * nwords)
    return np.array([(v >> (32 * j)) & 0xFFFFFFFF for j in range(nwords)], np.uint32)


def ef_decode(words, c, l, U):
    """(positions, tail_is_zero) of a batch: words [m, nw] u32; c, l, U [m]."""
    words = np.ascontiguousarray(words, np.uint32)
    m, nw = words.shape
    bits = np.unpackbits(words.view(np.uint8).reshape(m, nw * 4), axis=1, bitorder="little")
    col = np.arange(nw * 32)
    c, l, U = (np.asarray(a, np.int64) for a in (c, l, U))
    hi_r, hi_c = np.nonzero(bits & (col[None, :] < U[:, None]))
    cnt = np.bincount(hi_r, minlength=m)
    first = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    rank = np.arange(len(hi_r)) - first[hi_r]
    high = hi_c - rank
    low = np.zeros(len(hi_r), np.int64)
    lr, Ur = l[hi_r], U[hi_r]
    for t in range(int(l.max()) if m else 0):
        on = t < lr
        idx = np.minimum(Ur + rank * lr + t, nw * 32 - 1)
        low |= (bits[hi_r, idx].astype(np.int64) * on) << t
    tail_ok = ~(bits & (col[None, :] >= (U + c * l)[:, None])).any(axis=1)
    return hi_r, (high << lr) | low, cnt, tail_ok


# ---- reference ---------------------------------------------------------------------
class Reference:
    """Per-slot reference quantities of an undirected simple graph's CSR
    (rows sorted by id, self-loops allowed)."""

    def __init__(self, csr, chunk=1 << 22):
        off = np.asarray(csr["offsets"], np.int64)
        nb = np.asarray(csr["nbrs"], np.int64)
        n, nnz = len(off) - 1, len(nb)
        deg = np.diff(off)
        self.off, self.nb, self.n, self.nnz, self.deg = off, nb, n, nnz, deg
        self.u = np.repeat(np.arange(n, dtype=np.int64), deg)
        self.x = nb
        self.d = deg[nb]
        self.du = deg[self.u]
        self.offx = off[nb]
        key = self.u * n + nb  # ascending: rows are sorted
        assert (np.diff(key) > 0).all(), "rows must be sorted and duplicate-free"
        self._key = key
        self.rev = np.searchsorted(key, nb * n + self.u)
        assert (key[self.rev] == nb * n + self.u).all(), "graph must be undirected"
        self.kp = self.rev - self.offx
        # common positions: every undirected edge once, the shorter row s
        # searched in the longer row t; a hit w = N(s)[i] = N(t)[j] is common
        # position j of slot (s -> t) unless w == s, and i of (t -> s) unless w == t
        own = (self.du < self.d) | ((self.du == self.d) & (self.u <= self.x))
        es = np.nonzero(own)[0]  # slots (s -> t): s = u, t = x
        keys = []
        cost = np.cumsum(self.du[es])
        start = 0
        while start < len(es):
            stop = int(np.searchsorted(cost, (cost[start - 1] if start else 0) + chunk, side="right"))
            stop = max(stop, start + 1)
            e = es[start:stop]
            ds = self.du[e]
            se, te = self.u[e], self.x[e]
            row = np.repeat(np.arange(len(e)), ds)  # index into e of every element of the shorter rows
            first = np.cumsum(ds) - ds
            idx = np.arange(len(row)) + (off[se] - first)[row]
            w = nb[idx]
            q = (te * n)[row] + w
            p = np.minimum(np.searchsorted(key, q), nnz - 1)
            h = np.nonzero(key[p] == q)[0]
            row, w, p, idx = row[h], w[h], p[h], idx[h]
            s, t = se[row], te[row]
            a = w != s
            keys.append((e[row[a]] << 32) | (p[a] - off[t[a]]))
            b = (w != t) & (s != t)
            keys.append((self.rev[e[row[b]]] << 32) | (idx[b] - off[s[b]]))
            start = stop
        allk = np.sort(np.concatenate(keys)) if keys else np.zeros(0, np.int64)
        self.cslot = allk >> 32
        self.cpos = allk & 0xFFFFFFFF
        self.c = np.bincount(self.cslot, minlength=nnz).astype(np.int64)
        self.cptr = np.concatenate([[0], np.cumsum(self.c)])
        self.crank = np.arange(len(allk)) - self.cptr[self.cslot]
        self.c_rev = self.c[self.rev]
        self.mode = mode_of(self.c, self.d)
        self.dual = ((self.c <= DUAL_C) & (self.c_rev <= DUAL_C) & (self.d < PACK_D) & (self.du < PACK_D)
                     & (self.u != self.x))
        self.l = np.where(self.mode == EF, ef_l(self.c, self.d), 0)
        self.U = np.where(self.mode == EF, ef_U(self.c, self.d, self.l), 0)
        self.ndir = ndir_of(self.d)
        self.meta = np.where(self.dual, META_DUAL | (self.c_rev << 2),
                             self.mode | (self.l << 2) | (self.U << 7)
                             | (np.where(self.mode == REGION, bits_offset(self.d) // BLK, 0) << 16))

    def common(self, e):
        return self.cpos[self.cptr[e]:self.cptr[e + 1]]

    def coverage(self):
        m, d, c = self.mode, self.d, self.c
        reg = m == REGION
        return dict(list=int(((m == LIST) & ~self.dual).sum()), inline=int((m == INLINE).sum()),
                    ef=int((m == EF).sum()), region=int(reg.sum()), dual=int(self.dual.sum()),
                    entry_dir=int((reg & (d > DIR_BITS) & (d <= PDIR * DIR_BITS)).sum()),
                    region_dir=int((reg & (d > PDIR * DIR_BITS)).sum()),
                    wide_ef=int(((m == EF) & (d >= PACK_D)).sum()),
                    wide_region=int((reg & (d >= PACK_D)).sum()),
                    wide_region_c0=int((reg & (d >= PACK_D) & (c == 0)).sum()),
                    selfloop=int((self.u == self.x).sum()))

    def pool_words(self, lists_only=False):
        if lists_only:
            return 1
        return max(1, int(region_words(self.d[self.mode == REGION]).sum()))


def brute_common(csr):
    """O(d^2) per slot: the definition, for tiny graphs."""
    off, nb = csr["offsets"], csr["nbrs"]
    out = []
    for u in range(len(off) - 1):
        Nu = [int(v) for v in nb[off[u]:off[u + 1]]]
        for x in Nu:
            Nx = [int(v) for v in nb[off[x]:off[x + 1]]]
            out.append([k for k in range(len(Nx)) if Nx[k] != u and any(Nx[k] == w for w in Nu)])
    return out


def csr_from_edges(edges, n=None):
    """Sorted, duplicate-free undirected CSR of (a, b) pairs (dense ids)."""
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    n = int(e.max()) + 1 if n is None else n
    a = np.concatenate([e[:, 0], e[:, 1]])
    b = np.concatenate([e[:, 1], e[:, 0]])
    k = np.unique(a * n + b)
    off = np.concatenate([[0], np.cumsum(np.bincount(k // n, minlength=n))]).astype(np.int64)
    return dict(offsets=off, nbrs=(k % n).astype(np.int32))


# ---- checker ---------------------------------------------------------------------------
def _first(bad):
    return int(np.nonzero(bad)[0][0])


def _or_scatter(shape, rows, word, bit):
    """u32 image [shape] with bit `bit` of word (rows, word) set; (rows, word, bit) triples are distinct."""
    flat = np.bincount(rows * shape[1] + word, weights=np.ldexp(1.0, bit.astype(np.int32)),
                       minlength=shape[0] * shape[1])
    return flat.astype(np.uint64).astype(np.uint32).reshape(shape)


def _payload(E, d):
    """[nnz, 11] payload words (d >= 65536: ten words and a zero column)."""
    P = E[:, 5:16].copy()
    wide = d >= PACK_D
    P[wide, :10] = E[wide, 6:16]
    P[wide, 10] = 0
    return P


def _pairs(ref, sel):
    """(row in sel, position, rank) of every common position of the selected slots."""
    idx = np.full(ref.nnz, -1, np.int64)
    idx[sel] = np.arange(len(sel))
    r = idx[ref.cslot]
    on = r >= 0
    return r[on], ref.cpos[on], ref.crank[on]


def _filters(ref, sel, lists_only):
    """Expected filter image [len(sel), 11] of REGION slots `sel`, placed at their first filter word."""
    w0, F = filter_shape(ref.d[sel], lists_only)
    r, k, _ = _pairs(ref, sel)
    b0, b1 = filter_buckets(k, ref.d[sel][r], F[r])
    assert ((b1 - b0) >= 0).all() and ((b1 - b0) <= 1).all()  # d > F: a position spans at most two buckets
    rows = np.concatenate([r, r[b1 > b0]])
    b = np.concatenate([b0, b1[b1 > b0]])
    t = np.unique(rows * 512 + b)  # neighbouring positions share buckets
    rows, b = t // 512, t % 512
    return _or_scatter((len(sel), 11), rows, w0[rows] + (b >> 5), b & 31), w0, F


def check_tables(ref, entries, region, lists_only=False):
    """Raise TableMismatch for the first field of the exported tables that
    differs from the reference; returns the number of slots checked."""
    E = np.frombuffer(entries, np.uint32).reshape(-1, 16) if not isinstance(entries, np.ndarray) else \
        entries.view(np.uint32).reshape(-1, 16)
    region = np.asarray(region, np.uint32)
    assert E.shape[0] == ref.nnz, (E.shape, ref.nnz)
    wide = ref.d >= PACK_D

    def fail(field, slots_bad, got, want, extra=""):
        s = _first(slots_bad)
        g = got[s] if isinstance(got, np.ndarray) else got
        w = want[s] if isinstance(want, np.ndarray) else want
        raise TableMismatch(field, s, ref, g, w, extra)

    # header
    for name, col, want in (("x", 0, ref.x), ("d", 1, ref.d), ("off", 2, ref.offx)):
        bad = E[:, col] != want
        if bad.any():
            fail(name, bad, E[:, col], want)
    kp = np.where(wide, E[:, 4], E[:, 4] & 0xFFFF).astype(np.int64)
    c = np.where(wide, E[:, 5], E[:, 4] >> 16).astype(np.int64)
    if (kp != ref.kp).any():
        fail("kp", kp != ref.kp, kp, ref.kp)
    if (c != ref.c).any():
        fail("c", c != ref.c, c, ref.c)
    meta = E[:, 3].astype(np.int64)
    if (meta != ref.meta).any():
        s = _first(meta != ref.meta)
        raise TableMismatch("meta", s, ref, hex(meta[s]), hex(ref.meta[s]), f"c_rev={int(ref.c_rev[s])}")
    P = _payload(E, ref.d)
    npw = pw(ref.d)

    # LIST (not dual): c ascending u16 positions, 0xFFFF up to halfword 2 pw = 22
    sel = np.nonzero((ref.mode == LIST) & ~ref.dual)[0]
    if len(sel):
        H = P[sel].view(np.uint16).reshape(len(sel), 22).astype(np.int64)
        want = np.full((len(sel), 22), 0xFFFF, np.int64)
        r, k, rk = _pairs(ref, sel)
        want[r, rk] = k
        isval = np.arange(22)[None, :] < ref.c[sel][:, None]
        bad = ((H != want) & isval).any(axis=1)
        if bad.any():
            i = _first(bad)
            raise TableMismatch("list", sel[i], ref, H[i][:ref.c[sel[i]]].tolist(), want[i][:ref.c[sel[i]]].tolist())
        bad = ((H != want) & ~isval).any(axis=1)
        if bad.any():
            i = _first(bad)
            h = _first((H[i] != want[i]) & ~isval[i])
            raise TableMismatch("list_pad", sel[i], ref, hex(H[i, h]), "0xffff", f"halfword {h}")

    # dual: own list in halfwords 0..5, the reverse slot's in 6..11, words 6.. zero
    sel = np.nonzero(ref.dual)[0]
    if len(sel):
        H = P[sel].view(np.uint16).reshape(len(sel), 22).astype(np.int64)
        want = np.full((len(sel), 12), 0xFFFF, np.int64)
        r, k, rk = _pairs(ref, sel)
        want[r, rk] = k
        back = np.full(ref.nnz, -1, np.int64)
        back[ref.rev[sel]] = np.arange(len(sel))  # the reverse slot of a dual slot is dual too
        rr = back[ref.cslot]
        on = rr >= 0
        want[rr[on], DUAL_C + ref.crank[on]] = ref.cpos[on]
        for name, lo, hi in (("dual_own", 0, 6), ("dual_rev", 6, 12)):
            bad = (H[:, lo:hi] != want[:, lo:hi]).any(axis=1)
            if bad.any():
                i = _first(bad)
                raise TableMismatch(name, sel[i], ref, H[i, lo:hi].tolist(), want[i, lo:hi].tolist(),
                                    f"c_rev={int(ref.c_rev[sel[i]])}")
        bad = (H[:, 12:] != 0).any(axis=1)
        if bad.any():
            i = _first(bad)
            raise TableMismatch("dual_tail", sel[i], ref, H[i, 12:].tolist(), "zeros")

    # INLINE: bit k <=> k in C (so no bit at or past d)
    sel = np.nonzero(ref.mode == INLINE)[0]
    if len(sel):
        r, k, _ = _pairs(ref, sel)
        want = _or_scatter((len(sel), 11), r, k >> 5, k & 31)
        bad = (P[sel] != want).any(axis=1)
        if bad.any():
            i = _first(bad)
            wd = _first(P[sel[i]] != want[i])
            raise TableMismatch("inline_bits", sel[i], ref, hex(P[sel[i], wd]), hex(want[i, wd]), f"payload word {wd}")

    # Elias-Fano: decode, compare with C, the rest of the payload zero
    sel_all = np.nonzero(ref.mode == EF)[0]
    for s0 in range(0, len(sel_all), 1 << 16):
        sel = sel_all[s0:s0 + (1 << 16)]
        W = P[sel].copy()
        row, pos, cnt, tail_ok = ef_decode(W, ref.c[sel], ref.l[sel], ref.U[sel])
        bad = cnt != ref.c[sel]
        if bad.any():
            i = _first(bad)
            raise TableMismatch("ef_high_count", sel[i], ref, int(cnt[i]), int(ref.c[sel[i]]))
        _, k, _ = _pairs(ref, sel)
        if (pos != k).any():
            j = _first(pos != k)
            i = row[j]
            raise TableMismatch("ef_positions", sel[i], ref, pos[row == i].tolist(), ref.common(sel[i]).tolist())
        if not tail_ok.all():
            i = _first(~tail_ok)
            raise TableMismatch("ef_tail", sel[i], ref, "set bits past U + c*l", "zeros")

    # REGION
    sel = np.nonzero(ref.mode == REGION)[0]
    pool = ref.pool_words(lists_only)
    if len(region) != pool:
        raise AssertionError(f"region pool holds {len(region)} words, expected {pool}")
    if len(sel):
        want, w0, F = _filters(ref, sel, lists_only)
        d = ref.d[sel]
        if lists_only:
            fmask = np.arange(11)[None, :] < 10
        else:
            fmask = (np.arange(11)[None, :] >= w0[:, None]) & (np.arange(11)[None, :] < npw[sel][:, None])
            # region layout: w[0] blocks, each region bs_words(d) long, disjoint, filling the pool
            size = region_words(d)
            base = P[sel, 0].astype(np.int64) * BLK
            scan = np.concatenate([[0], np.cumsum(size)[:-1]])
            o = np.argsort(base, kind="stable")
            ends = base[o] + size[o]
            ok = (base[o][0] == 0) and (ends[:-1] == base[o][1:]).all() and ends[-1] == pool
            if not ok:
                bad = base != scan
                i = _first(bad) if bad.any() else int(o[0])
                raise TableMismatch("region_index", sel[i], ref, int(base[i] // BLK), int(scan[i] // BLK),
                                    "regions must be disjoint, inside the pool and fill it")
            # in-entry directory: u16 counts before each 512-bit block in w[1..4], unused halfwords zero
            nd = ref.ndir[sel]
            ent = np.nonzero((nd > 0) & (nd <= PDIR))[0]
            r, k, _ = _pairs(ref, sel)
            if len(ent):
                loc = np.full(len(sel), -1, np.int64)
                loc[ent] = np.arange(len(ent))
                on = loc[r] >= 0
                hist = np.bincount(loc[r[on]] * PDIR + (k[on] >> 9), minlength=len(ent) * PDIR).reshape(-1, PDIR)
                wantd = np.cumsum(hist, axis=1) - hist
                wantd[np.arange(PDIR)[None, :] >= nd[ent][:, None]] = 0
                got = P[sel[ent], 1:5].copy().view(np.uint16).reshape(len(ent), PDIR).astype(np.int64)
                bad = (got != wantd).any(axis=1)
                if bad.any():
                    i = _first(bad)
                    g = _first(got[i] != wantd[i])
                    raise TableMismatch("entry_dir", sel[ent[i]], ref, int(got[i, g]), int(wantd[i, g]),
                                        f"directory block {g}")
            # the pool image: in-region directories and bits at the claimed offsets, zero elsewhere
            boff = bits_offset(d)
            img = np.zeros(pool, np.uint32)
            if len(r):
                wi = base[r] + boff[r] + (k >> 5)
                img = _or_scatter((1, pool), np.zeros(len(r), np.int64), wi, k & 31)[0]
            for i in np.nonzero(nd > PDIR)[0]:
                cp = ref.common(sel[i])
                img[base[i]:base[i] + nd[i]] = np.searchsorted(cp, np.arange(nd[i]) * DIR_BITS)
            if (img != region).any():
                wd = _first(img != region)
                i = int(np.searchsorted(base[o], wd, side="right")) - 1
                i = int(o[i])
                rel = wd - base[i]
                if rel < boff[i]:
                    name, what = "region_dir", f"directory block {rel}"
                else:
                    name, what = "region_bits", f"bit word {rel - boff[i]} of the region"
                raise TableMismatch(name, sel[i], ref, hex(region[wd]), hex(img[wd]), what)
        # draw filter: equality with the exact bucket set, both directions
        got = P[sel] & np.where(fmask, 0xFFFFFFFF, 0).astype(np.uint32)
        bad = (got != want).any(axis=1)
        if bad.any():
            i = _first(bad)
            wd = _first(got[i] != want[i])
            miss, extra = want[i, wd] & ~got[i, wd], got[i, wd] & ~want[i, wd]
            raise TableMismatch("filter", sel[i], ref, hex(got[i, wd]), hex(want[i, wd]),
                                f"payload word {wd} of a {int(F[i])}-bucket filter from word {int(w0[i])}: "
                                f"missing {hex(miss)}, spurious {hex(extra)}")
        if lists_only:
            bad = P[sel, 10] != 0
            if bad.any():
                fail_slot = sel[_first(bad)]
                raise TableMismatch("payload_tail", fail_slot, ref, hex(P[fail_slot, 10]), "0x0")
    elif not lists_only and region[0] != 0:
        raise AssertionError(f"placeholder region word is {hex(region[0])}, expected 0")
    if lists_only and region[0] != 0:
        raise AssertionError(f"placeholder region word is {hex(region[0])}, expected 0")
    return ref.nnz


# ---- threshold gadgets -----------------------------------------------------------------
def ef_positions(c, d):
    """First, last, and the rest as one run from the start of an Elias-Fano
    bucket (a bucket of 2^l positions is filled, or holds the whole run)."""
    l = int(ef_l(c, d))
    start = max(1 << l, ((d // 3) >> l) << l)
    pos = sorted({0, d - 1} | set(range(start, start + c - 2)))
    assert len(pos) == c and pos[-1] == d - 1
    return pos


def region_positions(c, d):
    """{0, 31, 32, 511, 512, d-1} (those below d); c >= 1024: a run filling the
    whole 512-bit block 4 with block 5 left empty and the rest spread behind
    it; else one run in block 2 (or right behind position 32 when d is small)."""
    pos = {k for k in (0, 31, 32, 511, 512, d - 1) if k < d}
    if c >= 1024:
        pos |= set(range(4 * 512, 5 * 512))
        rest = c - len(pos)
        pos |= set(np.linspace(6 * 512, d - 3, rest).astype(np.int64).tolist())
    else:
        start = 1024 if d > 1024 + c else 40
        pos |= set(range(start, start + c - len(pos)))
    assert len(pos) == c and max(pos) == d - 1, (c, d, len(pos))
    return sorted(pos)


def gadget(base, c, d, positions, loop_u=False, ballast=False, off_ballast=5):
    """x = base with neighbours base+1 .. base+d (position k of N(x) is vertex
    base+1+k); u among them, adjacent to exactly the c others at `positions`,
    so slot (u -> x) has (c, d) and (x -> u) has c (c + 1 with a self-loop at
    u).  ballast: a further neighbour z adjacent to every other neighbour of x
    but u and `off_ballast` leaves (leaf slots then have c = 1, the leaves left
    off z have c = 0).  Returns (edges [m, 2], next free id, dict of ids)."""
    assert len(positions) == c and len(set(positions)) == c
    taken = set(positions)
    free = [k for k in range(d - 2, 0, -1) if k not in taken][:2 + off_ballast]
    kp = free[0]
    x, u = base, base + 1 + kp
    k_all = np.arange(d, dtype=np.int64)
    E = [np.stack([np.full(d, x, np.int64), base + 1 + k_all], 1),
         np.stack([np.full(c, u, np.int64), base + 1 + np.asarray(positions, np.int64)], 1)]
    if loop_u:
        E.append(np.array([[u, u]], np.int64))
    ids = dict(x=x, u=u, kp=kp)
    if ballast:
        kz, off = free[1], free[2:]
        z = base + 1 + kz
        on = np.ones(d, bool)
        on[[kp, kz] + off] = False
        E.append(np.stack([np.full(int(on.sum()), z, np.int64), base + 1 + k_all[on]], 1))
        ids.update(z=z, off_leaves=[base + 1 + k for k in off])
    return np.concatenate(E), base + d + 1, ids


THRESHOLD_GADGETS = (
    # (c, d, positions, loop_u): dual / list / not dual next to a self-loop
    [(6, 40, "ef", False), (7, 40, "ef", False), (6, 40, "ef", True)]
    # list / Elias-Fano / inline / region thresholds at 353, 352
    + [(22, 353, "ef", False), (23, 353, "ef", False), (23, 352, "ef", False), (87, 353, "ef", False),
       (88, 353, "region", False)]
    # Elias-Fano / region at 4096, 4097
    + [(41, 4096, "ef", False), (42, 4096, "region", False), (42, 4097, "region", False)]
    # no directory / in-entry directory / in-region directory
    + [(100, 512, "region", False), (100, 513, "region", False), (300, 4096, "region", False),
       (300, 4097, "region", False)])

WIDE_GADGETS = [(c, d) for d in (65535, 65536, 70000) for c in (1, 24, 25, 3000)]


def _positions(c, d, kind):
    if kind == "region" or c >= 1024:
        return region_positions(c, d)
    if c == 1:
        return [d - 1]
    return ef_positions(c, d)


def threshold_graph():
    """The threshold gadgets as disjoint components; returns (edges, list of (c, d, ids))."""
    E, base, out = [], 0, []
    for c, d, kind, loop in THRESHOLD_GADGETS:
        e, base, ids = gadget(base, c, d, _positions(c, d, kind), loop)
        E.append(e)
        out.append((c, d, ids))
    return np.concatenate(E), out


def wide_graph():
    """Gadgets at d in {65535, 65536, 70000} with ballast (the unpacked-header form of an entry)."""
    E, base, out = [], 0, []
    for c, d in WIDE_GADGETS:
        e, base, ids = gadget(base, c, d, _positions(c, d, "ef"), False, ballast=True)
        E.append(e)
        out.append((c, d, ids))
    return np.concatenate(E), out


def gadget_slot(ref, a, b):
    """Slot index of (a -> b)."""
    e = int(np.searchsorted(ref._key, a * ref.n + b))
    assert ref._key[e] == a * ref.n + b
    return e


# ---- single-field mutations (the checker must name each) ---------------------------------
MUTATION_FIELD = dict(region_bit="region_bits", filter_clear="filter", filter_set="filter",
                      entry_dir_count="entry_dir", region_dir_count="region_dir", list_pad="list_pad",
                      region_index="region_index")


def mutations(ref, E, pool):
    """name -> (entries, pool, slot) with one field of a full build's tables changed."""
    E = E.view(np.uint32).reshape(-1, 16)
    out = {}
    reg = np.nonzero((ref.mode == REGION) & (ref.c > 0))[0]
    assert len(reg)

    def pcol(s):  # column of payload word 0
        return 5 if ref.d[s] < PACK_D else 6

    s = int(reg[len(reg) // 2])
    base = int(E[s, pcol(s)]) * BLK + int(bits_offset(ref.d[s]))
    p2 = pool.copy()
    k = int(ref.common(s)[0])
    p2[base + (k >> 5)] ^= np.uint32(1 << (k & 31))
    out["region_bit"] = (E, p2, s)
    w0, F = (int(v) for v in filter_shape(ref.d[s]))
    words = E[s, pcol(s) + w0:pcol(s) + w0 + F // 32]
    bits = np.unpackbits(words.copy().view(np.uint8), bitorder="little")
    for name, val in (("filter_clear", 1), ("filter_set", 0)):
        b = int(np.nonzero(bits == val)[0][0])
        E2 = E.copy()
        E2[s, pcol(s) + w0 + (b >> 5)] ^= np.uint32(1 << (b & 31))
        out[name] = (E2, pool, s)
    ent = reg[(ref.ndir[reg] > 0) & (ref.ndir[reg] <= PDIR)]
    if len(ent):
        s = int(ent[0])
        E2 = E.copy()
        E2[s, pcol(s) + 1] += np.uint32(1 << 16)  # halfword 1: the count before block 1
        out["entry_dir_count"] = (E2, pool, s)
    big = reg[ref.ndir[reg] > PDIR]
    if len(big):
        s = int(big[-1])
        p2 = pool.copy()
        p2[int(E[s, pcol(s)]) * BLK + int(ref.ndir[s]) - 1] += 1
        out["region_dir_count"] = (E, p2, s)
    lst = np.nonzero((ref.mode == LIST) & ~ref.dual & (ref.c < 22))[0]
    if len(lst):
        s = int(lst[0])
        E2 = E.copy()
        h = E2[s, pcol(s):].view(np.uint16)
        h[int(ref.c[s])] = 0
        E2[s, pcol(s):] = h.view(np.uint32)
        out["list_pad"] = (E2, pool, s)
    s = int(reg[0])
    E2 = E.copy()
    E2[s, pcol(s)] += 1
    out["region_index"] = (E2, pool, s)
    return out


# ---- the graphs of test_bitset_tables_gpu.py ----------------------------------------------
def graphs():
    """name -> (kind, maker): "writer" writes an edge list to a path, "edges"
    returns an [m, 2] array, "file" is a path, "rmat" holds GWGraph.rmat's arguments."""
    import os

    from conftest import DATA
    from test_bitset_walk_loads_gpu import _edgelist as _phases_edgelist
    from test_n2v_gpu import (_ef_bucket_edgelist, _hub_edgelist, _mixed_mode_edgelist, _multichunk_hub_edgelist,
                              _selfloop_sparse_edgelist)
    return dict(mixed=("writer", _mixed_mode_edgelist), hub=("writer", _hub_edgelist),
                multichunk=("writer", _multichunk_hub_edgelist), selfloop=("writer", _selfloop_sparse_edgelist),
                ef_bucket=("writer", _ef_bucket_edgelist), phases=("writer", _phases_edgelist),
                karate=("file", os.path.join(DATA, "karate.edgelist")), rmat12=("rmat", ((12, 16), dict(seed=11))),
                thresholds=("edges", lambda: threshold_graph()[0]), wide=("edges", lambda: wide_graph()[0]))


# classes of slots each graph is meant to hold (Reference.coverage keys)
EXPECTED_COVERAGE = dict(
    mixed=("list", "inline", "ef", "region", "dual", "entry_dir", "selfloop"),
    hub=("list", "ef", "region", "dual", "region_dir"),
    multichunk=("list", "region", "dual", "region_dir"),
    selfloop=("list", "dual", "selfloop"),
    ef_bucket=("ef", "dual"),
    phases=("list", "inline", "ef", "region", "dual", "entry_dir", "region_dir"),
    karate=("list", "dual"),
    rmat12=("list", "inline", "ef", "region", "dual", "entry_dir"),
    thresholds=("list", "inline", "ef", "region", "dual", "entry_dir", "region_dir", "selfloop"),
    wide=("list", "ef", "region", "dual", "entry_dir", "region_dir", "wide_ef", "wide_region", "wide_region_c0"))
