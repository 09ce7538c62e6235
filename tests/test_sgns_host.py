"""CPU: the SGNS trainer's host side (gw_sgns_*, device = -1) - vocabulary and
sampler tables, the training law against an independent numpy restatement,
the word2vec text writer and the argument checks.

The restatement below is written from the law as include/graphwalk.h states
it and draws through gw_philox4x32(-1, ...), which test_philox_kat.py pins.
It exists twice: in fp64 (dot products by np.dot) and in fp32 with the dot
products summed in plain index order.  Neither is the code under test; the
library's lane-strided tree is a third summation order of the same length,
so it may differ from the fp64 result by a small multiple of what the fp32
restatement differs by (4x, see test_host_law_matches_restatement).
"""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import DATA, load_golden

TAG_TOK, TAG_NEG, TAG_INIT = 0x73675430, 0x73674E30, 0x73674930
EXP_SCALE = float(np.float32(1000.0 / 12.0))


def _C():
    from gwamd import _lib as C
    C.lib()
    return C


def philox(rows):
    """rows [m][6] uint32 (c0..c3, k0, k1) -> [m][4] through the library's host evaluation."""
    C = _C()
    a = np.ascontiguousarray(rows, np.uint32).reshape(-1, 6)
    out = np.empty((a.shape[0], 4), np.uint32)
    assert C.lib().gw_philox4x32(-1, C.ptr(a), a.shape[0], C.ptr(out)) == 0
    return out


def golden_walks(name):
    """Dense-id int32 walks (-1 padded) and the vertex count of a golden walk file."""
    d = load_golden(name)
    dense = {int(l): i for i, l in enumerate(d["labels"])}
    W = np.full(d["walks"].shape, -1, np.int32)
    for i, n in enumerate(d["lens"]):
        W[i, :n] = [dense[int(v)] for v in d["walks"][i, :n]]
    return W, len(d["labels"]), d["labels"].astype(np.int64)


def barbell_corpus():
    """Two 6-cliques joined by the bridge 5-6; 24 uniform walks of 10 (fixed seed), some rows cut short
    by -1 and one row all -1."""
    adj = {v: [u for u in range(6) if u != v] for v in range(6)}
    adj.update({v: [u for u in range(6, 12) if u != v] for v in range(6, 12)})
    adj[5].append(6)
    adj[6].append(5)
    rng = np.random.RandomState(12345)
    W = np.full((24, 10), -1, np.int32)
    for w in range(24):
        v = w % 12
        for i in range(10):
            W[w, i] = v
            v = adj[v][rng.randint(len(adj[v]))]
    W[3, 7:] = -1
    W[10, 1:] = -1   # a single token: no pair
    W[17, :] = -1    # empty walk
    W[20, 4:] = -1
    return W, 12


def uniform_corpus(n, nwalks, width, seed, lens=None):
    """`nwalks` rows of uniform ids in [0, n) (fixed seed); row w is cut to lens[w] tokens by -1."""
    W = np.random.RandomState(seed).randint(0, n, (nwalks, width)).astype(np.int32)
    for w, ln in enumerate(lens or ()):
        W[w, ln:] = -1
    return W, n


# walk lengths around the kernel's 64-position trips, the reference's default 80 and the full width
LONG_LENS = (130, 0, 1, 63, 64, 65, 80, 128, 130, 97)


def long_walk_corpus(width=130):
    """40 vertices, 10 walks of `width` with the lengths LONG_LENS (capped at the width)."""
    return uniform_corpus(40, len(LONG_LENS), width, 77, [min(x, width) for x in LONG_LENS])


# (dim, window, K, epochs, sample); the GPU parity test reuses them
CASES = [(8, 3, 2, 2, 0.0), (100, 1, 5, 1, 0.01), (8, 3, 0, 1, 0.0)]


def train_lib(W, n, dim, window, K, epochs, sample, seed=5, device=-1, concurrency=1, **extra):
    """Train with the library; returns (syn0, syn1neg, stats tuple, sampler tables, counts).  `extra`: further
    gw_sgns_params_t fields (alpha, min_alpha)."""
    from gwamd.embed import SGNS
    m = SGNS(n, device=device, dim=dim, window=window, negative=K, epochs=epochs, sample=sample, seed=seed, **extra)
    if device >= 0:
        import torch
        Wd = torch.as_tensor(W, device=f"cuda:{device}")
        wp = ctypes.c_void_p(Wd.data_ptr())
    else:
        wp = ctypes.c_void_p(W.ctypes.data)
    m.build_vocab(wp, W.shape[0], W.shape[1])
    tables = m.sampler()
    st = m.train(wp, W.shape[0], W.shape[1], 0, epochs, concurrency)
    syn0, syn1, cnt = m.export()
    m.free()
    return syn0, syn1, st.as_tuple(), tables, cnt


def restate(W, n, dim, window, K, epochs, sample, seed, tables, dtype):
    """The law, sequentially, in numpy.  dtype float64: np.dot; float32: products summed in index order."""
    J, thr, keep_thr = tables
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    expt = np.array([np.exp((i / 1000 * 2 - 1) * 6.0) for i in range(1000)])
    expt = (expt / (expt + 1)).astype(np.float32)
    rows = [(v, 0, d, 0, k0, k1 ^ TAG_INIT) for v in range(n) for d in range(dim)]
    u = philox(rows)[:, 0].astype(np.float64) * 2.0 ** -32
    syn0 = ((u - 0.5) / dim).astype(np.float32).reshape(n, dim).astype(dtype)
    syn1 = np.zeros((n, dim), dtype)
    nwalks = W.shape[0]
    st = [0, 0, 0, 0, 0]

    def dot(a, b):
        if dtype == np.float64:
            return float(np.dot(a, b))
        return float(np.cumsum(a * b, dtype=np.float32)[-1])

    for e in range(epochs):
        for w in range(nwalks):
            alpha = np.float32(0.025 - (0.025 - 0.0001) * ((e * nwalks + w) / (epochs * nwalks)))
            alpha = dtype(alpha)
            ids = []
            for i, v in enumerate(W[w]):
                if v == -1:
                    break
                ids.append((i, int(v)))
            if not ids:
                continue
            dr = philox([(w, 0, i, e, k0, k1 ^ TAG_TOK) for i, _ in ids])
            kept = [(i, v, int(dr[r, 1]) % window) for r, (i, v) in enumerate(ids)
                    if int(dr[r, 0]) < int(keep_thr[v]) or int(keep_thr[v]) == 0xFFFFFFFF]
            st[0] += len(kept)
            for i, (pos, centre, b) in enumerate(kept):
                for j in range(max(i - window + b, 0), min(i + window - b, len(kept) - 1) + 1):
                    if j == i:
                        continue
                    slot = j - (i - window)
                    src = kept[j][1]
                    st[1] += 1
                    st[2] += K
                    targets = [(centre, 1.0)]
                    if K:
                        nd = philox([(w, 0, pos, (e << 20) | (slot << 9) | k, k0, k1 ^ TAG_NEG) for k in range(K)])
                        for k in range(K):
                            c = (int(nd[k, 0]) * n) >> 32
                            t = c if int(nd[k, 1]) < int(thr[c]) else int(J[c])
                            if t == centre:
                                st[3] += 1
                            else:
                                targets.append((t, 0.0))
                    l1 = syn0[src].copy()
                    neu = np.zeros(dim, dtype)
                    for t, label in targets:
                        f = dot(l1, syn1[t])
                        if dtype == np.float32:
                            f = np.float32(f)
                        if not (-6.0 < f < 6.0):
                            st[4] += 1
                            continue
                        idx = min(int((dtype(f) + dtype(6.0)) * dtype(EXP_SCALE)), 999)
                        g = dtype((dtype(label) - dtype(expt[idx])) * alpha)
                        neu = neu + g * syn1[t]
                        syn1[t] = syn1[t] + g * l1
                    syn0[src] = l1 + neu
    return syn0, syn1, tuple(st)


def test_vocabulary_and_sampler():
    W, n, _ = golden_walks("n2v_karate_p1_q1_s0.npz")
    sample = 1e-3
    from gwamd.embed import SGNS
    m = SGNS(n, device=-1, dim=4, sample=sample)
    m.build_vocab(ctypes.c_void_p(W.ctypes.data), W.shape[0], W.shape[1])
    J, thr, keep_thr = m.sampler()
    cnt = m.export()[2]
    ref = np.bincount(W[W >= 0], minlength=n)
    assert np.array_equal(cnt, ref)
    # mass per vertex implied by the alias table, exactly, in integers: a draw lands in column k with 1/n and
    # stays with probability thr[k] / 2^32 (a full threshold with J[k] = k keeps everything)
    num = [0] * n
    for k in range(n):
        stay = int(thr[k])
        if stay == 0xFFFFFFFF:
            assert J[k] == k
            stay = 1 << 32
        num[k] += stay
        num[int(J[k])] += (1 << 32) - stay
    mass = np.array([x / (n * 2.0 ** 32) for x in num])
    p = ref.astype(np.float64) ** 0.75
    p /= p.sum()
    # <= n + 1 thresholds contribute to a vertex, each floored by < 2^-32 / n; the rest is fp64 rounding
    assert np.abs(mass - p).max() <= 2.0 ** -31
    T = float(ref.sum())
    keep = np.minimum(1.0, (np.sqrt(ref / (sample * T)) + 1) * (sample * T) / ref)
    assert (keep < 1).any()
    want = np.where(keep >= 1.0, float(0xFFFFFFFF), np.floor(keep * 2.0 ** 32))
    assert np.abs(keep_thr.astype(np.float64) - want).max() <= 1.0


def check_restatement(W, n, case):
    dim, window, K, epochs, sample = case
    syn0, syn1, st, tables, _ = train_lib(W, n, dim, window, K, epochs, sample)
    r64 = restate(W, n, dim, window, K, epochs, sample, 5, tables, np.float64)
    r32 = restate(W, n, dim, window, K, epochs, sample, 5, tables, np.float32)
    assert st[:4] == r64[2][:4] == r32[2][:4]
    ntok = int((np.cumprod(W >= 0, axis=1)).sum()) * epochs
    if sample > 0:
        assert 0.25 * ntok < st[0] < 0.85 * ntok  # subsampling fired
    else:
        assert st[0] == ntok
    assert st[1] > 0 and st[2] == K * st[1]
    # Tolerance: 4 x the largest deviation of the plain-order fp32 restatement from the fp64 one (the
    # library's lane-strided tree is a third order of the same length).  Measured on this corpus
    # (deviation of r32 / of the library, max over syn0 and syn1neg):
    #   dim 8, window 3, K 2, 2 epochs:  r32 2.93e-08, library 2.93e-08
    #   dim 100, window 1, K 5, sample 0.01:  r32 1.30e-09, library 1.30e-09
    #   dim 8, window 3, K 0:  r32 2.89e-08, library 2.89e-08
    dev32 = max(np.abs(r32[0] - r64[0]).max(), np.abs(r32[1] - r64[1]).max())
    devlib = max(np.abs(syn0 - r64[0]).max(), np.abs(syn1 - r64[1]).max())
    print(f"case {case}: fp32 restatement deviates {dev32:.3e}, library {devlib:.3e}, clipped {st[4]}")
    assert dev32 > 0
    assert devlib <= 4 * dev32
    assert np.abs(syn1).max() > 0 and np.abs(syn0 - r64[0]).max() < np.abs(syn0).max()
    return st


@pytest.mark.parametrize("case", CASES, ids=lambda c: "dim%d_w%d_K%d_e%d_s%g" % c)
def test_host_law_matches_restatement(case):
    check_restatement(*barbell_corpus(), case)


# The shapes at which the kernel is compared with the host law beyond its first loop trips (test_sgns_gpu.py):
# rows of more than one 16 B chunk per lane (dim 300: 75 chunks, lanes 0..10 hold two; dim 1024: four on every
# lane), walks longer than 64 positions with subsampling on, and more than 64 negatives per pair.  Measured
# deviation from the fp64 restatement (plain-order fp32 / library):
#   barbell dim 300, window 2, K 2:             1.987e-07 / 1.987e-07
#   barbell dim 1024, window 2, K 2:            5.518e-08 / 5.518e-08
#   long walks dim 8, window 3, K 2, s 0.004:   2.255e-08 / 2.255e-08
#   4 x 30 over 12 vertices, window 2, K 66:    6.224e-06 / 6.224e-06
SHAPE_CASES = [("barbell", (300, 2, 2, 1, 0.0)), ("barbell", (1024, 2, 2, 1, 0.0)), ("long", (8, 3, 2, 1, 0.004)),
               ("k66", (8, 2, 66, 1, 0.0))]


@pytest.mark.parametrize("name,case", SHAPE_CASES, ids=lambda x: x if isinstance(x, str) else "dim%d_w%d_K%d_e%d_s%g" % x)
def test_host_law_matches_restatement_at_kernel_shapes(name, case):
    W, n = {"barbell": barbell_corpus, "long": long_walk_corpus, "k66": lambda: uniform_corpus(12, 4, 30, 21)}[name]()
    st = check_restatement(W, n, case)
    if name == "k66":
        assert st[3] > 0   # negatives equal to the centre were drawn and skipped


def test_word2vec_writer(tmp_path):
    W, n, labels = golden_walks("n2v_karate_p1_q1_s0.npz")
    from gwamd.embed import learn_embeddings
    emb = learn_embeddings(W, labels, dimensions=128, window_size=10, iter=1, device=-1)
    path = str(tmp_path / "karate.emb")
    emb.save_word2vec_format(path)
    lines = open(path).read().split("\n")
    assert lines[-1] == "" and lines[0] == "34 128" and len(lines) == 36
    fixture = open(os.path.join(DATA, "karate.emb")).read().split("\n")
    shape = re.compile(r"^\d+( -?\d+\.\d{6}){128}$")
    assert fixture[0] == "34 128" and all(shape.match(l) for l in fixture[1:35])
    assert all(shape.match(l) for l in lines[1:35])
    order = [int(l.split(" ")[0]) for l in lines[1:35]]
    cnt = {int(labels[v]): int(emb.counts[v]) for v in range(n)}
    assert order == sorted(cnt, key=lambda l: (-cnt[l], l))
    assert emb.index2word == [str(l) for l in order]
    # node2vec/src/classify.py:81-93 read_embedding: split on " ", float()
    num, dimension = int(lines[0].split(" ")[0]), int(lines[0].split(" ")[1])
    got = {}
    for line in lines[1:1 + num]:
        words = line.split(" ")
        got[int(words[0])] = [float(x) for x in words[1:]]
    assert dimension == 128
    for v in range(n):
        assert np.abs(np.array(got[int(labels[v])]) - emb.vectors[v].astype(np.float64)).max() <= 5e-7
        assert np.array_equal(emb[int(labels[v])], emb.vectors[v])
    assert np.abs(emb.vectors).max() > 0.5 / 128  # trained: left the initial range


def test_list_of_lists_input_matches_array_input():
    W, n, labels = golden_walks("n2v_directed_sinks_p0.5_q2_s3.npz")
    from gwamd.embed import learn_embeddings
    lists = [[int(labels[v]) for v in row if v >= 0] for row in W]
    a = learn_embeddings(lists, labels, dimensions=12, window_size=2, iter=1, device=-1)
    b = learn_embeddings(W, labels, dimensions=12, window_size=2, iter=1, device=-1)
    assert np.array_equal(a.vectors, b.vectors) and a.stats.as_tuple() == b.stats.as_tuple()


def test_errors_and_struct_size():
    C = _C()
    L = C.lib()

    def create(**kw):
        p = C.SgnsParams(**kw)
        h = ctypes.c_void_p()
        rc = L.gw_sgns_create(-1, 12, ctypes.byref(p), ctypes.byref(h))
        if rc == 0:
            L.gw_sgns_free(h)
        return rc

    assert create() == C.GW_OK
    for bad in (dict(dim=0), dict(dim=1025), dict(window=0), dict(negative=-1)):
        assert create(**bad) == C.GW_ERR_INVALID
        assert L.gw_sgns_last_error(None)
    W, n = barbell_corpus()
    h = ctypes.c_void_p()
    assert L.gw_sgns_create(-1, n, None, ctypes.byref(h)) == 0
    st = C.SgnsStats()
    assert L.gw_sgns_train(h, C.ptr(W), 24, 10, 0, 1, 1, ctypes.byref(st), None) == C.GW_ERR_STATE
    assert b"build_vocab" in L.gw_sgns_last_error(h)
    out = np.empty((n, 128), np.float32)
    assert L.gw_sgns_export(h, C.ptr(out), None, None) == C.GW_ERR_STATE
    bad = W.copy()
    bad[2, 3] = n
    assert L.gw_sgns_build_vocab(h, C.ptr(bad), 24, 10) == C.GW_ERR_RANGE
    bad[2, 3] = -2
    assert L.gw_sgns_build_vocab(h, C.ptr(bad), 24, 10) == C.GW_ERR_RANGE
    assert L.gw_sgns_build_vocab(h, C.ptr(W), 24, 10) == 0
    assert L.gw_sgns_train(h, C.ptr(W), 24, 10, 4, 2, 1, None, None) == C.GW_ERR_INVALID  # past the 5 epochs
    assert L.gw_sgns_train(h, C.ptr(W), 24, 10, 0, 1, 1, ctypes.byref(st), None) == 0 and st.pairs > 0
    L.gw_sgns_free(h)
    # a caller compiled against a shorter struct: only its bytes are read, the rest keeps the defaults
    p = C.SgnsParams(dim=16, window=2, negative=3, epochs=7, alpha=123.0, sample=0.5, seed=99)
    p.struct_size = C.SgnsParams.window.offset + 4  # struct_size, dim, window
    assert L.gw_sgns_create(-1, n, ctypes.byref(p), ctypes.byref(h)) == 0
    assert L.gw_sgns_build_vocab(h, C.ptr(W), 24, 10) == 0
    ptr, pitch = ctypes.c_void_p(), ctypes.c_int64()
    assert L.gw_sgns_vectors_dev(h, ctypes.byref(ptr), ctypes.byref(pitch)) == 0 and pitch.value == 16 and ptr.value
    assert L.gw_sgns_train(h, C.ptr(W), 24, 10, 5, 1, 1, None, None) == C.GW_ERR_INVALID  # epochs stayed 5, not 7
    st = C.SgnsStats()
    assert L.gw_sgns_train(h, C.ptr(W), 24, 10, 0, 1, 1, ctypes.byref(st), None) == 0
    assert st.negatives == 5 * st.pairs  # negative stayed 5, not 3
    ref = np.empty((n, 16), np.float32)
    assert L.gw_sgns_export(h, C.ptr(ref), None, None) == 0 and np.isfinite(ref).all()  # alpha stayed 0.025
    L.gw_sgns_free(h)
    p.struct_size = 2
    assert L.gw_sgns_create(-1, n, ctypes.byref(p), ctypes.byref(h)) == C.GW_ERR_INVALID
