"""GPU: the SGNS training kernel (gw_sgns.hip) against the host evaluation of
the same law (device = -1) - on toy shapes and past the first trip of every
chunked loop (walk length, row chunks, negatives, epochs, waves) -, its
independence from the launch geometry, that concurrent (Hogwild) training
learns, and the CLI end to end."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import DATA, PKG
from test_sgns_host import CASES, barbell_corpus, golden_walks, long_walk_corpus, train_lib, uniform_corpus

pytestmark = pytest.mark.gpu


def _parity_cases():
    out = [("barbell", c) for c in CASES]
    out += [("barbell", (128, 2, 3, 1, 0.0)), ("barbell", (192, 2, 3, 1, 0.0)),  # 192: 48 chunks of 16 B, still NCH = 1
            ("barbell", (301, 2, 2, 1, 0.0)),                                    # pitch 304: a ragged second chunk
            ("sinks", (20, 4, 5, 2, 1e-3))]                                     # rows that end early
    # 16 B chunks per lane (k_sgns_train<NCH>): 256 fills NCH = 1; 257 and 260 are one chunk into NCH = 2 (pitch
    # 260, lane 0 alone holds two); 512 fills it; 513 / 768: NCH = 3; 769 / 1024: NCH = 4
    out += [("barbell", (dim, 2, 2, 1, 0.0)) for dim in (256, 257, 260, 512, 513, 768, 769, 1024)]
    return out


def _corpus(name):
    if name == "barbell":
        return barbell_corpus()
    W, n, _ = golden_walks("n2v_directed_sinks_p0.5_q2_s3.npz")
    return np.ascontiguousarray(W[:64]), n


@pytest.mark.parametrize("name,case", _parity_cases(), ids=lambda x: x if isinstance(x, str) else "d%d_w%d_K%d_e%d_s%g" % x)
def test_sequential_parity_with_host_law(name, case):
    """concurrency = 1 runs the same kernel code as any other launch and must equal the host law bit for bit."""
    W, n = _corpus(name)
    assert W.shape[0] <= 64 and W.shape[1] <= 20
    h0, h1, hst, _, hc = train_lib(W, n, *case, device=-1)
    d0, d1, dst, _, dc = train_lib(W, n, *case, device=0, concurrency=1)
    assert np.array_equal(hc, dc)
    assert dst == hst and hst[1] > 0
    assert np.array_equal(d0, h0)
    assert np.array_equal(d1, h1)
    assert np.abs(h1).max() > 0


# ---- past the first trip of every loop of k_sgns_train -------------------------------
def assert_parity(W, n, case, concurrency=1, **extra):
    """The kernel against the host law as in test_sequential_parity_with_host_law: counts, all five stats, syn0
    and syn1neg.  Returns the host's stats."""
    h0, h1, hst, _, hc = train_lib(W, n, *case, device=-1, **extra)
    d0, d1, dst, _, dc = train_lib(W, n, *case, device=0, concurrency=concurrency, **extra)
    assert np.array_equal(hc, dc)
    assert dst == hst and hst[1] > 0
    assert np.array_equal(d0, h0)
    assert np.array_equal(d1, h1)
    assert np.abs(h1).max() > 0
    return hst


def tokens(W):
    return int(np.cumprod(W >= 0, axis=1).sum())


@pytest.mark.parametrize("sample", [0.0, 0.004])
@pytest.mark.parametrize("window", [3, 10])
@pytest.mark.parametrize("width", [130, 64, 65, 80])
def test_long_walks(width, window, sample):
    """Walks of 0, 1, 63, 64, 65, 80, 97, 128 and 130 tokens: the kept sequence is compacted 64 positions at a
    time, so these take the second and third trip, the running offset into LDS, and a walk that ends exactly at a
    trip's edge.  The width is the row stride, so 64, 65 and 80 are matrices of their own."""
    W, n = long_walk_corpus(width)
    st = assert_parity(W, n, (8, window, 2, 1, sample))
    if sample > 0:
        assert 0.25 * tokens(W) < st[0] < 0.85 * tokens(W)   # subsampling fired (130 wide: 58 % kept)
    else:
        assert st[0] == tokens(W)


def test_longest_walk():
    """walk_len = 2048 is the most the kernel takes: 64 KB of dynamic LDS.  One more is refused on the device and
    accepted by the host evaluation."""
    from gwamd import _lib as C
    from gwamd.embed import SGNS
    import torch
    W, n = uniform_corpus(40, 4, 2048, 3, [2048, 2047, 1000, 2048])
    assert_parity(W, n, (8, 2, 1, 1, 0.0))
    m = SGNS(n, device=0, dim=8, window=2, negative=1, epochs=1)
    static = m.kernel_attrs(1)["lds_bytes"] - 4 * 2 * 1 * 4
    assert static >= 0 and m.kernel_attrs(2048)["lds_bytes"] == 65536 + static
    W1, _ = uniform_corpus(40, 4, 2049, 3)
    Wd = torch.as_tensor(W1, device="cuda:0")
    m.build_vocab(ctypes.c_void_p(Wd.data_ptr()), 4, 2049)
    with pytest.raises(C.UnsupportedError, match="2049"):
        m.train(ctypes.c_void_p(Wd.data_ptr()), 4, 2049, 0, 1, 1)
    m.free()
    st = train_lib(W1, n, 8, 2, 1, 1, 0.0, device=-1)[2]
    assert st[0] == 4 * 2049


@pytest.mark.parametrize("dim", [128, 512, 768, 1024])
def test_kernel_attrs_of_every_chunk_count(dim):
    """k_sgns_train<1..4>: what hipFuncGetAttributes reports (printed; DESIGN section 10 records it).  Measured on
    the MI355X: 59 / 75 / 93 / 109 VGPRs at NCH = 1 / 2 / 3 / 4, no scratch, no static LDS."""
    from gwamd.embed import SGNS
    m = SGNS(12, device=0, dim=dim)
    a = m.kernel_attrs(80)
    m.free()
    print(f"dim {dim}: NCH {(dim // 4 + 63) // 64}, {a}")
    assert a["scratch_bytes"] == 0 and 0 < a["vgprs"] <= 128 and a["lds_bytes"] == 4 * 2 * 80 * 4


@pytest.mark.parametrize("n,K", [(12, 64), (12, 65), (12, 130), (12, 511), (200, 130)])
def test_many_negatives(n, K):
    """Negatives are drawn 64 at a time: K = 64 fills one draw, 65 and 130 redraw once and twice with a ragged
    tail, 511 is the law's most.  Over 12 vertices one negative in twelve equals the centre and is skipped, and
    equal negatives follow each other (the row carried over in registers)."""
    W, _ = uniform_corpus(n, 16, 20, 31)
    st = assert_parity(W, n, (8, 2, K, 1, 0.0))
    assert st[2] == K * st[1] and st[3] > 0


@pytest.mark.parametrize("n,nwalks,K,epochs,alpha", [(12, 24, 5, 3, 0.5), (200, 16, 130, 1, 0.025)])
def test_parity_where_targets_are_clipped(n, nwalks, K, epochs, alpha):
    """Dot products past +-6, so that the skipped-target branch runs on both sides: alpha = 0.5 over 3 epochs
    (32 of 32,262 targets on the host), and 130 negatives per pair at the default alpha (711 of 161,916)."""
    W, _ = uniform_corpus(n, nwalks, 20, 41)
    st = assert_parity(W, n, (8, 3, K, epochs, 0.0), alpha=alpha)
    print(f"n {n} K {K}: {st[4]} clipped targets")
    assert st[4] > 0


@pytest.mark.parametrize("nwalks,width", [(16, 20), (2, 600)])
def test_window_at_its_limit(nwalks, width):
    """window = GW_SGNS_MAX_WINDOW: the window draw takes every value below 1023 and both clamps of the pair
    range act on every centre.  On walks of 20 the pair slots stay near 1023; the 600-token walk spreads them
    over 424..1622, into the top bit of the 11-bit slot field of the negative draw's counter."""
    W, n = uniform_corpus(12, nwalks, width, 51, [width, width - 13][:nwalks])
    st = assert_parity(W, n, (8, 1023, 1, 1, 0.0))
    assert st[1] > (width - 13) * (width - 14) // 4


def _train_calls(W, n, device, calls, **params):
    """build_vocab, then one train call per (epoch_begin, epoch_count); (syn0, syn1neg, [stats tuple per call])."""
    import torch
    from gwamd.embed import SGNS
    m = SGNS(n, device=device, **params)
    Wd = torch.as_tensor(W, device="cuda:0") if device >= 0 else W
    wp = ctypes.c_void_p(Wd.data_ptr() if device >= 0 else W.ctypes.data)
    m.build_vocab(wp, W.shape[0], W.shape[1])
    stats = [m.train(wp, W.shape[0], W.shape[1], b, c, 1).as_tuple() for b, c in calls]
    syn0, syn1, _ = m.export()
    m.free()
    return syn0, syn1, stats


def test_split_epochs():
    """epochs = 3: train(0, 1) then train(1, 2) gives the bits of train(0, 3), on the device and on the host, and
    the stats of the two calls add up to the one call's."""
    W, n = barbell_corpus()
    kw = dict(dim=8, window=3, negative=2, epochs=3, sample=0.01, seed=5)
    runs = [_train_calls(W, n, dev, calls, **kw) for dev in (-1, 0) for calls in ([(0, 3)], [(0, 1), (1, 2)])]
    ref = runs[0]
    assert len(ref[2][0]) == 5 and ref[2][0][1] > 0
    for s0, s1, stats in runs:
        assert np.array_equal(s0, ref[0]) and np.array_equal(s1, ref[1])
        assert tuple(sum(x) for x in zip(*stats)) == ref[2][0]
    one = _train_calls(W, n, 0, [(0, 1)], **kw)
    assert not np.array_equal(one[0], ref[0])   # the later epochs did train


def disjoint_corpus(c, nwalks, width, per=8):
    """Walk w visits only the vertices [per * (w % c), per * (w % c + 1)): wave w % c of c owns them."""
    W = np.random.RandomState(61).randint(0, per, (nwalks, width)).astype(np.int32)
    W += ((np.arange(nwalks) % c) * per).astype(np.int32)[:, None]
    W[1, 7:] = -1
    return W, c * per


@pytest.mark.parametrize("c,nwalks,conc", [(2, 23, 2), (5, 23, 5), (6, 23, 6), (7, 7, 100)])
def test_concurrent_waves_on_disjoint_rows(c, nwalks, conc):
    """concurrency = c over c disjoint vertex sets, walk w inside set w % c, no negatives: wave w % c alone
    touches its set's rows, in the law's order, so the launch equals the host law bit for bit.  The walk count
    is no multiple of c; 5 and 6 waves need a second workgroup with idle waves; 100 waves for 7 walks are clamped
    to 7 (one walk and one set each)."""
    assert nwalks % c or conc > nwalks
    W, n = disjoint_corpus(c, nwalks, 20)
    st = assert_parity(W, n, (8, 3, 0, 2, 0.005), concurrency=conc)
    assert 0 < st[0] < 2 * tokens(W)   # subsampling is on


def test_range_errors_past_the_first_64_positions():
    """An id >= n at position 70 of 80 fails build_vocab, and train on a corpus other than the counted one, on the
    device as on the host; after an earlier -1 it is not part of the walk."""
    import torch
    from gwamd.embed import SGNS
    W, n = uniform_corpus(40, 6, 80, 71)
    bad = W.copy()
    bad[3, 70] = n
    for device in (-1, 0):
        keep = [torch.as_tensor(x, device="cuda:0") if device >= 0 else x for x in (W, bad)]
        good_p, bad_p = (ctypes.c_void_p(x.data_ptr() if device >= 0 else x.ctypes.data) for x in keep)
        m = SGNS(n, device=device, dim=8, window=3, negative=2, epochs=1)
        with pytest.raises(IndexError):
            m.build_vocab(bad_p, 6, 80)
        m.build_vocab(good_p, 6, 80)
        with pytest.raises(IndexError):
            m.train(bad_p, 6, 80, 0, 1, 1)
        m.free()
    for end in (66, 10):   # a -1 in the same 64 positions as the id, and in the trip before
        cut = bad.copy()
        cut[3, end] = -1
        st = assert_parity(cut, n, (8, 3, 2, 1, 0.0))
        assert st[0] == tokens(cut) == 5 * 80 + end


def test_draws_do_not_depend_on_geometry():
    W, n, _ = golden_walks("n2v_directed_sinks_p0.5_q2_s3.npz")
    case = (16, 3, 5, 2, 1e-3)
    ref = train_lib(W, n, *case, device=-1)[2]
    for conc in (1, 7, 0):
        st = train_lib(W, n, *case, device=0, concurrency=conc)[2]
        assert st[:4] == ref[:4], (conc, st, ref)
    assert ref[0] > 0 and ref[3] > 0


# ---- concurrent training learns -----------------------------------------------------
B, S = 32, 64  # planted partition: 32 blocks of 64 vertices


def planted_partition(seed=7):
    """Intra-block degree about 8, inter-block about 1."""
    rng = np.random.RandomState(seed)
    n = B * S
    src, dst = [], []
    for v in range(n):
        for _ in range(4):
            u = (v // S) * S + rng.randint(S)
            if u != v:
                src.append(v)
                dst.append(u)
    for _ in range(n // 2):
        a, b = rng.randint(n), rng.randint(n)
        if a // S != b // S:
            src.append(a)
            dst.append(b)
    return np.array(src, np.int64), np.array(dst, np.int64), n


def block_share(syn0, block):
    x = syn0 / np.maximum(np.linalg.norm(syn0, axis=1, keepdims=True), 1e-30)
    c = x @ x.T
    np.fill_diagonal(c, -2.0)
    nn = c.argmax(1)
    return float(np.mean(block[nn] == block))


def objective(syn0, syn1, pos, neg):
    """Mean SGNS loss of fixed (input, target) pairs with fixed negatives."""
    def logsig(x):
        return -np.logaddexp(0.0, -x)
    u = syn0[pos[:, 0]].astype(np.float64)
    lp = logsig(np.einsum("ij,ij->i", u, syn1[pos[:, 1]].astype(np.float64)))
    ln = logsig(-np.einsum("ij,ikj->ik", u, syn1[neg].astype(np.float64))).sum(1)
    return float(-(lp + ln).mean())


def test_concurrent_training_learns(gw):
    import torch
    from gwamd import _lib as C
    from gwamd.embed import SGNS
    src, dst, n = planted_partition()
    g = gw.GWGraph.from_edges(src, dst).to_device(0)
    assert g.n == n
    C.check(C.lib().gw_n2v_prepare(g.handle, 1.0, 1.0, C.N2V_REJECTION), g.handle)
    nw, L = 4 * n, 20
    Wd = torch.empty((nw, L), dtype=torch.int32, device="cuda:0")
    C.check(C.lib().gw_n2v_walks(g.handle, L, 11, 0, nw, 1, C.ptr(Wd), None, None, None), g.handle)
    torch.cuda.synchronize()
    W = Wd.cpu().numpy()
    block = np.asarray(g.export_csr()["labels"]) // S  # dense id -> block
    rng = np.random.RandomState(2)
    rows, cols = rng.randint(nw, size=4096), rng.randint(L - 1, size=4096)
    pos = np.stack([W[rows, cols], W[rows, cols + 1]], 1)
    pos = pos[(pos >= 0).all(1)]
    neg = rng.randint(n, size=(len(pos), 5))
    # 2 epochs: chosen on the host as the count at which the sequential run alone reaches a share >= 0.9
    # (1 epoch: 0.83, 2 epochs: 1.00 on uniform walks over this graph)
    epochs = 2
    kw = dict(dim=32, window=5, negative=5, epochs=epochs, seed=3)
    res = {}
    for dev in (-1, 0):
        m = SGNS(n, device=dev, **kw)
        wp = ctypes.c_void_p(W.ctypes.data if dev < 0 else Wd.data_ptr())
        m.build_vocab(wp, nw, L)
        s0, s1, _ = m.export()
        init = objective(s0, s1, pos, neg)
        conc = m.auto_concurrency(nw)
        st = m.train(wp, nw, L, 0, epochs, 0)
        s0, s1, _ = m.export()
        res[dev] = (init, objective(s0, s1, pos, neg), block_share(s0, block), st.as_tuple(), conc)
        m.free()
    (i_h, o_h, sh_h, st_h, _), (i_d, o_d, sh_d, st_d, conc) = res[-1], res[0]
    print(f"objective {i_h:.4f} -> host {o_h:.4f}, device {o_d:.4f}; share host {sh_h:.3f}, device {sh_d:.3f}; "
          f"auto concurrency {conc}")
    assert conc == n // 32  # the auto rule: never more than one wave per 32 vertices
    assert st_d[:4] == st_h[:4]
    assert i_d == i_h and sh_h >= 0.9
    assert i_d - o_d >= 0.5 * (i_h - o_h)
    assert sh_d >= 0.8 * sh_h


# ---- end to end ----------------------------------------------------------------------
def _cli(args, cwd):
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "gwamd.cli"] + args, cwd=cwd, env=env, capture_output=True, text=True,
                          timeout=300)


def test_cli_edgelist_to_emb(tmp_path):
    common = ["--mode", "scale", "--input", os.path.join(DATA, "karate.edgelist"), "--delimiter", " "]
    a = _cli(common + ["--walks", "a.txt", "--output", "X.emb", "--dimensions", "16", "--iter", "2"], str(tmp_path))
    assert a.returncode == 0, a.stderr[-2000:]
    b = _cli(common + ["--walks", "b.txt"], str(tmp_path))
    assert b.returncode == 0, b.stderr[-2000:]
    assert open(tmp_path / "a.txt", "rb").read() == open(tmp_path / "b.txt", "rb").read()
    lines = open(tmp_path / "X.emb").read().split("\n")
    assert lines[0] == "34 16" and lines[-1] == "" and len(lines) == 36
    assert sorted(int(l.split(" ")[0]) for l in lines[1:35]) == list(range(1, 35))
    vals = np.array([[float(x) for x in l.split(" ")[1:]] for l in lines[1:35]])
    assert vals.shape == (34, 16) and np.isfinite(vals).all() and np.abs(vals).max() > 0.5 / 16


def test_learn_embeddings_trains_the_device_tensor_in_place():
    import torch
    from gwamd.embed import learn_embeddings
    W, n, labels = golden_walks("n2v_karate_p1_q1_s0.npz")
    Wd = torch.as_tensor(W, device="cuda:0")
    emb = learn_embeddings(Wd, labels, dimensions=24, window_size=4, iter=1, seed=1)
    assert emb.walks_ptr == Wd.data_ptr()  # the trainer read the tensor itself: no host copy, no device copy
    ptr, pitch = emb.model.vectors_dev()
    assert pitch == 24 and ptr
    # syn0 is device memory: torch wraps it without a copy
    dev = emb.model.vectors_torch()
    assert dev.is_cuda and dev.data_ptr() == ptr and tuple(dev.shape) == (n, 24) and dev.stride(0) == pitch
    assert np.array_equal(dev.cpu().numpy(), emb.vectors)
    assert np.array_equal(emb[int(labels[0])], emb.vectors[0])
    host_emb = learn_embeddings(W, labels, dimensions=24, window_size=4, iter=1, seed=1, device=-1)
    assert host_emb.stats.as_tuple()[:4] == emb.stats.as_tuple()[:4]


def test_device_range_errors_and_kernel_attrs():
    import torch
    from gwamd.embed import SGNS
    W, n = barbell_corpus()
    bad = W.copy()
    bad[5, 2] = n
    Wd, Bd = torch.as_tensor(W, device="cuda:0"), torch.as_tensor(bad, device="cuda:0")
    m = SGNS(n, device=0, dim=8, window=3, negative=2, epochs=1)
    with pytest.raises(IndexError):
        m.build_vocab(ctypes.c_void_p(Bd.data_ptr()), 24, 10)
    with pytest.raises(Exception, match="build_vocab"):
        m.train(ctypes.c_void_p(Wd.data_ptr()), 24, 10)
    m.build_vocab(ctypes.c_void_p(Wd.data_ptr()), 24, 10)
    with pytest.raises(IndexError):  # a corpus other than the counted one: the kernel ends the walk at the bad id
        m.train(ctypes.c_void_p(Bd.data_ptr()), 24, 10)
    a = m.kernel_attrs(10)
    assert a["scratch_bytes"] == 0 and 0 < a["vgprs"] <= 128 and a["lds_bytes"] == 4 * 2 * 10 * 4
    m.free()
