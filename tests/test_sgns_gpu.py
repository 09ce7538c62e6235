"""GPU: the SGNS training kernel (gw_sgns.hip) against the host evaluation of
the same law (device = -1), its independence from the launch geometry, that
concurrent (Hogwild) training learns, and the CLI end to end."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import DATA, PKG
from test_sgns_host import CASES, barbell_corpus, golden_walks, train_lib

pytestmark = pytest.mark.gpu


def _parity_cases():
    out = [("barbell", c) for c in CASES]
    out += [("barbell", (128, 2, 3, 1, 0.0)), ("barbell", (192, 2, 3, 1, 0.0)),  # 192: two row chunks on some lanes
            ("barbell", (301, 2, 2, 1, 0.0)),                                    # pitch 304: a ragged second chunk
            ("sinks", (20, 4, 5, 2, 1e-3))]                                     # rows that end early
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
