"""GPU: the one-vs-rest kernels (gw_ovr.hip) against the host evaluation of the
same law (device = -1): bit parity of the weights, the decision values, the
Newton counts and the counts at the kernels' edges, zero-copy scoring of the
SGNS and DeepSim trainers' vectors, the kernel attributes and determinism.
"""
import ctypes

import numpy as np
import pytest

from test_ovr_host import csr, planted, scorer

pytestmark = pytest.mark.gpu

RB, LC, JT = 64, 32, 64   # GW_OVR_RB (the law's row block); the pass kernel's label chunk and column tile


def shaped(T, d, L, seed):
    """n = T + 37 rows; column L-1 absent from training and column L-2 on every training row (L >= 4), so constant
    columns sit beside fitted ones; a held-out row with no label and one with every label; a non-monotone order."""
    n = T + 37
    X, Y = planted(n, d, L, seed, extra=0.2)
    order = np.random.RandomState(seed + 1).permutation(n).astype(np.int64)
    if L >= 4:
        Y[:, L - 1] = False
        Y[order[:T], L - 2] = True
        Y[order[T + 2], L - 1] = True
    Y[order[T]] = False
    Y[order[T + 1]] = True
    return X, Y, order


def padded(X, pad):
    """The features on the device with `pad` NaN floats after every row."""
    import torch
    wide = np.full((X.shape[0], X.shape[1] + pad), np.nan, np.float32)
    wide[:, :X.shape[1]] = X
    return torch.as_tensor(wide, device="cuda:0")


def assert_same(dev, host, order, T):
    ed, eh = dev.export(), host.export()
    assert np.array_equal(ed["state"], eh["state"])
    assert np.array_equal(ed["newton_iters"], eh["newton_iters"])
    assert np.array_equal(ed["W"].view(np.uint64), eh["W"].view(np.uint64))
    assert np.array_equal(ed["gnorm"].view(np.uint64), eh["gnorm"].view(np.uint64))
    rows = np.concatenate([order[T:], order[:5]])
    assert np.array_equal(dev.decision(rows).view(np.uint64), host.decision(rows).view(np.uint64))
    cd, ch = dev.score(order[T:]), host.score(order[T:])
    assert np.array_equal(cd, ch)
    return eh, ch


# train_count at the row block's edges and past it, dim at the 16 B chunk's and the column tile's edges and at the
# device limit, L at the label chunk's edges and past it (see DESIGN §12 for what each value leaves)
PARITY = [
    (1, 5, 3, 0),
    (63, 1, 1, 0),
    (64, 3, 2, 1),
    (65, 4, 39, 3),
    (130, 5, 63, 0),
    (257, 127, 64, 1),
    (130, 128, 65, 0),
    (65, 129, 130, 2),
    (130, 256, LC + 1, 0),
    (65, 257, 7, 3),
    (257, 1024, 5, 0),
    (2 * RB, JT, LC, 0),
    (2 * RB + 1, JT + 1, LC - 1, 1),
]


@pytest.mark.parametrize("T,d,L,pad", PARITY)
def test_kernel_equals_host_bitwise(T, d, L, pad):
    X, Y, order = shaped(T, d, L, seed=T + d + L)
    host = scorer(X, Y)
    dev = scorer(padded(X, pad), Y, device=0, dim=d)
    sh, sd = host.fit(order, T), dev.fit(order, T)
    assert (sd.passes, sd.fitted, sd.constant, sd.not_converged, sd.newton_max) == \
        (sh.passes, sh.fitted, sh.constant, sh.not_converged, sh.newton_max)
    eh, counts = assert_same(dev, host, order, T)
    if T > 1 and L >= 4:
        from gwamd import _lib as C
        assert eh["state"][L - 1] == C.OVR_CONST_NEG and eh["state"][L - 2] == C.OVR_CONST_POS
        assert (eh["state"][:L - 2] == C.OVR_FITTED).any()
    assert counts.sum() > 0
    # a second fit on the same handles, over fewer rows: nothing of the first is left behind
    T2 = max(1, T // 2)
    host.fit(order[::-1].copy(), T2)
    dev.fit(order[::-1].copy(), T2)
    assert_same(dev, host, order[::-1].copy(), T2)


def test_frozen_label_beside_a_running_one():
    """Labels that stop after different Newton counts: the earlier ones are skipped by the later passes."""
    X, Y = planted(100, 16, 7, 1)
    order = np.arange(100, dtype=np.int64)
    host, dev = scorer(X, Y), scorer(X, Y, device=0)
    host.fit(order, 100)
    dev.fit(order, 100)
    eh, _ = assert_same(dev, host, order, 100)
    assert eh["newton_iters"].min() < eh["newton_iters"].max()
    one = scorer(X, Y, device=0, max_newton=1)
    ref = scorer(X, Y, max_newton=1)
    one.fit(order, 100)
    ref.fit(order, 100)
    assert_same(one, ref, order, 100)


def test_two_fits_on_fresh_handles_are_identical():
    X, Y, order = shaped(200, 33, 9, 5)
    out = []
    for _ in range(2):
        m = scorer(X, Y, device=0)
        m.fit(order, 200)
        out.append((m.export()["W"].copy(), m.decision(order[200:]).copy(), m.score(order[200:])))
        m.free()
    assert np.array_equal(out[0][0].view(np.uint64), out[1][0].view(np.uint64))
    assert np.array_equal(out[0][1].view(np.uint64), out[1][1].view(np.uint64))
    assert np.array_equal(out[0][2], out[1][2])


def test_kernel_attrs():
    """The pass kernel keeps its accumulators in registers: 0 B scratch at dim 128 and at dim 1024."""
    for d in (128, 1024):
        X, Y = planted(10, d, 3, 0)
        a = scorer(X, Y, device=0).kernel_attrs()
        assert set(a) == {"k_ovr_pass", "k_ovr_reduce", "k_ovr_step", "k_ovr_decision", "k_ovr_count"}
        print(d, a)
        assert a["k_ovr_pass"]["scratch_bytes"] == 0
        assert 0 < a["k_ovr_pass"]["lds_bytes"] <= 64 * 1024 and a["k_ovr_step"]["lds_bytes"] == 7 * (d + 1) * 8
        assert all(v["vgprs"] > 0 for v in a.values())


def block_scores(K, x, block, nblocks, device, seed):
    """micro-F1 of `x` scored on the block labels and on the same labels permuted."""
    n = len(block)
    out = []
    for lab in (block, np.random.RandomState(seed).permutation(block)):
        Y = np.zeros((n, nblocks), bool)
        Y[np.arange(n), lab] = True
        m = K.OneVsRest(n, nblocks, device=device, dim=x.shape[1])
        m.set_features(x)
        m.set_labels(*csr(Y))
        o = K.order(seed, 0, n)
        m.fit(o, n // 2)
        counts = m.score(o[n // 2:])
        out.append((counts, K.f1_from_counts(counts)["micro"]))
        m.free()
    return out


def test_zero_copy_sgns(gw):
    import torch
    from gwamd import _lib as C
    from gwamd import classify as K
    from gwamd.embed import SGNS
    from test_sgns_gpu import S, planted_partition
    src, dst, n = planted_partition()
    g = gw.GWGraph.from_edges(src, dst).to_device(0)
    C.check(C.lib().gw_n2v_prepare(g.handle, 1.0, 1.0, C.N2V_REJECTION), g.handle)
    nw, L = 4 * n, 20
    Wd = torch.empty((nw, L), dtype=torch.int32, device="cuda:0")
    C.check(C.lib().gw_n2v_walks(g.handle, L, 11, 0, nw, 1, C.ptr(Wd), None, None, None), g.handle)
    torch.cuda.synchronize()
    block = np.asarray(g.export_csr()["labels"]) // S
    m = SGNS(n, device=0, dim=32, window=5, negative=5, epochs=2, seed=3)
    wp = ctypes.c_void_p(Wd.data_ptr())
    m.build_vocab(wp, nw, L)
    m.train(wp, nw, L, 0, 2, 0)
    x = m.vectors_torch()
    assert x.data_ptr() == m.vectors_dev()[0]
    syn0 = m.export()[0]
    (cd, f_true), (_, f_perm) = block_scores(K, x, block, n // S, 0, 5)
    (ch, _), _ = block_scores(K, syn0, block, n // S, -1, 5)
    assert np.array_equal(cd, ch)
    print(f"micro-F1 on the block labels {f_true:.3f}, on permuted labels {f_perm:.3f}")
    assert f_true > f_perm
    # the Embedding object is scored where its trainer holds it
    res = K.scoring(x, csr(np.eye(n // S, dtype=bool)[block]), training_percents=[0.5], number_shuffles=1, seed=5)
    assert res[0.5][0]["micro"] == f_true


def test_zero_copy_deepsim():
    from gwamd import classify as K
    from test_deepsim_host import synth, trainer
    V, nblocks = 34, 2
    ids, sc, W = synth(V, topk=7, nwalks=72, L=11, seed=7, short=False)
    m = trainer(V, ids, sc, W, None, device=0, dim=32, window=2, batch=32, seed=7)
    m.train(0, 20, loss=False)
    x = m.vectors_torch()
    w1 = m.export(states=False)["w1"]
    block = (np.arange(V) * nblocks) // V
    (cd, f_true), _ = block_scores(K, x, block, nblocks, 0, 3)
    (ch, f_host), _ = block_scores(K, w1, block, nblocks, -1, 3)
    assert np.array_equal(cd, ch) and f_true == f_host
    res = K.scoring(m, csr(np.eye(nblocks, dtype=bool)[block]), training_percents=[0.5], number_shuffles=1, seed=3)
    assert res[0.5][0]["micro"] == f_true


def _karate_groups(path):
    with open(path, "w") as f:
        for v in range(1, 35):
            f.write(f"{v},{1 + v % 2}\n")
            if v % 5 == 0:
                f.write(f"{v},3\n")


def test_cli_groups_scores_the_embedding(tmp_path, capsys):
    """gwamd.cli --output --groups prints the reference's table after the walks and the embeddings; without
    --groups nothing is printed, as before."""
    import os
    from conftest import DATA
    from gwamd import cli
    grp = str(tmp_path / "groups.csv")
    _karate_groups(grp)
    argv = ["--mode", "scale", "--input", os.path.join(DATA, "karate.edgelist"), "--delimiter", " ", "--walks",
            str(tmp_path / "walks.txt"), "--output", str(tmp_path / "karate.emb"), "--dimensions", "16", "--iter", "1",
            "--walk-length", "20", "--seed", "3"]
    assert cli.main(argv) == 0
    assert capsys.readouterr().out == ""
    assert cli.main(argv + ["--groups", grp]) == 0
    out = capsys.readouterr().out.splitlines()
    i = out.index("Results, using embeddings of dimensionality 16")
    assert i == 2 * 27 and out[i + 2] == "Train percent: 0.1" and out[i + 3].startswith("{'micro': ")
    assert all(0.0 <= float(v) <= 1.0 for v in out[:i])
    assert os.path.getsize(tmp_path / "karate.emb") > 0


def test_deepsim_cli_groups_scores_w1(tmp_path, capsys):
    import os
    from conftest import DATA
    from gwamd import deepsim
    grp, sim = str(tmp_path / "groups.csv"), str(tmp_path / "k.sim.txt")
    _karate_groups(grp)
    rng = np.random.RandomState(0)
    with open(sim, "w") as f:
        for v in range(35):
            ids = rng.permutation(35)[:6]
            sc = np.sort(rng.uniform(0.01, 0.9, 6))[::-1]
            f.write(f"{v}," + ",".join(f"{i}:{s:.6f}" for i, s in zip(ids, sc)) + "\n")
    argv = ["--input", os.path.join(DATA, "karate.edgelist"), "--delimiter", " ", "--simrank_path", sim,
            "--emb_output", str(tmp_path / "k.emb"), "--vertex-num", "35", "--dimensions", "32", "--window-size", "2",
            "--walk-length", "11", "--num-walks", "10", "--steps", "20", "--batch", "32", "--seed", "3",
            "--checkpoint-every", "0"]
    assert deepsim.cli(argv) == 0
    assert capsys.readouterr().out == ""
    assert deepsim.cli(argv + ["--groups", grp]) == 0
    out = capsys.readouterr().out.splitlines()
    i = out.index("Results, using embeddings of dimensionality 32")
    assert i == 2 * 27 and out[i + 2] == "Train percent: 0.1"
