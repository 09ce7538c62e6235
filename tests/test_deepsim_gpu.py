"""GPU: the DeepSim kernels (gw_deepsim.hip) against the host evaluation of the
same law (device = -1): bit parity of every parameter, Adam state and batch
array at the kernel's edges, the reported loss, gradients, determinism,
zero-copy access, a table straight from gw_topsim, the unsupported shapes, the
kernel attributes and the command line end to end.
"""
import os
import subprocess
import sys
import types

import numpy as np
import pytest

from conftest import DATA, PKG, ROOT
from test_deepsim_host import synth, trainer

pytestmark = pytest.mark.gpu

TW = 64   # GW_DS_TW, the law's column-tile width
TENSORS = ("w1", "b1", "w2", "b2")


def corpus(V, k, L, nwalks, seed):
    ids, sc, W = synth(V, topk=7, nwalks=nwalks, L=L, seed=seed, short=False)
    W[1, 2 * k:] = -1        # one token short of 2k+1: never drawn
    W[5, :] = -1
    W[9, k:] = -1
    return ids, sc, W


def pair(V, B, d, k, L, fallback, labelled, seed=7, nwalks=None):
    ids, sc, W = corpus(V, k, L, nwalks or B + 40, seed)
    labels = np.random.RandomState(seed).permutation(V).astype(np.int64) if labelled else None
    kw = dict(dim=d, window=k, batch=B, fallback=fallback, seed=seed, score_scale=0.5)
    return trainer(V, ids, sc, W, labels, device=0, **kw), trainer(V, ids, sc, W, labels, device=-1, **kw)


def assert_state_equal(a, b):
    ea, eb = a.export(), b.export()
    for t in TENSORS:
        assert np.array_equal(ea[t].view(np.uint32), eb[t].view(np.uint32)), t
        assert np.array_equal(ea["m"][t].view(np.uint32), eb["m"][t].view(np.uint32)), "m " + t
        assert np.array_equal(ea["v"][t].view(np.uint32), eb["v"][t].view(np.uint32)), "v " + t


def assert_batch_equal(a, b, step):
    ba, bb = a.batch(step), b.batch(step)
    for key in ba:
        assert np.array_equal(ba[key].view(np.uint32), bb[key].view(np.uint32)), key
    return ba


# V at the tile edges, (B, d) at the ends and in the middle, k in {1, 2, 5}, walk_len = 2k+1 (one legal
# position) and 4k+3, both fallbacks (the tables have empty rows), with and without a label map
PARITY = [
    (34, 32, 32, 2, 11, 0, False),
    (TW - 1, 32, 32, 1, 3, 1, True),
    (TW, 64, 96, 2, 11, 0, True),
    (TW + 1, 64, 96, 5, 11, 1, False),
    (3 * TW + 5, 128, 128, 5, 23, 0, False),
    (3 * TW + 5, 128, 128, 1, 7, 1, True),
    (34, 32, 32, 5, 23, 1, True),
    # the MFMA block maps (block q = wave + 4u against nblk) where B / 32 and d / 32 differ or are odd
    (3 * TW + 5, 96, 32, 2, 11, 0, False),
    (3 * TW + 5, 96, 64, 2, 11, 1, True),
    (3 * TW + 5, 32, 128, 2, 11, 0, True),
    (3 * TW + 5, 128, 32, 2, 11, 1, False),
]


@pytest.mark.parametrize("V,B,d,k,L,fallback,labelled", PARITY)
def test_kernel_equals_host_bitwise(V, B, d, k, L, fallback, labelled):
    """After 1, 3 and 20 steps every parameter, m, v and every batch array is bit-equal; the reported loss is
    within 1e-5 relative: both sides hold the same logits, maxima and exp-sums bit for bit, and the loss differs
    only by the two libraries' fp64 log."""
    dev, host = pair(V, B, d, k, L, fallback, labelled)
    b0 = assert_batch_equal(dev, host, 0)
    if V == 34:
        assert len(set(b0["centre"].tolist())) < B   # centres repeat within the batch: dw1 rows collide
    done = 0
    for upto in (1, 3, 20):
        ld, lh = dev.train(done, upto - done), host.train(done, upto - done)
        done = upto
        assert_state_equal(dev, host)
        assert np.all(np.isfinite(lh)) and np.all(np.abs(ld - lh) <= 1e-5 * np.abs(lh))   # per step
    assert_batch_equal(dev, host, 19)


def check_steps(dev, host, marks):
    """Batch 0, then state, Adam moments and losses after each count of steps in `marks`, then the last batch."""
    b0 = assert_batch_equal(dev, host, 0)
    done = 0
    for upto in marks:
        ld, lh = dev.train(done, upto - done), host.train(done, upto - done)
        done = upto
        assert_state_equal(dev, host)
        assert np.all(np.isfinite(lh)) and np.all(np.abs(ld - lh) <= 1e-5 * np.abs(lh))
    assert_batch_equal(dev, host, done - 1)
    return b0


# k_ds_rowstats walks the tile partials in runs of 16 tiles, 8 runs per outer trip: 17 tiles hand S from run 0 to
# run 1, 128 tiles fill one trip exactly, 129 start the second, 162 is blog's V.  k_ds_reduce_dh and the part /
# tmax / tsum strides see the same tile counts.
@pytest.mark.parametrize("V,B,d,marks", [(1025, 32, 32, (1, 3, 20)), (8192, 64, 32, (1, 3)), (8193, 64, 64, (1, 3)),
                                         (10313, 128, 128, (1, 3))])
def test_many_tiles(V, B, d, marks):
    assert (V + TW - 1) // TW in (17, 128, 129, 162)
    dev, host = pair(V, B, d, 2, 11, 0, V != 8192)
    check_steps(dev, host, marks)
    dev.free()
    host.free()


@pytest.mark.parametrize("fallback", [0, 1])
@pytest.mark.parametrize("k", [32, 33, 64])
def test_wide_windows(k, fallback):
    """W = 2k+1 in {65, 67, 129}: the 64-lane loops of k_ds_batch take a second and a third trip."""
    dev, host = pair(200, 32, 32, k, 140, fallback, fallback == 1)
    b0 = check_steps(dev, host, (1, 3))
    print(f"k {k}: max tgt_n {b0['tgt_n'].max()}")
    if k == 64:
        assert b0["tgt_n"].max() > 64   # more distinct targets than lanes
    else:
        assert b0["tgt_n"].max() > 32


def test_deep_table():
    """topk = 1024 (GW_DS_MAX_TOPK) with rows that are full: ten rounds of the binary search.  The walks pass
    through the full rows' vertices, so those rows are looked up as centres; found values come from the row, the
    rest are the row's smallest."""
    from gwamd import _lib as Cl
    from gwamd import deepsim
    V, topk, full, scale = 1100, 1024, 24, 0.5
    rng = np.random.RandomState(13)
    ids = np.full((V, topk), -1, np.int32)
    sc = np.zeros((V, topk), np.float64)
    for v in range(V):
        n = topk if v < full else int(rng.randint(1, 8))
        ids[v, :n] = rng.choice(V, n, replace=False)
        sc[v, :n] = np.sort(rng.uniform(0.01, 0.9, n))[::-1]
    W = rng.randint(0, V, (80, 11)).astype(np.int32)
    W[:, ::2] = rng.randint(0, full, W[:, ::2].shape)
    kw = dict(dim=32, window=2, batch=32, seed=7, score_scale=scale)
    dev, host = trainer(V, ids, sc, W, device=0, **kw), trainer(V, ids, sc, W, device=-1, **kw)
    hits = misses = 0
    for step in (0, 3):
        b = assert_batch_equal(dev, host, step)
        for s in range(32):
            c = int(b["centre"][s])
            if c >= full:
                continue
            row = {int(i): np.float32(x * scale) for i, x in zip(ids[c], sc[c])}
            for q in range(b["tgt_n"][s]):
                j = int(b["tgt_id"][s, q])
                assert b["tgt_val"][s, q] == row.get(j, np.float32(sc[c, -1] * scale))
                hits += j in row
                misses += j not in row
    assert hits > 32 and misses > 0
    dev.train(0, 2)
    host.train(0, 2)
    assert_state_equal(dev, host)
    wide = deepsim.DeepSim(V, device=0, **kw)
    with pytest.raises(Cl.UnsupportedError, match="kernels take"):
        wide.set_simrank(np.full((V, topk + 1), -1, np.int32), np.zeros((V, topk + 1)))
    deepsim.DeepSim(V, device=-1, **kw).set_simrank(np.full((V, topk + 1), -1, np.int32), np.zeros((V, topk + 1)))


def test_label_map_longer_than_the_vertex_count():
    """Tokens in [0, 2V) through a map of 2V entries into [0, V): tokens t and t + V are the same vertex, so the
    batches equal those of the unshifted walks under the map's first half."""
    V, B, d, k = 3 * TW + 5, 32, 32, 2
    ids, sc, W = corpus(V, k, 11, B + 40, 7)
    rng = np.random.RandomState(5)
    perm = rng.permutation(V).astype(np.int64)
    labels = np.concatenate([perm, perm])
    W2 = np.where(W >= 0, W + V * rng.randint(0, 2, W.shape), -1).astype(np.int32)
    assert W2.max() >= V and (W2 < V).any()
    kw = dict(dim=d, window=k, batch=B, seed=7, score_scale=0.5)
    dev, host = trainer(V, ids, sc, W2, labels, device=0, **kw), trainer(V, ids, sc, W2, labels, device=-1, **kw)
    check_steps(dev, host, (1, 3))
    assert_batch_equal(host, trainer(V, ids, sc, W, perm, device=-1, **kw), 2)
    assert_state_equal(dev, host)


@pytest.mark.parametrize("V,B,d,k", [(34, 32, 32, 2), (3 * TW + 5, 64, 96, 5), (8193, 64, 64, 2)])
def test_gradients_equal_host_bitwise(V, B, d, k):
    dev, host = pair(V, B, d, k, 4 * k + 3, 0, False, seed=3)
    for step in (0, 5):
        gd, gh = dev.gradients(step), host.gradients(step)
        for t in TENSORS:
            assert np.array_equal(gd[t].view(np.uint32), gh[t].view(np.uint32)), (step, t)
        assert gh["w2"].any() and gh["w1"].any()
        if step == 0:
            assert_state_equal(dev, host)   # nothing was updated
            dev.train(0, 5)
            host.train(0, 5)
    assert_state_equal(dev, host)


def test_two_runs_and_split_calls_give_the_same_bits():
    V, B, d, k = 3 * TW + 5, 64, 64, 2
    a, _ = pair(V, B, d, k, 11, 0, True)
    b, _ = pair(V, B, d, k, 11, 0, True)
    c, _ = pair(V, B, d, k, 11, 0, True)
    la = a.train(0, 20)
    lb = b.train(0, 20)
    lc = np.concatenate([c.train(0, 7), c.train(7, 13)])
    assert np.array_equal(la, lb) and np.array_equal(la, lc)
    assert_state_equal(a, b)
    assert_state_equal(a, c)


def test_vectors_torch_aliases_w1():
    import torch
    dev, _ = pair(TW + 1, 32, 32, 2, 11, 0, False)
    v = dev.vectors_torch()
    assert tuple(v.shape) == (TW + 1, 32) and v.is_cuda
    before = v.clone()
    assert np.array_equal(before.cpu().numpy(), dev.export()["w1"])
    dev.train(0, 2)
    torch.cuda.synchronize()
    assert not torch.equal(v, before)                       # the view changed with no export
    assert np.array_equal(v.cpu().numpy(), dev.export()["w1"])


def test_table_straight_from_topsim():
    """The CUDA tensors a gw_topsim call wrote (moreno, every vertex a source) give the same batches as the same
    rows passed through the host."""
    import torch
    from gwamd import _lib as Cl
    from gwamd import deepsim, topsim
    V, K, SAMPLE = 1380, 12, 100
    g = topsim.Graph(os.path.join(DATA, "moreno_crime_crime.txt"), V, separator="\t")
    g._ensure_device()
    src = torch.arange(V, dtype=torch.int32, device="cuda:0")
    ids = torch.empty((V, K), dtype=torch.int32, device="cuda:0")
    sc = torch.empty((V, K), dtype=torch.float64, device="cuda:0")
    Cl.check(Cl.lib().gw_topsim(g._g.handle, 0, SAMPLE, 3, 0.6, 5, Cl.ptr(src), V, K, Cl.ptr(ids), Cl.ptr(sc), None,
                                None), g._g.handle)
    torch.cuda.synchronize()
    hi, hs = ids.cpu().numpy(), sc.cpu().numpy()
    assert (hi >= 0).sum() > V   # a real table
    rng = np.random.RandomState(1)
    W = rng.randint(0, V, (80, 9)).astype(np.int32)
    for w in range(80):          # neighbours in the table, so that lookups hit
        for i in range(1, 9):
            r = hi[W[w, i - 1]]
            r = r[r >= 0]
            if len(r):
                W[w, i] = r[rng.randint(len(r))]
    kw = dict(dim=32, window=2, batch=32, score_scale=1.0 / SAMPLE, seed=2)
    dev = deepsim.DeepSim(V, device=0, **kw)
    dev.set_simrank(ids, sc)     # device pointers, no host trip by the caller
    dev.set_walks(torch.as_tensor(W, device="cuda:0"))
    host = trainer(V, hi, hs, W, device=-1, **kw)
    hit = 0
    for step in (0, 3):
        b = assert_batch_equal(dev, host, step)
        hit += int((b["tgt_val"] > 0).sum())
    assert hit > 0
    dev.train(0, 2)
    host.train(0, 2)
    assert_state_equal(dev, host)


@pytest.mark.parametrize("kw", [{"dim": 48}, {"batch": 160}, {"window": 65}])
def test_unsupported_shapes(kw):
    from gwamd import _lib as Cl
    from gwamd import deepsim
    with pytest.raises(Cl.UnsupportedError, match="kernels take"):
        deepsim.DeepSim(100, device=0, **kw)   # refused at create: there is no handle to launch from
    deepsim.DeepSim(100, device=-1, **dict({"dim": 8, "batch": 4, "window": 1}, **kw)).free()


def test_kernel_attrs():
    dev, _ = pair(3 * TW + 5, 128, 128, 5, 23, 0, False)
    at = dev.kernel_attrs()
    assert list(at) == ["k_ds_batch", "k_ds_hidden", "k_ds_forward", "k_ds_rowstats", "k_ds_backward",
                        "k_ds_reduce_dh", "k_ds_dw1", "k_ds_adam_w1", "k_ds_zero_rows"]
    for name, a in at.items():
        assert a["scratch_bytes"] == 0 and a["vgprs"] > 0, (name, a)   # measured: no kernel spills
    assert at["k_ds_forward"]["lds_bytes"] == 128 * (33 + 65) * 4
    assert at["k_ds_backward"]["lds_bytes"] == (128 * 64 + 64 * 128) * 4


def test_command_line_end_to_end(tmp_path):
    """python -m gwamd.deepsim on karate: the table comes from gw_topsim_write_text in a child process, the walks
    are generated, 50 steps; the file parses back to [35][dim] (karate's labels are 1..34, and a label is the
    vertex index, so vertex_num is 35) and equals export()'s w1 through the writer."""
    from gwamd import deepsim, io
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, ROOT, os.environ.get("PYTHONPATH", "")]))
    karate = os.path.join(DATA, "karate.edgelist")
    sim = str(tmp_path / "karate_top10.txt")
    code = ("import sys; from gwamd import topsim; "
            "g = topsim.Graph(sys.argv[1], 35, separator=' '); "
            "topsim.TopSim_singleSample(g, 200, 3, seed=4).writeText(sys.argv[2], 10)")
    r = subprocess.run([sys.executable, "-c", code, karate, sim], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    out = str(tmp_path / "karate.emb")
    argv = ["--input", karate, "--delimiter", " ", "--simrank_path", sim + ".sim.txt", "--emb_output", out,
            "--vertex-num", "35", "--dimensions", "32", "--window-size", "2", "--walk-length", "11", "--num-walks",
            "10", "--steps", "50", "--batch", "32", "--score-scale", "0.005", "--seed", "3", "--checkpoint-every", "25"]
    r = subprocess.run([sys.executable, "-m", "gwamd.deepsim"] + argv, env=env, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [line.split() for line in open(out).read().splitlines()]
    assert rows[0] == ["35", "32"] and [int(x[0]) for x in rows[1:]] == list(range(35))
    got = np.array([[np.float32(x) for x in r_[1:]] for r_ in rows[1:]], np.float32)
    assert got.shape == (35, 32) and np.isfinite(got).all()
    assert os.path.exists(out + "0") and os.path.exists(out + "25")
    # the same run in this process: export()'s w1 through the writer gives the same bytes
    args = deepsim.parse_args(argv)
    args.emb_output = str(tmp_path / "again.emb")
    walks, labels = deepsim._generate_walks(args)
    m = deepsim.main(args, io.read_simrank(args.simrank_path), walks, labels)
    assert np.array_equal(m.export()["w1"], got)
    assert open(args.emb_output, "rb").read() == open(out, "rb").read()
    assert (m.batch(0)["tgt_val"] > 0).any()
