"""CPU: the DeepSim trainer's host side (gw_deepsim_*, device = -1) - table
build, batch law, initial values, gradients against autograd, Adam, resuming,
learning on a planted graph, the save_embeddings writer and the error paths.

The restatements below are written from the law as include/graphwalk.h states
it; draws go through gw_philox4x32(-1, ...), which test_philox_kat.py pins.
"""
import ctypes
import os
import subprocess
import types

import numpy as np
import pytest

from conftest import DATA, PKG, ROOT

TAG_B, TAG_I, TAG_P = 0x64734230, 0x64734930, 0x64735030
SIM333 = os.path.join(DATA, "0_333_5038_simrank_navie_top10.txt.sim.txt")


def _C():
    from gwamd import _lib as C
    C.lib()
    return C


def _D():
    from gwamd import deepsim
    return deepsim


def philox(rows):
    C = _C()
    a = np.ascontiguousarray(rows, np.uint32).reshape(-1, 6)
    out = np.empty((a.shape[0], 4), np.uint32)
    assert C.lib().gw_philox4x32(-1, C.ptr(a), a.shape[0], C.ptr(out)) == 0
    return out


# ---- restatements -------------------------------------------------------------
def feistel(i, n, k0, k1, tweak):
    if n <= 1:
        return 0
    bits = 2
    while (1 << bits) < n:
        bits += 2
    half = bits // 2
    mask = (1 << half) - 1
    x = i
    while True:
        L, R = x >> half, x & mask
        for r in range(4):
            f = philox([[R & 0xFFFFFFFF, R >> 32, tweak, r, k0, k1]])[0]
            F = ((int(f[1]) << 32) | int(f[0])) & mask
            L, R = R, L ^ F
        x = (L << half) | R
        if x < n:
            return x


def draw(seed, t, s, elig, lens, k):
    """(walk index, position) of slot s of step t."""
    lo, hi = seed & 0xFFFFFFFF, seed >> 32
    e = feistel(s, len(elig), lo ^ (t >> 32), hi ^ TAG_P, t & 0xFFFFFFFF)
    word = int(philox([[t & 0xFFFFFFFF, t >> 32, s, 0, lo, hi ^ TAG_B]])[0][0])
    return elig[e], k + ((word * (lens[e] - 2 * k)) >> 32)


def walk_lens(W):
    return [int(np.argmax(r == -1)) if (r == -1).any() else len(r) for r in W]


def reference_rows(ids, scores, scale=1.0):
    """read_simrank + DeepSim.main :407-414: per row the kept (id, value) list sorted by id, and tem."""
    rows, tem = [], []
    for v in range(ids.shape[0]):
        row = [(int(i), float(s) * scale) for i, s in zip(ids[v], scores[v]) if i != -1 and float(s) * scale > 1e-8]
        tem.append(row[-1][1] if row else 0.0)
        rows.append(sorted(row, key=lambda x: (x[0], x[1])))
    return rows, tem


def reference_lookup(sim, j, fallback):
    """get_batch :303-319."""
    start, end = 0, len(sim) - 1
    while start <= end:
        mid = int((start + end) / 2.0)
        if j == sim[mid][0]:
            return sim[mid][1]
        if j > sim[mid][0]:
            start = mid + 1
        else:
            end = mid - 1
    return fallback


def reference_batch(W, labels, ids, scores, seed, t, B, k, fallback, scale=1.0):
    lens = walk_lens(W)
    elig = [w for w in range(len(W)) if lens[w] >= 2 * k + 1]
    el = [lens[w] for w in elig]
    rows, tem = reference_rows(ids, scores, scale)
    out = []
    for s in range(B):
        w, pos = draw(seed, t, s, elig, el, k)
        toks = [int(x) if labels is None else int(labels[x]) for x in W[w, pos - k:pos + k + 1]]
        c = toks[k]
        uniq = list(dict.fromkeys(toks))
        fb = tem[c] if fallback == 0 else tem[pos]
        vals = [np.float32(reference_lookup(rows[c], j, fb)) for j in uniq]
        ys = np.float32(0)
        for x in vals:
            ys = np.float32(ys + x)
        out.append((w, pos, c, uniq, vals, ys))
    return out


# ---- fixtures -------------------------------------------------------------------
def synth(V, topk=6, nwalks=80, L=11, seed=3, short=True):
    """A table with empty rows, short rows and values <= 1e-8, and walks some of which are cut short."""
    rng = np.random.RandomState(seed)
    ids = np.full((V, topk), -1, np.int32)
    sc = np.zeros((V, topk), np.float64)
    for v in range(V):
        n = 0 if v % 7 == 3 else int(rng.randint(1, topk + 1))
        ids[v, :n] = rng.choice(V, n, replace=False)
        sc[v, :n] = np.sort(rng.uniform(0.01, 0.9, n))[::-1]
        if n >= 3 and v % 5 == 0:
            sc[v, n - 1] = 1e-9   # dropped: tem is the value before it
        if n >= 2 and v % 11 == 1:
            sc[v, n - 1] = 1e-8   # dropped too (<=)
    W = rng.randint(0, V, (nwalks, L)).astype(np.int32)
    # walks wander near their start so that window vertices are sometimes in the centre's row
    for w in range(nwalks):
        for i in range(1, L):
            r = ids[W[w, i - 1]]
            r = r[r >= 0]
            if len(r) and rng.rand() < 0.7:
                W[w, i] = r[rng.randint(len(r))]
    if short:
        W[1, 3:] = -1
        W[5, :] = -1
        W[9, L - 1:] = -1
    return ids, sc, W


def trainer(V, ids, sc, W, labels=None, device=-1, **kw):
    m = _D().DeepSim(V, device=device, **kw)
    m.set_simrank(ids, sc)
    m.set_walks(W, labels)
    return m


def sim333():
    ids = np.full((333, 10), -1, np.int32)
    sc = np.zeros((333, 10), np.float64)
    with open(SIM333) as f:
        for line in f:
            w = line.split()
            for e, t in enumerate(w[1:]):
                i, s = t.split(":")
                ids[int(w[0]), e] = int(i)
                sc[int(w[0]), e] = float(s)
    return ids, sc


# ---- table build + batch law ---------------------------------------------------------
@pytest.mark.parametrize("fallback", [0, 1])
@pytest.mark.parametrize("which", ["synthetic", "sim333", "labels"])
def test_batch_matches_reference_lookup(which, fallback):
    k, B, seed = 2, 32, 0x1234567887654321
    labels = None
    if which == "sim333":
        V = 333
        ids, sc = sim333()
        W = np.random.RandomState(5).randint(0, V, (60, 9)).astype(np.int32)
        W[::2, 4] = ids[W[::2, 3], 0]   # some window vertices are in the centre's row
        W[7, 4:] = -1
    else:
        V = 41
        ids, sc, W = synth(V)
        if which == "labels":
            labels = np.random.RandomState(1).permutation(V).astype(np.int64)
    m = trainer(V, ids, sc, W, labels, dim=8, window=k, batch=B, fallback=fallback, seed=seed, score_scale=0.5)
    hits = 0
    for t in (0, 1, 7):
        b = m.batch(t)
        ref = reference_batch(W, labels, ids, sc, seed, t, B, k, fallback, 0.5)
        assert len({r[0] for r in ref}) == B                 # distinct walks within a step
        lens = walk_lens(W)
        for s, (w, pos, c, uniq, vals, ys) in enumerate(ref):
            assert lens[w] >= 2 * k + 1 and k <= pos < lens[w] - k
            n = b["tgt_n"][s]
            assert b["centre"][s] == c and n == len(uniq)
            assert list(b["tgt_id"][s, :n]) == uniq and (b["tgt_id"][s, n:] == -1).all()
            assert np.array_equal(b["tgt_val"][s, :n], np.array(vals, np.float32))
            assert b["ysum"][s] == ys
            rows, tem = reference_rows(ids, sc, 0.5)
            hits += sum(1 for j in uniq if any(j == i for i, _ in rows[c]))
    assert hits > 0   # the binary search's found branch was exercised


def test_eligibility_and_range_errors():
    V = 41
    ids, sc, W = synth(V)
    D = _D()
    m = D.DeepSim(V, device=-1, dim=8, window=2, batch=32)
    m.set_simrank(ids, sc)
    with pytest.raises(ValueError, match="fewer than the batch"):
        m.set_walks(W[:20])            # 18 eligible walks < 32
    m.set_walks(W)
    # walks 1 (3 tokens) and 5 (none) are shorter than 2k+1 = 5.  Every slot the library returns is matched to
    # the walk windows that can have produced it (centre and first-occurrence order of the window's vertices):
    # each comes from an eligible walk, and none only from a short one.  test_batch_matches_reference_lookup
    # pins the same slots to the stated draw.
    lens = walk_lens(W)
    assert lens[1] == 3 and lens[5] == 0
    windows = {}
    for w in range(len(W)):
        for pos in range(2, lens[w] - 2):
            toks = [int(x) for x in W[w, pos - 2:pos + 3]]
            windows.setdefault((toks[2], tuple(dict.fromkeys(toks))), set()).add(w)
    for t in range(6):
        b = m.batch(t)
        for s in range(32):
            key = (int(b["centre"][s]), tuple(int(x) for x in b["tgt_id"][s, :b["tgt_n"][s]]))
            assert key in windows and not windows[key] <= {1, 5}
    bad = W.copy()
    bad[2, 1] = V
    with pytest.raises(IndexError):
        m.set_walks(bad)
    lab = np.arange(V, dtype=np.int64)
    lab[int(W[0, 0])] = V   # a used label outside [0, V)
    with pytest.raises(IndexError):
        m.set_walks(W, lab)
    with pytest.raises(IndexError):
        m.set_walks(W, np.arange(V - 1, dtype=np.int64)[:int(W.max())])   # a token beyond the label map
    bad_ids = ids.copy()
    bad_ids[0, 0] = V
    with pytest.raises(IndexError):
        m.set_simrank(bad_ids, sc)
    # fallback by position indexes tem by the walk position: walk_len - window <= V
    m2 = D.DeepSim(5, device=-1, dim=8, window=1, batch=2, fallback=1)
    with pytest.raises(IndexError, match="position"):
        m2.set_walks(np.zeros((4, 9), np.int32))


def test_state_and_argument_errors():
    C, D = _C(), _D()
    m = D.DeepSim(10, device=-1, dim=4, window=1, batch=2)
    with pytest.raises(C.StateError):
        m.train(0, 1)
    with pytest.raises(C.StateError):
        m.batch(0)
    for kw in ({"dim": 0}, {"window": 0}, {"batch": 0}, {"fallback": 2}, {"learning_rate": 0.0}, {"beta1": 1.0}):
        with pytest.raises(ValueError):
            D.DeepSim(10, device=-1, **kw)
    with pytest.raises(ValueError):
        D.DeepSim(0, device=-1)
    with pytest.raises(ValueError):
        D.DeepSim(10, device=-2)
    h = ctypes.c_void_p()
    assert C.lib().gw_deepsim_create(-1, None, ctypes.byref(h)) == C.GW_ERR_INVALID   # vertex_num is required
    assert b"vertex_num" in C.lib().gw_deepsim_last_error(None)
    assert C.lib().gw_deepsim_free(None) == 0
    with pytest.raises(ValueError):
        D.save_embeddings("/nonexistent-dir/x", np.zeros(3, np.float32))
    with pytest.raises(OSError):
        D.save_embeddings("/nonexistent-dir/x", np.zeros((2, 3), np.float32))


def test_struct_size_smaller_keeps_defaults():
    """A caller compiled against a shorter params struct: the fields it does not have keep the defaults."""
    C, D = _C(), _D()
    p = C.DeepSimParams(vertex_num=12, dim=8, window=1, batch=4, learning_rate=123.0, seed=99)
    p.struct_size = C.DeepSimParams.learning_rate.offset   # ends before learning_rate
    h = ctypes.c_void_p()
    assert C.lib().gw_deepsim_create(-1, ctypes.byref(p), ctypes.byref(h)) == 0
    full = D.DeepSim(12, device=-1, dim=8, window=1, batch=4)   # lr 0.001, seed 0
    ids = np.tile(np.arange(1, 4, dtype=np.int32), (12, 1))
    sc = np.tile(np.array([0.5, 0.4, 0.3]), (12, 1))
    W = np.random.RandomState(0).randint(0, 12, (8, 5)).astype(np.int32)
    full.set_simrank(ids, sc)
    full.set_walks(W)
    assert C.lib().gw_deepsim_set_simrank(h, C.ptr(ids), C.ptr(sc), 3) == 0
    assert C.lib().gw_deepsim_set_walks(h, C.ptr(W), 8, 5, None, 0) == 0
    assert C.lib().gw_deepsim_train(h, 0, 2, None, None) == 0
    full.train(0, 2)
    w1 = np.empty((12, 8), np.float32)
    arr = (ctypes.c_void_p * 4)(w1.ctypes.data, None, None, None)
    assert C.lib().gw_deepsim_export(h, arr, None, None) == 0
    assert np.array_equal(w1, full.export()["w1"])   # same seed (0) and learning rate (0.001): the defaults
    C.lib().gw_deepsim_free(h)
    p.struct_size = 2
    assert C.lib().gw_deepsim_create(-1, ctypes.byref(p), ctypes.byref(h)) == C.GW_ERR_INVALID


# ---- initial values ---------------------------------------------------------------
def test_init_is_truncated_normal():
    m = _D().DeepSim(1000, device=-1, dim=128, window=1, batch=1, seed=11)
    e = m.export()
    for t in ("w1", "w2"):
        x = e[t].astype(np.float64).ravel()
        assert x.size >= 10 ** 5
        assert np.abs(e[t]).max() <= np.float32(0.2)
        assert abs(x.mean()) < 5 * 0.088 / np.sqrt(x.size)
        assert abs(x.std() / (0.1 * 0.8796) - 1.0) < 0.02
    assert not e["b1"].any() and not e["b2"].any()
    assert not np.array_equal(e["w1"].ravel()[:1000], e["w2"].ravel()[:1000])
    # the first elements against the stated draw: Box-Muller on Philox words, redrawn while |z| > 2
    for tensor, name in ((0, "w1"), (2, "w2")):
        for i in range(40):
            a = 0
            while True:
                u = philox([[i, 0, tensor, a, 11, TAG_I]])[0]
                z = np.sqrt(-2.0 * np.log((float(u[0]) + 1.0) * 2.0 ** -32)) * np.cos(2 * np.pi * float(u[1]) * 2.0 ** -32)
                if abs(z) <= 2.0:
                    break
                a += 1
            assert abs(float(e[name].ravel()[i]) - 0.1 * z) <= np.spacing(np.float32(0.1))   # the float32 cast


# ---- the model in numpy (any dtype) ---------------------------------------------------
def dense_y(b, V, dtype):
    Y = np.zeros((len(b["centre"]), V), dtype)
    for s, n in enumerate(b["tgt_n"]):
        Y[s, b["tgt_id"][s, :n]] = b["tgt_val"][s, :n]
    return Y


def np_grad(P, b, V, dtype):
    """loss and gradients of "The model" in `dtype`, plain numpy."""
    w1, b1, w2, b2 = (P[t].astype(dtype) for t in ("w1", "b1", "w2", "b2"))
    c, Y = b["centre"], dense_y(b, V, dtype)
    B = dtype(len(c))
    pre = w1[c] + b1
    hid = np.maximum(pre, dtype(0))
    lg = hid @ w2 + b2
    mx = lg.max(1, keepdims=True)
    ex = np.exp(lg - mx)
    S = ex.sum(1, keepdims=True)
    loss = (-(Y * (lg - mx - np.log(S))).sum(1)).mean()
    dl = (ex / S * Y.sum(1, keepdims=True) - Y) / B
    dh = (dl @ w2.T) * (pre > 0)
    g1 = np.zeros_like(w1)
    np.add.at(g1, c, dh)
    return loss, {"w1": g1, "b1": dh.sum(0), "w2": hid.T @ dl, "b2": dl.sum(0)}


def adam_consts(t, lr=0.001, b1=0.9, b2=0.999):
    return lr * np.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)


def np_adam(P, Ms, Vs, g, t, dtype):
    lr_t = dtype(adam_consts(t))
    for n in g:
        Ms[n] = dtype(0.9) * Ms[n] + dtype(1.0 - 0.9) * g[n]
        Vs[n] = dtype(0.999) * Vs[n] + dtype(1.0 - 0.999) * (g[n] * g[n])
        P[n] = P[n] - lr_t * Ms[n] / (np.sqrt(Vs[n]) + dtype(1e-8))


GRAD_RATIOS = {}


@pytest.mark.parametrize("V", [34, 300, 8200])
def test_gradients_match_autograd(V):
    """gw_deepsim_gradients against torch autograd in fp64; per tensor max|g - g64| <= 16 * E32, E32 the same
    measure of a plain numpy float32 evaluation.  Measured ratios max|g - g64| / E32 (this test prints them):
    V = 34: w1 0.94, b1 1.81, w2 1.00, b2 1.00; V = 300: w1 1.65, b1 1.24, w2 1.00, b2 1.00; V = 8200 (129 column
    tiles: the second outer trip of the kernels' row statistics): w1 1.31, b1 0.74, w2 1.00, b2 1.00."""
    import torch
    ids, sc, W = synth(V, nwalks=90, L=9, seed=V)
    m = trainer(V, ids, sc, W, dim=32, window=2, batch=32, seed=5)
    m.train(0, 3)   # away from the zero biases
    P, b, g = m.export(), m.batch(3), m.gradients(3)
    if V == 34:
        assert len(set(b["centre"])) < 32   # centres repeat: dw1 rows collide
    T = {t: torch.tensor(P[t].astype(np.float64), requires_grad=True) for t in ("w1", "b1", "w2", "b2")}
    Y = torch.tensor(dense_y(b, V, np.float64))
    hid = torch.relu(T["w1"][torch.tensor(b["centre"].astype(np.int64))] + T["b1"])
    logits = hid @ T["w2"] + T["b2"]
    loss = (-(Y * torch.log_softmax(logits, 1)).sum(1)).mean()
    loss.backward()
    _, g32 = np_grad(P, b, V, np.float32)
    for t in ("w1", "b1", "w2", "b2"):
        g64 = T[t].grad.numpy()
        E32 = np.abs(g32[t].astype(np.float64) - g64).max()
        err = np.abs(g[t].astype(np.float64) - g64).max()
        print(f"V={V} {t}: err {err:.3e} E32 {E32:.3e} ratio {err / E32:.2f} max|g64| {np.abs(g64).max():.3e}")
        assert E32 > 0 and err <= 16 * E32
    assert np.array_equal(m.export()["w1"], P["w1"])   # gradients() updates nothing


def ulps(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


def test_adam_states_and_update():
    V = 34
    ids, sc, W = synth(V, nwalks=90, L=9, seed=2)
    m = trainer(V, ids, sc, W, dim=32, window=2, batch=32, seed=8)
    used = set()
    prev = m.export()
    for step in range(3):
        g = m.gradients(step)
        used |= set(m.batch(step)["centre"].tolist())
        m.train(step, 1)
        cur = m.export()
        lr_t = np.float32(adam_consts(step + 1))
        for t in ("w1", "b1", "w2", "b2"):
            if step == 0:
                nz = g[t] != 0
                assert ulps(cur["m"][t], np.float32(1.0 - 0.9) * g[t])[nz].max() <= 2
                assert ulps(cur["v"][t], np.float32(1.0 - 0.999) * (g[t] * g[t]))[nz].max() <= 2
                assert not cur["m"][t][~nz].any() and not cur["v"][t][~nz].any()
            # the update from the exported states: theta' = theta - q, q = lr_t * m / (sqrt(v) + eps) in float32;
            # the new parameter is theta - q rounded once, so it is compared as a parameter, to 4 ulp of q
            q = (lr_t * cur["m"][t]) / (np.sqrt(cur["v"][t]) + np.float32(1e-8))
            want = prev[t] - q
            assert (np.abs(cur[t].astype(np.float64) - want.astype(np.float64)) <= 4 * np.spacing(np.abs(q))).all()
        prev = cur
    idle = np.array(sorted(set(range(V)) - used))
    assert len(idle) > 0
    init = trainer(V, ids, sc, W, dim=32, window=2, batch=32, seed=8).export()
    assert not prev["m"]["w1"][idle].any() and not prev["v"]["w1"][idle].any()
    assert np.array_equal(prev["w1"][idle], init["w1"][idle])


def test_resume_and_determinism():
    V = 50
    ids, sc, W = synth(V, nwalks=70, L=9, seed=4)
    a = trainer(V, ids, sc, W, dim=16, window=2, batch=24, seed=3)
    b = trainer(V, ids, sc, W, dim=16, window=2, batch=24, seed=3)
    c = trainer(V, ids, sc, W, dim=16, window=2, batch=24, seed=4)
    la = np.concatenate([a.train(0, 5), a.train(5, 5)])
    lb = b.train(0, 10)
    c.train(0, 10)
    ea, eb, ec = a.export(), b.export(), c.export()
    assert np.array_equal(la, lb)
    for t in ("w1", "b1", "w2", "b2"):
        assert np.array_equal(ea[t], eb[t])
        assert np.array_equal(ea["m"][t], eb["m"][t]) and np.array_equal(ea["v"][t], eb["v"][t])
    assert not np.array_equal(ea["w1"], ec["w1"])


def test_learning_on_planted_blocks():
    """Two blocks of 20 vertices, scores high within a block, walks that stay in their block.  200 steps of the
    host law beside an fp64 and a float32 numpy trajectory on the same batches: the fp64 loss falls, and the host's
    reported loss stays within 16x the float32 trajectory's own deviation of it.
    Measured: fp64 loss 11.2671 -> 9.9400; host max relative deviation 9.3e-8, float32 numpy 1.6e-7."""
    V, half = 40, 20
    rng = np.random.RandomState(9)
    ids = np.zeros((V, half - 1), np.int32)
    sc = np.zeros((V, half - 1), np.float64)
    for v in range(V):
        blk = [u for u in range(v // half * half, v // half * half + half) if u != v]
        ids[v] = rng.permutation(blk)
        sc[v] = np.sort(rng.uniform(0.5, 0.9, half - 1))[::-1]
    W = np.zeros((100, 9), np.int32)
    for w in range(100):
        W[w] = rng.randint(0, half, 9) + (w % 2) * half
    m = trainer(V, ids, sc, W, dim=32, window=2, batch=32, seed=1)
    P0 = m.export(states=False)
    traj = {}
    batches = [m.batch(t) for t in range(200)]
    for dtype in (np.float64, np.float32):
        P = {t: P0[t].astype(dtype) for t in P0}
        Ms = {t: np.zeros_like(P[t]) for t in P}
        Vs = {t: np.zeros_like(P[t]) for t in P}
        losses = []
        for t in range(200):
            loss, g = np_grad(P, batches[t], V, dtype)
            losses.append(float(loss))
            np_adam(P, Ms, Vs, g, t + 1, dtype)
        traj[dtype] = np.array(losses)
    host = m.train(0, 200)
    l64 = traj[np.float64]
    rel32 = (np.abs(traj[np.float32] - l64) / l64).max()
    relh = (np.abs(host - l64) / l64).max()
    print(f"fp64 loss {l64[0]:.4f} -> {l64[-1]:.4f}; host rel dev {relh:.3e}, float32 numpy rel dev {rel32:.3e}")
    assert rel32 > 0
    assert l64[-10:].mean() < l64[:10].mean() - 0.5
    assert relh <= 16 * rel32


# ---- writer -------------------------------------------------------------------------
def expected_embedding_text(e):
    """The format as the issue states it: "<n> 128\\n" (the reference's literal 128), then one row per index,
    "<i> v v ... v\\n", each value as str(numpy.float32) prints it."""
    return f"{len(e)} 128\n" + "".join(" ".join([str(i)] + [str(np.float32(v)) for v in row]) + "\n"
                                       for i, row in enumerate(e))


def test_writer_bytes(tmp_path):
    special = [0.1, -0.012345679, 1.2e-05, 1e-4, 123456.79, 0.0, -0.0, 1e-45, -3e-41, 1.1754942e-38, 1e16, 9.9e15,
               3.0, 1.5e20, 1e-5, 0.00010001, 16777216.0, 3.4028235e38, 0.3, 2.5e-4, 123.0, 1e15]
    rng = np.random.RandomState(0)
    e = np.zeros((5, 128), np.float32)
    e[0, :len(special)] = special
    e[1] = rng.normal(0, 0.1, 128)
    e[2] = rng.normal(0, 1e-4, 128)
    e[3] = np.exp(rng.uniform(-90, 80, 128)) * rng.choice([-1, 1], 128)
    e[4] = rng.randint(-1000, 1000, 128)
    a = tmp_path / "a.emb"
    _D().save_embeddings(a, e)
    assert a.read_bytes() == expected_embedding_text(e).encode()
    _D().save_embeddings(a, e[:, :3])
    assert a.read_text().splitlines()[0] == "5 3"   # the row length, where the reference writes 128


def test_main_round_trip_on_sim333(tmp_path):
    """read_simrank -> main -> file on the 333-vertex fixture (comma-separated as the reference's reader wants)."""
    from gwamd import io
    D = _D()
    src = tmp_path / "sim.txt"
    with open(SIM333) as f:
        src.write_text("".join(",".join(line.split()) + "\n" for line in f))
    simrank = io.read_simrank(str(src))
    assert len(simrank) == 333 and simrank[0][0] == ("329", "0.05161244")
    rng = np.random.RandomState(2)
    walks = [[str(x) for x in rng.randint(0, 333, 9)] for _ in range(50)]
    io.save_list(walks, str(tmp_path / "walks.txt"))
    out = str(tmp_path / "x.emb")
    args = types.SimpleNamespace(vertex_num=333, dimensions=16, window_size=2, emb_output=out, steps=4, batch=32,
                                 device=-1, seed=6, checkpoint_every=2)
    m = D.main(args, simrank, io.read_list(str(tmp_path / "walks.txt")))
    w1 = m.export()["w1"]
    rows = [line.split() for line in open(out).read().splitlines()]
    assert rows[0] == ["333", "16"] and [int(r[0]) for r in rows[1:]] == list(range(333))
    assert np.array_equal(np.array([[np.float32(x) for x in r[1:]] for r in rows[1:]], np.float32), w1)
    assert os.path.exists(out + "0") and os.path.exists(out + "2") and not os.path.exists(out + "1")
    # the table the handle built equals the fixture parsed directly
    ids, sc = sim333()
    m2 = trainer(333, ids, sc, D.walks_from_list(walks), dim=16, window=2, batch=32, seed=6)
    m2.train(0, 4)
    assert np.array_equal(m2.export()["w1"], w1)


# ---- stand-alone sanitizer run ----------------------------------------------------------
def test_host_check_under_sanitizers(tmp_path):
    """gw_deepsim_host.cpp + host/deepsim_host_check.cpp (its own main) under ASan + UBSan, run as a plain program."""
    exe = str(tmp_path / "deepsim_host_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-static-libasan", "-static-libubsan",
           "-ffp-contract=off", "-DGW_DEEPSIM_HOST_ONLY", f"-I{os.path.join(ROOT, 'include')}",
           os.path.join(PKG, "csrc", "gw_deepsim_host.cpp"), os.path.join(PKG, "host", "deepsim_host_check.cpp"),
           "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, str(tmp_path / "check.emb")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "deepsim host check ok" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr
