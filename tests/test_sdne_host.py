"""CPU: the SDNE trainer on the host (gw_sdne_*, device = -1) against an fp64 restatement of the model written
here with torch autograd and numpy: gradients, the batch schedule, determinism, the error paths, the encoding, a
200-step trajectory, the stand-alone sanitizer program, SDNE(Xtrain, XCV, Xtest) and the command line.

The model (csrc/gw_sdne_law.h): h1 = relu(x w1 + b1), z2 = h1 w2 + b2 (the embedding), h2 = relu(z2),
h3 = relu(h2 w3 + b3), y = h3 w4 + b4; loss = sum((y - x)^2) / 2 / B + 0.1 * sum_theta sum(theta^2) / 2
+ 0.1 * KL(0.005 || mean(h2)); TF1 Adam(0.01); step t takes rows [(t mod floor(N / B)) * B, +B).
"""
import os
import subprocess

import numpy as np
import pytest

from conftest import DATA, PKG, ROOT

KARATE = os.path.join(DATA, "karate.edgelist")
TENSORS = ("w1", "b1", "w2", "b2", "w3", "b3", "w4", "b4")
WD, KLW, P_KL, LR = 0.1, 0.1, 0.005, 0.01


def _S():
    from gwamd import _lib as C
    from gwamd import sdne
    C.lib()
    return sdne


def rows_for(N, u0, seed, density=0.3):
    """Sparse-ish non-negative rows, as an adjacency or a top-k row would be."""
    rng = np.random.RandomState(seed)
    X = rng.uniform(0.2, 1.0, (N, u0)) * (rng.uniform(size=(N, u0)) < density)
    return X.astype(np.float32)


def csr_of(X):
    offs = np.zeros(len(X) + 1, np.int64)
    cols, vals = [], []
    for r, row in enumerate(X):
        nz = np.nonzero(row)[0]
        cols += nz.tolist()
        vals += row[nz].tolist()
        offs[r + 1] = len(cols)
    return offs, np.asarray(cols, np.int32), np.asarray(vals, np.float32)


def batch_rows(X, B, t):
    nb = len(X) // B
    return X[(t % nb) * B:(t % nb) * B + B]


# ---- the model in numpy (any dtype), backward written out ---------------------------------------
def np_model(P, x, dtype):
    """(loss, reconstruction term, gradients, z2) of one batch in `dtype`."""
    T = {t: P[t].astype(dtype) for t in TENSORS}
    x = x.astype(dtype)
    B = dtype(len(x))
    z1 = x @ T["w1"] + T["b1"]
    h1 = np.maximum(z1, 0)
    z2 = h1 @ T["w2"] + T["b2"]
    h2 = np.maximum(z2, 0)
    z3 = h2 @ T["w3"] + T["b3"]
    h3 = np.maximum(z3, 0)
    y = h3 @ T["w4"] + T["b4"]
    q = h2.mean(dtype=dtype)
    p, eps = dtype(P_KL), dtype(1e-8)
    rec = ((y - x) ** 2).sum(dtype=dtype) / dtype(2) / B
    reg = dtype(WD) * sum((T[t] ** 2).sum(dtype=dtype) for t in TENSORS) / dtype(2)
    kl = dtype(KLW) * (p * np.log(p / (q + eps)) + (dtype(1) - p) * np.log((dtype(1) - p) / (dtype(1) - q + eps)))
    dy = (y - x) / B
    klg = dtype(KLW) * (-p / (q + eps) + (dtype(1) - p) / (dtype(1) - q + eps)) / dtype(h2.size)
    dz3 = (dy @ T["w4"].T) * (z3 > 0)
    dz2 = (dz3 @ T["w3"].T + klg) * (z2 > 0)
    dz1 = (dz2 @ T["w2"].T) * (z1 > 0)
    g = {}
    for l, (a, dz) in enumerate(((x, dz1), (h1, dz2), (h2, dz3), (h3, dy))):
        w, b = TENSORS[2 * l], TENSORS[2 * l + 1]
        g[w] = a.T @ dz + dtype(WD) * T[w]
        g[b] = dz.sum(0, dtype=dtype) + dtype(WD) * T[b]
    return rec + reg + kl, rec, g, z2


def torch_grads(P, x):
    """The same loss in fp64 torch; its gradients by autograd."""
    import torch
    T = {t: torch.tensor(P[t].astype(np.float64), requires_grad=True) for t in TENSORS}
    x = torch.tensor(x.astype(np.float64))
    h1 = torch.relu(x @ T["w1"] + T["b1"])
    z2 = h1 @ T["w2"] + T["b2"]
    h2 = torch.relu(z2)
    h3 = torch.relu(h2 @ T["w3"] + T["b3"])
    y = h3 @ T["w4"] + T["b4"]
    q = h2.mean()
    loss = ((y - x) ** 2).sum() / 2 / len(x) + WD * sum((T[t] ** 2).sum() for t in TENSORS) / 2 \
        + KLW * (P_KL * torch.log(P_KL / (q + 1e-8)) + (1 - P_KL) * torch.log((1 - P_KL) / (1 - q + 1e-8)))
    loss.backward()
    return float(loss.detach()), {t: T[t].grad.numpy() for t in TENSORS}, z2.detach().numpy()


def adam_np(P, M, V, g, step, dtype):
    t = step + 1
    lr_t = dtype(LR * np.sqrt(1.0 - 0.999 ** t) / (1.0 - 0.9 ** t))
    for k in TENSORS:
        M[k] = dtype(0.9) * M[k] + dtype(1.0 - 0.9) * g[k]
        V[k] = dtype(0.999) * V[k] + dtype(1.0 - 0.999) * g[k] * g[k]
        P[k] = P[k] - lr_t * M[k] / (np.sqrt(V[k]) + dtype(1e-8))


def state_equal(a, b):
    return all(np.array_equal(a[t], b[t]) and np.array_equal(a["m"][t], b["m"][t]) and
               np.array_equal(a["v"][t], b["v"][t]) for t in TENSORS)


# ---- gradients --------------------------------------------------------------------------------------
@pytest.mark.parametrize("units,B", [((20, 12, 7, 9), 5), ((300, 40, 10, 30), 16)])
def test_gradients_match_autograd(units, B):
    """gw_sdne_gradients against torch autograd in fp64 after two training steps (non-zero biases), on step 3's
    batch, rows [B, 2B); per tensor max|g - g64| <= 16 * E32, E32 the same measure of a plain numpy float32
    evaluation.  Some h2 units are dead and some active, so the KL scalar and its mask take part.
    Measured ratios max|g - g64| / E32 (this test prints them):
    (20, 12, 7, 9) B = 5: w1 0.86, b1 1.00, w2 0.73, b2 1.13, w3 1.00, b3 1.00, w4 0.65, b4 1.00;
    (300, 40, 10, 30) B = 16: w1 1.31, b1 0.76, w2 1.04, b2 1.00, w3 1.00, b3 0.50, w4 1.13, b4 1.00."""
    S = _S()
    X = rows_for(2 * B + 3, units[0], 3)
    m = S.SdneModel(units, device=-1, batch=B, seed=11)
    m.set_rows(X)
    m.train(0, 2)
    P = m.export(states=False)
    g = m.gradients(3)
    x = batch_rows(X, B, 3)
    assert np.array_equal(x, X[B:2 * B])
    loss64, g64, z2 = torch_grads(P, x)
    assert (z2 > 0).any() and (z2 <= 0).any()
    _, _, g32, _ = np_model(P, x, np.float32)
    l64, _, gnp, _ = np_model(P, x, np.float64)   # the written-out backward is the autograd one
    assert abs(l64 - loss64) <= 1e-12 * abs(loss64)
    for t in TENSORS:
        assert np.abs(gnp[t] - g64[t]).max() <= 1e-12 * max(1.0, np.abs(g64[t]).max())
        E32 = np.abs(g32[t].astype(np.float64) - g64[t]).max()
        err = np.abs(g[t].astype(np.float64) - g64[t]).max()
        print(f"units={units} {t}: err {err:.3e} E32 {E32:.3e} ratio {err / E32:.2f} max|g64| {np.abs(g64[t]).max():.3e}")
        assert E32 > 0 and err <= 16 * E32
    assert all(np.array_equal(m.export(states=False)[t], P[t]) for t in TENSORS)   # gradients() updates nothing
    assert abs(m.train(2, 1)[0] - np_model(P, batch_rows(X, B, 2), np.float64)[0]) <= 1e-5 * abs(loss64)
    m.free()


# ---- schedule -----------------------------------------------------------------------------------------
def test_schedule_wraps_and_skips_the_tail():
    S = _S()
    B, units = 6, (23, 9, 5, 7)
    X = rows_for(2 * B + 3, units[0], 5)
    m = S.SdneModel(units, device=-1, batch=B, seed=2)
    m.set_rows(X)
    g0, g1, g2 = m.gradients(0), m.gradients(1), m.gradients(2)
    assert all(np.array_equal(g0[t], g2[t]) for t in TENSORS)           # steps 0 and 2: rows [0, B)
    assert not np.array_equal(g0["w1"], g1["w1"])                         # step 1: rows [B, 2B)
    P = m.export(states=False)
    for step, lo in ((0, 0), (1, B), (2, 0)):
        g64 = torch_grads(P, X[lo:lo + B])[1]
        assert np.abs(m.gradients(step)["w4"] - g64["w4"]).max() <= 1e-5 * np.abs(g64["w4"]).max()
    m.train(0, 3)
    a, enc_a = m.export(), m.encode()
    Y = X.copy()
    Y[2 * B:] = rows_for(3, units[0], 99, density=0.6)
    m2 = S.SdneModel(units, device=-1, batch=B, seed=2)
    m2.set_rows(Y)
    m2.train(0, 3)
    b, enc_b = m2.export(), m2.encode()
    assert state_equal(a, b)                                              # the last 3 rows never influence the state
    assert np.array_equal(enc_a[:2 * B], enc_b[:2 * B])
    assert not np.array_equal(enc_a[2 * B:], enc_b[2 * B:])               # but they are encoded
    assert np.array_equal(m2.encode(2 * B, 3), enc_b[2 * B:])
    with pytest.raises(ValueError):
        m.set_rows(X[:B - 1])                                             # N < B
    with pytest.raises(ValueError):
        m.set_csr(*csr_of(X[:B - 1]))
    m.free()
    m2.free()


# ---- determinism --------------------------------------------------------------------------------------
def test_pieces_equal_one_call():
    S = _S()
    B, units = 7, (150, 33, 6, 10)
    X = rows_for(3 * B + 2, units[0], 8)
    out = []
    for pieces in (((0, 7),), ((0, 3), (3, 4))):
        m = S.SdneModel(units, device=-1, batch=B, seed=4)
        m.set_rows(X)
        losses = np.concatenate([m.train(a, n) for a, n in pieces])
        out.append((m.export(), losses))
        m.free()
    assert state_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


def test_csr_equals_dense():
    S = _S()
    B, units = 7, (150, 33, 6, 10)
    X = rows_for(3 * B + 2, units[0], 8)
    out = []
    for sparse in (False, True):
        m = S.SdneModel(units, device=-1, batch=B, seed=4)
        m.set_csr(*csr_of(X)) if sparse else m.set_rows(X)
        m.train(0, 5)
        out.append((m.export(), m.encode()))
        m.free()
    assert state_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    ones = (X != 0).astype(np.float32)                                    # vals = NULL means 1
    offs, cols, _ = csr_of(X)
    a = S.SdneModel(units, device=-1, batch=B, seed=4)
    a.set_csr(offs, cols)
    b = S.SdneModel(units, device=-1, batch=B, seed=4)
    b.set_rows(ones)
    assert np.array_equal(a.train(0, 2), b.train(0, 2)) and state_equal(a.export(), b.export())
    a.free()
    b.free()


# ---- errors ---------------------------------------------------------------------------------------------
def test_errors():
    S = _S()
    from gwamd import _lib as C
    m = S.SdneModel((10, 4, 3, 4), device=-1, batch=2)
    with pytest.raises(C.StateError):
        m.train(0, 1)
    offs = np.array([0, 2, 3, 3], np.int64)
    with pytest.raises(ValueError, match="twice"):
        m.set_csr(offs, np.array([4, 4, 1], np.int32))
    with pytest.raises(IndexError):
        m.set_csr(offs, np.array([4, 10, 1], np.int32))
    with pytest.raises(IndexError):
        m.set_csr(offs, np.array([4, -1, 1], np.int32))
    m.set_csr(offs, np.array([4, 9, 1], np.int32))
    with pytest.raises(ValueError):
        m.encode(2, 2)
    assert m.encode().shape == (3, 3)
    m.free()
    with pytest.raises(ValueError, match="units"):
        S.SdneModel((10, 4, 3, 4, 11), device=-1)                          # u4 != u0
    with pytest.raises(ValueError):
        S.SdneModel((10, 0, 3, 4), device=-1)
    with pytest.raises(ValueError):
        S.SdneModel((10, 4, 3, 4), device=-1, kl_target=0.0)
    assert C.lib().gw_sdne_free(None) == 0
    big = S.SdneModel((10, 4, 3, 4), device=-1, batch=129)                 # past the device caps: the host takes it
    big.free()


# ---- encode -----------------------------------------------------------------------------------------------
def test_encode_is_the_pre_activation():
    """encode = h1 w2 + b2, not relu'd; to float32 accuracy: max|enc - z64| <= 16 * E32 (E32: numpy float32).
    Measured ratio 0.69."""
    S = _S()
    B, units = 8, (300, 40, 10, 30)
    X = rows_for(2 * B + 5, units[0], 12)
    m = S.SdneModel(units, device=-1, batch=B, seed=1)
    m.set_rows(X)
    m.train(0, 4)
    P = m.export(states=False)
    enc = m.encode()
    z64 = np_model(P, X, np.float64)[3]
    z32 = np_model(P, X, np.float32)[3]
    E32 = np.abs(z32.astype(np.float64) - z64).max()
    err = np.abs(enc.astype(np.float64) - z64).max()
    print(f"encode: err {err:.3e} E32 {E32:.3e} ratio {err / E32:.2f}")
    assert enc.shape == (len(X), 10) and E32 > 0 and err <= 16 * E32
    assert (enc < 0).any() and (enc > 0).any()
    m.free()


def test_initial_values():
    S = _S()
    m = S.SdneModel((784, 400, 100, 300), device=-1, seed=3)
    e = m.export(states=False)
    for t in ("w1", "w2", "w3", "w4"):
        x = e[t].astype(np.float64).ravel()
        assert np.abs(e[t]).max() <= np.float32(0.2)
        assert abs(x.mean()) < 5 * 0.088 / np.sqrt(x.size)
        assert abs(x.std() / (0.1 * 0.8796) - 1.0) < 0.03
    assert not any(e[t].any() for t in ("b1", "b2", "b3", "b4"))
    assert not np.array_equal(e["w1"].ravel()[:1000], e["w2"].ravel()[:1000])
    m.free()


# ---- trajectory ---------------------------------------------------------------------------------------------
def karate_rows():
    from gwamd import GWGraph
    csr = GWGraph.from_edgelist(KARATE, " ", "nx").export_csr()
    n = len(csr["offsets"]) - 1
    X = np.zeros((n, n), np.float32)
    for r in range(n):
        X[r, csr["nbrs"][csr["offsets"][r]:csr["offsets"][r + 1]]] = 1.0
    return csr, X


def test_trajectory_on_karate():
    """Karate's adjacency, units (34, 16, 8, 12, 34), B = 17, 200 steps of the host law beside an fp64 and a float32
    numpy trajectory: the fp64 reconstruction term falls, and the host's reported loss stays within 8x the float32
    trajectory's own deviation from the fp64 one (the margin for a different but equally valid summation order).
    Measured: fp64 reconstruction (mean of the two batches) 2.2502 at the first visit -> 1.7529 at the last; max
    deviation of the loss relative to its maximum: host 1.1e-8, float32 numpy 1.0e-7."""
    S = _S()
    _, X = karate_rows()
    assert X.shape == (34, 34)
    B, units, steps = 17, (34, 16, 8, 12), 200
    m = S.SdneModel(units, device=-1, batch=B, seed=6)
    m.set_rows(X)
    P0 = m.export(states=False)
    traj, rec = {}, {}
    for dtype in (np.float64, np.float32):
        P = {t: P0[t].astype(dtype) for t in TENSORS}
        Ms = {t: np.zeros_like(P[t]) for t in TENSORS}
        Vs = {t: np.zeros_like(P[t]) for t in TENSORS}
        losses, recs = [], []
        for step in range(steps):
            loss, r, g, _ = np_model(P, batch_rows(X, B, step), dtype)
            losses.append(float(loss))
            recs.append(float(r))
            adam_np(P, Ms, Vs, g, step, dtype)
            assert all(P[t].dtype == dtype for t in TENSORS)
        traj[dtype], rec[dtype] = np.array(losses), np.array(recs)
    host = m.train(0, steps)
    m.free()
    l64 = traj[np.float64]
    dev32 = np.abs(traj[np.float32] - l64).max() / np.abs(l64).max()
    devh = np.abs(host - l64).max() / np.abs(l64).max()
    print(f"fp64 reconstruction {rec[np.float64][:2].mean():.4f} -> {rec[np.float64][-2:].mean():.4f}; deviation host "
          f"{devh:.2e} float32 numpy {dev32:.2e}")
    assert rec[np.float64][-2:].mean() < rec[np.float64][:2].mean()    # both batches, first visit against last
    assert dev32 > 0 and devh <= 8 * dev32


# ---- sanitizers -----------------------------------------------------------------------------------------------
def test_host_check_under_sanitizers(tmp_path):
    """gw_sdne_host.cpp + host/sdne_host_check.cpp (its own main) under ASan + UBSan, run as a plain program."""
    exe = str(tmp_path / "sdne_host_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-static-libasan", "-static-libubsan",
           "-ffp-contract=off", "-DGW_SDNE_HOST_ONLY", f"-I{os.path.join(ROOT, 'include')}",
           os.path.join(PKG, "csrc", "gw_sdne_host.cpp"), os.path.join(PKG, "host", "sdne_host_check.cpp"),
           "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "sdne host check ok" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr


# ---- the Python layer and the command line -----------------------------------------------------------------------
def test_sdne_function():
    S = _S()
    Xtr, Xcv, Xte = rows_for(25, 40, 1), rows_for(4, 40, 2), rows_for(13, 40, 3)
    kw = dict(units=(12, 5, 9), steps=6, device=-1, batch=10, seed=3)
    a, b, c = S.SDNE(Xtr, Xcv, Xte, **kw)
    assert a.shape == (25, 5) and b.shape == (4, 5) and c.shape == (13, 5)
    assert a.dtype == b.dtype == c.dtype == np.float32
    m = S.SdneModel((40, 12, 5, 9), device=-1, batch=10, seed=3)
    m.set_rows(Xtr)
    m.train(0, 6)
    assert np.array_equal(m.encode(), a)
    m.set_rows(Xte)                                                        # trained on Xtrain only
    assert np.array_equal(m.encode(), c)
    m.free()
    a2, _, _ = S.SDNE(Xtr, Xcv[:0], Xte[:0], **kw)
    assert np.array_equal(a, a2)


def test_cli_on_the_host(tmp_path):
    S = _S()
    from gwamd import deepsim
    csr, X = karate_rows()
    out = str(tmp_path / "k.emb")
    argv = ["--units", "16,8,12", "--batch", "17", "--steps", "20", "--seed", "5", "--device", "-1"]
    assert S.cli(["--input", KARATE, "--delimiter", " ", "--output", out] + argv) == 0
    m = S.SdneModel((34, 16, 8, 12), device=-1, batch=17, seed=5)
    m.set_csr(csr["offsets"], csr["nbrs"])
    m.train(0, 20)
    want = str(tmp_path / "want.emb")
    deepsim.save_embeddings(want, m.encode())
    m.free()
    with open(out, "rb") as f, open(want, "rb") as g:
        text = f.read()
        assert text == g.read()
    lines = text.decode().splitlines()
    assert lines[0] == "34 8" and len(lines) == 35
    assert all(len(l.split()) == 9 and l.split()[0] == str(i) for i, l in enumerate(lines[1:]))
    npy = str(tmp_path / "x.npy")
    np.save(npy, X)
    out2 = str(tmp_path / "k2.emb")
    assert S.cli(["--rows", npy, "--output", out2] + argv) == 0              # the same rows given dense
    with open(out2, "rb") as f:
        assert f.read() == text
    wel = str(tmp_path / "w.edgelist")                                       # weights, found from the third column
    with open(wel, "w") as f:
        for a in range(20):
            for b in (a + 1, a + 3):
                f.write(f"{a} {b % 20} {0.5 + ((a * 7 + b) % 5) / 4}\n")
    outw = str(tmp_path / "w.emb")
    assert S.cli(["--input", wel, "--delimiter", " ", "--output", outw, "--units", "9,4,6", "--batch", "8", "--steps",
                  "5", "--device", "-1"]) == 0
    from gwamd import GWGraph
    wcsr = GWGraph.from_edgelist(wel, " ", "nx", False, True).export_csr()
    assert len(set(wcsr["weights"].tolist())) > 2
    m = S.SdneModel((20, 9, 4, 6), device=-1, batch=8)
    m.set_csr(wcsr["offsets"], wcsr["nbrs"], wcsr["weights"])
    m.train(0, 5)
    deepsim.save_embeddings(want, m.encode())
    m.free()
    with open(outw, "rb") as f, open(want, "rb") as g:
        assert f.read() == g.read()
    sim = str(tmp_path / "x.sim.txt")
    with open(sim, "w") as f:
        for v in range(40):
            f.write(f"{v}," + ",".join(f"{(v + 1 + 3 * e) % 40}:{0.5 / (1 + e)}" for e in range(4)) + "\n")
    out3 = str(tmp_path / "s.emb")
    assert S.cli(["--simrank", sim, "--output", out3, "--units", "9,4,6", "--batch", "10", "--steps", "5",
                  "--device", "-1"]) == 0
    with open(out3) as f:
        assert f.readline().split() == ["40", "4"]
