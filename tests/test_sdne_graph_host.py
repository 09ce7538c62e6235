"""CPU: the SDNE graph loss on the host (gw_sdne_*, device = -1): nonzero_weight (beta), first_order (alpha) and
shuffle, against an fp64 restatement written here with torch autograd and numpy.

Loss of a batch of rows ids (x = X[ids], B rows): sum(w (y - x)^2) / 2 / B with w = beta^2 where x != 0 else 1,
+ the decay and KL terms of test_sdne_host.py, + (alpha / B) sum_ij a_ij |z2_i - z2_j|^2 with a_ij = x[i][ids[j]].
"""
import ctypes

import numpy as np
import pytest

from test_sdne_host import KLW, P_KL, TENSORS, WD, csr_of, karate_rows, state_equal

BETA, ALPHA = 3.0, 0.7
ON = dict(nonzero_weight=BETA, first_order=ALPHA, shuffle=1)


def _S():
    from gwamd import _lib as C
    from gwamd import sdne
    C.lib()
    return sdne


def square_rows(n, seed, weighted, density=0.5):
    """A square matrix with a zero diagonal: symmetric 0/1, or asymmetric with weights (a_ij != a_ji)."""
    rng = np.random.RandomState(seed)
    if weighted:
        X = rng.uniform(0.2, 1.5, (n, n)) * (rng.uniform(size=(n, n)) < density)
    else:
        X = np.triu((rng.uniform(size=(n, n)) < density).astype(np.float64), 1)
        X = X + X.T
    np.fill_diagonal(X, 0.0)
    return X.astype(np.float32)


def torch_graph(P, x, ids, beta, alpha):
    """(loss, gradients, z2) of the batch in fp64 torch, gradients by autograd."""
    import torch
    T = {t: torch.tensor(P[t].astype(np.float64), requires_grad=True) for t in TENSORS}
    x = torch.tensor(x.astype(np.float64))
    B = len(x)
    h1 = torch.relu(x @ T["w1"] + T["b1"])
    z2 = h1 @ T["w2"] + T["b2"]
    h2 = torch.relu(z2)
    h3 = torch.relu(h2 @ T["w3"] + T["b3"])
    y = h3 @ T["w4"] + T["b4"]
    q = h2.mean()
    w = torch.where(x != 0, torch.tensor(beta * beta, dtype=torch.float64), torch.tensor(1.0, dtype=torch.float64))
    loss = (w * (y - x) ** 2).sum() / 2 / B + WD * sum((T[t] ** 2).sum() for t in TENSORS) / 2 \
        + KLW * (P_KL * torch.log(P_KL / (q + 1e-8)) + (1 - P_KL) * torch.log((1 - P_KL) / (1 - q + 1e-8)))
    if alpha:
        A = x[:, torch.as_tensor(np.asarray(ids))]
        D = ((z2[:, None, :] - z2[None, :, :]) ** 2).sum(-1)
        loss = loss + alpha / B * (A * D).sum()
    loss.backward()
    return float(loss.detach()), {t: T[t].grad.numpy() for t in TENSORS}, z2.detach().numpy()


def np_graph(P, x, ids, beta, alpha, dtype):
    """The same gradients written out in numpy in `dtype` (float32: the plain evaluation E32 is measured on)."""
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
    w = np.where(x != 0, dtype(beta) * dtype(beta), dtype(1))
    dy = w * (y - x) / B
    klg = dtype(KLW) * (-p / (q + eps) + (dtype(1) - p) / (dtype(1) - q + eps)) / dtype(h2.size)
    dz3 = (dy @ T["w4"].T) * (z3 > 0)
    dz2 = (dz3 @ T["w3"].T + klg) * (z2 > 0)
    if alpha:
        A = x[:, ids]
        S = A + A.T
        dz2 = dz2 + dtype(2 * alpha) / B * (S.sum(1, dtype=dtype)[:, None] * z2 - S @ z2)
    dz1 = (dz2 @ T["w2"].T) * (z1 > 0)
    g = {}
    for l, (a, dz) in enumerate(((x, dz1), (h1, dz2), (h2, dz3), (h3, dy))):
        wn, bn = TENSORS[2 * l], TENSORS[2 * l + 1]
        g[wn] = a.T @ dz + dtype(WD) * T[wn]
        g[bn] = dz.sum(0, dtype=dtype) + dtype(WD) * T[bn]
    return g


# ---- 1. gradients ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True], ids=["sym01", "asymw"])
@pytest.mark.parametrize("hidden,B", [((12, 7, 9), 5), ((40, 10, 30), 16)])
def test_gradients_match_autograd(hidden, B, weighted):
    """gradients() with beta = 3, alpha = 0.7 and shuffle on against torch autograd in fp64, after two training
    steps, on step 3's batch (the rows batch_rows(3) names); per tensor max|g - g64| <= 16 * E32, E32 the same
    error of a plain numpy float32 evaluation.
    Measured ratios max|g - g64| / E32 (this test prints them), w1 b1 w2 b2 w3 b3 w4 b4:
    (12, 7, 9) B = 5 sym01: 0.74 0.51 0.42 0.76 1.45 1.00 1.02 1.00; asymw: 0.46 1.00 0.70 1.00 1.43 1.00 0.90 1.00;
    (40, 10, 30) B = 16 sym01: 0.86 1.00 1.00 0.63 1.00 0.90 0.90 1.00; asymw: 0.41 0.47 1.50 4.36 0.54 1.52 1.24 1.00."""
    S = _S()
    n = 2 * B + 3
    units = (n,) + hidden
    X = square_rows(n, 3 + B, weighted)
    assert weighted == bool((X != X.T).any())
    m = S.SdneModel(units, device=-1, batch=B, seed=11, **ON)
    m.set_rows(X)
    m.train(0, 2)
    P = m.export(states=False)
    ids = m.batch_rows(3)
    g = m.gradients(3)
    x = X[ids]
    A = x[:, ids]
    assert np.count_nonzero(A + A.T) >= B                                  # the first-order term takes part
    loss64, g64, z2 = torch_graph(P, x, ids, BETA, ALPHA)
    assert (z2 > 0).any() and (z2 <= 0).any()                              # ... on both sides of the relu
    g32 = np_graph(P, x, ids, BETA, ALPHA, np.float32)
    gnp = np_graph(P, x, ids, BETA, ALPHA, np.float64)                     # the written-out backward is autograd's
    ratios = []
    for t in TENSORS:
        assert np.abs(gnp[t] - g64[t]).max() <= 1e-12 * max(1.0, np.abs(g64[t]).max())
        E32 = np.abs(g32[t].astype(np.float64) - g64[t]).max()
        err = np.abs(g[t].astype(np.float64) - g64[t]).max()
        ratios.append(err / E32)
        print(f"units={units} weighted={weighted} {t}: err {err:.3e} E32 {E32:.3e} ratio {err / E32:.2f}")
        assert E32 > 0 and err <= 16 * E32
    print("ratios " + " ".join(f"{r:.2f}" for r in ratios))
    g_no = torch_graph(P, x, ids, BETA, 0.0)[1]                            # and the term is not a rounding error
    assert np.abs(g_no["w2"] - g64["w2"]).max() > 1e-3 * np.abs(g64["w2"]).max()
    assert all(np.array_equal(m.export(states=False)[t], P[t]) for t in TENSORS)
    m.free()


# ---- 2. schedule ----------------------------------------------------------------------------------------
def test_ordered_schedule_is_the_identity():
    S = _S()
    B, n = 6, 15
    m = S.SdneModel((n, 9, 5, 7), device=-1, batch=B, seed=2)
    m.set_rows(square_rows(n, 1, False))
    for t in range(5):
        assert np.array_equal(m.batch_rows(t), (t % 2) * B + np.arange(B))
    m.free()


def test_shuffled_schedule():
    S = _S()
    B, n = 6, 15
    units = (n, 9, 5, 7)
    X = square_rows(n, 5, True)
    m = S.SdneModel(units, device=-1, batch=B, seed=2, shuffle=1)
    m.set_rows(X)
    epochs = [np.concatenate([m.batch_rows(2 * e), m.batch_rows(2 * e + 1)]) for e in range(20)]
    for rows in epochs:
        assert len(set(rows.tolist())) == 2 * B and rows.min() >= 0 and rows.max() < n
    assert not np.array_equal(epochs[0], epochs[1])
    assert set(np.concatenate(epochs).tolist()) == set(range(n))          # the tail rows are drawn too
    other = S.SdneModel(units, device=-1, batch=B, seed=3, shuffle=1)
    other.set_rows(X)
    assert not np.array_equal(np.concatenate([other.batch_rows(0), other.batch_rows(1)]), epochs[0])
    other.free()
    P = m.export(states=False)
    for t in (0, 1, 2, 5):
        ids = m.batch_rows(t)
        g64 = torch_graph(P, X[ids], ids, 1.0, 0.0)[1]
        assert np.abs(m.gradients(t)["w4"] - g64["w4"]).max() <= 1e-5 * np.abs(g64["w4"]).max()
    m.free()


def test_pieces_across_an_epoch_boundary_equal_one_call():
    S = _S()
    B, n = 6, 15
    X = square_rows(n, 8, True)
    out = []
    for pieces in (((0, 7),), ((0, 3), (3, 4)), ((0, 2), (2, 5))):          # epochs begin at steps 0, 2, 4, 6
        m = S.SdneModel((n, 9, 5, 7), device=-1, batch=B, seed=4, **ON)
        m.set_rows(X)
        losses = np.concatenate([m.train(a, k) for a, k in pieces])
        out.append((m.export(), losses))
        m.free()
    for o in out[1:]:
        assert state_equal(out[0][0], o[0]) and np.array_equal(out[0][1], o[1])


# ---- 3. defaults keep the parent's law ------------------------------------------------------------------------
def test_short_struct_is_the_default_law():
    """A gw_sdne_params_t whose struct_size ends before nonzero_weight (the parent's struct; the bytes behind it
    hold other values, which must not be read) against the full struct at its defaults: state, Adam moments, losses
    and encodings identical after 5 steps."""
    S = _S()
    from gwamd import _lib as C
    B, n = 6, 15
    X = square_rows(n, 9, True)
    full = S.SdneModel((n, 9, 5, 7), device=-1, batch=B, seed=4)
    assert full.params.nonzero_weight == 1.0 and full.params.first_order == 0.0 and full.params.shuffle == 0
    short = S.SdneModel((n, 9, 5, 7), device=-1, batch=B, seed=4)
    short.free()
    short.params.struct_size = C.SdneParams.nonzero_weight.offset
    assert short.params.struct_size == C.SdneParams.seed.offset + 8 < ctypes.sizeof(C.SdneParams)
    short.params.nonzero_weight, short.params.first_order = 7.0, 2.0
    h = ctypes.c_void_p()
    C.check(C.lib().gw_sdne_create(-1, ctypes.byref(short.params), ctypes.byref(h)), sdne=True)
    short._h = h
    out = []
    for m in (full, short):
        m.set_rows(X)
        out.append((m.train(0, 5), m.export(), m.encode()))
        m.free()
    assert np.array_equal(out[0][0], out[1][0]) and state_equal(out[0][1], out[1][1])
    assert np.array_equal(out[0][2], out[1][2])


# ---- 4. input forms and errors ----------------------------------------------------------------------------------
def test_csr_equals_dense_with_the_options_on():
    S = _S()
    B, n = 7, 23
    units = (n, 33, 6, 10)
    X = square_rows(n, 8, True)
    out = []
    for sparse in (False, True):
        m = S.SdneModel(units, device=-1, batch=B, seed=4, **ON)
        m.set_csr(*csr_of(X)) if sparse else m.set_rows(X)
        out.append((m.train(0, 5), m.export(), m.encode()))
        m.free()
    assert np.array_equal(out[0][0], out[1][0]) and state_equal(out[0][1], out[1][1])
    assert np.array_equal(out[0][2], out[1][2])
    offs, cols, _ = csr_of(X)                                              # vals = NULL: ones, for a_ij too
    a = S.SdneModel(units, device=-1, batch=B, seed=4, **ON)
    a.set_csr(offs, cols)
    b = S.SdneModel(units, device=-1, batch=B, seed=4, **ON)
    b.set_rows((X != 0).astype(np.float32))
    c = S.SdneModel(units, device=-1, batch=B, seed=4, **ON)
    c.set_rows(X)
    la, lb, lc = a.train(0, 3), b.train(0, 3), c.train(0, 3)
    assert np.array_equal(la, lb) and state_equal(a.export(), b.export())
    assert not np.array_equal(la, lc)
    for m in (a, b, c):
        m.free()


def test_errors():
    S = _S()
    m = S.SdneModel((10, 4, 3, 4), device=-1, batch=2, first_order=0.5)
    X = square_rows(10, 1, False)
    with pytest.raises(ValueError, match="adjacency"):
        m.set_rows(X[:9])
    with pytest.raises(ValueError, match="adjacency"):
        m.set_csr(*csr_of(X[:9]))
    with pytest.raises(ValueError, match="adjacency"):
        m.set_csr(*csr_of(np.concatenate([X, X[:1]])))
    m.set_rows(X)
    m.set_csr(*csr_of(X))
    m.free()
    m = S.SdneModel((10, 4, 3, 4), device=-1, batch=2, nonzero_weight=2.0, shuffle=1)   # alpha = 0: any N
    m.set_rows(np.concatenate([X, X[:3]]))
    m.train(0, 2)
    m.free()
    for bad in (dict(nonzero_weight=0.0), dict(nonzero_weight=-1.0), dict(nonzero_weight=float("nan")),
                dict(first_order=-1.0), dict(first_order=float("inf")), dict(shuffle=2)):
        with pytest.raises(ValueError):
            S.SdneModel((10, 4, 3, 4), device=-1, batch=2, **bad)


# ---- 5. the reported loss ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True], ids=["sym01", "asymw"])
def test_reported_loss(weighted):
    S = _S()
    B, n = 16, 35
    X = square_rows(n, 4, weighted)
    m = S.SdneModel((n, 40, 10, 30), device=-1, batch=B, seed=7, **ON)
    m.set_rows(X)
    for t in range(4):
        P = m.export(states=False)
        ids = m.batch_rows(t)
        want = torch_graph(P, X[ids], ids, BETA, ALPHA)[0]
        plain = torch_graph(P, X[ids], ids, 1.0, 0.0)[0]
        got = m.train(t, 1)[0]
        assert abs(got - want) <= 1e-5 * abs(want), (t, got, want)
        assert abs(plain - want) > 1e-2 * abs(want)                        # both terms are in it
    m.free()


# ---- 6. what the weighting is for -------------------------------------------------------------------------------------
def test_nonzero_weight_reconstructs_the_edges_of_karate():
    """Karate's adjacency, units (34, 16, 8, 12), B = 17, 200 steps of the host law, seed 6, ordered batches, no
    first-order term; y in fp64 from the exported parameters.  The sum over the nonzero entries of (y - x)^2 at
    beta = 5 is below half of the same sum at beta = 1.
    Measured (154 nonzero entries): beta = 1: 99.868, and all 34 encodings are one vector (largest pairwise distance
    exactly 0); beta = 5: 3.585, largest pairwise distance 3.292."""
    S = _S()
    _, X = karate_rows()
    assert X.shape == (34, 34)
    print(f"{np.count_nonzero(X)} nonzero entries")
    err, spread = {}, {}
    for beta in (1.0, 5.0):
        m = S.SdneModel((34, 16, 8, 12), device=-1, batch=17, seed=6, nonzero_weight=beta)
        m.set_rows(X)
        m.train(0, 200, loss=False)
        P = {t: v.astype(np.float64) for t, v in m.export(states=False).items()}
        enc = m.encode().astype(np.float64)
        m.free()
        x = X.astype(np.float64)
        h1 = np.maximum(x @ P["w1"] + P["b1"], 0)
        h2 = np.maximum(h1 @ P["w2"] + P["b2"], 0)
        h3 = np.maximum(h2 @ P["w3"] + P["b3"], 0)
        y = h3 @ P["w4"] + P["b4"]
        err[beta] = float((((y - x) ** 2) * (x != 0)).sum())
        spread[beta] = float(np.sqrt(((enc[:, None, :] - enc[None, :, :]) ** 2).sum(-1)).max())
        print(f"beta {beta}: sum over nonzeros of (y - x)^2 = {err[beta]:.3f}, largest pairwise distance of the "
              f"encodings {spread[beta]:.4g}")
    assert err[5.0] < 0.5 * err[1.0]


# ---- the Python layer -----------------------------------------------------------------------------------------------
def test_sdne_function_with_the_options_on():
    """SDNE(Xtrain, XCV, Xtest) with first_order > 0: Xtrain is square; XCV (shorter than u0) and Xtest (longer) are
    only encoded, in pieces of u0 rows, and equal the encoder applied to those rows."""
    S = _S()
    n = 25
    Xtr = square_rows(n, 1, True)
    rng = np.random.RandomState(2)
    Xcv = (rng.uniform(0.2, 1.0, (4, n)) * (rng.uniform(size=(4, n)) < 0.4)).astype(np.float32)
    Xte = (rng.uniform(0.2, 1.0, (60, n)) * (rng.uniform(size=(60, n)) < 0.4)).astype(np.float32)
    kw = dict(units=(12, 5, 9), steps=6, device=-1, batch=10, seed=3, **ON)
    a, b, c = S.SDNE(Xtr, Xcv, Xte, **kw)
    assert a.shape == (n, 5) and b.shape == (4, 5) and c.shape == (60, 5)
    m = S.SdneModel((n, 12, 5, 9), device=-1, batch=10, seed=3, **ON)
    m.set_rows(Xtr)
    m.train(0, 6)
    P = m.export(states=False)
    assert np.array_equal(m.encode(), a)
    m.free()
    for X, got in ((Xcv, b), (Xte, c)):
        z = np.maximum(X.astype(np.float64) @ P["w1"] + P["b1"], 0) @ P["w2"] + P["b2"]
        assert np.abs(got - z).max() <= 1e-5 * max(1.0, np.abs(z).max())
