"""CPU: the one-vs-rest scorer's host side (gw_ovr_*, device = -1) - the optimum
against liblinear, the top-k rule and F1 against sklearn, the structural edges,
the error paths, the law's permutation, and the Python layer (gwamd.classify).

The bounds are derived, not tuned: f_c is 1-strongly convex, so
|w - w*| <= |grad f_c(w)|, and two approximate minimisers are no further apart
than the sum of their gradient norms (both recomputed here in numpy fp64).
"""
import ctypes
import io
import os
import subprocess

import numpy as np
import pytest

from conftest import DATA, PKG, ROOT

GROUPS = os.path.join(DATA, "blog_groups.csv")
EPS = np.finfo(np.float64).eps


def _C():
    from gwamd import _lib as C
    C.lib()
    return C


def _K():
    from gwamd import classify
    _C()
    return classify


# ---- data ----------------------------------------------------------------------------
def planted(n, d, L, seed, extra=0.1, noise=1.0):
    """Label centroids plus noise: X float32 [n][d], Y bool [n][L] (a primary label, `extra` more at random)."""
    rs = np.random.RandomState(seed)
    cen = rs.randn(L, d)
    lab = rs.randint(0, L, n)
    Y = np.zeros((n, L), bool)
    Y[np.arange(n), lab] = True
    Y |= rs.rand(n, L) < extra
    X = ((Y @ cen) / np.sqrt(Y.sum(1, keepdims=True)) + noise * rs.randn(n, d)).astype(np.float32)
    return X, Y


def csr(Y):
    Y = np.asarray(Y, bool)
    return np.concatenate([[0], np.cumsum(Y.sum(1))]).astype(np.int64), np.nonzero(Y)[1].astype(np.int32)


def scorer(X, Y, device=-1, **kw):
    m = _K().OneVsRest(X.shape[0], Y.shape[1], device=device, dim=kw.pop("dim", X.shape[1]), **kw)
    m.set_features(X)
    m.set_labels(*csr(Y))
    return m


def tilde(X):
    return np.hstack([np.asarray(X, np.float64), np.ones((len(X), 1))])


def grad(Xt, y, w, C=1.0):
    """grad f_c(w) in numpy fp64 (sigma without cancellation at either end)."""
    z = Xt @ w
    e = np.exp(-np.abs(z))
    sig = np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
    return w + C * (Xt.T @ (sig - y))


def grad_slack(Xt, w, C=1.0):
    """The rounding of grad() itself: each of its len(Xt) + 1 terms per entry is good to a few ulps."""
    return 8 * EPS * (np.linalg.norm(w) + C * np.linalg.norm(Xt, axis=1).sum())


def rule_counts(z, Y):
    """TopKRanker on decision values: argsort (stable) and the last k; tp / fp / fn per label."""
    P = np.zeros_like(Y, bool)
    for i in range(len(z)):
        k = int(Y[i].sum())
        if k:
            P[i, np.argsort(z[i], kind="stable")[-k:]] = True
    return np.stack([(P & Y).sum(0), (P & ~Y).sum(0), (~P & Y).sum(0)], 1).astype(np.int64), P


# ---- the three cases of the optimum / prediction tests ----------------------------------
# seeds: chosen so that sklearn's own decision values meet the gap condition of test_predictions_and_f1
CASES = {"65x5x3": 1, "100x16x7": 1, "blog": 2}
_cache = {}


def case(name):
    """(X, Y, order, train_count), computed once."""
    if name in _cache:
        return _cache[name]
    K = _K()
    seed = CASES[name]
    if name == "blog":
        groups = K.read_groups(GROUPS)
        _, names, row_off, ids = K.groups_csr(groups)
        n, L, d = len(row_off) - 1, len(names), 128
        Y = np.zeros((n, L), bool)
        Y[np.repeat(np.arange(n), np.diff(row_off)), ids] = True
        rs = np.random.RandomState(seed)
        cen = rs.randn(L, d)
        X = ((Y @ cen) / np.sqrt(np.maximum(Y.sum(1, keepdims=True), 1)) + 0.5 * rs.randn(n, d)).astype(np.float32)
        order = K.order(seed, 0, n)
        T = K.training_size(0.1, n)
    else:
        T, d, L = (int(t) for t in name.split("x"))
        n = T + 40
        X, Y = planted(n, d, L, seed)
        order = np.random.RandomState(seed + 100).permutation(n).astype(np.int64)
    _cache[name] = (X, Y, order, T)
    return _cache[name]


def ours(name):
    key = ("ours", name)
    if key not in _cache:
        X, Y, order, T = case(name)
        m = scorer(X, Y)
        st = m.fit(order, T)
        _cache[key] = (m, m.export(), st)
    return _cache[key]


def sk(name):
    """liblinear's weights per label (None for a constant column) on the case's training rows."""
    key = ("sk", name)
    if key not in _cache:
        LogisticRegression = pytest.importorskip("sklearn.linear_model").LogisticRegression
        X, Y, order, T = case(name)
        tr = order[:T]
        Xd = np.asarray(X[tr], np.float64)
        W = []
        for c in range(Y.shape[1]):
            y = Y[tr, c]
            if y.all() or not y.any():
                W.append(None)
                continue
            clf = LogisticRegression(solver="liblinear", C=1, tol=1e-10, max_iter=10000).fit(Xd, y)
            W.append(np.concatenate([clf.coef_[0], clf.intercept_]))
        _cache[key] = W
    return _cache[key]


def weight_bounds(name):
    """Per fitted label: |grad f(w_ours)| + |grad f(w_sklearn)| and the test's own rounding on top."""
    X, Y, order, T = case(name)
    tr = order[:T]
    Xt = tilde(X[tr])
    e, W = ours(name)[1], sk(name)
    out = {}
    for c, ws in enumerate(W):
        if ws is None:
            continue
        y = Y[tr, c].astype(np.float64)
        wo = e["W"][c]
        out[c] = (np.linalg.norm(grad(Xt, y, wo)) + np.linalg.norm(grad(Xt, y, ws)) + grad_slack(Xt, wo) +
                  grad_slack(Xt, ws) + 16 * EPS * np.linalg.norm(wo))
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_optimum(name):
    C = _C()
    X, Y, order, T = case(name)
    tr = order[:T]
    Xt = tilde(X[tr])
    m, e, st = ours(name)
    W = sk(name)
    const = [c for c in range(Y.shape[1]) if W[c] is None]
    if name == "blog":
        assert const, "BlogCatalog at a 10 % split has labels absent from training"
    assert st.not_converged == 0 and st.constant == len(const) and st.fitted == Y.shape[1] - len(const)
    gtol = m.params.gtol
    bounds = weight_bounds(name)
    worst = 0.0
    for c in range(Y.shape[1]):
        y = Y[tr, c].astype(np.float64)
        if W[c] is None:
            assert e["state"][c] == (C.OVR_CONST_POS if y.all() else C.OVR_CONST_NEG)
            assert not e["W"][c].any()
            continue
        assert e["state"][c] == C.OVR_FITTED
        w = e["W"][c]
        g, g0 = np.linalg.norm(grad(Xt, y, w)), np.linalg.norm(grad(Xt, y, np.zeros_like(w)))
        # the law's own stop condition (c), recomputed
        assert g <= gtol * g0 + grad_slack(Xt, w), (c, g, g0)
        assert abs(e["gnorm"][c] - g) <= grad_slack(Xt, w)
        dist = np.linalg.norm(w - W[c])
        assert dist <= bounds[c], (c, dist, bounds[c])
        worst = max(worst, dist / np.linalg.norm(W[c]))
    print(f"{name}: passes {st.passes}, newton max {st.newton_max}, worst relative distance to liblinear {worst:.2e}")


@pytest.mark.parametrize("name", list(CASES))
def test_predictions_and_f1(name):
    f1_score = pytest.importorskip("sklearn.metrics").f1_score
    K = _K()
    X, Y, order, T = case(name)
    te = order[T:]
    Xt = tilde(X[te])
    m = ours(name)[0]
    W = sk(name)
    bounds = weight_bounds(name)
    bound = max(bounds.values())
    tr = order[:T]
    Z = np.empty((len(te), Y.shape[1]))
    for c, ws in enumerate(W):
        Z[:, c] = Xt @ ws if ws is not None else (np.inf if Y[tr, c].all() else -np.inf)
    # every test row: sklearn's k-th and (k+1)-th decision values are further apart than both sides' error
    xn = np.linalg.norm(Xt, axis=1)
    for i in range(len(te)):
        k = int(Y[te[i]].sum())
        if 0 < k < Y.shape[1]:
            s = np.sort(Z[i])[::-1]
            gap = 0.0 if s[k - 1] == s[k] else s[k - 1] - s[k]
            assert gap > 2 * bound * xn[i], (i, k, gap, 2 * bound * xn[i])
    ref, P = rule_counts(Z, Y[te])
    counts = m.score(te)
    assert np.array_equal(counts, ref)
    f = K.f1_from_counts(counts)
    assert abs(f["micro"] - f1_score(Y[te], P, average="micro", zero_division=0)) <= 1e-12
    assert abs(f["macro"] - f1_score(Y[te], P, average="macro", zero_division=0)) <= 1e-12
    present = (Y[te] | P).any(0)
    assert abs(f["macro_present"] - f1_score(Y[te][:, present], P[:, present], average="macro",
                                              zero_division=0)) <= 1e-12
    # the counts are the rule on the scorer's own decision values too
    assert np.array_equal(rule_counts(m.decision(te), Y[te])[0], counts)


# ---- edges ---------------------------------------------------------------------------
def test_single_label():
    X, Y = planted(90, 4, 2, 5)
    Y = Y[:, :1]
    m = scorer(X, Y)
    m.fit(np.arange(90), 60)
    e = m.export()
    assert e["state"][0] == _C().OVR_FITTED and e["W"].shape == (1, 5)
    te = np.arange(60, 90)
    # one label: a row with k = 1 gets it, a row with k = 0 nothing
    assert np.array_equal(m.score(te), [[int(Y[te].sum()), 0, 0]])


def test_train_count_one_and_all():
    C, K = _C(), _K()
    X, Y = planted(50, 3, 4, 6)
    m = scorer(X, Y)
    st = m.fit(np.arange(50), 1)
    e = m.export()
    assert st.constant == 4 and st.passes == 0
    assert np.array_equal(e["state"], np.where(Y[0], C.OVR_CONST_POS, C.OVR_CONST_NEG))
    z = m.decision(np.arange(1, 50))
    assert np.array_equal(z, np.broadcast_to(np.where(Y[0], np.inf, -np.inf), z.shape))
    assert np.array_equal(m.score(np.arange(1, 50)), rule_counts(z, Y[1:])[0])
    m.fit(np.arange(50), 50)
    counts = m.score(np.arange(0))
    assert not counts.any()
    assert K.f1_from_counts(counts) == {"micro": 0.0, "macro": 0.0, "macro_present": 0.0}


def test_rows_with_no_and_every_label_and_infinite_columns():
    C = _C()
    X, Y = planted(120, 6, 6, 7)
    Y[:, 4] = False          # never positive: -inf, ranked last
    Y[:, 5] = True           # always positive in training: +inf, ranked first
    Y[100] = False           # k = 0
    Y[101] = True            # k = L
    Y[102:110, 5] = False    # test rows that do not carry the constant-positive label
    m = scorer(X, Y)
    m.fit(np.arange(120), 100)
    e = m.export()
    assert e["state"][4] == C.OVR_CONST_NEG and e["state"][5] == C.OVR_CONST_POS
    te = np.arange(100, 120)
    z = m.decision(te)
    assert np.isneginf(z[:, 4]).all() and np.isposinf(z[:, 5]).all() and np.isfinite(z[:, :4]).all()
    ref, P = rule_counts(z, Y[te])
    counts = m.score(te)
    assert np.array_equal(counts, ref)
    assert not P[0].any() and P[1].all()
    # +inf is predicted for every row with k >= 1 (a false positive where the row lacks it); -inf only at k = L
    assert counts[5, 0] + counts[5, 1] == (Y[te].sum(1) >= 1).sum() and counts[5, 1] >= 1
    assert counts[4, 0] == 1 and counts[4, 1] == 0


def test_exact_tie_goes_to_the_larger_index():
    X, Y = planted(150, 5, 4, 8, extra=0.3)
    Y[:, 3] = Y[:, 1]        # two identical label columns: identical weights, identical decision values
    m = scorer(X, Y)
    m.fit(np.arange(150), 100)
    e = m.export()
    assert np.array_equal(e["W"][1].view(np.uint64), e["W"][3].view(np.uint64))
    te = np.arange(100, 150)
    z = m.decision(te)
    assert np.array_equal(z[:, 1], z[:, 3])
    ref, P = rule_counts(z, Y[te])
    assert np.array_equal(m.score(te), ref)
    split = P[:, 3] & ~P[:, 1]
    assert split.any() and not (P[:, 1] & ~P[:, 3]).any()


def test_single_positive_label():
    C = _C()
    X, Y = planted(80, 4, 3, 9)
    Y[:, 2] = False
    Y[17, 2] = True
    m = scorer(X, Y)
    m.fit(np.arange(80), 80)
    e = m.export()
    assert e["state"][2] == C.OVR_FITTED
    Xt = tilde(X)
    y = Y[:, 2].astype(np.float64)
    g, g0 = np.linalg.norm(grad(Xt, y, e["W"][2])), np.linalg.norm(grad(Xt, y, np.zeros(5)))
    assert g <= m.params.gtol * g0 + grad_slack(Xt, e["W"][2])


def test_labels_converge_apart_and_a_frozen_label_changes_nothing():
    """Labels that need different Newton counts: the faster one is frozen while the slower runs on, and the slower
    one fitted alone gives the same bits."""
    X, Y = planted(100, 16, 7, 1)
    m = scorer(X, Y)
    m.fit(np.arange(100), 100)
    e = m.export()
    it = e["newton_iters"]
    assert it.min() < it.max()
    slow = int(np.argmax(it))
    alone = scorer(X, Y[:, slow:slow + 1])
    alone.fit(np.arange(100), 100)
    ea = alone.export()
    assert ea["newton_iters"][0] == it[slow]
    assert np.array_equal(ea["W"][0].view(np.uint64), e["W"][slow].view(np.uint64))
    assert ea["gnorm"][0] == e["gnorm"][slow]


def test_max_newton_one_reports_not_converged():
    C = _C()
    X, Y = planted(100, 16, 7, 1)
    m = scorer(X, Y, max_newton=1)
    st = m.fit(np.arange(100), 100)
    e = m.export()
    assert st.not_converged == 7 and (e["state"] == C.OVR_NOT_CONVERGED).all() and (e["newton_iters"] == 1).all()
    assert e["W"].any(1).all()     # the last accepted iterate, not zeros


def test_two_fits_are_identical():
    X, Y = planted(130, 9, 5, 11)
    o = np.random.RandomState(0).permutation(130)
    a, b = scorer(X, Y), scorer(X, Y)
    a.fit(o, 90)
    b.fit(o, 90)
    assert np.array_equal(a.export()["W"].view(np.uint64), b.export()["W"].view(np.uint64))
    a.fit(o, 40)       # a handle fits again from scratch
    a.fit(o, 90)
    assert np.array_equal(a.export()["W"].view(np.uint64), b.export()["W"].view(np.uint64))


def test_pitch_and_nan_pad():
    X, Y = planted(70, 5, 3, 12)
    wide = np.full((70, 8), np.nan, np.float32)
    wide[:, :5] = X
    a, b = scorer(X, Y), scorer(wide, Y, dim=5)
    a.fit(np.arange(70), 50)
    b.fit(np.arange(70), 50)
    assert np.array_equal(a.export()["W"].view(np.uint64), b.export()["W"].view(np.uint64))
    assert np.array_equal(a.score(np.arange(50, 70)), b.score(np.arange(50, 70)))


# ---- errors and plumbing ---------------------------------------------------------------
def test_errors():
    C, K = _C(), _K()
    X, Y = planted(30, 3, 4, 13)
    ro, ids = csr(Y)
    m = K.OneVsRest(30, 4, device=-1, dim=3)
    o = np.arange(30)
    with pytest.raises(C.StateError):
        m.fit(o, 10)
    m.set_features(X)
    with pytest.raises(C.StateError):
        m.fit(o, 10)
    bad = ids.copy()
    bad[3] = 4
    with pytest.raises(IndexError):
        m.set_labels(ro, bad)
    bad[3] = -1
    with pytest.raises(IndexError):
        m.set_labels(ro, bad)
    with pytest.raises(C.StateError):      # a failed set_labels leaves none
        m.fit(o, 10)
    m.set_labels(ro, ids)
    for call in (lambda: m.score(o), lambda: m.decision(o), m.export):
        with pytest.raises(C.StateError):
            call()
    for count in (0, -1):
        with pytest.raises(ValueError):
            m.fit(o, count)
    L = C.lib()
    assert L.gw_ovr_fit(m.handle, C.ptr(o), 31, None, None) == C.GW_ERR_INVALID
    dup = o.copy()
    dup[5] = dup[2]
    with pytest.raises(ValueError):
        m.fit(dup, 10)
    m.fit(dup, 5)                           # the repeat lies past train_count
    for v in (30, -1):
        far = o.copy()
        far[1] = v
        m.fit(o, 10)
        with pytest.raises(IndexError):
            m.score(far)
        with pytest.raises(IndexError):
            m.decision(far)
        with pytest.raises(IndexError):
            m.fit(far, 10)
        with pytest.raises(C.StateError):   # a failing fit leaves the handle unfitted
            m.score(o)
    assert L.gw_ovr_set_features(m.handle, C.ptr(X), 2) == C.GW_ERR_INVALID      # pitch below dim
    assert L.gw_ovr_set_features(m.handle, None, 3) == C.GW_ERR_INVALID
    h = ctypes.c_void_p()
    for kw in (dict(labels=0), dict(labels=2, dim=0), dict(labels=2, max_newton=0), dict(labels=2, max_cg=0),
               dict(labels=2, C=0.0), dict(labels=2, gtol=1.0), dict(labels=2, gtol=-1e-9)):
        p = C.OvrParams(**kw)
        assert L.gw_ovr_create(-1, 10, ctypes.byref(p), ctypes.byref(h)) == C.GW_ERR_INVALID, kw
    p = C.OvrParams(labels=2)
    assert L.gw_ovr_create(-1, 0, ctypes.byref(p), ctypes.byref(h)) == C.GW_ERR_INVALID
    assert L.gw_ovr_create(-2, 10, ctypes.byref(p), ctypes.byref(h)) == C.GW_ERR_INVALID
    assert b"device" in L.gw_ovr_last_error(None)
    # the device limits are checked before any device is touched; the host path takes any size
    for kw in (dict(labels=2, dim=1025), dict(labels=1025, dim=4)):
        p = C.OvrParams(**kw)
        assert L.gw_ovr_create(0, 10, ctypes.byref(p), ctypes.byref(h)) == C.GW_ERR_UNSUPPORTED
        assert L.gw_ovr_create(-1, 10, ctypes.byref(p), ctypes.byref(h)) == C.GW_OK
        L.gw_ovr_free(h)
    with pytest.raises(C.StateError):
        m.kernel_attrs()


def test_struct_size_shorter_than_the_librarys():
    """Only struct_size bytes are read: what lies past them keeps the defaults, whatever the caller's memory holds."""
    C = _C()
    L = C.lib()
    p = C.OvrParams(labels=3, dim=4, max_newton=-7, max_cg=-7, C=-1.0, gtol=5.0)
    p.struct_size = 12     # struct_size, dim, labels
    h = ctypes.c_void_p()
    assert L.gw_ovr_create(-1, 60, ctypes.byref(p), ctypes.byref(h)) == C.GW_OK
    X, Y = planted(60, 4, 3, 14)
    ro, ids = csr(Y)
    o = np.arange(60, dtype=np.int64)
    assert L.gw_ovr_set_features(h, C.ptr(X), 4) == 0 and L.gw_ovr_set_labels(h, C.ptr(ro), C.ptr(ids)) == 0
    assert L.gw_ovr_fit(h, C.ptr(o), 60, None, None) == 0
    W = np.empty((3, 5))
    assert L.gw_ovr_export(h, C.ptr(W), None, None, None) == 0
    L.gw_ovr_free(h)
    ref = scorer(X, Y)
    ref.fit(o, 60)
    assert np.array_equal(W.view(np.uint64), ref.export()["W"].view(np.uint64))
    p.struct_size = 3
    assert L.gw_ovr_create(-1, 60, ctypes.byref(p), ctypes.byref(h)) == C.GW_ERR_INVALID


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 10312])
def test_order_is_a_bijection(n):
    K = _K()
    o = K.order(5, 0, n)
    assert np.array_equal(np.sort(o), np.arange(n))
    if n >= 63:
        assert not np.array_equal(o, K.order(6, 0, n)) and not np.array_equal(o, K.order(5, 1, n))
        assert not np.array_equal(o, K.order(5, 1 << 32, n)) and not np.array_equal(o, K.order(5 + (1 << 32), 0, n))
        assert not np.array_equal(o, np.arange(n))
    assert np.array_equal(o, K.order(5, 0, n))


# ---- the Python layer -------------------------------------------------------------------
def test_read_groups_fixture():
    K = _K()
    groups = K.read_groups(GROUPS)
    nodes, names, row_off, ids = K.groups_csr(groups)
    assert len(groups) == 10312 and len(names) == 39 and sum(len(v) for v in groups.values()) == 14476
    assert nodes[0] == "1" and nodes[-1] == "10312" and names == [str(i) for i in range(1, 40)]
    assert row_off[-1] == 14476 and len(ids) == 14476 and np.bincount(ids, minlength=39).min() == 8


def test_training_sizes_are_the_references():
    K = _K()
    percents = np.asarray(range(1, 10)) * .1
    assert [K.training_size(p, 10312) for p in percents] == [1031, 2062, 3093, 4124, 5156, 6187, 7218, 8249, 9280]
    assert percents[2] != 0.3 and K.training_size(percents[2], 10) == 3 and K.training_size(0.7, 10) == 7


def reference_scoring(X, Y, orders, percents):
    """classify.scoring restated with today's sklearn (liblinear is what its LogisticRegression(penalty='l2')
    ran), fed the given permutations; also the smallest gap margin met."""
    from sklearn.linear_model import LogisticRegression
    from sklearn.metrics import f1_score
    from sklearn.multiclass import OneVsRestClassifier
    out = {}
    for p in percents:
        for o in orders:
            T = int(p * X.shape[0])
            tr, te = o[:T], o[T:]
            clf = OneVsRestClassifier(LogisticRegression(solver="liblinear", C=1, tol=1e-10, max_iter=10000))
            clf.fit(np.asarray(X[tr], np.float64), Y[tr])
            Z = np.empty((len(te), Y.shape[1]))
            for c, est in enumerate(clf.estimators_):
                Z[:, c] = (est.decision_function(np.asarray(X[te], np.float64)) if hasattr(est, "coef_")
                           else (np.inf if Y[tr, c].all() else -np.inf))
            _, P = rule_counts(Z, Y[te])
            out.setdefault(p, []).append({a: f1_score(Y[te], P, average=a, zero_division=0) for a in ("micro", "macro")})
    return out


def test_scoring_equals_the_reference_restated(capsys):
    pytest.importorskip("sklearn")
    K = _K()
    X, Y = planted(300, 16, 5, 21, noise=0.7)
    orders = [np.random.RandomState(s).permutation(300).astype(np.int64) for s in (1, 2)]
    percents = np.asarray(range(1, 10)) * .1
    got = K.scoring(X, csr(Y), training_percents=percents, orders=orders, device=-1)
    ref = reference_scoring(X, Y, orders, percents)
    assert sorted(got) == sorted(ref)
    for p in ref:
        assert len(got[p]) == 2
        for a, b in zip(got[p], ref[p]):
            assert abs(a["micro"] - b["micro"]) <= 1e-12 and abs(a["macro"] - b["macro"]) <= 1e-12
    out = capsys.readouterr().out.splitlines()
    assert out[:2] == [str(got[percents[0]][0]["micro"]), str(got[percents[0]][0]["macro"])]
    assert out[36] == "Results, using embeddings of dimensionality 16" and out[37] == "-------------------"
    assert out[38] == f"Train percent: {percents[0]}"
    assert out[39] == str({"micro": got[percents[0]][0]["micro"], "macro": got[percents[0]][0]["macro"]})
    assert out[41] == "-------------------" and out[42] == f"Train percent: {percents[1]}"
    assert len(out) == 36 + 2 + 9 * 4


def test_scoring_default_orders_are_the_laws():
    K = _K()
    X, Y = planted(200, 8, 4, 22)
    buf = io.StringIO()
    a = K.scoring(X, csr(Y), training_percents=[0.5], number_shuffles=2, seed=9, device=-1, file=buf)
    b = K.scoring(X, csr(Y), training_percents=[0.5], orders=[K.order(9, 0, 200), K.order(9, 1, 200)], device=-1,
                  file=buf)
    assert a == b and len(a[0.5]) == 2 and a[0.5][0] != a[0.5][1]


def test_cli_prints_the_references_table(tmp_path, capsys):
    K = _K()
    X, Y = planted(120, 6, 3, 23)
    emb, grp = tmp_path / "x.emb", tmp_path / "groups.csv"
    rows = np.random.RandomState(0).permutation(120)      # the file's row order is not the label order
    with open(emb, "w") as f:
        f.write("120 6\n")
        for v in rows:
            f.write(f"{v + 1} " + " ".join(repr(float(t)) for t in X[v]) + "\n")
    with open(grp, "w") as f:
        for v in range(120):
            for c in np.nonzero(Y[v])[0]:
                f.write(f"{v + 1},{c + 1}\n")
    labels, E = K.read_embedding(str(emb))
    assert labels == [str(v + 1) for v in rows] and np.array_equal(E, X[rows])
    assert K.cli(["--emb", str(emb), "--groups", str(grp), "--device", "-1", "--shuffles", "1"]) == 0
    out = capsys.readouterr().out.splitlines()
    i = out.index("Results, using embeddings of dimensionality 6")
    assert i == 18 and out[i + 1] == "-------------------" and out[i + 2] == "Train percent: 0.1"
    assert out[i + 3].startswith("{'micro': ") and ", 'macro': " in out[i + 3]
    direct = K.scoring(X[rows], csr(Y[rows]), number_shuffles=1, device=-1, file=io.StringIO())
    assert out[i + 3] == str({k: direct[0.1][0][k] for k in ("micro", "macro")})


def test_host_check_under_sanitizers(tmp_path):
    """gw_ovr_host.cpp + host/ovr_host_check.cpp (its own main) under ASan + UBSan, run as a plain program."""
    exe = str(tmp_path / "ovr_host_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-static-libasan", "-static-libubsan",
           "-ffp-contract=off", "-DGW_OVR_HOST_ONLY", f"-I{os.path.join(ROOT, 'include')}",
           os.path.join(PKG, "csrc", "gw_ovr_host.cpp"), os.path.join(PKG, "host", "ovr_host_check.cpp"),
           "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ovr host check ok" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr
