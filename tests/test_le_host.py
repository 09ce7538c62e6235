"""CPU: Laplacian eigenmaps on the host (gw_le_*, device = -1) against dense numpy on the 333-vertex SimRank
fixture and against closed forms; the input rules, the error paths, determinism, normalisation, gw_le_apply, the
stand-alone sanitizer program, the Python layer and the command line.

The law (csrc/gw_le_law.h): w_ij = (a_ij + a_ji) / 2 or max, d_i = sum_j w_ij, isolated rows (d_i = 0) left out,
S = D^-1/2 W D^-1/2; D^-1 L f = lambda f  <=>  S u = (1 - lambda) u with f = s o u, s_i = 1 / sqrt(d_i).
"""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import DATA, PKG, ROOT

SIM333 = os.path.join(DATA, "0_333_5038_simrank_navie_top10.txt.sim.txt")
TOL = 1e-8


def _E():
    from gwamd import _lib as C
    from gwamd import eigenmaps
    C.lib()
    return eigenmaps


def fixture_rows():
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


def dense_w(ids, sc, sym):
    """The symmetrised W of the issue's input rules, dense, with the test's own numpy."""
    n = len(ids)
    a = np.zeros((n, n))
    for i in range(n):
        for j, s in zip(ids[i], sc[i]):
            if j == -1:
                break
            if j != i and s > 0:  # NaN > 0 is False
                a[i, j] = s
    return (a + a.T) / 2 if sym == "mean" else np.maximum(a, a.T)


def dense_s(w):
    """(S on the non-isolated rows, their mask, s on them)."""
    d = w.sum(1)
    nz = d > 0
    s = 1 / np.sqrt(d[nz])
    return w[nz][:, nz] * s[:, None] * s[None, :], nz, s


_REF = {}


def reference(sym):
    """Computed once per symmetrisation and shared: rows, W, S, mask, s, and eigh of I - S."""
    if sym not in _REF:
        ids, sc = fixture_rows()
        w = dense_w(ids, sc, sym)
        S, nz, s = dense_s(w)
        lam, U = np.linalg.eigh(np.eye(len(S)) - S)
        for a in (w, S, nz, s, lam, U):
            a.setflags(write=False)
        _REF[sym] = dict(ids=ids, sc=sc, w=w, S=S, nz=nz, s=s, lam=lam, U=U)
    return _REF[sym]


_SOLVED = {}


def solved(sym, dim):
    if (sym, dim) not in _SOLVED:
        E = _E()
        r = reference(sym)
        m = E.Eigenmaps(333, device=-1, dim=dim, block=32, symmetrize=sym, tol=TOL)
        m.set_rows(r["ids"], r["sc"])
        st = m.solve()
        lam, vec, res = m.export()
        _SOLVED[(sym, dim)] = dict(m=m, st=st, lam=lam, vec=vec, res=res, f32=m.vectors_numpy())
    return _SOLVED[(sym, dim)]


# ---- 1, 2: the fixture --------------------------------------------------------------------
@pytest.mark.parametrize("sym", ["mean", "max"])
@pytest.mark.parametrize("dim", [4, 16])
def test_fixture_eigenvalues_and_subspace(sym, dim):
    r, o = reference(sym), solved(sym, dim)
    st = o["st"]
    assert st.state == 0 and st.skipped == 2 and st.isolated == 7 and st.block_used == 32
    assert st.applies == st.iters + (st.iters - 1) * 20
    k = st.skipped
    err = np.abs(o["lam"] - r["lam"][k:k + dim]).max()
    print("eigenvalue error", err, "max residual", st.max_residual)
    assert err <= TOL  # symmetric matrix: |theta - lambda| <= ||r||
    assert np.all(np.diff(o["lam"]) >= 0) and np.all(o["res"] <= TOL) and st.max_residual <= TOL
    assert np.all(o["vec"][~r["nz"]] == 0)
    if dim == 4:  # the wanted set is separated: Davis-Kahan
        gap = r["lam"][k + dim] - r["lam"][k + dim - 1]
        if sym == "mean":
            assert abs(r["lam"][k] - 0.00237) < 1e-5 and abs(r["lam"][k + 3] - 0.00709) < 1e-5
            assert abs(r["lam"][k + 4] - 0.0253) < 1e-4
        Uw = r["U"][:, k:k + dim]
        for c in range(dim):
            u = o["vec"][r["nz"], c] / r["s"]
            u = u / np.linalg.norm(u)
            out = np.linalg.norm(u - Uw @ (Uw.T @ u))
            print("column", c, "outside the wanted subspace", out, "bound", TOL / gap * np.sqrt(dim))
            assert out <= TOL / gap * np.sqrt(dim)


@pytest.mark.parametrize("sym", ["mean", "max"])
def test_fixture_residual_in_the_reference_form(sym):
    """|| D^-1 L f - lambda f || / || f ||, dense, on the non-isolated rows."""
    r, o = reference(sym), solved(sym, 16)
    w = r["w"][r["nz"]][:, r["nz"]]
    D = np.diag(w.sum(1))
    X = np.linalg.inv(D) @ (D - w)
    bound = TOL * r["s"].max() / r["s"].min() + 1e-12
    for c in range(16):
        f = o["vec"][r["nz"], c]
        res = np.linalg.norm(X @ f - o["lam"][c] * f) / np.linalg.norm(f)
        print("column", c, "residual", res, "bound", bound)
        assert res <= bound


# ---- 3: a symmetric input against the reference's dense recipe ------------------------------
def test_symmetric_input_matches_the_dense_recipe():
    E = _E()
    W = reference("mean")["w"]
    n, dim = len(W), 16
    offsets = np.concatenate([[0], np.cumsum((W > 0).sum(1))]).astype(np.int64)
    nbrs = np.concatenate([np.nonzero(W[i])[0] for i in range(n)]).astype(np.int32)
    weights = np.concatenate([W[i][np.nonzero(W[i])[0]] for i in range(n)])
    m = E.Eigenmaps(n, device=-1, dim=dim, block=32, tol=TOL)
    m.set_csr(offsets, nbrs, weights)
    st = m.solve()
    lam, _, _ = m.export()
    # simRank.py:102-121: W, D with 1e-6 on an empty row, eig(D.I * L)
    D = np.diag(np.where(W.sum(1) == 0, 1e-6, W.sum(1)))
    ref = np.sort(np.linalg.eig(np.linalg.inv(D) @ (D - W))[0].real)
    ref = ref[ref > 1e-5][:dim]
    print("against eig(D^-1 L):", np.abs(lam - ref).max())
    assert st.state == 0 and np.abs(lam - ref).max() <= TOL


# ---- 4: closed forms ----------------------------------------------------------------------
def rings(lens, extra=0):
    off, nb, base = [0], [], 0
    for L in lens:
        for i in range(L):
            nb += [base + (i - 1) % L, base + (i + 1) % L]
            off.append(len(nb))
        base += L
    off += [len(nb)] * extra
    return np.asarray(off, np.int64), np.asarray(nb, np.int32)


@pytest.mark.parametrize("block", [8, 32])
def test_ring_of_12(block):
    """lambda_k = 1 - cos(2 pi k / 12) in degenerate pairs; block 32 clamps to the 12 rows and one step is exact."""
    E = _E()
    off, nb = rings([12])
    m = E.Eigenmaps(12, device=-1, dim=4, block=block, cheb_degree=8, tol=TOL)
    m.set_csr(off, nb)
    st = m.solve()
    lam, vec, _ = m.export()
    assert st.state == 0 and st.skipped == 1 and st.isolated == 0
    assert st.block_used == min(block, 12) and (block < 12 or (st.iters == 1 and st.applies == 1))
    want = 1 - np.cos(2 * np.pi * np.array([1, 1, 2, 2]) / 12)
    assert np.abs(lam - want).max() <= TOL
    t = 2 * np.pi * np.arange(12) / 12
    for k, cols in ((1, (0, 1)), (2, (2, 3))):
        B = np.stack([np.cos(k * t), np.sin(k * t)], 1) / np.sqrt(6)  # the eigenspace of lambda_k, orthonormal
        gap = (1 - np.cos(2 * np.pi * (k + 1) / 12)) - (1 - np.cos(2 * np.pi * k / 12))
        for c in cols:
            assert np.linalg.norm(vec[:, c] - B @ (B.T @ vec[:, c])) <= TOL / gap * 2


def test_two_rings_and_an_isolated_vertex():
    E = _E()
    off, nb = rings([12, 9], extra=1)
    m = E.Eigenmaps(22, device=-1, dim=3, block=8, cheb_degree=8, tol=TOL)
    m.set_csr(off, nb)
    st = m.solve()
    lam, vec, _ = m.export()
    assert st.state == 0 and st.skipped == 2 and st.isolated == 1
    assert np.all(vec[21] == 0) and np.all(m.vectors_numpy()[21] == 0)
    want = np.sort(np.concatenate([1 - np.cos(2 * np.pi * np.arange(1, 12) / 12),
                                   1 - np.cos(2 * np.pi * np.arange(1, 9) / 9)]))[:3]
    assert np.abs(lam - want).max() <= TOL


# ---- 5: input rules and error paths ---------------------------------------------------------
def test_input_rules():
    E = _E()
    nan = float("nan")
    ids = np.array([[1, 0, 1, -1, 2], [2, 3, -1, 3, 3], [3, 0, 1, 2, -1], [-1, 0, 1, 2, 1], [0, 0, 0, 0, 0]], np.int32)
    sc = np.array([[.25, 9., .5, 0., 7.], [1., .125, 0., 8., 8.], [nan, -1., 2., 5., 0.], [0., 1., 1., 1., 1.],
                   [0., -3., nan, 0., 0.]])
    # what remains: (0,1) = .5 (the last of the two), (1,2) = 1, (1,3) = .125, (2,1) = 2; rows 3 and 4 list nothing
    a = np.zeros((5, 5))
    a[0, 1], a[1, 2], a[1, 3], a[2, 1] = .5, 1., .125, 2.
    x = np.random.default_rng(0).standard_normal((5, 3))
    for sym, w in (("mean", (a + a.T) / 2), ("max", np.maximum(a, a.T))):
        assert np.array_equal(w, dense_w(ids, sc, sym))
        m = E.Eigenmaps(5, device=-1, dim=1, block=4, symmetrize=sym)
        m.set_rows(ids, sc)
        S, nz, _ = dense_s(w)
        want = np.zeros_like(x)
        want[nz] = S @ x[nz]
        assert np.allclose(m.apply(x), want, rtol=1e-14, atol=1e-15)
        st = m.solve()
        assert st.isolated == 1  # vertex 4; vertex 3 is listed by vertex 1
    bad = ids.copy()
    bad[1, 1] = 5
    with pytest.raises(IndexError):
        m.set_rows(bad, sc)
    bad[1, 1] = -2
    with pytest.raises(IndexError):
        m.set_rows(bad, sc)
    bad[1, 3] = 77  # behind the padding: never read
    bad[1, 1] = 3
    m.set_rows(bad, sc)


def test_error_paths():
    E = _E()
    from gwamd import _lib as C
    with pytest.raises(ValueError):
        E.Eigenmaps(10, device=-1, dim=4, block=4)
    with pytest.raises(ValueError):
        E.Eigenmaps(10, device=-1, dim=0, block=4)
    m = E.Eigenmaps(10, device=-1, dim=2, block=4)
    with pytest.raises(C.StateError):
        m.solve()
    off, nb = rings([12, 9], extra=1)  # two zero eigenvalues: they, dim 2 and one more need a block of 5
    m = E.Eigenmaps(22, device=-1, dim=2, block=4, cheb_degree=8)
    m.set_csr(off, nb)
    with pytest.raises(C.CapacityError, match="block 5 needed"):
        m.solve()
    with pytest.raises(C.StateError):
        m.export()
    m = E.Eigenmaps(22, device=-1, dim=1, block=2)  # nothing but isolated rows
    m.set_csr(np.zeros(23, np.int64), np.zeros(0, np.int32))
    with pytest.raises(C.CapacityError):
        m.solve()


def test_max_iters_one_is_not_converged_and_finite():
    E = _E()
    r = reference("mean")
    m = E.Eigenmaps(333, device=-1, dim=16, block=32, max_iters=1)
    m.set_rows(r["ids"], r["sc"])
    st = m.solve()
    lam, vec, res = m.export()
    assert st.state == 1 and st.iters == 1 and st.applies == 1 and st.max_residual > TOL
    assert np.isfinite(vec).all() and np.isfinite(lam).all() and np.isfinite(res).all()
    assert np.isfinite(m.vectors_numpy()).all()


# ---- 6: determinism --------------------------------------------------------------------------
def _digest(o):
    return hashlib.sha256(o["lam"].tobytes() + o["vec"].tobytes() + o["res"].tobytes() + o["f32"].tobytes()).hexdigest()


CHILD = """
import hashlib, sys
sys.path[:0] = [{root!r}, {pkg!r}, {tests!r}]
import test_le_host as T
T._SOLVED.clear()
print(T._digest(T.solved("mean", 16)))
"""


def test_same_seed_same_bits_for_any_thread_count():
    first = _digest(solved("mean", 16))
    _SOLVED.pop(("mean", 16))
    assert _digest(solved("mean", 16)) == first
    code = CHILD.format(root=ROOT, pkg=PKG, tests=os.path.join(ROOT, "tests"))
    for threads in ("1", "4"):
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True,
                           env=dict(os.environ, OMP_NUM_THREADS=threads))
        assert r.returncode == 0, r.stderr
        assert r.stdout.split()[-1] == first, threads


# ---- 7: normalisation -------------------------------------------------------------------------
@pytest.mark.parametrize("sym", ["mean", "max"])
def test_norm_sign_and_the_fp32_copy(sym):
    o = solved(sym, 16)
    vec = o["vec"]
    assert np.abs(np.linalg.norm(vec, axis=0) - 1).max() <= 1e-15 * 333
    for c in range(16):
        top = int(np.argmax(np.abs(vec[:, c])))  # the lowest row among equals
        assert vec[top, c] > 0
    assert o["f32"].dtype == np.float32 and np.array_equal(o["f32"], vec.astype(np.float32))


# ---- 8: gw_le_apply ---------------------------------------------------------------------------
@pytest.mark.parametrize("sym", ["mean", "max"])
def test_apply_against_numpy(sym):
    r, o = reference(sym), solved(sym, 4)
    x = np.random.default_rng(1).standard_normal((333, 7))
    want = np.zeros_like(x)
    want[r["nz"]] = r["S"] @ x[r["nz"]]
    y = o["m"].apply(x)
    assert np.abs(y - want).max() <= 1e-14 * np.abs(want).max()
    assert np.all(y[~r["nz"]] == 0)


# ---- 9: sanitizers -----------------------------------------------------------------------------
def test_host_check_under_sanitizers(tmp_path):
    """gw_le_host.cpp + host/le_host_check.cpp (its own main) under ASan + UBSan, run as a plain program."""
    exe = str(tmp_path / "le_host_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-static-libasan", "-static-libubsan",
           "-ffp-contract=off", "-DGW_LE_HOST_ONLY", f"-I{os.path.join(ROOT, 'include')}",
           os.path.join(PKG, "csrc", "gw_le_host.cpp"), os.path.join(PKG, "host", "le_host_check.cpp"),
           "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "le host check ok" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr


# ---- 10: the Python layer and the command line ---------------------------------------------------
def test_eigenmaps_function_feeds_scoring_and_neighbors():
    E = _E()
    from gwamd import classify, neighbors
    r = reference("mean")
    emb = E.eigenmaps((r["ids"], r["sc"]), dim=8, device=-1, block=32)
    o = solved("mean", 16)
    assert emb.vectors.shape == (333, 8) and emb.labels[5] == "5" and emb.stats.skipped == 2
    assert np.abs(emb.eigenvalues - o["lam"][:8]).max() <= TOL
    ids, sc = neighbors.most_similar(emb, topk=5, device=-1)
    ids2, sc2 = neighbors.most_similar(emb.vectors, topk=5, device=-1)
    assert np.array_equal(ids, ids2) and np.array_equal(sc, sc2)
    groups = {str(i): [str(i % 3)] for i in range(333)}
    res = classify.scoring(emb, groups, training_percents=[0.5], number_shuffles=1, device=-1, file=open(os.devnull, "w"))
    res2 = classify.scoring(emb.vectors, groups, training_percents=[0.5], number_shuffles=1, device=-1,
                            file=open(os.devnull, "w"))
    assert res == res2


def test_cli_round_trip(tmp_path, capsys):
    E = _E()
    from gwamd import classify
    out, nn, groups = str(tmp_path / "x.emb"), str(tmp_path / "x.nn"), str(tmp_path / "g.csv")
    with open(groups, "w") as f:
        f.writelines(f"{i},{i % 3}\n" for i in range(333))
    assert E.cli(["--simrank", SIM333, "--output", out, "--dimensions", "8", "--block", "32", "--symmetrize", "max",
                  "--min-eigenvalue", "1e-2", "--groups", groups, "--neighbors", nn, "--device", "-1"]) == 0
    labels, X = classify.read_embedding(out)
    lam_all = reference("max")["lam"]
    k = int((lam_all <= 1e-2).sum())  # simRank.py:137's threshold skips more than the two zeros
    m = E.Eigenmaps(333, device=-1, dim=8, block=32, symmetrize="max", min_eigenvalue=1e-2)
    m.set_rows(*fixture_rows())
    st = m.solve()
    assert st.skipped == k > 2
    assert labels == [str(i) for i in range(333)] and np.array_equal(X, m.vectors_numpy())
    assert "Train percent:" in capsys.readouterr().out
    with open(nn) as f:
        assert len(f.readlines()) == 333
    # the graph's own adjacency as W
    out2 = str(tmp_path / "k.emb")
    assert E.cli(["--input", os.path.join(DATA, "karate.edgelist"), "--delimiter", " ", "--output", out2,
                  "--dimensions", "4", "--device", "-1"]) == 0
    labels, X = classify.read_embedding(out2)
    assert len(labels) == 34 and X.shape == (34, 4) and np.isfinite(X).all()
