"""CPU: the nearest-neighbour host side (gw_knn_*, device = -1) - exact on an integer grid, against numpy fp64
on Gaussian rows, the error paths, gw_topk_label_agreement, the writers and the Python layer (gwamd.neighbors).

The law (csrc/gw_knn_law.h): dot(i,j) is an fma chain over k ascending in fp64 on the widened fp32 features,
cosine is dot / (nrm(i) * nrm(j)), a row lists the topk candidates j != v by score descending, then id ascending,
padded with (-1, 0.0).
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT


def _C():
    from gwamd import _lib as C
    C.lib()
    return C


def _N():
    from gwamd import neighbors
    _C()
    return neighbors


# ---- references ------------------------------------------------------------------------
def numpy_rows(x, topk, metric, sources=None):
    """The issue's numpy reference: g = x @ x.T, n = sqrt(diag g), g / (n[:,None]*n[None,:]), a stable sort by
    (-score, id); rows of zero norm list nothing and are listed nowhere (cosine), NaN scores are dropped."""
    x = np.asarray(x, np.float64)
    g = x @ x.T
    if metric == "cosine":
        n = np.sqrt(np.diag(g))
        with np.errstate(invalid="ignore", divide="ignore"):
            s = g / (n[:, None] * n[None, :])
        s[n == 0, :] = np.nan
        s[:, n == 0] = np.nan
    else:
        s = g
    src = np.arange(len(x)) if sources is None else np.asarray(sources)
    ids = np.full((len(src), topk), -1, np.int32)
    sc = np.zeros((len(src), topk), np.float64)
    for r, v in enumerate(src):
        row = s[v].copy()
        row[v] = np.nan
        cand = np.nonzero(~np.isnan(row))[0]
        o = cand[np.argsort(-row[cand], kind="stable")][:topk]
        ids[r, :len(o)] = o
        sc[r, :len(o)] = row[o]
    return ids, sc


def grid(seed=3):
    """The integer grid of test 1: every partial sum is a small integer, so any order gives the same bits."""
    rng = np.random.default_rng(seed)
    x = rng.integers(-3, 4, (300, 6)).astype(np.float32)
    x[17] = x[5]
    x[123] = x[5]
    x[299] = x[200]
    x[42] = 0
    return x


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.int64), np.asarray(b, np.float64).view(np.int64))


# ---- 1: integer grid, exact -----------------------------------------------------------------
@pytest.mark.parametrize("metric", ["cosine", "dot"])
@pytest.mark.parametrize("topk", [8, 299])
def test_integer_grid_is_exact(metric, topk):
    N = _N()
    x = grid()
    ids, sc = N.most_similar(x, topk=topk, metric=metric, device=-1)
    rid, rsc = numpy_rows(x, topk, metric)
    assert np.array_equal(ids, rid)
    assert same_bits(sc, rsc)
    if metric == "cosine":
        assert (ids[42] == -1).all() and not (ids == 42).any()          # the zero row
        row = list(ids[5])                                              # duplicates: equal bits, ties by id
        assert row.index(17) + 1 == row.index(123) and sc[5, row.index(17)] == sc[5, row.index(123)]
    if topk == 299:
        listed = (ids >= 0).sum(1)
        want = 298 if metric == "cosine" else 299
        assert (np.delete(listed, 42) == want).all() and (sc[ids < 0] == 0.0).all()


# ---- 2: Gaussian, fp32 inputs ------------------------------------------------------------------
@pytest.mark.parametrize("V,d,topk,seed", [(1000, 20, 10, 0), (700, 130, 20, 1), (300, 5, 8, 2)])
def test_gaussian_against_numpy_fp64(V, d, topk, seed):
    N = _N()
    x = np.random.default_rng(seed).standard_normal((V, d)).astype(np.float32)
    for metric in ("cosine", "dot"):
        ids, sc = N.most_similar(x, topk=topk, metric=metric, device=-1)
        rid, rsc = numpy_rows(x, topk + 1, metric)
        if metric == "cosine":
            gap = np.abs(np.diff(rsc, axis=1)).min()
            print(f"({V}, {d}, {topk}, {seed}): smallest gap among the top-(k+1) scores {gap:.2e}")
        assert np.array_equal(ids, rid[:, :topk])          # every row
        assert np.allclose(sc, rsc[:, :topk], rtol=1e-12, atol=0.0)


def test_sources_repeat_unordered_and_pitch():
    N = _N()
    x = np.random.default_rng(5).standard_normal((60, 7)).astype(np.float32)
    wide = np.full((60, 10), np.nan, np.float32)
    wide[:, :7] = x
    src = np.array([59, 3, 3, 0, 41, 59], np.int32)
    full = N.most_similar(x, topk=5, device=-1)
    a = N.most_similar(x, sources=src, topk=5, device=-1)
    assert np.array_equal(a[0], full[0][src]) and same_bits(a[1], full[1][src])
    m = N.Neighbors(60, device=-1, dim=7, topk=5)
    m.set_vectors(wide[:, :7])       # pitch 10: the NaN pads are never read
    b = m.query(src)
    assert np.array_equal(a[0], b[0]) and same_bits(a[1], b[1])
    # the last row allocated without its pad
    flat = np.full(60 * 10 - 3, np.nan, np.float32)
    flat[:] = wide.reshape(-1)[:597]
    m.set_vectors(flat.ctypes.data, pitch=10)
    c = m.query(src)
    assert np.array_equal(a[0], c[0]) and same_bits(a[1], c[1])
    m.free()


# ---- 3: error paths ---------------------------------------------------------------------------------
def test_errors():
    C, N = _C(), _N()
    L = C.lib()
    x = np.random.default_rng(6).standard_normal((30, 4)).astype(np.float32)
    m = N.Neighbors(30, device=-1, dim=4, topk=3)
    with pytest.raises(C.StateError):
        m.query()
    m.set_vectors(x)
    ids = np.full((3, 3), 77, np.int32)
    sc = np.full((3, 3), 77.0)
    for v in (30, -1):
        src = np.array([1, v, 2], np.int32)
        assert L.gw_knn_query(m.handle, C.ptr(src), 3, C.ptr(ids), C.ptr(sc), None) == C.GW_ERR_RANGE
        assert (ids == 77).all() and (sc == 77.0).all()     # checked before anything is written
        with pytest.raises(IndexError):
            m.query(src)
    src = np.array([1, 2, 3], np.int32)
    assert L.gw_knn_query(m.handle, C.ptr(src), 0, None, None, None) == C.GW_OK        # nsrc = 0: a no-op
    assert L.gw_knn_query(m.handle, C.ptr(src), 0, C.ptr(ids), C.ptr(sc), None) == C.GW_OK and (ids == 77).all()
    assert L.gw_knn_query(m.handle, C.ptr(src), -1, C.ptr(ids), C.ptr(sc), None) == C.GW_ERR_INVALID
    assert L.gw_knn_query(m.handle, C.ptr(src), 3, None, C.ptr(sc), None) == C.GW_ERR_INVALID
    assert L.gw_knn_set_vectors(m.handle, C.ptr(x), 3) == C.GW_ERR_INVALID             # pitch below dim
    assert L.gw_knn_set_vectors(m.handle, None, 4) == C.GW_ERR_INVALID
    with pytest.raises(C.StateError):
        m.tiles()
    with pytest.raises(C.StateError):
        m.kernel_attrs()
    m.set_rows(20)                                           # another row count: the vectors must be set again
    with pytest.raises(C.StateError):
        m.query()
    m.set_vectors(x[:20])
    assert np.array_equal(m.query()[0], N.most_similar(x[:20], topk=3, device=-1)[0])
    m.free()
    h = ctypes.c_void_p()
    for kw in (dict(dim=0), dict(topk=0), dict(dim=-3), dict(metric=2), dict(metric=-1)):
        p = C.KnnParams(**kw)
        assert L.gw_knn_create(-1, 10, ctypes.byref(p), ctypes.byref(h)) == C.GW_ERR_INVALID, kw
    p = C.KnnParams()
    p.struct_size = 3
    assert L.gw_knn_create(-1, 10, ctypes.byref(p), ctypes.byref(h)) == C.GW_ERR_INVALID
    assert b"struct_size" in L.gw_knn_last_error(None)
    p = C.KnnParams()
    assert L.gw_knn_create(-1, 0, ctypes.byref(p), ctypes.byref(h)) == C.GW_ERR_INVALID
    assert L.gw_knn_create(-2, 10, ctypes.byref(p), ctypes.byref(h)) == C.GW_ERR_INVALID
    # the device limits are checked before any device is touched; the host path takes any size
    for kw, n in ((dict(dim=1025), 10), (dict(topk=129), 10), (dict(), 1 << 31)):
        p = C.KnnParams(**kw)
        assert L.gw_knn_create(0, n, ctypes.byref(p), ctypes.byref(h)) == C.GW_ERR_UNSUPPORTED
        assert L.gw_knn_create(-1, n, ctypes.byref(p), ctypes.byref(h)) == C.GW_OK
        L.gw_knn_free(h)


def test_struct_size_shorter_than_the_librarys():
    """Only struct_size bytes are read: what lies past them keeps the defaults (topk 20, cosine)."""
    C, N = _C(), _N()
    L = C.lib()
    p = C.KnnParams(dim=4, topk=-7, metric=9)
    p.struct_size = 8      # struct_size, dim
    h = ctypes.c_void_p()
    assert L.gw_knn_create(-1, 40, ctypes.byref(p), ctypes.byref(h)) == C.GW_OK
    x = np.random.default_rng(7).standard_normal((40, 4)).astype(np.float32)
    ids, sc = np.empty((40, 20), np.int32), np.empty((40, 20))
    assert L.gw_knn_set_vectors(h, C.ptr(x), 4) == 0
    assert L.gw_knn_query(h, None, 0, C.ptr(ids), C.ptr(sc), None) == 0
    L.gw_knn_free(h)
    ref = N.most_similar(x, device=-1)
    assert np.array_equal(ids, ref[0]) and same_bits(sc, ref[1])


# ---- 4: label agreement ------------------------------------------------------------------------------
def agreement_restated(ids, labels_of, row_ids=None):
    """preprocess_simrank (DeepSim/src/main.py:132-167) on padded rows."""
    out = []
    for topk in range(1, ids.shape[1] + 1):
        cnt = tot = 0
        for i, row in enumerate(ids):
            v = i if row_ids is None else row_ids[i]
            listed = [j for j in row if j >= 0]
            for j in listed[:topk]:
                cnt += len(set(labels_of[v]) & set(labels_of[j])) > 0
            tot += min(len(listed), topk)
        out.append(cnt / tot if tot else 0.0)
    return np.array(out)


def test_label_agreement():
    C, N = _C(), _N()
    rng = np.random.default_rng(8)
    n, topk = 50, 6
    groups = {str(v + 1): [str(l) for l in rng.choice(5, rng.integers(1, 3), replace=False)] for v in range(n)}
    del groups["8"]                                    # an unlabelled vertex
    node_labels = [str(v + 1) for v in range(n)]
    ids = np.stack([rng.permutation(n)[:topk] for _ in range(n)]).astype(np.int32)
    ids[3, 2:] = -1                                    # padded rows
    ids[9] = -1
    ids[7, 0] = 7
    labels_of = [groups.get(l, []) for l in node_labels]
    acc = N.label_agreement(ids, groups, node_labels)
    ref = agreement_restated(ids, labels_of)
    assert np.allclose(acc, ref, rtol=1e-15, atol=0) and 0 < acc.min() and acc.max() < 1
    rows = np.array([4, 7, 7, 30], np.int32)
    acc2 = N.label_agreement(ids[rows], groups, node_labels, row_ids=rows)
    assert np.allclose(acc2, agreement_restated(ids[rows], labels_of, rows), rtol=1e-15, atol=0)
    assert not N.label_agreement(np.full((4, 3), -1, np.int32), groups, node_labels).any()    # 0 / 0 -> 0
    bad = ids.copy()
    bad[0, 0] = n
    with pytest.raises(IndexError):
        N.label_agreement(bad, groups, node_labels)


# ---- 5: round trip ----------------------------------------------------------------------------------------
def test_round_trip_through_the_sim_text_writer(tmp_path):
    from gwamd import topsim
    N = _N()
    x = np.random.default_rng(9).standard_normal((80, 6)).astype(np.float32)
    ids, sc = N.most_similar(x, topk=5, device=-1)
    path = str(tmp_path / "x.nn")
    N.write_neighbors(path, ids, sc)
    lines = open(path, newline="").read().split("\r\n")
    assert lines[0] == "0," + ",".join(str(j) for j in ids[0]) and len(lines) == 81
    first = open(path + ".sim.txt", newline="").read().split("\r\n")[0].split(",")
    assert first[1] == f"{ids[0, 0]}:{sc[0, 0]:.6f}"
    assert topsim.precision(path + ".sim.txt", path + ".sim.txt", str(tmp_path / "pre.txt"), 5, topk=5) == 1.0


def test_cli_on_a_file(tmp_path, capsys):
    """python -m gwamd.neighbors: rows in label order whatever the file's order, ids written as labels, the
    precision against a gold file and the agreement curve."""
    from gwamd import topsim
    N = _N()
    x = np.random.default_rng(10).standard_normal((40, 5)).astype(np.float32)
    order = np.random.default_rng(11).permutation(40)
    emb, grp = tmp_path / "x.emb", tmp_path / "groups.csv"
    with open(emb, "w") as f:
        f.write("40 5\n")
        for v in order:
            f.write(f"{v + 100} " + " ".join(repr(float(t)) for t in x[v]) + "\n")
    with open(grp, "w") as f:
        for v in range(40):
            f.write(f"{v + 100},{v % 3}\n")
    out = str(tmp_path / "x.nn")
    assert N.cli(["--emb", str(emb), "--output", out, "--topk", "4", "--device", "-1", "--gold", out + ".sim.txt",
                  "--groups", str(grp)]) == 0
    ids, sc = N.most_similar(x, topk=4, device=-1)
    lines = open(out, newline="").read().split("\r\n")[:-1]
    assert lines == [f"{v + 100}," + ",".join(str(j + 100) for j in ids[v]) for v in range(40)]
    printed = capsys.readouterr().out.splitlines()
    assert printed[0].endswith(": 1.0")               # the file against itself
    acc = N.label_agreement(ids, ([v for v in range(41)], (np.arange(40) % 3).astype(np.int32)))
    assert printed[1:5] == ["Top: %d, acc:  %s" % (t + 1, a) for t, a in enumerate(acc)]
    assert topsim.precision(out + ".sim.txt", out + ".sim.txt", str(tmp_path / "p.txt"), 4, topk=4) == 1.0


def test_deepsim_cli_neighbors_equal_the_saved_files(tmp_path, capsys):
    """--neighbors of gwamd.deepsim (host evaluation: --device -1 with a walks file) writes the bytes that
    python -m gwamd.neighbors writes from the saved embedding, whose text form is exact."""
    from gwamd import deepsim, io
    N = _N()
    V, L = 35, 11
    rng = np.random.RandomState(0)
    walks = [[str(t) for t in rng.randint(0, V, L)] for _ in range(120)]
    io.save_list(walks, str(tmp_path / "walks.txt"))
    with open(tmp_path / "sr.sim.txt", "w", newline="") as f:
        for v in range(V):
            nb = rng.permutation(V)[:4]
            f.write(f"{v}," + ",".join(f"{j}:{s:.6f}" for j, s in zip(nb, np.sort(rng.uniform(0.01, 0.9, 4))[::-1])) +
                    "\r\n")
    argv = ["--simrank_path", str(tmp_path / "sr.sim.txt"), "--walks", str(tmp_path / "walks.txt"), "--emb_output",
            str(tmp_path / "k.emb"), "--vertex-num", str(V), "--dimensions", "16", "--window-size", "2", "--steps", "5",
            "--batch", "16", "--seed", "3", "--checkpoint-every", "0", "--device", "-1"]
    assert deepsim.cli(argv) == 0
    assert not os.path.exists(tmp_path / "a.nn")       # without the flag: as before
    assert deepsim.cli(argv + ["--neighbors", str(tmp_path / "a.nn")]) == 0
    assert N.cli(["--emb", str(tmp_path / "k.emb"), "--output", str(tmp_path / "b.nn"), "--device", "-1"]) == 0
    for ext in ("", ".sim.txt"):
        a, b = open(str(tmp_path / "a.nn") + ext, "rb").read(), open(str(tmp_path / "b.nn") + ext, "rb").read()
        assert a == b and len(a) > V * 20
    capsys.readouterr()


# ---- 6: sanitizers ----------------------------------------------------------------------------------------
def test_host_check_under_sanitizers(tmp_path):
    """gw_knn_host.cpp + host/knn_host_check.cpp (its own main) under ASan + UBSan, run as a plain program."""
    exe = str(tmp_path / "knn_host_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-static-libasan", "-static-libubsan",
           "-ffp-contract=off", "-DGW_KNN_HOST_ONLY", f"-I{os.path.join(ROOT, 'include')}",
           os.path.join(PKG, "csrc", "gw_knn_host.cpp"), os.path.join(PKG, "host", "knn_host_check.cpp"),
           "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "knn host check ok" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr
