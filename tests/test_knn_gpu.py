"""GPU: the nearest-neighbour kernels (gw_knn.hip) against the host evaluation of the law (device = -1), bit for
bit: ids array_equal, scores as int64 views.  The shapes sit on the edges of the launch geometry gw_knn_tiles
reports (tq source rows per workgroup, tc candidates per tile, kc columns per LDS chunk, buf entries of a row's
candidate buffer).
"""
import os

import numpy as np
import pytest

from conftest import DATA

pytestmark = pytest.mark.gpu


def _N():
    from gwamd import _lib as C
    from gwamd import neighbors
    C.lib()
    return neighbors


_tiles = {}


def tiles(topk=20):
    if topk not in _tiles:
        m = _N().Neighbors(4, device=0, dim=4, topk=topk)
        _tiles[topk] = m.tiles()
        m.free()
    return _tiles[topk]


def padded(x, pad=3):
    """x on the GPU with pitch dim + pad, the pad columns NaN and the last row allocated without its pad:
    (tensor that owns the memory, pitch)."""
    import torch
    n, d = x.shape
    flat = np.full(n * (d + pad) - pad, np.nan, np.float32)
    for v in range(n):
        flat[v * (d + pad):v * (d + pad) + d] = x[v]
    return torch.as_tensor(flat, device="cuda:0"), d + pad


def both(x, topk, metric, sources=None, pad=3):
    """(device ids, scores), (host ids, scores) of the same query; the device reads a padded matrix."""
    N = _N()
    n, d = x.shape
    t, pitch = padded(x, pad)
    dev = N.Neighbors(n, device=0, dim=d, topk=topk, metric=metric)
    dev.set_vectors(t.data_ptr(), pitch=pitch)
    got = dev.query(sources)
    dev.free()
    host = N.Neighbors(n, device=-1, dim=d, topk=topk, metric=metric)
    host.set_vectors(np.ascontiguousarray(x))
    want = host.query(sources)
    host.free()
    return got, want


def assert_same(got, want):
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1].view(np.int64), want[1].view(np.int64))


def test_geometry():
    t = tiles(20)
    print("gw_knn_tiles:", t, tiles(128))
    assert t["tq"] >= 2 and t["tc"] >= 2 and t["kc"] >= 2 and t["buf"] >= 20 and tiles(128)["buf"] >= 128


def edge_cases():
    """(n, nsrc, dim, topk, metric) in terms of the geometry: every listed n, nsrc, dim and topk occurs, both
    metrics, pruned to a dozen."""
    t = tiles()
    tq, tc, kc = t["tq"], t["tc"], t["kc"]
    return [(1, 1, 1, 1, "cosine"), (2, 1, kc - 1, 20, "dot"), (tc - 1, tq - 1, kc + 1, 20, "cosine"),
            (tc, tq + 1, 128, 1, "dot"), (tc + 1, tq + 1, 1024, 20, "cosine"), (2 * tc + 3, tq - 1, 128, 128, "cosine"),
            (2 * tc + 3, tq + 1, kc + 1, 128, "dot"), (tc + 1, 1, 1, 128, "cosine"), (tc, tq - 1, kc - 1, 1, "cosine"),
            (2, 1, 1024, 1, "dot"), (tc - 1, tq + 1, 128, 20, "dot"), (2 * tc + 3, tq + 1, 1, 20, "dot")]


@pytest.mark.parametrize("case", range(12))
def test_edges(case):
    n, nsrc, dim, topk, metric = edge_cases()[case]
    rng = np.random.default_rng(100 + case)
    x = rng.standard_normal((n, dim)).astype(np.float32)
    if dim == 1:
        x = rng.integers(-2, 3, (n, 1)).astype(np.float32)     # ties, zero rows
    src = np.sort(rng.integers(0, n, nsrc))[::-1].astype(np.int32)  # descending, with repeats where nsrc > n
    got, want = both(x, topk, metric, src)
    assert got[0].shape == (nsrc, topk)
    assert_same(got, want)
    got, want = both(x, topk, metric, None)                    # sources = NULL: all rows
    assert got[0].shape == (n, topk)
    assert_same(got, want)


def fan(n, rising):
    """Row 0 is (1, 0); row j >= 1 stands at an angle to it that falls (rising similarity) or grows with j, and is
    longer the nearer it is, so that cosine and dot product order the candidates alike."""
    j = np.arange(n, dtype=np.float64)
    theta = (n - j) / n if rising else j / n
    r = 2.0 - theta
    x = np.stack([r * np.cos(theta), r * np.sin(theta)], 1).astype(np.float32)
    x[0] = (1.0, 0.0)
    return x


@pytest.mark.parametrize("metric", ["cosine", "dot"])
@pytest.mark.parametrize("topk", [20, 128])
def test_selection_at_its_worst_and_its_mirror(topk, metric):
    buf = tiles(topk)["buf"]
    n = topk + 3 * buf + 40
    src = np.array([0, n - 1, n // 2], np.int32)
    x = fan(n, True)            # every later candidate of source 0 beats the bound: n - 1 >= topk + 3 * buf get past it
    got, want = both(x, topk, metric, src)
    assert_same(got, want)
    assert np.array_equal(got[0][0], np.arange(n - 1, n - 1 - topk, -1))
    x = fan(n, False)           # nothing after the first tile does
    got, want = both(x, topk, metric, src)
    assert_same(got, want)
    assert np.array_equal(got[0][0], np.arange(1, topk + 1))


@pytest.mark.parametrize("metric", ["cosine", "dot"])
def test_all_rows_identical(metric):
    n, topk = 2 * tiles()["tc"] + 44, 20
    x = np.tile(np.array([[0.5, -1.25, 3.0]], np.float32), (n, 1))
    got, want = both(x, topk, metric)
    assert_same(got, want)
    for v in (0, 7, n - 1):
        assert np.array_equal(got[0][v], [j for j in range(n) if j != v][:topk])   # ties: ids ascending


@pytest.mark.parametrize("metric", ["cosine", "dot"])
@pytest.mark.parametrize("topk", [8, 128])
def test_integer_grid_against_numpy(metric, topk):
    from test_knn_host import grid, numpy_rows
    x = grid()
    got, _ = both(x, topk, metric)
    rid, rsc = numpy_rows(x, topk, metric)
    assert np.array_equal(got[0], rid)
    assert np.array_equal(got[1].view(np.int64), rsc.view(np.int64))


def test_torch_tensor_in_place_and_pitch_from_stride():
    import torch
    N = _N()
    x = np.random.default_rng(40).standard_normal((150, 24)).astype(np.float32)
    wide = torch.full((150, 29), float("nan"), device="cuda:0")
    wide[:, :24] = torch.as_tensor(x, device="cuda:0")
    got = N.most_similar(wide[:, :24], topk=7)                  # stride 29: used where it is
    assert_same(got, N.most_similar(x, topk=7, device=-1))
    got = N.most_similar(x, sources=[3, 3, 149], topk=7, metric="dot", device=0)   # numpy: uploaded
    assert_same(got, N.most_similar(x, sources=[3, 3, 149], topk=7, metric="dot", device=-1))


def test_zero_copy_from_a_trainer():
    """Two SGNS epochs on karate: most_similar(trainer) reads syn0 where it lies and equals the host evaluation of
    the exported rows."""
    import ctypes
    import torch
    import gwamd
    from gwamd import _lib as C
    from gwamd.embed import SGNS
    N = _N()
    G = gwamd.GWGraph.from_edgelist(os.path.join(DATA, "karate.edgelist"), " ", "nx").to_device(0)
    C.check(C.lib().gw_n2v_prepare(G.handle, 0.25, 4.0, C.N2V_REJECTION), G.handle)
    nw, L = 340, 20
    W = torch.empty((nw, L), dtype=torch.int32, device="cuda:0")
    C.check(C.lib().gw_n2v_walks(G.handle, L, 7, 0, nw, 1, C.ptr(W), None, None, None), G.handle)
    torch.cuda.synchronize()
    m = SGNS(G.n, device=0, dim=16, window=5, negative=5, epochs=2, seed=7)
    m.build_vocab(ctypes.c_void_p(W.data_ptr()), nw, L)
    m.train(ctypes.c_void_p(W.data_ptr()), nw, L, 0, 2, 0)
    got = N.most_similar(m, topk=10)
    want = N.most_similar(m.export()[0], topk=10, device=-1)
    assert_same(got, want)
    assert (got[0] >= 0).all()
    m.free()


def test_handle_reuse_with_more_rows():
    """One handle, then a larger n and a new pointer (the norms buffer grows), then a smaller one (stale norms
    behind the live part)."""
    N = _N()
    rng = np.random.default_rng(41)
    dev = N.Neighbors(50, device=0, dim=9, topk=6)
    for n in (50, 700, 33):
        x = rng.standard_normal((n, 9)).astype(np.float32)
        if n != dev.n:
            dev.set_rows(n)
        dev.set_vectors(x)
        got = dev.query()
        assert_same(got, N.most_similar(x, topk=6, device=-1))
        src = np.array([n - 1, 0, n - 1], np.int32)
        assert_same(dev.query(src), N.most_similar(x, sources=src, topk=6, device=-1))
    dev.free()


def test_errors_on_the_device():
    import torch
    from gwamd import _lib as C
    N = _N()
    x = np.random.default_rng(42).standard_normal((40, 5)).astype(np.float32)
    m = N.Neighbors(40, device=0, dim=5, topk=3)
    with pytest.raises(C.StateError):
        m.query()
    m.set_vectors(x)
    ids = torch.full((3, 3), 77, dtype=torch.int32, device="cuda:0")
    sc = torch.full((3, 3), 77.0, dtype=torch.float64, device="cuda:0")
    for v in (40, -1):
        src = torch.as_tensor(np.array([1, v, 2], np.int32), device="cuda:0")
        rc = C.lib().gw_knn_query(m.handle, C.ptr(src), 3, C.ptr(ids), C.ptr(sc), None)
        assert rc == C.GW_ERR_RANGE and b"entry 1" in C.lib().gw_knn_last_error(m.handle)
        assert (ids == 77).all().item() and (sc == 77.0).all().item()      # nothing was written
    assert C.lib().gw_knn_query(m.handle, C.ptr(src), 0, None, None, None) == C.GW_OK
    assert_same(m.query([5]), N.most_similar(x, sources=[5], topk=3, device=-1))   # the handle still works
    m.free()


def test_kernel_attrs():
    m = _N().Neighbors(100, device=0, dim=128, topk=20)
    a = m.kernel_attrs()
    m.free()
    big = _N().Neighbors(100, device=0, dim=128, topk=128)
    b = big.kernel_attrs()
    big.free()
    print("gw_knn_kernel_attrs (topk 20):", a)
    print("gw_knn_kernel_attrs (topk 128):", b)
    assert set(a) == {"k_knn_check", "k_knn_norms", "k_knn_main"}
    for name, k in a.items():
        assert k["scratch_bytes"] == 0, name
        assert 0 < k["vgprs"] <= 128, name           # two workgroups of 256 lanes per CU keep their registers


def sim_rows(path):
    rows = []
    for line in open(path, newline="").read().split("\r\n")[:-1]:
        t = line.split(",")
        rows.append((t[0], [e.split(":")[0] for e in t[1:]], np.array([float(e.split(":")[1]) for e in t[1:]])))
    return rows


def test_cli_neighbors_equal_those_of_the_saved_embedding(tmp_path, capsys):
    """gwamd.cli --neighbors on karate against python -m gwamd.neighbors on the saved .emb: the neighbour file is
    byte-equal.  The .emb is word2vec text, six decimals per value, so the scores of the second run are those of
    rows moved by up to 5e-7 per column (and 6e-8 relative, the fp32 parse): they are held to the bound that
    follows, |d cos| <= (|da| / |a| + |db| / |b|) (1 + 1e-3) + two print roundings of 5e-7, not to the bytes."""
    from gwamd import classify, cli
    N = _N()
    emb, nn = str(tmp_path / "karate.emb"), str(tmp_path / "karate.nn")
    argv = ["--mode", "scale", "--input", os.path.join(DATA, "karate.edgelist"), "--delimiter", " ", "--walks",
            str(tmp_path / "walks.txt"), "--output", emb, "--dimensions", "16", "--iter", "1", "--walk-length", "20",
            "--seed", "3"]
    assert cli.main(argv) == 0
    assert not os.path.exists(nn)                      # without the flag: as before
    assert cli.main(argv + ["--neighbors", nn]) == 0
    assert capsys.readouterr().out == ""
    for dev, name in ((0, "gpu.nn"), (-1, "host.nn")):
        other = str(tmp_path / name)
        assert N.cli(["--emb", emb, "--output", other, "--device", str(dev)]) == 0
        assert open(nn, "rb").read() == open(other, "rb").read()
        labels, X = classify.read_embedding(emb)
        norm = dict(zip(labels, np.linalg.norm(X.astype(np.float64), axis=1)))
        worst = 0.0
        for (v, ia, sa), (w, ib, sb) in zip(sim_rows(nn + ".sim.txt"), sim_rows(other + ".sim.txt")):
            assert v == w and ia == ib
            da = 4 * (5e-7 + 6e-8 * norm[v]) / norm[v]          # sqrt(16) columns
            db = np.array([4 * (5e-7 + 6e-8 * norm[j]) / norm[j] for j in ia])
            assert (np.abs(sa - sb) <= (da + db) * (1 + 1e-3) + 1e-6).all()
            worst = max(worst, float(np.abs(sa - sb).max()))
        print(f"device {dev}: largest score difference to the run on the saved file {worst:.2e}")
    a, b = open(str(tmp_path / "gpu.nn.sim.txt"), "rb").read(), open(str(tmp_path / "host.nn.sim.txt"), "rb").read()
    assert a == b                                      # the same file: kernels and host evaluation, byte for byte
