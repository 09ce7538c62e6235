"""CPU: Isomap of points on the host (gwamd.isomap, device = -1): the spectrum and the coordinates against the
test's own doubly centred matrix, landmark consistency, sklearn, a disconnected input and the command line."""
import numpy as np
import pytest

N, K = 2000, 10


def centred(D):
    """B of classical MDS from a distance matrix, as gwamd.isomap states it."""
    d2 = D ** 2
    b = -0.5 * (d2 - d2.mean(1)[:, None] - d2.mean(0)[None, :] + d2.mean())
    return 0.5 * (b + b.T)


def signed(y):
    y = y.copy()
    for c in range(y.shape[1]):
        if y[np.argmax(np.abs(y[:, c])), c] < 0:
            y[:, c] = -y[:, c]
    return y


@pytest.fixture(scope="module")
def roll(gw):
    """The roll's fp32 points, the full host Isomap (no self entry, as sklearn's graph) and the geodesics."""
    from gwamd import geodesics, isomap, pointgraph
    X = pointgraph.make_swiss_roll(N, seed=0)[0].astype(np.float32)
    ids, _, d2 = pointgraph.knn_graph(X, K, 0.0, include_self=False, device=-1, d2=True)
    g = geodesics.Geodesics(N, device=-1, squared=True)
    g.set_rows(ids, d2)
    assert g.stats().components == 1  # connected
    D = g.query()
    emb = isomap.isomap(X, k=K, dim=2, device=-1, include_self=False)
    return X, D, emb


def test_eigenvalues(roll):
    _, D, emb = roll
    lam = np.linalg.eigvalsh(centred(D))[::-1][:2]
    print("eigenvalues", emb.eigenvalues, "eigvalsh", lam)
    assert emb.vectors.shape == (N, 2) and emb.vectors.dtype == np.float64
    assert len(emb.outside) == 0 and np.array_equal(emb.landmarks, np.arange(N))
    assert np.all(np.abs(emb.eigenvalues - lam) <= 1e-10 * lam[0])


def test_coordinates_are_eigenvectors(roll):
    _, D, emb = roll
    B = centred(D)
    for c in range(2):
        y = emb.vectors[:, c]
        res = np.linalg.norm(B @ y - emb.eigenvalues[c] * y)
        print(f"column {c}: residual {res:.3g}, bound {1e-9 * emb.eigenvalues[0] * np.linalg.norm(y):.3g}")
        assert res <= 1e-9 * emb.eigenvalues[0] * np.linalg.norm(y)
        assert y[np.argmax(np.abs(y))] > 0


def test_all_rows_as_landmarks_is_classical(roll):
    from gwamd import isomap
    X, _, emb = roll
    e2 = isomap.isomap(X, k=K, dim=2, device=-1, include_self=False, landmarks=np.arange(N))
    assert np.array_equal(e2.vectors.view(np.int64), emb.vectors.view(np.int64))
    assert np.array_equal(e2.eigenvalues.view(np.int64), emb.eigenvalues.view(np.int64))


def test_landmark_rows_are_their_own_mds(roll):
    """In exact arithmetic the placement formula puts landmark j at row j of V sqrt(lam)."""
    from gwamd import isomap
    X, D, _ = roll
    e = isomap.isomap(X, k=K, dim=2, device=-1, include_self=False, landmarks=256, seed=1)
    lm = e.landmarks
    assert len(lm) == 256 and np.all(np.diff(lm) > 0)
    assert np.array_equal(lm, np.sort(np.random.RandomState(1).permutation(N)[:256]))
    lam, vec = np.linalg.eigh(centred(D[np.ix_(lm, lm)]))
    want = vec[:, ::-1][:, :2] * np.sqrt(lam[::-1][:2])
    # the sign rule looks at all n rows; align the landmark rows' signs column by column
    got = e.vectors[lm]
    for c in range(2):
        if np.dot(want[:, c], got[:, c]) < 0:
            want[:, c] = -want[:, c]
    err = np.abs(got - want).max()
    print(f"landmark rows against V sqrt(lam): {err:.3g}, bound {1e-9 * np.abs(e.vectors).max():.3g}")
    assert err <= 1e-9 * np.abs(e.vectors).max()
    # a chunked run (two queries of the landmarks, in pieces) gives the same embedding up to the sums' order
    e2 = isomap.isomap(X, k=K, dim=2, device=-1, include_self=False, landmarks=256, seed=1, chunk_bytes=8 * N * 100)
    assert np.abs(e2.vectors - e.vectors).max() <= 1e-9 * np.abs(e.vectors).max()


def test_against_sklearn(roll):
    """sklearn.manifold.Isomap(n_neighbors=10, n_components=2) on the same fp32-rounded points (held as float64, so
    that sklearn's own distances are fp64 too).  Measured with this host path: per column up to sign, max abs
    difference 7.9e-14 at coordinates of magnitude 56 (n = 2000, k = 10); 1.6e-13 at n = 600, k = 6.  The bound is
    100 x the measured value: the eigen-gap lam2 / lam3 is 2.2 at this shape and LAPACK builds differ."""
    manifold = pytest.importorskip("sklearn.manifold")
    X, _, emb = roll
    Y = manifold.Isomap(n_neighbors=K, n_components=2).fit_transform(X.astype(np.float64))
    for c in range(2):
        err = min(np.abs(Y[:, c] - emb.vectors[:, c]).max(), np.abs(Y[:, c] + emb.vectors[:, c]).max())
        print(f"column {c}: max abs difference {err:.3g} at magnitude {np.abs(Y[:, c]).max():.3g}")
        assert err <= 100 * 7.9e-14


def test_disconnected_input(gw):
    from gwamd import isomap, pointgraph
    a = pointgraph.make_swiss_roll(300, seed=0)[0]
    b = pointgraph.make_swiss_roll(120, seed=1)[0] + 1e4
    X = np.concatenate([b[:60], a, b[60:]]).astype(np.float32)
    small = np.concatenate([np.arange(60), np.arange(360, 420)])
    e = isomap.isomap(X, k=8, dim=2, device=-1)
    assert np.array_equal(e.outside, small) and np.all(e.vectors[small] == 0.0)
    assert np.array_equal(e.landmarks, np.arange(60, 360)) and e.stats["components"] >= 2
    assert np.all(np.abs(e.vectors[60:360]).sum(1) > 0)
    with pytest.raises(ValueError):
        isomap.isomap(X, k=8, dim=2, device=-1, landmarks=[0, 100, 200])  # row 0 lies outside
    with pytest.raises(ValueError):
        isomap.isomap(X, k=8, dim=2, device=-1, landmarks=301)


def test_cli_round_trip(gw, tmp_path):
    from gwamd import classify, isomap, pointgraph
    X = pointgraph.make_swiss_roll(400, seed=2)[0].astype(np.float32)
    np.save(tmp_path / "x.npy", X)
    out = tmp_path / "x.emb"
    assert isomap.cli(["--points", str(tmp_path / "x.npy"), "--knn", "8", "--dimensions", "2", "--landmarks", "64",
                       "--seed", "3", "--output", str(out), "--device", "-1"]) == 0
    labels, V = classify.read_embedding(out)
    e = isomap.isomap(X, k=8, dim=2, landmarks=64, seed=3, device=-1)
    assert labels == [str(i) for i in range(400)] and V.shape == (400, 2)
    assert np.allclose(V, e.vectors.astype(np.float32), rtol=1e-5, atol=1e-5)
