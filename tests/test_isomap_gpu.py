"""GPU: Isomap of the swiss roll (n = 2000, k = 10) on the device against the host run: the geodesics bit for bit,
the spectrum to rtol 1e-10, the coordinates per column under the sign rule to 100 x the figure test_isomap_host.py
records against sklearn (7.9e-14): the eigensolver is the only difference between the two runs."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, K = 2000, 10
COORD_TOL = 100 * 7.9e-14  # 100 x the measured host-against-sklearn figure


@pytest.fixture(scope="module")
def roll():
    from gwamd import _lib as C
    from gwamd import pointgraph
    C.lib()
    return pointgraph.make_swiss_roll(N, seed=0)[0].astype(np.float32)


def test_geodesics_bitwise(roll):
    from gwamd import geodesics, pointgraph
    ids, _, d2 = pointgraph.knn_graph(roll, K, 0.0, device=-1, d2=True)
    out = []
    for device in (0, -1):
        g = geodesics.Geodesics(N, device=device, squared=True)
        g.set_rows(ids, d2)
        out.append(g.query())
        if device == 0:
            st = g.stats()
            print(f"rounds_max {st.rounds_max}, relaxations per source / entries "
                  f"{st.relaxations / (N * st.entries):.2f}, fallbacks {st.fallbacks}")
            assert st.fallbacks == 0
        g.free()
    assert np.array_equal(out[0].view(np.int64), out[1].view(np.int64))


@pytest.mark.parametrize("landmarks", [None, 256])
def test_isomap_matches_the_host_run(roll, landmarks):
    from gwamd import isomap
    h = isomap.isomap(roll, k=K, dim=2, landmarks=landmarks, seed=1, device=-1)
    d = isomap.isomap(roll, k=K, dim=2, landmarks=landmarks, seed=1, device=0)
    assert np.array_equal(h.landmarks, d.landmarks) and len(d.outside) == 0
    print("eigenvalues", d.eigenvalues, h.eigenvalues)
    assert np.all(np.abs(d.eigenvalues - h.eigenvalues) <= 1e-10 * h.eigenvalues[0])
    err = np.abs(d.vectors - h.vectors).max(0)
    print("coordinates: max abs difference per column", err)
    assert np.all(err <= COORD_TOL)
    assert d.model.vectors_torch().is_cuda
