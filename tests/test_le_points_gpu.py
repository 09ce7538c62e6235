"""GPU: points -> gw_nng -> gw_le with self_loops, all on the device, against the host path bit for bit and against
the reference's spectra (tests/golden/le_points_*.npz); gw_le's self_loops rule at its row edges; device-resident
vectors -> eigenmaps_of_points -> most_similar without a host copy of the vectors.
"""
import numpy as np
import pytest

from test_le_points_host import FIXTURES, golden_case, roll, spearman

pytestmark = pytest.mark.gpu


def _E():
    from gwamd import _lib as C
    from gwamd import eigenmaps
    C.lib()
    return eigenmaps


def bits(emb):
    st = emb.stats
    return (emb.eigenvalues.tobytes(), emb.vectors64.tobytes(), emb.residuals.tobytes(), emb.vectors.tobytes(), st.state,
            st.iters, st.applies, st.skipped, st.isolated, st.block_used)


@pytest.mark.parametrize("name", FIXTURES)
def test_golden_spectrum_on_the_device(name):
    """The bound and its reasoning are test_le_points_host's; the device pairs are the host's bits."""
    E = _E()
    x, k, t, ref, zeros = golden_case(name)
    n = len(x)
    kw = dict(dim=len(ref), block=n, tol=1e-12)
    dev = E.eigenmaps_of_points(x, k, t, device=0, **kw)
    err = np.abs(dev.eigenvalues - ref).max()
    print(f"{name}: device max |difference| {err:.2e}")
    assert dev.stats.state == 0 and dev.stats.skipped == zeros
    assert err <= 1e-10
    host = E.eigenmaps_of_points(x, k, t, device=-1, **kw)
    assert bits(dev) == bits(host)
    lam, f = E.laplaEigen(x, k, t, device=0, **kw)
    assert np.array_equal(lam, host.eigenvalues) and np.array_equal(f, host.vectors64)


def test_swiss_roll_device_equals_host():
    E = _E()
    x, t = roll()
    dev = E.eigenmaps_of_points(x, 10, 15.0, dim=2, device=0)
    host = E.eigenmaps_of_points(x, 10, 15.0, dim=2, device=-1)
    assert bits(dev) == bits(host)
    assert dev.stats.state == 0 and dev.stats.skipped == 1 and abs(spearman(dev.vectors64[:, 0], t)) >= 0.99


@pytest.mark.parametrize("n", [2, 513])
def test_self_loops_device_equals_host(n):
    """gw_le with self_loops = 1 at n = 2 and one past the law's row chunk; the last row has only its self-loop."""
    E = _E()
    rng = np.random.default_rng(n)
    topk = 2 if n == 2 else 6
    ids = np.full((n, topk), -1, np.int32)
    sc = np.zeros((n, topk))
    for v in range(n - 1):
        others = rng.choice(n - 1, min(topk - 1, n - 1), replace=False)     # may hold v itself: a repeated id
        ids[v, 0], sc[v, 0] = v, rng.uniform(0.2, 1.0)
        ids[v, 1:1 + len(others)] = others
        sc[v, 1:1 + len(others)] = rng.uniform(0.05, 1.0, len(others))
    ids[n - 1, 0], sc[n - 1, 0] = n - 1, 0.5
    out = []
    for device in (0, -1):
        m = E.Eigenmaps(n, device=device, dim=1 if n == 2 else 5, block=2 if n == 2 else 24, max_iters=4, cheb_degree=5,
                        seed=11, self_loops=1, min_eigenvalue=-1.0)
        m.set_rows(ids, sc)
        st = m.solve()
        out.append(tuple(a.tobytes() for a in m.export()) + (m.vectors_numpy().tobytes(), st.iters, st.applies, st.skipped,
                                                            st.isolated, st.block_used, st.state))
        if device == -1:
            S = m.apply(np.eye(n)) if n == 2 else None
        m.free()
    assert out[0] == out[1]
    assert out[0][-3] == 0                                  # nobody is isolated: the last row has its loop
    if n == 2:
        assert abs(S[1, 1] - 1.0) <= 4e-16 and abs(S[0, 0] - 1.0) <= 4e-16 and S[0, 1] == 0.0


def test_device_resident_vectors_to_eigenmap_to_most_similar():
    """Random vectors that live on the GPU only -> the neighbour graph read in place -> the eigenmap -> cosine
    neighbours of the solver's own fp32 vectors, read in place; the same chain on the host gives the same bits."""
    import torch
    from gwamd import neighbors
    E = _E()
    g = torch.Generator(device="cuda:0")
    g.manual_seed(5)
    store = torch.randn((400, 24), generator=g, device="cuda:0", dtype=torch.float32)
    x = store[:, :16]                                        # a view with pitch 24: used in place
    emb = E.eigenmaps_of_points(x, 8, 40.0, dim=4, device=0)
    assert emb.model.device == 0 and emb.stats.state == 0
    ids, sc = neighbors.most_similar(emb, topk=5)            # reads gw_le_vectors_dev where it lies
    host = E.eigenmaps_of_points(x.cpu().numpy(), 8, 40.0, dim=4, device=-1)
    assert bits(emb) == bits(host)
    hid, hsc = neighbors.most_similar(host.vectors, topk=5, device=-1)
    assert np.array_equal(ids, hid) and np.array_equal(sc.view(np.int64), hsc.view(np.int64))
