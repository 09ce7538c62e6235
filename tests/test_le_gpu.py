"""GPU: the Laplacian-eigenmap kernels (csrc/gw_le.hip) against the host evaluation of the same law (device = -1),
bit for bit, at the edges of their geometry (gw_le_tiles); the fixture solved to tol on the device; a pipeline
gw_topsim -> Eigenmaps -> most_similar / classify on the device-resident vectors; the kernel table.

Convergence is not needed for the bit comparison: most cases run 3 Rayleigh-Ritz steps with a filter of degree 3.
"""
import os

import numpy as np
import pytest

from conftest import DATA

pytestmark = pytest.mark.gpu

CHUNK = 512  # GW_LE_CHUNK; test_geometry holds gw_le_tiles to it
MAX_BLOCK = 256


def _E():
    from gwamd import _lib as C
    from gwamd import eigenmaps
    C.lib()
    return eigenmaps


def random_rows(n, topk, seed, alive=None):
    """Seeded sparse rows among the vertices `alive` (default: all): ids, scores, -1 padded at random lengths."""
    rng = np.random.default_rng(seed)
    alive = np.arange(n) if alive is None else np.asarray(alive)
    ids = np.full((n, topk), -1, np.int32)
    sc = np.zeros((n, topk))
    for v in alive:
        k = int(rng.integers(1, topk + 1))
        ids[v, :k] = rng.choice(alive, k)
        sc[v, :k] = rng.uniform(0.01, 1.0, k)
    return ids, sc


def csr_of(n, edges):
    """An exactly sized CSR of directed weighted entries (i, j, w)."""
    rows = [[] for _ in range(n)]
    for i, j, w in edges:
        rows[i].append((j, w))
    off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    nb = np.asarray([j for r in rows for j, _ in r], np.int32)
    wt = np.asarray([w for r in rows for _, w in r], np.float64)
    return off, nb, wt


def run(device, n, rows=None, csr=None, **kw):
    """(error class or None, results) of one solve."""
    E = _E()
    kw = dict(dict(max_iters=3, cheb_degree=3, seed=11), **kw)
    m = E.Eigenmaps(n, device=device, **kw)
    if rows is not None:
        m.set_rows(*rows)
    else:
        m.set_csr(*csr)
    try:
        st = m.solve()
    except Exception as e:  # noqa: BLE001 - the same failure must come from both modes
        m.free()
        return type(e).__name__ + ": " + str(e), None
    lam, vec, res = m.export()
    out = dict(lam=lam, vec=vec, res=res, f32=m.vectors_numpy(), iters=st.iters, applies=st.applies, skipped=st.skipped,
               state=st.state, isolated=st.isolated, block=st.block_used)
    m.free()
    return None, out


def same_bits(n, expect_ok=True, **kw):
    eh, h = run(-1, n, **kw)
    ed, d = run(0, n, **kw)
    assert eh == ed
    if expect_ok:
        assert eh is None, eh
    if h is None:
        return None
    for k in ("lam", "vec", "res"):
        assert np.array_equal(h[k].view(np.int64), d[k].view(np.int64)), k
    assert np.array_equal(h["f32"].view(np.int32), d["f32"].view(np.int32))
    for k in ("iters", "applies", "skipped", "state", "isolated", "block"):
        assert h[k] == d[k], k
    assert np.isfinite(h["vec"]).all()
    return h


def test_geometry():
    E = _E()
    m = E.Eigenmaps(4, device=0, dim=1, block=2)
    assert m.tiles() == {"rows_per_wg": 4, "chunk": CHUNK, "cols_per_pass": 64}
    assert E.Eigenmaps(4, device=-1, dim=1, block=2).tiles()["chunk"] == CHUNK


@pytest.mark.parametrize("sym", ["mean", "max"])
@pytest.mark.parametrize("n", [2, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3])
def test_rows_at_the_chunk_edges(n, sym):
    rows = random_rows(n, 6, n) if n > 2 else (np.array([[1], [0]], np.int32), np.array([[.5], [.25]]))
    h = same_bits(n, rows=rows, dim=1 if n == 2 else 5, block=2 if n == 2 else 8, symmetrize=sym, min_eigenvalue=-1.0)
    assert h["iters"] == (1 if n == 2 else 3)


def test_one_row_is_all_isolated_in_both_modes():
    assert same_bits(1, expect_ok=False, rows=(np.array([[0]], np.int32), np.array([[1.]])), dim=1, block=2) is None


@pytest.mark.parametrize("block", [2, 63, 64, 65, 129, MAX_BLOCK])
@pytest.mark.parametrize("wide", [True, False])
def test_block_widths(block, wide):
    """dim = block - 1 (nothing skipped: min_eigenvalue -1) and dim = 1."""
    n = CHUNK + 90
    rows = random_rows(n, 6, 5)
    h = same_bits(n, rows=rows, dim=block - 1 if wide else 1, block=block, min_eigenvalue=-1.0,
                  max_iters=2 if block > 128 else 3)
    assert h["block"] == block and h["skipped"] == 0


def star_graph():
    """Rows of S of length 0 (vertex 0), 1 (every leaf), 63, 64 and 65 (the hubs 1, 2, 3)."""
    edges, nxt = [], 4
    rng = np.random.default_rng(2)
    for hub, deg in ((1, 63), (2, 64), (3, 65)):
        for _ in range(deg):
            edges.append((hub, nxt, float(rng.uniform(0.1, 1.0))))
            nxt += 1
    return nxt, csr_of(nxt, edges)


def test_row_lengths_of_s():
    n, csr = star_graph()
    h = same_bits(n, csr=csr, dim=3, block=8, min_eigenvalue=-1.0)
    assert h["isolated"] == 1 and np.all(h["vec"][0] == 0)


def test_a_hub_row_stays_with_its_wave():
    n = 1200
    ids, sc = random_rows(n, 5, 9)
    rng = np.random.default_rng(4)
    hub = [(0, int(j), float(rng.uniform(0.01, 1.0))) for j in rng.choice(np.arange(1, n), 1000, replace=False)]
    edges = hub + [(i, int(j), float(s)) for i in range(n) for j, s in zip(ids[i], sc[i]) if j >= 0]
    same_bits(n, csr=csr_of(n, edges), dim=4, block=16, min_eigenvalue=-1.0)


def test_isolated_rows_first_last_and_interleaved():
    n = CHUNK + 40
    dead = set([0, 1, n - 1, n - 2]) | set(range(10, n, 7))
    alive = [v for v in range(n) if v not in dead]
    h = same_bits(n, rows=random_rows(n, 6, 3, alive), dim=4, block=16, min_eigenvalue=-1.0)
    assert h["isolated"] == len(dead) and np.all(h["vec"][sorted(dead)] == 0)


@pytest.mark.parametrize("cols", [1, 64, 65, 256])
def test_apply_alone(cols):
    import torch
    E = _E()
    n_star, star = star_graph()
    cases = [(n, dict(rows=random_rows(n, 6, n))) for n in (CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3)]
    cases += [(n_star, dict(csr=star)), (2, dict(rows=(np.array([[1], [0]], np.int32), np.array([[.5], [.25]])))),
              (1, dict(rows=(np.array([[0]], np.int32), np.array([[1.]]))))]
    for n, kw in cases:
        x = np.random.default_rng(cols).standard_normal((n, cols))
        ys = []
        for dev in (-1, 0):
            m = E.Eigenmaps(n, device=dev, dim=1, block=2)
            m.set_rows(*kw["rows"]) if "rows" in kw else m.set_csr(*kw["csr"])
            y = m.apply(x if dev < 0 else torch.as_tensor(x, device="cuda:0"))
            ys.append(y if dev < 0 else y.cpu().numpy())
            m.free()
        assert np.array_equal(ys[0].view(np.int64), ys[1].view(np.int64))


def test_fixture_solved_on_the_device():
    """Host test 1's eigenvalue check, on the GPU: against numpy's eigvalsh of the dense I - S within tol."""
    import test_le_host as T
    E = _E()
    for sym in ("mean", "max"):
        r = T.reference(sym)
        m = E.Eigenmaps(333, device=0, dim=16, block=32, symmetrize=sym, tol=T.TOL)
        m.set_rows(r["ids"], r["sc"])
        st = m.solve()
        lam, vec, res = m.export()
        assert st.state == 0 and st.skipped == 2 and st.isolated == 7
        err = np.abs(lam - r["lam"][2:18]).max()
        print(sym, "eigenvalue error", err, "iters", st.iters)
        assert err <= T.TOL and res.max() <= T.TOL
        o = T.solved(sym, 16)  # and the host's bits
        assert np.array_equal(vec.view(np.int64), o["vec"].view(np.int64)) and st.iters == o["st"].iters
        m.free()


def test_pipeline_on_the_gpu():
    """gw_topsim rows -> Eigenmaps -> most_similar and classify on the vectors where the solver left them: the same
    as on the exported copy."""
    import torch
    E = _E()
    from gwamd import classify, neighbors, topsim
    V = 1380
    g = topsim.Graph(os.path.join(DATA, "moreno_crime_crime.txt"), V, separator="\t")
    ids, sc = topsim.TopSim_singleSample(g, 200, 3, seed=5).topK(10)
    # moreno's top-10 rows fall into more components than a small block holds: keep the zero eigenvalues
    emb = E.eigenmaps((ids, sc), dim=8, device=0, block=24, max_iters=30, min_eigenvalue=-1.0)
    assert emb.model.device == 0 and emb.vectors.shape == (V, 8) and np.isfinite(emb.vectors).all()
    view = emb.model.vectors_torch()
    assert view.is_cuda and np.array_equal(view.cpu().numpy(), emb.vectors)
    assert np.array_equal(emb.vectors, emb.vectors64.astype(np.float32))
    a = neighbors.most_similar(emb, topk=5, device=0)
    b = neighbors.most_similar(torch.as_tensor(emb.vectors, device="cuda:0"), topk=5, device=0)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    groups = {str(i): [str(i % 3)] for i in range(V)}
    kw = dict(training_percents=[0.5], number_shuffles=1, device=0, file=open(os.devnull, "w"))
    assert classify.scoring(emb, groups, **kw) == classify.scoring(emb.vectors, groups, **kw)


def test_kernel_attrs():
    E = _E()
    m = E.Eigenmaps(8, device=0, dim=1, block=2)
    attrs = m.kernel_attrs()
    assert set(attrs) == {"k_le_init", "k_le_apply", "k_le_gram", "k_le_gram_reduce", "k_le_rotate", "k_le_residual",
                          "k_le_col_reduce", "k_le_output"}
    for name, a in attrs.items():
        print(name, a)
        assert a["lds_bytes"] <= 160 * 1024 and a["scratch_bytes"] == 0 and 0 < a["vgprs"] <= 512
