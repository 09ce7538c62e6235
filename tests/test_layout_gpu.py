"""GPU: the spring-layout kernels (gw_layout.hip) against the host evaluation of the law (device = -1), bit for bit on
int64 views: both sides sum in the order csrc/gw_layout_law.h fixes.  The graphs are test_geo_gpu's synthetic CSRs
(v -> v+1 plus 3 seeded random partners per vertex, values uniform in [0.5, 1.5)), used as listed: directed, with the
odd repeated entry and self loop.  The shapes sit on the edges of the geometry gw_layout_tiles reports: a workgroup of
the all-pairs kernel owns R rows and one chunk of C columns (test_tiles holds the constants below to it)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG
from test_geo_gpu import graph
from test_layout_host import GRAPHS, L, bits, branch_inputs, karate_edges, stop_threshold

pytestmark = pytest.mark.gpu

R, C, STRANDS, BLOCK = 128, 1024, 4, 64
BIG = 2 * C + R + 1


def start(n, dim, seed=0):
    return np.random.RandomState(seed).rand(n, dim)


def pair(n, dim=2):
    lay = L()
    return lay.SpringLayout(n, dim=dim, device=0), lay.SpringLayout(n, dim=dim, device=-1)


def run_both(n, g, dim=2, fixed=None, pos=None, rows=None, **kw):
    """((device iterations_done, positions), (host ...)) of the same inputs."""
    out = []
    pos = start(n, dim) if pos is None else pos
    for m in pair(n, dim):
        if rows is not None:
            m.set_rows(*rows)
        else:
            m.set_csr(*g)
        if fixed is not None:
            m.set_fixed(fixed)
        out.append((m.run(pos, **kw), m.positions_numpy()))
        m.free()
    return out


def same_run(n, g, dim=2, **kw):
    (dd, dp), (hd, hp) = run_both(n, g, dim, **kw)
    assert dd == hd and dp.shape == hp.shape and np.array_equal(bits(dp), bits(hp))
    assert np.isfinite(hp).all()
    return dd, dp


def test_tiles():
    d, h = pair(4)
    assert d.tiles() == {"rows": R, "chunk": C, "strands": STRANDS, "block": BLOCK}
    assert h.tiles() == {"rows": 0, "chunk": C, "strands": STRANDS, "block": BLOCK}
    d.free()
    h.free()


@pytest.mark.parametrize("n", [2, 3, R - 1, R, R + 1, C - 1, C, C + 1, BIG])
def test_whole_runs_at_the_tile_edges(n):
    done, _ = same_run(n, graph(n, seed=n))
    assert done == 50


@pytest.mark.parametrize("n", [R + 1, BIG])
def test_whole_runs_in_three_dimensions(n):
    done, _ = same_run(n, graph(n, seed=n), dim=3)
    assert done == 50


@pytest.mark.parametrize("dim", [2, 3])
def test_one_step_both_outputs(dim):
    g = graph(BIG, seed=5)
    pos = start(BIG, dim, 1)
    d, h = pair(BIG, dim)
    out = []
    for m in (d, h):
        m.set_csr(*g)
        out.append(m.step(pos, k=0.03, t=0.07))
        m.free()
    assert np.array_equal(bits(out[0][0]), bits(out[1][0])) and np.array_equal(bits(out[0][1]), bits(out[1][1]))
    assert np.abs(out[1][0]).min() > 0


@pytest.mark.parametrize("name", ["coincident", "collinear", "fixed"])
def test_the_branches(name):
    n, g, pos, fixed = branch_inputs()[name]
    d, h = pair(n)
    steps = []
    for m in (d, h):
        m.set_csr(*g)
        if fixed is not None:
            m.set_fixed(fixed)
        steps.append(m.step(pos, k=0.0, t=0.1))
        m.free()
    assert np.array_equal(bits(steps[0][0]), bits(steps[1][0])) and np.array_equal(bits(steps[0][1]), bits(steps[1][1]))
    _, end = same_run(n, g, fixed=fixed, pos=pos)
    if name == "collinear":  # in the step: over a run the outer two drift apart by roundings and the middle follows
        assert np.array_equal(bits(steps[0][0][1]), bits([0.0, 0.0])) and np.array_equal(bits(steps[0][1][1]), bits(pos[1]))
    if name == "fixed":
        assert np.array_equal(bits(end[fixed]), bits(pos[fixed]))


@pytest.mark.parametrize("after", [1, 2, 17])
def test_early_stop_and_the_launches_after_it(after):
    """All 50 iterations are launched; the ones after the stop find the flag and must change nothing: the positions
    are the host's, which stopped computing there."""
    n, g = GRAPHS["karate"]
    pos = start(n, 2)
    done, _ = same_run(n, g, pos=pos, threshold=stop_threshold(pos, after))
    assert done == after


def test_zero_iterations_and_a_second_run():
    n, g = GRAPHS["karate"]
    pos = start(n, 2)
    d, h = pair(n)
    ends = []
    for m in (d, h):
        m.set_csr(*g)
        assert m.run(pos, iterations=0) == 0 and np.array_equal(bits(m.positions_numpy()), bits(pos))
        m.run(iterations=7)
        m.run(iterations=5, k=0.4)  # from where the first run ended
        ends.append(m.positions_numpy())
    assert d.positions_torch().is_cuda and np.array_equal(bits(ends[0]), bits(ends[1]))
    d.free()
    h.free()


def test_long_rows_and_empty_rows_in_the_gather():
    """A wave takes 64 entries of a row per trip: rows of 200, 64 and 65 entries, an empty row, and the same matrix as
    top-k rows (-1 padded)."""
    n = 300
    rng = np.random.RandomState(8)
    length = rng.randint(1, 6, n)
    length[[5, 6, 7, 9, n - 1]] = [200, 64, 65, 0, 129]
    off = np.concatenate([[0], np.cumsum(length)]).astype(np.int64)
    nb = rng.randint(0, n, off[-1]).astype(np.int32)
    v = 0.5 + rng.rand(off[-1])
    v[::11] *= -1.0
    ids = np.full((n, 200), -1, np.int32)
    val = np.zeros((n, 200))
    for i in range(n):
        ids[i, :length[i]] = nb[off[i]:off[i + 1]]
        val[i, :length[i]] = v[off[i]:off[i + 1]]
    _, a = same_run(n, (off, nb, v))
    _, b = same_run(n, None, rows=(ids, val))
    assert np.array_equal(bits(a), bits(b))
    _, c = same_run(n, (off, nb, v), dim=3)


@pytest.mark.parametrize("dim", [2, 3])
def test_rescale(dim):
    rng = np.random.RandomState(6)
    for n in (1, BLOCK - 1, BLOCK, BLOCK + 1, 1024 * BLOCK + 3):
        pos = rng.rand(n, dim) * 5 - 2
        out = []
        for m in pair(n, dim):
            m.rescale(0.75, np.arange(dim) - 1.5, pos=pos)
            out.append(m.positions_numpy())
            m.rescale(3.0, None)
            out.append(m.positions_numpy())
            m.rescale(2.0, np.ones(dim), pos=np.zeros((n, dim)))  # max |pos| = 0
            out.append(m.positions_numpy())
            m.free()
        for a, b in zip(out[:3], out[3:]):
            assert np.array_equal(bits(a), bits(b))
        assert np.array_equal(out[2], np.ones((n, dim)))


def test_kernel_attrs():
    m = L().SpringLayout(100, device=0)
    attrs = m.kernel_attrs()
    m.free()
    assert set(attrs) == {"k_layout_init_2", "k_layout_init_3", "k_layout_pairs_2", "k_layout_pairs_3",
                          "k_layout_update_2", "k_layout_update_3", "k_layout_commit", "k_layout_rescale_2",
                          "k_layout_rescale_3"}
    print(attrs)
    for name, a in attrs.items():
        assert a["scratch_bytes"] == 0, name
        assert 0 < a["vgprs"] <= 128, name
    assert attrs["k_layout_pairs_2"]["lds_bytes"] == C * 2 * 8 and attrs["k_layout_pairs_3"]["lds_bytes"] == C * 3 * 8


def test_spring_layout_on_the_device_is_the_hosts():
    from gwamd.graph import GWGraph
    e = karate_edges()
    G = GWGraph.from_edges(e[:, 0], e[:, 1], semantics="nx")
    for kw in (dict(), dict(scale=None), dict(pos={0: (0.0, 0.0), 3: (2.0, 1.0)}, fixed=[0], dim=2),
               dict(dim=3, center=(1, 2, 3))):
        a = L().spring_layout(G, seed=4, device=0, **kw)
        b = L().spring_layout(G, seed=4, device=-1, **kw)
        assert list(a) == list(b) and all(np.array_equal(bits(a[u]), bits(b[u])) for u in a)


def test_cli_parity(tmp_path):
    edges = tmp_path / "karate0.txt"
    np.savetxt(edges, karate_edges(), fmt="%d")
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    files = []
    for device in ("0", "-1"):
        out = tmp_path / f"karate{device}.pos"
        r = subprocess.run([sys.executable, "-m", "gwamd.layout", "--input", str(edges), "--output", str(out),
                            "--device", device, "--seed", "0"], env=env, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        files.append(out.read_bytes())
    assert files[0] == files[1] and files[0].startswith(b"34 2\n")
