"""GPU: the SDNE kernels (gw_sdne.hip) against the host evaluation of the same law (device = -1), bit for bit:
all eight parameters, both Adam moments and the encodings after 1 and 3 steps (more where stated); the losses, which
are fp64 sums outside the bit law, to 1e-5 relative.

The shapes walk the kernels' edges: 64x64 output tiles of 32x32 MFMA blocks (widths and batches around 32 and 64),
reduction chunks of GW_SDNE_KC = 128 (u0 around 128 and 256), the in-kernel chunk loop (at most 4 chunks) against
the split launch with its ordered reduce (784 = 7 chunks, 10313 = 81 chunks, more than the reduce's unrolled trip
of 8), the schedule's wrap and the untrained row tail.
"""
import os

import numpy as np
import pytest

from conftest import DATA
from test_sdne_host import TENSORS, csr_of, rows_for, state_equal

pytestmark = pytest.mark.gpu

KARATE = os.path.join(DATA, "karate.edgelist")
KC = 128


def _S():
    from gwamd import _lib as C
    from gwamd import sdne
    C.lib()
    return sdne


def feed(m, X, how):
    """how: 'dense' (a numpy matrix; uploaded for a device handle), 'device' (a CUDA tensor, read where it lies),
    'csr', or a ready (offsets, cols, vals) triple."""
    import torch
    if isinstance(how, tuple):
        m.set_csr(*how)
    elif how == "csr":
        m.set_csr(*csr_of(X))
    elif how == "device" and m.device >= 0:
        m.set_rows(torch.as_tensor(X, device=f"cuda:{m.device}"))
    else:
        m.set_rows(X)


def check_pair(units, B, X, how="device", checkpoints=(1, 3), seed=7, **params):
    """Train a device and a host handle side by side; compare at every checkpoint."""
    S = _S()
    dev = S.SdneModel(units, device=0, batch=B, seed=seed, **params)
    host = S.SdneModel(units, device=-1, batch=B, seed=seed, **params)
    feed(dev, X, how)
    feed(host, X, how)
    assert state_equal(dev.export(), host.export())
    done = 0
    for n in checkpoints:
        ld, lh = dev.train(done, n - done), host.train(done, n - done)
        done = n
        a, b = dev.export(), host.export()
        for t in TENSORS:
            assert np.array_equal(a[t], b[t]), f"{t} after {n} steps"
            assert np.array_equal(a["m"][t], b["m"][t]) and np.array_equal(a["v"][t], b["v"][t]), f"Adam {t} after {n}"
        assert np.array_equal(dev.encode(), host.encode()), f"encoding after {n} steps"
        assert np.all(np.isfinite(lh)) and np.abs(ld - lh).max() <= 1e-5 * np.abs(lh).max(), (ld, lh)
    assert np.array_equal(dev.vectors_torch().cpu().numpy(), host.encode())
    dev.free()
    host.free()


def test_reference_shape():
    """(784, 400, 100, 300, 784), B = 100, N = 250, the matrix in device memory: tile tails in every dimension, 7
    chunks over u0 (the split launch), 4 over u1 (the in-kernel loop), the schedule wraps and 50 rows are untrained
    but encoded; also after 20 steps."""
    check_pair((784, 400, 100, 300), 100, rows_for(250, 784, 1, density=0.2), checkpoints=(1, 3, 20))


@pytest.mark.parametrize("hidden,B,u0", [((1, 31, 32), 1, 37), ((31, 32, 33), 31, 64), ((32, 33, 64), 32, 65),
                                         ((33, 64, 65), 33, 100), ((64, 65, 1), 100, 33), ((65, 1, 31), 32, 129)])
def test_tile_edges(hidden, B, u0):
    check_pair((u0,) + hidden, B, rows_for(2 * B + 1, u0, 2, density=0.5))


@pytest.mark.parametrize("u0", [KC - 1, KC, KC + 1, 2 * KC + 1, 4 * KC + 1])
def test_chunk_edges(u0):
    """u0 around one and two chunks (the in-kernel chunk loop) and just past four (the first split launch)."""
    check_pair((u0, 33, 8, 20), 10, rows_for(23, u0, 3))


def test_hidden_chunks():
    """Hidden widths past one chunk and past four: u1 = 129 (2 chunks), u3 = 513 (5 chunks: forward layer 4 and
    the backward product over u3 take the split launch), B = 128 (the cap)."""
    check_pair((70, 129, 16, 513), 128, rows_for(130, 70, 4))


def test_many_chunks():
    """u0 = 10313 (81 chunks; the reduce adds 8 a trip), CSR rows of about ten entries, N = 2B."""
    rng = np.random.RandomState(5)
    u0, B = 10313, 100
    offs = np.zeros(2 * B + 1, np.int64)
    cols = []
    for r in range(2 * B):
        cols += sorted(rng.choice(u0, rng.randint(6, 15), replace=False).tolist())
        offs[r + 1] = len(cols)
    vals = rng.uniform(0.2, 1.0, len(cols)).astype(np.float32)
    check_pair((u0, 400, 100, 300), B, None, how=(offs, np.asarray(cols, np.int32), vals))


def test_csr_equals_dense_on_the_device():
    S = _S()
    import torch
    units, B = (200, 48, 12, 40), 20
    X = rows_for(3 * B + 7, units[0], 6)
    out = []
    for how in ("csr", "device"):
        m = S.SdneModel(units, device=0, batch=B, seed=9)
        feed(m, X, how)
        losses = m.train(0, 5)
        out.append((m.export(), m.encode(), losses))
        m.free()
    assert state_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    assert np.array_equal(out[0][2], out[1][2])
    # a pitched view of a wider device matrix is read where it lies
    wide = torch.zeros((len(X), units[0] + 5), device="cuda:0")
    wide[:, :units[0]] = torch.as_tensor(X, device="cuda:0")
    m = S.SdneModel(units, device=0, batch=B, seed=9)
    m.set_rows(wide[:, :units[0]])
    m.train(0, 5)
    assert state_equal(m.export(), out[0][0])
    m.free()


def test_weighted_graph_rows():
    """A weighted graph's adjacency rows through GWGraph, weights as the values."""
    from gwamd import GWGraph
    rng = np.random.RandomState(8)
    n = 90
    src = rng.randint(0, n, 600)
    dst = rng.randint(0, n, 600)
    keep = src != dst
    g = GWGraph.from_edges(src[keep], dst[keep], rng.uniform(0.5, 3.0, keep.sum()))
    csr = g.export_csr()
    N = len(csr["offsets"]) - 1
    assert len(set(np.round(csr["weights"], 6))) > 10
    check_pair((N, 40, 10, 24), 30, None, how=(csr["offsets"], csr["nbrs"], csr["weights"].astype(np.float32)))


def test_gradients_on_the_device():
    S = _S()
    units, B = (300, 65, 33, 31), 33
    X = rows_for(2 * B + 3, units[0], 10)
    dev = S.SdneModel(units, device=0, batch=B, seed=3)
    host = S.SdneModel(units, device=-1, batch=B, seed=3)
    for m in (dev, host):
        m.set_rows(X)
        m.train(0, 2)
    before = dev.export()
    for step in (2, 3):
        a, b = dev.gradients(step), host.gradients(step)
        for t in TENSORS:
            assert np.array_equal(a[t], b[t]), t
    assert state_equal(dev.export(), before)                               # gradients() updates nothing
    assert not np.array_equal(dev.gradients(2)["w1"], dev.gradients(3)["w1"])
    dev.free()
    host.free()


def test_caps():
    S = _S()
    from gwamd import _lib as C
    for units, B in (((40, 8, 4, 8), 129), ((40, 1025, 4, 8), 4), ((40, 8, 1025, 8), 4), ((40, 8, 4, 1025), 4)):
        with pytest.raises(C.UnsupportedError):
            S.SdneModel(units, device=0, batch=B)
        S.SdneModel(units, device=-1, batch=B).free()                      # the host takes it
    S.SdneModel((40, 1024, 4, 8), device=0, batch=128).free()
    attrs = S.SdneModel((40, 8, 4, 8), device=0, batch=4).kernel_attrs()
    assert {"k_sdne_batch", "k_sdne_gemm", "k_sdne_reduce", "k_sdne_q", "k_sdne_bias"} <= set(attrs)
    assert all(a["scratch_bytes"] == 0 for a in attrs.values())


def test_regrow():
    """One handle, rows set twice, the second time more rows and more entries (u0 kept): the buffers regrow; the
    result is a fresh handle's, and the host's."""
    S = _S()
    units, B = (120, 24, 6, 16), 8
    X1, X2 = rows_for(2 * B, units[0], 1, density=0.1), rows_for(5 * B + 3, units[0], 2, density=0.4)
    a = S.SdneModel(units, device=0, batch=B, seed=5)
    a.set_csr(*csr_of(X1))
    e1 = a.encode()
    a.set_csr(*csr_of(X2))
    fresh = S.SdneModel(units, device=0, batch=B, seed=5)
    fresh.set_csr(*csr_of(X2))
    host = S.SdneModel(units, device=-1, batch=B, seed=5)
    host.set_csr(*csr_of(X1))
    assert np.array_equal(host.encode(), e1)
    host.set_csr(*csr_of(X2))
    for m in (a, fresh, host):
        m.train(0, 6)
    assert state_equal(a.export(), fresh.export()) and state_equal(a.export(), host.export())
    ea = a.encode()
    assert ea.shape == (5 * B + 3, 6) and np.array_equal(ea, fresh.encode()) and np.array_equal(ea, host.encode())
    for m in (a, fresh, host):
        m.free()


def test_cli_end_to_end(tmp_path):
    S = _S()
    out = {}
    for dev in (0, -1):
        out[dev] = str(tmp_path / f"k{dev}.emb")
        assert S.cli(["--input", KARATE, "--delimiter", " ", "--output", out[dev], "--units", "16,8,12", "--batch",
                      "17", "--steps", "50", "--seed", "5", "--device", str(dev)]) == 0
    with open(out[0], "rb") as f, open(out[-1], "rb") as g:
        a = f.read()
        assert a == g.read() and a.startswith(b"34 8\n")
