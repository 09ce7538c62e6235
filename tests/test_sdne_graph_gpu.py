"""GPU: the SDNE graph loss in the kernels (gw_sdne.hip: the weighted layer-4 epilogue, k_sdne_first, the add after
the mask, the shuffled k_sdne_batch) against the host evaluation of the same law (device = -1), bit for bit, with
nonzero_weight = 3, first_order = 0.7 and shuffle on: all eight parameters, both Adam moments, the encodings and
batch_rows after 1 and 3 steps; the losses (fp64 sums outside the bit law) to 1e-5 relative.  N = u0 = 2B + 3 unless
given, so step 2 lies in epoch 1.
"""
import os

import numpy as np
import pytest

from conftest import DATA
from test_sdne_gpu import feed
from test_sdne_graph_host import ALPHA, BETA, ON, square_rows
from test_sdne_host import TENSORS, state_equal

pytestmark = pytest.mark.gpu

KARATE = os.path.join(DATA, "karate.edgelist")


def _S():
    from gwamd import _lib as C
    from gwamd import sdne
    C.lib()
    return sdne


def check_pair(units, B, X, how="device", checkpoints=(1, 3), seed=7):
    """Train a device and a host handle side by side with the options on; compare at every checkpoint."""
    S = _S()
    dev = S.SdneModel(units, device=0, batch=B, seed=seed, **ON)
    host = S.SdneModel(units, device=-1, batch=B, seed=seed, **ON)
    feed(dev, X, how)
    feed(host, X, how)
    done = 0
    for n in checkpoints:
        for t in range(done, n):
            assert np.array_equal(dev.batch_rows(t), host.batch_rows(t)), f"rows of step {t}"
        ld, lh = dev.train(done, n - done), host.train(done, n - done)
        done = n
        a, b = dev.export(), host.export()
        for t in TENSORS:
            assert np.array_equal(a[t], b[t]), f"{t} after {n} steps"
            assert np.array_equal(a["m"][t], b["m"][t]) and np.array_equal(a["v"][t], b["v"][t]), f"Adam {t} after {n}"
        assert np.array_equal(dev.encode(), host.encode()), f"encoding after {n} steps"
        assert np.all(np.isfinite(lh)) and np.abs(ld - lh).max() <= 1e-5 * np.abs(lh).max(), (ld, lh)
    out = dev.export()
    dev.free()
    host.free()
    return out


@pytest.mark.parametrize("hidden,B,n", [((1, 31, 32), 1, None), ((31, 32, 33), 31, None), ((32, 33, 64), 33, None),
                                        ((64, 65, 1), 100, None), ((129, 513, 64), 128, 259), ((16, 1024, 16), 128, 259),
                                        ((40, 16, 24), 100, 513)])
def test_bits_against_the_host(hidden, B, n):
    """Batches 1, 31, 33, 100 (one and two waves of S, with tails) and 128 (a full 128 x 128 S block; u2 = 513 and
    the cap 1024: more than one trip over c); N = u0 = 513: the split launch, whose reduce applies the weighted
    layer-4 epilogue.  B = 1 has no pair (a_ii = 0): S = 0."""
    n = n or 2 * B + 3
    check_pair((n,) + hidden, B, square_rows(n, 2 + B, weighted=False, density=0.4))


def test_no_edge_inside_a_batch():
    """A graph without an edge inside any of the three batches trained on: S = 0 and g1 is all +0."""
    S = _S()
    B, n = 31, 65
    probe = S.SdneModel((n, 31, 32, 33), device=-1, batch=B, seed=7, **ON)
    probe.set_rows(np.zeros((n, n), np.float32))
    X = square_rows(n, 40, weighted=False, density=0.5)
    for t in range(3):
        ids = probe.batch_rows(t)
        X[np.ix_(ids, ids)] = 0.0
    probe.free()
    assert np.array_equal(X, X.T) and np.count_nonzero(X) > n
    check_pair((n, 31, 32, 33), B, X)


def test_asymmetric_weighted_csr():
    """a_ij != a_ji with weights, given as CSR (scattered by k_sdne_batch) and as the same matrix dense in device
    memory: both equal the host, hence each other."""
    n, B = 69, 33
    X = square_rows(n, 12, weighted=True, density=0.3)
    assert (X != X.T).any() and len(set(X.ravel().tolist())) > 100
    a = check_pair((n, 32, 33, 64), B, X, how="csr")
    b = check_pair((n, 32, 33, 64), B, X, how="device")
    assert state_equal(a, b)


def test_gradients_on_the_device():
    S = _S()
    n, B = 69, 33
    units = (n, 65, 33, 31)
    X = square_rows(n, 10, weighted=True)
    dev = S.SdneModel(units, device=0, batch=B, seed=3, **ON)
    host = S.SdneModel(units, device=-1, batch=B, seed=3, **ON)
    for m in (dev, host):
        m.set_rows(X)
        m.train(0, 2)
    before = dev.export()
    for step in (2, 3):
        a, b = dev.gradients(step), host.gradients(step)
        for t in TENSORS:
            assert np.array_equal(a[t], b[t]), t
    assert state_equal(dev.export(), before)                               # gradients() updates nothing
    plain = S.SdneModel(units, device=0, batch=B, seed=3, nonzero_weight=BETA, shuffle=1)
    plain.set_rows(X)
    plain.train(0, 2)
    assert ALPHA > 0 and not np.array_equal(plain.gradients(0)["w2"], dev.gradients(0)["w2"])
    for m in (dev, host, plain):
        m.free()


def test_cli_end_to_end(tmp_path):
    S = _S()
    out = {}
    for dev in (0, -1):
        out[dev] = str(tmp_path / f"k{dev}.emb")
        assert S.cli(["--input", KARATE, "--delimiter", " ", "--output", out[dev], "--units", "16,8,12", "--batch",
                      "17", "--steps", "50", "--seed", "5", "--beta", "5", "--alpha", "0.1", "--shuffle",
                      "--device", str(dev)]) == 0
    plain = str(tmp_path / "plain.emb")
    assert S.cli(["--input", KARATE, "--delimiter", " ", "--output", plain, "--units", "16,8,12", "--batch", "17",
                  "--steps", "50", "--seed", "5", "--device", "-1"]) == 0
    with open(out[0], "rb") as f, open(out[-1], "rb") as g, open(plain, "rb") as h:
        a = f.read()
        assert a == g.read() and a.startswith(b"34 8\n") and a != h.read()


def test_kernel_attrs_name_the_first_order_kernel():
    S = _S()
    m = S.SdneModel((40, 8, 4, 8), device=0, batch=4, first_order=0.5)
    attrs = m.kernel_attrs()
    m.free()
    print({k: attrs[k] for k in ("k_sdne_first", "k_sdne_batch", "k_sdne_gemm", "k_sdne_loss_part")})
    assert "k_sdne_first" in attrs and attrs["k_sdne_first"]["vgprs"] > 0
    assert attrs["k_sdne_first"]["lds_bytes"] >= 2 * 128 * 4                # S_i. and its j list
