"""GPU: one trainer handle used again and again (gw_sgns, gw_deepsim, gw_ovr): buffers that grow in place, tables
and corpora uploaded a second time, a late-allocated buffer, create / free cycles.  Every case drives one device
handle and one device = -1 handle through the same calls; after every step the arrays the device handle exports
equal the host handle's bit for bit.  The host evaluation of the law is the reference.
"""
import ctypes

import numpy as np
import pytest

from test_deepsim_gpu import TENSORS, assert_state_equal, corpus, pair
from test_deepsim_host import synth, trainer
from test_ovr_host import csr, planted, scorer
from test_sgns_host import barbell_corpus, uniform_corpus

pytestmark = pytest.mark.gpu

RB = 64   # GW_OVR_RB: rows per partial block of the one-vs-rest pass


# ---- one-vs-rest ---------------------------------------------------------------------
def ovr_equal(dev, host):
    ed, eh = dev.export(), host.export()
    assert np.array_equal(ed["state"], eh["state"])
    assert np.array_equal(ed["newton_iters"], eh["newton_iters"])
    assert np.array_equal(ed["W"].view(np.uint64), eh["W"].view(np.uint64))
    assert np.array_equal(ed["gnorm"].view(np.uint64), eh["gnorm"].view(np.uint64))
    return eh


def ovr_fit(dev, host, order, T):
    sd, sh = dev.fit(order, T), host.fit(order, T)
    assert (sd.passes, sd.fitted, sd.constant, sd.not_converged, sd.newton_max) == \
        (sh.passes, sh.fitted, sh.constant, sh.not_converged, sh.newton_max)
    return ovr_equal(dev, host)


def ovr_scored(dev, host, rows):
    assert np.array_equal(dev.score(rows), host.score(rows))
    assert np.array_equal(dev.decision(rows[:3]).view(np.uint64), host.decision(rows[:3]).view(np.uint64))


def test_ovr_handle_reuse():
    """Fits over 5, 130 and 7 rows on one handle: the row list, y, z and the partials (1 -> 3 blocks) grow, then a
    short fit runs with stale data behind its live part.  A score over 190 rows grows y / z past any fit.  Labels
    are uploaded again with another nonzero count and with none at all."""
    from gwamd import _lib as C
    n, d, L = 200, 5, 3
    X, Y = planted(n, d, L, 11, extra=0.2)
    order = np.random.RandomState(12).permutation(n).astype(np.int64)
    dev, host = scorer(X, Y, device=0), scorer(X, Y)
    for T in (5, 130, 7):
        assert (T + RB - 1) // RB == (3 if T == 130 else 1)
        eh = ovr_fit(dev, host, order, T)
        assert (eh["state"] == C.OVR_FITTED).any() or T == 5
    assert (eh["state"] == C.OVR_FITTED).any()
    rows = order[7:197]
    assert len(rows) == 190
    cd, ch = dev.score(rows), host.score(rows)
    assert np.array_equal(cd, ch) and ch.sum() > 0
    assert np.array_equal(dev.decision(order[:3]).view(np.uint64), host.decision(order[:3]).view(np.uint64))
    ovr_equal(dev, host)
    # labels again: another nonzero count, then every row empty
    Y2 = np.roll(Y, 1, axis=1) | (np.random.RandomState(13).rand(n, L) < 0.3)
    assert len(csr(Y2)[1]) != len(csr(Y)[1])
    for Yn in (Y2, np.zeros_like(Y)):
        for m in (dev, host):
            m.set_labels(*csr(Yn))
        eh = ovr_fit(dev, host, order, 130)
        ovr_scored(dev, host, order[130:])
        if not Yn.any():
            assert (eh["state"] == C.OVR_CONST_NEG).all()
    # and labels after none
    for m in (dev, host):
        m.set_labels(*csr(Y))
    ovr_fit(dev, host, order, 70)
    ovr_scored(dev, host, order[70:])
    dev.free()
    host.free()


# ---- DeepSim -------------------------------------------------------------------------
def ds_train(dev, host, begin, count, loss=True):
    """The same train call on both; the state bit for bit.  The reported losses agree to 1e-5 relative: both sides
    hold the same logits, maxima and exp-sums bit for bit, and the loss differs only by the two libraries' fp64
    log (test_deepsim_gpu.test_kernel_equals_host_bitwise)."""
    ld, lh = dev.train(begin, count, loss=loss), host.train(begin, count, loss=loss)
    assert_state_equal(dev, host)
    if loss:
        assert ld.shape == lh.shape == (count,)
        print(f"steps [{begin}, {begin + count}): max relative loss difference {np.max(np.abs(ld - lh) / np.abs(lh)):.3g}")
        assert np.all(np.isfinite(lh)) and np.all(np.abs(ld - lh) <= 1e-5 * np.abs(lh))
    else:
        assert ld is None and lh is None


def test_deepsim_handle_reuse():
    """Train calls of 2, 5, 1 and 2 steps on one handle (the loss buffer grows, is kept, is not asked for), a
    gradient evaluation between two of them (the late-allocated w2 gradient buffer, the w1 gradient rows zeroed
    again), the walks set again with more walks and a label map and again without one, the table set again with
    another topk; a train call after each."""
    V, B, d, k, L = 34, 32, 32, 2, 11
    dev, host = pair(V, B, d, k, L, 0, False)
    ds_train(dev, host, 0, 2)
    ds_train(dev, host, 2, 5)
    ds_train(dev, host, 7, 1)
    ds_train(dev, host, 8, 2, loss=False)
    gd, gh = dev.gradients(10), host.gradients(10)
    for t in TENSORS:
        assert np.array_equal(gd[t].view(np.uint32), gh[t].view(np.uint32)), t
    assert gh["w1"].any() and gh["w2"].any()
    assert_state_equal(dev, host)   # nothing was updated
    ds_train(dev, host, 10, 1)
    # more walks, tokens that are labels
    _, _, W2 = corpus(V, k, L, 150, 21)
    labels = np.random.RandomState(22).permutation(V).astype(np.int64)
    for m in (dev, host):
        m.set_walks(W2, labels)
    ds_train(dev, host, 11, 3)
    # fewer walks again, no label map
    _, _, W3 = corpus(V, k, L, B + 9, 23)
    for m in (dev, host):
        m.set_walks(W3, None)
    ds_train(dev, host, 14, 3)
    # another table: topk 7 -> 3 -> 12
    for topk, begin in ((3, 17), (12, 20)):
        ids, sc, _ = synth(V, topk=topk, nwalks=1, L=L, seed=30 + topk, short=False)
        for m in (dev, host):
            m.set_simrank(ids, sc)
        ds_train(dev, host, begin, 3)
    dev.free()
    host.free()


# ---- SGNS ----------------------------------------------------------------------------
def sgns_handle(n, device):
    from gwamd.embed import SGNS
    return SGNS(n, device=device, dim=8, window=3, negative=2, epochs=2, sample=0.0, seed=5)


def sgns_run(m, W):
    """build_vocab + train (concurrency 1: the sequential law) on the handle; everything it exports."""
    if m.device >= 0:
        import torch
        Wd = torch.as_tensor(W, device=f"cuda:{m.device}")
        wp = ctypes.c_void_p(Wd.data_ptr())
    else:
        wp = ctypes.c_void_p(W.ctypes.data)
    m.build_vocab(wp, W.shape[0], W.shape[1])
    st = m.train(wp, W.shape[0], W.shape[1], 0, 2, 1)
    return m.export() + m.sampler() + (np.asarray(st.as_tuple(), np.int64),)


def sgns_equal(a, b):
    assert len(a) == len(b) == 7
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.shape == y.shape
        assert np.array_equal(x.view(np.uint32 if x.itemsize == 4 else np.uint64),
                              y.view(np.uint32 if y.itemsize == 4 else np.uint64))


def test_sgns_handle_reuse():
    """build_vocab a second time on one handle with another corpus: the tables are uploaded again and the vectors
    start again, so the handle equals the host handle that did the same and a fresh device handle that saw the
    second corpus only."""
    W1, n = barbell_corpus()
    W2, _ = uniform_corpus(n, 31, 13, 9, lens=[13, 0, 1, 7])
    dev, host, fresh = sgns_handle(n, 0), sgns_handle(n, -1), sgns_handle(n, 0)
    first = sgns_run(host, W1)
    sgns_equal(sgns_run(dev, W1), first)
    second = sgns_run(host, W2)
    assert not np.array_equal(first[0], second[0]) and second[6][1] > 0   # pairs were trained
    sgns_equal(sgns_run(dev, W2), second)
    sgns_equal(sgns_run(fresh, W2), second)
    for m in (dev, host, fresh):
        m.free()


# ---- create / free -------------------------------------------------------------------
def test_create_free_cycles():
    """20 create / free cycles of each family, then one parity check each: state that outlived its handle, or
    that a later handle took over, shows as wrong bits."""
    from gwamd.classify import OneVsRest
    from gwamd.deepsim import DeepSim
    W, n = barbell_corpus()
    for _ in range(20):
        sgns_handle(n, 0).free()
        DeepSim(34, device=0, dim=32, window=2, batch=32, seed=7).free()
        OneVsRest(200, 3, device=0, dim=5).free()
    dev, host = sgns_handle(n, 0), sgns_handle(n, -1)
    sgns_equal(sgns_run(dev, W), sgns_run(host, W))
    dev.free()
    host.free()
    dev, host = pair(34, 32, 32, 2, 11, 0, False)
    ds_train(dev, host, 0, 2)
    dev.free()
    host.free()
    X, Y = planted(200, 5, 3, 11, extra=0.2)
    order = np.arange(200, dtype=np.int64)
    dev, host = scorer(X, Y, device=0), scorer(X, Y)
    ovr_fit(dev, host, order, 130)
    ovr_scored(dev, host, order[130:])
    dev.free()
    host.free()
