"""The tables gw_dev_bitset_build leaves in HBM, exported with
gw_n2v_export_bitset and checked slot by slot, field by field, against the
numpy reference of tests/bitset_tables.py: headers, all four payload
encodings, dual lists, in-entry and in-region directories, region layout,
unused memory and the draw filters (as an equality of sets: a spurious filter
bit cannot change a walk, only the requests per step).  Both the GW_N2V_BITSET
build and the lists-only build of the listed rejection sampler, on the graphs
of the walk-parity tests plus gadgets placed on every (c, d) threshold and
gadgets of degree >= 65536 (the unpacked-header form of an entry)."""
import numpy as np
import pytest

import bitset_tables as T

pytestmark = pytest.mark.gpu

GRAPHS = sorted(T.EXPECTED_COVERAGE)
BUILDS = {"bitset": (0.25, 4.0), "listed": (1.0, 0.5)}
_SRC = {}
SENTINEL = 0xA5A5A5A5


def _source(gw, name, tmp_path_factory):
    """(constructor of a fresh GWGraph, csr, Reference) of a graph; built once per session."""
    if name not in _SRC:
        kind, make = T.graphs()[name]
        if kind == "edges":
            e = make()
            ctor = lambda: gw.GWGraph.from_edges(e[:, 0], e[:, 1])  # noqa: E731
        elif kind == "rmat":
            ctor = lambda: gw.GWGraph.rmat(*make[0], **make[1])  # noqa: E731
        else:
            path = make
            if kind == "writer":
                path = str(tmp_path_factory.mktemp("bstab") / f"{name}.edgelist")
                make(path)
            ctor = lambda: gw.GWGraph.from_edgelist(path, " ", "nx")  # noqa: E731
        G = ctor()
        csr = G.export_csr()
        G.free()
        ref = T.Reference(csr)
        _SRC[name] = (ctor, csr, ref)
    return _SRC[name]


def _prepare(G, build):
    from gwamd import _lib as C
    p, q = BUILDS[build]
    if build == "listed":
        G.options(listed=1)
    C.check(C.lib().gw_n2v_prepare(G.handle, p, q, C.N2V_BITSET if build == "bitset" else C.N2V_REJECTION), G.handle)
    inf = G.info()
    if build == "listed":
        assert inf.listed == 1
    return inf


def _export(G, inf, build):
    """(entries [nnz, 16] u32, pool words); the pool buffer has the size gw_graph_info implies."""
    from gwamd import _lib as C
    nnz = inf.nnz
    room = (inf.sampler_bytes - 64 * nnz) // 4
    assert room >= 1
    E = np.full((nnz, 16), SENTINEL, np.uint32)
    pool = np.full(room, SENTINEL, np.uint32)
    C.check(C.lib().gw_n2v_export_bitset(G.handle, C.ptr(E), C.ptr(pool)), G.handle)
    if build == "listed":
        # sampler_bytes also counts the rejection sampler's neighbour hash
        # (16 B per slot); the pool is the one placeholder word
        assert inf.sampler_bytes in (64 * nnz + 4, 64 * nnz + 4 + 16 * nnz)
        assert (pool[1:] == SENTINEL).all()
        pool = pool[:1]
    E2 = np.full((nnz, 16), SENTINEL, np.uint32)
    C.check(C.lib().gw_n2v_export_bitset(G.handle, C.ptr(E2), None), G.handle)  # region is optional
    assert (E == E2).all()
    return E, pool


@pytest.mark.parametrize("build", sorted(BUILDS))
@pytest.mark.parametrize("name", GRAPHS)
def test_tables_equal_reference(gw, tmp_path_factory, name, build):
    ctor, csr, ref = _source(gw, name, tmp_path_factory)
    cov = ref.coverage()
    for k in T.EXPECTED_COVERAGE[name]:
        assert cov[k] > 0, (name, k)
    G = ctor().to_device(0)
    try:
        inf = _prepare(G, build)
        assert inf.nnz == ref.nnz
        E, pool = _export(G, inf, build)
        inf2 = _prepare(G, build)  # a second build writes the same bytes
        E2, pool2 = _export(G, inf2, build)
    finally:
        G.free()
    assert inf2.sampler_bytes == inf.sampler_bytes
    assert E.tobytes() == E2.tobytes() and pool.tobytes() == pool2.tobytes()
    lists_only = build == "listed"
    if not lists_only:
        assert inf.sampler_bytes == 64 * ref.nnz + 4 * ref.pool_words()
    assert T.check_tables(ref, E, pool, lists_only) == ref.nnz


def test_checker_names_mutated_fields_of_an_exported_copy(gw, tmp_path_factory):
    """One exported copy, one field changed on the host at a time: a region
    bit flipped, a set filter bit cleared, a clear one set, a directory count
    (in the entry, in the region) raised by one, a list pad replaced by 0,
    w[0] moved by one block."""
    ctor, csr, ref = _source(gw, "thresholds", tmp_path_factory)
    G = ctor().to_device(0)
    try:
        E, pool = _export(G, _prepare(G, "bitset"), "bitset")
    finally:
        G.free()
    T.check_tables(ref, E, pool)
    muts = T.mutations(ref, E, pool)
    assert sorted(muts) == sorted(T.MUTATION_FIELD)
    for name, (E2, pool2, slot) in muts.items():
        assert E2.tobytes() != E.tobytes() or pool2.tobytes() != pool.tobytes()
        with pytest.raises(T.TableMismatch) as ei:
            T.check_tables(ref, E2, pool2)
        assert ei.value.field == T.MUTATION_FIELD[name] and ei.value.slot == slot, (name, str(ei.value))


def test_export_needs_resident_tables(gw, tmp_path_factory):
    """GW_ERR_STATE without bitset or listed tables: not prepared, REPLAY,
    rejection without listed entries (q >= 1, listed = 0), p = q = 1, weighted graphs."""
    import os

    from conftest import DATA
    from gwamd import _lib as C
    karate = os.path.join(DATA, "karate.edgelist")

    def refused(G):
        buf = np.zeros((G.nnz, 16), np.uint32)
        with pytest.raises(C.StateError):
            C.check(C.lib().gw_n2v_export_bitset(G.handle, C.ptr(buf), None), G.handle)

    G = gw.GWGraph.from_edgelist(karate, " ", "nx").to_device(0)
    refused(G)
    for p, q, mode, listed in ((0.25, 4.0, C.N2V_REPLAY, -1), (0.25, 4.0, C.N2V_REJECTION, 1),
                               (1.0, 0.5, C.N2V_REJECTION, 0), (1.0, 1.0, C.N2V_BITSET, -1)):
        G.options(listed=listed)
        C.check(C.lib().gw_n2v_prepare(G.handle, p, q, mode), G.handle)
        refused(G)
    G.options(listed=1)
    C.check(C.lib().gw_n2v_prepare(G.handle, 1.0, 0.5, C.N2V_REJECTION), G.handle)
    buf = np.zeros((G.nnz, 16), np.uint32)
    C.check(C.lib().gw_n2v_export_bitset(G.handle, C.ptr(buf), None), G.handle)  # and back again
    assert buf.any()
    G.free()
    W = gw.GWGraph.from_edgelist(os.path.join(DATA, "weighted_quirks.edgelist"), " ", "nx", False, True).to_device(0)
    W.options(listed=1)
    C.check(C.lib().gw_n2v_prepare(W.handle, 1.0, 0.5, C.N2V_REJECTION), W.handle)
    refused(W)
    W.free()


@pytest.mark.parametrize("mode", ["bitset", "rejection"])
@pytest.mark.parametrize("p,q", [(0.25, 4.0), (4.0, 0.25)])
def test_wide_entries_walks_equal_oracle(gw, oracle, tmp_path_factory, mode, p, q):
    """Walk parity where deg(x) >= 65536 (kp and c in words of their own, a
    40 B payload): 2,004 walks of length 20 without the start shuffle, in
    windows that begin at each gadget's x and around its u (the leaves left
    off the ballast vertex, whose entries are c = 0 regions, sit next to u)."""
    import torch
    from gwamd import _lib as C
    ctor, csr, ref = _source(gw, "wide", tmp_path_factory)
    _, gadgets = T.wide_graph()
    order = csr["node_order"]
    where = np.empty(len(order), np.int64)
    where[order] = np.arange(len(order))
    G = ctor().to_device(0)
    try:
        if mode == "rejection":
            G.options(listed=1)
        C.check(C.lib().gw_n2v_prepare(G.handle, p, q, C.N2V_BITSET if mode == "bitset" else C.N2V_REJECTION),
                G.handle)
        if mode == "rejection":
            assert G.info().listed == (1 if q < 1 else 0)
        L, seed = 20, 13
        windows = []
        for c, d, ids in gadgets:
            windows += [(int(where[ids["x"]]), 84), (int(where[ids["u"]]) - 41, 83)]
        got = []
        for begin, count in windows:
            out = torch.empty((count, L), dtype=torch.int32, device="cuda")
            lens = torch.empty(count, dtype=torch.int32, device="cuda")
            cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
            C.check(C.lib().gw_n2v_walks(G.handle, L, seed, begin, count, 0, C.ptr(out), C.ptr(lens), C.ptr(cnt),
                                         None), G.handle)
            got.append((out, lens, cnt))
        torch.cuda.synchronize()
    finally:
        G.free()
    steps_into_wide = 0
    for (begin, count), (out, lens, cnt) in zip(windows, got):
        if mode == "bitset":
            r, rl, rc = oracle.walks_bitset(csr, p, q, seed, L, begin, count, shuffle=False, nthreads=8)
        else:
            r, rl, rc = oracle.walks_scale(dict(csr, weights=None), p, q, seed, L, begin, count, shuffle=False,
                                           nthreads=8)
        np.testing.assert_array_equal(out.cpu().numpy(), r, err_msg=f"window {begin}+{count}")
        np.testing.assert_array_equal(lens.cpu().numpy(), rl)
        assert int(cnt[0]) == int(rc[0]) and int(cnt[1]) == int(rc[1])
        steps_into_wide += int((ref.deg[r[:, 1:][r[:, 1:] >= 0]] >= 65536).sum())
    assert sum(c for _, c in windows) == 2004
    assert steps_into_wide > 2000  # entries with the unpacked header are what these walks read
