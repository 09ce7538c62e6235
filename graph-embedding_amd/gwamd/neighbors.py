"""Nearest neighbours of an embedding on the GPU.

The reference's users load an embedding as gensim KeyedVectors
(DeepSim/src/main.py:287), whose most_similar is cosine top-n;
IsoMap_LE/LE.py:53-60 carries a brute-force knn.  Here the all-pairs scores and
the top-k selection run fused in HIP (gw_knn_* in include/graphwalk.h) on the
matrix where it already lies in HBM; device=-1 evaluates the same law on the
host, bit for bit.  Rows come back in gw_topsim's layout (ids int32, scores
float64, -1 padded), so gw_write_sim_text_topk writes them and
topsim.precision compares them with SimRank's top-k; label_agreement restates
preprocess_simrank (DeepSim/src/main.py:132-167).

    python -m gwamd.neighbors --emb x.emb --output x.nn [--topk 20] [--metric cosine|dot]
        [--gold g.sim.txt] [--groups groups.csv] [--device N]
"""
import argparse
import ctypes
import sys

import numpy as np

from . import _lib as C

try:
    import torch
except Exception:  # pragma: no cover - torch is optional for the host path
    torch = None

METRICS = {"cosine": C.KNN_COSINE, "dot": C.KNN_DOT}


class _PairsHandle:
    """What the owning handles over gw_knn and gw_nng share; `_prefix` is the C prefix and the C.check keyword."""

    _prefix = None

    def _fn(self, name):
        return getattr(C.lib(), f"gw_{self._prefix}_{name}")

    def _call(self, name, *args):
        C.check(self._fn(name)(self._h, *args), **{self._prefix: self._h})

    def _create(self, n, device, params):
        self.params = params
        self.n, self.device = int(n), int(device)
        h = ctypes.c_void_p()
        C.check(self._fn("create")(self.device, self.n, ctypes.byref(self.params), ctypes.byref(h)),
                **{self._prefix: True})
        self._h = h
        self._keep = []

    @property
    def handle(self):
        return self._h

    def set_rows(self, n):
        """Another row count for the next set_vectors."""
        self._call("set_rows", int(n))
        self.n = int(n)
        self._keep = []

    def set_vectors(self, x, pitch=None):
        """x: float32 [n][>= dim], rows contiguous: a torch CUDA tensor (device >= 0; read where it is), a numpy
        array (device = -1; uploaded when device >= 0) or a raw address with `pitch` in floats."""
        if isinstance(x, int):
            p = ctypes.c_void_p(x)
        else:
            if isinstance(x, np.ndarray):
                if x.dtype != np.float32 or x.ndim != 2 or x.strides[1] != 4 or x.strides[0] % 4:
                    x = np.ascontiguousarray(x, np.float32)
                if self.device >= 0:
                    x = torch.as_tensor(np.ascontiguousarray(x), device=f"cuda:{self.device}")
            elif x.dtype != torch.float32 or x.dim() != 2 or x.stride(1) != 1:
                raise ValueError("vectors tensor must be float32 [n][dim] with contiguous rows")
            if x.shape[0] != self.n or x.shape[1] < self.params.dim:
                raise ValueError(f"vectors must be [{self.n}][>= {self.params.dim}]")
            pitch = x.stride(0) if hasattr(x, "stride") else x.strides[0] // 4
            p = C.ptr(x)
            self._keep = [x]
        self._call("set_vectors", p, int(pitch))

    def tiles(self):
        """{'tq', 'tc', 'kc', 'buf'}: the main kernel's launch geometry and the per-row buffer length."""
        v = [ctypes.c_int32() for _ in range(4)]
        self._call("tiles", *[ctypes.byref(t) for t in v])
        return dict(zip(("tq", "tc", "kc", "buf"), (t.value for t in v)))

    def kernel_attrs(self):
        """{kernel name: {'vgprs', 'scratch_bytes', 'lds_bytes'}} (hipFuncGetAttributes)."""
        cap = 16
        names = (ctypes.c_char_p * cap)()
        v, s, l = ((ctypes.c_int32 * cap)() for _ in range(3))
        n = ctypes.c_int32()
        self._call("kernel_attrs", cap, names, v, s, l, ctypes.byref(n))
        return {names[i].decode(): {"vgprs": v[i], "scratch_bytes": s[i], "lds_bytes": l[i]}
                for i in range(min(n.value, cap))}

    def free(self):
        if getattr(self, "_h", None):
            self._fn("free")(self._h)
            self._h = None
            self._keep = []

    def __del__(self):
        try:
            self.free()
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass


class Neighbors(_PairsHandle):
    """Owning handle over a gw_knn."""

    _prefix = "knn"

    def __init__(self, n, device=0, dim=128, topk=20, metric="cosine"):
        self._create(n, device, C.KnnParams(dim=int(dim), topk=int(topk), metric=METRICS.get(metric, metric)))

    def query(self, sources=None, stream=None):
        """(ids int32 [nsrc][topk], scores float64 [nsrc][topk]) as numpy arrays; sources None: every row."""
        topk = self.params.topk
        if sources is not None:
            sources = np.ascontiguousarray(sources, np.int32).reshape(-1)
        nsrc = self.n if sources is None else len(sources)
        if self.device < 0:
            ids = np.empty((nsrc, topk), np.int32)
            sc = np.empty((nsrc, topk), np.float64)
            self._call("query", C.ptr(sources), nsrc, C.ptr(ids), C.ptr(sc), None)
            return ids, sc
        dev = f"cuda:{self.device}"
        src = None if sources is None else torch.as_tensor(sources, device=dev)
        ids = torch.empty((nsrc, topk), dtype=torch.int32, device=dev)
        sc = torch.empty((nsrc, topk), dtype=torch.float64, device=dev)
        if stream is None:
            stream = ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        self._call("query", C.ptr(src), nsrc, C.ptr(ids), C.ptr(sc), stream)
        return ids.cpu().numpy(), sc.cpu().numpy()

    def fma_rate(self, blocks=2048, iters=20000):
        """fp64 fused multiply-adds per second of 16 independent chains per lane (the main loop's ceiling)."""
        r = ctypes.c_double()
        self._call("fma_rate", int(blocks), int(iters), ctypes.byref(r))
        return r.value


def _vectors_of(vectors, device):
    """(what set_vectors takes, device) of a tensor, an array, an Embedding (gwamd.embed) or a live SGNS / DeepSim
    trainer.  A trainer on a GPU is read where its vectors lie, on its own device."""
    if hasattr(vectors, "model") and hasattr(vectors, "vectors"):  # Embedding
        if device >= 0 and vectors.model.device >= 0 and getattr(vectors.model, "_h", None):
            return vectors.model.vectors_torch(), vectors.model.device
        return np.asarray(vectors.vectors, np.float32), device
    if hasattr(vectors, "vectors_torch") and hasattr(vectors, "export"):  # SGNS, DeepSim
        if vectors.device >= 0 and device >= 0:
            return vectors.vectors_torch(), vectors.device
        e = vectors.export(states=False)["w1"] if hasattr(vectors, "gradients") else vectors.export()[0]
        return e, device
    if torch is not None and isinstance(vectors, torch.Tensor):
        if vectors.is_cuda:
            return vectors, vectors.device.index if vectors.device.index is not None else torch.cuda.current_device()
        vectors = vectors.numpy()
    return vectors, device


def most_similar(vectors, sources=None, topk=20, metric="cosine", device=0):
    """For every source row (None: all) the `topk` other rows of largest cosine (gensim's most_similar) or dot
    product: (ids int32 [nsrc][topk], scores float64 [nsrc][topk]), score descending then id ascending, -1 / 0.0
    padded.  `vectors`: a torch CUDA float32 tensor (used in place, pitch from its stride), a numpy array, or a
    live SGNS / DeepSim trainer (zero-copy through *_vectors_dev)."""
    x, device = _vectors_of(vectors, device)
    m = Neighbors(x.shape[0], device=device, dim=x.shape[1], topk=topk, metric=metric)
    try:
        m.set_vectors(x)
        return m.query(sources)
    finally:
        m.free()


def label_agreement(ids, groups, node_labels=None, row_ids=None):
    """preprocess_simrank (DeepSim/src/main.py:132-167) on top-k rows: acc[t-1], t = 1 .. topk, is the share of the
    first min(t, listed) neighbours of every row that have a label in common with the row's vertex.  `groups`:
    classify.read_groups' dict (vertex i = the i-th entry of `node_labels`, or the i-th node in numeric order), or a
    pair (row_off, label ids) in vertex order.  `row_ids`: the vertex of each row (None: row r is vertex r)."""
    from . import classify
    if isinstance(groups, dict):
        _, _, row_off, lab = classify.groups_csr(groups, node_labels)
    else:
        row_off, lab = groups
    row_off = np.ascontiguousarray(row_off, np.int64)
    lab = np.ascontiguousarray(lab, np.int32)
    ids = np.ascontiguousarray(ids, np.int32)
    if ids.ndim != 2:
        raise ValueError("ids must be [nrows][topk]")
    rid = None if row_ids is None else np.ascontiguousarray(row_ids, np.int32)
    acc = np.zeros(ids.shape[1], np.float64)
    C.check(C.lib().gw_topk_label_agreement(C.ptr(ids), ids.shape[0], ids.shape[1], C.ptr(rid), C.ptr(row_off),
                                            C.ptr(lab), len(row_off) - 1, C.ptr(acc)), knn=True)
    return acc


def write_neighbors(path, ids, scores, labels=None, decimals=6):
    """`path` gets "v,id,...\\r\\n" and `path`.sim.txt "v,id:score,...\\r\\n" (gw_write_sim_text_topk), row r being
    vertex r; with `labels` (one integer per vertex) rows and ids are written as labels."""
    ids = np.ascontiguousarray(ids, np.int32)
    scores = np.ascontiguousarray(scores, np.float64)
    rid = None
    if labels is not None:
        lab = np.asarray([int(l) for l in labels], np.int64)
        if len(lab) and (lab.min() < 0 or lab.max() >= 2 ** 31):
            raise ValueError("labels must be non-negative 32-bit integers")
        rid = np.ascontiguousarray(lab, np.int32)
        ids = np.where(ids >= 0, rid[np.maximum(ids, 0)], -1).astype(np.int32)
    C.check(C.lib().gw_write_sim_text_topk(str(path).encode(), C.ptr(ids), C.ptr(scores), C.ptr(rid), ids.shape[0],
                                           ids.shape[1], b",", int(decimals)))


def report(path, ids, node_labels=None, gold=None, groups=None, topk=20, file=None):
    """What the command line prints for the rows written to `path`: topsim.precision against `gold`, and the label
    agreement curve for `groups` (a groups file)."""
    if gold:
        from . import topsim
        pre = topsim.precision(gold, path + ".sim.txt", path + ".pre.txt", topk, topk=topk)
        print(f"precision against {gold}: {pre}", file=file)
    if groups:
        from . import classify
        acc = label_agreement(ids, classify.read_groups(groups), node_labels)
        for t, a in enumerate(acc):
            print("Top: %d, acc: " % (t + 1), a, file=file)
        print("mean acc:", float(acc.mean()), file=file)


def neighbors_of(vectors, path, labels=None, topk=20, metric="cosine", device=0, gold=None, groups=None, file=None):
    """most_similar of every row, written to `path` / `path`.sim.txt, then report().  With `labels` (one integer
    per row) the rows are taken in ascending label order first, so that the files do not depend on the order the
    embedding was stored in (a word2vec text file lists its rows by count).  Returns (ids, scores) in the order
    written."""
    if labels is not None:
        lab = np.asarray([int(l) for l in labels], np.int64)
        perm = np.argsort(lab, kind="stable")
        if not np.array_equal(perm, np.arange(len(lab))):
            vectors, device = _vectors_of(vectors, device)
            vectors = vectors[perm if isinstance(vectors, np.ndarray) else torch.as_tensor(perm, device=vectors.device)]
        labels = lab[perm]
    ids, scores = most_similar(vectors, topk=topk, metric=metric, device=device)
    write_neighbors(path, ids, scores, labels)
    report(str(path), ids, None if labels is None else [str(l) for l in labels], gold, groups, topk, file)
    return ids, scores


def cli(argv=None):
    from . import classify
    ap = argparse.ArgumentParser(description="Top-k nearest neighbours of an embedding on MI355X.")
    ap.add_argument("--emb", required=True, help="embeddings (word2vec text / save_embeddings format)")
    ap.add_argument("--output", required=True, help="rows `v,id,...`; OUTPUT.sim.txt gets `v,id:score,...`")
    ap.add_argument("--topk", type=int, default=20)
    ap.add_argument("--metric", choices=sorted(METRICS), default="cosine")
    ap.add_argument("--gold", default=None, help="a .sim.txt (e.g. SimRank's top-k): print Eval.precision against it")
    ap.add_argument("--groups", default=None, help="lines `node,label`: print the label agreement of the neighbours")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args(argv)
    labels, X = classify.read_embedding(args.emb)
    neighbors_of(X, args.output, labels, args.topk, args.metric, args.device, args.gold, args.groups)
    print(f"{len(labels)} x {args.topk} neighbours -> {args.output}", file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(cli())
