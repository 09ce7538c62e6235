"""learn_embeddings (node2vec/src/main.py:92-101) on the GPU.

The reference trains gensim's Word2Vec(walks, size, window, min_count=0, sg=1,
workers, iter) and calls save_word2vec_format(output).  Here the same
skip-gram / negative-sampling training runs in HIP on the device-resident walk
matrix gw_n2v_walks wrote (gw_sgns_* in include/graphwalk.h); device=-1
evaluates the same law on the host.
"""
import ctypes

import numpy as np

from . import _lib as C

try:
    import torch
except Exception:  # pragma: no cover - torch is optional for the host path
    torch = None


class SGNS:
    """Owning handle over a gw_sgns trainer."""

    def __init__(self, n, device=0, **params):
        self.params = C.SgnsParams(**params)
        self.n = int(n)
        self.device = int(device)
        h = ctypes.c_void_p()
        C.check(C.lib().gw_sgns_create(self.device, self.n, ctypes.byref(self.params), ctypes.byref(h)))
        self._h = h

    @property
    def handle(self):
        return self._h

    def build_vocab(self, walks_ptr, nwalks, walk_len):
        C.check(C.lib().gw_sgns_build_vocab(self._h, walks_ptr, nwalks, walk_len), sgns=self._h)

    def train(self, walks_ptr, nwalks, walk_len, epoch_begin=0, epoch_count=None, concurrency=0, stream=None):
        st = C.SgnsStats()
        if epoch_count is None:
            epoch_count = self.params.epochs - epoch_begin
        C.check(C.lib().gw_sgns_train(self._h, walks_ptr, nwalks, walk_len, epoch_begin, epoch_count, concurrency,
                                      ctypes.byref(st), stream), sgns=self._h)
        return st

    def export(self):
        dim = self.params.dim
        syn0 = np.empty((self.n, dim), np.float32)
        syn1 = np.empty((self.n, dim), np.float32)
        cnt = np.empty(self.n, np.int64)
        C.check(C.lib().gw_sgns_export(self._h, C.ptr(syn0), C.ptr(syn1), C.ptr(cnt)), sgns=self._h)
        return syn0, syn1, cnt

    def sampler(self):
        J = np.empty(self.n, np.int32)
        thr = np.empty(self.n, np.uint32)
        keep = np.empty(self.n, np.uint32)
        C.check(C.lib().gw_sgns_sampler_export(self._h, C.ptr(J), C.ptr(thr), C.ptr(keep)), sgns=self._h)
        return J, thr, keep

    def vectors_dev(self):
        """(address of syn0 where it lives, pitch in floats)."""
        p = ctypes.c_void_p()
        pitch = ctypes.c_int64()
        C.check(C.lib().gw_sgns_vectors_dev(self._h, ctypes.byref(p), ctypes.byref(pitch)), sgns=self._h)
        return p.value, pitch.value

    def vectors_torch(self):
        """syn0 as a torch view [n][dim] of the trainer's own HBM (no copy); valid while this handle lives."""
        if self.device < 0:
            raise ValueError("host evaluation keeps its vectors in host memory (use export())")
        ptr, pitch = self.vectors_dev()

        class _View:  # the CUDA array interface torch.as_tensor reads
            __cuda_array_interface__ = {"shape": (self.n, pitch), "typestr": "<f4", "data": (ptr, False),
                                        "version": 2, "strides": None}
        return torch.as_tensor(_View(), device=f"cuda:{self.device}")[:, :self.params.dim]

    def auto_concurrency(self, nwalks):
        c = ctypes.c_int32()
        C.check(C.lib().gw_sgns_auto_concurrency_for(self._h, nwalks, ctypes.byref(c)), sgns=self._h)
        return c.value

    def kernel_attrs(self, walk_len):
        v, s, l = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        C.check(C.lib().gw_sgns_kernel_attrs(self._h, walk_len, ctypes.byref(v), ctypes.byref(s), ctypes.byref(l)),
                sgns=self._h)
        return {"vgprs": v.value, "scratch_bytes": s.value, "lds_bytes": l.value}

    def free(self):
        if getattr(self, "_h", None):
            C.lib().gw_sgns_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass


def write_word2vec_text(path, syn0, counts, labels=None):
    syn0 = np.ascontiguousarray(syn0, np.float32)
    counts = np.ascontiguousarray(counts, np.int64)
    lab = None if labels is None else np.ascontiguousarray(labels, np.int64)
    C.check(C.lib().gw_write_word2vec_text(str(path).encode(), C.ptr(syn0), C.ptr(counts), C.ptr(lab),
                                           syn0.shape[0], syn0.shape[1]))


class Embedding:
    """What learn_embeddings returns: the subset of gensim's KeyedVectors the
    reference uses (model[label], save_word2vec_format) plus the raw arrays."""

    def __init__(self, vectors, syn1neg, counts, labels, stats, walks_ptr, model):
        self.vectors = vectors          # [n][dim] float32, row = dense id
        self.syn1neg = syn1neg
        self.counts = counts
        self.labels = labels            # dense id -> label
        self.stats = stats
        self.walks_ptr = walks_ptr      # the address the trainer read the walks from
        self.model = model              # the SGNS handle (vectors_dev() for zero-copy use)
        order = np.lexsort((labels, -counts))
        self.index2word = [str(labels[v]) for v in order if counts[v] > 0]
        self._row = {int(l): i for i, l in enumerate(labels)}

    def __getitem__(self, label):
        return self.vectors[self._row[int(label)]]

    def __contains__(self, label):
        try:
            return self.counts[self._row[int(label)]] > 0
        except (KeyError, ValueError):
            return False

    def save_word2vec_format(self, path):
        write_word2vec_text(path, self.vectors, self.counts, self.labels)


def _labels_of(graph_or_labels):
    if graph_or_labels is None:
        return None
    if hasattr(graph_or_labels, "export_csr"):
        return np.asarray(graph_or_labels.export_csr()["labels"], np.int64)
    return np.ascontiguousarray(graph_or_labels, np.int64)


def learn_embeddings(walks, graph_or_labels=None, dimensions=128, window_size=10, iter=10, negative=5, sample=1e-3,
                     seed=0, device=0, concurrency=0):
    """main.py:92-101.  `walks`: a torch int32 CUDA tensor [nwalks][walk_len] of
    dense ids, -1 padded (trained where it is, no host copy), a numpy array of
    the same (device=-1: host evaluation; otherwise uploaded), or the
    reference's list of lists of labels.  `graph_or_labels`: a GWGraph or the
    dense id -> label array (None: labels are the dense ids)."""
    labels = _labels_of(graph_or_labels)
    if torch is not None and isinstance(walks, torch.Tensor):
        if walks.dtype != torch.int32 or walks.dim() != 2 or not walks.is_contiguous():
            raise ValueError("walks tensor must be a contiguous int32 [nwalks][walk_len]")
        if walks.is_cuda:
            device = walks.device.index if walks.device.index is not None else torch.cuda.current_device()
            W = walks
        else:
            W = walks.numpy()
    elif isinstance(walks, np.ndarray):
        W = np.ascontiguousarray(walks, np.int32)
        if W.ndim != 2:
            raise ValueError("walks array must be [nwalks][walk_len]")
    else:  # list of lists of labels (simulate_walks' return value)
        walks = [list(map(int, w)) for w in walks]
        if labels is None:
            labels = np.array(sorted({v for w in walks for v in w}), np.int64)
        dense = {int(l): i for i, l in enumerate(labels)}
        L = max((len(w) for w in walks), default=1) or 1
        W = np.full((len(walks), L), -1, np.int32)
        for i, w in enumerate(walks):
            W[i, :len(w)] = [dense[v] for v in w]
    if isinstance(W, np.ndarray) and device >= 0:
        if torch is None:
            raise ImportError("training on a GPU from a host array needs torch for the upload")
        W = torch.as_tensor(W, device=f"cuda:{device}")
    nwalks, L = int(W.shape[0]), int(W.shape[1])
    if labels is None:
        top = int(W.max()) if nwalks else -1
        labels = np.arange(max(top + 1, 1), dtype=np.int64)
    n = len(labels)
    m = SGNS(n, device=device, dim=dimensions, window=window_size, negative=negative, epochs=iter, sample=sample,
             seed=seed)
    wp = C.ptr(W)
    stream = None
    if device >= 0:
        stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
        torch.cuda.current_stream(device).synchronize()  # the walks are complete before the default-stream copies
    m.build_vocab(wp, nwalks, L)
    st = m.train(wp, nwalks, L, 0, iter, concurrency, stream)
    syn0, syn1, cnt = m.export()
    return Embedding(syn0, syn1, cnt, labels, st, wp.value, m)
