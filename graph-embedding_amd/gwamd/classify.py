"""classify.scoring (node2vec/src/classify.py, DeepSim/src/classify.py) on the GPU.

The reference shuffles the vertices, fits a one-vs-rest
LogisticRegression(penalty='l2') on a share of the embedding rows, predicts for
every held-out vertex as many labels as it really has (TopKRanker) and prints
micro- and macro-F1.  Here the fit, the prediction and the counts run in HIP
(gw_ovr_* in include/graphwalk.h) on the embedding where it already lies in
HBM; device=-1 evaluates the same law on the host, bit for bit.

    python -m gwamd.classify --emb blog.emb --groups groups.csv
"""
import argparse
import ctypes
import sys

import numpy

from . import _lib as C

try:
    import torch
except Exception:  # pragma: no cover - torch is optional for the host path
    torch = None

np = numpy
STATES = {C.OVR_CONST_NEG: "constant-negative", C.OVR_CONST_POS: "constant-positive", C.OVR_FITTED: "fitted",
          C.OVR_NOT_CONVERGED: "not-converged"}


def read_groups(path):
    """DeepSim/src/main.py:109-130: lines `node,label` -> {node: [label, ...]} (strings, in file order)."""
    groups = {}
    with open(path) as f:
        for line in f:
            words = line.split(",")
            if len(words) < 2:
                continue
            groups.setdefault(words[0], []).append(words[1].rstrip("\n"))
    return groups


def groups_csr(groups, node_labels=None):
    """{node: [label, ...]} -> (nodes, label names, row_off int64 [n + 1], ids int32 [nnz]).  Rows follow
    `node_labels` (the label of every feature row) or, without it, the nodes sorted numerically; label names are
    sorted numerically, so column c is the c-th smallest label."""
    key = lambda s: (0, int(s)) if str(s).lstrip("-").isdigit() else (1, str(s))  # noqa: E731
    names = sorted({l for ls in groups.values() for l in ls}, key=key)
    col = {l: i for i, l in enumerate(names)}
    nodes = sorted(groups, key=key) if node_labels is None else [str(v) for v in node_labels]
    row_off = np.zeros(len(nodes) + 1, np.int64)
    ids = []
    for i, v in enumerate(nodes):
        row = sorted({col[l] for l in groups.get(v, [])})
        ids.extend(row)
        row_off[i + 1] = len(ids)
    return nodes, names, row_off, np.asarray(ids, np.int32)


def read_embedding(path):
    """The word2vec text format (save_word2vec_format) and save_embeddings' (DeepSim.py:344-362): a header
    `<rows> <dim>`, then `<label> v v ... v`.  Returns (labels as strings, float32 [rows][dim])."""
    with open(path) as f:
        head = f.readline().split()
        labels, rows = [], []
        for line in f:
            t = line.split()
            if not t:
                continue
            labels.append(t[0])
            rows.append(np.asarray(t[1:], np.float32))
    X = np.vstack(rows) if rows else np.zeros((0, int(head[1])), np.float32)
    return labels, X


def order(seed, shuffle, n):
    """The law's permutation of [0, n) for (seed, shuffle index)."""
    o = np.empty(n, np.int64)
    C.check(C.lib().gw_ovr_order(seed, shuffle, n, C.ptr(o)), ovr=True)
    return o


def training_size(train_percent, n):
    """classify.py:212: int(train_percent * X.shape[0]) in Python floats (0.30000000000000004 * n and its like)."""
    return int(train_percent * n)


def f1_from_counts(counts):
    """counts int64 [L][3] = tp, fp, fn -> {'micro', 'macro', 'macro_present'} as sklearn's f1_score gives them
    (macro over all L columns; macro_present over the labels with a true or predicted row)."""
    c = np.asarray(counts, np.int64).reshape(-1, 3)
    tp, fp, fn = c[:, 0], c[:, 1], c[:, 2]
    den = 2 * tp + fp + fn
    tot = int(den.sum())
    per = np.where(den > 0, 2.0 * tp / np.maximum(den, 1), 0.0)
    present = den > 0
    return {"micro": 2.0 * int(tp.sum()) / tot if tot else 0.0,
            "macro": float(per.mean()) if len(per) else 0.0,
            "macro_present": float(per[present].mean()) if present.any() else 0.0}


class OneVsRest:
    """Owning handle over a gw_ovr scorer."""

    def __init__(self, n, labels, device=0, **params):
        self.params = C.OvrParams(labels=int(labels), **params)
        self.n, self.L, self.device = int(n), int(labels), int(device)
        h = ctypes.c_void_p()
        C.check(C.lib().gw_ovr_create(self.device, self.n, ctypes.byref(self.params), ctypes.byref(h)), ovr=True)
        self._h = h
        self._keep = []

    @property
    def handle(self):
        return self._h

    def set_features(self, x, pitch=None):
        """x: float32 [n][>= dim], rows contiguous: a torch CUDA tensor (device >= 0; read where it is), a numpy
        array (device = -1; uploaded when device >= 0) or a raw address with `pitch` in floats."""
        if isinstance(x, int):
            p = ctypes.c_void_p(x)
        else:
            if isinstance(x, np.ndarray):
                x = np.ascontiguousarray(x, np.float32)
                if self.device >= 0:
                    x = torch.as_tensor(x, device=f"cuda:{self.device}")
            elif x.dtype != torch.float32 or x.dim() != 2 or x.stride(1) != 1:
                raise ValueError("features tensor must be float32 [n][dim] with contiguous rows")
            if x.shape[0] != self.n or x.shape[1] < self.params.dim:
                raise ValueError(f"features must be [{self.n}][>= {self.params.dim}]")
            pitch = x.stride(0) if hasattr(x, "stride") else x.strides[0] // 4
            p = C.ptr(x)
            self._keep = [x]
        C.check(C.lib().gw_ovr_set_features(self._h, p, int(pitch)), ovr=self._h)

    def set_labels(self, row_off, ids):
        row_off = np.ascontiguousarray(row_off, np.int64)
        ids = np.ascontiguousarray(ids, np.int32)
        if len(row_off) != self.n + 1:
            raise ValueError(f"row_off must have {self.n + 1} entries")
        C.check(C.lib().gw_ovr_set_labels(self._h, C.ptr(row_off), C.ptr(ids)), ovr=self._h)

    def _stream(self, stream):
        if stream is None and self.device >= 0 and torch is not None:
            stream = ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        return stream

    def fit(self, order, train_count, stream=None):
        order = np.ascontiguousarray(order, np.int64)
        if train_count > len(order):
            raise ValueError("train_count exceeds the order's length")
        st = C.OvrStats()
        C.check(C.lib().gw_ovr_fit(self._h, C.ptr(order), int(train_count), ctypes.byref(st), self._stream(stream)),
                ovr=self._h)
        return st

    def score(self, rows, stream=None):
        """tp, fp, fn per label (int64 [L][3]) of the top-k prediction of `rows`."""
        rows = np.ascontiguousarray(rows, np.int64)
        counts = np.zeros((self.L, 3), np.int64)
        C.check(C.lib().gw_ovr_score(self._h, C.ptr(rows), len(rows), C.ptr(counts), self._stream(stream)),
                ovr=self._h)
        return counts

    def decision(self, rows):
        rows = np.ascontiguousarray(rows, np.int64)
        z = np.empty((len(rows), self.L), np.float64)
        C.check(C.lib().gw_ovr_decision(self._h, C.ptr(rows), len(rows), C.ptr(z)), ovr=self._h)
        return z

    def export(self):
        """{'W': float64 [L][dim + 1] (bias last), 'state', 'newton_iters', 'gnorm'}."""
        W = np.empty((self.L, self.params.dim + 1), np.float64)
        st = np.empty(self.L, np.int32)
        it = np.empty(self.L, np.int32)
        gn = np.empty(self.L, np.float64)
        C.check(C.lib().gw_ovr_export(self._h, C.ptr(W), C.ptr(st), C.ptr(it), C.ptr(gn)), ovr=self._h)
        return {"W": W, "state": st, "newton_iters": it, "gnorm": gn}

    def kernel_attrs(self):
        """{kernel name: {'vgprs', 'scratch_bytes', 'lds_bytes'}} (hipFuncGetAttributes)."""
        cap = 16
        names = (ctypes.c_char_p * cap)()
        v, s, l = ((ctypes.c_int32 * cap)() for _ in range(3))
        n = ctypes.c_int32()
        C.check(C.lib().gw_ovr_kernel_attrs(self._h, cap, names, v, s, l, ctypes.byref(n)), ovr=self._h)
        return {names[i].decode(): {"vgprs": v[i], "scratch_bytes": s[i], "lds_bytes": l[i]}
                for i in range(min(n.value, cap))}

    def free(self):
        if getattr(self, "_h", None):
            C.lib().gw_ovr_free(self._h)
            self._h = None
            self._keep = []

    def __del__(self):
        try:
            self.free()
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass


def _features_of(features, device):
    """(what set_features takes, n, dim, row labels or None, device) of a tensor, an array, an Embedding (gwamd.embed)
    or a DeepSim trainer (gwamd.deepsim)."""
    if hasattr(features, "model") and hasattr(features, "vectors"):  # Embedding
        labels = features.labels
        if device >= 0 and features.model.device >= 0:
            x = features.model.vectors_torch()
            return x, x.shape[0], x.shape[1], labels, features.model.device
        return np.asarray(features.vectors, np.float32), len(labels), features.vectors.shape[1], labels, device
    if hasattr(features, "vectors_torch") and hasattr(features, "export"):  # DeepSim
        if features.device >= 0 and device >= 0:
            x = features.vectors_torch()
            return x, x.shape[0], x.shape[1], None, features.device
        w1 = features.export(states=False)["w1"]
        return w1, w1.shape[0], w1.shape[1], None, device
    if torch is not None and isinstance(features, torch.Tensor):
        if features.is_cuda:
            device = features.device.index if features.device.index is not None else torch.cuda.current_device()
        else:
            features = features.numpy()
    return features, features.shape[0], features.shape[1], None, device


def scoring(features, groups, training_percents=numpy.asarray(range(1, 10)) * .1, number_shuffles=3, seed=0,
            device=0, orders=None, file=None, **params):
    """classify.scoring.  `groups`: read_groups' dict, or a pair (row_off, ids) in feature-row order.  With a dict
    the feature rows are matched by label: an Embedding brings its own, any other input has row i = the i-th node
    of the dict in numeric order.  `orders`: one permutation of the rows per shuffle (default: the law's, from
    `seed`).  Returns {percent: [{'micro', 'macro', 'macro_present'}, ...]} and prints the reference's table
    (classify.py:247-253)."""
    x, n, dim, row_labels, device = _features_of(features, device)
    if isinstance(groups, dict):
        _, names, row_off, ids = groups_csr(groups, row_labels)
    else:
        row_off, ids = groups
        names = range(int(np.max(ids)) + 1 if len(ids) else 1)
    if len(row_off) != n + 1:
        raise ValueError(f"{len(row_off) - 1} label rows for {n} feature rows")
    m = OneVsRest(n, len(names), device=device, dim=dim, seed=seed, **params)
    m.set_features(x)
    m.set_labels(row_off, ids)
    if orders is None:
        orders = [order(seed, s, n) for s in range(number_shuffles)]
    all_results = {}
    for train_percent in training_percents:
        for o in orders:
            o = np.ascontiguousarray(o, np.int64)
            size = training_size(train_percent, n)
            st = m.fit(o, size)
            if st.not_converged:
                print(f"warning: {st.not_converged} labels did not converge", file=sys.stderr)
            results = f1_from_counts(m.score(o[size:]))
            for average in ("micro", "macro"):
                print(results[average], file=file)
            all_results.setdefault(train_percent, []).append(results)
    print("Results, using embeddings of dimensionality", dim, file=file)
    print("-------------------", file=file)
    for train_percent in sorted(all_results.keys()):
        print("Train percent:", train_percent, file=file)
        for r in all_results[train_percent]:
            print({"micro": r["micro"], "macro": r["macro"]}, file=file)
        print("-------------------", file=file)
    m.free()
    return all_results


def cli(argv=None):
    ap = argparse.ArgumentParser(description="Score embeddings by one-vs-rest logistic regression F1 on MI355X.")
    ap.add_argument("--emb", required=True, help="embeddings (word2vec text / save_embeddings format)")
    ap.add_argument("--groups", required=True, help="lines `node,label`")
    ap.add_argument("--shuffles", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args(argv)
    labels, X = read_embedding(args.emb)
    groups = read_groups(args.groups)
    _, _, row_off, ids = groups_csr(groups, labels)
    scoring(X, (row_off, ids), number_shuffles=args.shuffles, seed=args.seed, device=args.device)
    return 0


if __name__ == "__main__":
    sys.exit(cli())
