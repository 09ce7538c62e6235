"""SDNE (SDNE/SDNE.py) on the GPU.

The reference trains a four-layer dense autoencoder (TensorFlow 1, Adam, 200,000 steps of 100 rows taken in
order) and returns the second layer's pre-activation of every row as its embedding.  Here the same model trains
in HIP (gw_sdne_* in include/graphwalk.h) on a dense matrix or on sparse rows (a graph's adjacency, top-k SimRank
rows); device=-1 evaluates the same law on the host, bit for bit.  Three options, off by default, turn the
reference's loss into the SDNE paper's loss for graphs: nonzero_weight (beta: an entry with x != 0 weighs beta^2 in
the reconstruction term), first_order (alpha: (alpha / B) * sum a_ij |z2_i - z2_j|^2 over the rows of a batch; the
rows must be a square matrix) and shuffle (a row permutation per epoch instead of batches of consecutive rows).

    python -m gwamd.sdne --input edges.txt --output graph.emb [--units 400,100,300] [--steps 200000]
                         [--beta 5] [--alpha 0.1] [--shuffle]
    python -m gwamd.sdne --simrank x.sim.txt --output x.emb
    python -m gwamd.sdne --rows X.npy --output x.emb
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

TENSORS = ("w1", "b1", "w2", "b2", "w3", "b3", "w4", "b4")


def _ptr8(arrs):
    return (ctypes.c_void_p * 8)(*[None if a is None else a.ctypes.data for a in arrs])


class SdneModel:
    """Owning handle over a gw_sdne trainer.  units = (u0, u1, u2, u3): the row width and the three hidden widths;
    params: batch, learning_rate, beta1, beta2, epsilon, weight_decay, kl_weight, kl_target, seed, nonzero_weight
    (beta), first_order (alpha), shuffle."""

    def __init__(self, units, device=0, **params):
        self.params = C.SdneParams(units=units, **params)
        self.units = tuple(self.params.units)
        self.device = int(device)
        self.N = 0
        h = ctypes.c_void_p()
        C.check(C.lib().gw_sdne_create(self.device, ctypes.byref(self.params), ctypes.byref(h)), sdne=True)
        self._h = h
        self._keep = []  # the caller's dense matrix stays alive with the handle

    @property
    def handle(self):
        return self._h

    @property
    def dim(self):
        return self.units[2]

    def _shapes(self):
        u = self.units
        return [s for l in range(4) for s in ((u[l], u[l + 1]), (u[l + 1],))]

    def set_rows(self, X):
        """A dense float32 [N][u0] matrix: a torch CUDA tensor (device >= 0; read where it is) or a numpy array
        (uploaded when device >= 0)."""
        if isinstance(X, np.ndarray):
            X = np.ascontiguousarray(X, np.float32)
            if self.device >= 0:
                X = torch.as_tensor(X, device=f"cuda:{self.device}")
        elif self.device < 0:
            X = np.ascontiguousarray(X.cpu().numpy(), np.float32)
        elif X.dtype != torch.float32 or X.dim() != 2 or X.stride(1) != 1 or not X.is_cuda:
            raise ValueError("rows tensor must be a float32 CUDA [N][u0] with unit column stride")
        if len(X.shape) != 2 or X.shape[1] != self.units[0]:
            raise ValueError(f"rows must be [N][{self.units[0]}]")
        pitch = X.stride(0) if hasattr(X, "stride") else X.strides[0] // 4
        if self.device >= 0:
            torch.cuda.synchronize(self.device)
        self._keep = [X]
        self.N = 0
        C.check(C.lib().gw_sdne_set_rows_dense(self._h, C.ptr(X), int(X.shape[0]), int(pitch)), sdne=self._h)
        self.N = int(X.shape[0])

    def set_csr(self, offsets, cols, vals=None):
        """Sparse rows (host arrays): offsets int64 [N + 1], cols int32 in [0, u0) and distinct within a row,
        vals float32 or None (= 1)."""
        offsets = np.ascontiguousarray(offsets, np.int64)
        cols = np.ascontiguousarray(cols, np.int32)
        vals = None if vals is None else np.ascontiguousarray(vals, np.float32)
        if offsets.ndim != 1 or len(offsets) < 2 or len(cols) < offsets[-1] or (vals is not None and len(vals) < offsets[-1]):
            raise ValueError("bad CSR arrays")
        self._keep = []
        self.N = 0
        C.check(C.lib().gw_sdne_set_rows_csr(self._h, C.ptr(offsets), C.ptr(cols), C.ptr(vals), len(offsets) - 1),
                sdne=self._h)
        self.N = len(offsets) - 1

    def train(self, step_begin, step_count, stream=None, loss=True):
        """Steps [step_begin, step_begin + step_count); returns each step's loss before its update (float64)."""
        out = np.zeros(step_count, np.float64) if loss else None
        if stream is None and self.device >= 0 and torch is not None:
            stream = ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        C.check(C.lib().gw_sdne_train(self._h, step_begin, step_count, C.ptr(out), stream), sdne=self._h)
        return out

    def gradients(self, step):
        g = [np.empty(s, np.float32) for s in self._shapes()]
        C.check(C.lib().gw_sdne_gradients(self._h, step, _ptr8(g)), sdne=self._h)
        return dict(zip(TENSORS, g))

    def batch_rows(self, step):
        """The input rows step trains on, in slot order (int64 [batch])."""
        out = np.empty(self.params.batch, np.int64)
        C.check(C.lib().gw_sdne_batch_rows(self._h, step, C.ptr(out)), sdne=self._h)
        return out

    def encode(self, row_begin=0, row_count=None):
        """z2 of the current rows [row_begin, +row_count) as float32 [row_count][u2]."""
        if row_count is None:
            row_count = self.N - row_begin
        out = np.empty((row_count, self.dim), np.float32)
        C.check(C.lib().gw_sdne_encode(self._h, row_begin, row_count, C.ptr(out)), sdne=self._h)
        return out

    def export(self, states=True):
        """{'w1', 'b1', .., 'w4', 'b4'} and, with states, {'m': {...}, 'v': {...}} (Adam)."""
        par = [np.empty(s, np.float32) for s in self._shapes()]
        am = [np.empty(s, np.float32) for s in self._shapes()] if states else [None] * 8
        av = [np.empty(s, np.float32) for s in self._shapes()] if states else [None] * 8
        C.check(C.lib().gw_sdne_export(self._h, _ptr8(par), _ptr8(am), _ptr8(av)), sdne=self._h)
        out = dict(zip(TENSORS, par))
        if states:
            out["m"] = dict(zip(TENSORS, am))
            out["v"] = dict(zip(TENSORS, av))
        return out

    def vectors_torch(self):
        """The encoding as a torch view [N][u2] of the trainer's own HBM (no copy); complete after encode() of all
        rows, valid while this handle lives and until its next set_rows / set_csr."""
        if self.device < 0:
            raise ValueError("host evaluation keeps its vectors in host memory (use encode())")
        p = ctypes.c_void_p()
        pitch = ctypes.c_int64()
        C.check(C.lib().gw_sdne_vectors_dev(self._h, ctypes.byref(p), ctypes.byref(pitch)), sdne=self._h)

        class _View:  # the CUDA array interface torch.as_tensor reads
            __cuda_array_interface__ = {"shape": (self.N, pitch.value), "typestr": "<f4", "data": (p.value, False),
                                        "version": 2, "strides": None}
        return torch.as_tensor(_View(), device=f"cuda:{self.device}")[:, :self.dim]

    def kernel_attrs(self):
        """{kernel name: {'vgprs', 'scratch_bytes', 'lds_bytes'}} of the step chain (hipFuncGetAttributes)."""
        cap = 16
        names = (ctypes.c_char_p * cap)()
        v, s, l = ((ctypes.c_int32 * cap)() for _ in range(3))
        n = ctypes.c_int32()
        C.check(C.lib().gw_sdne_kernel_attrs(self._h, cap, names, v, s, l, ctypes.byref(n)), sdne=self._h)
        return {names[i].decode(): {"vgprs": v[i], "scratch_bytes": s[i], "lds_bytes": l[i]}
                for i in range(min(n.value, cap))}

    def free(self):
        if getattr(self, "_h", None):
            C.lib().gw_sdne_free(self._h)
            self._h = None
            self._keep = []

    def __del__(self):
        try:
            self.free()
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass


def SDNE(Xtrain, XCV, Xtest, units=(400, 100, 300), steps=200000, device=0, **params):
    """SDNE.py:66-176: train on Xtrain only, return the encodings (Xtrain_, XCV_, Xtest_) as float32 arrays.
    units: the three hidden widths; params: batch, learning_rate, weight_decay, kl_weight, kl_target, seed, and
    nonzero_weight, first_order (Xtrain square), shuffle.  XCV and Xtest are only encoded."""
    Xtrain = np.ascontiguousarray(Xtrain, np.float32)
    m = SdneModel((Xtrain.shape[1],) + tuple(units), device=device, **params)
    try:
        m.set_rows(Xtrain)
        m.train(0, steps, loss=False)
        out = [m.encode()]
        for X in (XCV, Xtest):
            X = np.ascontiguousarray(X, np.float32)
            if len(X) == 0:
                out.append(np.empty((0, m.dim), np.float32))
                continue
            # a matrix shorter than the batch is padded, the padding dropped; with first_order > 0 the handle takes
            # square matrices only, so the rows go through in pieces of u0 rows, each padded to u0
            piece = X.shape[1] if m.params.first_order > 0 else len(X)
            enc = []
            for r0 in range(0, len(X), piece):
                Xp = X[r0:r0 + piece]
                pad = max(0, (piece if m.params.first_order > 0 else m.params.batch) - len(Xp))
                m.set_rows(np.concatenate([Xp, np.zeros((pad, X.shape[1]), np.float32)]) if pad else Xp)
                enc.append(m.encode(0, len(Xp)))
            out.append(np.concatenate(enc))
    finally:
        m.free()
    return tuple(out)


def csr_from_simrank(simrank, n=None):
    """read_simrank's list of rows of (id, value) strings -> (offsets, cols, vals); a repeated id keeps its first
    value."""
    n = len(simrank) if n is None else n
    offs = np.zeros(n + 1, np.int64)
    cols, vals = [], []
    for v in range(n):
        seen = set()
        for i, s in (simrank[v] if v < len(simrank) else []):
            i = int(i)
            if i not in seen:
                seen.add(i)
                cols.append(i)
                vals.append(float(s))
        offs[v + 1] = len(cols)
    return offs, np.asarray(cols, np.int32), np.asarray(vals, np.float32)


def _has_weights(path, delimiter):
    """True when the edge list's first data line has a third, numeric column."""
    with open(path) as f:
        for line in f:
            t = line.strip()
            if not t or t.startswith("#"):
                continue
            w = t.split(delimiter) if delimiter else t.split()
            try:
                return len(w) >= 3 and float(w[2]) == float(w[2])
            except ValueError:
                return False
    return False


def cli(argv=None):
    ap = argparse.ArgumentParser(description="SDNE of a graph's adjacency, of SimRank rows or of a dense matrix on MI355X.")
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--input", default=None, help="an edge list: the rows are the graph's adjacency (weights if present)")
    src.add_argument("--simrank", default=None, help="a .sim.txt: the rows are its top-k rows")
    src.add_argument("--rows", default=None, help="a .npy dense matrix")
    ap.add_argument("--delimiter", default=None)
    ap.add_argument("--weighted", action="store_true", help="the edge list's third column holds weights (also "
                                                            "detected from its first line)")
    ap.add_argument("--output", required=True, help="embeddings in deepsim.save_embeddings' text: `<rows> <dim>`, then "
                                                    "`<row> v ... v`; for --input row r is the r-th node in ascending "
                                                    "label order")
    ap.add_argument("--units", default="400,100,300", help="the three hidden widths; the second is the dimension")
    ap.add_argument("--batch", type=int, default=100)
    ap.add_argument("--steps", type=int, default=200000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--beta", type=float, default=1.0, help="weight of the nonzero entries in the reconstruction "
                                                            "term (squared); the SDNE paper uses values above 1")
    ap.add_argument("--alpha", type=float, default=0.0, help="weight of the first-order proximity term; needs square "
                                                             "rows (--input always is)")
    ap.add_argument("--shuffle", action="store_true", help="a row permutation per epoch instead of ordered batches")
    ap.add_argument("--groups", default=None, help="lines `node,label`: print classify.scoring's table")
    ap.add_argument("--neighbors", default=None, help="write the top-20 cosine neighbours there")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args(argv)
    hidden = tuple(int(t) for t in args.units.split(","))
    if len(hidden) != 3:
        raise SystemExit("--units takes three widths")
    labels = None
    opts = dict(device=args.device, batch=args.batch, seed=args.seed, nonzero_weight=args.beta,
                first_order=args.alpha, shuffle=int(args.shuffle))
    if args.input:
        from .graph import GWGraph
        weighted = args.weighted or _has_weights(args.input, args.delimiter)
        csr = GWGraph.from_edgelist(args.input, args.delimiter, "nx", False, weighted).export_csr()
        labels = [int(l) for l in csr["labels"]]
        n = len(csr["offsets"]) - 1
        m = SdneModel((n,) + hidden, **opts)
        m.set_csr(csr["offsets"], csr["nbrs"], csr["weights"] if weighted else None)
    elif args.simrank:
        from . import io
        offs, cols, vals = csr_from_simrank(io.read_simrank(args.simrank))
        n = len(offs) - 1
        m = SdneModel((max(n, int(cols.max()) + 1 if len(cols) else 1),) + hidden, **opts)
        m.set_csr(offs, cols, vals)
    else:
        X = np.load(args.rows)
        n = len(X)
        m = SdneModel((X.shape[1],) + hidden, **opts)
        m.set_rows(X)
    m.train(0, args.steps, loss=False)
    emb = m.encode()
    from . import deepsim
    deepsim.save_embeddings(args.output, emb)
    print(f"{n} x {m.dim} embeddings -> {args.output}", file=sys.stderr)
    vec = m.vectors_torch() if args.device >= 0 else emb  # scored and searched where it lies in HBM
    rows = labels if labels is not None else range(n)
    if args.groups:
        from . import classify
        _, _, row_off, ids = classify.groups_csr(classify.read_groups(args.groups), rows)
        classify.scoring(vec, (row_off, ids), seed=args.seed, device=args.device)
    if args.neighbors:
        from . import neighbors
        neighbors.neighbors_of(vec, args.neighbors, rows, device=args.device, groups=args.groups)
    m.free()
    return 0


if __name__ == "__main__":
    sys.exit(cli())
