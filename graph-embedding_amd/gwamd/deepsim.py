"""DeepSim (DeepSim/src/DeepSim.py) on the GPU.

The reference trains a one-hidden-layer net whose targets are the SimRank
scores of a walk window (TensorFlow 1, Adam) and saves w1 as the embedding.
Here the same model trains in HIP (gw_deepsim_* in include/graphwalk.h) from
the SimRank rows gw_topsim wrote (or a `.sim.txt`) and the walk matrix
gw_n2v_walks wrote; device=-1 evaluates the same law on the host, bit for bit.

    python -m gwamd.deepsim --input edges.txt --simrank_path x.sim.txt \\
        --vertex-num 10313 --emb_output blog.emb [--walks walks.txt]
"""
import argparse
import ctypes
import os
import sys

import numpy as np

from . import _lib as C

try:
    import torch
except Exception:  # pragma: no cover - torch is optional for the host path
    torch = None

TENSORS = ("w1", "b1", "w2", "b2")
FALLBACKS = {"row-min": C.DEEPSIM_FALLBACK_ROW_MIN, "position": C.DEEPSIM_FALLBACK_POSITION}


def _ptr4(arrs):
    return (ctypes.c_void_p * 4)(*[None if a is None else a.ctypes.data for a in arrs])


class DeepSim:
    """Owning handle over a gw_deepsim trainer."""

    def __init__(self, vertex_num, device=0, **params):
        self.params = C.DeepSimParams(vertex_num=int(vertex_num), **params)
        self.V = int(vertex_num)
        self.device = int(device)
        h = ctypes.c_void_p()
        C.check(C.lib().gw_deepsim_create(self.device, ctypes.byref(self.params), ctypes.byref(h)), deepsim=True)
        self._h = h
        self._keep = []  # the caller's walk matrix stays alive with the handle

    @property
    def handle(self):
        return self._h

    @property
    def W(self):
        return 2 * self.params.window + 1

    def _shapes(self):
        d = self.params.dim
        return [(self.V, d), (d,), (d, self.V), (self.V,)]

    def set_simrank(self, ids, scores):
        """ids int32 / scores float64 [V][topk]: torch CUDA tensors (device >= 0) or numpy arrays (device = -1;
        uploaded when device >= 0)."""
        if isinstance(ids, np.ndarray) or isinstance(scores, np.ndarray):
            ids = np.ascontiguousarray(ids, np.int32)
            scores = np.ascontiguousarray(scores, np.float64)
            if self.device >= 0:
                ids = torch.as_tensor(ids, device=f"cuda:{self.device}")
                scores = torch.as_tensor(scores, device=f"cuda:{self.device}")
        elif not (ids.is_contiguous() and scores.is_contiguous() and ids.dtype == torch.int32
                  and scores.dtype == torch.float64):
            raise ValueError("table tensors must be contiguous int32 ids and float64 scores")
        if tuple(ids.shape) != tuple(scores.shape) or len(ids.shape) != 2 or ids.shape[0] != self.V:
            raise ValueError(f"table must be two [{self.V}][topk] arrays")
        C.check(C.lib().gw_deepsim_set_simrank(self._h, C.ptr(ids), C.ptr(scores), int(ids.shape[1])), deepsim=self._h)

    def set_walks(self, walks, labels=None):
        """walks int32 [nwalks][walk_len], -1 padded: a torch CUDA tensor (device >= 0; read where it is) or a
        numpy array (device = -1; uploaded when device >= 0).  labels: token -> vertex index (int64) or None."""
        if isinstance(walks, np.ndarray):
            walks = np.ascontiguousarray(walks, np.int32)
            if self.device >= 0:
                walks = torch.as_tensor(walks, device=f"cuda:{self.device}")
        elif walks.dtype != torch.int32 or not walks.is_contiguous():
            raise ValueError("walks tensor must be a contiguous int32 [nwalks][walk_len]")
        if len(walks.shape) != 2:
            raise ValueError("walks must be [nwalks][walk_len]")
        lab = None if labels is None else np.ascontiguousarray(labels, np.int64)
        self._keep = [walks]
        C.check(C.lib().gw_deepsim_set_walks(self._h, C.ptr(walks), int(walks.shape[0]), int(walks.shape[1]),
                                             C.ptr(lab), 0 if lab is None else len(lab)), deepsim=self._h)

    def train(self, step_begin, step_count, stream=None, loss=True):
        """Steps [step_begin, step_begin + step_count); returns each step's loss before its update (float64)."""
        out = np.zeros(step_count, np.float64) if loss else None
        if stream is None and self.device >= 0 and torch is not None:
            stream = ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        C.check(C.lib().gw_deepsim_train(self._h, step_begin, step_count, C.ptr(out), stream), deepsim=self._h)
        return out

    def gradients(self, step):
        g = [np.empty(s, np.float32) for s in self._shapes()]
        C.check(C.lib().gw_deepsim_gradients(self._h, step, *[C.ptr(a) for a in g]), deepsim=self._h)
        return dict(zip(TENSORS, g))

    def batch(self, step):
        B, W = self.params.batch, self.W
        out = {"centre": np.empty(B, np.int32), "tgt_id": np.empty((B, W), np.int32),
               "tgt_val": np.empty((B, W), np.float32), "tgt_n": np.empty(B, np.int32),
               "ysum": np.empty(B, np.float32)}
        C.check(C.lib().gw_deepsim_batch(self._h, step, *[C.ptr(a) for a in out.values()]), deepsim=self._h)
        return out

    def export(self, states=True):
        """{'w1', 'b1', 'w2', 'b2'} and, with states, {'m': {...}, 'v': {...}} (Adam)."""
        par = [np.empty(s, np.float32) for s in self._shapes()]
        am = [np.empty(s, np.float32) for s in self._shapes()] if states else [None] * 4
        av = [np.empty(s, np.float32) for s in self._shapes()] if states else [None] * 4
        C.check(C.lib().gw_deepsim_export(self._h, _ptr4(par), _ptr4(am), _ptr4(av)), deepsim=self._h)
        out = dict(zip(TENSORS, par))
        if states:
            out["m"] = dict(zip(TENSORS, am))
            out["v"] = dict(zip(TENSORS, av))
        return out

    def vectors_torch(self):
        """w1 as a torch view [V][dim] of the trainer's own HBM (no copy); valid while this handle lives."""
        if self.device < 0:
            raise ValueError("host evaluation keeps its vectors in host memory (use export())")
        p = ctypes.c_void_p()
        pitch = ctypes.c_int64()
        C.check(C.lib().gw_deepsim_vectors_dev(self._h, ctypes.byref(p), ctypes.byref(pitch)), deepsim=self._h)

        class _View:  # the CUDA array interface torch.as_tensor reads
            __cuda_array_interface__ = {"shape": (self.V, pitch.value), "typestr": "<f4", "data": (p.value, False),
                                        "version": 2, "strides": None}
        return torch.as_tensor(_View(), device=f"cuda:{self.device}")[:, :self.params.dim]

    def kernel_attrs(self):
        """{kernel name: {'vgprs', 'scratch_bytes', 'lds_bytes'}} of the step chain (hipFuncGetAttributes)."""
        cap = 16
        names = (ctypes.c_char_p * cap)()
        v, s, l = ((ctypes.c_int32 * cap)() for _ in range(3))
        n = ctypes.c_int32()
        C.check(C.lib().gw_deepsim_kernel_attrs(self._h, cap, names, v, s, l, ctypes.byref(n)), deepsim=self._h)
        return {names[i].decode(): {"vgprs": v[i], "scratch_bytes": s[i], "lds_bytes": l[i]}
                for i in range(min(n.value, cap))}

    def free(self):
        if getattr(self, "_h", None):
            C.lib().gw_deepsim_free(self._h)
            self._h = None
            self._keep = []

    def __del__(self):
        try:
            self.free()
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass


def save_embeddings(path, embeddings):
    """DeepSim.py:344-362 (the header's second number is the row length; the reference writes 128)."""
    e = np.ascontiguousarray(embeddings, np.float32)
    if e.ndim != 2:
        raise ValueError("embeddings must be [n][dim]")
    C.check(C.lib().gw_write_deepsim_text(str(path).encode(), C.ptr(e), e.shape[0], e.shape[1]), deepsim=True)


def table_from_simrank(simrank, vertex_num):
    """read_simrank's list of rows of (id, value) strings -> ids int32 / scores float64 [V][topk], -1 padded."""
    topk = max([len(r) for r in simrank] + [1])
    ids = np.full((vertex_num, topk), -1, np.int32)
    sc = np.zeros((vertex_num, topk), np.float64)
    if len(simrank) > vertex_num:
        raise ValueError(f"{len(simrank)} SimRank rows for vertex_num {vertex_num}")
    for v, row in enumerate(simrank):
        for e, (i, s) in enumerate(row):
            ids[v, e] = int(i)
            sc[v, e] = float(s)
    return ids, sc


def walks_from_list(walks):
    """read_list's list of lists of id strings -> int32 [nwalks][max len], -1 padded."""
    rows = [[int(t) for t in w if str(t).strip() != ""] for w in walks]
    L = max([len(r) for r in rows] + [1])
    W = np.full((len(rows), L), -1, np.int32)
    for i, r in enumerate(rows):
        W[i, :len(r)] = r
    return W


def main(args, simrank, walks, labels=None):
    """DeepSim.main (:386-422).  `simrank`: read_simrank's list, or a pair (ids, scores) of [V][topk] torch CUDA
    tensors / numpy arrays as gw_topsim writes them.  `walks`: a torch int32 CUDA tensor, a numpy array (dense ids
    with `labels`, or vertex indices), or read_list's list of strings.  Reads from args: vertex_num, dimensions,
    window_size, emb_output and, when present, steps, batch, learning_rate, fallback, score_scale, seed, device,
    checkpoint_every.  Returns the trainer (export()['w1'] is what was saved)."""
    device = getattr(args, "device", 0)
    V = int(args.vertex_num)
    fb = getattr(args, "fallback", "row-min")
    m = DeepSim(V, device=device, dim=args.dimensions, window=args.window_size, batch=getattr(args, "batch", 128),
                fallback=FALLBACKS.get(fb, fb), learning_rate=getattr(args, "learning_rate", 0.001),
                score_scale=getattr(args, "score_scale", 1.0), seed=getattr(args, "seed", 0))
    if isinstance(simrank, (tuple, list)) and len(simrank) == 2 and hasattr(simrank[0], "shape"):
        ids, sc = simrank
    else:
        ids, sc = table_from_simrank(simrank, V)
    m.set_simrank(ids, sc)
    if isinstance(walks, list):
        walks = walks_from_list(walks)
    m.set_walks(walks, labels)
    steps = int(getattr(args, "steps", 50000))
    every = int(getattr(args, "checkpoint_every", 1000))
    pos = 0
    while pos < steps:
        # the reference saves emb_output + str(i) after step i whenever i % 1000 == 0 (:182-186)
        if every > 0:
            nxt = pos if pos % every == 0 else (pos // every + 1) * every
            end = min(steps, nxt + 1)
        else:
            nxt, end = -1, steps
        m.train(pos, end - pos, loss=False)
        if nxt >= 0 and end == nxt + 1:
            save_embeddings(args.emb_output + str(nxt), m.export(states=False)["w1"])
        pos = end
    save_embeddings(args.emb_output, m.export(states=False)["w1"])
    return m


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="Run DeepSim on MI355X.")
    ap.add_argument("--input", nargs="?", default="../../data/BlogCatalog-dataset/data/edges.txt")
    ap.add_argument("--simrank_path", nargs="?", default="../output_u_u/SimRank/blog_simrank_navie_top20.txt.sim.txt")
    ap.add_argument("--emb_output", nargs="?", default="../emb/blog.emb")
    ap.add_argument("--groups", default=None, help="lines `node,label` (node = embedding row): score the embedding "
                                                   "where it lies in HBM (main.py:287-289, classify.scoring)")
    ap.add_argument("--neighbors", default=None, help="the 20 nearest neighbours (cosine) of every embedding row, computed "
                                                      "where the embedding lies in HBM (gwamd.neighbors): rows "
                                                      "`v,id,...` and NEIGHBORS.sim.txt with `v,id:score,...`; with "
                                                      "--groups also their label agreement")
    ap.add_argument("--TOPK", default=1000, type=int)
    ap.add_argument("--vertex-num", type=int, default=10313)
    ap.add_argument("--dimensions", type=int, default=128)
    ap.add_argument("--walk-length", type=int, default=80)
    ap.add_argument("--num-walks", type=int, default=10)
    ap.add_argument("--window-size", type=int, default=10)
    ap.add_argument("--iter", default=10, type=int)
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--p", type=float, default=0.25)
    ap.add_argument("--q", type=float, default=0.25)
    ap.add_argument("--delimiter", type=str, default=",")
    ap.add_argument("--weighted", dest="weighted", action="store_true")
    ap.add_argument("--unweighted", dest="unweighted", action="store_false")
    ap.set_defaults(weighted=False)
    ap.add_argument("--directed", dest="directed", action="store_true")
    ap.add_argument("--undirected", dest="undirected", action="store_false")
    ap.set_defaults(directed=False)
    ap.add_argument("--walks", default=None, help="walks file (save_list format); generated on the GPU when it "
                                                  "is not given or does not exist")
    ap.add_argument("--steps", type=int, default=50000)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--learning-rate", type=float, default=0.001)
    ap.add_argument("--fallback", choices=sorted(FALLBACKS), default="row-min")
    ap.add_argument("--score-scale", type=float, default=1.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--checkpoint-every", type=int, default=1000)
    return ap.parse_args(argv)


def _generate_walks(args):
    """node2vec walks of the input graph on the GPU: (int32 CUDA tensor of dense ids, dense id -> label)."""
    from .graph import GWGraph
    g = GWGraph.from_edgelist(args.input, args.delimiter, "nx", args.directed, args.weighted)
    g.to_device(args.device)
    C.check(C.lib().gw_n2v_prepare(g.handle, args.p, args.q, C.N2V_AUTO), g.handle)
    nwalks, L = args.num_walks * g.n, args.walk_length
    W = torch.empty((nwalks, L), dtype=torch.int32, device=f"cuda:{args.device}")
    st = torch.cuda.current_stream(args.device)
    C.check(C.lib().gw_n2v_walks(g.handle, L, args.seed, 0, nwalks, 1, C.ptr(W), None, None,
                                 ctypes.c_void_p(st.cuda_stream)), g.handle)
    torch.cuda.synchronize(args.device)
    return W, np.asarray(g.export_csr()["labels"], np.int64)


def cli(argv=None):
    from . import io
    args = parse_args(argv)
    simrank = io.read_simrank(args.simrank_path)
    labels = None
    if args.walks and os.path.exists(args.walks):
        walks = io.read_list(args.walks)
    else:
        if args.device < 0:
            raise SystemExit("generating the walks needs a GPU: give --walks with --device -1")
        walks, labels = _generate_walks(args)
    m = main(args, simrank, walks, labels)
    print(f"{m.V} x {args.dimensions} embeddings -> {args.emb_output}", file=sys.stderr)
    if args.groups:
        from . import classify
        _, _, row_off, ids = classify.groups_csr(classify.read_groups(args.groups), range(m.V))
        classify.scoring(m, (row_off, ids), seed=args.seed, device=args.device)
    if args.neighbors:
        from . import neighbors
        neighbors.neighbors_of(m, args.neighbors, range(m.V), device=args.device, groups=args.groups)
    return 0


if __name__ == "__main__":
    sys.exit(cli())
