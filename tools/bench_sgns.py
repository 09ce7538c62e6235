"""SGNS trainer throughput on one MI355X, beside a plain torch baseline.

    timeout -k 10 900 python tools/bench_sgns.py [--scale 20] [--reps 3] [--out profiles/sgns/bench_sgns.json]

Workload: one epoch of gw_sgns_train on R-MAT-<scale> (edge factor 16,
gw_graph_rmat), 1 walk per vertex of length 80 from gw_n2v_walks (kept in
HBM), dim 128, window 10, 5 negatives, auto concurrency.  Each repetition
trains a fresh handle from the same initial state; a small warm-up call on
another handle loads the kernel first.  Time = host clock around
gw_sgns_train, which synchronises its stream.

Baseline ("what a user would do today"): a batched SGNS step in torch-ROCm
on the same GPU over the same number of pairs - gather the input rows and
the 1 + 5 target rows, bmm, sigmoid, and index_add_ of both updates.  Its
pairs are random indices (it is a rate baseline, not the same model).

Prints one JSON line (and writes it to --out).  Accounted bytes = rows read
and written x dim x 4: per pair one syn0 row read and written, per target
one syn1neg row read, and written unless the target was clipped.
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graph-embedding_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--walk-length", type=int, default=80)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--window", type=int, default=10)
    ap.add_argument("--negative", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--concurrency", type=int, default=0)
    ap.add_argument("--torch-batch", type=int, default=1 << 18)
    ap.add_argument("--skip-torch", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    import gwamd
    from gwamd import _lib as C
    from gwamd.embed import SGNS
    if not torch.cuda.is_available():
        raise SystemExit("bench_sgns.py needs a GPU (there is no CPU fallback for a rate)")
    g = gwamd.GWGraph.rmat(a.scale, 16).to_device(0)
    C.check(C.lib().gw_n2v_prepare(g.handle, 1.0, 1.0, C.N2V_REJECTION), g.handle)
    n, L = g.n, a.walk_length
    W = torch.empty((n, L), dtype=torch.int32, device="cuda:0")
    C.check(C.lib().gw_n2v_walks(g.handle, L, 1, 0, n, 1, C.ptr(W), None, None, None), g.handle)
    torch.cuda.synchronize()
    wp = ctypes.c_void_p(W.data_ptr())
    kw = dict(dim=a.dim, window=a.window, negative=a.negative, epochs=1, seed=1)

    warm = SGNS(n, device=0, **kw)
    warm.build_vocab(wp, min(n, 4096), L)
    warm.train(wp, min(n, 4096), L, 0, 1, a.concurrency)
    attrs = warm.kernel_attrs(L)
    warm.free()

    times, st = [], None
    for _ in range(a.reps):
        m = SGNS(n, device=0, **kw)
        m.build_vocab(wp, n, L)
        conc = a.concurrency or m.auto_concurrency(n)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s = m.train(wp, n, L, 0, 1, a.concurrency)
        times.append(time.perf_counter() - t0)
        st = s.as_tuple()
        m.free()
    times.sort()
    t = times[len(times) // 2]
    kept, pairs, negs, negc, clipped = st
    targets = pairs + negs - negc
    rows_read, rows_written = pairs + targets, pairs + targets - clipped
    nbytes = (rows_read + rows_written) * a.dim * 4
    res = {"workload": f"rmat{a.scale}_ef16_1x{L}_dim{a.dim}_w{a.window}_K{a.negative}_1epoch", "n": n,
           "tokens_kept": kept, "pairs": pairs, "targets": targets, "clipped": clipped, "concurrency": conc,
           "train_s": round(t, 4), "train_s_min_max": [round(times[0], 4), round(times[-1], 4)],
           "pairs_per_s": round(pairs / t), "row_updates_per_s": round(rows_written / t),
           "accounted_bytes": nbytes, "accounted_GBps": round(nbytes / t / 1e9, 1), "kernel_attrs": attrs}

    if not a.skip_torch:
        dev = torch.device("cuda:0")
        B, K, dim = a.torch_batch, a.negative, a.dim
        syn0 = (torch.rand((n, dim), device=dev) - 0.5) / dim
        syn1 = torch.zeros((n, dim), device=dev)
        label = torch.zeros((1, K + 1), device=dev)
        label[0, 0] = 1.0
        gen = torch.Generator(device=dev)
        gen.manual_seed(1)

        def step():
            src = torch.randint(n, (B,), device=dev, generator=gen)
            tgt = torch.randint(n, (B, K + 1), device=dev, generator=gen)
            l1 = syn0[src]                                              # gather [B][dim]
            r = syn1[tgt.view(-1)].view(B, K + 1, dim)                  # gather [B][K+1][dim]
            f = torch.bmm(r, l1.unsqueeze(2)).squeeze(2)                # [B][K+1]
            gg = (label - torch.sigmoid(f)) * 0.025
            neu = torch.bmm(gg.unsqueeze(1), r).squeeze(1)              # [B][dim]
            syn1.index_add_(0, tgt.view(-1), (gg.unsqueeze(2) * l1.unsqueeze(1)).view(-1, dim))
            syn0.index_add_(0, src, neu)

        for _ in range(3):
            step()
        torch.cuda.synchronize()
        steps = max(1, (pairs + B - 1) // B)
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        torch.cuda.synchronize()
        tt = time.perf_counter() - t0
        res.update({"torch_batch": B, "torch_pairs": steps * B, "torch_s": round(tt, 4),
                    "torch_pairs_per_s": round(steps * B / tt),
                    "hip_over_torch": round((pairs / t) / (steps * B / tt), 2)})
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
