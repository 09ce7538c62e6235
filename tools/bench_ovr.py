"""One-vs-rest scoring on one MI355X, beside sklearn's liblinear on the host.

    timeout -k 10 1100 python tools/bench_ovr.py [--out profiles/ovr/bench.json] [--skip-rmat] [--skip-e2e]

Three measurements, each a classify.scoring schedule (training shares
0.1 .. 0.9, 3 shuffles = 27 fits, each followed by the top-k scoring of the
held-out rows), timed split by split with the host clock around fit + score
(both synchronise their stream):

  blog    BlogCatalog's shape and labels (tests/golden/data/blog_groups.csv:
          10,312 rows, 39 labels), planted features of dim 128;
  rmat    the R-MAT-20 corpus' shape (646,323 rows, dim 128), 39 synthetic
          labels, planted features generated on the GPU;
  e2e     tests/golden/data/blog.txt -> gw_n2v_walks (p = q = 1, 10 walks of 80
          per vertex) -> SGNS (dim 128, window 10, 1 epoch: the defaults of
          node2vec/src/main.py) -> scoring of the vectors where they lie.

Baseline: sklearn's OneVsRestClassifier(LogisticRegression(solver=
'liblinear'), n_jobs=--jobs) on the same rows, features copied to the host,
the top-k rule and the counts in numpy.  On `rmat` the baseline runs only the
splits named by --rmat-sk-splits (default: the first 0.1 split) and is
compared with the GPU's time for the same splits.

Prints one JSON line (and writes it to --out).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graph-embedding_amd"))
DATA = os.path.join(ROOT, "tests", "golden", "data")
PERCENTS = np.asarray(range(1, 10)) * .1


def splits(K, n, shuffles, seed):
    orders = [K.order(seed, s, n) for s in range(shuffles)]
    return [(p, o) for p in PERCENTS for o in orders]


def gpu_scoring(K, x, row_off, ids, L, sp, device=0):
    """[(seconds, passes, micro, macro)] per split."""
    import torch
    n = len(row_off) - 1
    m = K.OneVsRest(n, L, device=device, dim=x.shape[1])
    m.set_features(x)
    m.set_labels(row_off, ids)
    m.fit(sp[0][1], min(n, 256))  # warm-up: loads the kernels; the timed fits still size their own buffers
    out = []
    for p, o in sp:
        T = K.training_size(p, n)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        st = m.fit(o, T)
        counts = m.score(o[T:])
        dt = time.perf_counter() - t0
        f = K.f1_from_counts(counts)
        out.append((dt, st.passes, f["micro"], f["macro"], st.not_converged))
    attrs = m.kernel_attrs()
    m.free()
    return out, attrs


def sk_scoring(K, X, Y, sp, jobs):
    from sklearn.linear_model import LogisticRegression
    from sklearn.multiclass import OneVsRestClassifier
    n, L = Y.shape
    out = []
    for p, o in sp:
        T = K.training_size(p, n)
        tr, te = o[:T], o[T:]
        t0 = time.perf_counter()
        clf = OneVsRestClassifier(LogisticRegression(solver="liblinear"), n_jobs=jobs).fit(X[tr], Y[tr])
        Z = np.empty((len(te), L))
        for c, est in enumerate(clf.estimators_):
            Z[:, c] = est.decision_function(X[te]) if hasattr(est, "coef_") else (np.inf if Y[tr, c].all() else -np.inf)
        k = Y[te].sum(1)
        rank = np.argsort(np.argsort(-Z, axis=1, kind="stable"), axis=1, kind="stable")
        P = rank < k[:, None]   # ties: a timing baseline, not the law's tie rule
        counts = np.stack([(P & Y[te]).sum(0), (P & ~Y[te]).sum(0), (~P & Y[te]).sum(0)], 1)
        dt = time.perf_counter() - t0
        f = K.f1_from_counts(counts)
        out.append((dt, 0, f["micro"], f["macro"], 0))
    return out


def summary(rows):
    t = [r[0] for r in rows]
    return {"splits": len(rows), "total_s": round(sum(t), 3), "per_split_s_min_max": [round(min(t), 4), round(max(t), 4)],
            "passes": int(sum(r[1] for r in rows)), "not_converged": int(sum(r[4] for r in rows)),
            "micro_first_last_split": [round(rows[0][2], 4), round(rows[-1][2], 4)]}


def indicator(row_off, ids, L):
    n = len(row_off) - 1
    Y = np.zeros((n, L), bool)
    Y[np.repeat(np.arange(n), np.diff(row_off)), ids] = True
    return Y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shuffles", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--jobs", type=int, default=16)
    ap.add_argument("--rmat-n", type=int, default=646323)
    ap.add_argument("--rmat-sk-splits", type=int, default=1)
    ap.add_argument("--skip-rmat", action="store_true")
    ap.add_argument("--skip-e2e", action="store_true")
    ap.add_argument("--skip-sklearn", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    import gwamd
    from gwamd import _lib as C
    from gwamd import classify as K
    if not torch.cuda.is_available():
        raise SystemExit("bench_ovr.py needs a GPU (there is no CPU fallback for a rate)")
    res = {"shuffles": a.shuffles, "sklearn_jobs": a.jobs}

    groups = K.read_groups(os.path.join(DATA, "blog_groups.csv"))
    _, names, row_off, ids = K.groups_csr(groups)
    n, L, d = len(row_off) - 1, len(names), 128
    Y = indicator(row_off, ids, L)
    rs = np.random.RandomState(a.seed)
    X = ((Y @ rs.randn(L, d)) / np.sqrt(np.maximum(Y.sum(1, keepdims=True), 1)) + 0.5 * rs.randn(n, d)).astype(np.float32)
    sp = splits(K, n, a.shuffles, a.seed)
    g, attrs = gpu_scoring(K, torch.as_tensor(X, device="cuda:0"), row_off, ids, L, sp)
    res["kernel_attrs"] = attrs
    res["blog"] = {"n": n, "dim": d, "labels": L, "gpu": summary(g)}
    print("blog gpu", res["blog"]["gpu"], file=sys.stderr, flush=True)
    if not a.skip_sklearn:
        s = sk_scoring(K, X.astype(np.float64), Y, sp, a.jobs)
        res["blog"]["sklearn"] = summary(s)
        res["blog"]["sklearn_over_gpu"] = round(sum(r[0] for r in s) / sum(r[0] for r in g), 2)
        res["blog"]["max_abs_micro_difference"] = float(max(abs(x[2] - y[2]) for x, y in zip(g, s)))
        print("blog sklearn", res["blog"]["sklearn"], file=sys.stderr, flush=True)

    if not a.skip_e2e:
        from gwamd.embed import learn_embeddings
        t0 = time.perf_counter()
        gr = gwamd.GWGraph.from_edgelist(os.path.join(DATA, "blog.txt"), ",", "nx", False, False)
        gr.to_device(0)
        C.check(C.lib().gw_n2v_prepare(gr.handle, 1.0, 1.0, C.N2V_AUTO), gr.handle)
        nw, wl = 10 * gr.n, 80
        W = torch.empty((nw, wl), dtype=torch.int32, device="cuda:0")
        C.check(C.lib().gw_n2v_walks(gr.handle, wl, a.seed, 0, nw, 1, C.ptr(W), None, None, None), gr.handle)
        torch.cuda.synchronize()
        t_walks = time.perf_counter() - t0
        t0 = time.perf_counter()
        emb = learn_embeddings(W, gr, dimensions=128, window_size=10, iter=1, seed=a.seed, device=0)
        t_sgns = time.perf_counter() - t0
        _, _, ro, ii = K.groups_csr(groups, emb.labels)
        sp = splits(K, gr.n, a.shuffles, a.seed)
        g, _ = gpu_scoring(K, emb.model.vectors_torch(), ro, ii, L, sp)
        e2e = {"n": gr.n, "graph_and_walks_s": round(t_walks, 3), "sgns_s": round(t_sgns, 3), "gpu": summary(g),
               "gpu_micro_by_share": [round(float(np.mean([r[2] for r in g[i * a.shuffles:(i + 1) * a.shuffles]])), 4)
                                      for i in range(9)],
               "gpu_macro_by_share": [round(float(np.mean([r[3] for r in g[i * a.shuffles:(i + 1) * a.shuffles]])), 4)
                                      for i in range(9)]}
        if not a.skip_sklearn:
            s = sk_scoring(K, emb.vectors.astype(np.float64), indicator(ro, ii, L), sp, a.jobs)
            e2e["sklearn"] = summary(s)
            e2e["sklearn_micro_by_share"] = [round(float(np.mean([r[2] for r in s[i * a.shuffles:(i + 1) * a.shuffles]])), 4)
                                             for i in range(9)]
            e2e["sklearn_macro_by_share"] = [round(float(np.mean([r[3] for r in s[i * a.shuffles:(i + 1) * a.shuffles]])), 4)
                                             for i in range(9)]
            e2e["sklearn_over_gpu"] = round(sum(r[0] for r in s) / sum(r[0] for r in g), 2)
        res["e2e"] = e2e
        print("e2e", e2e, file=sys.stderr, flush=True)

    if not a.skip_rmat:
        n = a.rmat_n
        gen = torch.Generator(device="cuda:0")
        gen.manual_seed(a.seed)
        lab = torch.randint(L, (n,), device="cuda:0", generator=gen)
        Yd = torch.rand((n, L), device="cuda:0", generator=gen) < 0.01
        Yd[torch.arange(n, device="cuda:0"), lab] = True
        cen = torch.randn((L, d), device="cuda:0", generator=gen)
        x = (Yd.float() @ cen) / Yd.sum(1, keepdim=True).float().sqrt() + torch.randn((n, d), device="cuda:0", generator=gen)
        Y = Yd.cpu().numpy()
        row_off = np.concatenate([[0], np.cumsum(Y.sum(1))]).astype(np.int64)
        ids = np.nonzero(Y)[1].astype(np.int32)
        sp = splits(K, n, a.shuffles, a.seed)
        g, _ = gpu_scoring(K, x.contiguous(), row_off, ids, L, sp)
        res["rmat"] = {"n": n, "dim": d, "labels": L, "gpu": summary(g)}
        print("rmat gpu", res["rmat"]["gpu"], file=sys.stderr, flush=True)
        if not a.skip_sklearn and a.rmat_sk_splits > 0:
            sub = sp[:a.rmat_sk_splits]
            s = sk_scoring(K, x.cpu().numpy().astype(np.float64), Y, sub, a.jobs)
            res["rmat"]["sklearn_first_splits"] = summary(s)
            res["rmat"]["gpu_same_splits_s"] = round(sum(r[0] for r in g[:len(sub)]), 3)
            res["rmat"]["sklearn_over_gpu_same_splits"] = round(sum(r[0] for r in s) / sum(r[0] for r in g[:len(sub)]), 2)

    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
