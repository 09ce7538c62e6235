"""DeepSim training rate on blog's shape, beside an eager torch step.

    python tools/bench_deepsim.py [--steps 300] [--warmup 30] [--out profiles/deepsim/bench.json]

V = 10313, B = 128, d = 128, k = 10, a synthetic top-20 table and 2000
synthetic walks of 80.  Three child processes, each under its own `timeout`:
  gw      steps/s of gw_deepsim_train (one call of --steps steps, wall clock);
  torch   steps/s of the same model and Adam formula written in eager torch
          ops on the same GPU, fed the same batches (built beforehand);
  trace   the gw run under `rocprofv3 --kernel-trace`: each kernel's share of
          a step (left out, and reported as not measured, without rocprofv3).
Reports what is measured; no ratio is expected or asserted.
"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graph-embedding_amd"))

V, B, D, K, TOPK, NWALKS, L = 10313, 128, 128, 10, 20, 2000, 80


def problem():
    import numpy as np
    rng = np.random.RandomState(0)
    ids = rng.randint(0, V, (V, TOPK)).astype(np.int32)
    sc = np.sort(rng.uniform(1e-3, 0.2, (V, TOPK)), axis=1)[:, ::-1].copy()
    W = rng.randint(0, V, (NWALKS, L)).astype(np.int32)
    for i in range(1, L):   # walks follow the table, so that lookups hit
        W[:, i] = np.where(rng.rand(NWALKS) < 0.7, ids[W[:, i - 1], rng.randint(0, TOPK, NWALKS)], W[:, i])
    return ids, sc, W


def make_trainer():
    from gwamd.deepsim import DeepSim
    ids, sc, W = problem()
    m = DeepSim(V, device=0, dim=D, window=K, batch=B, seed=1)
    m.set_simrank(ids, sc)
    m.set_walks(W)
    return m


def child_gw(steps, warmup):
    import torch
    m = make_trainer()
    m.train(0, warmup, loss=False)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    m.train(warmup, steps, loss=False)   # synchronises its stream
    dt = time.perf_counter() - t0
    loss = m.train(warmup + steps, 1)
    print(json.dumps({"steps": steps, "seconds": dt, "steps_per_s": steps / dt, "ms_per_step": 1e3 * dt / steps,
                      "loss_after": float(loss[0]), "kernel_attrs": m.kernel_attrs()}))


def child_torch(steps, warmup):
    import numpy as np
    import torch
    m = make_trainer()
    dev = torch.device("cuda:0")
    P0 = m.export(states=False)
    P = {t: torch.tensor(P0[t], device=dev) for t in P0}
    Ms = {t: torch.zeros_like(P[t]) for t in P}
    Vs = {t: torch.zeros_like(P[t]) for t in P}
    batches = []
    for t in range(warmup + steps):   # the batches are built beforehand: only the model step is timed
        b = m.batch(t)
        n = b["tgt_n"]
        rows = np.repeat(np.arange(B), n)
        mask = np.arange(b["tgt_id"].shape[1])[None, :] < n[:, None]
        batches.append((torch.tensor(b["centre"].astype(np.int64), device=dev),
                        torch.tensor(rows, device=dev), torch.tensor(b["tgt_id"][mask].astype(np.int64), device=dev),
                        torch.tensor(b["tgt_val"][mask], device=dev)))

    def step(t, c, rows, cols, vals):
        Y = torch.zeros((B, V), device=dev)
        Y[rows, cols] = vals
        pre = P["w1"][c] + P["b1"]
        hid = torch.relu(pre)
        lg = hid @ P["w2"] + P["b2"]
        p = torch.softmax(lg, 1)
        dl = (p * Y.sum(1, keepdim=True) - Y) / B
        dh = (dl @ P["w2"].T) * (pre > 0)
        g = {"w2": hid.T @ dl, "b2": dl.sum(0), "b1": dh.sum(0),
             "w1": torch.zeros_like(P["w1"]).index_add_(0, c, dh)}
        lr_t = 0.001 * (1.0 - 0.999 ** t) ** 0.5 / (1.0 - 0.9 ** t)
        for n_ in g:
            Ms[n_].mul_(0.9).add_(g[n_], alpha=0.1)
            Vs[n_].mul_(0.999).addcmul_(g[n_], g[n_], value=0.001)
            P[n_].addcdiv_(Ms[n_], Vs[n_].sqrt().add_(1e-8), value=-lr_t)

    for t in range(warmup):
        step(t + 1, *batches[t])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in range(warmup, warmup + steps):
        step(t + 1, *batches[t])
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(json.dumps({"steps": steps, "seconds": dt, "steps_per_s": steps / dt, "ms_per_step": 1e3 * dt / steps,
                      "torch": torch.__version__}))


def run_child(kind, steps, warmup, limit, prefix=()):
    cmd = ["timeout", "-k", "10", str(limit)] + list(prefix) + [sys.executable, os.path.abspath(__file__), "--child",
                                                                  kind, "--steps", str(steps), "--warmup", str(warmup)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        return {"error": f"exit {r.returncode}", "stderr": r.stderr[-1500:]}
    for line in reversed(r.stdout.splitlines()):
        if line.startswith("{"):
            return json.loads(line)
    return {"error": "no result line", "stdout": r.stdout[-1500:]}


def kernel_shares(steps, warmup, limit):
    if shutil.which("rocprofv3") is None:
        return {"not_measured": "rocprofv3 not found"}
    d = tempfile.mkdtemp(prefix="ds_kt_")
    try:
        res = run_child("gw", steps, warmup, limit,
                        prefix=["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "kt", "--"])
        files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        if "error" in res or not files:
            return {"not_measured": res.get("error", "no kernel trace written"), "stderr": res.get("stderr", "")}
        acc = {}
        for r in csv.DictReader(open(files[0])):
            name = r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
            if name.startswith("k_ds_"):
                e = acc.setdefault(name, [0, 0])
                e[0] += 1
                e[1] += int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
        total = sum(e[1] for e in acc.values()) or 1
        return {k: {"calls": e[0], "avg_us": e[1] / e[0] / 1e3, "share": e[1] / total}
                for k, e in sorted(acc.items(), key=lambda x: -x[1][1])}
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--limit", type=int, default=240, help="seconds per timed process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deepsim", "bench.json"))
    ap.add_argument("--child", choices=["gw", "torch"])
    a = ap.parse_args()
    if a.child:
        (child_gw if a.child == "gw" else child_torch)(a.steps, a.warmup)
        return 0
    res = {"shape": {"V": V, "batch": B, "dim": D, "window": K, "topk": TOPK, "nwalks": NWALKS, "walk_len": L},
           "gw_deepsim": run_child("gw", a.steps, a.warmup, a.limit)}
    if "error" in res["gw_deepsim"]:   # nothing more is started on the GPU after a failed step
        print(json.dumps(res))
        return 1
    res["torch_eager"] = run_child("torch", a.steps, a.warmup, a.limit)
    if "error" not in res["torch_eager"]:
        res["kernel_share_of_step"] = kernel_shares(min(a.steps, 60), 5, a.limit)
        res["gw_over_torch_steps_per_s"] = res["gw_deepsim"]["steps_per_s"] / res["torch_eager"]["steps_per_s"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    return 0 if "error" not in res["torch_eager"] else 1


if __name__ == "__main__":
    sys.exit(main())
