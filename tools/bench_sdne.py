"""SDNE training time per step at the reference's shape and at blog's adjacency shape, beside an eager torch step.

    python tools/bench_sdne.py [--steps 300] [--warmup 30] [--out profiles/sdne/bench.json]
    python tools/bench_sdne.py --trace [--out profiles/sdne/kernels.json]

Shapes: `ref`  units (784, 400, 100, 300, 784), B = 100, 1000 dense rows in device memory;
        `blog` units (10313, 400, 100, 300, 10313), B = 100, 10313 CSR rows of about 65 entries.
Child processes, each under its own `timeout`:
  gw      ms per step of one gw_sdne_train call of --steps steps after a warm-up, the host clock around the
          synchronising call, the median of 5 calls;
  graph   (blog only, its rows being a square matrix) the same gw measurement with the graph loss on
          (nonzero_weight = 5, first_order = 0.1, shuffle), in the same run, beside the default law;
  torch   ms per step of the same model and Adam formula written in eager torch ops on the same GPU, fed batches
          built beforehand, the median of 5;
  --trace one gw run per shape under `rocprofv3 --kernel-trace --stats`: each kernel's share of a step, with the
          registers, scratch and LDS gw_sdne_kernel_attrs reports (a run of its own; not part of the default run).
Also stated per shape: the bytes the two wide layers must move per step (value and both Adam moments of w1 and w4,
read and written) and the fp32 multiply-adds of a step.  Reports what is measured; no ratio is expected or asserted.
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

HIDDEN, B = (400, 100, 300), 100
SHAPES = {"ref": 784, "blog": 10313}
GRAPH = dict(nonzero_weight=5.0, first_order=0.1, shuffle=1)


def make_trainer(shape, graph=False):
    import numpy as np
    from gwamd.sdne import SdneModel
    u0 = SHAPES[shape]
    rng = np.random.RandomState(0)
    m = SdneModel((u0,) + HIDDEN, device=0, batch=B, seed=1, **(GRAPH if graph else {}))
    if shape == "ref":
        X = (rng.uniform(0.2, 1.0, (1000, u0)) * (rng.uniform(size=(1000, u0)) < 0.19)).astype(np.float32)
        m.set_rows(X)
        return m, X
    deg = rng.randint(2, 129, u0)
    offs = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    cols = np.concatenate([np.sort(rng.choice(u0, d, replace=False)) for d in deg]).astype(np.int32)
    m.set_csr(offs, cols)
    return m, (offs, cols)


def counts(shape):
    u = (SHAPES[shape],) + HIDDEN + (SHAPES[shape],)
    weights = sum(u[l] * u[l + 1] for l in range(4))
    wide = u[0] * u[1] + u[3] * u[4]
    # forward 4 products, backward data 3 (none for layer 1), backward weight 4
    fma = B * (2 * weights + sum(u[l] * u[l + 1] for l in range(1, 4)))
    return {"wide_layer_bytes_per_step": wide * 4 * 3 * 2, "all_parameter_bytes_per_step": (weights + sum(u[1:])) * 24,
            "fp32_fma_per_step": fma}


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def child_gw(shape, steps, warmup, graph=False):
    m, _ = make_trainer(shape, graph)
    m.train(0, warmup, loss=False)
    times, pos = [], warmup
    for _ in range(5):
        t0 = time.perf_counter()
        m.train(pos, steps, loss=False)   # synchronises its stream
        times.append(time.perf_counter() - t0)
        pos += steps
    loss = m.train(pos, 1)
    print(json.dumps({"steps": steps, "ms_per_step": 1e3 * median(times) / steps,
                      "ms_per_step_all": [1e3 * t / steps for t in times], "loss_after": float(loss[0]),
                      "kernel_attrs": m.kernel_attrs()}))


def child_torch(shape, steps, warmup):
    import numpy as np
    import torch
    m, rows = make_trainer(shape)
    dev = torch.device("cuda:0")
    u0 = SHAPES[shape]
    names = ("w1", "b1", "w2", "b2", "w3", "b3", "w4", "b4")
    P0 = m.export(states=False)
    P = {t: torch.tensor(P0[t], device=dev) for t in names}
    Ms = {t: torch.zeros_like(P[t]) for t in names}
    Vs = {t: torch.zeros_like(P[t]) for t in names}
    nb = m.N // B
    batches = []
    for i in range(min(nb, warmup + steps)):   # the batches are built beforehand: only the model step is timed
        if shape == "ref":
            x = rows[i * B:(i + 1) * B]
        else:
            offs, cols = rows
            x = np.zeros((B, u0), np.float32)
            for b in range(B):
                x[b, cols[offs[i * B + b]:offs[i * B + b + 1]]] = 1.0
        batches.append(torch.tensor(x, device=dev))

    def step(t, x):
        z1 = x @ P["w1"] + P["b1"]
        h1 = torch.relu(z1)
        z2 = h1 @ P["w2"] + P["b2"]
        h2 = torch.relu(z2)
        z3 = h2 @ P["w3"] + P["b3"]
        h3 = torch.relu(z3)
        y = h3 @ P["w4"] + P["b4"]
        q = h2.mean()
        dy = (y - x) / B
        klg = 0.1 * (-0.005 / (q + 1e-8) + 0.995 / (1.0 - q + 1e-8)) / h2.numel()
        dz3 = (dy @ P["w4"].T) * (z3 > 0)
        dz2 = (dz3 @ P["w3"].T + klg) * (z2 > 0)
        dz1 = (dz2 @ P["w2"].T) * (z1 > 0)
        g = {}
        for l, (a, dz) in enumerate(((x, dz1), (h1, dz2), (h2, dz3), (h3, dy))):
            g[names[2 * l]] = torch.addmm(P[names[2 * l]], a.T, dz, beta=0.1)
            g[names[2 * l + 1]] = dz.sum(0).add_(P[names[2 * l + 1]], alpha=0.1)
        lr_t = 0.01 * (1.0 - 0.999 ** t) ** 0.5 / (1.0 - 0.9 ** t)
        for n_ in names:
            Ms[n_].mul_(0.9).add_(g[n_], alpha=0.1)
            Vs[n_].mul_(0.999).addcmul_(g[n_], g[n_], value=0.001)
            P[n_].addcdiv_(Ms[n_], Vs[n_].sqrt().add_(1e-8), value=-lr_t)

    for t in range(warmup):
        step(t + 1, batches[t % len(batches)])
    times, pos = [], warmup
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for t in range(pos, pos + steps):
            step(t + 1, batches[t % len(batches)])
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
        pos += steps
    print(json.dumps({"steps": steps, "ms_per_step": 1e3 * median(times) / steps,
                      "ms_per_step_all": [1e3 * t / steps for t in times], "torch": torch.__version__}))


def run_child(kind, shape, steps, warmup, limit, prefix=(), graph=False):
    cmd = ["timeout", "-k", "10", str(limit)] + list(prefix) + [
        sys.executable, os.path.abspath(__file__), "--child", kind, "--shape", shape, "--steps", str(steps), "--warmup",
        str(warmup)] + (["--graph"] if graph else [])
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        return {"error": f"exit {r.returncode}", "stderr": r.stderr[-1500:]}
    for line in reversed(r.stdout.splitlines()):
        if line.startswith("{"):
            return json.loads(line)
    return {"error": "no result line", "stdout": r.stdout[-1500:]}


def kernel_shares(shape, steps, warmup, limit, graph=False):
    if shutil.which("rocprofv3") is None:
        return {"not_measured": "rocprofv3 not found"}
    d = tempfile.mkdtemp(prefix="sdne_kt_")
    try:
        res = run_child("gw", shape, steps, warmup, limit,
                        prefix=["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "kt",
                                "--"], graph=graph)
        files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        if "error" in res or not files:
            return {"not_measured": res.get("error", "no kernel trace written"), "stderr": res.get("stderr", "")}
        acc = {}
        for r in csv.DictReader(open(files[0])):
            name = r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
            if name.startswith("k_sdne_"):
                e = acc.setdefault(name, [0, 0])
                e[0] += 1
                e[1] += int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
        total = sum(e[1] for e in acc.values()) or 1
        nsteps = warmup + 5 * steps + 1
        out = {k: dict(calls_per_step=e[0] / nsteps, avg_us=e[1] / e[0] / 1e3, us_per_step=e[1] / nsteps / 1e3,
                       share=e[1] / total, **res["kernel_attrs"].get(k, {}))
               for k, e in sorted(acc.items(), key=lambda x: -x[1][1])}
        out["kernel_us_per_step"] = total / nsteps / 1e3
        return out
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--limit", type=int, default=240, help="seconds per timed process")
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", action="store_true", help="only the per-kernel shares (rocprofv3 --kernel-trace --stats)")
    ap.add_argument("--child", choices=["gw", "torch"])
    ap.add_argument("--shape", choices=sorted(SHAPES), default="ref")
    ap.add_argument("--graph", action="store_true", help="child: the graph loss on")
    a = ap.parse_args()
    if a.child:
        if a.child == "gw":
            child_gw(a.shape, a.steps, a.warmup, a.graph)
        else:
            child_torch(a.shape, a.steps, a.warmup)
        return 0
    out = a.out or os.path.join(ROOT, "profiles", "sdne", "kernels.json" if a.trace else "bench.json")
    res, rc = {}, 0
    for shape in ("ref", "blog"):
        r = {"units": [SHAPES[shape], *HIDDEN, SHAPES[shape]], "batch": B, **counts(shape)}
        res[shape] = r
        if a.trace:
            r["kernel_share_of_step"] = kernel_shares(shape, min(a.steps, 40), 5, a.limit)
            if "not_measured" in r["kernel_share_of_step"]:
                rc = 1
                break
            if shape == "blog":
                r["graph_kernel_share_of_step"] = kernel_shares(shape, min(a.steps, 40), 5, a.limit, graph=True)
                if "not_measured" in r["graph_kernel_share_of_step"]:
                    rc = 1
                    break
            continue
        r["gw_sdne"] = run_child("gw", shape, a.steps, a.warmup, a.limit)
        if "error" in r["gw_sdne"]:   # nothing more is started on the GPU after a failed step
            rc = 1
            break
        if shape == "blog":
            r["graph_options"] = GRAPH
            r["gw_sdne_graph"] = run_child("gw", shape, a.steps, a.warmup, a.limit, graph=True)
            if "error" in r["gw_sdne_graph"]:
                rc = 1
                break
            r["graph_minus_default_us_per_step"] = 1e3 * (r["gw_sdne_graph"]["ms_per_step"] -
                                                          r["gw_sdne"]["ms_per_step"])
        r["torch_eager"] = run_child("torch", shape, a.steps, a.warmup, a.limit)
        if "error" in r["torch_eager"]:
            rc = 1
            break
        r["gw_over_torch_ms_per_step"] = r["gw_sdne"]["ms_per_step"] / r["torch_eager"]["ms_per_step"]
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    return rc


if __name__ == "__main__":
    sys.exit(main())
