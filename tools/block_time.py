"""Block kriging at config C (256 patches x 2000 points, 2-D Spline34(1/15), sigma2 = 1e-5, fp64, R = 1, linear trend): what
the variance of group sums costs beside the point route it replaces.

Stage times on HIP events (pmk_ctx_timer_ms), the median of --reps runs after one warm-up, all in one process:

  items_block      pmk_query_items_block with the variance for --nq points (default 2^20) in groups of 1, 4, 16 and 64: a
                   group is a centre uniform in the domain and g points within +-0.02 of it, so its members share their
                   regions; a = 1 / g
  items_multi      pmk_query_items_multi_fitted with the variance on the same plan (the point route: one swept column per
                   item), and its ratio to items_block
  dense            at --nq-dense points (default 16384, the limit of the Nq x Nq result), groups of 16:
                   pmk_query_items_cov_multi + pmk_query_mix_cov on the library's timers and a^T Cov a as one device GEMM
                   pair timed on the wall clock, beside items_block on the same plan
  bytes            device memory taken while the query object lived (hipMemGetInfo before and after; the model's strip
                   workspace, which grows on first use, counts in the first case that needs it)

Writes one JSON object to --out (default profiles/block_time_C.json) and prints it.
Usage: python tools/block_time.py [--reps 5] [--nq 1048576] [--nq-dense 16384] [--groups 1,4,16,64] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import patchmixturekriging_amd as pmk                      # noqa: E402
from patchmixturekriging_amd import mixture as M           # noqa: E402


def med(v):
    return float(np.median(v))


def grouped_queries(rng, nq, g):
    F = nq // g
    c = np.stack([rng.uniform(-4.9, 4.9, F), rng.uniform(-9.9, 9.9, F)], 1)
    Xq = (c[:, None, :] + rng.uniform(-0.02, 0.02, (F, g, 2))).reshape(-1, 2)
    return np.ascontiguousarray(Xq), np.repeat(np.arange(F, dtype=np.int32), g), np.full(F * g, 1.0 / g)


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--nq", type=int, default=1 << 20)
    ap.add_argument("--nq-dense", type=int, default=16384)
    ap.add_argument("--groups", default="1,4,16,64")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "block_time_C.json"))
    args = ap.parse_args()
    P, levels, a, sigma2, delta, D = 256, 9, 1 / 15, 1e-5, 1e-5, 2
    rng = np.random.Generator(np.random.PCG64(25))
    N = 512000
    X = np.stack([rng.uniform(-5, 5, N), rng.uniform(-10, 10, N)], 1)
    radius = 0.1 * np.sqrt(200.0 / P)
    root, X_parts, X_inds = pmk.setuppartition(X, levels, device=True)
    y = np.sin(0.5 * X[:, 0]) * np.cos(0.3 * X[:, 1]) + 2.0 + 0.3 * X[:, 0]
    th, wth = pmk.Spline34KernelType(a), pmk.Spline34KernelType(1 / radius)
    ctx = pmk.default_context()
    ctx.enable_timers(True)
    ys = [y[i].copy() for i in X_inds]
    model = M.DeviceModel(X_parts, ys)
    model.set_bsp(root, 0)
    model.fit(th, sigma2)
    assert np.all(model.info() == 0)
    model.set_targets_multi(ys)
    model.set_trend("linear")
    model.solve_multi()
    out = {"tool": "block_time", "config": "C", "patches": P, "D": D, "R": 1, "trend": "linear", "reps": args.reps,
           "dtype": "f64", "nq": args.nq, "groups": {}}

    def free_bytes():
        ctx.synchronize()
        return int(torch.cuda.mem_get_info()[0])

    for g in [int(v) for v in args.groups.split(",")]:
        Xq, group, coef = grouped_queries(rng, args.nq, g)
        before = free_bytes()
        q = M.DeviceQuery(model, Xq)
        q.plan(radius, delta)
        t = {"items_multi": [], "items_block": []}
        for _ in range(args.reps + 1):
            q.items_multi_fitted(True)
            ctx.synchronize()
            t["items_multi"].append(ctx.timer_ms("items_multi"))
            q.items_block(group, coef, wth)
            Yb, Vb = q.fetch_block()
            t["items_block"].append(ctx.timer_ms("items_block"))
        r = {k + "_ms": med(v[1:]) for k, v in t.items()}
        r.update({k + "_runs_ms": v[1:] for k, v in t.items()})
        r["items_multi_over_items_block"] = r["items_multi_ms"] / r["items_block_ms"]
        r["items"] = int(q.total)
        r["aggregates"] = int(len(q.item_blocks()["count"]))
        r["bytes"] = before - free_bytes()
        r["finite"] = bool(np.all(np.isfinite(Yb)) and np.all(np.isfinite(Vb)) and np.all(Vb > 0))
        out["groups"][str(g)] = r
        del q

    # the dense route at its limit
    g = 16
    Xq, group, coef = grouped_queries(rng, args.nq_dense, g)
    F = args.nq_dense // g
    before = free_bytes()
    q = M.DeviceQuery(model, Xq)
    q.plan(radius, delta)
    t = {k: [] for k in ("items_cov_multi", "mix_cov", "a_cov_a", "items_block")}
    dev = torch.device("cuda")
    A = torch.zeros((F, len(Xq)), dtype=torch.float64, device=dev)
    A[torch.as_tensor(group.astype(np.int64), device=dev), torch.arange(len(Xq), device=dev)] = 1.0 / g
    Cov = torch.empty((len(Xq), len(Xq)), dtype=torch.float64, device=dev)
    for _ in range(args.reps + 1):
        q.items_multi_fitted(True)
        q.mix_multi(wth)
        q.items_cov_multi()
        q.mix_cov(wth)
        q.fetch_cov_into(Cov)
        ctx.synchronize()
        t["items_cov_multi"].append(ctx.timer_ms("items_cov"))
        t["mix_cov"].append(ctx.timer_ms("mix_cov"))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dense = ((A @ Cov) * A).sum(1)
        torch.cuda.synchronize()
        t["a_cov_a"].append(1e3 * (time.perf_counter() - t0))
        q.items_block(group, coef, wth)
        Yb, Vb = q.fetch_block()
        t["items_block"].append(ctx.timer_ms("items_block"))
    r = {k + "_ms": med(v[1:]) for k, v in t.items()}
    r.update({k + "_runs_ms": v[1:] for k, v in t.items()})
    r["dense_ms"] = r["items_cov_multi_ms"] + r["mix_cov_ms"] + r["a_cov_a_ms"]
    r["dense_over_items_block"] = r["dense_ms"] / r["items_block_ms"]
    r["max_rel_diff"] = float(np.max(np.abs(dense.cpu().numpy() - Vb) / Vb))
    r["bytes_with_the_dense_route"] = before - free_bytes()
    r["items"] = int(q.total)
    out["dense"] = {"nq": args.nq_dense, "group": g, **r}
    txt = json.dumps(out, indent=1, sort_keys=True)
    with open(args.out, "w") as f:
        f.write(txt + "\n")
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
