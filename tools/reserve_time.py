"""Reserved rows at config C (256 patches x 2000 points, 2-D Spline34(1/15), sigma2 = 1e-5, fp64; a patch of 2000 points has
ld = 2048, so 48 free rows): what pmk_model_reserve costs, what it costs a fit, and what appends across a block row cost
against building and fitting a fresh model of the extended sets.  Medians of --reps repetitions after one warm-up.

  reserve        reserve(128) on the fitted model (ld 2048 -> 2176): the "reserve" timer on HIP events (the two kernels of
                 pmk_reserve.hip), the host clock around the call (allocations, kernels, freeing the old layout), the
                 bytes the kernels move (active part read, new layout written) and the bandwidth the event time implies
  fits           the "fit" timer of the reserved model beside that of an unreserved model of the same sets, alternating
                 in one process, both models fitted once before
  appends        three appends of 48 points to every patch on the reserved model, 2000 -> 2048 -> 2096 -> 2144 (the
                 second enters a block row: nt 16 -> 17): the three stage timers, the host clock around the call (which
                 on the crossing call also rebuilds the factorisation order and drops the leave-one-out tasks), and
                 beside each the creation and fit of a fresh model of the extended sets (host clock and "fit" timer)

Writes one JSON object to --out (default profiles/reserve_time_C.json) and prints it.

--ab: nothing of the above; the fit and a 2^20-query items_multi with variance at R = 1, which run on any build of the
library (PMK_LIB): the comparison of a build with its parent in alternating processes.  Prints one JSON line.
Usage: python tools/reserve_time.py [--reps 5] [--out FILE] [--ab]
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

STAGES = ["append_sweep", "append_border", "append_solve"]
ROWS, STEP, CALLS = 128, 48, 3


def med(v):
    return float(np.median(v))


def target(X):
    return np.sin(0.5 * X[:, 0]) * np.cos(0.3 * X[:, 1]) + 2.0 + 0.3 * X[:, 0]


def ab(args, ctx, root, X_parts, y_parts, th, sigma2):
    model = M.DeviceModel(X_parts, y_parts)
    fit = []
    for _ in range(args.reps + 1):
        model.fit(th, sigma2)
        assert np.all(model.info() == 0)
        fit.append(ctx.timer_ms("fit"))
    rng = np.random.Generator(np.random.PCG64(26))
    nq = 1 << 20
    Xq = np.stack([rng.uniform(-5, 5, nq), rng.uniform(-10, 10, nq)], 1)
    radius = 0.1 * np.sqrt(200.0 / len(X_parts))
    model.set_bsp(root, 0)
    model.set_targets_multi([y.reshape(-1, 1) for y in y_parts])
    model.solve_multi()
    q = M.DeviceQuery(model, Xq)
    items = []
    for _ in range(args.reps + 1):
        q.plan(radius, 1e-5)
        q.items_multi(th, True)
        q.mix_multi(pmk.Spline34KernelType(1 / radius))
        q.fetch_multi(1)
        items.append(ctx.timer_ms("items_multi"))
    print(json.dumps({"tool": "reserve_time --ab", "lib": os.environ.get("PMK_LIB", "in-tree"), "fit_ms": med(fit[1:]),
                      "fit_runs_ms": fit[1:], "items_multi_R1_var_ms": med(items[1:]), "items_multi_runs_ms": items[1:]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reserve_time_C.json"))
    ap.add_argument("--ab", action="store_true")
    args = ap.parse_args()
    P, levels, a, sigma2 = 256, 9, 1 / 15, 1e-5
    rng = np.random.Generator(np.random.PCG64(25))
    N = 512000
    X = np.stack([rng.uniform(-5, 5, N), rng.uniform(-10, 10, N)], 1)
    root, X_parts, X_inds = pmk.setuppartition(X, levels, device=True)
    y_parts = [target(x) for x in X_parts]
    th = pmk.Spline34KernelType(a)
    ctx = pmk.default_context()
    ctx.enable_timers(True)
    if args.ab:
        return ab(args, ctx, root, X_parts, y_parts, th, sigma2)
    lo, hi = [x.min(0) for x in X_parts], [x.max(0) for x in X_parts]
    n = np.array([len(x) for x in X_parts])
    tiles = lambda v: (v + 127) // 128
    ld0, ld1 = 128 * tiles(n), 128 * tiles(n + ROWS)
    moved = 8 * int(((128 * tiles(n)) ** 2).sum() + (ld1 ** 2).sum())       # the slabs: the vectors are a few MB
    out = {"tool": "reserve_time", "config": "C", "patches": P, "D": 2, "reps": args.reps, "dtype": "f64",
           "n": [int(n.min()), int(n.max())], "ld": [int(ld0.max()), int(ld1.max())], "reserve_rows": ROWS,
           "reserve_bytes_moved": moved}
    # the new points of the three calls, inside the bounding box of their patch, and the extended sets after each
    Xn = [[rng.uniform(lo[r], hi[r], (STEP, 2)) for r in range(P)] for _ in range(CALLS)]
    yn = [[target(x) for x in step] for step in Xn]
    t = {k: [] for k in ["reserve_event", "reserve_call", "fit_unreserved", "fit_reserved"]}
    ta = [{k: [] for k in STAGES + ["append_call", "fresh_fit", "fresh_call"]} for _ in range(CALLS)]
    crossed = []
    for _ in range(args.reps + 1):
        plain = M.DeviceModel(X_parts, y_parts)
        model = M.DeviceModel(X_parts, y_parts)
        model.fit(th, sigma2)
        assert np.all(model.info() == 0)
        ctx.synchronize()
        t0 = time.perf_counter()
        free = model.reserve(ROWS)
        ctx.synchronize()
        t["reserve_call"].append(1e3 * (time.perf_counter() - t0))
        t["reserve_event"].append(ctx.timer_ms("reserve"))
        assert int(free.min()) >= ROWS
        plain.fit(th, sigma2)                            # the first fit of a newly created model is slower: not compared
        for _ in range(2):                               # alternating: unreserved, reserved, unreserved, reserved
            plain.fit(th, sigma2)
            assert np.all(plain.info() == 0)
            t["fit_unreserved"].append(ctx.timer_ms("fit"))
            model.fit(th, sigma2)
            assert np.all(model.info() == 0)
            t["fit_reserved"].append(ctx.timer_ms("fit"))
        del plain
        Xe, ye = list(X_parts), list(y_parts)
        crossed = []
        for k in range(CALLS):
            before = tiles(model.n.copy())
            ctx.synchronize()
            t0 = time.perf_counter()
            info = model.append(Xn[k], yn[k])
            ctx.synchronize()
            ta[k]["append_call"].append(1e3 * (time.perf_counter() - t0))
            assert np.all(info == 0)
            for s in STAGES:
                ta[k][s].append(ctx.timer_ms(s))
            crossed.append(int((tiles(model.n) != before).sum()))
            Xe = [np.ascontiguousarray(np.vstack([x, xn])) for x, xn in zip(Xe, Xn[k])]
            ye = [np.concatenate([y, v]) for y, v in zip(ye, yn[k])]
            ctx.synchronize()
            t0 = time.perf_counter()
            fresh = M.DeviceModel(Xe, ye)
            fresh.fit(th, sigma2)
            assert np.all(fresh.info() == 0)
            ta[k]["fresh_call"].append(1e3 * (time.perf_counter() - t0))
            ta[k]["fresh_fit"].append(ctx.timer_ms("fit"))
            del fresh
        del model
    out["reserve_event_ms"] = med(t["reserve_event"][1:])
    out["reserve_call_ms"] = med(t["reserve_call"][1:])
    out["reserve_runs_ms"] = {k: t[k][1:] for k in ("reserve_event", "reserve_call")}
    out["reserve_GBps"] = moved / (1e6 * out["reserve_event_ms"])
    for k in ("fit_unreserved", "fit_reserved"):
        out[k + "_ms"] = med(t[k][2:])                   # two fits per repetition: the warm-up repetition is the first two
        out[k + "_runs_ms"] = t[k][2:]
    out["fit_reserved_over_unreserved"] = out["fit_reserved_ms"] / out["fit_unreserved_ms"]
    out["appends"] = []
    for k in range(CALLS):
        r = {s + "_ms": med(v[1:]) for s, v in ta[k].items()}
        r.update({s + "_runs_ms": v[1:] for s, v in ta[k].items()})
        r["append_stages_ms"] = sum(r[s + "_ms"] for s in STAGES)
        r["patches_that_entered_a_block_row"] = crossed[k]
        r["points_per_patch"] = [int(n.min()) + STEP * k, int(n.min()) + STEP * (k + 1)]
        out["appends"].append(r)
    txt = json.dumps(out, indent=1, sort_keys=True)
    with open(args.out, "w") as f:
        f.write(txt + "\n")
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
