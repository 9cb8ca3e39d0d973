"""Posterior draws at config C (256 patches x 2000 points, 2-D Spline34(1/15), sigma2 = 1e-5, fp64), 64 draws: the dense
route of samplemixtureGP (the Nq x Nq covariance, one torch.linalg.cholesky_ex, z @ L.T) beside the block route
(pmk_query_factor_cov and pmk_query_draw on the region blocks), both in one process and on one plan per Nq.

  dense, Nq = 1024, 4096, 16384:  mix_cov (HIP events of the library), the copy into a torch tensor (fetch_cov_into; wall
          clock between two synchronisations: it runs on the library's stream), cholesky_ex and z @ L.T (torch events; one
          factorisation, at jitter 0 -- a covariance that needs the ladder pays it once per rung)
  blocks, the same sizes and 65536, 131072:  factor_cov (every call of the jitter ladder summed: rel = 0 for all regions,
          then the failed regions only) and draw, HIP events of the library, z and E on the device; the bytes the query owns
          A region that the ladder of the front ends does not reach (rel > 2^-26; they raise LinAlgError there) is taken
          further, x 10 a rung, so that the time is that of the whole batch; such regions are counted and three described.

Medians of --reps runs after one warm-up.  Required: at 16384 factor_cov + draw take less time than cholesky_ex alone.
Writes one JSON object to --out (default profiles/draw_time_C.json) and prints it.
Usage: python tools/draw_time.py [--reps 5] [--dense 1024,4096,16384] [--blocks 65536,131072] [--out FILE]
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

TQ, TILE, DRAW_TILE, DRAWS = 256, 128, 32, 64


def med(v):
    return float(np.median(v))


def ladder(q, P, ctx):
    """the jitter ladder of the front ends, continued past its end at rel = 2^-26 so that every region is factored and the
    time is that of the whole batch -> (ms of all factor_cov calls, calls, rel [P], jitter [P], finfo at rel = 0)"""
    rel, ms, calls, first = np.zeros(P), 0.0, 0, None
    while True:
        q.factor_cov(rel)
        finfo, jit = q.factor_info()
        first = finfo if first is None else first
        ms += ctx.timer_ms("factor_cov")
        calls += 1
        bad = finfo > 0
        if not bad.any():
            return ms, calls, rel, jit, first
        rel[bad] = np.where(rel[bad] == 0.0, 2.0 ** -52, 10.0 * rel[bad])
        assert np.all(rel <= 1.0) and not np.any(finfo < 0)


def hard_region(q, r, first, rel):
    """what the block of a region that the ladder of the front ends does not factor looks like"""
    idx, S = q.item_covs(r)
    lam = np.linalg.eigvalsh(S)
    d = np.diag(S)
    return {"region": int(r), "m": int(len(idx)), "first_failed_pivot": int(first[r]), "rel": float(rel[r]),
            "repeated_queries": int((np.diff(idx) == 0).sum()), "diag_min": float(d.min()), "diag_max": float(d.max()),
            "eig_min": float(lam[0]), "eig_max": float(lam[-1]), "clamped_diagonals": int((d == 1e-12).sum())}


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dense", default="1024,4096,16384")
    ap.add_argument("--blocks", default="65536,131072")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "draw_time_C.json"))
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
    dev = torch.device("cuda", ctx.device)
    model = M.DeviceModel(X_parts, [y[i].copy() for i in X_inds])
    model.set_bsp(root, 0)
    model.fit(th, sigma2)
    assert np.all(model.info() == 0)
    out = {"tool": "draw_time", "config": "C", "patches": P, "D": D, "reps": args.reps, "dtype": "f64", "draws": DRAWS,
           "Nq": {}}
    dense = [int(v) for v in args.dense.split(",") if v]
    for Nq in dense + [int(v) for v in args.blocks.split(",") if v]:
        Xq = np.stack([rng.uniform(-5, 5, Nq), rng.uniform(-10, 10, Nq)], 1)
        q = M.DeviceQuery(model, Xq)
        q.plan(radius, delta)
        q.items_fitted()
        q.mix(wth)
        counts = np.diff(q.region_offsets(P))
        total = int(q.total)
        r = {"items": total, "largest_block": int(counts.max())}
        gen = torch.Generator(device=dev).manual_seed(1)
        if Nq in dense:
            t = {k: [] for k in ("mix_cov", "copy", "cholesky_ex", "z_lt")}
            Cov = torch.empty((Nq, Nq), dtype=torch.float64, device=dev)
            z = torch.randn((DRAWS, Nq), dtype=torch.float64, device=dev, generator=gen)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            for _ in range(args.reps + 1):
                q.items_cov()
                q.mix_cov(wth)
                ctx.synchronize()
                t["mix_cov"].append(ctx.timer_ms("mix_cov"))
                t0 = time.perf_counter()
                q.fetch_cov_into(Cov)
                ctx.synchronize()
                t["copy"].append(1e3 * (time.perf_counter() - t0))
                ev[0].record()
                L, info = torch.linalg.cholesky_ex(Cov)
                ev[1].record()
                E = z @ L.T
                ev[2].record()
                torch.cuda.synchronize(dev)
                t["cholesky_ex"].append(ev[0].elapsed_time(ev[1]))
                t["z_lt"].append(ev[1].elapsed_time(ev[2]))
            r["dense"] = {k + "_ms": med(v[1:]) for k, v in t.items()}
            r["dense"].update({k + "_runs_ms": v[1:] for k, v in t.items()})
            r["dense"]["cholesky_info"] = int(info)
            r["dense"]["bytes"] = {"result": 8 * Nq * Nq, "torch_copy": 8 * Nq * Nq, "torch_factor": 8 * Nq * Nq}
            del Cov, L, E, z
        t = {k: [] for k in ("factor_cov", "draw")}
        z = torch.randn((DRAWS, total), dtype=torch.float64, device=dev, generator=gen)
        E = torch.empty((DRAWS, Nq), dtype=torch.float64, device=dev)
        torch.cuda.synchronize(dev)
        for _ in range(args.reps + 1):
            q.items_cov_blocks()                        # new blocks discard the factors: every rep factors all regions
            ms, calls, rel, jit, first = ladder(q, P, ctx)
            t["factor_cov"].append(ms)
            q.draw(wth, z, E)
            ctx.synchronize()
            t["draw"].append(ctx.timer_ms("draw"))
        b = {k + "_ms": med(v[1:]) for k, v in t.items()}
        b.update({k + "_runs_ms": v[1:] for k, v in t.items()})
        over = np.nonzero(rel > 2.0 ** -26)[0]
        b.update(factor_calls=calls, regions_with_jitter=int((rel > 0).sum()), jitter=float(jit.max()), rel_max=float(rel.max()),
                 regions_past_the_ladder=int(len(over)), hard_regions=[hard_region(q, r, first, rel) for r in over[:3]],
                 finite=bool(torch.isfinite(E).all()))
        nt = (counts + DRAW_TILE - 1) // DRAW_TILE
        ld = TILE * ((np.asarray(model.n) + TILE - 1) // TILE)
        chunk = min(max(((1 << 25) // max(total, 1)) // DRAW_TILE * DRAW_TILE, DRAW_TILE), 256, DRAWS)
        b["bytes"] = {"V_arena": int((((counts + TQ - 1) // TQ) * ld * TQ * 8).sum()), "blocks": int(8 * (counts ** 2).sum()),
                      "factors": int(8 * ((DRAW_TILE * nt) ** 2).sum()), "workspace": 8 * total * chunk,
                      "z_and_E_of_the_caller": 8 * DRAWS * (total + Nq)}
        r["blocks"] = b
        if Nq in dense:
            r["blocks_over_cholesky_ex"] = (b["factor_cov_ms"] + b["draw_ms"]) / r["dense"]["cholesky_ex_ms"]
        out["Nq"][str(Nq)] = r
        del q, z, E
    txt = json.dumps(out, indent=1, sort_keys=True)
    with open(args.out, "w") as f:
        f.write(txt + "\n")
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
