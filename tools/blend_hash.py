"""Bits of the item and blend kernels, for comparing two builds of the library: one SHA-256 per case over the raw bytes
of fetch / fetch_multi / fetch_grad, item_values_multi, item_grads, loo_values_multi, trend() and debug()["item_w"].
Run it once per build, each in a fresh process, and compare the lists (tools/fit_hash.py does the same for the fit):

    PMK_LIB=/path/to/parent/libpmk_hip.so python tools/blend_hash.py --out parent.json
    python tools/blend_hash.py --out new.json          # then: python tools/blend_hash.py --compare parent.json new.json

The cases are the smallest shapes at which these kernels take another path: D = 1 .. 4, Spline34 and the rational
quadratic (the run-time family switch), fp64 and fp32 models, one theta or one per patch, R = 1, 15, 16 and what a trend
leaves of 16, trend none / constant / linear, leaves of 1, 7, 8, 9, 128 and 129 points, regions with 0, 1, 15, 16, 17 and
33 items, noisy and variance on and off, a patch whose factorisation failed, patches of n < q and n = q points, queries
whose only item is the home item, and eps-sets (a point in several patches).  A call the library refuses enters the hash
with its message, so a refusal that changes shows too.  A few seconds on one GPU."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import patchmixturekriging_amd as pmk                      # noqa: E402
from patchmixturekriging_amd import mixture as M           # noqa: E402
from patchmixturekriging_amd._lib import PmkError          # noqa: E402

SIGMA2, DELTA, BOX = 1e-3, 1e-5, 2.0
COUNTS = [0, 1, 15, 16, 17, 33]                 # queries aimed at leaf r: COUNTS[r % 6]
FAMILY = {"s34": lambda: pmk.Spline34KernelType(1 / 3.0), "rq": lambda: pmk.RationalQuadraticKernelType(1.5)}

# name: D, family, dtype, theta per patch, R, trend, N, levels, eps, special
CASES = {
    "d1_s34_f64_R1_n1": (1, "s34", "f64", False, 1, None, 4, 3, None, None),
    "d2_rq_f64_pp_R15_const_n7_8": (2, "rq", "f64", True, 15, "constant", 60, 4, None, None),
    "d3_s34_f32_R16_n8_9": (3, "s34", "f32", False, 16, None, 68, 4, None, None),
    "d4_rq_f32_pp_R11_linear_n128_129": (4, "rq", "f32", True, 11, "linear", 514, 3, None, None),
    "d2_s34_f64_pp_R13_linear_eps": (2, "s34", "f64", True, 13, "linear", 514, 4, 0.3, None),
    "d1_rq_f64_R14_linear_n9": (1, "rq", "f64", False, 14, "linear", 72, 4, None, None),
    "d3_s34_f64_R12_linear_n_eq_q": (3, "s34", "f64", False, 12, "linear", 16, 3, None, None),
    "d2_s34_f64_R2_linear_n_lt_q": (2, "s34", "f64", False, 2, "linear", 8, 3, None, None),
    "d2_s34_f64_R3_const_failed": (2, "s34", "f64", False, 3, "constant", 120, 4, None, "failed"),
    "d2_rq_f32_pp_R3_linear_failed_eps": (2, "rq", "f32", True, 3, "linear", 120, 4, 0.3, "failed"),
    "d4_s34_f64_pp_R16_n129": (4, "s34", "f64", True, 16, None, 516, 3, None, None),
    "d2_rq_f32_R1_const_n1": (2, "rq", "f32", False, 1, "constant", 4, 3, None, None),
    "d3_rq_f64_pp_R15_const_eps": (3, "rq", "f64", True, 15, "constant", 257, 3, 0.4, None),
    "d4_s34_f32_R1_n7": (4, "s34", "f32", False, 1, None, 28, 3, None, None),
}


class Digest:
    def __init__(self):
        self.h, self.refused, self.arrays = hashlib.sha256(), [], 0

    def add(self, what, *arrays):
        self.h.update(what.encode())
        for a in arrays:
            if a is not None:
                a = np.ascontiguousarray(a)
                self.h.update(str(a.shape).encode() + a.tobytes())
                self.arrays += 1

    def call(self, what, f):
        """f() -> arrays; a refusal is part of the behaviour"""
        try:
            out = f()
        except PmkError as e:
            self.refused.append("%s: %s" % (what, e))
            self.h.update(("%s refused: %s" % (what, e)).encode())
            return None
        self.add(what, *(out if isinstance(out, tuple) else (out,)))
        return out


def aimed_queries(model, X, rng):
    """COUNTS[r % 6] points next to training points of leaf r"""
    off, inds = model.patch_index()
    rows = []
    for r in range(model.P):
        own = inds[off[r]:off[r + 1]]
        for k in range(COUNTS[r % len(COUNTS)]):
            rows.append(X[own[k % len(own)]] + 1e-3 * rng.uniform(-1, 1, X.shape[1]))
    return np.array(rows).reshape(-1, X.shape[1])


def run_case(name):
    D, fam, dtype, per_patch, R, trend, N, levels, eps, special = CASES[name]
    rng = np.random.Generator(np.random.PCG64(int(hashlib.sha256(name.encode()).hexdigest()[:8], 16)))
    X = rng.uniform(-BOX, BOX, (N, D))
    if dtype == "f32":
        X = X.astype(np.float32).astype(np.float64)
    Y = np.asfortranarray(np.stack([np.sin((1 + 0.2 * c) * X[:, 0]) + 0.1 * c * X[:, -1] + 0.05 * c for c in range(R)], 1))
    dg = Digest()
    root, _, _ = pmk.setuppartition(X, levels)
    model = M.DeviceModel.from_tree(root, X, np.ascontiguousarray(Y[:, 0]), eps=eps, dtype=dtype)
    th = FAMILY[fam]()
    if special == "failed":
        diag = np.zeros(N)
        diag[model.patch_index()[1][model.patch_index()[0][1] + 2]] = -3.0      # a point of patch 1: its pivot goes negative
        model.set_diag_global(diag)
    if per_patch:
        scale = [1.0 + 0.05 * (r % 3) for r in range(model.P)]
        model.fit_patches([type(th)(th.params[0] * s) for s in scale], [SIGMA2 * s for s in scale])
    else:
        model.fit(th, SIGMA2)
    arg = None if per_patch else th
    model.loo()
    model.set_targets_multi_global(Y)
    model.set_trend(trend)
    model.solve_multi()
    dg.add("info", model.info(), model.trend_info(), model.n)
    dg.call("trend", lambda: tuple(model.trend()[0]) + tuple(model.trend()[1]))
    dg.call("loo_values_multi", lambda: tuple(model.loo_values_multi()[0]) + tuple(model.loo_values_multi()[1]))

    radii = {"home": 1e-6, "wide": 1.5 * BOX}
    wth = {"home": pmk.Spline34KernelType(1 / 0.5), "wide": pmk.RationalQuadraticKernelType(2.0)}
    sets = {"aimed": aimed_queries(model, X, rng), "random": rng.uniform(-BOX, BOX, (37, D))}
    shape = {}
    for qname, Xq in sets.items():
        if len(Xq) == 0:
            continue
        q = M.DeviceQuery(model, Xq)
        for rname, radius in radii.items():
            tag = "%s/%s" % (qname, rname)
            total = q.plan(radius, DELTA)
            shape[tag] = [int(total), np.diff(q.region_offsets(model.P)).tolist()]
            dg.call(tag + " items", lambda: q.items(th) if arg is not None else q.items_fitted())
            dg.call(tag + " mix", lambda: q.mix(wth[rname]))
            dg.call(tag + " fetch", q.fetch)
            dg.call(tag + " item_w", lambda: q.debug()["item_w"])
            for variance in (True, False):
                v = tag + " var%d" % variance
                dg.call(v + " items_multi",
                        lambda: q.items_multi(th, variance) if arg is not None else q.items_multi_fitted(variance))
                dg.call(v + " item_values_multi", q.item_values_multi)
                dg.call(v + " mix_multi", lambda: q.mix_multi(wth[rname]))
                dg.call(v + " fetch_multi", lambda: q.fetch_multi(R))
                dg.call(v + " items_grad", lambda: q.items_grad(arg))
                dg.call(v + " item_grads", q.item_grads)
                dg.call(v + " mix_grad", lambda: q.mix_grad(wth[rname]))
                dg.call(v + " fetch_grad", q.fetch_grad)
    q = M.DeviceQuery(model, X)                             # leave-one-out: query j is training point j
    for rname, radius in radii.items():
        for noisy in (False, True):
            tag = "loo/%s noisy%d" % (rname, noisy)
            q.plan(radius, DELTA)
            counts = dg.call(tag + " items_loo", lambda: np.array(q.items_loo(noisy)))
            shape[tag] = None if counts is None else counts.tolist()
            dg.call(tag + " mix", lambda: q.mix(wth[rname]))
            dg.call(tag + " fetch", q.fetch)
            dg.call(tag + " item_w", lambda: q.debug()["item_w"])
            for variance in (True, False):
                v = tag + " var%d" % variance
                dg.call(v + " items_loo_multi", lambda: np.array(q.items_loo_multi(noisy, variance)))
                dg.call(v + " item_values_multi", q.item_values_multi)
                dg.call(v + " mix_multi", lambda: q.mix_multi(wth[rname]))
                dg.call(v + " fetch_multi", lambda: q.fetch_multi(R))
    return dict(sha256=dg.h.hexdigest(), arrays=dg.arrays, refused=dg.refused, n=[int(model.n.min()), int(model.n.max())],
                info=model.info().tolist(), trend_info=model.trend_info().tolist(), shape=shape)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", help="write the full record (hashes, shapes, refusals) as JSON")
    ap.add_argument("--compare", nargs=2, metavar="JSON", help="compare two records instead of running")
    a = ap.parse_args()
    if a.compare:
        one, two = (json.load(open(p))["cases"] for p in a.compare)
        bad = sorted(k for k in set(one) | set(two) if one.get(k, {}).get("sha256") != two.get(k, {}).get("sha256"))
        print("%d cases, %d differ%s" % (len(set(one) | set(two)), len(bad), "".join("\n  " + k for k in bad)))
        return 1 if bad else 0
    out = {"lib": os.environ.get("PMK_LIB", "(in-tree build)"), "cases": {}}
    for name in CASES:
        try:
            r = run_case(name)
        except PmkError as e:                               # a refusal outside the hashed calls: the case is its message
            r = dict(sha256="refused: %s" % e, arrays=0, refused=[str(e)], n=None)
        out["cases"][name] = r
        print("%s  %s  (%d arrays, %d refusals, n %s)" % (r["sha256"], name, r["arrays"], len(r["refused"]), r["n"]))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
