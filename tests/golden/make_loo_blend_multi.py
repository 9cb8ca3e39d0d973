"""Writes tests/golden/loo_blend_multi_refits.npz: the long-double refits of tests/_loo_blend_multi_refs.py for every row
of every patch (patch r fitted without global point j, trend included, then the universal-kriging predictor at x_j), for
the eps values of _loo_blend_refs.CASES and the trends "constant" and "linear", rounded to double.

    python tests/golden/make_loo_blend_multi.py          (about three minutes on one core; --jobs N to spread it)

Per (eps, trend), under the key MultiOracle.golden_key(): _rj int32 [n, 2] (patch, global point), _mu float64 [n, 3],
_v float64 [n] (latent variance).  The tests fall back to computing an entry the file does not hold.
"""
import argparse
import os
import sys
from multiprocessing import Pool

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import _loo_blend_refs as BR            # noqa: E402
import _loo_blend_multi_refs as MR      # noqa: E402

_O = {}


def _oracle(eps, trend):
    if (eps, trend) not in _O:
        X, Y = MR.targets(MR.GOLDEN_R)
        _O[(eps, trend)] = MR.MultiOracle(X, Y, eps, [(("s34", BR.A), BR.SIGMA2)], trend)
    return _O[(eps, trend)]


def _one(job):
    eps, trend, r, j = job
    mu, v = _oracle(eps, trend).refitref_compute(r, j)
    return np.asarray(mu, dtype=np.float64), float(v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=1)
    a = ap.parse_args()
    out = {}
    with Pool(a.jobs) as pool:
        for eps in sorted({e for e, _ in BR.CASES}):
            for trend in ("constant", "linear"):
                o = _oracle(eps, trend)
                rj = [(r, int(j)) for r in range(o.P) for j in o.sets[r]]
                res = pool.map(_one, [(eps, trend, r, j) for r, j in rj], chunksize=16)
                k = o.golden_key()
                out[k + "_rj"] = np.array(rj, dtype=np.int32)
                out[k + "_mu"] = np.array([m for m, _ in res])
                out[k + "_v"] = np.array([v for _, v in res])
                print(k, len(rj), "refits")
    np.savez_compressed(MR.GOLDEN, **out)


if __name__ == "__main__":
    main()
