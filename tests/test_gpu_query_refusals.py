"""The refusals of the query side of the C ABI, pinned: return code and pmk_last_error() text of every precondition
that the query entry points share (the every-leaf check, the blending-profile and query-range checks of the mix
stages, the leading dimensions of the multi-output and gradient fetches and one-shot calls, the variance that was not
computed, the gradient after the lookups of the blended leave-one-out, and every reachable branch of the model checks
of the blended leave-one-out).  The expected texts are written out here, not derived from the library.

Shapes: D = 2, 64 points, a one-level tree (2 leaves), R = 2.  Every refusal returns before it launches anything.

One branch cannot be reached through the ABI and is not driven: "the model holds no kernels" of the blended
leave-one-out needs a fitted tree-built model without kernels, and only pmk_model_load (a list-built model) leaves a
factor without kernels.
"""
import ctypes as C

import numpy as np
import pytest

import patchmixturekriging_amd as pmk
from patchmixturekriging_amd import _lib

pytestmark = pytest.mark.gpu

N, D, LEVELS, R, NQ = 64, 2, 2, 2, 8
EPS, RADIUS, DELTA, SIGMA2 = 0.2, 0.4, 1e-5, 1e-4
DP = C.POINTER(C.c_double)


def _p(a):
    return a.ctypes.data_as(DP)


@pytest.fixture(scope="module")
def W():
    rng = np.random.Generator(np.random.PCG64(7))
    X = np.ascontiguousarray(rng.uniform(-1, 1, (N, D)))
    Y = np.asfortranarray(np.stack([np.sin(2 * X[:, 0]) + X[:, 1], np.cos(X[:, 0] * X[:, 1])], 1))
    Xq = np.ascontiguousarray(rng.uniform(-1, 1, (NQ, D)))
    root = pmk.setuppartition(X, LEVELS)[0]
    th, wth = pmk.Spline34KernelType(1.0), pmk.Spline34KernelType(1 / RADIUS)
    full = pmk.DeviceModel.from_tree(root, X, np.ascontiguousarray(Y[:, 0]), eps=EPS)
    assert full.P == 2
    full.fit(th, SIGMA2)
    full.loo()
    full.set_targets_multi_global(Y)
    full.solve_multi()
    shard = pmk.DeviceModel.from_tree(root, X, np.ascontiguousarray(Y[:, 0]), eps=EPS, leaf_base=1, P=1)
    shard.fit(th, SIGMA2)
    return dict(X=X, Y=Y, Xq=Xq, root=root, th=th.desc(), wth=wth.desc(), full=full, shard=shard, L=pmk.lib(),
                bb10=_lib.KernelDesc(family=10, flags=0))


def _planned(m, Xq):
    q = pmk.DeviceQuery(m, Xq)
    q.plan(RADIUS, DELTA)
    return q


def _refused(L, rc, code, text):
    assert rc == code, (rc, L.pmk_last_error().decode())
    assert L.pmk_last_error().decode() == text


# ------------------------------------------------------------------------------------------ the model must hold every leaf
def test_every_leaf_refusal_of_each_entry_point(W):
    L, m, Xq, th, wth = W["L"], W["shard"], W["Xq"], W["th"], W["wth"]
    X = W["X"]
    Yq, Vq, Ym, dY = np.empty(N), np.empty(N), np.empty((R, N)), np.empty((R * D, N))
    staged = "the model holds 1 of 2 leaves; use the staged pmk_query_* calls"
    blend = "the model holds 1 of 2 leaves; the blended leave-one-out needs every leaf"
    multi = "the model holds 1 of 2 leaves; multi-output prediction needs a model that holds every leaf"
    grad = "the model holds 1 of 2 leaves; the gradient needs a model that holds every leaf"
    _refused(L, L.pmk_predict_mixture(m.h, C.byref(th), C.byref(wth), NQ, _p(Xq), RADIUS, DELTA, _p(Yq), _p(Vq)), -1,
             "pmk_predict_mixture: " + staged)
    _refused(L, L.pmk_predict_mixture_fitted(m.h, C.byref(wth), NQ, _p(Xq), RADIUS, DELTA, _p(Yq), _p(Vq)), -1,
             "pmk_predict_mixture_fitted: " + staged)
    q = _planned(m, X)
    _refused(L, L.pmk_query_items_loo(q.h, 0, None, None), -3, "pmk_query_items_loo: " + blend)
    _refused(L, L.pmk_query_items_loo_multi(q.h, 0, 1, None, None), -3, "pmk_query_items_loo_multi: " + blend)
    _refused(L, L.pmk_predict_mixture_loo(m.h, C.byref(wth), _p(X), RADIUS, DELTA, 0, _p(Yq), _p(Vq)), -3,
             "pmk_predict_mixture_loo: " + blend)
    _refused(L, L.pmk_predict_mixture_loo_multi(m.h, C.byref(wth), _p(X), RADIUS, DELTA, 0, _p(Ym), N, _p(Vq)), -3,
             "pmk_predict_mixture_loo_multi: " + blend)
    _refused(L, L.pmk_query_items_multi(q.h, C.byref(th), 1), -4, "pmk_query_items_multi: " + multi)
    _refused(L, L.pmk_query_items_multi_fitted(q.h, 1), -4, "pmk_query_items_multi: " + multi)
    _refused(L, L.pmk_predict_mixture_multi(m.h, C.byref(th), C.byref(wth), NQ, _p(Xq), RADIUS, DELTA, _p(Ym), NQ, _p(Vq)),
             -4, "pmk_predict_mixture_multi: " + multi)
    _refused(L, L.pmk_predict_mixture_multi_fitted(m.h, C.byref(wth), NQ, _p(Xq), RADIUS, DELTA, _p(Ym), NQ, _p(Vq)), -4,
             "pmk_predict_mixture_multi_fitted: " + multi)
    _refused(L, L.pmk_query_items_grad(q.h, C.byref(th)), -4, "pmk_query_items_grad: " + grad)
    _refused(L, L.pmk_predict_mixture_grad_fitted(m.h, C.byref(wth), NQ, _p(Xq), RADIUS, DELTA, _p(Ym), NQ, _p(dY), NQ), -4,
             "pmk_predict_mixture_grad_fitted: " + grad)


# ------------------------------------------------------------------------------------------ blending profile, query range
def test_blending_profile_and_query_range_of_the_mix_stages(W):
    L, th, wth, bb10 = W["L"], W["th"], W["wth"], W["bb10"]
    q = _planned(W["full"], W["Xq"])
    assert L.pmk_query_items_multi(q.h, C.byref(th), 0) == 0
    assert L.pmk_query_items_grad(q.h, C.byref(th)) == 0
    for name in ("pmk_query_mix", "pmk_query_mix_multi"):
        f = getattr(L, name)
        _refused(L, f(q.h, C.byref(bb10), 0, NQ), -2,
                 name + ": the blending profile must be a stationary kernel (evalkernel(tau, theta))")
        _refused(L, f(q.h, None, 0, NQ), -2,
                 name + ": the blending profile must be a stationary kernel (evalkernel(tau, theta))")
    _refused(L, L.pmk_query_mix_grad(q.h, C.byref(bb10), 0, NQ), -2,
             "pmk_query_mix_grad: the blending profile is a Brownian-bridge family (PMK_BB10, 10): not differentiable on "
             "the diagonal, no gradient")
    for name in ("pmk_query_mix", "pmk_query_mix_multi", "pmk_query_mix_grad"):
        f = getattr(L, name)
        for q0, q1 in ((-1, NQ), (0, NQ + 1), (2, 1)):
            _refused(L, f(q.h, C.byref(wth), q0, q1), -3, name + ": bad query range")
    # nothing above left a mark: the good calls follow
    assert L.pmk_query_mix_multi(q.h, C.byref(wth), 0, NQ) == 0 and L.pmk_query_mix_grad(q.h, C.byref(wth), 0, NQ) == 0


# ------------------------------------------------------------------------------------------ leading dimensions, missing variance
def test_leading_dimensions_and_the_variance_that_was_not_computed(W):
    L, m, Xq, X, th, wth = W["L"], W["full"], W["Xq"], W["X"], W["th"], W["wth"]
    Ym, Vq, dY = np.empty((R, N)), np.empty(N), np.empty((R * D, N))
    # one-shot calls
    _refused(L, L.pmk_predict_mixture_multi(m.h, C.byref(th), C.byref(wth), NQ, _p(Xq), RADIUS, DELTA, _p(Ym), NQ - 1, None),
             -4, "pmk_predict_mixture_multi: ldyq = 7 < Nq = 8")
    _refused(L, L.pmk_predict_mixture_multi_fitted(m.h, C.byref(wth), NQ, _p(Xq), RADIUS, DELTA, _p(Ym), NQ - 1, None), -4,
             "pmk_predict_mixture_multi_fitted: ldyq = 7 < Nq = 8")
    _refused(L, L.pmk_predict_mixture_loo_multi(m.h, C.byref(wth), _p(X), RADIUS, DELTA, 0, _p(Ym), N - 1, None), -4,
             "pmk_predict_mixture_loo_multi: ldyq = 63 < N = 64")
    _refused(L, L.pmk_predict_mixture_grad_fitted(m.h, C.byref(wth), NQ, _p(Xq), RADIUS, DELTA, _p(Ym), NQ - 1, _p(dY), NQ), -4,
             "pmk_predict_mixture_grad_fitted: ldyq = 7 or lddy = 8 < Nq = 8")
    _refused(L, L.pmk_predict_mixture_grad_fitted(m.h, C.byref(wth), NQ, _p(Xq), RADIUS, DELTA, _p(Ym), NQ, _p(dY), NQ - 1), -4,
             "pmk_predict_mixture_grad_fitted: ldyq = 8 or lddy = 7 < Nq = 8")
    # fetches of a query mixed without variances
    q = _planned(m, Xq)
    assert L.pmk_query_items_multi(q.h, C.byref(th), 0) == 0
    assert L.pmk_query_items_grad(q.h, C.byref(th)) == 0
    assert L.pmk_query_mix_multi(q.h, C.byref(wth), 0, NQ) == 0 and L.pmk_query_mix_grad(q.h, C.byref(wth), 0, NQ) == 0
    _refused(L, L.pmk_query_fetch_multi(q.h, _p(Ym), NQ - 1, None), -4, "pmk_query_fetch_multi: ldyq = 7 < Nq = 8")
    _refused(L, L.pmk_query_fetch_multi_dev(q.h, Ym.ctypes.data, NQ - 1, None), -4,
             "pmk_query_fetch_multi_dev: ldyq = 7 < Nq = 8")
    _refused(L, L.pmk_query_fetch_grad(q.h, _p(dY), NQ - 1), -4, "pmk_query_fetch_grad: lddy = 7 < Nq = 8")
    _refused(L, L.pmk_query_fetch_grad_dev(q.h, dY.ctypes.data, NQ - 1), -4, "pmk_query_fetch_grad_dev: lddy = 7 < Nq = 8")
    _refused(L, L.pmk_query_fetch_multi(q.h, _p(Ym), NQ, _p(Vq)), -3,
             "pmk_query_fetch_multi: Vq was not computed (pmk_query_items_multi ran with want_var = 0)")
    _refused(L, L.pmk_query_fetch_multi_dev(q.h, Ym.ctypes.data, NQ, Vq.ctypes.data), -3,
             "pmk_query_fetch_multi_dev: Vq was not computed (pmk_query_items_multi ran with want_var = 0)")
    U, v = np.empty((q.total, R)), np.empty(q.total)
    _refused(L, L.pmk_query_get_items_multi(q.h, _p(U), R, _p(v)), -3,
             "pmk_query_get_items_multi: v was not computed (the items ran with want_var = 0)")
    # the good fetches follow
    assert L.pmk_query_fetch_multi(q.h, _p(Ym), NQ, None) == 0 and L.pmk_query_fetch_grad(q.h, _p(dY), NQ) == 0
    assert L.pmk_query_get_items_multi(q.h, _p(U), R, None) == 0


# ------------------------------------------------------------------------------------------ gradient after the lookups
def test_items_grad_after_items_loo_multi(W):
    L, th = W["L"], W["th"]
    q = _planned(W["full"], W["X"])
    assert L.pmk_query_items_loo_multi(q.h, 0, 0, None, None) == 0
    _refused(L, L.pmk_query_items_grad(q.h, C.byref(th)), -2,
             "pmk_query_items_grad: the last items on this plan must be those of pmk_query_items_multi or _multi_fitted "
             "(a member item of pmk_query_items_loo_multi is a lookup, not a function of x)")


# ------------------------------------------------------------------------------------------ model checks of the blended LOO
def test_every_branch_of_the_blended_leave_one_out_model_checks(W):
    L, X, Y, root, wth = W["L"], W["X"], W["Y"], W["root"], W["wth"]
    Yq, Vq, Ym = np.empty(N), np.empty(N), np.empty((R, N))
    th = pmk.Spline34KernelType(1.0)

    def all_four(m, code, tail):
        q = _planned(m, X)
        _refused(L, L.pmk_query_items_loo(q.h, 0, None, None), code, "pmk_query_items_loo: " + tail)
        _refused(L, L.pmk_query_items_loo_multi(q.h, 0, 1, None, None), code, "pmk_query_items_loo_multi: " + tail)
        _refused(L, L.pmk_predict_mixture_loo(m.h, C.byref(wth), _p(X), RADIUS, DELTA, 0, _p(Yq), _p(Vq)), code,
                 "pmk_predict_mixture_loo: " + tail)
        _refused(L, L.pmk_predict_mixture_loo_multi(m.h, C.byref(wth), _p(X), RADIUS, DELTA, 0, _p(Ym), N, _p(Vq)), code,
                 "pmk_predict_mixture_loo_multi: " + tail)

    fresh = pmk.DeviceModel.from_tree(root, X, np.ascontiguousarray(Y[:, 0]), eps=EPS)
    all_four(fresh, -1, "model is not fitted")
    fresh.fit(th, SIGMA2)
    all_four(fresh, -3, "pmk_model_loo has not run on the resident factor")
    fresh.loo()
    q = _planned(fresh, X)
    _refused(L, L.pmk_query_items_loo_multi(q.h, 0, 1, None, None), -3,
             "pmk_query_items_loo_multi: pmk_model_solve_multi has not run on the resident factor")
    _refused(L, L.pmk_predict_mixture_loo_multi(fresh.h, C.byref(wth), _p(X), RADIUS, DELTA, 0, _p(Ym), N, _p(Vq)), -3,
             "pmk_predict_mixture_loo_multi: pmk_model_solve_multi has not run on the resident factor")
    assert L.pmk_query_items_loo(q.h, 0, None, None) == 0          # the single-output form has all it needs
    # a model built from lists of patches
    sets = pmk.organizetrainingsets(root, LEVELS, X, EPS)[1]
    lists = pmk.DeviceModel([X[s] for s in sets], [Y[s, 0] for s in sets])
    lists.set_bsp(root, 0)
    lists.fit(th, SIGMA2)
    lists.loo()
    all_four(lists, -3, "the model was not made by pmk_model_create_from_bsp (no map from patch rows to global points)")
    # a query that is not the training points
    q = _planned(W["full"], np.ascontiguousarray(X[:-1]))
    tail = "the query has 63 points, the model 64: query j must be global training point j"
    _refused(L, L.pmk_query_items_loo(q.h, 0, None, None), -3, "pmk_query_items_loo: " + tail)
    _refused(L, L.pmk_query_items_loo_multi(q.h, 0, 1, None, None), -3, "pmk_query_items_loo_multi: " + tail)
