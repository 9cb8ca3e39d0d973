"""Launch dispatch coverage of the later stages: every (D, FAM, PP, dtype) instantiation behind launch_items_grad (pmk_grad.hip),
launch_items_vgrad (pmk_vgrad.hip: the strip sweep and the second dispatched kernel), launch_items_cov (pmk_cov.hip:
cov_strip_kernel, cov_block_kernel; through items_cov, items_cov_multi and items_cov_blocks) and launch_items_block
(pmk_block.hip: block_strip_kernel, block_self_kernel) is reached, and is the right one.  tests/test_gpu_dispatch.py does
the same for the three launchers of the fit and the items.

Every launcher takes `th`: a descriptor (PP = false, FAM from that descriptor) or null for the model's own kernels, which
after a plain fit is the model's one descriptor (PP = false again, FAM from the model) and after fit_patches the device
arrays (PP = true, FAM = Spline34 only if every patch is Spline34).  So

  a. fit(th) + stage(th), fit(th) + stage(None), fit_patches([th] * P) + stage(th) and fit_patches([th] * P) + stage(None)
     must give every array the stage exposes with equal bits, NaN included.  No header of the four files documents a pair
     of instantiations as not bit-equal, so <D, 0, false> and <D, 0, true> are held to this as well;
  b. one of the four (the per-patch one) is held against the stage's long-double reference in the stage's own unit: a wrong
     D or FAM that all four share;
  c. P copies of one theta cannot tell th_arg[region] from th_arg[0]: the DISTINCT lists (another range and sigma2 in every
     patch; FAM = Spline34 and FAM = 0, PP = true) and the MIXED list run stage(None) against per-patch references;
  d. a Spline32 descriptor on a Spline34 fit: the argument, not the model (TwoKernel of tests/_dispatch_stage_cases.py);
  e. one model refitted across families gives the bits of a fresh model after every fit;
  f. a Brownian bridge at D = 2 in a per-patch list: the product over the coordinates in the covariance and block stages,
     and the refusal of the two gradients for the model's own list.

References, units and bounds are the stages' own, no tolerance is new:
  grad    tests/test_gpu_grad.py: items against GR.item_grad_ref on the device's weights, |err| <= (n + 32) u lip sum |C|;
          the blend against GR.mix_grad_ref on the device's items, 16 m 2^-53 of its magnitude
  vgrad   tests/test_gpu_vgrad.py: items against PatchRef, 10 units, without a trend and under a linear one (the second
          kernel runs only under a trend), the trend's part within 1 unit of its own; the blend against VR.mix_vgrad_ref
  cov     tests/test_gpu_cov.py, tests/test_gpu_cov_multi.py (linear trend, R = 2): blocks and blend, 10 units; the blocks of
          items_cov_blocks are those of items_cov (tests/test_gpu_draw.py) and their factors L L^T = S + jitter I within 10
          units of tests/_draw_refs.py
  block   tests/test_gpu_block.py: _check (variance and pieces 10 units, means 1 bound)
tests/test_dispatch_stage_refs.py asserts on the CPU, of the same inputs, what these rest on, and that the kernels that
must be told apart lie more than 100 units from each other.

Every measured ratio is printed ("DISPATCH_STAGE {json}", run with -s); with PMK_WRITE_PROFILES=1 a run of the whole module
writes them to profiles/dispatch_stages_accuracy.json, each with `plain`, the figure of a plain numpy / LAPACK evaluation of
the same case in the model's precision against the same reference and unit.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import patchmixturekriging_amd as pmk
from patchmixturekriging_amd import mixture as M
from patchmixturekriging_amd.partition import hyperplane_arrays
import _cov_refs as CR
import _dispatch_stage_cases as DC
import _draw_refs as DR
import _grad_refs as GR
import _vgrad_refs as VR
from test_gpu_block import _check as _block_check
from test_gpu_cov import _check_blocks, _device_blocks
from test_gpu_cov_multi import _bits

pytestmark = pytest.mark.gpu

P, LD, U_OF, RATIO_MAX = DC.P, DC.LD, DC.U_OF, DC.RATIO_MAX
FORMS = [("fit", True), ("fit", False), ("fit_patches", True), ("fit_patches", False)]        # (the fit, stage(th) or stage(None))
REL = {"f64": 2.0 ** -20, "f32": 2.0 ** -6}     # factor_cov: relative jitter above the error of a block that is singular in exact arithmetic
_RECORDS, _CACHE = [], {}
ALL_TESTS = {"forms", "lists", "explicit", "refit", "bb"}
ACCURACY_JSON = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "dispatch_stages_accuracy.json")


def _record(**kw):
    _RECORDS.append(kw)
    print("DISPATCH_STAGE " + json.dumps(kw, sort_keys=True))


@pytest.fixture(scope="module", autouse=True)
def _write_accuracy_file():
    """only a run of the whole module replaces the file"""
    yield
    if os.environ.get("PMK_WRITE_PROFILES") == "1" and ALL_TESTS <= {r["test"] for r in _RECORDS}:
        with open(ACCURACY_JSON, "w") as f:
            f.write("[\n" + ",\n".join(" " + json.dumps(r, sort_keys=True) for r in _RECORDS) + "\n]\n")


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


# ------------------------------------------------------------------------------------------ models and stage runs
def _fit(m, hs, mode):
    ths = [DC.kernel(f, a)[0] for f, a, _ in hs]
    if mode == "fit":
        assert len(set(hs)) == 1
        m.fit(ths[0], hs[0][2])
    else:
        m.fit_patches(ths, [s2 for _, _, s2 in hs])
    assert np.all(m.info() == 0), m.info()


def _attach(m, w):
    """what a fit makes stale: the tree, the R target columns, no trend, the multi-output solve"""
    m.set_bsp(w.root, 0)
    m.set_targets_multi(w.Ys)
    m.set_trend(None)
    m.solve_multi()


def _model(w, hs, mode):
    """one fitted model per (workload, hyperparameter list, fit call)"""
    def make():
        m = M.DeviceModel(w.Xs, [np.ascontiguousarray(y[:, 0]) for y in w.Ys], dtype=w.dtype)
        _fit(m, hs, mode)
        _attach(m, w)
        return m
    return _cached(("model", id(w), tuple(hs), mode), make)


def _planned(w, m):
    q = M.DeviceQuery(m, w.Xq)
    q.plan(w.RADIUS, w.DELTA)
    return q


def _items_multi(q, th, variance):
    q.items_multi_fitted(variance) if th is None else q.items_multi(th, variance)


def _run(w, m, stage, th, factor=True):
    """-> (arrays: every array the stage exposes, by name; aux: what the references are fed with).  th: a kernel for every
    patch, or None for the model's own.  factor=False: the blocks of items_cov_blocks are not factored (a kernel that is not
    the fit's gives blocks that are no covariance)."""
    q = _planned(w, m)
    dbg = q.debug()
    assert np.array_equal(dbg["item_offsets"], w.items[0]) and np.array_equal(dbg["item_region"], w.items[1])
    aux = dict(q=q, t=dbg["item_t"], items=(dbg["item_offsets"], dbg["item_region"], dbg["item_t"]))
    if stage == "grad":
        _items_multi(q, th, False)
        q.mix_multi(w.wth)
        q.items_grad(th)
        q.mix_grad(w.wth)
        G, aux["plane"] = q.item_grads()
        aux["U"] = q.item_values_multi()[0]
        return dict(G=G, dY=q.fetch_grad()), aux
    if stage == "vgrad":
        _items_multi(q, th, True)
        q.mix_multi(w.wth)
        q.items_vgrad(th)
        q.mix_vgrad(w.wth)
        aux["plane"], aux["v"] = q.item_grads()[1], q.item_values_multi()[1]
        out = dict(GV=q.item_vgrads(), dV=q.fetch_vgrad())
        # under a linear trend: the second dispatched kernel of pmk_vgrad.hip runs only then
        m.set_trend(DC.TREND)
        m.solve_multi()
        assert np.all(m.trend_info() == 0)
        q2 = _planned(w, m)
        _items_multi(q2, th, True)
        q2.mix_multi(w.wth)
        q2.items_vgrad(th)
        q2.mix_vgrad(w.wth)
        aux["vt"] = q2.item_values_multi()[1]
        out["GVt"], out["dVt"] = q2.item_vgrads(), q2.fetch_vgrad()
        m.set_trend(None)
        m.solve_multi()
        return out, aux
    if stage == "block":
        _items_multi(q, th, False)
        q.items_block(w.group, w.a, w.wth, theta=th)
        out = {k: np.asarray(v, dtype=np.float64) for k, v in q.item_blocks().items()}
        out["Yb"], out["Vb"] = q.fetch_block()
        return out, aux
    assert stage == "cov"
    out = {}
    # items_cov: the single-output path
    q.items_fitted() if th is None else q.items(th)
    q.mix(w.wth)
    q.items_cov(th)
    q.mix_cov(w.wth)
    aux["single"] = _device_blocks(q, P)
    out.update({"S%d" % r: S for r, (_, S) in aux["single"].items()})
    out["Cov"] = q.fetch_cov()
    # items_cov_blocks and the factors of its blocks
    q.items_cov_blocks(th)
    aux["blocks"] = {r: (idx, S, None) for r, (idx, S) in _device_blocks(q, P).items()}
    if factor:
        q.factor_cov(np.full(P, REL[w.dtype]))
        finfo, aux["jitter"] = q.factor_info()
        assert np.all(finfo == 0), finfo
        aux["blocks"] = {r: (idx, S, q.item_cov_factor(r)) for r, (idx, S, _) in aux["blocks"].items()}
        out.update({"L%d" % r: L for r, (_, _, L) in aux["blocks"].items()})
        out["jitter"] = aux["jitter"]
    out.update({"B%d" % r: S for r, (_, S, _) in aux["blocks"].items()})
    # items_cov_multi under a linear trend, R = 2
    m.set_trend(DC.TREND)
    m.solve_multi()
    assert np.all(m.trend_info() == 0)
    q2 = _planned(w, m)
    _items_multi(q2, th, True)
    q2.mix_multi(w.wth)
    q2.items_cov_multi(th)
    q2.mix_cov(w.wth)
    aux["multi"], aux["q2"] = _device_blocks(q2, P), q2
    out.update({"T%d" % r: S for r, (_, S) in aux["multi"].items()})
    out["TCov"] = q2.fetch_cov()
    m.set_trend(None)
    m.solve_multi()
    return out, aux


def _same_bits(a, b, what):
    assert sorted(a) == sorted(b), what
    for k in a:
        assert _bits(a[k], b[k]), "%s: %s differs" % (what, k)


# ------------------------------------------------------------------------------------------ one run against the references
def _ratio(got, want, unit):
    return DC.ratio(np.abs(np.asarray(got, dtype=LD) - want), unit)


def _check(w, m, stage, key, out, aux, ev=None):
    """-> the worst ratios of one run of a stage under the list `key` against the references of its patches (ev = (family,
    a): the stage was handed that kernel, TwoKernel), asserted against the stage's own bounds"""
    hs, u, off, reg = DC.hypers(w, key, stage), U_OF[w.dtype], w.items[0], w.items[1]
    oths = [DC.kernel(*(h[:2] if ev is None else ev))[1] for h in hs]
    res = {}
    if stage == "grad":
        Cs, worst = m.weights_multi(), 0.0
        for r in range(P):
            ref = DC.item_grads(oths[r], w.Xs[r], Cs[r], w.points(r))
            bound = DC.grad_unit(oths[r], len(w.Xs[r]), Cs[r], u)
            worst = max(worst, _ratio(out["G"][w.sel[r]], ref, np.broadcast_to(bound[None, :, None], ref.shape)))
        hp_v, blend = hyperplane_arrays(w.root)[0], 0.0
        for j in range(len(w.Xq)):
            items = range(off[j], off[j + 1])
            ref, mag = GR.mix_grad_ref(items, out["G"], aux["U"], aux["t"], aux["plane"], hp_v, w.owth)
            blend = max(blend, _ratio(out["dY"][j], ref, 16 * len(items) * 2.0 ** -53 * mag.astype(np.float64)))
        res = dict(items=worst, blend=blend)
        assert worst <= 1.0 and blend <= 1.0, res
    elif stage == "vgrad":
        worst = trend = part = 0.0
        for r in range(P):
            ref = DC.patch_ref(w, r, hs[r]) if ev is None else DC.TwoKernel.on(DC.region_ref(w, r, hs[r]), oths[r])
            o, nu, sel = ref.items(w.points(r)), (len(w.Xs[r]) + 32) * u, w.sel[r]
            assert not o["clamped"].any()
            worst = max(worst, _ratio(out["GV"][sel], o["grad"], nu * o["unit"]))
            # under the trend: the sum in its unit, 10 units; the trend's part, the difference of the two device results
            # up to two double roundings of the whole gradient, in its own unit, 1 unit (tests/test_gpu_vgrad.py)
            o = DC.patch_ref(w, r, hs[r], DC.TREND, ev).items(w.points(r))
            trend = max(trend, _ratio(out["GVt"][sel], o["grad"], nu * o["unit"]))
            err = np.abs(np.asarray(out["GVt"][sel], dtype=LD) - np.asarray(out["GV"][sel], dtype=LD) - o["trend"]).astype(np.float64)
            part = max(part, DC.ratio(np.maximum(err - 4 * 2.0 ** -53 * np.abs(o["grad"]).astype(np.float64), 0.0), nu * o["tunit"]))
        hp_v, blend = hyperplane_arrays(w.root)[0], 0.0
        for GV, dV, v in ((out["GV"], out["dV"], aux["v"]), (out["GVt"], out["dVt"], aux["vt"])):
            for j in range(len(w.Xq)):
                items = range(off[j], off[j + 1])
                ref, mag = VR.mix_vgrad_ref(items, GV, v, aux["t"], aux["plane"], hp_v, w.owth)
                blend = max(blend, _ratio(dV[j], ref, 16 * len(items) * 2.0 ** -53 * mag.astype(np.float64)))
        res = dict(items=worst, blend=blend, trend_items=trend, trend_part=part)
        assert worst <= RATIO_MAX and trend <= RATIO_MAX and part <= 1.0 and blend <= 1.0, res
    elif stage == "cov":
        for name, blocks, trend, cov in (("single", aux["single"], None, out["Cov"]), ("multi", aux["multi"], DC.TREND, out["TCov"])):
            worst, _, S_ref, units = _check_blocks(blocks, w.Xq, DC.refs_of(w, key, stage, trend, ev), w.dtype)
            ref_cov, unit = CR.mix_cov_ref(aux["items"][:2], S_ref, aux["t"], w.owth, units)
            res[name], res[name + "_blend"] = worst, _ratio(cov, ref_cov, unit)
            assert np.array_equal(cov, cov.T)
        # the blocks of items_cov_blocks are those of items_cov, bit for bit; their factors
        for r, (idx, S, L) in aux["blocks"].items():
            assert _bits(S, aux["single"][r][1]), r
            if L is not None:
                assert np.all(np.triu(L, 1) == 0) and np.all(np.diag(L) > 0), r
                res["factor"] = max(res.get("factor", 0.0), DR.factor_ratio(L, S + aux["jitter"][r] * np.eye(len(S))))
        assert max(res.values()) <= RATIO_MAX, res
    else:
        refs = DC.refs_of(w, key, stage, None, ev)
        res, _, _, _ = _block_check(aux["q"], m, aux["items"], w.group, w.a, w.F, refs, oths, w.Xs, w.Xq, w.owth, None, w.dtype,
                                    sigma2=hs[0][2])
        res.pop("plain")                                        # of one sigma2 for every patch: DC.plain knows the list
        assert res["var"] <= RATIO_MAX and res["pieces"] <= RATIO_MAX and res["mean"] <= 1.0, res
    return res


def _fresh(w, key, stage, mode, own):
    """the cached run of a stage on the model of (list, fit call): stage(None) if own, else stage(th) of a uniform list"""
    hs = DC.hypers(w, key, stage)
    m = _model(w, hs, mode)
    return _cached(("run", id(w), tuple(hs), mode, own, stage), lambda: _run(w, m, stage, None if own else DC.kernel(*hs[0][:2])[0])) + (m,)


# ------------------------------------------------------------------------------------------ a, b
CASES = [(s, D, f, dt) for s in DC.STAGES for D in DC.DIMS for f in DC.FAMS for dt in DC.DTYPES]


@pytest.mark.parametrize("stage,D,fam,dtype", CASES, ids=["%s-%dd-%s-%s" % c for c in CASES])
def test_four_call_forms_give_one_answer_and_it_is_the_references(stage, D, fam, dtype):
    """<D, FAM, false> with th from the argument and from the model, <D, FAM, true> after fit_patches with th from the
    argument (PP = false on a per-patch model) and from the device arrays"""
    w = DC.workload(D, dtype)
    runs = {(mode, explicit): _fresh(w, fam, stage, mode, not explicit) for mode, explicit in FORMS}
    first = runs[FORMS[0]][0]
    for form in FORMS[1:]:
        _same_bits(first, runs[form][0], "%s, %s" % form)
    out, aux, m = runs[("fit_patches", False)]
    res = _check(w, m, stage, fam, out, aux)
    _record(test="forms", stage=stage, D=D, family=fam, dtype=dtype, plain=DC.plain(w, fam, stage), arrays=sorted(out), **res)


# ------------------------------------------------------------------------------------------ c
LIST_CASES = [(s, D, k, dt) for s in DC.STAGES for D in DC.DIMS for k in ("distinct34", "distinct32", "mixed") for dt in DC.DTYPES]


@pytest.mark.parametrize("stage,D,key,dtype", LIST_CASES, ids=["%s-%dd-%s-%s" % c for c in LIST_CASES])
def test_per_patch_values_come_from_their_own_patch(stage, D, key, dtype):
    """<D, PMK_SPLINE34, true> and <D, 0, true> on lists whose patches differ in range and sigma2, and the mixed list:
    tests/test_dispatch_stage_refs.py holds a kernel that reads patch 0's theta in every region more than 100 units away"""
    w = DC.workload(D, dtype)
    out, aux, m = _fresh(w, key, stage, "fit_patches", True)
    assert len(set(DC.hypers(w, key, stage))) == (P if key != "mixed" else 2)
    res = _check(w, m, stage, key, out, aux)
    _record(test="lists", stage=stage, D=D, list=key, dtype=dtype, plain=DC.plain(w, key, stage), **res)


# ------------------------------------------------------------------------------------------ d
def _main_arrays(w, stage, out):
    """per region, flattened: the arrays of a run that tests/_dispatch_stage_cases.py: stage_outputs has the units of"""
    if stage == "block":
        return [(out["kappa"] - out["vnorm2"])[out["region"] == r] for r in range(P)]
    if stage == "cov":
        return [out["S%d" % r].reshape(-1) for r in range(P)]
    return [out["G" if stage == "grad" else "GV"][w.sel[r]].reshape(-1) for r in range(P)]


@pytest.mark.parametrize("stage", DC.STAGES)
@pytest.mark.parametrize("D,dtype", sorted(DC.TWO_KERNEL))
def test_the_argument_is_not_the_models(D, dtype, stage):
    """a Spline32 descriptor on a model fitted with Spline34: FAM and theta come from the descriptor handed in"""
    w = DC.workload(D, dtype)
    key = ("spline34", DC.TWO_KERNEL[(D, dtype)][stage])
    own, _, m = _fresh(w, key, stage, "fit", True)
    th, ev = DC.kernel("spline32")[0], ("spline32", DC.A)
    out, aux = _run(w, m, stage, th, factor=False)
    res = _check(w, m, stage, key, out, aux, ev)
    apart = min(DC.ratio(np.abs(a - b), DC.stage_outputs(w, key, stage, r)[1])
                for r, (a, b) in enumerate(zip(_main_arrays(w, stage, out), _main_arrays(w, stage, own))))
    _record(test="explicit", stage=stage, D=D, dtype=dtype, sigma2=key[1], units_from_the_models_own=apart, **res)
    assert apart > DC.APART_MIN, apart


# ------------------------------------------------------------------------------------------ e
REFITS = [("fit", "spline34"), ("fit_patches", "mixed"), ("fit", "spline32"), ("fit_patches", "spline34")]


@pytest.mark.parametrize("D", [2, 3])
def test_refits_across_families_leave_nothing_behind(D):
    """fit(Spline34) -> fit_patches(MIXED) -> fit(Spline32) -> fit_patches([Spline34] * P) on one model: after each, every
    stage on the model's own kernels gives the bits of a fresh model fitted the same way"""
    w = DC.workload(D, "f64")
    m = M.DeviceModel(w.Xs, [np.ascontiguousarray(y[:, 0]) for y in w.Ys], dtype="f64")
    for mode, key in REFITS:
        hs = DC.hypers(w, key, "cov")                       # fp64: one sigma2 for every stage
        _fit(m, hs, mode)
        _attach(m, w)
        for stage in DC.STAGES:
            assert DC.hypers(w, key, stage) == hs
            out, _ = _run(w, m, stage, None)
            _same_bits(_fresh(w, key, stage, mode, True)[0], out, "%s after %s(%s)" % (stage, mode, key))
    _record(test="refit", D=D, fits=len(REFITS), stages=len(DC.STAGES))


# ------------------------------------------------------------------------------------------ f
def test_brownian_bridge_at_two_dimensions_in_a_per_patch_list():
    """kern_eval's product over the coordinates in cov_strip_kernel, cov_block_kernel, block_strip_kernel and
    block_self_kernel <2, 0, true>; and the two gradients refuse the model's own list as they refuse an explicit theta"""
    L = pmk.lib()
    for dtype in DC.BB_DTYPES:
        w = DC.workload(2, dtype, unit_square=True)
        for stage in ("cov", "block"):
            out, aux, m = _fresh(w, "bb", stage, "fit_patches", True)
            res = _check(w, m, stage, "bb", out, aux)
            _record(test="bb", stage=stage, dtype=dtype, plain=DC.plain(w, "bb", stage), **res)
        q = _planned(w, m)
        q.items_multi_fitted(True)
        U0, v0 = q.item_values_multi()
        for name in ("pmk_query_items_grad", "pmk_query_items_vgrad"):
            assert getattr(L, name)(q.h, None) == -2
            assert (name + ": the model's own theta is a Brownian-bridge family (PMK_BB10, 10): not differentiable on the "
                    "diagonal, no gradient").encode() in L.pmk_last_error(), L.pmk_last_error()
            assert getattr(L, name)(q.h, C.byref(pmk.BrownianBridge10(1.0).desc())) == -2
            assert (name + ": theta is a Brownian-bridge family (PMK_BB10, 10): not differentiable on the diagonal, no "
                    "gradient").encode() in L.pmk_last_error(), L.pmk_last_error()
        U1, v1 = q.item_values_multi()
        assert _bits(U1, U0) and _bits(v1, v0)
        assert L.pmk_query_get_items_vgrad(q.h, M._d(np.empty((q.total, 2))), 2) != 0      # and no gradient was left behind
