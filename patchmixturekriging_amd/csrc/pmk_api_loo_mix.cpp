// C ABI of libpmk_hip.so (declared in include/pmk.h): the blended leave-one-out, single-output (pmk_loo_mix.hip) and for
// R target columns with a trend (pmk_loo_mix_multi.hip): the items stage and the one-shot call of each.
#include "pmk_host.h"

using namespace pmk;

// buffers of the blended leave-one-out items for up to `total` sorted items, grow only.  ONE allocation; d_loo_x is its base.
static int loo_reserve(pmk_query *q, int64_t total)
{
    if (total <= q->loo_cap) return 0;
    dev_free(q->d_loo_x);
    q->loo_cap = 0;
    const size_t cap = (size_t)(total + total / 8 + 1024);
    Arena a;
    a.add(q->d_loo_x, cap * (size_t)q->m->D);
    a.add(q->d_loo_diag, cap);
    a.add(q->d_loo_ru, cap);
    a.add(q->d_loo_rv, cap);
    a.add(q->d_loo_off, cap + 1);
    a.add(q->d_loo_mark, cap + 1);
    a.add(q->d_loo_region, cap);
    if (int rc = a.commit()) return rc;
    q->loo_cap = (int64_t)cap;
    return 0;
}

// every refusal of the blended leave-one-out that depends on the model, host state only: nothing is launched before this
// returns 0.  Nq: the number of query points that will stand for the training points.
static int loo_model_ok(const pmk_model *m, int64_t Nq, const char *who)
{
    if (!m->fitted) { set_error("%s: model is not fitted", who); return -1; }
    if (!m->from_bsp) {
        set_error("%s: the model was not made by pmk_model_create_from_bsp (no map from patch rows to global points)", who);
        return -3;
    }
    if (Nq != m->N_global) {
        set_error("%s: the query has %lld points, the model %lld: query j must be global training point j", who,
                  (long long)Nq, (long long)m->N_global);
        return -3;
    }
    if (int rc = whole_tree_ok(m, who, "the blended leave-one-out needs every leaf", -3)) return rc;
    if (m->ths.empty()) { set_error("%s: the model holds no kernels (pmk_model_set_kernels)", who); return -3; }
    if (!m->loo_valid) { set_error("%s: pmk_model_loo has not run on the resident factor", who); return -3; }
    return 0;
}

// loo_model_ok plus the multi-output state; host state only
static int loo_multi_model_ok(const pmk_model *m, int64_t Nq, const char *who)
{
    if (int rc = loo_model_ok(m, Nq, who)) return rc;
    if (!m->multi_solved) { set_error("%s: pmk_model_solve_multi has not run on the resident factor", who); return -3; }
    return 0;
}

// What the two items stages share, up to the results of the non-members: member(s) looks every sorted item up and marks
// the rest, a scan counts them (*ns); if there are any they are compacted into requests and run by inner_items as the
// explicit items of the inner query (the request / response pattern of pmk_query_predict_sharded with this process as its
// own leaf owner; created on first need), with q's addends and variance floor.  The caller scatters the results.
template <typename Member, typename Items>
static int loo_requests(pmk_query *q, const char *who, Member member, Items inner_items, int64_t *ns)
{
    pmk_model *m = q->m;
    hipStream_t s = m->ctx->stream;
    int rc;
    *ns = 0;
    if (q->total > 0) {
        if ((rc = loo_reserve(q, q->total))) return rc;
        // members: a lookup per item, and the marks of the rest
        if ((rc = member(s))) return rc;
        if (exclusive_scan_i32_to_i64(q->d_loo_mark, q->d_loo_off, q->total, &q->d_tmp, &q->tmp_bytes, s)) {
            set_error("%s: prefix scan failed", who);
            return -100;
        }
        PMK_HIP(hipMemcpyAsync(ns, q->d_loo_off + q->total, sizeof(int64_t), hipMemcpyDeviceToHost, s));
        PMK_HIP(hipStreamSynchronize(s));
    }
    if (*ns == 0) return 0;
    if (!q->loo_inner && (rc = pmk_query_create(m, 0, nullptr, &q->loo_inner))) return rc;
    pmk_query *in = q->loo_inner;
    if ((rc = PMK_BY_DTYPE(m, launch_loo_compact(q, q->d_loo_mark, q->d_loo_off, q->d_loo_x, q->d_loo_region, q->d_loo_diag, s))))
        return rc;
    if ((rc = query_set_items(in, *ns, q->d_loo_x, q->d_loo_region))) return rc;
    // the addends in request order = the inner query's item order; borrowed for this launch only (the arena is q's)
    in->d_qdiag = q->d_qdiag ? q->d_loo_diag : nullptr;
    in->min_v = q->min_v;
    rc = inner_items(in);
    in->d_qdiag = nullptr;
    return rc;
}

extern "C" {

int pmk_query_items_loo(pmk_query *q, int noisy, int64_t *n_member, int64_t *n_strip)
{
    if (!q || !q->planned) { set_error("pmk_query_items_loo: query is not planned"); return -1; }
    pmk_model *m = q->m;
    if (int rc = loo_model_ok(m, q->Nq, "pmk_query_items_loo")) return rc;
    pmk_ctx *c = m->ctx;
    PMK_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    int64_t ns = 0;
    noisy = noisy != 0;
    c->tic("loo_items");
    int rc = loo_requests(
        q, "pmk_query_items_loo", [&](hipStream_t st) { return PMK_BY_DTYPE(m, launch_loo_member(q, noisy, q->d_loo_mark, st)); },
        pmk_query_items_fitted, &ns);               // non-members: queryinner! on the strip kernel
    if (!rc && ns > 0) rc = launch_export_results(q->loo_inner, q->d_loo_ru, q->d_loo_rv, s);
    if (!rc && ns > 0)
        rc = PMK_BY_DTYPE(m, launch_loo_scatter(q, noisy, q->d_loo_mark, q->d_loo_off, q->d_loo_ru, q->d_loo_rv, s));
    if (rc) return rc;
    c->toc("loo_items");
    if (n_member) *n_member = q->total - ns;
    if (n_strip) *n_strip = ns;
    return 0;
}

int pmk_predict_mixture_loo(pmk_model *m, const pmk_kernel_desc *weight_th, const double *X, double radius, double delta,
                            int noisy, double *Yq, double *Vq)
{
    if (!m) { set_error("pmk_predict_mixture_loo: model is NULL"); return -1; }
    if (int rc = loo_model_ok(m, m->N_global, "pmk_predict_mixture_loo")) return rc;
    if (!X) { set_error("pmk_predict_mixture_loo: X is NULL"); return -2; }
    return one_shot(m, m->N_global, X, radius, delta, [&](pmk_query *q) { return pmk_query_items_loo(q, noisy, nullptr, nullptr); },
                    [&](pmk_query *q) { return pmk_query_mix(q, weight_th, 0, q->Nq); },
                    [&](pmk_query *q) { return pmk_query_fetch(q, Yq, Vq); });
}

int pmk_query_items_loo_multi(pmk_query *q, int noisy, int want_var, int64_t *n_member, int64_t *n_other)
{
    if (!q || !q->planned) { set_error("pmk_query_items_loo_multi: query is not planned"); return -1; }
    pmk_model *m = q->m;
    if (int rc = loo_multi_model_ok(m, q->Nq, "pmk_query_items_loo_multi")) return rc;
    pmk_ctx *c = m->ctx;
    PMK_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const int R = m->R_multi, qt = m->trend_q;
    int64_t ns = 0;
    noisy = noisy != 0;
    want_var = want_var != 0;
    reset_item_state(q);
    if (int rc = grow(q->d_um, q->um_cap, q->total * (R + qt), s)) return rc;
    q->R_items = R;
    q->um_ld = R + qt;
    c->tic("loo_items_multi");
    int rc = loo_requests(
        q, "pmk_query_items_loo_multi",
        [&](hipStream_t st) { return PMK_BY_DTYPE(m, launch_loo_member_multi(q, noisy, want_var, q->d_loo_mark, st)); },
        [&](pmk_query *in) { return pmk_query_items_multi_fitted(in, want_var); }, &ns);    // non-members: its items
    if (!rc && ns > 0) rc = launch_loo_scatter_multi(q, q->loo_inner, noisy, want_var, q->d_loo_mark, q->d_loo_off, s);
    if (rc) { q->R_items = 0; return rc; }
    c->toc("loo_items_multi");
    q->var_items = want_var != 0;
    if (n_member) *n_member = q->total - ns;
    if (n_other) *n_other = ns;
    return 0;
}

int pmk_predict_mixture_loo_multi(pmk_model *m, const pmk_kernel_desc *weight_th, const double *X, double radius, double delta,
                                  int noisy, double *Yq, int64_t ldyq, double *Vq)
{
    if (!m) { set_error("pmk_predict_mixture_loo_multi: model is NULL"); return -1; }
    if (int rc = loo_multi_model_ok(m, m->N_global, "pmk_predict_mixture_loo_multi")) return rc;
    if (!X) { set_error("pmk_predict_mixture_loo_multi: X is NULL"); return -2; }
    if (Yq && ldyq < m->N_global) {
        set_error("pmk_predict_mixture_loo_multi: ldyq = %lld < N = %lld", (long long)ldyq, (long long)m->N_global);
        return -4;
    }
    return one_shot(m, m->N_global, X, radius, delta,
                    [&](pmk_query *q) { return pmk_query_items_loo_multi(q, noisy, Vq != nullptr, nullptr, nullptr); },
                    [&](pmk_query *q) { return pmk_query_mix_multi(q, weight_th, 0, q->Nq); },
                    [&](pmk_query *q) { return pmk_query_fetch_multi(q, Yq, ldyq, Vq); });
}

}  // extern "C"
