// C ABI of libpmk_hip.so (declared in include/pmk.h), the query side: the query object (create, plan, export), its
// single-output, multi-output and gradient stages (items, mix, fetch), the one-shot pmk_predict_mixture* calls, and the
// calls that evaluate a kernel without a model or on one patch of it (pmk_kernel_matrix, pmk_query_mean,
// pmk_model_queryinner).  The blended leave-one-out is in pmk_api_loo_mix.cpp; contexts, trees and models in pmk_api.cpp.
#include <algorithm>
#include <cstring>
#include <new>

#include "pmk_host.h"

namespace pmk {

// per-query-point buffers for up to Nq points, grow only.  ONE allocation; d_xq is its base (the only pointer freed).
int query_reserve(pmk_query *q, int64_t Nq)
{
    if (Nq <= q->nq_cap) return 0;
    const bool regrow = q->nq_cap > 0;
    dev_free(q->d_xq);
    q->nq_cap = 0;
    const size_t cap = (size_t)(Nq + (regrow ? Nq / 8 : 0)), c1 = std::max<size_t>(cap, 1);
    Arena a;
    a.add(q->d_xq, c1 * (size_t)q->m->D);
    a.add(q->d_stage_t, 4 * c1);                // PLAN_STAGE rows
    a.add(q->d_yq, c1);
    a.add(q->d_vq, c1);
    a.add(q->d_qoff, c1 + 1);
    a.add(q->d_home, c1);
    a.add(q->d_cnt, c1 + 1);
    a.add(q->d_stage_r, 4 * c1);
    a.add(q->d_stage_p, 4 * c1);
    if (int rc = a.commit()) return rc;
    q->nq_cap = (int64_t)cap;
    return 0;
}

// per-item buffers, grow only: repeated plans of one query batch reuse them.  ONE allocation; d_item_t is its base.
int grow_item_buffers(pmk_query *q, int64_t total)
{
    if (total <= q->item_cap) return 0;
    dev_free(q->d_item_t);
    q->item_cap = 0;
    const size_t cap = (size_t)(total + total / 8 + 1024);
    Arena a;
    a.add(q->d_item_t, cap);
    a.add(q->d_u, cap);
    a.add(q->d_v, cap);
    a.add(q->d_w, cap);
    a.add(q->d_item_region, cap);
    a.add(q->d_item_query, cap);
    a.add(q->d_sorted_item, cap);
    a.add(q->d_item_pos, cap);
    a.add(q->d_item_plane, cap);
    if (int rc = a.commit()) return rc;
    q->item_cap = (int64_t)cap;
    return 0;
}

// (re)load a query object with n explicit (point, region) items, one per point (host or device pointers): what
// pmk_query_create_items does after allocating; reuses the object's buffers.  Blocks (region offsets come back).
int query_set_items(pmk_query *q, int64_t n, const double *xq, const int32_t *region)
{
    pmk_model *m = q->m;
    pmk_ctx *c = m->ctx;
    hipStream_t s = c->stream;
    int rc;
    if ((rc = query_reserve(q, n))) return rc;
    q->Nq = n;
    q->total = n;
    q->planned = false;
    reset_plan_state(q);
    q->explicit_items = true;
    q->roff.assign((size_t)(m->P_global + 1), 0);
    q->ntasks = 0;
    if (n > 0) {
        int bad = 0;
        if ((rc = grow_item_buffers(q, n))) return rc;
        if (!q->d_flag && dev_alloc(&q->d_flag, 1)) return -100;
        hipError_t e = hipMemcpyAsync(q->d_xq, xq, sizeof(double) * (size_t)(n * m->D), hipMemcpyDefault, s);
        if (e == hipSuccess) e = hipMemcpyAsync(q->d_item_region, region, sizeof(int32_t) * (size_t)n, hipMemcpyDefault, s);
        if (e == hipSuccess) e = hipMemsetAsync(q->d_flag, 0, sizeof(int), s);
        if (e == hipSuccess) e = hipMemsetAsync(q->d_item_plane, 0xff, sizeof(int32_t) * (size_t)n, s);   // -1: no plane
        if (e == hipSuccess) rc = launch_explicit_items(q, q->d_flag, s);
        if (e == hipSuccess && !rc) rc = launch_sort_items(q, s);
        if (e == hipSuccess && !rc) e = hipMemcpyAsync(&bad, q->d_flag, sizeof(int), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess && !rc)
            e = hipMemcpyAsync(q->roff.data(), q->d_roff, sizeof(int64_t) * q->roff.size(), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess && !rc) e = hipStreamSynchronize(s);
        if (e != hipSuccess) { set_error("query_set_items: %s", hipGetErrorString(e)); return -100; }
        if (rc) return rc;
        if (bad) {
            set_error("pmk_query_create_items: a region is outside this model's leaves [%lld, %lld)",
                      (long long)m->leaf_base, (long long)(m->leaf_base + m->P));
            return -3;
        }
        if ((rc = PMK_BY_DTYPE(m, build_strip_tasks(q, s)))) return rc;
    }
    q->planned = true;
    return 0;
}

}  // namespace pmk

using namespace pmk;

// `cols` columns of the rows of a buffer in sorted order (leading dimension ld) -> rows of dst in item order (the order
// of pmk_query_debug).  Synchronous; the caller has drained the stream.
static int download_item_rows(pmk_query *q, const double *d_src, size_t ld, size_t cols, double *dst, size_t lddst)
{
    const size_t T = (size_t)q->total;
    std::vector<int32_t> pos(T);
    std::vector<double> tmp(T * ld);
    PMK_HIP(hipMemcpy(pos.data(), q->d_item_pos, sizeof(int32_t) * T, hipMemcpyDeviceToHost));
    PMK_HIP(hipMemcpy(tmp.data(), d_src, sizeof(double) * tmp.size(), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < T; ++i)
        for (size_t j = 0; j < cols; ++j) dst[i * lddst + j] = tmp[(size_t)pos[i] * ld + j];
    return 0;
}

static int query_range_ok(const pmk_query *q, int64_t q0, int64_t q1, const char *who)
{
    if (q0 < 0 || q1 > q->Nq || q0 > q1) { set_error("%s: bad query range", who); return -3; }
    return 0;
}

// what whole_tree_ok says to the callers of the multi-output and of the gradient stages
static const char MULTI_NEEDS_ALL[] = "multi-output prediction needs a model that holds every leaf";
static const char GRAD_NEEDS_ALL[] = "the gradient needs a model that holds every leaf";
static const char USE_STAGED[] = "use the staged pmk_query_* calls";

extern "C" {

// ------------------------------------------------------------------------------------------ calls without a query object
int pmk_kernel_matrix(pmk_ctx *ctx, const pmk_kernel_desc *th, int D, int64_t n, const double *X, int64_t m,
                      const double *Z, double *K, int64_t ldk)
{
    if (!ctx) { set_error("pmk_kernel_matrix: ctx is NULL"); return -1; }
    if (!kernel_ok(th)) { set_error("pmk_kernel_matrix: unknown kernel family"); return -2; }
    if (D < 1 || D > MAX_D) { set_error("pmk_kernel_matrix: D=%d outside 1..%d", D, MAX_D); return -3; }
    if (n < 1 || !X || !K) { set_error("pmk_kernel_matrix: empty input"); return -4; }
    const bool sym = (Z == nullptr);
    const int64_t mc = sym ? n : m;
    if (mc < 1 || ldk < n) { set_error("pmk_kernel_matrix: bad m/ldk"); return -6; }
    PMK_HIP(hipSetDevice(ctx->device));
    std::vector<double> hx((size_t)(n * D)), hz;
    pack_soa(D, n, n, X, hx.data());
    DevTmp<double> dx, dz, dK;
    if (dx.alloc(n * D)) return -100;
    PMK_HIP(hipMemcpyAsync(dx, hx.data(), sizeof(double) * hx.size(), hipMemcpyHostToDevice, ctx->stream));
    if (!sym) {
        hz.resize((size_t)(mc * D));
        pack_soa(D, mc, mc, Z, hz.data());
        if (dz.alloc(mc * D)) return -100;
        PMK_HIP(hipMemcpyAsync(dz, hz.data(), sizeof(double) * hz.size(), hipMemcpyHostToDevice, ctx->stream));
    }
    if (dK.alloc(n * mc)) return -100;
    int rc = launch_kernel_matrix_dense(*th, D, n, dx, n, mc, sym ? dx : dz, sym ? n : mc, dK, n, sym, ctx->stream);
    if (!rc) {
        PMK_HIP(hipMemcpy2DAsync(K, sizeof(double) * ldk, dK, sizeof(double) * n, sizeof(double) * n, (size_t)mc,
                                 hipMemcpyDeviceToHost, ctx->stream));
    }
    PMK_HIP(hipStreamSynchronize(ctx->stream));     // also on failure: the temporaries must outlive the queued copies
    return rc;
}

int pmk_query_mean(pmk_ctx *ctx, const pmk_kernel_desc *th, int D, int64_t n, const double *X, const double *c,
                   int64_t Nq, const double *Xq, double *Yq)
{
    if (!ctx) { set_error("pmk_query_mean: ctx is NULL"); return -1; }
    if (!kernel_ok(th)) { set_error("pmk_query_mean: unknown kernel family"); return -2; }
    if (D < 1 || D > MAX_D) { set_error("pmk_query_mean: D=%d outside 1..%d", D, MAX_D); return -3; }
    if (n < 1 || !X || !c) { set_error("pmk_query_mean: empty model"); return -4; }
    if (Nq < 1 || !Xq || !Yq) { set_error("pmk_query_mean: empty query (the reference asserts !isempty(Xq))"); return -7; }
    PMK_HIP(hipSetDevice(ctx->device));
    std::vector<double> hx((size_t)(n * D));
    pack_soa(D, n, n, X, hx.data());
    DevTmp<double> dx, dc, dq, dy;
    if (dx.alloc(n * D) || dc.alloc(n) || dq.alloc(Nq * D) || dy.alloc(Nq)) return -100;
    PMK_HIP(hipMemcpyAsync(dx, hx.data(), sizeof(double) * hx.size(), hipMemcpyHostToDevice, ctx->stream));
    PMK_HIP(hipMemcpyAsync(dc, c, sizeof(double) * n, hipMemcpyHostToDevice, ctx->stream));
    PMK_HIP(hipMemcpyAsync(dq, Xq, sizeof(double) * Nq * D, hipMemcpyHostToDevice, ctx->stream));
    int rc = launch_query_mean(th, 1, D, n, dx, n, dc, Nq, dq, dy, ctx->stream);
    if (!rc) PMK_HIP(hipMemcpyAsync(Yq, dy, sizeof(double) * Nq, hipMemcpyDeviceToHost, ctx->stream));
    PMK_HIP(hipStreamSynchronize(ctx->stream));
    return rc;
}

int pmk_query_mean_multi(pmk_ctx *ctx, const pmk_kernel_desc *ths, int D, int64_t n, const double *X, const double *c,
                         int64_t Nq, const double *Xq, double *Yq)
{
    if (!ctx) { set_error("pmk_query_mean_multi: ctx is NULL"); return -1; }
    if (!ths) { set_error("pmk_query_mean_multi: no kernels"); return -2; }
    if (D < 1 || D > MAX_D) { set_error("pmk_query_mean_multi: D=%d outside 1..%d", D, MAX_D); return -3; }
    if (n < 1 || !X || !c) { set_error("pmk_query_mean_multi: empty model"); return -4; }
    for (int64_t i = 0; i < n; ++i)
        if (!kernel_ok(ths + i)) { set_error("pmk_query_mean_multi: unknown kernel family at centre %lld", (long long)i); return -2; }
    if (Nq < 1 || !Xq || !Yq) { set_error("pmk_query_mean_multi: empty query (the reference asserts !isempty(Xq))"); return -7; }
    PMK_HIP(hipSetDevice(ctx->device));
    std::vector<double> hx((size_t)(n * D));
    pack_soa(D, n, n, X, hx.data());
    DevTmp<double> dx, dc, dq, dy;
    DevTmp<pmk_kernel_desc> dth;
    if (dx.alloc(n * D) || dc.alloc(n) || dq.alloc(Nq * D) || dy.alloc(Nq) || dth.alloc(n)) return -100;
    PMK_HIP(hipMemcpyAsync(dx, hx.data(), sizeof(double) * hx.size(), hipMemcpyHostToDevice, ctx->stream));
    PMK_HIP(hipMemcpyAsync(dc, c, sizeof(double) * n, hipMemcpyHostToDevice, ctx->stream));
    PMK_HIP(hipMemcpyAsync(dq, Xq, sizeof(double) * Nq * D, hipMemcpyHostToDevice, ctx->stream));
    PMK_HIP(hipMemcpyAsync(dth, ths, sizeof(pmk_kernel_desc) * n, hipMemcpyHostToDevice, ctx->stream));
    int rc = n == 1 ? launch_query_mean(ths, 1, D, n, dx, n, dc, Nq, dq, dy, ctx->stream)
                    : launch_query_mean(dth, (int)n, D, n, dx, n, dc, Nq, dq, dy, ctx->stream);
    if (!rc) PMK_HIP(hipMemcpyAsync(Yq, dy, sizeof(double) * Nq, hipMemcpyDeviceToHost, ctx->stream));
    PMK_HIP(hipStreamSynchronize(ctx->stream));
    return rc;
}

int pmk_model_queryinner(pmk_model *m, int64_t patch, const pmk_kernel_desc *th, int64_t Nq, const double *Xq,
                         double *mu, double *var)
{
    return pmk_model_queryinner_ex(m, patch, th, Nq, Xq, 1e-12, mu, var);
}

int pmk_model_queryinner_ex(pmk_model *m, int64_t patch, const pmk_kernel_desc *th, int64_t Nq, const double *Xq,
                            double min_v, double *mu, double *var)
{
    if (!m || !m->fitted) { set_error("pmk_model_queryinner: model is not fitted"); return -1; }
    if (patch < 0 || patch >= m->P) { set_error("pmk_model_queryinner: patch %lld of %lld", (long long)patch, (long long)m->P); return -2; }
    if (!kernel_ok(th)) { set_error("pmk_model_queryinner: unknown kernel family"); return -3; }
    if (Nq < 1 || Nq > 0x7fffffff || !Xq || !mu || !var) { set_error("pmk_model_queryinner: empty query"); return -4; }
    pmk_ctx *c = m->ctx;
    PMK_HIP(hipSetDevice(c->device));
    // a plan by hand: every query is one item of region `patch`, already "sorted"
    pmk_query q;
    q.m = m; q.Nq = Nq; q.total = Nq; q.min_v = min_v;
    int rc = 0;
    rc |= dev_alloc(&q.d_xq, Nq * m->D);
    rc |= dev_alloc(&q.d_sorted_item, Nq);
    rc |= dev_alloc(&q.d_u, Nq);
    rc |= dev_alloc(&q.d_v, Nq);
    if (!rc) {
        q.d_item_query = q.d_sorted_item;            // both are the identity permutation
        q.roff.assign((size_t)(m->leaf_base + m->P + 1), 0);
        for (int64_t r = m->leaf_base + patch + 1; r <= m->leaf_base + m->P; ++r) q.roff[(size_t)r] = Nq;
        if (hipMemcpyAsync(q.d_xq, Xq, sizeof(double) * (size_t)(Nq * m->D), hipMemcpyHostToDevice, c->stream) != hipSuccess) rc = -100;
        if (!rc) rc = launch_iota(q.d_sorted_item, Nq, c->stream);
        if (!rc) rc = PMK_BY_DTYPE(m, build_strip_tasks(&q, c->stream));
        if (!rc) rc = PMK_BY_DTYPE(m, launch_items(&q, th, c->stream));
        if (!rc && (hipMemcpyAsync(mu, q.d_u, sizeof(double) * (size_t)Nq, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
                    hipMemcpyAsync(var, q.d_v, sizeof(double) * (size_t)Nq, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
                    hipStreamSynchronize(c->stream) != hipSuccess)) {
            set_error("pmk_model_queryinner: copy back failed");
            rc = -100;
        }
    } else {
        rc = -100;
    }
    dev_free(q.d_xq); dev_free(q.d_sorted_item); dev_free(q.d_u); dev_free(q.d_v);
    if (q.d_tasks) (void)hipFree(q.d_tasks);
    if (q.d_sync) (void)hipFree(q.d_sync);
    q.d_item_query = nullptr;
    return rc;
}

// ------------------------------------------------------------------------------------------ the query object
void pmk_query_destroy(pmk_query *q)
{
    if (!q) return;
    // d_xq and d_item_t are the bases of the two arenas (query_reserve, grow_item_buffers): the other per-point and
    // per-item pointers live inside them
    dev_free(q->d_xq); dev_free(q->d_item_t); dev_free(q->d_qdiag); dev_free(q->d_roff); dev_free(q->d_flag);
    if (q->d_tmp) (void)hipFree(q->d_tmp);
    if (q->d_sort_scratch) (void)hipFree(q->d_sort_scratch);
    if (q->d_tasks) (void)hipFree(q->d_tasks);
    if (q->d_sync) (void)hipFree(q->d_sync);
    dev_free(q->d_um); dev_free(q->d_yqm); dev_free(q->d_mcpre); dev_free(q->d_gm); dev_free(q->d_dyq);
    dev_free(q->d_gv); dev_free(q->d_gh); dev_free(q->d_dvq); dev_free(q->d_vgpre);
    dev_free(q->d_cov_v); dev_free(q->d_cov_s); dev_free(q->d_cov); dev_free(q->d_cov_tasks); dev_free(q->d_cov_pairs);
    dev_free(q->d_cov_goff); dev_free(q->d_cov_z); dev_free(q->d_cov_flags);
    dev_free(q->d_cov_f); dev_free(q->d_fdesc); dev_free(q->d_forder); dev_free(q->d_ftasks); dev_free(q->d_finfo);
    dev_free(q->d_fact); dev_free(q->d_fjit); dev_free(q->d_frel); dev_free(q->d_draw_t); dev_free(q->d_draw_z);
    dev_free(q->d_draw_e);
    dev_free(q->d_blk_group); dev_free(q->d_blk_a); dev_free(q->d_blk_gq); dev_free(q->d_blk_w); dev_free(q->d_blk_head);
    dev_free(q->d_blk_agg_of); dev_free(q->d_blk_scan); dev_free(q->d_blk_aggs); dev_free(q->d_blk_piece);
    dev_free(q->d_blk_tasks); dev_free(q->d_blk_aoff); dev_free(q->d_blk_y); dev_free(q->d_blk_v);
    dev_free(q->d_loo_x);              // base of the leave-one-out arena (loo_reserve)
    pmk_query_destroy(q->loo_inner);
    delete q;
}

int pmk_query_create(pmk_model *m, int64_t Nq, const double *Xq, pmk_query **out)
{
    if (!out) { set_error("pmk_query_create: out is NULL"); return -4; }
    *out = nullptr;
    if (!m) { set_error("pmk_query_create: model is NULL"); return -1; }
    if (Nq < 0 || Nq > 0x7fffffff || (Nq > 0 && !Xq)) { set_error("pmk_query_create: bad Nq"); return -2; }
    if (m->P_global == 0) { set_error("pmk_query_create: attach a tree with pmk_model_set_bsp first"); return -1; }
    PMK_HIP(hipSetDevice(m->ctx->device));
    pmk_query *q = new (std::nothrow) pmk_query();
    if (!q) { set_error("out of memory"); return -100; }
    q->m = m; q->Nq = Nq; q->roff_P = m->P_global;
    int rc = query_reserve(q, std::max<int64_t>(Nq, 1));
    rc |= dev_alloc(&q->d_roff, m->P_global + 1);
    if (rc) { pmk_query_destroy(q); return -100; }
    if (Nq > 0) PMK_HIP(hipMemcpy(q->d_xq, Xq, sizeof(double) * (size_t)(Nq * m->D), hipMemcpyDefault));
    *out = q;
    return 0;
}

int pmk_query_create_items(pmk_model *m, int64_t n, const double *xq, const int32_t *region, pmk_query **out)
{
    if (!out) { set_error("pmk_query_create_items: out is NULL"); return -4; }
    *out = nullptr;
    if (n > 0 && (!region || !xq)) { set_error("pmk_query_create_items: NULL points or regions"); return -2; }
    pmk_query *q = nullptr;
    int rc = pmk_query_create(m, 0, nullptr, &q);
    if (rc) return rc;
    if ((rc = query_set_items(q, n, xq, region))) { pmk_query_destroy(q); return rc; }
    *out = q;
    return 0;
}

int pmk_query_set_diag(pmk_query *q, const double *diag)
{
    if (!q) { set_error("pmk_query_set_diag: query is NULL"); return -1; }
    pmk_ctx *c = q->m->ctx;
    PMK_HIP(hipSetDevice(c->device));
    PMK_HIP(hipStreamSynchronize(c->stream));
    dev_free(q->d_qdiag);
    if (!diag || q->Nq == 0) return 0;
    if (dev_alloc(&q->d_qdiag, q->Nq)) return -100;
    PMK_HIP(hipMemcpy(q->d_qdiag, diag, sizeof(double) * (size_t)q->Nq, hipMemcpyDefault));   // host or device
    return 0;
}

int pmk_query_export_requests(pmk_query *q, int64_t first, int64_t n, double *xq_dev, int32_t *region_dev)
{
    if (!q || !q->planned) { set_error("pmk_query_export_requests: query is not planned"); return -1; }
    if (first < 0 || n < 0 || first + n > q->total) { set_error("pmk_query_export_requests: bad item range"); return -3; }
    if (n > 0 && (!xq_dev || !region_dev)) { set_error("pmk_query_export_requests: NULL output"); return -2; }
    pmk_ctx *c = q->m->ctx;
    PMK_HIP(hipSetDevice(c->device));
    return launch_export_requests(q, first, n, xq_dev, region_dev, c->stream);
}

int pmk_query_export_request_diag(pmk_query *q, int64_t first, int64_t n, double *diag_dev)
{
    if (!q || !q->planned) { set_error("pmk_query_export_request_diag: query is not planned"); return -1; }
    if (first < 0 || n < 0 || first + n > q->total) { set_error("pmk_query_export_request_diag: bad item range"); return -3; }
    if (n > 0 && !diag_dev) { set_error("pmk_query_export_request_diag: NULL output"); return -2; }
    pmk_ctx *c = q->m->ctx;
    PMK_HIP(hipSetDevice(c->device));
    if (int rc = launch_export_request_diag(q, first, n, diag_dev, c->stream)) return rc;
    return q->d_qdiag ? 1 : 0;
}

int pmk_query_export_results(pmk_query *q, double *u_dev, double *v_dev)
{
    if (!q || !q->planned) { set_error("pmk_query_export_results: query is not planned"); return -1; }
    pmk_ctx *c = q->m->ctx;
    PMK_HIP(hipSetDevice(c->device));
    return launch_export_results(q, u_dev, v_dev, c->stream);
}

int pmk_query_plan(pmk_query *q, double radius, double delta)
{
    if (!q) { set_error("pmk_query_plan: query is NULL"); return -1; }
    pmk_model *m = q->m;
    pmk_ctx *c = m->ctx;
    PMK_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    if (q->roff_P != m->P_global) {
        set_error("pmk_query_plan: the model's tree changed (%lld -> %lld leaves) after the query was created",
                  (long long)q->roff_P, (long long)m->P_global);
        return -4;
    }
    c->tic("plan");
    q->planned = false;
    reset_plan_state(q);
    q->explicit_items = false;
    q->total = 0;
    q->roff.assign((size_t)(m->P_global + 1), 0);
    if (q->Nq > 0) {
        int rc;
        PMK_HIP(hipMemsetAsync(q->d_cnt, 0, sizeof(int32_t) * (size_t)(q->Nq + 1), s));
        if ((rc = launch_plan_count(q, radius, delta, s))) return rc;
        if (exclusive_scan_i32_to_i64(q->d_cnt, q->d_qoff, q->Nq, &q->d_tmp, &q->tmp_bytes, s)) {
            set_error("pmk_query_plan: prefix scan failed");
            return -100;
        }
        PMK_HIP(hipMemcpyAsync(&q->total, q->d_qoff + q->Nq, sizeof(int64_t), hipMemcpyDeviceToHost, s));
        PMK_HIP(hipStreamSynchronize(s));
        if (q->total > 0x7fffffff) { set_error("pmk_query_plan: too many work items (%lld)", (long long)q->total); return -5; }
        if ((rc = grow_item_buffers(q, q->total))) return rc;
        if ((rc = launch_plan_fill(q, radius, delta, s))) return rc;
        if ((rc = launch_sort_items(q, s))) return rc;
        PMK_HIP(hipMemcpyAsync(q->roff.data(), q->d_roff, sizeof(int64_t) * q->roff.size(), hipMemcpyDeviceToHost, s));
        PMK_HIP(hipStreamSynchronize(s));
        if ((rc = PMK_BY_DTYPE(m, build_strip_tasks(q, s)))) return rc;
    }
    c->toc("plan");
    q->planned = true;
    return 0;
}

int pmk_query_counts(pmk_query *q, int64_t *total_items, int64_t *first_owned, int64_t *num_owned)
{
    if (!q || !q->planned) { set_error("pmk_query_counts: query is not planned"); return -1; }
    const pmk_model *m = q->m;
    if (total_items) *total_items = q->total;
    if (first_owned) *first_owned = q->roff[(size_t)m->leaf_base];
    if (num_owned) *num_owned = q->roff[(size_t)(m->leaf_base + m->P)] - q->roff[(size_t)m->leaf_base];
    return 0;
}

int pmk_query_region_offsets(pmk_query *q, int64_t *region_offsets)
{
    if (!q || !q->planned || !region_offsets) { set_error("pmk_query_region_offsets: query is not planned"); return -1; }
    std::memcpy(region_offsets, q->roff.data(), sizeof(int64_t) * q->roff.size());
    return 0;
}

// ------------------------------------------------------------------------------------------ single output
int pmk_query_items(pmk_query *q, const pmk_kernel_desc *th)
{
    if (!q || !q->planned) { set_error("pmk_query_items: query is not planned"); return -1; }
    if (!kernel_ok(th)) { set_error("pmk_query_items: unknown kernel family"); return -2; }
    if (!q->m->fitted) { set_error("pmk_query_items: model is not fitted"); return -1; }
    pmk_ctx *c = q->m->ctx;
    PMK_HIP(hipSetDevice(c->device));
    c->tic("items");
    int rc = PMK_BY_DTYPE(q->m, launch_items(q, th, c->stream));
    c->toc("items");
    return rc;
}

int pmk_query_items_fitted(pmk_query *q)
{
    if (!q || !q->planned) { set_error("pmk_query_items_fitted: query is not planned"); return -1; }
    pmk_model *m = q->m;
    if (!m->fitted) { set_error("pmk_query_items_fitted: model is not fitted"); return -1; }
    if (m->ths.empty()) { set_error("pmk_query_items_fitted: the model holds no kernels (pmk_model_set_kernels)"); return -3; }
    pmk_ctx *c = m->ctx;
    PMK_HIP(hipSetDevice(c->device));
    c->tic("items");
    int rc = PMK_BY_DTYPE(m, launch_items(q, fitted_theta(m), c->stream));
    c->toc("items");
    return rc;
}

int pmk_query_item_buffers(pmk_query *q, void **u_dev, void **v_dev)
{
    if (!q || !q->planned) { set_error("pmk_query_item_buffers: query is not planned"); return -1; }
    if (u_dev) *u_dev = q->d_u;
    if (v_dev) *v_dev = q->d_v;
    return 0;
}

int pmk_query_mix(pmk_query *q, const pmk_kernel_desc *weight_th, int64_t q0, int64_t q1)
{
    if (!q || !q->planned) { set_error("pmk_query_mix: query is not planned"); return -1; }
    if (int rc = blend_profile_ok(weight_th, "pmk_query_mix")) return rc;
    if (int rc = query_range_ok(q, q0, q1, "pmk_query_mix")) return rc;
    pmk_ctx *c = q->m->ctx;
    PMK_HIP(hipSetDevice(c->device));
    c->tic("mix");
    int rc = launch_mix(q, *weight_th, q0, q1, c->stream);
    c->toc("mix");
    return rc;
}

}  // extern "C"

// Yq and Vq of the last mix into host or device arrays (`kind`); only enqueues
static int fetch_common(pmk_query *q, double *Yq, double *Vq, hipMemcpyKind kind, const char *who)
{
    if (!q) { set_error("%s: query is NULL", who); return -1; }
    pmk_ctx *c = q->m->ctx;
    PMK_HIP(hipSetDevice(c->device));
    if (q->Nq > 0) {
        if (Yq) PMK_HIP(hipMemcpyAsync(Yq, q->d_yq, sizeof(double) * (size_t)q->Nq, kind, c->stream));
        if (Vq) PMK_HIP(hipMemcpyAsync(Vq, q->d_vq, sizeof(double) * (size_t)q->Nq, kind, c->stream));
    }
    return 0;
}

static int fetch_multi_common(pmk_query *q, double *Yq, int64_t ldyq, double *Vq, hipMemcpyKind kind, const char *who)
{
    if (!q) { set_error("%s: query is NULL", who); return -1; }
    if (!q->mixed_multi || q->R_items < 1) { set_error("%s: pmk_query_mix_multi has not run", who); return -2; }
    if (Vq && !q->var_items) {
        set_error("%s: Vq was not computed (pmk_query_items_multi ran with want_var = 0)", who);
        return -3;
    }
    if (Yq && ldyq < q->Nq) { set_error("%s: ldyq = %lld < Nq = %lld", who, (long long)ldyq, (long long)q->Nq); return -4; }
    pmk_ctx *c = q->m->ctx;
    PMK_HIP(hipSetDevice(c->device));
    if (q->Nq > 0) {
        if (Yq)
            PMK_HIP(hipMemcpy2DAsync(Yq, sizeof(double) * (size_t)ldyq, q->d_yqm, sizeof(double) * (size_t)q->Nq,
                                     sizeof(double) * (size_t)q->Nq, (size_t)q->R_items, kind, c->stream));
        if (Vq) PMK_HIP(hipMemcpyAsync(Vq, q->d_vq, sizeof(double) * (size_t)q->Nq, kind, c->stream));
    }
    return 0;
}

static int fetch_vgrad_common(pmk_query *q, double *dVq, int64_t lddv, hipMemcpyKind kind, const char *who)
{
    if (!q) { set_error("%s: query is NULL", who); return -1; }
    if (!q->mixed_vgrad || !q->vgrad_items) { set_error("%s: pmk_query_mix_vgrad has not run", who); return -2; }
    if (!dVq) { set_error("%s: dVq is NULL", who); return -2; }
    if (lddv < q->Nq) { set_error("%s: lddv = %lld < Nq = %lld", who, (long long)lddv, (long long)q->Nq); return -4; }
    pmk_ctx *c = q->m->ctx;
    PMK_HIP(hipSetDevice(c->device));
    if (q->Nq > 0)
        PMK_HIP(hipMemcpy2DAsync(dVq, sizeof(double) * (size_t)lddv, q->d_dvq, sizeof(double) * (size_t)q->Nq,
                                 sizeof(double) * (size_t)q->Nq, (size_t)q->m->D, kind, c->stream));
    return 0;
}

static int fetch_grad_common(pmk_query *q, double *dYq, int64_t lddy, hipMemcpyKind kind, const char *who)
{
    if (!q) { set_error("%s: query is NULL", who); return -1; }
    if (!q->mixed_grad || !q->grad_items) { set_error("%s: pmk_query_mix_grad has not run", who); return -2; }
    if (!dYq) { set_error("%s: dYq is NULL", who); return -2; }
    if (lddy < q->Nq) { set_error("%s: lddy = %lld < Nq = %lld", who, (long long)lddy, (long long)q->Nq); return -4; }
    pmk_ctx *c = q->m->ctx;
    PMK_HIP(hipSetDevice(c->device));
    if (q->Nq > 0)
        PMK_HIP(hipMemcpy2DAsync(dYq, sizeof(double) * (size_t)lddy, q->d_dyq, sizeof(double) * (size_t)q->Nq,
                                 sizeof(double) * (size_t)q->Nq, (size_t)(q->m->D * q->R_items), kind, c->stream));
    return 0;
}

extern "C" {

int pmk_query_fetch(pmk_query *q, double *Yq, double *Vq)
{
    if (int rc = fetch_common(q, Yq, Vq, hipMemcpyDeviceToHost, "pmk_query_fetch")) return rc;
    PMK_HIP(hipStreamSynchronize(q->m->ctx->stream));
    return 0;
}

int pmk_query_fetch_dev(pmk_query *q, double *Yq_dev, double *Vq_dev)
{
    return fetch_common(q, Yq_dev, Vq_dev, hipMemcpyDeviceToDevice, "pmk_query_fetch_dev");
}

int pmk_query_debug(pmk_query *q, int64_t *home, int64_t *item_offsets, int64_t *item_region, double *item_t,
                    double *item_w, double *item_u, double *item_v)
{
    if (!q || !q->planned) { set_error("pmk_query_debug: query is not planned"); return -1; }
    pmk_ctx *c = q->m->ctx;
    PMK_HIP(hipSetDevice(c->device));
    PMK_HIP(hipStreamSynchronize(c->stream));
    const size_t Nq = (size_t)q->Nq, T = (size_t)q->total;
    if (home && Nq) {
        std::vector<int32_t> h(Nq);
        PMK_HIP(hipMemcpy(h.data(), q->d_home, sizeof(int32_t) * Nq, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < Nq; ++i) home[i] = h[i];
    }
    if (item_offsets) PMK_HIP(hipMemcpy(item_offsets, q->d_qoff, sizeof(int64_t) * (Nq + 1), hipMemcpyDeviceToHost));
    if (T == 0) return 0;
    if (item_region) {
        std::vector<int32_t> r(T);
        PMK_HIP(hipMemcpy(r.data(), q->d_item_region, sizeof(int32_t) * T, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < T; ++i) item_region[i] = r[i];
    }
    if (item_t) PMK_HIP(hipMemcpy(item_t, q->d_item_t, sizeof(double) * T, hipMemcpyDeviceToHost));
    if (item_w) PMK_HIP(hipMemcpy(item_w, q->d_w, sizeof(double) * T, hipMemcpyDeviceToHost));
    if (item_u)
        if (int rc = download_item_rows(q, q->d_u, 1, 1, item_u, 1)) return rc;
    if (item_v)
        if (int rc = download_item_rows(q, q->d_v, 1, 1, item_v, 1)) return rc;
    return 0;
}

int pmk_predict_mixture(pmk_model *m, const pmk_kernel_desc *th, const pmk_kernel_desc *weight_th, int64_t Nq,
                        const double *Xq, double radius, double delta, double *Yq, double *Vq)
{
    if (!m) { set_error("pmk_predict_mixture: model is NULL"); return -1; }
    if (int rc = whole_tree_ok(m, "pmk_predict_mixture", USE_STAGED, -1)) return rc;
    return one_shot(m, Nq, Xq, radius, delta, [&](pmk_query *q) { return pmk_query_items(q, th); },
                    [&](pmk_query *q) { return pmk_query_mix(q, weight_th, 0, Nq); },
                    [&](pmk_query *q) { return pmk_query_fetch(q, Yq, Vq); });
}

int pmk_predict_mixture_fitted(pmk_model *m, const pmk_kernel_desc *weight_th, int64_t Nq, const double *Xq, double radius,
                               double delta, double *Yq, double *Vq)
{
    if (!m) { set_error("pmk_predict_mixture_fitted: model is NULL"); return -1; }
    if (int rc = whole_tree_ok(m, "pmk_predict_mixture_fitted", USE_STAGED, -1)) return rc;
    return one_shot(m, Nq, Xq, radius, delta, pmk_query_items_fitted,
                    [&](pmk_query *q) { return pmk_query_mix(q, weight_th, 0, Nq); },
                    [&](pmk_query *q) { return pmk_query_fetch(q, Yq, Vq); });
}

}  // extern "C"

// ------------------------------------------------------------------------------------------ multi-output targets
// th == NULL: the model's own per-patch kernels (pmk_query_items_multi_fitted)
static int items_multi_common(pmk_query *q, const pmk_kernel_desc *th, int want_var)
{
    pmk_model *m = q->m;
    if (int rc = whole_tree_ok(m, "pmk_query_items_multi", MULTI_NEEDS_ALL, -4)) return rc;
    if (!m->multi_solved) { set_error("pmk_query_items_multi: pmk_model_solve_multi has not run"); return -3; }
    if (want_var && !m->fitted) { set_error("pmk_query_items_multi: model is not fitted"); return -3; }
    pmk_ctx *c = m->ctx;
    PMK_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const int R = m->R_multi, qt = m->trend_q;      // with a trend the items kernel also emits kq . C_H: R + q columns
    reset_item_state(q);
    multi_chunk_prefix(q);
    PMK_HIP(hipStreamSynchronize(s));       // earlier launches may still read the buffers replaced below
    if (grow(q->d_mcpre, q->mcpre_cap, m->P + 1, s) || grow(q->d_um, q->um_cap, q->total * (R + qt), s)) return -100;
    PMK_HIP(hipMemcpyAsync(q->d_mcpre, q->mcpre.data(), sizeof(int64_t) * q->mcpre.size(), hipMemcpyHostToDevice, s));
    q->R_items = R;
    q->um_ld = R + qt;
    c->tic("items_multi");
    int rc = PMK_BY_DTYPE(m, launch_items_multi(q, th, s));
    // v exactly as pmk_query_items / pmk_query_items_fitted (u ignored)
    if (!rc && want_var) rc = PMK_BY_DTYPE(m, launch_items(q, th, s));
    c->toc("items_multi");
    // mu += h^T beta and, after the clamp of v at min_v, v += |L_G^-1 (h - kq . C_H)|^2
    if (!rc && qt > 0) {
        c->tic("trend_items");
        rc = launch_trend_items(q, R, qt, want_var != 0, s);
        c->toc("trend_items");
    }
    if (rc) { q->R_items = 0; return rc; }
    q->var_items = want_var != 0;
    q->items_fn = true;
    return 0;
}

extern "C" {

int pmk_query_items_multi(pmk_query *q, const pmk_kernel_desc *th, int want_var)
{
    if (!q || !q->planned) { set_error("pmk_query_items_multi: query is not planned"); return -1; }
    if (!kernel_ok(th)) { set_error("pmk_query_items_multi: unknown kernel family"); return -2; }
    return items_multi_common(q, th, want_var);
}

int pmk_query_items_multi_fitted(pmk_query *q, int want_var)
{
    if (!q || !q->planned) { set_error("pmk_query_items_multi_fitted: query is not planned"); return -1; }
    pmk_model *m = q->m;
    if (m->ths.empty()) { set_error("pmk_query_items_multi_fitted: the model holds no kernels (pmk_model_set_kernels)"); return -3; }
    return items_multi_common(q, fitted_theta(m), want_var);
}

int pmk_query_mix_multi(pmk_query *q, const pmk_kernel_desc *weight_th, int64_t q0, int64_t q1)
{
    if (!q || !q->planned) { set_error("pmk_query_mix_multi: query is not planned"); return -1; }
    if (q->R_items < 1) { set_error("pmk_query_mix_multi: pmk_query_items_multi has not run on this plan"); return -1; }
    if (int rc = blend_profile_ok(weight_th, "pmk_query_mix_multi")) return rc;
    if (int rc = query_range_ok(q, q0, q1, "pmk_query_mix_multi")) return rc;
    pmk_ctx *c = q->m->ctx;
    PMK_HIP(hipSetDevice(c->device));
    if (int rc = grow(q->d_yqm, q->yqm_cap, q->Nq * q->R_items, c->stream)) return rc;
    c->tic("mix_multi");
    int rc = q->var_items ? launch_mix(q, *weight_th, q0, q1, c->stream) : 0;     // Vq exactly as pmk_query_mix
    if (!rc) rc = launch_mix_multi(q, *weight_th, q0, q1, c->stream);
    c->toc("mix_multi");
    if (rc) return rc;
    q->mixed_multi = true;
    return 0;
}

int pmk_query_fetch_multi(pmk_query *q, double *Yq, int64_t ldyq, double *Vq)
{
    if (int rc = fetch_multi_common(q, Yq, ldyq, Vq, hipMemcpyDeviceToHost, "pmk_query_fetch_multi")) return rc;
    PMK_HIP(hipStreamSynchronize(q->m->ctx->stream));
    return 0;
}

int pmk_query_fetch_multi_dev(pmk_query *q, double *Yq_dev, int64_t ldyq, double *Vq_dev)
{
    return fetch_multi_common(q, Yq_dev, ldyq, Vq_dev, hipMemcpyDeviceToDevice, "pmk_query_fetch_multi_dev");
}

int pmk_predict_mixture_multi(pmk_model *m, const pmk_kernel_desc *th, const pmk_kernel_desc *weight_th, int64_t Nq,
                              const double *Xq, double radius, double delta, double *Yq, int64_t ldyq, double *Vq)
{
    if (!m) { set_error("pmk_predict_mixture_multi: model is NULL"); return -1; }
    if (int rc = whole_tree_ok(m, "pmk_predict_mixture_multi", MULTI_NEEDS_ALL, -4)) return rc;
    if (Yq && ldyq < Nq) { set_error("pmk_predict_mixture_multi: ldyq = %lld < Nq = %lld", (long long)ldyq, (long long)Nq); return -4; }
    return one_shot(m, Nq, Xq, radius, delta, [&](pmk_query *q) { return pmk_query_items_multi(q, th, Vq != nullptr); },
                    [&](pmk_query *q) { return pmk_query_mix_multi(q, weight_th, 0, Nq); },
                    [&](pmk_query *q) { return pmk_query_fetch_multi(q, Yq, ldyq, Vq); });
}

int pmk_predict_mixture_multi_fitted(pmk_model *m, const pmk_kernel_desc *weight_th, int64_t Nq, const double *Xq,
                                     double radius, double delta, double *Yq, int64_t ldyq, double *Vq)
{
    if (!m) { set_error("pmk_predict_mixture_multi_fitted: model is NULL"); return -1; }
    if (int rc = whole_tree_ok(m, "pmk_predict_mixture_multi_fitted", MULTI_NEEDS_ALL, -4)) return rc;
    if (Yq && ldyq < Nq) { set_error("pmk_predict_mixture_multi_fitted: ldyq = %lld < Nq = %lld", (long long)ldyq, (long long)Nq); return -4; }
    return one_shot(m, Nq, Xq, radius, delta, [&](pmk_query *q) { return pmk_query_items_multi_fitted(q, Vq != nullptr); },
                    [&](pmk_query *q) { return pmk_query_mix_multi(q, weight_th, 0, Nq); },
                    [&](pmk_query *q) { return pmk_query_fetch_multi(q, Yq, ldyq, Vq); });
}

int pmk_query_get_items_multi(pmk_query *q, double *U, int64_t ldu, double *v)
{
    if (!q || !q->planned) { set_error("pmk_query_get_items_multi: query is not planned"); return -1; }
    if (q->R_items < 1) { set_error("pmk_query_get_items_multi: pmk_query_items_multi has not run on this plan"); return -2; }
    if (v && !q->var_items) {
        set_error("pmk_query_get_items_multi: v was not computed (the items ran with want_var = 0)");
        return -3;
    }
    if (U && ldu < q->R_items) {
        set_error("pmk_query_get_items_multi: ldu = %lld < R = %d", (long long)ldu, q->R_items);
        return -4;
    }
    pmk_ctx *c = q->m->ctx;
    PMK_HIP(hipSetDevice(c->device));
    PMK_HIP(hipStreamSynchronize(c->stream));
    if (q->total == 0) return 0;
    if (U)
        if (int rc = download_item_rows(q, q->d_um, (size_t)q->um_ld, (size_t)q->R_items, U, (size_t)ldu)) return rc;
    if (v)
        if (int rc = download_item_rows(q, q->d_v, 1, 1, v, 1)) return rc;
    return 0;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------ gradient of the blended mean
static const char *family_name(int family)
{
    switch (family) {
    case PMK_SPLINE34: return "PMK_SPLINE34";
    case PMK_SPLINE12: return "PMK_SPLINE12";
    case PMK_SPLINE32: return "PMK_SPLINE32";
    case PMK_GAUSSIAN: return "PMK_GAUSSIAN";
    case PMK_RQ: return "PMK_RQ";
    case PMK_TRQ: return "PMK_TRQ";
    case PMK_MODSQEXP: return "PMK_MODSQEXP";
    case PMK_BB10: return "PMK_BB10";
    case PMK_BB20: return "PMK_BB20";
    case PMK_BB1EPS: return "PMK_BB1EPS";
    case PMK_BB2EPS: return "PMK_BB2EPS";
    default: return "unknown";
    }
}

// a kernel whose profile has a psi = phi' / tau (pmk_device.h): stationary, and ModSqExp only at D = 1
static int grad_kernel_ok(const pmk_kernel_desc *th, int D, const char *who, const char *role)
{
    if (!kernel_ok(th)) { set_error("%s: unknown kernel family (%s)", who, role); return -2; }
    if (th->family >= PMK_BB10) {
        set_error("%s: %s is a Brownian-bridge family (%s, %d): not differentiable on the diagonal, no gradient", who, role,
                  family_name(th->family), th->family);
        return -2;
    }
    if (th->family == PMK_MODSQEXP && D > 1) {
        set_error("%s: %s is PMK_MODSQEXP, which is defined for D = 1 only (D = %d)", who, role, D);
        return -2;
    }
    return 0;
}

extern "C" {

int pmk_query_items_grad(pmk_query *q, const pmk_kernel_desc *th)
{
    if (!q || !q->planned) { set_error("pmk_query_items_grad: query is not planned"); return -1; }
    pmk_model *m = q->m;
    if (int rc = whole_tree_ok(m, "pmk_query_items_grad", GRAD_NEEDS_ALL, -4)) return rc;
    if (!m->multi_solved) {
        set_error("pmk_query_items_grad: pmk_model_solve_multi has not run on the resident factor");
        return -3;
    }
    if (q->R_items < 1 || !q->items_fn) {
        set_error("pmk_query_items_grad: the last items on this plan must be those of pmk_query_items_multi or "
                  "_multi_fitted (a member item of pmk_query_items_loo_multi is a lookup, not a function of x)");
        return -2;
    }
    if (th) {
        if (int rc = grad_kernel_ok(th, m->D, "pmk_query_items_grad", "theta")) return rc;
    } else {
        if (m->ths.empty()) { set_error("pmk_query_items_grad: the model holds no kernels (pmk_model_set_kernels)"); return -3; }
        for (size_t r = 0; r < m->ths.size(); ++r)
            if (int rc = grad_kernel_ok(&m->ths[r], m->D, "pmk_query_items_grad", "the model's own theta")) return rc;
        th = fitted_theta(m);
    }
    pmk_ctx *c = m->ctx;
    PMK_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    q->grad_items = q->mixed_grad = false;
    if (int rc = grow(q->d_gm, q->gm_cap, q->total * m->D * q->R_items, s)) return rc;
    c->tic("items_grad");
    const int rc = PMK_BY_DTYPE(m, launch_items_grad(q, th, s));
    c->toc("items_grad");
    if (rc) return rc;
    q->grad_items = true;
    return 0;
}

int pmk_query_mix_grad(pmk_query *q, const pmk_kernel_desc *weight_th, int64_t q0, int64_t q1)
{
    if (!q || !q->planned) { set_error("pmk_query_mix_grad: query is not planned"); return -1; }
    if (!q->grad_items || q->R_items < 1) { set_error("pmk_query_mix_grad: pmk_query_items_grad has not run on this plan"); return -2; }
    if (int rc = grad_kernel_ok(weight_th, 1, "pmk_query_mix_grad", "the blending profile")) return rc;
    if (int rc = query_range_ok(q, q0, q1, "pmk_query_mix_grad")) return rc;
    pmk_model *m = q->m;
    pmk_ctx *c = m->ctx;
    PMK_HIP(hipSetDevice(c->device));
    if (int rc = grow(q->d_dyq, q->dyq_cap, q->Nq * m->D * q->R_items, c->stream)) return rc;
    c->tic("mix_grad");
    const int rc = launch_mix_grad(q, *weight_th, q0, q1, c->stream);
    c->toc("mix_grad");
    if (rc) return rc;
    q->mixed_grad = true;
    return 0;
}

int pmk_query_fetch_grad(pmk_query *q, double *dYq, int64_t lddy)
{
    if (int rc = fetch_grad_common(q, dYq, lddy, hipMemcpyDeviceToHost, "pmk_query_fetch_grad")) return rc;
    PMK_HIP(hipStreamSynchronize(q->m->ctx->stream));
    return 0;
}

int pmk_query_fetch_grad_dev(pmk_query *q, double *dYq_dev, int64_t lddy)
{
    return fetch_grad_common(q, dYq_dev, lddy, hipMemcpyDeviceToDevice, "pmk_query_fetch_grad_dev");
}

int pmk_query_get_items_grad(pmk_query *q, double *G, int64_t ldg, int32_t *plane)
{
    if (!q || !q->planned) { set_error("pmk_query_get_items_grad: query is not planned"); return -1; }
    if (G && !q->grad_items) { set_error("pmk_query_get_items_grad: pmk_query_items_grad has not run on this plan"); return -2; }
    const size_t T = (size_t)q->total, DR = G ? (size_t)(q->m->D * q->R_items) : 0;
    if (G && ldg < (int64_t)DR) { set_error("pmk_query_get_items_grad: ldg = %lld < D R = %lld", (long long)ldg, (long long)DR); return -4; }
    pmk_ctx *c = q->m->ctx;
    PMK_HIP(hipSetDevice(c->device));
    PMK_HIP(hipStreamSynchronize(c->stream));
    if (T == 0) return 0;
    if (plane) PMK_HIP(hipMemcpy(plane, q->d_item_plane, sizeof(int32_t) * T, hipMemcpyDeviceToHost));
    if (G) return download_item_rows(q, q->d_gm, DR, DR, G, (size_t)ldg);
    return 0;
}

int pmk_predict_mixture_grad_fitted(pmk_model *m, const pmk_kernel_desc *weight_th, int64_t Nq, const double *Xq,
                                    double radius, double delta, double *Yq, int64_t ldyq, double *dYq, int64_t lddy)
{
    if (!m) { set_error("pmk_predict_mixture_grad_fitted: model is NULL"); return -1; }
    if (int rc = whole_tree_ok(m, "pmk_predict_mixture_grad_fitted", GRAD_NEEDS_ALL, -4)) return rc;
    if ((Yq && ldyq < Nq) || (dYq && lddy < Nq)) {
        set_error("pmk_predict_mixture_grad_fitted: ldyq = %lld or lddy = %lld < Nq = %lld", (long long)ldyq, (long long)lddy,
                  (long long)Nq);
        return -4;
    }
    return one_shot(
        m, Nq, Xq, radius, delta,
        [&](pmk_query *q) { int rc = pmk_query_items_multi_fitted(q, 0); return rc ? rc : pmk_query_items_grad(q, nullptr); },
        [&](pmk_query *q) { int rc = pmk_query_mix_multi(q, weight_th, 0, Nq); return rc ? rc : pmk_query_mix_grad(q, weight_th, 0, Nq); },
        [&](pmk_query *q) {
            int rc = Yq ? pmk_query_fetch_multi(q, Yq, ldyq, nullptr) : 0;
            return !rc && dYq ? pmk_query_fetch_grad(q, dYq, lddy) : rc;
        });
}

// ------------------------------------------------------------------------------------------ gradient of the blended variance
int pmk_query_items_vgrad(pmk_query *q, const pmk_kernel_desc *th)
{
    if (!q || !q->planned) { set_error("pmk_query_items_vgrad: query is not planned"); return -1; }
    pmk_model *m = q->m;
    if (int rc = whole_tree_ok(m, "pmk_query_items_vgrad", GRAD_NEEDS_ALL, -4)) return rc;
    if (!m->multi_solved) {
        set_error("pmk_query_items_vgrad: pmk_model_solve_multi has not run on the resident factor");
        return -3;
    }
    if (q->R_items < 1 || !q->items_fn || !q->var_items) {
        set_error("pmk_query_items_vgrad: the last items on this plan must be those of pmk_query_items_multi or "
                  "_multi_fitted with want_var = 1 (a member item of pmk_query_items_loo_multi is a lookup, not a function "
                  "of x)");
        return -2;
    }
    if (q->d_qdiag) {
        set_error("pmk_query_items_vgrad: the query carries pmk_query_set_diag addends, whose dependence on x the library "
                  "does not know");
        return -2;
    }
    if (th) {
        if (int rc = grad_kernel_ok(th, m->D, "pmk_query_items_vgrad", "theta")) return rc;
    } else {
        if (m->ths.empty()) { set_error("pmk_query_items_vgrad: the model holds no kernels (pmk_model_set_kernels)"); return -3; }
        for (size_t r = 0; r < m->ths.size(); ++r)
            if (int rc = grad_kernel_ok(&m->ths[r], m->D, "pmk_query_items_vgrad", "the model's own theta")) return rc;
        th = fitted_theta(m);
    }
    pmk_ctx *c = m->ctx;
    PMK_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    q->vgrad_items = q->mixed_vgrad = false;
    // strips per region: the host prefix the kernel finds its region by (q->vgpre stays: it is the source of the upload)
    const int64_t cap = vgrad_strip_items(m->D);
    q->vgpre.assign((size_t)m->P + 1, 0);
    for (int64_t r = 0; r < m->P; ++r)
        q->vgpre[(size_t)r + 1] = q->vgpre[(size_t)r] + (q->roff[(size_t)r + 1] - q->roff[(size_t)r] + cap - 1) / cap;
    q->vstrips = q->vgpre[(size_t)m->P];
    if (int rc = grow(q->d_vgpre, q->vgpre_cap, m->P + 1, s)) return rc;
    if (int rc = grow(q->d_gv, q->gv_cap, q->total * m->D, s)) return rc;
    if (int rc = grow(q->d_gh, q->gh_cap, q->total * m->D * m->trend_q, s)) return rc;
    PMK_HIP(hipMemcpyAsync(q->d_vgpre, q->vgpre.data(), sizeof(int64_t) * q->vgpre.size(), hipMemcpyHostToDevice, s));
    c->tic("items_vgrad");
    int rc = PMK_BY_DTYPE(m, launch_items_vgrad(q, th, s));
    if (!rc) rc = launch_trend_vgrad(q, s);
    c->toc("items_vgrad");
    if (rc) return rc;
    q->vgrad_items = true;
    return 0;
}

int pmk_query_mix_vgrad(pmk_query *q, const pmk_kernel_desc *weight_th, int64_t q0, int64_t q1)
{
    if (!q || !q->planned) { set_error("pmk_query_mix_vgrad: query is not planned"); return -1; }
    if (!q->vgrad_items || !q->var_items) { set_error("pmk_query_mix_vgrad: pmk_query_items_vgrad has not run on this plan"); return -2; }
    if (int rc = grad_kernel_ok(weight_th, 1, "pmk_query_mix_vgrad", "the blending profile")) return rc;
    if (int rc = query_range_ok(q, q0, q1, "pmk_query_mix_vgrad")) return rc;
    pmk_model *m = q->m;
    pmk_ctx *c = m->ctx;
    PMK_HIP(hipSetDevice(c->device));
    if (int rc = grow(q->d_dvq, q->dvq_cap, q->Nq * m->D, c->stream)) return rc;
    c->tic("mix_vgrad");
    const int rc = launch_mix_vgrad(q, *weight_th, q0, q1, c->stream);
    c->toc("mix_vgrad");
    if (rc) return rc;
    q->mixed_vgrad = true;
    return 0;
}

int pmk_query_fetch_vgrad(pmk_query *q, double *dVq, int64_t lddv)
{
    if (int rc = fetch_vgrad_common(q, dVq, lddv, hipMemcpyDeviceToHost, "pmk_query_fetch_vgrad")) return rc;
    PMK_HIP(hipStreamSynchronize(q->m->ctx->stream));
    return 0;
}

int pmk_query_fetch_vgrad_dev(pmk_query *q, double *dVq_dev, int64_t lddv)
{
    return fetch_vgrad_common(q, dVq_dev, lddv, hipMemcpyDeviceToDevice, "pmk_query_fetch_vgrad_dev");
}

int pmk_query_get_items_vgrad(pmk_query *q, double *GV, int64_t ldg)
{
    if (!q || !q->planned) { set_error("pmk_query_get_items_vgrad: query is not planned"); return -1; }
    if (!q->vgrad_items) { set_error("pmk_query_get_items_vgrad: pmk_query_items_vgrad has not run on this plan"); return -2; }
    if (!GV) { set_error("pmk_query_get_items_vgrad: GV is NULL"); return -2; }
    const size_t D = (size_t)q->m->D;
    if (ldg < (int64_t)D) { set_error("pmk_query_get_items_vgrad: ldg = %lld < D = %lld", (long long)ldg, (long long)D); return -4; }
    pmk_ctx *c = q->m->ctx;
    PMK_HIP(hipSetDevice(c->device));
    PMK_HIP(hipStreamSynchronize(c->stream));
    if (q->total == 0) return 0;
    return download_item_rows(q, q->d_gv, D, D, GV, (size_t)ldg);
}

int pmk_predict_mixture_vgrad_fitted(pmk_model *m, const pmk_kernel_desc *weight_th, int64_t Nq, const double *Xq,
                                     double radius, double delta, double *Yq, int64_t ldyq, double *Vq, double *dYq,
                                     int64_t lddy, double *dVq, int64_t lddv)
{
    if (!m) { set_error("pmk_predict_mixture_vgrad_fitted: model is NULL"); return -1; }
    if (int rc = whole_tree_ok(m, "pmk_predict_mixture_vgrad_fitted", GRAD_NEEDS_ALL, -4)) return rc;
    if ((Yq && ldyq < Nq) || (dYq && lddy < Nq) || (dVq && lddv < Nq)) {
        set_error("pmk_predict_mixture_vgrad_fitted: ldyq = %lld, lddy = %lld or lddv = %lld < Nq = %lld", (long long)ldyq,
                  (long long)lddy, (long long)lddv, (long long)Nq);
        return -4;
    }
    return one_shot(
        m, Nq, Xq, radius, delta,
        [&](pmk_query *q) {
            int rc = pmk_query_items_multi_fitted(q, 1);
            if (!rc) rc = pmk_query_items_grad(q, nullptr);
            return rc ? rc : pmk_query_items_vgrad(q, nullptr);
        },
        [&](pmk_query *q) {
            int rc = pmk_query_mix_multi(q, weight_th, 0, Nq);
            if (!rc) rc = pmk_query_mix_grad(q, weight_th, 0, Nq);
            return rc ? rc : pmk_query_mix_vgrad(q, weight_th, 0, Nq);
        },
        [&](pmk_query *q) {
            int rc = (Yq || Vq) ? pmk_query_fetch_multi(q, Yq, ldyq, Vq) : 0;
            if (!rc && dYq) rc = pmk_query_fetch_grad(q, dYq, lddy);
            return !rc && dVq ? pmk_query_fetch_vgrad(q, dVq, lddv) : rc;
        });
}

}  // extern "C"

// ------------------------------------------------------------------------------------------ joint covariance of the batch
static const char COV_NEEDS_ALL[] = "the joint covariance needs a model that holds every leaf";

static int cov_batch_ok(int64_t Nq, const char *who)
{
    if (Nq > PMK_COV_MAX_QUERIES) {
        set_error("%s: %lld queries, the Nq x Nq result is limited to PMK_COV_MAX_QUERIES = %d", who, (long long)Nq,
                  PMK_COV_MAX_QUERIES);
        return -5;
    }
    return 0;
}

// The strips of the covariance sweep, the pairs of strips of a region and the offsets of the region blocks, from the
// plan's region offsets.  A region's items are dealt evenly over its strips, as build_strip_tasks (pmk_predict.hip)
// deals them.  Returns the elements of the V arena.
static int64_t cov_tasks_from_plan(pmk_query *q, std::vector<CovTask> &tasks, std::vector<CovPair> &pairs)
{
    const pmk_model *m = q->m;
    int64_t voff = 0;
    q->cov_goff.assign((size_t)m->P + 1, 0);
    for (int64_t r = 0; r < m->P; ++r) {
        const int64_t b = q->roff[(size_t)(m->leaf_base + r)], e = q->roff[(size_t)(m->leaf_base + r + 1)], mr = e - b;
        q->cov_goff[(size_t)r + 1] = q->cov_goff[(size_t)r] + mr * mr;
        if (mr == 0) continue;
        const int64_t nstrips = (mr + TQ - 1) / TQ, w = (mr + nstrips - 1) / nstrips;
        const size_t t0 = tasks.size();
        for (int64_t f = b; f < e; f += w) {
            CovTask t;
            t.region = (int32_t)r;
            t.count = (int32_t)std::min(e - f, w);
            t.first = f;
            t.voff = voff;
            t.goff = q->cov_goff[(size_t)r];
            t.m = (int32_t)mr;
            t.a0 = (int32_t)(f - b);
            tasks.push_back(t);
            voff += (int64_t)m->desc[(size_t)r].ld * TQ;
        }
        for (size_t ta = t0; ta < tasks.size(); ++ta)
            for (size_t tb = ta; tb < tasks.size(); ++tb) pairs.push_back({(int32_t)ta, (int32_t)tb});
    }
    return voff;
}

static int fetch_cov_common(pmk_query *q, double *Cov, int64_t ldc, hipMemcpyKind kind, const char *who)
{
    if (!q) { set_error("%s: query is NULL", who); return -1; }
    if (!q->mixed_cov || !q->cov_items) { set_error("%s: pmk_query_mix_cov has not run on this plan", who); return -2; }
    if (!Cov) { set_error("%s: Cov is NULL", who); return -2; }
    if (ldc < q->Nq) { set_error("%s: ldc = %lld < Nq = %lld", who, (long long)ldc, (long long)q->Nq); return -4; }
    pmk_ctx *c = q->m->ctx;
    PMK_HIP(hipSetDevice(c->device));
    if (q->Nq > 0)
        PMK_HIP(hipMemcpy2DAsync(Cov, sizeof(double) * (size_t)ldc, q->d_cov, sizeof(double) * (size_t)q->Nq,
                                 sizeof(double) * (size_t)q->Nq, (size_t)q->Nq, kind, c->stream));
    return 0;
}

// The region blocks of the current plan.  multi: the multi-output path (pmk_query_items_cov_multi), whose blocks carry the
// term z_a . z_b of the model's trend; its checks come before any launch, and with no trend in force it runs what the
// single-output call runs.  limit: refuse a batch above PMK_COV_MAX_QUERIES (the calls whose blocks feed the Nq x Nq result).
static int items_cov_common(pmk_query *q, const pmk_kernel_desc *th, bool multi, bool limit, const char *who)
{
    if (!q || !q->planned) { set_error("%s: query is not planned", who); return -1; }
    pmk_model *m = q->m;
    if (!m->fitted) { set_error("%s: the model holds no resident factor", who); return -1; }
    if (int rc = whole_tree_ok(m, who, COV_NEEDS_ALL, -3)) return rc;
    if (multi) {
        if (!m->multi_solved) {
            set_error("%s: pmk_model_solve_multi has not run on the resident factor (the multi-output weights are stale)", who);
            return -3;
        }
        if (q->R_items < 1 || !q->items_fn) {
            set_error("%s: the last items on this plan must be those of pmk_query_items_multi or _multi_fitted (a member "
                      "item of pmk_query_items_loo_multi is a lookup, not a function of x)", who);
            return -2;
        }
        if (q->um_ld - q->R_items != m->trend_q) {
            set_error("%s: the items were computed under a trend with q = %d, the model's has q = %d: run the items again",
                      who, q->um_ld - q->R_items, m->trend_q);
            return -2;
        }
    }
    const int qt = multi ? m->trend_q : 0;
    if (th) {
        if (int rc = cov_kernel_ok(th, m->D, who, "theta")) return rc;
    } else {
        if (m->ths.empty()) { set_error("%s: the model holds no kernels (pmk_model_set_kernels)", who); return -3; }
        for (size_t r = 0; r < m->ths.size(); ++r)
            if (int rc = cov_kernel_ok(&m->ths[r], m->D, who, "the model's own theta")) return rc;
        th = fitted_theta(m);
    }
    if (limit)
        if (int rc = cov_batch_ok(q->Nq, who)) return rc;
    pmk_ctx *c = m->ctx;
    PMK_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    q->cov_items = q->mixed_cov = q->cov_factored = false;
    q->cov_trend_q = 0;
    std::vector<CovTask> tasks;
    std::vector<CovPair> pairs;
    const int64_t velems = cov_tasks_from_plan(q, tasks, pairs);
    q->cov_ntasks = (int64_t)tasks.size();
    q->cov_npairs = (int64_t)pairs.size();
    if (int rc = grow_sized(q->d_cov_v, q->cov_v_cap, velems * (int64_t)m->esz, s, who, "the V arena")) return rc;
    if (int rc = grow_sized(q->d_cov_s, q->cov_s_cap, q->cov_goff[(size_t)m->P], s, who, "the region blocks")) return rc;
    if (int rc = grow_sized(q->d_cov_tasks, q->cov_tasks_cap, q->cov_ntasks, s, who, "the strip tasks")) return rc;
    if (int rc = grow_sized(q->d_cov_pairs, q->cov_pairs_cap, q->cov_npairs, s, who, "the strip pairs")) return rc;
    if (int rc = grow_sized(q->d_cov_goff, q->cov_goff_cap, m->P + 1, s, who, "the block offsets")) return rc;
    if (qt > 0) {
        if (int rc = grow_sized(q->d_cov_z, q->cov_z_cap, q->total * TQ_MAX, s, who, "the items' trend vectors")) return rc;
        if (int rc = grow_sized(q->d_cov_flags, q->cov_flags_cap, m->P, s, who, "the patch marks")) return rc;
    }
    PMK_HIP(hipMemcpyAsync(q->d_cov_goff, q->cov_goff.data(), sizeof(int64_t) * q->cov_goff.size(), hipMemcpyHostToDevice, s));
    if (!tasks.empty()) {
        PMK_HIP(hipMemcpyAsync(q->d_cov_tasks, tasks.data(), sizeof(CovTask) * tasks.size(), hipMemcpyHostToDevice, s));
        PMK_HIP(hipMemcpyAsync(q->d_cov_pairs, pairs.data(), sizeof(CovPair) * pairs.size(), hipMemcpyHostToDevice, s));
    }
    PMK_HIP(hipStreamSynchronize(s));       // `tasks` and `pairs` are locals
    c->tic("items_cov");
    int rc = PMK_BY_DTYPE(m, launch_items_cov(q, th, s));
    // S[a, b] += z_a . z_b, on the diagonal after the clamp at min_v
    if (!rc && qt > 0) {
        c->tic("cov_trend");
        rc = launch_cov_trend(q, s);
        c->toc("cov_trend");
    }
    c->toc("items_cov");
    if (rc) return rc;
    q->cov_items = true;
    q->cov_trend_q = qt;
    return 0;
}

extern "C" {

int pmk_query_items_cov(pmk_query *q, const pmk_kernel_desc *th)
{
    return items_cov_common(q, th, false, true, "pmk_query_items_cov");
}

int pmk_query_items_cov_multi(pmk_query *q, const pmk_kernel_desc *th)
{
    return items_cov_common(q, th, true, true, "pmk_query_items_cov_multi");
}

int pmk_query_mix_cov(pmk_query *q, const pmk_kernel_desc *weight_th)
{
    static const char who[] = "pmk_query_mix_cov";
    if (!q || !q->planned) { set_error("%s: query is not planned", who); return -1; }
    if (q->explicit_items) {
        set_error("%s: the query was made by pmk_query_create_items: its items belong to no blend", who);
        return -2;
    }
    if (!q->cov_items) { set_error("%s: pmk_query_items_cov has not run on this plan", who); return -2; }
    if (int rc = blend_profile_ok(weight_th, who)) return rc;
    if (int rc = cov_batch_ok(q->Nq, who)) return rc;       // blocks of pmk_query_items_cov_blocks on a larger batch
    pmk_ctx *c = q->m->ctx;
    PMK_HIP(hipSetDevice(c->device));
    q->mixed_cov = false;
    if (int rc = grow_sized(q->d_cov, q->cov_cap, q->Nq * q->Nq, c->stream, who, "the Nq x Nq result")) return rc;
    c->tic("mix_cov");
    const int rc = launch_mix_cov(q, *weight_th, c->stream);
    c->toc("mix_cov");
    if (rc) return rc;
    q->mixed_cov = true;
    return 0;
}

int pmk_query_fetch_cov(pmk_query *q, double *Cov, int64_t ldc)
{
    if (int rc = fetch_cov_common(q, Cov, ldc, hipMemcpyDeviceToHost, "pmk_query_fetch_cov")) return rc;
    PMK_HIP(hipStreamSynchronize(q->m->ctx->stream));
    return 0;
}

int pmk_query_fetch_cov_dev(pmk_query *q, double *Cov_dev, int64_t ldc)
{
    return fetch_cov_common(q, Cov_dev, ldc, hipMemcpyDeviceToDevice, "pmk_query_fetch_cov_dev");
}

int pmk_query_get_items_cov(pmk_query *q, int64_t region, int64_t *m_out, int32_t *query, double *S, int64_t lds)
{
    static const char who[] = "pmk_query_get_items_cov";
    if (!q || !q->planned) { set_error("%s: query is not planned", who); return -1; }
    if (!q->cov_items) { set_error("%s: pmk_query_items_cov has not run on this plan", who); return -2; }
    const pmk_model *m = q->m;
    if (region < m->leaf_base || region >= m->leaf_base + m->P) {
        set_error("%s: region %lld is outside this model's leaves [%lld, %lld)", who, (long long)region,
                  (long long)m->leaf_base, (long long)(m->leaf_base + m->P));
        return -3;
    }
    const int64_t b = q->roff[(size_t)region], mr = q->roff[(size_t)region + 1] - b;
    if (m_out) *m_out = mr;
    if (S && lds < mr) { set_error("%s: lds = %lld < m = %lld", who, (long long)lds, (long long)mr); return -4; }
    pmk_ctx *c = m->ctx;
    PMK_HIP(hipSetDevice(c->device));
    PMK_HIP(hipStreamSynchronize(c->stream));
    if (mr == 0) return 0;
    if (query) {
        // the rows are the region's sorted items: ascending query index
        std::vector<int32_t> item((size_t)mr), iq((size_t)q->total);
        PMK_HIP(hipMemcpy(item.data(), q->d_sorted_item + b, sizeof(int32_t) * (size_t)mr, hipMemcpyDeviceToHost));
        PMK_HIP(hipMemcpy(iq.data(), q->d_item_query, sizeof(int32_t) * (size_t)q->total, hipMemcpyDeviceToHost));
        for (int64_t a = 0; a < mr; ++a) query[a] = iq[(size_t)item[(size_t)a]];
    }
    if (S)
        PMK_HIP(hipMemcpy2D(S, sizeof(double) * (size_t)lds, q->d_cov_s + q->cov_goff[(size_t)(region - m->leaf_base)],
                            sizeof(double) * (size_t)mr, sizeof(double) * (size_t)mr, (size_t)mr, hipMemcpyDeviceToHost));
    return 0;
}

int pmk_predict_mixture_cov_fitted(pmk_model *m, const pmk_kernel_desc *weight_th, int64_t Nq, const double *Xq,
                                   double radius, double delta, double *Yq, double *Vq, double *Cov, int64_t ldc)
{
    static const char who[] = "pmk_predict_mixture_cov_fitted";
    if (!m) { set_error("%s: model is NULL", who); return -1; }
    if (int rc = whole_tree_ok(m, who, COV_NEEDS_ALL, -3)) return rc;
    if (Cov && ldc < Nq) { set_error("%s: ldc = %lld < Nq = %lld", who, (long long)ldc, (long long)Nq); return -4; }
    if (Cov)
        if (int rc = cov_batch_ok(Nq, who)) return rc;
    // with Cov NULL no covariance stage runs
    return one_shot(
        m, Nq, Xq, radius, delta,
        [&](pmk_query *q) { int rc = pmk_query_items_fitted(q); return !rc && Cov ? pmk_query_items_cov(q, nullptr) : rc; },
        [&](pmk_query *q) { int rc = pmk_query_mix(q, weight_th, 0, Nq); return !rc && Cov ? pmk_query_mix_cov(q, weight_th) : rc; },
        [&](pmk_query *q) { int rc = pmk_query_fetch(q, Yq, Vq); return !rc && Cov ? pmk_query_fetch_cov(q, Cov, ldc) : rc; });
}

int pmk_predict_mixture_cov_multi_fitted(pmk_model *m, const pmk_kernel_desc *weight_th, int64_t Nq, const double *Xq,
                                         double radius, double delta, double *Yq, int64_t ldyq, double *Vq, double *Cov,
                                         int64_t ldc)
{
    static const char who[] = "pmk_predict_mixture_cov_multi_fitted";
    if (!m) { set_error("%s: model is NULL", who); return -1; }
    if (int rc = whole_tree_ok(m, who, COV_NEEDS_ALL, -3)) return rc;
    if ((Yq && ldyq < Nq) || (Cov && ldc < Nq)) {
        set_error("%s: ldyq = %lld or ldc = %lld < Nq = %lld", who, (long long)ldyq, (long long)ldc, (long long)Nq);
        return -4;
    }
    if (Cov)
        if (int rc = cov_batch_ok(Nq, who)) return rc;
    // with Cov NULL no covariance stage runs
    return one_shot(
        m, Nq, Xq, radius, delta,
        [&](pmk_query *q) {
            int rc = pmk_query_items_multi_fitted(q, Vq != nullptr);
            return !rc && Cov ? pmk_query_items_cov_multi(q, nullptr) : rc;
        },
        [&](pmk_query *q) {
            int rc = pmk_query_mix_multi(q, weight_th, 0, Nq);
            return !rc && Cov ? pmk_query_mix_cov(q, weight_th) : rc;
        },
        [&](pmk_query *q) {
            int rc = (Yq || Vq) ? pmk_query_fetch_multi(q, Yq, ldyq, Vq) : 0;
            return !rc && Cov ? pmk_query_fetch_cov(q, Cov, ldc) : rc;
        });
}

}  // extern "C"

// ------------------------------------------------------------------------------------------ draws from the region blocks
// The factors' geometry from the plan's region offsets: the padded offsets, the regions by descending tile count (step k
// of the factorisation takes the first fstep_regions[k] of them) and every tile row of every region.
static int factor_layout(pmk_query *q, hipStream_t s, const char *who)
{
    const pmk_model *m = q->m;
    const int64_t P = m->P;
    std::vector<DrawRegion> desc((size_t)P);
    std::vector<int32_t> order((size_t)P);
    std::vector<DrawTask> tasks;
    q->cov_foff.assign((size_t)P + 1, 0);
    int32_t max_nt = 0;
    for (int64_t r = 0; r < P; ++r) {
        const int64_t b = q->roff[(size_t)(m->leaf_base + r)], mr = q->roff[(size_t)(m->leaf_base + r + 1)] - b;
        DrawRegion &d = desc[(size_t)r];
        d.soff = q->cov_goff[(size_t)r];
        d.foff = q->cov_foff[(size_t)r];
        d.p0 = b;
        d.m = (int32_t)mr;
        d.nt = (int32_t)((mr + DRAW_TILE - 1) / DRAW_TILE);
        const int64_t ld = (int64_t)DRAW_TILE * d.nt;
        q->cov_foff[(size_t)r + 1] = d.foff + ld * ld;
        max_nt = std::max(max_nt, d.nt);
        order[(size_t)r] = (int32_t)r;
        for (int32_t i = 0; i < d.nt; ++i) tasks.push_back({(int32_t)r, i});
    }
    std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return desc[(size_t)a].nt > desc[(size_t)b].nt; });
    q->fstep_regions.assign((size_t)max_nt, 0);
    for (int64_t r = 0; r < P; ++r)
        for (int32_t k = 0; k < desc[(size_t)r].nt; ++k) ++q->fstep_regions[(size_t)k];
    q->nftasks = (int64_t)tasks.size();
    if (int rc = grow_sized(q->d_cov_f, q->cov_f_cap, q->cov_foff[(size_t)P], s, who, "the padded factors")) return rc;
    if (int rc = grow_sized(q->d_fdesc, q->fdesc_cap, P, s, who, "the region descriptors")) return rc;
    if (int rc = grow_sized(q->d_forder, q->forder_cap, P, s, who, "the region order")) return rc;
    if (int rc = grow_sized(q->d_ftasks, q->ftasks_cap, q->nftasks, s, who, "the tile rows")) return rc;
    if (int rc = grow_sized(q->d_finfo, q->finfo_cap, P, s, who, "the status words")) return rc;
    if (int rc = grow_sized(q->d_fact, q->fact_cap, P, s, who, "the region marks")) return rc;
    if (int rc = grow_sized(q->d_fjit, q->fjit_cap, P, s, who, "the jitter values")) return rc;
    if (int rc = grow_sized(q->d_frel, q->frel_cap, 2 * P, s, who, "the relative jitters")) return rc;
    if (P > 0) {
        PMK_HIP(hipMemcpyAsync(q->d_fdesc, desc.data(), sizeof(DrawRegion) * (size_t)P, hipMemcpyHostToDevice, s));
        PMK_HIP(hipMemcpyAsync(q->d_forder, order.data(), sizeof(int32_t) * (size_t)P, hipMemcpyHostToDevice, s));
    }
    if (!tasks.empty())
        PMK_HIP(hipMemcpyAsync(q->d_ftasks, tasks.data(), sizeof(DrawTask) * tasks.size(), hipMemcpyHostToDevice, s));
    PMK_HIP(hipStreamSynchronize(s));       // the sources are locals
    return 0;
}

// draws of a chunk: the workspace holds total x chunk doubles, at most 256 MiB, at least one tile of draws
static int64_t draw_chunk(int64_t total, int64_t n_draws)
{
    const int64_t fit = ((int64_t)1 << 25) / std::max<int64_t>(total, 1) / DRAW_TILE * DRAW_TILE;
    const int64_t chunk = std::min<int64_t>(std::max<int64_t>(fit, DRAW_TILE), 256);
    return std::min(chunk, (n_draws + DRAW_TILE - 1) / DRAW_TILE * DRAW_TILE);
}

extern "C" {

int pmk_query_items_cov_blocks(pmk_query *q, const pmk_kernel_desc *th, int multi)
{
    return items_cov_common(q, th, multi != 0, false, "pmk_query_items_cov_blocks");
}

int pmk_query_factor_cov(pmk_query *q, const double *rel)
{
    static const char who[] = "pmk_query_factor_cov";
    if (!q || !q->planned) { set_error("%s: query is not planned", who); return -1; }
    if (!q->cov_items) { set_error("%s: no region blocks on this plan (pmk_query_items_cov, _multi or _blocks)", who); return -2; }
    const pmk_model *m = q->m;
    const int64_t P = m->P;
    std::vector<double> relv((size_t)P, 0.0);
    if (rel)
        for (int64_t r = 0; r < P; ++r) {
            if (!(rel[r] >= 0.0) || !(rel[r] <= 1.79769313486231570815e308)) {
                set_error("%s: rel[%lld] = %g is negative or not finite", who, (long long)r, rel[r]);
                return -2;
            }
            relv[(size_t)r] = rel[r];
        }
    pmk_ctx *c = m->ctx;
    PMK_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const bool have = q->cov_factored;
    q->cov_factored = false;
    if (!have)
        if (int rc = factor_layout(q, s, who)) return rc;
    if (P > 0) {
        PMK_HIP(hipMemcpyAsync(q->d_frel + P, relv.data(), sizeof(double) * (size_t)P, hipMemcpyHostToDevice, s));
        PMK_HIP(hipStreamSynchronize(s));   // `relv` is a local
    }
    c->tic("factor_cov");
    const int rc = launch_factor_cov(q, have ? 1 : 0, s);
    c->toc("factor_cov");
    if (rc) return rc;
    q->cov_factored = true;
    return 0;
}

int pmk_query_factor_info(pmk_query *q, int32_t *finfo, double *jitter)
{
    static const char who[] = "pmk_query_factor_info";
    if (!q || !q->planned) { set_error("%s: query is not planned", who); return -1; }
    if (!q->cov_items || !q->cov_factored) { set_error("%s: pmk_query_factor_cov has not run on these blocks", who); return -2; }
    const pmk_model *m = q->m;
    pmk_ctx *c = m->ctx;
    PMK_HIP(hipSetDevice(c->device));
    PMK_HIP(hipStreamSynchronize(c->stream));
    std::vector<int32_t> fi((size_t)m->P);
    if (m->P > 0) PMK_HIP(hipMemcpy(fi.data(), q->d_finfo, sizeof(int32_t) * (size_t)m->P, hipMemcpyDeviceToHost));
    if (jitter && m->P > 0) PMK_HIP(hipMemcpy(jitter, q->d_fjit, sizeof(double) * (size_t)m->P, hipMemcpyDeviceToHost));
    int any = 0;
    for (int64_t r = 0; r < m->P; ++r) {
        if (finfo) finfo[r] = fi[(size_t)r];
        any |= fi[(size_t)r] != 0;
    }
    return any;
}

int pmk_query_get_items_cov_factor(pmk_query *q, int64_t region, int64_t *m_out, double *L, int64_t ldl)
{
    static const char who[] = "pmk_query_get_items_cov_factor";
    if (!q || !q->planned) { set_error("%s: query is not planned", who); return -1; }
    if (!q->cov_items) { set_error("%s: pmk_query_items_cov has not run on this plan", who); return -2; }
    if (!q->cov_factored) { set_error("%s: pmk_query_factor_cov has not run on these blocks", who); return -2; }
    const pmk_model *m = q->m;
    if (region < m->leaf_base || region >= m->leaf_base + m->P) {
        set_error("%s: region %lld is outside this model's leaves [%lld, %lld)", who, (long long)region,
                  (long long)m->leaf_base, (long long)(m->leaf_base + m->P));
        return -3;
    }
    const int64_t mr = q->roff[(size_t)region + 1] - q->roff[(size_t)region];
    if (m_out) *m_out = mr;
    if (L && ldl < mr) { set_error("%s: ldl = %lld < m = %lld", who, (long long)ldl, (long long)mr); return -4; }
    pmk_ctx *c = m->ctx;
    PMK_HIP(hipSetDevice(c->device));
    PMK_HIP(hipStreamSynchronize(c->stream));
    if (mr == 0 || !L) return 0;
    const int64_t ld = (mr + DRAW_TILE - 1) / DRAW_TILE * DRAW_TILE;
    PMK_HIP(hipMemcpy2D(L, sizeof(double) * (size_t)ldl, q->d_cov_f + q->cov_foff[(size_t)(region - m->leaf_base)],
                        sizeof(double) * (size_t)ld, sizeof(double) * (size_t)mr, (size_t)mr, hipMemcpyDeviceToHost));
    // the tiles above the diagonal are never written on the device
    for (int64_t b = 1; b < mr; ++b)
        for (int64_t a = 0; a < b; ++a) L[a + ldl * b] = 0.0;
    return 0;
}

int pmk_query_draw(pmk_query *q, const pmk_kernel_desc *weight_th, int64_t n_draws, const double *z, int64_t ldz, double *E,
                   int64_t lde)
{
    static const char who[] = "pmk_query_draw";
    if (!q || !q->planned) { set_error("%s: query is not planned", who); return -1; }
    if (q->explicit_items) {
        set_error("%s: the query was made by pmk_query_create_items: its items belong to no blend", who);
        return -2;
    }
    if (!q->cov_items || !q->cov_factored) { set_error("%s: pmk_query_factor_cov has not run on these blocks", who); return -2; }
    if (int rc = blend_profile_ok(weight_th, who)) return rc;
    if (n_draws < 0) { set_error("%s: n_draws = %lld", who, (long long)n_draws); return -2; }
    if (n_draws == 0) return 0;
    if (!z || !E) { set_error("%s: %s is NULL", who, z ? "E" : "z"); return -2; }
    if (ldz < q->total || lde < q->Nq) {
        set_error("%s: ldz = %lld, lde = %lld: at least total_items = %lld and Nq = %lld", who, (long long)ldz, (long long)lde,
                  (long long)q->total, (long long)q->Nq);
        return -4;
    }
    if (q->Nq == 0) return 0;
    pmk_ctx *c = q->m->ctx;
    PMK_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const bool z_dev = is_device_pointer(z), e_dev = is_device_pointer(E);
    const int64_t chunk = draw_chunk(q->total, n_draws);
    if (int rc = grow_sized(q->d_draw_t, q->draw_t_cap, q->total * chunk, s, who, "the workspace of L Z")) return rc;
    if (!z_dev)
        if (int rc = grow_sized(q->d_draw_z, q->draw_z_cap, q->total * chunk, s, who, "the device copy of z")) return rc;
    if (!e_dev)
        if (int rc = grow_sized(q->d_draw_e, q->draw_e_cap, q->Nq * chunk, s, who, "the device copy of E")) return rc;
    c->tic("draw");
    int rc = 0;
    for (int64_t s0 = 0; s0 < n_draws && !rc; s0 += chunk) {
        const int64_t n = std::min(chunk, n_draws - s0);
        const double *dz = z + ldz * s0;
        int64_t dldz = ldz;
        if (!z_dev) {
            PMK_HIP(hipMemcpy2DAsync(q->d_draw_z, sizeof(double) * (size_t)q->total, dz, sizeof(double) * (size_t)ldz,
                                     sizeof(double) * (size_t)q->total, (size_t)n, hipMemcpyHostToDevice, s));
            dz = q->d_draw_z;
            dldz = q->total;
        }
        rc = launch_draw(q, *weight_th, dz, dldz, n, e_dev ? E + lde * s0 : q->d_draw_e, e_dev ? lde : q->Nq, s);
        if (!rc && !e_dev)
            PMK_HIP(hipMemcpy2DAsync(E + lde * s0, sizeof(double) * (size_t)lde, q->d_draw_e, sizeof(double) * (size_t)q->Nq,
                                     sizeof(double) * (size_t)q->Nq, (size_t)n, hipMemcpyDeviceToHost, s));
        // a host chunk is read or written by the copies above: the next one reuses the staging buffers
        if (!rc && (!z_dev || !e_dev)) PMK_HIP(hipStreamSynchronize(s));
    }
    c->toc("draw");
    return rc;
}

}  // extern "C"
