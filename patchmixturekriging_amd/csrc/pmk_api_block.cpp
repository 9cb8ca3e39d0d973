// C ABI of libpmk_hip.so (declared in include/pmk.h): block kriging, the mean and the kriging variance of weighted sums of
// the blended field over groups of queries (pmk_query_items_block and what serves its results; the kernels of
// pmk_block.hip).  The other query stages are in pmk_api_query.cpp.
#include <algorithm>
#include <new>
#include <vector>

#include "pmk_host.h"

using namespace pmk;

static const char BLOCK_NEEDS_ALL[] = "block kriging needs a model that holds every leaf";

// The strips of the block sweep from the regions' first aggregates: a region's aggregates are dealt evenly over
// ceil(count / TQ) strips, as build_strip_tasks (pmk_predict.hip) deals items.
static void block_tasks_from_regions(const pmk_model *m, const std::vector<int64_t> &aoff, std::vector<BlockTask> &tasks)
{
    for (int64_t r = 0; r < m->P; ++r) {
        const int64_t b = aoff[(size_t)r], e = aoff[(size_t)r + 1], mr = e - b;
        if (mr == 0) continue;
        const int64_t nstrips = (mr + TQ - 1) / TQ, w = (mr + nstrips - 1) / nstrips;
        for (int64_t f = b; f < e; f += w) {
            BlockTask t;
            t.region = (int32_t)r;
            t.count = (int32_t)std::min(e - f, w);
            t.first = f;
            tasks.push_back(t);
        }
    }
}

static int fetch_block_common(pmk_query *q, double *Yb, int64_t ldyb, double *Vb, hipMemcpyKind kind, const char *who)
{
    if (!q) { set_error("%s: query is NULL", who); return -1; }
    if (!q->block_items) { set_error("%s: pmk_query_items_block has not run on the current items", who); return -2; }
    if (Vb && !q->block_var) { set_error("%s: Vb was not computed (pmk_query_items_block ran with want_var = 0)", who); return -3; }
    if (Yb && ldyb < q->blk_F) { set_error("%s: ldyb = %lld < F = %lld", who, (long long)ldyb, (long long)q->blk_F); return -4; }
    pmk_ctx *c = q->m->ctx;
    PMK_HIP(hipSetDevice(c->device));
    if (q->blk_F > 0) {
        if (Yb)
            PMK_HIP(hipMemcpy2DAsync(Yb, sizeof(double) * (size_t)ldyb, q->d_blk_y, sizeof(double) * (size_t)q->blk_F,
                                     sizeof(double) * (size_t)q->blk_F, (size_t)q->R_items, kind, c->stream));
        if (Vb) PMK_HIP(hipMemcpyAsync(Vb, q->d_blk_v, sizeof(double) * (size_t)q->blk_F, kind, c->stream));
    }
    return 0;
}

extern "C" {

int pmk_query_items_block(pmk_query *q, const pmk_kernel_desc *th, const pmk_kernel_desc *weight_th, int64_t F,
                          const int32_t *group, const double *a, int want_var)
{
    static const char who[] = "pmk_query_items_block";
    if (!q || !q->planned) { set_error("%s: query is not planned", who); return -1; }
    pmk_model *m = q->m;
    if (!m->fitted) { set_error("%s: the model holds no resident factor", who); return -1; }
    if (q->explicit_items) {
        set_error("%s: the query was made by pmk_query_create_items: its items belong to no blend", who);
        return -2;
    }
    if (q->R_items < 1 || !q->items_fn) {
        set_error("%s: the last items on this plan must be those of pmk_query_items_multi or _multi_fitted", who);
        return -2;
    }
    if (q->um_ld - q->R_items != m->trend_q) {
        set_error("%s: the items were computed under a trend with q = %d, the model's has q = %d: run the items again", who,
                  q->um_ld - q->R_items, m->trend_q);
        return -2;
    }
    if (th) {
        if (int rc = cov_kernel_ok(th, m->D, who, "theta")) return rc;
    } else {
        if (m->ths.empty()) { set_error("%s: the model holds no kernels (pmk_model_set_kernels)", who); return -3; }
        for (size_t r = 0; r < m->ths.size(); ++r)
            if (int rc = cov_kernel_ok(&m->ths[r], m->D, who, "the model's own theta")) return rc;
        th = fitted_theta(m);
    }
    if (int rc = blend_profile_ok(weight_th, who)) return rc;
    if (!m->multi_solved) {
        set_error("%s: pmk_model_solve_multi has not run on the resident factor (the multi-output weights are stale)", who);
        return -3;
    }
    if (int rc = whole_tree_ok(m, who, BLOCK_NEEDS_ALL, -3)) return rc;
    if (F < 0 || F > 0x7fffffff || (q->Nq > 0 && (!group || !a))) { set_error("%s: bad F, or NULL group or a", who); return -3; }
    // the first query of every group: group is non-decreasing, so a group's queries are contiguous
    std::vector<int64_t> gq;
    try {
        gq.assign((size_t)F + 1, q->Nq);
    } catch (const std::bad_alloc &) {
        set_error("%s: %lld bytes of host memory for the first queries of F = %lld groups are not available", who,
                  (long long)(8 * (F + 1)), (long long)F);
        return -100;
    }
    {
        int64_t f = 0;
        for (int64_t j = 0; j < q->Nq; ++j) {
            const int64_t g = group[j];
            if (g < 0 || g >= F || (j > 0 && g < group[j - 1])) {
                set_error("%s: group[%lld] = %lld %s", who, (long long)j, (long long)g,
                          (g < 0 || g >= F) ? "is outside [0, F)" : "is below its predecessor: the groups must be contiguous");
                return -3;
            }
            for (; f <= g; ++f) gq[(size_t)f] = j;
        }
    }
    pmk_ctx *c = m->ctx;
    PMK_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const int R = q->R_items, qt = m->trend_q;
    const bool var = want_var != 0;
    q->block_items = q->block_var = false;
    q->blk_F = F;
    q->blk_naggs = q->blk_ntasks = 0;
    if (q->blk_q_cap < q->Nq) {
        PMK_HIP(hipStreamSynchronize(s));
        dev_free(q->d_blk_group); dev_free(q->d_blk_a);
        q->blk_q_cap = 0;
        if (dev_alloc(&q->d_blk_group, q->Nq) || dev_alloc(&q->d_blk_a, q->Nq)) {
            set_error("%s: hipMalloc of %lld bytes for the groups and coefficients failed", who, (long long)(12 * q->Nq));
            return -100;
        }
        q->blk_q_cap = q->Nq;
    }
    if (q->blk_item_cap < q->total + 1) {
        PMK_HIP(hipStreamSynchronize(s));
        dev_free(q->d_blk_w); dev_free(q->d_blk_head); dev_free(q->d_blk_agg_of); dev_free(q->d_blk_scan);
        q->blk_item_cap = 0;
        const int64_t cap = q->total + 1;
        if (dev_alloc(&q->d_blk_w, cap) || dev_alloc(&q->d_blk_head, cap) || dev_alloc(&q->d_blk_agg_of, cap) ||
            dev_alloc(&q->d_blk_scan, cap + 1)) {
            set_error("%s: hipMalloc of %lld bytes for the items' weights and aggregates failed", who, (long long)(24 * cap));
            return -100;
        }
        q->blk_item_cap = cap;
    }
    if (int rc = grow_sized(q->d_blk_gq, q->blk_gq_cap, F + 1, s, who, "the groups' first queries")) return rc;
    if (int rc = grow_sized(q->d_blk_y, q->blk_y_cap, F * R, s, who, "the group means")) return rc;
    if (int rc = grow_sized(q->d_blk_v, q->blk_v_cap, F, s, who, "the group variances")) return rc;
    if (int rc = grow_sized(q->d_blk_aoff, q->blk_aoff_cap, m->P + 2, s, who, "the regions' first aggregates")) return rc;
    if (q->Nq > 0) {
        PMK_HIP(hipMemcpyAsync(q->d_blk_group, group, sizeof(int32_t) * (size_t)q->Nq, hipMemcpyHostToDevice, s));
        PMK_HIP(hipMemcpyAsync(q->d_blk_a, a, sizeof(double) * (size_t)q->Nq, hipMemcpyHostToDevice, s));
    }
    PMK_HIP(hipMemcpyAsync(q->d_blk_gq, gq.data(), sizeof(int64_t) * gq.size(), hipMemcpyHostToDevice, s));
    PMK_HIP(hipStreamSynchronize(s));       // `gq` is a local, group and a are the caller's
    c->tic("items_block");
    // every launch and every buffer that follows the aggregate count, in one place: the stage timer closes on every exit
    auto stage = [&]() -> int {
        int rc = launch_block_weights(q, *weight_th, s);
        if (!rc && var && q->total > 0) {
            // the aggregate list: heads, their scan, ONE count back, the compaction
            if ((rc = launch_block_heads(q, s))) return rc;
            int64_t naggs = 0;
            PMK_HIP(hipMemcpyAsync(&naggs, q->d_blk_scan + q->total, sizeof(int64_t), hipMemcpyDeviceToHost, s));
            PMK_HIP(hipStreamSynchronize(s));
            if (q->blk_agg_cap < naggs) {
                dev_free(q->d_blk_aggs); dev_free(q->d_blk_piece);
                q->blk_agg_cap = 0;
                const int64_t cap = naggs + naggs / 8 + 64;
                if (dev_alloc(&q->d_blk_aggs, cap) || dev_alloc(&q->d_blk_piece, 4 * cap)) {
                    set_error("%s: hipMalloc of %lld bytes for the aggregates failed", who, (long long)(56 * cap));
                    return -100;
                }
                q->blk_agg_cap = cap;
            }
            q->blk_naggs = naggs;
            // the regions' first aggregates (P + 1) and, behind them, the first aggregate above the member cap
            std::vector<int64_t> aoff((size_t)m->P + 2, 0);
            unsigned long long *d_over = reinterpret_cast<unsigned long long *>(q->d_blk_aoff + m->P + 1);
            const unsigned long long none = (unsigned long long)naggs;
            PMK_HIP(hipMemcpyAsync(d_over, &none, sizeof(none), hipMemcpyHostToDevice, s));
            if ((rc = launch_block_aggregates(q, PMK_BLOCK_MAX_MEMBERS, d_over, q->d_blk_aoff, s))) return rc;
            PMK_HIP(hipMemcpyAsync(aoff.data(), q->d_blk_aoff, sizeof(int64_t) * aoff.size(), hipMemcpyDeviceToHost, s));
            PMK_HIP(hipStreamSynchronize(s));
            if (aoff[(size_t)m->P + 1] < naggs) {
                BlockAgg ag;
                PMK_HIP(hipMemcpy(&ag, q->d_blk_aggs + aoff[(size_t)m->P + 1], sizeof(ag), hipMemcpyDeviceToHost));
                set_error("%s: group %d holds %d items of region %lld, an aggregate is limited to PMK_BLOCK_MAX_MEMBERS = %d", who,
                          ag.group, ag.count, (long long)(m->leaf_base + ag.region), PMK_BLOCK_MAX_MEMBERS);
                return -5;
            }
            std::vector<BlockTask> tasks;
            block_tasks_from_regions(m, aoff, tasks);
            q->blk_ntasks = (int64_t)tasks.size();
            if (int rc2 = grow_sized(q->d_blk_tasks, q->blk_tasks_cap, q->blk_ntasks, s, who, "the strip tasks")) return rc2;
            PMK_HIP(hipMemcpyAsync(q->d_blk_tasks, tasks.data(), sizeof(BlockTask) * tasks.size(), hipMemcpyHostToDevice, s));
            PMK_HIP(hipStreamSynchronize(s));   // `tasks` is a local
            q->blk_grid = std::min<int64_t>(q->blk_ntasks, (int64_t)c->num_cu);      // one 8-wave workgroup per CU
            if ((rc = reserve_strips(m, q->blk_grid))) return rc;
            if (qt > 0) {
                if (int rc2 = grow_sized(q->d_cov_z, q->cov_z_cap, q->total * TQ_MAX, s, who, "the items' trend vectors")) return rc2;
                rc = launch_cov_trend_items(q, s);
            }
            if (!rc) rc = PMK_BY_DTYPE(m, launch_items_block(q, th, s));
        }
        if (!rc) rc = launch_block_reduce(q, var, qt, s);
        return rc;
    };
    const int rc = stage();
    c->toc("items_block");
    if (rc) return rc;
    q->block_items = true;
    q->block_var = var;
    return 0;
}

int pmk_query_fetch_block(pmk_query *q, double *Yb, int64_t ldyb, double *Vb)
{
    if (int rc = fetch_block_common(q, Yb, ldyb, Vb, hipMemcpyDeviceToHost, "pmk_query_fetch_block")) return rc;
    PMK_HIP(hipStreamSynchronize(q->m->ctx->stream));
    return 0;
}

int pmk_query_fetch_block_dev(pmk_query *q, double *Yb_dev, int64_t ldyb, double *Vb_dev)
{
    return fetch_block_common(q, Yb_dev, ldyb, Vb_dev, hipMemcpyDeviceToDevice, "pmk_query_fetch_block_dev");
}

int pmk_query_get_items_block(pmk_query *q, int64_t *n_out, int32_t *region, int32_t *group, int64_t *first, int32_t *count,
                              double *kappa, double *vnorm2, double *znorm2, double *sw2)
{
    static const char who[] = "pmk_query_get_items_block";
    if (!q || !q->planned) { set_error("%s: query is not planned", who); return -1; }
    if (!q->block_items || !q->block_var) {
        set_error("%s: pmk_query_items_block has not run with want_var = 1 on the current items", who);
        return -2;
    }
    pmk_ctx *c = q->m->ctx;
    PMK_HIP(hipSetDevice(c->device));
    PMK_HIP(hipStreamSynchronize(c->stream));
    const size_t n = (size_t)q->blk_naggs;
    if (n_out) *n_out = q->blk_naggs;
    if (n == 0) return 0;
    if (region || group || first || count) {
        std::vector<BlockAgg> ag(n);
        PMK_HIP(hipMemcpy(ag.data(), q->d_blk_aggs, sizeof(BlockAgg) * n, hipMemcpyDeviceToHost));
        for (size_t k = 0; k < n; ++k) {
            if (region) region[k] = (int32_t)(q->m->leaf_base + ag[k].region);
            if (group) group[k] = ag[k].group;
            if (first) first[k] = ag[k].first;
            if (count) count[k] = ag[k].count;
        }
    }
    double *dst[4] = {kappa, vnorm2, znorm2, sw2};
    for (int p = 0; p < 4; ++p)
        if (dst[p])
            PMK_HIP(hipMemcpy(dst[p], q->d_blk_piece + (int64_t)p * q->blk_agg_cap, sizeof(double) * n, hipMemcpyDeviceToHost));
    return 0;
}

int pmk_predict_mixture_block_fitted(pmk_model *m, const pmk_kernel_desc *weight_th, int64_t Nq, const double *Xq,
                                     double radius, double delta, int64_t F, const int32_t *group, const double *a,
                                     double *Yb, int64_t ldyb, double *Vb)
{
    static const char who[] = "pmk_predict_mixture_block_fitted";
    if (!m) { set_error("%s: model is NULL", who); return -1; }
    if (int rc = whole_tree_ok(m, who, BLOCK_NEEDS_ALL, -3)) return rc;
    if (Yb && ldyb < F) { set_error("%s: ldyb = %lld < F = %lld", who, (long long)ldyb, (long long)F); return -4; }
    return one_shot(
        m, Nq, Xq, radius, delta,
        [&](pmk_query *q) {
            int rc = pmk_query_items_multi_fitted(q, 0);
            return rc ? rc : pmk_query_items_block(q, nullptr, weight_th, F, group, a, Vb != nullptr);
        },
        [](pmk_query *) { return 0; }, [&](pmk_query *q) { return pmk_query_fetch_block(q, Yb, ldyb, Vb); });
}

}  // extern "C"
