// C ABI of libpmk_hip.so (declared in include/pmk.h): appending observations to a fitted model in place.  The checks, the
// staging of the items, the task list of the covariance sweep, the border (pmk_append.hip), the back substitution and the
// host state that follows; the rule of the whole is stated at pmk_model_append in the header.
#include <algorithm>
#include <cmath>
#include <limits>
#include <new>
#include <utility>

#include "pmk_host.h"

using namespace pmk;

namespace pmk {

void append_release(pmk_model *m)
{
    if (pmk_query *q = m->append_q) {
        dev_free(q->d_xq); dev_free(q->d_qdiag); dev_free(q->d_cov_v); dev_free(q->d_cov_s); dev_free(q->d_cov_tasks);
        dev_free(q->d_cov_pairs);
        delete q;
        m->append_q = nullptr;
    }
    dev_free(m->d_app_y); dev_free(m->d_app_diag); dev_free(m->d_app_iota);
}

}  // namespace pmk

// The index list of a tree-built model with the new entries at the end of their patches, by a host round trip (the list
// is read back, merged and uploaded again: it has to move anyway, its segments grow in place of one another).  In two
// steps, so that a call that fails leaves the list it found: `prepare` builds the new list beside the old one before
// anything is launched, `commit` puts it in place once the border has been launched.
struct NewPatchIndex {
    int32_t *d_pidx = nullptr;
    std::vector<int64_t> off;
    ~NewPatchIndex() { dev_free(d_pidx); }
};

static int prepare_patch_index(pmk_model *m, const std::vector<int64_t> &count, const std::vector<int64_t> &first,
                               const std::vector<int64_t> &gidx, NewPatchIndex &out)
{
    static const char who[] = "pmk_model_append";
    hipStream_t s = m->ctx->stream;
    const int64_t P = m->P, old_total = m->pidx_off[(size_t)P];
    std::vector<int32_t> old((size_t)old_total);
    PMK_HIP(hipMemcpyAsync(old.data(), m->d_pidx, sizeof(int32_t) * (size_t)old_total, hipMemcpyDeviceToHost, s));
    PMK_HIP(hipStreamSynchronize(s));
    out.off.assign((size_t)P + 1, 0);
    for (int64_t r = 0; r < P; ++r)
        out.off[(size_t)r + 1] = out.off[(size_t)r] + (m->pidx_off[(size_t)r + 1] - m->pidx_off[(size_t)r]) + count[(size_t)r];
    const int64_t total = out.off[(size_t)P];
    if (total >= 0x7fffffff) { set_error("%s: the number of (point, leaf) pairs must stay below 2^31-1", who); return -5; }
    std::vector<int32_t> merged((size_t)total);
    for (int64_t r = 0; r < P; ++r) {
        const int64_t b = m->pidx_off[(size_t)r], nr = m->pidx_off[(size_t)r + 1] - b;
        std::copy(old.begin() + b, old.begin() + b + nr, merged.begin() + out.off[(size_t)r]);
        for (int64_t a = 0; a < count[(size_t)r]; ++a)
            merged[(size_t)(out.off[(size_t)r] + nr + a)] = (int32_t)gidx[(size_t)(first[(size_t)r] + a)];
    }
    if (dev_alloc(&out.d_pidx, total)) {
        set_error("%s: hipMalloc of %lld bytes for the index list failed", who, (long long)(total * 4));
        return -100;
    }
    PMK_HIP(hipMemcpyAsync(out.d_pidx, merged.data(), sizeof(int32_t) * (size_t)total, hipMemcpyHostToDevice, s));
    PMK_HIP(hipStreamSynchronize(s));       // `merged` is a local; nothing enqueued earlier still gathers through the old list
    return 0;
}

static int commit_patch_index(pmk_model *m, NewPatchIndex &idx, int64_t N_new)
{
    dev_free(m->d_pidx);                    // only this call's launches are in flight, and they do not read it
    m->d_pidx = idx.d_pidx;
    idx.d_pidx = nullptr;
    m->pidx_off = idx.off;
    m->N_global = N_new;
    // the source is the model's own host copy: it outlives the copy
    PMK_HIP(hipMemcpyAsync(m->d_pidx_off, m->pidx_off.data(), sizeof(int64_t) * m->pidx_off.size(), hipMemcpyHostToDevice,
                           m->ctx->stream));
    return 0;
}

// What the host keeps by tile count, after an append has taken patches into block rows that pmk_model_reserve laid out
// (m->desc[].nt already follows): max_nt, the factorisation order and the active prefix as model_geometry builds them,
// the leave-one-out tasks (dropped: rebuilt on their next use) and the strip workspace, whose slots are max_nt block rows
// long and which planned queries use without asking again: `longer` is that workspace for the new max_nt, allocated by
// the caller before anything was launched (null where max_nt stays or no workspace exists yet), so that nothing in here
// can leave a planned query with a workspace shorter than its patches.  split_mode stays as chosen at creation.
static int follow_tile_counts(pmk_model *m, DevTmp<char> &longer)
{
    const int64_t P = m->P;
    hipStream_t s = m->ctx->stream;
    int max_nt = 0;
    std::vector<int32_t> order((size_t)P);
    for (int64_t r = 0; r < P; ++r) {
        order[(size_t)r] = (int32_t)r;
        max_nt = std::max(max_nt, (int)m->desc[(size_t)r].nt);
    }
    std::stable_sort(order.begin(), order.end(),
                     [&](int32_t a, int32_t b) { return m->desc[(size_t)a].nt > m->desc[(size_t)b].nt; });
    m->active_prefix.assign((size_t)max_nt + 2, 0);
    for (int64_t r = 0; r < P; ++r)
        for (int t = 0; t <= m->desc[(size_t)r].nt; ++t) ++m->active_prefix[(size_t)t];
    // first what cannot fail: the workspace and max_nt are a matching pair before anything below returns
    if (max_nt > m->max_nt) {
        if (longer.p) {
            (void)hipFree(m->d_strip);      // waits for the kernels that may still use it
            m->d_strip = longer.p;
            longer.p = nullptr;
        }
        m->max_nt = max_nt;
    }
    m->loo_ntasks = 0;                      // the task list belongs to the old tile counts: built again on its next use
    if (m->d_loo_tasks) {
        (void)hipFree(m->d_loo_tasks);
        m->d_loo_tasks = nullptr;
    }
    PMK_HIP(hipMemcpyAsync(m->d_order, order.data(), sizeof(int32_t) * (size_t)P, hipMemcpyHostToDevice, s));
    PMK_HIP(hipStreamSynchronize(s));       // `order` is a local
    return 0;
}

extern "C" {

int pmk_model_capacity(pmk_model *m, int64_t *free_rows)
{
    if (!m || !free_rows) { set_error("pmk_model_capacity: NULL argument"); return -1; }
    for (int64_t r = 0; r < m->P; ++r) free_rows[r] = (int64_t)m->desc[(size_t)r].ld - m->desc[(size_t)r].n;
    return 0;
}

int pmk_model_append(pmk_model *m, int64_t n_items, const double *x, const double *y, const double *diag,
                     const int32_t *patch, const int64_t *global_index)
{
    static const char who[] = "pmk_model_append";
    if (!m) { set_error("%s: model is NULL", who); return -1; }
    if (n_items < 0) { set_error("%s: n_items = %lld", who, (long long)n_items); return -2; }
    if (n_items == 0) return 0;
    if (!m->fitted) { set_error("%s: the model is not fitted: there is no factor to border (pmk_model_fit first)", who); return -1; }
    if (m->loaded || m->ths.empty()) {
        set_error("%s: the model was built by pmk_model_load and holds no targets: z cannot be extended", who);
        return -1;
    }
    if (!x || !y || !patch) { set_error("%s: NULL points, targets or patches", who); return -2; }
    if (m->from_bsp && !global_index) {
        set_error("%s: the model was made by pmk_model_create_from_bsp: global_index is required", who);
        return -2;
    }
    if (!m->from_bsp && global_index) {
        set_error("%s: global_index must be NULL, the model was not made by pmk_model_create_from_bsp", who);
        return -2;
    }
    if (diag && !m->d_diag) {
        set_error("%s: diag given, but the model holds no addends (pmk_model_set_diag before the fit)", who);
        return -2;
    }
    if (n_items > PMK_COV_MAX_QUERIES) {
        set_error("%s: %lld items in one call, the limit is PMK_COV_MAX_QUERIES = %d", who, (long long)n_items,
                  PMK_COV_MAX_QUERIES);
        return -5;
    }
    const int D = m->D;
    const int64_t P = m->P;
    std::vector<int64_t> count((size_t)P, 0);
    int64_t N_new = m->N_global;
    for (int64_t i = 0; i < n_items; ++i) {
        if (patch[i] < 0 || patch[i] >= P) {
            set_error("%s: item %lld names patch %d, outside 0 .. %lld", who, (long long)i, (int)patch[i], (long long)(P - 1));
            return -3;
        }
        ++count[(size_t)patch[i]];
        if (global_index) {
            // a new observation is a new global point: an index below N would hand an old point's target to the new row
            if (global_index[i] < m->N_global || global_index[i] >= 0x7ffffffe) {
                set_error("%s: item %lld has global index %lld, outside N = %lld .. 2^31-3", who, (long long)i,
                          (long long)global_index[i], (long long)m->N_global);
                return -3;
            }
            N_new = std::max(N_new, global_index[i] + 1);
        }
    }
    if (global_index) {
        // one global point is one row of a patch (it may be a row of several patches)
        std::vector<std::pair<int32_t, int64_t>> rows((size_t)n_items);
        for (int64_t i = 0; i < n_items; ++i) rows[(size_t)i] = {patch[i], global_index[i]};
        std::sort(rows.begin(), rows.end());
        const auto dup = std::adjacent_find(rows.begin(), rows.end());
        if (dup != rows.end()) {
            set_error("%s: global index %lld is given twice for patch %d", who, (long long)dup->second, (int)dup->first);
            return -3;
        }
        // a patch's index list stays ascending (patch_holds of pmk_items.h searches it by bisection), and the rows follow
        // the order given: so that order has to ascend.  The first new index of a patch is >= N, above its old entries
        std::vector<int64_t> last((size_t)P, -1);
        for (int64_t i = 0; i < n_items; ++i) {
            int64_t &prev = last[(size_t)patch[i]];
            if (global_index[i] < prev) {
                set_error("%s: item %lld gives patch %d the global index %lld after %lld: the global indices of a patch must "
                          "ascend in the order given", who, (long long)i, (int)patch[i], (long long)global_index[i],
                          (long long)prev);
                return -3;
            }
            prev = global_index[i];
        }
    }
    for (int64_t i = 0; i < n_items; ++i) {
        bool finite = std::isfinite(y[i]) && (!diag || std::isfinite(diag[i]));
        for (int d = 0; d < D; ++d) finite = finite && std::isfinite(x[i * D + d]);
        if (!finite) {
            set_error("%s: item %lld has a non-finite coordinate, target or addend", who, (long long)i);
            return -6;
        }
    }
    for (int64_t r = 0; r < P; ++r) {
        const int64_t free_rows = (int64_t)m->desc[(size_t)r].ld - m->desc[(size_t)r].n;
        if (count[(size_t)r] > free_rows) {
            set_error("%s: patch %lld has %lld free rows (n = %d, ld = %d), %lld rows asked for", who, (long long)r,
                      (long long)free_rows, (int)m->desc[(size_t)r].n, (int)m->desc[(size_t)r].ld, (long long)count[(size_t)r]);
            return -4;
        }
    }
    // the border factors S in an LDS image of TILE x (TILE + 1); only a model with reserved rows can get here
    for (int64_t r = 0; r < P; ++r)
        if (count[(size_t)r] > TILE) {
            set_error("%s: %lld points for patch %lld in one call, the limit is %d per patch", who, (long long)count[(size_t)r],
                      (long long)r, TILE);
            return -5;
        }

    // the items grouped by patch, in the order given within a patch; one strip of the sweep per receiving patch
    std::vector<int64_t> first((size_t)P + 1, 0), fill((size_t)P);
    for (int64_t r = 0; r < P; ++r) first[(size_t)r + 1] = first[(size_t)r] + count[(size_t)r];
    std::copy(first.begin(), first.end() - 1, fill.begin());
    std::vector<double> hx((size_t)(n_items * D)), hy((size_t)n_items), hd((size_t)n_items, 0.0), hq((size_t)n_items);
    std::vector<int64_t> hg(global_index ? (size_t)n_items : 0);
    for (int64_t i = 0; i < n_items; ++i) {
        const int64_t r = patch[i], at = fill[(size_t)r]++;
        std::copy(x + i * D, x + (i + 1) * D, hx.begin() + at * D);
        hy[(size_t)at] = y[i];
        if (diag) hd[(size_t)at] = diag[i];
        hq[(size_t)at] = m->sigma2s[(size_t)r] + hd[(size_t)at];       // what the diagonal of S takes beside k(x, x)
        if (global_index) hg[(size_t)at] = global_index[i];
    }
    std::vector<CovTask> tasks;
    std::vector<CovPair> pairs;
    int64_t velems = 0, selems = 0;
    for (int64_t r = 0; r < P; ++r) {
        if (count[(size_t)r] == 0) continue;
        CovTask t;
        t.region = (int32_t)r;
        t.count = (int32_t)count[(size_t)r];
        t.first = first[(size_t)r];
        t.voff = velems;
        t.goff = selems;
        t.m = t.count;
        t.a0 = 0;
        pairs.push_back({(int32_t)tasks.size(), (int32_t)tasks.size()});
        tasks.push_back(t);
        velems += (int64_t)m->desc[(size_t)r].ld * TQ;
        selems += count[(size_t)r] * count[(size_t)r];
    }

    pmk_ctx *c = m->ctx;
    PMK_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    if (!m->append_q) {
        m->append_q = new (std::nothrow) pmk_query();
        if (!m->append_q) { set_error("out of memory"); return -100; }
        m->append_q->m = m;
        m->append_q->explicit_items = true;
        m->append_q->min_v = -std::numeric_limits<double>::infinity();     // the diagonal of S is not a variance: no floor
    }
    pmk_query *q = m->append_q;
    const int64_t ntasks = (int64_t)tasks.size();
    int rc;
    if ((rc = grow_sized(q->d_cov_v, q->cov_v_cap, velems * (int64_t)m->esz, s, who, "the V arena"))) return rc;
    if ((rc = grow_sized(q->d_cov_s, q->cov_s_cap, selems, s, who, "the blocks of S"))) return rc;
    if ((rc = grow_sized(q->d_cov_tasks, q->cov_tasks_cap, ntasks, s, who, "the strip tasks"))) return rc;
    if ((rc = grow_sized(q->d_cov_pairs, q->cov_pairs_cap, ntasks, s, who, "the strip pairs"))) return rc;
    if ((rc = grow_sized(q->d_xq, m->app_x_cap, n_items * D, s, who, "the staged points"))) return rc;
    if ((rc = grow_sized(q->d_qdiag, m->app_qdiag_cap, n_items, s, who, "the staged diagonal"))) return rc;
    if ((rc = grow_sized(m->d_app_y, m->app_y_cap, n_items, s, who, "the staged targets"))) return rc;
    if ((rc = grow_sized(m->d_app_diag, m->app_diag_cap, n_items, s, who, "the staged addends"))) return rc;
    if (m->app_iota_cap < n_items) {
        if ((rc = grow_sized(m->d_app_iota, m->app_iota_cap, n_items, s, who, "the item order"))) return rc;
        std::vector<int32_t> iota((size_t)n_items);
        for (int64_t i = 0; i < n_items; ++i) iota[(size_t)i] = (int32_t)i;
        PMK_HIP(hipMemcpy(m->d_app_iota, iota.data(), sizeof(int32_t) * (size_t)n_items, hipMemcpyHostToDevice));
    }
    q->Nq = q->total = n_items;
    q->d_sorted_item = q->d_item_query = m->d_app_iota;     // item i is point i, already in region order
    q->cov_ntasks = q->cov_npairs = ntasks;
    PMK_HIP(hipMemcpyAsync(q->d_xq, hx.data(), sizeof(double) * hx.size(), hipMemcpyHostToDevice, s));
    PMK_HIP(hipMemcpyAsync(q->d_qdiag, hq.data(), sizeof(double) * hq.size(), hipMemcpyHostToDevice, s));
    PMK_HIP(hipMemcpyAsync(m->d_app_y, hy.data(), sizeof(double) * hy.size(), hipMemcpyHostToDevice, s));
    PMK_HIP(hipMemcpyAsync(m->d_app_diag, hd.data(), sizeof(double) * hd.size(), hipMemcpyHostToDevice, s));
    PMK_HIP(hipMemcpyAsync(q->d_cov_tasks, tasks.data(), sizeof(CovTask) * tasks.size(), hipMemcpyHostToDevice, s));
    PMK_HIP(hipMemcpyAsync(q->d_cov_pairs, pairs.data(), sizeof(CovPair) * pairs.size(), hipMemcpyHostToDevice, s));
    PMK_HIP(hipStreamSynchronize(s));       // the sources are locals
    NewPatchIndex new_index;
    if (m->from_bsp)
        if ((rc = prepare_patch_index(m, count, first, hg, new_index))) return rc;
    // rows that enter new block rows may raise max_nt, and the strip workspace's slots are max_nt block rows long: the
    // longer one is allocated here, while a failure still leaves the model untouched
    DevTmp<char> longer_strips;
    {
        int64_t new_max_nt = m->max_nt;
        for (int64_t r = 0; r < P; ++r)
            new_max_nt = std::max<int64_t>(new_max_nt, (m->desc[(size_t)r].n + count[(size_t)r] + TILE - 1) / TILE);
        if (new_max_nt > m->max_nt && m->strip_slots > 0) {
            const int64_t bytes = (int64_t)m->esz * new_max_nt * TILE * TQ * m->strip_slots;
            if (longer_strips.alloc(bytes)) {
                (void)hipGetLastError();
                set_error("%s: hipMalloc of %lld bytes for the strip workspace of %lld block rows failed", who,
                          (long long)bytes, (long long)new_max_nt);
                return -100;
            }
        }
    }

    c->tic("append_sweep");
    rc = PMK_BY_DTYPE(m, launch_items_cov(q, fitted_theta(m), s));
    c->toc("append_sweep");
    if (rc) return rc;
    c->tic("append_border");
    rc = PMK_BY_DTYPE(m, launch_append_border(m, q, m->d_app_y, diag ? m->d_app_diag : nullptr, s));
    c->toc("append_border");
    if (rc) return rc;
    // from here on the device holds n + m: the host follows whatever the later calls say
    if (m->from_bsp)
        if ((rc = commit_patch_index(m, new_index, N_new))) return rc;
    bool crossed = false;
    for (int64_t r = 0; r < P; ++r) {
        PatchDesc &d = m->desc[(size_t)r];
        d.n += (int32_t)count[(size_t)r];
        const int32_t nt = (d.n + TILE - 1) / TILE;
        crossed = crossed || nt != d.nt;
        d.nt = nt;                          // the border has written it into the device descriptor
    }
    m->loo_valid = false;
    m->R_multi = 0;                         // the target block has n_r rows: pmk_model_set_targets_multi again
    m->multi_solved = false;
    m->trend_q = 0;
    if (crossed)                            // after the flags: a failure in here must not leave them standing
        if ((rc = follow_tile_counts(m, longer_strips))) return rc;
    // over every patch: one launch whatever received points, and the split path solves all patches together anyway (it
    // forms z = L^-1 y again from the targets the border has just extended, then c)
    c->tic("append_solve");
    rc = PMK_BY_DTYPE(m, launch_backsolve(m, s, 0, P));
    c->toc("append_solve");
    return rc;
}

}  // extern "C"
