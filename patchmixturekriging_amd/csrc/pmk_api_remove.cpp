// C ABI of libpmk_hip.so (declared in include/pmk.h): removing observations from a fitted model in place.  The checks, the
// row list of the call, the deletion (pmk_remove.hip), the back substitution and the host state that follows; the rule of
// the whole is stated at pmk_model_remove in the header.
#include <algorithm>
#include <utility>

#include "pmk_host.h"

using namespace pmk;

// The index list of a tree-built model without the removed entries, by a host round trip like the append's: `prepare`
// builds the new list beside the old one before anything is launched, `commit` puts it in place once the deletion has
// been launched.  The entries that stay keep their order, so every patch's list stays ascending.
struct ReducedPatchIndex {
    int32_t *d_pidx = nullptr;
    std::vector<int64_t> off;
    ~ReducedPatchIndex() { dev_free(d_pidx); }
};

// rows: per patch, ascending, first[r] .. first[r + 1]
static int prepare_patch_index(pmk_model *m, const std::vector<int64_t> &first, const std::vector<int32_t> &rows,
                               ReducedPatchIndex &out)
{
    static const char who[] = "pmk_model_remove";
    hipStream_t s = m->ctx->stream;
    const int64_t P = m->P, old_total = m->pidx_off[(size_t)P];
    std::vector<int32_t> old((size_t)old_total);
    PMK_HIP(hipMemcpyAsync(old.data(), m->d_pidx, sizeof(int32_t) * (size_t)old_total, hipMemcpyDeviceToHost, s));
    PMK_HIP(hipStreamSynchronize(s));
    out.off.assign((size_t)P + 1, 0);
    std::vector<int32_t> kept;
    kept.reserve((size_t)old_total);
    for (int64_t r = 0; r < P; ++r) {
        const int64_t b = m->pidx_off[(size_t)r], nr = m->pidx_off[(size_t)r + 1] - b;
        int64_t next = first[(size_t)r];
        for (int64_t i = 0; i < nr; ++i) {
            if (next < first[(size_t)r + 1] && rows[(size_t)next] == i) { ++next; continue; }
            kept.push_back(old[(size_t)(b + i)]);
        }
        out.off[(size_t)r + 1] = (int64_t)kept.size();
    }
    const int64_t total = (int64_t)kept.size();
    if (dev_alloc(&out.d_pidx, total)) {
        set_error("%s: hipMalloc of %lld bytes for the index list failed", who, (long long)(total * 4));
        return -100;
    }
    PMK_HIP(hipMemcpyAsync(out.d_pidx, kept.data(), sizeof(int32_t) * (size_t)total, hipMemcpyHostToDevice, s));
    PMK_HIP(hipStreamSynchronize(s));       // `kept` is a local; nothing enqueued earlier still gathers through the old list
    return 0;
}

static int commit_patch_index(pmk_model *m, ReducedPatchIndex &idx)
{
    dev_free(m->d_pidx);                    // only this call's launches are in flight, and they do not read it
    m->d_pidx = idx.d_pidx;
    idx.d_pidx = nullptr;
    m->pidx_off = idx.off;
    // the source is the model's own host copy: it outlives the copy
    PMK_HIP(hipMemcpyAsync(m->d_pidx_off, m->pidx_off.data(), sizeof(int64_t) * m->pidx_off.size(), hipMemcpyHostToDevice,
                           m->ctx->stream));
    return 0;
}

// the rows patch r can lose and stay in its last block row
static int64_t removable_rows(const PatchDesc &d) { return (int64_t)d.n - (int64_t)TILE * (d.nt - 1) - 1; }

extern "C" {

int pmk_model_removable(pmk_model *m, int64_t *rows)
{
    if (!m || !rows) { set_error("pmk_model_removable: NULL argument"); return -1; }
    for (int64_t r = 0; r < m->P; ++r) rows[r] = removable_rows(m->desc[(size_t)r]);
    return 0;
}

int pmk_model_remove(pmk_model *m, int64_t n_items, const int32_t *patch, const int64_t *row)
{
    static const char who[] = "pmk_model_remove";
    if (!m) { set_error("%s: model is NULL", who); return -1; }
    if (n_items < 0) { set_error("%s: n_items = %lld", who, (long long)n_items); return -2; }
    if (n_items == 0) return 0;
    if (!m->fitted) { set_error("%s: the model is not fitted: there is no factor to take rows from (pmk_model_fit first)", who); return -1; }
    if (m->loaded || m->ths.empty()) {
        set_error("%s: the model was built by pmk_model_load and holds no targets: z cannot follow", who);
        return -1;
    }
    if (!patch || !row) { set_error("%s: NULL patches or rows", who); return -2; }
    const int64_t P = m->P;
    std::vector<int64_t> count((size_t)P, 0);
    for (int64_t i = 0; i < n_items; ++i) {
        if (patch[i] < 0 || patch[i] >= P) {
            set_error("%s: item %lld names patch %d, outside 0 .. %lld", who, (long long)i, (int)patch[i], (long long)(P - 1));
            return -3;
        }
        const int64_t nr = m->desc[(size_t)patch[i]].n;
        if (row[i] < 0 || row[i] >= nr) {
            set_error("%s: item %lld names row %lld of patch %d, outside 0 .. %lld", who, (long long)i, (long long)row[i],
                      (int)patch[i], (long long)(nr - 1));
            return -3;
        }
        ++count[(size_t)patch[i]];
    }
    {
        std::vector<std::pair<std::pair<int32_t, int64_t>, int64_t>> items((size_t)n_items);
        for (int64_t i = 0; i < n_items; ++i) items[(size_t)i] = {{patch[i], row[i]}, i};
        std::sort(items.begin(), items.end());
        for (int64_t i = 1; i < n_items; ++i)
            if (items[(size_t)i].first == items[(size_t)i - 1].first) {
                set_error("%s: item %lld gives row %lld of patch %d a second time (first: item %lld)", who,
                          (long long)items[(size_t)i].second, (long long)items[(size_t)i].first.second,
                          (int)items[(size_t)i].first.first, (long long)items[(size_t)i - 1].second);
                return -3;
            }
    }
    for (int64_t r = 0; r < P; ++r) {
        const PatchDesc &d = m->desc[(size_t)r];
        if (count[(size_t)r] > removable_rows(d)) {
            set_error("%s: patch %lld has %lld removable rows (n = %d, nt = %d: at least %d rows stay), %lld rows asked for", who,
                      (long long)r, (long long)removable_rows(d), (int)d.n, (int)d.nt, TILE * (d.nt - 1) + 1,
                      (long long)count[(size_t)r]);
            return -4;
        }
    }
    for (int64_t r = 0; r < P; ++r)
        if (count[(size_t)r] > PMK_REMOVE_MAX_ROWS) {
            set_error("%s: %lld rows of patch %lld in one call, the limit is PMK_REMOVE_MAX_ROWS = %d", who,
                      (long long)count[(size_t)r], (long long)r, PMK_REMOVE_MAX_ROWS);
            return -5;
        }

    // the rows grouped by patch, ascending; one task per patch that loses rows
    std::vector<int64_t> first((size_t)P + 1, 0), fill((size_t)P);
    for (int64_t r = 0; r < P; ++r) first[(size_t)r + 1] = first[(size_t)r] + count[(size_t)r];
    std::copy(first.begin(), first.end() - 1, fill.begin());
    std::vector<int32_t> hrows((size_t)n_items);
    for (int64_t i = 0; i < n_items; ++i) hrows[(size_t)fill[(size_t)patch[i]]++] = (int32_t)row[i];
    std::vector<RemoveTask> tasks;
    for (int64_t r = 0; r < P; ++r) {
        if (count[(size_t)r] == 0) continue;
        std::sort(hrows.begin() + first[(size_t)r], hrows.begin() + first[(size_t)r + 1]);
        tasks.push_back({(int32_t)r, (int32_t)count[(size_t)r], first[(size_t)r]});
    }

    pmk_ctx *c = m->ctx;
    PMK_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const int64_t ntasks = (int64_t)tasks.size();
    int rc;
    if ((rc = grow_sized(m->d_rm_tasks, m->rm_tasks_cap, ntasks, s, who, "the tasks"))) return rc;
    if ((rc = grow_sized(m->d_rm_rows, m->rm_rows_cap, n_items, s, who, "the row list"))) return rc;
    PMK_HIP(hipMemcpyAsync(m->d_rm_tasks, tasks.data(), sizeof(RemoveTask) * tasks.size(), hipMemcpyHostToDevice, s));
    PMK_HIP(hipMemcpyAsync(m->d_rm_rows, hrows.data(), sizeof(int32_t) * hrows.size(), hipMemcpyHostToDevice, s));
    PMK_HIP(hipStreamSynchronize(s));       // the sources are locals
    ReducedPatchIndex new_index;
    if (m->from_bsp)
        if ((rc = prepare_patch_index(m, first, hrows, new_index))) return rc;

    c->tic("remove_rows");
    rc = PMK_BY_DTYPE(m, launch_remove_rows(m, m->d_rm_tasks, ntasks, m->d_rm_rows, s));
    c->toc("remove_rows");
    if (rc) return rc;
    // from here on the device holds n - m: the host follows whatever the later calls say
    if (m->from_bsp)
        if ((rc = commit_patch_index(m, new_index))) return rc;
    for (int64_t r = 0; r < P; ++r) m->desc[(size_t)r].n -= (int32_t)count[(size_t)r];
    m->loo_valid = false;
    m->R_multi = 0;                         // the target block has n_r rows: pmk_model_set_targets_multi again
    m->multi_solved = false;
    m->trend_q = 0;
    // over every patch, as the append ends: one launch whatever lost rows, and the split path solves all patches together
    // anyway (it forms z = L^-1 y again from the targets that have just moved, then c)
    c->tic("remove_solve");
    rc = PMK_BY_DTYPE(m, launch_backsolve(m, s, 0, P));
    c->toc("remove_solve");
    return rc;
}

}  // extern "C"
