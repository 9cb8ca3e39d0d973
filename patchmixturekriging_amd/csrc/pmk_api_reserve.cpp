// C ABI of libpmk_hip.so (declared in include/pmk.h): room to grow in a model.  The checks, the new layout, the move
// (pmk_reserve.hip), the swap and the host state that follows; the rule of the whole is stated at pmk_model_reserve in the
// header.
#include <algorithm>

#include "pmk_host.h"

using namespace pmk;

namespace {

// the buffers of a layout; released unless `keep` says the model has taken them
struct NewLayout {
    PatchDesc *d_desc = nullptr;
    void *x = nullptr, *y = nullptr, *z = nullptr, *c = nullptr, *diag = nullptr, *a = nullptr, *inv = nullptr;
    bool keep = false;
    ~NewLayout()
    {
        if (keep) return;
        dev_free(d_desc);
        for (void *p : {x, y, z, c, diag, a, inv})
            if (p) (void)hipFree(p);
    }
};

}  // namespace

extern "C" {

int pmk_model_reserve(pmk_model *m, const int64_t *rows)
{
    static const char who[] = "pmk_model_reserve";
    if (!m || !rows) { set_error("%s: NULL argument", who); return -1; }
    const int64_t P = m->P;
    for (int64_t r = 0; r < P; ++r)
        if (rows[r] < 0) { set_error("%s: rows[%lld] = %lld", who, (long long)r, (long long)rows[r]); return -2; }
    if (m->split_mode) {
        set_error("%s: the model factors on the split path, whose solves read ld as the patch's extent", who);
        return -3;
    }
    for (int64_t r = 0; r < P; ++r)
        if ((int64_t)m->desc[(size_t)r].n + rows[r] > (1 << 24)) {
            set_error("%s: patch %lld has n = %d, %lld more rows pass the limit of 2^24", who, (long long)r,
                      (int)m->desc[(size_t)r].n, (long long)rows[r]);
            return -4;
        }
    // a patch keeps its stride where that has the room, and is never shrunk
    std::vector<PatchDesc> nd = m->desc;
    bool grows = false;
    int64_t a = 0, xo = 0, yo = 0, io = 0, max_ld = 0;
    for (int64_t r = 0; r < P; ++r) {
        PatchDesc &d = nd[(size_t)r];
        const int64_t need = ((int64_t)d.n + rows[r] + TILE - 1) / TILE * TILE;
        if (need > d.ld) { d.ld = (int32_t)need; grows = true; }
        d.aoff = a; d.xoff = xo; d.yoff = yo; d.ioff = io;
        a += (int64_t)d.ld * d.ld;
        xo += (int64_t)d.ld * m->D;
        yo += d.ld;
        io += (int64_t)(d.ld / TILE) * 4 * 32 * 32;
        max_ld = std::max<int64_t>(max_ld, d.ld);
    }
    if (!grows) return 0;

    pmk_ctx *c = m->ctx;
    PMK_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    // the whole new layout beside the old one: a failed allocation leaves the model as it was
    NewLayout nl;
    auto alloc_real = [&](void **p, int64_t count) {
        return hipMalloc(p, m->esz * (size_t)std::max<int64_t>(count, 1)) == hipSuccess ? 0 : -100;
    };
    int rc = dev_alloc(&nl.d_desc, P);
    rc |= alloc_real(&nl.x, xo);
    rc |= alloc_real(&nl.y, yo);
    rc |= alloc_real(&nl.z, yo);
    rc |= alloc_real(&nl.c, yo);
    rc |= alloc_real(&nl.a, a);
    rc |= alloc_real(&nl.inv, io);
    if (m->d_diag) rc |= alloc_real(&nl.diag, yo);
    if (rc) {
        (void)hipGetLastError();
        set_error("%s: hipMalloc of the new layout failed (%lld bytes of slabs)", who, (long long)(a * (int64_t)m->esz));
        return -100;
    }
    PMK_HIP(hipMemcpyAsync(nl.d_desc, nd.data(), sizeof(PatchDesc) * (size_t)P, hipMemcpyHostToDevice, s));
    PMK_HIP(hipStreamSynchronize(s));       // `nd` is a local: no early return below leaves its copy in flight
    c->tic("reserve");
    rc = PMK_BY_DTYPE(m, launch_reserve(m, nl.d_desc, nl.x, nl.y, nl.z, nl.c, nl.diag, nl.a, nl.inv, max_ld, s));
    c->toc("reserve");
    if (rc) return rc;
    PMK_HIP(hipStreamSynchronize(s));       // the old buffers go: nothing may still read them
    // from here on nothing of the old layout is kept: the chunk prefix of the gather kernels follows ld, and it is only
    // written now that the move has succeeded (a blocking copy: `chunk` is a local)
    std::vector<int32_t> chunk;
    if (m->from_bsp) {
        chunk.assign((size_t)P + 1, 0);
        for (int64_t r = 0; r < P; ++r) chunk[(size_t)r + 1] = chunk[(size_t)r] + (nd[(size_t)r].ld + 255) / 256;
        PMK_HIP(hipMemcpy(m->d_gchunk, chunk.data(), sizeof(int32_t) * (size_t)(P + 1), hipMemcpyHostToDevice));
    }

    // the swap: the model's pointers are read at every launch, so query objects follow without knowing
    std::swap(m->d_desc, nl.d_desc);
    std::swap(m->d_x, nl.x); std::swap(m->d_y, nl.y); std::swap(m->d_z, nl.z); std::swap(m->d_c, nl.c);
    std::swap(m->d_a, nl.a); std::swap(m->d_inv, nl.inv);
    if (m->d_diag) std::swap(m->d_diag, nl.diag);
    m->desc = nd;
    m->tot_a = a; m->tot_x = xo; m->tot_y = yo; m->tot_inv = io;
    if (m->from_bsp) m->gchunks = chunk[(size_t)P];
    // what is laid out by yoff goes, as after an append: the multi-output blocks, the trend state, the leave-one-out
    // values (their tasks depend on nt alone, but d_dloo is allocated with them)
    for (void **p : {&m->d_ym, &m->d_cm, &m->d_loo_tasks}) {
        if (*p) (void)hipFree(*p);
        *p = nullptr;
    }
    dev_free(m->d_dloo);
    m->loo_ntasks = 0;
    m->loo_valid = false;
    m->R_multi = 0;
    m->multi_solved = false;
    m->trend_q = 0;
    m->trend_cols_dirty = false;
    return 0;                               // nl now holds the old layout and frees it
}

}  // extern "C"
