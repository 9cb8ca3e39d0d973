// C ABI of libpmk_hip.so (declared in include/pmk.h): error state, contexts and timers, trees, models and model selection.
// The query side is in pmk_api_query.cpp and pmk_api_loo_mix.cpp.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>

#include "pmk_host.h"

namespace pmk {

static thread_local char g_err[1024] = "";

void set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int bsp_build(int D, int64_t N, const double *X, int levels, int sign_mode, int dot_mode, BspArrays &t);
int bsp_from_hyperplanes(int D, int levels, const double *hp_v, const double *hp_c, int dot_mode, BspArrays &t);
int bsp_build_device(pmk_ctx *c, int D, int64_t N, const double *X, int levels, int sign_mode, int dot_mode, BspArrays &t);
int bsp_assign_device(pmk_ctx *c, const BspArrays &t, int64_t N, const double *X, double eps, int64_t *offsets,
                      int64_t *inds, int64_t *list_offsets, int64_t *lists);
int bsp_patch_index_device(pmk_ctx *c, const BspArrays &t, int64_t N, const double *X, double eps, int64_t *offsets,
                           int32_t **d_inds, double **d_X);
int64_t bsp_find(const BspArrays &t, const double *x);
int bsp_assign(const BspArrays &t, int64_t N, const double *X, double eps, int64_t *offsets, int64_t *inds,
               int64_t *list_offsets, int64_t *lists);
int64_t bsp_neighbours(const BspArrays &t, const double *p, double radius, double delta, int64_t home,
                       int64_t *region_inds, double *ts, double *zs, uint8_t *keep);

// host double buffer -> device buffer of the model's element type (and back)
static int upload_real(const pmk_model *m, void *dst, int64_t elem_off, const double *src, size_t count)
{
    if (m->dtype == PMK_F32) {
        std::vector<float> tmp(count);
        for (size_t i = 0; i < count; ++i) tmp[i] = (float)src[i];
        PMK_HIP(hipMemcpy((char *)dst + elem_off * 4, tmp.data(), 4 * count, hipMemcpyHostToDevice));
    } else {
        PMK_HIP(hipMemcpy((char *)dst + elem_off * 8, src, 8 * count, hipMemcpyHostToDevice));
    }
    return 0;
}
// rows x cols block with device leading dimension ldd -> host leading dimension ldh (synchronous)
static int download_real_2d(const pmk_model *m, double *dst, int64_t ldh, const void *src, int64_t elem_off, int64_t ldd,
                            int64_t rows, int64_t cols, hipStream_t s)
{
    if (m->dtype == PMK_F32) {
        std::vector<float> tmp((size_t)(rows * cols));
        PMK_HIP(hipMemcpy2DAsync(tmp.data(), 4 * rows, (const char *)src + elem_off * 4, 4 * ldd, 4 * rows, (size_t)cols,
                                 hipMemcpyDeviceToHost, s));
        PMK_HIP(hipStreamSynchronize(s));
        for (int64_t j = 0; j < cols; ++j)
            for (int64_t i = 0; i < rows; ++i) dst[i + j * ldh] = (double)tmp[(size_t)(i + j * rows)];
    } else {
        PMK_HIP(hipMemcpy2DAsync(dst, 8 * ldh, (const char *)src + elem_off * 8, 8 * ldd, 8 * rows, (size_t)cols,
                                 hipMemcpyDeviceToHost, s));
        PMK_HIP(hipStreamSynchronize(s));
    }
    return 0;
}

// the strip workspace of the model: one max_nt * TILE x TQ block per workgroup slot of a strip kernel (prediction,
// leave-one-out), grow only.  hipFree waits for the kernels that may still use the old one.
int reserve_strips(pmk_model *m, int64_t slots)
{
    if (m->strip_slots >= slots) return 0;
    if (m->d_strip) PMK_HIP(hipFree(m->d_strip));
    m->d_strip = nullptr;
    m->strip_slots = 0;
    PMK_HIP(hipMalloc(&m->d_strip, m->esz * (size_t)((int64_t)m->max_nt * TILE * TQ * slots)));
    m->strip_slots = slots;
    return 0;
}

// chunks of 16 items per region (item_means_kernel): the host prefix over the regions of q's plan, and their count.
// tests/_multi_refs.py restates this rule and asserts that it still stands in this file, so it stays here.
void multi_chunk_prefix(pmk_query *q)
{
    const int64_t P = q->m->P;
    q->mcpre.assign((size_t)P + 1, 0);
    for (int64_t r = 0; r < P; ++r)
        q->mcpre[(size_t)r + 1] = q->mcpre[(size_t)r] + (q->roff[(size_t)r + 1] - q->roff[(size_t)r] + 15) / 16;
    q->mchunks = q->mcpre[(size_t)P];
}

}  // namespace pmk

using namespace pmk;

void pmk_ctx::tic(const char *name)
{
    if (!timers) return;
    for (auto &t : tm)
        if (t.name == name) { (void)hipEventRecord(t.a, stream); t.valid = false; return; }
    Timer t;
    t.name = name;
    (void)hipEventCreate(&t.a);
    (void)hipEventCreate(&t.b);
    t.valid = false;
    (void)hipEventRecord(t.a, stream);
    tm.push_back(t);
}

void pmk_ctx::toc(const char *name)
{
    if (!timers) return;
    for (auto &t : tm)
        if (t.name == name) { (void)hipEventRecord(t.b, stream); t.valid = true; return; }
}

extern "C" {

int pmk_version(void) { return PMK_VERSION; }
const char *pmk_last_error(void) { return g_err; }

// ------------------------------------------------------------------------------------------ context
int pmk_ctx_create(int device, pmk_ctx **out)
{
    if (!out) { set_error("pmk_ctx_create: out is NULL"); return -2; }
    *out = nullptr;
    int ndev = 0;
    PMK_HIP(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) { set_error("pmk_ctx_create: device %d of %d", device, ndev); return -1; }
    PMK_HIP(hipSetDevice(device));
    pmk_ctx *c = new (std::nothrow) pmk_ctx();
    if (!c) { set_error("out of memory"); return -100; }
    c->device = device;
    hipDeviceProp_t prop;
    // the context's own stream gets the greatest priority the device offers, ahead of other streams that share the device
    int prio_least = 0, prio_greatest = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest);
    if (hipGetDeviceProperties(&prop, device) != hipSuccess ||
        hipStreamCreateWithPriority(&c->own_stream, hipStreamNonBlocking, prio_greatest) != hipSuccess) {
        set_error("pmk_ctx_create: device %d: %s", device, hipGetErrorString(hipGetLastError()));
        pmk_ctx_destroy(c);
        return -100;
    }
    c->num_cu = prop.multiProcessorCount;
    c->stream = c->own_stream;
    if (hipMalloc((void **)&c->d_clk, sizeof(unsigned long long) * 130 * 8) != hipSuccess ||
        hipMemset(c->d_clk, 0, sizeof(unsigned long long) * 130 * 8) != hipSuccess) {
        set_error("pmk_ctx_create: device %d: %s", device, hipGetErrorString(hipGetLastError()));
        pmk_ctx_destroy(c);
        return -100;
    }
    // kernel attributes are per device: set them for this context's device (current after hipSetDevice above)
    if (pmk::f64::set_device_attributes() || pmk::f32::set_device_attributes() || pmk::set_plan_attributes() ||
        pmk::f64::set_append_attributes() || pmk::f32::set_append_attributes() || pmk::f64::set_remove_attributes() ||
        pmk::f32::set_remove_attributes()) {
        pmk_ctx_destroy(c);
        return -100;
    }
    *out = c;
    return 0;
}

int pmk_ctx_set_stream(pmk_ctx *ctx, void *hip_stream)
{
    if (!ctx) { set_error("pmk_ctx_set_stream: ctx is NULL"); return -1; }
    ctx->stream = hip_stream ? (hipStream_t)hip_stream : ctx->own_stream;
    return 0;
}

int pmk_ctx_set_stream_null(pmk_ctx *ctx)
{
    if (!ctx) { set_error("pmk_ctx_set_stream_null: ctx is NULL"); return -1; }
    ctx->stream = nullptr;               // the device's legacy default stream
    return 0;
}

int pmk_ctx_synchronize(pmk_ctx *ctx)
{
    if (!ctx) { set_error("pmk_ctx_synchronize: ctx is NULL"); return -1; }
    PMK_HIP(hipStreamSynchronize(ctx->stream));
    return 0;
}

void pmk_ctx_destroy(pmk_ctx *ctx)
{
    if (!ctx) return;
    for (auto &t : ctx->tm) { (void)hipEventDestroy(t.a); (void)hipEventDestroy(t.b); }
    for (auto &e : ctx->panel_ev) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
    if (ctx->d_clk) (void)hipFree(ctx->d_clk);
    delete ctx;
}

int pmk_ctx_shader_clock(pmk_ctx *ctx, int which, double *ghz)
{
    if (!ctx || !ghz || which < 0 || which > 1) { set_error("pmk_ctx_shader_clock: bad argument"); return -1; }
    PMK_HIP(hipSetDevice(ctx->device));
    unsigned long long h[130 * 8];
    PMK_HIP(hipMemcpyAsync(h, ctx->d_clk, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
    PMK_HIP(hipStreamSynchronize(ctx->stream));
    double cyc = 0, ticks = 0;          // time-weighted mean over the launches and the 8 probing workgroups
    for (int x = 0; x < 8; ++x)
        for (int i = which ? 64 : 0; i < (which ? 65 : 64); ++i) {
            cyc += (double)h[130 * x + 2 * i];
            ticks += (double)h[130 * x + 2 * i + 1];
        }
    *ghz = ticks > 0 ? cyc / (ticks * 10.0) : 0.0;          // ticks of 10 ns
    return 0;
}

int pmk_ctx_enable_timers(pmk_ctx *ctx, int on)
{
    if (!ctx) { set_error("ctx is NULL"); return -1; }
    ctx->timers = on;
    return 0;
}

int pmk_ctx_timer_ms(pmk_ctx *ctx, const char *stage, double *ms)
{
    if (!ctx || !stage || !ms) { set_error("pmk_ctx_timer_ms: NULL argument"); return -1; }
    if (std::string(stage) == "panel" && ctx->panel_n > 0) {     // summed over the panel launches of the last fit
        double tot = 0;
        for (int i = 0; i < ctx->panel_n; ++i) {
            PMK_HIP(hipEventSynchronize(ctx->panel_ev[(size_t)i].second));
            float f = 0;
            PMK_HIP(hipEventElapsedTime(&f, ctx->panel_ev[(size_t)i].first, ctx->panel_ev[(size_t)i].second));
            tot += f;
        }
        *ms = tot;
        return 0;
    }
    if (std::strncmp(stage, "step:", 5) == 0) {                    // one factorisation step launch of the last fit
        const int i = atoi(stage + 5);
        if (i < 0 || i >= ctx->panel_n) { set_error("no timing recorded for stage '%s'", stage); return -2; }
        PMK_HIP(hipEventSynchronize(ctx->panel_ev[(size_t)i].second));
        float f = 0;
        PMK_HIP(hipEventElapsedTime(&f, ctx->panel_ev[(size_t)i].first, ctx->panel_ev[(size_t)i].second));
        *ms = f;
        return 0;
    }
    for (auto &t : ctx->tm)
        if (t.name == stage && t.valid) {
            PMK_HIP(hipEventSynchronize(t.b));
            float f = 0;
            PMK_HIP(hipEventElapsedTime(&f, t.a, t.b));
            *ms = f;
            return 0;
        }
    set_error("no timing recorded for stage '%s'", stage);
    return -2;
}

// ------------------------------------------------------------------------------------------ BSP
int pmk_bsp_build(int D, int64_t N, const double *X, int levels, int sign_mode, int dot_mode, pmk_bsp **out)
{
    if (!out) { set_error("pmk_bsp_build: out is NULL"); return -6; }
    *out = nullptr;
    if (D < 1 || D > MAX_D) { set_error("pmk_bsp_build: D=%d outside 1..%d", D, MAX_D); return -1; }
    if (N < 1 || !X) { set_error("pmk_bsp_build: empty point set"); return -2; }
    if (levels < 2 || levels > 31) { set_error("pmk_bsp_build: levels=%d must be in 2..31", levels); return -4; }
    if ((N >> (levels - 1)) < 1) { set_error("pmk_bsp_build: N=%lld < 2^(levels-1)", (long long)N); return -4; }
    pmk_bsp *b = new (std::nothrow) pmk_bsp();
    if (!b) { set_error("out of memory"); return -100; }
    int rc = bsp_build(D, N, X, levels, sign_mode, dot_mode != 0, b->t);
    if (rc) { delete b; return rc; }
    *out = b;
    return 0;
}

int pmk_bsp_build_device(pmk_ctx *ctx, int D, int64_t N, const double *X, int levels, int sign_mode, int dot_mode,
                         pmk_bsp **out)
{
    if (!out) { set_error("pmk_bsp_build_device: out is NULL"); return -6; }
    *out = nullptr;
    if (!ctx) { set_error("pmk_bsp_build_device: context is NULL"); return -1; }
    if (D < 1 || D > MAX_D) { set_error("pmk_bsp_build_device: D=%d outside 1..%d", D, MAX_D); return -1; }
    if (N < 1 || N >= 0x7fffffff || !X) { set_error("pmk_bsp_build_device: N must be in 1..2^31-2"); return -2; }
    if (levels < 2 || levels > 31) { set_error("pmk_bsp_build_device: levels=%d must be in 2..31", levels); return -4; }
    if ((N >> (levels - 1)) < 1) { set_error("pmk_bsp_build_device: N=%lld < 2^(levels-1)", (long long)N); return -4; }
    PMK_HIP(hipSetDevice(ctx->device));
    pmk_bsp *b = new (std::nothrow) pmk_bsp();
    if (!b) { set_error("out of memory"); return -100; }
    int rc = bsp_build_device(ctx, D, N, X, levels, sign_mode, dot_mode != 0, b->t);
    if (rc) { delete b; return rc; }
    *out = b;
    return 0;
}

int pmk_bsp_from_hyperplanes(int D, int levels, const double *hp_v, const double *hp_c, int dot_mode, pmk_bsp **out)
{
    if (!out || !hp_v || !hp_c) { set_error("pmk_bsp_from_hyperplanes: NULL argument"); return -1; }
    *out = nullptr;
    if (D < 1 || D > MAX_D || levels < 2 || levels > 31) { set_error("pmk_bsp_from_hyperplanes: bad D/levels"); return -1; }
    pmk_bsp *b = new (std::nothrow) pmk_bsp();
    if (!b) { set_error("out of memory"); return -100; }
    bsp_from_hyperplanes(D, levels, hp_v, hp_c, dot_mode != 0, b->t);
    *out = b;
    return 0;
}

void pmk_bsp_destroy(pmk_bsp *bsp) { delete bsp; }
int pmk_bsp_dim(const pmk_bsp *bsp) { return bsp ? bsp->t.D : -1; }
int pmk_bsp_levels(const pmk_bsp *bsp) { return bsp ? bsp->t.levels : -1; }
int pmk_bsp_dot_mode(const pmk_bsp *bsp) { return bsp ? bsp->t.dot_mode : -1; }
int64_t pmk_bsp_num_leaves(const pmk_bsp *bsp) { return bsp ? bsp->t.P : -1; }
int64_t pmk_bsp_num_points(const pmk_bsp *bsp) { return bsp ? bsp->t.N : -1; }

int pmk_bsp_arrays(const pmk_bsp *bsp, double *hp_v, double *hp_c, int64_t *leaf_offsets, int64_t *leaf_inds)
{
    if (!bsp) { set_error("pmk_bsp_arrays: bsp is NULL"); return -1; }
    const BspArrays &t = bsp->t;
    for (int64_t k = 0; k < t.P - 1; ++k) {
        const int64_t h = t.pre[(size_t)k];
        if (hp_v) for (int d = 0; d < t.D; ++d) hp_v[k * t.D + d] = t.v[(size_t)(h * t.D + d)];
        if (hp_c) hp_c[k] = t.c[(size_t)h];
    }
    if (leaf_offsets) std::memcpy(leaf_offsets, t.leaf_off.data(), sizeof(int64_t) * (size_t)(t.P + 1));
    if (leaf_inds && !t.leaf_inds.empty()) std::memcpy(leaf_inds, t.leaf_inds.data(), sizeof(int64_t) * t.leaf_inds.size());
    return 0;
}

int pmk_bsp_assign(const pmk_bsp *bsp, int64_t N, const double *X, double eps, int64_t *offsets, int64_t *inds,
                   int64_t *list_offsets, int64_t *lists)
{
    if (!bsp || !offsets || (N > 0 && !X)) { set_error("pmk_bsp_assign: NULL argument"); return -1; }
    return bsp_assign(bsp->t, N, X, eps, offsets, inds, list_offsets, lists);
}

int pmk_bsp_assign_device(pmk_ctx *ctx, const pmk_bsp *bsp, int64_t N, const double *X, double eps, int64_t *offsets,
                          int64_t *inds, int64_t *list_offsets, int64_t *lists)
{
    if (!ctx || !bsp || !offsets || (N > 0 && !X)) { set_error("pmk_bsp_assign_device: NULL argument"); return -1; }
    if (N < 0 || N >= 0x7fffffff) { set_error("pmk_bsp_assign_device: N must be below 2^31-1"); return -2; }
    PMK_HIP(hipSetDevice(ctx->device));
    return bsp_assign_device(ctx, bsp->t, N, X, eps, offsets, inds, list_offsets, lists);
}

int64_t pmk_bsp_findpartition(const pmk_bsp *bsp, const double *x)
{
    if (!bsp || !x) { set_error("pmk_bsp_findpartition: NULL argument"); return -1; }
    return bsp_find(bsp->t, x);
}

int64_t pmk_bsp_neighbours(const pmk_bsp *bsp, const double *p, double radius, double delta, int64_t home,
                           int64_t *region_inds, double *ts, double *zs, uint8_t *keep)
{
    if (!bsp || !p || !region_inds) { set_error("pmk_bsp_neighbours: NULL argument"); return -1; }
    return bsp_neighbours(bsp->t, p, radius, delta, home, region_inds, ts, zs, keep);
}

// ------------------------------------------------------------------------------------------ model
void pmk_model_destroy(pmk_model *m)
{
    if (!m) return;
    append_release(m);
    dev_free(m->d_rm_tasks); dev_free(m->d_rm_rows);
    dev_free(m->d_desc); dev_free(m->d_info); dev_free(m->d_hv); dev_free(m->d_hc); dev_free(m->d_pre);
    dev_free(m->d_order); dev_free(m->d_dloo); dev_free(m->d_loo_cnt); dev_free(m->d_ths); dev_free(m->d_sigma2s);
    dev_free(m->d_pidx_off); dev_free(m->d_pidx); dev_free(m->d_gchunk); dev_free(m->d_gstage);
    dev_free(m->d_tbeta); dev_free(m->d_tL); dev_free(m->d_tG); dev_free(m->d_tinfo);
    for (void **p : {&m->d_diag, &m->d_x, &m->d_y, &m->d_z, &m->d_c, &m->d_a, &m->d_inv, &m->d_strip, &m->d_partial, &m->d_solve_part, &m->d_chain,
                     &m->d_ym, &m->d_cm, &m->d_loo_tasks}) {
        if (*p) (void)hipFree(*p);
        *p = nullptr;
    }
    delete m;
}

static int upload_targets(pmk_model *m, const double *const *y)
{
    std::vector<double> hy((size_t)m->tot_y, 0.0);
    for (int64_t r = 0; r < m->P; ++r) {
        if (!y[r]) { set_error("targets of patch %lld are NULL", (long long)r); return -6; }
        std::memcpy(hy.data() + m->desc[(size_t)r].yoff, y[r], sizeof(double) * (size_t)m->desc[(size_t)r].n);
    }
    return upload_real(m, m->d_y, 0, hy.data(), hy.size());
}

int pmk_model_create(pmk_ctx *ctx, int D, int64_t P, const int64_t *n, const double *const *X,
                     const double *const *y, pmk_model **out)
{
    return pmk_model_create_ex(ctx, D, P, n, X, y, PMK_F64, out);
}

// The geometry of a model from its patch sizes, shared by every way of creating one (host lists: pmk_model_create_ex;
// tree + global points: pmk_model_create_from_bsp): the PatchDesc layout, the device buffers, the factorisation order
// and the split-path rule.  `first_leaf` only numbers the patch in the error text of an empty one.  The buffers come back
// allocated and empty; d_desc, d_order and the zeroed d_info are on the device.
static int model_geometry(pmk_ctx *ctx, int D, int64_t P, const int64_t *n, int dtype, const char *who, int64_t first_leaf,
                          pmk_model **out)
{
    pmk_model *m = new (std::nothrow) pmk_model();
    if (!m) { set_error("out of memory"); return -100; }
    m->ctx = ctx; m->D = D; m->P = P;
    m->dtype = dtype; m->esz = dtype == PMK_F32 ? 4 : 8;
    m->desc.resize((size_t)P);
    int64_t a = 0, xo = 0, yo = 0, io = 0;
    for (int64_t r = 0; r < P; ++r) {
        if (n[r] < 1 || n[r] > (1 << 24)) {
            set_error("%s: patch %lld has n=%lld (the reference asserts a non-empty patch)", who, (long long)(first_leaf + r),
                      (long long)n[r]);
            delete m;
            return -4;
        }
        PatchDesc &d = m->desc[(size_t)r];
        d.n = (int32_t)n[r];
        d.nt = (int32_t)((n[r] + TILE - 1) / TILE);
        d.ld = d.nt * TILE;
        d.pad_ = 0;
        d.aoff = a; d.xoff = xo; d.yoff = yo; d.ioff = io;
        a += (int64_t)d.ld * d.ld;
        xo += (int64_t)d.ld * D;
        yo += d.ld;
        io += (int64_t)d.nt * 4 * 32 * 32;
        m->max_nt = std::max(m->max_nt, (int)d.nt);
    }
    m->tot_a = a; m->tot_x = xo; m->tot_y = yo; m->tot_inv = io;
    int rc = 0;
    rc |= dev_alloc(&m->d_desc, P);
    auto alloc_real = [&](void **p, int64_t count) {
        *p = nullptr;
        return hipMalloc(p, m->esz * (size_t)std::max<int64_t>(count, 1)) == hipSuccess ? 0 : -100;
    };
    rc |= alloc_real(&m->d_x, xo);
    rc |= alloc_real(&m->d_y, yo);
    rc |= alloc_real(&m->d_z, yo);
    rc |= alloc_real(&m->d_c, yo);
    rc |= alloc_real(&m->d_a, a);
    rc |= alloc_real(&m->d_inv, io);
    rc |= dev_alloc(&m->d_info, P);
    rc |= dev_alloc(&m->d_order, P);
    if (rc) { pmk_model_destroy(m); return -100; }
    // factorisation order: by tile count, largest first (stable, so equal sizes keep the caller's order)
    std::vector<int32_t> order((size_t)P);
    for (int64_t r = 0; r < P; ++r) order[(size_t)r] = (int32_t)r;
    std::stable_sort(order.begin(), order.end(),
                     [&](int32_t a2, int32_t b2) { return m->desc[(size_t)a2].nt > m->desc[(size_t)b2].nt; });
    // one workgroup per block row fills the chip only if there are enough patches: P (max_nt - 1) / 2 block rows per
    // step on average against two workgroups per CU.  Below that -- single large problems, fitRKHS! at scale -- the
    // factorisation takes the split path (pmk_chol.hip).  The two paths sum in different orders (last-bit differences
    // in L), so the choice is kept away from everyday batches: only patches of >= 32 tiles (n > 3968) qualify, and a
    // model and its shards -- which hold the same patch sizes -- then decide alike unless they straddle P's bound.
    // On the split path the factor's bits are a function of the patch and of max_nt (launch_cholesky: nsplit_of), so
    // shards reproduce the single model bit for bit where their largest patch has as many tiles as the model's.
    m->split_mode = m->max_nt >= 32 && P * (int64_t)(m->max_nt - 1) / 2 < 2 * (int64_t)ctx->num_cu;
    m->active_prefix.assign((size_t)m->max_nt + 2, 0);
    for (int64_t r = 0; r < P; ++r)
        for (int t = 0; t <= m->desc[(size_t)r].nt; ++t) ++m->active_prefix[(size_t)t];
    // d_info on the context's (non-blocking) stream: a null-stream memset would not be ordered with the fit that follows
    if (hipMemcpy(m->d_order, order.data(), sizeof(int32_t) * (size_t)P, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(m->d_desc, m->desc.data(), sizeof(PatchDesc) * (size_t)P, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemsetAsync(m->d_info, 0, sizeof(int32_t) * (size_t)P, ctx->stream) != hipSuccess) {
        set_error("%s: upload failed", who);
        pmk_model_destroy(m);
        return -100;
    }
    *out = m;
    return 0;
}

int pmk_model_create_ex(pmk_ctx *ctx, int D, int64_t P, const int64_t *n, const double *const *X,
                        const double *const *y, int dtype, pmk_model **out)
{
    if (!out) { set_error("pmk_model_create: out is NULL"); return -7; }
    *out = nullptr;
    if (dtype != PMK_F64 && dtype != PMK_F32) { set_error("pmk_model_create: unknown dtype %d", dtype); return -8; }
    if (!ctx) { set_error("pmk_model_create: ctx is NULL"); return -1; }
    if (D < 1 || D > MAX_D) { set_error("pmk_model_create: D=%d outside 1..%d", D, MAX_D); return -2; }
    if (P < 1 || !n || !X || !y) { set_error("pmk_model_create: no patches"); return -3; }
    PMK_HIP(hipSetDevice(ctx->device));
    for (int64_t r = 0; r < P; ++r) {
        if (n[r] < 1 || n[r] > (1 << 24) || !X[r]) {
            set_error("pmk_model_create: patch %lld has n=%lld (the reference asserts a non-empty patch)", (long long)r,
                      (long long)n[r]);
            return -4;
        }
    }
    pmk_model *m = nullptr;
    int rc = model_geometry(ctx, D, P, n, dtype, "pmk_model_create", 0, &m);
    if (rc) return rc;
    {
        std::vector<double> hx((size_t)m->tot_x);
        for (int64_t r = 0; r < P; ++r) {
            const PatchDesc &d = m->desc[(size_t)r];
            pack_soa(D, d.n, d.ld, X[r], hx.data() + d.xoff);
        }
        if (upload_real(m, m->d_x, 0, hx.data(), hx.size())) {
            set_error("pmk_model_create: upload failed");
            pmk_model_destroy(m);
            return -100;
        }
    }
    rc = upload_targets(m, y);
    if (rc) { pmk_model_destroy(m); return rc; }
    *out = m;
    return 0;
}

// ------------------------------------------------------------------------------------------ tree + global points
// a global array of `count` doubles where the gather kernels can read it: the caller's device pointer as it is (nothing
// waits), or a copy in the model's staging buffer (returns once the host array has been read)
static int global_source(pmk_model *m, const double *src, size_t count, const double **d_src)
{
    hipStream_t s = m->ctx->stream;
    if (is_device_pointer(src)) { *d_src = src; return 0; }
    const size_t bytes = sizeof(double) * std::max<size_t>(count, 1);
    if (m->gstage_bytes < bytes) {
        PMK_HIP(hipStreamSynchronize(s));        // an earlier gather may still read the old one
        dev_free(m->d_gstage);
        m->gstage_bytes = 0;
        PMK_HIP(hipMalloc((void **)&m->d_gstage, bytes));
        m->gstage_bytes = bytes;
    }
    PMK_HIP(hipMemcpyAsync(m->d_gstage, src, sizeof(double) * count, hipMemcpyHostToDevice, s));
    PMK_HIP(hipStreamSynchronize(s));
    *d_src = m->d_gstage;
    return 0;
}

int pmk_model_create_from_bsp(pmk_ctx *ctx, const pmk_bsp *bsp, int64_t N, const double *X, const double *y, double eps,
                              int64_t leaf_base, int64_t P, int dtype, pmk_model **out)
{
    if (!out) { set_error("pmk_model_create_from_bsp: out is NULL"); return -7; }
    *out = nullptr;
    if (dtype != PMK_F64 && dtype != PMK_F32) { set_error("pmk_model_create_from_bsp: unknown dtype %d", dtype); return -8; }
    if (!ctx || !bsp || !X) { set_error("pmk_model_create_from_bsp: NULL argument"); return -1; }
    const BspArrays &t = bsp->t;
    if (t.D < 1 || t.D > MAX_D) { set_error("pmk_model_create_from_bsp: D=%d outside 1..%d", t.D, MAX_D); return -2; }
    if (N < 1) { set_error("pmk_model_create_from_bsp: no points"); return -3; }
    if (N >= 0x7fffffff) { set_error("pmk_model_create_from_bsp: N must be below 2^31-1"); return -5; }
    // only eps < 0 selects the tree's own leaves; a NaN is an eps like any other: it assigns no point to any leaf (every
    // comparison of find-eps-partitions fails), exactly as pmk_bsp_assign does, and the empty patch is refused below
    const bool leaves = eps < 0;
    if (leaves && N != t.N) {
        set_error("pmk_model_create_from_bsp: the tree's own leaves hold %lld points, N = %lld", (long long)t.N, (long long)N);
        return -3;
    }
    if (P == 0) P = t.P - leaf_base;
    if (leaf_base < 0 || P < 1 || leaf_base + P > t.P) {
        set_error("pmk_model_create_from_bsp: leaves [%lld, %lld) outside the tree's %lld leaves", (long long)leaf_base,
                  (long long)(leaf_base + P), (long long)t.P);
        return -3;
    }
    PMK_HIP(hipSetDevice(ctx->device));
    std::vector<int64_t> off((size_t)t.P + 1);
    DevTmp<int32_t> d_all;                       // the index list of ALL leaves
    DevTmp<double> d_X;
    int rc = bsp_patch_index_device(ctx, t, N, X, leaves ? -1.0 : eps, off.data(), &d_all.p, &d_X.p);
    if (rc) return rc;
    std::vector<int64_t> n((size_t)P);
    for (int64_t r = 0; r < P; ++r) n[(size_t)r] = off[(size_t)(leaf_base + r + 1)] - off[(size_t)(leaf_base + r)];
    pmk_model *m = nullptr;
    rc = model_geometry(ctx, t.D, P, n.data(), dtype, "pmk_model_create_from_bsp", leaf_base, &m);
    if (rc) return rc;
    // the model's own index list: the leaves [leaf_base, leaf_base + P) of the sorted list, offsets from 0
    m->from_bsp = true;
    m->N_global = N;
    m->pidx_off.resize((size_t)P + 1);
    std::vector<int32_t> chunk((size_t)P + 1, 0);
    for (int64_t r = 0; r <= P; ++r) m->pidx_off[(size_t)r] = off[(size_t)(leaf_base + r)] - off[(size_t)leaf_base];
    for (int64_t r = 0; r < P; ++r) chunk[(size_t)r + 1] = chunk[(size_t)r] + (m->desc[(size_t)r].ld + 255) / 256;
    m->gchunks = chunk[(size_t)P];
    const int64_t total = m->pidx_off[(size_t)P];
    hipStream_t s = ctx->stream;
    const double *d_y = nullptr;
    if (dev_alloc(&m->d_pidx, total) || dev_alloc(&m->d_pidx_off, P + 1) || dev_alloc(&m->d_gchunk, P + 1) ||
        (y && global_source(m, y, (size_t)N, &d_y)) ||
        hipMemcpyAsync(m->d_pidx, d_all.p + off[(size_t)leaf_base], sizeof(int32_t) * (size_t)total, hipMemcpyDeviceToDevice, s) != hipSuccess ||
        hipMemcpyAsync(m->d_pidx_off, m->pidx_off.data(), sizeof(int64_t) * (size_t)(P + 1), hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemcpyAsync(m->d_gchunk, chunk.data(), sizeof(int32_t) * (size_t)(P + 1), hipMemcpyHostToDevice, s) != hipSuccess) {
        set_error("pmk_model_create_from_bsp: upload failed");
        pmk_model_destroy(m);
        return -100;
    }
    rc = PMK_BY_DTYPE(m, launch_gather_points(m, d_X.p, d_y, s));
    if (!rc && hipStreamSynchronize(s) != hipSuccess) { set_error("pmk_model_create_from_bsp: gather failed"); rc = -100; }
    if (!rc) rc = pmk_model_set_bsp(m, bsp, leaf_base);
    if (rc) { pmk_model_destroy(m); return rc; }
    *out = m;
    return 0;
}

int pmk_model_patch_index(pmk_model *m, int64_t *N, int64_t *offsets, int64_t *inds)
{
    if (!m) { set_error("pmk_model_patch_index: model is NULL"); return -1; }
    if (!m->from_bsp) { set_error("pmk_model_patch_index: the model was not made by pmk_model_create_from_bsp"); return -3; }
    if (N) *N = m->N_global;
    if (offsets) std::copy(m->pidx_off.begin(), m->pidx_off.end(), offsets);
    if (inds) {
        const int64_t total = m->pidx_off[(size_t)m->P];
        std::vector<int32_t> h32((size_t)total);
        PMK_HIP(hipSetDevice(m->ctx->device));
        PMK_HIP(hipMemcpyAsync(h32.data(), m->d_pidx, sizeof(int32_t) * (size_t)total, hipMemcpyDeviceToHost, m->ctx->stream));
        PMK_HIP(hipStreamSynchronize(m->ctx->stream));
        for (int64_t i = 0; i < total; ++i) inds[i] = h32[(size_t)i];
    }
    return 0;
}

int pmk_model_set_targets_global(pmk_model *m, const double *y)
{
    if (!m || !y) { set_error("pmk_model_set_targets_global: NULL argument"); return -1; }
    if (!m->from_bsp) { set_error("pmk_model_set_targets_global: the model was not made by pmk_model_create_from_bsp"); return -3; }
    PMK_HIP(hipSetDevice(m->ctx->device));
    m->fitted = false;
    const double *d_src = nullptr;
    if (int rc = global_source(m, y, (size_t)m->N_global, &d_src)) return rc;
    return PMK_BY_DTYPE(m, launch_gather_vector(m, d_src, m->d_y, m->ctx->stream));
}

int pmk_model_set_diag_global(pmk_model *m, const double *diag)
{
    if (!m) { set_error("pmk_model_set_diag_global: model is NULL"); return -1; }
    if (!m->from_bsp) { set_error("pmk_model_set_diag_global: the model was not made by pmk_model_create_from_bsp"); return -3; }
    PMK_HIP(hipSetDevice(m->ctx->device));
    m->fitted = false;
    if (!diag) {
        // the buffer may still be read by an enqueued fit: drain the stream before it goes (the one blocking case)
        PMK_HIP(hipStreamSynchronize(m->ctx->stream));
        if (m->d_diag) (void)hipFree(m->d_diag);
        m->d_diag = nullptr;
        return 0;
    }
    if (!m->d_diag && hipMalloc(&m->d_diag, m->esz * (size_t)std::max<int64_t>(m->tot_y, 1)) != hipSuccess) {
        set_error("pmk_model_set_diag_global: out of device memory");
        return -100;
    }
    const double *d_src = nullptr;
    if (int rc = global_source(m, diag, (size_t)m->N_global, &d_src)) return rc;
    return PMK_BY_DTYPE(m, launch_gather_vector(m, d_src, m->d_diag, m->ctx->stream));
}

int pmk_model_set_targets_multi_global(pmk_model *m, int R, const double *Y, int64_t ldy)
{
    if (!m || !Y) { set_error("pmk_model_set_targets_multi_global: NULL argument"); return -1; }
    if (!m->from_bsp) {
        set_error("pmk_model_set_targets_multi_global: the model was not made by pmk_model_create_from_bsp");
        return -3;
    }
    if (R < 1 || R > PMK_MAX_OUTPUTS) {
        set_error("pmk_model_set_targets_multi_global: R=%d outside 1..%d", R, PMK_MAX_OUTPUTS);
        return -2;
    }
    if (ldy < m->N_global) {
        set_error("pmk_model_set_targets_multi_global: ldy = %lld < N = %lld", (long long)ldy, (long long)m->N_global);
        return -3;
    }
    PMK_HIP(hipSetDevice(m->ctx->device));
    const size_t count = (size_t)m->tot_y * PMK_MAX_OUTPUTS;
    if (!m->d_ym) {
        if (hipMalloc(&m->d_ym, m->esz * count) != hipSuccess || hipMalloc(&m->d_cm, m->esz * count) != hipSuccess) {
            set_error("pmk_model_set_targets_multi_global: out of device memory");
            return -100;
        }
    }
    m->R_multi = 0;
    m->multi_solved = false;
    const double *d_src = nullptr;
    if (int rc = global_source(m, Y, (size_t)(ldy * (R - 1) + m->N_global), &d_src)) return rc;
    if (int rc = PMK_BY_DTYPE(m, launch_gather_multi(m, R, d_src, ldy, m->ctx->stream))) return rc;
    m->trend_cols_dirty = false;        // the whole block was rewritten: columns >= R are zero
    m->R_multi = R;
    return 0;
}

int pmk_model_set_diag(pmk_model *m, const double *const *diag)
{
    if (!m) { set_error("pmk_model_set_diag: model is NULL"); return -1; }
    PMK_HIP(hipSetDevice(m->ctx->device));
    PMK_HIP(hipStreamSynchronize(m->ctx->stream));
    m->fitted = false;
    if (!diag) {
        if (m->d_diag) (void)hipFree(m->d_diag);
        m->d_diag = nullptr;
        return 0;
    }
    if (!m->d_diag && hipMalloc(&m->d_diag, m->esz * (size_t)std::max<int64_t>(m->tot_y, 1)) != hipSuccess) {
        set_error("pmk_model_set_diag: out of device memory");
        return -100;
    }
    std::vector<double> hd((size_t)m->tot_y, 0.0);
    for (int64_t r = 0; r < m->P; ++r) {
        if (!diag[r]) { set_error("pmk_model_set_diag: the addends of patch %lld are NULL", (long long)r); return -2; }
        std::memcpy(hd.data() + m->desc[(size_t)r].yoff, diag[r], sizeof(double) * (size_t)m->desc[(size_t)r].n);
    }
    return upload_real(m, m->d_diag, 0, hd.data(), hd.size());
}

int pmk_model_set_targets(pmk_model *m, const double *const *y)
{
    if (!m || !y) { set_error("pmk_model_set_targets: NULL argument"); return -1; }
    PMK_HIP(hipSetDevice(m->ctx->device));
    PMK_HIP(hipStreamSynchronize(m->ctx->stream));
    m->fitted = false;
    return upload_targets(m, y);
}

/* include/pmk_test.h: force the factorisation path of a model (tests compare the two on the same data) */
int pmk_test_model_set_split(pmk_model *m, int on)
{
    if (!m) { set_error("pmk_test_model_set_split: model is NULL"); return -1; }
    for (const PatchDesc &d : m->desc)
        if (on != 0 && d.ld != d.nt * TILE) {       // the split solves read ld as the patch's extent
            set_error("pmk_test_model_set_split: the model holds reserved rows (pmk_model_reserve)");
            return -3;
        }
    m->split_mode = on != 0 && m->max_nt >= 2;
    m->chain_mode = on == 2 ? 0 : on == 3 ? 1 : -1;
    return 0;
}

/* include/pmk_test.h: where the model's buffers are */
int pmk_test_model_buffers(pmk_model *m, int64_t *slabs, int64_t *points, int64_t *weights)
{
    if (!m) { set_error("pmk_test_model_buffers: model is NULL"); return -1; }
    if (slabs) *slabs = (int64_t)reinterpret_cast<intptr_t>(m->d_a);
    if (points) *points = (int64_t)reinterpret_cast<intptr_t>(m->d_x);
    if (weights) *weights = (int64_t)reinterpret_cast<intptr_t>(m->d_c);
    return 0;
}

/* include/pmk_test.h: the two pure functions behind the loop form of the factorisation steps' GEMMs */
int pmk_test_gemm_buf_extent_ok(int64_t K, int64_t ld, int pfj, int elem_size)
{
    return gemm_buf_extent_ok(K, ld, pfj, elem_size) ? 1 : 0;
}

int pmk_test_step_gemm_rule(int G, int k, int f32, int fused) { return step_gemm_rule(G, k, f32 != 0, fused != 0); }

/* include/pmk_test.h: the packed buffers of one patch, padding rows included */
int pmk_test_model_packed(pmk_model *m, int64_t patch, int what, int64_t *ld, double *out)
{
    if (!m || patch < 0 || patch >= m->P) { set_error("pmk_test_model_packed: bad model or patch"); return -1; }
    const PatchDesc &d = m->desc[(size_t)patch];
    if (ld) *ld = d.ld;
    const void *src = what == 0 ? m->d_x : what == 1 ? m->d_y : what == 2 ? m->d_diag : what == 3 ? m->d_ym : nullptr;
    if (what < 0 || what > 3) { set_error("pmk_test_model_packed: unknown buffer %d", what); return -2; }
    if (!src || (what == 3 && m->R_multi < 1)) { set_error("pmk_test_model_packed: the buffer is not set"); return -3; }
    if (!out) return 0;
    PMK_HIP(hipSetDevice(m->ctx->device));
    const int64_t off = what == 0 ? d.xoff : what == 3 ? d.yoff * PMK_MAX_OUTPUTS : d.yoff;
    const int64_t count = (int64_t)d.ld * (what == 0 ? m->D : what == 3 ? PMK_MAX_OUTPUTS : 1);
    return download_real_2d(m, out, count, src, off, count, count, 1, m->ctx->stream);
}

// PMK_STEP_GEMM: the loop form of the factorisation steps' GEMMs (pmk_chol.hip).  ptr | buf force one form in every
// launch (A/B runs, tests); auto, the default, asks step_gemm_rule per launch.  Both forms give the same bits.  Any other
// value is an error (-2): a misspelt arm of an A/B run must not quietly measure the default.
static int step_gemm_env(int *form)
{
    const char *e = std::getenv("PMK_STEP_GEMM");
    if (!e || !*e || !std::strcmp(e, "auto")) *form = -1;
    else if (!std::strcmp(e, "ptr")) *form = pmk::STEP_GEMM_PTR;
    else if (!std::strcmp(e, "buf")) *form = pmk::STEP_GEMM_BUF;
    else { set_error("PMK_STEP_GEMM=%s: expected ptr, buf or auto", e); return -2; }
    return 0;
}

// The three timed stages of a fit: kernel matrix (th as the launchers take it, m->fuse_k1 decided by the caller),
// factorisation, solve.  The "fit" timer around them and the fitted flag stay with the caller.
static int fit_stages(pmk_model *m, const pmk_kernel_desc *th, double sigma2)
{
    pmk_ctx *c = m->ctx;
    int rc;
    c->tic("kernel_matrix");
    if ((rc = PMK_BY_DTYPE(m, launch_kernel_matrix_slabs(m, th, sigma2, c->stream, 0, m->P, m->fuse_k1)))) return rc;
    c->toc("kernel_matrix");
    c->tic("cholesky");
    if ((rc = PMK_BY_DTYPE(m, launch_cholesky(m, c->stream, 0, m->P)))) return rc;
    c->toc("cholesky");
    c->tic("solve");
    if ((rc = PMK_BY_DTYPE(m, launch_backsolve(m, c->stream, 0, m->P)))) return rc;
    c->toc("solve");
    return 0;
}

int pmk_model_fit(pmk_model *m, const pmk_kernel_desc *th, double sigma2)
{
    if (!m) { set_error("pmk_model_fit: model is NULL"); return -1; }
    if (!kernel_ok(th)) { set_error("pmk_model_fit: unknown kernel family"); return -2; }
    PMK_HIP(hipSetDevice(m->ctx->device));
    pmk_ctx *c = m->ctx;
    m->th = *th;
    m->sigma2 = sigma2;
    m->ths.assign((size_t)m->P, *th);   // the model's hyperparameters (pmk_model_get_hyper, the *_fitted calls): host only
    m->sigma2s.assign((size_t)m->P, sigma2);
    m->hyper_uniform = true;
    m->hyper_s34 = th->family == PMK_SPLINE34;
    m->multi_solved = false;            // a new factor: the multi-output weights are stale
    m->loo_valid = false;               // ... and so is diag((L L^T)^-1)
    m->loaded = false;
    c->tic("fit");
    // Fused kernel-matrix build (PMK_FUSE_K1=0 turns it off): for the compact Spline34 profile in 2 or 3 dimensions K1
    // writes the diagonal 128 x 128 tiles only, and the factorisation's step launches evaluate every tile below them at
    // its one use instead of reading it from the slab (same kern_eval: the same bits).  Not on the split path.
    const char *fe = std::getenv("PMK_FUSE_K1");
    const bool fuse_env = !(fe && std::atoi(fe) == 0);
    m->fuse_k1 = fuse_env && th->family == PMK_SPLINE34 && (m->D == 2 || m->D == 3) && !m->split_mode && m->max_nt >= 2;
    if (int rc = step_gemm_env(&m->step_gemm)) return rc;
    if (int rc = fit_stages(m, th, sigma2)) return rc;
    c->toc("fit");
    m->fitted = true;
    return 0;
}

// ------------------------------------------------------------------------------------------ per-patch hyperparameters
// ths[P] checked (family known, ModSqExp only in one dimension), remembered, and copied to the device.  The stream is
// drained first: an earlier *_fitted launch may still be reading the device arrays.
static int set_patch_kernels(pmk_model *m, const pmk_kernel_desc *ths, const double *sigma2, const char *who)
{
    for (int64_t r = 0; r < m->P; ++r) {
        if (!kernel_ok(&ths[r])) {
            set_error("%s: unknown kernel family %d in patch %lld", who, (int)ths[r].family, (long long)r);
            return -2;
        }
        if (ths[r].family == PMK_MODSQEXP && m->D > 1) {
            set_error("%s: patch %lld has the modulated squared-exponential kernel, which is defined for D = 1 (D = %d)", who,
                      (long long)r, m->D);
            return -2;
        }
    }
    PMK_HIP(hipSetDevice(m->ctx->device));
    PMK_HIP(hipStreamSynchronize(m->ctx->stream));
    if (!m->d_ths && (dev_alloc(&m->d_ths, m->P) || dev_alloc(&m->d_sigma2s, m->P))) return -100;
    m->ths.assign(ths, ths + m->P);
    if (sigma2) m->sigma2s.assign(sigma2, sigma2 + m->P);
    else m->sigma2s.assign((size_t)m->P, std::nan(""));        // a loaded model: the factor's noise variance is not known
    m->hyper_uniform = false;
    m->hyper_s34 = true;
    for (int64_t r = 0; r < m->P; ++r) m->hyper_s34 = m->hyper_s34 && ths[r].family == PMK_SPLINE34;
    PMK_HIP(hipMemcpy(m->d_ths, m->ths.data(), sizeof(pmk_kernel_desc) * (size_t)m->P, hipMemcpyHostToDevice));
    PMK_HIP(hipMemcpy(m->d_sigma2s, m->sigma2s.data(), sizeof(double) * (size_t)m->P, hipMemcpyHostToDevice));
    return 0;
}

int pmk_model_fit_patches(pmk_model *m, const pmk_kernel_desc *ths, const double *sigma2)
{
    if (!m || !ths || !sigma2) { set_error("pmk_model_fit_patches: NULL argument"); return -1; }
    pmk_ctx *c = m->ctx;
    int rc;
    if ((rc = set_patch_kernels(m, ths, sigma2, "pmk_model_fit_patches"))) return rc;
    m->th = ths[0];                     // what the step launches are handed; unread without the fused build
    m->sigma2 = sigma2[0];
    m->multi_solved = false;            // a new factor: the multi-output weights are stale
    m->loo_valid = false;               // ... and so is diag((L L^T)^-1)
    m->loaded = false;
    m->fitted = false;
    c->tic("fit");
    // always the whole lower triangle: the fused build evaluates tiles inside the factorisation, which knows one theta
    m->fuse_k1 = false;
    if ((rc = step_gemm_env(&m->step_gemm))) return rc;
    if ((rc = fit_stages(m, nullptr, 0.0))) return rc;
    c->toc("fit");
    m->fitted = true;
    return 0;
}

int pmk_model_set_kernels(pmk_model *m, const pmk_kernel_desc *ths)
{
    if (!m || !ths) { set_error("pmk_model_set_kernels: NULL argument"); return -1; }
    if (!m->loaded) {
        set_error("pmk_model_set_kernels: only for a model built by pmk_model_load (a fit records its own kernels)");
        return -3;
    }
    return set_patch_kernels(m, ths, nullptr, "pmk_model_set_kernels");
}

int pmk_model_get_hyper(pmk_model *m, pmk_kernel_desc *ths, double *sigma2)
{
    if (!m) { set_error("pmk_model_get_hyper: model is NULL"); return -1; }
    if (m->ths.empty()) { set_error("pmk_model_get_hyper: the model holds no kernels"); return -3; }
    if (ths) std::memcpy(ths, m->ths.data(), sizeof(pmk_kernel_desc) * (size_t)m->P);
    if (sigma2) std::memcpy(sigma2, m->sigma2s.data(), sizeof(double) * (size_t)m->P);
    return 0;
}

int pmk_model_info(pmk_model *m, int32_t *info)
{
    if (!m || !info) { set_error("pmk_model_info: NULL argument"); return -1; }
    PMK_HIP(hipSetDevice(m->ctx->device));
    PMK_HIP(hipMemcpyAsync(info, m->d_info, sizeof(int32_t) * (size_t)m->P, hipMemcpyDeviceToHost, m->ctx->stream));
    int32_t chain_err = 0;
    if (m->chain_used)
        PMK_HIP(hipMemcpyAsync(&chain_err, m->d_chain, sizeof(int32_t), hipMemcpyDeviceToHost, m->ctx->stream));
    PMK_HIP(hipStreamSynchronize(m->ctx->stream));
    if (chain_err != 0) {
        // solve_chain_kernel: a block waited 3 s for the block it depends on (never seen; bounded so that a fault ends)
        PMK_HIP(hipMemsetAsync(m->d_chain, 0, sizeof(int32_t), m->ctx->stream));
        set_error("pmk_model_fit: the chained back substitution timed out waiting for block %d", (int)chain_err - 1);
        return -4;
    }
    int worst = 0;
    for (int64_t r = 0; r < m->P; ++r) {
        // a failure reported from the identity padding (pivots n+1 .. ld are exactly 1 whatever the patch holds) would be a
        // wrong tile index or a status word written for the wrong patch: an error, not something to fold into info = n
        // (tests/test_gpu_breakdown.py plants failures at n - 1 and in the last tile of patches of every size)
        if (info[r] > m->desc[(size_t)r].n) {
            set_error("pmk_model_info: patch %lld (n = %d) reports leading minor %d", (long long)r, (int)m->desc[(size_t)r].n,
                      (int)info[r]);
            return -5;
        }
        if (info[r] > 0 && !worst) worst = 1;
    }
    return worst;
}

int64_t pmk_model_num_patches(const pmk_model *m) { return m ? m->P : -1; }

int pmk_model_get(pmk_model *m, int64_t patch, int what, double *out, int64_t ld)
{
    if (!m || !out) { set_error("pmk_model_get: NULL argument"); return -1; }
    if (patch < 0 || patch >= m->P) { set_error("pmk_model_get: patch %lld of %lld", (long long)patch, (long long)m->P); return -2; }
    const PatchDesc &d = m->desc[(size_t)patch];
    pmk_ctx *c = m->ctx;
    PMK_HIP(hipSetDevice(c->device));
    if (what != PMK_GET_K && !m->fitted) { set_error("pmk_model_get: model is not fitted"); return -3; }
    switch (what) {
    case PMK_GET_C:
        return download_real_2d(m, out, d.n, m->d_c, d.yoff, d.ld, d.n, 1, c->stream);
    case PMK_GET_L: {
        if (ld < d.n) { set_error("pmk_model_get: ld too small"); return -5; }
        if (int rc = download_real_2d(m, out, ld, m->d_a, d.aoff, d.ld, d.n, d.n, c->stream)) return rc;
        for (int64_t j = 1; j < d.n; ++j)
            for (int64_t i = 0; i < j; ++i) out[i + j * ld] = 0.0;   // .L of the reference: strict upper = 0
        return 0;
    }
    case PMK_GET_K: {
        // U_set entry (mixtureGP.jl:99): K without noise, rebuilt on demand from the resident points
        if (ld < d.n) { set_error("pmk_model_get: ld too small"); return -5; }
        if (m->ths.empty()) { set_error("pmk_model_get: no kernel set (fit first)"); return -3; }
        const pmk_kernel_desc kth = m->ths[(size_t)patch];      // the patch's own theta after pmk_model_fit_patches
        DevTmp<double> dK, dxs;
        if (dK.alloc((int64_t)d.n * d.n) || dxs.alloc((int64_t)d.ld * m->D)) return -100;
        {   // the dense host-API kernel is fp64: give it fp64 coordinates whatever the model's element type
            std::vector<double> hx((size_t)(d.ld * m->D));
            if (int rc2 = download_real_2d(m, hx.data(), d.ld, m->d_x, d.xoff, d.ld, d.ld, m->D, c->stream)) return rc2;
            PMK_HIP(hipMemcpy(dxs, hx.data(), sizeof(double) * hx.size(), hipMemcpyHostToDevice));
        }
        int rc = launch_kernel_matrix_dense(kth, m->D, d.n, dxs, d.ld, d.n, dxs, d.ld, dK, d.n, true, c->stream);
        if (!rc)
            PMK_HIP(hipMemcpy2DAsync(out, sizeof(double) * ld, dK, sizeof(double) * d.n, sizeof(double) * d.n, (size_t)d.n,
                                     hipMemcpyDeviceToHost, c->stream));
        PMK_HIP(hipStreamSynchronize(c->stream));
        if (!rc && m->d_diag) {                   // the kernel's own diagonal term is part of K (not the noise)
            std::vector<double> hd((size_t)d.n);
            if (int rc2 = download_real_2d(m, hd.data(), d.n, m->d_diag, d.yoff, d.ld, d.n, 1, c->stream)) return rc2;
            for (int64_t i = 0; i < d.n; ++i) out[i + i * ld] += hd[(size_t)i];
        }
        return rc;
    }
    case PMK_GET_LINV_DIAG:
        return download_real_2d(m, out, (int64_t)d.nt * 4096, m->d_inv, d.ioff, (int64_t)d.nt * 4096, (int64_t)d.nt * 4096, 1,
                                c->stream);
    default:
        set_error("pmk_model_get: unknown selector %d", what);
        return -3;
    }
}

int pmk_fit_batched(pmk_ctx *ctx, const pmk_kernel_desc *th, double sigma2, int D, int64_t P, const int64_t *n,
                    const double *const *X, const double *const *y, pmk_model **out, double *const *c_out,
                    int32_t *info)
{
    if (!out) { set_error("pmk_fit_batched: out is NULL"); return -9; }
    int rc = pmk_model_create(ctx, D, P, n, X, y, out);
    if (rc) return rc;
    rc = pmk_model_fit(*out, th, sigma2);
    if (rc) { pmk_model_destroy(*out); *out = nullptr; return rc; }
    std::vector<int32_t> tmp((size_t)P);
    int st = pmk_model_info(*out, info ? info : tmp.data());
    if (st < 0) return st;
    if (c_out) {
        bool every = true;
        for (int64_t r = 0; r < P; ++r) every = every && c_out[r] != nullptr;
        if (every) {
            if ((rc = pmk_model_get_weights(*out, c_out))) return rc;
        } else {
            for (int64_t r = 0; r < P; ++r)
                if (c_out[r] && (rc = pmk_model_get(*out, r, PMK_GET_C, c_out[r], 0))) return rc;
        }
    }
    return st;
}

int pmk_model_load(pmk_ctx *ctx, int D, int64_t P, const int64_t *n, const double *const *X, const double *const *c,
                   const double *const *L, const int64_t *ldl, pmk_model **out)
{
    if (!out) { set_error("pmk_model_load: out is NULL"); return -9; }
    *out = nullptr;
    if (!c || !L || !ldl) { set_error("pmk_model_load: NULL factors"); return -6; }
    // geometry + coordinates through the ordinary constructor (targets are not needed: pass c as a stand-in)
    int rc = pmk_model_create(ctx, D, P, n, X, c, out);
    if (rc) return rc;
    pmk_model *m = *out;
    std::vector<double> slab;
    for (int64_t r = 0; r < P; ++r) {
        const PatchDesc &d = m->desc[(size_t)r];
        if (!L[r] || !c[r] || ldl[r] < d.n) { set_error("pmk_model_load: bad factor of patch %lld", (long long)r); pmk_model_destroy(m); *out = nullptr; return -7; }
        slab.assign((size_t)d.ld * d.ld, 0.0);
        for (int64_t j = 0; j < d.ld; ++j) {
            if (j < d.n) for (int64_t i = j; i < d.n; ++i) slab[(size_t)(i + j * d.ld)] = L[r][i + j * ldl[r]];
            else slab[(size_t)(j + j * d.ld)] = 1.0;                      // identity padding
        }
        std::vector<double> cc((size_t)d.ld, 0.0);
        std::memcpy(cc.data(), c[r], sizeof(double) * (size_t)d.n);
        if ((rc = upload_real(m, m->d_a, d.aoff, slab.data(), slab.size())) ||
            (rc = upload_real(m, m->d_c, d.yoff, cc.data(), cc.size()))) {
            pmk_model_destroy(m);
            *out = nullptr;
            return rc;
        }
    }
    if (!(rc = PMK_BY_DTYPE(m, launch_ninv_from_slabs(m, ctx->stream))) && hipStreamSynchronize(ctx->stream) != hipSuccess) {
        set_error("pmk_model_load: %s", hipGetErrorString(hipGetLastError()));
        rc = -100;
    }
    if (rc) { pmk_model_destroy(m); *out = nullptr; return rc; }
    m->fitted = true;
    m->loaded = true;
    return 0;
}

int pmk_model_set_weights(pmk_model *m, const double *const *c)
{
    if (!m || !c) { set_error("pmk_model_set_weights: NULL argument"); return -1; }
    if (!m->fitted) { set_error("pmk_model_set_weights: model is not fitted"); return -3; }
    PMK_HIP(hipSetDevice(m->ctx->device));
    PMK_HIP(hipStreamSynchronize(m->ctx->stream));
    for (int64_t r = 0; r < m->P; ++r) {
        if (!c[r]) { set_error("pmk_model_set_weights: weights of patch %lld are NULL", (long long)r); return -2; }
        const PatchDesc &d = m->desc[(size_t)r];
        std::vector<double> cc((size_t)d.ld, 0.0);
        std::memcpy(cc.data(), c[r], sizeof(double) * (size_t)d.n);
        if (int rc = upload_real(m, m->d_c, d.yoff, cc.data(), cc.size())) return rc;
    }
    return 0;
}

int pmk_model_get_weights(pmk_model *m, double *const *c)
{
    if (!m || !c) { set_error("pmk_model_get_weights: NULL argument"); return -1; }
    if (!m->fitted) { set_error("pmk_model_get_weights: model is not fitted"); return -3; }
    PMK_HIP(hipSetDevice(m->ctx->device));
    // one transfer of the padded vector, then the patches' parts are cut out on the host
    std::vector<double> all((size_t)std::max<int64_t>(m->tot_y, 1));
    if (int rc = download_real_2d(m, all.data(), m->tot_y, m->d_c, 0, m->tot_y, m->tot_y, 1, m->ctx->stream)) return rc;
    for (int64_t r = 0; r < m->P; ++r) {
        const PatchDesc &d = m->desc[(size_t)r];
        if (!c[r]) { set_error("pmk_model_get_weights: output of patch %lld is NULL", (long long)r); return -2; }
        std::memcpy(c[r], all.data() + d.yoff, sizeof(double) * (size_t)d.n);
    }
    return 0;
}

// ------------------------------------------------------------------------------------------ the tree of a model
int pmk_model_set_bsp(pmk_model *m, const pmk_bsp *bsp, int64_t leaf_base)
{
    if (!m || !bsp) { set_error("pmk_model_set_bsp: NULL argument"); return -1; }
    const BspArrays &t = bsp->t;
    // The tree may live in the first t.D of the model's D coordinates (warp-feature kernels: the partition is built on the
    // positions, the kernel runs on positions + appended warp values).  The normals are padded with zeros: v . x, the foot
    // points z = p + t v and their distances then come out bit for bit as in t.D dimensions (the extra products are exact
    // zeros), so leaf ids, neighbour lists and t values are those of the tree's own space.
    if (t.D > m->D) { set_error("pmk_model_set_bsp: tree dimension %d > model dimension %d", t.D, m->D); return -2; }
    if (leaf_base < 0 || leaf_base + m->P > t.P) {
        set_error("pmk_model_set_bsp: leaves [%lld, %lld) outside the tree's %lld leaves", (long long)leaf_base,
                  (long long)(leaf_base + m->P), (long long)t.P);
        return -3;
    }
    PMK_HIP(hipSetDevice(m->ctx->device));
    dev_free(m->d_hv); dev_free(m->d_hc); dev_free(m->d_pre);
    if (dev_alloc(&m->d_hv, (t.P - 1) * m->D) || dev_alloc(&m->d_hc, t.P - 1) || dev_alloc(&m->d_pre, t.P - 1)) return -100;
    std::vector<int32_t> pre32((size_t)(t.P - 1));
    for (size_t i = 0; i < pre32.size(); ++i) pre32[i] = (int32_t)t.pre[i];
    if (t.P > 1) {
        std::vector<double> hv((size_t)((t.P - 1) * m->D), 0.0);
        for (int64_t h = 0; h < t.P - 1; ++h)
            for (int d = 0; d < t.D; ++d) hv[(size_t)(h * m->D + d)] = t.v[(size_t)(h * t.D + d)];
        PMK_HIP(hipMemcpy(m->d_hv, hv.data(), sizeof(double) * hv.size(), hipMemcpyHostToDevice));
        PMK_HIP(hipMemcpy(m->d_hc, t.c.data(), sizeof(double) * t.c.size(), hipMemcpyHostToDevice));
        PMK_HIP(hipMemcpy(m->d_pre, pre32.data(), sizeof(int32_t) * pre32.size(), hipMemcpyHostToDevice));
    }
    m->levels = t.levels;
    m->dot_mode = t.dot_mode;
    m->P_global = t.P;
    m->leaf_base = leaf_base;
    return 0;
}

// ------------------------------------------------------------------------------------------ multi-output targets
int pmk_model_set_targets_multi(pmk_model *m, int R, const double *const *Y, const int64_t *ldy)
{
    if (!m || !Y || !ldy) { set_error("pmk_model_set_targets_multi: NULL argument"); return -1; }
    if (R < 1 || R > PMK_MAX_OUTPUTS) {
        set_error("pmk_model_set_targets_multi: R=%d outside 1..%d", R, PMK_MAX_OUTPUTS);
        return -2;
    }
    for (int64_t r = 0; r < m->P; ++r) {
        if (!Y[r]) { set_error("pmk_model_set_targets_multi: targets of patch %lld are NULL", (long long)r); return -3; }
        if (ldy[r] < m->desc[(size_t)r].n) {
            set_error("pmk_model_set_targets_multi: ldy[%lld] = %lld < n = %d", (long long)r, (long long)ldy[r],
                      m->desc[(size_t)r].n);
            return -3;
        }
    }
    PMK_HIP(hipSetDevice(m->ctx->device));
    PMK_HIP(hipStreamSynchronize(m->ctx->stream));
    const size_t count = (size_t)m->tot_y * PMK_MAX_OUTPUTS;
    if (!m->d_ym) {
        if (hipMalloc(&m->d_ym, m->esz * count) != hipSuccess || hipMalloc(&m->d_cm, m->esz * count) != hipSuccess) {
            set_error("pmk_model_set_targets_multi: out of device memory");
            return -100;
        }
    }
    // row-major blocks of PMK_MAX_OUTPUTS columns (pmk_multi.hip): columns >= R and padding rows stay zero
    std::vector<double> hy(count, 0.0);
    for (int64_t r = 0; r < m->P; ++r) {
        const PatchDesc &d = m->desc[(size_t)r];
        double *blk = hy.data() + d.yoff * PMK_MAX_OUTPUTS;
        for (int j = 0; j < R; ++j)
            for (int64_t i = 0; i < d.n; ++i) blk[i * PMK_MAX_OUTPUTS + j] = Y[r][i + j * ldy[r]];
    }
    m->R_multi = 0;
    m->multi_solved = false;
    if (int rc = upload_real(m, m->d_ym, 0, hy.data(), count)) return rc;
    m->trend_cols_dirty = false;        // the whole block was rewritten: columns >= R are zero
    m->R_multi = R;
    return 0;
}

// basis functions of the trend the model is set to: 0, 1 or 1 + D
static int trend_q_of(const pmk_model *m)
{
    return m->trend_degree == PMK_TREND_CONSTANT ? 1 : m->trend_degree == PMK_TREND_LINEAR ? 1 + m->D : 0;
}

int pmk_model_solve_multi(pmk_model *m)
{
    if (!m) { set_error("pmk_model_solve_multi: model is NULL"); return -1; }
    if (!m->fitted) {
        set_error("pmk_model_solve_multi: no factor (run pmk_model_fit or build the model with pmk_model_load)");
        return -2;
    }
    if (m->R_multi < 1) { set_error("pmk_model_solve_multi: no multi-output targets (pmk_model_set_targets_multi)"); return -3; }
    const int R = m->R_multi, qt = trend_q_of(m);
    if (R + qt > PMK_MAX_OUTPUTS) {
        set_error("pmk_model_solve_multi: R=%d target columns and q=%d trend columns exceed %d", R, qt, PMK_MAX_OUTPUTS);
        return -3;
    }
    pmk_ctx *c = m->ctx;
    PMK_HIP(hipSetDevice(c->device));
    m->multi_solved = false;
    if (qt > 0 && !m->d_tbeta) {
        if (dev_alloc(&m->d_tbeta, m->P * 5 * PMK_MAX_OUTPUTS) || dev_alloc(&m->d_tL, m->P * 25) ||
            dev_alloc(&m->d_tG, m->P * 25) || dev_alloc(&m->d_tinfo, m->P))
            return -100;
    }
    c->tic("solve_multi");
    int rc = 0;
    // H into columns R .. R+q-1 of Y; with the trend back at none, one fill with q = 0 clears what an earlier solve left
    if (qt > 0 || m->trend_cols_dirty) {
        rc = PMK_BY_DTYPE(m, launch_trend_fill(m, R, qt, c->stream));
        if (!rc) m->trend_cols_dirty = qt > 0;
    }
    if (!rc) rc = PMK_BY_DTYPE(m, launch_solve_multi(m, c->stream));
    c->toc("solve_multi");
    if (rc) return rc;
    if (qt > 0) {
        c->tic("trend_gls");
        rc = PMK_BY_DTYPE(m, launch_trend_gls(m, R, qt, c->stream));
        c->toc("trend_gls");
        if (rc) return rc;
    }
    m->trend_q = qt;
    m->multi_solved = true;
    return 0;
}

int pmk_model_set_trend(pmk_model *m, int degree)
{
    if (!m) { set_error("pmk_model_set_trend: model is NULL"); return -1; }
    if (degree != PMK_TREND_NONE && degree != PMK_TREND_CONSTANT && degree != PMK_TREND_LINEAR) {
        set_error("pmk_model_set_trend: unknown degree %d (PMK_TREND_NONE, _CONSTANT or _LINEAR)", degree);
        return -2;
    }
    m->trend_degree = degree;
    m->multi_solved = false;            // the resident weights belong to the previous trend
    return 0;
}

int pmk_model_get_trend(pmk_model *m, int *q, double *beta, double *G)
{
    if (!m) { set_error("pmk_model_get_trend: model is NULL"); return -1; }
    if (!m->multi_solved) { set_error("pmk_model_get_trend: pmk_model_solve_multi has not run"); return -3; }
    const int qt = m->trend_q, R = m->R_multi;
    if (q) *q = qt;
    if (qt == 0 || (!beta && !G)) return 0;
    PMK_HIP(hipSetDevice(m->ctx->device));
    std::vector<double> hb((size_t)m->P * 5 * PMK_MAX_OUTPUTS), hg((size_t)m->P * 25);
    if (beta) PMK_HIP(hipMemcpyAsync(hb.data(), m->d_tbeta, sizeof(double) * hb.size(), hipMemcpyDeviceToHost, m->ctx->stream));
    if (G) PMK_HIP(hipMemcpyAsync(hg.data(), m->d_tG, sizeof(double) * hg.size(), hipMemcpyDeviceToHost, m->ctx->stream));
    PMK_HIP(hipStreamSynchronize(m->ctx->stream));
    for (int64_t r = 0; r < m->P; ++r) {
        if (beta)
            for (int j = 0; j < R; ++j)
                for (int a = 0; a < qt; ++a) beta[a + qt * (j + (int64_t)R * r)] = hb[(size_t)((r * PMK_MAX_OUTPUTS + j) * 5 + a)];
        if (G)
            for (int b = 0; b < qt; ++b)
                for (int a = 0; a < qt; ++a) G[a + qt * (b + (int64_t)qt * r)] = hg[(size_t)(r * 25 + a + 5 * b)];
    }
    return 0;
}

int pmk_model_trend_info(pmk_model *m, int32_t *tinfo)
{
    if (!m || !tinfo) { set_error("pmk_model_trend_info: NULL argument"); return -1; }
    if (!m->multi_solved) { set_error("pmk_model_trend_info: pmk_model_solve_multi has not run"); return -3; }
    if (m->trend_q == 0) {
        for (int64_t r = 0; r < m->P; ++r) tinfo[r] = 0;
        return 0;
    }
    PMK_HIP(hipSetDevice(m->ctx->device));
    PMK_HIP(hipMemcpyAsync(tinfo, m->d_tinfo, sizeof(int32_t) * (size_t)m->P, hipMemcpyDeviceToHost, m->ctx->stream));
    PMK_HIP(hipStreamSynchronize(m->ctx->stream));
    for (int64_t r = 0; r < m->P; ++r)
        if (tinfo[r] != 0) return 1;
    return 0;
}

int pmk_model_get_weights_multi(pmk_model *m, double *const *C, const int64_t *ldc)
{
    if (!m || !C || !ldc) { set_error("pmk_model_get_weights_multi: NULL argument"); return -1; }
    if (!m->multi_solved) { set_error("pmk_model_get_weights_multi: pmk_model_solve_multi has not run"); return -3; }
    for (int64_t r = 0; r < m->P; ++r)
        if (!C[r] || ldc[r] < m->desc[(size_t)r].n) {
            set_error("pmk_model_get_weights_multi: bad output of patch %lld", (long long)r);
            return -2;
        }
    PMK_HIP(hipSetDevice(m->ctx->device));
    const int64_t count = m->tot_y * PMK_MAX_OUTPUTS;
    std::vector<double> all((size_t)count);
    if (int rc = download_real_2d(m, all.data(), count, m->d_cm, 0, count, count, 1, m->ctx->stream)) return rc;
    for (int64_t r = 0; r < m->P; ++r) {
        const PatchDesc &d = m->desc[(size_t)r];
        const double *blk = all.data() + d.yoff * PMK_MAX_OUTPUTS;
        for (int j = 0; j < m->R_multi; ++j)
            for (int64_t i = 0; i < d.n; ++i) C[r][i + j * ldc[r]] = blk[i * PMK_MAX_OUTPUTS + j];
    }
    return 0;
}

// ------------------------------------------------------------------------------------------ model selection
static int evidence_common(pmk_model *m, int R, double *logdet, double *quad)
{
    pmk_ctx *c = m->ctx;
    PMK_HIP(hipSetDevice(c->device));
    const int cols = R ? R : 1;
    DevTmp<double> dl, dq;
    if ((logdet && dl.alloc(m->P)) || (quad && dq.alloc(m->P * cols))) return -100;
    c->tic("evidence");
    const int rc = PMK_BY_DTYPE(m, launch_evidence(m, R, dl, dq, c->stream));
    c->toc("evidence");
    if (rc) return rc;
    if (logdet) PMK_HIP(hipMemcpyAsync(logdet, dl, sizeof(double) * (size_t)m->P, hipMemcpyDeviceToHost, c->stream));
    if (quad) PMK_HIP(hipMemcpyAsync(quad, dq, sizeof(double) * (size_t)(m->P * cols), hipMemcpyDeviceToHost, c->stream));
    PMK_HIP(hipStreamSynchronize(c->stream));
    return 0;
}

int pmk_model_evidence(pmk_model *m, double *logdet, double *quad)
{
    if (!m) { set_error("pmk_model_evidence: model is NULL"); return -1; }
    if (!m->fitted) {
        set_error("pmk_model_evidence: no factor (run pmk_model_fit or build the model with pmk_model_load)");
        return -2;
    }
    if (quad && m->loaded) {
        set_error("pmk_model_evidence: a model built by pmk_model_load holds no targets; pass quad = NULL");
        return -3;
    }
    return evidence_common(m, 0, logdet, quad);
}

int pmk_model_evidence_multi(pmk_model *m, double *logdet, double *quad)
{
    if (!m) { set_error("pmk_model_evidence_multi: model is NULL"); return -1; }
    if (!m->fitted) {
        set_error("pmk_model_evidence_multi: no factor (run pmk_model_fit or build the model with pmk_model_load)");
        return -2;
    }
    if (!m->multi_solved) { set_error("pmk_model_evidence_multi: pmk_model_solve_multi has not run"); return -3; }
    return evidence_common(m, m->R_multi, logdet, quad);
}

int pmk_model_loo(pmk_model *m)
{
    if (!m) { set_error("pmk_model_loo: model is NULL"); return -1; }
    if (!m->fitted) {
        set_error("pmk_model_loo: no factor (run pmk_model_fit or build the model with pmk_model_load)");
        return -2;
    }
    pmk_ctx *c = m->ctx;
    PMK_HIP(hipSetDevice(c->device));
    m->loo_valid = false;
    c->tic("loo");
    const int rc = PMK_BY_DTYPE(m, launch_loo(m, c->stream));
    c->toc("loo");
    if (rc) return rc;
    m->loo_valid = true;
    return 0;
}

// res (layout of the weights: tot_y x RP row-major, RP = 1 or PMK_MAX_OUTPUTS) and var (tot_y) on the host
static int loo_values_common(pmk_model *m, int R, std::vector<double> *res, std::vector<double> *var)
{
    pmk_ctx *c = m->ctx;
    PMK_HIP(hipSetDevice(c->device));
    const int64_t rp = R ? PMK_MAX_OUTPUTS : 1, ny = std::max<int64_t>(m->tot_y, 1);
    DevTmp<double> dr, dv;
    if ((res && dr.alloc(ny * rp)) || (var && dv.alloc(ny))) return -100;
    if (R && m->trend_q > 0) {
        if (int rc = PMK_BY_DTYPE(m, launch_trend_loo_values(m, R, m->trend_q, dr, dv, c->stream))) return rc;
    } else if (int rc = PMK_BY_DTYPE(m, launch_loo_values(m, R, dr, dv, c->stream))) return rc;
    if (res) {
        res->resize((size_t)(ny * rp));
        PMK_HIP(hipMemcpyAsync(res->data(), dr, sizeof(double) * res->size(), hipMemcpyDeviceToHost, c->stream));
    }
    if (var) {
        var->resize((size_t)ny);
        PMK_HIP(hipMemcpyAsync(var->data(), dv, sizeof(double) * var->size(), hipMemcpyDeviceToHost, c->stream));
    }
    PMK_HIP(hipStreamSynchronize(c->stream));
    return 0;
}

static int loo_state_ok(pmk_model *m, const char *who)
{
    if (!m) { set_error("%s: model is NULL", who); return -1; }
    if (!m->fitted) { set_error("%s: no factor (run pmk_model_fit or build the model with pmk_model_load)", who); return -2; }
    if (!m->loo_valid) { set_error("%s: pmk_model_loo has not run on the resident factor", who); return -3; }
    return 0;
}

int pmk_model_get_loo(pmk_model *m, double *const *res, double *const *var)
{
    if (int rc = loo_state_ok(m, "pmk_model_get_loo")) return rc;
    for (int64_t r = 0; r < m->P; ++r)
        if ((res && !res[r]) || (var && !var[r])) {
            set_error("pmk_model_get_loo: output of patch %lld is NULL", (long long)r);
            return -4;
        }
    std::vector<double> hr, hv;
    if (int rc = loo_values_common(m, 0, res ? &hr : nullptr, var ? &hv : nullptr)) return rc;
    for (int64_t r = 0; r < m->P; ++r) {
        const PatchDesc &d = m->desc[(size_t)r];
        if (res) std::memcpy(res[r], hr.data() + d.yoff, sizeof(double) * (size_t)d.n);
        if (var) std::memcpy(var[r], hv.data() + d.yoff, sizeof(double) * (size_t)d.n);
    }
    return 0;
}

int pmk_model_get_loo_multi(pmk_model *m, double *const *RES, const int64_t *ldres, double *const *var)
{
    if (int rc = loo_state_ok(m, "pmk_model_get_loo_multi")) return rc;
    if (!m->multi_solved) { set_error("pmk_model_get_loo_multi: pmk_model_solve_multi has not run"); return -3; }
    if (RES && !ldres) { set_error("pmk_model_get_loo_multi: ldres is NULL"); return -4; }
    for (int64_t r = 0; r < m->P; ++r)
        if ((RES && (!RES[r] || ldres[r] < m->desc[(size_t)r].n)) || (var && !var[r])) {
            set_error("pmk_model_get_loo_multi: bad output of patch %lld", (long long)r);
            return -4;
        }
    std::vector<double> hr, hv;
    if (int rc = loo_values_common(m, m->R_multi, RES ? &hr : nullptr, var ? &hv : nullptr)) return rc;
    for (int64_t r = 0; r < m->P; ++r) {
        const PatchDesc &d = m->desc[(size_t)r];
        if (RES) {
            const double *blk = hr.data() + d.yoff * PMK_MAX_OUTPUTS;
            for (int j = 0; j < m->R_multi; ++j)
                for (int64_t i = 0; i < d.n; ++i) RES[r][i + j * ldres[r]] = blk[i * PMK_MAX_OUTPUTS + j];
        }
        if (var) std::memcpy(var[r], hv.data() + d.yoff, sizeof(double) * (size_t)d.n);
    }
    return 0;
}

}  // extern "C"
