// C ABI of libpmk_hip.so (declared in include/pmk.h): contexts, models, queries.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>

#include "pmk_internal.h"

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

static bool kernel_ok(const pmk_kernel_desc *th)
{
    if (!th) return false;
    switch (th->family) {
    case PMK_SPLINE34: case PMK_SPLINE12: case PMK_SPLINE32: case PMK_GAUSSIAN: case PMK_RQ: case PMK_TRQ:
    case PMK_MODSQEXP: case PMK_BB10: case PMK_BB20: case PMK_BB1EPS: case PMK_BB2EPS:
        return true;
    default:
        return false;
    }
}

template <typename T>
static int dev_alloc(T **p, int64_t count)
{
    *p = nullptr;
    if (count <= 0) count = 1;
    PMK_HIP(hipMalloc((void **)p, sizeof(T) * (size_t)count));
    return 0;
}

template <typename T>
static void dev_free(T *&p)
{
    if (p) (void)hipFree((void *)p);
    p = nullptr;
}

// device temporary of a blocking host-API call: released on every return path
template <typename T>
struct DevTmp {
    T *p = nullptr;
    DevTmp() = default;
    DevTmp(const DevTmp &) = delete;
    DevTmp &operator=(const DevTmp &) = delete;
    ~DevTmp() { if (p) (void)hipFree((void *)p); }
    int alloc(int64_t count) { return dev_alloc(&p, count); }
    operator T *() const { return p; }
};

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

// point-major host points (D x n) -> SoA rows of length ld.  Padding entries are 1e300: their distance
// to any real point overflows to +inf, so a compactly supported profile evaluates to exactly 0 there.
static void pack_soa(int D, int64_t n, int64_t ld, const double *X, double *out)
{
    for (int d = 0; d < D; ++d) {
        double *row = out + (int64_t)d * ld;
        for (int64_t i = 0; i < n; ++i) row[i] = X[i * D + d];
        for (int64_t i = n; i < ld; ++i) row[i] = 1e300;
    }
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
    if (pmk::f64::set_device_attributes() || pmk::f32::set_device_attributes() || pmk::set_plan_attributes()) {
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

// ------------------------------------------------------------------------------------------ kernel matrix
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

// ------------------------------------------------------------------------------------------ model
void pmk_model_destroy(pmk_model *m)
{
    if (!m) return;
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
// true if p is device memory (what the gather kernels can read); a plain or pinned host array is staged first
static bool is_device_pointer(const void *p)
{
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();                 // an unregistered host pointer: not an error of ours
        return false;
    }
    return at.type == hipMemoryTypeDevice || at.type == hipMemoryTypeManaged;
}

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
    m->split_mode = on != 0 && m->max_nt >= 2;
    m->chain_mode = on == 2 ? 0 : on == 3 ? 1 : -1;
    return 0;
}

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

// the theta the launchers take for the model's own hyperparameters: one descriptor after a plain fit, else null for the
// per-patch device arrays
static const pmk_kernel_desc *fitted_theta(const pmk_model *m) { return m->hyper_uniform ? &m->th : nullptr; }

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

// ------------------------------------------------------------------------------------------ predict
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
    dev_free(q->d_loo_x);               // base of the leave-one-out arena (loo_reserve)
    pmk_query_destroy(q->loo_inner);
    delete q;
}

}  // extern "C"

namespace pmk {

// One device allocation cut into 256-byte aligned pieces: a query object used to own two dozen small buffers, and every
// hipFree is a device synchronisation (pmk_query_destroy: 3.4 ms of a 108 ms querymixtureGP! at config C).
struct ArenaLayout {
    size_t bytes = 0;
    size_t add(size_t n) { const size_t at = bytes; bytes = (bytes + n + 255) & ~(size_t)255; return at; }
};

// per-query-point buffers for up to Nq points, grow only.  ONE allocation; d_xq is its base (the only pointer freed).
int query_reserve(pmk_query *q, int64_t Nq)
{
    pmk_model *m = q->m;
    if (Nq <= q->nq_cap) return 0;
    const bool regrow = q->nq_cap > 0;
    dev_free(q->d_xq);
    q->d_home = nullptr; q->d_cnt = nullptr; q->d_qoff = nullptr; q->d_yq = nullptr; q->d_vq = nullptr;
    q->d_stage_r = nullptr; q->d_stage_t = nullptr; q->d_stage_p = nullptr;
    q->nq_cap = 0;
    const size_t cap = (size_t)(Nq + (regrow ? Nq / 8 : 0)), c1 = std::max<size_t>(cap, 1);
    ArenaLayout a;
    const size_t o_xq = a.add(sizeof(double) * c1 * (size_t)m->D), o_st = a.add(sizeof(double) * 4 * c1),      // PLAN_STAGE rows
                 o_yq = a.add(sizeof(double) * c1), o_vq = a.add(sizeof(double) * c1), o_qoff = a.add(sizeof(int64_t) * (c1 + 1)),
                 o_home = a.add(sizeof(int32_t) * c1), o_cnt = a.add(sizeof(int32_t) * (c1 + 1)), o_sr = a.add(sizeof(int32_t) * 4 * c1),
                 o_sp = a.add(sizeof(int32_t) * 4 * c1);
    char *base = nullptr;
    PMK_HIP(hipMalloc((void **)&base, a.bytes));
    q->d_xq = reinterpret_cast<double *>(base + o_xq);                 // o_xq == 0
    q->d_stage_t = reinterpret_cast<double *>(base + o_st);
    q->d_yq = reinterpret_cast<double *>(base + o_yq);
    q->d_vq = reinterpret_cast<double *>(base + o_vq);
    q->d_qoff = reinterpret_cast<int64_t *>(base + o_qoff);
    q->d_home = reinterpret_cast<int32_t *>(base + o_home);
    q->d_cnt = reinterpret_cast<int32_t *>(base + o_cnt);
    q->d_stage_r = reinterpret_cast<int32_t *>(base + o_sr);
    q->d_stage_p = reinterpret_cast<int32_t *>(base + o_sp);
    q->nq_cap = (int64_t)cap;
    return 0;
}

int grow_item_buffers(pmk_query *q, int64_t total);

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
    q->R_items = 0;
    q->mixed_multi = false;
    q->items_fn = q->grad_items = q->mixed_grad = false;
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

// per-item buffers, grow only: repeated plans of one query batch reuse them.  ONE allocation; d_item_t is its base.
int grow_item_buffers(pmk_query *q, int64_t total)
{
    if (total <= q->item_cap) return 0;
    dev_free(q->d_item_t);
    q->d_item_region = nullptr; q->d_item_query = nullptr; q->d_sorted_item = nullptr; q->d_item_pos = nullptr;
    q->d_item_plane = nullptr;
    q->d_u = nullptr; q->d_v = nullptr; q->d_w = nullptr;
    q->item_cap = 0;
    const size_t cap = (size_t)(total + total / 8 + 1024);
    ArenaLayout a;
    const size_t o_t = a.add(sizeof(double) * cap), o_u = a.add(sizeof(double) * cap), o_v = a.add(sizeof(double) * cap),
                 o_w = a.add(sizeof(double) * cap), o_r = a.add(sizeof(int32_t) * cap), o_q = a.add(sizeof(int32_t) * cap),
                 o_s = a.add(sizeof(int32_t) * cap), o_p = a.add(sizeof(int32_t) * cap), o_pl = a.add(sizeof(int32_t) * cap);
    char *base = nullptr;
    PMK_HIP(hipMalloc((void **)&base, a.bytes));
    q->d_item_t = reinterpret_cast<double *>(base + o_t);              // o_t == 0
    q->d_u = reinterpret_cast<double *>(base + o_u);
    q->d_v = reinterpret_cast<double *>(base + o_v);
    q->d_w = reinterpret_cast<double *>(base + o_w);
    q->d_item_region = reinterpret_cast<int32_t *>(base + o_r);
    q->d_item_query = reinterpret_cast<int32_t *>(base + o_q);
    q->d_sorted_item = reinterpret_cast<int32_t *>(base + o_s);
    q->d_item_pos = reinterpret_cast<int32_t *>(base + o_p);
    q->d_item_plane = reinterpret_cast<int32_t *>(base + o_pl);
    q->item_cap = (int64_t)cap;
    return 0;
}

}  // namespace pmk

extern "C" {

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
    if (m->P_global != q->roff_P) {
        set_error("pmk_query_plan: the model's tree changed (%lld -> %lld leaves) after the query was created",
                  (long long)q->roff_P, (long long)m->P_global);
        return -4;
    }
    c->tic("plan");
    q->planned = false;
    q->R_items = 0;
    q->mixed_multi = false;
    q->items_fn = q->grad_items = q->mixed_grad = false;
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
    if (!kernel_ok(weight_th) || weight_th->family >= PMK_BB10) {
        set_error("pmk_query_mix: the blending profile must be a stationary kernel (evalkernel(tau, theta))");
        return -2;
    }
    if (q0 < 0 || q1 > q->Nq || q0 > q1) { set_error("pmk_query_mix: bad query range"); return -3; }
    pmk_ctx *c = q->m->ctx;
    PMK_HIP(hipSetDevice(c->device));
    c->tic("mix");
    int rc = launch_mix(q, *weight_th, q0, q1, c->stream);
    c->toc("mix");
    return rc;
}

int pmk_query_fetch(pmk_query *q, double *Yq, double *Vq)
{
    if (!q) { set_error("pmk_query_fetch: query is NULL"); return -1; }
    pmk_ctx *c = q->m->ctx;
    PMK_HIP(hipSetDevice(c->device));
    if (q->Nq > 0) {
        if (Yq) PMK_HIP(hipMemcpyAsync(Yq, q->d_yq, sizeof(double) * (size_t)q->Nq, hipMemcpyDeviceToHost, c->stream));
        if (Vq) PMK_HIP(hipMemcpyAsync(Vq, q->d_vq, sizeof(double) * (size_t)q->Nq, hipMemcpyDeviceToHost, c->stream));
    }
    PMK_HIP(hipStreamSynchronize(c->stream));
    return 0;
}

int pmk_query_fetch_dev(pmk_query *q, double *Yq_dev, double *Vq_dev)
{
    if (!q) { set_error("pmk_query_fetch_dev: query is NULL"); return -1; }
    pmk_ctx *c = q->m->ctx;
    PMK_HIP(hipSetDevice(c->device));
    if (q->Nq > 0) {
        if (Yq_dev) PMK_HIP(hipMemcpyAsync(Yq_dev, q->d_yq, sizeof(double) * (size_t)q->Nq, hipMemcpyDeviceToDevice, c->stream));
        if (Vq_dev) PMK_HIP(hipMemcpyAsync(Vq_dev, q->d_vq, sizeof(double) * (size_t)q->Nq, hipMemcpyDeviceToDevice, c->stream));
    }
    return 0;
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
    if (item_u || item_v) {
        std::vector<int32_t> pos(T);
        std::vector<double> tmp(T);
        PMK_HIP(hipMemcpy(pos.data(), q->d_item_pos, sizeof(int32_t) * T, hipMemcpyDeviceToHost));
        if (item_u) {
            PMK_HIP(hipMemcpy(tmp.data(), q->d_u, sizeof(double) * T, hipMemcpyDeviceToHost));
            for (size_t i = 0; i < T; ++i) item_u[i] = tmp[(size_t)pos[i]];
        }
        if (item_v) {
            PMK_HIP(hipMemcpy(tmp.data(), q->d_v, sizeof(double) * T, hipMemcpyDeviceToHost));
            for (size_t i = 0; i < T; ++i) item_v[i] = tmp[(size_t)pos[i]];
        }
    }
    return 0;
}

int pmk_predict_mixture(pmk_model *m, const pmk_kernel_desc *th, const pmk_kernel_desc *weight_th, int64_t Nq,
                        const double *Xq, double radius, double delta, double *Yq, double *Vq)
{
    if (!m) { set_error("pmk_predict_mixture: model is NULL"); return -1; }
    if (m->P_global != m->P || m->leaf_base != 0) {
        set_error("pmk_predict_mixture: the model holds %lld of %lld leaves; use the staged pmk_query_* calls",
                  (long long)m->P, (long long)m->P_global);
        return -1;
    }
    pmk_query *q = nullptr;
    int rc = pmk_query_create(m, Nq, Xq, &q);
    if (rc) return rc;
    if (!(rc = pmk_query_plan(q, radius, delta)) && !(rc = pmk_query_items(q, th)) &&
        !(rc = pmk_query_mix(q, weight_th, 0, Nq)))
        rc = pmk_query_fetch(q, Yq, Vq);
    pmk_query_destroy(q);
    return rc;
}

int pmk_predict_mixture_fitted(pmk_model *m, const pmk_kernel_desc *weight_th, int64_t Nq, const double *Xq, double radius,
                               double delta, double *Yq, double *Vq)
{
    if (!m) { set_error("pmk_predict_mixture_fitted: model is NULL"); return -1; }
    if (m->P_global != m->P || m->leaf_base != 0) {
        set_error("pmk_predict_mixture_fitted: the model holds %lld of %lld leaves; use the staged pmk_query_* calls",
                  (long long)m->P, (long long)m->P_global);
        return -1;
    }
    pmk_query *q = nullptr;
    int rc = pmk_query_create(m, Nq, Xq, &q);
    if (rc) return rc;
    if (!(rc = pmk_query_plan(q, radius, delta)) && !(rc = pmk_query_items_fitted(q)) &&
        !(rc = pmk_query_mix(q, weight_th, 0, Nq)))
        rc = pmk_query_fetch(q, Yq, Vq);
    pmk_query_destroy(q);
    return rc;
}

// ------------------------------------------------------------------------------------------ blended leave-one-out
// buffers of pmk_query_items_loo for up to `total` sorted items, grow only.  ONE allocation; d_loo_x is its base.
static int loo_reserve(pmk_query *q, int64_t total)
{
    if (total <= q->loo_cap) return 0;
    dev_free(q->d_loo_x);
    q->d_loo_diag = nullptr; q->d_loo_ru = nullptr; q->d_loo_rv = nullptr; q->d_loo_off = nullptr;
    q->d_loo_mark = nullptr; q->d_loo_region = nullptr;
    q->loo_cap = 0;
    const size_t cap = (size_t)(total + total / 8 + 1024);
    ArenaLayout a;
    const size_t o_x = a.add(sizeof(double) * cap * (size_t)q->m->D), o_d = a.add(sizeof(double) * cap),
                 o_u = a.add(sizeof(double) * cap), o_v = a.add(sizeof(double) * cap), o_o = a.add(sizeof(int64_t) * (cap + 1)),
                 o_m = a.add(sizeof(int32_t) * (cap + 1)), o_r = a.add(sizeof(int32_t) * cap);
    char *base = nullptr;
    PMK_HIP(hipMalloc((void **)&base, a.bytes));
    q->d_loo_x = reinterpret_cast<double *>(base + o_x);               // o_x == 0
    q->d_loo_diag = reinterpret_cast<double *>(base + o_d);
    q->d_loo_ru = reinterpret_cast<double *>(base + o_u);
    q->d_loo_rv = reinterpret_cast<double *>(base + o_v);
    q->d_loo_off = reinterpret_cast<int64_t *>(base + o_o);
    q->d_loo_mark = reinterpret_cast<int32_t *>(base + o_m);
    q->d_loo_region = reinterpret_cast<int32_t *>(base + o_r);
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
    if (m->P_global != m->P || m->leaf_base != 0) {
        set_error("%s: the model holds %lld of %lld leaves; the blended leave-one-out needs every leaf", who, (long long)m->P,
                  (long long)m->P_global);
        return -3;
    }
    if (m->ths.empty()) { set_error("%s: the model holds no kernels (pmk_model_set_kernels)", who); return -3; }
    if (!m->loo_valid) { set_error("%s: pmk_model_loo has not run on the resident factor", who); return -3; }
    return 0;
}

int pmk_query_items_loo(pmk_query *q, int noisy, int64_t *n_member, int64_t *n_strip)
{
    if (!q || !q->planned) { set_error("pmk_query_items_loo: query is not planned"); return -1; }
    pmk_model *m = q->m;
    if (int rc = loo_model_ok(m, q->Nq, "pmk_query_items_loo")) return rc;
    pmk_ctx *c = m->ctx;
    PMK_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    int rc;
    int64_t ns = 0;
    noisy = noisy != 0;
    c->tic("loo_items");
    if (q->total > 0) {
        if ((rc = loo_reserve(q, q->total))) return rc;
        // members: a lookup per item, and the marks of the rest
        if ((rc = PMK_BY_DTYPE(m, launch_loo_member(q, noisy, q->d_loo_mark, s)))) return rc;
        if (exclusive_scan_i32_to_i64(q->d_loo_mark, q->d_loo_off, q->total, &q->d_tmp, &q->tmp_bytes, s)) {
            set_error("pmk_query_items_loo: prefix scan failed");
            return -100;
        }
        PMK_HIP(hipMemcpyAsync(&ns, q->d_loo_off + q->total, sizeof(int64_t), hipMemcpyDeviceToHost, s));
        PMK_HIP(hipStreamSynchronize(s));
    }
    if (ns > 0) {
        // non-members: queryinner! on the strip kernel, as explicit items of an inner query (the request / response
        // pattern of pmk_query_predict_sharded with this process as its own leaf owner)
        if (!q->loo_inner && (rc = pmk_query_create(m, 0, nullptr, &q->loo_inner))) return rc;
        pmk_query *in = q->loo_inner;
        if ((rc = PMK_BY_DTYPE(m, launch_loo_compact(q, q->d_loo_mark, q->d_loo_off, q->d_loo_x, q->d_loo_region,
                                                     q->d_loo_diag, s))))
            return rc;
        if ((rc = query_set_items(in, ns, q->d_loo_x, q->d_loo_region))) return rc;
        // the addends in request order = the inner query's item order; borrowed for this launch only (the arena is q's)
        in->d_qdiag = q->d_qdiag ? q->d_loo_diag : nullptr;
        in->min_v = q->min_v;
        rc = pmk_query_items_fitted(in);
        in->d_qdiag = nullptr;
        if (rc) return rc;
        if ((rc = launch_export_results(in, q->d_loo_ru, q->d_loo_rv, s))) return rc;
        if ((rc = PMK_BY_DTYPE(m, launch_loo_scatter(q, noisy, q->d_loo_mark, q->d_loo_off, q->d_loo_ru, q->d_loo_rv, s))))
            return rc;
    }
    c->toc("loo_items");
    if (n_member) *n_member = q->total - ns;
    if (n_strip) *n_strip = ns;
    return 0;
}

int pmk_predict_mixture_loo(pmk_model *m, const pmk_kernel_desc *weight_th, const double *X, double radius, double delta,
                            int noisy, double *Yq, double *Vq)
{
    if (!m) { set_error("pmk_predict_mixture_loo: model is NULL"); return -1; }
    int rc = loo_model_ok(m, m->N_global, "pmk_predict_mixture_loo");
    if (rc) return rc;
    if (!X) { set_error("pmk_predict_mixture_loo: X is NULL"); return -2; }
    pmk_query *q = nullptr;
    if ((rc = pmk_query_create(m, m->N_global, X, &q))) return rc;
    if (!(rc = pmk_query_plan(q, radius, delta)) && !(rc = pmk_query_items_loo(q, noisy, nullptr, nullptr)) &&
        !(rc = pmk_query_mix(q, weight_th, 0, q->Nq)))
        rc = pmk_query_fetch(q, Yq, Vq);
    pmk_query_destroy(q);
    return rc;
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

// th == NULL: the model's own per-patch kernels (pmk_query_items_multi_fitted)
static int items_multi_common(pmk_query *q, const pmk_kernel_desc *th, int want_var)
{
    pmk_model *m = q->m;
    if (m->P_global != m->P || m->leaf_base != 0) {
        set_error("pmk_query_items_multi: the model holds %lld of %lld leaves; multi-output prediction needs a model that "
                  "holds every leaf", (long long)m->P, (long long)m->P_global);
        return -4;
    }
    if (!m->multi_solved) { set_error("pmk_query_items_multi: pmk_model_solve_multi has not run"); return -3; }
    if (want_var && !m->fitted) { set_error("pmk_query_items_multi: model is not fitted"); return -3; }
    pmk_ctx *c = m->ctx;
    PMK_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const int R = m->R_multi, qt = m->trend_q;      // with a trend the items kernel also emits kq . C_H: R + q columns
    q->R_items = 0;
    q->mixed_multi = false;
    q->items_fn = q->grad_items = q->mixed_grad = false;
    // chunks of 16 items per region (item_means_kernel): prefix over the regions
    q->mcpre.assign((size_t)m->P + 1, 0);
    for (int64_t r = 0; r < m->P; ++r)
        q->mcpre[(size_t)r + 1] = q->mcpre[(size_t)r] + (q->roff[(size_t)r + 1] - q->roff[(size_t)r] + 15) / 16;
    q->mchunks = q->mcpre[(size_t)m->P];
    PMK_HIP(hipStreamSynchronize(s));       // earlier launches may still read the buffers replaced below
    if (q->mcpre_cap < m->P + 1) {
        dev_free(q->d_mcpre);
        q->mcpre_cap = 0;
        if (dev_alloc(&q->d_mcpre, m->P + 1)) return -100;
        q->mcpre_cap = m->P + 1;
    }
    if (q->um_cap < q->total * (R + qt)) {
        dev_free(q->d_um);
        q->um_cap = 0;
        if (dev_alloc(&q->d_um, q->total * (R + qt))) return -100;
        q->um_cap = q->total * (R + qt);
    }
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
    if (!kernel_ok(weight_th) || weight_th->family >= PMK_BB10) {
        set_error("pmk_query_mix_multi: the blending profile must be a stationary kernel (evalkernel(tau, theta))");
        return -2;
    }
    if (q0 < 0 || q1 > q->Nq || q0 > q1) { set_error("pmk_query_mix_multi: bad query range"); return -3; }
    pmk_ctx *c = q->m->ctx;
    PMK_HIP(hipSetDevice(c->device));
    if (q->yqm_cap < q->Nq * q->R_items) {
        PMK_HIP(hipStreamSynchronize(c->stream));
        dev_free(q->d_yqm);
        q->yqm_cap = 0;
        if (dev_alloc(&q->d_yqm, q->Nq * q->R_items)) return -100;
        q->yqm_cap = q->Nq * q->R_items;
    }
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
    if (!q) { set_error("pmk_query_fetch_multi: query is NULL"); return -1; }
    if (!q->mixed_multi || q->R_items < 1) { set_error("pmk_query_fetch_multi: pmk_query_mix_multi has not run"); return -2; }
    if (Vq && !q->var_items) {
        set_error("pmk_query_fetch_multi: Vq was not computed (pmk_query_items_multi ran with want_var = 0)");
        return -3;
    }
    if (Yq && ldyq < q->Nq) { set_error("pmk_query_fetch_multi: ldyq = %lld < Nq = %lld", (long long)ldyq, (long long)q->Nq); return -4; }
    pmk_ctx *c = q->m->ctx;
    PMK_HIP(hipSetDevice(c->device));
    if (q->Nq > 0) {
        if (Yq)
            PMK_HIP(hipMemcpy2DAsync(Yq, sizeof(double) * (size_t)ldyq, q->d_yqm, sizeof(double) * (size_t)q->Nq,
                                     sizeof(double) * (size_t)q->Nq, (size_t)q->R_items, hipMemcpyDeviceToHost, c->stream));
        if (Vq) PMK_HIP(hipMemcpyAsync(Vq, q->d_vq, sizeof(double) * (size_t)q->Nq, hipMemcpyDeviceToHost, c->stream));
    }
    PMK_HIP(hipStreamSynchronize(c->stream));
    return 0;
}

int pmk_query_fetch_multi_dev(pmk_query *q, double *Yq_dev, int64_t ldyq, double *Vq_dev)
{
    if (!q) { set_error("pmk_query_fetch_multi_dev: query is NULL"); return -1; }
    if (!q->mixed_multi || q->R_items < 1) { set_error("pmk_query_fetch_multi_dev: pmk_query_mix_multi has not run"); return -2; }
    if (Vq_dev && !q->var_items) {
        set_error("pmk_query_fetch_multi_dev: Vq was not computed (pmk_query_items_multi ran with want_var = 0)");
        return -3;
    }
    if (Yq_dev && ldyq < q->Nq) {
        set_error("pmk_query_fetch_multi_dev: ldyq = %lld < Nq = %lld", (long long)ldyq, (long long)q->Nq);
        return -4;
    }
    pmk_ctx *c = q->m->ctx;
    PMK_HIP(hipSetDevice(c->device));
    if (q->Nq > 0) {
        if (Yq_dev)
            PMK_HIP(hipMemcpy2DAsync(Yq_dev, sizeof(double) * (size_t)ldyq, q->d_yqm, sizeof(double) * (size_t)q->Nq,
                                     sizeof(double) * (size_t)q->Nq, (size_t)q->R_items, hipMemcpyDeviceToDevice, c->stream));
        if (Vq_dev) PMK_HIP(hipMemcpyAsync(Vq_dev, q->d_vq, sizeof(double) * (size_t)q->Nq, hipMemcpyDeviceToDevice, c->stream));
    }
    return 0;
}

int pmk_predict_mixture_multi(pmk_model *m, const pmk_kernel_desc *th, const pmk_kernel_desc *weight_th, int64_t Nq,
                              const double *Xq, double radius, double delta, double *Yq, int64_t ldyq, double *Vq)
{
    if (!m) { set_error("pmk_predict_mixture_multi: model is NULL"); return -1; }
    if (m->P_global != m->P || m->leaf_base != 0) {
        set_error("pmk_predict_mixture_multi: the model holds %lld of %lld leaves; multi-output prediction needs a model "
                  "that holds every leaf", (long long)m->P, (long long)m->P_global);
        return -4;
    }
    if (Yq && ldyq < Nq) { set_error("pmk_predict_mixture_multi: ldyq = %lld < Nq = %lld", (long long)ldyq, (long long)Nq); return -4; }
    pmk_query *q = nullptr;
    int rc = pmk_query_create(m, Nq, Xq, &q);
    if (rc) return rc;
    if (!(rc = pmk_query_plan(q, radius, delta)) && !(rc = pmk_query_items_multi(q, th, Vq != nullptr)) &&
        !(rc = pmk_query_mix_multi(q, weight_th, 0, Nq)))
        rc = pmk_query_fetch_multi(q, Yq, ldyq, Vq);
    pmk_query_destroy(q);
    return rc;
}

int pmk_predict_mixture_multi_fitted(pmk_model *m, const pmk_kernel_desc *weight_th, int64_t Nq, const double *Xq,
                                     double radius, double delta, double *Yq, int64_t ldyq, double *Vq)
{
    if (!m) { set_error("pmk_predict_mixture_multi_fitted: model is NULL"); return -1; }
    if (m->P_global != m->P || m->leaf_base != 0) {
        set_error("pmk_predict_mixture_multi_fitted: the model holds %lld of %lld leaves; multi-output prediction needs a "
                  "model that holds every leaf", (long long)m->P, (long long)m->P_global);
        return -4;
    }
    if (Yq && ldyq < Nq) { set_error("pmk_predict_mixture_multi_fitted: ldyq = %lld < Nq = %lld", (long long)ldyq, (long long)Nq); return -4; }
    pmk_query *q = nullptr;
    int rc = pmk_query_create(m, Nq, Xq, &q);
    if (rc) return rc;
    if (!(rc = pmk_query_plan(q, radius, delta)) && !(rc = pmk_query_items_multi_fitted(q, Vq != nullptr)) &&
        !(rc = pmk_query_mix_multi(q, weight_th, 0, Nq)))
        rc = pmk_query_fetch_multi(q, Yq, ldyq, Vq);
    pmk_query_destroy(q);
    return rc;
}

// ------------------------------------------------------------------------------------------ blended leave-one-out, R columns
// loo_model_ok plus the multi-output state; host state only
static int loo_multi_model_ok(const pmk_model *m, int64_t Nq, const char *who)
{
    if (int rc = loo_model_ok(m, Nq, who)) return rc;
    if (!m->multi_solved) { set_error("%s: pmk_model_solve_multi has not run on the resident factor", who); return -3; }
    return 0;
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
    int rc;
    int64_t ns = 0;
    noisy = noisy != 0;
    want_var = want_var != 0;
    q->R_items = 0;
    q->mixed_multi = false;
    q->items_fn = q->grad_items = q->mixed_grad = false;
    if (q->um_cap < q->total * (R + qt)) {
        PMK_HIP(hipStreamSynchronize(s));       // earlier launches may still read the buffer replaced below
        dev_free(q->d_um);
        q->um_cap = 0;
        if (dev_alloc(&q->d_um, q->total * (R + qt))) return -100;
        q->um_cap = q->total * (R + qt);
    }
    q->R_items = R;
    q->um_ld = R + qt;
    c->tic("loo_items_multi");
    if (q->total > 0) {
        if ((rc = loo_reserve(q, q->total))) { q->R_items = 0; return rc; }
        // members: a lookup per item, and the marks of the rest
        if ((rc = PMK_BY_DTYPE(m, launch_loo_member_multi(q, noisy, want_var, q->d_loo_mark, s)))) { q->R_items = 0; return rc; }
        if (exclusive_scan_i32_to_i64(q->d_loo_mark, q->d_loo_off, q->total, &q->d_tmp, &q->tmp_bytes, s)) {
            set_error("pmk_query_items_loo_multi: prefix scan failed");
            q->R_items = 0;
            return -100;
        }
        PMK_HIP(hipMemcpyAsync(&ns, q->d_loo_off + q->total, sizeof(int64_t), hipMemcpyDeviceToHost, s));
        PMK_HIP(hipStreamSynchronize(s));
    }
    if (ns > 0) {
        // non-members: the items of pmk_query_items_multi_fitted, as explicit items of the inner query
        rc = 0;
        if (!q->loo_inner) rc = pmk_query_create(m, 0, nullptr, &q->loo_inner);
        pmk_query *in = q->loo_inner;
        if (!rc)
            rc = PMK_BY_DTYPE(m, launch_loo_compact(q, q->d_loo_mark, q->d_loo_off, q->d_loo_x, q->d_loo_region, q->d_loo_diag, s));
        if (!rc) rc = query_set_items(in, ns, q->d_loo_x, q->d_loo_region);
        if (!rc) {
            // the addends in request order = the inner query's item order; borrowed for this launch only (the arena is q's)
            in->d_qdiag = q->d_qdiag ? q->d_loo_diag : nullptr;
            in->min_v = q->min_v;
            rc = pmk_query_items_multi_fitted(in, want_var);
            in->d_qdiag = nullptr;
        }
        if (!rc) rc = launch_loo_scatter_multi(q, in, noisy, want_var, q->d_loo_mark, q->d_loo_off, s);
        if (rc) { q->R_items = 0; return rc; }
    }
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
    int rc = loo_multi_model_ok(m, m->N_global, "pmk_predict_mixture_loo_multi");
    if (rc) return rc;
    if (!X) { set_error("pmk_predict_mixture_loo_multi: X is NULL"); return -2; }
    if (Yq && ldyq < m->N_global) {
        set_error("pmk_predict_mixture_loo_multi: ldyq = %lld < N = %lld", (long long)ldyq, (long long)m->N_global);
        return -4;
    }
    pmk_query *q = nullptr;
    if ((rc = pmk_query_create(m, m->N_global, X, &q))) return rc;
    if (!(rc = pmk_query_plan(q, radius, delta)) && !(rc = pmk_query_items_loo_multi(q, noisy, Vq != nullptr, nullptr, nullptr)) &&
        !(rc = pmk_query_mix_multi(q, weight_th, 0, q->Nq)))
        rc = pmk_query_fetch_multi(q, Yq, ldyq, Vq);
    pmk_query_destroy(q);
    return rc;
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
    const size_t T = (size_t)q->total, R = (size_t)q->R_items, ld = (size_t)q->um_ld;
    if (T == 0 || (!U && !v)) return 0;
    std::vector<int32_t> pos(T);
    PMK_HIP(hipMemcpy(pos.data(), q->d_item_pos, sizeof(int32_t) * T, hipMemcpyDeviceToHost));
    if (U) {
        std::vector<double> tmp(T * ld);
        PMK_HIP(hipMemcpy(tmp.data(), q->d_um, sizeof(double) * tmp.size(), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < T; ++i)
            for (size_t j = 0; j < R; ++j) U[i * (size_t)ldu + j] = tmp[(size_t)pos[i] * ld + j];
    }
    if (v) {
        std::vector<double> tmp(T);
        PMK_HIP(hipMemcpy(tmp.data(), q->d_v, sizeof(double) * T, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < T; ++i) v[i] = tmp[(size_t)pos[i]];
    }
    return 0;
}

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

int pmk_query_items_grad(pmk_query *q, const pmk_kernel_desc *th)
{
    if (!q || !q->planned) { set_error("pmk_query_items_grad: query is not planned"); return -1; }
    pmk_model *m = q->m;
    if (m->P_global != m->P || m->leaf_base != 0) {
        set_error("pmk_query_items_grad: the model holds %lld of %lld leaves; the gradient needs a model that holds every "
                  "leaf", (long long)m->P, (long long)m->P_global);
        return -4;
    }
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
    const int64_t need = q->total * m->D * q->R_items;
    if (q->gm_cap < need) {
        PMK_HIP(hipStreamSynchronize(s));       // earlier launches may still read the buffer replaced below
        dev_free(q->d_gm);
        q->gm_cap = 0;
        if (dev_alloc(&q->d_gm, need)) return -100;
        q->gm_cap = need;
    }
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
    if (q0 < 0 || q1 > q->Nq || q0 > q1) { set_error("pmk_query_mix_grad: bad query range"); return -3; }
    pmk_model *m = q->m;
    pmk_ctx *c = m->ctx;
    PMK_HIP(hipSetDevice(c->device));
    const int64_t need = q->Nq * m->D * q->R_items;
    if (q->dyq_cap < need) {
        PMK_HIP(hipStreamSynchronize(c->stream));
        dev_free(q->d_dyq);
        q->dyq_cap = 0;
        if (dev_alloc(&q->d_dyq, need)) return -100;
        q->dyq_cap = need;
    }
    c->tic("mix_grad");
    const int rc = launch_mix_grad(q, *weight_th, q0, q1, c->stream);
    c->toc("mix_grad");
    if (rc) return rc;
    q->mixed_grad = true;
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
    if (G) {
        std::vector<int32_t> pos(T);
        std::vector<double> tmp(T * DR);
        PMK_HIP(hipMemcpy(pos.data(), q->d_item_pos, sizeof(int32_t) * T, hipMemcpyDeviceToHost));
        PMK_HIP(hipMemcpy(tmp.data(), q->d_gm, sizeof(double) * tmp.size(), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < T; ++i)
            for (size_t j = 0; j < DR; ++j) G[i * (size_t)ldg + j] = tmp[(size_t)pos[i] * DR + j];
    }
    return 0;
}

int pmk_predict_mixture_grad_fitted(pmk_model *m, const pmk_kernel_desc *weight_th, int64_t Nq, const double *Xq,
                                    double radius, double delta, double *Yq, int64_t ldyq, double *dYq, int64_t lddy)
{
    if (!m) { set_error("pmk_predict_mixture_grad_fitted: model is NULL"); return -1; }
    if (m->P_global != m->P || m->leaf_base != 0) {
        set_error("pmk_predict_mixture_grad_fitted: the model holds %lld of %lld leaves; the gradient needs a model that "
                  "holds every leaf", (long long)m->P, (long long)m->P_global);
        return -4;
    }
    if ((Yq && ldyq < Nq) || (dYq && lddy < Nq)) {
        set_error("pmk_predict_mixture_grad_fitted: ldyq = %lld or lddy = %lld < Nq = %lld", (long long)ldyq, (long long)lddy,
                  (long long)Nq);
        return -4;
    }
    pmk_query *q = nullptr;
    int rc = pmk_query_create(m, Nq, Xq, &q);
    if (rc) return rc;
    if (!(rc = pmk_query_plan(q, radius, delta)) && !(rc = pmk_query_items_multi_fitted(q, 0)) &&
        !(rc = pmk_query_items_grad(q, nullptr)) && !(rc = pmk_query_mix_multi(q, weight_th, 0, Nq)) &&
        !(rc = pmk_query_mix_grad(q, weight_th, 0, Nq))) {
        if (Yq) rc = pmk_query_fetch_multi(q, Yq, ldyq, nullptr);
        if (!rc && dYq) rc = pmk_query_fetch_grad(q, dYq, lddy);
    }
    pmk_query_destroy(q);
    return rc;
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
