// K4: per-(query, region) prediction, queryinner! of the reference (src/RKHS/mixtureGP.jl:296-316)
// batched over all the queries that touch a region:
//     kq = k(xq, X_r)            (cross-kernel tile, evaluated in registers, never written to HBM)
//     u  = kq . c_r              (mean)
//     V  = L_r^-1 kq             (blocked forward substitution, every product on fp64 MFMA)
//     v  = clamp(k(xq,xq) - |V|^2, 1e-12, inf)
// The reference runs one dtrsv per (query, region) and streams the 4 n^2-byte factor each time; here a
// workgroup owns a strip of TQ = 256 query columns (8 waves x 32 columns: one workgroup per CU, two waves per
// SIMD) and sweeps the block rows of L once for all of them.
//
// Strip task, block row i:  acc(128 x 32) = Kq_i - sum_{j<i} L[i,j] V_j   (gemm_nt_indexed, V_j re-read from the
// wave's strip in global memory, which is stored negated so the MFMA accumulates the subtraction)
//                           -V_i = -L[ii]^-1 acc                          (tri_solve_global: block substitution,
//                                                                          operands prefetched from the factor)
// The schedule of a strip (what is kept off the critical path, and how) is described at the kernel.
//
// HBM traffic.  A strip streams the factor once (n^2/2 elements per TQ columns) and re-reads its own V block rows
// (n^2/(2*128) elements per column).  The factor is the operand every strip of a region shares: strips of one region
// that run at the same time on one XCD are kept in LOCK-STEP (a bounded spin on an arrival counter once per block
// row -- timing only, no data is handed over, so a missed rendezvous costs time, never correctness)
// and the block row of L is then served to all of them by ONE fetch into that XCD's L2.
#include <algorithm>
#include <tuple>

#include "pmk_dispatch.h"
#include "pmk_mfma.h"

namespace pmk {
namespace PMK_NS {

constexpr int SYNC_TICKS = 4000;    // lock-step rendezvous: give up after 40 us (s_memrealtime ticks of 10 ns)
constexpr int ROUND_TICKS = 300000; // round barrier: give up after 3 ms, and then for the rest of the launch

#ifdef PMK_TRACE
// diagnostic build only: rendezvous statistics [0] syncs, [1] timeouts, [2] total wait ticks (10 ns), [3] max wait
__device__ unsigned long long g_sync_stats[4];
// phase stamps of block row PMK_TRACE_ROW in round PMK_TRACE_ROUND: [wg][wave][8]
__device__ unsigned long long g_row_stamp[512 * 40];
#ifndef PMK_TRACE_ROW
#define PMK_TRACE_ROW 8
#endif
#ifndef PMK_TRACE_ROUND
#define PMK_TRACE_ROUND 3
#endif
#define PMK_PSTAMP(k)                                                                                        \
    do {                                                                                                     \
        if (round == PMK_TRACE_ROUND && i == PMK_TRACE_ROW && lane == 0 && blockIdx.x < 64)                   \
            g_row_stamp[(blockIdx.x * 8 + (threadIdx.x >> 6)) * 8 + (k)] = __builtin_amdgcn_s_memrealtime();               \
    } while (0)
#define PMK_TRACED (round == PMK_TRACE_ROUND)
#else
#define PMK_PSTAMP(k)
#define PMK_TRACED false
#endif

}  // namespace PMK_NS
}  // namespace pmk

// strip_block_row and the shape of a strip (shared with the leave-one-out kernel); in a trace build it stamps into
// g_row_stamp above
#ifdef PMK_TRACE
#define PMK_STRIP_STAMPS
#endif
#include "pmk_strip.h"

namespace pmk {
namespace PMK_NS {

// a wave owns a 128 x 32 tile of the strip: eight waves, two per SIMD (256 registers each)
constexpr int WCOLS = 32;           // query columns of a wave
constexpr int PRED_WAVES = TQ / WCOLS;
constexpr int PRED_THREADS = 64 * PRED_WAVES;
constexpr int NC = 2;               // query columns of a lane
static_assert(WCOLS == STRIP_WCOLS && NC == STRIP_NC, "the strip shape of pmk_strip.h");

struct StripTask {
    int32_t region;    // local patch index in the model
    int32_t count;     // valid columns (<= TQ)
    int64_t first;     // first sorted item of the strip
    int32_t group;     // lock-step group (arrival counter index); -1: alone
    int32_t gsize;     // strips in the group
};

// Kq tile of one block row (query is the first kernel argument, mixtureGP.jl:304) into the wave's accumulator, 32 rows
// at a time in a ROLLED loop whose results pass through a lane-private LDS slot: fully unrolled, the 64 evaluations
// of a tile and the accumulator they fill were allocated hundreds of spilled registers (scratch traffic was a quarter
// of this kernel's HBM bytes) and 3 k instructions of code per block row.  Adds the tile's share of the mean.
template <int D, int FAM>
__device__ __forceinline__ void eval_tile(WaveTile<4, 1> &acc, const real *pt, real2_t *mine, real *pk, const pmk_kernel_desc &th,
                                          int row0, int n, int lane)
{
    // the lane's two query points and running means live in its LDS park between block rows (see the kernel)
    real q[NC][D], mu[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
#pragma unroll
        for (int d = 0; d < D; ++d) q[c][d] = pk[(c * D + d) * PRED_THREADS];
        mu[c] = pk[(NC * D + c) * PRED_THREADS];
    }
#pragma unroll
    for (int pi = 0; pi < 4; ++pi) {
#pragma clang loop unroll_count(2)
        for (int sl = 0; sl < 8; ++sl) {
            const int r = 32 * pi + 2 * frag_irow(lane >> 4, sl >> 1) + (sl & 1);     // row within the block row
            real xr[D];
#pragma unroll
            for (int d = 0; d < D; ++d) xr[d] = pt[d * TILE + r];
            const real cw = pt[D * TILE + r];
            // padding rows carry coordinates of 1e300 (pack_soa): a compactly supported profile is
            // exactly 0 there, so the Spline34 instantiation needs no bounds test
            const bool inside = (FAM == PMK_SPLINE34) || row0 + r < n;
            real2_t kv;
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                kv[c] = inside ? kern_eval<D, FAM, real>(th, q[c], xr) : (real)0;
                mu[c] += kv[c] * cw;
            }
            mine[sl * 64] = kv;
        }
#pragma unroll
        for (int sl = 0; sl < 8; ++sl) {
            const real2_t kv = mine[sl * 64];
#pragma unroll
            for (int c = 0; c < NC; ++c) acc.f[2 * pi + (sl & 1)][c][sl >> 1] = kv[c];
        }
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) pk[(NC * D + c) * PRED_THREADS] = mu[c];
}

// Schedule of a strip.  One barrier per block row.  Everything that is not an MFMA is kept off the critical path:
//  * the block row's training points are staged into a three-deep LDS ring two block rows ahead;
//  * the TRSM operands are prefetched from the factor into registers (tri_solve_global);
//  * of the two waves that share a SIMD the older one (waves 0..3) gets most of the matrix pipe and finishes its
//    block row ~100 us before the younger one (waves 4..7).  The older wave evaluates its NEXT kernel tile in that
//    idle time, before the barrier; the younger wave evaluates its tile after the barrier, while the older wave --
//    which has the pipe anyway -- is already in its GEMM.  Both evaluations run in the shadow of the other wave's MFMAs;
//  * the lock-step rendezvous with the other strips of the region is split-phase: thread 0 (wave 0, an early
//    finisher) arrives for the next block row and spins, bounded, before the barrier.
// PP = true (pmk_query_items_fitted): theta of the task's region comes from the model's device array, loaded once per
// task; the region is uniform over the workgroup, so the descriptor stays in scalar registers.  Nothing else differs.
template <int D, int FAM, bool PP = false>
__global__ __launch_bounds__(PRED_THREADS, 2) void predict_strip_kernel(const PatchDesc *__restrict__ descs,
                                                               const real *__restrict__ x, const real *__restrict__ A,
                                                               const real *__restrict__ inv, const real *__restrict__ cvec,
                                                               const StripTask *__restrict__ tasks, int ntasks,
                                                               const int32_t *__restrict__ sorted_item,
                                                               const int32_t *__restrict__ item_query,
                                                               const double *__restrict__ xq, real *__restrict__ strips,
                                                               int64_t strip_stride, typename HyperArgs<PP>::th_t th_arg,
                                                               uint32_t *__restrict__ sync_cnt, int round_base, double min_v,
                                                               double *__restrict__ u_out, double *__restrict__ v_out,
                                                               unsigned long long *__restrict__ clk,
                                                               const double *__restrict__ qdiag)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // shader-clock probe: cycles and 10 ns ticks of the lifetime of workgroups 0..7, one per XCD (pmk_ctx_shader_clock)
    unsigned long long c0 = 0, r0 = 0;
    if (clk && blockIdx.x < 8 && threadIdx.x == 0) { c0 = __builtin_amdgcn_s_memtime(); r0 = __builtin_amdgcn_s_memrealtime(); }
    real *V = strips + (int64_t)blockIdx.x * strip_stride + WCOLS * wave;   // this wave's columns, ld = TQ
    constexpr int PTS = (MAX_D + 1) * TILE;
    // training points (SoA) and weights of consecutive block rows: a ring of three with one barrier per block row
    constexpr int RING = 3;
    __shared__ real pts[RING * PTS];
    __shared__ real priv[PRED_WAVES * 8 * 64 * NC];   // lane-private staging of the kernel evaluations (8 slots a lane)
    real2_t *mine = reinterpret_cast<real2_t *>(priv) + (wave * 8) * 64 + lane;
    // Per-thread values that are only needed between the MFMA phases (the two query points, the running means and
    // squared norms) are PARKED in LDS: around its GEMM the kernel has no register to spare (128 accumulator + 80 ring
    // registers of 256), and what the compiler spills instead goes to scratch memory, in the middle of the hot loops.
    __shared__ real park[(NC * MAX_D + 2 * NC) * PRED_THREADS];
    real *pk = park + threadIdx.x;      // slot k of this thread: pk[k * PRED_THREADS]

    // XCD-aware task order: the workgroups of one XCD take consecutive tasks (= strips of the same
    // region, which stream the same factor L) so that L is fetched into one L2 once per region
    const int nround = (ntasks + (int)gridDim.x - 1) / (int)gridDim.x;
    bool round_sync = true;       // thread 0 only: dropped for good after one missed round barrier
    for (int round = 0; round < nround; ++round) {
        const int base = round * (int)gridDim.x;
        const int nin = min((int)gridDim.x, ntasks - base);          // tasks of this round
        if ((int)blockIdx.x >= nin) break;
        if (round > 0 && threadIdx.x == 0) {
            // round barrier of this XCD's workgroups (speed only, bounded): the strips of a round start together, so
            // that the per-block-row rendezvous below only has to absorb small drifts.  Only the workgroups that have a task
            // in this round arrive (the last round is usually partial: the others have left the loop above).
            uint32_t *cnt = sync_cnt + round_base + 8 * (round - 1) + (blockIdx.x & 7);
            const uint32_t want = ((uint32_t)nin + 7u - (blockIdx.x & 7)) >> 3;   // participants with this id mod 8
            __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (round_sync) {
                const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
                bool ok;
                while (!(ok = __hip_atomic_load(cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= want) &&
                       __builtin_amdgcn_s_memrealtime() - t0 < (uint64_t)ROUND_TICKS)
                    __builtin_amdgcn_s_sleep(32);
                round_sync = ok;
            }
        }
        const int task = base + xcd_remap(blockIdx.x, nin);
        const StripTask tk = tasks[task];
        const bool active = WCOLS * wave < tk.count;     // wave-uniform
        const PatchDesc pd = descs[tk.region];
        pmk_kernel_desc th;
        if constexpr (PP) th = th_arg[tk.region];
        else th = th_arg;
        const real *S = A + pd.aoff;
        const real *xs = x + pd.xoff;
        const real *cr = cvec + pd.yoff;
        const int64_t ld = pd.ld;

        // lock-step rendezvous of the strips that share this factor on this XCD (speed only: a bounded spin on an
        // arrival counter, no data is handed over): thread 0 arrives for block row `row` and waits for the others
        auto rendezvous = [&](int row) {
            uint32_t *cnt = sync_cnt + tk.group;
            const uint32_t want = (uint32_t)tk.gsize * (uint32_t)(row + 1);
            __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
            while (__hip_atomic_load(cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < want &&
                   __builtin_amdgcn_s_memrealtime() - t0 < (uint64_t)SYNC_TICKS)
                __builtin_amdgcn_s_sleep(8);
#ifdef PMK_TRACE
            const unsigned long long w = __builtin_amdgcn_s_memrealtime() - t0;
            atomicAdd(&g_sync_stats[0], 1ull);
            if (w >= (unsigned long long)SYNC_TICKS) atomicAdd(&g_sync_stats[1], 1ull);
            atomicAdd(&g_sync_stats[2], w);
            atomicMax(&g_sync_stats[3], w);
#endif
        };
        // the training points and weights of block row `br`, the same for every lane of the workgroup, by 128 threads
        auto stage_points = [&](int br, int t) {
            real *dst = pts + (br % RING) * PTS;
            const int row = br * TILE + t;
#pragma unroll
            for (int d = 0; d < D; ++d) dst[d * TILE + t] = xs[(int64_t)d * ld + row];
            dst[D * TILE + t] = cr[row];
        };

        // the lane's query columns: 2 (lane & 15) + c of the wave's WCOLS (padding columns repeat a valid item)
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const int col = WCOLS * wave + 2 * (lane & 15) + c;
            const int64_t p = tk.first + (col < tk.count ? col : 0);
            const int64_t qi = item_query[sorted_item[p]];
#pragma unroll
            for (int d = 0; d < D; ++d) pk[(c * D + d) * PRED_THREADS] = (real)xq[qi * D + d];
            pk[(NC * D + c) * PRED_THREADS] = (real)0;            // mean
            pk[(NC * D + NC + c) * PRED_THREADS] = (real)0;       // |V|^2
        }
        // rows of the last block row that are not identity padding, in 32-row pairs (n = 2000: 3 of 4)
        const int last_pairs = (pd.n - (pd.nt - 1) * TILE + 31) >> 5;

        __syncthreads();                              // every wave is done with the previous task's points
        if (threadIdx.x < 2 * TILE && (int)(threadIdx.x >> 7) < pd.nt) stage_points(threadIdx.x >> 7, threadIdx.x & (TILE - 1));
        if (threadIdx.x == 0 && tk.group >= 0) rendezvous(0);
        WaveTile<4, 1> acc;
        bool have = false;                            // acc already holds this block row's kernel tile
        for (int i = 0; i < pd.nt; ++i) {
            __syncthreads();                          // block row i - 1 is complete in every wave; points of row i, i + 1 visible
            PMK_PSTAMP(0);
            if (threadIdx.x < TILE && i + 2 < pd.nt) stage_points(i + 2, threadIdx.x);
            if (active) {
                if (!have) eval_tile<D, FAM>(acc, pts + (i % RING) * PTS, mine, pk, th, i * TILE, pd.n, lane);
                PMK_PSTAMP(2);
#ifdef PMK_TRACE
                if (round == PMK_TRACE_ROUND && i == PMK_TRACE_ROW && lane == 0 && blockIdx.x < 64)
                    g_row_stamp[(blockIdx.x * 8 + (threadIdx.x >> 6)) * 8 + 1] = __builtin_amdgcn_s_memtime();
#endif
                // ---- acc -= L[i, 0:i] V_0:i  (the strip holds -V), then acc <- -V_i = -L[ii]^-1 acc (block substitution;
                //      the strip wants -V anyway).  Padding rows of the last block row are zero and stay zero: skip them.
                const real *Li = S + (int64_t)i * TILE;
                const real *Lii = Li + (int64_t)i * TILE * ld;
                const real *ninv_i = inv + pd.ioff + (int64_t)i * 4096;
                if (i + 1 == pd.nt && last_pairs == 3) strip_block_row<3>(acc, Li, ld, V, i, Lii, ninv_i, lane, PMK_TRACED);
                else if (i + 1 == pd.nt && last_pairs == 2) strip_block_row<2>(acc, Li, ld, V, i, Lii, ninv_i, lane, PMK_TRACED);
                else if (i + 1 == pd.nt && last_pairs == 1) strip_block_row<1>(acc, Li, ld, V, i, Lii, ninv_i, lane, PMK_TRACED);
                else strip_block_row<4>(acc, Li, ld, V, i, Lii, ninv_i, lane, PMK_TRACED);
                PMK_PSTAMP(4);
                {
                    real vs[NC];
#pragma unroll
                    for (int c = 0; c < NC; ++c) vs[c] = pk[(NC * D + NC + c) * PRED_THREADS];
#pragma unroll
                    for (int fi = 0; fi < 8; ++fi)
#pragma unroll
                        for (int qq = 0; qq < 4; ++qq)
#pragma unroll
                            for (int c = 0; c < NC; ++c) vs[c] += acc.f[fi][c][qq] * acc.f[fi][c][qq];
#pragma unroll
                    for (int c = 0; c < NC; ++c) pk[(NC * D + NC + c) * PRED_THREADS] = vs[c];
                }
                have = false;
                if (i + 1 < pd.nt) {
                    int srow = tile_i(0, lane, 0);
                    asm volatile("" : "+v"(srow));
#pragma unroll
                    for (int fi = 0; fi < 8; ++fi)
#pragma unroll
                        for (int qq = 0; qq < 4; ++qq) {
                            const int row = i * TILE + srow + (tile_i(fi, 0, qq) - tile_i(0, 0, 0));
                            real2_t o;
                            o[0] = acc.f[fi][0][qq];
                            o[1] = acc.f[fi][1][qq];
                            __builtin_nontemporal_store(o, reinterpret_cast<real2_t *>(V + (int64_t)row * TQ + 2 * (lane & 15)));
                        }
                    PMK_PSTAMP(5);
                    if (wave < PRED_WAVES / 2) {      // the older wave of its SIMD: next tile now, in its idle time
                        eval_tile<D, FAM>(acc, pts + ((i + 1) % RING) * PTS, mine, pk, th, (i + 1) * TILE, pd.n, lane);
                        have = true;
                    }
                }
                PMK_PSTAMP(6);
            }
            if (threadIdx.x == 0 && tk.group >= 0 && i + 1 < pd.nt) rendezvous(i + 1);
        }
        // ---- reduce over the four lane groups that share a column, then write (u, v)
#pragma unroll
        for (int c = 0; c < NC && active; ++c) {
            real a = pk[(NC * D + c) * PRED_THREADS], b = pk[(NC * D + NC + c) * PRED_THREADS];
            a += __shfl_xor(a, 16); b += __shfl_xor(b, 16);
            a += __shfl_xor(a, 32); b += __shfl_xor(b, 32);
            const int col = WCOLS * wave + 2 * (lane & 15) + c;
            if ((lane >> 4) == 0 && col < tk.count) {
                real qe[D];
#pragma unroll
                for (int d = 0; d < D; ++d) qe[d] = pk[(c * D + d) * PRED_THREADS];
                const real kself = kern_eval<D, FAM, real>(th, qe, qe);
                double var = (double)kself - (double)b;               // mixtureGP.jl:312
                // the kernel's own diagonal term at the query point (pmk_query_set_diag: DPP kernels, kernel.jl:74, 108)
                if (qdiag) var = ((double)kself + qdiag[item_query[sorted_item[tk.first + col]]]) - (double)b;
                var = var < min_v ? min_v : var;                     // clamp(..., min_v, Inf)
                u_out[tk.first + col] = (double)a;
                v_out[tk.first + col] = var;
            }
        }
        // the next task reuses the strip: order its first stores after this task's last loads
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    }
    if (clk && blockIdx.x < 8 && threadIdx.x == 0) {
        clk[130 * blockIdx.x + 128] = __builtin_amdgcn_s_memtime() - c0;
        clk[130 * blockIdx.x + 129] = __builtin_amdgcn_s_memrealtime() - r0;
    }
}

// The strip kernel is the longest compile of the library, so its instantiations are split over two translation units
// that build side by side: this file emits launch_strips<false> (one theta by value), and pmk_predict_patches.hip, which
// includes this file with PMK_PREDICT_PATCHES_TU defined, emits launch_strips<true> (theta from the model's device
// array) and nothing else.  launch_items below picks between the two.
template <bool PP>
int launch_strips(pmk_query *q, const pmk_kernel_desc *th, hipStream_t s)
{
    pmk_model *m = q->m;
    const int64_t stride = (int64_t)m->max_nt * TILE * TQ;
    const StripTask *d_tasks = reinterpret_cast<const StripTask *>(q->d_tasks);
    return dispatch_dim_family(m->D, hyper_spline34(m, th), [&](auto dd, auto fam) {
        hipLaunchKernelGGL((predict_strip_kernel<dd(), fam(), PP>), dim3((unsigned)q->strip_grid), dim3(PRED_THREADS), 0, s,
                           m->d_desc, (real *)m->d_x, (real *)m->d_a, (real *)m->d_inv, (real *)m->d_c, d_tasks,
                           (int)q->ntasks, q->d_sorted_item, q->d_item_query, q->d_xq, (real *)m->d_strip, stride,
                           hyper_th<PP>(m, th), q->d_sync, (int)q->round_base, q->min_v, q->d_u, q->d_v, m->ctx->d_clk,
                           q->d_qdiag);
        return 0;
    });
}
#ifdef PMK_PREDICT_PATCHES_TU
template int launch_strips<true>(pmk_query *, const pmk_kernel_desc *, hipStream_t);
#else
template int launch_strips<false>(pmk_query *, const pmk_kernel_desc *, hipStream_t);
extern template int launch_strips<true>(pmk_query *, const pmk_kernel_desc *, hipStream_t);
#endif

#ifndef PMK_PREDICT_PATCHES_TU
#if defined(PMK_TRACE) && !defined(PMK_REAL_F32)
extern "C" int pmk_trace_sync_stats(unsigned long long *out, int reset)
{
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_sync_stats), sizeof(unsigned long long) * 4) != hipSuccess) return -1;
    if (reset == 2) return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_row_stamp), sizeof(unsigned long long) * 512 * 40) == hipSuccess ? 0 : -1;
    if (reset) {
        const unsigned long long z[4] = {0, 0, 0, 0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_sync_stats), z, sizeof(z)) != hipSuccess) return -1;
    }
    return 0;
}
#endif

// the XCD that xcd_remap() gives logical position p of a round of nin workgroups
static int xcd_of_position(int p, int nin)
{
    const int q = nin >> 3, r = nin & 7;
    const int big = r * (q + 1);
    return p < big ? p / (q + 1) : r + (q ? (p - big) / q : 0);
}

// strip tasks for the regions this model owns (host side, after the plan's region offsets are known)
int build_strip_tasks(pmk_query *q, hipStream_t s)
{
    pmk_model *m = q->m;
    std::vector<StripTask> tasks;
    for (int64_t r = 0; r < m->P; ++r) {
        const int64_t b = q->roff[m->leaf_base + r], e = q->roff[m->leaf_base + r + 1];
        if (e <= b) continue;
        // the region's items are dealt evenly over its strips (not TQ, TQ, ..., remainder): strips of one region then
        // take the same time, which is what keeps them in lock-step
        const int64_t nstrips = (e - b + TQ - 1) / TQ, w = (e - b + nstrips - 1) / nstrips;
        for (int64_t f = b; f < e; f += w) {
            StripTask t;
            t.region = (int32_t)r;
            t.count = (int32_t)((e - f) < w ? (e - f) : w);
            t.first = f;
            t.group = -1;
            t.gsize = 1;
            tasks.push_back(t);
        }
    }
    q->ntasks = (int64_t)tasks.size();
    q->nsync = 0;
    if (tasks.empty()) return 0;
    const int64_t slots = std::min<int64_t>(q->ntasks, (int64_t)m->ctx->num_cu);     // one 8-wave workgroup per CU
    // lock-step groups: consecutive tasks of one round that land on one XCD and stream the same factor
    {
        int64_t g0 = 0;
        auto key = [&](int64_t t) {
            const int64_t round = t / slots, p = t - round * slots;
            const int nin = (int)std::min<int64_t>(slots, q->ntasks - round * slots);
            return std::make_tuple(round, (int64_t)xcd_of_position((int)p, nin), (int64_t)tasks[(size_t)t].region);
        };
        for (int64_t t = 1; t <= q->ntasks; ++t) {
            if (t == q->ntasks || key(t) != key(g0)) {
                if (t - g0 > 1) {
                    for (int64_t u = g0; u < t; ++u) {
                        tasks[(size_t)u].group = (int32_t)q->nsync;
                        tasks[(size_t)u].gsize = (int32_t)(t - g0);
                    }
                    ++q->nsync;
                }
                g0 = t;
            }
        }
    }
    if (q->tasks_cap < q->ntasks) {          // grow only: repeated plans of one query batch reuse the buffer
        if (q->d_tasks) { PMK_HIP(hipFree(q->d_tasks)); q->d_tasks = nullptr; }
        q->tasks_cap = 0;
        const int64_t cap = q->ntasks + q->ntasks / 8 + 64;
        PMK_HIP(hipMalloc(&q->d_tasks, sizeof(StripTask) * (size_t)cap));
        q->tasks_cap = cap;
    }
    // arrival counters: one per lock-step group, then one per (round, XCD) for the round barrier
    q->round_base = q->nsync;
    q->nsync += 8 * ((q->ntasks + slots - 1) / slots);
    if (q->sync_cap < q->nsync) {
        if (q->d_sync) { PMK_HIP(hipFree(q->d_sync)); q->d_sync = nullptr; }
        q->sync_cap = 0;
        const int64_t cap = q->nsync + q->nsync / 8 + 64;
        PMK_HIP(hipMalloc((void **)&q->d_sync, sizeof(uint32_t) * (size_t)cap));
        q->sync_cap = cap;
    }
    PMK_HIP(hipMemcpyAsync(q->d_tasks, tasks.data(), sizeof(StripTask) * tasks.size(), hipMemcpyHostToDevice, s));
    PMK_HIP(hipStreamSynchronize(s));        // `tasks` is a local
    if (int rc = reserve_strips(m, slots)) return rc;
    q->strip_grid = slots;
    return 0;
}

// th null: the model's per-patch kernels (the convention of pmk_dispatch.h)
int launch_items(pmk_query *q, const pmk_kernel_desc *th, hipStream_t s)
{
    if (q->ntasks == 0) return 0;
    if (q->nsync > 0) PMK_HIP(hipMemsetAsync(q->d_sync, 0, sizeof(uint32_t) * (size_t)q->nsync, s));
    if (int rc = th ? launch_strips<false>(q, th, s) : launch_strips<true>(q, nullptr, s)) return rc;
    PMK_HIP(hipGetLastError());
    return 0;
}

#endif  // PMK_PREDICT_PATCHES_TU

}  // namespace PMK_NS
}  // namespace pmk
