// Posterior draws of the blended field from the region blocks, without the Nq x Nq covariance.
//
// The patches are independent GPs, so with S_r = L_r L_r^T the blocks of pmk_query_items_cov(_multi)
//
//   E_s(x_j) = sum over the items i of j:  wn_i (L_{r(i)} zeta_{r(i), s})[a(i)]
//
// is a zero-mean draw whose covariance is the entry mix_cov_kernel (pmk_cov.hip) computes: sum_r wn wn' S_r[a, a'].
//
//   cov_potrf_prep_kernel    per region: which regions this call factors, the status word, the trace (one fixed order)
//                            and the jitter rel (trace / m)
//   cov_potrf_diag_kernel    block step k, one workgroup per region with more than k tiles: the diagonal tile
//                            S[k,k] + jitter - sum_{j<k} L[k,j] L[k,j]^T as one MFMA chain in ascending j, factored in LDS
//   cov_potrf_panel_kernel   block step k, one workgroup per (region, tile row i > k): S[i,k] - sum_{j<k} L[i,j] L[k,j]^T
//                            by the same chain, then the triangular solve against L[k,k] by substitution
//   draw_trmm_kernel         T_r = L_r Z_r for a chunk of draws on the MFMA, rows in sorted-item order
//   draw_mix_kernel          the blend in gather form: one thread per (query, draw), one fma chain in the item order of
//                            pmk_query_mix, no atomics
//
// The factorisation is left-looking over block columns of DRAW_TILE = 32: two launches per step, each batched over every
// region that still has tiles (the regions are ordered by descending tile count, so step k takes the first
// fstep_regions[k] of them).  A tile is read from S, updated in registers, solved and written once.  The factor buffer is
// padded per region to a multiple of the tile with the identity in the padding: rows and columns past m_r are loaded
// as the identity and factor as such.
//
// Bits.  An entry of a factor is a function of its region's block and jitter alone: the MFMA chain of a tile runs over the
// columns 0 .. 32 k - 1 in steps of four, the LDS factorisation and the substitution are fma chains in ascending column
// index, and a tile belongs to one workgroup.  Nothing is accumulated across workgroups; no atomics.  A pivot that is NaN
// or <= 0 to rounding (not above 2^-50 of its diagonal entry S_kk + jitter: the difference of two equal numbers of that
// size, as the second copy of a duplicated item leaves it) stores its index (from 1) in the region's status word, and the
// later launches skip that region only.  All double: the file is compiled once and serves the models of both element
// types.
#include "pmk_items.h"
#include "pmk_mfma.h"

namespace pmk {

using f64::frag_irow;
using f64::mfma_real;
using f64::real4_t;

constexpr int DT = DRAW_TILE;
constexpr int DLD = DT + 1;                     // leading dimension of a tile in LDS
constexpr int DRAW_THREADS = 64;                // one wave: a 32 x 32 tile is 2 x 2 MFMA fragments
constexpr int DRAW_COPIES = DT * DT / DRAW_THREADS;

// Register q of fragment (ia, ib) of lane (lg, li) holds the entry (16 ia + frag_irow(lg, q), 16 ib + li) of the tile.
__device__ __forceinline__ void tile_to_acc(const double (*t)[DLD], real4_t (&acc)[2][2], int li, int lg)
{
#pragma unroll
    for (int ia = 0; ia < 2; ++ia)
#pragma unroll
        for (int ib = 0; ib < 2; ++ib)
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[ia][ib][q] = t[16 * ia + frag_irow(lg, q)][16 * ib + li];
}
__device__ __forceinline__ void acc_to_tile(double (*t)[DLD], const real4_t (&acc)[2][2], int li, int lg)
{
#pragma unroll
    for (int ia = 0; ia < 2; ++ia)
#pragma unroll
        for (int ib = 0; ib < 2; ++ib)
#pragma unroll
            for (int q = 0; q < 4; ++q) t[16 * ia + frag_irow(lg, q)][16 * ib + li] = acc[ia][ib][q];
}

// acc -= A[0:32, 0:K] B[0:32, 0:K]^T, both column-major with leading dimension ld, K a multiple of 32: entry (a, b) is one
// accumulator register updated by the MFMAs of k0 = 0, 4, ..., K - 4 in that order
__device__ __forceinline__ void chain_nt(real4_t (&acc)[2][2], const double *A, const double *B, int64_t ld, int K, int li, int lg)
{
    const double *pa = A + li + ld * lg, *pb = B + li + ld * lg;
    for (int k0 = 0; k0 < K; k0 += 8) {
        double va[2][2], vb[2][2];
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int f = 0; f < 2; ++f) {
                va[u][f] = -pa[ld * (k0 + 4 * u) + 16 * f];
                vb[u][f] = pb[ld * (k0 + 4 * u) + 16 * f];
            }
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int ia = 0; ia < 2; ++ia)
#pragma unroll
                for (int ib = 0; ib < 2; ++ib) acc[ia][ib] = mfma_real(va[u][ia], vb[u][ib], acc[ia][ib]);
    }
}

// the tile (ti, tj) of S_r padded with the identity, into LDS; jt joins the diagonal entries of the block itself
__device__ __forceinline__ void stage_block_tile(double (*t)[DLD], const double *S, const DrawRegion &d, int ti, int tj, double jt,
                                                 int tid)
{
#pragma unroll 4
    for (int e = 0; e < DRAW_COPIES; ++e) {
        const int idx = tid + DRAW_THREADS * e, row = idx & (DT - 1), col = idx / DT;
        const int gr = DT * ti + row, gc = DT * tj + col;
        double v = gr == gc ? 1.0 : 0.0;
        if (gr < d.m && gc < d.m) {
            v = S[d.soff + gr + (int64_t)d.m * gc];
            if (gr == gc) v += jt;
        }
        t[row][col] = v;
    }
}

// One wave per region.  The trace is summed by lane l over the diagonal entries l, l + 64, ... in that order and the 64
// partial sums by a fixed butterfly.  have: the status words and rel of an earlier call on the same blocks are valid; a
// region it factored with the same rel keeps its factor.
__global__ __launch_bounds__(DRAW_THREADS) void cov_potrf_prep_kernel(const DrawRegion *__restrict__ desc, const double *__restrict__ S,
                                                                     const int32_t *__restrict__ info, int have,
                                                                     double *__restrict__ rel_held,
                                                                     const double *__restrict__ rel_new, int32_t *__restrict__ finfo,
                                                                     int32_t *__restrict__ act, double *__restrict__ jit)
{
    const int r = blockIdx.x, lane = threadIdx.x;
    const DrawRegion d = desc[r];
    const double rel = rel_new[r];
    if (have && finfo[r] == 0 && rel_held[r] == rel) {
        if (lane == 0) act[r] = 0;
        return;
    }
    const bool bad = patch_is_bad(info, nullptr, r);
    double tr = 0.0;
    if (!bad)
        for (int a = lane; a < d.m; a += DRAW_THREADS) tr += S[d.soff + (int64_t)a * (d.m + 1)];
#pragma unroll
    for (int o = 1; o < DRAW_THREADS; o <<= 1) tr += __shfl_xor(tr, o, DRAW_THREADS);
    if (lane == 0) {
        rel_held[r] = rel;
        const bool run = d.m > 0 && !bad;
        finfo[r] = d.m > 0 && bad ? -1 : 0;
        act[r] = run ? 1 : 0;
        jit[r] = run ? rel * (tr / (double)d.m) : 0.0;
    }
}

__global__ __launch_bounds__(DRAW_THREADS) void cov_potrf_diag_kernel(const DrawRegion *__restrict__ desc, const int32_t *__restrict__ order,
                                                                     int k, const double *__restrict__ S, double *__restrict__ F,
                                                                     const double *__restrict__ jit, const int32_t *__restrict__ act,
                                                                     int32_t *__restrict__ finfo)
{
    __shared__ double T[DT][DLD];
    __shared__ int fail;
    const int r = order[blockIdx.x];
    if (!act[r] || finfo[r] != 0) return;                       // workgroup-uniform
    const DrawRegion d = desc[r];
    const int tid = threadIdx.x, li = tid & 15, lg = tid >> 4;
    const int64_t ld = (int64_t)DT * d.nt;
    double *Fr = F + d.foff;
    stage_block_tile(T, S, d, k, k, jit[r], tid);
    if (tid == 0) fail = 0;
    __syncthreads();
    real4_t acc[2][2];
    tile_to_acc(T, acc, li, lg);
    chain_nt(acc, Fr + DT * k, Fr + DT * k, ld, DT * k, li, lg);
    __syncthreads();
    acc_to_tile(T, acc, li, lg);
    __syncthreads();
    // left-looking in LDS: lane t owns row t, kept in registers; column j after the columns before it
    const int t = tid & (DT - 1);
    // the diagonal entry the pivot of row t started from: a pivot that is not above 2^-50 of it holds no digit (the second
    // copy of a duplicated item leaves d - fl(d / fl(sqrt d))^2, at most 4 u d of either sign) and counts as <= 0
    const int gt = DT * k + t;
    const double dt = gt < d.m ? S[d.soff + (int64_t)gt * (d.m + 1)] + jit[r] : 1.0;
    double row[DT];
#pragma unroll
    for (int p = 0; p < DT; ++p) row[p] = T[t][p];
#pragma unroll
    for (int j = 0; j < DT; ++j) {
        double s = row[j];
#pragma unroll
        for (int p = 0; p < j; ++p) s = __builtin_fma(-row[p], T[j][p], s);
        if (tid == j) {
            if (!(s > 0.0 && s > 0x1p-50 * dt)) fail = j + 1;   // <= 0 to rounding, or NaN
            else T[j][j] = __builtin_sqrt(s);
        }
        __syncthreads();
        if (fail) break;
        if (tid < DT && tid > j) {
            row[j] = s / T[j][j];
            T[tid][j] = row[j];
        }
        __syncthreads();
    }
    if (fail) {
        if (tid == 0) finfo[r] = DT * k + fail;
        return;
    }
#pragma unroll 4
    for (int e = 0; e < DRAW_COPIES; ++e) {
        const int idx = tid + DRAW_THREADS * e, rw = idx & (DT - 1), cl = idx / DT;
        Fr[DT * k + rw + ld * (DT * k + cl)] = rw >= cl ? T[rw][cl] : 0.0;
    }
}

__global__ __launch_bounds__(DRAW_THREADS) void cov_potrf_panel_kernel(const DrawRegion *__restrict__ desc, const int32_t *__restrict__ order,
                                                                      int k, const double *__restrict__ S, double *__restrict__ F,
                                                                      const int32_t *__restrict__ act, const int32_t *__restrict__ finfo)
{
    __shared__ double X[DT][DLD], Lk[DT][DLD];
    const int r = order[blockIdx.x];
    const DrawRegion d = desc[r];
    const int i = k + 1 + (int)blockIdx.y;
    if (i >= d.nt || !act[r] || finfo[r] != 0) return;          // workgroup-uniform
    const int tid = threadIdx.x, li = tid & 15, lg = tid >> 4;
    const int64_t ld = (int64_t)DT * d.nt;
    double *Fr = F + d.foff;
    stage_block_tile(X, S, d, i, k, 0.0, tid);
#pragma unroll 4
    for (int e = 0; e < DRAW_COPIES; ++e) {
        const int idx = tid + DRAW_THREADS * e, rw = idx & (DT - 1), cl = idx / DT;
        Lk[rw][cl] = Fr[DT * k + rw + ld * (DT * k + cl)];
    }
    __syncthreads();
    real4_t acc[2][2];
    tile_to_acc(X, acc, li, lg);
    chain_nt(acc, Fr + DT * i, Fr + DT * k, ld, DT * k, li, lg);
    __syncthreads();
    acc_to_tile(X, acc, li, lg);
    __syncthreads();
    // x L[k,k]^T = c for row t: x_c = (c_c - sum_{p < c} x_p L[c, p]) / L[c, c], the sum as an fma chain in p order
    if (tid < DT) {
        double x[DT];
#pragma unroll
        for (int c = 0; c < DT; ++c) {
            double s = X[tid][c];
#pragma unroll
            for (int p = 0; p < c; ++p) s = __builtin_fma(-x[p], Lk[c][p], s);
            x[c] = s / Lk[c][c];
        }
#pragma unroll
        for (int c = 0; c < DT; ++c) X[tid][c] = x[c];
    }
    __syncthreads();
#pragma unroll 4
    for (int e = 0; e < DRAW_COPIES; ++e) {
        const int idx = tid + DRAW_THREADS * e, rw = idx & (DT - 1), cl = idx / DT;
        Fr[DT * i + rw + ld * (DT * k + cl)] = X[rw][cl];
    }
}

// blockIdx.x: a tile row (region, i), blockIdx.y: 32 draws of the chunk.  T[p0 + a, s] = sum_{b <= a} L[a, b] z[p0 + b, s] as
// one MFMA chain over b = 0 .. 32 (i + 1) - 1 in steps of four (the factor's diagonal tile holds zeros above the diagonal).
// z rows past m and draws past n are taken as zeros and never stored.
__global__ __launch_bounds__(DRAW_THREADS) void draw_trmm_kernel(const DrawRegion *__restrict__ desc, const DrawTask *__restrict__ tasks,
                                                                const int32_t *__restrict__ finfo, const double *__restrict__ F,
                                                                const double *__restrict__ z, int64_t ldz, int64_t n,
                                                                double *__restrict__ T, int64_t total)
{
    __shared__ double Zt[DT][DLD];                              // [draw][row]
    const DrawTask tk = tasks[blockIdx.x];
    if (finfo[tk.region] != 0) return;                          // its queries are NaN in draw_mix_kernel
    const DrawRegion d = desc[tk.region];
    const int tid = threadIdx.x, li = tid & 15, lg = tid >> 4;
    const int64_t ld = (int64_t)DT * d.nt, s0 = (int64_t)DT * blockIdx.y;
    const double *Fi = F + d.foff + DT * tk.tile;
    real4_t acc[2][2];
#pragma unroll
    for (int ia = 0; ia < 2; ++ia)
#pragma unroll
        for (int ib = 0; ib < 2; ++ib) acc[ia][ib] = real4_t{0, 0, 0, 0};
    for (int j = 0; j <= tk.tile; ++j) {
        __syncthreads();
#pragma unroll 4
        for (int e = 0; e < DRAW_COPIES; ++e) {
            const int idx = tid + DRAW_THREADS * e, rw = idx & (DT - 1), dr = idx / DT;
            const int b = DT * j + rw;
            Zt[dr][rw] = (b < d.m && s0 + dr < n) ? z[d.p0 + b + ldz * (s0 + dr)] : 0.0;
        }
        __syncthreads();
        const double *pa = Fi + li + ld * (DT * j + lg);
#pragma unroll
        for (int kk = 0; kk < DT; kk += 4) {
            double va[2], vb[2];
#pragma unroll
            for (int f = 0; f < 2; ++f) {
                va[f] = pa[ld * kk + 16 * f];
                vb[f] = Zt[16 * f + li][kk + lg];
            }
#pragma unroll
            for (int ia = 0; ia < 2; ++ia)
#pragma unroll
                for (int ib = 0; ib < 2; ++ib) acc[ia][ib] = mfma_real(va[ia], vb[ib], acc[ia][ib]);
        }
    }
    __syncthreads();
#pragma unroll
    for (int ia = 0; ia < 2; ++ia)
#pragma unroll
        for (int ib = 0; ib < 2; ++ib)
#pragma unroll
            for (int q = 0; q < 4; ++q) Zt[16 * ib + li][16 * ia + frag_irow(lg, q)] = acc[ia][ib][q];
    __syncthreads();
#pragma unroll 4
    for (int e = 0; e < DRAW_COPIES; ++e) {
        const int idx = tid + DRAW_THREADS * e, rw = idx & (DT - 1), dr = idx / DT;
        const int a = DT * tk.tile + rw;
        if (a < d.m && s0 + dr < n) T[d.p0 + a + total * (s0 + dr)] = Zt[dr][rw];
    }
}

// One thread per (query j, draw s): E[j, s] = sum over the items of j of wn_i T[item_pos[i], s], one fma chain in item order
// with the weights of mix_cov_kernel.  A query that blends an item of a region whose status word is not 0 is NaN.
__global__ __launch_bounds__(256) void draw_mix_kernel(int64_t Nq, const int64_t *__restrict__ qoff, const double *__restrict__ item_t,
                                                       const int32_t *__restrict__ item_region, const int32_t *__restrict__ item_pos,
                                                       const int32_t *__restrict__ finfo, pmk_kernel_desc wth,
                                                       const double *__restrict__ T, int64_t total, double *__restrict__ E, int64_t lde)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x, s = blockIdx.y;
    if (j >= Nq) return;
    const int64_t b = qoff[j], e = qoff[j + 1];
    const double sw = blend_weight_sum(wth, item_t, b, e);
    double acc = 0.0;
    bool bad = false;
    for (int64_t it = b; it < e; ++it) {
        bad = bad || finfo[item_region[it]] != 0;
        const double wn = blend_weight(wth, item_t, it, e) / sw;
        const double v = T[item_pos[it] + total * s];
        acc = it == b ? wn * v : __builtin_fma(wn, v, acc);
    }
    E[j + lde * s] = bad ? __builtin_nan("") : acc;
}

// the descriptors, the order, the step counts and the buffers are the caller's (pmk_query_factor_cov)
int launch_factor_cov(pmk_query *q, int have_factors, hipStream_t s)
{
    const pmk_model *m = q->m;
    if (m->P == 0) return 0;
    const int32_t *info = q->cov_trend_q > 0 ? q->d_cov_flags : (const int32_t *)m->d_info;
    hipLaunchKernelGGL(cov_potrf_prep_kernel, dim3((unsigned)m->P), dim3(DRAW_THREADS), 0, s, q->d_fdesc, q->d_cov_s, info,
                       have_factors, q->d_frel, q->d_frel + m->P, q->d_finfo, q->d_fact, q->d_fjit);
    PMK_HIP(hipGetLastError());
    const int steps = (int)q->fstep_regions.size();
    for (int k = 0; k < steps; ++k) {
        const unsigned nr = (unsigned)q->fstep_regions[(size_t)k];
        hipLaunchKernelGGL(cov_potrf_diag_kernel, dim3(nr), dim3(DRAW_THREADS), 0, s, q->d_fdesc, q->d_forder, k, q->d_cov_s,
                           q->d_cov_f, q->d_fjit, q->d_fact, q->d_finfo);
        PMK_HIP(hipGetLastError());
        if (k + 1 == steps) break;
        // the regions with a tile row below the diagonal tile, and the most such rows any of them has
        const unsigned nr1 = (unsigned)q->fstep_regions[(size_t)k + 1];
        hipLaunchKernelGGL(cov_potrf_panel_kernel, dim3(nr1, (unsigned)(steps - k - 1)), dim3(DRAW_THREADS), 0, s, q->d_fdesc,
                           q->d_forder, k, q->d_cov_s, q->d_cov_f, q->d_fact, q->d_finfo);
        PMK_HIP(hipGetLastError());
    }
    return 0;
}

// n draws (a chunk: the workspace holds total x n): z[p + ldz s], E[j + lde s], both on the device
int launch_draw(pmk_query *q, const pmk_kernel_desc &wth, const double *d_z, int64_t ldz, int64_t n, double *d_E, int64_t lde,
                hipStream_t s)
{
    if (n == 0 || q->Nq == 0) return 0;
    if (q->nftasks > 0) {
        hipLaunchKernelGGL(draw_trmm_kernel, dim3((unsigned)q->nftasks, (unsigned)((n + DT - 1) / DT)), dim3(DRAW_THREADS), 0, s,
                           q->d_fdesc, q->d_ftasks, q->d_finfo, q->d_cov_f, d_z, ldz, n, q->d_draw_t, q->total);
        PMK_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(draw_mix_kernel, dim3((unsigned)((q->Nq + 255) / 256), (unsigned)n), dim3(256), 0, s, q->Nq, q->d_qoff,
                       q->d_item_t, q->d_item_region, q->d_item_pos, q->d_finfo, wth, q->d_draw_t, q->total, d_E, lde);
    PMK_HIP(hipGetLastError());
    return 0;
}

}  // namespace pmk
