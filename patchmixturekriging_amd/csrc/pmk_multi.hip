// Multi-output targets: R right-hand sides per patch that share one resident factor.
//
//   multi_solve_kernel   C = (L L^T)^-1 Y for all R columns of every patch from the resident L and the negated inverted
//                        32 x 32 diagonal blocks (the operands of chol_backsolve_kernel): forward, then backward block
//                        substitution, one workgroup (16 waves) per patch, every off-diagonal tile product on MFMA
//   item_means_kernel    U[item][j] = kq . C_r[:, j] for every (query, region) item: the cross-kernel tile is evaluated in
//                        registers and multiplied by C_r on MFMA; no TRSM, no strips (the mean needs only kq . c)
//   mix_multi_kernel     the mixture of mix_kernel with R means per query (same weights, same order per column)
//
// Layout of the R-column blocks (targets Y and weights C): patch r owns rows [yoff, yoff + ld) of a row-major
// (tot_y x PMK_MAX_OUTPUTS) array, element (i, j) at (yoff + i) * 16 + j.  Columns j >= R and rows i >= n are zero, so
// the MFMA's 16 columns need no masking and the identity padding of the slab keeps the padding rows of C at zero.
// A row of 16 is one contiguous 128-byte (fp64) line: exactly the B operand of one k-step of a 16 x 16 x 4 MFMA.
//
// HBM traffic of the solve: the lower triangle of L twice (forward row-wise, backward column-wise) for all R columns at
// once, plus 2 x ld x 16 elements of Y / C per patch.  The items kernel reads only the points and C_r (L2-resident per
// region); it is VALU bound on the kernel evaluations.
#include "pmk_dispatch.h"
#include "pmk_items.h"
#include "pmk_mfma.h"

namespace pmk {
namespace PMK_NS {

constexpr int RP = PMK_MAX_OUTPUTS;         // columns of a block (R padded)
constexpr int MS_THREADS = 1024;            // 16 waves: 8 row (column) fragments x 2 halves of the reduction range

__device__ __forceinline__ real4_t zero4()
{
    real4_t z;
    z[0] = z[1] = z[2] = z[3] = (real)0;
    return z;
}

__global__ __launch_bounds__(MS_THREADS) void multi_solve_kernel(const PatchDesc *__restrict__ descs, const real *__restrict__ A,
                                                                 const real *__restrict__ ninv, const real *__restrict__ Y,
                                                                 real *Cm)
{
    const PatchDesc pd = descs[blockIdx.x];
    __shared__ real red[TILE * RP], v[TILE * RP], w[TILE * RP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, lg = lane >> 4;
    const int fr = wave & 7, h = wave >> 3;                  // fragment of 16 rows (columns) of the tile, half of the range
    const int di = tid >> 4, dj = tid & 15;                  // diagonal solves: threads 0..511 own entry (di, dj) of a 32 x 16 block
    const real *S = A + pd.aoff;
    const int64_t ld = pd.ld;
    const real *Yb = Y + pd.yoff * RP;
    real *Cb = Cm + pd.yoff * RP;
    const real *Ni = ninv + pd.ioff;

    // ---- forward: Z_k = L[kk]^-1 (Y_k - sum_{t<k} L[k,t] Z_t), Z written into C's block
    for (int k = 0; k < pd.nt; ++k) {
        const int64_t d0 = (int64_t)k * TILE;
        real4_t acc0 = zero4(), acc1 = zero4();
        // A[i = li][kk = lg] = L[d0 + 16 fr + li, c + lg], B[kk = lg][j = li] = Z[c + lg][li]; half h takes columns
        // [128 t + 64 h, 128 t + 64 h + 64) of every tile t < k: sixteen k-steps, all loads in flight before the MFMAs
        const real *Ap = S + d0 + 16 * fr + li + (int64_t)lg * ld;
        const real *Bp = Cb + lg * RP + li;
        for (int t = 0; t < k; ++t) {
            const int64_t cb = (int64_t)t * TILE + 64 * h;
            real a[16], b[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                a[u] = Ap[(cb + 4 * u) * ld];
                b[u] = Bp[(cb + 4 * u) * RP];
            }
#pragma unroll
            for (int u = 0; u < 16; u += 2) {
                acc0 = mfma_real(a[u], b[u], acc0);
                acc1 = mfma_real(a[u + 1], b[u + 1], acc1);
            }
        }
        const real4_t acc = acc0 + acc1;
        if (h == 1)
#pragma unroll
            for (int q = 0; q < 4; ++q) red[(16 * fr + frag_irow(lg, q)) * RP + li] = acc[q];
        __syncthreads();
        if (h == 0)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int row = 16 * fr + frag_irow(lg, q);
                v[row * RP + li] = Yb[(d0 + row) * RP + li] - (acc[q] + red[row * RP + li]);
            }
        __syncthreads();
        // the 128 x 128 diagonal tile: v_s -= sum_{jb<s} L[s][jb] w_jb ; w_s = -Ninv_s v_s  (Ninv_s = -(L_ss)^-1)
        for (int s = 0; s < 4; ++s) {
            if (di < 32) {
                real t = v[(32 * s + di) * RP + dj];
                const real *Lr = S + d0 + 32 * s + di + d0 * ld;
                for (int jb = 0; jb < s; ++jb)
                    for (int c = 0; c < 32; ++c) t -= Lr[(int64_t)(32 * jb + c) * ld] * w[(32 * jb + c) * RP + dj];
                v[(32 * s + di) * RP + dj] = t;
            }
            __syncthreads();
            if (di < 32) {
                const real *nb = Ni + (int64_t)k * 4096 + 1024 * s;
                real t = 0;
                for (int c = 0; c <= di; ++c) t -= nb[di + 32 * c] * v[(32 * s + c) * RP + dj];
                w[(32 * s + di) * RP + dj] = t;
            }
            __syncthreads();
        }
        for (int e = tid; e < TILE * RP; e += MS_THREADS) Cb[d0 * RP + e] = w[e];
        __syncthreads();
    }

    // ---- backward: C_k = L[kk]^-T (Z_k - sum_{t>k} L[t,k]^T C_t), in place over Z
    for (int k = pd.nt - 1; k >= 0; --k) {
        const int64_t d0 = (int64_t)k * TILE;
        real4_t acc0 = zero4(), acc1 = zero4();
        // A[i = li][kk] = L[row, d0 + 16 fr + li], B[kk][j = li] = C[row][li]: a lane loads four consecutive rows of its
        // column (one 32-byte piece; the four lane groups cover 16 rows) and k-step (g, q) takes row 16 g + 4 lg + q
        const real *Lc = S + (d0 + 16 * fr + li) * ld + 4 * lg;
        const real *Bq = Cb + 4 * lg * RP + li;
        for (int t = k + 1; t < pd.nt; ++t) {
            const int64_t rb = (int64_t)t * TILE + 64 * h;
            real4_t a[4];
            real b[16];
#pragma unroll
            for (int g = 0; g < 4; ++g) a[g] = *reinterpret_cast<const real4_t *>(Lc + rb + 16 * g);
#pragma unroll
            for (int g = 0; g < 4; ++g)
#pragma unroll
                for (int q = 0; q < 4; ++q) b[4 * g + q] = Bq[(rb + 16 * g + q) * RP];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                acc0 = mfma_real(a[g][0], b[4 * g + 0], acc0);
                acc1 = mfma_real(a[g][1], b[4 * g + 1], acc1);
                acc0 = mfma_real(a[g][2], b[4 * g + 2], acc0);
                acc1 = mfma_real(a[g][3], b[4 * g + 3], acc1);
            }
        }
        const real4_t acc = acc0 + acc1;
        if (h == 1)
#pragma unroll
            for (int q = 0; q < 4; ++q) red[(16 * fr + frag_irow(lg, q)) * RP + li] = acc[q];
        __syncthreads();
        if (h == 0)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int col = 16 * fr + frag_irow(lg, q);
                v[col * RP + li] = Cb[(d0 + col) * RP + li] - (acc[q] + red[col * RP + li]);
            }
        __syncthreads();
        // v_s -= sum_{jb>s} L[jb][s]^T w_jb ; w_s = -Ninv_s^T v_s
        for (int s = 3; s >= 0; --s) {
            if (di < 32) {
                real t = v[(32 * s + di) * RP + dj];
                const real *Lcol = S + d0 + (d0 + 32 * s + di) * ld;
                for (int jb = s + 1; jb < 4; ++jb)
                    for (int r = 0; r < 32; ++r) t -= Lcol[32 * jb + r] * w[(32 * jb + r) * RP + dj];
                v[(32 * s + di) * RP + dj] = t;
            }
            __syncthreads();
            if (di < 32) {
                const real *nb = Ni + (int64_t)k * 4096 + 1024 * s + 32 * di;
                real t = 0;
                for (int r = di; r < 32; ++r) t -= nb[r] * v[(32 * s + r) * RP + dj];
                w[(32 * s + di) * RP + dj] = t;
            }
            __syncthreads();
        }
        for (int e = tid; e < TILE * RP; e += MS_THREADS) Cb[d0 * RP + e] = w[e];
        __syncthreads();
    }
}

int launch_solve_multi(pmk_model *m, hipStream_t s)
{
    hipLaunchKernelGGL(multi_solve_kernel, dim3((unsigned)m->P), dim3(MS_THREADS), 0, s, m->d_desc, (const real *)m->d_a,
                       (const real *)m->d_inv, (const real *)m->d_ym, (real *)m->d_cm);
    PMK_HIP(hipGetLastError());
    return 0;
}

// One wave per chunk of (up to) 16 items of one region: lane l evaluates k(xq of item l & 15, x of point k0 + (l >> 4))
// -- the A operand of the MFMA, query first as in queryinner! (mixtureGP.jl:304) -- and the B operand is row k0 + (l >> 4)
// of C_r.  Chunk g of the whole list lies in the region r with cpre[r] <= g < cpre[r + 1] (chunks per region, host
// prefix).  Consecutive chunks share their region's C_r: xcd_remap keeps them on one XCD's L2.  R is the number of
// columns emitted and the row length of U: the target columns, plus the q columns of C_H with a trend (pmk_trend.hip).
// PP = true (pmk_query_items_multi_fitted): theta of the chunk's region from the model's device array; a wave handles one
// region, so the descriptor is wave-uniform.
constexpr int IM_THREADS = 256;

template <int D, int FAM, bool PP = false>
__global__ __launch_bounds__(IM_THREADS) void item_means_kernel(const PatchDesc *__restrict__ descs, const real *__restrict__ x,
                                                                const real *__restrict__ Cm, const int64_t *__restrict__ roff,
                                                                const int64_t *__restrict__ cpre, int P, int64_t nchunks,
                                                                const int32_t *__restrict__ sorted_item,
                                                                const int32_t *__restrict__ item_query,
                                                                const double *__restrict__ xq,
                                                                typename HyperArgs<PP>::th_t th_arg, int R,
                                                                double *__restrict__ U)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t g = (int64_t)xcd_remap((int)blockIdx.x, (int)gridDim.x) * (IM_THREADS / 64) + wave;
    if (g >= nchunks) return;
    const int r = chunk_region(cpre, P, g);
    const int64_t first = roff[r] + (g - cpre[r]) * 16;
    const int count = (int)min((int64_t)16, roff[r + 1] - first);
    const PatchDesc pd = descs[r];
    pmk_kernel_desc th;
    if constexpr (PP) th = th_arg[__builtin_amdgcn_readfirstlane(r)];
    else th = th_arg;
    const int li = lane & 15, lg = lane >> 4;
    real q[D];
    chunk_query_point(first, count, li, sorted_item, item_query, xq, q);
    const real *xs = x + pd.xoff;
    const real *Cb = Cm + pd.yoff * RP + li;
    const int ld = pd.ld, n = pd.n;
    real4_t acc0 = zero4(), acc1 = zero4();
    // k0 < n <= ld and ld is a multiple of 128: k0 + 7 < ld, every load stays inside the patch's padded rows
    for (int k0 = 0; k0 < n; k0 += 8) {
        const int ka = k0 + lg, kb = k0 + 4 + lg;
        real xa[D], xb[D];
#pragma unroll
        for (int d = 0; d < D; ++d) {
            xa[d] = xs[d * ld + ka];
            xb[d] = xs[d * ld + kb];
        }
        const real ba = Cb[(int64_t)ka * RP], bb = Cb[(int64_t)kb * RP];
        const real kva = kern_eval<D, FAM, real>(th, q, xa), kvb = kern_eval<D, FAM, real>(th, q, xb);
        acc0 = mfma_real(ka < n ? kva : (real)0, ba, acc0);
        acc1 = mfma_real(kb < n ? kvb : (real)0, bb, acc1);
    }
    const real4_t acc = acc0 + acc1;
    if (li < R)
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) {
            const int i = frag_irow(lg, qq);
            if (i < count) U[(first + i) * R + li] = (double)acc[qq];
        }
}

// th null: the model's per-patch kernels (the convention of pmk_dispatch.h)
int launch_items_multi(pmk_query *q, const pmk_kernel_desc *th, hipStream_t s)
{
    pmk_model *m = q->m;
    if (q->mchunks == 0) return 0;
    const unsigned grid = (unsigned)((q->mchunks + IM_THREADS / 64 - 1) / (IM_THREADS / 64));
    const int rc = dispatch_hyper(m, th, [&](auto dd, auto fam, auto pp) {
        hipLaunchKernelGGL((item_means_kernel<dd(), fam(), pp()>), dim3(grid), dim3(IM_THREADS), 0, s, m->d_desc,
                           (const real *)m->d_x, (const real *)m->d_cm, q->d_roff, q->d_mcpre, (int)m->P, q->mchunks,
                           q->d_sorted_item, q->d_item_query, q->d_xq, hyper_th<pp()>(m, th), q->um_ld, q->d_um);
        return 0;
    });
    if (rc) return rc;
    PMK_HIP(hipGetLastError());
    return 0;
}

}  // namespace PMK_NS

#ifndef PMK_REAL_F32
// mix_kernel (pmk_kernels.hip) with R means: the same weights (blend_weight and blend_weight_sum of pmk_items.h:
// neighbours phi_w(|t|) in hyperplane order, home 1 last, normalised) and, per column, the same order of operations as its Yq.  Yq is Nq x R column-major (ld Nq).  A row of U
// has ldu >= R columns (ldu > R with a trend, pmk_trend.hip: the extra columns are not mixed).
__global__ __launch_bounds__(256) void mix_multi_kernel(int64_t q0, int64_t q1, int64_t Nq, const int64_t *__restrict__ qoff,
                                                        const double *__restrict__ item_t, const int32_t *__restrict__ item_pos,
                                                        const double *__restrict__ U, int ldu, int R, pmk_kernel_desc wth,
                                                        double *__restrict__ yq)
{
    const int64_t j = q0 + (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= q1) return;
    const int64_t b = qoff[j], e = qoff[j + 1];
    const double sw = blend_weight_sum(wth, item_t, b, e);
    for (int col = 0; col < R; ++col) {
        double y = 0.0;
        for (int64_t it = b; it < e; ++it) {
            const double w = blend_weight(wth, item_t, it, e) / sw;
            const double ui = U[(int64_t)item_pos[it] * ldu + col];
            y = (it == b) ? w * ui : y + w * ui;
        }
        yq[col * Nq + j] = y;
    }
}

int launch_mix_multi(pmk_query *q, const pmk_kernel_desc &wth, int64_t q0, int64_t q1, hipStream_t s)
{
    if (q1 <= q0) return 0;
    hipLaunchKernelGGL(mix_multi_kernel, grid256(q1 - q0), dim3(256), 0, s, q0, q1, q->Nq, q->d_qoff,
                       q->d_item_t, q->d_item_pos, q->d_um, q->um_ld, q->R_items, wth, q->d_yqm);
    PMK_HIP(hipGetLastError());
    return 0;
}
#endif

}  // namespace pmk
