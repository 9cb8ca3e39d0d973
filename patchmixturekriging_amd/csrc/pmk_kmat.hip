// K1: batched kernel-matrix build into the factorisation slabs (compiled for real = double and float).
#include "pmk_dispatch.h"
#include "pmk_real.h"

namespace pmk {
namespace PMK_NS {

// =============================================================================================
// K1: batched kernel-matrix build into the factorisation slabs.
// Replaces the evalkernel real loop of constructkernelmatrix! (src/RKHS/RKHS.jl:21-31) and the
// diagonal "+= sigma2" of fitmixtureGP! (src/RKHS/mixtureGP.jl:102-104).  HBM-write bound:
// 8 * ld^2 / 2 bytes per patch (lower triangle; diagonal 64x64 tiles are written whole and exactly
// symmetric).  One workgroup = one 64 x 64 tile, one thread = 4 contiguous rows x 4 columns, so a
// 16-thread row group stores 512 contiguous bytes per column.  Padding rows/columns (index >= n) are
// written as identity so the padded factorisation stays positive definite.
// =============================================================================================
// diag_only = false: the whole lower triangle of every patch (grid.x = its 64 x 64 tiles).  diag_only = true (fused fit):
// only the diagonal 128 x 128 tiles (grid.x = 3 per diagonal tile of the tallest patch).
// PP = true (pmk_model_fit_patches): theta and sigma2 of the workgroup's patch come from the model's device arrays, which
// the host offsets by p0 like descs, so that all three are indexed by blockIdx.y.  The index is uniform over the
// workgroup: the descriptor is a scalar load.
template <int D, int FAM, bool PP = false>
__global__ __launch_bounds__(256) void kmat_slab_kernel(const PatchDesc *__restrict__ descs, const real *__restrict__ x,
                                                        real *__restrict__ A, typename HyperArgs<PP>::th_t th_arg,
                                                        typename HyperArgs<PP>::s2_t sigma2_arg,
                                                        bool diag_only, const real *__restrict__ dg)
{
    const PatchDesc pd = descs[blockIdx.y];
    pmk_kernel_desc th;
    real sigma2;
    if constexpr (PP) {
        th = th_arg[blockIdx.y];
        sigma2 = (real)sigma2_arg[blockIdx.y];
    } else {
        th = th_arg;
        sigma2 = (real)sigma2_arg;
    }
    int ti, tj;
    if (diag_only) {
        // potrf and look-ahead read the diagonal tiles from the slab; the tiles below are evaluated by the factorisation
        // at their first use.  Three 64 x 64 tiles per diagonal tile.
        const int c = blockIdx.x / 3, r = blockIdx.x - 3 * c;
        if (c >= pd.nt) return;
        ti = 2 * c + (r > 0);
        tj = 2 * c + (r > 1);
    } else {
        const int nt64 = pd.nt * (TILE / 64);     // the active block rows: what lies past them up to ld stays identity
        const int ntiles = nt64 * (nt64 + 1) / 2;
        const int t = blockIdx.x;
        if (t >= ntiles) return;
        ti = (int)((sqrt(8.0 * t + 1.0) - 1.0) * 0.5);
        while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
        while (ti * (ti + 1) / 2 > t) --ti;
        tj = t - ti * (ti + 1) / 2;
    }
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int i0 = ti * 64 + 4 * tx, j0 = tj * 64 + 4 * ty;
    const real *xs = x + pd.xoff;
    real xi[4][D], xj[4][D];
#pragma unroll
    for (int d = 0; d < D; ++d) {
        const real4_t vi = *reinterpret_cast<const real4_t *>(xs + (int64_t)d * pd.ld + i0);
        const real4_t vj = *reinterpret_cast<const real4_t *>(xs + (int64_t)d * pd.ld + j0);
#pragma unroll
        for (int a = 0; a < 4; ++a) { xi[a][d] = vi[a]; xj[a][d] = vj[a]; }
    }
    real *S = A + pd.aoff;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const int j = j0 + b;
        real4_t o;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const int i = i0 + a;
            real v;
            if (i < pd.n && j < pd.n) {
                v = (i >= j) ? kern_eval<D, FAM, real>(th, xi[a], xj[b]) : kern_eval<D, FAM, real>(th, xj[b], xi[a]);
                if (i == j) {
                    if (dg) v = v + dg[pd.yoff + i];      // the kernel's own point-dependent diagonal term (pmk_model_set_diag)
                    v = v + sigma2;
                }
            } else {
                v = (i == j) ? (real)1 : (real)0;
            }
            o[a] = v;
        }
        *reinterpret_cast<real4_t *>(S + i0 + (int64_t)j * pd.ld) = o;
    }
}

// th non-null: this theta and sigma2 for every patch.  th null (per-patch hyperparameters): the model's device arrays from
// patch p0 on, and always the whole lower triangle -- the fused build evaluates tiles inside the factorisation's step
// launches, which know one theta.
int launch_kernel_matrix_slabs(const pmk_model *m, const pmk_kernel_desc *th, double sigma2, hipStream_t s, int64_t p0,
                               int64_t np, bool diag_only)
{
    if (!th) diag_only = false;
    const int nt64 = m->max_nt * (TILE / 64);
    const dim3 grid((unsigned)(diag_only ? 3 * m->max_nt : nt64 * (nt64 + 1) / 2), (unsigned)np);
    const int rc = dispatch_hyper(m, th, [&](auto dd, auto fam, auto pp) {
        hipLaunchKernelGGL((kmat_slab_kernel<dd(), fam(), pp()>), grid, dim3(256), 0, s, m->d_desc + p0, (const real *)m->d_x,
                           (real *)m->d_a, hyper_th<pp()>(m, th, p0), hyper_sigma2<pp()>(m, sigma2, p0), diag_only,
                           (const real *)m->d_diag);
        return 0;
    });
    if (rc) return rc;
    PMK_HIP(hipGetLastError());
    return 0;
}

}  // namespace PMK_NS
}  // namespace pmk
