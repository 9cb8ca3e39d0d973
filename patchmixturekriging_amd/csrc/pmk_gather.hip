// Device-side set-up of a model from one global point array and an index list (pmk_model_create_from_bsp and the *_global
// setters): what pack_soa / upload_targets / pmk_model_set_diag / pmk_model_set_targets_multi of pmk_api.cpp do on the host
// from per-patch arrays, done here from global arrays through the model's index list, into the same buffers with the
// same bits.
//
//   gather_points_kernel   x[d][i] = X[inds[off_r + i]][d] (SoA rows of length ld_r), y[i] = y_global[inds[off_r + i]]
//   gather_vector_kernel   dst[i] = src[inds[off_r + i]]            (targets, diagonal addend)
//   gather_multi_kernel    Ym[i][j] = Y[inds[off_r + i] + j ldy]    (row-major blocks of PMK_MAX_OUTPUTS columns)
//
// One thread per slab row i of a patch.  Rows n_r <= i < ld_r get the padding the host route leaves there: 1e300
// converted to the element type for coordinates (+inf in fp32: the same conversion as the host's upload), zero for
// everything else.  The source arrays are double; the conversion to the element type is a plain cast, as on the host.
//
// Grid: one workgroup per (patch, chunk of 256 rows), located through the prefix over ceil(ld_r / 256) that the model
// keeps (gchunk): with ragged patches a P x max chunk grid would be mostly idle.  A point's D doubles are contiguous in
// X (a gather by nature); the SoA writes are coalesced along i.  The traffic is a few MB: nothing here is tuned.
#include "pmk_dispatch.h"
#include "pmk_real.h"

namespace pmk {
namespace PMK_NS {

constexpr int GCHUNK = 256;

// the patch whose chunks contain `chunk`: the largest r with pre[r] <= chunk (every patch has at least one chunk, so pre
// is strictly increasing)
__device__ __forceinline__ int patch_of_chunk(const int32_t *__restrict__ pre, int P, int chunk)
{
    int lo = 0, hi = P - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (pre[mid] <= chunk) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// the padding coordinate: 1e300 converted to the element type as the host's upload converts it (+inf in fp32)
__device__ __forceinline__ real pad_coordinate()
{
    if constexpr (sizeof(real) == 8) return (real)1e300;
    else return (real)__builtin_inff();
}

template <int D>
__global__ __launch_bounds__(GCHUNK) void gather_points_kernel(const PatchDesc *__restrict__ descs, const int32_t *__restrict__ pre,
                                                               int P, const int64_t *__restrict__ off,
                                                               const int32_t *__restrict__ inds, const double *__restrict__ X,
                                                               const double *__restrict__ y, real *__restrict__ xs,
                                                               real *__restrict__ ys)
{
    const int r = patch_of_chunk(pre, P, (int)blockIdx.x);
    const PatchDesc pd = descs[r];
    const int i = ((int)blockIdx.x - pre[r]) * GCHUNK + (int)threadIdx.x;
    if (i >= pd.ld) return;
    real *row = xs + pd.xoff + i;
    if (i < pd.n) {
        const int64_t idx = inds[off[r] + i];
#pragma unroll
        for (int d = 0; d < D; ++d) row[(int64_t)d * pd.ld] = (real)X[idx * D + d];
        ys[pd.yoff + i] = y ? (real)y[idx] : (real)0;
    } else {
#pragma unroll
        for (int d = 0; d < D; ++d) row[(int64_t)d * pd.ld] = pad_coordinate();
        ys[pd.yoff + i] = (real)0;
    }
}

__global__ __launch_bounds__(GCHUNK) void gather_vector_kernel(const PatchDesc *__restrict__ descs, const int32_t *__restrict__ pre,
                                                               int P, const int64_t *__restrict__ off,
                                                               const int32_t *__restrict__ inds, const double *__restrict__ src,
                                                               real *__restrict__ dst)
{
    const int r = patch_of_chunk(pre, P, (int)blockIdx.x);
    const PatchDesc pd = descs[r];
    const int i = ((int)blockIdx.x - pre[r]) * GCHUNK + (int)threadIdx.x;
    if (i >= pd.ld) return;
    dst[pd.yoff + i] = i < pd.n ? (real)src[inds[off[r] + i]] : (real)0;
}

__global__ __launch_bounds__(GCHUNK) void gather_multi_kernel(const PatchDesc *__restrict__ descs, const int32_t *__restrict__ pre,
                                                              int P, const int64_t *__restrict__ off,
                                                              const int32_t *__restrict__ inds, int R, const double *__restrict__ Y,
                                                              int64_t ldy, real *__restrict__ Ym)
{
    const int r = patch_of_chunk(pre, P, (int)blockIdx.x);
    const PatchDesc pd = descs[r];
    const int i = ((int)blockIdx.x - pre[r]) * GCHUNK + (int)threadIdx.x;
    if (i >= pd.ld) return;
    real *row = Ym + (pd.yoff + i) * PMK_MAX_OUTPUTS;
    const bool live = i < pd.n;
    const int64_t idx = live ? inds[off[r] + i] : 0;
#pragma unroll
    for (int j = 0; j < PMK_MAX_OUTPUTS; ++j) row[j] = (live && j < R) ? (real)Y[idx + (int64_t)j * ldy] : (real)0;
}

int launch_gather_points(const pmk_model *m, const double *d_X, const double *d_y, hipStream_t s)
{
    const dim3 grid((unsigned)m->gchunks), block(GCHUNK);
    real *xs = (real *)m->d_x, *ys = (real *)m->d_y;
    const int P = (int)m->P;
    const int rc = dispatch_dim(m->D, [&](auto dd) {
        hipLaunchKernelGGL(gather_points_kernel<dd()>, grid, block, 0, s, m->d_desc, m->d_gchunk, P, m->d_pidx_off, m->d_pidx,
                           d_X, d_y, xs, ys);
        return 0;
    });
    if (rc) return rc;
    PMK_HIP(hipGetLastError());
    return 0;
}

int launch_gather_vector(const pmk_model *m, const double *d_src, void *d_dst, hipStream_t s)
{
    hipLaunchKernelGGL(gather_vector_kernel, dim3((unsigned)m->gchunks), dim3(GCHUNK), 0, s, m->d_desc, m->d_gchunk, (int)m->P,
                       m->d_pidx_off, m->d_pidx, d_src, (real *)d_dst);
    PMK_HIP(hipGetLastError());
    return 0;
}

int launch_gather_multi(const pmk_model *m, int R, const double *d_Y, int64_t ldy, hipStream_t s)
{
    hipLaunchKernelGGL(gather_multi_kernel, dim3((unsigned)m->gchunks), dim3(GCHUNK), 0, s, m->d_desc, m->d_gchunk, (int)m->P,
                       m->d_pidx_off, m->d_pidx, R, d_Y, ldy, (real *)m->d_ym);
    PMK_HIP(hipGetLastError());
    return 0;
}

}  // namespace PMK_NS
}  // namespace pmk
