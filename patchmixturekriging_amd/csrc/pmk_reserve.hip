// Moving a model into a layout with room to grow (pmk_model_reserve): every patch keeps its nt active block rows and gets
// a new stride ld' >= ld, so all offsets change.  The two kernels write the NEW buffers completely and read the old ones:
// the active part (rows and columns below 128 nt) as copies, everything from 128 nt up to ld' in the state a fit leaves
// in padding -- identity in the slab, the padding coordinate, zeros in y, z, c and the addends, -I in the inverse blocks
// (with the signed zeros ninv_from_slab_kernel gives an identity block).  What the old buffers hold past 128 nt is not
// read: it is that same padding.
//
//   reserve_slab_kernel     a workgroup walks whole columns of one patch's new slab; a thread moves 16 bytes (real2_t or
//                           real4_t) of a column at a time, consecutive threads consecutive pieces.  Slab offsets, strides
//                           and 128 nt are multiples of 128 elements, so every piece is aligned and lies wholly inside
//                           or wholly outside the active part.  Pure bandwidth: ld^2 + ld'^2 elements per patch,
//                           streamed past the caches (nothing is read twice).
//   reserve_vectors_kernel  the coordinates, y, z, c, the addends and the inverse blocks of one patch: a few KB.
#include <algorithm>

#include "pmk_real.h"

namespace pmk {
namespace PMK_NS {

constexpr int RS_THREADS = 256;
constexpr int RS_VEC = 16 / (int)sizeof(real);         // elements of a 16-byte piece
typedef real rs_vec_t __attribute__((ext_vector_type(RS_VEC)));

__global__ __launch_bounds__(RS_THREADS) void reserve_slab_kernel(const PatchDesc *__restrict__ old_descs,
                                                                  const PatchDesc *__restrict__ new_descs,
                                                                  const real *__restrict__ Ao, real *__restrict__ An,
                                                                  int gx)
{
    // blockIdx.x = patch * gx + first column: the patch is not a grid dimension of its own, so P has no bound of 65535 here
    const int patch = (int)(blockIdx.x / (unsigned)gx), j0 = (int)(blockIdx.x % (unsigned)gx);
    const PatchDesc po = old_descs[patch], pn = new_descs[patch];
    const int act = po.nt * TILE, ldn = pn.ld;
    const real *src = Ao + po.aoff;
    real *dst = An + pn.aoff;
    for (int j = j0; j < ldn; j += gx) {
        const real *sc = src + (int64_t)j * po.ld;
        real *dc = dst + (int64_t)j * ldn;
        for (int i = RS_VEC * (int)threadIdx.x; i < ldn; i += RS_VEC * RS_THREADS) {
            rs_vec_t v;
            if (j < act && i < act) {
                v = __builtin_nontemporal_load(reinterpret_cast<const rs_vec_t *>(sc + i));
            } else {
#pragma unroll
                for (int u = 0; u < RS_VEC; ++u) v[u] = (i + u == j) ? (real)1 : (real)0;
            }
            __builtin_nontemporal_store(v, reinterpret_cast<rs_vec_t *>(dc + i));
        }
    }
}

// blockIdx.x: the patch.  diag_o / diag_n are null on a model without addends.
__global__ __launch_bounds__(RS_THREADS) void reserve_vectors_kernel(const PatchDesc *__restrict__ old_descs,
                                                                     const PatchDesc *__restrict__ new_descs, int D,
                                                                     const real *__restrict__ xo, real *__restrict__ xn,
                                                                     const real *__restrict__ yo, real *__restrict__ yn,
                                                                     const real *__restrict__ zo, real *__restrict__ zn,
                                                                     const real *__restrict__ co, real *__restrict__ cn,
                                                                     const real *__restrict__ diag_o, real *__restrict__ diag_n,
                                                                     const real *__restrict__ inv_o, real *__restrict__ inv_n)
{
    const PatchDesc po = old_descs[blockIdx.x], pn = new_descs[blockIdx.x];
    const int act = po.nt * TILE, ldn = pn.ld, tid = threadIdx.x;
    real pad;                                           // 1e300 as the host's upload converts it (+inf in fp32)
    if constexpr (sizeof(real) == 8) pad = (real)1e300;
    else pad = (real)__builtin_inff();
    for (int i = tid; i < ldn; i += RS_THREADS) {
        const bool live = i < act;
        for (int d = 0; d < D; ++d)
            xn[pn.xoff + (int64_t)d * ldn + i] = live ? xo[po.xoff + (int64_t)d * po.ld + i] : pad;
        yn[pn.yoff + i] = live ? yo[po.yoff + i] : (real)0;
        zn[pn.yoff + i] = live ? zo[po.yoff + i] : (real)0;
        cn[pn.yoff + i] = live ? co[po.yoff + i] : (real)0;
        if (diag_n) diag_n[pn.yoff + i] = live ? diag_o[po.yoff + i] : (real)0;
    }
    // four 32 x 32 blocks per block row of the new stride, column-major: entry e of block b is (e & 31, e >> 5)
    const int64_t live_inv = (int64_t)po.nt * 4096, all_inv = (int64_t)(ldn / TILE) * 4096;
    for (int64_t e = tid; e < all_inv; e += RS_THREADS) {
        real v;
        if (e < live_inv) {
            v = inv_o[po.ioff + e];
        } else {
            const int i = (int)(e & 31), c = (int)((e >> 5) & 31);
            v = i == c ? (real)-1 : (i > c ? -(real)0 : (real)0);
        }
        inv_n[pn.ioff + e] = v;
    }
}

// m still holds the old layout (d_desc and the buffers); the arguments are the new one.  max_ld: the largest new stride.
int launch_reserve(const pmk_model *m, const PatchDesc *d_new_desc, void *x, void *y, void *z, void *c, void *diag, void *a,
                   void *inv, int64_t max_ld, hipStream_t s)
{
    // enough workgroups to keep every memory channel busy whatever P is; a workgroup takes every gx-th column
    const int64_t gx = std::min<int64_t>(max_ld, std::max<int64_t>(1, 8192 / m->P));
    hipLaunchKernelGGL(reserve_slab_kernel, dim3((unsigned)(gx * m->P)), dim3(RS_THREADS), 0, s, m->d_desc, d_new_desc,
                       (const real *)m->d_a, (real *)a, (int)gx);
    hipLaunchKernelGGL(reserve_vectors_kernel, dim3((unsigned)m->P), dim3(RS_THREADS), 0, s, m->d_desc, d_new_desc, m->D,
                       (const real *)m->d_x, (real *)x, (const real *)m->d_y, (real *)y, (const real *)m->d_z, (real *)z,
                       (const real *)m->d_c, (real *)c, (const real *)m->d_diag, (real *)diag, (const real *)m->d_inv,
                       (real *)inv);
    PMK_HIP(hipGetLastError());
    return 0;
}

}  // namespace PMK_NS
}  // namespace pmk
