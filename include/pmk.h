/*
 * pmk.h -- C ABI of libpmk_hip.so: the MI355X (gfx950) implementation of the per-patch
 * GP-regression hot path of PatchMixtureKriging.
 *
 * The reference (pure Julia) has no FFI; the surface this ABI replaces is the set of Julia
 * functions that examples/mixGP.jl and examples/IBB1D.jl call.  Each entry point cites the
 * reference function (file:line relative to the reference tree) whose work it takes over.
 * The Julia binding (julia/PatchMixtureKriging) and the Python mirror
 * (patchmixturekriging_amd) both sit on exactly these symbols; INTEGRATION.md shows the
 * ccall stubs.
 *
 * Conventions
 *   - plain C types only; no exceptions or callbacks cross the boundary
 *   - every function returns int status: 0 ok, <0 bad argument / runtime failure
 *     (text via pmk_last_error()), >0 numerical failure
 *   - points are packed point-major: X[d + D*i]  (the D x N column-major matrix of
 *     array2matrix, src/misc/utilities.jl:25-36)
 *   - dense matrices are column-major; all indices are 0-based (Julia wrappers add 1)
 *   - host pointers unless the name says _dev; the caller owns host buffers, the library
 *     owns device memory behind the opaque handles
 *   - fp64 (the reference is Float64-only: src/RKHS/RKHS.jl:4-11, partition.jl:135)
 *   - one call at a time per context (the reference is single-threaded); calls that return
 *     host data block until it is there, the staged *_run / *_fit calls only enqueue on the
 *     context's stream
 */
#ifndef PMK_H
#define PMK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PMK_VERSION 103
#define PMK_MAX_OUTPUTS 16   /* target columns per patch of the multi-output entry points (pmk_model_set_targets_multi) */
#define PMK_BLOCK_MAX_MEMBERS 4096  /* items of one (region, group) aggregate of pmk_query_items_block */
#define PMK_COV_MAX_QUERIES 16384   /* queries of a batch whose joint covariance is asked for (pmk_query_items_cov) */
#define PMK_REMOVE_MAX_ROWS 32   /* rows one patch can lose in one call (pmk_model_remove) */

/* kernel families = the isbits kernel structs of src/misc/declarations.jl:18-45,65-67,75-111 */
enum {
    PMK_SPLINE34 = 1,  /* Spline34KernelType(a)                    kernel.jl:299-313 */
    PMK_SPLINE12 = 2,  /* Spline12KernelType(a)                    kernel.jl:316-330 */
    PMK_SPLINE32 = 3,  /* Spline32KernelType(a)                    kernel.jl:333-347 */
    PMK_GAUSSIAN = 4,  /* GaussianKernel1DType(eps_sq)             kernel.jl:350-357 */
    PMK_RQ       = 5,  /* RationalQuadraticKernelType(a)           kernel.jl:360-366 */
    PMK_TRQ      = 6,  /* TunableRationalQuadraticKernelType(a,w)  kernel.jl:368-374 */
    PMK_MODSQEXP = 7,  /* ModulatedSqExpKernelType(eps_sq,nu), D=1 kernel.jl:376-391 */
    PMK_BB10     = 10, /* BrownianBridge10                         kernel.jl:156-158 */
    PMK_BB20     = 11, /* BrownianBridge20                         kernel.jl:218-225 */
    PMK_BB1EPS   = 12, /* BrownianBridge1eps(eps)                  kernel.jl:168-174 */
    PMK_BB2EPS   = 13  /* BrownianBridge2eps(eps)                  kernel.jl:176-193 */
};
#define PMK_FLAG_SEMIINF 1 /* BrownianBridgeSemiInfDomain{base}      kernel.jl:256-263 */

typedef struct pmk_kernel_desc {
    int32_t family;
    int32_t flags;
    double  p[4];
} pmk_kernel_desc;

/* arithmetic type of the device path.  The reference is Float64-only (RKHS.jl:4-11): PMK_F64 is the parity
 * path; PMK_F32 (fp32 storage + v_mfma_f32, BASELINE config E) has no exact reference semantics and is judged
 * against the fp64 oracle with eps32-scaled bounds.  Host buffers are double in both cases. */
enum { PMK_F64 = 0, PMK_F32 = 1 };

typedef struct pmk_ctx   pmk_ctx;    /* device + stream + workspaces */
typedef struct pmk_bsp   pmk_bsp;    /* host BSP tree (root of setuppartition) */
typedef struct pmk_model pmk_model;  /* fitted MixtureGPType on the device */
typedef struct pmk_query pmk_query;  /* a resident batch of query points + its work items */

int         pmk_version(void);
const char *pmk_last_error(void);

/* ---- context ------------------------------------------------------------------------- */
int  pmk_ctx_create(int device, pmk_ctx **out);
/* launch on a caller-owned hipStream_t (e.g. torch's current stream); NULL -> context's own (a non-blocking stream:
 * NOT ordered with the device's default stream) */
int  pmk_ctx_set_stream(pmk_ctx *ctx, void *hip_stream);
/* launch on the device's legacy default (null) stream -- the stream a framework's "default stream" is: the handle of that
 * stream is 0, which pmk_ctx_set_stream reads as "the context's own" */
int  pmk_ctx_set_stream_null(pmk_ctx *ctx);
int  pmk_ctx_synchronize(pmk_ctx *ctx);
void pmk_ctx_destroy(pmk_ctx *ctx);
/* elapsed ms of the most recent staged call's named stage ("kernel_matrix", "cholesky",
 * "solve", "plan", "items", "mix", "solve_multi", "items_multi", "mix_multi", "loo", "evidence", "trend_gls", "trend_items", "loo_items", "loo_items_multi", "items_grad", "mix_grad", "items_vgrad", "mix_vgrad", "items_cov", "mix_cov", "cov_trend", "factor_cov", "draw"); enabled by pmk_ctx_enable_timers(ctx, 1) */
int  pmk_ctx_enable_timers(pmk_ctx *ctx, int on);
int  pmk_ctx_timer_ms(pmk_ctx *ctx, const char *stage, double *ms);
/* shader clock (GHz) that workgroups 0..7 (one per XCD) saw over their lifetime in the factorisation step launches of
 * the last fit (which = 0) or in the last prediction strip kernel (which = 1), time-weighted mean; 0 if none has run.  The fp64 MFMA peak that the
 * rooflines are priced against assumes the nominal 2.4 GHz; under these kernels the chip runs slower. */
int  pmk_ctx_shader_clock(pmk_ctx *ctx, int which, double *ghz);

/* ---- BSP: host, exact (integer outputs are part of the parity contract) --------------- */
/* setuppartition(X, levels)  src/patchwork/partition.jl:106-129 (+ gethyperplane :86-100,
 * splitpoints :64-83, createchildren :166-217, labelleafnodes :131-159).
 * Two Julia-stdlib behaviours that the reference's text does not fix are switches, stored with the tree and honoured by
 * every later search on it (host and device):
 *   sign_mode +1: v = +z/|z| ; -1: v = -sign(z1) z/|z|           (sign convention of svd)
 *   dot_mode   0: dot(v, x) = separate multiplies and adds ; 1: a chain of fused multiply-adds
 *                 (LinearAlgebra.dot -> BLAS ddot: whether its short loop was contracted depends on the BLAS build) */
int     pmk_bsp_build(int D, int64_t N, const double *X, int levels, int sign_mode, int dot_mode, pmk_bsp **out);
/* the same build on the GPU (X: host or device pointer, point-major N x D; N < 2^31): level-by-level segmented
 * pairwise sums, radix-sort medians and stable splits; every output equals pmk_bsp_build's bit for bit.  Blocks. */
int     pmk_bsp_build_device(pmk_ctx *ctx, int D, int64_t N, const double *X, int levels, int sign_mode, int dot_mode,
                             pmk_bsp **out);
/* rebuild a tree from its pre-order hyperplanes (for shipping a tree between processes) */
int     pmk_bsp_from_hyperplanes(int D, int levels, const double *hp_v, const double *hp_c, int dot_mode, pmk_bsp **out);
void    pmk_bsp_destroy(pmk_bsp *bsp);
int     pmk_bsp_dim(const pmk_bsp *bsp);
int     pmk_bsp_levels(const pmk_bsp *bsp);
int     pmk_bsp_dot_mode(const pmk_bsp *bsp);
int64_t pmk_bsp_num_leaves(const pmk_bsp *bsp);
int64_t pmk_bsp_num_points(const pmk_bsp *bsp);
/* fetchhyperplanes(root)  src/RKHS/mixtureGP.jl:322-334 : pre-order; hp_v is D x (P-1).
 * leaf_offsets[P+1], leaf_inds[N]: X_parts_inds of setuppartition (ascending per leaf).
 * Any pointer may be NULL. */
int     pmk_bsp_arrays(const pmk_bsp *bsp, double *hp_v, double *hp_c,
                       int64_t *leaf_offsets, int64_t *leaf_inds);
/* organizetrainingsets(root, levels, X0, eps)  partition.jl:301-357 (+ :269-298).
 * offsets[P+1] always written; inds[offsets[P]] = X_set_inds grouped by region;
 * list_offsets[N+1] + lists = regions_list_set.  inds/list_offsets/lists may be NULL
 * (call once with NULLs to size the buffers). */
int     pmk_bsp_assign(const pmk_bsp *bsp, int64_t N, const double *X, double eps,
                       int64_t *offsets, int64_t *inds, int64_t *list_offsets, int64_t *lists);
/* the same assignment on the GPU (X: host or device pointer; outputs on the host, identical to pmk_bsp_assign's) */
int     pmk_bsp_assign_device(pmk_ctx *ctx, const pmk_bsp *bsp, int64_t N, const double *X, double eps,
                              int64_t *offsets, int64_t *inds, int64_t *list_offsets, int64_t *lists);
/* findpartition(x, root, levels)  partition.jl:248-262 ; returns the leaf or <0 */
int64_t pmk_bsp_findpartition(const pmk_bsp *bsp, const double *x);
/* findneighbourpartitions(p, radius, root, levels, hps, home; delta)  mixtureGP.jl:339-405.
 * returns the number kept (or <0); region_inds[<=P-1]; ts[P-1], zs[D x (P-1)], keep[P-1]
 * may be NULL. */
int64_t pmk_bsp_neighbours(const pmk_bsp *bsp, const double *p, double radius, double delta,
                           int64_t home, int64_t *region_inds, double *ts, double *zs, uint8_t *keep);

/* ---- kernel matrix (device compute, host in/out) -------------------------------------- */
/* constructkernelmatrix(X, theta)  src/RKHS/RKHS.jl:4-34  (Z == NULL: n x n, exactly symmetric)
 * constructkernelmatrix(X, Z, theta)  RKHS.jl:95-110      (Z != NULL: n x m) */
int pmk_kernel_matrix(pmk_ctx *ctx, const pmk_kernel_desc *th, int D,
                      int64_t n, const double *X, int64_t m, const double *Z,
                      double *K, int64_t ldk);

/* ---- fit ------------------------------------------------------------------------------ */
/* MixtureGPType(X_set, hps) + upload: src/RKHS/mixtureGP.jl:54-66.  P patches, patch r has
 * n[r] points X[r] (D x n[r]) and targets y[r].  Inputs become device-resident. */
int  pmk_model_create(pmk_ctx *ctx, int D, int64_t P, const int64_t *n,
                      const double *const *X, const double *const *y, pmk_model **out);
/* same with an explicit arithmetic type (PMK_F64 / PMK_F32) */
int  pmk_model_create_ex(pmk_ctx *ctx, int D, int64_t P, const int64_t *n,
                         const double *const *X, const double *const *y, int dtype, pmk_model **out);
/* fitmixtureGP!(eta, y_parts, theta, sigma2)  mixtureGP.jl:70-118 on the resident inputs:
 * per patch K (RKHS.jl:13-34), U = K + sigma2 I, L = chol(U), c = U^-1 y (one Cholesky
 * serves both; the reference's separate LU of :106 is not repeated).  Enqueues only. */
int  pmk_model_fit(pmk_model *m, const pmk_kernel_desc *th, double sigma2);
/* blocks; info[P]: 0 ok, k>0 leading minor k not positive definite (PosDefException(k)), 1 <= k <= n.  Returns 1 if any
 * patch failed, 0 if none, < 0 on error (-4: the chained solves timed out, -5: a status word outside 1..n) */
int  pmk_model_info(pmk_model *m, int32_t *info);
/* replace the resident targets (same sizes) */
int  pmk_model_set_targets(pmk_model *m, const double *const *y);
/* Per-point addend of the kernel's DIAGONAL: the next fits use K[i][i] = k(x_i, x_i) + diag[r][i] (+ sigma2).  This is
 * what the reference's AdaptiveKernelDPPType / AdaptiveKernelMultiWarpDPPType add where p == q (src/RKHS/kernel.jl:70-75,
 * 102-110: 1 + g(p)^2, resp. 1 + self_gain sum a_m |w_m(p)|), the rest of those kernels being a stationary kernel on
 * positions + appended warp values.  diag = NULL clears it.  Blocks. */
int  pmk_model_set_diag(pmk_model *m, const double *const *diag);
enum { PMK_GET_C = 0, PMK_GET_L = 1, PMK_GET_K = 2, PMK_GET_LINV_DIAG = 3 };
/* pull c_set[r] (n), L_set[r] (n x n lower, strict upper zero), U_set[r] (n x n, K without
 * noise, rebuilt on demand), or the negated inverses of the 32 x 32 diagonal blocks of L
 * (4 ceil(n/128) blocks, 32 x 32 column-major each; the TRSM operands, for tests) */
int  pmk_model_get(pmk_model *m, int64_t patch, int what, double *out, int64_t ld);
int64_t pmk_model_num_patches(const pmk_model *m);
void pmk_model_destroy(pmk_model *m);
/* one-shot convenience = create + fit + info + c_out (rows 13 and 17 of the scope table;
 * fitRKHS! src/RKHS/RKHS.jl:182-217 is the P == 1 case).  c_out[r] may be NULL. */
int  pmk_fit_batched(pmk_ctx *ctx, const pmk_kernel_desc *th, double sigma2, int D, int64_t P,
                     const int64_t *n, const double *const *X, const double *const *y,
                     pmk_model **out, double *const *c_out, int32_t *info);

/* rebuild a device model from host factors (c_set, L_set of a fitted MixtureGPType; L[r] is n[r] x n[r]
 * column-major with leading dimension ldl[r], lower triangle used): the checkpoint/resume path, and what
 * queryinner(xq, X, theta, c, L) needs.  The TRSM operands are recomputed on the device. */
int  pmk_model_load(pmk_ctx *ctx, int D, int64_t P, const int64_t *n, const double *const *X,
                    const double *const *c, const double *const *L, const int64_t *ldl, pmk_model **out);
/* queryinner(xq, X, theta, c, L)  src/RKHS/mixtureGP.jl:296-320, batched over Nq points against ONE patch:
 * mu[j] = k(xq_j, X).c,  var[j] = clamp(k(xq_j,xq_j) - |L^-1 k(xq_j, X)|^2, 1e-12, inf).  No tree needed. */
int  pmk_model_queryinner(pmk_model *m, int64_t patch, const pmk_kernel_desc *th, int64_t Nq, const double *Xq,
                          double *mu, double *var);
/* the same with the keyword min_v of queryinner! (mixtureGP.jl:296): var = max(k(x,x) - |L^-1 k|^2, min_v).  min_v =
 * -HUGE_VAL gives the unclamped variance term1 - term2 of evalqueryGP! (src/RKHS/querying.jl:61-79) */
int  pmk_model_queryinner_ex(pmk_model *m, int64_t patch, const pmk_kernel_desc *th, int64_t Nq, const double *Xq,
                             double min_v, double *mu, double *var);
/* replace the resident weights c_set (setupGPquery(c, X, theta, sigma2), querying.jl:43-59, takes c from its caller:
 * fit for the factor of K + sigma2 I, then put the caller's c in place) */
int  pmk_model_set_weights(pmk_model *m, const double *const *c);
/* all weight vectors at once: c[r] receives the n_r weights of patch r (one device-to-host transfer for the whole
 * model; what fitmixtureGP! stores into c_set, mixtureGP.jl:106,115) */
int  pmk_model_get_weights(pmk_model *m, double *const *c);

/* ---- predict -------------------------------------------------------------------------- */
/* attach the tree; this model holds the global leaves [leaf_base, leaf_base + P) */
int  pmk_model_set_bsp(pmk_model *m, const pmk_bsp *bsp, int64_t leaf_base);
/* upload Nq query points (Xq: host or device pointer, point-major Nq x D) */
int  pmk_query_create(pmk_model *m, int64_t Nq, const double *Xq, pmk_query **out);
/* stage 1: home leaf (partition.jl:248-262) + neighbour items (mixtureGP.jl:339-405) for
 * every query, items sorted by region (stable).  Blocks (sizes come back to the host). */
int  pmk_query_plan(pmk_query *q, double radius, double delta);
/* number of (query, region) items in total and in this model's regions */
int  pmk_query_counts(pmk_query *q, int64_t *total_items, int64_t *first_owned, int64_t *num_owned);
/* region_offsets[P_global+1] of the sorted item list (host copy) */
int  pmk_query_region_offsets(pmk_query *q, int64_t *region_offsets);
/* stage 2: queryinner! (mixtureGP.jl:296-316) for every owned item: u = kq.c,
 * v = clamp(k(x,x) - |L^-1 kq|^2, 1e-12, inf).  Enqueues only. */
int  pmk_query_items(pmk_query *q, const pmk_kernel_desc *th);
/* device pointers of the per-item results in sorted order (length total_items each): where a multi-GPU caller that
 * drives the exchange itself deposits the (u, v) it gets back from the leaf owners between stage 2 and 3 */
int  pmk_query_item_buffers(pmk_query *q, void **u_dev, void **v_dev);
/* ---- multi-GPU, queries sharded over ranks: a rank plans only its own queries against the
 * global tree, sends the (point, region) requests of every sorted-list segment to the rank that owns those leaves,
 * which evaluates queryinner! for them and sends (u, v) back into the requester's item buffers.
 * requests of the sorted items [first, first + n) -> DEVICE arrays xq_dev [n x D point-major], region_dev [n] */
int  pmk_query_export_requests(pmk_query *q, int64_t first, int64_t n, double *xq_dev, int32_t *region_dev);
/* per-query addend of k(xq, xq) in the predictive variance (the same diagonal term for a query point; host or device
 * pointer, Nq values; NULL clears) */
int  pmk_query_set_diag(pmk_query *q, const double *diag);
/* the addends of the sorted items [first, first + n) -> DEVICE array diag_dev [n] (zeros when the query has none): what a
 * requester ships with its requests, for the owner's pmk_query_set_diag on the received items.  1 if the query carries
 * addends, 0 if not.  Enqueues. */
int  pmk_query_export_request_diag(pmk_query *q, int64_t first, int64_t n, double *diag_dev);
/* a planned batch of n explicit (point, region) items, one per point (host or device pointers); every region must
 * lie in this model's leaves (-3 otherwise).  Follow with pmk_query_items + pmk_query_export_results. */
int  pmk_query_create_items(pmk_model *m, int64_t n, const double *xq, const int32_t *region, pmk_query **out);
/* (u, v) of all items in item order (the order given to pmk_query_create_items; reference order for a planned
 * query) -> DEVICE arrays of length total_items (either may be NULL).  Enqueues. */
int  pmk_query_export_results(pmk_query *q, double *u_dev, double *v_dev);
/* ---- multi-GPU inside the library: an RCCL communicator (one rank per GPU, xGMI) owned by a context --------------
 * rank 0 calls pmk_comm_unique_id and ships the 128 bytes to the other ranks by any host channel (MPI.jl, a file,
 * torch.distributed ...); every rank then calls pmk_comm_create (collective).  RCCL is bound at run time. */
#define PMK_COMM_ID_BYTES 128
typedef struct pmk_comm pmk_comm;
int  pmk_comm_unique_id(void *id_out);
int  pmk_comm_create(pmk_ctx *ctx, int rank, int world, const void *id, pmk_comm **out);
int  pmk_comm_rank(const pmk_comm *comm);
int  pmk_comm_size(const pmk_comm *comm);
void pmk_comm_destroy(pmk_comm *comm);
/* (first, count) of every rank's segment of a region-sorted item list (rank r owns leaves [r P/world, (r+1) P/world)) */
int  pmk_shard_segments(const int64_t *region_offsets, int64_t P_global, int world, int64_t *first, int64_t *count);
/* one predict step of a model whose leaves and queries are sharded over the communicator (collective):
 * querymixtureGP! (mixtureGP.jl:159-294) for THIS rank's queries = plan -> requests to the leaf owners (grouped
 * ncclSend/ncclRecv) -> queryinner! for everything received -> (u, v) back -> mixture.  Enqueues on the context's
 * stream after the plan; results with pmk_query_fetch.  total_items (may be NULL): this rank's item count. */
int  pmk_query_predict_sharded(pmk_query *q, pmk_comm *comm, const pmk_kernel_desc *th,
                               const pmk_kernel_desc *weight_th, double radius, double delta, int64_t *total_items);
/* the same step with REPLICATED queries (every rank passes all queries): plan of all queries -> queryinner! for the items
 * in this rank's leaves -> one ncclAllGather of padded (u, v) slices (every rank knows every slice's size from its own
 * plan) -> mixture of all queries on every rank.  BASELINE.json's "RCCL all-gather ... of the per-patch predictions before
 * the mixture weights are applied", literally; collective. */
int  pmk_query_predict_allgather(pmk_query *q, pmk_comm *comm, const pmk_kernel_desc *th,
                                 const pmk_kernel_desc *weight_th, double radius, double delta, int64_t *total_items);
/* payload bytes this rank sent / received in the exchange of its last predict step (either form) */
int  pmk_comm_last_bytes(const pmk_comm *comm, int64_t *sent, int64_t *received);
/* stage 3: mixture weights and blend (mixtureGP.jl:224-272) for queries [q0, q1).  Enqueues. */
int  pmk_query_mix(pmk_query *q, const pmk_kernel_desc *weight_th, int64_t q0, int64_t q1);
/* blocks; Yq, Vq [Nq] (either may be NULL) */
int  pmk_query_fetch(pmk_query *q, double *Yq, double *Vq);
/* debug_vars of MixtureGPDebugType (mixtureGP.jl:5-35): home[Nq], item_offsets[Nq+1],
 * then per item in reference order (neighbours in hyperplane order, home last):
 * item_region, item_t (0 for home), item_w (unnormalised), item_u, item_v.  NULLs allowed. */
int  pmk_query_debug(pmk_query *q, int64_t *home, int64_t *item_offsets, int64_t *item_region,
                     double *item_t, double *item_w, double *item_u, double *item_v);
void pmk_query_destroy(pmk_query *q);
/* one-shot querymixtureGP!(Yq,Vq,Xq,eta,root,levels,radius,delta,theta,sigma2,weight_theta,..)
 * src/RKHS/mixtureGP.jl:159-294 for a model that holds every leaf */
int  pmk_predict_mixture(pmk_model *m, const pmk_kernel_desc *th, const pmk_kernel_desc *weight_th,
                         int64_t Nq, const double *Xq, double radius, double delta,
                         double *Yq, double *Vq);
/* ---- multi-output targets: R target columns per patch that share one factor ---------------------------------------
 * The factor of K + sigma2 I depends only on the points and theta (mixtureGP.jl:99-112), so R fields on the same points
 * (image channels, vector-field components, a time series on fixed sensors) need one factorisation and R solves.  One
 * theta and sigma2 for every column.  Not available through the sharded / all-gather exchanges. */
/* the targets y_parts of fitmixtureGP! (mixtureGP.jl:70-118) as R columns: Y[r] is n[r] x R column-major with leading
 * dimension ldy[r] >= n[r], 1 <= R <= PMK_MAX_OUTPUTS.  Blocks.  Does not touch the single-output y / z / c. */
int  pmk_model_set_targets_multi(pmk_model *m, int R, const double *const *Y, const int64_t *ldy);
/* c = U \ y of fitmixtureGP! (mixtureGP.jl:106) for all R columns of every patch, C = (L L^T)^-1 Y, from the RESIDENT
 * factor (after pmk_model_fit or pmk_model_load): no refactorisation.  Enqueues. */
int  pmk_model_solve_multi(pmk_model *m);
/* blocks; C[r] (n[r] x R column-major, leading dimension ldc[r] >= n[r]) receives the weights of patch r */
int  pmk_model_get_weights_multi(pmk_model *m, double *const *C, const int64_t *ldc);
/* stage 2 with R columns, queryinner! (mixtureGP.jl:296-316) for every item: U[item][j] = kq . C[:, j] (no
 * triangular solve); want_var != 0 also computes v exactly as pmk_query_items does.  The model must hold every leaf.
 * Enqueues. */
int  pmk_query_items_multi(pmk_query *q, const pmk_kernel_desc *th, int want_var);
/* stage 3 with R columns: the mixture weights and blend of pmk_query_mix (mixtureGP.jl:224-272) for every column of U
 * (and v, if it was computed) for queries [q0, q1).  Enqueues. */
int  pmk_query_mix_multi(pmk_query *q, const pmk_kernel_desc *weight_th, int64_t q0, int64_t q1);
/* blocks; Yq: Nq x R column-major with leading dimension ldyq >= Nq; Vq [Nq] or NULL (must be NULL if the items ran
 * with want_var = 0) */
int  pmk_query_fetch_multi(pmk_query *q, double *Yq, int64_t ldyq, double *Vq);
/* one-shot querymixtureGP! (mixtureGP.jl:159-294) with R columns, like pmk_predict_mixture; Vq == NULL skips the
 * variance (no triangular solve at all): R = 1 without Vq is the mean-only prediction */
int  pmk_predict_mixture_multi(pmk_model *m, const pmk_kernel_desc *th, const pmk_kernel_desc *weight_th, int64_t Nq,
                               const double *Xq, double radius, double delta, double *Yq, int64_t ldyq, double *Vq);

/* ---- kriging with a trend: one generalised-least-squares drift per patch, on the multi-output path -------------------
 * Every fit above is SIMPLE kriging: c = U^-1 y assumes a zero-mean field, so a prediction falls to 0 where the kernel's
 * support runs out of data.  A trend makes it ordinary kriging (unknown constant mean, q = 1, h = [1]) or universal
 * kriging with a linear drift (q = 1 + D, h(x) = [1, x_1 .. x_D]).  The coordinates are the RAW coordinates the model
 * stores, all D of them, uncentred: beta is with respect to raw coordinates.  With H the n x q basis of a patch:
 *   [C_Y | C_H] = U^-1 [Y | H],  G = H^T C_H,  beta = G^-1 H^T C_Y (q x R),  C = C_Y - C_H beta  (so H^T C = 0)
 *   query x*:  mu_j = kq^T C[:, j] + h(x*)^T beta_j,   v = v_sk + |L_G^-1 (h(x*) - kq^T C_H)|^2,  G = L_G L_G^T
 * where v_sk is the variance of pmk_query_items, ALREADY clamped at its floor (1e-12): the trend term is added after the
 * clamp.  One beta per patch; the mixture blends the per-patch (mu, v) as before.
 * The trend is state of the MULTI-OUTPUT path only: pmk_model_fit's c, pmk_query_items, pmk_predict_mixture,
 * pmk_model_evidence and pmk_model_get_loo ignore it and keep their bits; a single target with a trend is R = 1 here.  It
 * works on whatever factor is resident (pmk_model_fit, pmk_model_fit_patches, pmk_model_load; diagonal addends; split
 * mode; fp64 and fp32) and needs R + q <= PMK_MAX_OUTPUTS.  Not available through the sharded / all-gather exchanges.
 * With a trend set, pmk_model_solve_multi writes H into columns R .. R+q-1 of the target block, solves all R + q columns
 * in its one launch and runs the per-patch GLS (-3 if R + q > PMK_MAX_OUTPUTS); pmk_model_get_weights_multi then returns
 * the universal-kriging weights C; pmk_query_items_multi / _fitted return mu and v as above; pmk_model_get_loo_multi
 * returns res_ij = C_ij / Q_ii and var_i = 1 / Q_ii with Q_ii = d_i - |L_G^-1 C_H[i,:]^T|^2 (the leave-one-out of the
 * universal-kriging predictor, beta refitted without point i); pmk_model_evidence_multi's quad = Y^T C is the GLS
 * quadratic form (y - H beta)^T U^-1 (y - H beta) without any change (H^T C = 0), and log det G for a restricted
 * likelihood comes from pmk_model_get_trend.  Back at PMK_TREND_NONE the next solve clears the extra columns and every
 * result is bit-identical to a model that never had a trend.  Stage timers "trend_gls" and "trend_items".
 * Per-patch status tinfo[r]: 0 ok; a in 1..q: pivot a of the Cholesky of G_r is <= 0 or NaN (a basis column that is
 * exactly zero or exactly dependent, e.g. a coordinate that is 0 for every point); n_r + 1: the patch has n_r < q points
 * (flagged without computing; n_r + 1 <= q then, so a value in 1..q means this whenever n_r < q and a pivot otherwise:
 * tell the two apart by n_r).  A flagged patch, and a patch whose factorisation failed (pmk_model_info != 0; its tinfo
 * stays 0), gets NaN in beta, in its R weight columns and in everything derived from them; other patches keep their bits.
 * A NEARLY singular G (points that are almost collinear in an oblique direction) is NOT flagged: G is returned so that
 * the caller can judge its conditioning. */
enum { PMK_TREND_NONE = -1, PMK_TREND_CONSTANT = 0, PMK_TREND_LINEAR = 1 };
/* host state only; marks the multi-output weights stale (run pmk_model_solve_multi again).  -2: unknown degree */
int  pmk_model_set_trend(pmk_model *m, int degree);
/* blocks. *q: basis functions of the last solve (0 without a trend); beta[a + q*(j + R*r)]: coefficient a of column j of
 * patch r; G[a + q*(b + q*r)] = (H^T U^-1 H)_ab of patch r.  Any pointer may be NULL.  -3 before pmk_model_solve_multi. */
int  pmk_model_get_trend(pmk_model *m, int *q, double *beta, double *G);
/* blocks. tinfo[P] as above (zeros without a trend); returns 1 if any patch is flagged, 0 if none, -3 before
 * pmk_model_solve_multi */
int  pmk_model_trend_info(pmk_model *m, int32_t *tinfo);

/* ---- model selection from the resident factor -------------------------------------------------------------------------
 * Two per-patch scores of a fit at (theta, sigma2), both from what pmk_model_fit leaves on the device (Rasmussen &
 * Williams, Gaussian Processes for Machine Learning, eq. 5.8 and 5.10-5.12); the reference picks theta and sigma2 by hand
 * (examples/mixGP.jl:32-35).  With U = K + sigma2 I = L L^T and c = U^-1 y:
 *   log marginal likelihood of patch r = -1/2 quad - 1/2 logdet - n/2 log(2 pi)
 *   leave-one-out prediction of training point i from the other n - 1:  y_i - mu_-i = c_i / d_i,  variance 1 / d_i,
 *   d = diag(U^-1), for every i at once and without refitting.
 * The scores are PER PATCH: a training point that lies in several overlapping patches has one score in each.  A patch
 * whose factorisation failed (info != 0) returns NaN in all of logdet, quad, res, var.  Not available through the
 * sharded / all-gather exchanges. */
/* blocks. logdet[P]: 2 sum_i log L_ii of every patch (log det of K + sigma2 I); quad[P]: y^T c.
 * Either may be NULL.  A model built by pmk_model_load holds no targets: quad must be NULL there. */
int  pmk_model_evidence(pmk_model *m, double *logdet, double *quad);
/* the same for the R columns of pmk_model_set_targets_multi after pmk_model_solve_multi:
 * quad[r + P*j] = Y[:,j]^T C[:,j] */
int  pmk_model_evidence_multi(pmk_model *m, double *logdet, double *quad);
/* d = diag((L L^T)^-1) of every patch from the RESIDENT factor (after pmk_model_fit or pmk_model_load): the squared
 * column norms of L^-1, n^3/3 flop per patch on MFMA.  d depends on the factor only: it stays valid until the next
 * pmk_model_fit, whatever pmk_model_set_weights / pmk_model_solve_multi do to the weights.  Enqueues.  Stage timer "loo". */
int  pmk_model_loo(pmk_model *m);
/* blocks. res[r][i] = c_i / d_i (= y_i - mu_-i, so mu_-i = y_i - res[r][i]) from the weights resident at the time of the
 * call, var[r][i] = 1 / d_i (includes sigma2).  Either may be NULL. */
int  pmk_model_get_loo(pmk_model *m, double *const *res, double *const *var);
/* R columns: RES[r] is n[r] x R column-major, leading dimension ldres[r] >= n[r]; var is shared by the columns.
 * With a trend of q basis functions, a patch of n_r <= q points returns NaN in RES and var: leaving one point out leaves
 * fewer points than basis functions, so no leave-one-out prediction exists (at n_r == q the fit itself is fine, tinfo is
 * 0 and Q_ii is 0 up to rounding).  beta, the weights and ordinary queries of such a patch are unchanged. */
int  pmk_model_get_loo_multi(pmk_model *m, double *const *RES, const int64_t *ldres, double *const *var);

/* ---- blended leave-one-out: cross-validate the MIXTURE predictor, no refits ---------------------------------------------
 * The scores above are per patch; what is deployed is the blend of querymixtureGP! (mixtureGP.jl:159-294): home leaf plus
 * the neighbours within radius, weights phi_w(|t|), normalised.  Leaving global point j out of the model removes it from
 * every patch that holds it and changes nothing else (the patches are independent GPs; the tree is held fixed), so for
 * the query x_j an item (j, region r) is
 *   member (patch r holds j as row i):  u = y_i - c_i / d_i,  v = 1 / d_i if noisy, else max(1 / d_i - sigma2_r, min_v):
 *     the Schur complement of row i of U = K + sigma2 I, from d = diag(U^-1) of pmk_model_loo.  Double, IEEE division: the
 *     values numpy computes from pmk_model_get_loo's res and var.  sigma2_r is the noise the resident factor was fitted
 *     with (pmk_model_fit's, or pmk_model_fit_patches' of that patch).  A patch with info != 0 gives NaN in both.
 *   non-member (a neighbour region reached with radius > eps, which never saw j):  the (u, v) of pmk_query_items_fitted for
 *     that (point, region), the same bits, pmk_query_set_diag's addend honoured; with noisy, sigma2_r is added with one
 *     add after the clamp.  NaN in both if the patch's factorisation failed.
 * and blending these items with pmk_query_mix is exactly the leave-one-out of the blended predictor.  In 1 / d - sigma2
 * the two terms agree to within the patch's leverage at the point: where the data determine the point (1 / d close to
 * sigma2) the latent variance loses about log2(sigma2 / (1 / d - sigma2)) bits, and is clamped at min_v like any
 * predictive variance; the noisy form has no subtraction.
 * Limits.  The scores use the RESIDENT y and c: after pmk_model_set_weights they mean what the caller makes of them.  This
 * call is the single-output path and ignores the trend; R target columns and the trend are pmk_query_items_loo_multi's
 * below.  Not available through the sharded / all-gather exchanges.  Stage timer "loo_items" (and "items" inside it, if and only if strips ran). */
/* stage 2 for a query whose points ARE the model's training points: query j is global point j of
 * pmk_model_create_from_bsp (Nq == N).  After pmk_query_plan, instead of pmk_query_items*; pmk_query_mix, pmk_query_fetch(_dev)
 * and pmk_query_debug then work unchanged.  n_member / n_strip (either may be NULL): how many items took each route; with
 * n_strip == 0 no strip kernel is launched and no inner query is created.  Blocks once for the number of non-members and,
 * if there are any, once more while the inner query of explicit items is set up (as pmk_query_create_items does); the
 * strips, the scatter and everything after only enqueue.
 * Refusals, before any launch: -1 not planned or not fitted; -3 the model was not made by pmk_model_create_from_bsp,
 * Nq != N, the model does not hold every leaf, it holds no kernels, or pmk_model_loo has not run since the last fit. */
int  pmk_query_items_loo(pmk_query *q, int noisy, int64_t *n_member, int64_t *n_strip);
/* one-shot: create(X) + plan + items_loo + mix + fetch, like pmk_predict_mixture_fitted; X: the N training points in
 * global order (host or device pointer) */
int  pmk_predict_mixture_loo(pmk_model *m, const pmk_kernel_desc *weight_th, const double *X,
                             double radius, double delta, int noisy, double *Yq, double *Vq);

/* ---- blended leave-one-out of the multi-output path: R target columns, with or without a trend ---------------------------
 * The same identity on what pmk_model_solve_multi left resident (the R columns Y, the weights C, with a trend C_H, L_G and
 * beta per patch) and d of pmk_model_loo.  For the query x_j an item (j, region r) is
 *   member (patch r holds j as row i):  Q_ii = d_i - |L_G^-1 C_H[i, :]^T|^2 (Q_ii = d_i without a trend), and for every
 *     column c < R:  mu_c = Y[i, c] - C[i, c] / Q_ii;  v = 1 / Q_ii if noisy, else max(1 / Q_ii - sigma2_r, min_v).  C is the
 *     resident weight block: with a trend the universal-kriging weights C_Y - C_H beta.  Double, IEEE division, Q by the
 *     forward substitution of the per-patch values: what numpy computes from pmk_model_get_loo_multi's RES and var.
 *   non-member:  the item of pmk_query_items_multi_fitted for that (point, region), the same bits: mu_c with h(x)^T beta_c
 *     added, v with the trend term added after the clamp; with noisy, sigma2_r is added with one add after that.
 * NaN in every column and in v for a patch with info != 0 or, with a trend, tinfo != 0.  With a trend of q basis functions
 * a MEMBER item of a patch of n_r <= q points is NaN in every column and in v as well (no leave-one-out prediction from
 * fewer than q points, as in pmk_model_get_loo_multi); a non-member item of a patch of n_r == q points stays the fitted
 * predictor's, bit for bit.  In 1 / Q - sigma2 the cancellation
 * is that of the single-output form, with the leverage of the point under the trend model; clamped at min_v.
 * want_var = 0: means only; no strip kernel runs anywhere, v is not computed and pmk_query_fetch_multi refuses Vq.
 * After pmk_query_plan, instead of pmk_query_items_multi*; pmk_query_mix_multi, pmk_query_fetch_multi(_dev) and
 * pmk_query_get_items_multi then serve unchanged.  n_member / n_other (either may be NULL): how many items took each route;
 * with n_other == 0 nothing runs after the scan of the marks and no inner query is created.  Blocks as pmk_query_items_loo.
 * Refusals, before any launch: those of pmk_query_items_loo, and -3 if pmk_model_solve_multi has not run on the resident
 * factor (a new fit, pmk_model_set_targets_multi* and pmk_model_set_trend each make it stale).  pmk_query_items_loo itself
 * keeps its bits and still ignores the trend.  Limits: no sharded or all-gather exchange; the model must hold every leaf.
 * Stage timer "loo_items_multi" ("items_multi" and "trend_items" inside it, if and only if there are non-members). */
int  pmk_query_items_loo_multi(pmk_query *q, int noisy, int want_var, int64_t *n_member, int64_t *n_other);
/* one-shot: create(X) + plan + items_loo_multi + mix_multi + fetch_multi; Yq is N x R column-major with ldyq >= N;
 * Vq == NULL: means only */
int  pmk_predict_mixture_loo_multi(pmk_model *m, const pmk_kernel_desc *weight_th, const double *X, double radius,
                                   double delta, int noisy, double *Yq, int64_t ldyq, double *Vq);
/* the per-item results of pmk_query_items_multi, _multi_fitted or _loo_multi on the host: U[i * ldu + c] is mean c of item i
 * (ldu >= R), v[i] its variance, items in the order of pmk_query_debug (per query: neighbours in hyperplane order, home
 * last).  Either may be NULL; v must be NULL after a mean-only run (-3).  -2 if no multi-output items ran on this plan.
 * Blocks. */
int  pmk_query_get_items_multi(pmk_query *q, double *U, int64_t ldu, double *v);

/* ---- per-patch kernels and noise ---------------------------------------------------------------------------------------
 * MixtureGPType carries one noise variance per patch (sigma2_set::Vector, mixtureGP.jl:44,114), and fitmixtureGP!
 * (mixtureGP.jl:70-118) fills it with one value; here every patch may have its own kernel and its own noise variance, which
 * is what the per-patch scores above are for.  ths[P] and sigma2[P] are indexed by the model's local patch; families may
 * differ between patches.  The device runs the Spline34 instantiation of its kernels if EVERY patch is PMK_SPLINE34 and
 * the run-time family switch otherwise (as the uniform calls do for one theta), so a patch's factor has the bits of the
 * uniform fit that takes the same instantiation.  The mixture weight kernel weight_th stays global.  Not available
 * through the sharded / all-gather exchanges (pmk_query_predict_sharded / _allgather) nor through pmk_fit_batched. */
/* fitmixtureGP! (mixtureGP.jl:70-118) with one kernel and one noise variance PER PATCH.  The kernel matrix is always built
 * whole (no fused build).  An unknown family in ths[r], or PMK_MODSQEXP with D > 1, returns -2 and the error text names
 * patch r; NULL arrays return -1.  Enqueues only (after draining the stream once to replace the device copies of both
 * arrays); the model remembers both arrays. */
int  pmk_model_fit_patches(pmk_model *m, const pmk_kernel_desc *ths, const double *sigma2);
/* kernels of a model built by pmk_model_load (which holds factors, mixtureGP.jl:112, but no theta), for the *_fitted
 * calls below; -3 on any other model (a fit records its own kernels).  Blocks. */
int  pmk_model_set_kernels(pmk_model *m, const pmk_kernel_desc *ths);
/* the hyperparameters the resident factor belongs to: ths[P], sigma2[P] (either may be NULL).  After a plain pmk_model_fit
 * P copies of its theta and sigma2; after pmk_model_set_kernels sigma2 is NaN (the factor's noise is not known).  -3 if
 * the model holds no kernels. */
int  pmk_model_get_hyper(pmk_model *m, pmk_kernel_desc *ths, double *sigma2);
/* stage 2 (queryinner!, mixtureGP.jl:296-316) with the model's OWN kernels: region r is evaluated with the theta it was
 * fitted with.  After a plain pmk_model_fit the same bits as pmk_query_items(q, theta).  -3 if the model holds no kernels
 * (pmk_model_load before pmk_model_set_kernels).  Enqueues only. */
int  pmk_query_items_fitted(pmk_query *q);
/* pmk_query_items_multi with the model's own kernels */
int  pmk_query_items_multi_fitted(pmk_query *q, int want_var);
/* one-shot querymixtureGP! (mixtureGP.jl:159-294): pmk_predict_mixture / _multi without the th argument */
int  pmk_predict_mixture_fitted(pmk_model *m, const pmk_kernel_desc *weight_th, int64_t Nq, const double *Xq,
                                double radius, double delta, double *Yq, double *Vq);
int  pmk_predict_mixture_multi_fitted(pmk_model *m, const pmk_kernel_desc *weight_th, int64_t Nq, const double *Xq,
                                      double radius, double delta, double *Yq, int64_t ldyq, double *Vq);

/* ---- device-resident set-up: a model from a tree and ONE global point array -----------------------------------------
 * MixtureGPType(X_set, hps) after organizetrainingsets (partition.jl:301-357) or setuppartition (partition.jl:106-129)
 * without the host lists in between: the library assigns, gathers and packs on the GPU, and keeps the index list
 * (patch row -> global point) so that targets and the diagonal addend can be set from GLOBAL per-point arrays.  The
 * model is the one pmk_model_create_ex builds from the host-cut sets, bit for bit, for every later call.
 * Pointers marked "host or device" are classified by the runtime.  With a device pointer a call only enqueues on the
 * context's stream: the caller orders the producer of that array with the context's stream, either by putting the
 * context on the producer's stream (pmk_ctx_set_stream / pmk_ctx_set_stream_null) or by synchronising first.  With a host
 * pointer a call returns once the array has been read. */
/* X: host or device, point-major N x D with D = pmk_bsp_dim(bsp); y: host or device, N values, or NULL (targets zero
 * until a *_global setter runs).  eps >= 0: patch r is the eps-set of leaf leaf_base + r (the sets of pmk_bsp_assign, in
 * the same ascending order); eps < 0: patch r is the tree's own leaf list (needs N == pmk_bsp_num_points(bsp), else -3).
 * The model holds the leaves [leaf_base, leaf_base + P); P == 0: all leaves from leaf_base on.  Attaches the tree (no
 * pmk_model_set_bsp needed).  Blocks (the patch sizes come back to lay out the slabs).  -4: an empty patch (the text
 * names the leaf); -5: N or the number of (point, leaf) pairs does not fit 31 bits. */
int  pmk_model_create_from_bsp(pmk_ctx *ctx, const pmk_bsp *bsp, int64_t N, const double *X, const double *y, double eps,
                               int64_t leaf_base, int64_t P, int dtype, pmk_model **out);
/* the map from patch rows to global points: *N, offsets[P+1], inds[offsets[P]] (any pointer may be NULL); what the
 * per-patch leave-one-out values and weights are indexed by.  Blocks if inds is given.  This and the three setters
 * below return -3 on a model that was not made by pmk_model_create_from_bsp. */
int  pmk_model_patch_index(pmk_model *m, int64_t *N, int64_t *offsets, int64_t *inds);
/* pmk_model_set_targets through the index list: y holds the N targets of all points (host or device) */
int  pmk_model_set_targets_global(pmk_model *m, const double *y);
/* pmk_model_set_targets_multi through the index list: Y is N x R column-major with ldy >= N (host or device) */
int  pmk_model_set_targets_multi_global(pmk_model *m, int R, const double *Y, int64_t ldy);
/* pmk_model_set_diag through the index list: N addends (host or device); NULL clears the addend (and blocks) */
int  pmk_model_set_diag_global(pmk_model *m, const double *diag);
/* pmk_query_fetch / pmk_query_fetch_multi into DEVICE arrays: device-to-device copies enqueued on the context's stream,
 * no host synchronisation.  Same argument rules as the host forms (Vq_dev must be NULL after a mean-only items_multi). */
int  pmk_query_fetch_dev(pmk_query *q, double *Yq_dev, double *Vq_dev);
int  pmk_query_fetch_multi_dev(pmk_query *q, double *Yq_dev, int64_t ldyq, double *Vq_dev);

/* ---- gradient of the blended mean of the multi-output path (R columns, with or without a trend; fp64 and fp32 models) ---
 * For every stationary family grad_x k(x, z) = psi(tau) (x - z) with psi = phi'(tau) / tau, finite at tau = 0.  Per item
 * (query x, region r) and column c:  G[d + D c] = sum_k psi(|x - z_k|) (x_d - z_{k,d}) C_r[k, c], plus beta_r[1 + d, c]
 * with a linear trend (a constant trend adds nothing).  With w_i = phi_w(|t_i|) (home: w = 1), S = sum_i w_i and
 * Y_c = sum_i w_i u_{i,c} / S, in the item order of pmk_query_mix_multi:
 *   dY_c/dx_d = (1 / S) sum_i [ w_i G_{i,d,c} + (u_{i,c} - Y_c) dw_i/dx_d ],
 *   dw_i/dx_d = -psi_w(|t_i|) t_i v_{plane(i),d} for a neighbour (t = c - v . x of the hyperplane the plan accepted the
 *   item at), 0 for the home item.
 * This is the derivative with the ITEM LIST HELD FIXED.  Where the list changes the blend itself jumps -- at the radius
 * cut-off unless phi_w vanishes there, at a delta test, and where the home leaf changes -- and no derivative exists there.
 * A patch with info != 0, or tinfo != 0 under a trend, gives NaN in all D R values of its items and in every query that
 * blends one of them.  The gradient of the variance is the next section.  Not available through the sharded / all-gather
 * exchanges; the model must hold every leaf.  Stage timers "items_grad" and "mix_grad".  A new plan discards the gradients,
 * as it does the items. */
/* per-item gradients of the items that pmk_query_items_multi or _multi_fitted last computed on this plan.  th: the kernel
 * for every patch, or NULL for the model's own kernels (-3 if it holds none).  Enqueues only.  -1: no plan; -2: the last
 * items on this plan are not those of pmk_query_items_multi / _multi_fitted (none yet, or pmk_query_items_loo_multi, whose
 * member items are lookups and not functions of x), a Brownian-bridge family (not differentiable on the diagonal; the text
 * names the family), or PMK_MODSQEXP with D > 1; -3: the multi-output weights are stale (pmk_model_solve_multi has not run
 * on the resident factor: a new fit, pmk_model_set_targets_multi* and pmk_model_set_trend each make them stale). */
int  pmk_query_items_grad(pmk_query *q, const pmk_kernel_desc *th);
/* the gradient of the blend for queries [q0, q1), weight_th as in pmk_query_mix_multi (a Brownian-bridge weight kernel:
 * -2).  Enqueues.  -2 before pmk_query_items_grad has run on this plan. */
int  pmk_query_mix_grad(pmk_query *q, const pmk_kernel_desc *weight_th, int64_t q0, int64_t q1);
/* blocks; dYq[j + lddy * (d + D * c)] = dY_c/dx_d at query j, lddy >= Nq.  -2 before pmk_query_mix_grad. */
int  pmk_query_fetch_grad(pmk_query *q, double *dYq, int64_t lddy);
/* the same into a DEVICE array: device-to-device on the context's stream, no host synchronisation */
int  pmk_query_fetch_grad_dev(pmk_query *q, double *dYq_dev, int64_t lddy);
/* the per-item gradients G[i * ldg + d + D * c] (ldg >= D R) and the hyperplane of every item (plane[i]: the pre-order
 * index into hp_v / hp_c of pmk_bsp_arrays for a neighbour item, -1 for a home item and for every item of
 * pmk_query_create_items), items in the order of pmk_query_debug.  Either pointer may be NULL; G needs
 * pmk_query_items_grad (-2).  Blocks. */
int  pmk_query_get_items_grad(pmk_query *q, double *G, int64_t ldg, int32_t *plane);
/* one-shot: create + plan + mean-only pmk_query_items_multi_fitted + pmk_query_items_grad(NULL) + pmk_query_mix_multi +
 * pmk_query_mix_grad + both fetches; no strip kernel runs anywhere on this path.  Yq: Nq x R column-major, ldyq >= Nq
 * (may be NULL); dYq as in pmk_query_fetch_grad (may be NULL). */
int  pmk_predict_mixture_grad_fitted(pmk_model *m, const pmk_kernel_desc *weight_th, int64_t Nq, const double *Xq,
                                     double radius, double delta, double *Yq, int64_t ldyq, double *dYq, int64_t lddy);

/* ---- gradient of the blended variance of the multi-output path (with or without a trend; fp64 and fp32 models) ----------
 * Per item (query x, region r), with U_r = K + sigma2 I = L L^T, kq_k = phi(tau_k), g_{d,k} = psi(tau_k) (x_d - z_{k,d}),
 * V = L^-1 kq, W_d = L^-1 g_d and b = |V|^2: the simple-kriging variance is v_sk = max(k(x,x) - b, min_v), k(x,x) is
 * constant in x for every family admitted here, and
 *   d v_sk / dx_d = -2 V . W_d  where k(x,x) - b >= min_v,  exactly 0 where the clamp holds
 * (decided from the b of the gradient's own sweep).  With a trend of q basis functions v = v_sk + |z|^2, z = L_G^-1 rho,
 * rho_a = h_a(x) - (kq^T C_H)_a, and the trend adds
 *   2 z . (L_G^-1 d_d rho),  (d_d rho)_a = [a = 1 + d, linear trend only] - (g_d^T C_H)_a.
 * The blend is Vq = sum_i wn_i^2 v_i with wn_i = w_i / S (w, S and the item order as above); with the item list held fixed
 *   dVq/dx_d = sum_i [ wn_i^2 d_d v_i + 2 wn_i v_i d_d wn_i ],  d_d wn_i = (d_d w_i - wn_i sum_j d_d w_j) / S,
 * d_d w_i as in the gradient of the mean.  The same caveat holds: where the item list changes the blend jumps and has no
 * derivative.  An item's D values have the same bits whatever other items share its strip and wherever it sits in it.  A
 * patch with info != 0, or tinfo != 0 under a trend, gives NaN in all D values of its items and in every query that blends
 * one of them.  No route of this interface sets a query's min_v (it is 1e-12), so the clamp needs k(x,x) - b < 1e-12.
 * No sharded or all-gather form; the model must hold every leaf.  Stage timers "items_vgrad" and "mix_vgrad".  A new plan
 * or new items discard the results. */
/* per-item variance gradients of the items that pmk_query_items_multi or _multi_fitted last computed on this plan WITH
 * want_var = 1.  th: the kernel for every patch, or NULL for the model's own kernels (-3 if it holds none).  Enqueues only.
 * The refusals of pmk_query_items_grad, and -2 also after items with want_var = 0 and for a query that carries
 * pmk_query_set_diag addends (their dependence on x is unknown to the library); -3: stale multi-output weights. */
int  pmk_query_items_vgrad(pmk_query *q, const pmk_kernel_desc *th);
/* the gradient of the blended variance for queries [q0, q1), weight_th as in pmk_query_mix_grad.  Enqueues.  -2 before
 * pmk_query_items_vgrad has run on this plan. */
int  pmk_query_mix_vgrad(pmk_query *q, const pmk_kernel_desc *weight_th, int64_t q0, int64_t q1);
/* blocks; dVq[j + lddv * d] = dVq/dx_d at query j, lddv >= Nq.  -2 before pmk_query_mix_vgrad. */
int  pmk_query_fetch_vgrad(pmk_query *q, double *dVq, int64_t lddv);
/* the same into a DEVICE array: device-to-device on the context's stream, no host synchronisation */
int  pmk_query_fetch_vgrad_dev(pmk_query *q, double *dVq_dev, int64_t lddv);
/* the per-item gradients GV[i * ldg + d] (ldg >= D), items in the order of pmk_query_debug.  -2 before
 * pmk_query_items_vgrad.  Blocks. */
int  pmk_query_get_items_vgrad(pmk_query *q, double *GV, int64_t ldg);
/* one-shot: create + plan + pmk_query_items_multi_fitted with the variance + pmk_query_items_grad(NULL) +
 * pmk_query_items_vgrad(NULL) + pmk_query_mix_multi + pmk_query_mix_grad + pmk_query_mix_vgrad + the fetches.  Yq: Nq x R
 * column-major, ldyq >= Nq; Vq: Nq; dYq as in pmk_query_fetch_grad; dVq as in pmk_query_fetch_vgrad.  Any output pointer
 * may be NULL. */
int  pmk_predict_mixture_vgrad_fitted(pmk_model *m, const pmk_kernel_desc *weight_th, int64_t Nq, const double *Xq,
                                      double radius, double delta, double *Yq, int64_t ldyq, double *Vq, double *dYq,
                                      int64_t lddy, double *dVq, int64_t lddv);

/* ---- joint posterior covariance of a query batch under the blend (single-output path; fp64 and fp32 models) ---------------
 * The patches are independent GPs, so with V_{r,j} = L_r^-1 k_r(X_r, x_j) and wn the normalised weights of pmk_query_mix
 *   Cov[j, j'] = sum over the regions r that hold an item of BOTH j and j':
 *                wn_{r,j} wn_{r,j'} ( k_r(x_j, x_j') - V_{r,j} . V_{r,j'} ).
 * For j = j' this is Vq = sum wn^2 v.  Per region r with m_r items the stage computes the block
 *   S_r[a, b] = k_r(x_a, x_b) - V_a . V_b                                             for a != b (not clamped),
 *   S_r[a, a] = max( k_r(x_a, x_a) + the addend of pmk_query_set_diag - |V_a|^2, min_v ),
 * the rows being the region's items in ascending query index.  The neighbour search can accept one leaf through two
 * hyperplanes; such a query holds two items (two rows) of the region, every pair of items of j and j' in a common region
 * is a term of Cov[j, j'], and its diagonal entry carries the cross term that Vq does not.  Entry (a, b) of a block has the same bits whatever else is
 * in the batch; blocks and result are symmetric bit for bit and the same from run to run; queries that share no region
 * give exact zeros.  A patch with info != 0 gives NaN in its whole block and in the whole row and column of every query
 * that blends one of its items.  This is the single-output path: it ignores the trend, as pmk_query_items does, and does
 * not depend on targets; it needs a resident factor only, so models of pmk_model_load + pmk_model_set_kernels serve too.
 * Out of scope: a trend's term z . z' (here: pmk_query_items_cov_multi below adds it), the sharded and all-gather exchanges
 * (the model must hold every leaf), and fusing the means into the covariance sweep.  Every family is admitted (nothing here differentiates), PMK_MODSQEXP at D = 1 only.
 * Memory, owned by the query, grow only: sum over strips of ld x 256 elements of the model's type (a region's items are
 * dealt over ceil(m_r / 256) strips, ld the padded size of its patch), 8 sum m_r^2 bytes of blocks and 8 Nq^2 bytes of
 * result; a failed allocation returns -100 with the bytes asked for in the text.  Stage timers "items_cov" (sweep, Gram and
 * blocks) and "mix_cov".  A new plan discards the results.  At most PMK_COV_MAX_QUERIES queries a batch. */
/* the region blocks of the current plan.  th: the kernel for every patch, or NULL for the model's own kernels.  Enqueues.
 * Serves a query made by pmk_query_create_items too (the joint form of pmk_model_queryinner for a patch).  -1: no plan or
 * no resident factor; -2: unknown family, PMK_MODSQEXP with D > 1; -3: th NULL on a model that holds no kernels, or the
 * model does not hold every leaf; -5: Nq > PMK_COV_MAX_QUERIES. */
int  pmk_query_items_cov(pmk_query *q, const pmk_kernel_desc *th);
/* the blend of the whole batch, weight_th as in pmk_query_mix.  Enqueues.  -2 before pmk_query_items_cov has run on this
 * plan, and on a query made by pmk_query_create_items. */
int  pmk_query_mix_cov(pmk_query *q, const pmk_kernel_desc *weight_th);
/* blocks; Cov[j + ldc * j'], Nq x Nq column-major, ldc >= Nq.  -2 before pmk_query_mix_cov. */
int  pmk_query_fetch_cov(pmk_query *q, double *Cov, int64_t ldc);
/* the same into a DEVICE array: device-to-device on the context's stream, no host synchronisation */
int  pmk_query_fetch_cov_dev(pmk_query *q, double *Cov_dev, int64_t ldc);
/* the block of one global region: *m its item count, query[m] the query index of each row (ascending), S m x m
 * column-major with lds >= m.  Any pointer may be NULL, so a first call can size the buffers.  Blocks.  -2 before
 * pmk_query_items_cov; -3: the region is not one of the model's leaves. */
int  pmk_query_get_items_cov(pmk_query *q, int64_t region, int64_t *m, int32_t *query, double *S, int64_t lds);
/* one-shot: create + plan + pmk_query_items_fitted + pmk_query_mix + pmk_query_items_cov(NULL) + pmk_query_mix_cov + the
 * fetches.  Any output pointer may be NULL; with Cov NULL no covariance stage runs. */
int  pmk_predict_mixture_cov_fitted(pmk_model *m, const pmk_kernel_desc *weight_th, int64_t Nq, const double *Xq,
                                    double radius, double delta, double *Yq, double *Vq, double *Cov, int64_t ldc);

/* ---- the joint covariance on the multi-output path: under a trend, and for R target columns -------------------------------
 * A model solved with a trend (pmk_model_set_trend + pmk_model_solve_multi) predicts as a universal-kriging predictor, and
 * its joint covariance carries the drift's uncertainty: with H the basis of a patch, C_H = U^-1 H, G = H^T C_H = L_G L_G^T,
 *   S_r[a, b] = k_r(x_a, x_b) - V_a . V_b + z_a . z_b,   z = L_G^-1 rho,   rho = h(x) - C_H^T k_r(X_r, x),
 *   S_r[a, a] = max( k_r(x_a, x_a) + the addend of pmk_query_set_diag - |V_a|^2, min_v ) + |z_a|^2,
 * the trend's term after the clamp, as the item variance of pmk_query_items_multi has it: the diagonal of the blend is the
 * Vq of pmk_query_fetch_multi up to rounding (and the cross term of a query with two items of one region).  The blend is
 * that of pmk_query_mix_cov.  The covariance does not depend on the targets: the R columns are independent fields with a
 * common kernel and share it.  z comes from a = kq^T C_H, which pmk_query_items_multi leaves in the item rows, through the
 * operations of the item variance; z_a . z_b is one chain of fused multiply-adds in ascending basis index, added to the
 * entry with one addition, so the bit promises of pmk_query_items_cov hold here too.  A patch whose trend is flagged
 * (pmk_model_trend_info != 0) answers as one whose factorisation failed: NaN in its block and in the row and column of
 * every query that blends it.  Memory: 40 bytes per item and 4 bytes per patch on top of pmk_query_items_cov's, owned by
 * the query, grow only.  Out of scope: the sharded and all-gather exchanges, fusing the means into the sweep, and batches
 * above PMK_COV_MAX_QUERIES. */
/* the region blocks of the current plan on the multi-output path.  th: the kernel that was given to the items call, or NULL
 * for the model's own (the library does not compare the two).  Runs what pmk_query_items_cov runs and then, if the model's
 * trend has q > 0, the trend's term; with no trend in force the blocks are those of pmk_query_items_cov bit for bit.
 * Enqueues.  pmk_query_mix_cov, pmk_query_fetch_cov(_dev) and pmk_query_get_items_cov serve its results unchanged; new
 * items discard them.  Serves a query made by pmk_query_create_items too (the joint universal-kriging covariance of
 * explicit points against one patch).  Stage timer "cov_trend", inside "items_cov".  Before any launch: -1: no plan or no
 * resident factor; -2: the last items on this plan are not those of pmk_query_items_multi / _multi_fitted, or they were
 * computed under another trend (run the items again), or unknown family, PMK_MODSQEXP with D > 1; -3: the multi-output
 * weights are stale (pmk_model_solve_multi), th NULL on a model that holds no kernels, or the model does not hold every
 * leaf; -5: Nq > PMK_COV_MAX_QUERIES; -100: an allocation failed (the text gives the bytes asked for). */
int  pmk_query_items_cov_multi(pmk_query *q, const pmk_kernel_desc *th);
/* one-shot: create + plan + pmk_query_items_multi_fitted (variance iff Vq) + pmk_query_mix_multi +
 * pmk_query_items_cov_multi(NULL) + pmk_query_mix_cov + the fetches.  Yq is Nq x R column-major with ldyq >= Nq.  Any output
 * pointer may be NULL; with Cov NULL no covariance stage runs. */
int  pmk_predict_mixture_cov_multi_fitted(pmk_model *m, const pmk_kernel_desc *weight_th, int64_t Nq, const double *Xq,
                                          double radius, double delta, double *Yq, int64_t ldyq, double *Vq, double *Cov,
                                          int64_t ldc);

/* ---- block kriging: mean and kriging variance of weighted sums of the field over groups of queries --------------------
 * Query j belongs to group[j] in [0, F), NON-DECREASING in j (the queries of a group are contiguous; a group may have no
 * query), and carries the coefficient a[j] (any sign, zeros allowed).  With w_i = a_{j(i)} wn_i, wn the normalised weights
 * of pmk_query_mix, the items of one (region r, group f) pair, an aggregate -- a run of the sorted item list -- give
 *   kbar = sum_i w_i k_r(X_r, x_i),   Vbar = L_r^-1 kbar                       one column of the strip sweep
 *   kappa = sum_{i,i'} w_i w_i' k_r(x_i, x_i') + sum_i w_i^2 addend_{j(i)}      (pmk_query_set_diag)
 *   zbar = sum_i w_i z_i,  z_i = L_G^-1 (h(x_i) - C_H^T k_r(X_r, x_i))          under a trend with q > 0
 *   s_{r,f} = max(kappa - |Vbar|^2, min_v sum_i w_i^2) + |zbar|^2               the trend's term after the floor
 *   Vb[f] = sum_r s_{r,f}          Yb[f, c] = sum over the items i of f: w_i u_{i,c},  c < R
 * which is a^T Cov a and a^T Yq of pmk_query_items_cov_multi + pmk_query_mix_cov by bilinearity, the cross term of a query
 * that holds two items of one region included; a group of one query with a = 1 answers that query's Vq and Yq up to
 * rounding.  Nothing of size Nq^2 or m_r^2 is allocated and a group of g points costs one swept column per region it
 * touches, not g: the batch is not limited by PMK_COV_MAX_QUERIES.
 * Order of operations.  w_i = a_j (blend weight / weight sum).  An entry of kbar is one chain of fused multiply-adds from
 * 0 over the members in ascending sorted-item order, in the model's element type, so a column has the same bits whatever
 * shares its strip; |Vbar|^2 is summed as the strip kernel of pmk_query_items sums |V|^2.  kappa: lane l of a wave takes the
 * members i' = l, l + 64, .. and with each the members i <= i' (off-diagonal pairs twice), one chain; 64 partial sums meet
 * in a fixed butterfly.  Yb, zbar and |zbar|^2 are chains of fused multiply-adds from 0 in item, member and basis order;
 * Vb adds s at the first item of every aggregate, in item order.  A group's results depend on the group's queries alone.
 * A group that blends an item of a patch with info != 0 or a flagged trend is NaN in Yb and Vb, the others keep their bits;
 * an empty group answers 0 and +0.  Memory, owned by the query, grow only: 24 bytes per item, 12 per query, 56 per
 * aggregate, 8 (R + 2) per group; the strip workspace is the model's.  Stage timer "items_block".
 * Out of scope: the covariance between groups, non-contiguous groups, the sharded and all-gather exchanges, gradients of
 * block quantities. */
/* after pmk_query_items_multi / _multi_fitted on the current plan.  th: the kernel given to the items call, NULL for the
 * model's own; weight_th: the blending profile; group [Nq] and a [Nq]: host arrays; want_var = 0 runs the weights and the
 * mean reduction only.  Blocks (the aggregate count comes back to the host).  Before any launch: -1: no plan or no
 * resident factor; -2: the last items are not those of pmk_query_items_multi / _multi_fitted or were taken under another
 * trend, a query of explicit items, unknown family, PMK_MODSQEXP with D > 1, a Brownian-bridge blending profile; -3: the
 * multi-output weights are stale (pmk_model_solve_multi), th NULL on a model without kernels, the model does not hold
 * every leaf, or group decreases or leaves [0, F) (the text names the first offending j); -100: an allocation failed
 * (the text gives the bytes asked for).  After the aggregate list and before the sweep: -5: an aggregate of more than
 * PMK_BLOCK_MAX_MEMBERS items (the text names group and region).  New items and a new plan discard the results. */
int  pmk_query_items_block(pmk_query *q, const pmk_kernel_desc *th, const pmk_kernel_desc *weight_th, int64_t F,
                           const int32_t *group, const double *a, int want_var);
/* Yb: F x R column-major with ldyb >= F; Vb: F.  Either may be NULL.  -2: before pmk_query_items_block; -3: Vb after
 * want_var = 0; -4: ldyb < F.  _dev: device pointers, enqueues only. */
int  pmk_query_fetch_block(pmk_query *q, double *Yb, int64_t ldyb, double *Vb);
int  pmk_query_fetch_block_dev(pmk_query *q, double *Yb_dev, int64_t ldyb, double *Vb_dev);
/* blocks.  The aggregates in the order of the sorted items: n their number, and per aggregate the global region, the
 * group, the first sorted item, the member count, kappa, |Vbar|^2, |zbar|^2 and sum w^2.  Every pointer may be NULL (call
 * once for n).  -1: no plan; -2: pmk_query_items_block has not run with want_var = 1 on the current items. */
int  pmk_query_get_items_block(pmk_query *q, int64_t *n, int32_t *region, int32_t *group, int64_t *first, int32_t *count,
                               double *kappa, double *vnorm2, double *znorm2, double *sw2);
/* one-shot: create + plan + pmk_query_items_multi_fitted(0) + pmk_query_items_block(NULL, ..., Vb != NULL) + the fetch */
int  pmk_predict_mixture_block_fitted(pmk_model *m, const pmk_kernel_desc *weight_th, int64_t Nq, const double *Xq,
                                      double radius, double delta, int64_t F, const int32_t *group, const double *a,
                                      double *Yb, int64_t ldyb, double *Vb);

/* ---- posterior draws from the region blocks: no Nq x Nq covariance ---------------------------------------------------
 * The patches are independent GPs, so with S_r = L_r L_r^T the region blocks of pmk_query_items_cov(_multi),
 *   E_s(x_j) = sum over the items i of j:  wn_i (L_{r(i)} zeta_{r(i),s})[a(i)],   zeta independent standard normals,
 * is a zero-mean joint draw of the blend whose covariance is the entry pmk_query_mix_cov computes, the cross term of a
 * query that holds two items of one region included.  Cost: sum m_r^3 / 3 flop and 8 sum m_r^2 bytes instead of
 * Nq^3 / 3 and 16 Nq^2: the batch is limited by the items per region and by memory, not by PMK_COV_MAX_QUERIES.
 * Double only; serves fp64 and fp32 models (the blocks are doubles in both).  A region's factor is a function of its
 * block and its jitter alone: the same bits in every run, whatever other regions the batch holds.  Stage timers
 * "factor_cov" and "draw".  Memory, owned by the query object, grow only: the factors padded to tiles of 32 rows (about
 * 8 sum m_r^2 bytes), a total_items x (draw chunk) workspace of at most 256 MiB, 68 bytes per patch, 8 bytes per tile row,
 * and for host pointers a chunk of z and of E.  Out of scope: the sharded and all-gather exchanges, random numbers inside
 * the library, a one-shot call (the length of z depends on the plan). */
/* the block stage of pmk_query_items_cov (multi = 0) or pmk_query_items_cov_multi (multi != 0) without the refusal above
 * PMK_COV_MAX_QUERIES: the same checks, kernels and bits.  pmk_query_get_items_cov serves the blocks; pmk_query_mix_cov
 * refuses them with -5 on a batch above the limit. */
int  pmk_query_items_cov_blocks(pmk_query *q, const pmk_kernel_desc *th, int multi);
/* enqueues the Cholesky factorisation of every region block of the current plan into a second buffer (the blocks stay):
 * block r is factored as S_r + rel[r] (trace S_r / m_r) I, the trace summed in one fixed order.  rel: P host values, NULL
 * for zeros.  A region that an earlier call on the same blocks factored (status 0) with the same rel[r] is not factored
 * again and keeps its bits: a retry costs the regions that failed.  New blocks, new items under a trend and a new plan
 * discard the factors.  Serves a query made by pmk_query_create_items too.  -1: no plan; -2: no blocks on this plan, or
 * a negative or non-finite rel[r]; -100: an allocation failed (the text gives the bytes asked for). */
int  pmk_query_factor_cov(pmk_query *q, const double *rel);
/* blocks.  finfo[r]: 0 the block was factored (or is empty); k in 1 .. m_r: pivot k is NaN or <= 0 to rounding, that is
 * not above 2^-50 (S_kk + jitter), what two copies of one item leave (the leading-minor convention of pmk_model_info),
 * the factor of that region is unusable; -1: the patch is failed or its trend is flagged
 * (what pmk_query_mix_cov reads as bad), the block was not factored.  jitter[r]: the absolute value added to the
 * diagonal.  P entries each, either may be NULL.  Returns 1 if any finfo is non-zero, else 0; -1: no plan; -2: before
 * pmk_query_factor_cov. */
int  pmk_query_factor_info(pmk_query *q, int32_t *finfo, double *jitter);
/* blocks; L_r, m x m column-major with ldl >= m, the strict upper triangle zero; rows in the order of
 * pmk_query_get_items_cov.  m and L may be NULL.  Refusals as pmk_query_get_items_cov, and -2 before a factorisation. */
int  pmk_query_get_items_cov_factor(pmk_query *q, int64_t region, int64_t *m, double *L, int64_t ldl);
/* E[j + lde s] = the zero-mean part of draw s at query j (the caller adds Yq; for R target columns, column c to draws
 * made from independent z), s < n_draws, lde >= Nq.  z[p + ldz s]: the normal of the sorted item at position p (region r
 * owns the positions roff[r] .. roff[r + 1] - 1 of pmk_query_region_offsets, in the row order of pmk_query_get_items_cov),
 * ldz >= total_items.  z and E are host or device pointers, classified by the runtime as pmk_query_create classifies Xq:
 * with device pointers the call only enqueues, with a host pointer it blocks.  The sum over a query's items is one chain
 * of fused multiply-adds in the item order and with the weights of pmk_query_mix.  A query that blends an item of a region
 * with finfo != 0 is NaN in every draw; the others keep their bits.  n_draws = 0 returns 0.  -1: no plan; -2: before
 * pmk_query_factor_cov, a query of explicit items, a Brownian-bridge or unknown weight kernel, z or E NULL; -4: a leading
 * dimension is too small; -100: an allocation failed (the text gives the bytes asked for). */
int  pmk_query_draw(pmk_query *q, const pmk_kernel_desc *weight_th, int64_t n_draws, const double *z, int64_t ldz, double *E,
                    int64_t lde);

/* ---- appending observations to a fitted model in place: the border of the Cholesky factor ---------------------------
 * A patch's buffers are laid out for ld_r = 128 ceil(n_r / 128) rows, so up to ld_r - n_r new points fit without moving
 * anything.  For the m new points Xn of a patch with resident factor L:
 *   L' = [ L 0 ; L21 L22 ],  L21^T = V = L^-1 k_r(X, Xn),  L22 L22^T = k_r(Xn, Xn) + sigma2_r I (+ addends) - V^T V,
 *   z' = [ z ; L22^-1 (yn - L21 z) ],  c' = L'^-T z',
 * with the patch's own theta_r and sigma2_r.  V and V^T V come from the covariance sweep of pmk_query_items_cov (its
 * kernels as they are, no variance floor on the diagonal), the border from one workgroup per receiving patch, c from the
 * back substitution of the fit, run over every patch (one launch whatever received points; the split path has no other
 * form).  Rows and columns < n_r of L, z and the -D^-1 blocks that do not meet the new rows keep their bits; c changes in
 * every row.  Both precisions; works on a model on the split path.  Memory, owned by the model, grow only, freed with it:
 * one ld_r x 256 strip of the model's type per receiving patch, 8 sum m_r^2 bytes of blocks and the staged items; a failed
 * allocation returns -100 with the bytes asked for in the text.  Stage timers "append_sweep", "append_border" and
 * "append_solve".
 * With rows reserved (pmk_model_reserve below) ld_r is larger than 128 ceil(n_r / 128) and the new rows may run on into
 * the block rows laid out past the patch's last one: everything from 128 nt_r up to ld_r is identity padding, so entering
 * a block row is the new entries, the -D^-1 blocks of the whole block row entered, and nt_r' = ceil((n_r + m_r) / 128)
 * written beside n_r + m_r.  The host then follows with what depends on tile counts: max_nt, the factorisation order
 * (stable, largest first, as at creation), its active prefix, the leave-one-out tasks and the strip workspace.  The split
 * mode stays as chosen at creation.  The arithmetic on a patch that stays inside its last block row is what it was.
 * Where the new rows raise max_nt the longer strip workspace is allocated before anything is launched (-100, nothing
 * changed, if that fails) and put in place together with max_nt; the host flags of "After the call" below are reset
 * before the tile counts are followed.
 * Out of scope: device-resident x / y arguments, the sharded exchanges, and the leaf lists of the tree itself
 * (pmk_bsp_arrays still describes the points it was built on). */
/* free_rows[P]: ld_r - n_r, the points patch r can still take */
int  pmk_model_capacity(pmk_model *m, int64_t *free_rows);
/* Room to grow: after the call every patch r has pmk_model_capacity >= rows[r] (host array of P entries).  A patch has
 * nt_r = ceil(n_r / 128) active block rows and a stride ld_r = 128 nt_cap_r >= 128 nt_r; a model that was never given a
 * reserve has nt_cap_r = nt_r and behaves as it always did.  Invariant, kept by everything that runs on a model: the rows
 * and columns of a patch's buffers from 128 nt_r up to ld_r are in the state a fit leaves in padding -- identity in the
 * slab, 1e300 coordinates, zeros in y, z, c and the addends, -I in the -D^-1 blocks (which are laid out for nt_cap_r block
 * rows) -- and only this call and pmk_model_append write there.  The fit, the solves and every sweep work on nt_r block
 * rows whatever the stride.
 * A patch that has the room keeps its ld_r, none is ever shrunk, and a call that has nothing to grow does nothing.
 * Otherwise the whole new layout (slabs, coordinates, y, z, c, addends if set, -D^-1 blocks, descriptors) is allocated
 * beside the old one, written completely by the kernels of pmk_reserve.hip (the active part copied, the rest padding;
 * 16-byte accesses along the columns), swapped in, and the old one is freed; the offsets and the chunk prefix of the
 * *_global setters follow.  Blocks.  Works before and after a fit, in both precisions: a fitted model keeps L, z, c, the
 * -D^-1 blocks, info, the hyperparameters, the tree, the index list and N bit for bit.  As after an append the
 * leave-one-out values, the multi-output targets and the trend state have to be set again.  Query objects created
 * earlier keep their plan (every launch reads the model's buffers through the model); their results are stale.
 * Memory: both layouts exist side by side during the call.  Stage timer "reserve".
 * -1 NULL argument; -2 a negative entry; -3 the model factors on the split path (its solves read ld_r as the extent;
 * pmk_test_model_set_split refuses a model that holds reserved rows for the same reason); -4 n_r + rows[r] above 2^24,
 * the limit at creation; -100 an allocation failed: the model is exactly as it was.
 * Out of scope: shrinking, the split path, removal out of the last block row (pmk_model_remove keeps its band rule: a
 * patch that entered a block row with one point cannot lose that point). */
int  pmk_model_reserve(pmk_model *m, const int64_t *rows);
/* n_items items (point, target, patch): x host, point-major n_items x D; y host; diag host addends of the kernel's
 * diagonal, or NULL (zeros; -2 if given for a model without pmk_model_set_diag addends); patch[i] the local patch of
 * item i.  The items of one patch become its rows n_r, n_r + 1, ... in the order given; a point of several patches is
 * several items.  global_index[i], the global point of item i, is required on a model of pmk_model_create_from_bsp and
 * must be NULL otherwise; it is at least the model's N (a new observation is a new global point), occurs once per
 * patch, and the indices of one patch strictly ascend in the order given (the rows follow that order and a patch's index
 * list is searched by bisection, so the call does not sort: it refuses): N grows to 1 + the largest index, the index list is rebuilt (one host round trip), and the
 * *_global setters then expect the new N.  Blocks while the items are staged, then enqueues.
 * A pivot of L22 that is <= 0 or NaN at new row a sets info[r] = n_r + a + 1 (the leading-minor convention of the fit);
 * the patch is then failed as after a failed fit, until the next fit, and no other patch is touched by it.  A patch that
 * had failed before takes its points, targets and n and stays failed.
 * After the call: leave-one-out values are stale (pmk_model_loo again), the multi-output targets and the trend state are
 * discarded (pmk_model_set_targets_multi again, with n_r + m_r rows, before pmk_model_solve_multi).  The geometry (nt, ld,
 * offsets, schedule, split mode) is unchanged unless reserved block rows are entered (above).  Query objects created earlier keep their plan; their item, gradient and
 * covariance results are stale and nothing tracks that: run the item stages again.
 * Refused before any device work, nothing changed: -1 model NULL, not fitted, or built by pmk_model_load (it holds no
 * targets); -2 NULL arrays, global_index given or missing against the model's kind, diag without addends in the model;
 * -3 a patch index out of range, a global index below N or beyond 2^31-3, one given twice for a patch, or the indices of a patch
 * not ascending in the order given (the text names the patch and the index); -4 a patch's
 * capacity exceeded (the text names the patch, its free rows and the rows asked for); -5 more than PMK_COV_MAX_QUERIES items, or more than 128 for one patch (S is factored in an LDS image of 128 x 129; the text names the patch); -6 a non-finite coordinate, target or addend.
 * n_items = 0 returns 0 and touches nothing. */
int  pmk_model_append(pmk_model *m, int64_t n_items, const double *x, const double *y, const double *diag,
                      const int32_t *patch, const int64_t *global_index);

/* ---- removing observations from a fitted model in place: row deletion from the Cholesky factor ------------------------
 * The mirror of the append.  The rows r_1 < ... < r_m of a patch with resident L, z = L^-1 y leave; k0 = r_1, n' = n - m.
 * L~ = L[keep, :] (n' x n) has L~ L~^T = U[keep, keep] and L~ z = y[keep], and its first k0 rows are lower triangular
 * already.  New row j of the trailing block B = L[keep >= k0, k0 : n] is the old row k0 + j + s_j (s_j removed rows before
 * it, 1 <= s_j <= m, non-decreasing) and ends at column j + s_j.  One Householder reflector per new column, of s_j + 1
 * entries, made from row j without cancellation, the column's sign then flipped so that the diagonal is +|x|, is applied
 * to the rows below and to z^T[k0:]:  B Q = [L'_22 0],  z' = [ z[:k0] ; (Q^T z[k0:])[:n' - k0] ],  c' = L'^-T z'.
 * The Cholesky factor is unique, so L' is the factor of the reduced matrix, with the patch's own theta_r and sigma2_r and
 * its addends; a new diagonal is at least the old one.  One workgroup per patch that loses rows (pmk_remove.hip) moves the
 * rows of the slab, the coordinates, the targets and the addends up, sweeps the trailing block in blocks of 32 columns
 * staged in LDS, restores the padding of the rows and columns n' .. n - 1 as a fit leaves it, inverts anew the 32 x 32
 * -D^-1 blocks from k0 / 32 on and writes n' last; c comes from the back substitution of the fit, run over every patch as
 * the append runs it.  Rows and columns < k0 of L, z below k0 and the -D^-1 blocks before k0 / 32 keep their bits, and so
 * do the moved rows left of column k0; removing only the last rows transforms nothing.  Both precisions; works on a model
 * on the split path.  Memory: the row list of the call, grow only, freed with the model.  Stage timers "remove_rows" and
 * "remove_solve".
 * Band rule: nt_r and ld_r are fixed, as for the append, so a patch stays in its last block row:
 * n'_r >= 128 (nt_r - 1) + 1.  One call removes at most PMK_REMOVE_MAX_ROWS rows from one patch (the reflectors of a
 * column block are staged in LDS); more rows take more calls.
 * Out of scope: leaving the last block row in either direction, device-resident arguments, the sharded exchanges, the leaf
 * lists of the tree itself (pmk_bsp_arrays still describes the points it was built on), renumbering global indices. */
/* rows[P]: n_r - 128 (nt_r - 1) - 1, the rows patch r can still lose */
int  pmk_model_removable(pmk_model *m, int64_t *rows);
/* n_items (patch, row) pairs, host arrays, in any order: row[i] is a row index of patch[i] as it stands BEFORE the call;
 * the rows that stay keep their order.  On a model of pmk_model_create_from_bsp the entries leave the index list (rebuilt
 * by one host round trip, prepared before any launch and put in place after); N does not change, the *_global setters
 * still take N values, and a removed point's value is read by nobody.  The lists stay ascending.  Blocks while the row
 * list is staged, then enqueues.
 * A new diagonal that is <= 0 or NaN at new row a sets info[r] = a + 1 if info[r] was 0 (the leading-minor convention of
 * the fit); the patch is then failed as after a failed fit and no other patch is touched by it.  A patch that had failed
 * before loses its points, targets and n and stays failed (an info above n'_r becomes n'_r: it names a leading minor).
 * After the call: leave-one-out values are stale (pmk_model_loo again), the multi-output targets and the trend state are
 * discarded (pmk_model_set_targets_multi again, with n'_r rows).  The geometry (nt, ld, offsets, schedule, split mode) is
 * unchanged.  Query objects created earlier keep their plan; their item, gradient and covariance results are stale and
 * nothing tracks that: run the item stages again.
 * Refused before any device work, nothing changed: -1 model NULL, not fitted, or built by pmk_model_load; -2 NULL arrays
 * or n_items < 0; -3 a patch or row out of range, or a (patch, row) given twice (the text names the item); -4 a patch
 * would fall below 128 (nt - 1) + 1 rows (the text names the patch, its removable rows and the rows asked for); -5 more
 * than PMK_REMOVE_MAX_ROWS rows of one patch.  n_items = 0 returns 0 and touches nothing. */
int  pmk_model_remove(pmk_model *m, int64_t n_items, const int32_t *patch, const int64_t *row);

/* query!(Yq, Xq, eta)  src/RKHS/RKHS.jl:220-247 : mean only, Yq = K(Xq, X) c */
int  pmk_query_mean(pmk_ctx *ctx, const pmk_kernel_desc *th, int D, int64_t n, const double *X,
                    const double *c, int64_t Nq, const double *Xq, double *Yq);
/* query!(Yq, Xq, eta::RKHSProblemType{Vector{KT}})  RKHS.jl:278-305 : one kernel per centre, ths[n] */
int  pmk_query_mean_multi(pmk_ctx *ctx, const pmk_kernel_desc *ths, int D, int64_t n, const double *X,
                          const double *c, int64_t Nq, const double *Xq, double *Yq);

#ifdef __cplusplus
}
#endif
#endif
