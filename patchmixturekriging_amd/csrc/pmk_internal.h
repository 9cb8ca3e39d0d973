// Internal declarations shared by the host side and the HIP kernels of libpmk_hip.so.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/pmk.h"

namespace pmk {

constexpr int TILE = 128;       // factorisation tile edge; slabs are padded to a multiple of it
constexpr int MAX_D = 4;        // input dimension limit (the reference's examples use 1, 2 and 3)
constexpr int TQ = 256;         // query columns per prediction strip (8 waves x 32)
// layout of the per-patch trend state and of the multi-output blocks, shared by pmk_trend.hip and pmk_loo_mix.hip
constexpr int TQ_MAX = 1 + MAX_D;             // basis functions of the linear trend at D = 4; leading dimension of L_G
constexpr int TR_RP = PMK_MAX_OUTPUTS;        // columns of a row of the target / weight block
// items of a strip of the variance-gradient sweep (pmk_vgrad.hip): an item takes D + 1 of the 16 lanes of a row, a lane
// holds two columns, a strip eight waves: 128 / 80 / 64 / 48 at D = 1 / 2 / 3 / 4
constexpr int vgrad_strip_items(int D) { return 8 * 2 * (16 / (D + 1)); }

// Can the buffer-load form of the wave-tile GEMM (pmk_mfma.h: gemm_nt_buf) address an operand of K columns with leading
// dimension ld?  Its offsets are 32-bit and signed, and the scalar column offset runs up to pfj k-steps (4 pfj columns)
// past K before the loop ends.  Where this does not hold (single problems with slabs of 2 GiB and more) the caller
// takes gemm_nt.
constexpr bool gemm_buf_extent_ok(int64_t K, int64_t ld, int pfj, int elem_size)
{
    return K > 0 && ld > 0 && pfj > 0 && elem_size > 0 &&
           (K + 4 * (int64_t)pfj) <= (((int64_t)1 << 31) - 1) / (ld * (int64_t)elem_size);
}

// Loop form of the step kernel's GEMMs (pmk_chol.hip: block-row product and look-ahead), one per launch.
constexpr int STEP_GEMM_PTR = 0;        // gemm_nt
constexpr int STEP_GEMM_BUF = 1;        // gemm_nt_buf
// The rule of PMK_STEP_GEMM=auto for the step launch that has G block rows below the diagonal and whose largest patches
// are at block column k, for the element type and the fused / unfused kernel-matrix build: a function of these four
// alone -- not of the number of patches or of their tile count.
//   fused build  -> buffer form in every launch,   unfused build -> pointer form.
// Measured per launch, 5 runs an arm against the parent build, alternating (profiles/step_gemm_forms.txt): with the
// fused build the buffer form everywhere takes 1-3 % off the launches that the deep product dominates and 3-4 % off the
// last two -- step launches 13.06-13.26 -> 12.87-12.95 ms at 16 tiles fp64, 7.24-7.28 -> 6.99-7.07 ms in fp32,
// 3.86-3.91 -> 3.78-3.83 ms at 10 tiles, neutral at 24 tiles (22.17-22.28 -> 22.02-22.29 ms).  Where the tiles are
// loaded instead of evaluated it loses (12.64-12.68 -> 12.70-12.76 ms).  Single launches move by 80-130 us with the form
// in either direction and not reproducibly from box to box, so the rule does not follow single launches; G and k are
// arguments because the choice is made per launch, and today the answer is the same for all of them.
constexpr int step_gemm_rule(int G, int k, bool f32, bool fused)
{
    return (void)G, (void)k, (void)f32, fused ? STEP_GEMM_BUF : STEP_GEMM_PTR;
}

void set_error(const char *fmt, ...);

#define PMK_HIP(expr)                                                                        \
    do {                                                                                     \
        hipError_t e__ = (expr);                                                             \
        if (e__ != hipSuccess) {                                                             \
            pmk::set_error("%s failed at %s:%d: %s", #expr, __FILE__, __LINE__,              \
                           hipGetErrorString(e__));                                          \
            return -100;                                                                     \
        }                                                                                    \
    } while (0)

// Per-patch geometry, resident on the device (one entry per patch).
struct PatchDesc {
    int32_t n;        // points in the patch
    int32_t nt;       // ceil(n / TILE)
    int32_t ld;       // leading dimension of the slab, a multiple of TILE, >= nt * TILE (more after pmk_model_reserve);
                      // rows and columns from nt * TILE on are identity and no kernel reads them as part of the patch
    int32_t pad_;
    int64_t aoff;     // element offset of the ld x ld slab (K, then L in place)
    int64_t xoff;     // element offset of the SoA coordinates: x[d][ld]
    int64_t yoff;     // element offset into y / z / c (ld each)
    int64_t ioff;     // element offset of the negated inverted 32 x 32 diagonal blocks: (ld / TILE) x 4 x (32 x 32)
};

// Hyperparameter arguments of the kernels that evaluate theta (K1, the prediction strips, the multi-output means).  The
// uniform instantiations (PP = false) take one descriptor and one noise variance by value; the per-patch ones
// (PP = true) take the model's device arrays, indexed by the local patch.
template <bool PP> struct HyperArgs { using th_t = pmk_kernel_desc; using s2_t = double; };
template <> struct HyperArgs<true> {
    // restrict: nothing the kernels write aliases the arrays, so a patch's descriptor is a scalar load into scalar registers
    using th_t = const pmk_kernel_desc *__restrict__;
    using s2_t = const double *__restrict__;
};

// A strip of the covariance sweep (pmk_cov.hip): up to TQ sorted items of one region and their strip of the V arena.
// Built on the host from the plan's region offsets (pmk_api_query.cpp), dealt over a region's strips as
// build_strip_tasks deals them.
struct CovTask {
    int32_t region;   // local patch
    int32_t count;    // items of the strip (<= TQ)
    int64_t first;    // first sorted item of the strip
    int64_t voff;     // element offset of the strip in the V arena: ld x TQ elements, leading dimension TQ
    int64_t goff;     // element offset of the region's m x m block in the block buffer
    int32_t m;        // items of the region
    int32_t a0;       // position of `first` in the region's sorted segment
};
struct CovPair { int32_t ta, tb; };   // two strips of one region, ta <= tb

// Block kriging (pmk_block.hip).  An aggregate: the sorted items [first, first + count) of one region that belong to one
// group of queries, built on the device.  A task: up to TQ consecutive aggregates of one region, dealt over the region's
// strips as build_strip_tasks deals items, built on the host from the regions' first aggregates.
struct BlockAgg {
    int32_t region;   // local patch
    int32_t group;    // the queries' group
    int64_t first;    // first sorted item
    int32_t count;    // members (<= PMK_BLOCK_MAX_MEMBERS)
    int32_t pad_;
};
struct BlockTask {
    int32_t region;   // local patch
    int32_t count;    // aggregates of the strip (<= TQ)
    int64_t first;    // first aggregate of the strip
};

// A region block and its Cholesky factor (pmk_draw.hip).  The factor is padded to nt tiles of DRAW_TILE rows, column-major
// with leading dimension DRAW_TILE nt, the identity in the padding.  Built on the host from the plan's region offsets.
constexpr int DRAW_TILE = 32;
struct DrawRegion {
    int64_t soff;     // element offset of the m x m block S_r in the block buffer (cov_goff)
    int64_t foff;     // element offset of the padded factor in the factor buffer
    int64_t p0;       // first sorted item of the region
    int32_t m;        // items of the region
    int32_t nt;       // tiles: ceil(m / DRAW_TILE)
};
struct DrawTask { int32_t region, tile; };   // a tile row of a region's factor

// A patch that loses rows (pmk_remove.hip): its rows are rows[first .. first + count), ascending.
struct RemoveTask {
    int32_t region;   // local patch
    int32_t count;    // rows removed (<= PMK_REMOVE_MAX_ROWS)
    int64_t first;    // first entry of the patch in the row list
};

// A BSP tree in heap order (root 0, children 2i+1 / 2i+2); leaves numbered left to right.
struct BspArrays {
    int D = 0, levels = 0;
    int dot_mode = 0;               // 0: v . x as separate multiplies and adds, 1: as a chain of fused multiply-adds
    int64_t P = 0, N = 0;
    std::vector<double> v;          // (P-1) x D heap order
    std::vector<double> c;          // P-1
    std::vector<int64_t> pre;       // pre-order rank -> heap index
    std::vector<int64_t> leaf_off;  // P+1
    std::vector<int64_t> leaf_inds; // N
};

}  // namespace pmk

struct pmk_bsp {
    pmk::BspArrays t;
};

struct pmk_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    int timers = 0;                 // 0 off, 1 per stage, 2 also per panel launch
    struct Timer { std::string name; hipEvent_t a, b; bool valid; };
    std::vector<Timer> tm;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> panel_ev;   // one pair per panel launch of the last fit
    int panel_n = 0;
    int num_cu = 0;                 // compute units of the device (sizes the persistent prediction grid)
    // shader-clock probe: workgroups 0..7 (one per XCD) of every factorisation step launch and of the prediction strip
    // kernel leave (shader cycles, 100 MHz ticks) of their own lifetime here: block x of 130 pairs for XCD slot x:
    // [2 l], [2 l + 1] for step launch l < 64, [128], [129] for the strip kernel.  The roofline's peak assumes the
    // nominal clock; this says what the kernels actually got (every XCD has its own clock).
    unsigned long long *d_clk = nullptr;
    void tic(const char *name);
    void toc(const char *name);
};

struct pmk_model {
    pmk_ctx *ctx = nullptr;
    int D = 0;
    int64_t P = 0;
    int max_nt = 0;
    std::vector<pmk::PatchDesc> desc;   // host copy
    pmk::PatchDesc *d_desc = nullptr;
    int dtype = PMK_F64;                // arithmetic type of the device path (element type of the buffers below)
    size_t esz = 8;
    void *d_x = nullptr;                // SoA coordinates
    void *d_y = nullptr;                // targets (padded with 0)
    void *d_diag = nullptr;             // per-point addend of the kernel's diagonal (pmk_model_set_diag), or null
    void *d_z = nullptr;                // L^-1 y
    void *d_c = nullptr;                // weights
    void *d_a = nullptr;                // slabs
    void *d_inv = nullptr;              // -(L[ss])^-1 for every 32 x 32 diagonal block of L
    int32_t *d_info = nullptr;          // per patch
    // factorisation schedule: patches sorted by tile count (largest first) and, for every threshold t, how many
    // patches have nt >= t (the active prefix of `order` at launch max_nt - t of the end-aligned schedule)
    int32_t *d_order = nullptr;
    std::vector<int32_t> active_prefix;
    // split path (few, large patches: the deep products of a step are cut along K over several workgroups and the two
    // triangular solves run block by block over many workgroups): chosen at creation from P and the tile counts
    bool split_mode = false;
    int step_gemm = -1;                 // loop form of the step kernel's GEMMs: -1 by rule (step_gemm_rule), else STEP_GEMM_* forced in every launch
    bool fuse_k1 = false;               // this fit evaluates the strictly lower kernel-matrix tiles inside the factorisation
    void *d_partial = nullptr; size_t partial_bytes = 0;      // partial product tiles of one step
    void *d_solve_part = nullptr; size_t solve_bytes = 0;     // partial matrix-vector products of one solve block
    void *d_chain = nullptr; size_t chain_words = 0;          // solve_chain_kernel: error word, then one flag word per block and direction
    int chain_epoch = 0; bool chain_used = false;             // the flags hold the epoch of the launch that set them
    int chain_mode = -1;                                      // -1: by size, 0: block-by-block solves, 1: chained solves (pmk_test.h)
    int64_t tot_a = 0, tot_x = 0, tot_y = 0, tot_inv = 0;
    bool fitted = false;
    pmk_kernel_desc th{};
    double sigma2 = 0;
    // the hyperparameters the resident factor belongs to, per local patch.  ths is empty while the model holds no kernels
    // (pmk_model_load before pmk_model_set_kernels).  hyper_uniform: a plain pmk_model_fit left P copies of (th, sigma2) and
    // the *_fitted calls run the uniform kernels with m->th; otherwise they run the per-patch instantiations on the device
    // copies below (written by pmk_model_fit_patches / pmk_model_set_kernels only).  hyper_s34: every patch is Spline34.
    std::vector<pmk_kernel_desc> ths;
    std::vector<double> sigma2s;
    bool hyper_uniform = false, hyper_s34 = false;
    pmk_kernel_desc *d_ths = nullptr;
    double *d_sigma2s = nullptr;
    // BSP for prediction (heap order on device)
    int levels = 0;
    int64_t P_global = 0, leaf_base = 0;
    int dot_mode = 0;
    double *d_hv = nullptr, *d_hc = nullptr;   // heap order
    int32_t *d_pre = nullptr;                  // pre-order -> heap
    // prediction strip workspace
    void *d_strip = nullptr;
    int64_t strip_slots = 0;
    // multi-output targets (pmk_model_set_targets_multi): R columns per patch in row-major tot_y x PMK_MAX_OUTPUTS blocks
    // (pmk_multi.hip), columns >= R and padding rows zero; C = (L L^T)^-1 Y once pmk_model_solve_multi has run
    int R_multi = 0;
    void *d_ym = nullptr;               // targets Y
    void *d_cm = nullptr;               // weights C (the forward solve's Z in between)
    bool multi_solved = false;
    // trend of the multi-output path (pmk_trend.hip): the degree asked for, the q the resident weights were solved with,
    // whether columns >= R of the target block still hold an earlier solve's basis, and the per-patch GLS state (double)
    int trend_degree = PMK_TREND_NONE;
    int trend_q = 0;
    bool trend_cols_dirty = false;
    double *d_tbeta = nullptr, *d_tL = nullptr, *d_tG = nullptr;   // P x 80, P x 25, P x 25 (layouts in pmk_trend.hip)
    int32_t *d_tinfo = nullptr;                                    // P
    // model selection from the resident factor (pmk_loo.hip): d = diag((L L^T)^-1), always double, yoff addressing;
    // valid from pmk_model_loo until the next pmk_model_fit.  The strip tasks depend on the geometry only: built once.
    double *d_dloo = nullptr;
    bool loo_valid = false;
    bool loaded = false;                // built by pmk_model_load: d_y holds no targets
    void *d_loo_tasks = nullptr;        // LooTask list, grouped by queue (one queue per XCD)
    uint32_t *d_loo_cnt = nullptr;      // 8 queue heads
    int64_t loo_ntasks = 0;
    int32_t loo_qoff[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    // built by pmk_model_create_from_bsp (pmk_gather.hip): row i of patch r is the global point d_pidx[pidx_off[r] + i].
    // The *_global setters gather through this list; the chunk prefix (one entry per 256 slab rows of a patch) is the
    // grid of the gather kernels.
    bool from_bsp = false;
    int64_t N_global = 0;
    std::vector<int64_t> pidx_off;      // P + 1 (host copy)
    int64_t *d_pidx_off = nullptr;      // P + 1
    int32_t *d_pidx = nullptr;          // pidx_off[P]
    int32_t *d_gchunk = nullptr;        // P + 1: prefix over ceil(ld_r / 256)
    int64_t gchunks = 0;
    double *d_gstage = nullptr; size_t gstage_bytes = 0;   // device copy of a host array handed to a *_global setter (grow only)
    // pmk_model_append (pmk_api_append.cpp, pmk_append.hip).  append_q is no query of the ABI: it carries the arguments
    // of launch_items_cov (tasks, pairs, V arena, blocks, points, addends, no variance floor) for the appended items,
    // grouped by patch, with the identity as item order (d_app_iota).  All buffers grow only and go with the model.
    pmk_query *append_q = nullptr;
    double *d_app_y = nullptr, *d_app_diag = nullptr;      // targets and addends of the staged items
    int32_t *d_app_iota = nullptr;
    int64_t app_x_cap = 0, app_qdiag_cap = 0, app_y_cap = 0, app_diag_cap = 0, app_iota_cap = 0;
    // pmk_model_remove (pmk_api_remove.cpp, pmk_remove.hip): the tasks and the row list of one call; grow only
    pmk::RemoveTask *d_rm_tasks = nullptr;
    int32_t *d_rm_rows = nullptr;
    int64_t rm_tasks_cap = 0, rm_rows_cap = 0;
};

struct pmk_query {
    pmk_model *m = nullptr;
    int64_t Nq = 0;
    int64_t nq_cap = 0;             // capacity of the per-point buffers below (grow only)
    int *d_flag = nullptr;          // device scratch flag (region range check of explicit items)
    double *d_xq = nullptr;         // point-major D x Nq
    double *d_qdiag = nullptr;      // per-query addend of k(xq, xq) (pmk_query_set_diag), or null
    int32_t *d_home = nullptr;      // Nq
    int32_t *d_cnt = nullptr;       // Nq : items per query (neighbours + 1)
    int32_t *d_stage_r = nullptr;   // PLAN_STAGE x nq_cap : first neighbour hits of the count pass (region), see plan_kernel
    double *d_stage_t = nullptr;    //                        ... and their t
    int32_t *d_stage_p = nullptr;   //                        ... and their hyperplane (pre-order index)
    int64_t *d_qoff = nullptr;      // Nq+1
    int64_t total = 0;
    int64_t item_cap = 0;           // capacity of the per-item buffers (reused across plans)
    int32_t *d_item_region = nullptr;   // total, reference order
    double *d_item_t = nullptr;         // total (0 for home)
    int32_t *d_item_query = nullptr;    // total
    int32_t *d_sorted_item = nullptr;   // total: sorted position -> item
    int32_t *d_item_pos = nullptr;      // total: item -> sorted position
    int32_t *d_item_plane = nullptr;    // total: pre-order hyperplane of a neighbour item (index into hp_v), -1 for home
    int64_t *d_roff = nullptr;          // P_global+1 (of the tree attached when the query was created: roff_P)
    int64_t roff_P = 0;
    std::vector<int64_t> roff;          // host copy
    double *d_u = nullptr, *d_v = nullptr;   // sorted order
    double *d_w = nullptr;                   // reference order (unnormalised), debug
    double *d_yq = nullptr, *d_vq = nullptr; // Nq
    void *d_tmp = nullptr; size_t tmp_bytes = 0;
    void *d_sort_scratch = nullptr; int64_t sort_cap = 0;
    void *d_tasks = nullptr; int64_t ntasks = 0, tasks_cap = 0, strip_grid = 0;
    uint32_t *d_sync = nullptr; int64_t sync_cap = 0, nsync = 0, round_base = 0;   // arrival counters of the strips' lock-step groups   // prediction strip tasks (owned regions)
    bool planned = false;
    // multi-output prediction (pmk_query_items_multi / _mix_multi): R means per item and per query
    int R_items = 0;                    // 0: items_multi has not run on the current plan
    bool var_items = false, mixed_multi = false;
    double *d_um = nullptr; int64_t um_cap = 0;       // sorted items x um_ld (row-major)
    int um_ld = 0;                      // R_items + q of the model's trend: the items kernel also emits kq . C_H
    double *d_yqm = nullptr; int64_t yqm_cap = 0;     // Nq x R column-major
    int64_t *d_mcpre = nullptr; int64_t mcpre_cap = 0, mchunks = 0;   // chunks of 16 items per region: prefix [P+1]
    std::vector<int64_t> mcpre;         // host copy (source of the upload)
    // gradient of the blended mean (pmk_grad.hip).  items_fn: the current U are functions of x (items_multi / _fitted,
    // not the lookups of items_loo_multi); grad_items: pmk_query_items_grad has run on them; a new plan or new items
    // discard both
    bool items_fn = false, grad_items = false, mixed_grad = false;
    double *d_gm = nullptr; int64_t gm_cap = 0;       // sorted items x (D x R_items): G[p][d + D c]
    double *d_dyq = nullptr; int64_t dyq_cap = 0;     // Nq x (D x R_items) column-major: dYq[j + Nq (d + D c)]
    // gradient of the blended variance (pmk_vgrad.hip), on items computed with want_var = 1; discarded like the above
    bool vgrad_items = false, mixed_vgrad = false;
    double *d_gv = nullptr; int64_t gv_cap = 0;       // sorted items x D: GV[p][d]
    double *d_gh = nullptr; int64_t gh_cap = 0;       // sorted items x (D x q), under a trend: GH[p][a + q d] = (g_d^T C_H)_a
    double *d_dvq = nullptr; int64_t dvq_cap = 0;     // Nq x D column-major: dVq[j + Nq d]
    int64_t *d_vgpre = nullptr; int64_t vgpre_cap = 0, vstrips = 0;   // strips of vgrad_strip_items(D) items per region: prefix [P+1]
    std::vector<int64_t> vgpre;         // host copy (source of the upload)
    // joint covariance of the batch (pmk_cov.hip).  cov_items: pmk_query_items_cov has run on the current plan;
    // mixed_cov: pmk_query_mix_cov after it.  A new plan or new items discard both.  All buffers grow only.
    bool cov_items = false, mixed_cov = false;
    bool explicit_items = false;        // the items are those of pmk_query_create_items: one per point, no blend
    char *d_cov_v = nullptr; int64_t cov_v_cap = 0;               // V arena, bytes: one ld x TQ strip of the model's type per task
    double *d_cov_s = nullptr; int64_t cov_s_cap = 0;             // region blocks, m_r x m_r column-major at cov_goff[r]
    double *d_cov = nullptr; int64_t cov_cap = 0;                 // the result, Nq x Nq column-major
    pmk::CovTask *d_cov_tasks = nullptr; int64_t cov_tasks_cap = 0, cov_ntasks = 0;
    pmk::CovPair *d_cov_pairs = nullptr; int64_t cov_pairs_cap = 0, cov_npairs = 0;
    int64_t *d_cov_goff = nullptr; int64_t cov_goff_cap = 0;      // P + 1
    std::vector<int64_t> cov_goff;      // host copy: prefix of m_r^2
    // the trend's term of the blocks (pmk_query_items_cov_multi, pmk_cov_trend.hip).  cov_trend_q > 0: the blocks carry
    // z_a . z_b of a trend with that many basis functions, computed from the item rows of pmk_query_items_multi, and the
    // blend reads d_cov_flags in place of the model's info; new items discard such blocks, pmk_query_items_cov replaces them
    int cov_trend_q = 0;
    double *d_cov_z = nullptr; int64_t cov_z_cap = 0;             // sorted items x TQ_MAX: z = L_G^-1 rho
    int32_t *d_cov_flags = nullptr; int64_t cov_flags_cap = 0;    // P: info != 0 or tinfo != 0
    // posterior draws from the region blocks (pmk_draw.hip).  cov_factored: pmk_query_factor_cov has run on the current
    // blocks; whatever discards the blocks, and new blocks, discard the factors.  All buffers grow only.
    bool cov_factored = false;
    double *d_cov_f = nullptr; int64_t cov_f_cap = 0;             // padded factors, at cov_foff[r]
    std::vector<int64_t> cov_foff;      // host copy: prefix of (DRAW_TILE nt_r)^2
    pmk::DrawRegion *d_fdesc = nullptr; int64_t fdesc_cap = 0;    // P
    int32_t *d_forder = nullptr; int64_t forder_cap = 0;          // P: the regions by descending tile count
    std::vector<int32_t> fstep_regions; // regions with more than k tiles, per block step k
    pmk::DrawTask *d_ftasks = nullptr; int64_t ftasks_cap = 0, nftasks = 0;     // every tile row of every region
    int32_t *d_finfo = nullptr; int64_t finfo_cap = 0;            // P status words (pmk_query_factor_info)
    int32_t *d_fact = nullptr; int64_t fact_cap = 0;              // P: the region is factored by the current call
    double *d_fjit = nullptr; int64_t fjit_cap = 0;               // P: the absolute jitter that was added
    double *d_frel = nullptr; int64_t frel_cap = 0;               // 2 P: rel of the factors held, rel of the current call
    double *d_draw_t = nullptr; int64_t draw_t_cap = 0;           // total x (draw chunk): T_r = L_r Z_r in sorted-item order
    double *d_draw_z = nullptr; int64_t draw_z_cap = 0;           // device copy of a chunk of host z
    double *d_draw_e = nullptr; int64_t draw_e_cap = 0;           // a chunk of E for a host pointer
    // block kriging (pmk_query_items_block, pmk_block.hip).  block_items: it has run on the current items; block_var: with
    // the variance, so the aggregates and their pieces are there.  New items or a new plan discard both.  Grow only.
    bool block_items = false, block_var = false;
    int64_t blk_F = 0, blk_naggs = 0, blk_ntasks = 0, blk_grid = 0;
    int32_t *d_blk_group = nullptr; double *d_blk_a = nullptr; int64_t blk_q_cap = 0;      // Nq: group and coefficient
    int64_t *d_blk_gq = nullptr; int64_t blk_gq_cap = 0;                                   // F + 1: first query of a group
    double *d_blk_w = nullptr; int32_t *d_blk_head = nullptr, *d_blk_agg_of = nullptr;     // per sorted item: weight, head
    int64_t *d_blk_scan = nullptr; int64_t blk_item_cap = 0;                               //   flag, aggregate; scan of the heads
    pmk::BlockAgg *d_blk_aggs = nullptr; double *d_blk_piece = nullptr; int64_t blk_agg_cap = 0;   // pieces: kappa, |Vbar|^2, |zbar|^2, sum w^2 (blk_agg_cap each)
    pmk::BlockTask *d_blk_tasks = nullptr; int64_t blk_tasks_cap = 0;
    int64_t *d_blk_aoff = nullptr; int64_t blk_aoff_cap = 0;                               // P + 2: first aggregate of a region, then the cap's offender
    double *d_blk_y = nullptr; int64_t blk_y_cap = 0;                                      // F x R column-major
    double *d_blk_v = nullptr; int64_t blk_v_cap = 0;                                      // F
    double min_v = 1e-12;           // floor of the predictive variance (queryinner!'s keyword min_v, mixtureGP.jl:296)
    // blended leave-one-out (pmk_query_items_loo, pmk_loo_mix.hip): non-member marks and their exclusive scan over the
    // sorted items, the compacted requests (points, regions, addends) and their results, ONE allocation with d_loo_x as
    // its base (grow only); the inner query of explicit items that runs the requests, created on first need
    double *d_loo_x = nullptr; int64_t loo_cap = 0;
    double *d_loo_diag = nullptr, *d_loo_ru = nullptr, *d_loo_rv = nullptr;
    int64_t *d_loo_off = nullptr;
    int32_t *d_loo_mark = nullptr, *d_loo_region = nullptr;
    pmk_query *loo_inner = nullptr;
};

namespace pmk {

// sigma2 of the resident factor per local patch: the device array after pmk_model_fit_patches, one value otherwise
inline const double *patch_sigma2s(const pmk_model *m) { return m->hyper_uniform ? nullptr : m->d_sigma2s; }

// grid of a kernel of 256 threads per workgroup with one thread per entry
inline dim3 grid256(int64_t n) { return dim3((unsigned)((n + 255) / 256)); }

// ---- launchers implemented in the .hip files (all enqueue on `s`) ----
// precision-generic kernels live in namespaces f64 / f32 (the same sources compiled twice)
// launch_kernel_matrix_slabs, launch_items, launch_items_multi: th non-null is that descriptor for every patch, null the
// model's per-patch device arrays (pmk_dispatch.h)
#define PMK_DECLARE_REAL_LAUNCHERS(NS)                                                                              \
    namespace NS {                                                                                                   \
    int launch_kernel_matrix_slabs(const pmk_model *m, const pmk_kernel_desc *th, double sigma2, hipStream_t s,      \
                                   int64_t p0, int64_t np, bool diag_only);                                          \
    int launch_cholesky(pmk_model *m, hipStream_t s, int64_t p0, int64_t np);                                        \
    int launch_backsolve(pmk_model *m, hipStream_t s, int64_t p0, int64_t np);                                       \
    int launch_ninv_from_slabs(pmk_model *m, hipStream_t s);                                                         \
    int set_device_attributes();                                                                                     \
    int build_strip_tasks(pmk_query *q, hipStream_t s);                                                              \
    int launch_items(pmk_query *q, const pmk_kernel_desc *th, hipStream_t s);                                        \
    int launch_solve_multi(pmk_model *m, hipStream_t s);                                                             \
    int launch_items_multi(pmk_query *q, const pmk_kernel_desc *th, hipStream_t s);                                  \
    int launch_loo(pmk_model *m, hipStream_t s);                                                                     \
    int launch_evidence(const pmk_model *m, int R, double *d_logdet, double *d_quad, hipStream_t s);                 \
    int launch_loo_values(const pmk_model *m, int R, double *d_res, double *d_var, hipStream_t s);                   \
    int launch_gather_points(const pmk_model *m, const double *d_X, const double *d_y, hipStream_t s);               \
    int launch_gather_vector(const pmk_model *m, const double *d_src, void *d_dst, hipStream_t s);                   \
    int launch_gather_multi(const pmk_model *m, int R, const double *d_Y, int64_t ldy, hipStream_t s);               \
    int launch_trend_fill(const pmk_model *m, int R, int q, hipStream_t s);                                          \
    int launch_trend_gls(pmk_model *m, int R, int q, hipStream_t s);                                                 \
    int launch_trend_loo_values(const pmk_model *m, int R, int q, double *d_res, double *d_var, hipStream_t s);      \
    int launch_loo_member(pmk_query *q, int noisy, int32_t *d_mark, hipStream_t s);                                  \
    int launch_loo_compact(pmk_query *q, const int32_t *d_mark, const int64_t *d_off, double *x_out,                 \
                           int32_t *region_out, double *diag_out, hipStream_t s);                                    \
    int launch_loo_scatter(pmk_query *q, int noisy, const int32_t *d_mark, const int64_t *d_off, const double *d_ru, \
                           const double *d_rv, hipStream_t s);                                                       \
    int launch_loo_member_multi(pmk_query *q, int noisy, int want_var, int32_t *d_mark, hipStream_t s);              \
    int launch_items_grad(pmk_query *q, const pmk_kernel_desc *th, hipStream_t s);                                   \
    int launch_items_vgrad(pmk_query *q, const pmk_kernel_desc *th, hipStream_t s);                                  \
    int launch_items_cov(pmk_query *q, const pmk_kernel_desc *th, hipStream_t s);                                    \
    int launch_items_block(pmk_query *q, const pmk_kernel_desc *th, hipStream_t s);                                  \
    int launch_append_border(pmk_model *m, const pmk_query *q, const double *d_y, const double *d_diag, hipStream_t s); \
    int set_append_attributes();                                                                                     \
    int launch_remove_rows(pmk_model *m, const RemoveTask *d_tasks, int64_t ntasks, const int32_t *d_rows,           \
                           hipStream_t s);                                                                           \
    int set_remove_attributes();                                                                                     \
    int launch_reserve(const pmk_model *m, const PatchDesc *d_new_desc, void *x, void *y, void *z, void *c,          \
                       void *diag, void *a, void *inv, int64_t max_ld, hipStream_t s);                               \
    }
PMK_DECLARE_REAL_LAUNCHERS(f64)
PMK_DECLARE_REAL_LAUNCHERS(f32)
#define PMK_BY_DTYPE(m, CALL) ((m)->dtype == PMK_F32 ? pmk::f32::CALL : pmk::f64::CALL)

int launch_kernel_matrix_dense(const pmk_kernel_desc &th, int D, int64_t n, const double *d_xs, int64_t ldx,
                               int64_t mcols, const double *d_zs, int64_t ldz, double *d_K, int64_t ldk,
                               bool symmetric, hipStream_t s);
// the strip workspace of the model (max_nt * TILE x TQ elements per slot), grow only; host side (pmk_api.cpp)
int reserve_strips(pmk_model *m, int64_t slots);
int set_plan_attributes();
int launch_iota(int32_t *d, int64_t n, hipStream_t s);
int query_reserve(pmk_query *q, int64_t Nq);
int query_set_items(pmk_query *q, int64_t n, const double *xq, const int32_t *region);
int launch_plan_count(pmk_query *q, double radius, double delta, hipStream_t s);
int launch_plan_fill(pmk_query *q, double radius, double delta, hipStream_t s);
int launch_sort_items(pmk_query *q, hipStream_t s);
int launch_mix(pmk_query *q, const pmk_kernel_desc &wth, int64_t q0, int64_t q1, hipStream_t s);
int launch_mix_multi(pmk_query *q, const pmk_kernel_desc &wth, int64_t q0, int64_t q1, hipStream_t s);
int launch_trend_items(pmk_query *q, int R, int qt, bool want_var, hipStream_t s);
int launch_mix_grad(pmk_query *q, const pmk_kernel_desc &wth, int64_t q0, int64_t q1, hipStream_t s);
int launch_trend_vgrad(pmk_query *q, hipStream_t s);
int launch_mix_vgrad(pmk_query *q, const pmk_kernel_desc &wth, int64_t q0, int64_t q1, hipStream_t s);
int launch_mix_cov(pmk_query *q, const pmk_kernel_desc &wth, hipStream_t s);
int launch_cov_trend(pmk_query *q, hipStream_t s);
int launch_cov_trend_items(pmk_query *q, hipStream_t s);
int launch_block_weights(pmk_query *q, const pmk_kernel_desc &wth, hipStream_t s);
int launch_block_heads(pmk_query *q, hipStream_t s);
int launch_block_aggregates(pmk_query *q, int cap, unsigned long long *d_over, int64_t *d_aoff, hipStream_t s);
int launch_block_reduce(pmk_query *q, bool want_var, int qt, hipStream_t s);
int launch_factor_cov(pmk_query *q, int have_factors, hipStream_t s);
int launch_draw(pmk_query *q, const pmk_kernel_desc &wth, const double *d_z, int64_t ldz, int64_t n, double *d_E,
                int64_t lde, hipStream_t s);
int launch_loo_scatter_multi(pmk_query *q, const pmk_query *in, int noisy, int want_var, const int32_t *d_mark,
                             const int64_t *d_off, hipStream_t s);
int launch_export_requests(pmk_query *q, int64_t first, int64_t n, double *x_out, int32_t *region_out, hipStream_t s);
int launch_export_request_diag(pmk_query *q, int64_t first, int64_t n, double *diag_out, hipStream_t s);
int launch_export_results(pmk_query *q, double *u_out, double *v_out, hipStream_t s);
int grow_item_buffers(pmk_query *q, int64_t total);
int launch_explicit_items(pmk_query *q, int *d_bad, hipStream_t s);
int launch_query_mean(const pmk_kernel_desc *th, int nth, int D, int64_t n, const double *d_xs, int64_t ldx,
                      const double *d_c, int64_t nq, const double *d_xq, double *d_yq, hipStream_t s);
int64_t exclusive_scan_i32_to_i64(const int32_t *d_in, int64_t *d_out, int64_t n, void **tmp, size_t *tmp_bytes,
                                  hipStream_t s);

}  // namespace pmk
