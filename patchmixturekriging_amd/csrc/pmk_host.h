// Host-side helpers shared by the sources of the C ABI (pmk_api.cpp, pmk_api_query.cpp, pmk_api_loo_mix.cpp,
// pmk_api_append.cpp): device allocations, the checks and the drivers that more than one of them needs.  Host code only:
// no .hip file includes this.
#pragma once

#include <vector>

#include "pmk_internal.h"

namespace pmk {

inline bool kernel_ok(const pmk_kernel_desc *th)
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

// the blending profile of pmk_query_mix / _mix_multi: a stationary kernel
inline int blend_profile_ok(const pmk_kernel_desc *weight_th, const char *who)
{
    if (!kernel_ok(weight_th) || weight_th->family >= PMK_BB10) {
        set_error("%s: the blending profile must be a stationary kernel (evalkernel(tau, theta))", who);
        return -2;
    }
    return 0;
}

// a kernel the covariance stages evaluate: any family, ModSqExp only at D = 1 (nothing here differentiates, so the
// Brownian-bridge families are admitted)
inline int cov_kernel_ok(const pmk_kernel_desc *th, int D, const char *who, const char *role)
{
    if (!kernel_ok(th)) { set_error("%s: unknown kernel family (%s)", who, role); return -2; }
    if (th->family == PMK_MODSQEXP && D > 1) {
        set_error("%s: %s is PMK_MODSQEXP, which is defined for D = 1 only (D = %d)", who, role, D);
        return -2;
    }
    return 0;
}

template <typename T>
int dev_alloc(T **p, int64_t count)
{
    *p = nullptr;
    if (count <= 0) count = 1;
    PMK_HIP(hipMalloc((void **)p, sizeof(T) * (size_t)count));
    return 0;
}

template <typename T>
void dev_free(T *&p)
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

// a device buffer of `cap` elements that only grows: replaced when `need` exceeds it, after the stream has drained
// (earlier launches may still read the old one); nothing waits when it is large enough
template <typename T>
int grow(T *&p, int64_t &cap, int64_t need, hipStream_t s)
{
    if (cap >= need) return 0;
    PMK_HIP(hipStreamSynchronize(s));
    dev_free(p);
    cap = 0;
    if (dev_alloc(&p, need)) return -100;
    cap = need;
    return 0;
}

// grow() for a buffer whose size follows the caller's batch (the covariance arenas): a failed allocation says how many
// bytes `what` asked for
template <typename T>
int grow_sized(T *&p, int64_t &cap, int64_t need, hipStream_t s, const char *who, const char *what)
{
    if (!grow(p, cap, need, s)) return 0;
    set_error("%s: hipMalloc of %lld bytes for %s failed", who, (long long)(need * (int64_t)sizeof(T)), what);
    return -100;
}

// One device allocation cut into 256-byte aligned pieces: a query object used to own two dozen small buffers, and every
// hipFree is a device synchronisation (pmk_query_destroy: 3.4 ms of a 108 ms querymixtureGP! at config C).  add() names
// a pointer and its element count, in the order of the pieces; commit() allocates and points every one of them into the
// block.  The first pointer added is the base (offset 0): the one its owner frees.  Until commit() succeeds they are null.
class Arena {
    struct Piece { void **p; size_t at; };
    std::vector<Piece> pieces;
    size_t bytes = 0;

public:
    template <typename T>
    void add(T *&p, size_t count)
    {
        p = nullptr;
        pieces.push_back({reinterpret_cast<void **>(&p), bytes});
        bytes = (bytes + sizeof(T) * count + 255) & ~(size_t)255;
    }
    int commit()
    {
        char *base = nullptr;
        PMK_HIP(hipMalloc((void **)&base, bytes));
        for (const Piece &x : pieces) *x.p = base + x.at;
        return 0;
    }
};

// true if p is device memory (what a kernel can read or write); a plain or pinned host array is staged
inline bool is_device_pointer(const void *p)
{
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();                 // an unregistered host pointer: not an error of ours
        return false;
    }
    return at.type == hipMemoryTypeDevice || at.type == hipMemoryTypeManaged;
}

// the theta the launchers take for the model's own hyperparameters: one descriptor after a plain fit, else null for the
// per-patch device arrays
inline const pmk_kernel_desc *fitted_theta(const pmk_model *m) { return m->hyper_uniform ? &m->th : nullptr; }

// point-major host points (D x n) -> SoA rows of length ld.  Padding entries are 1e300: their distance
// to any real point overflows to +inf, so a compactly supported profile evaluates to exactly 0 there.
inline void pack_soa(int D, int64_t n, int64_t ld, const double *X, double *out)
{
    for (int d = 0; d < D; ++d) {
        double *row = out + (int64_t)d * ld;
        for (int64_t i = 0; i < n; ++i) row[i] = X[i * D + d];
        for (int64_t i = n; i < ld; ++i) row[i] = 1e300;
    }
}

// the model must hold every leaf of its tree (no shard): `tail` says what for, `rc` is the caller's own code
inline int whole_tree_ok(const pmk_model *m, const char *who, const char *tail, int rc)
{
    if (m->P_global != m->P || m->leaf_base != 0) {
        set_error("%s: the model holds %lld of %lld leaves; %s", who, (long long)m->P, (long long)m->P_global, tail);
        return rc;
    }
    return 0;
}

// q->mcpre and q->mchunks from the region offsets of q's plan (pmk_api.cpp)
void multi_chunk_prefix(pmk_query *q);

// the buffers of pmk_model_append go with the model (pmk_api_append.cpp; called by pmk_model_destroy)
void append_release(pmk_model *m);

// a new plan or new items discard what the multi-output and gradient stages left on the query
inline void reset_item_state(pmk_query *q)
{
    q->R_items = 0;
    q->mixed_multi = false;
    q->items_fn = q->grad_items = q->mixed_grad = false;
    q->vgrad_items = q->mixed_vgrad = false;
    q->block_items = q->block_var = false;
    // blocks with a trend's term (pmk_query_items_cov_multi) were computed from the item rows that now go
    if (q->cov_trend_q > 0) {
        q->cov_items = q->mixed_cov = q->cov_factored = false;
        q->cov_trend_q = 0;
    }
}
// a new plan or new explicit items (not new item values: the covariance does not depend on them) discard the covariance
inline void reset_plan_state(pmk_query *q)
{
    reset_item_state(q);
    q->cov_items = q->mixed_cov = q->cov_factored = false;
    q->cov_trend_q = 0;
}

// The one-shot calls: a query object for Xq, its plan, the three stages as the caller gives them, and the object goes
// again.  Returns the first non-zero code.
template <typename Items, typename Mix, typename Fetch>
int one_shot(pmk_model *m, int64_t Nq, const double *Xq, double radius, double delta, Items items, Mix mix, Fetch fetch)
{
    pmk_query *q = nullptr;
    int rc = pmk_query_create(m, Nq, Xq, &q);
    if (rc) return rc;
    if (!(rc = pmk_query_plan(q, radius, delta)) && !(rc = items(q)) && !(rc = mix(q))) rc = fetch(q);
    pmk_query_destroy(q);
    return rc;
}

}  // namespace pmk
