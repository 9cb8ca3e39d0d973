// Launch dispatch: from the run-time input dimension, kernel family and hyperparameter mode to the <D, FAM, PP>
// instantiation of a kernel.  Host side only; every launcher of a templated kernel goes through here, so that a kernel's
// argument list is written once and the limits (and their error) are stated once.
#pragma once

#include <type_traits>

#include "pmk_internal.h"

namespace pmk {

// f(std::integral_constant<int, D>) for the run-time D; f returns the launcher's code.  The one switch over the dimension.
template <class F> int dispatch_dim(int D, F &&f)
{
    switch (D) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    case 4: return f(std::integral_constant<int, 4>{});
    default: set_error("unsupported input dimension %d (1..%d)", D, MAX_D); return -2;
    }
}

// f(D, FAM): Spline34 has instantiations of its own, every other family shares the run-time family switch (FAM = 0)
template <class F> int dispatch_dim_family(int D, bool spline34, F &&f)
{
    return dispatch_dim(D, [&](auto dd) {
        return spline34 ? f(dd, std::integral_constant<int, PMK_SPLINE34>{}) : f(dd, std::integral_constant<int, 0>{});
    });
}

// The hyperparameter convention of the launchers that evaluate theta: `th` non-null is this descriptor (and the sigma2
// passed with it) for every patch, null is the model's device arrays d_ths / d_sigma2s from patch p0 on (PP = true).  The
// family comes from `th` when there is one -- it need not be the model's -- and from the model only when there is none.
inline bool hyper_spline34(const pmk_model *m, const pmk_kernel_desc *th)
{
    return th ? th->family == PMK_SPLINE34 : m->hyper_s34;
}
// the kernel arguments of HyperArgs<PP>
template <bool PP> auto hyper_th(const pmk_model *m, const pmk_kernel_desc *th, int64_t p0 = 0)
{
    if constexpr (PP) return (const pmk_kernel_desc *)(m->d_ths + p0);
    else return *th;
}
template <bool PP> auto hyper_sigma2(const pmk_model *m, double sigma2, int64_t p0 = 0)
{
    if constexpr (PP) return (const double *)(m->d_sigma2s + p0);
    else return sigma2;
}

// f(D, FAM, PP) for a model and the `th` of the convention above
template <class F> int dispatch_hyper(const pmk_model *m, const pmk_kernel_desc *th, F &&f)
{
    return dispatch_dim_family(m->D, hyper_spline34(m, th), [&](auto dd, auto fam) {
        return th ? f(dd, fam, std::false_type{}) : f(dd, fam, std::true_type{});
    });
}

}  // namespace pmk
