// prior.h -- device evaluation of the independent prior densities (shared by the model-specific MH kernels)
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/smc_hip.h"
#include "smc_internal.h"

namespace smc {

__device__ __forceinline__ double prior_quiet_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

// scipy.stats pdf of one independent prior at x (Micmem_SMC_main.py:71-85).
//   uniform: support mask on the standardised value y = (x-loc)/scale, closed interval [0,1];
//   normal : exp(-y^2/2)/sqrt(2*pi)/scale.
__device__ __forceinline__ double prior_pdf(int kind, double a, double b, double x) {
    if (kind == SMC_PRIOR_FLAT) return 1.0;
    if (kind == SMC_PRIOR_UNIFORM) {
        const double scale = b - a;
        const double y = (x - a) / scale;
        if (x != x) return x;
        return (y >= 0.0 && y <= 1.0 && scale > 0.0) ? 1.0 / scale : 0.0;
    } else {
        const double y = (x - a) / b;
        if (!(b > 0.0)) return prior_quiet_nan();
        return exp(-(y * y) / 2.0) / 2.5066282746310002 / b;
    }
}

// The families of smc_set_prior_ex (include/smc_hip.h: PRIOR FAMILIES; priors.prior_log_kernel is the same in NumPy): the
// log-kernel k(x) of one parameter - the log-density without its normaliser - or -inf outside the support, NaN for a NaN
// argument.  `x in support` is `k > -inf` (false for NaN).  Every decision is a comparison of doubles formed in the order written
// here, without contraction.  Out of line, for count_draw.h's reason: a leaf (log and log1p are inlined into it, nothing is
// called), so it needs no stack, and the propose kernels do not pay for its registers on the path without new kinds.
__device__ __attribute__((noinline)) static double prior_log_kernel(int kind, double a, double b, double lo, double hi, double x) {
#pragma clang fp contract(off)
    const double ninf = -__longlong_as_double(0x7ff0000000000000LL);
    if (x != x) return x;
    if (kind == SMC_PRIOR_TRUNCNORMAL) {
        if (!(x >= lo && x <= hi)) return ninf;
        const double y = (x - a) / b;
        return -(y * y) / 2.0;
    }
    if (kind == SMC_PRIOR_BETA) {
        const double u = (x - lo) / (hi - lo);
        if (!(x > lo && x < hi && u > 0.0 && u < 1.0)) return ninf;      // an x whose u rounds to 0 or 1 (an ulp from an end) is outside
        return (a - 1.0) * log(u) + (b - 1.0) * log1p(-u);
    }
    if (!(x > 0.0 && x < -ninf)) return ninf;      // +inf: density 0, not the NaN of inf - inf
    const double L = log(x);
    if (kind == SMC_PRIOR_LOGNORMAL) {
        const double t = L - a;
        return -L - (t * t) / (2.0 * (b * b));
    }
    return (a - 1.0) * L - x / b;      // SMC_PRIOR_GAMMA
}

// The old kinds' factor of one parameter in P (a new kind has none there: 1.0 exactly, so P keeps its bits) ...
__device__ __forceinline__ double prior_pdf_old(const Prior &prior, int c, double x) {
    return prior.kind[c] >= SMC_PRIOR_LOGNORMAL ? 1.0 : prior_pdf(prior.kind[c], prior.a[c], prior.b[c], x);
}
// ... and the new kinds' term in K (0 for an old kind)
__device__ __forceinline__ double prior_k_new(const Prior &prior, int c, double x) {
    return prior.kind[c] >= SMC_PRIOR_LOGNORMAL ? prior_log_kernel(prior.kind[c], prior.a[c], prior.b[c], prior.lo[c], prior.hi[c], x) : 0.0;
}
// p0_2 / p0_1 from P(cand), P(cur), K(cand), K(cur); in_support: P(cand) > 0 and every new-kind parameter of cand in support
__device__ __forceinline__ double prior_ratio_new(double pdf, double cur_pdf, double kc, double kf, bool in_support) {
    return in_support ? pdf / cur_pdf * exp(kc - kf) : 0.0;
}

}  // namespace smc
