// prior_draw.h -- one prior draw of a family of smc_set_prior_ex on the Philox stream (include/smc_hip.h: PRIOR FAMILIES;
// DESIGN.md 4.18): a log-normal, gamma, beta or truncated normal value keyed by (seed, global particle, tag 0x505249, cell = the
// parameter's index) on count_draw.h's uniform supply, so that a value depends on neither the launch geometry nor the number of
// ranks nor the kinds of the other parameters.  sample_prior_kernel takes it for a parameter of a new kind;
// tests/prior_reference.py is the same in NumPy, decision for decision.
//
// Host/device portable like count_draw.h (tests/hostcheck/prior_draw_hostcheck.cpp compiles it stand-alone); no contraction, IEEE
// division; the heavy pieces are count_draw.h's leaves plus one exp.  kind, a, b, lo, hi obey smc_prior_check's rules - the
// gammas rely on its floor of 1 / 16 on a shape (below it gamma_boost underflows to 0 with probability exp(-745 shape)), the
// truncated normal's loop relies on its mass rule: a trial fails with probability at most 1/2, a dry supply (254 trials: NaN) has
// probability at most 2^-254.
#pragma once

#include "count_draw.h"

namespace smc_draw {

constexpr unsigned long long kTagPrior = 0x505249ull;
constexpr int kLogNormal = 3, kGamma = 4, kBeta = 5, kTruncNormal = 6;      // SMC_PRIOR_* (include/smc_hip.h)

SMC_DRAW_LEAF double prior_exp(double x) {
#pragma clang fp contract(off)
    return exp(x);
}

__host__ __device__ inline double prior_draw_on(Supply &s, int kind, double a, double b, double lo, double hi) {
#pragma clang fp contract(off)
    const double nan = __builtin_nan("");
    if (kind == kLogNormal) {
        const double z = normal(s);
        if (s.dry) return nan;
        return prior_exp(a + b * z);
    }
    if (kind == kGamma) {
        const double G = gamma_mt(s, a);
        if (s.dry) return nan;
        return b * G;
    }
    if (kind == kBeta) {
        const double G1 = gamma_mt(s, a);
        if (s.dry) return nan;
        const double G2 = gamma_mt(s, b);
        if (s.dry) return nan;
        return lo + (hi - lo) * (G1 / (G1 + G2));
    }
    if (kind != kTruncNormal) return nan;
    for (;;) {
        const double z = normal(s);
        if (s.dry) return nan;
        const double x = a + b * z;
        if (x >= lo && x <= hi) return x;
    }
}

static __host__ __device__ inline double prior_draw(int kind, double a, double b, double lo, double hi, unsigned long long seed,
                                                    unsigned long long g, unsigned long long cell) {
    Supply s = supply(seed, g, kTagPrior, cell);
    return prior_draw_on(s, kind, a, b, lo, hi);
}

}  // namespace smc_draw
