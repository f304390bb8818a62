// user_input.h -- time-varying measured inputs of a user model (include/smc_hip.h: smc_set_model_user5): what a source calls as
//   double smc_input(const double *cond, int k, double t)
// Device code only, handed to hiprtc as an in-memory header and included by the generated source ONLY for a model with inputs
// (user_model.hip: build_source defines SMC_USER_NCOND, SMC_USER_NIN and SMC_USER_KCAP in front of the #include); a model without
// inputs never sees this file, and its source is the text it always was.
//
// The table lies BEHIND each experiment's cond row in global memory: `cond` reaches every function of the
// model as a per-experiment pointer with a run-time stride, so the row simply grows - neither kernel file nor solve_sched.h knows.
// One row, in doubles, with C = SMC_USER_NCOND, K = SMC_USER_KCAP (the knot capacity: the power of two >= n_knot):
//   [0, C)                        the model's cond numbers
//   [C, C + K)                    tk: the row's m knots, then +inf
//   then per input k, 2 K + 1:    u[0 .. K]: the m values, then u[m - 1];  s[0 .. K): the slopes
//                                 s[j] = (u[j + 1] - u[j]) / (tk[j + 1] - tk[j]) for j < m - 1, 0 from there on
// The slopes are formed once on the host with IEEE division (user_model.hip: build_input_rows; user_models.input_value is the
// same arithmetic in NumPy), so the lookup divides nothing: it is the same number in the lean and in the IEEE namespace of the
// RK45 source, and a repeated attempt sees the input it saw before.
#pragma once
#ifndef __HIPCC_RTC__
#include <hip/hip_runtime.h>
#endif

namespace smc_in {

constexpr int kCond = SMC_USER_NCOND, kIn = SMC_USER_NIN, kCap = SMC_USER_KCAP;
static_assert(kIn >= 1 && kIn <= 8 && kCap >= 1 && (kCap & (kCap - 1)) == 0, "SMC_USER_NIN in 1 .. 8, SMC_USER_KCAP a power of two");
constexpr int kKnotAt = kCond, kInputAt = kCond + kCap, kInputWords = 2 * kCap + 1;
constexpr int kRowWords = kCond + kCap + kIn * kInputWords;

// np.interp(t, tk, u_k) for the experiment `cond` belongs to.  j = the last knot <= t (0 for t before the first): a bisection
// of log2 K selects, no branch, the same trip count for every lane whatever its experiment - the +inf padding is never <= t.
// Past the last knot s = 0 and u[j + 1] = u[j]; before the first the distance is clamped to 0.  At t == tk[j] the distance is 0
// and the value u[j] itself; between two knots the final clamp keeps a rounded u[j] + s (t - tk[j]) inside [u[j], u[j + 1]].
__device__ __forceinline__ double smc_input(const double *cond, int k, double t) {
    const double *tk = cond + kKnotAt;
    int j = 0;
#pragma unroll
    for (int step = kCap >> 1; step > 0; step >>= 1) j += (tk[j + step] <= t) ? step : 0;
    const double *u = cond + kInputAt + k * kInputWords;
    const double u0 = u[j], u1 = u[j + 1], s = u[kCap + 1 + j];
    const double dt = fmax(t - tk[j], 0.0);
    const double v = u0 + s * dt;
    return fmin(fmax(v, fmin(u0, u1)), fmax(u0, u1));
}

}  // namespace smc_in
