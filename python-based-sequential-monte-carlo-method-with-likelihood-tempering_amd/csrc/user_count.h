// user_count.h -- count observations of a user model (include/smc_hip.h: COUNT OBSERVATIONS): an output whose
// values are counts has a Poisson (family 1) or negative-binomial (family 2) term in the likelihood instead of a Gaussian one.
// The families come with the source (smc_user_obs_family, read by the library as it reads smc_user_root_dir); a model with a
// count output is compiled with SMC_USER_COUNT 1 and SMC_USER_FAMILY, the list as an initialiser, and gets this file as an
// in-memory header in front of user_obs_args.h (built-in types only, no #include).
//
// Mean and variance: the model output f is the mean mu, the variance is mu + (b mu)^2 with b the output's proportional entry
// (0 for Poisson; negative binomial: b > 0, size phi = 1 / b^2).  The image does not grow: a count output's record word holds
// the count, its additive entry is fixed 1 and its scale 1, so an item's weight q_k = (b_k / (a_k s_k))^2 IS b_k^2; and the
// image's "sum of log s_k" words, which a noise model does not read, hold C_e, the experiment's sum of c(y) over its Poisson
// values.
//
// As every term under a noise model (user_obs_args.h) a count adds its EXCESS x >= 0 over a floor that does not depend on the
// solve, so that an item's sum only grows and early rejection stays exact:
//   Poisson             floor -c(y), c(y) = lgamma(y + 1) - y log y + y (the saturated model, a data constant, summed on the host);
//                       x = y (d - L), d = (mu - y) / y, L = log1p(d) (d >= -1/2) or log mu - log y (d < -1/2: the same number,
//                       without losing a mu below y 2^-53);  x = mu for y = 0.   log p = -c(y) - x.
//   negative binomial   floor 0;  u = b^2 mu:  x = -[lgamma(y + phi) - lgamma(phi) - lgamma(y + 1) - phi log1p(u) + y log u - y log1p(u)]
//                       (y = 0: x = phi log1p(u)).
// Both: x clamped at >= 0 (a negative published sum means "cancelled" to the scheduler); mu NaN gives NaN, the route of a failed
// output; mu < 0, mu = +inf, or mu = 0 with y > 0 give +inf; mu = 0 with y = 0 gives 0.  user_models.count_excess is the same in
// NumPy, operation for operation.
#pragma once

#if defined(SMC_USER_COUNT)   /* the device part; this file is embedded whole */
namespace smc_cnt {
constexpr int kGaussian = 0, kPoisson = 1, kNegBin = 2;
// NOT inlined, for noise_half_log1p's reason (user_obs_args.h): the bulk attempt loop must not pay for the registers of log1p and
// lgamma.  Every product and sum is rounded on its own, in the RK45 kernel too: one text, one result for both integrators.
__device__ __attribute__((noinline)) double poisson_excess(double y, double mu) {
#pragma clang fp contract(off)
    const double inf = __builtin_huge_val();
    if (mu != mu) return mu;
    if (mu < 0.0 || mu == inf) return inf;
    if (y == 0.0) return mu;
    if (mu == 0.0) return inf;
    const double d = (mu - y) / y;
    const double l = (d < -0.5) ? log(mu) - log(y) : log1p(d);
    const double x = y * (d - l);
    return x < 0.0 ? 0.0 : x;      // NaN stays NaN
}
// b2 = b^2; not > 0 (the parameters make logL -inf: the item's weights are zeroed): 0, a sum that is never used
__device__ __attribute__((noinline)) double negbin_excess(double y, double mu, double b2) {
#pragma clang fp contract(off)
    const double inf = __builtin_huge_val();
    if (!(b2 > 0.0)) return 0.0;
    if (mu != mu) return mu;
    if (mu < 0.0 || mu == inf) return inf;
    const double phi = 1.0 / b2;
    const double u = b2 * mu;
    const double l1 = log1p(u);
    const double pl = phi * l1;
    double x = pl;
    if (y != 0.0) {
        if (mu == 0.0) return inf;
        const double g = (lgamma(y + phi) - lgamma(phi)) - lgamma(y + 1.0);
        const double yl = y * log(u);
        const double y1 = y * l1;
        x = -(((g - pl) + yl) - y1);
    }
    return x < 0.0 ? 0.0 : x;      // NaN stays NaN
}
}  // namespace smc_cnt
#endif
