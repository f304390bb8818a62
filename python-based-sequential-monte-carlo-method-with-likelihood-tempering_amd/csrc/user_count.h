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
//                       x = bd0(y, mu) = y log(y / mu) + mu - y;  x = mu for y = 0.   log p = -c(y) - x.
//   negative binomial   floor 0;  u = b^2 mu, phi = 1 / b^2, n = phi + y, n p = n / (1 + u), n q = mu (1 + b^2 y) / (1 + u), L = log1p(b^2 y):
//                       x = L - [stirlerr(n) - stirlerr(phi) - stirlerr(y) - bd0(phi, n p) - bd0(y, n q)] - 1/2 [L - log(2 pi y)]
//                       (y = 0: x = phi log1p(u)).
// This is Loader's saddle-point form of the two probabilities (C. Loader, "Fast and accurate computation of binomial
// probabilities", 2000), in which no large numbers cancel:
//   bd0(x, m)    the deviance x log(x / m) + m - x >= 0.  With v = (x - m) / (x + m): where |x - m| < 0.1 (x + m) the series
//                (x - m) v + 2 x (v^3 / 3 + ... + v^19 / 19) - one sign throughout, the first term left out below 1e-18 of the sum;
//                elsewhere x L + (m - x), L = log(x / m), or log x - log m for m < x / 2 (the same number, where x / m may overflow).
//   stirlerr(n)  lgamma(n + 1) - (n + 1/2) log n + n - 1/2 log(2 pi): as written up to n = 15 (terms below 45), above by the series
//                1/(12 n) - 1/(360 n^3) + 1/(1260 n^5) - 1/(1680 n^7) + 1/(1188 n^9) - 691/(360360 n^11) + 1/(156 n^13).
// The forms they replace, y (d - log1p(d)) and a difference of lgamma(y + phi), lgamma(phi) and lgamma(y + 1), were wrong by 1e-9
// relative at y = 2^53 and by 4.7e-3 absolute at b = 1e-6; no lgamma of an argument above 16 remains.  Measured against 60-digit
// values: tests/test_likelihood_terms_truth.py.
// Both: x clamped at >= 0 (a negative published sum means "cancelled" to the scheduler); mu NaN gives NaN, the route of a failed
// output; mu < 0, mu = +inf, or mu = 0 with y > 0 give +inf; mu = 0 with y = 0 gives 0.  user_models.count_excess (count_bd0,
// count_stirlerr) is the same in NumPy, operation for operation.
#pragma once

#if defined(SMC_USER_COUNT)   /* the device part; this file is embedded whole */
namespace smc_cnt {
constexpr int kGaussian = 0, kPoisson = 1, kNegBin = 2;
// Inlined into the two excess functions, which stay leaves.  Every product and sum is rounded on its own, in the RK45 kernel too:
// one text, one result for both integrators.  (The attribute is spelled out: this file is read in front of every other header.)
__device__ inline __attribute__((always_inline)) double bd0(double x, double m) {
#pragma clang fp contract(off)
    const double d = x - m;
    const double s = x + m;
    if (fabs(d) < 0.1 * s) {
        const double v = d / s;
        const double v2 = v * v;
        double p = 1.0 / 19.0;
        p = p * v2 + 1.0 / 17.0;
        p = p * v2 + 1.0 / 15.0;
        p = p * v2 + 1.0 / 13.0;
        p = p * v2 + 1.0 / 11.0;
        p = p * v2 + 1.0 / 9.0;
        p = p * v2 + 1.0 / 7.0;
        p = p * v2 + 1.0 / 5.0;
        p = p * v2 + 1.0 / 3.0;
        return d * v + ((2.0 * x) * v) * (v2 * p);
    }
    const double l = (m < 0.5 * x) ? log(x) - log(m) : log(x / m);
    return x * l + (m - x);
}
__device__ inline __attribute__((always_inline)) double stirlerr(double n) {
#pragma clang fp contract(off)
    if (n <= 15.0) return ((lgamma(n + 1.0) - (n + 0.5) * log(n)) + n) - 0.9189385332046727;
    const double r = 1.0 / n;
    const double r2 = r * r;
    return r * (1.0 / 12.0 - r2 * (1.0 / 360.0 - r2 * (1.0 / 1260.0 - r2 * (1.0 / 1680.0 - r2 * (1.0 / 1188.0 - r2 * (691.0 / 360360.0 - r2 * (1.0 / 156.0)))))));
}
// NOT inlined, for noise_half_log1p's reason (user_obs_args.h): the bulk attempt loop must not pay for the registers of log and
// lgamma.
__device__ __attribute__((noinline)) double poisson_excess(double y, double mu) {
#pragma clang fp contract(off)
    const double inf = __builtin_huge_val();
    if (mu != mu) return mu;
    if (mu < 0.0 || mu == inf) return inf;
    if (y == 0.0) return mu;
    if (mu == 0.0) return inf;
    const double x = bd0(y, mu);
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
        const double n = phi + y;
        const double den = 1.0 + u;
        const double b2y = b2 * y;
        const double ly = log1p(b2y);
        const double n_p = n / den;
        const double n_q = mu * ((1.0 + b2y) / den);
        const double lc = (((stirlerr(n) - stirlerr(phi)) - stirlerr(y)) - bd0(phi, n_p)) - bd0(y, n_q);
        x = (ly - lc) - 0.5 * (ly - log(6.283185307179586 * y));
    }
    return x < 0.0 ? 0.0 : x;      // NaN stays NaN
}
}  // namespace smc_cnt
#endif
