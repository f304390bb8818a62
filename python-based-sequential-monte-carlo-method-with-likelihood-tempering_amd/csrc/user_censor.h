// user_censor.h -- censored observations of a user model (include/smc_hip.h: smc_set_model_user7): a value the
// assay could not quantify is known to lie at or below a lower limit (left-censored) or at or above an upper one
// (right-censored), and contributes log Phi(z) to the likelihood instead of a density (Beal's M3).  Read by the library and,
// for a model compiled with SMC_USER_CENSOR, handed to hiprtc as an in-memory header in front of user_obs_args.h (built-in
// types only, no #include).
//
// Layout: a record of the LDS image (user_obs_args.h) gains ONE word, its last, that holds the flags of the record's outputs as
// an integer-valued double: sum over k of c_k 4^k, c_k = 0 quantified (or not measured), 1 left-censored, 2 right-censored -
// two bits per output, at most 4^8 - 1, exact in a double.  Records stay 16-byte multiples: with an even n_obs the pad word
// they already have holds the flags, with an odd n_obs a record grows by 16 bytes.  Sentinel records hold 0.
#pragma once

namespace smc {

constexpr int kCensorNone = 0, kCensorLeft = 1, kCensorRight = 2;      // c_k; the interface's flags are 0, -1, +1
__host__ __device__ constexpr inline int obs_rec_words_censor(int n_obs) { return (3 + n_obs) & ~1; }

}  // namespace smc

#if defined(SMC_USER_CENSOR)   /* the device part; not the marker csrc/strip_censor.awk looks for: this file is embedded whole */
namespace smc_cens {
// x = -log Phi(z) >= 0, the excess of a censored term over its floor 0: accurate in both tails and never negative in floating
// point.  z > 0: Phi = 1 - erfc(z / sqrt 2) / 2 with erfc / 2 in [0, 1/2), so log1p's argument lies in (-1/2, 0] and x >= 0;
// x = 0 exactly once erfc underflows (z >= 40).  z <= 0: Phi = exp(-z^2 / 2) erfcx(-z / sqrt 2) / 2 with erfcx <= 1 there, so
// x >= log 2; finite out to |z| = 1e154.  NaN for NaN.
// NOT inlined, for noise_half_log1p's reason (user_obs_args.h): the attempt loop must not pay for the registers of erfc / erfcx.
__device__ __attribute__((noinline)) double censor_excess(double z) {
    const double y = z * 0.70710678118654752440;
    if (z > 0.0) return -log1p(-0.5 * erfc(y));
    const double half = 0.5 * (z * z);
    const double lg = log(0.5 * erfcx(-y));
    return half - lg;
}
}  // namespace smc_cens
#endif
