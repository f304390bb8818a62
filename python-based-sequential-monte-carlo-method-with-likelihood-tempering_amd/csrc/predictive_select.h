// predictive_select.h -- the host-checkable core of the exact selection behind smc_user_predict_summary (include/smc_hip.h):
// the order-preserving 64-bit key of a double, the rank rule of the quantiles and one refinement step of the radix select.
// Plain C++ (built-in types only): predictive_kernels.hip runs it on the device, tests/hostcheck/predictive_select_hostcheck.cpp
// on the host, where sanitizers can watch it.
//
// Radix select, most significant digit first: a rank r among m keys is followed through kSelPasses digits of kSelBits bits.
// After pass k the first k digits of the wanted key are known (its "prefix"), and r has become the rank among the keys that
// share that prefix.  A pass counts, for every prefix still followed, how many keys with that prefix have each value of the next
// digit (a histogram of kSelBins bins); select_step then finds the bin the rank falls into.
#pragma once

#if defined(__HIPCC__) || defined(__HIPCC_RTC__)
#define SMC_SEL_HD __host__ __device__
#else
#define SMC_SEL_HD
#endif

namespace smc_sel {

typedef unsigned long long u64;

constexpr int kSelBits = 8;
constexpr int kSelBins = 1 << kSelBits;
constexpr int kSelPasses = 64 / kSelBits;
constexpr int kMaxProbs = 16;
constexpr int kMaxRanks = 2 * kMaxProbs;          // floor and ceil rank of every probability
constexpr u64 kNanKey = ~0ull;                    // what is not finite: sorts last, is never counted

SMC_SEL_HD inline u64 bits_of(double x) {
    union { double d; u64 u; } c;
    c.d = x;
    return c.u;
}
SMC_SEL_HD inline double double_of(u64 u) {
    union { double d; u64 u; } c;
    c.u = u;
    return c.d;
}

// a < b as doubles  <=>  key(a) < key(b) as unsigned integers (with -0 just below +0); NaN and +-inf give kNanKey.
// No finite double maps to kNanKey: that would be the bit pattern 0x7fff..., a NaN.
SMC_SEL_HD inline u64 key_of(double x) {
    const u64 b = bits_of(x);
    if ((b & 0x7ff0000000000000ull) == 0x7ff0000000000000ull) return kNanKey;
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
SMC_SEL_HD inline double value_of(u64 key) {
    return double_of((key >> 63) ? (key & 0x7fffffffffffffffull) : ~key);
}

// digit `pass` (0 = most significant) of a key, and the digits before it
SMC_SEL_HD inline unsigned digit_of(u64 key, int pass) { return (unsigned)(key >> (64 - kSelBits * (pass + 1))) & (kSelBins - 1); }
SMC_SEL_HD inline u64 prefix_of(u64 key, int pass) { return pass == 0 ? 0ull : key >> (64 - kSelBits * pass); }

// ranks of probability q among m >= 1 sorted values: floor and ceil of (m - 1) q - the elements that
// np.quantile(method="lower" / "higher") picks; *frac is the linear rule's weight of the upper one
SMC_SEL_HD inline void quantile_ranks(long long m, double q, long long *lo, long long *hi, double *frac) {
    const double pos = (double)(m - 1) * q;
    long long l = (long long)pos;          // pos >= 0: truncation is floor
    if (l > m - 1) l = m - 1;
    long long h = ((double)l < pos) ? l + 1 : l;
    if (h > m - 1) h = m - 1;
    *lo = l;
    *hi = h;
    *frac = pos - (double)l;
}

// one refinement: hist[kSelBins] counts the next digit of the keys under the rank's prefix; returns that digit for rank *r
// (0-based among those keys) and leaves in *r the rank among the keys of that bin.  The counts must add up to more than *r.
SMC_SEL_HD inline unsigned select_step(const unsigned *hist, u64 *r) {
    u64 below = 0;
    unsigned d = 0;
    for (; d < (unsigned)kSelBins - 1; ++d) {
        const u64 h = hist[d];
        if (below + h > *r) break;
        below += h;
    }
    *r -= below;
    return d;
}

}  // namespace smc_sel
