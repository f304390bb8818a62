// count_draw.h -- one replicated count observation on the Philox stream (include/smc_hip.h: COUNT OBSERVATIONS; DESIGN.md
// 4.17): an exact Poisson / gamma-mixed Poisson draw keyed by (seed, global particle, tag, global cell), so that a value does not
// depend on the launch geometry, the grouping of experiments or the number of ranks.  smc_user_predict_summary(noise = 2) takes
// it as the replicated value of a count cell (tag 0x505245), smc_user_pointwise_summary_opt as the replicate the observation is
// ranked against (tag 0x504954).  tests/count_draw_reference.py is the same in NumPy, decision for decision.
//
// Host/device portable: functions of built-in types over philox.h.  A stand-alone C++ program compiles it with __HIPCC_RTC__,
// __host__ and __device__ defined (philox.h's guard; tests/hostcheck/count_draw_hostcheck.cpp).
//
// The uniform supply of one draw: stream = tag << 32 | cell, blocks 1, 2, .. 254 of philox_block(seed, g, stream, block) in
// order.  Block 0 is never opened - under the predictive tag it is the cell's Gaussian z.  A uniform takes the next unused half
// of the open block (u01_from(x, y), then u01_from(z, w)) and opens the next block when none is left; a normal always opens a
// fresh block and uses all of it, in pred_keys_kernel's expression - an unused half is dropped.  A draw that would open block
// 255 gives NaN; every loop below ends with it at the latest.
//
// Arithmetic: no contraction, IEEE division and square root; every decision is a comparison of doubles formed in the order
// written here.  The heavy pieces - Box-Muller's log and cos, PTRS's lgamma bound, the gamma's pow - are NOT inlined, for
// noise_half_log1p's reason (user_obs_args.h): the callers' tiles must not pay for their registers.  They are leaves; the
// rejection loops around them are inlined into the kernel, because on gfx950 a function that itself calls has to keep its return
// address and callee-saved registers in scratch (measured: one out-of-line draw costs 68 B of scratch per lane and 248 VGPRs,
// this arrangement none and 137 / 175).
#pragma once

#include "philox.h"

#if !defined(__HIPCC__)
#include <math.h>
#endif

namespace smc_draw {

constexpr int kGaussian = 0, kPoisson = 1, kNegBin = 2;      // user_count.h's families
constexpr unsigned kLastBlock = 254u;
constexpr unsigned long long kTagPredict = 0x505245ull, kTagPit = 0x504954ull;

struct Supply {
    unsigned long long seed, g, stream;
    unsigned block;      // the last block opened; 0: none yet
    int left;            // unused halves of it
    bool dry;            // block 255 was asked for
    smc::u32x4 q;
};

__host__ __device__ inline Supply supply(unsigned long long seed, unsigned long long g, unsigned long long tag, unsigned long long cell) {
    Supply s;
    s.seed = seed;
    s.g = g;
    s.stream = (tag << 32) | (cell & 0xFFFFFFFFull);
    s.block = 0u;
    s.left = 0;
    s.dry = false;
    s.q = smc::u32x4{0u, 0u, 0u, 0u};
    return s;
}

__host__ __device__ inline bool open_block(Supply &s) {
    if (s.block >= kLastBlock) {
        s.dry = true;
        s.left = 0;
        return false;
    }
    s.block += 1u;
    s.q = smc::philox_block(s.seed, s.g, s.stream, s.block);
    s.left = 2;
    return true;
}

// in [0, 1); 0.5 from a dry supply (the caller looks at s.dry)
__host__ __device__ inline double uniform(Supply &s) {
    if (s.left == 0 && !open_block(s)) return 0.5;
    const double u = s.left == 2 ? smc::u01_from(s.q.x, s.q.y) : smc::u01_from(s.q.z, s.q.w);
    s.left -= 1;
    return u;
}

// an out-of-line leaf: no call inside, so no stack
#define SMC_DRAW_LEAF static __host__ __device__ __attribute__((noinline))

SMC_DRAW_LEAF double box_muller(double u1, double u2) {
#pragma clang fp contract(off)
    return sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
}
// The right-hand side of PTRS's last test, the log of the Poisson probability of k: -lam + k log lam - lgamma(k + 1).  Its terms
// are of the size lam log lam, so the difference is good to about lam log lam 2^-52 only: 1e-9 at lam = 3e5, but 16 at 4e15,
// where the test would be decided by the last bit of lgamma (a device and a C library that differ there then draw different
// counts - met on an MI355X against glibc).  From lam = 2^18 on the same number is formed without the large
// terms, with Stirling's series for lgamma(k + 1) (k > 2^17 there: the first term left out, 1 / (360 k^3), is below 1e-17):
//   -k (d - log1p(d)) - log(2 pi k) / 2 - 1 / (12 k),   d = (lam - k) / k
SMC_DRAW_LEAF double ptrs_bound(double lam, double k) {
#pragma clang fp contract(off)
    if (lam >= 262144.0) {
        const double d = (lam - k) / k;
        return -(k * (d - log1p(d))) - 0.5 * log(6.283185307179586 * k) - 1.0 / (12.0 * k);
    }
    return -lam + k * log(lam) - lgamma(k + 1.0);
}
SMC_DRAW_LEAF double gamma_boost(double u0, double shape) {
#pragma clang fp contract(off)
    return pow(u0, 1.0 / shape);
}

__host__ __device__ inline double normal(Supply &s) {
#pragma clang fp contract(off)
    if (!open_block(s)) return 0.0;
    s.left = 0;
    const double u1 = 1.0 - smc::u01_from(s.q.x, s.q.y), u2 = smc::u01_from(s.q.z, s.q.w);
    return box_muller(u1, u2);
}

// Poisson(lam): inversion below 10 (one uniform), Hoermann's PTRS (1993) from 10 on (two uniforms a trial)
__host__ __device__ inline double poisson(Supply &s, double lam) {
#pragma clang fp contract(off)
    const double nan = __builtin_nan(""), inf = __builtin_huge_val();
    if (!(lam >= 0.0) || lam == inf || lam >= 4503599627370496.0) return nan;
    if (lam == 0.0) return 0.0;
    if (lam < 10.0) {
        const double u = uniform(s);
        if (s.dry) return nan;
        double p = exp(-lam), c = p, k = 0.0;
        while (u > c && k < 128.0) {
            k += 1.0;
            p *= lam / k;
            c += p;
        }
        return k;
    }
    const double slam = sqrt(lam);
    const double b = 0.931 + 2.53 * slam;
    const double a = -0.059 + 0.02483 * b;
    const double invalpha = 1.1239 + 1.1328 / (b - 3.4);
    const double vr = 0.9277 - 3.6224 / (b - 2.0);
    for (;;) {
        const double U = uniform(s) - 0.5;
        const double V = uniform(s);
        if (s.dry) return nan;
        const double us = 0.5 - fabs(U);
        if (us == 0.0 || V == 0.0) continue;
        const double k = floor((2.0 * a / us + b) * U + lam + 0.43);
        if (us >= 0.07 && V <= vr) return k;
        if (k < 0.0 || (us < 0.013 && V > us)) continue;
        const double lhs = log(V) + log(invalpha) - log(a / (us * us) + b);
        if (lhs <= ptrs_bound(lam, k)) return k;
    }
}

// Gamma(shape, 1), Marsaglia & Tsang (2000); shape > 0 finite.  NaN from a dry supply.
__host__ __device__ inline double gamma_mt(Supply &s, double shape) {
#pragma clang fp contract(off)
    const double nan = __builtin_nan("");
    double boost = 1.0;
    if (shape < 1.0) {
        const double u0 = uniform(s);
        if (s.dry) return nan;
        boost = gamma_boost(u0, shape);
        shape += 1.0;
    }
    const double d = shape - 1.0 / 3.0;
    const double c = 1.0 / sqrt(9.0 * d);
    for (;;) {
        const double x = normal(s);
        if (s.dry) return nan;
        double v = 1.0 + c * x;
        if (v <= 0.0) continue;
        v = v * v * v;
        const double u = uniform(s);
        if (s.dry) return nan;
        const double x2 = x * x;
        if (u < 1.0 - 0.0331 * (x2 * x2) || (u > 0.0 && log(u) < 0.5 * x2 + d * (1.0 - v + log(v)))) return d * v * boost;
    }
}

// The draw on an open supply: the count with mean mu - Poisson (b is not read), or negative binomial with variance
// mu + (b mu)^2 as Poisson(mu b^2 G), G ~ Gamma(1 / b^2, 1).  NaN: a mean that is NaN, negative or infinite (before anything is
// drawn), b not finite and > 0 on a negative-binomial output (noise_valid's rule: the particle is invalid), lam >= 2^52, a dry
// supply.
__host__ __device__ inline double draw_on(Supply &s, int family, double mu, double b) {
#pragma clang fp contract(off)
    const double nan = __builtin_nan(""), inf = __builtin_huge_val();
    if (!(mu >= 0.0) || mu == inf) return nan;
    if (family != kNegBin) return poisson(s, mu);
    if (!(b > 0.0) || b == inf) return nan;
    const double b2 = b * b;
    const double G = gamma_mt(s, 1.0 / b2);
    if (s.dry) return nan;
    return poisson(s, mu * (b2 * G));
}

static __host__ __device__ inline double count_draw(int family, double mu, double b, unsigned long long seed, unsigned long long g,
                                                                       unsigned long long tag, unsigned long long cell) {
    Supply s = supply(seed, g, tag, cell);
    return draw_on(s, family, mu, b);
}

}  // namespace smc_draw
