// pointwise_reduce.h -- the arithmetic of the per-cell statistics of smc_user_pointwise_summary (include/smc_hip.h; DESIGN.md
// 4.16) that must agree between blocks and ranks: what a thread adds, how a block's partials are joined, and how the statistics
// of two disjoint blocks of particles merge (user_models.pointwise_merge is the same in NumPy).  Functions of built-in types
// only, so that a stand-alone C++ program runs them on the CPU (tests/hostcheck/pointwise_reduce_hostcheck.cpp).
//
// A cell's terms are l_0 .. l_(n-1); NaN = the particle has no term there (failed solve), -inf counts.  With T = kPwThreads:
//   thread t adds the pairs (l_2i, l_2i+1), i = t, t + T, t + 2T, ... (one 16-byte load each) in index order into its partial; the
//   partials are joined by the fixed tree s[i] = join(s[i], s[i + w]), w = T/2, T/4, .. 1.  The order depends on n alone: a
//   repeated call returns the same bits.
//   pass 1: count, max, sum      -> mean = sum / count
//   pass 2: sum exp(l - max), sum (l - mean)^2
#pragma once

#include <math.h>

#if defined(__HIPCC__)
#define SMC_PW_HD __host__ __device__
#else
#define SMC_PW_HD
#endif

namespace smc_pw {

constexpr int kPwThreads = 512;

struct Pass1 {
    double n, max, sum;      // max of nothing: -inf, as the identity of the join
};
struct Pass2 {
    double sum_exp, m2;
};
// the raw statistics of a block of particles, as user_models.pointwise_stats defines them
struct Stats {
    double n, max, sum_exp, mean, m2;
};

SMC_PW_HD inline double neg_inf() { return -HUGE_VAL; }
SMC_PW_HD inline double quiet_nan() { return HUGE_VAL - HUGE_VAL; }

SMC_PW_HD inline Pass1 pass1_zero() { return Pass1{0.0, neg_inf(), 0.0}; }
SMC_PW_HD inline void pass1_add(Pass1 &a, double v) {
    if (v == v) {      // NaN: no term
        a.n += 1.0;
        a.max = v > a.max ? v : a.max;
        a.sum += v;
    }
}
SMC_PW_HD inline Pass1 pass1_join(const Pass1 &a, const Pass1 &b) { return Pass1{a.n + b.n, b.max > a.max ? b.max : a.max, a.sum + b.sum}; }

SMC_PW_HD inline Pass2 pass2_zero() { return Pass2{0.0, 0.0}; }
// max = -inf (every term -inf) gives exp(NaN): sum_exp NaN, as NumPy's expression does; a -inf term under a finite max adds 0
SMC_PW_HD inline void pass2_add(Pass2 &a, double v, double max, double mean) {
    if (v == v) {
        a.sum_exp += exp(v - max);
        const double d = v - mean;
        a.m2 += d * d;
    }
}
SMC_PW_HD inline Pass2 pass2_join(const Pass2 &a, const Pass2 &b) { return Pass2{a.sum_exp + b.sum_exp, a.m2 + b.m2}; }

// the fixed tree over kPwThreads partials, as one thread after the other would run it
template <class T, class Join>
SMC_PW_HD inline T tree(T *s, Join join) {
    for (int w = kPwThreads / 2; w > 0; w >>= 1)
        for (int i = 0; i < w; ++i) s[i] = join(s[i], s[i + w]);
    return s[0];
}

// a cell's statistics from its terms: n = 0 gives NaN in everything but n
SMC_PW_HD inline Stats finish(const Pass1 &p1, const Pass2 &p2) {
    if (p1.n == 0.0) return Stats{0.0, quiet_nan(), quiet_nan(), quiet_nan(), quiet_nan()};
    return Stats{p1.n, p1.max, p2.sum_exp, p1.sum / p1.n, p2.m2};
}
// The whole rule on one processor: what a block of kPwThreads threads computes for v[0 .. n), in its order.
inline Stats cell_stats(const double *v, long long n) {
    static thread_local Pass1 s1[kPwThreads];
    static thread_local Pass2 s2[kPwThreads];
    for (int t = 0; t < kPwThreads; ++t) {
        s1[t] = pass1_zero();
        for (long long i = 2 * t; i < n; i += 2 * kPwThreads) {
            pass1_add(s1[t], v[i]);
            if (i + 1 < n) pass1_add(s1[t], v[i + 1]);
        }
    }
    const Pass1 p1 = tree(s1, pass1_join);
    if (p1.n == 0.0) return finish(p1, pass2_zero());
    const double mean = p1.sum / p1.n;
    for (int t = 0; t < kPwThreads; ++t) {
        s2[t] = pass2_zero();
        for (long long i = 2 * t; i < n; i += 2 * kPwThreads) {
            pass2_add(s2[t], v[i], p1.max, mean);
            if (i + 1 < n) pass2_add(s2[t], v[i + 1], p1.max, mean);
        }
    }
    return finish(p1, tree(s2, pass2_join));
}

// Two disjoint blocks a, b of particles into a + b (a first).  max / sum_exp by rescaling to the common max: a block whose max
// is -inf under a finite common max adds 0 (its own sum_exp is NaN); mean / m2 by Chan's update; a -inf anywhere makes the mean
// -inf and m2 NaN, as the expressions of the whole give.  An empty block changes nothing.
SMC_PW_HD inline double rescaled(double sum_exp, double max, double common) {
    if (max == common) return sum_exp;
    if (max == neg_inf()) return 0.0;
    return sum_exp * exp(max - common);
}
SMC_PW_HD inline Stats merge(const Stats &a, const Stats &b) {
    if (b.n == 0.0) return a;
    if (a.n == 0.0) return b;
    Stats r;
    r.n = a.n + b.n;
    r.max = b.max > a.max ? b.max : a.max;
    r.sum_exp = rescaled(a.sum_exp, a.max, r.max) + rescaled(b.sum_exp, b.max, r.max);
    if (a.mean == neg_inf() || b.mean == neg_inf()) {
        r.mean = neg_inf();
        r.m2 = quiet_nan();
        return r;
    }
    const double delta = b.mean - a.mean;
    r.mean = a.mean + delta * (b.n / r.n);
    r.m2 = (a.m2 + b.m2) + (delta * delta) * (a.n * b.n / r.n);
    return r;
}

}  // namespace smc_pw
