// user_obs_args.h -- the data side of a user model set through smc_set_model_user3 (include/smc_hip.h): n_obs outputs per
// data time, NaN for a value that was not measured, rows that end early, and the prediction kernel.  Like sweep_args.h this
// file is read by the library and handed to hiprtc as an in-memory header (built-in types only, no #include); the device part
// is compiled only into a multi-output source (SMC_USER_NOBS defined).
//
// The kernel's LDS, after the four waves' item pools (kPoolWords = 2 NS + 6 words of 64 lanes each), holds an image the host
// builds once (user_model.hip: build_obs_image):
//   [0, 8)                     1 / s_k, the inverse relative scale of output k (obs_scale; 1 past n_obs)
//   [8, 8 + n_ex)              m_e, the number of finite observations of experiment e (a double)
//   [8 + n_ex, 8 + 2 n_ex)     the sum of log s_k over those observations
//   [obs_table_at(n_ex), ...)  per experiment n_t + 1 records of obs_rec_words(n_obs) doubles: (t_i, obs_i0 .. obs_i(n_obs-1),
//                              zero padding) for the row's n_t_e finite times, then (+inf, t[e][n_t_e - 1], ...) up to and
//                              including record n_t - the +inf sentinel of solve_sched's dense-output loop at the row's own end
//                              and, in the last record, the row's end time.
// A model with a NOISE MODEL (smc_set_model_user4; the source is compiled with SMC_USER_NOISE 1) appends to the table, at
// obs_noise_at(n_ex, n_t, n_obs), kNoiseHdr + 8 n_ex words:
//   [0, 8)    add_index[k] as a double (-1: fixed)     [8, 16)   add_fixed[k]
//   [16, 24)  prop_index[k] (-1: fixed)                [24, 32)  prop_fixed[k] (0 without a proportional part)
//   [32, 40)  s_k                                      [40 + 8 e + k]  m_ek, the finite observations of output k in experiment e
#pragma once

namespace smc {

constexpr int kUserMaxObs = 8;        // SMC_USER_MAX_OBS
constexpr int kObsHdrMe = 8;

__host__ __device__ constexpr inline int obs_rec_words(int n_obs) { return (2 + n_obs) & ~1; }      // 16-byte records
__host__ __device__ constexpr inline int obs_table_at(int n_ex) { return (kObsHdrMe + 2 * n_ex + 1) & ~1; }
constexpr int kNoiseHdr = 40;
__host__ __device__ constexpr inline int obs_noise_at(int n_ex, int n_t, int n_obs) { return obs_table_at(n_ex) + n_ex * (n_t + 1) * obs_rec_words(n_obs); }
__host__ __device__ constexpr inline int obs_noise_words(int n_ex) { return kNoiseHdr + 8 * n_ex; }

// The noise model of smc_set_model_user4 as the library's own kernels take it (user_finish_noise_kernel, pred_keys_kernel);
// the run-time compiled kernels read the same numbers from the image.
struct UserNoise {
    int add_index[kUserMaxObs], prop_index[kUserMaxObs];      // a parameter number, or -1: the fixed value
    double add_fixed[kUserMaxObs], prop_fixed[kUserMaxObs];
    double scale[kUserMaxObs];                                // s_k
    int prop;                                                 // 1: with a proportional part (SMC_USER_NOISE_PROP 1)
};

// The second argument block of the multi-output solve and prediction kernels.
struct UserObsArgs {
    const double *img;          // the LDS image above, in device memory
    int img_len;                // its length in doubles
    double *pred;               // prediction kernel: [((p * n_ex + e) * n_t + i) * n_obs + k]; nullptr in a sweep
};

}  // namespace smc

#ifdef SMC_USER_NOBS
namespace smc_obs {
constexpr int kObs = SMC_USER_NOBS;
#ifdef SMC_USER_CENSOR
constexpr int kRec = smc::obs_rec_words_censor(kObs);      // user_censor.h: the record's last word holds its outputs' flags
#else  // SMC_USER_CENSOR
constexpr int kRec = smc::obs_rec_words(kObs);
#endif  // SMC_USER_CENSOR
// one data time: x = t, y[k] = obs_k; from the row's end on x = +inf and y[0] = the row's end time
struct alignas(16) Rec {
    double x;
    double y[kRec - 1];
};
constexpr int kHdrAt = 4 * (2 * SMC_USER_NS + 6) * 64;
__device__ __forceinline__ double *lds() {
    extern __shared__ double s_pool_all[];
    return s_pool_all + kHdrAt;
}
__device__ __forceinline__ double me(int e) { return lds()[smc::kObsHdrMe + e]; }
__device__ __forceinline__ double sum_log_scale(int e, int n_ex) { return lds()[smc::kObsHdrMe + n_ex + e]; }
__device__ __forceinline__ const Rec *table(int n_ex) { return reinterpret_cast<const Rec *>(lds() + smc::obs_table_at(n_ex)); }

// the model's outputs at (t, y): smc_user_obs_vec, or smc_user_obs for a one-output source that defines only that
__device__ __forceinline__ void model_obs(double t, const double *y, const double *th, const double *c, double *out) {
#if SMC_USER_HAS_OBS_VEC
    smc_user_ieee::smc_user_obs_vec(t, y, th, c, out);
#else
    out[0] = smc_user_ieee::smc_user_obs(t, y, th, c);
#endif
}

// One output time: ONE call of the model's outputs, the masked and scaled residuals added to sr2 and, in the prediction
// kernel, the outputs written to pred (which then moves on to the next time).  FUSE: sr2 + r * r as one contracted
// expression (the RK45 kernel's -ffp-contract=on), else rounded twice (the BDF kernel is compiled without contraction).
// With s_k = 1 and no NaN this is the one-output kernels' `sr2 += r * r` bit for bit.
template <bool PRED, bool FUSE>
__device__ __forceinline__ void emit(double &sr2, double *&pred, const double *yy, const double *th, const double *c, double t_out,
                                     const double *obs) {
    double m[kObs];
    model_obs(t_out, yy, th, c, m);
    const double *inv_s = lds();
#pragma unroll
    for (int k = 0; k < kObs; ++k) {
        const double r = (obs[k] - m[k]) * inv_s[k];
        if (FUSE) {
            sr2 = (obs[k] == obs[k]) ? sr2 + r * r : sr2;        // NaN: not measured
        } else {
            const double r2 = r * r;
            sr2 = (obs[k] == obs[k]) ? sr2 + r2 : sr2;
        }
    }
    if (PRED) {
#pragma unroll
        for (int k = 0; k < kObs; ++k) pred[k] = m[k];
        pred += kObs;
    }
}

#if defined(SMC_USER_NOISE) && SMC_USER_NOISE
// ---- the noise model of smc_set_model_user4: sd_ik^2 = (a_k s_k)^2 + (b_k f_ik)^2, a_k and b_k a parameter or a fixed number ----
// An item accumulates the EXCESS over the floor log(a_k s_k) every observation has before it is served:
//   x_ik = 1/2 log1p((b_k f_ik / (a_k s_k))^2) + r_ik^2 / (2 sd_ik^2) >= 0,
// so the sum only grows and the early-rejection bound stays exact.  Per item: w_k = 1 / (2 (a_k s_k)^2) and, with a
// proportional part (SMC_USER_NOISE_PROP 1), q_k = (b_k / (a_k s_k))^2; then u = q_k f^2 and x = 1/2 log1p(u) + r^2 w_k / (1 + u):
// one log1p and one division per observed value.  Without it x = r^2 w_k and neither is compiled.
constexpr int kProp = SMC_USER_NOISE_PROP;
#ifdef SMC_USER_COUNT
// Count observations (user_count.h): output k is Gaussian (family 0: everything as without counts), Poisson (1) or negative
// binomial (2).  The list is the source's smc_user_obs_family, handed over by the library as SMC_USER_FAMILY: compile-time
// constants, so that the unrolled loops over k below keep, per output, only its family's code.  A count output's additive entry
// is fixed 1 and its scale 1: w_k is not used and q_k = b_k^2.
__device__ constexpr int family_of(int k) {
    constexpr int f[] = SMC_USER_FAMILY;
    static_assert(sizeof(f) / sizeof(f[0]) == kObs, "smc_user_obs_family: one entry per output");
    return f[k];
}
#endif  // SMC_USER_COUNT
struct Noise {
    double w[kObs];
#if SMC_USER_NOISE_PROP
    double q[kObs];
#endif
};
#ifdef SMC_USER_CENSOR
__device__ __forceinline__ const double *noise_lds(int n_ex, int n_t) { return lds() + smc::obs_table_at(n_ex) + n_ex * (n_t + 1) * kRec; }
#else  // SMC_USER_CENSOR
__device__ __forceinline__ const double *noise_lds(int n_ex, int n_t) { return lds() + smc::obs_noise_at(n_ex, n_t, kObs); }
#endif  // SMC_USER_CENSOR
__device__ __forceinline__ double mek(int e, int k, int n_ex, int n_t) { return noise_lds(n_ex, n_t)[smc::kNoiseHdr + 8 * e + k]; }
// parameter number idx (as a double) of th, or fixed: selects, so that th stays in registers
__device__ __forceinline__ double noise_pick(const double *th, double idx, double fixed) {
    double v = fixed;
#pragma unroll
    for (int c = 0; c < SMC_USER_DIM; ++c) v = (idx == (double)c) ? th[c] : v;
    return v;
}
__device__ __forceinline__ double noise_add(const double *th, int k, int n_ex, int n_t) {
    const double *nz = noise_lds(n_ex, n_t);
    return noise_pick(th, nz[k], nz[8 + k]);
}
__device__ __forceinline__ double noise_prop(const double *th, int k, int n_ex, int n_t) {
    const double *nz = noise_lds(n_ex, n_t);
    return noise_pick(th, nz[16 + k], nz[24 + k]);
}
__device__ __forceinline__ double noise_scale(int k, int n_ex, int n_t) { return noise_lds(n_ex, n_t)[32 + k]; }
// every a_k > 0 and every b_k >= 0 (NaN: no); else logL = -inf
__device__ __forceinline__ bool noise_valid(const double *th, int n_ex, int n_t) {
    bool ok = true;
#pragma unroll
    for (int k = 0; k < kObs; ++k) ok = ok && noise_add(th, k, n_ex, n_t) > 0.0 && (!kProp || noise_prop(th, k, n_ex, n_t) >= 0.0);
#ifdef SMC_USER_COUNT
    // ... and b_k > 0 on a negative-binomial output (a source with one is compiled with the proportional part)
#pragma unroll
    for (int k = 0; k < kObs; ++k)
        if (family_of(k) == smc_cnt::kNegBin) ok = ok && noise_prop(th, k, n_ex, n_t) > 0.0;
#endif  // SMC_USER_COUNT
    return ok;
}
// the item's weights from its particle's parameters; zeros (no excess at all) for parameters that make logL -inf
__device__ __forceinline__ void noise_weights(Noise &nz, const double *th, int n_ex, int n_t) {
    const bool ok = noise_valid(th, n_ex, n_t);
#pragma unroll
    for (int k = 0; k < kObs; ++k) {
        const double as = noise_add(th, k, n_ex, n_t) * noise_scale(k, n_ex, n_t);
        const double as2 = as * as;
        nz.w[k] = ok ? 1.0 / (2.0 * as2) : 0.0;
#if SMC_USER_NOISE_PROP
        const double b = noise_prop(th, k, n_ex, n_t);
        const double b2 = b * b;
        nz.q[k] = ok ? b2 / as2 : 0.0;
#endif
    }
}
// 1/2 log1p(u), NOT inlined: inlined into the output branch of the attempt its registers push the RK45 kernel's bulk attempt loop
// into scratch (three reloads per attempt at four waves per SIMD); behind a call the loop is as free of scratch as without a noise
// model.  A call per observed value, in the rare branch, next to the log1p itself.
#if SMC_USER_NOISE_PROP
__device__ __attribute__((noinline)) double noise_half_log1p(double u) { return 0.5 * log1p(u); }
#endif
#ifdef SMC_USER_CENSOR
// A censored value (user_censor.h; flag c = 1: the true value is <= obs, 2: >= obs): its term is log Phi(z), z = (obs - f) / sd
// from the left and (f - obs) / sd from the right, with 1 / sd^2 = 2 w_k / (1 + q_k f^2) from the item's weights.  Floor 0, excess
// x = -log Phi(z) >= 0: the item's sum still only grows.  r = obs - f.  A z that is not finite (f NaN or infinite) gives NaN, the
// route a failed output takes; zeroed weights (parameters that make logL -inf) give z = 0 and a finite x that is never used.
template <bool FUSE>
__device__ __forceinline__ double censor_term(int c, double r, double f, const Noise &nz, int k) {
    double z;
#if SMC_USER_NOISE_PROP
    if (FUSE) {
        z = (c == smc::kCensorLeft ? r : -r) * sqrt(2.0 * nz.w[k] / (1.0 + nz.q[k] * (f * f)));
    } else {
        const double f2 = f * f;
        const double u = nz.q[k] * f2;
        const double den = 1.0 + u;
        const double w2 = 2.0 * nz.w[k];
        const double iv = w2 / den;
        const double inv_sd = sqrt(iv);
        const double rs = (c == smc::kCensorLeft) ? r : -r;
        z = rs * inv_sd;
    }
#else
    const double w2 = 2.0 * nz.w[k];
    const double inv_sd = sqrt(w2);
    const double rs = (c == smc::kCensorLeft) ? r : -r;
    z = rs * inv_sd;
    (void)f;
#endif
    return (fabs(z) < __longlong_as_double(0x7ff0000000000000LL)) ? smc_cens::censor_excess(z) : __longlong_as_double(0x7ff8000000000000LL);
}
#endif  // SMC_USER_CENSOR
// emit under a noise model: x_ik added to the item's sum.  FUSE as above: one contracted expression per step where the RK45
// kernel's -ffp-contract=on allows it, every product and sum rounded on its own in the BDF kernel.
template <bool PRED, bool FUSE>
__device__ __forceinline__ void emit_noise(double &sx, double *&pred, const Noise &nz, const double *yy, const double *th, const double *c,
                                           double t_out, const double *obs) {
    double m[kObs];
    model_obs(t_out, yy, th, c, m);
#ifdef SMC_USER_CENSOR
    const int flags = (int)obs[kRec - 2];       // the record's last word, read with the record (obs = its y)
#endif  // SMC_USER_CENSOR
#pragma unroll
    for (int k = 0; k < kObs; ++k) {
        const double r = obs[k] - m[k];
#ifdef SMC_USER_CENSOR
        const int ck = (flags >> (2 * k)) & 3;
        if (ck != 0) {                          // a flag stands on a finite value only (censor_layout)
            sx += censor_term<FUSE>(ck, r, m[k], nz, k);
            continue;
        }
#endif  // SMC_USER_CENSOR
#ifdef SMC_USER_COUNT
        if (family_of(k) != smc_cnt::kGaussian) {      // a count: its excess over the floor, behind a call; no flag stands on it
            if (obs[k] == obs[k]) {
#if SMC_USER_NOISE_PROP
                sx += family_of(k) == smc_cnt::kPoisson ? smc_cnt::poisson_excess(obs[k], m[k]) : smc_cnt::negbin_excess(obs[k], m[k], nz.q[k]);
#else
                sx += smc_cnt::poisson_excess(obs[k], m[k]);
#endif
            }
            continue;
        }
#endif  // SMC_USER_COUNT
#if SMC_USER_NOISE_PROP
        double x;
        if (FUSE) {
            const double u = nz.q[k] * (m[k] * m[k]);
            x = noise_half_log1p(u) + (r * r) * nz.w[k] / (1.0 + u);
        } else {
            const double f2 = m[k] * m[k];
            const double u = nz.q[k] * f2;
            const double r2 = r * r;
            const double rw = r2 * nz.w[k];
            const double den = 1.0 + u;
            const double quad = rw / den;
            const double half = noise_half_log1p(u);
            x = half + quad;
        }
        sx = (obs[k] == obs[k]) ? sx + x : sx;              // NaN: not measured
#else
        if (FUSE) {
            sx = (obs[k] == obs[k]) ? sx + (r * r) * nz.w[k] : sx;
        } else {
            const double r2 = r * r;
            const double x = r2 * nz.w[k];
            sx = (obs[k] == obs[k]) ? sx + x : sx;
        }
#endif
    }
    if (PRED) {
#pragma unroll
        for (int k = 0; k < kObs; ++k) pred[k] = m[k];
        pred += kObs;
    }
}
// The likelihood of a particle from the sums X_e, as user_finish_noise_kernel (user_model.hip) forms it, in its order:
//   lk = sum_e [ (-m_e / 2) log(2 pi) - sum_k m_ek log(a_k s_k) - X_e ].
// floor_of(e): the bracket without X_e.  Used by the early-rejection bound of both kernels.
__device__ __forceinline__ double noise_floor_of(int e, const double *la, int n_ex, int n_t) {
    double c0 = (-0.5 * me(e)) * 1.8378770664093453;
#pragma unroll
    for (int k = 0; k < kObs; ++k) {
        const double term = mek(e, k, n_ex, n_t) * la[k];
        c0 = c0 - term;
    }
#ifdef SMC_USER_COUNT
    c0 = c0 - sum_log_scale(e, n_ex);      // C_e, the Poisson floors of the experiment (user_count.h: the words a noise model does not read)
#endif  // SMC_USER_COUNT
    return c0;
}
#endif
}  // namespace smc_obs
#endif
