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
#pragma once

namespace smc {

constexpr int kUserMaxObs = 8;        // SMC_USER_MAX_OBS
constexpr int kObsHdrMe = 8;

__host__ __device__ constexpr inline int obs_rec_words(int n_obs) { return (2 + n_obs) & ~1; }      // 16-byte records
__host__ __device__ constexpr inline int obs_table_at(int n_ex) { return (kObsHdrMe + 2 * n_ex + 1) & ~1; }

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
constexpr int kRec = smc::obs_rec_words(kObs);
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
}  // namespace smc_obs
#endif
