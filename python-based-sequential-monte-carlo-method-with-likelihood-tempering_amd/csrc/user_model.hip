// user_model.hip -- SURVEY.md 8(f) N1: the reference is meant to be "modified for your problem" (README.md:4): a user
// writes Micmem_likelihood.py's three ingredients - the ODE right-hand side (:14-15), the initial state and what is
// compared with the data (:17-33) - and keeps the drivers.  Here the same three ingredients are given as HIP device
// functions; they are compiled at run time (hiprtc, gfx950) into the likelihood kernel below and plugged into the
// on-device loop (propose -> solve -> accept) exactly like the two built-in models.
//
// The kernel restates solve_ivp(method="RK45", t_eval=t, rtol, atol) for an NS-dimensional state as SciPy does it
// (scipy/integrate/_ivp: rk.py rk_step / _step_impl, common.py select_initial_step and RMS norm, ivp.py t_eval
// dispatch through the quartic dense output) and the Gaussian log-likelihood of Micmem_likelihood.py:62-73.
// For NS = 1 every operation is in the order of the built-in Michaelis-Menten kernel, so the MM model written as a user
// model reproduces it (tests/test_gpu_user_model.py); for NS > 1 the stage sums are plain left-to-right sums where
// NumPy calls BLAS, so agreement with SciPy is at rounding level per step, not bitwise.
// Scheduling as in the built-in kernel: (experiment, particle) items, persistent lanes that take the next item from a
// global counter when their solve ends; a small built-in kernel then sums the items of a particle into its logL.
#include <hip/hip_runtime.h>
#include <hip/hiprtc.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/smc_hip.h"
#include "smc_internal.h"
#include "solve_sched.h"   // kChunk: the grid is sized in chunks of the shared scheduler
#include "stage_kernels.h" // launch_aos_to_soa (smc_user_predict)
#include "user_censor.h"   // censored observations (smc_set_model_user7)
#include "user_count.h"    // count observations (smc_user_obs_family)
#include "count_floor.h"   // ... and the floor of a Poisson term, host code
#include "user_obs_args.h" // several outputs, missing values, ragged rows, predictions (smc_set_model_user3)
#include "predictive_kernels.h"   // smc_user_predict_summary's kernels
#include "pointwise_kernels.h"    // smc_user_pointwise, smc_user_pointwise_summary

namespace smc {

// solve_sched.h, sweep_args.h, philox.h and reject_bound.h as strings (csrc/Makefile generates the file from the headers
// themselves): hiprtc gets them as in-memory headers, so the run-time compiled kernel is scheduled, and ends its rejection bound,
// by the very code the built-in kernel uses.  The kernels themselves come the same way: user_rk45_kernel.h, user_bdf_kernel.h
// (one integrator per SMC_USER_METHOD_*) and user_cost_scan.h are device code only, appended to the user's text by
// build_source; user_item_ops.h, everything of a kernel that is not an integrator, is the header both of them include
#include "embedded_headers.inc"

// what the user's functions may call (include/smc_hip.h)
// The user's functions are compiled TWICE, in two namespaces that differ in what smc_div(a, b) is (include/smc_hip.h): the
// six-operation division of the built-in kernel, and a / b.  An attempt runs on the first and is repeated on the second
// whenever its error norm is not finite (smc_user::item_attempt) - the built-in kernel's scheme, for a model it does not know.
static const char *kUserPreludeLean = R"SRC(
#include "rk45_math.h"
namespace smc_user_lean {
__device__ __forceinline__ double smc_div(double a, double b) { return smc::lean_div6(a, b); }
)SRC";
static const char *kUserPreludeIeee = R"SRC(
}  // namespace smc_user_lean
namespace smc_user_ieee {
__device__ __forceinline__ double smc_div(double a, double b) { return a / b; }
)SRC";
// method BDF (user_bdf_kernel.h): the user's functions are compiled once, with smc_div(a, b) = a / b
static const char *kUserBdfPrelude = R"SRC(
#include "rk45_math.h"
namespace smc_user_ieee {
__device__ __forceinline__ double smc_div(double a, double b) { return a / b; }
)SRC";

// log-likelihood of Micmem_likelihood.py:62-73 per particle from the per-item sums; counters as in the built-in path
__global__ void __launch_bounds__(256)
user_finish_kernel(const double *__restrict__ theta, int64_t stride, int64_t n, int dim, uint8_t *__restrict__ p0mask,
                   const double *__restrict__ sum_r2, const int *__restrict__ info, int n_ex, const double *__restrict__ me,
                   const double *__restrict__ ls, int est_sigma, double sigma_fixed, double *__restrict__ lk_out,
                   SweepCounters *__restrict__ counters) {
    unsigned long long attempts = 0, failed = 0;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (int64_t)gridDim.x * blockDim.x) {
        const bool masked = p0mask && p0mask[p] == 0;   // proposal reset to the current point: the stored likelihood is used
        const double sigma = est_sigma ? theta[(int64_t)(dim - 1) * stride + p] : sigma_fixed;
        if (!masked && sigma <= 0.0) lk_out[p] = -__longlong_as_double(0x7ff0000000000000LL);   // Micmem_likelihood.py:53-54
        if (!masked && sigma > 0.0) {
            const double s2 = sigma * sigma;
            // per experiment c0 = -m_e / 2 log(2 pi sigma^2) - sum log s_k over its m_e observations: m_e = n_t and 0 for a model
            // of smc_set_model_user / smc_set_model_user2, whose c0 this is bit for bit.  The early-rejection bound of the
            // multi-output kernels (the SMC_USER_NOBS blocks of user_rk45_kernel.h / user_bdf_kernel.h) evaluates the same expression in the same order.
            const double lg = log(2.0 * 3.141592653589793 * s2);
            double lk = 0.0;
            unsigned pf = 0, cancelled = 0;
            for (int e = 0; e < n_ex; ++e) {
                lk += ((-0.5 * me[e]) * lg - ls[e]) - sum_r2[(int64_t)e * n + p] / (2.0 * s2);
                const int fl = info[(int64_t)e * n + p];
                attempts += (unsigned)(fl & 0x1fffffff);
                pf |= (unsigned)(fl >> 30) & 1u;
                cancelled |= (unsigned)(fl >> 29) & 1u;
            }
            failed += pf;
            if (cancelled) {      // a solve stopped because the rejection was certain: logL was never completed - the accept
                lk = __longlong_as_double(0x7ff8000000000000LL);   // kernel sees the flag and keeps p_filt, lk1
                if (p0mask) p0mask[p] = 2;
            }
            lk_out[p] = lk;
        }
    }
    if (failed) atomicAdd(&counters->n_failed, failed);
    if (attempts) atomicAdd(&counters->rk_attempts, attempts);
}

// ... under a noise model (smc_set_model_user4; user_obs_args.h): the items hold the excess sums X_e over the floors,
//   lk = sum_e [ (-m_e / 2) log(2 pi) - sum_k m_ek log(a_k s_k) - X_e ],     -inf if any a_k <= 0 or any b_k < 0.
// me: m_e; mek: [8 e + k].  The early-rejection bound of the run-time compiled kernels (smc_obs::noise_floor_of) evaluates the
// bracket in this order, every product and difference rounded on its own.
__global__ void __launch_bounds__(256)
user_finish_noise_kernel(const double *__restrict__ theta, int64_t stride, int64_t n, uint8_t *__restrict__ p0mask,
                         const double *__restrict__ sum_x, const int *__restrict__ info, int n_ex, int n_obs,
                         const double *__restrict__ me, const double *__restrict__ mek, const UserNoise nz,
                         double *__restrict__ lk_out, SweepCounters *__restrict__ counters, const double *__restrict__ ce = nullptr,
                         unsigned negbin = 0) {
    // ce, negbin: a model with count outputs (user_count.h; nullptr and 0 without) - ce[e] = C_e, the experiment's sum of the
    // Poisson floors c(y), leaves the bracket after the Gaussian floors; bit k of negbin: output k is negative binomial, b_k > 0
    unsigned long long attempts = 0, failed = 0;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (int64_t)gridDim.x * blockDim.x) {
        const bool masked = p0mask && p0mask[p] == 0;
        if (masked) continue;
        double la[kUserMaxObs];
        bool ok = true;
        for (int k = 0; k < n_obs; ++k) {
            const double a = nz.add_index[k] >= 0 ? theta[(int64_t)nz.add_index[k] * stride + p] : nz.add_fixed[k];
            const double b = !nz.prop ? 0.0 : (nz.prop_index[k] >= 0 ? theta[(int64_t)nz.prop_index[k] * stride + p] : nz.prop_fixed[k]);
            ok = ok && a > 0.0 && b >= 0.0 && !(((negbin >> k) & 1u) && !(b > 0.0));
            la[k] = log(a * nz.scale[k]);
        }
        if (!ok) {
            lk_out[p] = -__longlong_as_double(0x7ff0000000000000LL);
            continue;
        }
        double lk = 0.0;
        unsigned pf = 0, cancelled = 0;
        for (int e = 0; e < n_ex; ++e) {
            double c0 = (-0.5 * me[e]) * 1.8378770664093453;      // log(2 pi)
            for (int k = 0; k < n_obs; ++k) {
                const double term = mek[8 * e + k] * la[k];
                c0 = c0 - term;
            }
            if (ce) c0 = c0 - ce[e];
            lk += c0 - sum_x[(int64_t)e * n + p];
            const int fl = info[(int64_t)e * n + p];
            attempts += (unsigned)(fl & 0x1fffffff);
            pf |= (unsigned)(fl >> 30) & 1u;
            cancelled |= (unsigned)(fl >> 29) & 1u;
        }
        failed += pf;
        if (cancelled) {
            lk = __longlong_as_double(0x7ff8000000000000LL);
            if (p0mask) p0mask[p] = 2;
        }
        lk_out[p] = lk;
    }
    if (failed) atomicAdd(&counters->n_failed, failed);
    if (attempts) atomicAdd(&counters->rk_attempts, attempts);
}

// BDF models: the per-item work counters of a sweep summed into four totals (smc_user_sweep_counters); masked proposals
// (not solved: their items may hold an earlier sweep's counts) are left out
__global__ void __launch_bounds__(256)
user_bdf_count_kernel(const uint8_t *__restrict__ p0mask, const unsigned *__restrict__ counts, int64_t n, int n_ex,
                      unsigned long long *__restrict__ totals) {
    __shared__ unsigned long long s[4][256];
    unsigned long long acc[4] = {0, 0, 0, 0};
    const int64_t m = n * n_ex;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x) {
        if (p0mask && p0mask[i % n] == 0) continue;
        for (int k = 0; k < 4; ++k) acc[k] += counts[k * m + i];
    }
    for (int k = 0; k < 4; ++k) s[k][threadIdx.x] = acc[k];
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w)
            for (int k = 0; k < 4; ++k) s[k][threadIdx.x] += s[k][threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x < 4 && s[threadIdx.x][0]) atomicAdd(totals + threadIdx.x, s[threadIdx.x][0]);
}

// The compile-time geometry of a model with inputs (user_input.h): the model's n_cond, n_in inputs, kcap = the power of two >=
// n_knot.  n_in = 0: a model without inputs - its source and its cond rows are what they always were.
// ... and of a model with scheduled events (user_event.h): n_ev, the event capacity, and n_val values per event; the event
// table follows the input table (or the cond numbers).  n_ev = 0: a model without events.
struct UserInputGeom {
    int n_cond = 0, n_in = 0, kcap = 0;
    int n_ev = 0, n_val = 0;
    int in_words() const { return n_in > 0 ? n_cond + kcap + n_in * (2 * kcap + 1) : n_cond; }      // = the offset of the event table
    int ev_words() const { return n_ev > 0 ? n_ev + 1 + n_ev * n_val : 0; }
    int row_words() const { return in_words() + ev_words(); }
    bool tabled() const { return n_in > 0 || n_ev > 0; }      // a cond row holds more than the model's cond numbers
};
// the inputs as a set function receives them (nullptr: none)
struct UserInputs {
    const double *in_t, *in_u;      // n_ex x n_knot, n_ex x n_knot x n_in
    int n_in, n_knot;
};
// ... and the events (nullptr: none)
struct UserEvents {
    const double *ev_t, *ev_v;      // n_ex x n_ev, n_ex x n_ev x n_val (nullptr with n_val = 0)
    int n_ev, n_val;
};
static int knot_capacity(int n_knot) {
    int k = 1;
    while (k < n_knot) k <<= 1;
    return k;
}
// Everything that decides the text hiprtc reads for a source (build_source, user_headers): smc_user_source_spec (include/smc_hip.h)
// after user_source_spec_of has accepted it, n_knot as the knot capacity of geom.  n_obs = 0: the one-output source of
// smc_set_model_user / 2; n_obs >= 1: the multi-output source.  noise: 0 the sigma rule, 1 a noise model, 2 with its proportional
// part; censor: 1 censored observations (user_censor.h) - SMC_USER_CENSOR, records with a flag word.
struct UserSourceSpec {
    int n_states = 0, dim = 0, method = SMC_USER_METHOD_RK45, n_obs = 0;
    int noise = 0, censor = 0;
    UserInputGeom geom{};
};

// What a launch (launch_user_kernel) runs on, and what differs between the data and a group of a design other than the data's:
// the experiments, the blocks per CU of the kernel that runs them, and what the kernel writes per (experiment, particle).
// A plain set of pointers and sizes: whoever filled it owns the allocations (UserModel; DesignGroup and DesignItems).
struct UserLaunchData {
    double *d_img = nullptr;              // the LDS image (nullptr: one-output data the image cannot hold, img_error says why)
    int img_len = 0;
    double *d_cond = nullptr;
    double *d_const = nullptr;            // [2 n_ex]: m_e, then sum log s_k (user_finish_kernel); n_t and 0 for a one-output model
    int n_ex = 0, n_t = 0;
    int blocks_per_cu = 4;   // persistent blocks (4 waves each) per CU: what the compiled kernel's registers and LDS allow
    double *d_sum = nullptr;
    int *d_info = nullptr;
    unsigned *d_bdf_counts = nullptr;          // BDF: per item {accepted steps, Newton iterations, LU factorisations, Jacobians}
};

struct UserModel {
    hipModule_t module = nullptr;
    hipFunction_t fn = nullptr;
    hipFunction_t fn_scan = nullptr;      // smc_user_cost_scan_kernel: only for a source that defines smc_user_cost
    int32_t *d_list = nullptr;            // the two lists of a sweep (n_local entries), their flags and two alternating counter pairs
    uint8_t *d_listed = nullptr;
    unsigned *d_count = nullptr;
    int parity = 0;
    UserLaunchData data;                  // the data, for the sweep kernel (fn); set once by set_model_user_impl
    double *d_t = nullptr, *d_obs = nullptr;      // the data as the one-output sweep kernel reads it; no other kernel does
    int n_cond = 0, est_sigma = 1;
    double sigma_fixed = 0, rtol = 1e-3, atol = 1e-6;
    unsigned long long *d_bdf_totals = nullptr;   // BDF: the sums of d_bdf_counts over the last sweep (user_bdf_count_kernel)
    // smc_set_model_user3 (user_obs_args.h): `multi` models run the multi-output source, whose module also holds the
    // prediction kernel; a model of smc_set_model_user / 2 compiles that source with n_obs = 1 when it first predicts
    bool multi = false;
    int n_obs = 1;
    std::string source;
    std::string img_error;
    hipModule_t module_pred = nullptr;
    hipFunction_t fn_pred = nullptr;
    int blocks_per_cu_pred = 4;
    // the data for the prediction kernel (fn_pred): the same allocations, that kernel's blocks per CU
    UserLaunchData pred_data() const {
        UserLaunchData d = data;
        d.blocks_per_cu = blocks_per_cu_pred;
        return d;
    }
    double *d_pt = nullptr, *d_plk = nullptr, *d_ppred = nullptr;   // smc_user_predict's staging: parameters (AoS + SoA), lk, pred
    int64_t p_cap = 0;
    // smc_user_pointwise / smc_user_pointwise_summary (pointwise_kernels.h): per cell of the data's design its value, what it is and
    // count_floor of a Poisson value, built once with the image; the families; the staging of the host-particle entry point
    double *d_cell_obs = nullptr, *d_cell_floor = nullptr, *d_pll = nullptr;
    int *d_cell_code = nullptr;
    int family[kUserMaxObs] = {0, 0, 0, 0, 0, 0, 0, 0};
    int64_t pll_cap = 0;
    // what a design other than the data's needs again on the host (smc_user_predict_at, smc_user_predict_summary)
    std::vector<double> h_t, h_cond;
    double scale[kUserMaxObs] = {1, 1, 1, 1, 1, 1, 1, 1};
    // smc_set_model_user4: the noise model (user_obs_args.h); d_const then holds m_e, sum log s_k and m_ek [8 n_ex]
    bool noise = false;
    UserNoise nz{};
    // count outputs (user_count.h; the source's smc_user_obs_family): d_const's second n_ex words then hold C_e
    bool count = false;
    unsigned negbin = 0;      // bit k: output k is negative binomial
    // smc_set_model_user5: time-varying inputs (user_input.h).  The table lies behind each experiment's cond row, so d_cond holds
    // rows of spec.geom.row_words() doubles; h_rows keeps the data's rows and design_* the inputs of an explicit design
    // smc_set_model_user6: scheduled events (user_event.h).  Their table follows in the same rows; design_ev_* are the events of
    // an explicit design (smc_user_set_design_events)
    UserSourceSpec spec{};      // what the module was compiled for: n_states, method, the row geometry, ...
    std::vector<double> h_rows, design_t, design_u, design_ev_t, design_ev_v;
    int design_n_ex = 0, design_n_knot = 0, design_ev_n_ex = 0, design_ev_n_ev = 0;
    int cond_stride() const { return spec.geom.tabled() ? spec.geom.row_words() : n_cond; }
};

// an optional ingredient (smc_user_cost, smc_user_jac, smc_user_obs_vec; smc_div): a source that mentions it must define it
static bool mentions(const char *user_source, const char *name) { return strstr(user_source, name) != nullptr; }

// What hiprtc reads for a model: the #define head (sizes, and what the user's text mentions), the prelude(s) with the user's
// text, and the method's kernel file.  n_obs = 0: the one-output source of smc_set_model_user / 2.  n_obs >= 1: the
// multi-output source (smc_set_model_user3) - SMC_USER_NOBS selects the kernel file's multi-output blocks, and the file is
// appended twice: the sweep kernel, then with SMC_USER_PRED 1 the prediction kernel smc_user_predict_kernel.
// geom.n_in > 0 (smc_set_model_user5): SMC_USER_NCOND / NIN / KCAP and user_input.h in front, and smc_input made visible in the
// namespace(s) of the user's text.  A source that calls smc_input without inputs is stopped by an #error that says so.
// geom.n_ev > 0 (smc_set_model_user6): SMC_USER_EVENTS, SMC_USER_EVAT / NEV / NVAL and user_event.h in front, smc_event_value made
// visible to the user's text, and the kernel file with its SMC_USER_EVENTS blocks (k_..._ev).  The event names and a model
// without events, or events and a source without smc_user_event, stop with an #error that says so.
// A source that contains the name smc_user_root has state-triggered events (user_root.h): SMC_USER_ROOTS, and the kernel file
// with its SMC_USER_ROOTS blocks and its SMC_USER_EVENTS blocks (k_..._rt) - without scheduled events SMC_USER_EVENTS is defined
// here with SMC_USER_NO_SCHEDULE, for which user_root.h supplies a table that never holds an event.  Such a source defines
// smc_user_root_dir and smc_user_root_event too, or stops with an #error that says so; the number of event functions and their
// directions are checked by static_asserts of user_root.h.
static bool has_roots(const char *user_source) { return mentions(user_source, "smc_user_root"); }
// The directions of a source's event functions, read from its text: the initialiser list that follows the definition - the
// first "smc_user_root_dir" that is followed by '[', so that a comment or a use that names the array is passed over - up to the
// next ';' holds integer literals -1, 0, +1 and nothing else ("" = it does; else the refusal).
// The compiler cannot check it: the elements of a __device__ array are no constant expressions.
static std::string root_dir_error(const char *user_source) {
    const char *p = user_source;
    for (;;) {
        p = strstr(p, "smc_user_root_dir");
        if (!p) break;
        const char *q = p + strlen("smc_user_root_dir");
        while (*q == ' ' || *q == '\t') ++q;
        if (*q == '[') break;
        p = q;
    }
    const char *open = p ? strchr(p, '{') : nullptr, *semi = p ? strchr(p, ';') : nullptr;
    const char *close = open ? strchr(open, '}') : nullptr;
    const std::string how = "smc_user_root_dir: the directions are written as a list of the integers -1 (falling), 0 (either) or +1 (rising) "
                            "behind the first smc_user_root_dir[ of the source";
    if (!open || !close || (semi && semi < open)) return how;
    for (const char *q = open + 1; q < close;) {
        while (q < close && (*q == ' ' || *q == '\t' || *q == '\n' || *q == '\r')) ++q;
        if (q == close) break;
        char *end = nullptr;
        const long v = strtol(q, &end, 10);
        if (end == q) return how;
        if (v < -1 || v > 1) return "smc_user_root_dir: direction " + std::to_string(v) + " is none of -1 (falling), 0 (either), +1 (rising)";
        q = end;
        while (q < close && (*q == ' ' || *q == '\t' || *q == '\n' || *q == '\r')) ++q;
        if (q < close && *q != ',') return how;
        if (q < close) ++q;
    }
    return "";
}
// Count observations (user_count.h): the families of a source's outputs, read from its text as the directions above - the integer
// literals of the initialiser list behind the first "smc_user_obs_family" that is followed by '['.  Returns the number of entries
// (in fam, any integer: what an entry may be is obs_family_error's rule), 0 for a source without the name, -1 with `how` for a
// list that is not written so.
static const char *const kFamilyName = "smc_user_obs_family";
static int obs_family_list(const char *user_source, std::vector<int> &fam, std::string &how) {
    fam.clear();
    if (!user_source || !mentions(user_source, kFamilyName)) return 0;
    const char *p = user_source;
    for (;;) {
        p = strstr(p, kFamilyName);
        if (!p) break;
        const char *q = p + strlen(kFamilyName);
        while (*q == ' ' || *q == '\t') ++q;
        if (*q == '[') break;
        p = q;
    }
    const char *open = p ? strchr(p, '{') : nullptr, *semi = p ? strchr(p, ';') : nullptr;
    const char *close = open ? strchr(open, '}') : nullptr;
    how = "smc_user_obs_family: the families are written as a list of the integers 0 (Gaussian), 1 (Poisson) or 2 (negative binomial) "
          "behind the first smc_user_obs_family[ of the source";
    if (!open || !close || (semi && semi < open)) return -1;
    for (const char *q = open + 1; q < close;) {
        while (q < close && (*q == ' ' || *q == '\t' || *q == '\n' || *q == '\r')) ++q;
        if (q == close) break;
        char *end = nullptr;
        const long v = strtol(q, &end, 10);
        if (end == q || end > close) return -1;
        fam.push_back((int)(v < -1000 ? -1000 : v > 1000 ? 1000 : v));
        q = end;
        while (q < close && (*q == ' ' || *q == '\t' || *q == '\n' || *q == '\r')) ++q;
        if (q < close && *q != ',') return -1;
        if (q < close) ++q;
    }
    if (fam.empty()) return -1;
    how.clear();
    return (int)fam.size();
}
// the rules of a family list for a source of n_obs outputs (n_obs = 0: the one-output source); "" = valid
static std::string obs_family_error(const int *fam, int n_fam, int n_obs) {
    if (n_fam == 0) return "";
    if (n_fam < 0 || !fam) return "smc_user_obs_family: the list is malformed";
    if (n_obs == 0) return "smc_user_obs_family: the name in a one-output source (n_obs = 0) - count outputs need the multi-output source (smc_user_obs_vec, n_obs >= 1)";
    if (n_fam != n_obs)
        return "smc_user_obs_family: " + std::to_string(n_fam) + " entries for n_obs = " + std::to_string(n_obs) + " outputs (one entry per output)";
    for (int k = 0; k < n_fam; ++k)
        if (fam[k] < 0 || fam[k] > 2)
            return "smc_user_obs_family: entry " + std::to_string(fam[k]) + " of output " + std::to_string(k) +
                   " is none of 0 (Gaussian), 1 (Poisson), 2 (negative binomial)";
    return "";
}
// The families of a source for n_obs outputs: fam[k] (0 past n_obs); true if any output is a count.  bad: the refusal, if any.
static bool source_families(const char *user_source, int n_obs, int fam[kUserMaxObs], std::string &bad) {
    std::vector<int> list;
    std::fill_n(fam, kUserMaxObs, 0);
    const int n = obs_family_list(user_source, list, bad);
    if (n == 0) return false;
    if (n > 0) bad = obs_family_error(list.data(), n, n_obs);
    if (!bad.empty()) return false;
    bool any = false;
    for (int k = 0; k < n_obs; ++k) fam[k] = list[k], any = any || list[k] != 0;
    return any;
}
static std::string build_source(const char *user_source, const UserSourceSpec &sp) {
    const UserInputGeom &geom = sp.geom;
    const int n_obs = sp.n_obs, noise = sp.noise;
    const bool bdf = sp.method == SMC_USER_METHOD_BDF;
    std::string s;
    if (geom.n_in > 0)
        s = "#define SMC_USER_NCOND " + std::to_string(geom.n_cond) + "\n#define SMC_USER_NIN " + std::to_string(geom.n_in) +
            "\n#define SMC_USER_KCAP " + std::to_string(geom.kcap) + "\n#include \"user_input.h\"\n";
    else if (mentions(user_source, "smc_input"))
        s = "#error \"smc_input: this model has no inputs (n_in = 0) - set it with in_t / in_u through smc_set_model_user5\"\n";
    const bool events = geom.n_ev > 0;
    if (events) {
        s += "#define SMC_USER_EVENTS 1\n#define SMC_USER_EVAT " + std::to_string(geom.in_words()) + "\n#define SMC_USER_NEV " +
             std::to_string(geom.n_ev) + "\n#define SMC_USER_NVAL " + std::to_string(geom.n_val) + "\n#include \"user_event.h\"\n";
        if (!mentions(user_source, "smc_user_event"))
            s += "#error \"smc_user_event: this model has events and its source does not define smc_user_event\"\n";
    } else if (mentions(user_source, "smc_user_event") || mentions(user_source, "smc_event_value")) {
        s += "#error \"smc_user_event: this model has no events (n_ev = 0) - set it with ev_t / ev_v through smc_set_model_user6\"\n";
    }
    const bool roots = has_roots(user_source);
    if (roots) {
        if (!events) s += "#define SMC_USER_EVENTS 1\n#define SMC_USER_NO_SCHEDULE 1\n";
        s += "#define SMC_USER_ROOTS 1\n";
        if (!mentions(user_source, "smc_user_root_dir"))
            s += "#error \"smc_user_root: a source with state-triggered events defines smc_user_root_dir, the direction of every event function\"\n";
        else if (!root_dir_error(user_source).empty())
            s += "#error \"" + root_dir_error(user_source) + "\"\n";
        if (!mentions(user_source, "smc_user_root_event"))
            s += "#error \"smc_user_root: a source with state-triggered events defines smc_user_root_event, the jump at an event\"\n";
    }
    s += "#define SMC_USER_NS " + std::to_string(sp.n_states) + "\n#define SMC_USER_DIM " + std::to_string(sp.dim) + "\n";
    if (n_obs > 0)
        s += "#define SMC_USER_NOBS " + std::to_string(n_obs) + "\n#define SMC_USER_HAS_OBS_VEC " +
             ((n_obs > 1 || mentions(user_source, "smc_user_obs_vec")) ? "1\n" : "0\n");
    // smc_set_model_user4: the SMC_USER_NOISE blocks of the kernel files and of user_obs_args.h (noise = 2: with log1p and the division)
    // smc_set_model_user7: SMC_USER_CENSOR, user_censor.h in front and user_obs_args.h with its SMC_USER_CENSOR blocks (a noise model always)
    if (n_obs > 0 && noise > 0 && sp.censor) s += "#define SMC_USER_CENSOR 1\n#include \"user_censor.h\"\n";
    // a source with the name smc_user_obs_family and a count among its outputs: SMC_USER_COUNT, the list as SMC_USER_FAMILY, user_count.h in
    // front and user_obs_args.h with its SMC_USER_COUNT blocks (a noise model always).  An all-zero list changes nothing.
    {
        int fam[kUserMaxObs];
        std::string bad;
        if (source_families(user_source, n_obs, fam, bad)) {
            bool negbin = false;
            std::string list;
            for (int k = 0; k < n_obs; ++k) list += (k ? ", " : "") + std::to_string(fam[k]), negbin = negbin || fam[k] == 2;
            if (noise == 0)
                s += "#error \"smc_user_obs_family: a model with a count output is compiled with a noise model (noise >= 1)\"\n";
            else if (negbin && noise < 2)
                s += "#error \"smc_user_obs_family: a negative-binomial output needs the proportional part (noise = 2): its b_k is the overdispersion\"\n";
            else
                s += "#define SMC_USER_COUNT 1\n#define SMC_USER_FAMILY {" + list + "}\n#include \"user_count.h\"\n";
        } else if (!bad.empty()) {
            s += "#error \"" + bad + "\"\n";
        }
    }
    if (n_obs > 0 && noise > 0) s += std::string("#define SMC_USER_NOISE 1\n#define SMC_USER_NOISE_PROP ") + (noise > 1 ? "1\n" : "0\n");
    if (mentions(user_source, "smc_user_cost")) s += "#define SMC_USER_HAS_COST 1\n#define SMC_USER_LIST_COST 220.0\n#define SMC_USER_SOLO_COST 3700.0\n";
    if (bdf && mentions(user_source, "smc_user_jac")) s += "#define SMC_USER_HAS_JAC 1\n";
    if (!bdf) s += mentions(user_source, "smc_div") ? "#define SMC_USER_USES_DIV 1\n" : "#define SMC_USER_USES_DIV 0\n";
    // #line: hiprtc's diagnostics point into the user's text
    const std::string text = std::string(geom.n_in > 0 ? "using smc_in::smc_input;\n" : "") + (events ? "using smc_ev::smc_event_value;\n" : "") +
                             "#line 1 \"user_model\"\n" + user_source + "\n";
    s += bdf ? kUserBdfPrelude + text : kUserPreludeLean + text + kUserPreludeIeee + text;
    s += "}  // namespace smc_user_ieee\n";
    const char *kernel = bdf ? (roots ? k_user_bdf_kernel_h_rt : events ? k_user_bdf_kernel_h_ev : k_user_bdf_kernel_h)
                             : (roots ? k_user_rk45_kernel_h_rt : events ? k_user_rk45_kernel_h_ev : k_user_rk45_kernel_h);
    if (n_obs > 0) s = s + "#include \"user_obs_args.h\"\n" + kernel + "#define SMC_USER_PRED 1\n";
    return s + kernel + k_user_cost_scan_h;
}

// the in-memory headers of a compilation, and with the source itself the files of a dump (smc_user_model_dump_source*)
static const struct { const char *name, *text; } kUserHeaders[] = {
    {"sweep_args.h", k_sweep_args_h}, {"philox.h", k_philox_h}, {"reject_bound.h", k_reject_bound_h}, {"solve_sched.h", k_solve_sched_h},
    {"rk45_math.h", k_rk45_math_h}, {"user_item_ops.h", k_user_item_ops_h}, {"user_obs_args.h", k_user_obs_args_h},
    {"user_input.h", k_user_input_h}, {"user_event.h", k_user_event_h}, {"user_censor.h", k_user_censor_h},
    {"user_root.h", k_user_root_h}, {"user_count.h", k_user_count_h}};
constexpr int kUserHeaderCount = sizeof(kUserHeaders) / sizeof(kUserHeaders[0]);
// user_obs_args.h goes with a multi-output source only, user_input.h with a model that has inputs, user_event.h with one that
// has events - and user_item_ops.h then with its SMC_USER_EVENTS blocks -, user_censor.h with one that has censored observations
// - and user_obs_args.h then with its SMC_USER_CENSOR blocks -, user_root.h with a source that has state-triggered events - and
// user_item_ops.h then as it is, user_count.h with a source whose smc_user_obs_family holds a count - and user_obs_args.h then
// with its SMC_USER_COUNT blocks (k_..._ct; with censoring as well the file as it is, k_..._cnct)
static int user_headers(const char *user_source, const UserSourceSpec &sp, const char **texts, const char **names) {
    const UserInputGeom &geom = sp.geom;
    const bool roots = has_roots(user_source);
    int fam[kUserMaxObs];
    std::string bad;
    const bool count = source_families(user_source, sp.n_obs, fam, bad) && sp.noise > 0;      // user_count.h, and user_obs_args.h with its SMC_USER_COUNT blocks
    int n = 0;
    for (const auto &h : kUserHeaders) {
        if ((h.text == k_user_obs_args_h && sp.n_obs <= 0) || (h.text == k_user_input_h && geom.n_in <= 0) ||
            (h.text == k_user_event_h && geom.n_ev <= 0) || (h.text == k_user_censor_h && !sp.censor) ||
            (h.text == k_user_root_h && !roots) || (h.text == k_user_count_h && !count))
            continue;
        texts[n] = (h.text == k_user_item_ops_h && roots) ? k_user_item_ops_h_rt
                   : (h.text == k_user_item_ops_h && geom.n_ev > 0) ? k_user_item_ops_h_ev
                   : (h.text == k_user_obs_args_h && sp.censor) ? (count ? k_user_obs_args_h_cnct : k_user_obs_args_h_cn)
                   : (h.text == k_user_obs_args_h && count) ? k_user_obs_args_h_ct : h.text;
        names[n++] = h.name;
    }
    return n;
}

// compile build_source(...) for gfx950; on failure `log` holds hiprtc's diagnostics
static bool compile_user(const char *user_source, const UserSourceSpec &sp, std::vector<char> &code, std::string &log) {
    const std::string src = build_source(user_source, sp);
    hiprtcProgram prog;
    const char *headers[kUserHeaderCount], *names[kUserHeaderCount];
    const int n_headers = user_headers(user_source, sp, headers, names);
    if (hiprtcCreateProgram(&prog, src.c_str(), "smc_user_model.hip", n_headers, headers, names) != HIPRTC_SUCCESS) {
        log = "hiprtcCreateProgram failed";
        return false;
    }
    const char *opts[] = {"--offload-arch=gfx950", "-O3", "-ffp-contract=on", "-fno-fast-math"};
    const hiprtcResult r = hiprtcCompileProgram(prog, 4, opts);
    size_t ls = 0;
    if (hiprtcGetProgramLogSize(prog, &ls) == HIPRTC_SUCCESS && ls > 1) {
        log.resize(ls);
        (void)hiprtcGetProgramLog(prog, &log[0]);
    }
    bool ok = (r == HIPRTC_SUCCESS);
    if (ok) {
        size_t cs = 0;
        ok = hiprtcGetCodeSize(prog, &cs) == HIPRTC_SUCCESS && cs > 0;
        if (ok) {
            code.resize(cs);
            ok = hiprtcGetCode(prog, code.data()) == HIPRTC_SUCCESS;
        }
    }
    (void)hiprtcDestroyProgram(&prog);
    return ok;
}

void user_model_release(smc_ctx *c) {
    UserModel *u = (UserModel *)c->user;
    if (!u) return;
    (void)hipFree(u->d_t);
    (void)hipFree(u->d_obs);
    (void)hipFree(u->data.d_cond);
    (void)hipFree(u->data.d_sum);
    (void)hipFree(u->data.d_info);
    (void)hipFree(u->d_list);
    (void)hipFree(u->d_listed);
    (void)hipFree(u->d_count);
    (void)hipFree(u->data.d_bdf_counts);
    (void)hipFree(u->d_bdf_totals);
    (void)hipFree(u->data.d_const);
    (void)hipFree(u->data.d_img);
    (void)hipFree(u->d_pt);
    (void)hipFree(u->d_plk);
    (void)hipFree(u->d_ppred);
    (void)hipFree(u->d_cell_obs);
    (void)hipFree(u->d_cell_floor);
    (void)hipFree(u->d_cell_code);
    (void)hipFree(u->d_pll);
    if (u->module_pred) (void)hipModuleUnload(u->module_pred);
    if (u->module) (void)hipModuleUnload(u->module);
    delete u;
    c->user = nullptr;
}

// dynamic LDS of the compiled kernel: four waves' pools of started items, then the data times and observations
static size_t user_lds_bytes(int n_states, int n_ex, int n_t) {
    return ((size_t)4 * (2 * n_states + 6) * 64 + (size_t)2 * n_ex * (n_t + 1)) * sizeof(double);
}
// ... of the multi-output kernels: the pools, then the image of user_obs_args.h
// (noise: plus the noise block of a model of smc_set_model_user4; censor: records with the flag word of user_censor.h)
static size_t user_lds_bytes3(int n_states, int n_ex, int n_t, int n_obs, bool noise = false, bool censor = false) {
    return ((size_t)4 * (2 * n_states + 6) * 64 + (size_t)obs_table_at(n_ex) +
            (size_t)n_ex * (n_t + 1) * (censor ? obs_rec_words_censor(n_obs) : obs_rec_words(n_obs)) +
            (noise ? (size_t)obs_noise_words(n_ex) : 0)) * sizeof(double);
}
static const size_t kUserLdsCap = 150 * 1024;

// d: what it runs on - the model's data, or a group of a design.  pred != nullptr: the prediction kernel (smc_user_predict) - it
// writes there, and the BDF totals then add up over its chunks.  Of the model it changes `parity` alone.
static void launch_user_kernel(smc_ctx *c, const UserLaunchData &d, const double *theta, int64_t stride, int64_t n, uint8_t *p0mask,
                               double *lk, bool reject, double *pred = nullptr) {
    UserModel *u = (UserModel *)c->user;
    UserSolveArgs a{};
    a.theta = theta;
    a.stride = stride;
    a.n = n;
    a.p0 = p0mask;
    a.t = u->d_t;
    a.obs = u->d_obs;
    a.cond = d.d_cond;
    a.n_ex = d.n_ex;
    a.n_t = d.n_t;
    a.n_cond = u->cond_stride();      // the kernels know it as the stride of a cond row only
    a.dim = c->dim;
    a.est_sigma = u->est_sigma;
    a.sigma_fixed = u->sigma_fixed;
    a.rtol = u->rtol;
    a.atol = u->atol;
    a.sum_r2 = d.d_sum;
    a.info = d.d_info;
    a.queue = c->d_queue;
    a.rej = reject ? c->d_reject : nullptr;
    // persistent grid: the waves take chunks of kChunk items until the queue is empty (solve_sched.h); with a cost hint a
    // small sweep gets a wave per item so that solo solves do not queue behind each other (as mm_kernels.hip: solve_grid_blocks)
    const bool lists = u->fn_scan && c->stiff_first != 0;
    const int64_t chunks = (((n + 63) / 64) * 64 * d.n_ex + kChunk - 1) / kChunk;
    const int64_t need = (chunks + 3) / 4 + (lists ? (n * d.n_ex + 3) / 4 : 0);
    int64_t blocks = (int64_t)c->cu_count * d.blocks_per_cu;
    if (blocks > need) blocks = need;
    if (blocks < 1) blocks = 1;
    const bool multi = u->multi || pred;
    const unsigned lds = (unsigned)(multi ? user_lds_bytes3(u->spec.n_states, d.n_ex, d.n_t, u->n_obs, u->noise, u->spec.censor != 0) : user_lds_bytes(u->spec.n_states, d.n_ex, d.n_t));
    if (lists) {
        u->parity ^= 1;
        UserScanArgs sa{};
        sa.theta = theta;
        sa.stride = stride;
        sa.n = n;
        sa.p0 = p0mask;
        sa.listed = u->d_listed;
        sa.stiff_list = u->d_list;
        sa.count = u->d_count + 2 * u->parity;
        sa.count_next = u->d_count + 2 * (u->parity ^ 1);
        sa.stiff_cap = c->n_local;
        sa.solo_cap = (unsigned)(blocks * 4 / d.n_ex);      // one solo solve per wave of the grid
        // a heterogeneous Metropolis sweep large enough to have something to sort: cost order + in-phase waves, as for the
        // built-in model (mm_kernels.hip); the classes come from the model's hint
        const bool cost_order = p0mask != nullptr && c->cost_order != 0 && c->in_phase != 0 && n >= 16384 && c->d_bucket;
        if (cost_order) {
            sa.bucket = c->d_bucket;
            sa.done_sums = d.d_sum;
            sa.done_info = d.d_info;
            sa.n_ex = d.n_ex;
        }
        void *sargs[] = {&sa};
        const hipError_t e = hipModuleLaunchKernel(u->fn_scan, (unsigned)((n + 255) / 256), 1, 1, 256, 1, 1, 0, c->stream, sargs, nullptr);
        if (e != hipSuccess) {
            smc_fail(c, (std::string("launch of the user-model cost scan failed: ") + hipGetErrorString(e)).c_str());
            c->launch_failed = true;
            return;
        }
        a.listed = u->d_listed;
        a.stiff_list = u->d_list;
        a.stiff_count = sa.count;
        a.stiff_cap = sa.stiff_cap;
        a.solo_cap = sa.solo_cap;
        if (cost_order) {
            a.n_ordered = launch_cost_sort_order(c, n);
            if (a.n_ordered) {
                a.order = c->d_order;
                a.patience = kInPhasePatience;
            }
        }
    }
    UserObsArgs o{d.d_img, d.img_len, pred};
    void *args1[] = {&a, (void *)&d.d_bdf_counts};     // the RK45 kernel takes the first only
    void *args3[] = {&a, &o};                   // multi-output kernels: RK45 ...
    void *args3b[] = {&a, (void *)&d.d_bdf_counts, &o};   // ... and BDF
    void **args = !multi ? args1 : (u->spec.method == SMC_USER_METHOD_BDF ? args3b : args3);
    {
        ScopedTimer tm(c, SMC_T_SOLVE);
        (void)hipMemsetAsync(c->d_queue, 0, sizeof(unsigned long long), c->stream);
        const hipError_t e = hipModuleLaunchKernel(pred ? u->fn_pred : u->fn, (unsigned)blocks, 1, 1, 256, 1, 1, lds, c->stream, args, nullptr);
        if (e != hipSuccess) {
            smc_fail(c, (std::string("launch of the user-model kernel failed: ") + hipGetErrorString(e)).c_str());
            c->launch_failed = true;
            return;
        }
    }
    const int64_t g = (n + 255) / 256;
    if (u->noise)
        hipLaunchKernelGGL(user_finish_noise_kernel, dim3((unsigned)(g < 1024 ? g : 1024)), dim3(256), 0, c->stream, theta, stride, n,
                           p0mask, d.d_sum, d.d_info, d.n_ex, u->n_obs, d.d_const, d.d_const + 2 * d.n_ex, u->nz, lk, c->d_counters,
                           u->count ? d.d_const + d.n_ex : nullptr, u->negbin);
    else
        hipLaunchKernelGGL(user_finish_kernel, dim3((unsigned)(g < 1024 ? g : 1024)), dim3(256), 0, c->stream, theta, stride, n,
                           c->dim, p0mask, d.d_sum, d.d_info, d.n_ex, d.d_const, d.d_const + d.n_ex, u->est_sigma, u->sigma_fixed,
                           lk, c->d_counters);
    if (u->spec.method == SMC_USER_METHOD_BDF) {
        if (!pred) (void)hipMemsetAsync(u->d_bdf_totals, 0, 4 * sizeof(unsigned long long), c->stream);
        const int64_t items = n * d.n_ex, gb = (items + 255) / 256;
        hipLaunchKernelGGL(user_bdf_count_kernel, dim3((unsigned)(gb < 1024 ? gb : 1024)), dim3(256), 0, c->stream, p0mask, d.d_bdf_counts,
                           n, d.n_ex, u->d_bdf_totals);
    }
}

void launch_user_loglik(smc_ctx *c, const double *theta, int64_t stride, int64_t n, double *lk) {
    if (n > 0) launch_user_kernel(c, ((UserModel *)c->user)->data, theta, stride, n, nullptr, lk, false);
}

void launch_user_mh(smc_ctx *c, int64_t n, const MHParams &mh_in) {
    if (n <= 0) return;
    ParticleSet &P = c->set[SMC_SET_PRED];
    UserModel *u = (UserModel *)c->user;
    // exact early rejection (user_item_ops.h: Ops::certainly_rejected): off while the proposals' likelihoods are captured for inspection
    const bool reject = c->early_reject != 0 && c->debug_capture == 0 && mh_in.gamma > 0.0 && c->d_reject;
    MHParams mh = mh_in;
    if (reject) {
        mh.pending_sums = u->data.d_sum;     // the propose kernel marks every item of the sweep "not finished yet"
        mh.pending_n_ex = u->data.n_ex;
        mh.reject_out = c->d_reject;
        mh.reject_lk1 = c->set[SMC_SET_FILT].lk;
    }
    launch_generic_propose(c, n, mh);
    launch_user_kernel(c, u->data, P.theta, P.stride, n, c->d_p0, c->d_mlk2, reject);
    launch_generic_accept(c, n, mh, c->d_mlk2);
}

// smc_set_model_user3's data rules (include/smc_hip.h; user_models.obs_layout is the same in NumPy): every row of t is a
// strictly increasing run of n_t_e >= 1 finite times followed by NaN only; NaN in obs is a value not measured (what lies at a
// NaN time is ignored), an infinite one is refused; obs_scale (nullptr: ones) is finite and > 0.  On success me / ls hold
// m_e and the sum of log s_k over the observed values of each experiment; "" = valid, else what is wrong.
// censor (flags censor_layout_error has accepted, or nullptr): m_e and the sum count QUANTIFIED values only - a censored value
// has no density term and its floor is 0.
static std::string obs_layout(const double *t, const double *obs, const double *scale, int n_ex, int n_t, int n_obs,
                              std::vector<double> &me, std::vector<double> &ls, const signed char *censor = nullptr,
                              const int *family = nullptr) {      // family (nullptr: all Gaussian): a count output's values are left out too
    for (int k = 0; k < n_obs; ++k)
        if (scale && !(std::isfinite(scale[k]) && scale[k] > 0.0)) return "obs_scale must be finite and > 0";
    me.assign(n_ex, 0.0);
    ls.assign(n_ex, 0.0);
    for (int e = 0; e < n_ex; ++e) {
        const double *te = t + (size_t)e * n_t;
        int len = 0;
        while (len < n_t && !std::isnan(te[len])) ++len;
        const std::string row = "row " + std::to_string(e) + " of t ";
        for (int i = len; i < n_t; ++i)
            if (!std::isnan(te[i])) return row + "has a NaN time before a number (only a trailing run of NaN may shorten a row)";
        if (len == 0) return row + "has no finite time";
        for (int i = 0; i < len; ++i) {
            if (!std::isfinite(te[i])) return row + "holds an infinite time";
            if (i > 0 && !(te[i] > te[i - 1])) return row + "is not strictly increasing";
        }
        for (int i = 0; i < len; ++i)
            for (int k = 0; k < n_obs; ++k) {
                const double v = obs[((size_t)e * n_t + i) * n_obs + k];
                if (std::isnan(v)) continue;
                if (!std::isfinite(v)) return "obs holds an infinite value (NaN marks a value that was not measured)";
                if (censor && censor[((size_t)e * n_t + i) * n_obs + k] != 0) continue;
                if (family && family[k] != 0) continue;
                me[e] += 1.0;
                ls[e] += scale ? std::log(scale[k]) : 0.0;
            }
    }
    return "";
}

// the LDS image of user_obs_args.h for data obs_layout has accepted
// m_ek [8 e + k]: the finite observations of output k at the finite times of experiment e (censor: the quantified ones)
static std::vector<double> count_mek(const double *t, const double *obs, int n_ex, int n_t, int n_obs, const signed char *censor = nullptr,
                                     const int *family = nullptr) {      // ... and, of a model with count outputs, the Gaussian ones
    std::vector<double> mek(8 * (size_t)n_ex, 0.0);
    for (int e = 0; e < n_ex; ++e)
        for (int i = 0; i < n_t && !std::isnan(t[(size_t)e * n_t + i]); ++i)
            for (int k = 0; k < n_obs; ++k) {
                const size_t at = ((size_t)e * n_t + i) * n_obs + k;
                if (!std::isnan(obs[at]) && !(censor && censor[at] != 0) && !(family && family[k] != 0)) mek[8 * (size_t)e + k] += 1.0;
            }
    return mek;
}

using smc_cnt_host::count_floor;      // c(y), the floor of a Poisson term (count_floor.h)
// C_e: the sum of c(y) over the Poisson values of experiment e, for data the rules have accepted
static std::vector<double> count_floor_sums(const double *t, const double *obs, int n_ex, int n_t, int n_obs, const int *family) {
    std::vector<double> ce((size_t)n_ex, 0.0);
    for (int e = 0; e < n_ex; ++e)
        for (int i = 0; i < n_t && !std::isnan(t[(size_t)e * n_t + i]); ++i)
            for (int k = 0; k < n_obs; ++k) {
                const double v = obs[((size_t)e * n_t + i) * n_obs + k];
                if (family[k] == 1 && !std::isnan(v)) ce[e] += count_floor(v);
            }
    return ce;
}

// The per-cell tables of the pointwise kernels (pointwise_kernels.h) for data obs_layout has accepted: a cell (e, i, k) is observed
// when obs is finite at a finite time of its row; a censored value is observed.
static void build_cell_tables(const double *t, const double *obs, int n_ex, int n_t, int n_obs, const signed char *censor, const int *family,
                              std::vector<double> &value, std::vector<int> &code, std::vector<double> &floor_y) {
    const size_t cells = (size_t)n_ex * n_t * n_obs;
    value.assign(cells, std::nan(""));
    code.assign(cells, 0);
    floor_y.assign(cells, 0.0);
    for (int e = 0; e < n_ex; ++e)
        for (int i = 0; i < n_t && !std::isnan(t[(size_t)e * n_t + i]); ++i)
            for (int k = 0; k < n_obs; ++k) {
                const size_t at = ((size_t)e * n_t + i) * n_obs + k;
                if (std::isnan(obs[at])) continue;
                const int fam = family ? family[k] : 0;
                const signed char f = censor ? censor[at] : 0;
                value[at] = obs[at];
                code[at] = kCellObserved | ((f < 0 ? kCensorLeft : f > 0 ? kCensorRight : kCensorNone) << kCellFlagShift) | (fam << kCellFamilyShift);
                if (fam == 1) floor_y[at] = count_floor(obs[at]);
            }
}

// flagged: the image of a model compiled with SMC_USER_CENSOR - records of obs_rec_words_censor(n_obs) words, the last one the
// flags of the record's outputs (user_censor.h); censor: the flags (nullptr: none set, a design's image)
static std::vector<double> build_obs_image(const double *t, const double *obs, const double *scale, int n_ex, int n_t, int n_obs,
                                           const std::vector<double> &me, const std::vector<double> &ls, const UserNoise *nz = nullptr,
                                           bool flagged = false, const signed char *censor = nullptr, const int *family = nullptr) {
    const int R = flagged ? obs_rec_words_censor(n_obs) : obs_rec_words(n_obs), at = obs_table_at(n_ex);
    std::vector<double> img((size_t)at + (size_t)n_ex * (n_t + 1) * R + (nz ? (size_t)obs_noise_words(n_ex) : 0), 0.0);
    if (nz) {      // the noise block (user_obs_args.h)
        double *b = img.data() + at + (size_t)n_ex * (n_t + 1) * R;
        for (int k = 0; k < kUserMaxObs; ++k) {
            b[k] = k < n_obs ? (double)nz->add_index[k] : -1.0;
            b[8 + k] = k < n_obs ? nz->add_fixed[k] : 1.0;
            b[16 + k] = (k < n_obs && nz->prop) ? (double)nz->prop_index[k] : -1.0;
            b[24 + k] = (k < n_obs && nz->prop) ? nz->prop_fixed[k] : 0.0;
            b[32 + k] = k < n_obs ? nz->scale[k] : 1.0;
        }
        const std::vector<double> mek = count_mek(t, obs, n_ex, n_t, n_obs, censor, family);
        std::copy(mek.begin(), mek.end(), b + kNoiseHdr);
    }
    for (int k = 0; k < kObsHdrMe; ++k) img[k] = (scale && k < n_obs) ? 1.0 / scale[k] : 1.0;
    for (int e = 0; e < n_ex; ++e) {
        img[kObsHdrMe + e] = me[e];
        img[kObsHdrMe + n_ex + e] = ls[e];
        const double *te = t + (size_t)e * n_t;
        int len = 0;
        while (len < n_t && !std::isnan(te[len])) ++len;
        double *row = img.data() + at + (size_t)e * (n_t + 1) * R;
        for (int i = 0; i <= n_t; ++i) {
            double *r = row + (size_t)i * R;
            if (i < len) {
                r[0] = te[i];
                for (int k = 0; k < n_obs; ++k) r[1 + k] = obs[((size_t)e * n_t + i) * n_obs + k];
                if (flagged && censor) {
                    int bits = 0;
                    for (int k = 0; k < n_obs; ++k) {
                        const signed char f = censor[((size_t)e * n_t + i) * n_obs + k];
                        bits |= (f < 0 ? kCensorLeft : f > 0 ? kCensorRight : kCensorNone) << (2 * k);
                    }
                    r[R - 1] = (double)bits;
                }
            } else {
                r[0] = HUGE_VAL;          // the sentinel: no output time is ever >= it
                r[1] = te[len - 1];       // t_bound
            }
        }
    }
    return img;
}

// occupancy and LDS limit of the prediction kernel (u->fn_pred)
static int prepare_pred_kernel(smc_ctx *c, UserModel *u) {
    const size_t lds = user_lds_bytes3(u->spec.n_states, u->data.n_ex, u->data.n_t, u->n_obs, u->noise, u->spec.censor != 0);
    int nb = 0;
    if (hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&nb, u->fn_pred, 256, lds) == hipSuccess && nb >= 1) u->blocks_per_cu_pred = nb;
    if (lds > 48 * 1024 &&
        hipFuncSetAttribute(reinterpret_cast<const void *>(u->fn_pred), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return smc_fail(c, "smc_user_predict: raising the dynamic LDS limit of the prediction kernel failed");
    return 0;
}

// ---- a design other than the data's (smc_user_predict_at, smc_user_predict_summary) ----------------------------------------
// The prediction kernel takes n_ex and n_t as arguments and its data as an image, so a design is a UserLaunchData of its own,
// with every observation NaN (m_e = 0, no likelihood term).  A design whose image does not fit the LDS cap runs as several such
// bundles, one per run of consecutive experiments.

// what a launch writes per (experiment, particle): shared by the groups of a design, which run one after the other
struct DesignItems {
    double *d_sum = nullptr;
    int *d_info = nullptr;
    unsigned *d_bdf_counts = nullptr;
    void release() {
        (void)hipFree(d_sum);
        (void)hipFree(d_info);
        (void)hipFree(d_bdf_counts);
        d_sum = nullptr;
        d_info = nullptr;
        d_bdf_counts = nullptr;
    }
};
static size_t design_item_bytes(const UserModel *u) {      // per (experiment, particle)
    return sizeof(double) + sizeof(int) + (u->spec.method == SMC_USER_METHOD_BDF ? 4 * sizeof(unsigned) : 0);
}
static bool design_items_alloc(const UserModel *u, DesignItems &it, int64_t n, int g) {
    const size_t items = (size_t)n * g;
    return hipMalloc(&it.d_sum, items * sizeof(double)) == hipSuccess && hipMalloc(&it.d_info, items * sizeof(int)) == hipSuccess &&
           (u->spec.method != SMC_USER_METHOD_BDF || hipMalloc(&it.d_bdf_counts, 4 * items * sizeof(unsigned)) == hipSuccess);
}

// experiments [e0, e0 + n_ex) of a design as what a launch runs on.  The group owns the image, the cond rows and the constants
// of `d`; the per-item pointers of `d` are the design's DesignItems.
struct DesignGroup {
    UserLaunchData d;
    int e0 = 0;
    void release() {
        (void)hipFree(d.d_img);
        (void)hipFree(d.d_cond);
        (void)hipFree(d.d_const);
        d = UserLaunchData{};
    }
};

// experiments [e0, e0 + g) of the design (t: rows of n_t times, cond: rows of n_cond numbers) as a bundle on the device
static bool design_group_build(const UserModel *u, DesignGroup &dg, const DesignItems &it, const double *t, const double *cond, int e0, int g,
                               int n_t) {
    const std::vector<double> nan_obs((size_t)g * n_t * u->n_obs, std::nan("")), zero((u->noise ? 10 : 2) * (size_t)g, 0.0);
    std::vector<double> me, ls;
    if (!obs_layout(t + (size_t)e0 * n_t, nan_obs.data(), u->scale, g, n_t, u->n_obs, me, ls).empty()) return false;
    const std::vector<double> img = build_obs_image(t + (size_t)e0 * n_t, nan_obs.data(), u->scale, g, n_t, u->n_obs, me, ls,
                                                    u->noise ? &u->nz : nullptr, u->spec.censor != 0);      // no flag set
    const int cs = u->cond_stride();      // a model with inputs or events: cond holds whole rows, the tables included
    const size_t nc = (size_t)g * (cs > 0 ? cs : 1) * sizeof(double);
    UserLaunchData &d = dg.d;
    dg.e0 = e0;
    d.n_ex = g;
    d.n_t = n_t;
    d.img_len = (int)img.size();
    d.d_sum = it.d_sum;
    d.d_info = it.d_info;
    d.d_bdf_counts = it.d_bdf_counts;
    bool ok = hipMalloc(&d.d_img, img.size() * sizeof(double)) == hipSuccess && hipMalloc(&d.d_cond, nc) == hipSuccess &&
              hipMalloc(&d.d_const, zero.size() * sizeof(double)) == hipSuccess &&
              hipMemcpy(d.d_img, img.data(), img.size() * sizeof(double), hipMemcpyHostToDevice) == hipSuccess &&
              hipMemcpy(d.d_const, zero.data(), zero.size() * sizeof(double), hipMemcpyHostToDevice) == hipSuccess;
    if (ok && cs > 0)
        ok = hipMemcpy(d.d_cond, cond + (size_t)e0 * cs, nc, hipMemcpyHostToDevice) == hipSuccess;
    const size_t lds = user_lds_bytes3(u->spec.n_states, g, n_t, u->n_obs, u->noise, u->spec.censor != 0);
    int nb = 0;
    if (ok && hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&nb, u->fn_pred, 256, lds) == hipSuccess && nb >= 1) d.blocks_per_cu = nb;
    return ok;
}

// the largest run of experiments whose image fits the LDS cap (0: not even one row)
static int design_lds_group(const UserModel *u, int n_ex, int n_t) {
    int g = 0;
    while (g < n_ex && user_lds_bytes3(u->spec.n_states, g + 1, n_t, u->n_obs, u->noise, u->spec.censor != 0) <= kUserLdsCap) ++g;
    return g;
}

// the source of the prediction kernel of a one-output model: the multi-output source with one output under the sigma rule
static UserSourceSpec pred_source_spec(const UserModel *u) {
    UserSourceSpec sp = u->spec;
    sp.n_obs = 1;
    return sp;
}
// the prediction kernel of the model: part of a multi-output module, else compiled at the first call that needs it
static int ensure_pred_kernel(smc_ctx *c, UserModel *u, const char *who) {
    if (u->fn_pred) return 0;
    std::vector<char> code;
    std::string lg;
    if (!compile_user(u->source.c_str(), pred_source_spec(u), code, lg))
        return smc_fail(c, (std::string(who) + ": the prediction kernel does not compile:\n" + lg.substr(0, 3000)).c_str());
    if (hipModuleLoadData(&u->module_pred, code.data()) != hipSuccess ||
        hipModuleGetFunction(&u->fn_pred, u->module_pred, "smc_user_predict_kernel") != hipSuccess) {
        u->fn_pred = nullptr;
        return smc_fail(c, (std::string(who) + ": loading the prediction module failed").c_str());
    }
    // the data's own image may be one the kernel cannot hold (smc_user_predict refuses it): then only designs are predicted
    if (user_lds_bytes3(u->spec.n_states, u->data.n_ex, u->data.n_t, 1) <= kUserLdsCap && prepare_pred_kernel(c, u) != 0) {
        u->fn_pred = nullptr;
        return 1;
    }
    return 0;
}
// any design may need more dynamic LDS than the data's image: raised once to the cap
static int raise_pred_lds(smc_ctx *c, UserModel *u, const char *who) {
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(u->fn_pred), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kUserLdsCap) != hipSuccess)
        return smc_fail(c, (std::string(who) + ": raising the dynamic LDS limit of the prediction kernel failed").c_str());
    return 0;
}

// The experiments per group of a summary under its staging budget (max_staging_bytes; 0: most of what is free), for `fixed` bytes
// once and per_ex bytes per experiment of a group: at most g_lds, what the LDS cap allows.  0 with the refusal if not even one
// experiment fits; `noun`: what the caller stages beside the predictions.
static int design_staging_group(smc_ctx *c, const char *who, const char *noun, size_t max_staging_bytes, size_t fixed, size_t per_ex,
                                int64_t n, int g_lds, int n_ex) {
    size_t budget = max_staging_bytes;
    if (budget == 0) {      // default: most of what is free
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) {
            smc_fail(c, (std::string(who) + ": hipMemGetInfo failed").c_str());
            return 0;
        }
        budget = free_b / 10 * 8;
    }
    if (budget < fixed + per_ex) {
        smc_fail(c, (std::string(who) + ": one experiment of the design needs " + std::to_string(fixed + per_ex) +
                     " B of staging (predictions and " + noun + " of " + std::to_string(n) + " particles), max_staging_bytes allows " +
                     std::to_string(budget) + " B").c_str());
        return 0;
    }
    const int g_max = (int)std::min<size_t>((budget - fixed) / per_ex, (size_t)g_lds);
    return g_max > n_ex ? n_ex : g_max;
}

// One run of the prediction kernel over a design, group after group (smc_user_predict_at, smc_user_predict_summary,
// smc_user_pointwise_summary): the groups, what their launches write, the counters around them and, of a summary, its results
// and three events per group.  A caller: alloc() with its own buffers, begin(), a loop over `groups` - solve(k, ...), then its
// own kernels on d_ppred, then stamp(k) -, finish().  rc holds the first failure; solve() and stamp() expect rc == 0.  Everything
// is released when the run goes out of scope, on whichever path.
struct DesignRun {
    smc_ctx *const c;
    UserModel *const u;
    const std::string who;
    std::vector<DesignGroup> groups;
    DesignItems items;
    double *d_plk = nullptr, *d_ppred = nullptr;      // of one launch: the likelihoods the finish kernel writes, the predictions
    // a summary: what its kernels leave of all groups, which finish() brings to the host; per group an event before the solve,
    // one behind it and one behind the caller's kernels
    double *d_out = nullptr;
    std::vector<double> h_out;
    std::vector<hipEvent_t> ev;
    int rc = 0;
    DesignRun(smc_ctx *c_, UserModel *u_, const char *who_) : c(c_), u(u_), who(who_) {}
    DesignRun(const DesignRun &) = delete;
    ~DesignRun() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
        for (DesignGroup &dg : groups) dg.release();
        items.release();
        (void)hipFree(d_plk);
        (void)hipFree(d_ppred);
        (void)hipFree(d_out);
    }
    int fail(const std::string &what) { return rc = smc_fail(c, (who + ": " + what).c_str()); }
    // the design in groups of g_max experiments, for launches of up to n particles; out_words > 0: a summary with that many words
    // of results.  false: an allocation or an upload failed
    bool alloc(const double *t, const double *cond, int n_ex, int n_t, int64_t n, int g_max, size_t out_words) {
        groups.resize((size_t)(n_ex + g_max - 1) / g_max);
        h_out.resize(out_words);
        bool ok = design_items_alloc(u, items, n, g_max) && hipMalloc(&d_plk, (size_t)n * sizeof(double)) == hipSuccess &&
                  hipMalloc(&d_ppred, (size_t)n * g_max * n_t * u->n_obs * sizeof(double)) == hipSuccess &&
                  (out_words == 0 || hipMalloc(&d_out, out_words * sizeof(double)) == hipSuccess);
        for (size_t k = 0; ok && k < groups.size(); ++k) {
            const int e0 = (int)k * g_max;
            ok = design_group_build(u, groups[k], items, t, cond, e0, n_ex - e0 < g_max ? n_ex - e0 : g_max, n_t);
        }
        if (out_words > 0) ev.assign(3 * groups.size(), nullptr);
        for (size_t k = 0; ok && k < ev.size(); ++k) ok = hipEventCreate(&ev[k]) == hipSuccess;
        return ok;
    }
    // ok: alloc() and the caller's own allocations.  Clears the counters the launches add to.
    int begin(bool ok) {
        if (!ok) return fail("device allocation / upload failed");
        if (hipMemsetAsync(c->d_counters, 0, sizeof(SweepCounters), c->stream) != hipSuccess ||
            (u->spec.method == SMC_USER_METHOD_BDF && hipMemsetAsync(u->d_bdf_totals, 0, 4 * sizeof(unsigned long long), c->stream) != hipSuccess))
            return fail("clearing the counters failed");
        return 0;
    }
    // the solve of group k for the particles (theta, stride, n): its predictions are in d_ppred
    int solve(size_t k, const double *theta, int64_t stride, int64_t n) {
        if (!ev.empty()) (void)hipEventRecord(ev[3 * k], c->stream);
        launch_user_kernel(c, groups[k].d, theta, stride, n, nullptr, d_plk, false, d_ppred);
        if (c->launch_failed) {
            c->launch_failed = false;
            return rc = 1;
        }
        if (!ev.empty()) (void)hipEventRecord(ev[3 * k + 1], c->stream);
        return 0;
    }
    void stamp(size_t k) {
        if (!ev.empty()) (void)hipEventRecord(ev[3 * k + 2], c->stream);
    }
    // the one synchronisation, for results and counters: what the solves counted, and per part the time between the events
    int finish(int64_t *n_failed, int64_t *attempts, double *kernel_ms) {
        if (rc == 0 && ((d_out && hipMemcpyAsync(h_out.data(), d_out, h_out.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream) != hipSuccess) ||
                        hipMemcpyAsync(c->h_counters, c->d_counters, sizeof(SweepCounters), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
                        hipStreamSynchronize(c->stream) != hipSuccess))
            fail(hipGetErrorString(hipGetLastError()));
        if (rc != 0) {
            (void)hipStreamSynchronize(c->stream);
            return rc;
        }
        if (n_failed) *n_failed = (int64_t)c->h_counters->n_failed;
        if (attempts) *attempts = (int64_t)c->h_counters->rk_attempts;
        for (size_t k = 0; kernel_ms && 3 * k < ev.size(); ++k) {
            float a_ms = 0.f, b_ms = 0.f;
            if (hipEventElapsedTime(&a_ms, ev[3 * k], ev[3 * k + 1]) == hipSuccess) kernel_ms[0] += a_ms;
            if (hipEventElapsedTime(&b_ms, ev[3 * k + 1], ev[3 * k + 2]) == hipSuccess) kernel_ms[1] += b_ms;
        }
        return 0;
    }
};

}  // namespace smc

using namespace smc;

extern "C" {

static bool user_method_ok(int method) { return method == SMC_USER_METHOD_RK45 || method == SMC_USER_METHOD_BDF; }
static bool user_obs_ok(int n_obs) { return n_obs >= 1 && n_obs <= SMC_USER_MAX_OBS; }

// A spec struct as its caller knows it: the first min(struct_size, sizeof) bytes over zeros, so that a field a later feature
// appends reads as absent for an older caller.  False (the functions return 2 or fail) for a struct_size that ends before
// `required` bytes (the offset of the first field that may be left out) or exceeds the library's own struct.
static bool user_spec_copy(const void *in, size_t required, void *out, size_t size) {
    size_t n = 0;      // struct_size, the first field of both structs
    memset(out, 0, size);
    if (in) memcpy(&n, in, sizeof n);
    if (n < required || n > size) return false;
    memcpy(out, in, n);
    return true;
}

// The one validator of check and dump: the source spec as what build_source reads, false for arguments that are refused
// (return 2).  n_obs = 0, the one-output source, goes with no feature; n_in = 0: a model without inputs (n_knot is then not used),
// n_ev = 0: one without events; censored observations need a noise model's source.
static bool user_source_spec_of(const smc_user_source_spec *in, smc_user_source_spec &s, UserSourceSpec &sp) {
    if (!user_spec_copy(in, offsetof(smc_user_source_spec, noise), &s, sizeof s)) return false;
    if (!s.source || s.n_states < 1 || s.n_states > SMC_USER_MAX_STATES || s.dim < 1 || s.dim > SMC_MAX_DIM || !user_method_ok(s.method)) return false;
    if (s.n_obs == 0 ? (s.noise || s.n_in || s.n_ev || s.censor) : !user_obs_ok(s.n_obs)) return false;
    if (s.noise < 0 || s.noise > 2 || s.n_cond < 0 || s.n_in < 0 || s.n_in > SMC_USER_MAX_INPUTS) return false;
    if (s.n_in > 0 && (s.n_knot < 1 || s.n_knot > SMC_USER_MAX_KNOTS)) return false;
    if (s.n_ev < 0 || s.n_ev > SMC_USER_MAX_EVENTS || s.n_val < 0 || s.n_val > SMC_USER_MAX_EVENT_VALUES) return false;
    if (s.censor != 0 && s.noise == 0) return false;
    sp.n_states = s.n_states, sp.dim = s.dim, sp.method = s.method, sp.n_obs = s.n_obs;
    sp.noise = s.noise, sp.censor = s.censor != 0 ? 1 : 0;
    sp.geom.n_cond = s.n_cond;
    if (s.n_in > 0) sp.geom.n_in = s.n_in, sp.geom.kcap = knot_capacity(s.n_knot);
    if (s.n_ev > 0) sp.geom.n_ev = s.n_ev, sp.geom.n_val = s.n_val;
    return true;
}

int smc_user_model_check_spec(const smc_user_source_spec *spec, char *log, int log_cap) {
    smc_user_source_spec s;
    UserSourceSpec sp;
    if (!user_source_spec_of(spec, s, sp)) return 2;
    std::vector<char> code;
    std::string lg;
    const bool ok = compile_user(s.source, sp, code, lg);
    if (log && log_cap > 0) {
        strncpy(log, lg.c_str(), (size_t)log_cap - 1);
        log[log_cap - 1] = 0;
    }
    return ok ? 0 : 1;
}

// everything hiprtc would read, as files: `hipcc -I <dir>` compiles <dir>/smc_user_model.hip off line
int smc_user_model_dump_source_spec(const smc_user_source_spec *spec, const char *dir) {
    smc_user_source_spec s;
    UserSourceSpec sp;
    if (!dir || !user_source_spec_of(spec, s, sp)) return 2;
    const std::string src = build_source(s.source, sp);
    const char *texts[kUserHeaderCount], *names[kUserHeaderCount];
    const int n_headers = user_headers(s.source, sp, texts, names);
    for (int i = -1; i < n_headers; ++i) {
        FILE *f = fopen((std::string(dir) + "/" + (i < 0 ? "smc_user_model.hip" : names[i])).c_str(), "w");
        if (!f) return 1;
        const bool ok = fputs(i < 0 ? src.c_str() : texts[i], f) >= 0;
        if (fclose(f) != 0 || !ok) return 1;
    }
    return 0;
}

// The earlier entry points: each fills the fields it knows, in the struct's order, and leaves the rest zero.  Those that take an
// n_obs never meant the one-output source by it: one out of range is passed on as -1, which the validator refuses.
static int obs_or_bad(int n_obs) { return user_obs_ok(n_obs) ? n_obs : -1; }
static int user_check(const smc_user_source_spec &s, char *log, int log_cap) { return smc_user_model_check_spec(&s, log, log_cap); }
static int user_dump(const smc_user_source_spec &s, const char *dir) { return smc_user_model_dump_source_spec(&s, dir); }
int smc_user_model_check(const char *source, int n_states, int dim, char *log, int log_cap) {
    return user_check({sizeof(smc_user_source_spec), source, n_states, dim, SMC_USER_METHOD_RK45}, log, log_cap);
}
int smc_user_model_check2(const char *source, int n_states, int dim, int method, char *log, int log_cap) {
    return user_check({sizeof(smc_user_source_spec), source, n_states, dim, method}, log, log_cap);
}
int smc_user_model_check3(const char *source, int n_states, int dim, int method, int n_obs, char *log, int log_cap) {
    return user_check({sizeof(smc_user_source_spec), source, n_states, dim, method, obs_or_bad(n_obs)}, log, log_cap);
}
int smc_user_model_check4(const char *source, int n_states, int dim, int method, int n_obs, int proportional, char *log, int log_cap) {
    return user_check({sizeof(smc_user_source_spec), source, n_states, dim, method, obs_or_bad(n_obs),
                       proportional ? 2 : 1}, log, log_cap);
}
int smc_user_model_check5(const char *source, int n_states, int dim, int method, int n_obs, int noise, int n_cond, int n_in, int n_knot,
                          char *log, int log_cap) {
    return user_check({sizeof(smc_user_source_spec), source, n_states, dim, method, obs_or_bad(n_obs), noise, n_cond, n_in,
                       n_knot}, log, log_cap);
}
int smc_user_model_check6(const char *source, int n_states, int dim, int method, int n_obs, int noise, int n_cond, int n_in, int n_knot,
                          int n_ev, int n_val, char *log, int log_cap) {
    return user_check({sizeof(smc_user_source_spec), source, n_states, dim, method, obs_or_bad(n_obs), noise, n_cond, n_in, n_knot,
                       n_ev, n_val}, log, log_cap);
}
int smc_user_model_check7(const char *source, int n_states, int dim, int method, int n_obs, int noise, int n_cond, int n_in, int n_knot,
                          int n_ev, int n_val, int censor, char *log, int log_cap) {
    return user_check({sizeof(smc_user_source_spec), source, n_states, dim, method, obs_or_bad(n_obs), noise, n_cond, n_in, n_knot,
                       n_ev, n_val, censor}, log, log_cap);
}
int smc_user_model_dump_source(const char *source, int n_states, int dim, const char *dir) {
    return user_dump({sizeof(smc_user_source_spec), source, n_states, dim, SMC_USER_METHOD_RK45}, dir);
}
int smc_user_model_dump_source2(const char *source, int n_states, int dim, int method, const char *dir) {
    return user_dump({sizeof(smc_user_source_spec), source, n_states, dim, method}, dir);
}
int smc_user_model_dump_source3(const char *source, int n_states, int dim, int method, int n_obs, const char *dir) {
    return user_dump({sizeof(smc_user_source_spec), source, n_states, dim, method, obs_or_bad(n_obs)}, dir);
}
int smc_user_model_dump_source4(const char *source, int n_states, int dim, int method, int n_obs, int proportional, const char *dir) {
    return user_dump({sizeof(smc_user_source_spec), source, n_states, dim, method, obs_or_bad(n_obs), proportional ? 2 : 1}, dir);
}
int smc_user_model_dump_source5(const char *source, int n_states, int dim, int method, int n_obs, int noise, int n_cond, int n_in,
                                int n_knot, const char *dir) {
    return user_dump({sizeof(smc_user_source_spec), source, n_states, dim, method, obs_or_bad(n_obs), noise, n_cond, n_in,
                      n_knot}, dir);
}
int smc_user_model_dump_source6(const char *source, int n_states, int dim, int method, int n_obs, int noise, int n_cond, int n_in,
                                int n_knot, int n_ev, int n_val, const char *dir) {
    return user_dump({sizeof(smc_user_source_spec), source, n_states, dim, method, obs_or_bad(n_obs), noise, n_cond, n_in, n_knot,
                      n_ev, n_val}, dir);
}
int smc_user_model_dump_source7(const char *source, int n_states, int dim, int method, int n_obs, int noise, int n_cond, int n_in,
                                int n_knot, int n_ev, int n_val, int censor, const char *dir) {
    return user_dump({sizeof(smc_user_source_spec), source, n_states, dim, method, obs_or_bad(n_obs), noise, n_cond, n_in, n_knot,
                      n_ev, n_val, censor}, dir);
}

// the rules of the flags of censored observations (include/smc_hip.h: smc_set_model_user7; user_models.censor_layout is the same
// in NumPy), for t and obs that obs_layout accepts: censor has obs's shape (c_*: its own), every flag is -1, 0 or +1, and a
// nonzero flag stands on a finite value at a finite time of its row.  The first offence in row-major order; "" = valid.
static std::string censor_layout_error(const double *t, const double *obs, const signed char *censor, int n_ex, int n_t, int n_obs,
                                       int c_n_ex, int c_n_t, int c_n_obs) {
    if (!t || !obs || !censor) return "NULL t, obs or censor";
    if (n_ex < 1 || n_t < 1 || !user_obs_ok(n_obs)) return "bad data shape";
    if (c_n_ex != n_ex || c_n_t != n_t || c_n_obs != n_obs)
        return "censor must have the shape of obs (" + std::to_string(n_ex) + ", " + std::to_string(n_t) + ", " + std::to_string(n_obs) +
               "), got (" + std::to_string(c_n_ex) + ", " + std::to_string(c_n_t) + ", " + std::to_string(c_n_obs) + ")";
    for (int e = 0; e < n_ex; ++e) {
        int len = 0;
        while (len < n_t && !std::isnan(t[(size_t)e * n_t + len])) ++len;
        for (int i = 0; i < n_t; ++i)
            for (int k = 0; k < n_obs; ++k) {
                const int f = censor[((size_t)e * n_t + i) * n_obs + k];
                if (f == 0) continue;
                const std::string where = "row " + std::to_string(e) + ", time " + std::to_string(i) + ", output " + std::to_string(k);
                if (f != -1 && f != 1)
                    return "censor holds the flag " + std::to_string(f) + " at " + where + " (0: measured, -1: at or below obs, +1: at or above obs)";
                if (i >= len) return "censor flags a value past the end of its row at " + where;
                if (std::isnan(obs[((size_t)e * n_t + i) * n_obs + k])) return "censor flags a value that was not measured (obs is NaN) at " + where;
            }
    }
    return "";
}
int smc_user_censor_check(const double *t, const double *obs, const signed char *censor, int n_ex, int n_t, int n_obs, int c_n_ex,
                          int c_n_t, int c_n_obs) {
    const std::string bad = censor_layout_error(t, obs, censor, n_ex, n_t, n_obs, c_n_ex, c_n_t, c_n_obs);
    return bad.empty() ? 0 : smc_fail(nullptr, ("smc_user_censor_check: " + bad).c_str());
}

// the data rules of a model's inputs (include/smc_hip.h: smc_set_model_user5; user_models.input_layout is the same in NumPy):
// in_t n_ex x n_knot, a row by the row rules of t; in_u n_ex x n_knot x n_in, finite at the row's finite knots.  On success m[e]
// holds the knots of row e; "" = valid, else what is wrong.
static std::string input_layout_error(const double *in_t, const double *in_u, int n_ex, int n_in, int n_knot, std::vector<int> &m) {
    if (n_in < 1 || n_in > SMC_USER_MAX_INPUTS) return "n_in = " + std::to_string(n_in) + " outside 1 .. 8 (SMC_USER_MAX_INPUTS)";
    if (n_knot < 1) return "n_knot = " + std::to_string(n_knot) + ": a row needs at least one knot";
    if (n_knot > SMC_USER_MAX_KNOTS)
        return "n_knot = " + std::to_string(n_knot) + " above the knot capacity " + std::to_string(SMC_USER_MAX_KNOTS) + " (SMC_USER_MAX_KNOTS)";
    if (n_ex < 1) return "n_ex = " + std::to_string(n_ex) + ": no experiment";
    if (!in_t || !in_u) return "NULL in_t or in_u";
    m.assign(n_ex, 0);
    for (int e = 0; e < n_ex; ++e) {
        const double *te = in_t + (size_t)e * n_knot;
        int len = 0;
        while (len < n_knot && !std::isnan(te[len])) ++len;
        const std::string row = "row " + std::to_string(e) + " of in_t ";
        for (int i = len; i < n_knot; ++i)
            if (!std::isnan(te[i]))
                return row + "has a NaN knot before a number at knot " + std::to_string(i) + " (only a trailing run of NaN may shorten a row)";
        if (len == 0) return row + "has no finite knot";
        for (int i = 0; i < len; ++i) {
            if (!std::isfinite(te[i])) return row + "holds an infinite knot at knot " + std::to_string(i);
            if (i > 0 && !(te[i] > te[i - 1])) return row + "is not strictly increasing at knot " + std::to_string(i);
        }
        for (int i = 0; i < len; ++i)
            for (int k = 0; k < n_in; ++k) {
                const double *ue = in_u + ((size_t)e * n_knot + i) * n_in + k;
                if (!std::isfinite(*ue))
                    return "row " + std::to_string(e) + " of in_u is not finite at knot " + std::to_string(i) + " of input " + std::to_string(k);
                if (i > 0 && !std::isfinite((ue[0] - ue[-(ptrdiff_t)n_in]) / (te[i] - te[i - 1])))
                    return "row " + std::to_string(e) + " of in_u has a slope that overflows at knot " + std::to_string(i) + " of input " + std::to_string(k);
            }
        m[e] = len;
    }
    return "";
}
int smc_user_input_check(const double *in_t, const double *in_u, int n_ex, int n_in, int n_knot) {
    std::vector<int> m;
    const std::string bad = input_layout_error(in_t, in_u, n_ex, n_in, n_knot, m);
    return bad.empty() ? 0 : smc_fail(nullptr, ("smc_user_input_check: " + bad).c_str());
}
// The cond rows of a model with inputs (user_input.h) for inputs input_layout_error has accepted: per experiment the model's
// n_cond numbers, the knots padded with +inf, and per input the values (u[m - 1] repeated past the end) and the slopes (IEEE
// division, here and nowhere else; 0 from the last knot on).
static std::vector<double> build_input_rows(const double *cond, const UserInputGeom &g, const double *in_t, const double *in_u, int n_ex,
                                            int n_knot, const std::vector<int> &m) {
    const int K = g.kcap, W = g.in_words();
    std::vector<double> rows((size_t)n_ex * W, 0.0);
    for (int e = 0; e < n_ex; ++e) {
        double *r = rows.data() + (size_t)e * W;
        for (int j = 0; j < g.n_cond; ++j) r[j] = cond[(size_t)e * g.n_cond + j];
        const double *te = in_t + (size_t)e * n_knot;
        double *tk = r + g.n_cond;
        for (int j = 0; j < K; ++j) tk[j] = j < m[e] ? te[j] : HUGE_VAL;
        for (int k = 0; k < g.n_in; ++k) {
            double *u = r + g.n_cond + K + (size_t)k * (2 * K + 1), *sl = u + K + 1;
            for (int j = 0; j <= K; ++j) u[j] = in_u[((size_t)e * n_knot + (j < m[e] ? j : m[e] - 1)) * g.n_in + k];
            for (int j = 0; j < K; ++j) sl[j] = j < m[e] - 1 ? (u[j + 1] - u[j]) / (tk[j + 1] - tk[j]) : 0.0;
        }
    }
    return rows;
}

// the data rules of a model's scheduled events (include/smc_hip.h: smc_set_model_user6; user_models.event_layout is the same in
// NumPy): ev_t n_ex x n_ev, every row a strictly increasing finite run (it may be empty) and then only NaN, every finite event
// time > t[e][0]; ev_v n_ex x n_ev x n_val, finite at the row's finite events (nullptr with n_val = 0).  t == nullptr (the events
// of a design whose times are not known yet) leaves the rule about t[e][0] out.  On success m[e] holds the events of row e;
// "" = valid, else what is wrong.
static std::string event_layout_error(const double *t, const double *ev_t, const double *ev_v, int n_ex, int n_t, int n_ev, int n_val,
                                      std::vector<int> &m) {
    if (n_ev < 1) return "n_ev = " + std::to_string(n_ev) + ": a model with events needs room for at least one";
    if (n_ev > SMC_USER_MAX_EVENTS)
        return "n_ev = " + std::to_string(n_ev) + " above the event capacity " + std::to_string(SMC_USER_MAX_EVENTS) + " (SMC_USER_MAX_EVENTS)";
    if (n_val < 0 || n_val > SMC_USER_MAX_EVENT_VALUES) return "n_val = " + std::to_string(n_val) + " outside 0 .. 8 (SMC_USER_MAX_EVENT_VALUES)";
    if (n_ex < 1) return "n_ex = " + std::to_string(n_ex) + ": no experiment";
    if (t && n_t < 1) return "n_t = " + std::to_string(n_t) + ": no time";
    if (!ev_t) return "NULL ev_t";
    if ((n_val > 0) != (ev_v != nullptr)) return n_val > 0 ? "NULL ev_v with n_val > 0" : "ev_v given with n_val = 0 (it must be NULL)";
    m.assign(n_ex, 0);
    for (int e = 0; e < n_ex; ++e) {
        const double *te = ev_t + (size_t)e * n_ev;
        int len = 0;
        while (len < n_ev && !std::isnan(te[len])) ++len;
        const std::string row = "row " + std::to_string(e) + " of ev_t ";
        for (int i = len; i < n_ev; ++i)
            if (!std::isnan(te[i]))
                return row + "has a NaN event time before a number at event " + std::to_string(i) + " (only a trailing run of NaN may shorten a row)";
        for (int i = 0; i < len; ++i) {
            if (!std::isfinite(te[i])) return row + "holds an infinite event time at event " + std::to_string(i);
            if (i > 0 && !(te[i] > te[i - 1])) return row + "is not strictly increasing at event " + std::to_string(i);
            if (t && !(te[i] > t[(size_t)e * n_t])) return row + "is not later than the row's first time t[e][0] at event " + std::to_string(i);
        }
        for (int i = 0; i < len; ++i)
            for (int k = 0; k < n_val; ++k)
                if (!std::isfinite(ev_v[((size_t)e * n_ev + i) * n_val + k]))
                    return "row " + std::to_string(e) + " of ev_v is not finite at event " + std::to_string(i) + ", value " + std::to_string(k);
        m[e] = len;
    }
    return "";
}
int smc_user_event_check(const double *t, const double *ev_t, const double *ev_v, int n_ex, int n_t, int n_ev, int n_val) {
    std::vector<int> m;
    const std::string bad = t ? event_layout_error(t, ev_t, ev_v, n_ex, n_t, n_ev, n_val, m) : std::string("NULL t");
    return bad.empty() ? 0 : smc_fail(nullptr, ("smc_user_event_check: " + bad).c_str());
}
// The cond rows of a model with events (user_event.h) for events event_layout_error has accepted: `base` holds per experiment
// the g.in_words() words in front (the cond numbers, with inputs their table); behind them the row's m[e] event times, +inf up
// to and including index g.n_ev, and the values.  n_ev: the width of ev_t / ev_v as given, m[e] <= g.n_ev.
static std::vector<double> build_event_rows(const double *base, const UserInputGeom &g, const double *ev_t, const double *ev_v, int n_ex,
                                            int n_ev, const std::vector<int> &m) {
    const int B = g.in_words(), W = g.row_words();
    std::vector<double> rows((size_t)n_ex * W, 0.0);
    for (int e = 0; e < n_ex; ++e) {
        double *r = rows.data() + (size_t)e * W;
        for (int j = 0; j < B; ++j) r[j] = base[(size_t)e * B + j];
        for (int j = 0; j <= g.n_ev; ++j) r[B + j] = j < m[e] ? ev_t[(size_t)e * n_ev + j] : HUGE_VAL;
        for (int j = 0; j < m[e]; ++j)
            for (int k = 0; k < g.n_val; ++k) r[B + g.n_ev + 1 + j * g.n_val + k] = ev_v[((size_t)e * n_ev + j) * g.n_val + k];
    }
    return rows;
}

// the rules of a noise specification (include/smc_hip.h: smc_set_model_user4; user_models.noise_layout is the same in NumPy):
// "" = valid, else what is wrong
static std::string noise_spec_error(int n_obs, int dim, const int *add_index, const double *add_fixed, const int *prop_index,
                                    const double *prop_fixed) {
    if (!user_obs_ok(n_obs)) return "n_obs out of range (1 .. SMC_USER_MAX_OBS)";
    if (dim < 1 || dim > SMC_MAX_DIM) return "dim out of range";
    if (!add_index || !add_fixed) return "NULL add_index or add_fixed (one entry per output)";
    if ((prop_index == nullptr) != (prop_fixed == nullptr)) return "prop_index and prop_fixed must both be given or both be NULL";
    for (int k = 0; k < n_obs; ++k) {
        const std::string o = "output " + std::to_string(k) + ": ";
        if (add_index[k] < -1 || add_index[k] >= dim) return o + "add_index outside [0, dim) (-1 selects add_fixed)";
        if (add_index[k] == -1 && !(std::isfinite(add_fixed[k]) && add_fixed[k] > 0.0)) return o + "add_fixed must be finite and > 0";
        if (!prop_index) continue;
        if (prop_index[k] < -1 || prop_index[k] >= dim) return o + "prop_index outside [0, dim) (-1 selects prop_fixed)";
        if (prop_index[k] == -1 && !(std::isfinite(prop_fixed[k]) && prop_fixed[k] >= 0.0)) return o + "prop_fixed must be finite and >= 0";
    }
    return "";
}
int smc_user_noise_check(int n_obs, int dim, const int *add_index, const double *add_fixed, const int *prop_index, const double *prop_fixed) {
    const std::string bad = noise_spec_error(n_obs, dim, add_index, add_fixed, prop_index, prop_fixed);
    return bad.empty() ? 0 : smc_fail(nullptr, ("smc_user_noise_check: " + bad).c_str());
}

// The rules of a model with count outputs (include/smc_hip.h: COUNT OBSERVATIONS; user_models.count_layout is the same in NumPy),
// for t and obs that obs_layout accepts and flags that censor_layout_error accepts (nullptr: none): the family list (fam, n_fam
// entries as obs_family_list returns them) against n_obs; per count output the scale (obs_scale nullptr: ones), the additive
// entry (add_index nullptr: the sigma rule, under which a count output stands at fixed 1) and the proportional entry (prop_index
// nullptr: none); est_sigma under the sigma rule; then the values and the flags, the first offence in row-major order.
// "" = valid, else what is wrong.
static std::string count_rules_error(const int *fam, int n_fam, const double *t, const double *obs, const signed char *censor,
                                     const double *obs_scale, int n_ex, int n_t, int n_obs, int est_sigma, const int *add_index,
                                     const double *add_fixed, const int *prop_index, const double *prop_fixed) {
    const std::string bad = obs_family_error(fam, n_fam, n_obs);
    if (!bad.empty() || n_fam == 0) return bad;
    bool gaussian = false;
    for (int k = 0; k < n_obs; ++k) {
        gaussian = gaussian || fam[k] == 0;
        if (fam[k] == 0) continue;
        const std::string o = "output " + std::to_string(k) + ": ";
        if (obs_scale && obs_scale[k] != 1.0) return o + "the obs_scale of a count output must be 1";
        if (add_index && !(add_index[k] == -1 && add_fixed && add_fixed[k] == 1.0))
            return o + "the additive entry of a count output must be fixed at 1 (it is not used)";
        const bool has_b = prop_index && !(prop_index[k] == -1 && prop_fixed && prop_fixed[k] == 0.0);
        if (fam[k] == 1 && has_b) return o + "a Poisson output takes no proportional entry (absent, or fixed at 0)";
        if (fam[k] == 2 && !has_b)
            return o + "a negative-binomial output needs a proportional entry (its b_k: a parameter, or fixed > 0)";
    }
    if (!add_index && est_sigma && !gaussian)
        return "est_sigma without a noise model and no Gaussian output: the last parameter would be a noise level that nothing uses";
    if (!t || !obs) return "NULL t or obs";
    for (int e = 0; e < n_ex; ++e)
        for (int i = 0; i < n_t && !std::isnan(t[(size_t)e * n_t + i]); ++i)
            for (int k = 0; k < n_obs; ++k) {
                const size_t at = ((size_t)e * n_t + i) * n_obs + k;
                const double v = obs[at];
                if (fam[k] == 0 || std::isnan(v)) continue;
                const std::string where = " at row " + std::to_string(e) + ", time " + std::to_string(i) + ", output " + std::to_string(k);
                if (v < 0.0) return "obs holds a negative value on a count output" + where;
                if (v > 9007199254740992.0) return "obs holds a value above 2^53 on a count output" + where;
                if (v != std::floor(v)) return "obs holds a value that is not an integer on a count output" + where;
                if (censor && censor[at] != 0) return "censor flags a value of a count output" + where + " (censored counts are not supported)";
            }
    return "";
}
int smc_user_obs_family(const char *source, int *family, int cap) {
    std::vector<int> fam;
    std::string how;
    const int n = obs_family_list(source, fam, how);
    if (n < 0) {
        (void)smc_fail(nullptr, how.c_str());
        return -1;
    }
    for (int k = 0; k < n && k < cap && family; ++k) family[k] = fam[k];
    return n;
}
int smc_user_count_check(const int *family, int n_family, const double *t, const double *obs, const signed char *censor,
                         const double *obs_scale, int n_ex, int n_t, int n_obs, int est_sigma, const int *add_index,
                         const double *add_fixed, const int *prop_index, const double *prop_fixed) {
    std::string bad = obs_family_error(family, n_family, n_obs);
    if (bad.empty() && n_family > 0) {
        std::vector<double> m, l;
        if (n_ex < 1 || n_t < 1) bad = "bad data shape";
        if (bad.empty()) bad = (t && obs) ? obs_layout(t, obs, nullptr, n_ex, n_t, n_obs, m, l) : std::string("NULL t or obs");
        if (bad.empty() && censor) bad = censor_layout_error(t, obs, censor, n_ex, n_t, n_obs, n_ex, n_t, n_obs);
        if (bad.empty())
            bad = count_rules_error(family, n_family, t, obs, censor, obs_scale, n_ex, n_t, n_obs, est_sigma, add_index, add_fixed, prop_index,
                                    prop_fixed);
    }
    return bad.empty() ? 0 : smc_fail(nullptr, ("smc_user_count_check: " + bad).c_str());
}

// What the device part needs of a smc_user_model_spec: user_model_plan forms it, the one place where the rules live by which an
// absent feature takes the earlier path, and its bits with it.
struct UserModelPlan {
    bool multi = false;      // the multi-output source and data (n_obs >= 1); else the one-output model of smc_set_model_user / 2
    int n_obs = 1;
    bool noise = false;      // the noise path (nz), else the sigma rule (est_sigma, sigma_fixed)
    UserNoise nz{};
    int est_sigma = 1;
    double sigma_fixed = 0.0;
    bool in = false, ev = false;      // inputs, events: the spec's in_* and ev_* fields
    const signed char *censor = nullptr;      // flags with at least one set, which censor_layout_error has accepted
    bool count = false;      // a count among the outputs (the source's smc_user_obs_family): the noise path always
    int family[kUserMaxObs] = {0, 0, 0, 0, 0, 0, 0, 0};
};

// The spec as a plan, or the failure.  Messages about the arguments' consistency carry `who`, the called function; who == nullptr:
// a numbered entry point, and they carry the name of the newest feature its arguments use, as its chain of predecessors did.
static int user_model_plan(smc_ctx *c, const smc_user_model_spec &s, const char *who, UserModelPlan &p) {
    const size_t n_flags = (s.censor && s.n_ex >= 1 && s.n_t >= 1 && user_obs_ok(s.n_obs)) ? (size_t)s.n_ex * s.n_t * s.n_obs : 0;
    const bool censored = std::any_of(s.censor, s.censor + n_flags, [](signed char f) { return f != 0; });
    const bool inputs = s.n_in != 0, events = s.n_ev != 0;
    const std::string gen = censored ? "smc_set_model_user7" : events ? "smc_set_model_user6" : "smc_set_model_user5";
    const std::string me = who ? who : gen;
    std::vector<int> fam_list;      // count outputs: the families come with the source
    std::string fam_bad;
    const int n_fam = obs_family_list(s.source, fam_list, fam_bad);
    if (fam_bad.empty()) fam_bad = obs_family_error(fam_list.data(), n_fam, s.n_obs == 0 ? 0 : user_obs_ok(s.n_obs) ? s.n_obs : n_fam);
    if (!fam_bad.empty()) return smc_fail(c, (me + ": " + fam_bad).c_str());
    const bool counted = std::any_of(fam_list.begin(), fam_list.end(), [](int f) { return f != 0; });
    if (s.n_obs == 0) {      // the one-output model: none of the later features
        if (s.obs_scale || s.add_index || s.add_fixed || s.prop_index || s.prop_fixed || inputs || s.in_t || s.in_u || events || s.ev_t || s.ev_v || s.censor)
            return smc_fail(c, (me + ": n_obs = 0 (the one-output model) with obs_scale, a noise model, inputs, events or censor given").c_str());
        p.est_sigma = s.est_sigma, p.sigma_fixed = s.sigma_fixed;
        return 0;
    }
    p.multi = true;
    p.n_obs = s.n_obs;
    if (censored) {      // the data's own rules first (the flags' rules assume them), then the flags'
        std::vector<double> m, l;
        std::string bad = (s.t && s.obs) ? obs_layout(s.t, s.obs, s.obs_scale, s.n_ex, s.n_t, s.n_obs, m, l) : std::string("NULL t or obs");
        if (bad.empty()) bad = censor_layout_error(s.t, s.obs, s.censor, s.n_ex, s.n_t, s.n_obs, s.n_ex, s.n_t, s.n_obs);
        if (!bad.empty()) return smc_fail(c, ("smc_set_model_user7: " + bad).c_str());
        p.censor = s.censor;
    }
    if (counted) {      // the data's own rules first, then those of the counts
        std::vector<double> m, l;
        std::string bad = (s.t && s.obs && s.n_ex >= 1 && s.n_t >= 1) ? obs_layout(s.t, s.obs, s.obs_scale, s.n_ex, s.n_t, s.n_obs, m, l) : std::string("NULL t or obs");
        if (bad.empty())
            bad = count_rules_error(fam_list.data(), n_fam, s.t, s.obs, p.censor, s.obs_scale, s.n_ex, s.n_t, s.n_obs, s.est_sigma, s.add_index,
                                    s.add_fixed, s.prop_index, s.prop_fixed);
        if (!bad.empty()) return smc_fail(c, (me + ": " + bad).c_str());
        p.count = true;
        std::copy(fam_list.begin(), fam_list.end(), p.family);
    }
    if (!events && (s.ev_t || s.ev_v))
        return smc_fail(c, ((who ? who : censored ? gen : "smc_set_model_user6") + std::string(": n_ev = 0 with ev_t or ev_v given (both must be NULL)")).c_str());
    if (!inputs && (s.in_t || s.in_u)) return smc_fail(c, (me + ": n_in = 0 with in_t or in_u given (both must be NULL)").c_str());
    p.in = inputs, p.ev = events;
    const int *add_index = s.add_index;
    const double *add_fixed = s.add_fixed;
    int sigma_index[kUserMaxObs];
    double sigma_value[kUserMaxObs];
    if (!add_index) {      // the sigma rule; under censoring as the equivalent noise specification
        if (s.add_fixed || s.prop_index || s.prop_fixed)
            return smc_fail(c, (me + ": add_index is NULL (the sigma rule) and another part of a noise model is given").c_str());
        p.est_sigma = s.est_sigma, p.sigma_fixed = s.sigma_fixed;
        if (!censored && !counted) return 0;
        const bool gaussian = std::any_of(p.family, p.family + s.n_obs, [](int f) { return f == 0; });
        if (gaussian && !s.est_sigma && !(std::isfinite(s.sigma_fixed) && s.sigma_fixed > 0.0)) return smc_fail(c, (me + ": sigma_fixed must be finite and > 0").c_str());
        std::fill_n(sigma_index, kUserMaxObs, s.est_sigma ? c->dim - 1 : -1);
        std::fill_n(sigma_value, kUserMaxObs, s.est_sigma ? 0.0 : s.sigma_fixed);
        for (int k = 0; k < kUserMaxObs; ++k)
            if (p.family[k] != 0) sigma_index[k] = -1, sigma_value[k] = 1.0;      // a count output: fixed 1, not used
        add_index = sigma_index, add_fixed = sigma_value;
    }
    const std::string bad = noise_spec_error(s.n_obs, c->dim, add_index, add_fixed, s.prop_index, s.prop_fixed);
    if (!bad.empty()) return smc_fail(c, ((who ? who : censored || events ? gen : inputs ? "smc_set_model_user5" : "smc_set_model_user4") + (": " + bad)).c_str());
    if (!s.prop_index && !censored && !counted) {      // one sigma for every output: the sigma rule's path and its bits
        bool last = true, fixed = true;
        for (int k = 0; k < s.n_obs; ++k) {
            last = last && add_index[k] == c->dim - 1;
            fixed = fixed && add_index[k] == -1 && add_fixed[k] == add_fixed[0];
        }
        p.est_sigma = last ? 1 : 0, p.sigma_fixed = last ? 0.0 : add_fixed[0];
        if (last || fixed) return 0;
    }
    p.noise = true;
    p.est_sigma = 0, p.sigma_fixed = 1.0;
    for (int k = 0; k < kUserMaxObs; ++k) {
        p.nz.add_index[k] = k < s.n_obs ? add_index[k] : -1;
        p.nz.add_fixed[k] = (k < s.n_obs && add_index[k] < 0) ? add_fixed[k] : 1.0;
        p.nz.prop_index[k] = (k < s.n_obs && s.prop_index) ? s.prop_index[k] : -1;
        p.nz.prop_fixed[k] = (k < s.n_obs && s.prop_index && s.prop_index[k] < 0) ? s.prop_fixed[k] : 0.0;
        p.nz.scale[k] = (k < s.n_obs && s.obs_scale) ? s.obs_scale[k] : 1.0;
    }
    p.nz.prop = s.prop_index ? 1 : 0;
    return 0;
}

// Every set function: the spec as its caller gave it (user_spec_copy has applied struct_size), planned, checked against the
// kernel's limits and brought to the device.
static int set_model_user_impl(smc_ctx *c, const smc_user_model_spec &s, const char *who) {
    if (!c) return smc_fail(nullptr, "NULL context");
    UserModelPlan plan;
    if (user_model_plan(c, s, who, plan) != 0) return 1;
    const double *t = s.t, *obs = s.obs, *cond = s.cond, *obs_scale = s.obs_scale;
    const int n_states = s.n_states, n_obs = plan.n_obs, n_ex = s.n_ex, n_t = s.n_t, n_cond = s.n_cond, method = s.method;
    const bool multi = plan.multi;
    const UserNoise *nz = plan.noise ? &plan.nz : nullptr;
    const signed char *censor = plan.censor;
    const int *family = plan.count ? plan.family : nullptr;
    const UserInputs inputs{s.in_t, s.in_u, s.n_in, s.n_knot}, *in = plan.in ? &inputs : nullptr;
    const UserEvents events_{s.ev_t, s.ev_v, s.n_ev, s.n_val}, *ev = plan.ev ? &events_ : nullptr;
    if (!s.source) return smc_fail(c, "smc_set_model_user: NULL source");
    if (!user_method_ok(method)) return smc_fail(c, "smc_set_model_user: unknown method (SMC_USER_METHOD_RK45 or SMC_USER_METHOD_BDF)");
    if (n_states < 1 || n_states > SMC_USER_MAX_STATES) return smc_fail(c, "smc_set_model_user: n_states out of range");
    if (multi && !user_obs_ok(n_obs)) return smc_fail(c, "smc_set_model_user3: n_obs out of range (1 .. SMC_USER_MAX_OBS)");
    if (n_ex < 1 || n_t < 1 || n_cond < 0) return smc_fail(c, "smc_set_model_user: bad data shape");
    std::vector<double> me, ls;
    std::string bad = (t && obs) ? obs_layout(t, obs, obs_scale, n_ex, n_t, n_obs, me, ls, censor, family) : std::string("NULL t or obs");
    if (multi && !bad.empty()) return smc_fail(c, ("smc_set_model_user3: " + bad).c_str());
    // count outputs: the words that hold the sum of log s_k, which a noise model does not read, hold C_e (user_count.h) - in the
    // image and in the constants of user_finish_noise_kernel alike.  The image does not grow.
    if (family) ls = count_floor_sums(t, obs, n_ex, n_t, n_obs, family);
    if (multi && !nz && user_lds_bytes3(n_states, n_ex, n_t, n_obs) > kUserLdsCap)
        return smc_fail(c, "smc_set_model_user3: data set too large for the kernel's LDS table ((8 + 2 n_ex + n_ex (n_t + 1) "
                           "(n_obs + 2 rounded down to even)) x 8 B + pools > 150 KB)");
    if (nz && censor && user_lds_bytes3(n_states, n_ex, n_t, n_obs, true, true) > kUserLdsCap)
        return smc_fail(c, ("smc_set_model_user7: data set too large for the kernel's LDS table with the flags of censored observations "
                            "((8 + 2 n_ex + n_ex (n_t + 1) (n_obs + 3 rounded down to even) + 40 + 8 n_ex) x 8 B + pools): " +
                            std::to_string(user_lds_bytes3(n_states, n_ex, n_t, n_obs, true, true)) + " B needed, " + std::to_string(kUserLdsCap) +
                            " B available").c_str());
    if (nz && user_lds_bytes3(n_states, n_ex, n_t, n_obs, true) > kUserLdsCap)
        return smc_fail(c, ("smc_set_model_user4: data set too large for the kernel's LDS table ((8 + 2 n_ex + n_ex (n_t + 1) (n_obs + 2 "
                            "rounded down to even) + 40 + 8 n_ex) x 8 B + pools): " +
                            std::to_string(user_lds_bytes3(n_states, n_ex, n_t, n_obs, true)) + " B needed, " + std::to_string(kUserLdsCap) +
                            " B available").c_str());
    UserSourceSpec sp;
    sp.n_states = n_states, sp.dim = c->dim, sp.method = method, sp.n_obs = multi ? n_obs : 0;
    sp.noise = nz ? 1 + nz->prop : 0, sp.censor = censor ? 1 : 0;
    UserInputGeom &geom = sp.geom;
    std::vector<double> rows;      // the cond rows of a model with inputs, the table behind each
    if (in) {
        std::vector<int> knots;
        const std::string bad_in = input_layout_error(in->in_t, in->in_u, n_ex, in->n_in, in->n_knot, knots);
        if (!bad_in.empty()) return smc_fail(c, ("smc_set_model_user5: " + bad_in).c_str());
        if (n_cond > 0 && !cond) return smc_fail(c, "smc_set_model_user5: n_cond > 0 and cond is NULL");
        geom.n_cond = n_cond;
        geom.n_in = in->n_in;
        geom.kcap = knot_capacity(in->n_knot);
        rows = build_input_rows(cond, geom, in->in_t, in->in_u, n_ex, in->n_knot, knots);
    }
    if (ev) {
        std::vector<int> events;
        const std::string bad_ev = t ? event_layout_error(t, ev->ev_t, ev->ev_v, n_ex, n_t, ev->n_ev, ev->n_val, events) : std::string("NULL t");
        if (!bad_ev.empty()) return smc_fail(c, ("smc_set_model_user6: " + bad_ev).c_str());
        if (n_cond > 0 && !cond) return smc_fail(c, "smc_set_model_user6: n_cond > 0 and cond is NULL");
        geom.n_cond = n_cond;
        geom.n_ev = ev->n_ev;
        geom.n_val = ev->n_val;
        rows = build_event_rows(in ? rows.data() : cond, geom, ev->ev_t, ev->ev_v, n_ex, ev->n_ev, events);
    }
    if (hipSetDevice(c->device) != hipSuccess) return smc_fail(c, "hipSetDevice failed");
    std::vector<char> code;
    std::string lg;
    if (!compile_user(s.source, sp, code, lg)) {
        std::string msg = "user model does not compile:\n" + lg;
        if (msg.size() > 3500) msg.resize(3500);
        return smc_fail(c, msg.c_str());
    }
    (void)hipStreamSynchronize(c->stream);
    user_model_release(c);
    UserModel *u = new UserModel();
    c->user = u;
    if (hipModuleLoadData(&u->module, code.data()) != hipSuccess ||
        hipModuleGetFunction(&u->fn, u->module, "smc_user_solve_kernel") != hipSuccess ||
        (multi && hipModuleGetFunction(&u->fn_pred, u->module, "smc_user_predict_kernel") != hipSuccess)) {
        user_model_release(c);
        return smc_fail(c, "smc_set_model_user: loading the compiled module failed");
    }
    if (mentions(s.source, "smc_user_cost") && hipModuleGetFunction(&u->fn_scan, u->module, "smc_user_cost_scan_kernel") != hipSuccess) {
        user_model_release(c);
        return smc_fail(c, "smc_set_model_user: the source mentions smc_user_cost but the scan kernel is missing from the module");
    }
    const size_t nt = (size_t)n_ex * n_t * sizeof(double);
    const bool tabled = in || ev;      // the cond rows carry a table
    const size_t nc = tabled ? rows.size() * sizeof(double) : (size_t)n_ex * (n_cond > 0 ? n_cond : 1) * sizeof(double);
    bool ok = hipMalloc(&u->data.d_cond, nc) == hipSuccess;
    if (ok && !multi)      // the one-output kernel reads the data itself
        ok = hipMalloc(&u->d_t, nt) == hipSuccess && hipMalloc(&u->d_obs, nt) == hipSuccess &&
             hipMemcpy(u->d_t, t, nt, hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(u->d_obs, obs, nt, hipMemcpyHostToDevice) == hipSuccess;
    if (ok && tabled) ok = hipMemcpy(u->data.d_cond, rows.data(), nc, hipMemcpyHostToDevice) == hipSuccess;
    if (ok && !tabled && n_cond > 0) ok = hipMemcpy(u->data.d_cond, cond, nc, hipMemcpyHostToDevice) == hipSuccess;
    {   // likelihood constants; and the image (one-output model: only if its data is what smc_set_model_user3 would accept)
        std::vector<double> k(2 * (size_t)n_ex, 0.0);
        for (int e = 0; e < n_ex; ++e) {
            k[e] = multi ? me[e] : (double)n_t;
            k[n_ex + e] = multi ? ls[e] : 0.0;
        }
        if (nz) {      // user_finish_noise_kernel: m_ek follows
            const std::vector<double> mek = count_mek(t, obs, n_ex, n_t, n_obs, censor, family);
            k.insert(k.end(), mek.begin(), mek.end());
        }
        ok = ok && hipMalloc(&u->data.d_const, k.size() * sizeof(double)) == hipSuccess &&
             hipMemcpy(u->data.d_const, k.data(), k.size() * sizeof(double), hipMemcpyHostToDevice) == hipSuccess;
        if (bad.empty() && !multi) {
            for (int e = 0; e < n_ex; ++e)
                if (me[e] != (double)n_t) bad = "a missing observation (NaN)";
        }
        if (bad.empty()) {
            const std::vector<double> img = build_obs_image(t, obs, obs_scale, n_ex, n_t, n_obs, me, ls, nz, censor != nullptr, censor, family);
            u->data.img_len = (int)img.size();
            ok = ok && hipMalloc(&u->data.d_img, img.size() * sizeof(double)) == hipSuccess &&
                 hipMemcpy(u->data.d_img, img.data(), img.size() * sizeof(double), hipMemcpyHostToDevice) == hipSuccess;
            std::vector<double> cv, cf;      // the pointwise kernels' tables
            std::vector<int> cc;
            build_cell_tables(t, obs, n_ex, n_t, n_obs, censor, family, cv, cc, cf);
            ok = ok && hipMalloc(&u->d_cell_obs, cv.size() * sizeof(double)) == hipSuccess &&
                 hipMalloc(&u->d_cell_floor, cf.size() * sizeof(double)) == hipSuccess &&
                 hipMalloc(&u->d_cell_code, cc.size() * sizeof(int)) == hipSuccess &&
                 hipMemcpy(u->d_cell_obs, cv.data(), cv.size() * sizeof(double), hipMemcpyHostToDevice) == hipSuccess &&
                 hipMemcpy(u->d_cell_floor, cf.data(), cf.size() * sizeof(double), hipMemcpyHostToDevice) == hipSuccess &&
                 hipMemcpy(u->d_cell_code, cc.data(), cc.size() * sizeof(int), hipMemcpyHostToDevice) == hipSuccess;
        } else {
            u->img_error = "smc_user_predict: the data of this model (set through smc_set_model_user / smc_set_model_user2) cannot be "
                           "predicted: " + bad + "; set it through smc_set_model_user3";
        }
    }
    if (ok && !c->d_mlk2) ok = hipMalloc(&c->d_mlk2, (size_t)c->n_local * sizeof(double)) == hipSuccess;
    ok = ok && hipMalloc(&u->data.d_sum, (size_t)c->n_local * n_ex * sizeof(double)) == hipSuccess &&
         hipMalloc(&u->data.d_info, (size_t)c->n_local * n_ex * sizeof(int)) == hipSuccess;
    if (ok && method == SMC_USER_METHOD_BDF)
        ok = hipMalloc(&u->data.d_bdf_counts, (size_t)4 * c->n_local * n_ex * sizeof(unsigned)) == hipSuccess &&
             hipMalloc(&u->d_bdf_totals, 4 * sizeof(unsigned long long)) == hipSuccess &&
             hipMemset(u->d_bdf_totals, 0, 4 * sizeof(unsigned long long)) == hipSuccess;
    if (ok && u->fn_scan)
        ok = hipMalloc(&u->d_list, (size_t)c->n_local * sizeof(int32_t)) == hipSuccess &&
             hipMalloc(&u->d_listed, (size_t)c->n_local) == hipSuccess && hipMalloc(&u->d_count, 4 * sizeof(unsigned)) == hipSuccess &&
             hipMemset(u->d_count, 0, 4 * sizeof(unsigned)) == hipSuccess;
    if (!ok) {
        user_model_release(c);
        return smc_fail(c, "smc_set_model_user: device allocation / upload failed");
    }
    u->n_obs = n_obs;
    u->multi = multi;
    if (nz) {
        u->noise = true;
        u->nz = *nz;
    }
    if (family) {
        u->count = true;
        for (int k = 0; k < n_obs; ++k) u->negbin |= family[k] == 2 ? 1u << k : 0u;
        for (int k = 0; k < n_obs; ++k) u->family[k] = family[k];
    }
    {   // occupancy of the compiled kernel with its pool in LDS
        int nb = 0;
        const size_t lds = multi ? user_lds_bytes3(n_states, n_ex, n_t, n_obs, nz != nullptr, censor != nullptr) : user_lds_bytes(n_states, n_ex, n_t);
        if (lds > kUserLdsCap) {
            user_model_release(c);
            return smc_fail(c, "smc_set_model_user: data set too large for the kernel's LDS table (n_ex * n_t * 16 B + pools > 150 KB)");
        }
        if (hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&nb, u->fn, 256, lds) == hipSuccess && nb >= 1) u->data.blocks_per_cu = nb;
        if (lds > 48 * 1024 &&
            hipFuncSetAttribute(reinterpret_cast<const void *>(u->fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
            user_model_release(c);
            return smc_fail(c, "smc_set_model_user: raising the dynamic LDS limit of the compiled kernel failed");
        }
    }
    u->source = s.source;
    u->spec = sp;
    u->h_rows.swap(rows);
    if (t) u->h_t.assign(t, t + (size_t)n_ex * n_t);
    if (n_cond > 0) u->h_cond.assign(cond, cond + (size_t)n_ex * n_cond);
    for (int k = 0; k < n_obs && obs_scale; ++k) u->scale[k] = obs_scale[k];
    u->data.n_ex = n_ex;
    u->data.n_t = n_t;
    u->n_cond = n_cond;
    u->est_sigma = plan.est_sigma;
    u->sigma_fixed = plan.sigma_fixed;
    u->rtol = s.rtol;
    u->atol = s.atol;
    if (multi && prepare_pred_kernel(c, u) != 0) {
        user_model_release(c);
        return 1;
    }
    c->model_kind = 3;
    c->have_model = true;
    return 0;
}

int smc_set_model_user_spec(smc_ctx *c, const smc_user_model_spec *spec) {
    smc_user_model_spec s;
    if (!user_spec_copy(spec, offsetof(smc_user_model_spec, in_t), &s, sizeof s))
        return smc_fail(c, "smc_set_model_user_spec: NULL spec, or a struct_size that ends before in_t or exceeds this library's struct");
    return set_model_user_impl(c, s, "smc_set_model_user_spec");
}

// The earlier entry points: each fills the fields it knows, in the struct's order, and leaves the rest zero.  Those that take an
// n_obs never meant the one-output model by it (obs_or_bad: one out of range fails as it always did).
int smc_set_model_user(smc_ctx *c, const char *source, int n_states, const double *t, const double *obs, const double *cond,
                       int n_ex, int n_t, int n_cond, int est_sigma, double sigma_fixed, double rtol, double atol) {
    return smc_set_model_user2(c, source, n_states, t, obs, cond, n_ex, n_t, n_cond, est_sigma, sigma_fixed, rtol, atol, SMC_USER_METHOD_RK45);
}
int smc_set_model_user2(smc_ctx *c, const char *source, int n_states, const double *t, const double *obs, const double *cond,
                        int n_ex, int n_t, int n_cond, int est_sigma, double sigma_fixed, double rtol, double atol, int method) {
    return set_model_user_impl(c, {sizeof(smc_user_model_spec), source, n_states, method, 0, t, obs, cond, nullptr, n_ex, n_t, n_cond,
                                   est_sigma, sigma_fixed, nullptr, nullptr, nullptr, nullptr, rtol, atol}, nullptr);
}
int smc_set_model_user3(smc_ctx *c, const char *source, int n_states, int n_obs, const double *t, const double *obs, const double *cond,
                        const double *obs_scale, int n_ex, int n_t, int n_cond, int est_sigma, double sigma_fixed, double rtol,
                        double atol, int method) {
    return set_model_user_impl(c, {sizeof(smc_user_model_spec), source, n_states, method, obs_or_bad(n_obs), t, obs, cond, obs_scale,
                                   n_ex, n_t, n_cond, est_sigma, sigma_fixed, nullptr, nullptr, nullptr, nullptr, rtol,
                                   atol}, nullptr);
}
int smc_set_model_user4(smc_ctx *c, const char *source, int n_states, int n_obs, const double *t, const double *obs, const double *cond,
                        const double *obs_scale, int n_ex, int n_t, int n_cond, const int *add_index, const double *add_fixed,
                        const int *prop_index, const double *prop_fixed, double rtol, double atol, int method) {
    if (c && !add_index)      // no sigma rule here: the specification's own rules say what is missing
        return smc_fail(c, ("smc_set_model_user4: " + noise_spec_error(n_obs, c->dim, add_index, add_fixed, prop_index, prop_fixed)).c_str());
    return set_model_user_impl(c, {sizeof(smc_user_model_spec), source, n_states, method, obs_or_bad(n_obs), t, obs, cond, obs_scale,
                                   n_ex, n_t, n_cond, 0, 0.0, add_index, add_fixed, prop_index, prop_fixed, rtol, atol}, nullptr);
}
int smc_set_model_user5(smc_ctx *c, const char *source, int n_states, int n_obs, const double *t, const double *obs, const double *cond,
                        const double *obs_scale, int n_ex, int n_t, int n_cond, const int *add_index, const double *add_fixed,
                        const int *prop_index, const double *prop_fixed, double rtol, double atol, int method, int est_sigma,
                        double sigma_fixed, const double *in_t, const double *in_u, int n_in, int n_knot) {
    return set_model_user_impl(c, {sizeof(smc_user_model_spec), source, n_states, method, obs_or_bad(n_obs), t, obs, cond, obs_scale,
                                   n_ex, n_t, n_cond, est_sigma, sigma_fixed, add_index, add_fixed, prop_index, prop_fixed, rtol,
                                   atol, in_t, in_u, n_in, n_knot}, nullptr);
}
int smc_set_model_user6(smc_ctx *c, const char *source, int n_states, int n_obs, const double *t, const double *obs, const double *cond,
                        const double *obs_scale, int n_ex, int n_t, int n_cond, const int *add_index, const double *add_fixed,
                        const int *prop_index, const double *prop_fixed, double rtol, double atol, int method, int est_sigma,
                        double sigma_fixed, const double *in_t, const double *in_u, int n_in, int n_knot, const double *ev_t,
                        const double *ev_v, int n_ev, int n_val) {
    return set_model_user_impl(c, {sizeof(smc_user_model_spec), source, n_states, method, obs_or_bad(n_obs), t, obs, cond, obs_scale,
                                   n_ex, n_t, n_cond, est_sigma, sigma_fixed, add_index, add_fixed, prop_index, prop_fixed, rtol,
                                   atol, in_t, in_u, n_in, n_knot, ev_t, ev_v, n_ev, n_val}, nullptr);
}
int smc_set_model_user7(smc_ctx *c, const char *source, int n_states, int n_obs, const double *t, const double *obs, const double *cond,
                        const double *obs_scale, int n_ex, int n_t, int n_cond, const int *add_index, const double *add_fixed,
                        const int *prop_index, const double *prop_fixed, double rtol, double atol, int method, int est_sigma,
                        double sigma_fixed, const double *in_t, const double *in_u, int n_in, int n_knot, const double *ev_t,
                        const double *ev_v, int n_ev, int n_val, const signed char *censor) {
    return set_model_user_impl(c, {sizeof(smc_user_model_spec), source, n_states, method, obs_or_bad(n_obs), t, obs, cond, obs_scale,
                                   n_ex, n_t, n_cond, est_sigma, sigma_fixed, add_index, add_fixed, prop_index, prop_fixed, rtol,
                                   atol, in_t, in_u, n_in, n_knot, ev_t, ev_v, n_ev, n_val, censor}, nullptr);
}

int smc_user_spec_layout(int which, int *offsets, int cap) {
#define SRC(f) (int)offsetof(smc_user_source_spec, f)
#define MOD(f) (int)offsetof(smc_user_model_spec, f)
    static const int src[] = {SRC(struct_size), SRC(source), SRC(n_states), SRC(dim), SRC(method), SRC(n_obs), SRC(noise), SRC(n_cond), SRC(n_in),
                              SRC(n_knot), SRC(n_ev), SRC(n_val), SRC(censor)};
    static const int mod[] = {MOD(struct_size), MOD(source), MOD(n_states), MOD(method), MOD(n_obs), MOD(t), MOD(obs), MOD(cond), MOD(obs_scale),
                              MOD(n_ex), MOD(n_t), MOD(n_cond), MOD(est_sigma), MOD(sigma_fixed), MOD(add_index), MOD(add_fixed), MOD(prop_index),
                              MOD(prop_fixed), MOD(rtol), MOD(atol), MOD(in_t), MOD(in_u), MOD(n_in), MOD(n_knot), MOD(ev_t), MOD(ev_v), MOD(n_ev),
                              MOD(n_val), MOD(censor)};
#undef SRC
#undef MOD
    if (which != 0 && which != 1) return -1;
    const int n = which == 0 ? (int)(sizeof src / sizeof src[0]) : (int)(sizeof mod / sizeof mod[0]);
    for (int i = 0; i < n && i < cap && offsets; ++i) offsets[i] = which == 0 ? src[i] : mod[i];
    return which == 0 ? (int)sizeof(smc_user_source_spec) : (int)sizeof(smc_user_model_spec);
}

int smc_user_set_design_events(smc_ctx *c, const double *ev_t_new, const double *ev_v_new, int n_ex_new, int n_ev_new) {
    if (!c) return smc_fail(nullptr, "NULL context");
    UserModel *u = (UserModel *)c->user;
    if (c->model_kind != 3 || !u || !c->have_model) return smc_fail(c, "smc_user_set_design_events: no user model has been set");
    if (!ev_t_new && !ev_v_new) {
        u->design_ev_t.clear();
        u->design_ev_v.clear();
        u->design_ev_n_ex = u->design_ev_n_ev = 0;
        return 0;
    }
    if (u->spec.geom.n_ev == 0) return smc_fail(c, "smc_user_set_design_events: the model has no events (set it through smc_set_model_user6)");
    if (n_ev_new > u->spec.geom.n_ev)
        return smc_fail(c, ("smc_user_set_design_events: n_ev_new = " + std::to_string(n_ev_new) + " above the event capacity " +
                            std::to_string(u->spec.geom.n_ev) + " the model was compiled for (its n_ev)").c_str());
    std::vector<int> events;      // the rule about t[e][0] waits for the design's times (resolve_design)
    const std::string bad = event_layout_error(nullptr, ev_t_new, ev_v_new, n_ex_new, 0, n_ev_new, u->spec.geom.n_val, events);
    if (!bad.empty()) return smc_fail(c, ("smc_user_set_design_events: " + bad + " (of the design)").c_str());
    u->design_ev_t.assign(ev_t_new, ev_t_new + (size_t)n_ex_new * n_ev_new);
    u->design_ev_v.clear();
    if (ev_v_new) u->design_ev_v.assign(ev_v_new, ev_v_new + (size_t)n_ex_new * n_ev_new * u->spec.geom.n_val);
    u->design_ev_n_ex = n_ex_new;
    u->design_ev_n_ev = n_ev_new;
    return 0;
}

int smc_user_set_design_inputs(smc_ctx *c, const double *in_t_new, const double *in_u_new, int n_ex_new, int n_knot_new) {
    if (!c) return smc_fail(nullptr, "NULL context");
    UserModel *u = (UserModel *)c->user;
    if (c->model_kind != 3 || !u || !c->have_model) return smc_fail(c, "smc_user_set_design_inputs: no user model has been set");
    if (!in_t_new && !in_u_new) {
        u->design_t.clear();
        u->design_u.clear();
        u->design_n_ex = u->design_n_knot = 0;
        return 0;
    }
    if (u->spec.geom.n_in == 0) return smc_fail(c, "smc_user_set_design_inputs: the model has no inputs (set it through smc_set_model_user5)");
    std::vector<int> knots;
    const std::string bad = input_layout_error(in_t_new, in_u_new, n_ex_new, u->spec.geom.n_in, n_knot_new, knots);
    if (!bad.empty()) return smc_fail(c, ("smc_user_set_design_inputs: " + bad + " (of the design)").c_str());
    for (int e = 0; e < n_ex_new; ++e)
        if (knots[e] > u->spec.geom.kcap)
            return smc_fail(c, ("smc_user_set_design_inputs: row " + std::to_string(e) + " of in_t has " + std::to_string(knots[e]) +
                                " knots, above the knot capacity " + std::to_string(u->spec.geom.kcap) +
                                " the model was compiled for (the power of two >= its n_knot)").c_str());
    u->design_t.assign(in_t_new, in_t_new + (size_t)n_ex_new * n_knot_new);
    u->design_u.assign(in_u_new, in_u_new + (size_t)n_ex_new * n_knot_new * u->spec.geom.n_in);
    u->design_n_ex = n_ex_new;
    u->design_n_knot = n_knot_new;
    return 0;
}

// the noise of every output as the pointwise kernels take it: the model's noise model, or the sigma rule written as one
static PointwiseArgs pointwise_args_of(const smc_ctx *c, const UserModel *u) {
    PointwiseArgs a{};
    if (u->noise) {
        a.nz = u->nz;
    } else {
        for (int k = 0; k < kUserMaxObs; ++k) {
            a.nz.add_index[k] = u->est_sigma ? c->dim - 1 : -1;
            a.nz.add_fixed[k] = u->sigma_fixed;
            a.nz.prop_index[k] = -1;
            a.nz.prop_fixed[k] = 0.0;
            a.nz.scale[k] = u->scale[k];
        }
        a.nz.prop = 0;
    }
    for (int k = 0; k < kUserMaxObs; ++k) a.family[k] = u->family[k];
    a.n_obs = u->n_obs;
    a.cell_obs = u->d_cell_obs;
    a.cell_code = u->d_cell_code;
    a.cell_floor = u->d_cell_floor;
    return a;
}

// smc_user_predict, and with ll != nullptr smc_user_pointwise: the terms of every chunk's predictions, particle-major like pred
static int user_predict_impl(smc_ctx *c, const char *who, const double *particle, int64_t n, double *lk, double *pred, double *ll,
                             int64_t *n_failed, int64_t *attempts) {
    if (!c) return smc_fail(nullptr, "NULL context");
    UserModel *u = (UserModel *)c->user;
    if (c->model_kind != 3 || !u || !c->have_model) return smc_fail(c, (std::string(who) + ": no user model has been set").c_str());
    if (n < 0 || (n > 0 && (!particle || !lk))) return smc_fail(c, (std::string(who) + ": bad arguments").c_str());
    if (hipSetDevice(c->device) != hipSuccess) return smc_fail(c, "hipSetDevice failed");
    if (n_failed) *n_failed = 0;
    if (attempts) *attempts = 0;
    if (n == 0) return 0;
    if (!u->data.d_img) return smc_fail(c, u->img_error.c_str());
    // a one-output model of smc_set_model_user / 2: its prediction kernel, compiled once (a multi-output model's data has been
    // held to the cap when it was set)
    if (!u->fn_pred && user_lds_bytes3(u->spec.n_states, u->data.n_ex, u->data.n_t, 1) > kUserLdsCap)
        return smc_fail(c, "smc_user_predict: data set too large for the prediction kernel's LDS table");
    if (ensure_pred_kernel(c, u, "smc_user_predict") != 0) return 1;
    const int dim = c->dim;
    const int64_t chunk = n < c->n_local ? n : c->n_local;      // the per-item buffers hold n_local particles
    const size_t per = (size_t)u->data.n_ex * u->data.n_t * u->n_obs;
    if (chunk > u->p_cap) {
        (void)hipFree(u->d_pt);
        (void)hipFree(u->d_plk);
        (void)hipFree(u->d_ppred);
        u->d_pt = u->d_plk = u->d_ppred = nullptr;
        u->p_cap = 0;
        if (hipMalloc(&u->d_pt, (size_t)chunk * dim * 2 * sizeof(double)) != hipSuccess ||
            hipMalloc(&u->d_plk, (size_t)chunk * sizeof(double)) != hipSuccess ||
            hipMalloc(&u->d_ppred, (size_t)chunk * per * sizeof(double)) != hipSuccess)
            return smc_fail(c, "smc_user_predict: device allocation failed");
        u->p_cap = chunk;
    }
    if (ll && chunk > u->pll_cap) {
        (void)hipFree(u->d_pll);
        u->d_pll = nullptr;
        u->pll_cap = 0;
        if (hipMalloc(&u->d_pll, (size_t)chunk * per * sizeof(double)) != hipSuccess) return smc_fail(c, (std::string(who) + ": device allocation failed").c_str());
        u->pll_cap = chunk;
    }
    double *aos = u->d_pt, *soa = u->d_pt + (size_t)u->p_cap * dim;
    if (hipMemsetAsync(c->d_counters, 0, sizeof(SweepCounters), c->stream) != hipSuccess ||
        (u->spec.method == SMC_USER_METHOD_BDF && hipMemsetAsync(u->d_bdf_totals, 0, 4 * sizeof(unsigned long long), c->stream) != hipSuccess))
        return smc_fail(c, "smc_user_predict: clearing the counters failed");
    for (int64_t off = 0; off < n; off += chunk) {
        const int64_t m = (n - off < chunk) ? n - off : chunk;
        if (hipMemcpyAsync(aos, particle + off * dim, (size_t)m * dim * sizeof(double), hipMemcpyHostToDevice, c->stream) != hipSuccess)
            return smc_fail(c, "smc_user_predict: upload failed");
        launch_aos_to_soa(c, aos, soa, m, dim, m);
        launch_user_kernel(c, u->pred_data(), soa, m, m, nullptr, u->d_plk, false, u->d_ppred);
        if (c->launch_failed) {
            c->launch_failed = false;
            return 1;
        }
        if (ll) {
            PointwiseArgs a = pointwise_args_of(c, u);
            a.pred = u->d_ppred;
            a.ll = u->d_pll;
            a.n = m;
            a.cells = (int)per;
            a.cells_total = (int64_t)per;
            a.theta = soa;
            a.stride = m;
            launch_pointwise(c, a);
            if (hipMemcpyAsync(ll + (size_t)off * per, u->d_pll, (size_t)m * per * sizeof(double), hipMemcpyDeviceToHost, c->stream) != hipSuccess)
                return smc_fail(c, (std::string(who) + ": download failed").c_str());
        }
        if (hipMemcpyAsync(lk + off, u->d_plk, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
            (pred && hipMemcpyAsync(pred + (size_t)off * per, u->d_ppred, (size_t)m * per * sizeof(double), hipMemcpyDeviceToHost,
                                    c->stream) != hipSuccess))
            return smc_fail(c, "smc_user_predict: download failed");
    }
    if (hipMemcpyAsync(c->h_counters, c->d_counters, sizeof(SweepCounters), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess)
        return smc_fail(c, (std::string("smc_user_predict: ") + hipGetErrorString(hipGetLastError())).c_str());
    if (n_failed) *n_failed = (int64_t)c->h_counters->n_failed;
    if (attempts) *attempts = (int64_t)c->h_counters->rk_attempts;
    return 0;
}
int smc_user_predict(smc_ctx *c, const double *particle, int64_t n, double *lk, double *pred, int64_t *n_failed, int64_t *attempts) {
    return user_predict_impl(c, "smc_user_predict", particle, n, lk, pred, nullptr, n_failed, attempts);
}
int smc_user_pointwise(smc_ctx *c, const double *particle, int64_t n, double *ll, int64_t *n_failed, int64_t *attempts) {
    if (!c) return smc_fail(nullptr, "NULL context");
    if (n > 0 && !ll) return smc_fail(c, "smc_user_pointwise: NULL result array");
    std::vector<double> lk((size_t)(n > 0 ? n : 0) + 1);
    return user_predict_impl(c, "smc_user_pointwise", particle, n, lk.data(), nullptr, ll, n_failed, attempts);
}
// the design of a call: (t_new, cond_new) checked by the rules of smc_set_model_user3, or the data's own
// A model with inputs: cond becomes whole rows (cond_stride words, the table behind the numbers) - the data's own, or in `rows`
// those of cond_new and the design inputs of smc_user_set_design_inputs, which an explicit design must have.  A model with
// events: the same with the design events of smc_user_set_design_events.
static int resolve_design(smc_ctx *c, UserModel *u, const char *who, const double *&t, const double *&cond, int &n_ex, int &n_t,
                          std::vector<double> &rows) {
    const std::string w = std::string(who) + ": ";
    if (!t) {
        if (!u->data.d_img) return smc_fail(c, u->img_error.c_str());
        t = u->h_t.data();
        cond = u->spec.geom.tabled() ? u->h_rows.data() : u->h_cond.data();
        n_ex = u->data.n_ex;
        n_t = u->data.n_t;
        return 0;
    }
    if (n_ex < 1 || n_t < 1) return smc_fail(c, (w + "bad design shape").c_str());
    if (u->n_cond > 0 && !cond) return smc_fail(c, (w + "the model has n_cond > 0 and cond_new is NULL").c_str());
    const std::vector<double> nan_obs((size_t)n_ex * n_t * u->n_obs, std::nan(""));
    std::vector<double> me, ls;
    const std::string bad = obs_layout(t, nan_obs.data(), u->scale, n_ex, n_t, u->n_obs, me, ls);
    if (!bad.empty()) return smc_fail(c, (w + bad + " (t_new)").c_str());
    if (u->spec.geom.n_in > 0) {
        if (u->design_n_ex != n_ex)
            return smc_fail(c, (w + "the model has inputs and the design has no matching design inputs: " +
                                (u->design_n_ex ? "smc_user_set_design_inputs holds " + std::to_string(u->design_n_ex) + " rows"
                                                : std::string("none are set")) +
                                ", the design has " + std::to_string(n_ex) + " experiments (smc_user_set_design_inputs)").c_str());
        std::vector<int> knots;
        if (!input_layout_error(u->design_t.data(), u->design_u.data(), n_ex, u->spec.geom.n_in, u->design_n_knot, knots).empty())
            return smc_fail(c, (w + "the design inputs are no longer valid").c_str());
        // a row whose finite knots fit the capacity may still be stored wider (trailing NaN): only its knots are copied
        rows = build_input_rows(cond, u->spec.geom, u->design_t.data(), u->design_u.data(), n_ex, u->design_n_knot, knots);
        cond = rows.data();
    }
    if (u->spec.geom.n_ev > 0) {      // the what-if regimen: the design's own events, behind what the rows hold so far
        if (u->design_ev_n_ex != n_ex)
            return smc_fail(c, (w + "the model has events and the design has no matching design events: " +
                                (u->design_ev_n_ex ? "smc_user_set_design_events holds " + std::to_string(u->design_ev_n_ex) + " rows"
                                                   : std::string("none are set")) +
                                ", the design has " + std::to_string(n_ex) + " experiments (smc_user_set_design_events)").c_str());
        std::vector<int> events;
        const std::string bad_ev = event_layout_error(t, u->design_ev_t.data(), u->spec.geom.n_val > 0 ? u->design_ev_v.data() : nullptr, n_ex, n_t,
                                                      u->design_ev_n_ev, u->spec.geom.n_val, events);
        if (!bad_ev.empty()) return smc_fail(c, (w + bad_ev + " (of the design events)").c_str());
        rows = build_event_rows(cond, u->spec.geom, u->design_ev_t.data(), u->design_ev_v.data(), n_ex, u->design_ev_n_ev, events);
        cond = rows.data();
    }
    return 0;
}
static int design_too_large(smc_ctx *c, const UserModel *u, const char *who, int n_t) {
    return smc_fail(c, (std::string(who) + ": one row of the design does not fit the kernel's LDS table: " +
                        std::to_string(user_lds_bytes3(u->spec.n_states, 1, n_t, u->n_obs, u->noise, u->spec.censor != 0)) + " B needed, " + std::to_string(kUserLdsCap) +
                        " B available").c_str());
}

int smc_user_predict_at(smc_ctx *c, const double *particle, int64_t n, const double *t_new, const double *cond_new, int n_ex_new,
                        int n_t_new, double *pred, int64_t *n_failed, int64_t *attempts) {
    if (!c) return smc_fail(nullptr, "NULL context");
    UserModel *u = (UserModel *)c->user;
    if (c->model_kind != 3 || !u || !c->have_model) return smc_fail(c, "smc_user_predict_at: no user model has been set");
    if (n < 0 || (n > 0 && (!particle || !pred))) return smc_fail(c, "smc_user_predict_at: bad arguments");
    if (!t_new) {       // the data's design: smc_user_predict itself
        std::vector<double> lk((size_t)n);
        return smc_user_predict(c, particle, n, lk.data(), pred, n_failed, attempts);
    }
    if (hipSetDevice(c->device) != hipSuccess) return smc_fail(c, "hipSetDevice failed");
    if (n_failed) *n_failed = 0;
    if (attempts) *attempts = 0;
    const double *t = t_new, *cond = cond_new;
    int n_ex = n_ex_new, n_t = n_t_new;
    std::vector<double> design_rows;
    if (resolve_design(c, u, "smc_user_predict_at", t, cond, n_ex, n_t, design_rows) != 0) return 1;
    if (n == 0) return 0;
    const int g_max = design_lds_group(u, n_ex, n_t);
    if (g_max < 1) return design_too_large(c, u, "smc_user_predict_at", n_t);
    if (ensure_pred_kernel(c, u, "smc_user_predict_at") != 0 || raise_pred_lds(c, u, "smc_user_predict_at") != 0) return 1;
    const int dim = c->dim;
    const int64_t chunk = n < c->n_local ? n : c->n_local;      // the scan lists of a model with a cost hint hold n_local particles
    const size_t row = (size_t)n_t * u->n_obs;                   // one experiment of one particle
    DesignRun run(c, u, "smc_user_predict_at");
    double *d_pt = nullptr;
    run.begin(run.alloc(t, cond, n_ex, n_t, chunk, g_max, 0) && hipMalloc(&d_pt, (size_t)chunk * dim * 2 * sizeof(double)) == hipSuccess);
    double *aos = d_pt, *soa = d_pt + (size_t)chunk * dim;
    for (int64_t off = 0; run.rc == 0 && off < n; off += chunk) {
        const int64_t m = (n - off < chunk) ? n - off : chunk;
        if (hipMemcpyAsync(aos, particle + off * dim, (size_t)m * dim * sizeof(double), hipMemcpyHostToDevice, c->stream) != hipSuccess) {
            run.fail("upload failed");
            break;
        }
        launch_aos_to_soa(c, aos, soa, m, dim, m);
        for (size_t k = 0; run.rc == 0 && k < run.groups.size(); ++k) {
            if (run.solve(k, soa, m, m) != 0) break;
            // the group's experiments of every particle into their place in pred[p][e][i][k]
            const DesignGroup &dg = run.groups[k];
            if (hipMemcpy2DAsync(pred + ((size_t)off * n_ex + dg.e0) * row, (size_t)n_ex * row * sizeof(double), run.d_ppred,
                                 (size_t)dg.d.n_ex * row * sizeof(double), (size_t)dg.d.n_ex * row * sizeof(double), (size_t)m,
                                 hipMemcpyDeviceToHost, c->stream) != hipSuccess)
                run.fail("download failed");
        }
    }
    run.finish(n_failed, attempts, nullptr);
    (void)hipFree(d_pt);
    return run.rc;
}

int smc_user_predict_summary(smc_ctx *c, int set, const double *t_new, const double *cond_new, int n_ex_new, int n_t_new,
                             const double *probs, int n_probs, int noise, uint64_t seed, int64_t global_offset, size_t max_staging_bytes,
                             double *mean, double *sd, double *lower, double *upper, int64_t *n_finite, int64_t *n_failed,
                             int64_t *attempts, double *kernel_ms) {
    const char *who = "smc_user_predict_summary";
    if (!c) return smc_fail(nullptr, "NULL context");
    UserModel *u = (UserModel *)c->user;
    if (c->model_kind != 3 || !u || !c->have_model) return smc_fail(c, "smc_user_predict_summary: no user model has been set");
    if (set != SMC_SET_PRED && set != SMC_SET_FILT) return smc_fail(c, "smc_user_predict_summary: set must be SMC_SET_PRED or SMC_SET_FILT");
    if (n_probs < 1 || n_probs > smc_sel::kMaxProbs || !probs) return smc_fail(c, "smc_user_predict_summary: n_probs outside 1 .. 16");
    for (int j = 0; j < n_probs; ++j)
        if (!(probs[j] >= 0.0 && probs[j] <= 1.0)) return smc_fail(c, "smc_user_predict_summary: a probability outside [0, 1]");
    if (!mean || !sd || !lower || !upper || !n_finite) return smc_fail(c, "smc_user_predict_summary: NULL result array");
    if (noise != 0 && noise != SMC_PRED_NOISE_GAUSSIAN && noise != SMC_PRED_NOISE_FAMILY)
        return smc_fail(c, "smc_user_predict_summary: noise must be 0, 1 (SMC_PRED_NOISE_GAUSSIAN) or 2 (SMC_PRED_NOISE_FAMILY)");
    if (noise == SMC_PRED_NOISE_GAUSSIAN && u->count)
        return smc_fail(c, "smc_user_predict_summary: noise = 1 on a model with a count output: replicated count draws need a Poisson / gamma "
                           "sampler on the Philox stream, which noise = 1 does not call: noise = 2 (SMC_PRED_NOISE_FAMILY) draws every "
                           "output under its family (noise = 0 gives the bands of the mean)");
    if (hipSetDevice(c->device) != hipSuccess) return smc_fail(c, "hipSetDevice failed");
    if (n_failed) *n_failed = 0;
    if (attempts) *attempts = 0;
    if (kernel_ms) kernel_ms[0] = kernel_ms[1] = 0.0;
    const double *t = t_new, *cond = cond_new;
    int n_ex = n_ex_new, n_t = n_t_new;
    std::vector<double> design_rows;
    if (resolve_design(c, u, who, t, cond, n_ex, n_t, design_rows) != 0) return 1;
    const int64_t n = c->n_local;
    const int g_lds = design_lds_group(u, n_ex, n_t);
    if (g_lds < 1) return design_too_large(c, u, who, n_t);
    // staging: per experiment the predictions and their keys (n x n_t x n_obs words each) and the per-item words of a launch;
    // once, the likelihoods the finish kernel writes and the results
    const size_t row = (size_t)n_t * u->n_obs;
    const int64_t cells_total = (int64_t)n_ex * (int64_t)row;
    const size_t out_words = (size_t)cells_total * (3 + 2 * (size_t)n_probs);
    const size_t per_ex = (size_t)n * (row * sizeof(double) + design_item_bytes(u)) + pred_summary_key_bytes(n, (int)row);
    const size_t fixed = (size_t)n * sizeof(double) + out_words * sizeof(double);
    const int g_max = design_staging_group(c, who, "keys", max_staging_bytes, fixed, per_ex, n, g_lds, n_ex);
    if (g_max < 1) return 1;
    if (ensure_pred_kernel(c, u, who) != 0 || raise_pred_lds(c, u, who) != 0) return 1;

    DesignRun run(c, u, who);
    unsigned long long *d_keys = nullptr;
    run.begin(run.alloc(t, cond, n_ex, n_t, n, g_max, out_words) && hipMalloc(&d_keys, pred_summary_key_bytes(n, (int)(g_max * row))) == hipSuccess);
    const ParticleSet &P = c->set[set];
    for (size_t k = 0; run.rc == 0 && k < run.groups.size(); ++k) {
        if (run.solve(k, P.theta, P.stride, n) != 0) break;
        const DesignGroup &dg = run.groups[k];
        PredSummaryArgs a{};
        a.pred = run.d_ppred;
        a.keys = d_keys;
        a.n = n;
        a.cells = (int)(dg.d.n_ex * row);
        a.cell_base = (int64_t)dg.e0 * (int64_t)row;      // the GLOBAL cell index keys the noise: grouping cannot change a result
        a.cells_total = cells_total;
        a.n_obs = u->n_obs;
        a.noise = noise != 0;
        for (int j = 0; j < kUserMaxObs; ++j) a.family[j] = (noise == SMC_PRED_NOISE_FAMILY && u->count) ? u->family[j] : 0;
        a.theta = P.theta;
        a.stride = P.stride;
        a.dim = c->dim;
        a.est_sigma = u->est_sigma;
        a.sigma_fixed = u->sigma_fixed;
        for (int j = 0; j < kUserMaxObs; ++j) a.scale[j] = u->scale[j];
        a.has_noise_model = u->noise ? 1 : 0;
        a.nz = u->nz;
        a.seed = seed;
        a.global_offset = global_offset;
        a.n_probs = n_probs;
        for (int j = 0; j < n_probs; ++j) a.probs[j] = probs[j];
        a.out = run.d_out;
        launch_pred_summary(c, a);
        run.stamp(k);
    }
    if (run.finish(n_failed, attempts, kernel_ms) == 0) {
        const std::vector<double> &h_out = run.h_out;
        const size_t ct = (size_t)cells_total;
        for (size_t i = 0; i < ct; ++i) {
            mean[i] = h_out[i];
            sd[i] = h_out[ct + i];
            n_finite[i] = (int64_t)h_out[2 * ct + i];
        }
        for (size_t i = 0; i < ct * (size_t)n_probs; ++i) {
            lower[i] = h_out[3 * ct + i];
            upper[i] = h_out[(3 + (size_t)n_probs) * ct + i];
        }
    }
    (void)hipFree(d_keys);
    return run.rc;
}

int smc_user_pointwise_summary(smc_ctx *c, int set, size_t max_staging_bytes, int64_t *n_terms, double *max, double *sum_exp, double *mean,
                               double *m2, double *pit, int64_t *n_failed, int64_t *attempts, double *kernel_ms) {
    return smc_user_pointwise_summary_opt(c, set, max_staging_bytes, nullptr, n_terms, max, sum_exp, mean, m2, pit, n_failed, attempts, kernel_ms);
}

int smc_user_pointwise_summary_opt(smc_ctx *c, int set, size_t max_staging_bytes, const smc_pointwise_opts *opts, int64_t *n_terms, double *max,
                                   double *sum_exp, double *mean, double *m2, double *pit, int64_t *n_failed, int64_t *attempts,
                                   double *kernel_ms) {
    const char *who = "smc_user_pointwise_summary";
    if (!c) return smc_fail(nullptr, "NULL context");
    const bool count_pit = opts && opts->count_pit != 0;
    if (count_pit && (!opts->pit_below || !opts->pit_equal || !opts->pit_n))
        return smc_fail(c, "smc_user_pointwise_summary_opt: count_pit with a NULL pit_below, pit_equal or pit_n");
    UserModel *u = (UserModel *)c->user;
    if (c->model_kind != 3 || !u || !c->have_model) return smc_fail(c, "smc_user_pointwise_summary: no user model has been set");
    if (set != SMC_SET_PRED && set != SMC_SET_FILT) return smc_fail(c, "smc_user_pointwise_summary: set must be SMC_SET_PRED or SMC_SET_FILT");
    if (!n_terms || !max || !sum_exp || !mean || !m2 || !pit) return smc_fail(c, "smc_user_pointwise_summary: NULL result array");
    if (hipSetDevice(c->device) != hipSuccess) return smc_fail(c, "hipSetDevice failed");
    if (n_failed) *n_failed = 0;
    if (attempts) *attempts = 0;
    if (kernel_ms) kernel_ms[0] = kernel_ms[1] = 0.0;
    const double *t = nullptr, *cond = nullptr;      // the data's design: there are no observations elsewhere
    int n_ex = 0, n_t = 0;
    std::vector<double> design_rows;
    if (resolve_design(c, u, who, t, cond, n_ex, n_t, design_rows) != 0) return 1;
    const int64_t n = c->n_local;
    const int g_lds = design_lds_group(u, n_ex, n_t);
    if (g_lds < 1) return design_too_large(c, u, who, n_t);
    // staging: per experiment the predictions and their terms (n x n_t x n_obs words each), the PIT partials (2 words per 32
    // particles and cell: 1/32 of the two) and the per-item words of a launch; once, the likelihoods the finish kernel writes and
    // the results
    const size_t row = (size_t)n_t * u->n_obs;
    const int64_t cells_total = (int64_t)n_ex * (int64_t)row;
    // the PIT of count cells: three more result rows and one word per 32 particles and cell; a model without count outputs has no
    // such cell - the counts are 0 and the kernels are the ones of a call without options
    const bool draw = count_pit && u->count;
    const size_t out_words = (size_t)cells_total * (kPwOutWords + (draw ? kPwCountWords : 0));
    const size_t per_ex = (size_t)n * (row * sizeof(double) + design_item_bytes(u)) + pointwise_terms_bytes(n, (int)row) + pointwise_pit_bytes(n, (int)row) +
                          (draw ? pointwise_pit_count_bytes(n, (int)row) : 0);
    const size_t fixed = (size_t)n * sizeof(double) + out_words * sizeof(double);
    const int g_max = design_staging_group(c, who, "terms", max_staging_bytes, fixed, per_ex, n, g_lds, n_ex);
    if (g_max < 1) return 1;
    if (ensure_pred_kernel(c, u, who) != 0 || raise_pred_lds(c, u, who) != 0) return 1;

    DesignRun run(c, u, who);
    double *d_terms = nullptr, *d_pit = nullptr;
    unsigned *d_cnt = nullptr;
    run.begin(run.alloc(t, cond, n_ex, n_t, n, g_max, out_words) &&
              hipMalloc(&d_terms, pointwise_terms_bytes(n, (int)(g_max * row))) == hipSuccess &&
              hipMalloc(&d_pit, pointwise_pit_bytes(n, (int)(g_max * row))) == hipSuccess &&
              (!draw || hipMalloc(&d_cnt, pointwise_pit_count_bytes(n, (int)(g_max * row))) == hipSuccess));
    const ParticleSet &P = c->set[set];
    for (size_t k = 0; run.rc == 0 && k < run.groups.size(); ++k) {
        if (run.solve(k, P.theta, P.stride, n) != 0) break;
        const DesignGroup &dg = run.groups[k];
        PointwiseArgs a = pointwise_args_of(c, u);
        a.pred = run.d_ppred;
        a.terms = d_terms;
        a.pit_part = d_pit;
        a.pit_cnt = d_cnt;
        a.seed = draw ? opts->seed : 0;
        a.global_offset = draw ? opts->global_offset : 0;
        a.n = n;
        a.cells = (int)(dg.d.n_ex * row);
        a.cell_base = (int64_t)dg.e0 * (int64_t)row;
        a.cells_total = cells_total;
        a.theta = P.theta;
        a.stride = P.stride;
        a.out = run.d_out;
        launch_pointwise(c, a);
        run.stamp(k);
    }
    if (run.finish(n_failed, attempts, kernel_ms) == 0) {
        const std::vector<double> &h_out = run.h_out;
        const size_t ct = (size_t)cells_total;
        for (size_t i = 0; i < ct; ++i) {
            n_terms[i] = (int64_t)h_out[i];
            max[i] = h_out[ct + i];
            sum_exp[i] = h_out[2 * ct + i];
            mean[i] = h_out[3 * ct + i];
            m2[i] = h_out[4 * ct + i];
            pit[i] = h_out[5 * ct + i];
        }
        for (size_t i = 0; count_pit && i < ct; ++i) {
            opts->pit_below[i] = draw ? (int64_t)h_out[(kPwOutWords + 0) * ct + i] : 0;
            opts->pit_equal[i] = draw ? (int64_t)h_out[(kPwOutWords + 1) * ct + i] : 0;
            opts->pit_n[i] = draw ? (int64_t)h_out[(kPwOutWords + 2) * ct + i] : 0;
        }
    }
    (void)hipFree(d_terms);
    (void)hipFree(d_pit);
    (void)hipFree(d_cnt);
    return run.rc;
}

int smc_user_sweep_counters(smc_ctx *c, int64_t out[4]) {
    if (!c) return smc_fail(nullptr, "NULL context");
    UserModel *u = (UserModel *)c->user;
    if (c->model_kind != 3 || !u || u->spec.method != SMC_USER_METHOD_BDF)
        return smc_fail(c, "smc_user_sweep_counters: the model is not a user model with method SMC_USER_METHOD_BDF");
    if (hipSetDevice(c->device) != hipSuccess) return smc_fail(c, "hipSetDevice failed");
    unsigned long long h[4];
    if (hipMemcpyAsync(h, u->d_bdf_totals, sizeof h, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess)
        return smc_fail(c, "smc_user_sweep_counters: copying the counters failed");
    for (int k = 0; k < 4; ++k) out[k] = (int64_t)h[k];
    return 0;
}

}  // extern "C"
