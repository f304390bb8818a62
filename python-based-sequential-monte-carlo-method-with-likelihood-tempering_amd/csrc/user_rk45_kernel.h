// user_rk45_kernel.h -- the RK45 integrator of user models (SMC_USER_METHOD_RK45, include/smc_hip.h).  Device code only: the
// library appends this text to the user's source and hands the whole to hiprtc (user_model.hip: build_source).
//
// One text, three kernels:
//   * the one-output kernel of smc_set_model_user / 2 (SMC_USER_NOBS not defined): data as (time, observation) pairs;
//   * with SMC_USER_NOBS defined (smc_set_model_user3, user_obs_args.h), appended TWICE: first the sweep kernel over
//     records of n_obs outputs, then with SMC_USER_PRED 1 and under the names below the prediction kernel
//     smc_user_predict_kernel - so that the sweep kernel's code does not carry the prediction stores.
// What differs between them is in the blocks marked "data side" and "prediction".  No #pragma once; SMC_USER_PRED and the
// names are undefined again at the end.
#ifndef SMC_USER_PRED
#define SMC_USER_PRED 0
#endif
#if SMC_USER_PRED
#define smc_user smc_user_pred
#define UserOps UserOpsPred
#define smc_user_solve_kernel smc_user_predict_kernel
#endif
#include "sweep_args.h"     // in-memory headers handed to hiprtc by the library: the argument blocks,
#include "philox.h"         // the counter-based generator (the early-rejection bound re-derives the acceptance uniform),
#include "solve_sched.h"    // the scheduler the built-in Michaelis-Menten kernel uses,
#include "rk45_math.h"      // and its step-controller arithmetic (fast inverse fifth root, min_step)
#define NS SMC_USER_NS
namespace smc_user {
__device__ const double RK_A[6][5] = {
    {0, 0, 0, 0, 0},
    {1.0 / 5, 0, 0, 0, 0},
    {3.0 / 40, 9.0 / 40, 0, 0, 0},
    {44.0 / 45, -56.0 / 15, 32.0 / 9, 0, 0},
    {19372.0 / 6561, -25360.0 / 2187, 64448.0 / 6561, -212.0 / 729, 0},
    {9017.0 / 3168, -355.0 / 33, 46732.0 / 5247, 49.0 / 176, -5103.0 / 18656}};
__device__ const double RK_C[6] = {0.0, 1.0 / 5, 3.0 / 10, 4.0 / 5, 8.0 / 9, 1.0};
__device__ const double RK_B[6] = {35.0 / 384, 0, 500.0 / 1113, 125.0 / 192, -2187.0 / 6784, 11.0 / 84};
__device__ const double RK_E[7] = {-71.0 / 57600, 0, 71.0 / 16695, -71.0 / 1920, 17253.0 / 339200, -22.0 / 525, 1.0 / 40};
__device__ const double RK_P[7][4] = {
    {1, -8048581381.0 / 2820520608, 8663915743.0 / 2820520608, -12715105075.0 / 11282082432},
    {0, 0, 0, 0},
    {0, 131558114200.0 / 32700410799, -68118460800.0 / 10900136933, 87487479700.0 / 32700410799},
    {0, -1754552775.0 / 470086768, 14199869525.0 / 1410260304, -10690763975.0 / 1880347072},
    {0, 127303824393.0 / 49829197408, -318862633887.0 / 49829197408, 701980252875.0 / 199316789632},
    {0, -282668133.0 / 205662961, 2019193451.0 / 616988883, -1453857185.0 / 822651844},
    {0, 40617522.0 / 29380423, -110615467.0 / 29380423, 69997945.0 / 29380423}};

__device__ __forceinline__ double py_min(double a, double b) { return (b < a) ? b : a; }
__device__ __forceinline__ double py_max(double a, double b) { return (b > a) ? b : a; }
// the two compilations of the user's functions (see the prelude): with the six-operation division, and with a / b
struct Lean {
    static __device__ __forceinline__ void rhs(double t, const double *y, const double *th, const double *c, double *d) { smc_user_lean::smc_user_rhs(t, y, th, c, d); }
    static __device__ __forceinline__ double div(double a, double b) { return SMC_USER_USES_DIV ? smc::lean_div6(a, b) : a / b; }
};
struct Ieee {
    static __device__ __forceinline__ void y0(const double *th, const double *c, double *y) { smc_user_ieee::smc_user_y0(th, c, y); }
    static __device__ __forceinline__ void rhs(double t, const double *y, const double *th, const double *c, double *d) { smc_user_ieee::smc_user_rhs(t, y, th, c, d); }
    static __device__ __forceinline__ double div(double a, double b) { return a / b; }
};
// common.py:63-65  np.linalg.norm(x) / x.size ** 0.5
__device__ __forceinline__ double rms(const double *x) {
    if (NS == 1) return fabs(x[0]);   // sqrt(x*x) / sqrt(1) is |x| exactly in IEEE arithmetic (as the built-in kernel writes it)
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < NS; ++i) s += x[i] * x[i];
    return sqrt(s) / sqrt((double)NS);
}

// One solve_ivp(RK45, t_eval = t[0..n_t)) call as a resumable state: item_begin sets it up (initial state, first
// derivative, select_initial_step), every item_attempt is one pass of rk.py's `while not step_accepted` body plus,
// when the step is accepted, the t_eval outputs it covers.  sr2 accumulates (obs - smc_user_obs)^2.
struct Item {
    double t, h_abs, y[NS], f[NS], sr2;
    double t_bound, t_next;   // t_eval[n_t - 1]; t_eval[i_out] (+inf when every data time has been served) - copies of LDS
                              // values, so that an attempt without outputs (nearly all of a stiff solve) reads no memory
#ifdef SMC_USER_NOBS
    double *pred;   // prediction kernel: where the outputs of t_eval[i_out] go (UserOps::set_pred); else nullptr
#endif
#if defined(SMC_USER_NOISE) && SMC_USER_NOISE
    smc_obs::Noise nz;   // noise model (user_obs_args.h): the particle's weights; sr2 then holds the excess sum X_e
#endif
    int i_out, status;   // status: 0 running, 1 finished, -1 step size underflow (the reference's solver raises)
    bool rejected;
};
// ---- data side: one data time of an experiment, the end time of its row, and what an output adds to the item ----
#ifdef SMC_USER_NOBS
// several outputs: the records of user_obs_args.h; the row's own end time is kept in its last record
using DataRec = smc_obs::Rec;
__device__ __forceinline__ double t_bound_of(const DataRec *tp, int n_t) { return tp[n_t].y[0]; }
__device__ __forceinline__ void emit(Item &it, const double *yy, const double *theta, const double *cond, double t_out, const double *obs) {
#if defined(SMC_USER_NOISE) && SMC_USER_NOISE
    smc_obs::emit_noise<SMC_USER_PRED, true>(it.sr2, it.pred, it.nz, yy, theta, cond, t_out, obs);
#else
    smc_obs::emit<SMC_USER_PRED, true>(it.sr2, it.pred, yy, theta, cond, t_out, obs);
#endif
}
#else
// one output: n_t + 1 (time, observation) pairs, the last one the sentinel (+inf, 0) - as in the built-in kernel
// (mm_rk45.h: mm_table_fill), so that an output costs ONE ds_read_b128 and no test for the end of the row
using DataRec = double2;
__device__ __forceinline__ double t_bound_of(const DataRec *tp, int n_t) { return tp[n_t - 1].x; }
__device__ __forceinline__ void emit(Item &it, const double *yy, const double *theta, const double *cond, double t_out, double obs) {
    const double r = obs - smc_user_ieee::smc_user_obs(t_out, yy, theta, cond);
    it.sr2 += r * r;
}
#endif
// ---- end of the data side ----
__device__ __forceinline__ void item_cache_times(Item &it, const DataRec *tp, int n_t) {
    it.t_bound = t_bound_of(tp, n_t);
    it.t_next = tp[it.i_out].x;
}

__device__ void item_begin(Item &it, const double *theta, const double *cond, const DataRec *tp, int n_t,
                           double rtol, double atol) {
    const double t0 = tp[0].x, t_bound = t_bound_of(tp, n_t);
    const double inf = __longlong_as_double(0x7ff0000000000000LL);
    double tmp[NS];
    it.t = t0;
    it.sr2 = 0.0;
    it.i_out = 0;
    it.status = 0;
    it.rejected = false;
    Ieee::y0(theta, cond, it.y);
    Ieee::rhs(t0, it.y, theta, cond, it.f);
    // common.py select_initial_step, direction +1, order 4, max_step inf
    const double interval_length = fabs(t_bound - t0);
    if (interval_length == 0.0) {
        it.h_abs = 0.0;
    } else {
        double scale[NS], y1[NS], f1[NS];
#pragma unroll
        for (int i = 0; i < NS; ++i) { scale[i] = atol + fabs(it.y[i]) * rtol; tmp[i] = it.y[i] / scale[i]; }
        const double d0 = rms(tmp);
#pragma unroll
        for (int i = 0; i < NS; ++i) tmp[i] = it.f[i] / scale[i];
        const double d1 = rms(tmp);
        double h0 = (d0 < 1e-5 || d1 < 1e-5) ? 1e-6 : 0.01 * d0 / d1;
        h0 = py_min(h0, interval_length);
#pragma unroll
        for (int i = 0; i < NS; ++i) y1[i] = it.y[i] + h0 * 1.0 * it.f[i];
        Ieee::rhs(t0 + h0 * 1.0, y1, theta, cond, f1);
#pragma unroll
        for (int i = 0; i < NS; ++i) tmp[i] = (f1[i] - it.f[i]) / scale[i];
        const double d2 = rms(tmp) / h0;
        // x ** (1 / 5) as the built-in kernel evaluates it: the reciprocal of the fast inverse fifth root (rk45_math.h)
        const double h1 = (d1 <= 1e-15 && d2 <= 1e-15) ? py_max(1e-6, h0 * 1e-3) : 1.0 / smc::pow_minus_fifth<false>(0.01 / py_max(d1, d2));
        it.h_abs = py_min(py_min(py_min(100 * h0, h1), interval_length), inf);
    }
    if (it.t == t_bound) {   // base.py:181-187: nothing to integrate
        while (tp[it.i_out].x <= it.t) { emit(it, it.y, theta, cond, tp[it.i_out].x, tp[it.i_out].y); ++it.i_out; }   // stops at the sentinel
        it.status = 1;
    }
    item_cache_times(it, tp, n_t);
}

// rk_step (rk.py:64-71) and the error norm (rk.py:106-110,146-147) of one attempt: a pure function of the item's state.
// M = the model with smc_div as the six-operation division (Lean) or as the IEEE sequence (Ieee): see item_attempt.
struct Stages {
    double K[7][NS], y_new[NS], error_norm;
};
template <class M>
__device__ __forceinline__ void rk_stages(Stages &st, const Item &it, double t, double h, const double *theta, const double *cond,
                                          double rtol, double atol) {
    double tmp[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) st.K[0][i] = it.f[i];
#pragma unroll
    for (int s = 1; s < 6; ++s) {   // rk_step: dy = K[:s].T @ a[:s] * h
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            double acc = 0.0;
#pragma unroll
            for (int j = 0; j < s; ++j) acc += st.K[j][i] * RK_A[s][j];
            tmp[i] = it.y[i] + acc * h;
        }
        M::rhs(t + RK_C[s] * h, tmp, theta, cond, st.K[s]);
    }
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        double acc = 0.0;
#pragma unroll
        for (int j = 0; j < 6; ++j) acc += st.K[j][i] * RK_B[j];      // b2 = 0 included: 0 * NaN is NaN in NumPy's dot as well
        st.y_new[i] = it.y[i] + h * acc;
    }
    M::rhs(t + h, st.y_new, theta, cond, st.K[6]);
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        double scale = atol + fmax(fabs(it.y[i]), fabs(st.y_new[i])) * rtol;
        if (it.y[i] != it.y[i] || st.y_new[i] != st.y_new[i]) scale = it.y[i] + st.y_new[i];   // np.maximum propagates NaN
        double acc = 0.0;
#pragma unroll
        for (int j = 0; j < 7; ++j) acc += st.K[j][i] * RK_E[j];
        tmp[i] = M::div(acc * h, scale);
    }
    st.error_norm = rms(tmp);
}

// One pass of rk.py's `while not step_accepted` body.  Written like the built-in kernel's mm_item_attempt (mm_rk45.h): the
// accept / reject bookkeeping as selects, ONE rarely taken branch for everything else (failure, the IEEE re-run, the dense
// output) - with per-lane operands every compare -> exec-mask round trip costs several FP64 operations, and on the
// wave-uniform operands of a lone chain every compare -> scalar-branch round trip drains the pipeline.
// smc_div: the attempt runs on the model compiled with the six-operation division (no scaling, no fix-up: NaN where a / b
// needs a subnormal or infinite divisor or a * (1 / b) overflows); whenever the error norm does not come out finite the
// whole attempt is repeated on the model compiled with IEEE division, exactly as the built-in kernel does.
__device__ __forceinline__ void item_attempt(Item &it, const double *theta, const double *cond, const DataRec *tp, double rtol,
                                             double atol) {
    const double t_bound = it.t_bound;
    const double inf = __longlong_as_double(0x7ff0000000000000LL);
    const double t = it.t;
    const double min_step = (t >= 0.0) ? smc::min_step_of(t) : 10 * fabs(nextafter(t, inf) - t);
    // rk.py:111-121: clip at the start of a step (a value raised here stays raised for the re-tries of the step)
    double h_abs = (!it.rejected && it.h_abs < min_step) ? min_step : it.h_abs;
    const bool fail = h_abs < min_step;                  // rk.py:133-134 TOO_SMALL_STEP: handled in the rare branch below
    const double t_new = fmin(t + h_abs, t_bound);       // rk.py:137-141 (h_abs is never NaN: Python's min / max drop a NaN factor)
    const double h = t_new - t;
    h_abs = fabs(h);
    Stages st;
    rk_stages<Lean>(st, it, t, h, theta, cond, rtol, atol);
    // error_norm ** -0.2 (rk.py:155,169) by the dedicated inverse fifth root of the built-in kernel (<= 1.5 ulp; the generic
    // pow costs 350 ns on the dependent chain of an attempt): 0 -> inf, which min(10, .) turns into MAX_FACTOR
    double pw = 0.9 * smc::pow_minus_fifth<false>(st.error_norm);
    bool accept = st.error_norm < 1.0;                   // false for a NaN norm: Python's max(0.2, nan) is 0.2
    const bool redo = SMC_USER_USES_DIV && !__builtin_isfinite(st.error_norm);
    if (fail || redo || (accept && it.t_next <= t_new)) {
        if (fail) {
            it.status = -1;
            return;
        }
        if (redo) {
            rk_stages<Ieee>(st, it, t, h, theta, cond, rtol, atol);
            pw = 0.9 * smc::pow_minus_fifth<false>(st.error_norm);
            accept = st.error_norm < 1.0;
        }
        // outputs in (t, t_new] and t_eval[0] == t0 on the first step (ivp.py:700-720): quartic dense output
        if (accept && it.t_next <= t_new) {
            double Q[NS][4];
#pragma unroll
            for (int i = 0; i < NS; ++i)
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    double acc = 0.0;
#pragma unroll
                    for (int j = 0; j < 7; ++j)
                        if (RK_P[j][k] != 0.0) acc += st.K[j][i] * RK_P[j][k];   // an accepted step has finite K: the zeros change nothing
                    Q[i][k] = acc;
                }
            const double hd = t_new - t;
            int i_out = it.i_out;
            DataRec nx = tp[i_out];                      // (t_next, its observation)
            do {
                const double x = smc::checked_lean_div(nx.x - t, hd);
                const double p1 = x, p2 = p1 * x, p3 = p2 * x, p4 = p3 * x;
                double yy[NS];
#pragma unroll
                for (int i = 0; i < NS; ++i) {
                    double acc = 0.0;
                    acc += Q[i][0] * p1;
                    acc += Q[i][1] * p2;
                    acc += Q[i][2] * p3;
                    acc += Q[i][3] * p4;
                    yy[i] = hd * acc + it.y[i];
                }
                emit(it, yy, theta, cond, nx.x, nx.y);
                ++i_out;
                nx = tp[i_out];                          // i_out == n_t reads the sentinel (+inf, 0)
            } while (nx.x <= t_new);
            it.i_out = i_out;
            it.t_next = nx.x;
        }
    }
    double fac_acc = py_min(10.0, pw);
    fac_acc = it.rejected ? py_min(1.0, fac_acc) : fac_acc;
    const double fac_rej = py_max(0.2, pw);
    it.h_abs = h_abs * (accept ? fac_acc : fac_rej);
    it.rejected = !accept;
    it.t = accept ? t_new : t;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        it.y[i] = accept ? st.y_new[i] : it.y[i];
        it.f[i] = accept ? st.K[6][i] : it.f[i];
    }
    it.status = (accept && (t_new - t_bound >= 0)) ? 1 : 0;   // base.py:196
}
}  // namespace smc_user

// What solve_sched.h needs to know about an item of the user model (see the list at the top of that file): the built-in
// Michaelis-Menten kernel's scheduler - chunked dequeue, pool of started items in LDS, tight attempt loop, uniform tail,
// exact early rejection - runs the user's model unchanged.
struct UserOps {
    struct Item {
        smc_user::Item s;
        double th[SMC_USER_DIM];
        long long out_idx;      // e * n + p
        int e;
        unsigned attempts;
    };
    static constexpr int kPoolWords = 2 * NS + 6;
    const smc::UserSolveArgs &a;
    long long n;
    int n_ex;
    const int *list;            // the predictably long items of the sweep, handed out first - only for a model that comes with
    unsigned n_list;            // a cost hint (smc_user_cost; smc_user_cost_scan_kernel below builds the lists), else nullptr / 0
    const int *solo;            // ... and its longest solves, one per wave on uniform operands
    unsigned n_solo;
    int patience;               // in-phase waves (solve_sched.h): with the cost order of a model that comes with a cost hint
    long long n_pos;            // positions of the index-ordered pass

    __device__ __forceinline__ const double *cond(int e) const { return a.cond + (long long)e * a.n_cond; }
    const smc_user::DataRec *s_tp;   // the data of all experiments in LDS: rows of n_t + 1 records (the data side above)
    __device__ __forceinline__ const smc_user::DataRec *row(int e) const { return s_tp + e * (a.n_t + 1); }
    __device__ __forceinline__ void publish(long long idx, double sum, int info) const {
        // visible to the waves of other XCDs while the kernel runs (the early-rejection bound reads the siblings' sums)
        __hip_atomic_store(reinterpret_cast<unsigned long long *>(a.sum_r2) + idx, (unsigned long long)__double_as_longlong(sum),
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        a.info[idx] = info;
    }
    // ---- prediction: smc_user_predict_kernel (SMC_USER_PRED 1) writes the model's outputs to `pred`; an item's pointer to its
    // next output follows from out_idx and i_out (no pool word).  A one-output item has no such pointer.
    double *pred;               // UserObsArgs::pred; nullptr in every other kernel
#ifdef SMC_USER_NOBS
    __device__ __forceinline__ void set_pred(Item &it, int i) const {
        it.s.pred = SMC_USER_PRED ? pred + (((it.out_idx - (long long)it.e * a.n) * a.n_ex + it.e) * a.n_t + i) * smc_obs::kObs : nullptr;
    }
    __device__ __forceinline__ void pred_from_lane(Item &u, const Item &it, int src) const {
        u.s.pred = SMC_USER_PRED ? (double *)smc::lane_value_ll((long long)it.s.pred, src) : nullptr;
    }
    // NaN from the first output time not served on (past the row's end; from a failed solve's stop)
    __device__ __forceinline__ void pred_tail(const Item &it) const {
        if (SMC_USER_PRED) {
            for (int i = it.s.i_out; i < a.n_t; ++i)
                for (int k = 0; k < smc_obs::kObs; ++k) it.s.pred[(i - it.s.i_out) * smc_obs::kObs + k] = __longlong_as_double(0x7ff8000000000000LL);
        }
    }
#else
    __device__ __forceinline__ void set_pred(Item &, int) const {}
    __device__ __forceinline__ void pred_from_lane(Item &, const Item &, int) const {}
    __device__ __forceinline__ void pred_tail(const Item &) const {}
#endif
    // ---- end of prediction ----
    __device__ __forceinline__ void load_theta(Item &it, long long p) const {
#pragma unroll
        for (int c = 0; c < SMC_USER_DIM; ++c) it.th[c] = a.theta[c * a.stride + p];
#if defined(SMC_USER_NOISE) && SMC_USER_NOISE
        smc_obs::noise_weights(it.s.nz, it.th, a.n_ex, a.n_t);
#endif
    }
    __device__ __forceinline__ int start(long long p, int e, bool from_list, Item &nb) const {
        nb.out_idx = (long long)e * a.n + p;
        nb.e = e;
        nb.attempts = 0;
        // index-ordered pass: a particle of the lists has been handed out already.  The flag was written by the scan kernel
        // that built the lists - the hint is NOT evaluated a second time here (a user's expression need not round the same
        // way in two kernels, and an item skipped here but missing from the list would never be solved)
        if (!from_list && list && a.listed[p] != 0) return smc::kStartSkipped;
        if (a.p0 && a.p0[p] == 0) {          // masked proposal: not solved, the accept kernel keeps lk1
            publish(nb.out_idx, 0.0, 0);
            return smc::kStartDone;
        }
        load_theta(nb, p);
        set_pred(nb, 0);
        smc_user::item_begin(nb.s, nb.th, cond(e), row(e), a.n_t, a.rtol, a.atol);
        if (nb.s.status == 0) return smc::kStartStarted;
        pred_tail(nb);
        publish(nb.out_idx, nb.s.sr2, nb.s.status < 0 ? (1 << 30) : 0);
        return smc::kStartDone;
    }
    __device__ __forceinline__ void pack(const Item &nb, double *slot) const {
        slot[0 * 64] = nb.s.t;
        slot[1 * 64] = nb.s.h_abs;
        slot[2 * 64] = nb.s.sr2;
        slot[3 * 64] = __hiloint2double(nb.s.i_out, (int)nb.s.rejected);
        slot[4 * 64] = __hiloint2double((int)nb.attempts, nb.e);
        slot[5 * 64] = __longlong_as_double(nb.out_idx);
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            slot[(6 + i) * 64] = nb.s.y[i];
            slot[(6 + NS + i) * 64] = nb.s.f[i];
        }
    }
    __device__ __forceinline__ void unpack(Item &it, const double *slot) const {
        it.s.t = slot[0 * 64];
        it.s.h_abs = slot[1 * 64];
        it.s.sr2 = slot[2 * 64];
        const double w3 = slot[3 * 64], w4 = slot[4 * 64];
        it.s.rejected = __double2loint(w3) != 0;
        it.s.i_out = __double2hiint(w3);
        it.e = __double2loint(w4);
        it.attempts = (unsigned)__double2hiint(w4);
        it.out_idx = __double_as_longlong(slot[5 * 64]);
        set_pred(it, it.s.i_out);
        it.s.status = 0;
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            it.s.y[i] = slot[(6 + i) * 64];
            it.s.f[i] = slot[(6 + NS + i) * 64];
        }
        smc_user::item_cache_times(it.s, row(it.e), a.n_t);
        load_theta(it, it.out_idx - (long long)it.e * a.n);      // the parameters come from HBM / L2 again, not through the pool
    }
    __device__ __forceinline__ int attempt(Item &it) const {
        smc_user::item_attempt(it.s, it.th, cond(it.e), row(it.e), a.rtol, a.atol);
        ++it.attempts;
        if (it.attempts >= 0x1fffffffu) it.s.status = -1;        // hard bound so that every wave drains
        return it.s.status;
    }
    __device__ __forceinline__ int uniform_attempts(Item &it, int budget) const { return smc::uniform_attempts_plain(*this, it, budget); }
    __device__ __forceinline__ bool long_running(const Item &it) const { return it.attempts > 64u; }
    __device__ __forceinline__ long long positions() const { return n_pos; }
    __device__ __forceinline__ int start_at(long long pos, int e, Item &nb) const {
        return start(a.order ? (long long)a.order[pos] : pos, e, false, nb);
    }
    __device__ __forceinline__ void finish(Item &it, int st) const {
        pred_tail(it);
        publish(it.out_idx, it.s.sr2, (int)(it.attempts & 0x1fffffffu) | ((st < 0) ? (1 << 30) : 0));
    }
    __device__ __forceinline__ Item broadcast(const Item &it, int src) const {
        Item u;
        u.s.t = smc::lane_value(it.s.t, src);
        u.s.h_abs = smc::lane_value(it.s.h_abs, src);
        u.s.sr2 = smc::lane_value(it.s.sr2, src);
        u.s.t_bound = smc::lane_value(it.s.t_bound, src);
        u.s.t_next = smc::lane_value(it.s.t_next, src);
        pred_from_lane(u, it, src);
        u.s.i_out = __builtin_amdgcn_readlane(it.s.i_out, src);
        u.s.status = __builtin_amdgcn_readlane(it.s.status, src);
        u.s.rejected = __builtin_amdgcn_readlane((int)it.s.rejected, src) != 0;
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            u.s.y[i] = smc::lane_value(it.s.y[i], src);
            u.s.f[i] = smc::lane_value(it.s.f[i], src);
        }
#pragma unroll
        for (int c = 0; c < SMC_USER_DIM; ++c) u.th[c] = smc::lane_value(it.th[c], src);
#if defined(SMC_USER_NOISE) && SMC_USER_NOISE
#pragma unroll
        for (int k = 0; k < smc_obs::kObs; ++k) {
            u.s.nz.w[k] = smc::lane_value(it.s.nz.w[k], src);
#if SMC_USER_NOISE_PROP
            u.s.nz.q[k] = smc::lane_value(it.s.nz.q[k], src);
#endif
        }
#endif
        u.out_idx = smc::lane_value_ll(it.out_idx, src);
        u.e = __builtin_amdgcn_readlane(it.e, src);
        u.attempts = (unsigned)__builtin_amdgcn_readlane((int)it.attempts, src);
        return u;
    }
    __device__ __forceinline__ bool reject_enabled() const { return a.rej != nullptr; }
    // EXACT early rejection, as for the built-in model (mm_kernels.hip: mm_certainly_rejected): the Gaussian likelihood
    // lk2 = sum_e [c0 - sum_r2_e / (2 sigma^2)] (Micmem_likelihood.py:70-73) only falls while a solve accumulates squared
    // residuals, lk1 and rr are fixed before the sweep, so a proposal that fails exp((lk2 - lk1) gamma) >= rr with the sums
    // accumulated SO FAR (0 for a sibling still running) is rejected whatever the rest would add.  The expression is the
    // one user_finish_kernel evaluates, in the same order.
#if defined(SMC_USER_NOISE) && SMC_USER_NOISE
    // EXACT early rejection under a noise model (user_obs_args.h): every observation not yet served sits at its floor
    // log(a_k s_k), known from theta, and the published sums are excesses over it, which only grow - so the likelihood formed
    // from the sums SO FAR (0 for a sibling still running) is an upper bound.  user_finish_noise_kernel's expression, in its order.
    __device__ __forceinline__ bool certainly_rejected(const Item &it) const {
        const long long p = it.out_idx - (long long)it.e * a.n;
        if (!smc_obs::noise_valid(it.th, a.n_ex, a.n_t)) return false;
        double la[smc_obs::kObs];
#pragma unroll
        for (int k = 0; k < smc_obs::kObs; ++k) la[k] = log(smc_obs::noise_add(it.th, k, a.n_ex, a.n_t) * smc_obs::noise_scale(k, a.n_ex, a.n_t));
        double lk2_bound = 0.0;
        for (int k = 0; k < a.n_ex; ++k) {
            double S = 0.0;
            if (k == it.e) {
                S = it.s.sr2;
            } else {
                const double v = __longlong_as_double((long long)__hip_atomic_load(
                    reinterpret_cast<unsigned long long *>(a.sum_r2) + (long long)k * a.n + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
                if (v < 0.0) return true;      // a sibling has already established the rejection
                if (v == v) S = v;             // finished; NaN = still running: counts as 0
            }
            lk2_bound += smc_obs::noise_floor_of(k, la, a.n_ex, a.n_t) - S;
        }
        const smc::RejectArgs &r = *a.rej;
        double rr;
        if (r.device_rng) {
            const smc::u32x4 ru = smc::philox_block(r.seed, (unsigned long long)(r.global_offset + p), r.stream, SMC_PHILOX_BLOCK_UNIFORM);
            rr = smc::u01_from(ru.x, ru.y);
        } else {
            rr = r.rr[p];
        }
        double pp = exp((lk2_bound - r.lk1[p]) * r.gamma);
        if (r.prior_mode != 0) pp = pp * r.pratio[p];
        return pp < rr * (1.0 - 1e-12);
    }
#else
    __device__ __forceinline__ bool certainly_rejected(const Item &it) const {
        const long long p = it.out_idx - (long long)it.e * a.n;
        const double sigma = a.est_sigma ? it.th[SMC_USER_DIM - 1] : a.sigma_fixed;
        if (!(sigma > 0.0)) return false;
        const double s2 = sigma * sigma;
        const double lg = log(2.0 * 3.141592653589793 * s2);
#ifndef SMC_USER_NOBS   // data side: every experiment has n_t observations of scale 1
        const double c0 = (-0.5 * a.n_t) * lg;
#endif
        double lk2_bound = 0.0;
        for (int k = 0; k < a.n_ex; ++k) {
            double S = 0.0;
            if (k == it.e) {
                S = it.s.sr2;
            } else {
                const double v = __longlong_as_double((long long)__hip_atomic_load(
                    reinterpret_cast<unsigned long long *>(a.sum_r2) + (long long)k * a.n + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
                if (v < 0.0) return true;      // a sibling has already established the rejection
                if (v == v) S = v;             // finished; NaN = still running: counts as 0
            }
#ifdef SMC_USER_NOBS    // data side: the experiment's own count and scales
            const double c0 = (-0.5 * smc_obs::me(k)) * lg - smc_obs::sum_log_scale(k, a.n_ex);
#endif
            lk2_bound += c0 - S / (2.0 * s2);
        }
        const smc::RejectArgs &r = *a.rej;
        double rr;
        if (r.device_rng) {
            const smc::u32x4 ru = smc::philox_block(r.seed, (unsigned long long)(r.global_offset + p), r.stream, SMC_PHILOX_BLOCK_UNIFORM);
            rr = smc::u01_from(ru.x, ru.y);
        } else {
            rr = r.rr[p];
        }
        double pp = exp((lk2_bound - r.lk1[p]) * r.gamma);
        if (r.prior_mode != 0) pp = pp * r.pratio[p];      // SMC_PRIOR_MODE_MASK == 0
        return pp < rr * (1.0 - 1e-12);
    }
#endif
    __device__ __forceinline__ void cancel(Item &it) const {
        publish(it.out_idx, -1.0, (int)(it.attempts & 0x1fffffffu) | (1 << 29));
    }
};

// Outputs per item: the sum of squared residuals and attempts | cancelled << 29 | failed << 30.
// small models: hold the register allocation at four waves per SIMD (the built-in kernel's occupancy); the re-run with IEEE
// division would otherwise cost the bulk loop its fourth wave
#if NS <= 2
#define SMC_USER_WAVES_ATTR __attribute__((amdgpu_waves_per_eu(4, 4)))
#else
#define SMC_USER_WAVES_ATTR
#endif
// LDS per wave: a ring of 64 started items of UserOps::kPoolWords words; then the data, read by every output
#ifdef SMC_USER_NOBS   // data side: the image the host has built (user_obs_args.h)
extern "C" __global__ void __launch_bounds__(256) SMC_USER_WAVES_ATTR smc_user_solve_kernel(smc::UserSolveArgs a, smc::UserObsArgs o) {
    extern __shared__ double s_pool_all[];
    double *s_pool = s_pool_all + (threadIdx.x >> 6) * (UserOps::kPoolWords * 64);
    static_assert(4 * UserOps::kPoolWords * 64 == smc_obs::kHdrAt, "user_obs_args.h: the image follows the pools");
    const smc_obs::Rec *s_tp = smc_obs::table(a.n_ex);
    for (int i = threadIdx.x; i < o.img_len; i += blockDim.x) smc_obs::lds()[i] = o.img[i];
    double *const pred = o.pred;
#else                  // data side: the table of (time, observation) pairs, built here
extern "C" __global__ void __launch_bounds__(256) SMC_USER_WAVES_ATTR smc_user_solve_kernel(smc::UserSolveArgs a) {
    extern __shared__ double s_pool_all[];
    double *s_pool = s_pool_all + (threadIdx.x >> 6) * (UserOps::kPoolWords * 64);
    double2 *s_tp = reinterpret_cast<double2 *>(s_pool_all + 4 * (UserOps::kPoolWords * 64));
    for (int i = threadIdx.x; i < a.n_ex * (a.n_t + 1); i += blockDim.x) {
        const int e = i / (a.n_t + 1), k = i - e * (a.n_t + 1);
        s_tp[i] = (k < a.n_t) ? make_double2(a.t[e * a.n_t + k], a.obs[e * a.n_t + k])
                              : make_double2(__longlong_as_double(0x7ff0000000000000LL), 0.0);
    }
    double *const pred = nullptr;
#endif
    __syncthreads();
    const unsigned n_list = a.stiff_list ? (unsigned)__builtin_amdgcn_readfirstlane((int)a.stiff_count[0]) : 0u;
    unsigned n_solo = a.stiff_list ? (unsigned)__builtin_amdgcn_readfirstlane((int)a.stiff_count[1]) : 0u;
    if (n_solo > a.solo_cap) n_solo = a.solo_cap;   // the overflow went onto the ordinary list
    UserOps ops{a, a.n, a.n_ex, a.stiff_list, n_list, a.stiff_list ? a.stiff_list + (a.stiff_cap - 1) : nullptr, n_solo, a.patience,
                a.n_ordered ? (long long)__builtin_amdgcn_readfirstlane((int)a.n_ordered[0]) : a.n, s_tp, pred};
    smc::solve_persistent(ops, a.queue, s_pool);
}
#if SMC_USER_PRED
#undef smc_user
#undef UserOps
#undef smc_user_solve_kernel
#endif
#undef SMC_USER_PRED
