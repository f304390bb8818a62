// user_rk45_kernel.h -- the RK45 integrator of user models (SMC_USER_METHOD_RK45, include/smc_hip.h).  Device code only: the
// library appends this text to the user's source and hands the whole to hiprtc (user_model.hip: build_source).
//
// Only the integrator is here.  The data an item reads, the adapter for the scheduler (solve_sched.h), early rejection, the
// prediction stores and the kernel's body are user_item_ops.h's, shared with user_bdf_kernel.h; that file also says how one
// text gives three kernels (appended twice for a multi-output source, the second time with SMC_USER_PRED 1 and under other
// names).  No #pragma once; the names and SMC_USER_PRED are undefined again at the end.
#include "user_item_ops.h"  // in-memory headers handed to hiprtc by the library: all of a kernel that is not an integrator,
#include "rk45_math.h"      // and the built-in kernel's step-controller arithmetic (fast inverse fifth root, min_step)
#if SMC_USER_PRED
#define smc_user smc_user_pred
#endif
namespace smc_user {
using namespace smc_user_item;   // DataRec, t_bound_of, emit, item_cache_times, py_min, py_max
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
    static constexpr bool kFuseOutputs = true;   // an output's residuals may contract (user_item_ops.h: emit)
    double t, h_abs, y[NS], f[NS], sr2;
    double t_bound, t_next;   // t_eval[n_t - 1]; t_eval[i_out] (+inf when every data time has been served) - copies of LDS
                              // values, so that an attempt without outputs (nearly all of a stiff solve) reads no memory
#ifdef SMC_USER_NOBS
    double *pred;   // prediction kernel: where the outputs of t_eval[i_out] go (user_item_ops.h: Ops::set_pred); else nullptr
#endif
#if defined(SMC_USER_NOISE) && SMC_USER_NOISE
    smc_obs::Noise nz;   // noise model (user_obs_args.h): the particle's weights; sr2 then holds the excess sum X_e
#endif
    int i_out, status;   // status: 0 running, 1 finished, -1 step size underflow (the reference's solver raises)
    bool rejected;
#ifdef SMC_USER_EVENTS
    double t_end;   // scheduled events (user_item_ops.h: item_cache_times): the row's end; t_bound is the SEGMENT's bound
    int i_ev;       // the next event of the row: the first with tau > t
#ifdef SMC_USER_ROOTS
    double g[smc_root::kRoots], t_seg;   // state-triggered events (user_item_ops.h: root_segment): the event functions at (t, y); the
    int n_fire;                          // segment's start; the events that have fired
#endif  // SMC_USER_ROOTS
#endif  // SMC_USER_EVENTS
};
#ifdef SMC_USER_EVENTS
// The start of a segment at (it.t, it.y) that runs to it.t_bound - what a new solve_ivp call does first: the derivative
// there, common.py select_initial_step (direction +1, order 4, max_step inf) over the SEGMENT's length, and no rejected step to
// remember.  item_begin's own arithmetic for the first segment, statement by statement; the right-hand-side evaluations are not
// step attempts.
__device__ __forceinline__ void segment_start(Item &it, const double *theta, const double *cond, double rtol, double atol) {
    const double inf = __longlong_as_double(0x7ff0000000000000LL);
    const double t0 = it.t;
    double tmp[NS];
    it.rejected = false;
    Ieee::rhs(t0, it.y, theta, cond, it.f);
    const double interval_length = fabs(it.t_bound - t0);
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
    const double h1 = (d1 <= 1e-15 && d2 <= 1e-15) ? py_max(1e-6, h0 * 1e-3) : 1.0 / smc::pow_minus_fifth<false>(0.01 / py_max(d1, d2));
    it.h_abs = py_min(py_min(py_min(100 * h0, h1), interval_length), inf);
}
#endif  // SMC_USER_EVENTS

__device__ void item_begin(Item &it, const double *theta, const double *cond, const DataRec *tp, int n_t,
                           double rtol, double atol) {
#ifdef SMC_USER_EVENTS
    const double t0 = tp[0].x, t_bound = smc_ev::segment_bound(cond, 0, t_bound_of(tp, n_t));   // the first step is sized by the segment
#else  // SMC_USER_EVENTS
    const double t0 = tp[0].x, t_bound = t_bound_of(tp, n_t);
#endif  // SMC_USER_EVENTS
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
#ifdef SMC_USER_EVENTS
    item_cache_times(it, cond, tp, n_t);
#ifdef SMC_USER_ROOTS
    root_begin(it, it.y, theta, cond);
#endif  // SMC_USER_ROOTS
#else  // SMC_USER_EVENTS
    item_cache_times(it, tp, n_t);
#endif  // SMC_USER_EVENTS
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
#ifdef SMC_USER_ROOTS
    // State-triggered events (user_root.h; ivp.py's loop body after solver.step()).  The event functions are evaluated at the end
    // of every attempt - an accepted step needs them, and a select is cheaper than a branch around them - and an accepted step
    // on which one of them crosses in its direction joins the rare branch.  There, on the K of the stage run that was accepted
    // (Lean, or the IEEE re-run, after which the event functions are evaluated again on ITS y_new): the root of every active event
    // on the step's dense output, the earliest one t*, the outputs of the data times <= t* from the same dense output (a data
    // time equal to t* sees the state before the jump), then y* = sol(t*), the jump smc_user_root_event(k, t*, y*) and the
    // restart of a new solve_ivp call from (t*, y*): segment_start, the event functions there, t_seg = t*.  A root AT t_bound <
    // t_end also meets scheduled event i_ev: the triggered jump first, then the scheduled one, then the one restart.  A root at
    // the row's end finishes the solve.
    // Failures (status -1: info bit 30, NaN from the first output not served): a root solve that fails (user_root.h: brentq), a
    // root at the start of its own segment - the jump left the state on a firing surface, and the chain of solve_ivp calls would
    // stop there for ever -, and a fire beyond SMC_USER_MAX_ROOT_FIRES.
    // Termination: the loop over the events has kRoots <= 4 passes and each brentq at most 100 iterations.  A fire either fails
    // the solve or raises n_fire, and n_fire > 256 fails it, so an item has at most 256 triggered restarts besides the
    // SMC_USER_NEV scheduled ones argued below.  A segment that starts at a fire starts at t* > t_seg (t* == t_seg fails), and
    // t* <= t_bound, so every segment has positive length and t never decreases; inside a segment the item is the solve it always
    // was, and Ops::attempt's hard bound on the attempts stays.  No unbounded loop is added.
    double g_new[smc_root::kRoots];
    smc_root::eval(t_new, st.y_new, theta, cond, g_new);
    if (fail || redo || (accept && (smc_root::any_active(it.g, g_new) || it.t_next <= t_new || (t_new - t_bound >= 0 && t_bound < it.t_end)))) {
        if (fail) {
            it.status = -1;
            return;
        }
        if (redo) {
            rk_stages<Ieee>(st, it, t, h, theta, cond, rtol, atol);
            pw = 0.9 * smc::pow_minus_fifth<false>(st.error_norm);
            accept = st.error_norm < 1.0;
            smc_root::eval(t_new, st.y_new, theta, cond, g_new);
        }
        const bool fired = accept && smc_root::any_active(it.g, g_new);
        if (accept && (fired || it.t_next <= t_new)) {
            double Q[NS][4];      // the quartic dense output, as below
#pragma unroll
            for (int i = 0; i < NS; ++i)
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    double acc = 0.0;
#pragma unroll
                    for (int j = 0; j < 7; ++j)
                        if (RK_P[j][k] != 0.0) acc += st.K[j][i] * RK_P[j][k];
                    Q[i][k] = acc;
                }
            const double hd = t_new - t;
            const auto sol = [&](double s, double *yy) {
                const double x = smc::checked_lean_div(s - t, hd);
                const double p1 = x, p2 = p1 * x, p3 = p2 * x, p4 = p3 * x;
#pragma unroll
                for (int i = 0; i < NS; ++i) {
                    double acc = 0.0;
                    acc += Q[i][0] * p1;
                    acc += Q[i][1] * p2;
                    acc += Q[i][2] * p3;
                    acc += Q[i][3] * p4;
                    yy[i] = hd * acc + it.y[i];
                }
            };
            double t_stop = t_new;
            int k_fire = -1;
            if (fired) {
                k_fire = smc_root::first_root(it.g, g_new, sol, t, t_new, theta, cond, t_stop);
                if (k_fire < 0 || t_stop == it.t_seg) {
                    it.status = -1;
                    return;
                }
            }
            if (it.t_next <= t_stop) {
                int i_out = it.i_out;
                DataRec nx = tp[i_out];
                do {
                    double yy[NS];
                    sol(nx.x, yy);
                    emit(it, yy, theta, cond, nx.x, nx.y);
                    ++i_out;
                    nx = tp[i_out];
                } while (nx.x <= t_stop);
                it.i_out = i_out;
                it.t_next = nx.x;
            }
            if (fired) {
                double ys[NS];
                sol(t_stop, ys);
                it.t = t_stop;
#pragma unroll
                for (int i = 0; i < NS; ++i) it.y[i] = ys[i];
                smc_user_ieee::smc_user_root_event(k_fire, t_stop, it.y, theta, cond);
                ++it.n_fire;
                if (it.n_fire > smc_root::kMaxFires) {
                    it.status = -1;
                    return;
                }
                if (t_stop - it.t_end >= 0) {      // a root at the row's end
                    it.status = 1;
                    return;
                }
                if (t_stop - t_bound >= 0) {       // ... at a scheduled event's time (t_bound < t_end here)
                    smc_user_ieee::smc_user_event(it.i_ev, t_stop, it.y, theta, cond);
                    ++it.i_ev;
                    it.t_bound = smc_ev::segment_bound(cond, it.i_ev, it.t_end);
                }
                segment_start(it, theta, cond, rtol, atol);
                root_segment(it, it.y, theta, cond);
                it.status = 0;
                return;
            }
        }
        // the segment ends at scheduled event i_ev, as below; the next one starts with the event functions at (tau, y)
        if (accept && t_new - t_bound >= 0 && t_bound < it.t_end) {
            it.t = t_new;
#pragma unroll
            for (int i = 0; i < NS; ++i) it.y[i] = st.y_new[i];
            smc_user_ieee::smc_user_event(it.i_ev, t_new, it.y, theta, cond);
            ++it.i_ev;
            it.t_bound = smc_ev::segment_bound(cond, it.i_ev, it.t_end);
            segment_start(it, theta, cond, rtol, atol);
            root_segment(it, it.y, theta, cond);
            it.status = 0;
            return;
        }
    }
#else  // SMC_USER_ROOTS
#ifdef SMC_USER_EVENTS
    // ... and an accepted step that ends a segment in front of an event (t_bound < t_end: the row goes on behind it)
    if (fail || redo || (accept && (it.t_next <= t_new || (t_new - t_bound >= 0 && t_bound < it.t_end)))) {
#else  // SMC_USER_EVENTS
    if (fail || redo || (accept && it.t_next <= t_new)) {
#endif  // SMC_USER_EVENTS
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
#ifdef SMC_USER_EVENTS
        // The segment ends at event i_ev (t_new == t_bound == tau < t_end).  The outputs up to and including tau are out, from the
        // state BEFORE the event; now the event changes the end state and the next segment starts afresh from (tau, y), as a new
        // solve_ivp call would: segment_start.  The item goes on (status 0) and this return keeps the bookkeeping below from
        // overwriting the restarted h_abs, f and rejected.
        // Termination: every event application advances i_ev, and i_ev <= SMC_USER_NEV because an event fires only with a finite
        // tau < t_end and the table ends in +inf, so an item has at most SMC_USER_NEV + 1 segments.  Event times increase strictly
        // and lie above t0, so every segment has positive length, and inside it the item is the solve it always was: t reaches
        // t_bound, or the step-size failure above stops it (Ops::attempt bounds the attempts besides).  No loop is added.
        if (accept && t_new - t_bound >= 0 && t_bound < it.t_end) {
            it.t = t_new;
#pragma unroll
            for (int i = 0; i < NS; ++i) it.y[i] = st.y_new[i];
            smc_user_ieee::smc_user_event(it.i_ev, t_new, it.y, theta, cond);
            ++it.i_ev;
            it.t_bound = smc_ev::segment_bound(cond, it.i_ev, it.t_end);
            segment_start(it, theta, cond, rtol, atol);
            it.status = 0;
            return;
        }
#endif  // SMC_USER_EVENTS
    }
#endif  // SMC_USER_ROOTS
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
#ifdef SMC_USER_ROOTS
#pragma unroll
    for (int k = 0; k < smc_root::kRoots; ++k) it.g[k] = accept ? g_new[k] : it.g[k];   // ivp.py: g = g_new
#endif  // SMC_USER_ROOTS
    it.status = (accept && (t_new - t_bound >= 0)) ? 1 : 0;   // base.py:196
}
// What user_item_ops.h needs to know about the integrator (see the list at the top of that file).  Pool words 6 ..: y, f; the
// flag of word 3: the last attempt was rejected.  No work counters.
struct Rk45 {
    using Item = smc_user::Item;
    static __device__ __forceinline__ void begin(Item &s, const double *theta, const double *cond, const DataRec *tp, int n_t, double rtol,
                                                 double atol) { item_begin(s, theta, cond, tp, n_t, rtol, atol); }
    static __device__ __forceinline__ void attempt(Item &s, const double *theta, const double *cond, const DataRec *tp, double rtol,
                                                   double atol) { item_attempt(s, theta, cond, tp, rtol, atol); }
    static __device__ __forceinline__ int pool_flag(const Item &s) { return (int)s.rejected; }
    static __device__ __forceinline__ void set_pool_flag(Item &s, int flag) { s.rejected = flag != 0; }
    static __device__ __forceinline__ void pack(const Item &s, double *w) {
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            w[i * 64] = s.y[i];
            w[(NS + i) * 64] = s.f[i];
        }
    }
    static __device__ __forceinline__ void unpack(Item &s, const double *w) {
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            s.y[i] = w[i * 64];
            s.f[i] = w[(NS + i) * 64];
        }
    }
    static __device__ __forceinline__ void broadcast(Item &u, const Item &s, int src) {
        lane_progress(u, s, src);
        lane_outputs(u, s, src);
        u.rejected = __builtin_amdgcn_readlane((int)s.rejected, src) != 0;
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            u.y[i] = smc::lane_value(s.y[i], src);
            u.f[i] = smc::lane_value(s.f[i], src);
        }
    }
    static __device__ __forceinline__ void no_work(Item &) {}
    static __device__ __forceinline__ void publish_work(unsigned *, long long, long long, const Item &) {}
#ifdef SMC_USER_ROOTS
    // an item out of the pool (it stands at t0): the event functions there again, no fire yet
    static __device__ __forceinline__ void root_begin(Item &s, const double *theta, const double *cond) { smc_user_item::root_begin(s, s.y, theta, cond); }
#endif  // SMC_USER_ROOTS
};
}  // namespace smc_user

// small models: hold the register allocation at four waves per SIMD (the built-in kernel's occupancy); the re-run with IEEE
// division would otherwise cost the bulk loop its fourth wave
#if NS <= 2
#define SMC_USER_WAVES_ATTR __attribute__((amdgpu_waves_per_eu(4, 4)))
#else
#define SMC_USER_WAVES_ATTR
#endif
#ifdef SMC_USER_NOBS
extern "C" __global__ void __launch_bounds__(256) SMC_USER_WAVES_ATTR smc_user_solve_kernel(smc::UserSolveArgs a, smc::UserObsArgs o) {
    SMC_USER_KERNEL_BODY(smc_user::Rk45, nullptr)
}
#else
extern "C" __global__ void __launch_bounds__(256) SMC_USER_WAVES_ATTR smc_user_solve_kernel(smc::UserSolveArgs a) {
    SMC_USER_KERNEL_BODY(smc_user::Rk45, nullptr)
}
#endif
#undef smc_user
#undef smc_user_item
#undef smc_user_solve_kernel
#undef SMC_USER_PRED
