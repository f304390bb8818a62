// user_bdf_kernel.h -- the second integrator of user models (SMC_USER_METHOD_BDF, include/smc_hip.h).  Device code only: the
// library appends this text to the user's source and hands the whole to hiprtc (user_model.hip: build_source).  It restates
// solve_ivp(method="BDF", t_eval = t, rtol, atol) per lane as SciPy 1.15 has it (scipy/integrate/_ivp/bdf.py: the NDF
// coefficients, the difference array D with change_D / compute_R, solve_bdf_system, the current_jac logic, the error-norm step
// control with the order change over k-1, k, k+1, BdfDenseOutput; common.py: select_initial_step with order 1, num_jac).
//
// Only the integrator is here.  The data an item reads, the adapter for the scheduler (solve_sched.h), early rejection, the
// prediction stores, user_finish_kernel, the cost-hint scan and the kernel's body are what the RK45 kernel has:
// user_item_ops.h, which also says how one text gives three kernels (appended twice for a multi-output source, the second
// time with SMC_USER_PRED 1 and under other names).  No #pragma once; the names and SMC_USER_PRED are undefined again at the end.
//
// NumPy rounds every product and sum on its own: the integrator is compiled without contraction.  The small matrix products
// (change_D, psi, the LU and its solves, the dense output) are plain sequential sums where SciPy calls BLAS / LAPACK, so
// agreement with SciPy is at rounding level per step, not bitwise.  The user's functions are compiled once, with
// smc_div(a, b) = a / b.
#pragma clang fp contract(off)
#include "user_item_ops.h"  // in-memory header handed to hiprtc by the library: all of a kernel that is not an integrator
#if SMC_USER_PRED
#define smc_user_bdf smc_user_bdf_pred
#endif
namespace smc_user_bdf {
using namespace smc_user_item;   // DataRec, t_bound_of, emit, item_cache_times, py_min, py_max
constexpr double kEps = 0x1.0p-52;
constexpr int kMaxOrder = 5, kNewtonMaxIter = 4;
constexpr int kRows = kMaxOrder + 3;        // D[0 .. order + 2]
// bdf.py BDF.__init__: gamma, alpha = (1 - kappa) gamma, error_const = kappa gamma + 1 / (1 .. 6), exactly as NumPy rounds them
constexpr double kGamma[6] = {0x0.0p+0, 0x1.0000000000000p+0, 0x1.8000000000000p+0, 0x1.d555555555555p+0, 0x1.0aaaaaaaaaaaap+1, 0x1.2444444444444p+1};
constexpr double kAlpha[6] = {0x0.0p+0, 0x1.2f5c28f5c28f6p+0, 0x1.aaaaaaaaaaaabp+0, 0x1.fbf59f9b82ef8p+0, 0x1.15bbbbbbbbbbbp+1, 0x1.2444444444444p+1};
constexpr double kErrConst[6] = {0x1.0000000000000p+0, 0x1.428f5c28f5c29p-2, 0x1.5555555555555p-3, 0x1.95fb5b9d265dcp-4, 0x1.d111111111112p-4, 0x1.5555555555555p-3};
// compute_R(order, 1): (-1)^l C(j, l), upper triangular; compute_R of a lower order is its leading block
constexpr double kU[6][6] = {{1, 1, 1, 1, 1, 1}, {0, -1, -2, -3, -4, -5}, {0, 0, 1, 3, 6, 10},
                             {0, 0, 0, -1, -4, -10}, {0, 0, 0, 0, 1, 5}, {0, 0, 0, 0, 0, -1}};
// common.py num_jac
constexpr double kNumJacDiffReject = 0x1.6a09e667f3bcdp-46, kNumJacDiffSmall = 0x1.0p-39, kNumJacDiffBig = 0x1.0p-13;
constexpr double kNumJacMinFactor = 0x1.f4p-43;

__device__ __forceinline__ double np_max(double a, double b) { return (a != a || b != b) ? a + b : fmax(a, b); }   // np.maximum
// tab[k] for a per-lane k < 6, by selects (an indexed read of a register array would go through scratch)
__device__ __forceinline__ double pick(const double (&tab)[6], int k) {
    double r = tab[0];
#pragma unroll
    for (int j = 1; j < 6; ++j) r = (k == j) ? tab[j] : r;
    return r;
}
// common.py norm: np.linalg.norm(x) / x.size ** 0.5
__device__ __forceinline__ double norm(const double *x) {
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < NS; ++i) s += x[i] * x[i];
    return sqrt(s) / sqrt((double)NS);
}

// One solve_ivp(BDF, t_eval = t[0..n_t)) call as a resumable state.  item_begin: initial state, first derivative,
// select_initial_step (what the pool of solve_sched.h holds: t, h, y = D[0], f = D[1]); every item_attempt is one pass of
// bdf.py's `while not step_accepted` body (its Newton iterations, Jacobian refresh and LU factorisation included) and,
// when the step is accepted, the order change and the t_eval outputs it covers.  sr2 accumulates (obs - smc_user_obs)^2.
struct Item {
    static constexpr bool kFuseOutputs = false;   // NumPy rounds an output's residuals one by one (user_item_ops.h: emit)
    double t, h_abs, sr2;
    double t_bound, t_next;        // t_eval[n_t - 1]; t_eval[i_out] (+inf when every data time has been served)
    double D[kRows][NS];           // differences; before the first attempt D[1] holds f(t0, y0) (fresh)
    double J[NS][NS], LU[NS][NS];  // Jacobian and the factors of I - c J (row-major, L unit lower, U upper)
    double jac_factor[NS];         // num_jac's per-column factor (no smc_user_jac)
    int piv[NS];
#ifdef SMC_USER_NOBS
    double *pred;   // prediction kernel: where the outputs of t_eval[i_out] go (user_item_ops.h: Ops::set_pred); else nullptr
#endif
#if defined(SMC_USER_NOISE) && SMC_USER_NOISE
    smc_obs::Noise nz;   // noise model (user_obs_args.h): the particle's weights; sr2 then holds the excess sum X_e
#endif
    int order, n_equal_steps, i_out, status;   // status: 0 running, 1 finished, -1 TOO_SMALL_STEP
    bool fresh, in_step, current_jac, lu_valid;
    unsigned n_steps, n_newton, n_lu, n_jac;   // accepted steps, Newton iterations, LU factorisations, Jacobian evaluations
#ifdef SMC_USER_EVENTS
    double t_end;   // scheduled events (user_item_ops.h: item_cache_times): the row's end; t_bound is the SEGMENT's bound
    int i_ev;       // the next event of the row: the first with tau > t
#ifdef SMC_USER_ROOTS
    double g[smc_root::kRoots], t_seg;   // state-triggered events (user_item_ops.h: root_segment): the event functions at (t, y); the
    int n_fire;                          // segment's start; the events that have fired
#endif  // SMC_USER_ROOTS
#endif  // SMC_USER_EVENTS
};
// what a lane sets up for an item that has not had an attempt yet (item_begin and the pool's unpack)
__device__ __forceinline__ void item_reset_lane(Item &it) {
#pragma unroll
    for (int r = 2; r < kRows; ++r)
#pragma unroll
        for (int i = 0; i < NS; ++i) it.D[r][i] = 0.0;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        it.jac_factor[i] = 0x1.0p-26;      // EPS ** 0.5 (jac_factor None)
        it.piv[i] = i;
#pragma unroll
        for (int j = 0; j < NS; ++j) it.J[i][j] = it.LU[i][j] = 0.0;
    }
    it.order = 1;
    it.n_equal_steps = 0;
    it.status = 0;
    it.fresh = true;
    it.in_step = false;
    it.current_jac = false;
    it.lu_valid = false;
    it.n_steps = it.n_newton = it.n_lu = it.n_jac = 0u;
}

__device__ __forceinline__ void rhs(double t, const double *y, const double *theta, const double *cond, double *f) {
    smc_user_ieee::smc_user_rhs(t, y, theta, cond, f);
}

// J at (t, y): the user's smc_user_jac, or num_jac's forward differences with f = f(t, y) and the adapted factor
__device__ __forceinline__ void jacobian(Item &it, double t, const double *y, const double *f, const double *theta, const double *cond,
                                         double atol) {
    ++it.n_jac;
#ifdef SMC_USER_HAS_JAC
    (void)f;
    (void)atol;
    smc_user_ieee::smc_user_jac(t, y, theta, cond, &it.J[0][0]);
#else
#pragma unroll 1
    for (int j = 0; j < NS; ++j) {       // one column per pass; the column is picked and written by selects
        double yj = y[0], fj = f[0], factor = it.jac_factor[0];
#pragma unroll
        for (int q = 1; q < NS; ++q) {
            yj = (j == q) ? y[q] : yj;
            fj = (j == q) ? f[q] : fj;
            factor = (j == q) ? it.jac_factor[q] : factor;
        }
        const double f_sign = (fj >= 0.0) ? 1.0 : -1.0;
        const double y_scale = f_sign * np_max(atol, fabs(yj));
        double fs = factor * y_scale;
        double h = (yj + fs) - yj;
        while (h == 0.0) {               // "make sure that the step is not 0"
            factor *= 10;
            fs = factor * y_scale;
            h = (yj + fs) - yj;
        }
        double yy[NS], fn[NS], diff[NS];
#pragma unroll
        for (int i = 0; i < NS; ++i) yy[i] = y[i] + ((i == j) ? h : 0.0);
        rhs(t, yy, theta, cond, fn);
        double max_diff = -1.0, scale = 0.0;
#pragma unroll
        for (int i = 0; i < NS; ++i) {   // np.argmax: the first maximum
            diff[i] = fn[i] - f[i];
            const double a = fabs(diff[i]);
            if (a > max_diff) {
                max_diff = a;
                scale = np_max(fabs(f[i]), fabs(fn[i]));
            }
        }
        if (max_diff < kNumJacDiffReject * scale) {     // the refinement step
            const double new_factor = 10 * factor;
            const double fs2 = new_factor * y_scale;
            const double h_new = (yj + fs2) - yj;
            double diff_new[NS];
#pragma unroll
            for (int i = 0; i < NS; ++i) yy[i] = y[i] + ((i == j) ? h_new : 0.0);
            rhs(t, yy, theta, cond, fn);
            double max_diff_new = -1.0, scale_new = 0.0;
#pragma unroll
            for (int i = 0; i < NS; ++i) {
                diff_new[i] = fn[i] - f[i];
                const double a = fabs(diff_new[i]);
                if (a > max_diff_new) {
                    max_diff_new = a;
                    scale_new = np_max(fabs(f[i]), fabs(fn[i]));
                }
            }
            if (max_diff * scale_new < max_diff_new * scale) {
                factor = new_factor;
                h = h_new;
#pragma unroll
                for (int i = 0; i < NS; ++i) diff[i] = diff_new[i];
                scale = scale_new;
                max_diff = max_diff_new;
            }
        }
        if (max_diff < kNumJacDiffSmall * scale) factor *= 10;
        if (max_diff > kNumJacDiffBig * scale) factor *= 0.1;
        factor = np_max(factor, kNumJacMinFactor);
#pragma unroll
        for (int q = 0; q < NS; ++q) {
            it.jac_factor[q] = (j == q) ? factor : it.jac_factor[q];
#pragma unroll
            for (int i = 0; i < NS; ++i) it.J[i][q] = (j == q) ? diff[i] / h : it.J[i][q];
        }
    }
#endif
}

// lu_factor(I - c J): partial pivoting (the first largest |a| of the column, as idamax), rows swapped by selects
__device__ __forceinline__ void lu_factor(Item &it, double c) {
    double A[NS][NS];
#pragma unroll
    for (int i = 0; i < NS; ++i)
#pragma unroll
        for (int j = 0; j < NS; ++j) A[i][j] = ((i == j) ? 1.0 : 0.0) - c * it.J[i][j];
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        int p = k;
        double amax = fabs(A[k][k]);
#pragma unroll
        for (int i = k + 1; i < NS; ++i) {
            const double a = fabs(A[i][k]);
            p = (a > amax) ? i : p;
            amax = (a > amax) ? a : amax;
        }
        it.piv[k] = p;
#pragma unroll
        for (int i = k + 1; i < NS; ++i)
#pragma unroll
            for (int j = 0; j < NS; ++j) {
                const double akj = A[k][j];
                A[k][j] = (p == i) ? A[i][j] : akj;
                A[i][j] = (p == i) ? akj : A[i][j];
            }
        const double pivot = A[k][k];
        const double r = 1.0 / pivot;                  // dgetf2: scale by the reciprocal (a zero pivot leaves the column)
#pragma unroll
        for (int i = k + 1; i < NS; ++i) A[i][k] = (pivot != 0.0) ? A[i][k] * r : A[i][k];
#pragma unroll
        for (int i = k + 1; i < NS; ++i)
#pragma unroll
            for (int j = k + 1; j < NS; ++j) A[i][j] = A[i][j] - A[i][k] * A[k][j];
    }
#pragma unroll
    for (int i = 0; i < NS; ++i)
#pragma unroll
        for (int j = 0; j < NS; ++j) it.LU[i][j] = A[i][j];
    ++it.n_lu;
    it.lu_valid = true;
}

// lu_solve: b <- (I - c J)^-1 b
__device__ __forceinline__ void lu_solve(const Item &it, double *b) {
#pragma unroll
    for (int k = 0; k < NS; ++k)
#pragma unroll
        for (int i = k + 1; i < NS; ++i) {
            const double bk = b[k];
            b[k] = (it.piv[k] == i) ? b[i] : bk;
            b[i] = (it.piv[k] == i) ? bk : b[i];
        }
#pragma unroll
    for (int k = 0; k < NS; ++k)
#pragma unroll
        for (int i = k + 1; i < NS; ++i) b[i] = b[i] - b[k] * it.LU[i][k];
#pragma unroll
    for (int k = NS - 1; k >= 0; --k) {
        b[k] = b[k] / it.LU[k][k];
#pragma unroll
        for (int i = 0; i < k; ++i) b[i] = b[i] - b[k] * it.LU[i][k];
    }
}

// change_D: D[:order + 1] = (R U)^T D[:order + 1] with R = compute_R(order, factor), U = compute_R(order, 1), evaluated as
// U^T (R^T D): column l of R is a running product, so neither matrix is held (R U would need 72 doubles of registers).  For
// the per-lane order the order-5 matrices are used - compute_R of a lower order is their leading block - with the rows above
// `order` left out by selects.
__device__ __forceinline__ void change_D(Item &it, int order, double factor) {
    double E[6][NS];
#pragma unroll
    for (int l = 0; l < 6; ++l) {
        double r = 1.0;                                  // R[0][l]
#pragma unroll
        for (int s = 0; s < NS; ++s) E[l][s] = it.D[0][s];
#pragma unroll
        for (int i = 1; i < 6; ++i) {
            r = (l == 0) ? 0.0 : r * (((double)(i - 1) - factor * l) / i);
#pragma unroll
            for (int s = 0; s < NS; ++s) E[l][s] = (i <= order && l > 0) ? E[l][s] + r * it.D[i][s] : E[l][s];
        }
    }
#pragma unroll
    for (int j = 0; j < 6; ++j)
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            double acc = E[0][s];
#pragma unroll
            for (int l = 1; l <= j; ++l) acc += kU[l][j] * E[l][s];
            it.D[j][s] = (j <= order) ? acc : it.D[j][s];
        }
}

// solve_bdf_system: at most kNewtonMaxIter iterations with the convergence-rate test.  The loop has a fixed trip count;
// a lane that has stopped iterating only idles through the rest.
__device__ __forceinline__ void solve_bdf_system(Item &it, const double *theta, const double *cond, double t_new, const double *y_predict,
                                                 double c, const double *psi, const double *scale, double tol, bool &converged,
                                                 int &n_iter, double *y, double *d) {
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        y[i] = y_predict[i];
        d[i] = 0.0;
    }
    double dy_norm_old = 0.0;
    bool done = false;
    converged = false;
    n_iter = kNewtonMaxIter;
#pragma unroll 1
    for (int k = 0; k < kNewtonMaxIter; ++k) {
        if (!done) {
            double f[NS];
            rhs(t_new, y, theta, cond, f);
            ++it.n_newton;
            bool finite = true;
#pragma unroll
            for (int i = 0; i < NS; ++i) finite = finite && __builtin_isfinite(f[i]);
            if (!finite) {
                done = true;
                n_iter = k + 1;
            } else {
                double dy[NS], tmp[NS];
#pragma unroll
                for (int i = 0; i < NS; ++i) dy[i] = c * f[i] - psi[i] - d[i];
                lu_solve(it, dy);
#pragma unroll
                for (int i = 0; i < NS; ++i) tmp[i] = dy[i] / scale[i];
                const double dy_norm = norm(tmp);
                const double rate = dy_norm / dy_norm_old;      // used from the second iteration on (rate is None before)
                if (k > 0 && (rate >= 1 || pow(rate, (double)(kNewtonMaxIter - k)) / (1 - rate) * dy_norm > tol)) {
                    done = true;
                    n_iter = k + 1;
                } else {
#pragma unroll
                    for (int i = 0; i < NS; ++i) {
                        y[i] += dy[i];
                        d[i] += dy[i];
                    }
                    if (dy_norm == 0 || (k > 0 && rate / (1 - rate) * dy_norm < tol)) {
                        converged = true;
                        done = true;
                        n_iter = k + 1;
                    }
                    dy_norm_old = dy_norm;
                }
            }
        }
    }
}

__device__ void item_begin(Item &it, const double *theta, const double *cond, const DataRec *tp, int n_t, double rtol_in,
                           double atol) {
    const double rtol = (rtol_in < 100 * kEps) ? 100 * kEps : rtol_in;      // common.py validate_tol
#ifdef SMC_USER_EVENTS
    const double t0 = tp[0].x, t_bound = smc_ev::segment_bound(cond, 0, t_bound_of(tp, n_t));   // the first step is sized by the segment
#else  // SMC_USER_EVENTS
    const double t0 = tp[0].x, t_bound = t_bound_of(tp, n_t);
#endif  // SMC_USER_EVENTS
    const double inf = __longlong_as_double(0x7ff0000000000000LL);
    item_reset_lane(it);
    it.t = t0;
    it.sr2 = 0.0;
    it.i_out = 0;
    double *y = it.D[0], *f = it.D[1];
    smc_user_ieee::smc_user_y0(theta, cond, y);
    rhs(t0, y, theta, cond, f);
    // common.py select_initial_step, direction +1, order 1, max_step inf
    const double interval_length = fabs(t_bound - t0);
    if (interval_length == 0.0) {
        it.h_abs = 0.0;
    } else {
        double scale[NS], tmp[NS], y1[NS], f1[NS];
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            scale[i] = atol + fabs(y[i]) * rtol;
            tmp[i] = y[i] / scale[i];
        }
        const double d0 = norm(tmp);
#pragma unroll
        for (int i = 0; i < NS; ++i) tmp[i] = f[i] / scale[i];
        const double d1 = norm(tmp);
        double h0 = (d0 < 1e-5 || d1 < 1e-5) ? 1e-6 : 0.01 * d0 / d1;
        h0 = py_min(h0, interval_length);
#pragma unroll
        for (int i = 0; i < NS; ++i) y1[i] = y[i] + h0 * 1.0 * f[i];
        rhs(t0 + h0 * 1.0, y1, theta, cond, f1);
#pragma unroll
        for (int i = 0; i < NS; ++i) tmp[i] = (f1[i] - f[i]) / scale[i];
        const double d2 = norm(tmp) / h0;
        const double h1 = (d1 <= 1e-15 && d2 <= 1e-15) ? py_max(1e-6, h0 * 1e-3) : sqrt(0.01 / py_max(d1, d2));   // ** (1 / 2)
        it.h_abs = py_min(py_min(py_min(100 * h0, h1), interval_length), inf);
    }
    if (it.t == t_bound) {   // base.py: nothing to integrate (outputs from D[0] = y0)
        while (tp[it.i_out].x <= it.t) { emit(it, y, theta, cond, tp[it.i_out].x, tp[it.i_out].y); ++it.i_out; }
        it.status = 1;
    }
#ifdef SMC_USER_EVENTS
    item_cache_times(it, cond, tp, n_t);
#ifdef SMC_USER_ROOTS
    root_begin(it, it.D[0], theta, cond);
#endif  // SMC_USER_ROOTS
#else  // SMC_USER_EVENTS
    item_cache_times(it, tp, n_t);
#endif  // SMC_USER_EVENTS
}
#ifdef SMC_USER_EVENTS
// The start of a segment at (it.t, y) that runs to it.t_bound - what a new solve_ivp(BDF) call sets up, which is what
// item_begin sets up for the first: item_reset_lane (order 1, no Jacobian, no LU, num_jac's factors as new), D[0] = y,
// D[1] = f(t, y) - the first attempt then scales it and evaluates J there - and common.py select_initial_step (order 1) over
// the SEGMENT's length.  The work counters go on counting; the right-hand-side evaluations here are not step attempts.
__device__ __forceinline__ void segment_start(Item &it, const double *y_in, const double *theta, const double *cond, double rtol, double atol) {
    const double inf = __longlong_as_double(0x7ff0000000000000LL);
    const unsigned n_steps = it.n_steps, n_newton = it.n_newton, n_lu = it.n_lu, n_jac = it.n_jac;
    double y0[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) y0[i] = y_in[i];
    item_reset_lane(it);
    it.n_steps = n_steps;
    it.n_newton = n_newton;
    it.n_lu = n_lu;
    it.n_jac = n_jac;
    const double t0 = it.t;
    double *y = it.D[0], *f = it.D[1];
#pragma unroll
    for (int i = 0; i < NS; ++i) y[i] = y0[i];
    rhs(t0, y, theta, cond, f);
    const double interval_length = fabs(it.t_bound - t0);
    double scale[NS], tmp[NS], y1[NS], f1[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        scale[i] = atol + fabs(y[i]) * rtol;
        tmp[i] = y[i] / scale[i];
    }
    const double d0 = norm(tmp);
#pragma unroll
    for (int i = 0; i < NS; ++i) tmp[i] = f[i] / scale[i];
    const double d1 = norm(tmp);
    double h0 = (d0 < 1e-5 || d1 < 1e-5) ? 1e-6 : 0.01 * d0 / d1;
    h0 = py_min(h0, interval_length);
#pragma unroll
    for (int i = 0; i < NS; ++i) y1[i] = y[i] + h0 * 1.0 * f[i];
    rhs(t0 + h0 * 1.0, y1, theta, cond, f1);
#pragma unroll
    for (int i = 0; i < NS; ++i) tmp[i] = (f1[i] - f[i]) / scale[i];
    const double d2 = norm(tmp) / h0;
    const double h1 = (d1 <= 1e-15 && d2 <= 1e-15) ? py_max(1e-6, h0 * 1e-3) : sqrt(0.01 / py_max(d1, d2));   // ** (1 / 2)
    it.h_abs = py_min(py_min(py_min(100 * h0, h1), interval_length), inf);
}
#endif  // SMC_USER_EVENTS

// One pass of bdf.py _step_impl's `while not step_accepted` body; on acceptance also the rest of _step_impl (D update,
// order change) and the t_eval outputs of the step through BdfDenseOutput (built after the step, as solve_ivp does).
__device__ __forceinline__ void item_attempt(Item &it, const double *theta, const double *cond, const DataRec *tp, double rtol_in,
                                             double atol) {
    const double rtol = (rtol_in < 100 * kEps) ? 100 * kEps : rtol_in;
    const double newton_tol = py_max(10 * kEps / rtol, py_min(0.03, sqrt(rtol)));
    const double inf = __longlong_as_double(0x7ff0000000000000LL);
    if (it.fresh) {          // BDF.__init__: D[1] = f h, J at (t0, y0)
        double f0[NS];
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            f0[i] = it.D[1][i];
            it.D[1][i] = f0[i] * it.h_abs;
        }
        jacobian(it, it.t, it.D[0], f0, theta, cond, atol);
        it.fresh = false;
    }
    const double t = it.t, t_bound = it.t_bound;
    const double min_step = (t >= 0.0) ? smc::min_step_of(t) : 10 * fabs(nextafter(t, inf) - t);
    const int order = it.order;
    // the two rescalings of D before the Newton solve (start-of-step clip to min_step, last step clipped at t_bound) and the
    // one after it (Newton failure, error rejection, order change) each go through ONE inlined change_D
    bool cd_pre[2] = {false, false};
    double cd_pre_factor[2] = {1.0, 1.0};
    double h_abs = it.h_abs;
    if (!it.in_step) {       // start of a step (max_step = inf: only the lower clip)
        if (h_abs < min_step) {
            cd_pre[0] = true;
            cd_pre_factor[0] = min_step / h_abs;
            h_abs = min_step;
            it.n_equal_steps = 0;
        }
        it.current_jac = false;
        it.in_step = true;
    }
    if (h_abs < min_step) {  // TOO_SMALL_STEP
        it.status = -1;
        return;
    }
    double t_new = t + h_abs;
    if (t_new - t_bound > 0) {
        t_new = t_bound;
        cd_pre[1] = true;
        cd_pre_factor[1] = fabs(t_new - t) / h_abs;
        it.n_equal_steps = 0;
        it.lu_valid = false;
    }
#pragma unroll 1
    for (int q = 0; q < 2; ++q)
        if (q == 0 ? cd_pre[0] : cd_pre[1]) change_D(it, order, q == 0 ? cd_pre_factor[0] : cd_pre_factor[1]);
    const double h = t_new - t;
    h_abs = fabs(h);
    double y_predict[NS], scale[NS], psi[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        double acc = it.D[0][s];
#pragma unroll
        for (int j = 1; j < 6; ++j) acc = (j <= order) ? acc + it.D[j][s] : acc;
        y_predict[s] = acc;
        scale[s] = atol + rtol * fabs(acc);
    }
    const double alpha = pick(kAlpha, order);
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        double acc = 0.0;
#pragma unroll
        for (int j = 1; j < 6; ++j) acc = (j <= order) ? acc + it.D[j][s] * kGamma[j] : acc;
        psi[s] = acc / alpha;
    }
    const double c = h / alpha;
    bool converged = false;
    int n_iter = 0;
    double y_new[NS], d[NS];
    // first with the current J; if Newton fails and J is not fresh for this step, once more with J at (t_new, y_predict)
#pragma unroll 1
    for (int pass = 0; pass < 2; ++pass) {
        if (pass == 0 || (!converged && !it.current_jac)) {
            if (pass == 1) {
                double fp[NS];      // num_jac's f(t_new, y_predict) (jac_wrapped evaluates it)
#ifndef SMC_USER_HAS_JAC
                rhs(t_new, y_predict, theta, cond, fp);
#endif
                jacobian(it, t_new, y_predict, fp, theta, cond, atol);
                it.lu_valid = false;
                it.current_jac = true;
            }
            if (!it.lu_valid) lu_factor(it, c);
            solve_bdf_system(it, theta, cond, t_new, y_predict, c, psi, scale, newton_tol, converged, n_iter, y_new, d);
        }
    }
    bool accepted = false, cd = false;
    int cd_order = order;
    double cd_factor = 1.0;
    if (!converged) {
        h_abs *= 0.5;
        cd = true;
        cd_factor = 0.5;
        it.n_equal_steps = 0;
        it.lu_valid = false;
        it.h_abs = h_abs;
    } else {
        const double safety = 0.9 * (2 * kNewtonMaxIter + 1) / (2 * kNewtonMaxIter + n_iter);
        double err[NS];
        const double ec = pick(kErrConst, order);
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            scale[s] = atol + rtol * fabs(y_new[s]);
            err[s] = ec * d[s] / scale[s];
        }
        const double error_norm = norm(err);
        if (error_norm > 1) {    // rejected: the LU is kept (bdf.py: no convergence problem)
            const double factor = py_max(0.2, safety * pow(error_norm, -1.0 / (order + 1)));
            h_abs *= factor;
            cd = true;
            cd_factor = factor;
            it.n_equal_steps = 0;
            it.h_abs = h_abs;
        } else {
            accepted = true;
            ++it.n_steps;
            it.in_step = false;
            it.n_equal_steps += 1;
            it.t = t_new;
            it.h_abs = h_abs;
            {   // D[order + 2] = d - D[order + 1]; D[order + 1] = d; D[i] += D[i + 1] for i = order .. 0
                double Dop1[NS];
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    double v = it.D[2][s];
#pragma unroll
                    for (int r = 3; r < kRows - 1; ++r) v = (r == order + 1) ? it.D[r][s] : v;
                    Dop1[s] = v;
                }
#pragma unroll
                for (int r = 2; r < kRows; ++r)
#pragma unroll
                    for (int s = 0; s < NS; ++s) {
                        it.D[r][s] = (r == order + 2) ? d[s] - Dop1[s] : it.D[r][s];
                        it.D[r][s] = (r == order + 1) ? d[s] : it.D[r][s];
                    }
#pragma unroll
                for (int i = kMaxOrder; i >= 0; --i)
#pragma unroll
                    for (int s = 0; s < NS; ++s) it.D[i][s] = (i <= order) ? it.D[i][s] + it.D[i + 1][s] : it.D[i][s];
            }
            if (it.n_equal_steps >= order + 1) {     // order change over order - 1, order, order + 1
                double em[NS], ep[NS];
                const double ecm = pick(kErrConst, order - 1), ecp = pick(kErrConst, order + 1 < 6 ? order + 1 : 5);
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    double dm = it.D[1][s], dp = it.D[3][s];
#pragma unroll
                    for (int r = 2; r < 6; ++r) dm = (r == order) ? it.D[r][s] : dm;
#pragma unroll
                    for (int r = 4; r < kRows; ++r) dp = (r == order + 2) ? it.D[r][s] : dp;
                    em[s] = ecm * dm / scale[s];
                    ep[s] = ecp * dp / scale[s];
                }
                const double error_m_norm = (order > 1) ? norm(em) : inf;
                const double error_p_norm = (order < kMaxOrder) ? norm(ep) : inf;
                const double fm = pow(error_m_norm, -1.0 / order), f0 = pow(error_norm, -1.0 / (order + 1)),
                             fp = pow(error_p_norm, -1.0 / (order + 2));
                int delta = -1;             // np.argmax: the first maximum
                double fmax_ = fm;
                if (f0 > fmax_) { delta = 0; fmax_ = f0; }
                if (fp > fmax_) { delta = 1; fmax_ = fp; }
                if (fm != fm || f0 != f0 || fp != fp) fmax_ = fm + f0 + fp;   // np.max propagates NaN (min(10, nan) is 10 below)
                const int new_order = order + delta;
                it.order = new_order;
                const double factor = py_min(10.0, safety * fmax_);
                it.h_abs *= factor;
                cd = true;
                cd_order = new_order;
                cd_factor = factor;
                it.n_equal_steps = 0;
                it.lu_valid = false;
            }
        }
    }
    if (cd) change_D(it, cd_order, cd_factor);
#ifdef SMC_USER_ROOTS
    // State-triggered events (user_root.h; ivp.py's loop body after solver.step()): after an accepted step the event functions at
    // the solver's own (t_new, y_new); if one of them crossed in its direction, the root of every active event on the step's
    // BdfDenseOutput (built after the step, as solve_ivp builds it), the earliest one t*, the outputs of the data times <= t* from
    // the same dense output (a data time equal to t* sees the state before the jump), then y* = sol(t*), the jump
    // smc_user_root_event(k, t*, y*) and the restart of a new solve_ivp call from (t*, y*): segment_start (order 1, a new
    // Jacobian, the initial step rule), the event functions there, t_seg = t*.  The truncated step has been counted as a step,
    // as SciPy counts it.  A root AT t_bound < t_end also meets scheduled event i_ev: the triggered jump first, then the
    // scheduled one, then the one restart.  A root at the row's end finishes the solve.
    // Failures (status -1: info bit 30, NaN from the first output not served): a root solve that fails (user_root.h: brentq), a
    // root at the start of its own segment - the jump left the state on a firing surface, and the chain of solve_ivp calls would
    // stop there for ever -, and a fire beyond SMC_USER_MAX_ROOT_FIRES.
    // Termination: the loop over the events has kRoots <= 4 passes and each brentq at most 100 iterations.  A fire either fails
    // the solve or raises n_fire, and n_fire > 256 fails it, so an item has at most 256 triggered restarts besides the
    // SMC_USER_NEV scheduled ones argued below.  A segment that starts at a fire starts at t* > t_seg (t* == t_seg fails), and
    // t* <= t_bound, so every segment has positive length and t never decreases; inside a segment the item is the solve it always
    // was, and Ops::attempt's hard bound on the attempts stays.  No unbounded loop is added.
    if (accepted) {
        const int k = it.order;
        const double hd = it.h_abs;
        const auto sol = [&](double s, double *yy) {
            double p = 1.0;
#pragma unroll
            for (int q = 0; q < NS; ++q) yy[q] = 0.0;
#pragma unroll
            for (int j = 0; j < kMaxOrder; ++j) {
                const double t_shift = t_new - hd * j, denom = hd * (1 + j);
                p = (j == 0) ? (s - t_shift) / denom : p * ((s - t_shift) / denom);
#pragma unroll
                for (int q = 0; q < NS; ++q) yy[q] = (j < k) ? yy[q] + it.D[j + 1][q] * p : yy[q];
            }
#pragma unroll
            for (int q = 0; q < NS; ++q) yy[q] += it.D[0][q];
        };
        double g_new[smc_root::kRoots];
        smc_root::eval(t_new, y_new, theta, cond, g_new);
        const bool fired = smc_root::any_active(it.g, g_new);
        double t_stop = t_new;
        int k_fire = -1;
        if (fired) {
            k_fire = smc_root::first_root(it.g, g_new, sol, t, t_new, theta, cond, t_stop);
            if (k_fire < 0 || t_stop == it.t_seg) {
                it.status = -1;
                return;
            }
        }
#pragma unroll
        for (int q = 0; q < smc_root::kRoots; ++q) it.g[q] = g_new[q];      // ivp.py: g = g_new
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
            double y[NS];
            sol(t_stop, y);
            it.t = t_stop;
            smc_user_ieee::smc_user_root_event(k_fire, t_stop, y, theta, cond);
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
                smc_user_ieee::smc_user_event(it.i_ev, t_stop, y, theta, cond);
                ++it.i_ev;
                it.t_bound = smc_ev::segment_bound(cond, it.i_ev, it.t_end);
            }
            segment_start(it, y, theta, cond, rtol, atol);
            root_segment(it, it.D[0], theta, cond);
            it.status = 0;
            return;
        }
        // the segment ends at scheduled event i_ev, as below; the next one starts with the event functions at (tau, y)
        if (t_new - t_bound >= 0 && t_bound < it.t_end) {
            double y[NS];
#pragma unroll
            for (int s = 0; s < NS; ++s) y[s] = it.D[0][s];
            smc_user_ieee::smc_user_event(it.i_ev, t_new, y, theta, cond);
            ++it.i_ev;
            it.t_bound = smc_ev::segment_bound(cond, it.i_ev, it.t_end);
            segment_start(it, y, theta, cond, rtol, atol);
            root_segment(it, it.D[0], theta, cond);
            it.status = 0;
            return;
        }
    }
#else  // SMC_USER_ROOTS
    if (accepted && it.t_next <= t_new) {     // outputs in (t, t_new] (and t_eval[0] = t0 on the first step): BdfDenseOutput
        const int k = it.order;
        const double hd = it.h_abs;
        int i_out = it.i_out;
        DataRec nx = tp[i_out];
        do {
            double p = 1.0, yy[NS];
#pragma unroll
            for (int s = 0; s < NS; ++s) yy[s] = 0.0;
#pragma unroll
            for (int j = 0; j < kMaxOrder; ++j) {
                const double t_shift = t_new - hd * j, denom = hd * (1 + j);
                p = (j == 0) ? (nx.x - t_shift) / denom : p * ((nx.x - t_shift) / denom);
#pragma unroll
                for (int s = 0; s < NS; ++s) yy[s] = (j < k) ? yy[s] + it.D[j + 1][s] * p : yy[s];
            }
#pragma unroll
            for (int s = 0; s < NS; ++s) yy[s] += it.D[0][s];
            emit(it, yy, theta, cond, nx.x, nx.y);
            ++i_out;
            nx = tp[i_out];                          // i_out == n_t reads the sentinel (+inf, 0)
        } while (nx.x <= t_new);
        it.i_out = i_out;
        it.t_next = nx.x;
    }
#ifdef SMC_USER_EVENTS
    // The accepted step ends a segment in front of event i_ev (t_new == t_bound == tau < t_end).  The outputs up to and including
    // tau are out, from the state BEFORE the event; now the event changes the end state D[0] and the next segment starts afresh
    // from (tau, y), as a new solve_ivp call would: segment_start.  The item goes on (status 0).
    // Termination: every event application advances i_ev, and i_ev <= SMC_USER_NEV because an event fires only with a finite
    // tau < t_end and the table ends in +inf, so an item has at most SMC_USER_NEV + 1 segments.  Event times increase strictly
    // and lie above t0, so every segment has positive length, and inside it the item is the solve it always was: t reaches
    // t_bound, or TOO_SMALL_STEP above stops it (Ops::attempt bounds the attempts besides).  No loop is added.
    if (accepted && t_new - t_bound >= 0 && t_bound < it.t_end) {
        double y[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) y[s] = it.D[0][s];
        smc_user_ieee::smc_user_event(it.i_ev, t_new, y, theta, cond);
        ++it.i_ev;
        it.t_bound = smc_ev::segment_bound(cond, it.i_ev, it.t_end);
        segment_start(it, y, theta, cond, rtol, atol);
        it.status = 0;
        return;
    }
#endif  // SMC_USER_EVENTS
#endif  // SMC_USER_ROOTS
    it.status = (accepted && t_new - t_bound >= 0) ? 1 : 0;    // base.py
}
// What user_item_ops.h needs to know about the integrator (see the list at the top of that file).  Pool words 6 ..: y = D[0],
// f = D[1] - only an item that has not had an attempt yet goes through the pool - and no flag in word 3.  The four work
// counters of an item are published wherever it ends.
struct Bdf {
    using Item = smc_user_bdf::Item;
    static __device__ __forceinline__ void begin(Item &s, const double *theta, const double *cond, const DataRec *tp, int n_t, double rtol,
                                                 double atol) { item_begin(s, theta, cond, tp, n_t, rtol, atol); }
    static __device__ __forceinline__ void attempt(Item &s, const double *theta, const double *cond, const DataRec *tp, double rtol,
                                                   double atol) { item_attempt(s, theta, cond, tp, rtol, atol); }
    static __device__ __forceinline__ int pool_flag(const Item &) { return 0; }
    static __device__ __forceinline__ void set_pool_flag(Item &, int) {}
    static __device__ __forceinline__ void pack(const Item &s, double *w) {
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            w[i * 64] = s.D[0][i];            // y0
            w[(NS + i) * 64] = s.D[1][i];     // f(t0, y0)
        }
    }
    static __device__ __forceinline__ void unpack(Item &s, const double *w) {
        item_reset_lane(s);
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            s.D[0][i] = w[i * 64];
            s.D[1][i] = w[(NS + i) * 64];
        }
    }
    static __device__ __forceinline__ void broadcast(Item &u, const Item &s, int src) {
        lane_progress(u, s, src);
#pragma unroll
        for (int r = 0; r < kRows; ++r)
#pragma unroll
            for (int i = 0; i < NS; ++i) u.D[r][i] = smc::lane_value(s.D[r][i], src);
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            u.jac_factor[i] = smc::lane_value(s.jac_factor[i], src);
            u.piv[i] = __builtin_amdgcn_readlane(s.piv[i], src);
#pragma unroll
            for (int j = 0; j < NS; ++j) {
                u.J[i][j] = smc::lane_value(s.J[i][j], src);
                u.LU[i][j] = smc::lane_value(s.LU[i][j], src);
            }
        }
        u.order = __builtin_amdgcn_readlane(s.order, src);
        u.n_equal_steps = __builtin_amdgcn_readlane(s.n_equal_steps, src);
        lane_outputs(u, s, src);
        const int flags = (int)s.fresh | ((int)s.in_step << 1) | ((int)s.current_jac << 2) | ((int)s.lu_valid << 3);
        const int uf = __builtin_amdgcn_readlane(flags, src);
        u.fresh = (uf & 1) != 0;
        u.in_step = (uf & 2) != 0;
        u.current_jac = (uf & 4) != 0;
        u.lu_valid = (uf & 8) != 0;
        u.n_steps = (unsigned)__builtin_amdgcn_readlane((int)s.n_steps, src);
        u.n_newton = (unsigned)__builtin_amdgcn_readlane((int)s.n_newton, src);
        u.n_lu = (unsigned)__builtin_amdgcn_readlane((int)s.n_lu, src);
        u.n_jac = (unsigned)__builtin_amdgcn_readlane((int)s.n_jac, src);
    }
    static __device__ __forceinline__ void no_work(Item &s) { s.n_steps = s.n_newton = s.n_lu = s.n_jac = 0u; }
#ifdef SMC_USER_ROOTS
    // an item out of the pool (it stands at t0): the event functions there again, no fire yet
    static __device__ __forceinline__ void root_begin(Item &s, const double *theta, const double *cond) { smc_user_item::root_begin(s, s.D[0], theta, cond); }
#endif  // SMC_USER_ROOTS
    // counts[k * m + idx], k: accepted steps, Newton iterations, LU factorisations, Jacobians
    static __device__ __forceinline__ void publish_work(unsigned *counts, long long m, long long idx, const Item &s) {
        counts[idx] = s.n_steps;
        counts[m + idx] = s.n_newton;
        counts[2 * m + idx] = s.n_lu;
        counts[3 * m + idx] = s.n_jac;
    }
};
}  // namespace smc_user_bdf

#ifdef SMC_USER_NOBS
extern "C" __global__ void __launch_bounds__(256) smc_user_solve_kernel(smc::UserSolveArgs a, unsigned *counts, smc::UserObsArgs o) {
    SMC_USER_KERNEL_BODY(smc_user_bdf::Bdf, counts)
}
#else
extern "C" __global__ void __launch_bounds__(256) smc_user_solve_kernel(smc::UserSolveArgs a, unsigned *counts) {
    SMC_USER_KERNEL_BODY(smc_user_bdf::Bdf, counts)
}
#endif
#undef smc_user_bdf
#undef smc_user_item
#undef smc_user_solve_kernel
#undef SMC_USER_PRED
