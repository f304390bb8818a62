// user_root.h -- state-triggered events of a user model (include/smc_hip.h: STATE-TRIGGERED EVENTS): the source defines event
// functions g_k(t, y), a solve stops where one of them crosses zero in its direction, the state jumps and the integrator starts
// afresh - solve_ivp(events=...) with every event terminal, and the restart a SciPy user writes around it.  Device code only,
// handed to hiprtc as an in-memory header and included (by user_item_ops.h, under SMC_USER_ROOTS) ONLY for a source that contains
// the name smc_user_root; every other model never sees this file, and the kernel files reach it stripped of their
// SMC_USER_ROOTS blocks (csrc/Makefile: strip_roots.awk), the text they had before this feature existed.
//
// What is here is what the two integrators share: the test of scipy/integrate/_ivp/ivp.py find_active_events, the root solve
// of solve_event_equation - scipy/optimize/Zeros/brentq.c restated statement by statement, xtol = rtol = 4 EPS, 100 iterations -
// and handle_events' choice of the earliest root.  The dense output a root is sought on, the truncation of the step and the
// restart are the integrator's (the SMC_USER_ROOTS blocks of user_rk45_kernel.h and user_bdf_kernel.h).
//
// A model with state-triggered events is always compiled with the SMC_USER_EVENTS blocks as well - a triggered restart is a
// segment restart, and a root may fall on a scheduled event's time.  Where the model has no scheduled events
// (SMC_USER_NO_SCHEDULE, defined by build_source) the two names those blocks use are supplied here: a table that never holds an
// event, so that every segment's bound is the row's end and the scheduled-event branch is never taken.
#pragma once
#ifndef __HIPCC_RTC__
#include <hip/hip_runtime.h>
#endif

#ifdef SMC_USER_NO_SCHEDULE
namespace smc_ev {
__device__ __forceinline__ double segment_bound(const double *, int, double t_end) { return t_end; }
}  // namespace smc_ev
namespace smc_user_ieee {
__device__ __forceinline__ void smc_user_event(int, double, double *, const double *, const double *) {}
}  // namespace smc_user_ieee
#endif

namespace smc_root {

constexpr int kMaxRoots = 4;       // SMC_USER_MAX_ROOTS
constexpr int kMaxFires = 256;     // SMC_USER_MAX_ROOT_FIRES
constexpr int kMaxIter = 100;      // brentq's maxiter
constexpr int kRoots = (int)(sizeof(smc_user_ieee::smc_user_root_dir) / sizeof(smc_user_ieee::smc_user_root_dir[0]));
static_assert(kRoots >= 1 && kRoots <= kMaxRoots, "smc_user_root_dir: a source has 1 .. 4 event functions (SMC_USER_MAX_ROOTS)");
// (the directions themselves are read by the library before the compilation - user_model.hip: root_dir_error -, since the
// elements of a __device__ array are no constant expressions)

// g[0 .. kRoots) at (t, y): always the IEEE-division compilation of the user's text
__device__ __forceinline__ void eval(double t, const double *y, const double *theta, const double *cond, double *g) {
    smc_user_ieee::smc_user_root(t, y, theta, cond, g);
}
// v[k] for a per-lane k, by selects (an indexed read of a register array would go through scratch)
__device__ __forceinline__ double pick(const double *v, int k) {
    double r = v[0];
#pragma unroll
    for (int j = 1; j < kRoots; ++j) r = (k == j) ? v[j] : r;
    return r;
}
// ivp.py find_active_events for event k: a NaN on either side compares false and is never active
__device__ __forceinline__ bool active(int k, const double *g, const double *g_new) {
    const double a = pick(g, k), b = pick(g_new, k);
    int dir = smc_user_ieee::smc_user_root_dir[0];
#pragma unroll
    for (int j = 1; j < kRoots; ++j) dir = (k == j) ? smc_user_ieee::smc_user_root_dir[j] : dir;
    const bool up = a <= 0 && b >= 0, down = a >= 0 && b <= 0;
    return (up && dir > 0) || (down && dir < 0) || ((up || down) && dir == 0);
}
__device__ __forceinline__ bool any_active(const double *g, const double *g_new) {
    bool any = false;
#pragma unroll
    for (int k = 0; k < kRoots; ++k) any = any || active(k, g, g_new);
    return any;
}

// scipy.optimize.brentq(f, xa, xb, xtol = 4 EPS, rtol = 4 EPS, maxiter = 100): Zeros/brentq.c, every product and sum rounded on
// its own.  false where SciPy raises: f(xa) and f(xb) of one sign, a NaN value (_zeros_py.py wraps f so), no convergence within
// the iterations - and, a rule of this library, an infinite value.  The loop is bounded by kMaxIter.
template <class F>
__device__ __forceinline__ bool brentq(const F &f, double xa, double xb, double &root) {
#pragma clang fp contract(off)
    const double xtol = 4 * 0x1.0p-52, rtol = 4 * 0x1.0p-52;
    double xpre = xa, xcur = xb, xblk = 0.0, fblk = 0.0, spre = 0.0, scur = 0.0;
    double fpre = f(xpre);
    if (!__builtin_isfinite(fpre)) return false;
    double fcur = f(xcur);
    if (!__builtin_isfinite(fcur)) return false;
    root = xpre;
    if (fpre == 0) return true;
    root = xcur;
    if (fcur == 0) return true;
    if (__builtin_signbit(fpre) == __builtin_signbit(fcur)) return false;
#pragma unroll 1
    for (int i = 0; i < kMaxIter; ++i) {
        if (fpre != 0 && fcur != 0 && (__builtin_signbit(fpre) != __builtin_signbit(fcur))) {
            xblk = xpre;
            fblk = fpre;
            spre = scur = xcur - xpre;
        }
        if (fabs(fblk) < fabs(fcur)) {
            xpre = xcur;
            xcur = xblk;
            xblk = xpre;
            fpre = fcur;
            fcur = fblk;
            fblk = fpre;
        }
        const double delta = (xtol + rtol * fabs(xcur)) / 2;
        const double sbis = (xblk - xcur) / 2;
        if (fcur == 0 || fabs(sbis) < delta) {
            root = xcur;
            return true;
        }
        if (fabs(spre) > delta && fabs(fcur) < fabs(fpre)) {
            double stry;
            if (xpre == xblk) {      // interpolate
                stry = -fcur * (xcur - xpre) / (fcur - fpre);
            } else {                 // extrapolate
                const double dpre = (fpre - fcur) / (xpre - xcur);
                const double dblk = (fblk - fcur) / (xblk - xcur);
                stry = -fcur * (fblk * dblk - fpre * dpre) / (dblk * dpre * (fblk - fpre));
            }
            const double lim_a = fabs(spre), lim_b = 3 * fabs(sbis) - delta;
            if (2 * fabs(stry) < (lim_a < lim_b ? lim_a : lim_b)) {      // good short step
                spre = scur;
                scur = stry;
            } else {                 // bisect
                spre = sbis;
                scur = sbis;
            }
        } else {                     // bisect
            spre = sbis;
            scur = sbis;
        }
        xpre = xcur;
        fpre = fcur;
        if (fabs(scur) > delta)
            xcur += scur;
        else
            xcur += (sbis > 0 ? delta : -delta);
        fcur = f(xcur);
        if (!__builtin_isfinite(fcur)) return false;
    }
    return false;
}

// ivp.py handle_events with every event terminal: the root of each active event on the step's dense output `sol(s, y)`, the
// earliest of them, on a tie the lowest k (NumPy's argsort of so few roots is an insertion sort: stable).  Returns that k and its
// time in t_root, or -1 where a root solve fails.  One brentq in the text: the loop over the events is not unrolled.
template <class Sol>
__device__ __forceinline__ int first_root(const double *g, const double *g_new, const Sol &sol, double t_old, double t_new,
                                          const double *theta, const double *cond, double &t_root) {
    int k_first = -1;
    bool ok = true;
    t_root = __longlong_as_double(0x7ff0000000000000LL);
#pragma unroll 1
    for (int k = 0; k < kRoots; ++k) {
        if (active(k, g, g_new)) {
            const auto f = [&](double s) {
                double yy[SMC_USER_NS], gg[kRoots];
                sol(s, yy);
                eval(s, yy, theta, cond, gg);
                return pick(gg, k);
            };
            double r;
            if (!brentq(f, t_old, t_new, r)) {
                ok = false;
            } else if (r < t_root) {
                t_root = r;
                k_first = k;
            }
        }
    }
    return ok ? k_first : -1;
}

}  // namespace smc_root
