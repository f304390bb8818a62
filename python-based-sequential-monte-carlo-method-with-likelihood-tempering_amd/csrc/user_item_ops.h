// user_item_ops.h -- everything of a user-model kernel that is not an integrator: the data an item reads and what an output
// adds to it ("data side"), the adapter that lets the scheduler of the built-in Michaelis-Menten kernel (solve_sched.h) run
// the user's model, with exact early rejection and the prediction stores, and the body of the kernel entry.  Device code only,
// handed to hiprtc as an in-memory header; user_rk45_kernel.h and user_bdf_kernel.h (one per SMC_USER_METHOD_*) include it
// first and then define their integrator and a description of it, `Integ`, which the templates here consume:
//     using Item                       the resumable state of one solve.  This file reads and writes its t, h_abs, sr2, t_bound,
//                                      t_next, i_out, status (0 running, 1 finished, < 0 failed), with SMC_USER_NOBS pred, with
//                                      SMC_USER_NOISE nz; Item::kFuseOutputs says whether an output's residuals may contract
//     begin(s, theta, cond, row, n_t, rtol, atol), attempt(s, theta, cond, row, rtol, atol)
//     pool_flag(s), set_pool_flag(s, flag), pack(s, w), unpack(s, w)
//                                      the integrator's own part of a started item in the pool: a flag for the low half of word
//                                      3, and its 2 NS words from word 6 on (unpack also sets up whatever the pool does not hold)
//     broadcast(u, s, src)             ALL of s read from lane src: the integrator's own registers, and among them, where it wants
//                                      them, the two shared groups lane_progress and lane_outputs below
//     no_work(s), publish_work(counts, m, idx, s)
//                                      per-item work counters ([k * m + idx], m = n_ex * n): a masked proposal has none; written
//                                      wherever an item ends (start, finish, cancel).  Empty for an integrator that has no counters.
// A third integrator is such a struct; a new per-item feature is written here, once.  Where a hook is called, and the order
// of the statements around it, is what the two kernels had before they shared this text: the gfx950 code depends on it
// (DEVLOG.md), and tools/user_source_equiv.py compares a change of this file with the build before it.
//
// One text, three kernels:
//   * the one-output kernel of smc_set_model_user / 2 (SMC_USER_NOBS not defined): data as (time, observation) pairs;
//   * with SMC_USER_NOBS defined (smc_set_model_user3, user_obs_args.h) the kernel file is appended TWICE: first the sweep
//     kernel over records of n_obs outputs, then with SMC_USER_PRED 1 the prediction kernel smc_user_predict_kernel, so that the
//     sweep kernel's code does not carry the prediction stores.  The second time this namespace and the entry point go under
//     the names below (a kernel file renames its integrator's namespace the same way) and the kernel file undefines them, and
//     SMC_USER_PRED, at its end.  Hence no #pragma once.
// What differs between the three is in the blocks marked "data side" and "prediction".
#ifndef SMC_USER_PRED
#define SMC_USER_PRED 0
#endif
#if SMC_USER_PRED
#define smc_user_item smc_user_item_pred
#define smc_user_solve_kernel smc_user_predict_kernel
#endif
#include "sweep_args.h"     // in-memory headers handed to hiprtc by the library: the argument blocks,
#include "reject_bound.h"   // the tail of the early-rejection bound (with philox.h: it re-derives the acceptance uniform),
#include "solve_sched.h"    // the scheduler the built-in Michaelis-Menten kernel uses
#define NS SMC_USER_NS
#ifdef SMC_USER_ROOTS
#include "user_root.h"      // state-triggered events: the test, the root solve and the choice of the earliest root
#endif  // SMC_USER_ROOTS
namespace smc_user_item {
__device__ __forceinline__ double py_min(double a, double b) { return (b < a) ? b : a; }   // Python's min / max
__device__ __forceinline__ double py_max(double a, double b) { return (b > a) ? b : a; }

// ---- data side: one data time of an experiment, the end time of its row, and what an output adds to the item ----
#ifdef SMC_USER_NOBS
// several outputs: the records of user_obs_args.h; the row's own end time is kept in its last record
using DataRec = smc_obs::Rec;
__device__ __forceinline__ double t_bound_of(const DataRec *tp, int n_t) { return tp[n_t].y[0]; }
template <class It>
__device__ __forceinline__ void emit(It &it, const double *yy, const double *theta, const double *cond, double t_out, const double *obs) {
#if defined(SMC_USER_NOISE) && SMC_USER_NOISE
    smc_obs::emit_noise<SMC_USER_PRED, It::kFuseOutputs>(it.sr2, it.pred, it.nz, yy, theta, cond, t_out, obs);
#else
    smc_obs::emit<SMC_USER_PRED, It::kFuseOutputs>(it.sr2, it.pred, yy, theta, cond, t_out, obs);
#endif
}
#else
// one output: n_t + 1 (time, observation) pairs, the last one the sentinel (+inf, 0) - as in the built-in kernel
// (mm_rk45.h: mm_table_fill), so that an output costs ONE ds_read_b128 and no test for the end of the row
using DataRec = double2;
__device__ __forceinline__ double t_bound_of(const DataRec *tp, int n_t) { return tp[n_t - 1].x; }
template <class It>
__device__ __forceinline__ void emit(It &it, const double *yy, const double *theta, const double *cond, double t_out, double obs) {
    const double r = obs - smc_user_ieee::smc_user_obs(t_out, yy, theta, cond);
    if (It::kFuseOutputs) {
        it.sr2 += r * r;
    } else {
#pragma clang fp contract(off)
        it.sr2 += r * r;
    }
}
#endif
// ---- end of the data side ----
#ifdef SMC_USER_EVENTS
// Scheduled events: an item also holds t_end, the end time of its row, and i_ev, the index of its next event = the first
// event with tau > t; t_bound is the bound of the SEGMENT it is in (user_event.h: segment_bound).  This is for an item that has
// had no attempt (item_begin, the pool's unpack): it stands at t0, and every event time of a row is > t0, so i_ev = 0.
template <class It>
__device__ __forceinline__ void item_cache_times(It &it, const double *cond, const DataRec *tp, int n_t) {
    it.t_end = t_bound_of(tp, n_t);
    it.i_ev = 0;
    it.t_bound = smc_ev::segment_bound(cond, 0, it.t_end);
    it.t_next = tp[it.i_out].x;
}
#ifdef SMC_USER_ROOTS
// State-triggered events (user_root.h): an item also holds g, the event functions at its last accepted point, t_seg, the start
// of the segment it is in (a root there fails the solve), and n_fire, the events that have fired.  They are registers: the pool
// holds only items that have had no attempt, for which root_begin computes them again from (t0, y0) - the numbers item_begin
// computed, from the same operands through the same function - and the uniform tail reads them from the lane (lane_progress).
// root_segment: the start of a segment at (it.t, y).
template <class It>
__device__ __forceinline__ void root_segment(It &it, const double *y, const double *theta, const double *cond) {
    smc_root::eval(it.t, y, theta, cond, it.g);
    it.t_seg = it.t;
}
template <class It>
__device__ __forceinline__ void root_begin(It &it, const double *y, const double *theta, const double *cond) {
    root_segment(it, y, theta, cond);
    it.n_fire = 0;
}
#endif  // SMC_USER_ROOTS
#else  // SMC_USER_EVENTS
template <class It>
__device__ __forceinline__ void item_cache_times(It &it, const DataRec *tp, int n_t) {
    it.t_bound = t_bound_of(tp, n_t);
    it.t_next = tp[it.i_out].x;
}
#endif  // SMC_USER_EVENTS
// An item's registers read from lane src (the uniform tail of solve_sched.h), in two groups that an integrator's broadcast
// places among its own: where the solve stands, and which output comes next
template <class It>
__device__ __forceinline__ void lane_progress(It &u, const It &s, int src) {
    u.t = smc::lane_value(s.t, src);
    u.h_abs = smc::lane_value(s.h_abs, src);
    u.sr2 = smc::lane_value(s.sr2, src);
    u.t_bound = smc::lane_value(s.t_bound, src);
    u.t_next = smc::lane_value(s.t_next, src);
#ifdef SMC_USER_EVENTS
    u.t_end = smc::lane_value(s.t_end, src);
    u.i_ev = __builtin_amdgcn_readlane(s.i_ev, src);
#ifdef SMC_USER_ROOTS
#pragma unroll
    for (int k = 0; k < smc_root::kRoots; ++k) u.g[k] = smc::lane_value(s.g[k], src);
    u.t_seg = smc::lane_value(s.t_seg, src);
    u.n_fire = __builtin_amdgcn_readlane(s.n_fire, src);
#endif  // SMC_USER_ROOTS
#endif  // SMC_USER_EVENTS
}
template <class It>
__device__ __forceinline__ void lane_outputs(It &u, const It &s, int src) {
#ifdef SMC_USER_NOBS   // prediction
    u.pred = SMC_USER_PRED ? (double *)smc::lane_value_ll((long long)s.pred, src) : nullptr;
#endif
    u.i_out = __builtin_amdgcn_readlane(s.i_out, src);
    u.status = __builtin_amdgcn_readlane(s.status, src);
}

// What solve_sched.h needs to know about an item of the user model (see the list at the top of that file): the built-in
// Michaelis-Menten kernel's scheduler - chunked dequeue, pool of started items in LDS, tight attempt loop, uniform tail,
// exact early rejection - runs the user's model unchanged.
template <class Integ>
struct Ops {
    struct Item {
        typename Integ::Item s;
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
    unsigned n_list;            // a cost hint (smc_user_cost; smc_user_cost_scan_kernel builds the lists), else nullptr / 0
    const int *solo;            // ... and its longest solves, one per wave on uniform operands
    unsigned n_solo;
    int patience;               // in-phase waves (solve_sched.h): with the cost order of a model that comes with a cost hint
    long long n_pos;            // positions of the index-ordered pass
    const DataRec *s_tp;        // the data of all experiments in LDS: rows of n_t + 1 records (the data side above)
    unsigned *counts;           // Integ::publish_work's array; nullptr for an integrator without counters
    double *pred;               // UserObsArgs::pred; nullptr in every kernel but the prediction kernel

    __device__ __forceinline__ const double *cond(int e) const { return a.cond + (long long)e * a.n_cond; }
    __device__ __forceinline__ const DataRec *row(int e) const { return s_tp + e * (a.n_t + 1); }
    __device__ __forceinline__ long long particle(const Item &it) const { return it.out_idx - (long long)it.e * a.n; }
    __device__ __forceinline__ void publish(long long idx, double sum, int info) const {
        // visible to the waves of other XCDs while the kernel runs (the early-rejection bound reads the siblings' sums)
        __hip_atomic_store(reinterpret_cast<unsigned long long *>(a.sum_r2) + idx, (unsigned long long)__double_as_longlong(sum),
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        a.info[idx] = info;
    }
    __device__ __forceinline__ void publish_work(const Item &it) const { Integ::publish_work(counts, (long long)a.n_ex * a.n, it.out_idx, it.s); }
    // ---- prediction: smc_user_predict_kernel (SMC_USER_PRED 1) writes the model's outputs to `pred`; an item's pointer to its
    // next output follows from out_idx and i_out (no pool word).  A one-output item has no such pointer.
#ifdef SMC_USER_NOBS
    __device__ __forceinline__ void set_pred(Item &it, int i) const {
        it.s.pred = SMC_USER_PRED ? pred + ((particle(it) * a.n_ex + it.e) * a.n_t + i) * smc_obs::kObs : nullptr;
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
            Integ::no_work(nb.s);
            publish_work(nb);
            publish(nb.out_idx, 0.0, 0);
            return smc::kStartDone;
        }
        load_theta(nb, p);
        set_pred(nb, 0);
        Integ::begin(nb.s, nb.th, cond(e), row(e), a.n_t, a.rtol, a.atol);
        if (nb.s.status == 0) return smc::kStartStarted;
        publish_work(nb);
        pred_tail(nb);
        publish(nb.out_idx, nb.s.sr2, nb.s.status < 0 ? (1 << 30) : 0);
        return smc::kStartDone;
    }
    // the pool of started items: words 0 - 5 here, the integrator's 2 NS words behind them
    __device__ __forceinline__ void pack(const Item &nb, double *slot) const {
        slot[0 * 64] = nb.s.t;
        slot[1 * 64] = nb.s.h_abs;
        slot[2 * 64] = nb.s.sr2;
        slot[3 * 64] = __hiloint2double(nb.s.i_out, Integ::pool_flag(nb.s));
        slot[4 * 64] = __hiloint2double((int)nb.attempts, nb.e);
        slot[5 * 64] = __longlong_as_double(nb.out_idx);
        Integ::pack(nb.s, slot + 6 * 64);
    }
    __device__ __forceinline__ void unpack(Item &it, const double *slot) const {
        it.s.t = slot[0 * 64];
        it.s.h_abs = slot[1 * 64];
        it.s.sr2 = slot[2 * 64];
        const double w4 = slot[4 * 64], w3 = slot[3 * 64];
        Integ::set_pool_flag(it.s, __double2loint(w3));
        it.s.i_out = __double2hiint(w3);
        it.e = __double2loint(w4);
        it.attempts = (unsigned)__double2hiint(w4);
        it.out_idx = __double_as_longlong(slot[5 * 64]);
        set_pred(it, it.s.i_out);
        it.s.status = 0;
        Integ::unpack(it.s, slot + 6 * 64);
#ifdef SMC_USER_EVENTS
        item_cache_times(it.s, cond(it.e), row(it.e), a.n_t);
#else  // SMC_USER_EVENTS
        item_cache_times(it.s, row(it.e), a.n_t);
#endif  // SMC_USER_EVENTS
        load_theta(it, particle(it));      // the parameters come from HBM / L2 again, not through the pool
#ifdef SMC_USER_ROOTS
        Integ::root_begin(it.s, it.th, cond(it.e));
#endif  // SMC_USER_ROOTS
    }
    __device__ __forceinline__ int attempt(Item &it) const {
        Integ::attempt(it.s, it.th, cond(it.e), row(it.e), a.rtol, a.atol);
        ++it.attempts;
        if (it.attempts >= 0x1fffffffu) it.s.status = -1;        // hard bound so that every wave drains
        return it.s.status;
    }
    __device__ __forceinline__ int attempt_lane(Item &it) const { return attempt(it); }
    __device__ __forceinline__ int uniform_attempts(Item &it, int budget) const { return smc::uniform_attempts_plain(*this, it, budget); }
    __device__ __forceinline__ bool long_running(const Item &it) const { return it.attempts > 64u; }
    __device__ __forceinline__ long long positions() const { return n_pos; }
    __device__ __forceinline__ int start_at(long long pos, int e, Item &nb) const {
        return start(a.order ? (long long)a.order[pos] : pos, e, false, nb);
    }
    __device__ __forceinline__ void finish(Item &it, int st) const {
        pred_tail(it);
        publish_work(it);
        publish(it.out_idx, it.s.sr2, (int)(it.attempts & 0x1fffffffu) | ((st < 0) ? (1 << 30) : 0));
    }
    __device__ __forceinline__ void cancel(Item &it) const {
        publish_work(it);
        publish(it.out_idx, -1.0, (int)(it.attempts & 0x1fffffffu) | (1 << 29));
    }
    __device__ __forceinline__ Item broadcast(const Item &it, int src) const {
        Item u;
        Integ::broadcast(u.s, it.s, src);
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
    // EXACT early rejection, as for the built-in model (mm_kernels.hip: mm_certainly_rejected): lk1 and rr are fixed before the
    // sweep and the likelihood only falls while a solve serves outputs, so a proposal that fails the accept test with the sums
    // accumulated SO FAR (0 for a sibling still running) is rejected whatever the rest would add (reject_bound.h).
#if defined(SMC_USER_NOISE) && SMC_USER_NOISE
    // Under a noise model (user_obs_args.h) every observation not yet served sits at its floor log(a_k s_k), known from theta,
    // and the published sums are excesses over it, which only grow.  user_finish_noise_kernel's expression, in its order.
    __device__ __forceinline__ bool certainly_rejected(const Item &it) const {
        const long long p = particle(it);
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
                const double v = smc::sibling_sum(a.sum_r2, (long long)k * a.n + p);
                if (v < 0.0) return true;      // a sibling has already established the rejection
                if (v == v) S = v;             // finished; NaN = still running: counts as 0
            }
            lk2_bound += smc_obs::noise_floor_of(k, la, a.n_ex, a.n_t) - S;
        }
        return smc::reject_bound_fails(*a.rej, p, lk2_bound);
    }
#else
    // The Gaussian likelihood lk2 = sum_e [c0 - sum_r2_e / (2 sigma^2)] (Micmem_likelihood.py:70-73): the sums of squared
    // residuals only grow.  The expression is the one user_finish_kernel evaluates, in the same order.
    __device__ __forceinline__ bool certainly_rejected(const Item &it) const {
        const long long p = particle(it);
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
                const double v = smc::sibling_sum(a.sum_r2, (long long)k * a.n + p);
                if (v < 0.0) return true;      // a sibling has already established the rejection
                if (v == v) S = v;             // finished; NaN = still running: counts as 0
            }
#ifdef SMC_USER_NOBS    // data side: the experiment's own count and scales
            const double c0 = (-0.5 * smc_obs::me(k)) * lg - smc_obs::sum_log_scale(k, a.n_ex);
#endif
            lk2_bound += c0 - S / (2.0 * s2);
        }
        return smc::reject_bound_fails(*a.rej, p, lk2_bound);
    }
#endif
};

}  // namespace smc_user_item

// The body of smc_user_solve_kernel, SMC_USER_KERNEL_BODY(Integ, counts), with the kernel's arguments `a` (and with
// SMC_USER_NOBS `o`) in scope; `counts` is Ops::counts.  Outputs per item: the sum of squared residuals, attempts |
// cancelled << 29 | failed << 30 and what Integ::publish_work writes.  LDS per wave: a ring of 64 started items of
// Ops::kPoolWords words; then the data, read by every output.
// A macro and not a function: handed on to a function, by reference, pointer or value, the argument block is read from the
// kernel-argument segment all at once at the kernel's entry instead of where a field is used, and the attempt loops pay
// for it in spilled scalar registers (gfx950 listings of every case of tools/user_source_equiv.py).
#ifdef SMC_USER_NOBS   /* data side: the image the host has built (user_obs_args.h) */
#define SMC_USER_KERNEL_DATA(OPS)                                                                                          \
    static_assert(4 * OPS::kPoolWords * 64 == smc_obs::kHdrAt, "user_obs_args.h: the image follows the pools");            \
    const smc_obs::Rec *s_tp = smc_obs::table(a.n_ex);                                                                     \
    for (int i = threadIdx.x; i < o.img_len; i += blockDim.x) smc_obs::lds()[i] = o.img[i];                                \
    double *const pred = o.pred;
#else                  /* data side: the table of (time, observation) pairs, built here */
#define SMC_USER_KERNEL_DATA(OPS)                                                                                          \
    double2 *s_tp = reinterpret_cast<double2 *>(s_pool_all + 4 * (OPS::kPoolWords * 64));                                  \
    for (int i = threadIdx.x; i < a.n_ex * (a.n_t + 1); i += blockDim.x) {                                                 \
        const int e = i / (a.n_t + 1), k = i - e * (a.n_t + 1);                                                            \
        s_tp[i] = (k < a.n_t) ? make_double2(a.t[e * a.n_t + k], a.obs[e * a.n_t + k])                                     \
                              : make_double2(__longlong_as_double(0x7ff0000000000000LL), 0.0);                             \
    }                                                                                                                      \
    double *const pred = nullptr;
#endif
#define SMC_USER_KERNEL_BODY(INTEG, COUNTS)                                                                                \
    using UserOps = smc_user_item::Ops<INTEG>;                                                                             \
    extern __shared__ double s_pool_all[];                                                                                 \
    double *s_pool = s_pool_all + (threadIdx.x >> 6) * (UserOps::kPoolWords * 64);                                         \
    SMC_USER_KERNEL_DATA(UserOps)                                                                                          \
    __syncthreads();                                                                                                       \
    const unsigned n_list = a.stiff_list ? (unsigned)__builtin_amdgcn_readfirstlane((int)a.stiff_count[0]) : 0u;           \
    unsigned n_solo = a.stiff_list ? (unsigned)__builtin_amdgcn_readfirstlane((int)a.stiff_count[1]) : 0u;                 \
    if (n_solo > a.solo_cap) n_solo = a.solo_cap; /* the overflow went onto the ordinary list */                           \
    UserOps ops{a, a.n, a.n_ex, a.stiff_list, n_list, a.stiff_list ? a.stiff_list + (a.stiff_cap - 1) : nullptr, n_solo,   \
                a.patience, a.n_ordered ? (long long)__builtin_amdgcn_readfirstlane((int)a.n_ordered[0]) : a.n, s_tp,      \
                COUNTS, pred};                                                                                             \
    smc::solve_persistent(ops, a.queue, s_pool);
