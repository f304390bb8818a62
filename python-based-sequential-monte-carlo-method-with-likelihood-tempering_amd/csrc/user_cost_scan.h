#ifdef SMC_USER_HAS_COST
// The cost hint of the model (include/smc_hip.h): smc_user_cost(theta) ~ RK45 step attempts of one solve.  Above
// SMC_USER_LIST_COST attempts a particle's solves are handed out before the index-ordered items, above SMC_USER_SOLO_COST they
// run one per wave (solve_sched.h) - the thresholds of the built-in Michaelis-Menten kernel (Vmax > 60 Km, > 1000 Km) in
// attempts (3.7 Vmax / Km).  One atomic per listed lane, no cross-lane read after it; every particle at most once.
extern "C" __global__ void __launch_bounds__(256) smc_user_cost_scan_kernel(smc::UserScanArgs a) {
    if (blockIdx.x == 0 && threadIdx.x < 2) a.count_next[threadIdx.x] = 0u;
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= a.n) return;
    double th[SMC_USER_DIM];
#pragma unroll
    for (int c = 0; c < SMC_USER_DIM; ++c) th[c] = a.theta[c * a.stride + p];
    const bool masked = a.p0 && a.p0[p] == 0;
    const double cost = masked ? 0.0 : smc_user_ieee::smc_user_cost(th);
    const bool on_list = cost > SMC_USER_LIST_COST;     // false for NaN
    a.listed[p] = on_list ? 1 : 0;
    if (a.bucket) {      // cost class: four per factor of two in the hint, the longest first (NaN and < 1: the last real class)
        unsigned b = 127u;
        if (masked) {
            for (int e = 0; e < a.n_ex; ++e) {
                a.done_sums[(long long)e * a.n + p] = 0.0;
                a.done_info[(long long)e * a.n + p] = 0;
            }
        } else {
            const int u = (cost >= 1.0) ? (int)(__float_as_uint((float)cost) >> 21) - 127 * 4 : 0;
            b = (unsigned)(123 - (u < 0 ? 0 : (u > 123 ? 123 : u)));
        }
        a.bucket[p] = (unsigned char)b;
    }
    if (!on_list) return;
    if (cost > SMC_USER_SOLO_COST) {
        const unsigned k = atomicAdd(a.count + 1, 1u);
        if (k < a.solo_cap) {
            a.stiff_list[a.stiff_cap - 1 - (long long)k] = (int)p;
            return;
        }
    }
    a.stiff_list[atomicAdd(a.count, 1u)] = (int)p;
}
#endif
