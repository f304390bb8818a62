// reject_bound.h -- the tail every exact early-rejection bound ends in (mm_kernels.hip: mm_certainly_rejected; meth_smc.hip:
// meth_certainly_rejected; user_item_ops.h: Ops::certainly_rejected), and the read of a sibling's published sum on the way to
// it.  Each kernel forms an UPPER bound of the proposal's likelihood lk2 in its own way; what it does with the bound is the
// accept test of the sweep, exp((lk2 - lk1) * gamma) [* p0_2 / p0_1] >= rr, with the uniform the accept kernel will use.
// Device code; also handed to hiprtc as an in-memory header (sweep_args.h itself has to stay free of includes).
#pragma once
#include "sweep_args.h"
#include "philox.h"

namespace smc {
#ifdef SMC_PRIOR_MODE_MASK      // the library's own translation units include this file after include/smc_hip.h
static_assert(SMC_PRIOR_MODE_MASK == 0, "reject_bound_fails: the prior ratio is applied in every mode but MASK");
#endif

// The acceptance uniform of particle p: device-RNG mode re-derives it from its Philox counter (a pure function of the key),
// host-RNG mode reads the uniform that was uploaded for the sweep.
__device__ __forceinline__ double reject_uniform(const RejectArgs &r, long long p) {
    if (r.device_rng) {
        const u32x4 ru = philox_block(r.seed, (uint64_t)(r.global_offset + p), r.stream, SMC_PHILOX_BLOCK_UNIFORM);
        return u01_from(ru.x, ru.y);
    }
    return r.rr[p];
}

// true: a proposal whose lk2 cannot exceed lk2_bound fails the accept test, whatever the rest of its solves would add.
// The margin covers a last-bit non-monotonicity of exp; any NaN makes the comparison false.
__device__ __forceinline__ bool reject_bound_fails(const RejectArgs &r, long long p, double lk2_bound) {
    const double rr = reject_uniform(r, p);
    double pp = exp((lk2_bound - r.lk1[p]) * r.gamma);
    if (r.prior_mode != 0) pp = pp * r.pratio[p];      // SMC_PRIOR_MODE_MASK (include/smc_hip.h, which hiprtc does not see)
    return pp < rr * (1.0 - 1e-12);
}

// The sum a sibling item (another experiment of the same particle) has published at sums[idx], read while the kernel runs:
// one relaxed agent-scope load (L2 is per XCD; the store is the kernel's publish).  Three meanings:
//     v < 0     the sibling was cancelled: the rejection is already established;
//     v != v    NaN - still running (or failed): it counts as 0 in an upper bound;
//     else      finished, and v is its sum.
__device__ __forceinline__ double sibling_sum(const double *sums, long long idx) {
    return __longlong_as_double((long long)__hip_atomic_load(reinterpret_cast<const unsigned long long *>(sums) + idx, __ATOMIC_RELAXED,
                                                             __HIP_MEMORY_SCOPE_AGENT));
}

}  // namespace smc
