// meth_dae_wave.h -- wave primitives of K8, the DAE integrator with ONE SOLVE PER WAVE (meth_dae_elem.h) or per pair of waves
// (meth_dae_split.h): wave-uniform scalars, the work-counter dequeue, lane broadcast and the neighbour exchange of lane = node.
// (The model itself, the BDF constants and the host/device reference integrator are in meth_dae.h.)
#pragma once
#include <hip/hip_runtime.h>

#include "meth_dae.h"

namespace smc {
namespace meth {

// Wave-uniform loop control, BY CONSTRUCTION.  Everything that steers a loop of the one-wave-per-solve kernels (the index
// of the next solve, error and Newton norms, hence t, h, the order ...) has the same value in all 64 lanes - but a value
// that reaches the branch through a VGPR (a shuffle, a butterfly sum) is "divergent" to the compiler, which then manages
// the loop with exec masks and may run the two sides of an `if (lane == 0)` as separate trips through the loop.  That is
// what happened to the first dequeue loop of meth_particles_dae_kernel (`for (;;)` + lane-0 atomicAdd + __shfl + `continue`):
// lanes 1..63 reached the ds_bpermute of the __shfl with lane 0 parked on the atomic's side, read 0 from the inactive lane
// and solved item 0 for ever (ISA excerpts: profiles/r02_k8_dequeue_hang_isa.md).  v_readfirstlane puts such a value into
// an SGPR: the branches on it become scalar, no lane can leave a loop or skip a statement on its own, and the DPP / permlane
// / LDS exchanges of the integrator always run with the full wave.
__device__ __forceinline__ double wave_uniform(double v) {
    const int lo = __builtin_amdgcn_readfirstlane(__double2loint(v));
    const int hi = __builtin_amdgcn_readfirstlane(__double2hiint(v));
    return __hiloint2double(hi, lo);
}
// Next index of a work counter shared by all waves, as a scalar.  EVERY lane issues the atomic (lane 0 adds `step`, the others
// add 0; the compiler's atomic optimiser turns that into one wave reduction and one memory atomic) and v_readfirstlane
// takes lane 0's return value: there is NO divergent branch between the atomic and the cross-lane read.  The obvious
// `if (lane == 0) nxt = atomicAdd(...); idx = readfirstlane(nxt);` is not safe: HIP guarantees no re-convergence after the
// `if`, and the compiler is free to run the lanes that skipped it ahead on their own - readfirstlane then returns THEIR
// nxt = 0.  That is how the round-1 K8 dequeue loop hung, and how the first version of mm_tail_kernel hung in round 2
// (profiles/r02_k8_dequeue_hang_isa.md, both listings).  `split` is set when the wave is incomplete here anyway.
__device__ __forceinline__ long long wave_dequeue(unsigned long long *counter, int lane, unsigned &split,
                                                  unsigned long long step = 1ULL) {
    const unsigned long long nxt = atomicAdd(counter, lane == 0 ? step : 0ULL);
    split |= (unsigned)(__builtin_amdgcn_read_exec() != ~0ull);
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)nxt);
    const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(nxt >> 32));
    return (long long)(((unsigned long long)hi << 32) | lo);
}

__device__ __forceinline__ double lane_bcast(double v, int src) {  // src is wave-uniform
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), src);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), src);
    return __hiloint2double(hi, lo);
}

// neighbours' unknowns by shuffles (all lanes participate)
__device__ __forceinline__ void neighbours(const double *w0, double *wm, double *wp) {
SMC_UNROLL
    for (int f = 0; f < 7; ++f) {
        wm[f] = __shfl_up(w0[f], 1);
        wp[f] = __shfl_down(w0[f], 1);
    }
}

}  // namespace meth
}  // namespace smc
