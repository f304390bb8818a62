// mh_control.h -- the proposal factor (cov_m and its multivariate_normal factor) and the loop control of a batch of Metropolis
// iterations as device functions: mh_control_kernel (stage_kernels.hip) runs them as a one-block kernel, and on one rank the
// last block of the Michaelis-Menten accept kernel to finish (mm_kernels.hip: mm_finish_kernel) runs them in its place.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "smc_internal.h"

namespace smc {

// wave64 sum: six shuffle steps; the result is valid in lane 0
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    return v;
}

// cov_m = np.cov(p_filt.T, bias=True) * w_cov (Micmem_SMC_main.py:212-215) and the factor NumPy's legacy
// multivariate_normal multiplies standard normals with (:220): (u, s, v) = svd(cov_m); x = z @ (sqrt(s)[:, None] * v).
// cov_m is symmetric, so its SVD is its eigen-decomposition with s = |lambda| (sorted descending) and the rows of v the
// eigenvectors: a cyclic Jacobi iteration in ONE thread (d <= 8: a few hundred flops, against a sweep of >= 1 ms).
// Row signs are fixed by making the largest component of every row positive (LAPACK's are arbitrary; the distribution of
// z @ A does not depend on them).  Pinned against driver.mvn_transform in tests/test_gpu_parity.py.
struct WCov {
    double w[SMC_MAX_DIM * SMC_MAX_DIM];
};
// Two sources of the second moments:
//   sums != nullptr  two-pass (np.cov's own algorithm): `mom` = the d(d+1)/2 sums centred about the mean sums / N; the mean is
//                    stored as the shift vector of the iterations that follow;
//   sums == nullptr  carried: `mom` = [sum y (d) | sum y y^T (upper)] with y = x - shift, accumulated by the accept kernel of the
//                    previous iteration about the mean of the iteration before (so |E y| << spread: no cancellation to speak
//                    of): cov = E[y y^T] - E[y] E[y]^T, and the shift moves on to the new mean.
template <int D>
__device__ __forceinline__ void mh_transform_body(const double *__restrict__ mom, const double *__restrict__ sums, double n_global,
                                                  const WCov &wcov, double *__restrict__ shift_io, double *__restrict__ cov_out,
                                                  double *__restrict__ xform_out) {
    // D is a compile-time constant and every loop below is unrolled, so A and V live in registers: the first version, with
    // run-time d and SMC_MAX_DIM arrays in scratch, took 23 us per call - on the critical path of every iteration
    constexpr int d = D;
    double A[D][D], V[D][D];
    const double inv_n = 1.0 / n_global;     // np.true_divide(1, fact), then c *= that (np.cov)
    double ey[D];
#pragma unroll
    for (int a = 0; a < d; ++a) {
        if (sums) {
            ey[a] = 0.0;
            shift_io[a] = sums[a] / n_global;
        } else {
            ey[a] = mom[a] * inv_n;
            shift_io[a] = shift_io[a] + ey[a];
        }
    }
    const double *cent = sums ? mom : mom + d;
    {
        int k = 0;
#pragma unroll
        for (int a = 0; a < d; ++a)
#pragma unroll
            for (int b = a; b < d; ++b) {
                const double v = cent[k++] * inv_n - ey[a] * ey[b];
                A[a][b] = v * wcov.w[a * d + b];
                A[b][a] = v * wcov.w[b * d + a];
            }
    }
#pragma unroll
    for (int a = 0; a < d; ++a)
#pragma unroll
        for (int b = 0; b < d; ++b) {
            cov_out[a * d + b] = A[a][b];
            V[a][b] = (a == b) ? 1.0 : 0.0;
        }
    // w_cov is symmetric in the reference (Micmem_settings.py:94-97); should a caller pass an asymmetric one, the
    // decomposition below is that of the symmetric part
#pragma unroll
    for (int a = 0; a < d; ++a)
#pragma unroll
        for (int b = a + 1; b < d; ++b) A[a][b] = A[b][a] = 0.5 * (A[a][b] + A[b][a]);
#pragma unroll 1
    for (int sweep = 0; sweep < 30; ++sweep) {
        double off = 0.0, diag = 0.0;
#pragma unroll
        for (int p = 0; p < d; ++p) {
            diag += A[p][p] * A[p][p];
#pragma unroll
            for (int q = p + 1; q < d; ++q) off += A[p][q] * A[p][q];
        }
        if (!(off > 1e-34 * diag)) break;   // also leaves on NaN
#pragma unroll
        for (int p = 0; p < d; ++p)
#pragma unroll
            for (int q = p + 1; q < d; ++q) {
                const double apq = A[p][q];
                if (apq != 0.0) {
                    const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
                    const double t = ((theta >= 0.0) ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                    const double cs = 1.0 / sqrt(t * t + 1.0), sn = t * cs;
#pragma unroll
                    for (int r = 0; r < d; ++r) {   // A <- A J
                        const double arp = A[r][p], arq = A[r][q];
                        A[r][p] = cs * arp - sn * arq;
                        A[r][q] = sn * arp + cs * arq;
                    }
#pragma unroll
                    for (int r = 0; r < d; ++r) {   // A <- J^T A
                        const double apr = A[p][r], aqr = A[q][r];
                        A[p][r] = cs * apr - sn * aqr;
                        A[q][r] = sn * apr + cs * aqr;
                    }
#pragma unroll
                    for (int r = 0; r < d; ++r) {
                        const double vrp = V[r][p], vrq = V[r][q];
                        V[r][p] = cs * vrp - sn * vrq;
                        V[r][q] = sn * vrp + cs * vrq;
                    }
                }
            }
    }
    // rows of the factor by |lambda| descending (svd order): rank of column e = number of columns that come before it
#pragma unroll
    for (int e = 0; e < d; ++e) {
        const double le = fabs(A[e][e]);
        int rank = 0;
#pragma unroll
        for (int f = 0; f < d; ++f) {
            const double lf = fabs(A[f][f]);
            rank += (lf > le || (lf == le && f < e)) ? 1 : 0;
        }
        const double sv = sqrt(le);
        double big = V[0][e];
#pragma unroll
        for (int c = 1; c < d; ++c)
            if (fabs(V[c][e]) > fabs(big)) big = V[c][e];
        const double sg = (big < 0.0) ? -1.0 : 1.0;
#pragma unroll
        for (int c = 0; c < d; ++c) xform_out[rank * d + c] = sv * (sg * V[c][e]);
    }
}

// Loop control of a batch (the comment above mh_control_kernel, stage_kernels.hip, says what DECIDE and TRANSFORM do), run by
// all kScanBlock threads of ONE block.  COHERENT: the caller is the last block of the accept kernel to finish; the moment rows
// and the counters were written by other blocks of the SAME kernel, so they are read at agent scope (past the caches that are
// not coherent between the XCDs).  The summation order of the rows does not depend on it.
template <bool COHERENT>
__device__ __forceinline__ unsigned long long ctl_load(const unsigned long long *p) {
    return COHERENT ? __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : *p;
}
template <bool COHERENT>
__device__ __forceinline__ double ctl_load(const double *p) {
    return __longlong_as_double((long long)ctl_load<COHERENT>(reinterpret_cast<const unsigned long long *>(p)));
}
template <int D, bool COHERENT>
__device__ __forceinline__ void mh_control_body(const MHControlArgs &a, const WCov &wcov,
                                                double (*wpart)[D + D * (D + 1) / 2] /* LDS: kScanBlock / 64 rows */) {
    MHControl *ctl = a.ctl;
    const int t = threadIdx.x;
    if (a.mode & kCtlInit) {
        if (t == 0) {
            ctl->stop = 0;
            ctl->n_done = 0;
            ctl->ratio = a.ratio0;
            ctl->thr_stop = a.thr_stop;
            ctl->thr_halve = a.thr_halve;
        }
    } else if (ctl->stop) {
        return;
    }
    constexpr int nv = D + D * (D + 1) / 2;      // == a.nv (the Michaelis-Menten accept kernel writes rows of d + d(d+1)/2 values)
    const unsigned long long *cnt = reinterpret_cast<const unsigned long long *>(a.counters);
    constexpr int kNow = offsetof(SweepCounters, accepted_now) / 8, kEver = offsetof(SweepCounters, accepted_ever) / 8,
                  kFailed = offsetof(SweepCounters, n_failed) / 8;
    if (a.mode & kCtlDecide) {
        if (a.rows) {      // one rank: no all-reduce between the accept kernel and this one, so the row reduction happens here
            // moments_reduce_kernel's summation order per value - thread t adds rows t, t + 256, ... in turn, the wave sums by
            // shuffles, the four waves in order - with all nv values of a row (contiguous) taken in one pass over the rows
            double acc[nv];
#pragma unroll
            for (int v = 0; v < nv; ++v) acc[v] = 0.0;
            for (int i = t; i < a.n_rows; i += blockDim.x) {
                const double *row = a.rows + (size_t)i * nv;
#pragma unroll
                for (int v = 0; v < nv; ++v) acc[v] += ctl_load<COHERENT>(row + v);
            }
#pragma unroll
            for (int v = 0; v < nv; ++v) {
                const double ws = wave_sum(acc[v]);
                if ((t & 63) == 0) wpart[t >> 6][v] = ws;
            }
            __syncthreads();
            if (t < nv) {
                double r = wpart[0][t];
                for (int q = 1; q < kScanBlock / 64; ++q) r += wpart[q][t];
                a.vec[t] = r;
            }
            __syncthreads();      // thread 0 reads the vector back below
            if (t == 0) {
                a.vec[a.nv] = (double)ctl_load<COHERENT>(cnt + kNow);
                a.vec[a.nv + 1] = (double)ctl_load<COHERENT>(cnt + kEver);
                a.vec[a.nv + 2] = (double)ctl_load<COHERENT>(cnt + kFailed);
            }
        } else if (a.counts_local && t == 0) {
            a.vec[a.nv] = (double)ctl_load<COHERENT>(cnt + kNow);
            a.vec[a.nv + 1] = (double)ctl_load<COHERENT>(cnt + kEver);
            a.vec[a.nv + 2] = (double)ctl_load<COHERENT>(cnt + kFailed);
        }
    }
    if (t != 0) return;
    if (a.mode & kCtlDecide) {
        const double acc_now = a.vec[a.nv], acc_ever = a.vec[a.nv + 1], n_failed = a.vec[a.nv + 2];
        MHLogEntry &e = a.log[a.iteration - 1];
        e.accepted_now = acc_now;
        e.accepted_ever = acc_ever;
        e.n_failed = n_failed;
        unsigned long long *snap = reinterpret_cast<unsigned long long *>(&e.snap);
        for (int q = 0; q < (int)(sizeof(SweepCounters) / 8); ++q) snap[q] = ctl_load<COHERENT>(cnt + q);
        e.rk_attempts = e.snap.rk_attempts;       // this rank's
        e.long_items = e.snap.long_items;
        e.solved_items = e.snap.solved_items;
        ctl->n_done = a.iteration;
        if (acc_ever > ctl->thr_stop || n_failed != 0.0) {
            ctl->stop = 1;
            return;
        }
        if (acc_ever < ctl->thr_halve) ctl->ratio = ctl->ratio * 0.5;
    }
    if (a.mode & kCtlTransform) {
        static_assert(nv <= SMC_MAX_DIM + SMC_MAX_DIM * (SMC_MAX_DIM + 1) / 2, "");
        mh_transform_body<D>(a.mom, a.sums, a.n_global, wcov, a.shift_io, a.cov_out, a.xform_out);
        MHLogEntry &e = a.log[a.iteration];
        e.ratio = ctl->ratio;
        for (int i = 0; i < D * D; ++i) e.cov[i] = a.cov_out[i];
    }
}

// What the accept kernel of a Michaelis-Menten sweep needs for its "last block done" tail (mm_kernels.hip): a row of counts per
// block instead of contended atomics, the arrival counter, and - batch of iterations on one rank - the control step that follows
// the sweep, which the last block runs in place of a launch of mh_control_kernel.
constexpr int kFinishCountWords = 8;     // per block: rk_attempts, n_failed, accepted_now, accepted_ever, long_items, solved_items
struct FinishTail {
    unsigned long long *count_rows;      // gridDim.x rows of kFinishCountWords
    unsigned *arrive;                    // zero between kernels: the last block to arrive puts it back
    int fuse_control;                    // run mh_control_body<3> with the arguments below
    MHControlArgs ctl;
    WCov wcov;
};

}  // namespace smc
