// pointwise_kernels.hip -- pointwise log-likelihood, its per-cell statistics and the PIT on the device (include/smc_hip.h:
// smc_user_pointwise, smc_user_pointwise_summary).  The prediction kernel writes particle-major (one particle's
// cells are contiguous); the statistics are taken per cell over the particles.  Two kernels per group of experiments:
//   pw_terms_kernel   a tile of 32 particles x 32 cells: the term l of every (particle, cell) from the prediction, the particle's
//                     noise parameters and the cell's tables, transposed through LDS into cell-major order (8 B read + 8 B written
//                     per value); on the way Phi((obs - f) / sd) of the tile's particles is summed per cell in index order into
//                     one partial per (cell, tile), so that the PIT costs 16 B per 32 values instead of a second buffer.
//   pw_cell_kernel    one block per cell over the cell's contiguous terms: pass 1 count, max and sum, pass 2 sum exp(l - max) and
//                     sum (l - mean)^2 (2 x 8 B read per value), then the cell's PIT partials.
// Every sum runs per thread in index order and then through a fixed tree (pointwise_reduce.h): no atomics, and a repeated call
// returns the same bits.  The excess functions of censored and count terms are the text the run-time compiled kernels use.
#include <hip/hip_runtime.h>

#define SMC_USER_CENSOR 1
#define SMC_USER_COUNT 1
#include "user_censor.h"
#include "user_count.h"

#include "count_draw.h"
#include "pointwise_kernels.h"
#include "pointwise_reduce.h"
#include "smc_internal.h"

namespace smc {

// a cell's terms start on a 16-byte boundary: the stride is n rounded up to even, the odd one out holds NaN
__host__ __device__ inline int64_t pw_stride(int64_t n) { return (n + 1) & ~(int64_t)1; }
__host__ __device__ inline int64_t pw_tiles(int64_t n) { return (pw_stride(n) + kPwTile - 1) / kPwTile; }

// The term of one observed cell for one particle (user_models.pointwise_loglik is the same in NumPy, operation for operation;
// every product and sum rounded on its own).  code: the cell (pointwise_kernels.h); y: its value; floor_y: count_floor(y) of a
// Poisson value; f: the prediction; a, b, s: the output's a_k, b_k, s_k for this particle; valid: the particle's parameters
// allow a likelihood at all.  phi: Phi((y - f) / sd) where the PIT is defined - a quantified Gaussian value, f finite - else NaN.
__device__ __forceinline__ double pw_term(int code, double y, double floor_y, double f, double a, double b, double s, bool valid, double &phi) {
#pragma clang fp contract(off)
    const double nan = __longlong_as_double(0x7ff8000000000000LL), inf = __builtin_huge_val();
    phi = nan;
    if (!(code & kCellObserved) || f != f) return nan;
    if (!valid) return -inf;
    const int family = (code >> kCellFamilyShift) & 3, flag = (code >> kCellFlagShift) & 3;
    if (family == smc_cnt::kPoisson) return -(floor_y + smc_cnt::poisson_excess(y, f));
    if (family == smc_cnt::kNegBin) return -smc_cnt::negbin_excess(y, f, b * b);
    const double as = a * s, bf = b * f;
    const double sd2 = as * as + bf * bf;
    const double r = y - f;
    if (flag != kCensorNone) {
        const double z = (flag == kCensorLeft ? r : -r) / sqrt(sd2);
        return -smc_cens::censor_excess(z);
    }
    if (fabs(f) < inf) phi = 0.5 * erfc(-(r / sqrt(sd2)) / 1.4142135623730951);
    return (-0.9189385332046727 - 0.5 * log(sd2)) - (r * r) / (2.0 * sd2);
}

// kCountPit: the PIT counts of count cells are formed too (PointwiseArgs::pit_cnt) - the instantiation that holds the sampler,
// pw_terms_count_kernel; without, pw_terms_kernel is what it was before there was one
template <bool kCountPit>
__device__ __forceinline__ void pw_terms_body(const PointwiseArgs &a) {
    __shared__ double tile[kPwTile][kPwTile + 1], phis[kPwTile][kPwTile + 1];
    __shared__ unsigned cnts[kCountPit ? kPwTile : 1][kPwTile + 1];
    __shared__ double s_a[kPwTile][kUserMaxObs], s_b[kPwTile][kUserMaxObs];
    __shared__ int s_valid[kPwTile];
    const int tx = threadIdx.x % kPwTile, ty = threadIdx.x / kPwTile;      // 32 x 8
    const int64_t p0 = (int64_t)blockIdx.x * kPwTile;
    const int c0 = (int)blockIdx.y * kPwTile;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    {   // the noise parameters of the tile's particles, one (particle, output) per thread
        const int pl = threadIdx.x / kUserMaxObs, k = threadIdx.x % kUserMaxObs;
        const int64_t p = p0 + pl;
        double ak = 1.0, bk = 0.0;
        if (p < a.n && k < a.n_obs) {
            ak = a.nz.add_index[k] >= 0 ? a.theta[(int64_t)a.nz.add_index[k] * a.stride + p] : a.nz.add_fixed[k];
            bk = !a.nz.prop ? 0.0 : (a.nz.prop_index[k] >= 0 ? a.theta[(int64_t)a.nz.prop_index[k] * a.stride + p] : a.nz.prop_fixed[k]);
        }
        s_a[pl][k] = ak;
        s_b[pl][k] = bk;
    }
    __syncthreads();
    if (threadIdx.x < kPwTile) {      // every a_k > 0, every b_k >= 0, b_k > 0 on a negative-binomial output (NaN: no)
        bool ok = true;
        for (int k = 0; k < a.n_obs; ++k)
            ok = ok && s_a[threadIdx.x][k] > 0.0 && s_b[threadIdx.x][k] >= 0.0 && (a.family[k] != smc_cnt::kNegBin || s_b[threadIdx.x][k] > 0.0);
        s_valid[threadIdx.x] = ok ? 1 : 0;
    }
    __syncthreads();
    for (int r = ty; r < kPwTile; r += 256 / kPwTile) {
        const int64_t p = p0 + r;
        const int c = c0 + tx;
        double l = nan, phi = nan;
        unsigned cnt = 0u;
        if (p < a.n && c < a.cells) {
            const int64_t cell = a.cell_base + c;
            const int k = c % a.n_obs;
            const int code = a.cell_code[cell];
            const double y = a.cell_obs[cell], f = a.pred[p * a.cells + c];
            l = pw_term(code, y, a.cell_floor[cell], f, s_a[r][k], s_b[r][k], a.nz.scale[k], s_valid[r] != 0, phi);
            if (!a.terms) a.ll[p * a.cells + c] = l;
            if (kCountPit) {      // the replicated count of this particle against the observation
                const int family = (code >> kCellFamilyShift) & 3;
                if ((code & kCellObserved) && family != smc_cnt::kGaussian && s_valid[r] != 0 && fabs(f) < __builtin_huge_val()) {
                    const double yr = smc_draw::count_draw(family, f, s_b[r][k], a.seed, (uint64_t)(a.global_offset + p), smc_draw::kTagPit, (uint64_t)cell);
                    cnt = (1u << 16) | (yr == y ? 1u << 8 : 0u) | (yr < y ? 1u : 0u);      // a NaN draw is neither
                }
            }
        }
        tile[r][tx] = l;
        phis[r][tx] = phi;
        if (kCountPit) cnts[r][tx] = cnt;
    }
    if (!a.terms) return;
    __syncthreads();
    const int64_t stride = pw_stride(a.n);
    for (int r = ty; r < kPwTile; r += 256 / kPwTile) {
        const int c = c0 + r;
        const int64_t p = p0 + tx;
        if (p < stride && c < a.cells) a.terms[(int64_t)c * stride + p] = tile[tx][r];      // p == n: NaN
    }
    if (ty == 0 && c0 + tx < a.cells) {      // the tile's particles in index order
        double sum = 0.0, cnt = 0.0;
        for (int r = 0; r < kPwTile; ++r) {
            const double v = phis[r][tx];
            if (v == v) {
                sum += v;
                cnt += 1.0;
            }
        }
        double *part = a.pit_part + ((int64_t)(c0 + tx) * (int64_t)gridDim.x + blockIdx.x) * 2;
        part[0] = sum;
        part[1] = cnt;
        if (kCountPit) {      // three counts of at most 32 each: the fields cannot carry
            unsigned w = 0u;
            for (int r = 0; r < kPwTile; ++r) w += cnts[r][tx];
            a.pit_cnt[(int64_t)(c0 + tx) * (int64_t)gridDim.x + blockIdx.x] = w;
        }
    }
}

__global__ void __launch_bounds__(256) pw_terms_kernel(const PointwiseArgs a) { pw_terms_body<false>(a); }
__global__ void __launch_bounds__(256) pw_terms_count_kernel(const PointwiseArgs a) { pw_terms_body<true>(a); }

// the fixed tree of pointwise_reduce.h over the block's partials
template <class T, class Join>
__device__ __forceinline__ T pw_block_tree(T v, T *s, Join join) {
    const int tid = threadIdx.x;
    s[tid] = v;
    __syncthreads();
    for (int w = smc_pw::kPwThreads / 2; w > 0; w >>= 1) {
        if (tid < w) s[tid] = join(s[tid], s[tid + w]);
        __syncthreads();
    }
    const T r = s[0];
    __syncthreads();
    return r;
}

__global__ void __launch_bounds__(smc_pw::kPwThreads) pw_cell_kernel(const PointwiseArgs a) {
    __shared__ smc_pw::Pass1 s1[smc_pw::kPwThreads];
    __shared__ smc_pw::Pass2 s2[smc_pw::kPwThreads];
    const int c = blockIdx.x;
    if (c >= a.cells) return;
    const int tid = threadIdx.x;
    const int64_t stride = pw_stride(a.n), n_pairs = stride / 2;
    const double2 *v = reinterpret_cast<const double2 *>(a.terms + (int64_t)c * stride);
    const int64_t cell = a.cell_base + c, ct = a.cells_total;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    smc_pw::Pass1 p1 = smc_pw::pass1_zero();
    for (int64_t i = tid; i < n_pairs; i += smc_pw::kPwThreads) {
        const double2 x = v[i];
        smc_pw::pass1_add(p1, x.x);
        smc_pw::pass1_add(p1, x.y);
    }
    p1 = pw_block_tree(p1, s1, smc_pw::pass1_join);
    if (p1.n == 0.0) {      // no particle has a term here (and none a finite prediction: the PIT counts are 0)
        if (tid == 0) {
            a.out[cell] = 0.0;
            for (int j = 1; j < kPwOutWords; ++j) a.out[(int64_t)j * ct + cell] = nan;
            if (a.pit_cnt)
                for (int j = 0; j < kPwCountWords; ++j) a.out[(int64_t)(kPwOutWords + j) * ct + cell] = 0.0;
        }
        return;
    }
    const double mean = p1.sum / p1.n;
    smc_pw::Pass2 p2 = smc_pw::pass2_zero();
    for (int64_t i = tid; i < n_pairs; i += smc_pw::kPwThreads) {
        const double2 x = v[i];
        smc_pw::pass2_add(p2, x.x, p1.max, mean);
        smc_pw::pass2_add(p2, x.y, p1.max, mean);
    }
    p2 = pw_block_tree(p2, s2, smc_pw::pass2_join);
    // the PIT of a quantified Gaussian value: the tiles' partials (sum of Phi, number of terms) in index order
    const int code = a.cell_code[cell];
    double pit = nan;
    if ((code & kCellObserved) && ((code >> kCellFlagShift) & 3) == 0 && ((code >> kCellFamilyShift) & 3) == 0) {
        const int64_t tiles = pw_tiles(a.n);
        const double2 *part = reinterpret_cast<const double2 *>(a.pit_part) + (int64_t)c * tiles;
        smc_pw::Pass2 q = smc_pw::pass2_zero();
        for (int64_t i = tid; i < tiles; i += smc_pw::kPwThreads) {
            const double2 x = part[i];
            q.sum_exp += x.x;
            q.m2 += x.y;
        }
        q = pw_block_tree(q, s2, smc_pw::pass2_join);
        pit = q.sum_exp / q.m2;      // no term: 0 / 0
    }
    // the PIT counts of a count cell: the tiles' words in the same fixed order; integers below 2^53, exact in any order.
    // Pass1 carries them: n = below, max = equal, sum = n.
    if (a.pit_cnt) {
        const int64_t tiles = pw_tiles(a.n);
        const unsigned *w = a.pit_cnt + (int64_t)c * tiles;
        smc_pw::Pass1 q{0.0, 0.0, 0.0};
        for (int64_t i = tid; i < tiles; i += smc_pw::kPwThreads) {
            const unsigned x = w[i];
            q.n += (double)(x & 0xFFu);
            q.max += (double)((x >> 8) & 0xFFu);
            q.sum += (double)(x >> 16);
        }
        q = pw_block_tree(q, s1, [](const smc_pw::Pass1 &x, const smc_pw::Pass1 &y) { return smc_pw::Pass1{x.n + y.n, x.max + y.max, x.sum + y.sum}; });
        if (tid == 0) {
            a.out[(int64_t)kPwOutWords * ct + cell] = q.n;
            a.out[(int64_t)(kPwOutWords + 1) * ct + cell] = q.max;
            a.out[(int64_t)(kPwOutWords + 2) * ct + cell] = q.sum;
        }
    }
    if (tid == 0) {
        const smc_pw::Stats st = smc_pw::finish(p1, p2);
        a.out[cell] = st.n;
        a.out[ct + cell] = st.max;
        a.out[2 * ct + cell] = st.sum_exp;
        a.out[3 * ct + cell] = st.mean;
        a.out[4 * ct + cell] = st.m2;
        a.out[5 * ct + cell] = pit;
    }
}

size_t pointwise_terms_bytes(int64_t n, int cells) { return (size_t)pw_stride(n) * (size_t)cells * sizeof(double); }
size_t pointwise_pit_bytes(int64_t n, int cells) { return (size_t)pw_tiles(n) * (size_t)cells * 2 * sizeof(double); }
size_t pointwise_pit_count_bytes(int64_t n, int cells) { return (size_t)pw_tiles(n) * (size_t)cells * sizeof(unsigned); }

void launch_pointwise(smc_ctx *c, const PointwiseArgs &a) {
    if (a.n <= 0 || a.cells <= 0) return;
    const int64_t np = a.terms ? pw_stride(a.n) : a.n;
    const dim3 g((unsigned)((np + kPwTile - 1) / kPwTile), (unsigned)((a.cells + kPwTile - 1) / kPwTile));
    if (a.terms && a.pit_cnt)
        hipLaunchKernelGGL(pw_terms_count_kernel, g, dim3(256), 0, c->stream, a);
    else
        hipLaunchKernelGGL(pw_terms_kernel, g, dim3(256), 0, c->stream, a);
    if (a.terms) hipLaunchKernelGGL(pw_cell_kernel, dim3((unsigned)a.cells), dim3(smc_pw::kPwThreads), 0, c->stream, a);
}

}  // namespace smc
