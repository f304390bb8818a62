// predictive_kernels.hip -- posterior predictive summaries on the device (include/smc_hip.h: smc_user_predict_summary;
// DESIGN.md 4.8).  The prediction kernel writes particle-major (one particle's cells are contiguous), an order statistic is
// taken per cell over the particles.  Two kernels per group of experiments:
//   pred_keys_kernel    a tiled transpose through LDS into cell-major order; on the way the value gets its noise term (if asked
//                       for) and becomes its order-preserving 64-bit key (predictive_select.h).  8 B read + 8 B written per value.
//   pred_select_kernel  one block per cell: an exact most-significant-digit radix select of every wanted rank at once, 8 passes of
//                       8 bits over the cell's keys (contiguous, coalesced), with the count and the sum in pass 0 and the squared
//                       deviations in pass 1.  8 x 8 B read per value, nothing written but the cell's results.
// All sums run in an order fixed by the block size, so a repeated call returns the same bits.
#include <hip/hip_runtime.h>

#include "count_draw.h"
#include "philox.h"
#include "predictive_kernels.h"
#include "smc_internal.h"

namespace smc {

using smc_sel::u64;

constexpr int kTile = 32;
constexpr int kSelThreads = 512;
constexpr int kSelBatch = 2;          // 16-byte loads (two keys each) a thread issues before it counts them: more bytes in flight
// a cell's keys start on a 16-byte boundary: the stride is n rounded up to even, the odd one out holds kNanKey
__host__ __device__ inline int64_t key_stride(int64_t n) { return (n + 1) & ~(int64_t)1; }

// kCounts: some output of the model is a count (PredSummaryArgs::family) - the instantiation that holds the sampler; without,
// the kernel is what it was before there was one
template <bool kCounts>
__global__ void __launch_bounds__(256) pred_keys_kernel(const PredSummaryArgs a) {
    __shared__ u64 tile[kTile][kTile + 1];
    const int tx = threadIdx.x % kTile, ty = threadIdx.x / kTile;      // 32 x 8
    const int64_t p0 = (int64_t)blockIdx.x * kTile;
    const int c0 = (int)blockIdx.y * kTile;
    for (int r = ty; r < kTile; r += 256 / kTile) {
        const int64_t p = p0 + r;
        const int c = c0 + tx;
        u64 key = smc_sel::kNanKey;
        if (p < a.n && c < a.cells) {
            double v = a.pred[p * a.cells + c];
            const int fam = kCounts ? a.family[c % a.n_obs] : 0;
            if (kCounts && a.noise && fam != 0) {      // a replicated count: mean v, the particle's b_k (count_draw.h)
                const int k = c % a.n_obs;
                const double bk = !a.nz.prop ? 0.0 : (a.nz.prop_index[k] >= 0 ? a.theta[(int64_t)a.nz.prop_index[k] * a.stride + p] : a.nz.prop_fixed[k]);
                v = smc_draw::count_draw(fam, v, bk, a.seed, (uint64_t)(a.global_offset + p), smc_draw::kTagPredict, (uint64_t)(a.cell_base + c));
            } else if (a.noise) {
                const int64_t cell = a.cell_base + c;
                const double sigma = a.est_sigma ? a.theta[(int64_t)(a.dim - 1) * a.stride + p] : a.sigma_fixed;
                const u32x4 q = philox_block(a.seed, (uint64_t)(a.global_offset + p), (0x505245ull << 32) | (uint64_t)cell, 0);
                const double u1 = 1.0 - u01_from(q.x, q.y), u2 = u01_from(q.z, q.w);
                const double z = sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
                if (a.has_noise_model) {
                    const int k = c % a.n_obs;
                    const double ak = a.nz.add_index[k] >= 0 ? a.theta[(int64_t)a.nz.add_index[k] * a.stride + p] : a.nz.add_fixed[k];
                    const double bk = !a.nz.prop ? 0.0 : (a.nz.prop_index[k] >= 0 ? a.theta[(int64_t)a.nz.prop_index[k] * a.stride + p] : a.nz.prop_fixed[k]);
                    const double as = ak * a.nz.scale[k], bf = bk * v;
                    v = v + sqrt(as * as + bf * bf) * z;
                } else {
                    v = v + (sigma * a.scale[c % a.n_obs]) * z;
                }
            }
            key = smc_sel::key_of(v);
        }
        tile[r][tx] = key;
    }
    __syncthreads();
    for (int r = ty; r < kTile; r += 256 / kTile) {
        const int c = c0 + r;
        const int64_t p = p0 + tx;
        if (p < key_stride(a.n) && c < a.cells) a.keys[(int64_t)c * key_stride(a.n) + p] = tile[tx][r];      // p == n: kNanKey
    }
}

// sum over the block in a fixed order
__device__ __forceinline__ double block_sum(double v, double *s) {
    s[threadIdx.x] = v;
    __syncthreads();
    for (int w = kSelThreads / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) s[threadIdx.x] += s[threadIdx.x + w];
        __syncthreads();
    }
    const double r = s[0];
    __syncthreads();
    return r;
}

// One count per lane into an LDS histogram (bin < 0: none).  The keys of a cell are close to each other, so in the leading
// digits a whole wave meets in one bin: the lanes of the first lane's bin are counted with one ballot and ONE atomic, only the
// others add for themselves.  Every lane of the wave must call.
__device__ __forceinline__ void hist_add(unsigned *h, int bin) {
    const bool act = bin >= 0;
    const u64 mask = __ballot(act);
    if (mask == 0) return;
    const int leader = __ffsll((long long)mask) - 1;
    const int b = __shfl(bin, leader);
    const u64 same = __ballot(act && bin == b);
    if ((int)(threadIdx.x & 63) == leader) atomicAdd(&h[b], (unsigned)__popcll(same));
    if (act && bin != b) atomicAdd(&h[bin], 1u);
}

__global__ void __launch_bounds__(kSelThreads) pred_select_kernel(const PredSummaryArgs a) {
    __shared__ unsigned hist[smc_sel::kMaxRanks * smc_sel::kSelBins];
    __shared__ double red[kSelThreads];
    __shared__ u64 prefix[smc_sel::kMaxRanks], next_prefix[smc_sel::kMaxRanks], rem[smc_sel::kMaxRanks];
    __shared__ int slot[smc_sel::kMaxRanks];
    __shared__ int n_prefix;
    const int c = blockIdx.x;
    if (c >= a.cells) return;
    const int tid = threadIdx.x;
    const ulonglong2 *keys = reinterpret_cast<const ulonglong2 *>(a.keys + (int64_t)c * key_stride(a.n));
    const int64_t n_pairs = key_stride(a.n) / 2;
    const int n_ranks = 2 * a.n_probs;
    const int64_t cell = a.cell_base + c, ct = a.cells_total;
    double *o_mean = a.out + cell, *o_sd = a.out + ct + cell, *o_m = a.out + 2 * ct + cell;
    double *o_lower = a.out + 3 * ct + cell, *o_upper = a.out + (3 + (int64_t)a.n_probs) * ct + cell;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    if (tid == 0) {
        n_prefix = 1;
        prefix[0] = 0;
    }
    if (tid < n_ranks) slot[tid] = 0;
    __syncthreads();
    const int64_t step = (int64_t)kSelThreads * kSelBatch;
    const int64_t n_round = (n_pairs + step - 1) / step * step;  // every lane takes part in every ballot
    double mean = 0.0, m = 0.0;
    for (int pass = 0; pass < smc_sel::kSelPasses; ++pass) {
        const int np = n_prefix;
        for (int i = tid; i < np * smc_sel::kSelBins; i += kSelThreads) hist[i] = 0;
        __syncthreads();
        double acc = 0.0, cnt = 0.0;
        for (int64_t i0 = tid; i0 < n_round; i0 += step) {
            u64 k[2 * kSelBatch];
#pragma unroll
            for (int j = 0; j < kSelBatch; ++j) {
                const int64_t i = i0 + (int64_t)j * kSelThreads;
                const ulonglong2 v = i < n_pairs ? keys[i] : make_ulonglong2(smc_sel::kNanKey, smc_sel::kNanKey);
                k[2 * j] = v.x;
                k[2 * j + 1] = v.y;
            }
#pragma unroll
            for (int j = 0; j < 2 * kSelBatch; ++j) {
                const bool act = k[j] != smc_sel::kNanKey;
                int bin = -1;
                if (act) {
                    if (pass == 0) {
                        cnt += 1.0;
                        acc += smc_sel::value_of(k[j]);
                    } else if (pass == 1) {
                        const double d = smc_sel::value_of(k[j]) - mean;
                        acc += d * d;
                    }
                    const u64 pre = smc_sel::prefix_of(k[j], pass);
                    for (int s = 0; s < np; ++s)
                        if (prefix[s] == pre) bin = s * smc_sel::kSelBins + (int)smc_sel::digit_of(k[j], pass);
                }
                hist_add(hist, bin);
            }
        }
        __syncthreads();
        if (pass == 0) {
            m = block_sum(cnt, red);
            const double sum = block_sum(acc, red);
            if (m == 0.0) {       // nobody reached this cell
                if (tid == 0) {
                    *o_mean = nan;
                    *o_sd = nan;
                    *o_m = 0.0;
                }
                if (tid < a.n_probs) o_lower[(int64_t)tid * ct] = o_upper[(int64_t)tid * ct] = nan;
                return;
            }
            mean = sum / m;
            if (tid < n_ranks) {
                long long lo, hi;
                double frac;
                smc_sel::quantile_ranks((long long)m, a.probs[tid >> 1], &lo, &hi, &frac);
                rem[tid] = (u64)((tid & 1) ? hi : lo);
            }
            if (tid == 0) {
                *o_mean = mean;
                *o_m = m;
            }
        } else if (pass == 1) {
            const double ss = block_sum(acc, red);
            if (tid == 0) *o_sd = sqrt(ss / m);
        }
        if (tid < n_ranks) {
            const int s = slot[tid];
            u64 r = rem[tid];
            const unsigned d = smc_sel::select_step(hist + s * smc_sel::kSelBins, &r);
            rem[tid] = r;
            next_prefix[tid] = (prefix[s] << smc_sel::kSelBits) | d;
        }
        __syncthreads();
        if (tid == 0) {      // the distinct prefixes of the next pass
            int nd = 0;
            for (int r = 0; r < n_ranks; ++r) {
                int j = 0;
                while (j < nd && prefix[j] != next_prefix[r]) ++j;
                if (j == nd) prefix[nd++] = next_prefix[r];
                slot[r] = j;
            }
            n_prefix = nd;
        }
        __syncthreads();
    }
    // after the last pass a prefix is the whole key
    if (tid < n_ranks) {
        const double v = smc_sel::value_of(prefix[slot[tid]]);
        ((tid & 1) ? o_upper : o_lower)[(int64_t)(tid >> 1) * ct] = v;
    }
}

size_t pred_summary_key_bytes(int64_t n, int cells) { return (size_t)key_stride(n) * (size_t)cells * sizeof(u64); }

void launch_pred_summary(smc_ctx *c, const PredSummaryArgs &a) {
    if (a.n <= 0 || a.cells <= 0) return;
    const dim3 g((unsigned)((key_stride(a.n) + kTile - 1) / kTile), (unsigned)((a.cells + kTile - 1) / kTile));
    bool counts = false;
    for (int k = 0; k < a.n_obs; ++k) counts = counts || a.family[k] != 0;
    if (counts)
        hipLaunchKernelGGL(pred_keys_kernel<true>, g, dim3(256), 0, c->stream, a);
    else
        hipLaunchKernelGGL(pred_keys_kernel<false>, g, dim3(256), 0, c->stream, a);
    hipLaunchKernelGGL(pred_select_kernel, dim3((unsigned)a.cells), dim3(kSelThreads), 0, c->stream, a);
}

}  // namespace smc
