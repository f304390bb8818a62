// predictive_kernels.h -- the summary kernels of smc_user_predict_summary (include/smc_hip.h): per cell (experiment, time,
// output) the mean, the standard deviation and exact order statistics over the particle axis of a block of predictions that
// the prediction kernel has left in device memory.  Implemented in predictive_kernels.hip; called from user_model.hip.
#pragma once
#include <stdint.h>

#include "predictive_select.h"
#include "user_obs_args.h"   // UserNoise

struct smc_ctx;

namespace smc {

// One group of experiments: `pred` is what the prediction kernel wrote for n particles, particle-major
// (pred[p * cells + c], c = (e_local * n_t + i) * n_obs + k); `keys` (pred_summary_key_bytes) is the summary's own buffer.
struct PredSummaryArgs {
    const double *pred;
    unsigned long long *keys;      // cell-major: keys[c * stride + p] = smc_sel::key_of(value), stride = n rounded up to even
    int64_t n;
    int cells;                     // of this group
    int64_t cell_base, cells_total;   // the group's first cell in the whole design, and the design's cell count
    int n_obs;
    // replicated observations (noise != 0): value = pred + sigma_p * scale[k] * z(seed, global_offset + p, cell_base + c)
    int noise;
    // ... of every family (noise = 2 on a model with a count output): family[k] != 0 makes the value of output k the count
    // count_draw.h draws with mean pred and the particle's proportional entry b_k; a Gaussian output keeps the line above
    int family[8];
    const double *theta;           // SoA, theta[c * stride + p]
    int64_t stride;
    int dim, est_sigma;
    double sigma_fixed;
    double scale[8];
    // ... under a noise model (has_noise_model != 0): value = pred + sd z, sd^2 = (a_k s_k)^2 + (b_k pred)^2 with the particle's a_k, b_k
    int has_noise_model;
    UserNoise nz;
    uint64_t seed;
    int64_t global_offset;
    // order statistics
    int n_probs;
    double probs[smc_sel::kMaxProbs];
    // results, one value per cell of the whole design: [mean | sd | n_finite | lower[n_probs] | upper[n_probs]] x cells_total
    double *out;
};

size_t pred_summary_key_bytes(int64_t n, int cells);
// the two launches of a group, on ctx->stream: transpose into keys (adding the noise), then one block per cell; a model
// without count outputs (every family 0) launches the keys kernel that holds no sampler
void launch_pred_summary(smc_ctx *ctx, const PredSummaryArgs &a);

}  // namespace smc
