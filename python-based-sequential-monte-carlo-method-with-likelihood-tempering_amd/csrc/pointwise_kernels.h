// pointwise_kernels.h -- the kernels of smc_user_pointwise and smc_user_pointwise_summary (include/smc_hip.h):
// the log-likelihood term of every (particle, cell) from a block of predictions the prediction kernel has left in device memory,
// and per cell (experiment, time, output) the raw statistics of its terms over the particle axis plus the PIT.  Implemented in
// pointwise_kernels.hip; called from user_model.hip.
#pragma once
#include <stdint.h>

#include "user_obs_args.h"   // UserNoise

struct smc_ctx;

namespace smc {

// what a cell is, packed by the host once per model (user_model.hip: build_cell_tables): bit 0 observed, bits 1-2 the censor
// flag c_k of user_censor.h (0 quantified, 1 left, 2 right), bits 3-4 the family of user_count.h (0 Gaussian, 1 Poisson, 2
// negative binomial)
constexpr int kCellObserved = 1, kCellFlagShift = 1, kCellFamilyShift = 3;
constexpr int kPwTile = 32;          // particles (and cells) per tile of the terms kernel
constexpr int kPwOutWords = 6;       // results per cell: n, max, sum_exp, mean, m2, pit
constexpr int kPwCountWords = 3;     // ... and with the PIT of count cells (pit_cnt != nullptr): pit_below, pit_equal, pit_n

// One group of experiments: `pred` as PredSummaryArgs' (pred[p * cells + c]).
struct PointwiseArgs {
    const double *pred;
    double *terms;                 // cell-major: terms[c * stride + p], stride = n rounded up to even (the odd one out holds NaN);
                                   // nullptr: the terms go particle-major to ll (smc_user_pointwise)
    double *ll;                    // ll[p * cells + c]
    double *pit_part;              // [cells][tiles][2]: per tile of kPwTile particles the sum of Phi and the number of its terms
    int64_t n;
    int cells;                     // of this group
    int64_t cell_base, cells_total;
    int n_obs;
    const double *theta;           // SoA, theta[j * stride + p]
    int64_t stride;
    // the noise of every output as a noise model: the sigma rule is add_index = dim - 1 (or fixed), no proportional part
    UserNoise nz;
    int family[kUserMaxObs];       // per output (user_count.h): a negative-binomial output needs b_k > 0
    // the tables, one entry per cell of the whole design: the value, what the cell is, count_floor(y) of a Poisson value
    const double *cell_obs;
    const int *cell_code;
    const double *cell_floor;
    double *out;                   // [n | max | sum_exp | mean | m2 | pit] x cells_total
    // The PIT of count cells (smc_user_pointwise_summary_opt with count_pit; nullptr: not formed, and the terms kernel without the
    // sampler runs): per observed count cell, over the particles with a finite prediction and valid noise parameters, how many
    // replicated counts (count_draw.h, tag 0x504954, seed, global_offset + p, the global cell) lie below the observation and how
    // many equal it.  pit_cnt [cells][tiles]: one word per tile of kPwTile particles, below | equal << 8 | n << 16 (each <= 32);
    // out then has kPwCountWords more rows, [pit_below | pit_equal | pit_n], integers held in doubles.
    unsigned *pit_cnt;
    uint64_t seed;
    int64_t global_offset;
};

size_t pointwise_terms_bytes(int64_t n, int cells);
size_t pointwise_pit_bytes(int64_t n, int cells);
size_t pointwise_pit_count_bytes(int64_t n, int cells);
// the terms of a group on ctx->stream; with a.terms also the per-cell reduction
void launch_pointwise(smc_ctx *ctx, const PointwiseArgs &a);

}  // namespace smc
