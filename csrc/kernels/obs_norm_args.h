// Argument blocks of the running observation normaliser (obs_norm.hip), shared with csrc/bindings.cpp: plain C types
// only, so both hipcc and g++ compile this header. The binding fills them by field name.
//
// State (fp64, device): state[0] = count, state[1 .. D] = mean, state[1 + D .. 2 D] = m2 (sum of squared deviations).
// Tables (fp32, device): tables[0 .. D) = mean32 = (float)mean, tables[D .. 2 D) = istd32 =
// (float)(1 / sqrt(m2 / count + eps)); the identity (0, 1) while count == 0.
// Apply: y = fminf(fmaxf((x - mean32[c]) * istd32[c], -clip), clip), exactly subtract, multiply, clamp.
#pragma once
#include <stdint.h>

namespace aca {

constexpr int OBSN_ROWS = 64;   // observation rows per obs_norm_prepare workgroup

// obs_norm_prepare: the normalised plane of R rows + per-workgroup fp64 partial sums of the first R_stat rows about the
// running mean: part[w][c] = sum (x - mean[c]), part[w][D + c] = sum (x - mean[c])^2 over workgroup w's rows < R_stat
// (fixed order; every workgroup writes its row, zeros included)
struct ObsNormPrepArgs {
  const float* obs; int64_t ld_obs;   // [R][D], row stride in floats
  float* plane;                       // [R][D] contiguous
  const float* tables;                // [2][D]
  const double* state;                // [1 + 2 D]
  double* part;                       // [ceil(R / OBSN_ROWS)][2 D]
  int R, D, R_stat;
  float clip;
};

// obs_norm_merge (one workgroup). stage 0: batch[0 .. 2 D) = the partial rows summed in a fixed order (contiguous chunks
// of rows in index order, then the chunk sums in chunk order), batch[2 D] = nb;
// stage 1: Chan merge of batch into the state, tables rewritten; stage 2: both in one launch.
struct ObsNormMergeArgs {
  const double* part; int nparts;
  double* batch;                      // [2 D + 1]: S1, S2, nb (additive: data parallelism all-reduces it)
  double nb;                          // rows behind part (stage 0 / 2)
  double* state;                      // [1 + 2 D]
  float* tables;                      // [2][D]
  int D;
  int stage;
  double eps;
};

}  // namespace aca
