// Argument blocks of the running reward scaler (reward_norm.hip), shared with csrc/bindings.cpp: plain C types only, so
// both hipcc and g++ compile this header. The binding fills them by field name.
//
// State and tables are the observation normaliser's with D = 1 (obs_norm_args.h): state[0] = count, state[1] = mean,
// state[2] = m2 of every discounted return seen (fp64); tables[0] = mean32, tables[1] = istd32 =
// (float)(1 / sqrt(m2 / count + eps)), the identity (0, 1) while count == 0. obs_norm_merge folds the partial rows below
// into them; there is no second merge kernel.
// Scan, per env e, t = 0 .. T-1 in order, fp64, no contraction: R = R * gamma + r[t][e] (multiply, then add);
// d = R - mean; S1_e += d; S2_e += d * d; then R = 0 where done[t][e].
// Apply, fp32, in place: r = fminf(fmaxf(r * istd32, -clip), clip). No mean is subtracted.
#pragma once
#include <stdint.h>

namespace aca {

constexpr int RWN_THREADS = 64;   // one wave per workgroup, one env per lane
constexpr int RWN_UNROLL = 16;    // time steps whose loads one round of the scan issues together

// reward_norm_scan: strides are in elements; the launcher takes only contiguous rewards / dones [T][N], strides (N, 1)
// (the stride of a dimension of size 1 is not looked at)
struct RewardNormScanArgs {
  const float* rewards; int64_t r_stride_t, r_stride_n;     // [T][N], raw
  const uint8_t* dones; int64_t d_stride_t, d_stride_n;     // [T][N], 1 = episode boundary (time-limit cuts included)
  double* ret; int64_t ret_len;                             // [N] running discounted return, read and written back
  const double* state;                                      // [3]: count, mean, m2 (mean is read)
  double* part;                                             // [N][2]: (S1_e, S2_e), the merge's partial rows for D = 1
  int T, N;
  double gamma;
};

struct RewardNormApplyArgs {
  float* rewards; int64_t n;          // T N contiguous floats, scaled in place
  const float* tables;                // [2]: mean32, istd32 (istd32 is read)
  float clip;
};

}  // namespace aca
