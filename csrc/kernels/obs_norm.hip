// Running observation normalisation (VecNormalize-style) for the MLP engines: per-feature mean / variance of the raw
// observations, applied in front of both towers as clip((x - mean) / sqrt(var + eps), +-c). State, tables and the
// apply formula: obs_norm_args.h. Oracle: ops/obs_norm.py (ObsNormalizer.apply and the torch fallbacks).
//
//   obs_norm_prepare  once per update, after the rollout: writes the normalised plane the learner reads (PPO would
//                     otherwise redo it in every epoch) and fp64 partial sums of the rollout's rows about the running
//                     mean -- one row of partials per workgroup, no floating-point atomics.
//   obs_norm_merge    one workgroup: stage 0 sums the partial rows in a fixed order into the additive batch vector
//                     [S1, S2, nb] (data parallelism all-reduces it), stage 1 merges it into the state (Chan et al.)
//                     and rewrites the fp32 tables.
// Every reduction runs in a fixed order: the update stays bitwise reproducible. ~1 MB of data at the benchmark geometry;
// the targets are determinism and a short launch, not bandwidth (row reads are coalesced, nothing more).
#include "common.h"
#include "launch_api.h"

namespace aca {

constexpr int OBSN_THREADS = 256;
constexpr int OBSN_MAXD = 256;   // = MLP_MAXW (mlp.hip): the widest observation the MLP engine takes

// subtract, multiply, clamp: a subtract feeding a multiply cannot contract into an fma, so this rounds like torch
__device__ __forceinline__ float obs_norm_apply(float x, float mean, float istd, float clip) {
  return fminf(fmaxf((x - mean) * istd, -clip), clip);
}

// Thread (g, c) = (tid / D, tid % D) of a workgroup walks rows g, g + G, ... of the workgroup's OBSN_ROWS rows (G =
// 256 / D groups: consecutive threads read consecutive columns of a row), writes the plane and sums its rows' deviations;
// the G group sums of a column meet in LDS and thread c adds them in group order.
__global__ void __launch_bounds__(OBSN_THREADS) obs_norm_prepare_kernel(ObsNormPrepArgs a) {
  __shared__ double s1[OBSN_THREADS], s2[OBSN_THREADS];
  const int tid = threadIdx.x;
  const int D = a.D;
  const int G = OBSN_THREADS / D;
  const int g = tid / D, c = tid - g * D;
  const int row0 = blockIdx.x * OBSN_ROWS;
  const int rend = min(row0 + OBSN_ROWS, a.R);
  double d1 = 0.0, d2 = 0.0;
  if (g < G) {
    const float m32 = a.tables[c], is32 = a.tables[D + c];
    const double mean = a.state[1 + c];
    for (int r = row0 + g; r < rend; r += G) {
      const float x = a.obs[(int64_t)r * a.ld_obs + c];
      a.plane[(int64_t)r * D + c] = obs_norm_apply(x, m32, is32, a.clip);
      if (r < a.R_stat) {
        const double d = (double)x - mean;
        d1 += d;
        d2 += d * d;
      }
    }
  }
  s1[tid] = d1;
  s2[tid] = d2;
  __syncthreads();
  if (tid < D) {
    double t1 = 0.0, t2 = 0.0;
    for (int j = 0; j < G; ++j) {
      t1 += s1[j * D + tid];
      t2 += s2[j * D + tid];
    }
    double* p = a.part + (int64_t)blockIdx.x * 2 * D;
    p[tid] = t1;
    p[D + tid] = t2;
  }
}

// the merge of obs_norm_args.h, one column; no contraction, so the torch fallback's fp64 ops round alike
__device__ __forceinline__ void obs_norm_merge_col(double count, double nb, double S1, double S2, double& mean,
                                                   double& m2) {
#pragma clang fp contract(off)
  const double tot = count + nb;
  const double delta = S1 / nb;
  mean = mean + S1 / tot;
  m2 = m2 + ((S2 - S1 * S1 / nb) + delta * delta * count * nb / tot);
}

__device__ __forceinline__ float obs_norm_istd(double m2, double count, double eps) {
#pragma clang fp contract(off)
  return (float)(1.0 / sqrt(m2 / count + eps));
}

// column j of the partial rows [w0, w1), added in index order; the loads go out eight at a time (one load per add would
// wait out a memory round trip per row: 62 us for the 257 rows of the benchmark geometry, measured)
__device__ __forceinline__ double obs_norm_sum_rows(const double* __restrict__ part, int W, int j, int w0, int w1) {
  double s = 0.0;
  int w = w0;
  for (; w + 8 <= w1; w += 8) {
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = part[(int64_t)(w + u) * W + j];
#pragma unroll
    for (int u = 0; u < 8; ++u) s += v[u];
  }
  for (; w < w1; ++w) s += part[(int64_t)w * W + j];
  return s;
}

__global__ void __launch_bounds__(OBSN_THREADS) obs_norm_merge_kernel(ObsNormMergeArgs a) {
  __shared__ double s_g[OBSN_THREADS];
  const int tid = threadIdx.x;
  const int D = a.D;
  if (a.stage != 1) {
    // a fixed two-level order: G = 256 / 2D thread groups each add one contiguous chunk of the rows in index order,
    // then thread j adds the G chunk sums in chunk order (D > 128: one level)
    const int W = 2 * D;
    const int G = OBSN_THREADS / W;
    if (G >= 2) {
      const int g = tid / W, j = tid - g * W;
      const int chunk = (a.nparts + G - 1) / G;
      s_g[tid] = g < G ? obs_norm_sum_rows(a.part, W, j, min(g * chunk, a.nparts), min((g + 1) * chunk, a.nparts)) : 0.0;
      __syncthreads();
      if (tid < W) {
        double s = 0.0;
        for (int k = 0; k < G; ++k) s += s_g[k * W + tid];
        a.batch[tid] = s;
      }
    } else {
      for (int j = tid; j < W; j += OBSN_THREADS) a.batch[j] = obs_norm_sum_rows(a.part, W, j, 0, a.nparts);
    }
    if (tid == 0) a.batch[2 * D] = a.nb;
    if (a.stage == 0) return;
    __syncthreads();   // (global writes of this workgroup, read back below by other threads)
  }
  const double count = a.state[0];
  const double nb = a.batch[2 * D];
  __syncthreads();     // every thread holds the old count before thread 0 rewrites it
  if (nb <= 0.0) return;
  if (tid < D) {
    double mean = a.state[1 + tid], m2 = a.state[1 + D + tid];
    obs_norm_merge_col(count, nb, a.batch[tid], a.batch[D + tid], mean, m2);
    a.state[1 + tid] = mean;
    a.state[1 + D + tid] = m2;
    a.tables[tid] = (float)mean;
    a.tables[D + tid] = obs_norm_istd(m2, count + nb, a.eps);
  }
  if (tid == 0) a.state[0] = count + nb;
}

}  // namespace aca

extern "C" int aca_obs_norm_parts(int R) { return R <= 0 ? 0 : (R + aca::OBSN_ROWS - 1) / aca::OBSN_ROWS; }

extern "C" hipError_t aca_obs_norm_prepare(const aca::ObsNormPrepArgs* a, hipStream_t stream) {
  if (a->R <= 0) return hipSuccess;
  if (!a->obs || !a->plane || !a->tables || !a->state || !a->part || a->D < 1 || a->D > aca::OBSN_MAXD ||
      a->R_stat < 0 || a->R_stat > a->R || a->ld_obs < a->D)
    return hipErrorInvalidValue;
  aca::obs_norm_prepare_kernel<<<aca_obs_norm_parts(a->R), aca::OBSN_THREADS, 0, stream>>>(*a);
  return hipGetLastError();
}

extern "C" hipError_t aca_obs_norm_merge(const aca::ObsNormMergeArgs* a, hipStream_t stream) {
  if (!a->batch || a->D < 1 || a->D > aca::OBSN_MAXD || a->stage < 0 || a->stage > 2) return hipErrorInvalidValue;
  if (a->stage != 1 && (a->nparts < 0 || (a->nparts > 0 && !a->part))) return hipErrorInvalidValue;
  if (a->stage != 0 && (!a->state || !a->tables)) return hipErrorInvalidValue;
  aca::obs_norm_merge_kernel<<<1, aca::OBSN_THREADS, 0, stream>>>(*a);
  return hipGetLastError();
}
