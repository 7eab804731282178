// Running return-based reward scaling (VecNormalize's reward half) for the MLP engines: the rewards of a rollout are
// divided by the running standard deviation of the per-env discounted return and clipped. State, tables and formulas:
// reward_norm_args.h. Oracle: ops/reward_norm.py (the torch forms of RewardNormalizer).
//
//   reward_norm_scan   once per update, after the rollout: one env per lane walks its T raw rewards in order in fp64,
//                      carries the discounted return across updates and writes one partial row (S1_e, S2_e) of the
//                      returns' deviations about the running mean. No LDS, no atomics, no hand-off between workgroups.
//   (obs_norm_merge)   sums the N partial rows in a fixed order and merges them into the state, D = 1 (obs_norm.hip).
//   reward_norm_apply  in place: r = clamp(r * istd32, +-clip), istd32 read from device memory.
// 16 K elements at the benchmark geometry: the targets are determinism and a short launch. The walk over T is one
// dependent fp64 chain per lane, so what a launch costs is the number of memory round trips the chain waits out: the
// loads of RWN_UNROLL steps go out together, in full and in partial rounds alike (rwn_load), and the next round is
// requested before the current one is consumed.
#include "common.h"
#include "launch_api.h"

namespace aca {

struct RwnRound {
  float r[RWN_UNROLL];
  uint8_t d[RWN_UNROLL];
};

// the rows t0 .. t0 + RWN_UNROLL - 1 of env e, requested in one straight line. FULL: the caller knows all rows exist.
// Otherwise a row past T is read from row T - 1 instead (in bounds, never walked), so a partial round keeps as many
// loads in flight as a full one -- a load under its own `t < T` branch would draw its conversion into the branch and
// wait out a round trip per step. (The clamp stays out of the full rounds: with it they traced 2 us slower per launch.)
template <bool FULL>
__device__ __forceinline__ void rwn_load(RwnRound& b, const float* __restrict__ rew, const uint8_t* __restrict__ don,
                                         int64_t N, int e, int t0, int T) {
#pragma unroll
  for (int u = 0; u < RWN_UNROLL; ++u) {
    const int64_t i = (int64_t)(FULL ? t0 + u : min(t0 + u, T - 1)) * N + e;
    b.r[u] = rew[i];
    b.d[u] = don[i];
  }
  // the requests stay in front of the walk that follows them in program order (the scheduler would otherwise sink
  // them behind it to shorten their live ranges, and the walk would wait out every round trip)
  __builtin_amdgcn_sched_barrier(0);
}

template <bool FULL>
__device__ __forceinline__ void rwn_consume(const RwnRound& b, int t0, int T, double gamma, double mean, double& R,
                                            double& S1, double& S2) {
#pragma clang fp contract(off)
#pragma unroll
  for (int u = 0; u < RWN_UNROLL; ++u) {
    // (the same in every lane; a round is only walked when its first row exists, and saying so keeps that row's
    // loads with the others instead of behind a test of their own)
    if (FULL || u == 0 || t0 + u < T) {
      const double m = R * gamma;
      R = m + (double)b.r[u];
      const double d = R - mean;
      const double q = d * d;
      S1 = S1 + d;
      S2 = S2 + q;
      R = b.d[u] ? 0.0 : R;
    }
  }
  __builtin_amdgcn_sched_barrier(0);
}

// the last rows of an env: `cur` holds the full round at t0 and fewer than RWN_UNROLL rows follow it
__device__ __forceinline__ void rwn_tail(RwnRound& cur, RwnRound& nxt, const RewardNormScanArgs& a, int e, int t0,
                                         double mean, double& R, double& S1, double& S2) {
  const int t1 = t0 + RWN_UNROLL;
  if (t1 < a.T) {
    rwn_load<false>(nxt, a.rewards, a.dones, a.N, e, t1, a.T);
    rwn_consume<true>(cur, t0, a.T, a.gamma, mean, R, S1, S2);
    rwn_consume<false>(nxt, t1, a.T, a.gamma, mean, R, S1, S2);
  } else {
    rwn_consume<true>(cur, t0, a.T, a.gamma, mean, R, S1, S2);
  }
}

// Each branch below issues its loads and walks its rows in one straight line: the wait in front of a step then counts
// only the loads requested after it (a load and its walk on two sides of a join would wait for everything in flight).
__global__ void __launch_bounds__(RWN_THREADS) reward_norm_scan_kernel(RewardNormScanArgs a) {
  const int e = blockIdx.x * RWN_THREADS + threadIdx.x;
  if (e >= a.N) return;
  const int T = a.T;
  const double mean = a.state[1];
  double R = a.ret[e], S1 = 0.0, S2 = 0.0;
  RwnRound A, B;
  if (T < RWN_UNROLL) {
    rwn_load<false>(A, a.rewards, a.dones, a.N, e, 0, T);
    rwn_consume<false>(A, 0, T, a.gamma, mean, R, S1, S2);
  } else {
    rwn_load<true>(A, a.rewards, a.dones, a.N, e, 0, T);
    for (int t0 = 0;;) {
      // the next round is requested, then this one walked: the chain runs under the next round's memory round trip
      if (t0 + 2 * RWN_UNROLL > T) {
        rwn_tail(A, B, a, e, t0, mean, R, S1, S2);
        break;
      }
      rwn_load<true>(B, a.rewards, a.dones, a.N, e, t0 + RWN_UNROLL, T);
      rwn_consume<true>(A, t0, T, a.gamma, mean, R, S1, S2);
      t0 += RWN_UNROLL;
      if (t0 + 2 * RWN_UNROLL > T) {
        rwn_tail(B, A, a, e, t0, mean, R, S1, S2);
        break;
      }
      rwn_load<true>(A, a.rewards, a.dones, a.N, e, t0 + RWN_UNROLL, T);
      rwn_consume<true>(B, t0, T, a.gamma, mean, R, S1, S2);
      t0 += RWN_UNROLL;
    }
  }
  a.ret[e] = R;
  *reinterpret_cast<double2*>(a.part + 2 * (int64_t)e) = make_double2(S1, S2);
}

// a multiply feeding a clamp: nothing to contract, so this rounds like torch's mul_ + clamp_
__device__ __forceinline__ float rwn_apply(float r, float istd, float clip) {
  return fminf(fmaxf(r * istd, -clip), clip);
}

constexpr int RWN_APPLY_THREADS = 256;
constexpr int RWN_APPLY_MAXGRID = 2048;

// VEC: the base is 16-byte aligned -- float4 accesses over the first n / 4 * 4 elements, the rest one by one
template <bool VEC>
__global__ void __launch_bounds__(RWN_APPLY_THREADS) reward_norm_apply_kernel(RewardNormApplyArgs a) {
  const float istd = a.tables[1];
  const float clip = a.clip;
  const int64_t gid = (int64_t)blockIdx.x * RWN_APPLY_THREADS + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * RWN_APPLY_THREADS;
  const int64_t n4 = VEC ? a.n / 4 : 0;
  float4* p4 = reinterpret_cast<float4*>(a.rewards);
  for (int64_t i = gid; i < n4; i += stride) {
    float4 v = p4[i];
    v.x = rwn_apply(v.x, istd, clip);
    v.y = rwn_apply(v.y, istd, clip);
    v.z = rwn_apply(v.z, istd, clip);
    v.w = rwn_apply(v.w, istd, clip);
    p4[i] = v;
  }
  for (int64_t i = 4 * n4 + gid; i < a.n; i += stride) a.rewards[i] = rwn_apply(a.rewards[i], istd, clip);
}

}  // namespace aca

extern "C" int aca_reward_norm_unroll(void) { return aca::RWN_UNROLL; }

extern "C" hipError_t aca_reward_norm_scan(const aca::RewardNormScanArgs* a, hipStream_t stream) {
  if (!a->rewards || !a->dones || !a->ret || !a->state || !a->part || a->T < 1 || a->N < 1) return hipErrorInvalidValue;
  // contiguous [T][N]: the stride of a dimension of size 1 addresses nothing and may be anything
  const bool cols = a->N == 1 || (a->r_stride_n == 1 && a->d_stride_n == 1);
  const bool rows = a->T == 1 || (a->r_stride_t == a->N && a->d_stride_t == a->N);
  if (!cols || !rows || a->ret_len != a->N || reinterpret_cast<uintptr_t>(a->part) % 16 != 0)
    return hipErrorInvalidValue;
  const int grid = (a->N + aca::RWN_THREADS - 1) / aca::RWN_THREADS;
  aca::reward_norm_scan_kernel<<<grid, aca::RWN_THREADS, 0, stream>>>(*a);
  return hipGetLastError();
}

extern "C" hipError_t aca_reward_norm_apply(const aca::RewardNormApplyArgs* a, hipStream_t stream) {
  if (!a->rewards || !a->tables || a->n < 1 || !(a->clip > 0.0f)) return hipErrorInvalidValue;
  const bool vec = reinterpret_cast<uintptr_t>(a->rewards) % 16 == 0 && a->n >= 4;
  const int64_t items = vec ? a->n / 4 + 3 : a->n;   // (a tail of at most 3 elements rides on the first threads)
  int64_t grid = (items + aca::RWN_APPLY_THREADS - 1) / aca::RWN_APPLY_THREADS;
  if (grid > aca::RWN_APPLY_MAXGRID) grid = aca::RWN_APPLY_MAXGRID;
  if (vec) aca::reward_norm_apply_kernel<true><<<(int)grid, aca::RWN_APPLY_THREADS, 0, stream>>>(*a);
  else aca::reward_norm_apply_kernel<false><<<(int)grid, aca::RWN_APPLY_THREADS, 0, stream>>>(*a);
  return hipGetLastError();
}
