// Evaluation records from a stored rollout (the native per-step evaluation path, algos/evaluator.py): the reward and
// done columns [L][N] of an evaluation become the first E episode returns and lengths of every env. Semantics and
// argument block: eval_scan_args.h. Oracle (and CPU path): ops/evaluation.py eval_scan_ref.
//
// One env per lane, so the loads of a step are coalesced across envs. The walk over L is one dependent fp32 chain per
// lane; what a launch costs is the number of memory round trips that chain waits out, so the loads of EVS_UNROLL steps
// go out together before the first add (as reward_norm_scan does), in full and in partial rounds alike. The adds run in
// step order: bit-identical to the bank's own ep_ret arithmetic and to the oracle. No LDS, no atomics.
#include "common.h"
#include "launch_api.h"

namespace aca {

__global__ void __launch_bounds__(EVS_THREADS) eval_scan_kernel(EvalScanArgs a) {
  const int e = blockIdx.x * EVS_THREADS + threadIdx.x;
  if (e >= a.N) return;
  const int L = a.L, E = a.E;
  const int64_t N = a.N;
  float ret = 0.f;
  int len = 0, cnt = 0;
  for (int t0 = 0; t0 < L; t0 += EVS_UNROLL) {
    float r[EVS_UNROLL];
    uint8_t d[EVS_UNROLL];
    // a row past L is read from row L - 1 instead (in bounds, never walked): a partial round keeps as many loads in
    // flight as a full one
#pragma unroll
    for (int u = 0; u < EVS_UNROLL; ++u) {
      const int64_t i = (int64_t)min(t0 + u, L - 1) * N + e;
      r[u] = a.reward[i];
      d[u] = a.done[i];
    }
    // the requests stay in front of the walk (the scheduler would otherwise sink them behind it)
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < EVS_UNROLL; ++u) {
      if (t0 + u < L) {
        ret = ret + r[u];
        len = len + 1;
        if (d[u]) {   // rare: once per episode
          if (cnt < E) {
            a.ep_ret[(int64_t)e * E + cnt] = ret;
            a.ep_len[(int64_t)e * E + cnt] = len;
            ++cnt;
          }
          ret = 0.f;
          len = 0;
        }
      }
    }
  }
  a.cnt[e] = cnt;
}

}  // namespace aca

extern "C" int aca_eval_scan_unroll(void) { return aca::EVS_UNROLL; }

extern "C" hipError_t aca_eval_scan(const aca::EvalScanArgs* a, hipStream_t stream) {
  if (!a->reward || !a->done || !a->ep_ret || !a->ep_len || !a->cnt || a->L < 1 || a->N < 1 || a->E < 1)
    return hipErrorInvalidValue;
  const int grid = (a->N + aca::EVS_THREADS - 1) / aca::EVS_THREADS;
  aca::eval_scan_kernel<<<grid, aca::EVS_THREADS, 0, stream>>>(*a);
  return hipGetLastError();
}
