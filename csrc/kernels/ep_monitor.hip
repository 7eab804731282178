// Rolling window over the last K finished training episodes (TrainConfig.ep_window), kept and summarised on the device
// in a fixed order. State, semantics and argument blocks: ep_monitor_args.h. Oracle (and CPU path): ops/ep_monitor.py.
//
//   ep_monitor_scan    once per update, after the rollout wrote the raw rewards: one env per lane walks its T rewards
//                      in step order from the carried (cur_ret, cur_len) with plain fp32 adds -- the bank's own ep_ret
//                      arithmetic -- and at a done stores the finished episode's (return, length) at that cell of a
//                      dense [T][N] scratch; the carry is stored back. The loads of EPM_UNROLL steps go out together
//                      before the first add, in full and in partial rounds alike (as eval_scan does). No LDS, no atomics.
//   ep_monitor_commit  ONE workgroup: compacts the done column in the flattened (t, n) order -- per-thread contiguous
//                      chunks, counts of non-zero bytes in 16-byte loads, an exclusive scan of the counts (integers
//                      only) -- writes episode number r of this update to ring[(total + r) mod K], skipping the first
//                      C - K when the update finished C > K episodes, and after a barrier reduces the summary over the
//                      filled slots in a fixed order (per-thread strided partials, a shuffle tree per wave, the waves
//                      in order), in fp64. One workgroup because a hand-off between workgroups costs more than this
//                      whole launch; nothing here depends on timing.
#include "common.h"
#include "launch_api.h"

namespace aca {

__global__ void __launch_bounds__(EPM_THREADS) ep_monitor_scan_kernel(EpMonitorScanArgs a) {
  const int e = blockIdx.x * EPM_THREADS + threadIdx.x;
  if (e >= a.N) return;
  const int T = a.T;
  const int64_t N = a.N;
  float ret = a.cur_ret[e];
  int len = a.cur_len[e];
  for (int t0 = 0; t0 < T; t0 += EPM_UNROLL) {
    float r[EPM_UNROLL];
    uint8_t d[EPM_UNROLL];
    // a row past T is read from row T - 1 instead (in bounds, never walked): a partial round keeps as many loads in
    // flight as a full one
#pragma unroll
    for (int u = 0; u < EPM_UNROLL; ++u) {
      const int64_t i = (int64_t)min(t0 + u, T - 1) * N + e;
      r[u] = a.rewards[i];
      d[u] = a.dones[i];
    }
    // the requests stay in front of the walk (the scheduler would otherwise sink them behind it)
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < EPM_UNROLL; ++u) {
      if (t0 + u < T) {
        ret = ret + r[u];
        len = len + 1;
        if (d[u]) {   // rare: once per episode
          const int64_t i = (int64_t)(t0 + u) * N + e;
          a.ep_ret[i] = ret;
          a.ep_len[i] = len;
          ret = 0.f;
          len = 0;
        }
      }
    }
  }
  a.cur_ret[e] = ret;
  a.cur_len[e] = len;
}

// non-zero bytes of a word (a done is any non-zero byte, as in the scan)
__device__ __forceinline__ int epm_nonzero_bytes(uint32_t w) {
  const uint32_t m = (((w & 0x7f7f7f7fu) + 0x7f7f7f7fu) | w) & 0x80808080u;
  return __popc(m);
}

constexpr int EPM_WAVES = EPM_COMMIT_THREADS / 64;

// Sums (Q = 0), minima (Q = 1) or maxima (Q = 2) of one value per thread, in a fixed order: a shuffle tree inside each
// wave, then the waves' results in wave order; every thread returns the same bits. `sh` is reused between calls.
template <int NV>
__device__ __forceinline__ void epm_block_reduce(double (&v)[NV], const int (&q)[NV], double (*sh)[NV]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const double o = __shfl_down(v[k], off, 64);
      v[k] = q[k] == 0 ? v[k] + o : (q[k] == 1 ? fmin(v[k], o) : fmax(v[k], o));
    }
  }
  __syncthreads();   // (the previous call's readers are done with sh)
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < NV; ++k) sh[wave][k] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NV; ++k) v[k] = sh[0][k];
#pragma unroll 1
  for (int w = 1; w < EPM_WAVES; ++w) {   // (rolled: unrolled, its 16 NV loads at once spill)
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      const double o = sh[w][k];
      v[k] = q[k] == 0 ? v[k] + o : (q[k] == 1 ? fmin(v[k], o) : fmax(v[k], o));
    }
  }
}

__global__ void __launch_bounds__(EPM_COMMIT_THREADS) ep_monitor_commit_kernel(EpMonitorCommitArgs a) {
#pragma clang fp contract(off)
  __shared__ int s_wave[EPM_WAVES];
  __shared__ double s_red[EPM_WAVES][6];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t M = a.cells;
  const int K = a.K;
  // this thread's cells [lo, hi): chunks are a multiple of 16 bytes, so every 16-byte load below is aligned
  const int64_t chunk = ((M + EPM_COMMIT_THREADS - 1) / EPM_COMMIT_THREADS + 15) & ~(int64_t)15;
  const int64_t lo = min((int64_t)tid * chunk, M), hi = min(lo + chunk, M);
  const int64_t total = a.total[0];   // (thread 0 stores the new value after the last barrier)

  // ---- pass 1: dones per chunk
  const uint8_t* __restrict__ dones = a.dones;
  const float* __restrict__ ep_ret = a.ep_ret;
  const int32_t* __restrict__ ep_len = a.ep_len;
  float* ring_ret = a.ring_ret;   // (read back below after the barrier: not restrict)
  int32_t* ring_len = a.ring_len;
  int cnt = 0;
  int64_t i = lo;
#pragma unroll 4
  for (; i + 16 <= hi; i += 16) {
    const uint4 w = *reinterpret_cast<const uint4*>(dones + i);
    cnt += epm_nonzero_bytes(w.x) + epm_nonzero_bytes(w.y) + epm_nonzero_bytes(w.z) + epm_nonzero_bytes(w.w);
  }
  for (; i < hi; ++i) cnt += dones[i] != 0;

  // ---- exclusive scan of the counts: inside the wave by shuffles, then the waves before this one
  int inc = cnt;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int o = __shfl_up(inc, off, 64);
    if (lane >= off) inc += o;
  }
  if (lane == 63) s_wave[wave] = inc;
  __syncthreads();
  int before = 0, C = 0;
  for (int w = 0; w < EPM_WAVES; ++w) {
    const int c = s_wave[w];
    if (w < wave) before += c;
    C += c;
  }
  int r = before + inc - cnt;            // number, within this update, of this chunk's first finished episode
  const int skip = C > K ? C - K : 0;    // the first C - K would be overwritten by this same update
  const int base = (int)(total % K);

  // ---- pass 2: this chunk's episodes, in order, into their ring slots (distinct: at most K survive)
  double nsum = 0.0, nlen = 0.0;
  auto commit = [&](int64_t c) {   // cell c < M holds a done
    const float x = ep_ret[c];
    const int l = ep_len[c];
    nsum = nsum + (double)x;
    nlen = nlen + (double)l;
    if (r >= skip) {
      const int slot = (base + r) % K;
      ring_ret[slot] = x;
      ring_len[slot] = l;
    }
    ++r;
  };
  if (cnt) {
    i = lo;
    for (; i + 16 <= hi; i += 16) {
      const uint4 w = *reinterpret_cast<const uint4*>(dones + i);
      if ((w.x | w.y | w.z | w.w) == 0) continue;   // the common case
      // rare: the non-zero bytes of the two halves, lowest address first (little endian)
      uint64_t h = w.x | ((uint64_t)w.y << 32);
      int64_t c0 = i;
      for (int j = 0;; ++j) {
        while (h) {
          const int b = __builtin_ctzll(h) >> 3;
          commit(c0 + b);
          h &= ~((uint64_t)0xff << (8 * b));
        }
        if (j) break;
        h = w.z | ((uint64_t)w.w << 32);
        c0 = i + 8;
      }
    }
    for (; i < hi; ++i)
      if (dones[i]) commit(i);
  }
  __threadfence_block();
  __syncthreads();   // the ring is complete and visible to this workgroup

  // ---- summary over the filled slots
  const int64_t ntotal = total + C;
  const int filled = ntotal < K ? (int)ntotal : K;
  const double inf = __builtin_huge_val();
  double v[6] = {0.0, 0.0, inf, -inf, nsum, nlen};   // sum of returns, of lengths, min, max, this update's sums
  for (int s = tid; s < filled; s += EPM_COMMIT_THREADS) {
    const double x = (double)ring_ret[s];
    v[0] = v[0] + x;
    v[1] = v[1] + (double)ring_len[s];
    v[2] = fmin(v[2], x);
    v[3] = fmax(v[3], x);
  }
  const int q6[6] = {0, 0, 1, 2, 0, 0};
  epm_block_reduce<6>(v, q6, s_red);
  const double mean = filled ? v[0] / (double)filled : 0.0;
  double sq[1] = {0.0};
  for (int s = tid; s < filled; s += EPM_COMMIT_THREADS) {
    const double d = (double)ring_ret[s] - mean;
    const double d2 = d * d;
    sq[0] = sq[0] + d2;
  }
  const int q1[1] = {0};
  epm_block_reduce<1>(sq, q1, reinterpret_cast<double(*)[1]>(&s_red[0][0]));
  if (tid == 0) {
    a.total[0] = ntotal;
    double* o = a.summary;
    o[0] = (double)filled;
    o[1] = (double)ntotal;
    o[2] = mean;
    o[3] = filled ? sqrt(sq[0] / (double)filled) : 0.0;
    o[4] = filled ? v[2] : 0.0;
    o[5] = filled ? v[3] : 0.0;
    o[6] = filled ? v[1] / (double)filled : 0.0;
    o[7] = (double)C;
    o[8] = C ? v[4] / (double)C : 0.0;
    o[9] = C ? v[5] / (double)C : 0.0;
  }
}

}  // namespace aca

extern "C" int aca_ep_monitor_unroll(void) { return aca::EPM_UNROLL; }
extern "C" int aca_ep_monitor_max_k(void) { return aca::EPM_MAX_K; }
extern "C" int64_t aca_ep_monitor_max_cells(void) { return aca::EPM_MAX_CELLS; }

extern "C" hipError_t aca_ep_monitor_scan(const aca::EpMonitorScanArgs* a, hipStream_t stream) {
  if (!a->rewards || !a->dones || !a->cur_ret || !a->cur_len || !a->ep_ret || !a->ep_len || a->T < 1 || a->N < 1)
    return hipErrorInvalidValue;
  const int grid = (a->N + aca::EPM_THREADS - 1) / aca::EPM_THREADS;
  aca::ep_monitor_scan_kernel<<<grid, aca::EPM_THREADS, 0, stream>>>(*a);
  return hipGetLastError();
}

extern "C" hipError_t aca_ep_monitor_commit(const aca::EpMonitorCommitArgs* a, hipStream_t stream) {
  if (!a->dones || !a->ep_ret || !a->ep_len || !a->ring_ret || !a->ring_len || !a->total || !a->summary)
    return hipErrorInvalidValue;
  if (a->K < 1 || a->K > aca::EPM_MAX_K || a->cells < 1 || a->cells > aca::EPM_MAX_CELLS ||
      reinterpret_cast<uintptr_t>(a->dones) % 16 != 0)
    return hipErrorInvalidValue;
  aca::ep_monitor_commit_kernel<<<1, aca::EPM_COMMIT_THREADS, 0, stream>>>(*a);
  return hipGetLastError();
}
