// Argument blocks of the rolling episode window (ep_monitor.hip), shared with csrc/bindings.cpp: plain C types only, so
// both hipcc and g++ compile this header. The binding fills them by field name. Oracle: ops/ep_monitor.py.
//
// State: cur_ret [N] fp32 / cur_len [N] int32, the unfinished episode of each env (carried across updates);
// ring_ret [K] fp32 / ring_len [K] int32, the last K finished episodes; total int64 [1], episodes ever finished.
// Slot total mod K is written next; filled = min(total, K).
// Scan + commit, over the raw rewards / dones [T][N] of one update, in the flattened order i = t N + n:
//   cur_ret[n] = cur_ret[n] + r[t][n] (a plain fp32 add); cur_len[n] += 1;
//   at done[t][n] != 0: ring[total mod K] = (cur_ret[n], cur_len[n]); total += 1; cur_ret[n] = 0; cur_len[n] = 0.
// summary fp64 [10] over the filled slots: filled, total, ret_mean, ret_std (population, two passes), ret_min, ret_max,
// len_mean, new (episodes finished by this update), new_ret_mean, new_len_mean (0 where there is nothing to average).
#pragma once
#include <stdint.h>

namespace aca {

constexpr int EPM_THREADS = 64;          // scan: one wave per workgroup, one env per lane
constexpr int EPM_UNROLL = 16;           // scan: time steps whose loads one round issues together
constexpr int EPM_COMMIT_THREADS = 1024; // commit: ONE workgroup
constexpr int EPM_MAX_K = 4096;
constexpr int64_t EPM_MAX_CELLS = (int64_t)1 << 22;   // T N the one-workgroup commit takes (128 x 4096 is 2^19)
constexpr int EPM_SUMMARY = 10;

// both launches take only contiguous [T][N] columns
struct EpMonitorScanArgs {
  const float* rewards;     // [T][N] raw
  const uint8_t* dones;     // [T][N], != 0: episode boundary (time-limit cuts included)
  float* cur_ret;           // [N] read and written back
  int32_t* cur_len;         // [N] read and written back
  float* ep_ret;            // [T][N] scratch, written only where done: the finished episode's return
  int32_t* ep_len;          // [T][N] scratch, written only where done: its length
  int T, N;
};

struct EpMonitorCommitArgs {
  const uint8_t* dones;     // [T N], 16-byte aligned
  const float* ep_ret;      // [T N] from the scan
  const int32_t* ep_len;    // [T N] from the scan
  float* ring_ret;          // [K]
  int32_t* ring_len;        // [K]
  int64_t* total;           // [1]
  double* summary;          // [EPM_SUMMARY]
  int64_t cells;            // T N
  int K;
};

}  // namespace aca
