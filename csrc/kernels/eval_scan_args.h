// Argument block of the evaluation record scan (eval_scan.hip), shared with csrc/bindings.cpp: plain C types only, so
// both hipcc and g++ compile this header. The binding fills it by field name.
//
// Per env e, t = 0 .. L-1 in order, fp32: ret = ret + reward[t][e]; len = len + 1; where done[t][e], the episode
// (ret, len) goes to record slot cnt of the env if cnt < E (later episodes are ignored), cnt goes up by one and
// ret = 0, len = 0. Every env starts at ret = 0, len = 0, cnt = 0 (a bank right after its reset). cnt[e] is always
// written; record slots from cnt[e] on are left as they are (the caller's sentinels). Oracle: ops/evaluation.py
// eval_scan_ref.
#pragma once
#include <stdint.h>

namespace aca {

constexpr int EVS_THREADS = 64;   // one wave per workgroup, one env per lane
constexpr int EVS_UNROLL = 16;    // time steps whose loads one round of the scan issues together

struct EvalScanArgs {
  const float* reward;        // [L][N] contiguous
  const uint8_t* done;        // [L][N] contiguous, 1 = episode boundary (time-limit cuts included)
  float* ep_ret;              // [N][E]
  int32_t* ep_len;            // [N][E]
  int32_t* cnt;               // [N]
  int L, N, E;
};

}  // namespace aca
