// Argument blocks of the returns / minibatch kernels (returns.hip), shared with csrc/bindings.cpp: plain C types
// only, so both hipcc and g++ compile this header. The binding fills them by field name.
#pragma once
#include <stdint.h>

namespace aca {

struct RetScanArgs {
  const float* r;
  const float* v;
  const uint8_t* d;
  float* ret;
  float* adv;
  double* gz;            // [T, N] (truncated n-step windows only)
  double* part;          // [gridDim.x, 8]
  unsigned int* ticket;  // zero before the first launch; self-cleaning
  double* mom;           // [8]: count, then the RS_MOM sums
  float* ev_out;         // EV(ret, V[:T]) or null
  int T, N;
  int E, CH, K;          // launch geometry (aca_returns_scan_geometry): set by the launcher
  int mode, L, norm;
  float gamma, lam, eps;
};

// operands of aca_mb_gather (host side only: the launcher unpacks them into mb_gather_kernel's parameter list)
struct MbGatherArgs {
  const uint8_t* obs; int64_t R;   // rollout observations [n, R] uint8
  const int* act; const float* logp; const float* adv; const float* ret; const float* v;   // rollout rows [n]
  uint8_t* o_obs;                  // minibatch observations [mb, R], or null with o_idx
  int* o_act; float* o_logp; float* o_adv; float* o_ret; float* o_v;                        // minibatch rows [mb]
  int mb, n;
  uint32_t seed; int64_t* uc; int ep, off;   // rows prp_index(off + i, n, key(seed, *uc, ep))
  const double* mom; float eps;    // optional advantage normalisation from [count, sum, sum of squares]
  unsigned int* bump_ticket;       // optional
  int64_t* o_idx;                  // index mode: the source row of every minibatch row [mb]
};

// operands of aca_timeout_bootstrap: the time-limit bootstrap of a rollout whose terminal observations sit in S
// compact slots per env (mlp_desc.h RolloutArgs final_obs / final_step)
struct TimeoutBootArgs {
  float* reward;              // [T, N], in place: reward[step, i] += gamma * v_final[i, s] for every used slot
  const int32_t* final_step;  // [N, S]: the step of slot (i, s), or -1 (unused: its v_final is never read)
  const float* v_final;       // [N, S]: V(terminal observation) of every slot
  int T, N, S;
  float gamma;
};

}  // namespace aca
