// Argument blocks of the loss and A2C learner-head kernels (loss.hip), shared with csrc/bindings.cpp: plain C types
// only, so both hipcc and g++ compile this header. The binding fills them by field name; the kernels take them by
// value.
#pragma once
#include <stdint.h>

namespace aca {

struct LossArgs {
  const float* logits; int64_t ldl;     // or mu for the gaussian head
  const float* value; int64_t ldv;      // may be null (no critic term)
  const int32_t* act_i;                 // categorical actions
  const float* act_f;                   // gaussian actions [B, A]
  const float* log_std;                 // gaussian
  const float* logp_old;
  const float* adv;
  const float* ret;
  const float* v_old;                   // may be null
  const float* ent_coef;                // device scalar
  const float* kl_coef;                 // device scalar
  float vf_coef, ppo_clip, v_clip;
  uint16_t* dlogits; int64_t lddl;
  uint16_t* dvalue; int64_t lddv;
  float* dlog_std;                      // gaussian: fp32 [A] (atomic add)
  float* stats;
  int B, A;
  int gaussian;
  // fused returns (A2C): rew/done [T, N], val [T+1, N]; ret/adv (global scratch [B]) are written then read back
  int returns_mode;                     // 0: use ret/adv as given; 1: n-step (look-ahead L); 2: GAE(lambda)
  const float* rew; const float* val; const uint8_t* dn;
  int T, N, L;
  float gamma, lam;
  int norm_adv;
  float* ret_w; float* adv_w;
  float* dbias; int dbias_n;            // head bias gradient (A+1 columns: logits | value)
};

struct HeadBwdArgs {
  const float* z;            // [B, A1] logits | value
  const int32_t* act;
  const float* logp_old;
  const float* ent_coef; const float* kl_coef;
  float vf_coef;
  const float* rew; const float* val; const uint8_t* dn;
  int T, N, L, returns_mode, norm_adv;
  float gamma, lam;
  float* ret_w; float* adv_w;
  const uint16_t* h;         // [B, 512] bf16 (rollout activations)
  const uint16_t* Wh;        // [512, A1] bf16 shadow
  uint16_t* dh;              // [B, 512] out
  float* gWh; float* gbh; float* gbfc;   // (a2c_head_env: unused, its gradients go to the partial planes)
  float* stats;
  int B;                     // = T * N: set by the launcher
  uint64_t* stamps;          // optional [workgroups, 16] s_memrealtime phase stamps (diagnostics; null in production)
};

struct A2cHeadArgs {
  HeadBwdArgs h;
  const float* hpart; int S; int64_t plane_stride;   // last fc product (split-K planes) of s_T, or null: val holds V(s_T)
  const float* bfc; const float* bh;
  float* vboot;              // [N] = val + B (written in phase 0): set by the launcher
  unsigned int* bar;         // [0] arrivals, [1] departures, [2] timeout flag
};

struct A2cEnvArgs {
  HeadBwdArgs h;
  const float* hpart; int S; int64_t plane_stride;   // last fc product of s_T (split-K planes), or null: val[T] holds V
  const float* bfc; const float* bh;
  float* pWh; float* pbfc; float* pbh;               // planes [N][512 * A1], [N][512], [N][A1]
  double* spart;                                     // [N][A2C_STATS] statistics rows
};

}  // namespace aca
