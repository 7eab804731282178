// Argument blocks of the Nature-CNN kernels (cnn_fused.hip, env_atari.hip, fc_rollout.hip, fc_bwd.hip), shared with
// csrc/bindings.cpp: plain C types only, so both hipcc and g++ compile this header. The binding fills them by field
// name. FcParts, W1Fold, FcBwdArgs and FcRolloutArgs are kernel arguments (taken by value); TrunkArgs, PolicyArgs and
// TrunkBwdArgs are host side only: operand groups that several launchers share, unpacked into the kernels' parameter
// lists.
#pragma once
#include <stdint.h>

namespace aca {

struct FcParts {        // optional: h comes from the fc GEMM's split-K partial planes
  const float* hpart;    // null: h is read as a finished bf16 row
  int S;
  int64_t plane_stride;
  const float* bfc;
};

// The conv1 weight gradient folded into the persistent data-gradient chain (cnn_trunk_bwd_persist_kernel W1G):
// dW1[o][c] = scale * sum_p dy1[p][o] * obs[ch][4 oy + ky][4 ox + kx], c = (ch, ky, kx), p = (oy, ox).
struct W1Fold {
  const uint8_t* obs;        // [*, 4, 84, 84] uint8 frames
  const int64_t* obs_idx;    // sample b reads obs row obs_idx[b] (null: row b)
  float* planes;             // [B][32 * 256]
  float scale;               // 1 / 255
};

struct FcBwdArgs {
  const uint16_t* dh;      // [B][512] bf16
  const uint16_t* W;       // Wfc [3136][512] bf16 (row-major shadow)
  const uint16_t* y3;      // [B][3136] bf16 (saved activations, ReLU outputs)
  uint16_t* dy3;           // [B][3136] bf16
  float* dW;          // [3136][512] fp32
  int B;
  int n_dy;           // dy3 tiles: ceil(B / 32) x 98: set by the launcher
  uint64_t* stamps;   // diagnostics: per workgroup [entry, operands in, MFMAs done, stores issued]
  float* sq;          // optional: per (dWfc tile, wave) sum of squares [392 x 4] (the finaliser's norm partials
                      // then need no 6.4 MB re-read of dWfc)
};

struct FcRolloutArgs {
  const uint16_t* X; int64_t ldx; int M;
  const uint16_t* Wf; int K, N;
  float* P; int64_t pstride;
  unsigned long long* stamps;   // diagnostics: per wave [entry, operands landed, MFMAs done, stores drained]
};

// conv1..conv3 of the trunk: W1 [32, 256] (OIHW), W2 [64, 512] / W3 [64, 576] (OHWI, or their fragment-ordered
// copies), y1 [B*400, 32], y2 [B*81, 64], y3 [B*49, 64]; all 16-byte aligned
struct TrunkArgs {
  const uint16_t* W1; const float* b1;
  const uint16_t* W2; const float* b2;
  const uint16_t* W3; const float* b3;
  uint16_t* y1; uint16_t* y2; uint16_t* y3;
  float scale;           // of the uint8 frames (1 / 255)
  uint8_t* shift_out;    // optional: frames 1..3 of every observation shifted into the next stack
};

// policy / value head of a rollout step and its sampler: z = h Wh + bh [N, A + 1], Gumbel-max sampling keyed by the
// env counters
struct PolicyArgs {
  uint16_t* h;           // [N, 512] bf16 (written when it comes from the fc partial planes)
  const uint16_t* Wh;    // [512, A + 1] bf16
  const float* bh;       // [A + 1]
  int A;
  float* z; int32_t* act; float* logp; float* ent; float* value;
  int key_shift; uint32_t pseed;
};

// data-gradient chain of the trunk (aca_cnn_trunk_bwd)
struct TrunkBwdArgs {
  const uint16_t* dy3;   // [B*49, 64] (already masked by y3 > 0)
  const uint16_t* W3;    // [64, 576]
  const uint16_t* y2;    // [B*81, 64]
  const uint16_t* W2;    // [64, 512]
  const uint16_t* y1;    // [B*400, 32]
  uint16_t* dy2;
  uint16_t* dy1;         // null: not stored (persistent conv1 fold)
  float* biasp;          // [B or workgroups, 160]
  int B;
  uint64_t* stamps;
  W1Fold w1;             // obs null: no conv1 fold
};

}  // namespace aca
