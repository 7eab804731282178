// MuJoCo-shaped linear-Gaussian env (envs/mujoco.py): s' = A s + B a + noise, r = s'[8] - 0.1 |a|^2 (device side).
// Shared by the per-step bank kernel (env_classic.hip linear_step_kernel) and the one-launch rollout (mlp.hip
// mlp_rollout_kernel). The arithmetic carries its own `fp contract(off)`: it must round exactly like the PyTorch
// oracle in every including file.
#pragma once
#include "common.h"

namespace aca {

constexpr int LIN_OBS = 17, LIN_ACT = 6;

// 32 lanes per env, lane r < 17 owns state row r: the matrix-vector products, the noise hash and the frame write are
// spread over the lanes (each row's sum keeps the sequential column order of the oracle); lane 0 owns the scalar
// episode bookkeeping. The env's previous state / actions are read by every lane of its group (broadcast loads).
constexpr int LIN_LANES = 32;

// row r of the new state; s: the env's state, av: its clamped action, sA / sB: the dynamics, nz: the row's uniform
__device__ __forceinline__ float lin_row(const float* s, const float* av, const float* sA, const float* sB, int r,
                                         float nz) {
#pragma clang fp contract(off)
  float acc = 0.f, acc2 = 0.f;
  for (int c = 0; c < LIN_OBS; ++c) acc += s[c] * sA[r * LIN_OBS + c];
  for (int c = 0; c < LIN_ACT; ++c) acc2 += av[c] * sB[r * LIN_ACT + c];
  return acc + acc2 + (nz - 0.5f) * 0.02f;
}
__device__ __forceinline__ float lin_asq(const float* av) {
#pragma clang fp contract(off)
  float asq = 0.f;
  for (int j = 0; j < LIN_ACT; ++j) asq += av[j] * av[j];
  return asq;
}
// y8: row 8 of the new state
__device__ __forceinline__ float lin_reward(float y8, float asq) {
#pragma clang fp contract(off)
  return y8 - 0.1f * asq;
}
__device__ __forceinline__ float lin_reset(float u) {
#pragma clang fp contract(off)
  return (u - 0.5f) * 0.2f;
}

}  // namespace aca
