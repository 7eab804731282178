// Argument blocks of the env-bank kernels (env_classic.hip, env_atari.hip, cnn_fused.hip), shared with
// csrc/bindings.cpp: plain C types only, so both hipcc and g++ compile this header. The binding fills them by field
// name; the kernels take them by value.
#pragma once
#include <stdint.h>

namespace aca {

// vector-observation banks (CartPole, Pendulum, Acrobot, MountainCar, the linear-Gaussian system)
struct EnvIO {
  float* state;
  int32_t* t;
  int64_t* tg;
  float* ep_ret;
  float* ep_stats;  // [sum_ret, count, sum_len]
  const int64_t* env_ids;
  const float* prev;  // [N, k*D] frame stack in
  float* out;         // [N, k*D] frame stack out
  float* reward;
  uint8_t* done;
  uint8_t* truncated;
  float* final_out;   // optional [N, k*D]: the stack with the transition's new frame BEFORE any auto-reset (the
                      // terminal observation of a finished episode; time-limit bootstrapping values it)
  uint32_t seed;
  int max_steps;
  int k;
  int N;
};

// the one-thread-per-env tasks of env_classic.hip (aca_env_step_bank)
enum EnvTask { ENV_CARTPOLE, ENV_PENDULUM, ENV_ACROBOT, ENV_MOUNTAINCAR, ENV_MOUNTAINCAR_CONT };

// Pong-shaped banks (state [N, 8], frame stacks [N, k, 84, 84] uint8)
struct PongIO {
  float* state; int32_t* tsteps; int64_t* tglob; float* ep_ret; float* ep_stats; const int64_t* env_ids;
  const uint8_t* prev;   // the fused per-env step reads and writes one stack: set by the launcher (= out) there
  uint8_t* out; float* reward; uint8_t* done_out; uint8_t* trunc_out;
  uint32_t seed; int max_steps;
  int k;                 // the fused steps fix it at 4: set by the launcher there
};

// Episode records of a deterministic evaluation (env_atari.hip pong_policy_eval_kernel; ops/evaluation.py
// EvalRecords): the first E finished episodes of every env, written by the env's own workgroup as they end.
struct PongEvalRec {
  float* ep_ret;     // [N, E]
  int32_t* ep_len;   // [N, E]
  int32_t* cnt;      // [N]
  int E;
};

struct PongNext {   // the next parity's env state buffers (written by the committing workgroup)
  float* state;
  int32_t* tsteps;
  int64_t* tglob;
  float* ep_ret;
};

}  // namespace aca
