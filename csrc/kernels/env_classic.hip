// Vector-observation env banks: the gym 0.21 classic-control tasks (CartPole, Pendulum-v0, Acrobot-v1, MountainCar-v0,
// MountainCarContinuous-v0) and the MuJoCo-shaped linear-Gaussian system. Each launch advances the whole bank one
// step, auto-resets finished envs, pushes the new observation into the frame stack (Framer semantics,
// Basic_AC/run_AC.py:24-53) and accumulates episode statistics -- no host round trip, so a rollout step is
// hipGraph-capturable.
//
// A classic-control task is a struct with its state / observation widths, its action type and three functions (step,
// reset, frame); bank_step_kernel<Env>, one thread per env, is the bank bookkeeping around them, stated once. The
// linear system spreads an env over 32 lanes and has a kernel of its own (arithmetic: linear_env.h).
//
// Oracles: actor_critic_algs_on_tensorflow_amd/envs/classic.py and mujoco.py. This file is compiled with
// -ffp-contract=off and every expression below keeps the oracle's order of operations, so fp32 arithmetic rounds like
// PyTorch's (separately rounded mul/add).
#include <type_traits>

#include "common.h"
#include "launch_api.h"
#include "linear_env.h"

namespace aca {

// Framer push: shift the k-1 newest frames down and append `frame`; a reset fills the stack with k copies
template <int D>
__device__ __forceinline__ void push_frame(const EnvIO& io, float* dst, int i, const float* frame, bool reset) {
  const int k = io.k;
  const float* p = io.prev + (size_t)i * k * D;
  float* o = dst + (size_t)i * k * D;
  if (reset) {
    for (int s = 0; s < k; ++s)
      for (int j = 0; j < D; ++j) o[s * D + j] = frame[j];
  } else {
    for (int s = 0; s < k - 1; ++s)
      for (int j = 0; j < D; ++j) o[s * D + j] = p[(s + 1) * D + j];
    for (int j = 0; j < D; ++j) o[(k - 1) * D + j] = frame[j];
  }
}

// ------------------------------------------------------------------------------------------------ CartPole
struct CartPole {
  static constexpr int S = 4, D = 4;
  using Action = int32_t;

  static __device__ bool step(float* s, const Action* act, float* rew) {
    const float GRAVITY = 9.8f, MASSPOLE = 0.1f, TOTAL = 1.1f, LENGTH = 0.5f, PML = 0.05f, FORCE = 10.0f;
    const float TAU = 0.02f, THETA = (float)(12 * 2 * 3.141592653589793 / 360), XLIM = 2.4f;
    const float FOUR_THIRDS = (float)(4.0 / 3.0);
    float x = s[0], x_dot = s[1], th = s[2], th_dot = s[3];
    float force = act[0] == 1 ? FORCE : -FORCE;
    float c = cosf(th), sn = sinf(th);
    float temp = (force + PML * th_dot * th_dot * sn) / TOTAL;
    float thacc = (GRAVITY * sn - c * temp) / (LENGTH * (FOUR_THIRDS - MASSPOLE * c * c / TOTAL));
    float xacc = temp - PML * thacc * c / TOTAL;
    x = x + TAU * x_dot;
    x_dot = x_dot + TAU * xacc;
    th = th + TAU * th_dot;
    th_dot = th_dot + TAU * thacc;
    s[0] = x; s[1] = x_dot; s[2] = th; s[3] = th_dot;
    *rew = 1.0f;   // every step, the terminating one included
    return (x < -XLIM) || (x > XLIM) || (th < -THETA) || (th > THETA);
  }
  static __device__ void reset(float* s, uint32_t seed, uint32_t id, uint32_t st) {
    s[0] = uniform01(seed, id, st, 100) * 0.1f - 0.05f;
    s[1] = uniform01(seed, id, st, 101) * 0.1f - 0.05f;
    s[2] = uniform01(seed, id, st, 102) * 0.1f - 0.05f;
    s[3] = uniform01(seed, id, st, 103) * 0.1f - 0.05f;
  }
  static __device__ void frame(const float* s, float* f) {
    f[0] = s[0]; f[1] = s[1]; f[2] = s[2]; f[3] = s[3];
  }
};

// ------------------------------------------------------------------------------------------------ Pendulum
__device__ __forceinline__ float angle_normalize(float x) {
  const float PI = 3.14159265358979323846f, TWO_PI = (float)(2 * 3.141592653589793);
  float y = x + PI;
  // torch.remainder (python-style modulo): y - floor(y / m) * m
  float r = y - floorf(y / TWO_PI) * TWO_PI;
  return r - PI;
}

struct Pendulum {   // never terminates
  static constexpr int S = 2, D = 3;
  using Action = float;

  static __device__ bool step(float* s, const Action* act, float* rew) {
    const float PI = 3.14159265358979323846f;
    float th = s[0], thdot = s[1];
    float u = fminf(fmaxf(act[0], -2.0f), 2.0f);
    float an = angle_normalize(th);
    float costs = an * an + 0.1f * (thdot * thdot) + 0.001f * (u * u);
    float newthdot = thdot + (-15.0f * sinf(th + PI) + 3.0f * u) * 0.05f;
    float newth = th + newthdot * 0.05f;
    newthdot = fminf(fmaxf(newthdot, -8.0f), 8.0f);
    s[0] = newth;
    s[1] = newthdot;
    *rew = -costs;
    return false;
  }
  static __device__ void reset(float* s, uint32_t seed, uint32_t id, uint32_t st) {
    const float PI = 3.14159265358979323846f, TWO_PI = (float)(2 * 3.141592653589793);
    s[0] = uniform01(seed, id, st, 100) * TWO_PI - PI;
    s[1] = uniform01(seed, id, st, 101) * 2.0f - 1.0f;
  }
  static __device__ void frame(const float* s, float* f) {
    f[0] = cosf(s[0]);
    f[1] = sinf(s[0]);
    f[2] = s[1];
  }
};

// ------------------------------------------------------------------------------------------------ Acrobot
constexpr float ACRO_PI = 3.14159265358979323846f;

// d/dt of (theta1, theta2, omega1, omega2) under torque a: the "book" equations with m1 = m2 = l1 = I1 = I2 = 1,
// lc1 = lc2 = 0.5, g = 9.8 (AcrobotVecEnv._dsdt, constants folded as Python folds them before they meet a tensor)
__device__ void acrobot_dsdt(const float* y, float a, float* k) {
  const float HALF_PI = (float)(3.141592653589793 / 2);
  const float th1 = y[0], th2 = y[1], w1 = y[2], w2 = y[3];
  const float c2 = cosf(th2), s2 = sinf(th2);
  const float d1 = ((0.25f + (1.25f + c2)) + 1.0f) + 1.0f;
  const float d2 = (0.25f + 0.5f * c2) + 1.0f;
  const float phi2 = 4.9f * cosf((th1 + th2) - HALF_PI);
  const float phi1 =
      ((((-0.5f * w2) * w2) * s2 - (w2 * w1) * s2) + (float)(1.5 * 9.8) * cosf(th1 - HALF_PI)) + phi2;
  const float a2 = (((a + (d2 / d1) * phi1) - ((0.5f * w1) * w1) * s2) - phi2) / (1.25f - (d2 * d2) / d1);
  const float a1 = -(d2 * a2 + phi1) / d1;
  k[0] = w1;
  k[1] = w2;
  k[2] = a1;
  k[3] = a2;
}

// gym acrobot.wrap: repeated -+2 pi into [-pi, pi]. Bounded like the oracle's (WRAP_ITERS = 16): one RK4 step from
// clamped velocities moves an angle by a few turns at most, and a non-finite angle must not spin here
__device__ __forceinline__ float acrobot_wrap(float x) {
  const float TWO_PI = 2.0f * ACRO_PI;
  for (int n = 0; n < 16 && x > ACRO_PI; ++n) x = x - TWO_PI;
  for (int n = 0; n < 16 && x < -ACRO_PI; ++n) x = x + TWO_PI;
  return x;
}

struct Acrobot {
  static constexpr int S = 4, D = 6;
  using Action = int32_t;

  // one classical RK4 step of dt = 0.2; the stages are neither wrapped nor clamped
  static __device__ bool step(float* s, const Action* act, float* rew) {
    const float DT = 0.2f, HALF_DT = 0.1f, SIXTH_DT = (float)(0.2 / 6.0);
    const float MAX_VEL_1 = (float)(4 * 3.141592653589793), MAX_VEL_2 = (float)(9 * 3.141592653589793);
    const float a = (float)(act[0] - 1);
    float k1[4], k2[4], k3[4], k4[4], y[4];
    acrobot_dsdt(s, a, k1);
    for (int j = 0; j < 4; ++j) y[j] = s[j] + HALF_DT * k1[j];
    acrobot_dsdt(y, a, k2);
    for (int j = 0; j < 4; ++j) y[j] = s[j] + HALF_DT * k2[j];
    acrobot_dsdt(y, a, k3);
    for (int j = 0; j < 4; ++j) y[j] = s[j] + DT * k3[j];
    acrobot_dsdt(y, a, k4);
    for (int j = 0; j < 4; ++j) y[j] = s[j] + SIXTH_DT * (((k1[j] + 2.0f * k2[j]) + 2.0f * k3[j]) + k4[j]);
    s[0] = acrobot_wrap(y[0]);
    s[1] = acrobot_wrap(y[1]);
    s[2] = fminf(fmaxf(y[2], -MAX_VEL_1), MAX_VEL_1);
    s[3] = fminf(fmaxf(y[3], -MAX_VEL_2), MAX_VEL_2);
    const bool term = (-cosf(s[0]) - cosf(s[1] + s[0])) > 1.0f;
    *rew = term ? 0.0f : -1.0f;
    return term;
  }
  static __device__ void reset(float* s, uint32_t seed, uint32_t id, uint32_t st) {
    for (int j = 0; j < 4; ++j) s[j] = uniform01(seed, id, st, 100 + j) * 0.2f - 0.1f;
  }
  static __device__ void frame(const float* s, float* f) {
    f[0] = cosf(s[0]);
    f[1] = sinf(s[0]);
    f[2] = cosf(s[1]);
    f[3] = sinf(s[1]);
    f[4] = s[2];
    f[5] = s[3];
  }
};

// ------------------------------------------------------------------------------------------------ MountainCar
// The car step shared by both tasks for a unit force f (MountainCarVecEnv._move): clamped velocity and position; the
// left wall (position exactly at its clamp bound) stops a car that moves left. Returns the goal test.
__device__ __forceinline__ bool mountaincar_move(float* s, float f, float force, float goal) {
  const float MIN_POS = -1.2f, MAX_POS = 0.6f, MAX_SPEED = 0.07f, GRAVITY = 0.0025f;
  float p = s[0], v = s[1];
  v = v + (f * force + cosf(3.0f * p) * (-GRAVITY));
  v = fminf(fmaxf(v, -MAX_SPEED), MAX_SPEED);
  p = fminf(fmaxf(p + v, MIN_POS), MAX_POS);
  if (p == MIN_POS && v < 0.0f) v = 0.0f;
  s[0] = p;
  s[1] = v;
  return p >= goal && v >= 0.0f;
}

struct MountainCar {
  static constexpr int S = 2, D = 2;
  using Action = int32_t;

  static __device__ bool step(float* s, const Action* act, float* rew) {
    *rew = -1.0f;   // every step, the one that reaches the goal included
    return mountaincar_move(s, (float)(act[0] - 1), 0.001f, 0.5f);
  }
  static __device__ void reset(float* s, uint32_t seed, uint32_t id, uint32_t st) {
    s[0] = uniform01(seed, id, st, 100) * 0.2f - 0.6f;
    s[1] = 0.0f;
  }
  static __device__ void frame(const float* s, float* f) {
    f[0] = s[0];
    f[1] = s[1];
  }
};

struct MountainCarCont : MountainCar {
  using Action = float;

  static __device__ bool step(float* s, const Action* act, float* rew) {
    const float u = act[0];
    const bool term = mountaincar_move(s, fminf(fmaxf(u, -1.0f), 1.0f), 0.0015f, 0.45f);
    *rew = (term ? 100.0f : 0.0f) - (u * u) * 0.1f;   // the penalty reads the unclipped action
    return term;
  }
};

// ------------------------------------------------------------------------------------------------ the bank step
// actions: [N, act_dim]; column 0 is the env's action. act_dim = 1 for the discrete tasks: their stride is a constant,
// which keeps a dependent kernel-argument load out of the way of the action load
template <class Env>
constexpr bool DISCRETE = std::is_same<typename Env::Action, int32_t>::value;

template <class Env>
__global__ void __launch_bounds__(256) bank_step_kernel(EnvIO io, const typename Env::Action* __restrict__ actions,
                                                        int act_dim) {
  constexpr int S = Env::S, D = Env::D;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool active = i < io.N;
  bool done = false;
  float ret = 0.f, len = 0.f;
  if (active) {
    float* sp = io.state + (size_t)i * S;
    const int64_t tg = io.tg[i] + 1;
    io.tg[i] = tg;
    float s[S], frame[D];
    for (int j = 0; j < S; ++j) s[j] = sp[j];
    int t = io.t[i] + 1;        // the episode counters are requested before the physics, which hides their latency
    float er = io.ep_ret[i];
    float rew;
    const bool term = Env::step(s, actions + (size_t)i * (DISCRETE<Env> ? 1 : act_dim), &rew);
    const bool trunc = (t >= io.max_steps) && !term;
    done = term || trunc;
    er = er + rew;
    ret = er;
    len = (float)t;
    io.reward[i] = rew;
    io.done[i] = done;
    io.truncated[i] = trunc;
    if (io.final_out) {   // terminal observation (before the reset below)
      Env::frame(s, frame);
      push_frame<D>(io, io.final_out, i, frame, false);
    }
    if (done) {
      Env::reset(s, io.seed, (uint32_t)io.env_ids[i], (uint32_t)tg);
      t = 0;
      er = 0.f;
    }
    for (int j = 0; j < S; ++j) sp[j] = s[j];
    io.t[i] = t;
    io.ep_ret[i] = er;
    Env::frame(s, frame);
    push_frame<D>(io, io.out, i, frame, done);
  }
  add_ep_stats(io.ep_stats, active, done, ret, len);
}

template <class Env>
hipError_t launch_bank_step(const EnvIO* io, const void* actions, int act_dim, hipStream_t stream) {
  if (io->N <= 0 || io->k < 1 || act_dim < 1 || (DISCRETE<Env> && act_dim != 1)) return hipErrorInvalidValue;
  const int bs = 256;
  bank_step_kernel<Env><<<(io->N + bs - 1) / bs, bs, 0, stream>>>(
      *io, static_cast<const typename Env::Action*>(actions), act_dim);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ linear (MuJoCo-shape)
// LIN_LANES lanes per env (linear_env.h): lane r < LIN_OBS owns state row r, lane 0 the episode bookkeeping
__global__ void __launch_bounds__(256) linear_step_kernel(EnvIO io, const float* __restrict__ actions,
                                                          const float* __restrict__ A, const float* __restrict__ B) {
  __shared__ float sA[LIN_OBS * LIN_OBS], sB[LIN_OBS * LIN_ACT];
  for (int j = threadIdx.x; j < LIN_OBS * LIN_OBS; j += blockDim.x) sA[j] = A[j];
  for (int j = threadIdx.x; j < LIN_OBS * LIN_ACT; j += blockDim.x) sB[j] = B[j];
  __syncthreads();
  const int i = (blockIdx.x * blockDim.x + threadIdx.x) / LIN_LANES;
  const int r = threadIdx.x % LIN_LANES;
  const bool active = i < io.N;
  const bool owner = active && r == 0;
  bool done = false;
  float ret = 0.f, len = 0.f;
  if (active) {
    float* s = io.state + (size_t)i * LIN_OBS;
    const int64_t tg = io.tg[i] + 1;
    const uint32_t id = (uint32_t)io.env_ids[i], st = (uint32_t)tg;
    float a[LIN_ACT];
    for (int j = 0; j < LIN_ACT; ++j) a[j] = fminf(fmaxf(actions[(size_t)i * LIN_ACT + j], -1.0f), 1.0f);
    const float asq = lin_asq(a);
    float y = 0.f;
    if (r < LIN_OBS) y = lin_row(s, a, sA, sB, r, uniform01(io.seed, id, st, 300 + r));
    // reward reads row 8 (lane 8 of the group)
    const float y8 = __shfl(y, (threadIdx.x & 63 & ~(LIN_LANES - 1)) + 8, 64);
    const float rew = lin_reward(y8, asq);
    const int t = io.t[i] + 1;
    const bool trunc = t >= io.max_steps;
    done = trunc;
    const float er = io.ep_ret[i] + rew;
    ret = er;
    len = (float)t;
    if (io.final_out && r < LIN_OBS) {   // terminal observation (before the reset below)
      const int k = io.k;
      const float* pv = io.prev + (size_t)i * k * LIN_OBS;
      float* fo = io.final_out + (size_t)i * k * LIN_OBS;
      for (int f = 0; f < k - 1; ++f) fo[f * LIN_OBS + r] = pv[(f + 1) * LIN_OBS + r];
      fo[(k - 1) * LIN_OBS + r] = y;
    }
    if (done && r < LIN_OBS) y = lin_reset(uniform01(io.seed, id, st, 100 + r));
    if (r < LIN_OBS) {
      s[r] = y;
      // frame stack: shift the k-1 newest frames down, append y (reset: k copies of y)
      const int k = io.k;
      const float* pv = io.prev + (size_t)i * k * LIN_OBS;
      float* o = io.out + (size_t)i * k * LIN_OBS;
      for (int f = 0; f < k - 1; ++f) o[f * LIN_OBS + r] = done ? y : pv[(f + 1) * LIN_OBS + r];
      o[(k - 1) * LIN_OBS + r] = y;
    }
    if (owner) {
      io.tg[i] = tg;
      io.reward[i] = rew;
      io.done[i] = done;
      io.truncated[i] = trunc;
      io.t[i] = done ? 0 : t;
      io.ep_ret[i] = done ? 0.f : er;
    }
  }
  add_ep_stats(io.ep_stats, owner, done, ret, len);
}

}  // namespace aca

using namespace aca;

extern "C" hipError_t aca_env_step_bank(EnvTask task, const EnvIO* io, const void* actions, int act_dim,
                                        hipStream_t stream) {
  switch (task) {
    case ENV_CARTPOLE: return launch_bank_step<CartPole>(io, actions, act_dim, stream);
    case ENV_PENDULUM: return launch_bank_step<Pendulum>(io, actions, act_dim, stream);
    case ENV_ACROBOT: return launch_bank_step<Acrobot>(io, actions, act_dim, stream);
    case ENV_MOUNTAINCAR: return launch_bank_step<MountainCar>(io, actions, act_dim, stream);
    case ENV_MOUNTAINCAR_CONT: return launch_bank_step<MountainCarCont>(io, actions, act_dim, stream);
  }
  return hipErrorInvalidValue;
}

extern "C" hipError_t aca_env_step_linear(const EnvIO* io, const float* actions, const float* A, const float* B,
                                          hipStream_t stream) {
  const int bs = 256;
  linear_step_kernel<<<(io->N * LIN_LANES + bs - 1) / bs, bs, 0, stream>>>(*io, actions, A, B);
  return hipGetLastError();
}
