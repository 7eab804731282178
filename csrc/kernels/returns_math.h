// The one statement of the return, EV and advantage-normalisation maths (reference
// Basic_AC/run_AC.py:55-80, 241 and Basic_AC/util.py:4-12) for returns.hip and loss.hip. Inline device functions
// only; tests/oracles/returns_oracle.py counts its tolerances from the rounding points written here.
//   GAE      A_t = r_t + gamma V_{t+1} (1-d_t) - V_t + gamma lambda (1-d_t) A_{t+1},  A_T = 0,  R_t = A_t + V_t
//   n-step   window [t, h), h = min(t + L, T): discounted reward sum that stops at the first terminal transition,
//            plus gamma^(h-t) V_h only if the window did not end in a terminal; as a recurrence (the scan's form,
//            L >= T): x_t = r_t + gamma (1-d_t) x_{t+1}, x_T = V_T
#pragma once
#include "common.h"

namespace aca {

template <typename S>
__device__ __forceinline__ S not_done(bool done) { return done ? S(0) : S(1); }

// one reverse step of each recurrence; S = float (per-point kernels) or double (returns_scan_kernel); gl = gamma*lambda
template <typename S>
__device__ __forceinline__ S gae_step(S r, S v, S v_next, bool done, S gamma, S gl, S last) {
  const S nd = not_done<S>(done);
  const S delta = r + gamma * v_next * nd - v;
  return delta + gl * nd * last;
}

template <typename S>
__device__ __forceinline__ S nstep_step(S r, bool done, S gamma, S x) { return r + gamma * not_done<S>(done) * x; }

// fp32 return of point (t, col) of a rollout laid out rew / dn [T, stride], val [T + 1, stride]
__device__ __forceinline__ float nstep_point(const float* rew, const uint8_t* dn, const float* val, int t, int T, int L,
                                             float gamma, int stride, int col) {
  const int h = min(t + L, T);
  float acc = 0.f, disc = 1.f;
  bool alive = true;
  for (int k = t; k < h; ++k) {
    const size_t i = (size_t)k * stride + col;
    acc += disc * rew[i];
    disc *= gamma;
    if (dn[i]) { alive = false; break; }
  }
  if (alive) acc += disc * val[(size_t)h * stride + col];
  return acc;
}

__device__ __forceinline__ float gae_point(const float* rew, const uint8_t* dn, const float* val, int t, int T,
                                           float gamma, float lam, int stride, int col) {
  float last = 0.f;
  for (int k = T - 1; k >= t; --k) {
    const size_t i = (size_t)k * stride + col;
    last = gae_step<float>(rew[i], val[i], val[i + stride], dn[i], gamma, gamma * lam, last);
  }
  return last + val[(size_t)t * stride + col];
}

// returns_mode 1 = n-step, 2 = GAE (loss_args.h)
__device__ __forceinline__ float point_return(int mode, const float* rew, const uint8_t* dn, const float* val, int t,
                                              int T, int L, float gamma, float lam, int stride, int col) {
  return mode == 1 ? nstep_point(rew, dn, val, t, T, L, gamma, stride, col)
                   : gae_point(rew, dn, val, t, T, gamma, lam, stride, col);
}

// one point into the moments, in the slot order of the public `mom` layout (after its count):
// adv, adv^2, ret, ret^2, V, V^2, ret*V
__device__ __forceinline__ void accum_ret_moments(double (&m)[7], float ret, float adv, double v) {
  m[0] += adv; m[1] += (double)adv * adv; m[2] += ret; m[3] += (double)ret * ret;
  m[4] += v; m[5] += v * v; m[6] += (double)ret * v;
}

// one pair into (sum x, sum x^2, sum y, sum y^2, sum x*y)
__device__ __forceinline__ void accum_pair_moments(double (&m)[5], double x, double y) {
  m[0] += x; m[1] += x * x; m[2] += y; m[3] += y * y; m[4] += x * y;
}

// EV correlation of the reference (Basic_AC/util.py:4-12): mean(z(x) * z(y)) with the population std, from totals
__device__ __forceinline__ float ev_corr(double sx, double sxx, double sy, double syy, double sxy, double n) {
  const double mx = sx / n, my = sy / n;
  const double vx = sxx / n - mx * mx, vy = syy / n - my * my;
  const double cov = sxy / n - mx * my;
  return (float)(cov / sqrt(fmax(vx, 0.0) * fmax(vy, 0.0)));
}

// advantage normalisation (A - mean) * inv = (A - mean) / (eps + std_pop) (Basic_AC/run_AC.py:241), from totals
struct AdvNorm { float mean, inv; };
__device__ __forceinline__ AdvNorm adv_norm(double sum, double sumsq, double cnt, float eps) {
  const double mean = sum / cnt;
  const double var = fmax(sumsq / cnt - mean * mean, 0.0);
  return {(float)mean, 1.0f / (eps + (float)sqrt(var))};
}

}  // namespace aca
