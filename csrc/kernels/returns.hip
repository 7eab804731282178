// Return / advantage estimators over [T, N] rollouts and small statistics (K12). The maths --
// the GAE and n-step steps, the per-point returns, the moments, the EV correlation and the advantage-normalisation
// constants -- is stated once, in returns_math.h; the kernels here are its launch shapes:
// * gae:    reverse sweep per env column, one thread per column.
// * nstep:  one thread per (t, n) (PathAdv generalised to [T, N], Basic_AC/run_AC.py:55-80).
// * normalize_adv, moments, ev: one workgroup, fp64 sums; ev_multi / normalize_mom: the many-workgroup forms.
// * returns_scan: either estimator as a chunked associative scan, fused with the statistics (below).
// Oracles: ops/returns.py, utils/stats.py; tests/oracles/returns_oracle.py pins every kernel at its edges.
#include "common.h"
#include "launch_api.h"
#include "returns_math.h"

namespace aca {

__global__ void gae_kernel(const float* __restrict__ r, const float* __restrict__ v, const uint8_t* __restrict__ d,
                           float* __restrict__ ret, float* __restrict__ adv, int T, int N, float gamma, float lam) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  float last = 0.f;
  for (int t = T - 1; t >= 0; --t) {
    const size_t i = (size_t)t * N + n;
    last = gae_step<float>(r[i], v[i], v[i + N], d[i], gamma, gamma * lam, last);
    adv[i] = last;
    ret[i] = last + v[i];
  }
}

__global__ void nstep_kernel(const float* __restrict__ r, const float* __restrict__ v, const uint8_t* __restrict__ d,
                             float* __restrict__ tgt, float* __restrict__ adv, int T, int N, float gamma, int L) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= T * N) return;
  const float acc = nstep_point(r, d, v, idx / N, T, L, gamma, N, idx % N);
  tgt[idx] = acc;
  adv[idx] = acc - v[idx];
}

__global__ void __launch_bounds__(1024) normalize_kernel(const float* __restrict__ a, float* __restrict__ out, int n,
                                                         float eps) {
  __shared__ double sh[16];
  double s = 0.0, s2 = 0.0;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const double x = a[i];
    s += x;
    s2 += x * x;
  }
  s = block_sum_d(s, sh);
  s2 = block_sum_d(s2, sh);
  const AdvNorm c = adv_norm(s, s2, n, eps);
  for (int i = threadIdx.x; i < n; i += blockDim.x) out[i] = (a[i] - c.mean) * c.inv;
}

// one workgroup's (sum x, sum x^2, sum y, sum y^2, sum x*y), fp64, valid in every thread
__device__ __forceinline__ void block_pair_moments(const float* __restrict__ x, const float* __restrict__ y, int n,
                                                   double (&m)[5], double* sh) {
  for (int i = threadIdx.x; i < n; i += blockDim.x) accum_pair_moments(m, x[i], y[i]);
#pragma unroll
  for (int k = 0; k < 5; ++k) m[k] = block_sum_d(m[k], sh);
}

// out[0..4] = sum x, sum x^2, sum y, sum y^2, sum x*y  (fp64 accumulation, fp32 results)
__global__ void __launch_bounds__(1024) moments_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                       float* __restrict__ out, int n) {
  __shared__ double sh[16];
  double m[5] = {0, 0, 0, 0, 0};
  block_pair_moments(x, y, n, m, sh);
  if (threadIdx.x == 0)
#pragma unroll
    for (int k = 0; k < 5; ++k) out[k] = m[k];
}

// EV correlation (returns_math.h ev_corr) of x and y, written to *out.
__global__ void __launch_bounds__(1024) ev_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                  float* __restrict__ out, int n) {
  __shared__ double sh[16];
  double m[5] = {0, 0, 0, 0, 0};
  block_pair_moments(x, y, n, m, sh);
  if (threadIdx.x == 0) *out = ev_corr(m[0], m[1], m[2], m[3], m[4], n);
}

// PPO minibatch permutation of one epoch (csrc/kernels/common.h prp_index; oracle envs/rng.py prp)
__global__ void prp_perm_kernel(int64_t* __restrict__ out, int n, uint32_t seed, const int64_t* __restrict__ uc,
                                int ep) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = prp_index((uint32_t)i, (uint32_t)n, minibatch_key(seed, *uc, ep));
}

// PPO minibatch gather of the CNN engine (replaces six index_select copies + the permutation launch
// per minibatch): workgroup i copies batch row src = prp_index(off + i, n, key(seed, update, epoch)) -- the keyed
// epoch permutation of envs/rng.py, computed in place -- i.e. the frame stack (R bytes, 16 B vector copies) and the
// per-row action / logp / advantage / return / old value.
__global__ void __launch_bounds__(256) mb_gather_kernel(const uint8_t* __restrict__ obs, int64_t R,
                                                        const int* __restrict__ act, const float* __restrict__ logp,
                                                        const float* __restrict__ adv, const float* __restrict__ ret,
                                                        const float* __restrict__ v, uint8_t* __restrict__ o_obs,
                                                        int* __restrict__ o_act, float* __restrict__ o_logp,
                                                        float* __restrict__ o_adv, float* __restrict__ o_ret,
                                                        float* __restrict__ o_v, int n, uint32_t seed,
                                                        int64_t* uc, int ep, int off,
                                                        const double* __restrict__ mom, float eps,
                                                        unsigned int* __restrict__ bump_ticket,
                                                        int64_t* __restrict__ o_idx, int mb) {
  const int64_t ucv = *uc;
  // the per-row scalars of minibatch row i, from batch row src
  auto gather_row_scalars = [&](int i, uint32_t src) {
    float a_ = adv[src];
    if (mom) {   // advantage normalisation deferred from the returns scan (population std, fp64 totals)
      const AdvNorm c = adv_norm(mom[1], mom[2], mom[0], eps);
      a_ = (a_ - c.mean) * c.inv;
    }
    o_act[i] = act[src];
    o_logp[i] = logp[src];
    o_adv[i] = a_;
    o_ret[i] = ret[src];
    o_v[i] = v[src];
  };
  if (o_idx) {
    // index mode (o_obs null): one thread per row writes the source row index instead of copying the observation;
    // the minibatch's trunk forward and conv1 weight gradient read obs[o_idx[i]] directly (one 28 KB copy per row
    // less)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < mb) {
      const uint32_t src = prp_index((uint32_t)(off + i), (uint32_t)n, minibatch_key(seed, ucv, ep));
      o_idx[i] = src;
      gather_row_scalars(i, src);
    }
  } else {
  const int i = blockIdx.x;
  const uint32_t src = prp_index((uint32_t)(off + i), (uint32_t)n, minibatch_key(seed, ucv, ep));
  const uint8_t* s = obs + (size_t)src * R;
  uint8_t* d = o_obs + (size_t)i * R;
  if ((R & 15) == 0) {
    const uint4* s4 = reinterpret_cast<const uint4*>(s);
    uint4* d4 = reinterpret_cast<uint4*>(d);
    const int n4 = (int)(R >> 4);
    int j = threadIdx.x;
    for (; j + 3 * 256 < n4; j += 4 * 256) {   // four 16 B loads in flight per thread
      const uint4 a = s4[j], b = s4[j + 256], c = s4[j + 512], e = s4[j + 768];
      d4[j] = a; d4[j + 256] = b; d4[j + 512] = c; d4[j + 768] = e;
    }
    for (; j < n4; j += 256) d4[j] = s4[j];
  } else {
    for (int64_t j = threadIdx.x; j < R; j += 256) d[j] = s[j];
  }
  if (threadIdx.x == 0) gather_row_scalars(i, src);
  }
  if (bump_ticket) {
    // last minibatch of the update: the workgroup that finishes last advances the update counter. Only a count is
    // handed over (every workgroup read *uc before its ticket), so the ticket is relaxed, with no release fence.
    __syncthreads();
    if (threadIdx.x == 0) {
      const unsigned int prev = __hip_atomic_fetch_add(bump_ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (prev == gridDim.x - 1u) {
        *uc = ucv + 1;
        __hip_atomic_store(bump_ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
}

// Per-variable statistics of a flat fp32 parameter slab (the reference's variable_summaries, Basic_AC/policies.py:
// 9-18): out[v] = (mean, population stddev, max, min) of x[off_v, off_v + n_v). One workgroup per
// variable, double accumulation (single pass: E[x^2] - mean^2 in fp64 matches the two-pass fp32 form closely).
__global__ void __launch_bounds__(256) seg_stats_kernel(const float* __restrict__ x, const int64_t* __restrict__ segs,
                                                        float* __restrict__ out) {
  __shared__ double shd[16 * 2];
  __shared__ float shf[16];
  const int v = blockIdx.x;
  const int64_t off = segs[2 * v], n = segs[2 * v + 1];
  double s = 0.0, ss = 0.0;
  float mx = -INFINITY, mn = INFINITY;
  for (int64_t i = threadIdx.x; i < n; i += blockDim.x) {
    const float a = x[off + i];
    s += a;
    ss += (double)a * a;
    mx = fmaxf(mx, a);
    mn = fminf(mn, a);
  }
  double r[2] = {s, ss};
  block_sum_multi<2>(r, shd);
  mx = wave_max(mx);
  mn = -wave_max(-mn);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
  if (lane == 0) shf[wid] = mx;
  __syncthreads();
  float M = -INFINITY;
  for (int w = 0; w < nw; ++w) M = fmaxf(M, shf[w]);
  __syncthreads();
  if (lane == 0) shf[wid] = mn;
  __syncthreads();
  float m = INFINITY;
  for (int w = 0; w < nw; ++w) m = fminf(m, shf[w]);
  if (threadIdx.x == 0) {
    const double mean = n ? r[0] / n : 0.0;
    const double var = n ? fmax(r[1] / n - mean * mean, 0.0) : 0.0;
    out[4 * v] = (float)mean;
    out[4 * v + 1] = (float)sqrt(var);
    out[4 * v + 2] = M;
    out[4 * v + 3] = m;
  }
}

// ------------------------------------------------------------------------------------------------------------------
// Chunked associative return scan fused with the batch statistics (reference
// Basic_AC/run_AC.py:63-75, 241 and Basic_AC/util.py:4-12).
//
// Both estimators are reverse affine recurrences x_t = a_t + c_t x_{t+1}:
//   GAE      a_t = r_t + gamma V_{t+1} (1-d_t) - V_t,  c_t = gamma lambda (1-d_t),  x_T = 0      -> adv, ret = adv + V
//   n-step   a_t = r_t,                              c_t = gamma (1-d_t),           x_T = V_T  -> target (L >= T)
// A workgroup owns E env columns x CH time chunks of K steps (thread = (chunk, env), env-fastest so every time
// step is one coalesced row segment). Pass 1 composes each chunk's affine map (fp64), a Hillis-Steele suffix scan
// over the CH chunk maps in LDS gives every chunk its incoming carry, pass 2 replays the chunk with that carry and
// writes the outputs. A truncated window (n-step, L < T) scans the un-bootstrapped return Gz (x_T = 0) together
// with the next-terminal index (suffix min) and fixes each window in a third pass:
//   target_t = Gz_t + [no terminal in [t, h)] gamma^(h-t) (V_h - Gz_h),  h = min(t + L, T), Gz_T = 0,
// the prefix-sum form of the O(L) window of Basic_AC/run_AC.py:63-75.
// Every workgroup reduces its moments (adv, adv^2, ret, ret^2, V, V^2, ret*V) in fixed order into its partial
// slot; the last workgroup to arrive sums the slots in block order (bitwise reproducible), writes the totals
// (mom[0] = count, for the DP all-reduce), the EV-before correlation, and -- if `norm` -- normalises the whole
// advantage array in place, so returns + EV + advantage normalisation are ONE launch.
constexpr int RS_THREADS = 256;
constexpr int RS_MOM = 7;
constexpr int RS_KREG = 8;   // chunks up to this many steps stay in registers between the passes

__global__ void __launch_bounds__(RS_THREADS) returns_scan_kernel(RetScanArgs a) {
  __shared__ double s_a[RS_THREADS], s_c[RS_THREADS];
  __shared__ int s_ft[RS_THREADS];
  __shared__ double s_red[16 * RS_MOM];
  __shared__ double s_tot[8];
  __shared__ int s_flag;
  const int tid = threadIdx.x;
  const int e = tid % a.E, ch = tid / a.E;   // env-fastest: every time step of a chunk is one coalesced row
  const int T = a.T, N = a.N;
  const int n = blockIdx.x * a.E + e;
  const bool live = n < N && ch < a.CH;
  const int t0 = min(ch * a.K, T), t1 = min(t0 + a.K, T);
  const bool gae = a.mode == 2;
  const bool window = !gae && a.L < T;
  const double g = a.gamma, gl = (double)a.gamma * (double)a.lam;

  // every operand of the thread's chunk is requested up front (chunks of <= RS_KREG steps are kept in registers
  // for pass 2: one global round trip for the whole kernel instead of one per pass)
  const double init = (live && !gae && !window) ? (double)a.v[(size_t)T * N + n] : 0.0;
  const bool regs = a.K <= RS_KREG;
  float cr[RS_KREG], cv[RS_KREG], cvn[RS_KREG];
  uint8_t cd[RS_KREG];
  if (regs) {
#pragma unroll
    for (int u = 0; u < RS_KREG; ++u) {   // u-th step from the chunk's end; clamped (unconditional) loads
      const int t = max(t1 - 1 - u, 0);
      const size_t i = (size_t)t * N + (live ? n : 0);
      cr[u] = a.r[i];
      cv[u] = a.v[i];
      cvn[u] = a.v[i + N];
      cd[u] = a.d[i];
    }
  }
  // one step's operands, widened: the u-th register copy, or global loads (V_t only where the pass uses it)
  struct Step { double r, v, vn; bool dn; };
  auto from_regs = [&](int u) { return Step{cr[u], cv[u], cvn[u], cd[u] != 0}; };
  auto from_global = [&](int t, bool want_v) {
    const size_t i = (size_t)t * N + n;
    return Step{a.r[i], want_v ? a.v[i] : 0.f, gae ? a.v[i + N] : 0.f, a.d[i] != 0};
  };
  // body(t, step) over the thread's chunk, last step first
  auto for_chunk_reversed = [&](bool want_v, auto body) {
    if (live && regs) {
#pragma unroll
      for (int u = 0; u < RS_KREG; ++u) {
        const int t = t1 - 1 - u;
        if (t >= t0) body(t, from_regs(u));
      }
    } else if (live) {
      for (int t = t1 - 1; t >= t0; --t) body(t, from_global(t, want_v));
    }
  };
  // pass 1: chunk map x_{t0} = ca + cc x_{t1}, first terminal index in the chunk
  double ca = 0.0, cc = 1.0;
  int ft = T;
  for_chunk_reversed(gae, [&](int t, Step s) {
    ft = s.dn ? t : ft;
    ca = gae ? gae_step(s.r, s.v, s.vn, s.dn, g, gl, ca) : nstep_step(s.r, s.dn, g, ca);
    cc = (gae ? gl : g) * not_done<double>(s.dn) * cc;
  });
  // suffix scan over the chunks of each env: F_ch = f_ch o F_{ch+1}
  double x = init;
  int ntc = T;
  {
    s_a[tid] = ca;
    s_c[tid] = cc;
    s_ft[tid] = ft;
    __syncthreads();
    for (int off = 1; off < a.CH; off <<= 1) {
      double na = ca, nc = cc;
      int nf = ft;
      if (ch + off < a.CH) {
        const int j = tid + off * a.E;
        na = ca + cc * s_a[j];
        nc = cc * s_c[j];
        nf = min(ft, s_ft[j]);
      }
      __syncthreads();
      s_a[tid] = ca = na;
      s_c[tid] = cc = nc;
      s_ft[tid] = ft = nf;
      __syncthreads();
    }
    if (ch + 1 < a.CH) {
      const int j = tid + a.E;
      x = s_a[j] + s_c[j] * init;
      ntc = s_ft[j];
    }
  }

  // pass 2: replay the chunk from its carry
  double m[RS_MOM];
#pragma unroll
  for (int k = 0; k < RS_MOM; ++k) m[k] = 0.0;
  auto emit = [&](size_t i, double rt, double ad, double vt) {   // one fp32 rounding each, then the moments
    const float rf = (float)rt, af = (float)ad;
    a.ret[i] = rf;
    a.adv[i] = af;
    accum_ret_moments(m, rf, af, vt);
  };
  for_chunk_reversed(true, [&](int t, Step s) {
    const size_t i = (size_t)t * N + n;
    x = gae ? gae_step(s.r, s.v, s.vn, s.dn, g, gl, x) : nstep_step(s.r, s.dn, g, x);
    if (window) a.gz[i] = x;
    else if (gae) emit(i, x + s.v, x, s.v);
    else emit(i, x, x - s.v, s.v);
  });
  if (window) {   // uniform across the grid: every thread reaches the barrier
    __syncthreads();   // the later chunks' Gz (same workgroup) are visible
    if (live) {
      int nt = ntc;
      const double gL = pow(g, (double)a.L);
      for (int t = t1 - 1; t >= t0; --t) {
        const size_t i = (size_t)t * N + n;
        nt = a.d[i] ? t : nt;
        const int h = min(t + a.L, T);
        double tg = a.gz[i];
        if (nt >= h) {
          const double gh = (h - t == a.L) ? gL : pow(g, (double)(h - t));
          tg += gh * ((double)a.v[(size_t)h * N + n] - (h < T ? a.gz[(size_t)h * N + n] : 0.0));
        }
        const double vt = a.v[i];
        emit(i, tg, tg - vt, vt);
      }
    }
  }
  block_sum_multi<RS_MOM>(m, s_red);
  if (tid < RS_MOM) a.part[(size_t)blockIdx.x * 8 + tid] = m[tid];
  if (!last_block_arrival(a.ticket, gridDim.x, &s_flag)) return;
  {
    double s[RS_MOM];
    grid_records_sum<RS_MOM>(a.part, 8, gridDim.x, s, s_red);
    if (tid == 0)
#pragma unroll
      for (int k = 0; k < RS_MOM; ++k) s_tot[1 + k] = s[k];
  }
  __syncthreads();
  const double cnt = (double)T * N;
  if (tid == 0) {
    a.mom[0] = cnt;
    for (int k = 0; k < RS_MOM; ++k) a.mom[1 + k] = s_tot[1 + k];
    if (a.ev_out) *a.ev_out = ev_corr(s_tot[3], s_tot[4], s_tot[5], s_tot[6], s_tot[7], cnt);
  }
  if (a.norm) {
    const AdvNorm c = adv_norm(s_tot[1], s_tot[2], cnt, a.eps);
    const float fm = c.mean, inv = c.inv;
    const int tot = T * N;
    if ((tot & 3) == 0 && (((uintptr_t)a.adv) & 15) == 0) {
      float4* p = reinterpret_cast<float4*>(a.adv);
      const int n4 = tot / 4;
      int i = tid;
      for (; i + 7 * RS_THREADS < n4; i += 8 * RS_THREADS) {   // 8 loads in flight per thread, then 8 stores
        float4 q[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) q[u] = p[i + u * RS_THREADS];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          q[u].x = (q[u].x - fm) * inv; q[u].y = (q[u].y - fm) * inv;
          q[u].z = (q[u].z - fm) * inv; q[u].w = (q[u].w - fm) * inv;
          p[i + u * RS_THREADS] = q[u];
        }
      }
      for (; i < n4; i += RS_THREADS) {
        float4 q = p[i];
        q.x = (q.x - fm) * inv; q.y = (q.y - fm) * inv; q.z = (q.z - fm) * inv; q.w = (q.w - fm) * inv;
        p[i] = q;
      }
    } else {
      for (int i = tid; i < tot; i += RS_THREADS) a.adv[i] = (a.adv[i] - fm) * inv;
    }
  }
}

// Advantage normalisation from all-reduced totals (data-parallel runs: mom = sum over ranks of returns_scan's
// moments, mom[0] = global count): out = (a - mean) / (eps + std_pop). Elementwise, many workgroups.
__global__ void normalize_mom_kernel(const float* __restrict__ a, float* __restrict__ out,
                                     const double* __restrict__ mom, int n, float eps) {
  const AdvNorm c = adv_norm(mom[1], mom[2], mom[0], eps);
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    out[i] = (a[i] - c.mean) * c.inv;
}

// EV correlation over many workgroups: fixed-order partial moments + last-arriver combine (the one-workgroup
// ev_kernel above caps at one CU; this is the PPO-sized form).
__global__ void __launch_bounds__(RS_THREADS) ev_multi_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                              float* __restrict__ out, int n, double* part,
                                                              unsigned int* ticket) {
  __shared__ double sh[16 * 5];
  __shared__ double s_tot[5];
  __shared__ int s_flag;
  double m[5] = {0, 0, 0, 0, 0};
  for (int i = blockIdx.x * RS_THREADS + threadIdx.x; i < n; i += gridDim.x * RS_THREADS)
    accum_pair_moments(m, x[i], y[i]);
  block_sum_multi<5>(m, sh);
  if (threadIdx.x < 5) part[(size_t)blockIdx.x * 8 + threadIdx.x] = m[threadIdx.x];
  if (!last_block_arrival(ticket, gridDim.x, &s_flag)) return;
  {
    double s[5];
    grid_records_sum<5>(part, 8, gridDim.x, s, sh);
    if (threadIdx.x == 0)
#pragma unroll
      for (int k = 0; k < 5; ++k) s_tot[k] = s[k];
  }
  __syncthreads();
  if (threadIdx.x == 0) *out = ev_corr(s_tot[0], s_tot[1], s_tot[2], s_tot[3], s_tot[4], n);
}

// Time-limit bootstrap of a fused rollout (mlp.hip mlp_rollout_kernel keeps the terminal observations of truncated
// steps in S slots per env): one thread per slot adds gamma * V(terminal observation) to its step's reward. Every
// (step, env) sits in at most one slot, so plain stores; an unused slot (-1) reads nothing. Multiply, then add (no
// fma), like the per-step path's arithmetic. Oracle: ops/returns.py timeout_bootstrap_ref_.
__device__ __forceinline__ float boot_reward(float r, float gamma, float v) {
#pragma clang fp contract(off)
  const float b = gamma * v;
  return r + b;
}

__global__ void __launch_bounds__(256) timeout_bootstrap_kernel(TimeoutBootArgs a) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= a.N * a.S) return;
  const int step = a.final_step[idx];
  if (step < 0 || step >= a.T) return;
  const size_t o = (size_t)step * a.N + idx / a.S;
  a.reward[o] = boot_reward(a.reward[o], a.gamma, a.v_final[idx]);
}

}  // namespace aca

extern "C" hipError_t aca_timeout_bootstrap(const aca::TimeoutBootArgs* a, hipStream_t stream) {
  if (a->N <= 0 || a->S <= 0 || a->T <= 0) return hipSuccess;
  if (!a->reward || !a->final_step || !a->v_final || (int64_t)a->N * a->S > INT32_MAX) return hipErrorInvalidValue;
  aca::timeout_bootstrap_kernel<<<(a->N * a->S + 255) / 256, 256, 0, stream>>>(*a);
  return hipGetLastError();
}

extern "C" hipError_t aca_ev(const float* x, const float* y, float* out, int n, hipStream_t stream) {
  aca::ev_kernel<<<1, 1024, 0, stream>>>(x, y, out, n);
  return hipGetLastError();
}

extern "C" hipError_t aca_gae(const float* r, const float* v, const uint8_t* d, float* ret, float* adv, int T, int N,
                              float gamma, float lam, hipStream_t stream) {
  if (T <= 0 || N <= 0) return hipSuccess;
  aca::gae_kernel<<<(N + 255) / 256, 256, 0, stream>>>(r, v, d, ret, adv, T, N, gamma, lam);
  return hipGetLastError();
}

extern "C" hipError_t aca_nstep(const float* r, const float* v, const uint8_t* d, float* tgt, float* adv, int T,
                                int N, float gamma, int L, hipStream_t stream) {
  if (T <= 0 || N <= 0) return hipSuccess;
  if (L < 1) return hipErrorInvalidValue;   // the window [t, t + L) would end before it starts
  const int tot = T * N;
  aca::nstep_kernel<<<(tot + 255) / 256, 256, 0, stream>>>(r, v, d, tgt, adv, T, N, gamma, L);
  return hipGetLastError();
}

extern "C" hipError_t aca_normalize(const float* a, float* out, int n, float eps, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  aca::normalize_kernel<<<1, 1024, 0, stream>>>(a, out, n, eps);
  return hipGetLastError();
}

extern "C" hipError_t aca_moments(const float* x, const float* y, float* out, int n, hipStream_t stream) {
  aca::moments_kernel<<<1, 1024, 0, stream>>>(x, y, out, n);
  return hipGetLastError();
}

extern "C" hipError_t aca_prp_perm(int64_t* out, int n, uint32_t seed, const int64_t* uc, int ep,
                                   hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  aca::prp_perm_kernel<<<(n + 255) / 256, 256, 0, stream>>>(out, n, seed, uc, ep);
  return hipGetLastError();
}

extern "C" hipError_t aca_seg_stats(const float* x, const int64_t* segs, int nv, float* out, hipStream_t stream) {
  if (nv <= 0) return hipSuccess;
  aca::seg_stats_kernel<<<nv, 256, 0, stream>>>(x, segs, out);
  return hipGetLastError();
}

// Launch geometry of returns_scan: chunk length ~RS_KREG steps (kept in registers), CH chunks (power of two,
// <= 256) per env, E = 256 / CH envs per workgroup.
extern "C" void aca_returns_scan_geometry(int T, int N, int* E, int* CH, int* K, int* blocks) {
  int ch = 1;
  while (ch < 256 && ch * aca::RS_KREG < T) ch <<= 1;
  *CH = ch;
  *E = aca::RS_THREADS / ch;
  *K = (T + ch - 1) / ch;
  *blocks = (N + *E - 1) / *E;
}

extern "C" hipError_t aca_returns_scan(const aca::RetScanArgs* args, hipStream_t stream) {
  aca::RetScanArgs a = *args;
  if (a.T <= 0 || a.N <= 0) return hipSuccess;
  if (a.L < 1) return hipErrorInvalidValue;   // the window [t, t + L) would end before it starts
  int blocks;
  aca_returns_scan_geometry(a.T, a.N, &a.E, &a.CH, &a.K, &blocks);
  aca::returns_scan_kernel<<<blocks, aca::RS_THREADS, 0, stream>>>(a);
  return hipGetLastError();
}

extern "C" hipError_t aca_normalize_mom(const float* a, float* out, const double* mom, int n, float eps,
                                        hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  const int blocks = std::min((n + 255) / 256, 1024);
  aca::normalize_mom_kernel<<<blocks, 256, 0, stream>>>(a, out, mom, n, eps);
  return hipGetLastError();
}

extern "C" int aca_ev_multi_blocks(int n) { return std::max(1, std::min(64, (n + 2047) / 2048)); }

extern "C" hipError_t aca_ev_multi(const float* x, const float* y, float* out, int n, double* part,
                                   unsigned int* ticket, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  aca::ev_multi_kernel<<<aca_ev_multi_blocks(n), aca::RS_THREADS, 0, stream>>>(x, y, out, n, part, ticket);
  return hipGetLastError();
}

extern "C" hipError_t aca_mb_gather(const aca::MbGatherArgs* args, hipStream_t stream) {
  const aca::MbGatherArgs& a = *args;
  if (a.mb <= 0) return hipSuccess;
  if (!a.o_idx && !a.o_obs) return hipErrorInvalidValue;
  // index mode: one thread per minibatch row and no observation copy; else one workgroup per row
  const int grid = a.o_idx ? (a.mb + 255) / 256 : a.mb;
  aca::mb_gather_kernel<<<grid, 256, 0, stream>>>(a.obs, a.R, a.act, a.logp, a.adv, a.ret, a.v,
                                                  a.o_idx ? nullptr : a.o_obs, a.o_act, a.o_logp, a.o_adv, a.o_ret,
                                                  a.o_v, a.n, a.seed, a.uc, a.ep, a.off, a.mom, a.eps, a.bump_ticket,
                                                  a.o_idx, a.mb);
  return hipGetLastError();
}
