// Atari-shaped env bank (Pong-like game rendered to 84x84 uint8), BASELINE.json headline config.
//
// One 256-thread workgroup per env: thread 0 advances the 4 physics sub-steps (frameskip 4) and handles the
// auto-reset, then the whole workgroup renders the new 84x84 frame straight into the output stack with 16-byte
// stores and shifts the previous 3 frames in (frame stack [N, k, 84, 84]); finished envs get k copies of their
// first frame (Framer padding rule, Basic_AC/run_AC.py:37-40). Oracle: envs/atari.py (compiled with
// -ffp-contract=off so the physics rounds exactly like the PyTorch oracle).
#include "common.h"
#include "cnn_head.h"
#include "launch_api.h"
#include "pong_env.h"

namespace aca {

// One env step per workgroup with known actions: thread 0 runs the physics while the others shift the stack.
__global__ void __launch_bounds__(256) pong_step_kernel(PongIO io, const int32_t* __restrict__ actions) {
  const int e = blockIdx.x;
  __shared__ PongOut sh;
  if (threadIdx.x == 0) {
    const int a = actions[e];
    sh = pong_advance(io, e, (float)(pong_dir_index(a) - 1));
    pong_commit(io, e, sh);
  }
  pong_shift(io, e, 0, blockDim.x);
  __syncthreads();
  const PongOut r = sh;
  pong_render(io, e, r.s, r.done != 0);
}

constexpr int HEAD_HDIM = 512;                       // hidden width of the Nature-CNN trunk

// Rollout step of the native engine fused with the env: the policy/value head (z = h.Wh + bh, 512 -> A+1) of
// env e, Gumbel-max sampling with the env-counter RNG key, logp / entropy / value, then the env step with the
// sampled action -- one launch instead of head GEMM + sampling + env kernels. The head uses the whole workgroup:
// thread t owns hidden units 2t, 2t+1 (reduced from the fc GEMM's split-K partial planes, every plane's load in
// flight at once), multiplies them into its two rows of Wh (register-resident, A1 = A + 1 a template parameter so
// the GEMV has no data-dependent branch), and the A1 partial sums meet through wave shuffles + one LDS row per
// wave (fixed order). Meanwhile threads 64..66 advance the physics for all three paddle directions. Wave 0 then
// samples; after one barrier the sampled direction's outcome is committed and the newest frame rendered.

template <int A1>
__global__ void __launch_bounds__(256) pong_policy_step_kernel(PongIO io, FcParts fc, u16* __restrict__ h,
                                                               const u16* __restrict__ Wh,
                                                               const float* __restrict__ bh,
                                                               float* __restrict__ z_out, int32_t* __restrict__ act,
                                                               float* __restrict__ logp, float* __restrict__ ent,
                                                               float* __restrict__ vout, int key_shift,
                                                               uint32_t pseed, int pre_shifted,
                                                               uint64_t* __restrict__ stamps) {
  constexpr int A = A1 - 1;
  const int e = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  __shared__ int sh_act;
  __shared__ PongOut cand[3];
  __shared__ float s_acc[4][A1];
  stamp_if(stamps, 0, tid == 0);
  // operands of the sampling wave and the commit, requested first (they were dependent round trips after the
  // head's barrier): the RNG key's counters and the head bias
  const int64_t tg0 = io.tglob[e], id0 = io.env_ids[e];
  const float bhj = bh[lane < A1 ? lane : 0];
  // this thread's two Wh rows (2 * A1 bf16 = A1 32-bit words at byte offset 4 * A1 * tid)
  uint32_t wv[A1];
#pragma unroll
  for (int u = 0; u < A1; ++u) wv[u] = reinterpret_cast<const uint32_t*>(Wh)[A1 * tid + u];
  float hf[2];
  if (fc.hpart) {
    // h = relu(sum of the fc partial planes + bias), rounded to bf16 and stored for the learner
    fc_h2_from_parts(fc.hpart, fc.S, fc.plane_stride, fc.bfc, e, tid, h, hf);
  } else {
    const uint32_t hw = reinterpret_cast<const uint32_t*>(h + (size_t)e * HEAD_HDIM)[tid];
    hf[0] = __uint_as_float(hw << 16);
    hf[1] = __uint_as_float(hw & 0xFFFF0000u);
  }
  if (tid >= 64 && tid < 67) cand[tid - 64] = pong_advance(io, e, (float)(tid - 65));
  stamp_if(stamps, 8, tid == 0);
  float acc[A1];
#pragma unroll
  for (int j = 0; j < A1; ++j) {
    // Wh[2t][j] and Wh[2t+1][j] are elements j and A1 + j of the thread's 2 * A1 bf16
    const uint32_t w0 = wv[j >> 1], w1 = wv[(A1 + j) >> 1];
    const float a0 = __uint_as_float((j & 1) ? (w0 & 0xFFFF0000u) : (w0 << 16));
    const float a1 = __uint_as_float(((A1 + j) & 1) ? (w1 & 0xFFFF0000u) : (w1 << 16));
    acc[j] = wave_sum(hf[0] * a0 + hf[1] * a1);
  }
  if (lane == 0)
#pragma unroll
    for (int j = 0; j < A1; ++j) s_acc[wid][j] = acc[j];
  __syncthreads();
  stamp_if(stamps, 9, tid == 0);
  if (wid == 0) {
    const int64_t key = tg0 * ((int64_t)1 << key_shift) + id0;  // pre-step counter
    const int jj = lane < A1 ? lane : 0;
    float zj = ((s_acc[0][jj] + s_acc[1][jj]) + (s_acc[2][jj] + s_acc[3][jj])) + bhj;
    if (lane < A1) z_out[(size_t)e * A1 + lane] = zj;
    const float value = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(zj), A));
    stamp_if(stamps, 10, lane == 0);
    // categorical head over lanes 0..A-1 (same maths as categorical_sample_kernel; A1 <= 7: the 8-lane trees)
    const CatSample cs = cat_sample<8>(zj, A, lane, pseed, key);
    const int bi = cs.act;
    const float lpa = cs.lpa, H = cs.H;
    if (lane == 0) {
      act[e] = bi;
      logp[e] = lpa;
      ent[e] = H;
      vout[e] = value;
      sh_act = bi;
    }
    stamp_if(stamps, 1, lane == 0);
  } else if (!pre_shifted) {
    pong_shift(io, e, 64, blockDim.x - 64);   // else the trunk kernel already shifted the stack
  }
  stamp_if(stamps, 2, tid == 64);
  stamp_if(stamps, 3, tid == 64);
  __syncthreads();
  stamp_if(stamps, 4, tid == 0);
  const PongOut& r = cand[pong_dir_index(sh_act)];
  if (tid == 0) pong_commit(io, e, r, tg0);
  pong_render(io, e, r.s, r.done != 0);
  if (stamps) {
    stamp_if(stamps, 5, tid == 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    stamp_if(stamps, 6, tid == 0);
  }
}

// Deterministic evaluation step (algos/evaluator.py path "cnn"): the same hidden row, head GEMV, three physics
// candidates, shift and render as pong_policy_step_kernel, a kernel of its own so that the rollout step keeps its
// code. The action is the first index of the largest of the A logits (argmax_step's tie rule = torch.argmax's; a NaN
// logit never wins, all-NaN gives 0: the GREEDY categorical head of mlp.hip) over the 8-lane trees -- no key is
// hashed, no expf / logf, and h, z, log-prob, entropy and value are not stored. The commit advances state / t / tg /
// ep_ret exactly as pong_commit but leaves the bank's ep_stats alone; a finished episode goes to the env's next free
// record slot (ops/evaluation.py eval_scan_ref semantics). act / reward / done columns are optional.
__device__ __forceinline__ void pong_commit_eval(const PongIO& io, const PongEvalRec& rec, int e, const PongOut& r,
                                                 int64_t tg_old) {
  io.tglob[e] = tg_old + 1;
  if (io.reward) io.reward[e] = r.rew;
  if (io.done_out) io.done_out[e] = r.done;
  if (r.done) {
    const int c = rec.cnt[e];
    if (c >= 0 && c < rec.E) {
      rec.ep_ret[(size_t)e * rec.E + c] = r.er;
      rec.ep_len[(size_t)e * rec.E + c] = r.t;
      rec.cnt[e] = c + 1;
    }
  }
  io.tsteps[e] = r.done ? 0 : r.t;
  io.ep_ret[e] = r.done ? 0.0f : r.er;
  float* sp = io.state + (size_t)e * 8;
  const PongState& s = r.s;
  sp[0] = s.bx; sp[1] = s.by; sp[2] = s.vx; sp[3] = s.vy; sp[4] = s.pa; sp[5] = s.po; sp[6] = s.sa; sp[7] = s.so;
}

template <int A1>
__global__ void __launch_bounds__(256) pong_policy_eval_kernel(PongIO io, FcParts fc, const u16* __restrict__ h,
                                                               const u16* __restrict__ Wh,
                                                               const float* __restrict__ bh,
                                                               int32_t* __restrict__ act, PongEvalRec rec,
                                                               int pre_shifted) {
  constexpr int A = A1 - 1;
  static_assert(A1 >= 3 && A1 <= 8, "the arg-max runs on the 8-lane trees");
  const int e = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  __shared__ int sh_act;
  __shared__ PongOut cand[3];
  __shared__ float s_acc[4][A1];
  const int64_t tg0 = io.tglob[e];
  const float bhj = bh[lane < A1 ? lane : 0];
  uint32_t wv[A1];
#pragma unroll
  for (int u = 0; u < A1; ++u) wv[u] = reinterpret_cast<const uint32_t*>(Wh)[A1 * tid + u];
  float hf[2];
  if (fc.hpart) {
    fc_h2_from_parts(fc.hpart, fc.S, fc.plane_stride, fc.bfc, e, tid, nullptr, hf);   // h is not stored
  } else {
    const uint32_t hw = reinterpret_cast<const uint32_t*>(h + (size_t)e * HEAD_HDIM)[tid];
    hf[0] = __uint_as_float(hw << 16);
    hf[1] = __uint_as_float(hw & 0xFFFF0000u);
  }
  if (tid >= 64 && tid < 67) cand[tid - 64] = pong_advance(io, e, (float)(tid - 65));
  float acc[A1];
#pragma unroll
  for (int j = 0; j < A1; ++j) {
    // Wh[2t][j] and Wh[2t+1][j] are elements j and A1 + j of the thread's 2 * A1 bf16
    const uint32_t w0 = wv[j >> 1], w1 = wv[(A1 + j) >> 1];
    const float a0 = __uint_as_float((j & 1) ? (w0 & 0xFFFF0000u) : (w0 << 16));
    const float a1 = __uint_as_float(((A1 + j) & 1) ? (w1 & 0xFFFF0000u) : (w1 << 16));
    acc[j] = wave_sum(hf[0] * a0 + hf[1] * a1);
  }
  if (lane == 0)
#pragma unroll
    for (int j = 0; j < A1; ++j) s_acc[wid][j] = acc[j];
  __syncthreads();
  if (wid == 0) {
    const int jj = lane < A1 ? lane : 0;
    const float zj = ((s_acc[0][jj] + s_acc[1][jj]) + (s_acc[2][jj] + s_acc[3][jj])) + bhj;
    // lanes >= A (the value column included) and NaN logits hold the arg-max's neutral element
    const bool on = lane < A;
    float best = (on && zj == zj) ? zj : -INFINITY;
    int bi = on ? lane : 1 << 30;
    argmax_step(best, bi, xor4f(best), xor4i(bi));
    argmax_step(best, bi, xor2f(best), xor2i(bi));
    argmax_step(best, bi, xor1f(best), xor1i(bi));
    if (lane == 0) {
      if (act) act[e] = bi;
      sh_act = bi;
    }
  } else if (!pre_shifted) {
    pong_shift(io, e, 64, blockDim.x - 64);   // else the trunk kernel already shifted the stack
  }
  __syncthreads();
  const PongOut& r = cand[pong_dir_index(sh_act)];
  if (tid == 0) pong_commit_eval(io, rec, e, r, tg0);
  pong_render(io, e, r.s, r.done != 0);
}

}  // namespace aca

extern "C" hipError_t aca_env_step_pong(const aca::PongIO* io, const int32_t* actions, int N, hipStream_t stream) {
  if (N <= 0) return hipSuccess;
  aca::pong_step_kernel<<<N, 256, 0, stream>>>(*io, actions);
  return hipGetLastError();
}

extern "C" hipError_t aca_env_policy_step_pong(const aca::PongIO* io, const aca::FcParts* fc,
                                               const aca::PolicyArgs* pol, int hdim, int N, int pre_shifted,
                                               uint64_t* stamps, hipStream_t stream) {
  if (N <= 0) return hipSuccess;
  const aca::PolicyArgs& p = *pol;
  if (hdim != aca::HEAD_HDIM || reinterpret_cast<uintptr_t>(p.Wh) % 16 || reinterpret_cast<uintptr_t>(p.h) % 16)
    return hipErrorInvalidValue;
  if (fc->hpart && (fc->S < 1 || fc->S > aca::FC_MAX_PLANES || !fc->bfc || reinterpret_cast<uintptr_t>(fc->hpart) % 16 ||
                    reinterpret_cast<uintptr_t>(fc->bfc) % 16 || fc->plane_stride % 4))
    return hipErrorInvalidValue;
  switch (p.A + 1) {
#define ACA_POLICY_CASE(A1)                                                                                        \
  case A1:                                                                                                         \
    aca::pong_policy_step_kernel<A1><<<N, 256, 0, stream>>>(*io, *fc, p.h, p.Wh, p.bh, p.z, p.act, p.logp, p.ent,  \
                                                            p.value, p.key_shift, p.pseed, pre_shifted, stamps);   \
    break;
    ACA_POLICY_CASE(3) ACA_POLICY_CASE(4) ACA_POLICY_CASE(5) ACA_POLICY_CASE(6) ACA_POLICY_CASE(7)
    ACA_POLICY_CASE(8) ACA_POLICY_CASE(9) ACA_POLICY_CASE(10) ACA_POLICY_CASE(11) ACA_POLICY_CASE(12)
    ACA_POLICY_CASE(13) ACA_POLICY_CASE(14) ACA_POLICY_CASE(15) ACA_POLICY_CASE(16) ACA_POLICY_CASE(17)
    ACA_POLICY_CASE(18) ACA_POLICY_CASE(19) ACA_POLICY_CASE(20)
#undef ACA_POLICY_CASE
    default:
      return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

extern "C" hipError_t aca_env_policy_eval_pong(const aca::PongIO* io, const aca::FcParts* fc,
                                               const aca::PolicyArgs* pol, const aca::PongEvalRec* rec, int hdim,
                                               int N, int pre_shifted, hipStream_t stream) {
  const aca::PolicyArgs& p = *pol;
  if (hdim != aca::HEAD_HDIM || !p.Wh || !p.bh || reinterpret_cast<uintptr_t>(p.Wh) % 16 ||
      reinterpret_cast<uintptr_t>(p.h) % 16 || (!fc->hpart && !p.h))
    return hipErrorInvalidValue;
  if (fc->hpart && (fc->S < 1 || fc->S > aca::FC_MAX_PLANES || !fc->bfc || reinterpret_cast<uintptr_t>(fc->hpart) % 16 ||
                    reinterpret_cast<uintptr_t>(fc->bfc) % 16 || fc->plane_stride % 4))
    return hipErrorInvalidValue;
  if (rec->E < 1 || !rec->ep_ret || !rec->ep_len || !rec->cnt) return hipErrorInvalidValue;
  if (p.A + 1 < 3 || p.A + 1 > 8 || io->k < 1) return hipErrorInvalidValue;
  if (N <= 0) return hipSuccess;
  switch (p.A + 1) {
#define ACA_EVAL_CASE(A1)                                                                                          \
  case A1:                                                                                                         \
    aca::pong_policy_eval_kernel<A1><<<N, 256, 0, stream>>>(*io, *fc, p.h, p.Wh, p.bh, p.act, *rec, pre_shifted);  \
    break;
    ACA_EVAL_CASE(3) ACA_EVAL_CASE(4) ACA_EVAL_CASE(5) ACA_EVAL_CASE(6) ACA_EVAL_CASE(7) ACA_EVAL_CASE(8)
#undef ACA_EVAL_CASE
    default:
      return hipErrorInvalidValue;
  }
  return hipGetLastError();
}
