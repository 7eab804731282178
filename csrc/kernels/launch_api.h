// The C interface between the gfx950 kernels (csrc/kernels/*.hip, compiled by hipcc without torch) and the torch op
// bindings (csrc/bindings.cpp, compiled by g++): the ONE declaration of every aca_* entry point. Both sides include
// this header -- every .hip file that defines or calls a launcher, and the bindings -- so a definition that disagrees
// with a declaration fails to compile (C-linkage functions cannot be overloaded).
//
// Host-safe: <stdint.h>, the HIP runtime API types and the plain argument headers only (no common.h, no device code).
// Launchers take their operands as one argument block filled by field name (const aca::XArgs*), then the
// compile-time selectors (action count, fragment-ordered weights, ...), then the stream. Every launcher returns the
// launch status; bad operands are hipErrorInvalidValue.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <hip/hip_runtime_api.h>

#include "cnn_args.h"
#include "env_args.h"
#include "ep_monitor_args.h"
#include "eval_scan_args.h"
#include "gemm_desc.h"
#include "loss_args.h"
#include "mlp_desc.h"
#include "obs_norm_args.h"
#include "optim_args.h"
#include "ppo_head.h"
#include "returns_args.h"
#include "reward_norm_args.h"

extern "C" {

// ---- env banks (env_classic.hip, env_atari.hip)
// gym classic control, one thread per env: actions are [N, act_dim] of the task's action type (int32 with act_dim = 1
// for the discrete tasks, else float), column 0 drives the env
hipError_t aca_env_step_bank(aca::EnvTask task, const aca::EnvIO* io, const void* actions, int act_dim,
                             hipStream_t stream);
hipError_t aca_env_step_linear(const aca::EnvIO* io, const float* actions, const float* A, const float* B,
                               hipStream_t stream);
hipError_t aca_env_step_pong(const aca::PongIO* io, const int32_t* actions, int N, hipStream_t stream);
hipError_t aca_env_policy_step_pong(const aca::PongIO* io, const aca::FcParts* fc, const aca::PolicyArgs* pol,
                                    int hdim, int N, int pre_shifted, uint64_t* stamps, hipStream_t stream);
// deterministic evaluation step: arg-max action, env step, episode records. Of pol only h (read when fc has no
// planes), Wh, bh, A and the optional act column are used; io.reward / io.done_out are optional columns, io.ep_stats
// and io.trunc_out are not touched. A + 1 in 3..8, rec.E >= 1.
hipError_t aca_env_policy_eval_pong(const aca::PongIO* io, const aca::FcParts* fc, const aca::PolicyArgs* pol,
                                    const aca::PongEvalRec* rec, int hdim, int N, int pre_shifted,
                                    hipStream_t stream);

// ---- Nature-CNN engine (cnn_fused.hip, fc_rollout.hip, fc_bwd.hip, conv_wgrad.hip)
// fused rollout steps: io.k set by the launcher; nx = the other parity's env state (aca_pong_fused_env_step: null
// fields -> one workgroup per env, else two); frag: W2 / W3 are the fragment-ordered copies
hipError_t aca_pong_fused_step(const aca::PongIO* io, const aca::PongNext* nx, const aca::FcParts* fc,
                               const aca::PolicyArgs* pol, const aca::TrunkArgs* tr, uint64_t* stamps, int frag, int N,
                               hipStream_t stream);
hipError_t aca_pong_fused_env_step(const aca::PongIO* io, const aca::PongNext* nx, const aca::FcParts* fc,
                                   const aca::PolicyArgs* pol, const aca::TrunkArgs* tr, uint64_t* stamps, int frag,
                                   int N, hipStream_t stream);
hipError_t aca_fc_value(const float* hpart, int S, int64_t plane_stride, const float* bfc, const uint16_t* Wh, int A1,
                        const float* bh, float* out, uint16_t* h_out, int N, hipStream_t stream);
hipError_t aca_cnn_trunk_fwd_s16(const uint8_t* obs, const aca::TrunkArgs* tr, int B, const int64_t* obs_idx, int frag,
                                 hipStream_t stream);
hipError_t aca_cnn_trunk_rows(const uint8_t* obs, const aca::TrunkArgs* tr, int B, uint8_t* copy_out, uint64_t* stamps,
                              int late_w, int frag, hipStream_t stream);
hipError_t aca_cnn_trunk_bwd(const aca::TrunkBwdArgs* a, int persist, int bias_acc, hipStream_t stream);
hipError_t aca_fc_rollout(const aca::FcRolloutArgs* a, int variant, int max_planes, int* S_out, int msplit,
                          hipStream_t stream);
hipError_t aca_fc_bwd(const aca::FcBwdArgs* a, hipStream_t stream);
hipError_t aca_conv1_wgrad2(const uint8_t* obs, const uint16_t* dy1, float* planes, int B, int P, float scale,
                            const int64_t* obs_idx, hipStream_t stream);
hipError_t aca_conv_wgrad_gemm(int layer, const uint16_t* img, const uint16_t* dy, float* planes, int B, int P,
                               hipStream_t stream);

// ---- sampling heads (heads.hip)
hipError_t aca_wave_reduce_check(const float* x, float* out, int rows, hipStream_t stream);
hipError_t aca_categorical_sample(const float* logits, int ldl, int B, int A, const int64_t* keys, const int64_t* tg,
                                  const int64_t* env_ids, int key_shift, uint32_t seed, int32_t* act, float* logp,
                                  float* ent, float* vout, hipStream_t stream);
hipError_t aca_gaussian_sample(const float* mu, int ldm, int B, int A, const float* log_std, const int64_t* keys,
                               uint32_t seed, float* act, float* logp, float* ent, hipStream_t stream);

// ---- returns, statistics, minibatches (returns.hip)
hipError_t aca_ev(const float* x, const float* y, float* out, int n, hipStream_t stream);
hipError_t aca_gae(const float* r, const float* v, const uint8_t* d, float* ret, float* adv, int T, int N, float gamma,
                   float lam, hipStream_t stream);
hipError_t aca_nstep(const float* r, const float* v, const uint8_t* d, float* tgt, float* adv, int T, int N,
                     float gamma, int L, hipStream_t stream);
hipError_t aca_normalize(const float* a, float* out, int n, float eps, hipStream_t stream);
hipError_t aca_moments(const float* x, const float* y, float* out, int n, hipStream_t stream);
hipError_t aca_normalize_mom(const float* a, float* out, const double* mom, int n, float eps, hipStream_t stream);
hipError_t aca_prp_perm(int64_t* out, int n, uint32_t seed, const int64_t* uc, int ep, hipStream_t stream);
hipError_t aca_seg_stats(const float* x, const int64_t* segs, int nv, float* out, hipStream_t stream);
void aca_returns_scan_geometry(int T, int N, int* E, int* CH, int* K, int* blocks);
hipError_t aca_returns_scan(const aca::RetScanArgs* a, hipStream_t stream);
int aca_ev_multi_blocks(int n);
hipError_t aca_ev_multi(const float* x, const float* y, float* out, int n, double* part, unsigned int* ticket,
                        hipStream_t stream);
hipError_t aca_mb_gather(const aca::MbGatherArgs* a, hipStream_t stream);
hipError_t aca_timeout_bootstrap(const aca::TimeoutBootArgs* a, hipStream_t stream);

// ---- loss and learner heads (loss.hip, ppo_head.hip); A = number of actions
hipError_t aca_ac_loss(const aca::LossArgs* a, hipStream_t stream);
hipError_t aca_head_bwd(const aca::HeadBwdArgs* a, int A, hipStream_t stream);
hipError_t aca_a2c_head(const aca::A2cHeadArgs* a, int A, hipStream_t stream);
hipError_t aca_a2c_head_env(const aca::A2cEnvArgs* a, int A, hipStream_t stream);
hipError_t aca_ppo_head(const aca::PpoHeadArgs* a, int A1, hipStream_t stream);
int aca_ppo_head_planes(int B);

// ---- optimisers and gradient plumbing (optim.hip)
hipError_t aca_sumsq(const void* x, size_t n, float* partial, int bf16, hipStream_t stream);
hipError_t aca_sumsq_multi(const float* const* xs, const size_t* ns, float* const* partials, int nseg,
                           hipStream_t stream);
int aca_sumsq_parts();
hipError_t aca_grad_finalize(const int64_t* jobs, int njobs, float* partial, const double* spart, int sN, int B,
                             const float* ent_coef, const float* kl_coef, float* stats, int ppo, hipStream_t stream);
hipError_t aca_adam_step(const aca::OptStepArgs* a, hipStream_t stream);
hipError_t aca_rmsprop_step(const aca::OptStepArgs* a, hipStream_t stream);
hipError_t aca_opt_multi(const int64_t* words, const float* fvals, const int64_t* trans, int nseg, int adam, float b1,
                         float b2, float eps, int zero_grad, int t_off, hipStream_t stream);
void aca_opt_set_stamps(int64_t* p);
int aca_opt_set_unroll(int u);
hipError_t aca_grad_move(float* src, float* dst, size_t n, int* gate, int zero, hipStream_t stream);
hipError_t aca_cast_bf16(const float* x, uint16_t* y, size_t n, hipStream_t stream);

// ---- MLP engine (mlp.hip)
hipError_t aca_mlp_fwd(const aca::MlpArgs* a, int ntw, size_t lds, int spec, hipStream_t stream);
hipError_t aca_mlp_wgrad(const aca::WgradArgs* a, hipStream_t stream);
hipError_t aca_mlp_epoch_gather(const aca::EpochGatherArgs* a, hipStream_t stream);
hipError_t aca_mlp_tshadow(const aca::MlpTower* tw, int ntw, int total, hipStream_t stream);
hipError_t aca_mlp_rollout(const aca::RolloutArgs* a, size_t lds, hipStream_t stream);
// the same rollout for any actor whose weights fit in LDS (hidden tanh included): tw = the HOST copy of the
// device-resident descriptor a->tw, which the launcher validates and sizes the LDS from
hipError_t aca_mlp_rollout_towers(const aca::RolloutArgs* a, const aca::MlpTower* tw, size_t lds,
                                  hipStream_t stream);

// ---- running observation normalisation (obs_norm.hip)
int aca_obs_norm_parts(int R);   // partial rows (= workgroups) of aca_obs_norm_prepare over R observation rows
hipError_t aca_obs_norm_prepare(const aca::ObsNormPrepArgs* a, hipStream_t stream);
hipError_t aca_obs_norm_merge(const aca::ObsNormMergeArgs* a, hipStream_t stream);

// ---- running reward scaling (reward_norm.hip; its merge is aca_obs_norm_merge with D = 1)
int aca_reward_norm_unroll(void);   // RWN_UNROLL: time steps per load round of the scan
hipError_t aca_reward_norm_scan(const aca::RewardNormScanArgs* a, hipStream_t stream);
hipError_t aca_reward_norm_apply(const aca::RewardNormApplyArgs* a, hipStream_t stream);

// ---- evaluation records from stored reward / done columns (eval_scan.hip)
int aca_eval_scan_unroll(void);   // EVS_UNROLL: time steps per load round of the scan
hipError_t aca_eval_scan(const aca::EvalScanArgs* a, hipStream_t stream);

// ---- rolling window over the last K finished training episodes (ep_monitor.hip)
int aca_ep_monitor_unroll(void);          // EPM_UNROLL: time steps per load round of the scan
int aca_ep_monitor_max_k(void);           // EPM_MAX_K
int64_t aca_ep_monitor_max_cells(void);   // EPM_MAX_CELLS: the largest T N the commit takes
hipError_t aca_ep_monitor_scan(const aca::EpMonitorScanArgs* a, hipStream_t stream);
hipError_t aca_ep_monitor_commit(const aca::EpMonitorCommitArgs* a, hipStream_t stream);

// ---- GEMM and explicit conv plumbing (gemm*.hip, conv.hip)
int aca_gemm_tile_dims(int tile, int* bm, int* bn);
int aca_gemm_supported(int tile, int bk);
int aca_gemm_effective_splits(int K, int bk, int splits);
hipError_t aca_gemm_run(const AcaGemmDesc* d, hipStream_t stream);
hipError_t aca_gemm_group_run(const AcaGemmDesc* ds, int n, hipStream_t stream, int* grouped);
int64_t aca_gemm_big_ws(int M, int N, int splits);
hipError_t aca_gemm_big(const AcaGemmDesc* d, hipStream_t stream);
hipError_t aca_im2col_u8_nchw(const uint8_t* x, uint16_t* col, int B, int C, int H, int W, int KH, int KW, int S,
                              float scale, hipStream_t stream);
hipError_t aca_im2col_nhwc(const uint16_t* x, uint16_t* col, int B, int C, int H, int W, int KH, int KW, int S,
                           hipStream_t stream);
hipError_t aca_col2im_nhwc(const uint16_t* dcol, const uint16_t* ymask, uint16_t* dx, float* colsum, int B, int C,
                           int H, int W, int KH, int KW, int S, hipStream_t stream);
hipError_t aca_colsum_bf16(const uint16_t* x, int64_t M, int N, int64_t ld, float* out, hipStream_t stream);
hipError_t aca_colsum_reduce(const float* part, int R, int N, float* out, int mod, hipStream_t stream);

}  // extern "C"
