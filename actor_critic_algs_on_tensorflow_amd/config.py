"""Typed training configuration + presets.

The reference configures itself with argparse flags and module constants (defaults table: SURVEY §2.6). Here
one dataclass carries everything; presets mirror the reference defaults (``basic_ac``, ``a3c``) and the
BASELINE.json configs (``cartpole_cpu``, ``pong_a2c``, ``breakout_ppo``, ``a2c_dp8``, ``mujoco_ppo_dp8``).
"""
from __future__ import annotations

import dataclasses
from dataclasses import dataclass, field


@dataclass
class EngineOpts:
    """Kernel selection of the native CNN engine (``algos/engine.py``). Every switch is a path that is the default of
    some BASELINE config or the oracle of a test (tests/test_config_cpu.py pins the list); the defaults are the
    fastest measured configuration on MI355X (A/B evidence in ``profiles/``). ``TrainConfig.engine_opts`` carries one;
    plain dicts are accepted and converted."""
    # -- rollout -------------------------------------------------------------------------------------------------
    fused_step: bool = True           # Pong bank: policy/env step t fused with the trunk of obs t+1 (off: oracle)
    trunk_rows_max_b: int = 64        # row-split trunk (7 workgroups per env) up to this many envs, per-env above
    fused_env_split: bool = True      # per-env fused step (banks above trunk_rows_max_b): two workgroups per env
    adam_step_offsets: bool = True    # MLP PPO: grouped Adam launches take their step from the minibatch index (no ticket)
    frag_weights: bool = True         # conv weights also kept fragment-ordered (written by the optimiser step): the
                                      # MFMA weight loads become one contiguous 1 KB read per wave
    fc_max_planes: int = 32           # split-K partial planes of the rollout fc product (consumer-reduced)
    fc_frag_big: int = 17             # ... for banks of 33..128 envs (+16: 32-row blocks split over workgroups)
    fc_frag: int = 5                  # rollout fc product (<= 32 envs) on a fragment-ordered Wfc copy (fc_rollout.hip
                                      # variant 0..9; -1: the general GEMM on the row-major shadow)
    # -- learner -------------------------------------------------------------------------------------------------
    a2c_head: bool = True             # A2C: V(s_T) + returns + loss + head backward in one launch (loss.hip a2c_head)
    a2c_head_env: bool = True         # ... as one workgroup per env without a grid-wide hand-off (A2C without
                                      # advantage normalisation; head gradients as per-env planes the finaliser sums)
    fused_head: bool = True           # A2C: loss + head backward in one launch (round-2 head_bwd) when a2c_head is off
    grouped: bool = True              # independent backward products as ONE grouped GEMM launch (no side stream)
    det_wgrad: bool = True            # weight gradients as split-K planes reduced in fixed order (bitwise determinism)
    fused_bwd: bool = True            # dy3 -> dy2 -> dy1 in one per-sample kernel (cnn_trunk_bwd)
    mb_index: bool = True             # PPO minibatches read their observations in place through a row index
    ppo_head: bool = True             # large-batch head: z, loss, dz, dh and dWh / dbh / dbfc planes in one launch
    fc_bwd: bool = True               # learner batches of <= 256 rows: dy3 and dWfc in one dedicated launch (fc_bwd.hip)
    large_batch_min_b: int = 1024     # learner batches from this many rows: the persistent trunk backward (with the
                                      # conv1 weight gradient folded in), the batched-position conv2 / conv3 weight
                                      # gradients, gemm_big fc products, the backward on one stream
    trunk_bwd_persist: int = 256      # workgroups of the persistent trunk backward
    wgrad_planes: int = 64            # split-K planes of the GEMM weight gradients
    conv1_v2_planes: int = 256        # planes of the conv1 weight gradient when it is not folded (one workgroup each)
    nhwc_planes: int = 256            # planes of the conv2 / conv3 weight-gradient kernels

    def replace(self, **kw):
        return dataclasses.replace(self, **kw)


# string-valued TrainConfig fields and the values they accept (validated in __post_init__)
CHOICES = {
    "algo": {"a2c", "ppo", "a3c", "basic_ac"},
    "model": {"auto", "mlp", "cnn"},
    "model_variant": {"basic", "a3c"},
    "returns": {"nstep", "gae"},
    "optimizer": {"adam", "rmsprop"},
    "lr_schedule": {"constant", "linear"},
    "dtype": {"bf16", "fp32"},
    "engine": {"auto", "native", "torch"},
    "dist_backend": {"auto", "nccl", "gloo"},
    "overlap": {"strict", "lag1"},
    "grad_bucket_dtype": {"fp32", "bf16"},
    "dp_capture": {"auto", "segments"},
    "mode": {"train", "debug", "debug-light", "debug-full"},
    "hidden_act": {None, "tanh", "relu", "lrelu"},   # None: the reference's lrelu actor / relu critic
    "mlp_init": {"reference", "orthogonal"},
}

# Limits of the native MLP engine's tower shapes (csrc/kernels/mlp.hip; ops/mlp.py). The torch engine has none.
MLP_MAX_HIDDEN = 4        # MLP_MAXL = 5 layers of a tower descriptor, the head included
MLP_MAX_WIDTH = 256       # MLP_MAXW: one layer's activations are one LDS tile of at most 16 column tiles
MLP_PARTS = 256           # sum-of-squares slots of a tower (global-norm clip), one per 16 x 16 tile of every dW
MLP_MAX_LDS = 140 * 1024  # dynamic LDS the generic kernel's launcher grants


def _ngp2(w):
    g = (w + 15) // 16
    return 1 if g <= 1 else 2 if g <= 2 else 4 if g <= 4 else 8 if g <= 8 else 16


def mlp_tower_slots(widths):
    """Sum-of-squares slots of a tower ``[D, h_0, ..., out]``: one per 16 x 16 tile of every weight gradient."""
    return sum(((k + 15) // 16) * ((n + 15) // 16) for k, n in zip(widths[:-1], widths[1:]))


def mlp_tower_lds_bytes(widths):
    """Dynamic LDS of the generic kernel's train launch for a tower ``[D, h_0, ..., out]`` (``MLPEngine.lds_bytes``):
    the input tile, every layer's output tile, and the two data-gradient tiles."""
    return 4 * (sum(16 * (16 * _ngp2(w) + 4) for w in widths) + 2 * 16 * (MLP_MAX_WIDTH + 4))


def check_mlp_tower(field, hidden, in_dim=None, out_dim=None, extra_slots=0):
    """The native MLP engine's limits on one tower's hidden widths, as ``ValueError``s that name ``field`` and the
    limit. ``in_dim`` / ``out_dim`` (known once the env is: observation width, head width) add the checks that need
    the whole tower; ``extra_slots``: 1 for a continuous actor (its ``log_std`` takes one slot)."""
    hidden = tuple(int(w) for w in hidden)
    if not 1 <= len(hidden) <= MLP_MAX_HIDDEN:
        raise ValueError(f"{field}={hidden!r}: a tower has 1 to {MLP_MAX_HIDDEN} hidden layers (the engine's tower "
                         f"descriptor holds MLP_MAXL = {MLP_MAX_HIDDEN + 1} layers, the head included)")
    for w in hidden:
        if not 1 <= w <= MLP_MAX_WIDTH:
            raise ValueError(f"{field}={hidden!r}: width {w} is outside 1..{MLP_MAX_WIDTH} (MLP_MAXW)")
        if w > 32 and w % 16:
            raise ValueError(f"{field}={hidden!r}: width {w} is above 32 and not a multiple of 16 (the data-gradient "
                             "weight loads are 16-wide vectors)")
    # (before the env is known: the narrowest input and head there can be, a lower bound of what the tower needs)
    widths = [int(in_dim) if in_dim is not None else 1] + list(hidden) + [int(out_dim) if out_dim is not None else 1]
    if in_dim is not None and not 1 <= int(in_dim) <= MLP_MAX_WIDTH:
        raise ValueError(f"{field}: observation width {in_dim} is outside 1..{MLP_MAX_WIDTH} (MLP_MAXW)")
    slots = mlp_tower_slots(widths) + extra_slots
    if slots > MLP_PARTS:
        raise ValueError(f"{field}={hidden!r}: the tower's weight gradients are {slots} 16 x 16 tiles"
                         f"{' (+1 for log_std)' if extra_slots else ''}, and a tower has MLP_PARTS = {MLP_PARTS} "
                         "sum-of-squares slots, one per tile (sum of ceil(K/16) * ceil(N/16) over its layers; a "
                         "256 -> 256 layer alone needs 256)")
    if mlp_tower_lds_bytes(widths) > MLP_MAX_LDS:
        raise ValueError(f"{field}={hidden!r}: the tower's activation tiles need {mlp_tower_lds_bytes(widths)} bytes of "
                         f"LDS, above the {MLP_MAX_LDS} the kernel's launcher grants")
    return hidden


@dataclass
class TrainConfig:
    # -- problem ---------------------------------------------------------------------------------------------
    env: str = "Pendulum-v0"
    algo: str = "a2c"                 # a2c | ppo | a3c | basic_ac (reference-parity episode-batched trainer)
    num_envs: int = 1                 # envs per rank / GPU
    n_steps: int = 5                  # rollout length T
    frames: int = 1                   # frame stack for vector envs (Atari envs always stack 4)
    model: str = "auto"               # auto | mlp | cnn
    model_variant: str = "basic"      # basic | a3c (reference divergences)
    seed: int = 12321
    device: str = "cpu"
    # -- returns -----------------------------------------------------------------------------------------------
    gamma: float = 0.99
    returns: str = "nstep"            # nstep (PathAdv generalisation) | gae
    look_ahead: int | None = None     # n-step truncation L (reference: 40); None = whole rollout
    gae_lambda: float = 0.95
    norm_adv: bool = False
    # a time-limit cut stays an episode boundary, and its step's reward gets gamma * V(terminal observation). Runs on
    # the torch engine and the native MLP engine (classic banks per step; the MuJoCo-shaped bank inside the
    # one-launch fused rollout), not on the native CNN engine
    bootstrap_on_timeout: bool = False
    # running per-feature mean / variance of the raw vector observations, applied in front of both MLP towers as
    # clip((obs - mean) / sqrt(var + 1e-8), +-obs_clip) (ops/obs_norm.py). The tables are frozen for the whole of an
    # update; its rollout's observations are merged after its learner. MLP models under a2c / ppo only
    norm_obs: bool = False
    obs_clip: float = 10.0
    # running return-based reward scaling (ops/reward_norm.py): after each rollout the raw rewards are divided by the
    # running standard deviation of the per-env discounted return and clipped to +-reward_clip; no mean is subtracted.
    # The statistics include the rollout they scale (rewards never feed the policy, so nothing has to stay frozen as
    # with norm_obs); a time-limit bootstrap term is added after the scaling. MLP models under a2c / ppo only
    norm_reward: bool = False
    reward_clip: float = 10.0
    # -- losses ------------------------------------------------------------------------------------------------
    ent_coef: float = 0.01            # reference "gamma" (Basic_AC/policies.py:38)
    kl_coef: float = 0.0              # reference "beta" (squared log-prob drift proxy)
    vf_coef: float = 0.5
    # -- optimiser ---------------------------------------------------------------------------------------------
    optimizer: str = "adam"           # adam | rmsprop
    lr: float = 7e-4                  # shared-model lr / actor lr
    critic_lr: float = 1e-3           # separate-critic lr (reference 0.001)
    clip_value: float | None = None   # element-wise grad clip (reference actor: 1.0 Basic / 0.1 A3C)
    critic_clip_value: float | None = None
    max_grad_norm: float | None = 0.5
    # -- reference regularisation machinery -----------------------------------------------------------------------
    kl_adaptive_lr: bool = False
    desired_kl: float = 0.002
    min_lr: float = 1e-6
    max_lr: float = 1.0
    anneal_regularizers: bool = False  # log10 schedules of ent/kl coefs (Basic_AC/run_AC.py:181-182)
    lr_schedule: str = "constant"     # constant | linear (every optimiser's lr decays linearly to 0 at total_updates;
                                      # not combined with the KL-adaptive lr, which owns the actor lr)
    # -- PPO ---------------------------------------------------------------------------------------------------
    ppo_epochs: int = 4
    ppo_minibatches: int = 4
    ppo_clip: float = 0.1
    ppo_value_clip: float | None = None
    # early stopping on the approximate KL: before each minibatch step, approx_kl = mean(expm1(x) - x) with
    # x = logp - logp_old at the current parameters; once approx_kl > 1.5 * target_kl that step and every remaining
    # step of the update are not applied (parameters, moments and Adam step counts untouched). Decided on the device
    # (the captured update issues nothing from the host). PPO on the torch engine and the native MLP engine; no data
    # parallelism yet. None = off
    target_kl: float | None = None
    # -- evaluation ----------------------------------------------------------------------------------------------
    # periodic deterministic evaluation (algos/evaluator.py): after every eval_every-th update the policy's mean /
    # arg-max actions are scored on a second bank of eval_envs envs (same env id, frames and time limit; RNG seed
    # eval_seed) that is put back to the same start states each time, eval_episodes episodes per env, raw rewards. It
    # writes nothing the trainer reads. a2c / ppo on one rank: the MLP models, and the CNN model on a GPU; 0 = off
    eval_every: int = 0
    eval_envs: int = 16
    eval_episodes: int = 1
    eval_seed: int | None = None      # None: derived from seed (and different from it)
    # -- training-time episode statistics ------------------------------------------------------------------------------
    # rolling window over the last ep_window finished training episodes (ops/ep_monitor.py), kept on the device: after
    # each rollout the raw rewards / dones are walked in step order per env (a plain fp32 add, carried across updates)
    # and the finished episodes enter a ring in the order (step, env index); mean / std / min / max of the window are
    # reduced on the device in a fixed order, so a run repeats them bit for bit. Raw rewards: before norm_reward scales
    # them and before any bootstrap term. Read once per log row (ep_ret_mean, ... in the metrics stream); nothing the
    # trainer reads is written. a2c / ppo; under data parallelism every rank keeps the window of its own envs and
    # rank 0 logs its own. 0 = off, at most 4096
    ep_window: int = 0
    # stop training once the window is full and its mean return is >= stop_return (checked where a log row is
    # produced, so it needs ep_window > 0 and stdout_freq > 0; one rank only). trainer.stopped_at = that update
    stop_return: float | None = None
    # -- execution -----------------------------------------------------------------------------------------------
    dtype: str = "bf16"               # compute dtype of the GPU engine (fp32 masters always)
    engine: str = "auto"              # auto | native (hand-written HIP engine) | torch (autograd reference)
    cuda_graph: bool = True
    reuse_rollout_acts: bool = True   # native A2C: the rollout's activations are the learner's forward (exact)
    fused_rollout: bool = True        # native MLP engine + MuJoCo-shaped bank: the whole rollout in one launch
    # the one-launch rollout (and the one-launch evaluation) for custom actors as well: any tower the native MLP engine
    # takes, hidden tanh included, whose staged weights fit in LDS (ops/mlp.py MLPEngine.rollout_towers_fit; e.g.
    # (64, 64), (192, 64), (256, 64, 64) at one frame) runs the launch's generic-tower chain; one that does not fit
    # ((256, 128)) keeps the per-step rollout. Needs fused_rollout; a2c / ppo on the MLP models; no effect on
    # engine="torch" or on the reference actor, which keeps its register-resident chain
    fused_rollout_towers: bool = False
    # -- MLP towers (models/mlp.py) --------------------------------------------------------------------------------
    # hidden widths of the actor / critic (None: the reference's 128-128-64 / 256-128(-128, variant a3c)); the hidden
    # activation of both (None: the reference's lrelu actor / relu critic); the initialisers. A tower is "custom" when
    # its *_hidden or hidden_act is given: 1..4 hidden layers, widths 1..256 (above 32: multiples of 16), at most 256
    # 16 x 16 weight-gradient tiles per tower -- the native MLP engine's limits (check_mlp_tower), checked here for
    # engine "native" / "auto"; engine="torch" has none. a2c / ppo on the MLP models only. Custom towers run the
    # generic kernels; their rollout is per step unless fused_rollout_towers is set (above), the reference actor's
    # register-resident one-launch chain and the SPEC train path stay the reference's
    actor_hidden: tuple | None = None
    critic_hidden: tuple | None = None
    hidden_act: str | None = None     # tanh | relu | lrelu
    mlp_init: str = "reference"       # reference | orthogonal (gain sqrt 2 hidden, 0.01 policy head, 1 value head)
    engine_opts: EngineOpts = field(default_factory=EngineOpts)   # kernel selection of the native CNN engine
    total_updates: int = 1000
    # -- distributed -----------------------------------------------------------------------------------------------
    dist_backend: str = "auto"        # auto -> nccl (RCCL) on GPU, gloo on CPU
    overlap: str = "strict"           # strict | lag1 (all-reduce overlapped with next rollout, policy lag 1)
    grad_bucket_dtype: str = "fp32"   # fp32 | bf16 (all-reduce the gradient buckets as bf16: half the xGMI bytes)
    dp_capture: str = "auto"          # auto: RCCL collectives recorded INSIDE the update's hipGraph (one graph per
                                      # update); gloo (host-side collectives) -> a graph chain cut at each one |
                                      # segments: force the graph chain (A/B and equivalence tests)
    ps_num: int = 1                   # A3C parameter-server ranks
    # -- reference episode-batched trainer (basic_ac) -------------------------------------------------------------
    max_rolls: int = 7
    max_path_length: int | None = None
    ep_length_stop: int | None = None
    # -- logging / checkpoints ---------------------------------------------------------------------------------------
    outdir: str = "log.txt"
    metrics_path: str | None = None
    stdout_freq: int = 20
    flush_every: int = 100
    save_every: int = 600
    checkpoint_dir: str = "tmp/checkpoints"
    keep_checkpoints: int = 3
    quiet: bool = False
    legacy_step_index: bool = False
    tboard: bool = False              # TensorBoard event file under summaries_dir(outdir) (utils/tensorboard.py)
    tb_root: str = "summaries"
    mode: str = "train"               # train | debug | debug-light | debug-full
    trace: bool = False               # per-phase timers + ROCTx ranges (utils/trace.py), reported in the metrics stream
    # -- failure handling -------------------------------------------------------------------------------
    fault_inject: str | None = None   # "rank:iteration": that rank dies (os._exit) when it reaches that iteration
    resume: str | None = None         # "auto" = newest checkpoint in checkpoint_dir, or a checkpoint prefix
    dist_timeout_s: int = 300         # collective timeout: a dead peer surfaces as an exception, not a hang

    def __post_init__(self):
        for name, allowed in CHOICES.items():
            v = getattr(self, name)
            if v not in allowed:
                raise ValueError(f"TrainConfig.{name}={v!r}: expected one of {sorted(allowed, key=str)}")
        if self.lr_schedule == "linear" and self.kl_adaptive_lr:
            raise ValueError("lr_schedule='linear' with kl_adaptive_lr=True: the KL controller owns the actor lr, so "
                             "only the critic would decay; pick one")
        if not isinstance(self.engine_opts, EngineOpts):
            self.engine_opts = EngineOpts(**dict(self.engine_opts or {}))
        if self.norm_obs:
            if self.algo in ("a3c", "basic_ac"):
                raise ValueError(f"TrainConfig.norm_obs=True with algo={self.algo!r}: the reference-parity trainers "
                                 "keep the reference's raw observations; use a2c or ppo")
            if self.model == "cnn":
                raise ValueError("TrainConfig.norm_obs=True with model='cnn': its frames are already scaled by 1/255 "
                                 "in-kernel; observation normalisation is for the MLP models")
            if not self.obs_clip > 0:
                raise ValueError(f"TrainConfig.obs_clip={self.obs_clip}: must be > 0")
        if self.norm_reward:
            if self.algo in ("a3c", "basic_ac"):
                raise ValueError(f"TrainConfig.norm_reward=True with algo={self.algo!r}: the reference-parity trainers "
                                 "keep the reference's raw rewards; use a2c or ppo")
            if self.model == "cnn":
                raise ValueError("TrainConfig.norm_reward=True with model='cnn': the native A2C head computes returns "
                                 "in-kernel from the stored rewards and Atari rewards are unit-scale; reward scaling "
                                 "is for the MLP models")
            if not self.reward_clip > 0:
                raise ValueError(f"TrainConfig.reward_clip={self.reward_clip}: must be > 0")
        if self.target_kl is not None:
            if not float(self.target_kl) > 0:
                raise ValueError(f"TrainConfig.target_kl={self.target_kl}: must be > 0 (None = no early stopping)")
            if self.algo != "ppo":
                raise ValueError(f"TrainConfig.target_kl with algo={self.algo!r}: early stopping ends the remaining "
                                 "minibatch steps of a PPO update; use algo='ppo'")
            if self.engine == "native" and self.model == "cnn":
                raise ValueError("TrainConfig.target_kl with engine='native' and model='cnn': the native CNN engine "
                                 "has no early-stop gate; use engine='auto' or 'torch'")
        if int(self.eval_every) < 0:
            raise ValueError(f"TrainConfig.eval_every={self.eval_every}: must be >= 0 (updates; 0 = no evaluation)")
        if self.eval_every:
            if self.algo in ("a3c", "basic_ac"):
                raise ValueError(f"TrainConfig.eval_every with algo={self.algo!r}: the reference-parity trainers score "
                                 "policies with the reference's test loop (api.evaluate); use a2c or ppo")
            if self.model == "cnn" and str(self.device).startswith("cpu"):
                raise ValueError("TrainConfig.eval_every with model='cnn' on a CPU device: one evaluation is "
                                 "eval_episodes * max_episode_steps conv forwards of the whole bank, minutes on a "
                                 "CPU; train on a GPU, or score a checkpoint once with api.evaluate_policy")
        if int(self.eval_envs) < 1 or int(self.eval_episodes) < 1:
            raise ValueError(f"TrainConfig.eval_envs={self.eval_envs}, eval_episodes={self.eval_episodes}: both must "
                             "be >= 1")
        if not 0 <= int(self.ep_window) <= 4096:
            raise ValueError(f"TrainConfig.ep_window={self.ep_window}: must be in 0 .. 4096 (episodes; 0 = off)")
        if self.ep_window and self.algo in ("a3c", "basic_ac"):
            raise ValueError(f"TrainConfig.ep_window with algo={self.algo!r}: the reference-parity trainers keep the "
                             "reference's episode logging; use a2c or ppo")
        if self.stop_return is not None:
            if not self.ep_window:
                raise ValueError("TrainConfig.stop_return needs ep_window > 0: the threshold is compared with the mean "
                                 "return of the episode window")
            if not self.stdout_freq:
                raise ValueError("TrainConfig.stop_return needs stdout_freq > 0: the window is read where a log row is "
                                 "produced")
        for name in ("actor_hidden", "critic_hidden"):
            v = getattr(self, name)
            if v is None:
                continue
            if isinstance(v, (str, bytes)) or not hasattr(v, "__iter__"):
                raise ValueError(f"TrainConfig.{name}={v!r}: expected a sequence of hidden widths, e.g. (64, 64)")
            try:
                v = tuple(int(w) for w in v)
            except (TypeError, ValueError):
                raise ValueError(f"TrainConfig.{name}={getattr(self, name)!r}: hidden widths are integers") from None
            if not v or any(w < 1 for w in v):
                raise ValueError(f"TrainConfig.{name}={v!r}: needs at least one hidden layer, every width >= 1")
            if self.engine != "torch":
                check_mlp_tower(f"TrainConfig.{name}", v)
            setattr(self, name, v)
        if self.custom_mlp:
            if self.algo not in ("a2c", "ppo"):
                raise ValueError(f"TrainConfig.actor_hidden / critic_hidden / hidden_act / mlp_init with "
                                 f"algo={self.algo!r}: the reference-parity trainers keep the reference networks; use "
                                 "a2c or ppo")
            if self.model == "cnn":
                raise ValueError("TrainConfig.actor_hidden / critic_hidden / hidden_act / mlp_init with model='cnn': "
                                 "they configure the MLP towers; the CNN model has none")
        if self.fused_rollout_towers:
            if self.algo not in ("a2c", "ppo"):
                raise ValueError(f"TrainConfig.fused_rollout_towers=True with algo={self.algo!r}: the one-launch "
                                 "rollout belongs to the a2c / ppo trainer; use a2c or ppo")
            if self.model == "cnn":
                raise ValueError("TrainConfig.fused_rollout_towers=True with model='cnn': it selects the rollout of "
                                 "the MLP towers; the CNN model has none")
        if self.look_ahead is not None and int(self.look_ahead) < 1:
            raise ValueError(f"TrainConfig.look_ahead={self.look_ahead}: must be >= 1 (None = the whole rollout)")

    @property
    def custom_mlp(self):
        """Any MLP tower field away from "the reference towers"."""
        return (self.actor_hidden is not None or self.critic_hidden is not None or self.hidden_act is not None
                or self.mlp_init != "reference")

    def mlp_kwargs(self):
        """The tower arguments of ``models.policy.build_model``."""
        return dict(actor_hidden=self.actor_hidden, critic_hidden=self.critic_hidden, hidden_act=self.hidden_act,
                    mlp_init=self.mlp_init)

    def replace(self, **kw):
        return dataclasses.replace(self, **kw)

    def to_dict(self):
        return dataclasses.asdict(self)


PRESETS = {
    # Basic_AC/run_AC.py defaults
    "basic_ac": dict(algo="basic_ac", env="Pendulum-v0", gamma=0.98, look_ahead=40, norm_adv=True, ent_coef=0.01,
                     kl_coef=1.0, lr=0.005, critic_lr=0.001, clip_value=1.0, max_grad_norm=None,
                     kl_adaptive_lr=True, max_lr=1.0, anneal_regularizers=True, model_variant="basic",
                     optimizer="adam", device="cpu", cuda_graph=False),
    # A3C/process.py defaults
    "a3c": dict(algo="a3c", env="Pendulum-v0", gamma=0.98, look_ahead=40, norm_adv=True, ent_coef=0.01,
                kl_coef=1.0, lr=0.005, critic_lr=0.001, clip_value=0.1, max_grad_norm=None, kl_adaptive_lr=True,
                max_lr=0.1, anneal_regularizers=True, model_variant="a3c", optimizer="adam", device="cpu",
                cuda_graph=False),
    # The reference's flagship task (Pendulum-v0, README.md:18,33-37) solved by PPO-clip on the reference networks:
    # the A3C actor / critic (model_variant a3c), gamma 0.98 as the reference, one 200-step episode per
    # env per rollout (16 envs: 3200 steps, the scale of the reference's 1200-step batches), GAE(0.95), 10 epochs x
    # 8 minibatches, Adam 3e-4 with a 0.5 global-norm clip. Reaches a mean return above -200 within ~150k env steps
    # (profiles/r3_pendulum_learning.txt); the reference's own single-step KL-adaptive update is preset "a3c".
    "pendulum_ppo": dict(algo="ppo", env="Pendulum-v0", model="mlp", model_variant="a3c", num_envs=16, n_steps=200,
                         gamma=0.98, returns="gae", gae_lambda=0.95, norm_adv=True, ppo_epochs=10, ppo_minibatches=8,
                         ppo_clip=0.2, optimizer="adam", lr=3e-4, critic_lr=1e-3, ent_coef=0.0, kl_coef=0.0,
                         max_grad_norm=0.5, device="cuda", dtype="fp32"),
    # Acrobot-v1 (3-way categorical head, 6 observations, reward -1 per step until the tip swings above the bar) by
    # PPO-clip on the Basic towers: 16 envs x 128 steps, 4 epochs x 4 minibatches, Adam 1e-3 for both towers,
    # GAE(0.95), no entropy bonus. From -500 (a random policy never reaches the goal) to a mean finished-episode
    # return of -80 to -135 by update 120, 246 k env steps, on six seeds (profiles/classic_gym_envs.txt).
    "acrobot_ppo": dict(algo="ppo", env="Acrobot-v1", model="mlp", model_variant="basic", num_envs=16, n_steps=128,
                        gamma=0.99, returns="gae", gae_lambda=0.95, norm_adv=True, ppo_epochs=4, ppo_minibatches=4,
                        optimizer="adam", lr=1e-3, critic_lr=1e-3, ent_coef=0.0, device="cuda", dtype="fp32"),
    # BASELINE config 1
    "cartpole_cpu": dict(algo="a2c", env="CartPole-v1", num_envs=1, n_steps=5, gamma=0.99, model="mlp",
                         lr=1e-3, critic_lr=5e-3, norm_adv=True, device="cpu", cuda_graph=False,
                         max_grad_norm=0.5),
    # BASELINE config 2 (headline metric)
    "pong_a2c": dict(algo="a2c", env="PongNoFrameskip-v4", num_envs=32, n_steps=5, gamma=0.99, model="cnn",
                     optimizer="rmsprop", lr=7e-4, ent_coef=0.01, vf_coef=0.5, max_grad_norm=0.5,
                     device="cuda", dtype="bf16"),
    # BASELINE config 3
    "breakout_ppo": dict(algo="ppo", env="BreakoutNoFrameskip-v4", num_envs=128, n_steps=128, gamma=0.99,
                         returns="gae", gae_lambda=0.95, norm_adv=True, model="cnn", optimizer="adam", lr=2.5e-4,
                         ppo_epochs=4, ppo_minibatches=4, ppo_clip=0.1, ent_coef=0.01, vf_coef=0.5,
                         max_grad_norm=0.5, device="cuda", dtype="bf16"),
    # BASELINE config 4
    "a2c_dp8": dict(algo="a2c", env="PongNoFrameskip-v4", num_envs=32, n_steps=5, gamma=0.99, model="cnn",
                    optimizer="rmsprop", lr=7e-4, max_grad_norm=0.5, device="cuda", dtype="bf16"),
    # BASELINE config 5
    "mujoco_ppo_dp8": dict(algo="ppo", env="HalfCheetahShape-v0", num_envs=64, n_steps=256, gamma=0.99,
                           returns="gae", gae_lambda=0.95, norm_adv=True, model="mlp", optimizer="adam", lr=3e-4,
                           critic_lr=1e-3, ppo_epochs=10, ppo_minibatches=32, ppo_clip=0.2, ent_coef=0.0,
                           vf_coef=0.5, max_grad_norm=0.5, device="cuda", dtype="fp32"),
}
# the usual continuous-control networks on the same task: two tanh layers of 64 per tower, orthogonal init (custom
# towers: per-step rollout on the generic kernels, no one-launch rollout)
PRESETS["halfcheetah_ppo_tanh64"] = dict(PRESETS["mujoco_ppo_dp8"], actor_hidden=(64, 64), critic_hidden=(64, 64),
                                         hidden_act="tanh", mlp_init="orthogonal")


# ... and the same with the whole rollout (and evaluation) in one launch on the generic-tower chain
PRESETS["halfcheetah_ppo_tanh64_fused"] = dict(PRESETS["halfcheetah_ppo_tanh64"], fused_rollout_towers=True)


def preset(name, **overrides) -> TrainConfig:
    kw = dict(PRESETS[name])
    kw.update(overrides)
    return TrainConfig(**kw)
