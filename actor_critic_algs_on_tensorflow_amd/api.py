"""Public API: ``train(cfg) -> TrainResult``, ``Agent`` (batched ``act``), ``evaluate`` (the reference's
``test_process``, ``A3C/process.py:125-153``).

    import actor_critic_algs_on_tensorflow_amd as aca
    res = aca.train(aca.preset("cartpole_cpu", total_updates=2000))
    agent = aca.Agent.from_checkpoint("tests/fixtures/model-Pendulum_a3c", "Pendulum-v0")
    a, logp, ent = agent.act(obs)          # obs [N, obs_dim] -> actions [N(, A)], logp [N], entropy [N]
    aca.evaluate("tests/fixtures/model-Pendulum_a3c", "Pendulum-v0", num_episodes=3)
    aca.evaluate_policy("tests/fixtures/model-Pendulum_a3c", "Pendulum-v0", num_envs=16)   # batched, deterministic
"""
from __future__ import annotations

import dataclasses
import time

import numpy as np
import torch

from . import envs as E
from .config import TrainConfig, preset


@dataclasses.dataclass
class TrainResult:
    history: list
    iterations: int
    env_steps: int
    seconds: float
    checkpoint: str | None
    trainer: object = None

    @property
    def env_steps_per_sec(self):
        return self.env_steps / max(self.seconds, 1e-9)


def make_trainer(cfg: TrainConfig, dp=None):
    if cfg.algo == "basic_ac":
        from .algos.basic_ac import BasicACTrainer
        return BasicACTrainer(cfg)
    if cfg.algo == "a3c":
        raise ValueError("algo='a3c' runs as a multi-process job: use actor_critic_algs_on_tensorflow_amd.algos.a3c"
                         ".run(cfg) under torch.distributed (see cli/train.py)")
    from .algos.trainer import ActorCriticTrainer
    return ActorCriticTrainer(cfg, dp=dp)


def train(cfg: TrainConfig | str, **overrides) -> TrainResult:
    """Trains with a config (or preset name + overrides) on one process; returns the history and final state.

    Multi-GPU data parallelism: launch this under ``torch.distributed.run`` with ``dist_backend`` "nccl"/"gloo";
    the process group is initialised from the environment (one rank per GPU).
    """
    if isinstance(cfg, str):
        cfg = preset(cfg, **overrides)
    elif overrides:
        cfg = cfg.replace(**overrides)
    dp = None
    from .parallel import dp as DP
    rank, world, local = DP.init_from_env(cfg.dist_backend, timeout_s=cfg.dist_timeout_s)
    if world > 1:
        if cfg.device.startswith("cuda"):
            cfg = cfg.replace(device=f"cuda:{local}")
        dp = DP.DataParallel()
    tr = make_trainer(cfg, dp)
    n = None
    if cfg.resume:   # restart from the newest (or a given) checkpoint, run the remaining updates
        if cfg.algo == "basic_ac":
            raise ValueError("resume needs the vectorised trainers (the basic_ac parity loop keeps no resume state)")
        from . import ckpt
        path = ckpt.latest_checkpoint(cfg.checkpoint_dir) if cfg.resume == "auto" else cfg.resume
        if path is not None:
            tr.load_checkpoint(path)
        n = max(0, cfg.total_updates - tr.iteration)
    t0 = time.time()
    hist = tr.train(n) if n is not None else tr.train()
    if cfg.device.startswith("cuda"):
        torch.cuda.synchronize()
    dt = time.time() - t0
    ck = None
    if cfg.checkpoint_dir and cfg.save_every and (getattr(tr, "rank", 0) == 0 or getattr(tr, "dp", None) is not None):
        ck = tr.save_checkpoint()
    if hasattr(tr, "close"):
        tr.close()
    return TrainResult(hist, tr.iteration, tr.env_steps, dt, ck, tr)


class Agent:
    """A policy ready to act: wraps a model family and its device; ``act`` is batched over observations.

    On a GPU (``engine="auto"|"native"``) ``act`` runs the hand-written HIP engines the trainers use: the CNN family
    through :class:`.algos.engine.CNNEngine` (fused trunk + fc + head, bf16 MFMA) and the categorical sampling
    kernel; the MLP family through :class:`.ops.mlp.MLPEngine` (both towers + sampling in one launch). Sampling keys
    are ``(call counter << 20) + row``, so the native and the PyTorch paths draw the same actions from the same
    logits. ``engine="torch"`` (and every CPU agent) runs the PyTorch modules."""

    def __init__(self, model, env_id=None, device="cpu", seed=0, engine="auto"):
        self.model = model.to(device)
        self.model.eval()
        self.env_id = env_id
        self.device = torch.device(device)
        self.seed = seed
        self._ctr = 0
        self.engine_kind = engine
        self._eng = None
        self.obs_norm = None   # frozen ops/obs_norm.py ObsNormalizer of a norm_obs checkpoint (from_checkpoint)

    def _engine(self):
        """Lazily builds the native engine over the model's parameters (None on CPU / engine="torch")."""
        if self._eng is not None or self.engine_kind == "torch" or self.device.type != "cuda":
            return self._eng
        from .models.policy import CNNActorCritic, MLPActorCritic
        from .ops.optim import FlatParams
        from . import _native
        _native.require()
        mlp_ok = isinstance(self.model, MLPActorCritic) and self.model.actor.ac_dim <= 16
        if mlp_ok:
            # towers outside the engine's limits (a width-40 tower trained on the torch engine): native refuses, auto
            # takes the PyTorch modules -- decided before the parameters are re-homed
            from .ops.mlp import MLPEngine
            try:
                MLPEngine.check_towers(self.model)
            except ValueError:
                if self.engine_kind == "native":
                    raise
                return None
        flat = FlatParams(self.model.param_groups(), self.device)   # re-homes the parameters into one slab
        if isinstance(self.model, CNNActorCritic):
            from .algos.engine import CNNEngine
            shadow = flat.data.to(torch.bfloat16)
            self._eng = ("cnn", CNNEngine(self.model, flat, shadow), flat)
        elif mlp_ok:
            self._eng = ("mlp", MLPEngine(self.model, flat), flat)
            self._eng[1].obs_norm = self.obs_norm   # the launches normalise their input tiles
        elif self.engine_kind == "native":
            raise ValueError("no native engine for this model")
        return self._eng

    @torch.no_grad()
    def _act_native(self, o, keys_ctr, deterministic):
        from .ops import distributions as D
        kind, eng, _ = self._eng
        N = o.shape[0]
        if kind == "cnn":
            b = eng.bufs(N)
            z = eng.forward(o.to(torch.uint8).contiguous(), b)
            logits = z[:, :eng.A].contiguous()
            if deterministic:
                a = logits.argmax(-1).to(torch.int32)
                logp, ent = D.categorical_logp_entropy(logits, a)
                return a, logp, ent
            keys = torch.arange(N, dtype=torch.int64, device=self.device) + (keys_ctr << 20)
            return D.categorical_sample(logits, keys, self.seed)
        if deterministic:
            return None
        act = torch.empty((N,) if eng.discrete else (N, eng.A), dtype=torch.int32 if eng.discrete else torch.float32,
                          device=self.device)
        logp = torch.empty(N, device=self.device)
        ent = torch.empty(N, device=self.device)
        v = torch.empty(N, device=self.device)
        tg = torch.full((N,), keys_ctr, dtype=torch.int64, device=self.device)
        ids = torch.arange(N, dtype=torch.int64, device=self.device)
        eng.policy_step(o.float().contiguous(), act, logp, ent, v, tg, ids, 20, self.seed)
        return act, logp, ent

    @classmethod
    def for_env(cls, env_id, family="auto", variant="basic", frames=1, device="cpu", seed=0, **towers):
        """``towers``: ``actor_hidden`` / ``critic_hidden`` / ``hidden_act`` / ``mlp_init`` of ``build_model``."""
        from .models.policy import build_model
        env = E.make(env_id, 1, device="cpu", frame_stack=4 if ("Pong" in env_id or "Breakout" in env_id) else frames)
        return cls(build_model(env, family, variant, seed=seed, **towers), env_id, device, seed)

    @classmethod
    def from_checkpoint(cls, path, env_id, frames=1, device="cpu", variant=None):
        """Loads a TF-bundle checkpoint (reference names or this framework's)."""
        from . import ckpt
        t = ckpt.load_tensors(path)
        v = variant or ckpt.detect_variant(t.keys())
        if v == "custom" or (variant is not None and ckpt.detect_variant(t.keys()) == "custom"):
            # custom MLP towers: rebuilt from the architecture the bundle carries (_acamd/mlp_arch)
            arch = ckpt.mlp_arch(t)
            if arch is None:
                raise KeyError(f"checkpoint {path} has custom MLP tower tensors but no {ckpt.MLP_ARCH_PREFIX}* keys")
            agent = cls.for_env(env_id, family="mlp", variant=variant if variant in ("a3c", "basic") else "basic",
                                frames=frames, device="cpu", **arch)
            ckpt.check_mlp_arch(agent.model, t, path)   # (the per-tower activations the bundle records)
            ckpt.load_model(agent.model, t, "basic", strict=True)
        else:
            fam = "mlp" if v in ("a3c", "basic") else "auto"
            agent = cls.for_env(env_id, family=fam, variant=v if v != "generic" else "basic", frames=frames,
                                device="cpu")
            ckpt.load_model(agent.model, t, v if v != "generic" else "basic", strict=True)
        agent.model.to(device)
        agent.device = torch.device(device)
        sd = ckpt.obs_norm_state(t)
        if sd is not None:   # a norm_obs checkpoint: act / value normalise with its statistics, frozen
            from .ops.obs_norm import ObsNormalizer
            agent.obs_norm = ObsNormalizer(sd["mean"].numel(), float(sd["clip"]), device=agent.device)
            agent.obs_norm.load_state_dict(sd).freeze()
        return agent

    @torch.no_grad()
    def act(self, obs, deterministic=False):
        """obs ``[N, ...]`` (or a single observation) -> (action, logp, entropy) as numpy arrays."""
        o = torch.as_tensor(np.asarray(obs))
        single = o.dim() == self._obs_rank()
        if single:
            o = o.unsqueeze(0)
        o = o.to(self.device)
        N = o.shape[0]
        ctr = self._ctr
        self._ctr += 1
        res = self._act_native(o, ctr, deterministic) if self._engine() is not None else None
        if res is not None:
            a, logp, ent = res
        else:
            keys = torch.arange(N, dtype=torch.int64, device=self.device) + (ctr << 20)
            if self.obs_norm is not None:
                o = self.obs_norm.apply(o)
            a, logp, ent, _ = self.model.act(o, keys=keys, seed=self.seed, deterministic=deterministic)
        out = (a.cpu().numpy(), logp.cpu().numpy(), ent.cpu().numpy())
        return tuple(x[0] for x in out) if single else out

    def _obs_rank(self):
        from .models.policy import CNNActorCritic
        return 3 if isinstance(self.model, CNNActorCritic) else 1

    @torch.no_grad()
    def value(self, obs):
        o = torch.as_tensor(np.asarray(obs)).to(self.device)
        if o.dim() == self._obs_rank():
            o = o.unsqueeze(0)
        if self.obs_norm is not None:
            o = self.obs_norm.apply(o)
        return self.model.value(o).cpu().numpy()


def evaluate_policy(model_path, env_id, num_envs=16, episodes=1, seed=12321, frames=1, device="cpu", engine="auto",
                    variant=None, max_episode_steps=None, cuda_graph=False):
    """Batched deterministic evaluation of a saved MLP or CNN policy (``algos/evaluator.py`` Evaluator): the checkpoint
    is loaded as :meth:`Agent.from_checkpoint` does (the frozen tables of a ``norm_obs`` checkpoint included), a bank of
    ``num_envs`` envs with RNG seed ``seed`` runs ``episodes`` episodes per env under the policy's mean / arg-max
    actions, and the summary (``ret_mean``, ``ret_std``, ``ret_min``, ``ret_max``, ``len_mean``, ``episodes``) comes
    back with the per-episode arrays ``ep_ret`` / ``ep_len`` ``[num_envs, episodes]``. On a GPU (``engine="auto"`` /
    ``"native"``) the native engines run it -- the MLP engine (the MuJoCo-shaped bank in one launch) or the CNN engine
    on the Pong-shaped banks (path ``"cnn"``) --, ``engine="torch"`` and every CPU run take the PyTorch modules. The
    image banks always stack 4 frames. Stochastic evaluation is :func:`evaluate`."""
    from .algos.evaluator import Evaluator
    from .models.policy import CNNActorCritic
    if int(num_envs) < 1 or int(episodes) < 1:
        raise ValueError(f"evaluate_policy: num_envs={num_envs} and episodes={episodes} must be >= 1")
    if engine not in ("auto", "native", "torch"):
        raise ValueError(f"evaluate_policy: engine={engine!r}: expected 'auto', 'native' or 'torch'")
    agent = Agent.from_checkpoint(model_path, env_id, frames=frames, device=device, variant=variant)
    agent.engine_kind = engine
    cnn = isinstance(agent.model, CNNActorCritic)
    kw = {} if max_episode_steps is None else {"max_episode_steps": int(max_episode_steps)}
    env = E.make(env_id, int(num_envs), device=agent.device, seed=seed, frame_stack=4 if cnn else frames, **kw)
    eng = agent._engine()
    native = eng[1] if eng is not None and eng[0] == ("cnn" if cnn else "mlp") else None
    ev = Evaluator(agent.model, env, native, agent.obs_norm, int(episodes), cuda_graph=cuda_graph)
    if engine == "native" and ev.path == "torch":
        raise ValueError("evaluate_policy: engine='native' needs a GPU and an MLP model with at most 16 actions, or a "
                         "CNN model with at most 7 actions on a Pong-shaped bank")
    return ev.evaluate()


def evaluate(model_path, env_id, num_episodes=3, seed=12321, frames=1, animate=False, variant=None, verbose=True,
             max_path_length=None):
    """Runs ``num_episodes`` episodes of a saved policy, printing the reference's per-episode report."""
    agent = Agent.from_checkpoint(model_path, env_id, frames=frames, variant=variant)
    agent.seed = seed
    env = E.make(env_id, 1, device="cpu", seed=seed, frame_stack=frames)
    mpl, _ = E.get_roll_params(env_id, "a3c" if (variant or "a3c") == "a3c" else "basic")
    if max_path_length is not None:
        mpl = max_path_length
    rewards = []   # the env keeps its own time limit; mpl only bounds the loop (rollout(), run_AC.py:95)
    obs = env.reset().clone()
    for i in range(num_episodes):
        total, length = 0.0, 0
        while True:
            a, _, _ = agent.act(obs)
            a_t = torch.as_tensor(np.asarray(a)).reshape(1, *([-1] if not env.is_discrete else []))
            if env.is_discrete:
                a_t = a_t.to(torch.int32).reshape(1)
            obs_next, r, d, _ = env.step(a_t)
            total += float(r[0])
            length += 1
            obs = obs_next.clone()
            if bool(d[0]):
                break   # the bank auto-reset: obs already holds the next episode's first observation
            if length >= mpl:
                # cut by the loop bound without done: start the next episode fresh, as rollout() does with its
                # env.reset() per episode (Basic_AC/run_AC.py:88)
                obs = env.reset().clone()
                break
        rewards.append(total)
        if verbose:
            print("Iteration {}".format(i))
            print("Reward {}".format(total))
            print("Episode Length {}\n".format(length))
    avg = float(np.mean(rewards)) if rewards else float("nan")
    if verbose:
        print("Average reward over {} was {}".format(num_episodes, avg))
    return rewards
