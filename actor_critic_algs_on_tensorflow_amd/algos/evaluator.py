"""Deterministic, batched, on-device evaluation of an MLP policy (``TrainConfig.eval_every``,
``api.evaluate_policy``)."""
from __future__ import annotations

import numpy as np
import torch

from ..ops import evaluation as EV
from .storage import RolloutStorage

KEY_ENV_BITS = 20


class Evaluator:
    """Scores a policy by its deterministic actions on a fixed set of start states, without leaving the device.

    Semantics (the fused, the native per-step and the torch path all implement exactly these):

    Evaluation bank
      ``env`` is a bank of its own, separate from any training bank (the trainer builds it with the training bank's env
      id, ``frames`` and ``max_episode_steps``, ``eval_envs`` envs and RNG seed ``eval_seed``). It is reset once, here
      (``tg = 0``), and a snapshot is kept of ``state``, ``t``, ``tg``, ``ep_ret`` and the first observation stack.

    Start of every evaluation
      Every evaluation first restores the snapshot with device-side copies, so an evaluation is a pure function of
      (parameters, observation-normaliser tables, the bank's seed). The bank's state never persists and is not
      checkpointed.

    Actions
      Gaussian head: ``a = tanh(y) * ac_scale``, the mean; categorical head: the first index of the largest logit
      (``torch.argmax``'s tie rule) -- what ``model.act(deterministic=True)`` returns. No random number is drawn for
      the policy (the bank's own dynamics and resets keep their counter draws).

    Step budget and records
      The bank runs ``L = episodes * max_episode_steps`` steps. The first ``episodes`` finished episodes of each env
      are recorded, later ones ignored; the budget guarantees that every env finishes that many. Records: ``ep_ret
      [N][E]`` float32, ``ep_len [N][E]`` int32, ``cnt [N]`` int32. An episode's return is the fp32 sum of its rewards
      in step order, the bank's ``ep_ret`` arithmetic. Rewards are raw: ``norm_reward`` does not touch them.

    Normaliser
      With an observation normaliser the towers read its tables as they stand at that moment; evaluation observations
      are never merged into them.

    Summary
      fp64 over the records in ``[N][E]`` order with a handful of torch ops (``ops/evaluation.py`` summarize): mean,
      population standard deviation, minimum and maximum of the returns, mean length, episode count. The host read
      (:meth:`result`) asserts ``cnt == E`` everywhere.

    Side effects
      None on training: nothing a trainer reads is written (its storage, bank, parameters, fragment copies, optimiser
      and normaliser state are bit-identical with and without evaluations).

    Paths (``self.path``)
      ``"fused"``: the native MLP engine on the MuJoCo-shaped bank it can roll out in one launch
      (``engine.supports_fused_rollout``): one ``mlp_rollout_eval`` launch writes the records.
      ``"native"``: any other bank or tower the native MLP engine takes: ``L x`` (``policy_step(greedy=True)`` +
      ``env.step``) into an ``L``-step :class:`RolloutStorage` of its own (``self.storage``: observations, actions,
      rewards and dones are kept), then one ``eval_scan`` launch.
      ``"torch"``: no engine (CPU, ``engine="torch"``, towers the native engine refuses): ``model.act(deterministic=
      True)`` + ``env.step`` per step, then ``eval_scan_ref``. This is the oracle of the other two.

    :meth:`run` enqueues one evaluation and never synchronises with the host; with ``cuda_graph`` on a GPU the first
    call runs it once eagerly and then captures it as a graph of its own (restore, launches, summary; one stream, no
    forked branches), and every call replays that graph. Everything is allocated here, outside capture.
    :meth:`result` does one host read."""

    def __init__(self, model, env, engine=None, obs_norm=None, episodes=1, cuda_graph=False, fused=True):
        self.model, self.env, self.engine, self.obs_norm = model, env, engine, obs_norm
        self.episodes = int(episodes)
        if self.episodes < 1:
            raise ValueError(f"Evaluator: episodes must be >= 1, got {episodes}")
        if env.max_episode_steps is None or int(env.max_episode_steps) < 1:
            raise ValueError("Evaluator: the evaluation bank needs a time limit (max_episode_steps >= 1)")
        self.device = env.device
        self.N = env.num_envs
        self.L = self.episodes * int(env.max_episode_steps)
        self.rec = EV.EvalRecords(self.N, self.episodes, self.device)
        env.reset()
        self._snap = {k: getattr(env, k).clone() for k in ("state", "t", "tg", "ep_ret")}
        self.obs0 = env.obs.clone()
        self.storage = None
        if engine is not None and fused and engine.supports_fused_rollout(env):
            self.path = "fused"
        elif engine is not None:
            self.path = "native"
            act_shape = () if env.is_discrete else tuple(env.action_space.shape)
            act_dtype = torch.int32 if env.is_discrete else torch.float32
            self.storage = RolloutStorage(self.L, self.N, env.obs_shape, env.obs_dtype, act_shape, act_dtype,
                                          self.device)
        else:
            self.path = "torch"
            self.rewards = torch.zeros(self.L, self.N, dtype=torch.float32, device=self.device)
            self.dones = torch.zeros(self.L, self.N, dtype=torch.uint8, device=self.device)
        self._want_graph = bool(cuda_graph) and self.device.type == "cuda"
        self.graph = None
        self._packed = torch.zeros(len(EV.SUMMARY_KEYS) + 2 * self.N * self.episodes + self.N, dtype=torch.float64,
                                   device=self.device)

    # ------------------------------------------------------------------------------------------- one evaluation
    def restore(self):
        """The bank back at its snapshot and the records at their sentinels (device-side copies and fills)."""
        env = self.env
        for k, v in self._snap.items():
            getattr(env, k).copy_(v)
        env.obs.copy_(self.obs0)
        self.rec.clear()

    @torch.no_grad()
    def run_eager(self):
        self.restore()
        getattr(self, "_run_" + self.path)()
        self.rec.summarize()
        rec = self.rec
        torch.cat([rec.summary, rec.ep_ret.reshape(-1).to(torch.float64), rec.ep_len.reshape(-1).to(torch.float64),
                   rec.cnt.to(torch.float64)], out=self._packed)

    def _run_fused(self):
        self.engine.rollout_eval_linear(self.env, self.obs0, self.L, self.rec)

    def _run_native(self):
        st, env, eng = self.storage, self.env, self.engine
        st.obs[0].copy_(self.obs0)
        for t in range(self.L):
            eng.policy_step(st.obs[t], st.actions[t], st.logp[t], st.entropy[t], st.values[t], env.tg, env.env_ids,
                            KEY_ENV_BITS, 0, greedy=True)
            env.step(st.actions[t], prev_obs=st.obs[t], obs_out=st.obs[t + 1], reward_out=st.rewards[t],
                     done_out=st.dones[t], trunc_out=st.truncated[t])
        EV.eval_scan(st.rewards, st.dones, *self.rec.tensors())

    def _run_torch(self):
        env, model = self.env, self.model
        for t in range(self.L):
            obs = env.obs if self.obs_norm is None else self.obs_norm.apply(env.obs)
            a = model.act(obs, deterministic=True)[0]
            env.step(a, reward_out=self.rewards[t], done_out=self.dones[t])
        EV.eval_scan_ref(self.rewards, self.dones, *self.rec.tensors())

    def run(self):
        """Enqueues one evaluation; no host sync."""
        if not self._want_graph:
            self.run_eager()
            return
        if self.graph is None:
            self.run_eager()   # warm-up outside capture (kernel attributes, lazily built descriptors)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, capture_error_mode="thread_local"):
                self.run_eager()
            self.graph = g
        self.graph.replay()

    # ------------------------------------------------------------------------------------------- host read
    def result(self):
        """One host read: the summary (``SUMMARY_KEYS`` of ``ops/evaluation.py``) and the per-episode arrays ``ep_ret``
        ``[N, E]`` float32, ``ep_len`` ``[N, E]`` int32, ``cnt`` ``[N]`` int32."""
        p = self._packed.cpu().numpy()
        K, NE = len(EV.SUMMARY_KEYS), self.N * self.episodes
        out = {k: float(p[i]) for i, k in enumerate(EV.SUMMARY_KEYS)}
        out["episodes"] = int(out["episodes"])
        cnt = p[K + 2 * NE:].astype(np.int32)
        if not (cnt == self.episodes).all():
            raise RuntimeError(f"Evaluator: every env must record {self.episodes} episodes in {self.L} steps, got "
                               f"counts {cnt.tolist()}")
        out["ep_ret"] = p[K:K + NE].astype(np.float32).reshape(self.N, self.episodes)
        out["ep_len"] = p[K + NE:K + 2 * NE].astype(np.int32).reshape(self.N, self.episodes)
        out["cnt"] = cnt
        out["path"] = self.path
        return out

    def evaluate(self):
        """:meth:`run` + :meth:`result`."""
        self.run()
        return self.result()
