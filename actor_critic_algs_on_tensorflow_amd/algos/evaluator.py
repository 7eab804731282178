"""Deterministic, batched, on-device evaluation of a policy (``TrainConfig.eval_every``, ``api.evaluate_policy``): the
MLP models and the Nature-CNN on the Pong-shaped banks."""
from __future__ import annotations

import numpy as np
import torch

from ..ops import evaluation as EV
from .storage import RolloutStorage

KEY_ENV_BITS = 20


def chunk_plan(L, chunk_steps):
    """``(q, tail)``: an evaluation of ``L`` steps as ``q`` replays of one captured chunk of ``chunk_steps`` steps and
    one captured tail of ``tail = L - q * chunk_steps`` steps (``0 <= tail < chunk_steps``). ``chunk_steps`` is even,
    so every chunk and the tail start on slot 0 of the two-slot observation buffer."""
    L, chunk_steps = int(L), int(chunk_steps)
    if L < 1:
        raise ValueError(f"chunk_plan: L must be >= 1, got {L}")
    if chunk_steps < 2 or chunk_steps % 2:
        raise ValueError(f"chunk_plan: chunk_steps must be even and >= 2 (every chunk starts on slot 0 of the "
                         f"two-slot observation buffer), got {chunk_steps}")
    q = L // chunk_steps
    return q, L - q * chunk_steps


class _ChunkChain:
    """The captured form of a chunked evaluation: restore, ``q`` replays of the chunk, the tail with the summary."""

    def __init__(self, head, chunk, q, tail):
        self.head, self.chunk, self.q, self.tail = head, chunk, q, tail

    def replay(self):
        self.head.replay()
        for _ in range(self.q):
            self.chunk.replay()
        self.tail.replay()


class Evaluator:
    """Scores a policy by its deterministic actions on a fixed set of start states, without leaving the device.

    Semantics (the fused, the native per-step, the CNN and the torch path all implement exactly these):

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
      ``"cnn"``: the native CNN engine (``engine`` is a :class:`CNNEngine`) on a Pong-shaped bank with a 4-frame stack,
      fewer than ``large_batch_min_b`` envs and at most 7 actions: per step the trunk + fc planes of the current
      observation (``engine.forward_eval``; the row-split trunk up to ``trunk_rows_max_b`` envs, the per-env trunk
      above) and one ``env_policy_eval_pong`` launch (arg-max of the head, env step, records written by the env's
      workgroup as its episodes end). Observations ping-pong between two slots ``[2, N, 4, 84, 84]``; activations, fc
      planes and GEMM workspace are the evaluator's own (``engine.eval_bufs``), ``engine.last_fc`` is left as found
      and the bank's ``ep_stats`` is not touched. With ``keep_steps`` (tests, debugging) every observation, action,
      reward and done is kept in a :class:`RolloutStorage` of its own (``self.storage``). Any other bank or engine
      configuration of a CNN model takes ``"torch"``.
      ``"fused"``: the native MLP engine on the MuJoCo-shaped bank it can roll out in one launch
      (``engine.supports_fused_rollout``): one ``mlp_rollout_eval`` launch writes the records. With
      ``fused_towers`` (``TrainConfig.fused_rollout_towers``) any other actor whose weights fit in LDS takes the same
      launch on its generic-tower chain (``engine.supports_rollout_towers``); one that does not fit is ``"native"``.
      ``"native"``: any other bank or tower the native MLP engine takes: ``L x`` (``policy_step(greedy=True)`` +
      ``env.step``) into an ``L``-step :class:`RolloutStorage` of its own (``self.storage``: observations, actions,
      rewards and dones are kept), then one ``eval_scan`` launch.
      ``"torch"``: no engine (CPU, ``engine="torch"``, towers the native engine refuses): ``model.act(deterministic=
      True)`` + ``env.step`` per step, then ``eval_scan_ref``. This is the oracle of the others. On an image bank
      it always runs eagerly (a whole-``L`` graph of conv modules would have far too many nodes).

    :meth:`run` enqueues one evaluation and never synchronises with the host; with ``cuda_graph`` on a GPU the first
    call runs it once eagerly and then captures it as a graph of its own (restore, launches, summary; one stream, no
    forked branches), and every call replays that graph. The ``"cnn"`` path's ``L`` is 10 000 per episode at the Pong
    bank's default limit, three launches a step, so it captures no whole-``L`` graph: three small graphs -- the
    restore, one chunk of ``chunk_steps`` steps (even, so every chunk starts on slot 0) and the tail of
    ``L - q * chunk_steps`` steps with the summary -- replayed as restore, ``q`` x chunk, tail (:func:`chunk_plan`);
    with ``keep_steps`` it runs unchunked. Everything is allocated here, outside capture. :meth:`result` does one
    host read."""

    def __init__(self, model, env, engine=None, obs_norm=None, episodes=1, cuda_graph=False, fused=True,
                 chunk_steps=64, keep_steps=False, fused_towers=False):
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
        self._towers = False   # "fused" on the generic-tower chain
        self.chunk_steps, self.keep_steps = int(chunk_steps), bool(keep_steps)
        chunk_plan(self.L, self.chunk_steps)   # refuses an odd chunk length
        from ..envs.atari import PongVecEnv
        from .engine import CNNEngine
        cnn = isinstance(engine, CNNEngine)
        if cnn and not (isinstance(env, PongVecEnv) and env.frame_stack == 4 and engine.eval_ok(self.N)):
            self.engine = engine = None   # a bank the evaluation step does not take: the torch path
        if engine is None:
            self.path = "torch"
            self.rewards = torch.zeros(self.L, self.N, dtype=torch.float32, device=self.device)
            self.dones = torch.zeros(self.L, self.N, dtype=torch.uint8, device=self.device)
        elif cnn:
            self.path = "cnn"
            self._cb, self._hp, self._ws = engine.eval_bufs(self.N)
            if self.keep_steps:
                self.storage = RolloutStorage(self.L, self.N, env.obs_shape, env.obs_dtype, (), torch.int32,
                                              self.device)
                self._obs = self.storage.obs
            else:
                self._obs = torch.zeros((2, self.N) + tuple(env.obs_shape), dtype=torch.uint8, device=self.device)
        elif fused and engine.supports_fused_rollout(env):
            self.path = "fused"
        elif fused and fused_towers and engine.supports_rollout_towers(env):
            self.path, self._towers = "fused", True
        else:
            self.path = "native"
            act_shape = () if env.is_discrete else tuple(env.action_space.shape)
            act_dtype = torch.int32 if env.is_discrete else torch.float32
            self.storage = RolloutStorage(self.L, self.N, env.obs_shape, env.obs_dtype, act_shape, act_dtype,
                                          self.device)
        self._want_graph = bool(cuda_graph) and self.device.type == "cuda"
        if self.path == "torch" and env.obs_dtype == torch.uint8:
            self._want_graph = False   # conv modules x L steps: far too many nodes for one graph; runs eagerly
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
        if self.path == "cnn":
            self._obs[0].copy_(self.obs0)
        self.rec.clear()

    @torch.no_grad()
    def run_eager(self):
        self.restore()
        getattr(self, "_run_" + self.path)()
        self._finish()

    @torch.no_grad()
    def _finish(self):
        """Summary and the packed host-read buffer from the records."""
        self.rec.summarize()
        rec = self.rec
        torch.cat([rec.summary, rec.ep_ret.reshape(-1).to(torch.float64), rec.ep_len.reshape(-1).to(torch.float64),
                   rec.cnt.to(torch.float64)], out=self._packed)

    def _run_fused(self):
        self.engine.rollout_eval_linear(self.env, self.obs0, self.L, self.rec, towers=self._towers)

    def _run_native(self):
        st, env, eng = self.storage, self.env, self.engine
        st.obs[0].copy_(self.obs0)
        for t in range(self.L):
            eng.policy_step(st.obs[t], st.actions[t], st.logp[t], st.entropy[t], st.values[t], env.tg, env.env_ids,
                            KEY_ENV_BITS, 0, greedy=True)
            env.step(st.actions[t], prev_obs=st.obs[t], obs_out=st.obs[t + 1], reward_out=st.rewards[t],
                     done_out=st.dones[t], trunc_out=st.truncated[t])
        EV.eval_scan(st.rewards, st.dones, *self.rec.tensors())

    def _run_cnn(self):
        self._cnn_steps(0, self.L)

    @torch.no_grad()
    def _cnn_steps(self, t0, n):
        """Steps ``t0 .. t0 + n - 1``: step ``t`` reads its observation from slot ``t`` (``keep_steps``) or ``t & 1``
        and writes the next one into slot ``t + 1`` or ``1 - (t & 1)``."""
        from .. import _native
        ops, env, eng, st = _native.require(), self.env, self.engine, self.storage
        for t in range(t0, t0 + n):
            p = t if st is not None else t & 1
            src, dst = self._obs[p], self._obs[p + 1 if st is not None else 1 - p]
            shifted, S = eng.forward_eval(src, self._cb, dst, self._hp, self._ws)
            cols = (st.actions[t], st.rewards[t], st.dones[t]) if st is not None else (None, None, None)
            ops.env_policy_eval_pong(None, eng.sWh, eng.bh, env.state, env.t, env.tg, env.ep_ret, env.env_ids, src,
                                     dst, env.seed, env.max_episode_steps, env.frame_stack, shifted, self._hp, S,
                                     eng.bfc, *self.rec.tensors(), self.episodes, *cols)

    def _capture_chunks(self):
        """The chunked form of one evaluation as three graphs (no launch runs during capture)."""
        q, tail = chunk_plan(self.L, self.chunk_steps)

        def cap(fn):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, capture_error_mode="thread_local"):
                fn()
            return g

        head = cap(self.restore)
        chunk = cap(lambda: self._cnn_steps(0, self.chunk_steps)) if q else None

        def last():
            self._cnn_steps(q * self.chunk_steps, tail)
            self._finish()
        return _ChunkChain(head, chunk, q, cap(last))

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
            if self.path == "cnn" and not self.keep_steps:
                self.graph = self._capture_chunks()
            else:
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
