"""Native engine for the reference's MLP actor-critic (kernels K01/K02/K05/K07/K08 of SURVEY §2.4, ``mlp.hip``).

The reference builds its actor and critic as separate TF graphs (``Basic_AC/policies.py:33-162``,
``A3C/policies.py:34-182``) and runs each ``Session.run`` as ~10 TF ops per layer. Here each tower is ONE workgroup
per 16 rows with its activations in LDS, on f32 MFMA:

* :meth:`MLPEngine.policy_step` -- rollout: both towers in one launch; the actor workgroups also sample the action
  (Gaussian Box-Muller / categorical Gumbel-max, counter-based keys derived from the env counters, so the actions are
  bit-identical to :func:`..ops.distributions.gaussian_sample_ref` draws), and write log-prob and entropy; the critic
  workgroups write V(s).
* :meth:`MLPEngine.train` -- learner (mini)batch: one fused launch (gathered rows -> forward -> per-row loss gradient
  -> data-gradient chain) + one weight-gradient launch (every dW/db element written once, deterministic; per-tile
  sums of squares for the global-norm clip; loss statistics). The optimiser step follows (:mod:`.optim`).
* :meth:`MLPEngine.evaluate` / :meth:`value` -- log-prob / entropy of given actions and values (post-update KL proxy
  and EV of the reference, ``Basic_AC/run_AC.py:257-258``; bootstrap values).
* :meth:`MLPEngine.rollout_linear` -- the whole T-step rollout of the MuJoCo-shaped bank in ONE persistent launch
  (actor on 4x4x1 MFMA tiles + sampling + env dynamics + frame stack per 4-env workgroup, ``mlp_rollout_kernel``) followed by ONE
  batched critic launch over all ``(T+1) N`` observations (the rollout's Session.run-per-step loop of
  ``Basic_AC/run_AC.py:82-107``). With a :class:`TimeoutBootWorkspace` the same launch also keeps the terminal
  observation of every step the time limit cut, in :func:`timeout_slots` compact slots per env; one more critic launch
  over those ``N S`` stacks and one fix-up launch (``ops/returns.py`` ``timeout_bootstrap_``) then add
  ``gamma V(terminal observation)`` to the truncated steps' rewards (``TrainConfig.bootstrap_on_timeout``).
* :meth:`MLPEngine.rollout_eval_linear` -- the deterministic evaluation of that bank in ONE launch (the ``EVAL``
  instantiations of ``mlp_rollout_kernel``: the actor's mean, no noise, nothing stored per step, episode records
  written as episodes end); ``policy_step(greedy=True)`` is the per-step form for every other bank
  (``algos/evaluator.py``).

Weights are read in place from the fp32 parameter slab (TF ``[in, out]`` kernels, so checkpoints need no
transposes) and gradients are written straight into the gradient slab.
"""
from __future__ import annotations

import torch

from .. import _native

MAXL = 5
TOWER_WORDS = 2 + 11 * MAXL    # int64 words of one MlpTower (csrc/kernels/mlp_desc.h)
ACT_CODES = {None: 0, "none": 0, "relu": 1, "lrelu": 2, "tanh": 3}
BM = 16
MAXW = 256
PARTS = 256
MPART_W = 24    # per-workgroup partial row of the train kernel (mlp_desc.h)
LIN_OBS, LIN_ACT = 17, 6


def ngp2(w):
    """16-wide groups of a width rounded up to a power of two (common.h mlp_ngp2)."""
    g = (w + 15) // 16
    return 1 if g <= 1 else 2 if g <= 2 else 4 if g <= 4 else 8 if g <= 8 else 16


def _ld(w):
    """LDS row stride of a width (mlp.hip ld_of: 16 * power-of-two k-groups + 4)."""
    return 16 * ngp2(w) + 4


def _nct(w):
    """16-wide column tiles of a width (the training workspace's blocks per row tile)."""
    return (w + 15) // 16


def frag_f(W):
    """Forward fragment copy of a [K][N] weight (common.h mlp_frag_f): [ngp2(N) tiles][ngp2(K) groups][64 lanes][4],
    zero pad -- the layout the optimiser step and ``mlp_tshadow`` write."""
    K, N = W.shape
    gk, tn = ngp2(K), ngp2(N)
    P = torch.zeros(16 * gk, 16 * tn, dtype=W.dtype, device=W.device)
    P[:K, :N] = W
    # (tile, r) = c, (g, q, s) = k: element at ((tile * gk + g) * 64 + q * 16 + r) * 4 + s
    return P.reshape(gk, 4, 4, tn, 16).permute(3, 0, 1, 4, 2).reshape(-1)


def frag_g(W):
    """Data-gradient fragment copy of a [K][N] weight (common.h mlp_frag_g): [ngp2(K) tiles][ngp2(N) groups][64][4]."""
    return frag_f(W.t())


def timeout_slots(T, max_steps):
    """Terminal-observation slots per env of a T-step fused rollout: an env enters with ``t0 < max_steps`` steps of
    its episode behind it and is truncated ``floor((t0 + T) / max_steps) <= ceil(T / max_steps)`` times."""
    T, max_steps = int(T), int(max_steps)
    if T < 1 or max_steps < 1:
        raise ValueError(f"timeout_slots needs T >= 1 and max_steps >= 1, got {T}, {max_steps}")
    return (T + max_steps - 1) // max_steps


class TimeoutBootWorkspace:
    """Device buffers of the fused rollout's time-limit bootstrap (:meth:`MLPEngine.rollout_linear`): ``final_obs``
    ``[N, S, D]``, the terminal observation stacks; ``final_step`` int32 ``[N, S]``, the step of every slot (``-1``:
    unused; the rollout launch writes every entry); ``final_v`` ``[N, S]``, the critic's values of the slots; ``gamma``,
    the trainer's discount. ``S = timeout_slots(T, max_steps)``. Create outside any graph capture."""

    def __init__(self, T, N, D, max_steps, gamma, device):
        self.T, self.N, self.D, self.max_steps = int(T), int(N), int(D), int(max_steps)
        self.S = timeout_slots(T, max_steps)
        self.gamma = float(gamma)
        self.final_obs = torch.zeros(self.N, self.S, self.D, dtype=torch.float32, device=device)
        self.final_step = torch.full((self.N, self.S), -1, dtype=torch.int32, device=device)
        self.final_v = torch.zeros(self.N, self.S, dtype=torch.float32, device=device)

    def fits(self, T, N, D, max_steps):
        return (self.T, self.N, self.D, self.max_steps) == (int(T), int(N), int(D), int(max_steps))


class MLPEngine:
    def __init__(self, model, flat):
        from ..models.policy import MLPActorCritic
        if not isinstance(model, MLPActorCritic):
            raise ValueError(f"MLPEngine needs an MLPActorCritic, got {type(model).__name__}")
        self.model = model
        self.flat = flat
        self.dev = flat.data.device
        actor, critic = model.actor, model.critic
        self.discrete = model.discrete
        self.D = actor.ob_dim
        self.A = actor.ac_dim
        self.head = 1 if self.discrete else 2
        if self.A > 16:
            raise ValueError("MLP engine heads support at most 16 actions")
        self.towers = self.check_towers(model)
        self.hidden_tanh = [any(l.activation == "tanh" for l in tw[:-1]) for tw in self.towers]
        idx = {id(p): i for i, p in enumerate(flat.params)}

        def views(p):
            i = idx[id(p)]
            off, n = flat.offsets[i], p.numel()
            return flat.data[off:off + n], flat.grad[off:off + n]

        self._views = views
        if not self.discrete:
            self.log_std, self.g_log_std = views(actor.log_std)
            self.ac_scale = actor.ac_scale.to(self.dev, torch.float32).contiguous()
        else:
            self.log_std = self.g_log_std = self.ac_scale = None
        self.mstats = torch.zeros(8, dtype=torch.float32, device=self.dev)
        self.parts = [torch.zeros(PARTS, dtype=torch.float32, device=self.dev) for _ in range(2)]
        self.items = [sum(((l.in_features + 15) // 16) * ((l.out_features + 15) // 16) for l in tw)
                      for tw in self.towers]
        self._descs = {}
        self._hdescs = {}
        self._witems = {}
        self._mparts = {}
        self._dummy_stats = torch.zeros(16, dtype=torch.float32, device=self.dev)
        # fp32 FRAGMENT copies of every weight (common.h mlp_frag_f / mlp_frag_g, zero pad): F, the forward's B
        # operand, for every layer; G, the data gradient's, for layers >= 1 (layer 0 has no data gradient)
        self.F, self.G = {}, {}
        for tw in self.towers:
            for i, lay in enumerate(tw):
                n = ngp2(lay.in_features) * ngp2(lay.out_features) * 256
                self.F[id(lay)] = torch.zeros(n, dtype=torch.float32, device=self.dev)
                if i:
                    self.G[id(lay)] = torch.zeros(n, dtype=torch.float32, device=self.dev)
        self.n_weights = sum(l.in_features * l.out_features for tw in self.towers for l in tw)
        # reference tower widths: the train launches take the SPEC path (every weight fragment preloaded, mlp.hip). Its
        # activations are the slope form (relu / lrelu, read from the descriptor at run time): no hidden tanh
        self.spec = ([l.out_features for l in self.towers[0][:-1]] == [128, 128, 64]
                     and [l.out_features for l in self.towers[1][:-1]] == [256, 128] and self.D <= 64
                     and not any(self.hidden_tanh))
        # optional running observation normaliser (ops/obs_norm.py ObsNormalizer): when attached, policy_step, value,
        # evaluate and rollout_linear take RAW observations and normalise them as their input tiles are written;
        # train reads whatever it is given (the trainer feeds it the pre-normalised plane)
        self.obs_norm = None
        # tests and the microbench only: run every one-launch rollout / evaluation on the generic-tower chain, the
        # reference actor's too (where it is bitwise equal to the register-resident chain)
        self._force_rollout_towers = False
        self.sync_shadow()

    @staticmethod
    def check_towers(model):
        """The two towers' layers in forward order, [actor, critic], after the engine's limits: every violation is a
        ``ValueError`` that names the tower and the limit (``config.check_mlp_tower``)."""
        actor, critic = model.actor, model.critic
        D, discrete = actor.ob_dim, model.discrete
        # the layers each forward reads, in order (models/mlp.py: reference or custom towers alike)
        towers = [list(actor.hidden_layers) + [actor.out_layer], list(critic.hidden_layers) + [critic.out_layer]]
        from ..config import check_mlp_tower
        for name, tw in zip(("actor_hidden", "critic_hidden"), towers):
            if tw[0].in_features != D or any(b.in_features != a.out_features for a, b in zip(tw, tw[1:])):
                raise ValueError(f"MLPEngine: the {name[:-7]} tower's layers do not chain from the observation width "
                                 f"{D}: {[(l.in_features, l.out_features) for l in tw]}")
            for lay in tw[:-1]:
                if lay.activation not in ("tanh", "relu", "lrelu"):
                    raise ValueError(f"MLPEngine: hidden_act={lay.activation!r} on the {name[:-7]} tower: the kernels "
                                     "have tanh, relu and lrelu")
            # 1..4 hidden layers, widths 1..256 (above 32: multiples of 16 -- vectorised data-gradient weight loads,
            # mlp.hip), the sum-of-squares slots and the LDS of the generic kernel
            check_mlp_tower(f"MLPEngine: {name}", [l.out_features for l in tw[:-1]], D, tw[-1].out_features,
                            extra_slots=int(name == "actor_hidden" and not discrete))
        return towers

    def frag_copies(self):
        """Per tower (= optimiser group actor, critic): (W view, K, N, F, G or None) -- the fragment copies the
        optimiser step writes as it goes (``ops/optim.py`` FusedGroupStep item tables)."""
        return [[(self._views(l.kernel)[0], l.in_features, l.out_features, self.F[id(l)], self.G.get(id(l)))
                 for l in tw] for tw in self.towers]

    def sync_shadow(self):
        """Rewrites the weight fragment copies from the fp32 slab (the optimiser step writes them itself; this pass
        covers engine creation and parameter changes outside it: checkpoint load, broadcast, parameter-server pull)."""
        desc, _ = self.desc(None)
        _native.require().mlp_tshadow(desc, 2, self.n_weights)

    # ------------------------------------------------------------------------------------------- descriptors
    def desc(self, B=None):
        """Device descriptor (+ training workspace for batch ``B``; ``None`` = inference only)."""
        if B in self._descs:
            return self._descs[B]
        words = torch.zeros(2 * TOWER_WORDS, dtype=torch.int64)
        ws = []
        for t, tw in enumerate(self.towers):
            base = t * TOWER_WORDS
            words[base] = len(tw)
            for l, lay in enumerate(tw):
                W, gW = self._views(lay.kernel)
                b, gb = self._views(lay.bias)
                words[base + 2 + l] = lay.in_features
                words[base + 2 + MAXL + l] = lay.out_features
                words[base + 2 + 2 * MAXL + l] = ACT_CODES[lay.activation]
                for j, tns in enumerate((W, b, gW, gb)):
                    words[base + 2 + (3 + j) * MAXL + l] = tns.data_ptr()
                words[base + 2 + 9 * MAXL + l] = self.F[id(lay)].data_ptr()
                if id(lay) in self.G:
                    words[base + 2 + 10 * MAXL + l] = self.G[id(lay)].data_ptr()
                if B is not None:
                    # 16 x 16 blocks, column-major inside (mlp.hip blk_out), one row of blocks per 16-row tile
                    nrt = (B + BM - 1) // BM
                    xs = torch.zeros(nrt * _nct(lay.in_features) * 256, dtype=torch.float32, device=self.dev)
                    dp = torch.zeros(nrt * _nct(lay.out_features) * 256, dtype=torch.float32, device=self.dev)
                    ws += [xs, dp]
                    words[base + 2 + 7 * MAXL + l] = xs.data_ptr()
                    words[base + 2 + 8 * MAXL + l] = dp.data_ptr()
        # the launches' hidden_tanh flag (the launcher's choice of instantiation) must say what these very words say:
        # the descriptor lives on the device, where the launcher cannot read it back
        said = any(int(words[t * TOWER_WORDS + 2 + 2 * MAXL + l]) == ACT_CODES["tanh"]
                   for t, tw in enumerate(self.towers) for l in range(len(tw) - 1))
        if said != any(self.hidden_tanh):
            raise ValueError("MLPEngine: the descriptor's hidden activations and hidden_tanh disagree")
        d = (words.to(self.dev), ws)
        self._descs[B] = d
        self._hdescs[B] = words   # CPU copy: the SPEC train path takes the tower descriptors as kernel arguments
        return d

    def lds_bytes(self, mode, tw_base, ntw):
        best = 0
        for t in range(tw_base, tw_base + ntw):
            n = BM * _ld(self.D)
            for lay in self.towers[t]:
                n += BM * _ld(lay.out_features)
            if mode == 2:
                n += 2 * BM * (MAXW + 4)
            best = max(best, n)
        return best * 4

    def _mpart(self, B):
        """Per-workgroup partial rows of the train kernel (loss statistics + log-std gradient), summed by the
        weight-gradient kernel -- no same-address atomics from every workgroup."""
        if B not in self._mparts:
            self._mparts[B] = torch.zeros((B + BM - 1) // BM * MPART_W, dtype=torch.float32, device=self.dev)
        return self._mparts[B]

    def _fwd(self, mode, obs, B, tw_base=0, ntw=2, desc_B=None, idx=None, perm=None, tg=None, env_ids=None, key_shift=0,
             seed=0, act_out=None, logp_out=None, ent_out=None, v_out=None, act_in=None, logp_old=None, adv=None,
             ret=None, v_old=None, ent_coef=None, kl_coef=None, vf_coef=1.0, ppo_clip=0.0, v_clip=0.0, ppo=False,
             stamps=None, go=None, greedy=False):
        ops = _native.require()
        desc, _ = self.desc(desc_B)
        obs2 = obs.reshape(obs.shape[0], -1)
        puc, pep, poff, pn, pseed = perm if perm is not None else (None, 0, 0, 0, 0)
        tables, nclip = self.obs_norm.kernel_args() if (self.obs_norm is not None and mode != 2) else (None, 0.0)
        ops.mlp_fwd(desc, tw_base, ntw, mode, self.lds_bytes(mode, tw_base, ntw), obs2, idx, puc, pep, poff, pn,
                    pseed, B, self.head, self.A,
                    self.log_std, self.ac_scale, tg, env_ids, key_shift, seed, act_out, logp_out, ent_out, v_out,
                    act_in, logp_old, adv, ret, v_old, ent_coef, kl_coef, float(vf_coef), float(ppo_clip),
                    float(v_clip or 0.0), bool(ppo), self.g_log_std if mode == 2 else None,
                    self.mstats if mode == 2 else None, self._mpart(B) if mode == 2 else None, stamps,
                    self._hdescs[desc_B] if (mode == 2 and self.spec) else None, tables, nclip, go, bool(greedy),
                    any(self.hidden_tanh))

    # ------------------------------------------------------------------------------------------- API
    def policy_step(self, obs, act_out, logp_out, ent_out, v_out, tg, env_ids, key_shift, seed, greedy=False):
        """Rollout step over the env bank: actions, log-probs, entropies and values in one launch. ``greedy``: the
        deterministic action instead of a sample -- the Gaussian mean ``tanh(y) * ac_scale`` / the first index of the
        largest logit (``model.act(deterministic=True)``); no random number is drawn (``tg``, ``env_ids``, ``seed``
        are not read), the log-prob is that action's, entropy and value are unchanged."""
        self._fwd(0, obs, obs.shape[0], 0, 2, tg=tg, env_ids=env_ids, key_shift=key_shift, seed=seed,
                  act_out=act_out, logp_out=logp_out, ent_out=ent_out, v_out=v_out, greedy=greedy)

    def value(self, obs, out):
        self._fwd(1, obs, obs.shape[0], 1, 1, v_out=out)
        return out

    def evaluate(self, obs, actions, logp_out, ent_out=None, v_out=None):
        self._fwd(1, obs, obs.shape[0], 0, 2 if v_out is not None else 1, act_in=actions, logp_out=logp_out,
                  ent_out=ent_out, v_out=v_out)

    def train(self, obs, actions, logp_old, adv, ret, ent_coef, kl_coef, B, idx=None, v_old=None, vf_coef=1.0,
              ppo=False, ppo_clip=0.0, v_clip=0.0, stats=None, clips=(None, None), want_parts=True, perm=None,
              bump=None, stamps=None, kl_stat=None, go=None, kl_thr=0.0, kl_trace=None, kl_step=0):
        """One learner (mini)batch: rows ``idx`` / ``perm`` = (update_counter, epoch, offset, n, seed) -- the rows
        ``prp(offset + r)`` of the keyed permutation of ``[0, n)`` (envs/rng.py), computed in-kernel -- or the first
        ``B`` rows of the rollout -> gradients in the slab, statistics into ``stats[0:7]``, sums of squares into
        :attr:`parts` (when ``want_parts``). ``bump``: an int64 counter the weight-gradient launch advances by one
        (the PPO update counter, after the update's last minibatch -- no separate launch).

        PPO early stopping (``TrainConfig.target_kl``): ``kl_stat`` (fp32 [2]) receives the minibatch's ``approx_kl =
        mean(expm1(logp - logp_old) - (logp - logp_old))`` and, with ``go``, the steps applied so far; ``go`` (int32
        [flag, steps, stop_at]): while the flag is 1, ``approx_kl > kl_thr`` stores 0 into it and ``kl_step`` (this
        step's index within the update) into ``stop_at``, otherwise ``steps`` goes up by one; while it is 0 both
        launches write nothing but ``kl_trace = -1`` (and the ``bump``): the train launch and the bookkeeping read the
        flag, the weight-gradient items ``stop_at < kl_step``. ``kl_trace`` (one
        fp32 slot) receives ``approx_kl``. The caller gates the optimiser launch on the same flag
        (``FusedAdam.set_gate``) and re-arms it (``mlp_epoch_gather``)."""
        ops = _native.require()
        self._fwd(2, obs, B, 0, 2, desc_B=B, idx=idx, perm=perm, act_in=actions, logp_old=logp_old, adv=adv, ret=ret,
                  v_old=v_old, ent_coef=ent_coef, kl_coef=kl_coef, vf_coef=vf_coef, ppo_clip=ppo_clip,
                  v_clip=v_clip, ppo=ppo, stamps=stamps, go=go)
        nrt = (B + BM - 1) // BM
        nsplit = self.wgrad_nsplit(B)
        self.last_stores_all = nsplit == 1   # every gradient element stored (no atomics): no zeroing needed after use
        use_parts = want_parts and nsplit == 1
        st = stats if stats is not None else self._dummy_stats
        items = self.wgrad_items(B, use_parts, clips)
        ls_part = self.parts[0][self.items[0]:self.items[0] + 1] if (use_parts and self.g_log_std is not None) else None
        ops.mlp_wgrad(items, nrt, nsplit, self.g_log_std, self.A, ls_part, float(clips[0] or -1.0), st, ent_coef,
                      kl_coef, self._mpart(B), nrt, bump, kl_stat, go, float(kl_thr), kl_trace,
                      int(kl_step))
        return use_parts

    @staticmethod
    def wgrad_nsplit(B):
        """Row-tile splits of the weight-gradient launch for a batch of ``B`` rows: above 1 (from 4096 rows) the splits
        ADD their tiles into the gradient slab instead of storing them."""
        return max(1, min(16, (B + BM - 1) // BM // 128))

    def wgrad_items(self, B, parts=True, clips=(None, None)):
        """Item table of the weight-gradient launch (``mlp.hip`` mlp_wgrad_kernel, 8 int64 per 16 x 16 tile of every
        dW_l): operand block bases and strides, the gradient tile, its bias (first row of tiles), its sum-of-squares
        slot in :attr:`parts` and the clip applied before squaring; item 0 of a tower zeroes the tower's unused
        slots."""
        key = (B, bool(parts), clips)
        if key in self._witems:
            return self._witems[key]
        _, ws = self.desc(B)
        import struct
        recs = []
        wi = 0
        for t, tw in enumerate(self.towers):
            clip = float(clips[t] or -1.0)
            cbits = struct.unpack("<i", struct.pack("<f", clip))[0] & 0xFFFFFFFF
            local = 0
            first_unused = self.items[t] + (1 if t == 0 and self.g_log_std is not None else 0)
            for lay in tw:
                xs, dp = ws[wi], ws[wi + 1]
                wi += 2
                K, N = lay.in_features, lay.out_features
                gW = self._views(lay.kernel)[1]
                gb = self._views(lay.bias)[1]
                sx, sp = _nct(K) * 256, _nct(N) * 256
                for ti in range(_nct(K)):
                    for tj in range(_nct(N)):
                        ni, nj = min(16, K - 16 * ti), min(16, N - 16 * tj)
                        slot = self.parts[t].data_ptr() + 4 * local if parts else 0
                        zf = first_unused if (parts and local == 0) else 0
                        recs.append([xs.data_ptr() + 4 * 256 * ti, dp.data_ptr() + 4 * 256 * tj, sx | (sp << 32),
                                     ni | (nj << 8) | (N << 32), gW.data_ptr() + 4 * (16 * ti * N + 16 * tj),
                                     gb.data_ptr() + 4 * 16 * tj if ti == 0 else 0, slot, cbits | (zf << 32)])
                        local += 1
            assert local == self.items[t] and first_unused <= PARTS
        out = torch.tensor(recs, dtype=torch.int64).to(self.dev)
        self._witems[key] = out
        return out

    # ------------------------------------------------------------------------------------------- fused rollout
    def supports_fused_rollout(self, env):
        from ..envs.mujoco import MujocoShapeVecEnv
        return (isinstance(env, MujocoShapeVecEnv) and not self.discrete and self.A == LIN_ACT
                and self.D == LIN_OBS * env.frame_stack and env.frame_stack <= 3 and self.rollout_weights_in_lds()
                and [l.out_features for l in self.towers[0]] == [128, 128, 64, LIN_ACT]   # mlp_rollout_kernel shapes
                and [l.activation for l in self.towers[0][:-1]] == ["lrelu"] * 3)   # ... and the reference activations

    ROLLOUT_MAX_LDS = 150 * 1024
    ROLLOUT_NORM_LDS = 2 * 1024   # static LDS of the NORM instantiations (tables + normalised tile; mlp.hip)
    ROLL_RB = 4   # envs per rollout workgroup (mlp.hip ROLL_RB: 4x4x1 MFMA tiles)

    @staticmethod
    def rollout_lds_bytes_of(widths, wlds=True):
        """Dynamic LDS of mlp_rollout_kernel (layout in mlp.hip) for an actor ``[D, h_0, ..., A]``, from the widths
        alone (no device, no engine); ``wlds`` adds the staged actor weights + biases."""
        RB = MLPEngine.ROLL_RB
        widths = [int(w) for w in widths]
        n = 2 * RB * _ld(widths[0]) + sum(RB * _ld(w) for w in widths[1:])
        n += LIN_OBS * LIN_OBS + LIN_OBS * LIN_ACT + RB * LIN_OBS + RB * 16
        if wlds:
            n = (n + 3) // 4 * 4 + sum(o * _ld(i) + _ld(o) - 4 for i, o in zip(widths[:-1], widths[1:]))
        return 4 * n

    @staticmethod
    def rollout_towers_fit(widths, norm_obs=False):
        """Whether the one-launch rollout can hold an actor ``[D, h_0, ..., A]`` (tiles + weights) in LDS: the
        launcher's cap, less the static tables of the ``norm_obs`` instantiations."""
        cap = MLPEngine.ROLLOUT_MAX_LDS - (MLPEngine.ROLLOUT_NORM_LDS if norm_obs else 0)
        return MLPEngine.rollout_lds_bytes_of(widths, True) <= cap

    def rollout_lds_bytes(self, wlds):
        """:meth:`rollout_lds_bytes_of` this engine's actor."""
        return self.rollout_lds_bytes_of([self.D] + [l.out_features for l in self.towers[0]], wlds)

    def rollout_weights_in_lds(self):
        return self.rollout_towers_fit([self.D] + [l.out_features for l in self.towers[0]], self.obs_norm is not None)

    def supports_rollout_towers(self, env):
        """The generic-tower chain of the one-launch rollout (``TrainConfig.fused_rollout_towers``): any actor this
        engine takes, hidden tanh included, on the MuJoCo-shaped bank, as long as its weights fit in LDS."""
        from ..envs.mujoco import MujocoShapeVecEnv
        return (isinstance(env, MujocoShapeVecEnv) and not self.discrete and self.A == LIN_ACT
                and self.D == LIN_OBS * env.frame_stack and env.frame_stack <= 3 and self.rollout_weights_in_lds())

    def rollout_linear(self, env, st, key_shift, seed, stamps=None, boot=None, after_rollout=None, towers=False):
        """T steps of policy + env for the whole bank in one launch, then V(s) of all (T+1) N observations in one
        critic launch. Equal to T x (:meth:`policy_step` + ``env.step``) + :meth:`value` up to the actor's fp32
        summation order (4x4x1 tiles with the K range split over waves vs 16x16x4 tiles): same RNG keys and resets.

        ``boot`` (a :class:`TimeoutBootWorkspace` for this ``T``, ``N``, ``D`` and ``env.max_episode_steps``): the
        time-limit bootstrap (with an observation normaliser attached the slots hold raw stacks, normalised by the
        critic launch that values them). The rollout launch keeps the terminal observation of every truncated step in the
        workspace's slots, one more critic launch values the ``N S`` slots and one fix-up launch adds
        ``gamma V(terminal observation)`` to those steps' rewards (unused slots are valued but never read).

        ``after_rollout`` (a callable, optional) runs right after the rollout launch, when ``st.rewards`` holds the raw
        env rewards and before the fix-up launch adds any bootstrap term: the trainer's reward scaling.

        ``towers``: the launch runs the generic-tower chain (:meth:`supports_rollout_towers`) instead of the reference
        actor's register-resident one; everything else about it is the same. On the reference actor the two are
        bitwise equal, which is what tests select it for."""
        T, N = st.T, env.num_envs
        towers = bool(towers or self._force_rollout_towers)
        desc, _ = self.desc(None)
        wlds = self.rollout_weights_in_lds()
        if boot is not None and not boot.fits(T, N, self.D, env.max_episode_steps):
            raise ValueError("rollout_linear: the bootstrap workspace was built for another rollout geometry")
        # observation normaliser: the launch normalises the tile layer 0 reads; st.obs and the slots stay raw, and the
        # critic launches below normalise their own input tiles (_fwd)
        tables, nclip = self.obs_norm.kernel_args() if self.obs_norm is not None else (None, 0.0)
        _native.require().mlp_rollout(desc, self.rollout_lds_bytes(wlds), st.obs,
                                      st.actions, st.logp, st.entropy,
                                      st.rewards, st.dones, st.truncated, self.log_std, self.ac_scale, key_shift, seed,
                                      env.state, env.t, env.tg, env.ep_ret, env.ep_stats, env.env_ids, env.A, env.B,
                                      env.seed, env.max_episode_steps, env.frame_stack, wlds, stamps,
                                      None if boot is None else boot.final_obs,
                                      None if boot is None else boot.final_step, tables, nclip, self.hidden_tanh[0],
                                      self._hdescs[None] if towers else None)
        if after_rollout is not None:
            after_rollout()
        self.value(st.obs.view((T + 1) * N, -1), st.values.view(-1))
        if boot is not None:
            from .returns import timeout_bootstrap_
            self.value(boot.final_obs.view(N * boot.S, -1), boot.final_v.view(-1))
            timeout_bootstrap_(st.rewards, boot.final_step, boot.final_v, boot.gamma)

    def rollout_eval_linear(self, env, obs0, steps, rec, towers=False):
        """Deterministic evaluation of the MuJoCo-shaped bank ``env`` in ONE launch (the ``EVAL`` instantiations of
        ``mlp_rollout_kernel``): ``steps`` steps of actor mean + env step from the first observation stack ``obs0``
        ``[N, D]``; nothing is stored per step, no noise is drawn, and the first ``rec.E`` finished episodes of every
        env go to ``rec`` (an ``ops/evaluation.py`` EvalRecords). The bank's ``state``, ``t``, ``tg`` and ``ep_ret`` are
        advanced and written back; ``ep_stats`` and ``obs0`` are not touched. With an observation normaliser attached
        layer 0 reads the tile normalised by the tables as they stand. ``towers``: as in :meth:`rollout_linear`."""
        towers = bool(towers or self._force_rollout_towers)
        desc, _ = self.desc(None)
        wlds = self.rollout_weights_in_lds()
        tables, nclip = self.obs_norm.kernel_args() if self.obs_norm is not None else (None, 0.0)
        _native.require().mlp_rollout_eval(desc, self.rollout_lds_bytes(wlds), obs0, int(steps), self.log_std,
                                           self.ac_scale, env.state, env.t, env.tg, env.ep_ret, env.env_ids, env.A,
                                           env.B, env.seed, env.max_episode_steps, env.frame_stack, wlds,
                                           rec.ep_ret, rec.ep_len, rec.cnt, tables, nclip, None, None,
                                           self.hidden_tanh[0], self._hdescs[None] if towers else None)
