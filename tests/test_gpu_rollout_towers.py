"""The generic-tower chain of the one-launch MuJoCo rollout (``mlp_rollout_kernel``'s GEN instantiations, reached
through ``aca_mlp_rollout_towers``; ``TrainConfig.fused_rollout_towers``).

Two oracles. On the reference actor the generic chain keeps the register-resident chain's wave split, so both issue the
same MFMA sequence on the same operands: whole rollouts must be BITWISE equal (test 1). On custom actors the oracle is
the per-step path (``policy_step`` + ``env_step_linear`` launches) at the bar the existing fused-against-per-step tests
set, rtol = atol = 1e-4 (16x16x4 tiles against 4x4x1 tiles with a K split: another fp32 summation order); every measured
maximum is printed before it is asserted (``pytest -s``; profiles/rollout_towers.txt keeps one such run).

All rollouts: T = 24 with an episode limit of 7, so resets and truncations happen inside the launch, and two
consecutive ``collect()`` calls, so the second starts from the written-back env bank."""
import os
import sys

import numpy as np
import pytest
import torch

from actor_critic_algs_on_tensorflow_amd import envs as E
from actor_critic_algs_on_tensorflow_amd import preset
from actor_critic_algs_on_tensorflow_amd.algos.evaluator import Evaluator

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "oracles"))
import eval_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

T, LIMIT = 24, 7
FIELDS_EXACT = ("dones", "truncated")
FIELDS_CLOSE = ("obs", "actions", "logp", "entropy", "rewards", "values")
BANK = ("state", "t", "tg", "ep_ret")

# actor towers: the smallest shapes that reach every branch of the run-time wave split
TOWERS = [((64, 64), "tanh"),             # the preset
          ((48, 32), "tanh"),             # K pad 48 -> 64, N pad
          ((24,), "relu"),                # 2 layers, K_ = 32
          ((192, 64), "lrelu"),           # CG = 3, S = 2
          ((256, 16), "tanh"),            # CG = 4, K_ = 256, a 16-wide layer
          ((32, 16, 16, 8), "tanh"),      # 5 layers = MLP_MAXL, K_ = 16, S = 4
          ((128, 128, 64), "tanh")]       # the reference widths, which alone must not select the register chain
TOWER_IDS = ["x".join(map(str, h)) + "-" + a for h, a in TOWERS]


def _make(name, frames, num_envs, **over):
    from actor_critic_algs_on_tensorflow_amd.algos.trainer import ActorCriticTrainer
    kw = dict(num_envs=num_envs, n_steps=T, frames=frames, ppo_epochs=1, ppo_minibatches=2, device="cuda:0",
              outdir=None, quiet=True, stdout_freq=0, save_every=0, cuda_graph=False)
    kw.update(over)
    tr = ActorCriticTrainer(preset(name, **kw))
    assert tr.mlp is not None
    tr.env.max_episode_steps = LIMIT
    return tr


def _custom(hidden, act, frames, num_envs, **over):
    return _make("halfcheetah_ppo_tanh64", frames, num_envs, actor_hidden=hidden, hidden_act=act, **over)


def _no_per_step(*a, **k):
    raise AssertionError("the one-launch rollout was expected: policy_step was called")


def _spy(obj, name):
    """Wraps ``obj.name`` and records the keyword arguments of every call."""
    calls, real = [], getattr(obj, name)

    def wrapped(*a, **k):
        calls.append(k)
        return real(*a, **k)
    setattr(obj, name, wrapped)
    return calls


def _set_tables(norm, seed):
    """Tables away from the identity: means in +-0.5, stds in [0.5, 2], clip 1.5 so that clipping occurs."""
    g = torch.Generator().manual_seed(seed)
    sign = torch.where(torch.rand(norm.D, generator=g) < 0.5, -1.0, 1.0)
    norm.mean32.copy_(sign * (0.1 + 0.4 * torch.rand(norm.D, generator=g)))
    norm.istd32.copy_(1.0 / (0.5 + 1.5 * torch.rand(norm.D, generator=g)))
    norm.clip = 1.5


# ---------------------------------------------------------------------- 1. reference actor: generic == register chain
@pytest.mark.parametrize("variant", ["plain", "boot", "norm_obs"])
@pytest.mark.parametrize("frames,num_envs", [(1, 20), (3, 37)])
def test_generic_chain_is_bitwise_the_register_chain_on_the_reference_actor(cuda, frames, num_envs, variant):
    """Every storage field, the env bank and the bootstrap workspace with ``torch.equal``. One word is outside what
    either chain decides: ``ep_stats[0]``, the sum of the finished episodes' returns, is added up with fp32 atomics by
    the rollout's workgroups (``common.h`` add_ep_stats) in whatever order they get there, so two launches of the SAME
    kernel already differ in its last bits. Its summands are pinned bitwise by the fields above (rewards, dones and
    the bank's ``ep_ret``); the word itself is held to the reordering bound of an fp32 sum, 2 (m - 1) 2^-24 sum |term|
    for m terms, with sum |term| <= the sum of all |rewards| so far. The episode count and the length sum next to it
    are integers and exact."""
    extra = {"boot": dict(bootstrap_on_timeout=True), "norm_obs": dict(norm_obs=True)}.get(variant, {})
    reg, gen = (_make("mujoco_ppo_dp8", frames, num_envs, **extra) for _ in range(2))
    for tr in (reg, gen):
        assert tr.mlp.supports_fused_rollout(tr.env) and tr.mlp.supports_rollout_towers(tr.env)
        tr.mlp.policy_step = _no_per_step
    gen.mlp._force_rollout_towers = True   # the engine's private test hook
    calls = [_spy(tr.mlp, "rollout_linear") for tr in (reg, gen)]
    abs_total = 0.0   # upper bound of sum |finished episode return|: every |raw reward| so far

    def seen_rewards(tr):
        tot = float(tr.storage.rewards.double().abs().sum())
        if variant == "boot":   # stored = raw + gamma v on the truncated steps, so |raw| <= |stored| + gamma |v|
            ws = tr._boot_ws
            tot += ws.gamma * float(ws.final_v[ws.final_step >= 0].double().abs().sum())
        return tot
    if variant == "norm_obs":   # one update first, so that the tables are not the identity
        for tr in (reg, gen):
            tr.step()
        torch.cuda.synchronize()
        assert torch.equal(reg.flat.data, gen.flat.data) and torch.equal(reg.storage.rewards, gen.storage.rewards)
        abs_total += seen_rewards(gen)
        assert float(reg.obs_norm.mean32.abs().max()) > 0 and torch.equal(reg.obs_norm.tables, gen.obs_norm.tables)
    for it in range(2):
        for tr in (reg, gen):
            tr.collect()
        torch.cuda.synchronize()
        for name in FIELDS_EXACT + FIELDS_CLOSE:
            assert torch.equal(getattr(reg.storage, name), getattr(gen.storage, name)), (it, name)
        for name in BANK:
            assert torch.equal(getattr(reg.env, name), getattr(gen.env, name)), (it, name)
        abs_total += seen_rewards(gen)
        sa, sb = reg.env.ep_stats, gen.env.ep_stats
        assert torch.equal(sa[1:], sb[1:]) and float(sa[1]) > 0               # episodes, summed lengths
        m = float(sa[1])                                                      # at most one atomic add per episode
        bound = 2 * (m - 1) * 2.0 ** -24 * abs_total
        print(f"ep_stats[0] {float(sa[0])!r} vs {float(sb[0])!r}: |diff| {abs(float(sa[0]) - float(sb[0])):.3e}, "
              f"reordering bound {bound:.3e} (m = {m:.0f}, sum |reward| <= {abs_total:.4g})")
        assert abs(float(sa[0]) - float(sb[0])) <= bound
        if variant == "boot":
            assert torch.equal(reg._boot_ws.final_step, gen._boot_ws.final_step)
            assert torch.equal(reg._boot_ws.final_obs, gen._boot_ws.final_obs)
            assert int((gen._boot_ws.final_step >= 0).sum()) == int(gen.storage.truncated.sum()) > 0
        assert int(gen.storage.dones.sum()) > 0 and torch.isfinite(gen.storage.actions).all()
        for tr in (reg, gen):
            tr.storage.roll_over()
    assert len(calls[0]) == len(calls[1]) >= 2 and not any(k.get("towers") for k in calls[0])


# ---------------------------------------------------------------------- 2. custom towers against the per-step path
def _compare(fused, per_step, tag, boot=False):
    a, b = fused.storage, per_step.storage
    for name in FIELDS_EXACT:
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    ea, eb = fused.env, per_step.env
    for name in ("t", "tg"):
        assert torch.equal(getattr(ea, name), getattr(eb, name)), name
    pairs = [(n, getattr(a, n), getattr(b, n)) for n in FIELDS_CLOSE]
    pairs += [(n, getattr(ea, n), getattr(eb, n)) for n in ("state", "ep_ret", "ep_stats")]
    if boot:
        ws = fused._boot_ws
        step = ws.final_step.long()
        used = step >= 0
        env = torch.arange(step.shape[0], device=step.device)[:, None].expand_as(step)
        s_u, e_u = step[used], env[used]
        # final_step exactly consistent with truncated: every used slot names a truncated step of its env, once
        assert ((step == -1) | used).all() and (step < T).all()
        assert a.truncated[s_u, e_u].all() and int(used.sum()) == int(a.truncated.sum()) > 0
        assert torch.unique(s_u * step.shape[0] + e_u).numel() == s_u.numel()
        pairs.append(("final_obs", ws.final_obs[used], per_step._final_obs[s_u, e_u]))
    print(tag, " ".join(f"{n} {float((x.double() - y.double()).abs().max()):.2e}" for n, x, y in pairs))
    for n, x, y in pairs:
        assert torch.isfinite(x).all(), n
        torch.testing.assert_close(x, y, rtol=1e-4, atol=1e-4, msg=n)
    assert int(a.dones.sum()) > 0


def _pair(hidden, act, frames, num_envs, **extra):
    fused = _custom(hidden, act, frames, num_envs, fused_rollout_towers=True, **extra)
    per_step = _custom(hidden, act, frames, num_envs, fused_rollout=False, **extra)
    for tr in (fused, per_step):
        assert not tr.mlp.supports_fused_rollout(tr.env) and tr.mlp.supports_rollout_towers(tr.env)
    fused.mlp.policy_step = _no_per_step
    per_step.mlp.rollout_linear = _no_per_step
    return fused, per_step


@pytest.mark.parametrize("num_envs", [5, 37])
@pytest.mark.parametrize("frames", [1, 3])
@pytest.mark.parametrize("hidden,act", TOWERS, ids=TOWER_IDS)
def test_custom_towers_one_launch_matches_per_step(cuda, hidden, act, frames, num_envs):
    fused, per_step = _pair(hidden, act, frames, num_envs)
    calls = _spy(fused.mlp, "rollout_linear")
    for it in range(2):
        for tr in (fused, per_step):
            tr.collect()
        torch.cuda.synchronize()
        _compare(fused, per_step, f"towers {hidden} {act} k={frames} N={num_envs} #{it}:")
        for tr in (fused, per_step):
            tr.storage.roll_over()
    assert len(calls) == 2 and all(k["towers"] for k in calls)


# ---------------------------------------------------------------------- 3. ... with the bootstrap and with norm_obs
@pytest.mark.parametrize("variant", ["boot", "norm_obs"])
@pytest.mark.parametrize("frames,num_envs", [(1, 5), (3, 37)])
@pytest.mark.parametrize("hidden,act", [((64, 64), "tanh"), ((192, 64), "lrelu")], ids=["64x64-tanh", "192x64-lrelu"])
def test_custom_towers_bootstrap_and_norm_obs(cuda, hidden, act, frames, num_envs, variant):
    boot = variant == "boot"
    extra = dict(bootstrap_on_timeout=True) if boot else dict(norm_obs=True)
    fused, per_step = _pair(hidden, act, frames, num_envs, **extra)
    for tr in (fused, per_step):
        tr.env.t.copy_(torch.arange(num_envs, device=cuda) % LIMIT)   # staggered clocks: a tile's envs cut apart
        if not boot:
            _set_tables(tr.obs_norm, seed=frames)
    for it in range(2):
        for tr in (fused, per_step):
            tr.collect()
        torch.cuda.synchronize()
        _compare(fused, per_step, f"towers {hidden} {act} {variant} k={frames} N={num_envs} #{it}:", boot=boot)
        if not boot:   # storage stays raw: the newest frame of every stack is the env's state row
            a = fused.storage
            assert float((a.obs - fused.obs_norm.apply(a.obs)).abs().max()) > 0.1
            assert torch.equal(a.obs[T][:, 17 * (frames - 1):], fused.env.state.view(num_envs, 17))
        for tr in (fused, per_step):
            tr.storage.roll_over()


# ---------------------------------------------------------------------- 4. evaluation
@pytest.mark.parametrize("norm", [False, True])
def test_one_launch_evaluation_of_custom_towers(cuda, norm, monkeypatch):
    """eval_envs = 5, time limit 7, 2 episodes: the "fused" evaluation of a (64, 64) tanh policy against its per-step
    "native" evaluation, lengths and counts exactly, returns at the bar of test_gpu_eval.py's same comparison on the
    reference actor: 8 x the error of the fp32 CPU torch evaluation against the fp64 oracle for either path, hence
    twice that between the two."""
    N, EPS, frames = 5, 2, 1
    # the fp64 oracle names the reference actor's layers; hidden_layers / out_layer is the same list for any actor
    monkeypatch.setattr(O, "actor_layers", lambda model: list(model.actor.hidden_layers) + [model.actor.out_layer])
    tr = _custom((64, 64), "tanh", frames, 4, fused_rollout_towers=True, eval_every=1, eval_envs=N, eval_episodes=EPS,
                 norm_obs=norm)
    assert tr.evaluator.path == "fused" and tr.evaluator._towers
    off = _custom((64, 64), "tanh", frames, 4, eval_every=1, eval_envs=N, eval_episodes=EPS)
    assert off.evaluator.path == "native"   # the flag is what selects it
    m, eng = tr.model, tr.mlp
    tables = None
    if norm:
        _set_tables(tr.obs_norm, seed=3)
        tables = tr.obs_norm.tables.detach().cpu().clone()
    # the fp64 oracle and the fp32 CPU torch form, on a CPU copy of the same parameters
    import copy
    env_cpu = E.make("HalfCheetahShape-v0", N, device="cpu", seed=4242, frame_stack=frames, max_episode_steps=LIMIT)
    m_cpu = copy.deepcopy(m).to("cpu")
    oracle = O.run_linear(m_cpu, N, 4242, frames, LIMIT, EPS, tables, 1.5 if norm else None)
    on_cpu = None
    if norm:
        from actor_critic_algs_on_tensorflow_amd.ops.obs_norm import ObsNormalizer
        on_cpu = ObsNormalizer(17 * frames, 1.5, device="cpu")
        on_cpu.tables.copy_(tables)
        on_cpu = on_cpu.freeze()
    rc = Evaluator(m_cpu, env_cpu, None, on_cpu, EPS).evaluate()
    bar = 8 * float((torch.as_tensor(rc["ep_ret"]).double() - oracle["ep_ret"]).abs().max())
    got = {}
    for path, kw in (("fused", dict(fused_towers=True)), ("native", dict(fused=False))):
        env = E.make("HalfCheetahShape-v0", N, device=cuda, seed=4242, frame_stack=frames, max_episode_steps=LIMIT)
        ev = Evaluator(m, env, eng, tr.obs_norm, EPS, **kw)
        assert ev.path == path
        real = eng.policy_step
        if path == "fused":
            eng.policy_step = _no_per_step
        try:
            r = ev.evaluate()
        finally:
            eng.policy_step = real
        err = float((torch.as_tensor(r["ep_ret"]).double() - oracle["ep_ret"]).abs().max())
        print(f"eval towers norm={norm} {path}: ep_ret err {err:.3e} (bar {bar:.3e})")
        assert np.array_equal(r["ep_len"], oracle["ep_len"].numpy().astype(np.int32))
        assert np.array_equal(r["cnt"], oracle["cnt"].numpy().astype(np.int32)) and int(r["cnt"].sum()) == N * EPS
        assert err <= bar
        got[path] = r
    assert np.array_equal(got["fused"]["ep_len"], got["native"]["ep_len"])
    assert float(np.abs(got["fused"]["ep_ret"].astype(np.float64) - got["native"]["ep_ret"]).max()) <= 2 * bar
    assert abs(got["fused"]["ret_mean"] - got["native"]["ret_mean"]) <= 2 * bar


# ---------------------------------------------------------------------- 5. trainer
def _small(graph, engine="auto", **over):
    from actor_critic_algs_on_tensorflow_amd.algos.trainer import ActorCriticTrainer
    kw = dict(num_envs=4, n_steps=8, ppo_epochs=2, ppo_minibatches=2, device="cuda:0", outdir=None, quiet=True,
              stdout_freq=0, save_every=0, cuda_graph=graph, engine=engine)
    kw.update(over)
    return ActorCriticTrainer(preset("halfcheetah_ppo_tanh64_fused", **kw))


def test_trainer_captured_equals_eager_on_the_one_launch_rollout(cuda):
    g, e = _small(True), _small(False)
    calls = []
    for tr in (g, e):
        assert tr.cfg.fused_rollout_towers and tr.mlp.supports_rollout_towers(tr.env)
        assert not tr.mlp.supports_fused_rollout(tr.env)
        tr.mlp.policy_step = _no_per_step   # never during collect (captured or eager)
        calls.append(_spy(tr.mlp, "rollout_linear"))
    g.capture(warmup=1)
    assert g.graph is not None
    e.update_body()   # the capture's warm-up update
    p0 = e.flat.data.clone()
    for _ in range(3):
        g.step()
        e.step()
        torch.cuda.synchronize()
        assert torch.equal(g.flat.data, e.flat.data)
    assert torch.isfinite(e.flat.data).all() and (e.flat.data != p0).any()
    for fa, fb in zip(list(g.mlp.F.values()) + list(g.mlp.G.values()),
                      list(e.mlp.F.values()) + list(e.mlp.G.values())):
        assert torch.equal(fa, fb)
    assert len(calls[1]) == 4 and all(k["towers"] for k in calls[0] + calls[1]) and calls[0]


def test_trainer_update_matches_torch_engine_on_the_one_launch_rollout(cuda):
    """Direction (cosine > 0.999) and length (within 1e-2) of the whole parameter change, the bar of
    test_gpu_mlp_towers.py::test_trainer_update_matches_torch_engine and for its reason: an Adam step divides each
    element's gradient by its own running magnitude, so no per-element bound follows from a gradient error."""
    nat, ref = _small(False), _small(False, engine="torch")
    assert nat.mlp is not None and ref.mlp is None and torch.equal(nat.flat.data, ref.flat.data)
    nat.mlp.policy_step = _no_per_step
    for u in range(2):
        pn, pr = nat.flat.data.clone(), ref.flat.data.clone()
        nat.step()
        ref.step()
        torch.cuda.synchronize()
        torch.testing.assert_close(nat.storage.actions, ref.storage.actions, rtol=1e-4, atol=1e-4)
        d_n, d_r = (nat.flat.data - pn).double(), (ref.flat.data - pr).double()
        cos = float(torch.nn.functional.cosine_similarity(d_n, d_r, dim=0))
        print("update", u, "cos", cos, "norm ratio", float(d_n.norm() / d_r.norm()))
        assert float(d_r.norm()) > 0
        assert cos > 0.999 and abs(float(d_n.norm() / d_r.norm()) - 1) < 1e-2


# ---------------------------------------------------------------------- 6. fall-backs and refusals
def test_actor_that_does_not_fit_lds_takes_the_per_step_path(cuda):
    tr = _small(False, actor_hidden=(256, 128))
    assert tr.mlp.rollout_lds_bytes(True) == 184592 and not tr.mlp.supports_rollout_towers(tr.env)
    tr.mlp.rollout_linear = _no_per_step
    calls = _spy(tr.mlp, "policy_step")
    p0 = tr.flat.data.clone()
    tr.step()
    torch.cuda.synchronize()
    assert len(calls) == tr.cfg.n_steps and torch.isfinite(tr.flat.data).all() and (tr.flat.data != p0).any()


def test_other_banks_take_the_per_step_path(cuda):
    tr = _small(False, env="Pendulum-v0", eval_every=1, eval_envs=3)
    assert not tr.mlp.supports_rollout_towers(tr.env) and tr.evaluator.path == "native"
    tr.mlp.rollout_linear = _no_per_step
    calls = _spy(tr.mlp, "policy_step")
    tr.collect()
    torch.cuda.synchronize()
    assert len(calls) == tr.cfg.n_steps


def test_launcher_refusals_launch_nothing(cuda):
    """Everything the launcher refuses raises from the binding before any launch: no buffer of the rollout or the env
    bank changes."""
    from actor_critic_algs_on_tensorflow_amd import _native
    from actor_critic_algs_on_tensorflow_amd.algos.trainer import KEY_ENV_BITS
    from actor_critic_algs_on_tensorflow_amd.ops.mlp import MAXL, TOWER_WORDS
    tr = _custom((64, 64), "tanh", 1, 5, fused_rollout_towers=True)
    env, st, eng = tr.env, tr.storage, tr.mlp
    st.rewards.fill_(-7.0)
    st.obs[1:].fill_(-7.0)
    before = {n: getattr(env, n).clone() for n in ("state", "t", "tg", "ep_ret")}
    cap = eng.ROLLOUT_MAX_LDS
    need = eng.rollout_lds_bytes(True)
    assert need == 34576
    desc, _ = eng.desc(None)
    good = eng._hdescs[None]

    def launch(hdesc, k=1, wlds=True, lds=need):
        _native.require().mlp_rollout(desc, lds, st.obs, st.actions, st.logp, st.entropy, st.rewards, st.dones,
                                      st.truncated, eng.log_std, eng.ac_scale, KEY_ENV_BITS, 1, env.state, env.t,
                                      env.tg, env.ep_ret, env.ep_stats, env.env_ids, env.A, env.B, env.seed,
                                      env.max_episode_steps, k, wlds, None, None, None, None, 0.0, True, hdesc)

    def edited(word, value):
        w = good.clone()
        w[word] = value
        return w
    with pytest.raises(RuntimeError, match="mlp_rollout launch failed"):
        launch(good, lds=cap + 16)      # above the cap
    with pytest.raises(RuntimeError, match="mlp_rollout launch failed"):
        launch(good, lds=need - 16)     # fewer bytes than the kernel's layout of this tower needs
    bad = {"nl = 0": edited(0, 0), "nl above MLP_MAXL": edited(0, MAXL + 1),
           "first layer does not read D": edited(2, 34), "layers do not chain": edited(2 + 1, 48),
           "head is not LIN_ACT wide": edited(2 + MAXL + 2, 5), "width above 256": edited(2 + MAXL, 272),
           "unknown activation": edited(2 + 2 * MAXL, 9)}
    assert TOWER_WORDS == 2 + 11 * MAXL
    for why, words in bad.items():
        with pytest.raises(RuntimeError, match="mlp_rollout launch failed"):
            launch(words)
        print("refused:", why)
    with pytest.raises(RuntimeError, match="mlp_rollout launch failed"):
        launch(good, wlds=False)
    with pytest.raises(RuntimeError, match="hdesc must be the CPU desc"):
        launch(desc)
    with pytest.raises(RuntimeError, match="hdesc must be the CPU desc"):
        launch(good[:8].clone())
    # the reference-only entry keeps refusing a hidden tanh layer
    with pytest.raises(RuntimeError, match="mlp_rollout launch failed"):
        eng.rollout_linear(env, st, KEY_ENV_BITS, 1)
    torch.cuda.synchronize()
    assert (st.rewards == -7.0).all() and (st.obs[1:] == -7.0).all()
    for n, v in before.items():
        assert torch.equal(getattr(env, n), v), n
    launch(good)   # ... and the untouched words launch
    torch.cuda.synchronize()
    assert (st.rewards != -7.0).all()
