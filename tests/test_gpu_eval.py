"""Deterministic evaluation on the device: the greedy flag of ``mlp_fwd_kernel`` mode 0, ``eval_scan_kernel``, the EVAL
instantiations of ``mlp_rollout_kernel`` and the Evaluator's three paths, against the fp64 oracle of
tests/oracles/eval_oracle.py. Floating-point bars are 8 x the measured error of the fp32 CPU torch form against that
oracle on the same inputs (the rule of tests/test_gpu_sampling.py), never taken from a kernel's output."""
import copy
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "oracles"))
import eval_oracle as O  # noqa: E402
import sampling_oracle as SO  # noqa: E402

from actor_critic_algs_on_tensorflow_amd import envs as E  # noqa: E402
from actor_critic_algs_on_tensorflow_amd import preset  # noqa: E402
from actor_critic_algs_on_tensorflow_amd.algos.evaluator import Evaluator  # noqa: E402
from actor_critic_algs_on_tensorflow_amd.models.policy import MLPActorCritic, build_model  # noqa: E402
from actor_critic_algs_on_tensorflow_amd.ops import evaluation as EV  # noqa: E402
from actor_critic_algs_on_tensorflow_amd.ops.obs_norm import ObsNormalizer  # noqa: E402
from actor_critic_algs_on_tensorflow_amd.ops.optim import FlatParams  # noqa: E402

pytestmark = pytest.mark.gpu

HEADS = {"g17": (17, 6, False), "g3": (3, 1, False), "c4": (4, 2, True)}


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _cpu_model(ob, ac, disc, seed):
    g = torch.Generator().manual_seed(seed)
    m = MLPActorCritic(ob, ac, disc, None if disc else np.full(ac, 2.0, np.float32), "basic", generator=g)
    if not disc:
        with torch.no_grad():
            m.actor.log_std.copy_(torch.linspace(-0.7, 0.4, ac))
    return m


def _engine(model_cpu, cuda):
    from actor_critic_algs_on_tensorflow_amd.ops.mlp import MLPEngine
    m = copy.deepcopy(model_cpu).to(cuda)
    flat = FlatParams(m.param_groups(), cuda)
    return m, flat, MLPEngine(m, flat)


@functools.lru_cache(maxsize=None)
def _greedy_reference(head, seed):
    """fp64 oracle and fp32 torch form of the greedy head on the 36 shared rows, and the bars they give."""
    ob, ac, disc = HEADS[head]
    m = _cpu_model(ob, ac, disc, seed)
    obs = torch.randn(36, ob, generator=torch.Generator().manual_seed(100))
    y64 = O.actor_fp64(m, obs)
    with torch.no_grad():
        a32, lp32, _, _ = m.act(obs, deterministic=True)
        y32 = m.actor(obs)
    ref = dict(model=m, obs=obs, y64=y64)
    if disc:
        act, gap = O.argmax_gap(y64)
        bar = SO.tolerance(SO.err(y32, y64)[0], float(y64.abs().max()))
        ref.update(act=act, gap=gap, bar=bar, keep=gap > 2 * bar)
    else:
        ls = m.actor.log_std.detach().double().clamp(-2.5, 2.5)
        lp64 = (-ls - SO.HALF_LOG_2PI).sum().expand(36)
        ref.update(lp64=lp64, tol_a=SO.tolerance(SO.err(a32, y64)[0], float(y64.abs().max())),
                   tol_lp=SO.tolerance(SO.err(lp32, lp64)[0], float(lp64.abs().max())))
    return ref


def _policy_step(eng, obs, disc, ac, greedy, seed=1234, tg0=3):
    B = obs.shape[0]
    dev = obs.device
    act = torch.full((B,) if disc else (B, ac), -7, dtype=torch.int32 if disc else torch.float32, device=dev)
    logp, ent, v = (torch.full((B,), -7.0, device=dev) for _ in range(3))
    tg = torch.arange(B, device=dev, dtype=torch.int64) + tg0
    ids = torch.arange(B, device=dev, dtype=torch.int64) + 5
    eng.policy_step(obs, act, logp, ent, v, tg, ids, 20, seed, greedy=greedy)
    return act, logp, ent, v


# ------------------------------------------------------------------------------------------------ 1. greedy policy_step
@pytest.mark.parametrize("B", [1, 16, 36])
@pytest.mark.parametrize("head", ["g17", "g3"])
def test_greedy_gaussian_policy_step_against_fp64(cuda, head, B):
    ob, ac, disc = HEADS[head]
    ref = _greedy_reference(head, 7)
    _, _, eng = _engine(ref["model"], cuda)
    obs = ref["obs"][:B].to(cuda).contiguous()
    act, logp, ent, v = _policy_step(eng, obs, disc, ac, True)
    _, _, ent_s, v_s = _policy_step(eng, obs, disc, ac, False)
    ea = SO.err(act, ref["y64"][:B])[0]
    el = SO.err(logp, ref["lp64"][:B])[0]
    print(f"greedy {head} B={B}: action err {ea:.3e} (bar {ref['tol_a']:.3e}), logp err {el:.3e} "
          f"(bar {ref['tol_lp']:.3e})")
    assert ea <= ref["tol_a"] and el <= ref["tol_lp"]
    assert torch.equal(ent, ent_s) and torch.equal(v, v_s)
    # no random number: other seeds and env counters change nothing
    act2, logp2, ent2, v2 = _policy_step(eng, obs, disc, ac, True, seed=99, tg0=1 << 33)
    assert torch.equal(act, act2) and torch.equal(logp, logp2) and torch.equal(ent, ent2) and torch.equal(v, v2)


@pytest.mark.parametrize("B", [1, 16, 36])
@pytest.mark.parametrize("seed", [7, 5, 11])
def test_greedy_categorical_policy_step_against_fp64(cuda, seed, B):
    ob, ac, disc = HEADS["c4"]
    ref = _greedy_reference("c4", seed)
    assert int((~ref["keep"]).sum()) <= 1, "at most 1 row of 36 may sit inside the gap"
    _, _, eng = _engine(ref["model"], cuda)
    obs = ref["obs"][:B].to(cuda).contiguous()
    act, logp, ent, v = _policy_step(eng, obs, disc, ac, True)
    _, _, ent_s, v_s = _policy_step(eng, obs, disc, ac, False)
    keep = ref["keep"][:B]
    print(f"greedy c4 seed={seed} B={B}: smallest gap {float(ref['gap'].min()):.3e}, bar {ref['bar']:.3e}, "
          f"rows left out {int((~keep).sum())}")
    assert torch.equal(act.cpu().long()[keep], ref["act"][:B][keep])
    assert torch.equal(ent, ent_s) and torch.equal(v, v_s)
    act2, logp2, _, _ = _policy_step(eng, obs, disc, ac, True, seed=99, tg0=1 << 33)
    assert torch.equal(act, act2) and torch.equal(logp, logp2)


# ------------------------------------------------------------------------------------------------ 2. ties
def test_greedy_ties_take_the_first_index_on_the_device(cuda):
    m, flat, eng = _engine(_cpu_model(4, 2, True, 7), cuda)
    with torch.no_grad():
        m.actor.logits.kernel.zero_()
        m.actor.logits.bias.zero_()
    eng.sync_shadow()
    obs = torch.randn(36, 4, generator=torch.Generator().manual_seed(100)).to(cuda)
    act, logp, _, _ = _policy_step(eng, obs, True, 2, True)
    assert bool((act == 0).all())
    assert torch.equal(logp, torch.full_like(logp, float(torch.log(torch.tensor(0.5)))))


# ------------------------------------------------------------------------------------------------ 3. eval_scan
@pytest.mark.parametrize("E_", [1, 3])
@pytest.mark.parametrize("L", [1, 16, 17, 50])
@pytest.mark.parametrize("N", [1, 65])
def test_eval_scan_kernel_matches_the_torch_form(cuda, N, L, E_):
    assert EV.scan_unroll() == 16
    g = torch.Generator().manual_seed(L * 100 + N)
    random_cols = (torch.randn(L, N, generator=g) * 50.0, (torch.rand(L, N, generator=g) < 0.15).to(torch.uint8))
    for rewards, dones in (O.crafted_columns(L, N), random_cols):
        want = EV.EvalRecords(N, E_)
        EV.eval_scan_ref(rewards, dones, *want.tensors())
        rec = EV.EvalRecords(N, E_, cuda)
        EV.eval_scan(rewards.to(cuda), dones.to(cuda), *rec.tensors())
        assert _same(rec.ep_ret.cpu().numpy(), want.ep_ret.numpy())
        assert torch.equal(rec.ep_len.cpu(), want.ep_len) and torch.equal(rec.cnt.cpu(), want.cnt)


# ------------------------------------------------------------------------------------------------ 4. fused EVAL launch
MAXS, EPS = 7, 3


def _linear_setup(cuda, frames, N, norm):
    env_cpu = E.make("HalfCheetahShape-v0", N, device="cpu", seed=4242, frame_stack=frames, max_episode_steps=MAXS)
    model = build_model(env_cpu, "mlp", "basic", seed=7)
    D = 17 * frames
    tables = None
    if norm:
        g = torch.Generator().manual_seed(9)
        tables = torch.stack([0.05 * torch.randn(D, generator=g), 0.5 + 2.0 * torch.rand(D, generator=g)])
    return env_cpu, model, tables


def _normaliser(tables, device):
    if tables is None:
        return None
    on = ObsNormalizer(tables.shape[1], 10.0, device=device)
    on.tables.copy_(tables)
    return on.freeze()


@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("frames,N", [(1, 1), (1, 5), (3, 37)])
def test_fused_and_per_step_evaluation_against_fp64(cuda, frames, N, norm):
    """L = 21 steps with three resets inside the launch and partial 4-env tiles."""
    env_cpu, model, tables = _linear_setup(cuda, frames, N, norm)
    oracle = O.run_linear(model, N, 4242, frames, MAXS, EPS, tables, 10.0)
    cpu = Evaluator(model, env_cpu, None, _normaliser(tables, "cpu"), EPS)
    rc = cpu.evaluate()
    bar_ret = 8 * float((torch.as_tensor(rc["ep_ret"]).double() - oracle["ep_ret"]).abs().max())
    bar_state = 8 * float((env_cpu.state.double() - oracle["state"]).abs().max())
    assert np.array_equal(rc["ep_len"], oracle["ep_len"].numpy()) and torch.equal(env_cpu.tg, oracle["tg"])
    m, flat, eng = _engine(model, cuda)
    eng.obs_norm = _normaliser(tables, cuda)
    got = {}
    for path, fused in (("fused", True), ("native", False)):
        env = E.make("HalfCheetahShape-v0", N, device=cuda, seed=4242, frame_stack=frames, max_episode_steps=MAXS)
        ev = Evaluator(m, env, eng, eng.obs_norm, EPS, fused=fused)
        assert ev.path == path
        if fused:
            def no_per_step(*a, **k):
                raise AssertionError("the fused evaluation called policy_step")
            real, eng.policy_step = eng.policy_step, no_per_step
        try:
            r = ev.evaluate()
        finally:
            if fused:
                eng.policy_step = real
        e_ret = float((torch.as_tensor(r["ep_ret"]).double() - oracle["ep_ret"]).abs().max())
        e_state = float((env.state.cpu().double() - oracle["state"]).abs().max())
        print(f"eval frames={frames} N={N} norm={norm} {path}: ep_ret err {e_ret:.3e} (bar {bar_ret:.3e}), "
              f"state err {e_state:.3e} (bar {bar_state:.3e})")
        assert np.array_equal(r["ep_len"], oracle["ep_len"].numpy().astype(np.int32))
        assert np.array_equal(r["cnt"], oracle["cnt"].numpy().astype(np.int32))
        assert torch.equal(env.t.cpu().long(), oracle["t"]) and torch.equal(env.tg.cpu(), oracle["tg"])
        assert e_ret <= bar_ret and e_state <= bar_state
        got[path] = r
    assert abs(got["fused"]["ret_mean"] - got["native"]["ret_mean"]) <= 2 * bar_ret


# ------------------------------------------------------------------------------------------------ 5. CartPole per step
def test_per_step_evaluation_cartpole_teacher_forced(cuda):
    N, maxs, E_ = 5, 9, 2
    env_cpu = E.make("CartPole-v1", N, device="cpu", seed=31, max_episode_steps=maxs)
    model = build_model(env_cpu, "mlp", "basic", seed=7)
    m, flat, eng = _engine(model, cuda)
    env = E.make("CartPole-v1", N, device=cuda, seed=31, max_episode_steps=maxs)
    ev = Evaluator(m, env, eng, None, E_)
    assert ev.path == "native" and ev.L == E_ * maxs
    ev.run()
    st = ev.storage
    acts, rew, don, obs = st.actions.cpu(), st.rewards.cpu(), st.dones.cpu(), st.obs.cpu()
    # the accounting, teacher-forced: the CPU bank from the device's recorded observation (CartPole's state) under the
    # device's recorded action, step by step
    assert torch.equal(env_cpu.reset(), obs[0])
    for t in range(ev.L):
        env_cpu.state.copy_(obs[t])
        o, r, d, _ = env_cpu.step(acts[t])
        assert torch.equal(d, don[t]) and torch.equal(r, rew[t]), t
        torch.testing.assert_close(o, obs[t + 1], rtol=1e-5, atol=1e-6)
    want = EV.EvalRecords(N, E_)
    EV.eval_scan_ref(rew, don, *want.tensors())
    r = ev.result()
    assert _same(r["ep_ret"], want.ep_ret.numpy()) and np.array_equal(r["ep_len"], want.ep_len.numpy())
    # every recorded action is the fp64 arg-max at the recorded observation (gap rule of the greedy test)
    flat_obs = obs[:ev.L].reshape(-1, 4)
    z64 = O.actor_fp64(model, flat_obs)
    with torch.no_grad():
        z32 = model.actor(flat_obs)
    a64, gap = O.argmax_gap(z64)
    keep = gap > 2 * SO.tolerance(SO.err(z32, z64)[0], float(z64.abs().max()))
    print(f"cartpole teacher-forced: {int((~keep).sum())} of {keep.numel()} rows inside the gap")
    assert torch.equal(acts.reshape(-1).long()[keep], a64[keep])
    assert float(keep.double().mean()) >= 0.95


# ------------------------------------------------------------------------------------------------ 6. isolation, capture
def _trainer(cuda, every, extras):
    from actor_critic_algs_on_tensorflow_amd.algos.trainer import ActorCriticTrainer
    kw = dict(num_envs=8, n_steps=16, ppo_epochs=1, ppo_minibatches=2, device="cuda:0", outdir=None, quiet=True,
              stdout_freq=0, save_every=0, cuda_graph=True, eval_every=every, eval_envs=5, eval_episodes=2)
    if extras:
        kw.update(norm_obs=True, norm_reward=True, bootstrap_on_timeout=True)
    cfg = preset("mujoco_ppo_dp8", **kw)
    env = E.make(cfg.env, 8, device=cuda, seed=cfg.seed, max_episode_steps=7)
    return ActorCriticTrainer(cfg, env=env)


@pytest.mark.parametrize("extras", [False, True])
def test_eval_every_is_isolated_and_captured(cuda, extras):
    on, off = _trainer(cuda, 1, extras), _trainer(cuda, 0, extras)
    assert on.evaluator.path == "fused" and on.evaluator.L == 14
    for tr in (on, off):
        tr.train(3)
    torch.cuda.synchronize()
    assert on.graph is not None and on.evaluator.graph is not None and len(on.eval_history) == 3
    assert torch.equal(on.flat.data, off.flat.data)
    for fa, fb in zip(list(on.mlp.F.values()) + list(on.mlp.G.values()),
                      list(off.mlp.F.values()) + list(off.mlp.G.values())):
        assert torch.equal(fa, fb)
    for g in on.opts:
        sa, sb = on.opts[g].state_dict(), off.opts[g].state_dict()
        for k in sa:
            assert torch.equal(sa[k], sb[k]), (g, k)
    if extras:
        for a, b in ((on.obs_norm, off.obs_norm), (on.reward_norm, off.reward_norm)):
            sa, sb = a.state_dict(), b.state_dict()
            for k in sa:
                assert torch.equal(torch.as_tensor(sa[k]), torch.as_tensor(sb[k])), k
        assert torch.equal(on.reward_norm.ret, off.reward_norm.ret)
    for name in ("state", "t", "tg", "ep_ret"):
        assert torch.equal(getattr(on.env, name), getattr(off.env, name)), name
    # ep_stats: episode count and length sum are sums of small integers, exact in any order; the return sum is added
    # with float atomics from the rollout's workgroups in whatever order they arrive, so two identical runs may differ
    # in its last bits, with or without evaluation -- bounded by n * 2^-24 * sum |return| for the n episodes summed
    assert torch.equal(on.env.ep_stats[1:], off.env.ep_stats[1:])
    n_ep = float(on.env.ep_stats[1])
    bound = n_ep * 2.0 ** -24 * n_ep * 7 * 2.0   # |return| <= 7 steps x |reward| < 2 each
    assert abs(float(on.env.ep_stats[0]) - float(off.env.ep_stats[0])) <= bound
    for name in ("obs", "actions", "logp", "entropy", "rewards", "dones", "truncated", "values"):
        assert torch.equal(getattr(on.storage, name), getattr(off.storage, name)), name
    # captured == eager, and replays with unchanged parameters repeat bit for bit
    ev = on.evaluator
    a = ev.evaluate()
    b = ev.evaluate()
    ev.run_eager()
    c = ev.result()
    for x in (b, c):
        assert _same(a["ep_ret"], x["ep_ret"]) and np.array_equal(a["ep_len"], x["ep_len"])
        assert all(a[k] == x[k] for k in EV.SUMMARY_KEYS)
    assert a["ret_mean"] == on.eval_history[-1]["eval_ret_mean"]
    assert math.isfinite(a["ret_mean"]) and a["episodes"] == 10 and a["len_mean"] == 7.0


# ------------------------------------------------------------------------------------------------ 7. launcher rejections
def test_eval_launcher_rejections(cuda):
    env_cpu, model, _ = _linear_setup(cuda, 1, 5, False)
    m, flat, eng = _engine(model, cuda)
    env = E.make("HalfCheetahShape-v0", 5, device=cuda, seed=4242, max_episode_steps=MAXS)
    obs0 = env.reset().clone()
    rec = EV.EvalRecords(5, EPS, cuda)
    before = [t.clone() for t in (env.state, env.t, env.tg, env.ep_ret, rec.ep_ret, rec.ep_len, rec.cnt)]
    desc, _ = eng.desc(None)
    ops = torch.ops.acamd

    def launch(records, final):
        r = rec.tensors() if records else (None, None, None)
        f = (torch.zeros(5, 3, 17, device=cuda), torch.full((5, 3), -1, dtype=torch.int32, device=cuda)) if final \
            else (None, None)
        ops.mlp_rollout_eval(desc, eng.rollout_lds_bytes(True), obs0, MAXS * EPS, eng.log_std, eng.ac_scale, env.state,
                             env.t, env.tg, env.ep_ret, env.env_ids, env.A, env.B, env.seed, MAXS, 1, True, *r, None,
                             0.0, *f)

    with pytest.raises(RuntimeError, match="mlp_rollout_eval launch failed"):
        launch(True, True)      # EVAL together with a final_obs workspace
    with pytest.raises(RuntimeError, match="mlp_rollout_eval launch failed"):
        launch(False, False)    # null storage without records
    torch.cuda.synchronize()
    after = (env.state, env.t, env.tg, env.ep_ret, rec.ep_ret, rec.ep_len, rec.cnt)
    for x, y in zip(before, after):
        assert _same(x.cpu().numpy(), y.cpu().numpy())   # nothing was launched
    launch(True, False)         # the accepted form runs
    torch.cuda.synchronize()
    assert bool((rec.cnt == EPS).all()) and bool((env.tg == MAXS * EPS).all())
