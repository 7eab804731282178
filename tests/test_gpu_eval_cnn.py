"""Deterministic evaluation of the native CNN engine: ``env_policy_eval_pong`` (greedy head + env step + episode records)
and the Evaluator's ``"cnn"`` path, eager, chunk-captured and inside a trainer.

Test weights: random-init CNN logits cannot test an arg-max (every top-2 gap of the default init on Pong frames lies
inside the bf16 forward bar ``3e-2 * (max|z| + 1e-2)`` of test_cnn_engine_matches_autograd), so the heads kernel is
``0.05 * randn`` from a head seed and every parameter is rounded to bf16. Such a policy takes one action throughout:
head seeds 5 / 8 / 22 give up (2), stay (1) and down (3) on the Pong bank, so all three physics candidates get
committed. The opponent's score is set to 20 in the evaluator's snapshot, so first episodes end by score and later
ones by the time limit. Bars come from references alone, never from a kernel's output."""
import copy
import functools
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
from actor_critic_algs_on_tensorflow_amd.algos.evaluator import Evaluator, chunk_plan  # noqa: E402
from actor_critic_algs_on_tensorflow_amd.models.policy import build_model  # noqa: E402
from actor_critic_algs_on_tensorflow_amd.ops import evaluation as EV  # noqa: E402
from actor_critic_algs_on_tensorflow_amd.ops.optim import FlatParams  # noqa: E402

pytestmark = pytest.mark.gpu

PONG, BREAKOUT, BANK_SEED = "PongNoFrameskip-v4", "BreakoutNoFrameskip-v4", 31
# (env id, N, max_episode_steps, episodes, head seed, chunk_steps of the captured run)
SETUPS = {
    "pong5-up": (PONG, 5, 12, 2, 5, 10),        # L = 24: two chunk replays and a tail of 4
    "pong5-stay": (PONG, 5, 12, 2, 8, 10),
    "pong5-down": (PONG, 5, 12, 2, 22, 10),
    "breakout3": (BREAKOUT, 3, 12, 2, 5, 10),
    "pong1": (PONG, 1, 5, 1, 5, 2),             # odd L = 5: two chunks and a tail of 1
    "pong65": (PONG, 65, 4, 1, 5, 2),           # per-env trunk; L = 4: two chunks, empty tail
}
DIRECTION = {"pong5-up": {2, 4}, "pong5-stay": {0, 1}, "pong5-down": {3, 5}}


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@functools.lru_cache(maxsize=None)
def _recipe(env_id, hs):
    env = E.make(env_id, 1, device="cpu", frame_stack=4)
    m = build_model(env, "cnn", "basic", seed=3)
    with torch.no_grad():
        k = m.net.heads.kernel
        k.copy_(0.05 * torch.randn(k.shape, generator=torch.Generator().manual_seed(hs)))
        for p in m.parameters():
            p.copy_(p.to(torch.bfloat16).float())
    return m


def _engine(model_cpu, cuda):
    from actor_critic_algs_on_tensorflow_amd.algos.engine import CNNEngine
    m = copy.deepcopy(model_cpu).to(cuda)
    flat = FlatParams(m.param_groups(), cuda)
    return m, CNNEngine(m, flat, flat.data.to(torch.bfloat16))


def _evaluator(cuda, name, **kw):
    env_id, N, maxs, E_, hs, _ = SETUPS[name]
    m, eng = _engine(_recipe(env_id, hs), cuda)
    env = E.make(env_id, N, device=cuda, seed=BANK_SEED, frame_stack=4, max_episode_steps=maxs)
    ev = Evaluator(m, env, eng, None, E_, **kw)
    assert ev.path == "cnn" and ev.L == E_ * maxs
    ev._snap["state"][:, 7] = 20.0
    return ev, eng


def _final(env):
    return {k: getattr(env, k).cpu().clone() for k in ("state", "t", "tg", "ep_ret")}


@functools.lru_cache(maxsize=None)
def _keep_run(cuda, name):
    """One ``keep_steps`` evaluation of a setup: its result, stored columns and final bank, on the host (shared by the
    accounting test and the production-path test, computed once)."""
    ev, eng = _evaluator(cuda, name, keep_steps=True)
    stats0, fc0 = ev.env.ep_stats.clone(), eng.last_fc
    r = ev.evaluate()
    st = ev.storage
    return dict(result=r, obs=st.obs.cpu(), acts=st.actions.cpu(), rew=st.rewards.cpu(), don=st.dones.cpu(),
                final=_final(ev.env), snap={k: v.cpu() for k, v in ev._snap.items()}, obs0=ev.obs0.cpu(),
                stats_untouched=torch.equal(ev.env.ep_stats, stats0), last_fc_kept=eng.last_fc is fc0)


# ------------------------------------------------------------------------------------------------ A. the greedy head
def _direct_bank(cuda, N):
    env = E.make(PONG, N, device=cuda, seed=BANK_SEED, frame_stack=4, max_episode_steps=12)
    obs0 = env.reset().clone()
    snap = {k: getattr(env, k).clone() for k in ("state", "t", "tg", "ep_ret")}
    return env, obs0, snap


def _direct_step(cuda, env, obs0, snap, h, Wh, bh, tg=None, E_=1, rec=None, with_rec=True):
    for k, v in snap.items():
        getattr(env, k).copy_(v)
    if tg is not None:
        env.tg.fill_(tg)
    N = env.num_envs
    out = torch.zeros_like(obs0)
    act = torch.full((N,), -7, dtype=torch.int32, device=cuda)
    rew = torch.full((N,), -7.0, device=cuda)
    don = torch.full((N,), 7, dtype=torch.uint8, device=cuda)
    rec = rec if rec is not None else EV.EvalRecords(N, max(E_, 1), cuda)
    r = rec.tensors() if with_rec else (None, None, None)
    torch.ops.acamd.env_policy_eval_pong(h, Wh, bh, env.state, env.t, env.tg, env.ep_ret, env.env_ids, obs0, out,
                                         env.seed, env.max_episode_steps, 4, False, None, 0, None, *r, E_, act, rew,
                                         don)
    return act, rew, don, out


@functools.lru_cache(maxsize=None)
def _head_case(A, N):
    g = torch.Generator().manual_seed(1000 * A + N)
    h = torch.relu(torch.randn(N, 512, generator=g)).to(torch.bfloat16)
    Wh = (0.05 * torch.randn(512, A + 1, generator=g)).to(torch.bfloat16)
    bh = 0.1 * torch.randn(A + 1, generator=g)
    z64 = h.double() @ Wh.double() + bh.double()
    z32 = h.float() @ Wh.float() + bh
    act, gap = O.argmax_gap(z64[:, :A])
    bar = SO.tolerance(SO.err(z32, z64)[0], float(z64.abs().max()))
    return h, Wh, bh, act, gap, gap > 2 * bar, bar


@pytest.mark.parametrize("N", [1, 5, 65])
@pytest.mark.parametrize("A", [4, 6])
def test_greedy_head_against_fp64(cuda, A, N):
    h, Wh, bh, want, gap, keep, bar = _head_case(A, N)
    assert float(keep.double().mean()) >= 0.95, "the reference alone must keep 95 % of the rows"
    env, obs0, snap = _direct_bank(cuda, N)
    hd, Wd, bd = h.to(cuda), Wh.to(cuda), bh.to(cuda)
    act, rew, don, out = _direct_step(cuda, env, obs0, snap, hd, Wd, bd)
    print(f"greedy head A={A} N={N}: smallest gap {float(gap.min()):.3e}, bar {bar:.3e}, rows left out "
          f"{int((~keep).sum())}")
    assert torch.equal(act.cpu().long()[keep], want[keep])
    assert bool(((act >= 0) & (act < A)).all())
    # the env step took that action: the plain env kernel from the same state gives the same transition
    ref_env, ref_obs0, _ = _direct_bank(cuda, N)
    o2, r2, d2, _ = ref_env.step(act, prev_obs=ref_obs0, obs_out=torch.zeros_like(ref_obs0))
    assert torch.equal(out, o2) and torch.equal(rew, r2) and torch.equal(don, d2)
    for k in ("state", "t", "tg", "ep_ret"):
        assert torch.equal(getattr(env, k), getattr(ref_env, k)), k
    # no random number: the op takes no policy seed, and the env counter (the samplers' key) changes nothing
    act2, _, _, _ = _direct_step(cuda, env, obs0, snap, hd, Wd, bd, tg=1 << 33)
    assert torch.equal(act, act2)


def test_greedy_head_ties_take_the_first_index(cuda):
    N, A = 5, 6
    env, obs0, snap = _direct_bank(cuda, N)
    h = torch.relu(torch.randn(N, 512, generator=torch.Generator().manual_seed(1))).to(torch.bfloat16).to(cuda)
    Wz = torch.zeros(512, A + 1, dtype=torch.bfloat16, device=cuda)
    act, _, _, _ = _direct_step(cuda, env, obs0, snap, h, Wz, torch.zeros(A + 1, device=cuda))
    assert bool((act == 0).all())
    bh = torch.tensor([0.0, -1.0, 0.5, 0.25, 0.5, -2.0, 9.0], device=cuda)   # maxima at 2 and 4; 9 is the value
    act, _, _, _ = _direct_step(cuda, env, obs0, snap, h, Wz, bh)
    assert bool((act == 2).all())
    # a NaN logit never wins; all NaN gives 0 (the greedy rule of the MLP engine)
    nan = float("nan")
    act, _, _, _ = _direct_step(cuda, env, obs0, snap, h, Wz, torch.tensor([nan, 0.1, nan, 0.3, 0.3, nan, 1.0],
                                                                         device=cuda))
    assert bool((act == 3).all())
    act, _, _, _ = _direct_step(cuda, env, obs0, snap, h, Wz, torch.tensor([nan] * 6 + [1.0], device=cuda))
    assert bool((act == 0).all())


# ------------------------------------------------------------------------------------------------ B. accounting
@pytest.mark.parametrize("name", list(SETUPS))
def test_teacher_forced_accounting(cuda, name):
    env_id, N, maxs, E_, hs, _ = SETUPS[name]
    run = _keep_run(cuda, name)
    L = E_ * maxs
    obs, acts, rew, don = run["obs"], run["acts"], run["rew"], run["don"]
    # the CPU bank from the same snapshot under the device's recorded actions
    cpu = E.make(env_id, N, device="cpu", seed=BANK_SEED, frame_stack=4, max_episode_steps=maxs)
    assert torch.equal(cpu.reset(), run["obs0"]) and torch.equal(obs[0], run["obs0"])
    for k, v in run["snap"].items():
        getattr(cpu, k).copy_(v)
    assert bool((cpu.state[:, 7] == 20.0).all())
    for t in range(L):
        o, r, d, _ = cpu.step(acts[t])
        assert torch.equal(r, rew[t]) and torch.equal(d, don[t]), t
        assert torch.equal(o, obs[t + 1]), t
    for k, v in run["final"].items():
        assert _same(getattr(cpu, k).numpy(), v.numpy()), k
    want = EV.EvalRecords(N, E_)
    EV.eval_scan_ref(rew, don, *want.tensors())
    r = run["result"]
    assert _same(r["ep_ret"], want.ep_ret.numpy()) and np.array_equal(r["ep_len"], want.ep_len.numpy())
    assert np.array_equal(r["cnt"], want.cnt.numpy()) and r["path"] == "cnn"
    assert run["stats_untouched"] and run["last_fc_kept"]
    # every recorded action is an arg-max of the fp32 torch model (bf16-rounded parameters) at the recorded
    # observation, within twice the engine's forward bar; no row is left out
    model = _recipe(env_id, hs)
    A = model.net.num_actions
    with torch.no_grad():
        logits, v = model(obs[:L].reshape((L * N,) + tuple(obs.shape[2:])))
    z = torch.cat([logits, v[:, None]], 1)
    tol = 3e-2 * (float(z.abs().max()) + 1e-2)
    a = acts.reshape(-1).long()
    assert bool(((a >= 0) & (a < A)).all())
    _, gap = O.argmax_gap(logits.double())
    share = float((gap > 2 * tol).double().mean())
    print(f"{name}: lengths {sorted(set(r['ep_len'].reshape(-1).tolist()))}, returns "
          f"{sorted(set(r['ep_ret'].reshape(-1).tolist()))}, actions {sorted(set(a.tolist()))}, gap > 2 tol on "
          f"{share:.3f} of the steps, worst gap / tol {float(gap.min()) / tol:.2f}")
    assert share >= 0.95, "the reference alone must be decisive on 95 % of the steps"
    assert bool((logits.gather(1, a[:, None])[:, 0] >= logits.max(1).values - 2 * tol).all())
    if name in DIRECTION:
        assert set(a.tolist()) <= DIRECTION[name]
    if name == "pong5-up":   # episodes of both kinds: ended by the score and cut by the limit
        assert r["ep_len"].min() < maxs and r["ep_len"].max() == maxs


# ------------------------------------------------------------------------------------------------ C. production path
@pytest.mark.parametrize("name", list(SETUPS))
def test_production_path_equals_keep_steps(cuda, name):
    env_id, N, maxs, E_, hs, chunk = SETUPS[name]
    keep = _keep_run(cuda, name)
    want = keep["result"]
    got = {}
    for mode in ("eager", "captured"):
        ev, eng = _evaluator(cuda, name, cuda_graph=mode == "captured", chunk_steps=chunk)
        assert ev.storage is None and ev._obs.shape[0] == 2
        fc0 = eng.last_fc
        a = ev.evaluate()
        fin = _final(ev.env)
        b = ev.evaluate()
        if mode == "captured":
            q, tail = chunk_plan(ev.L, chunk)
            assert (ev.graph.q, ev.graph.chunk is not None) == (q, q > 0) and q * chunk + tail == ev.L
        else:
            assert ev.graph is None
        for x in (a, b):
            assert _same(x["ep_ret"], want["ep_ret"]) and np.array_equal(x["ep_len"], want["ep_len"])
            assert np.array_equal(x["cnt"], want["cnt"]) and all(x[k] == want[k] for k in EV.SUMMARY_KEYS)
        for k, v in keep["final"].items():   # no early exit: the bank ends where the kept run's did
            assert _same(fin[k].numpy(), v.numpy()), (mode, k)
            assert _same(getattr(ev.env, k).cpu().numpy(), v.numpy()), (mode, k)
        assert eng.last_fc is fc0 and not bool(ev.env.ep_stats.any())
        got[mode] = a
    assert _same(got["eager"]["ep_ret"], got["captured"]["ep_ret"])


# ------------------------------------------------------------------------------------------------ D. trainer
def _trainer(cuda, every):
    from actor_critic_algs_on_tensorflow_amd.algos.trainer import ActorCriticTrainer
    cfg = preset("pong_a2c", num_envs=4, n_steps=5, device="cuda:0", outdir=None, quiet=True, stdout_freq=0,
                 save_every=0, cuda_graph=True, eval_every=every, eval_envs=4, eval_episodes=1)
    env = E.make(cfg.env, 4, device=cuda, seed=cfg.seed, max_episode_steps=6)
    return ActorCriticTrainer(cfg, env=env)


def test_eval_every_is_isolated_in_the_cnn_trainer(cuda):
    on, off = _trainer(cuda, 1), _trainer(cuda, 0)
    assert on.engine is not None and on.evaluator.path == "cnn" and on.evaluator.engine is on.engine
    assert on.evaluator.N == on.env.num_envs and on.evaluator.L == 6
    for tr in (on, off):
        tr.train(3)
    torch.cuda.synchronize()
    assert on.graph is not None and on.evaluator.graph is not None and len(on.eval_history) == 3
    assert torch.equal(on.flat.data, off.flat.data) and torch.equal(on.shadow, off.shadow)
    for fa, fb in zip(on.engine.frag + [on.engine.wfc_frag], off.engine.frag + [off.engine.wfc_frag]):
        assert torch.equal(fa, fb)
    for g in on.opts:
        sa, sb = on.opts[g].state_dict(), off.opts[g].state_dict()
        for k in sa:
            assert torch.equal(torch.as_tensor(sa[k]), torch.as_tensor(sb[k])), (g, k)
    for name in ("state", "t", "tg", "ep_ret", "ep_stats"):   # returns are sums of +-1: exact in any order
        assert torch.equal(getattr(on.env, name), getattr(off.env, name)), name
    assert on.storage.phase == off.storage.phase and torch.equal(on.storage.slots, off.storage.slots)
    for name in ("actions", "logp", "entropy", "rewards", "dones", "truncated", "values"):
        assert torch.equal(getattr(on.storage, name), getattr(off.storage, name)), name
    r = on.evaluate()
    assert r["path"] == "cnn" and r["episodes"] == 4 and r["len_mean"] == 6.0
    assert r["ret_mean"] == on.eval_history[-1]["eval_ret_mean"]
    assert not bool(on.evaluator.env.ep_stats.any())


# ------------------------------------------------------------------------------------------------ E. rejections
def test_eval_step_launcher_rejections(cuda):
    N, A = 5, 6
    env, obs0, snap = _direct_bank(cuda, N)
    g = torch.Generator().manual_seed(3)
    h = torch.relu(torch.randn(N, 512, generator=g)).to(torch.bfloat16).to(cuda)
    Wh = (0.05 * torch.randn(512, A + 1, generator=g)).to(torch.bfloat16).to(cuda)
    bh = (0.1 * torch.randn(A + 1, generator=g)).to(cuda)
    rec = EV.EvalRecords(N, 2, cuda)
    before = [t.clone() for t in (env.state, env.t, env.tg, env.ep_ret, rec.ep_ret, rec.ep_len, rec.cnt)]
    outs = []
    with pytest.raises(RuntimeError, match="env_policy_eval_pong launch failed"):
        outs.append(_direct_step(cuda, env, obs0, snap, h, Wh, bh, E_=0, rec=rec))
    with pytest.raises(RuntimeError, match="env_policy_eval_pong launch failed"):
        outs.append(_direct_step(cuda, env, obs0, snap, h, Wh, bh, E_=2, rec=rec, with_rec=False))
    W9 = torch.zeros(512, 9, dtype=torch.bfloat16, device=cuda)
    with pytest.raises(RuntimeError, match="env_policy_eval_pong launch failed"):
        outs.append(_direct_step(cuda, env, obs0, snap, h, W9, torch.zeros(9, device=cuda), E_=2, rec=rec))
    torch.cuda.synchronize()
    after = (env.state, env.t, env.tg, env.ep_ret, rec.ep_ret, rec.ep_len, rec.cnt)
    for x, y in zip(before, after):
        assert _same(x.cpu().numpy(), y.cpu().numpy())   # nothing was launched
    act, _, _, _ = _direct_step(cuda, env, obs0, snap, h, Wh, bh, E_=2, rec=rec)   # the accepted form runs
    torch.cuda.synchronize()
    assert bool((env.tg == 1).all()) and bool(((act >= 0) & (act < A)).all())
