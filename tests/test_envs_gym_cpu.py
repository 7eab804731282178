"""Acrobot-v1, MountainCar-v0 and MountainCarContinuous-v0 banks on CPU: the torch oracles of ``envs/classic.py``
against an independent fp64 implementation of the gym equations (tests/oracles/gym_classic_oracle.py), planted goal
and wall cases, the bank mechanics every env shares, and the trainers on top."""
import math
import os
import sys

import numpy as np
import pytest
import torch

from actor_critic_algs_on_tensorflow_amd import envs as E
from actor_critic_algs_on_tensorflow_amd import preset
from actor_critic_algs_on_tensorflow_amd.algos.trainer import ActorCriticTrainer

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "oracles"))
import gym_classic_oracle as O  # noqa: E402

IDS = ["Acrobot-v1", "MountainCar-v0", "MountainCarContinuous-v0"]
LIMITS = {"Acrobot-v1": 500, "MountainCar-v0": 200, "MountainCarContinuous-v0": 999}
ORACLE = {"Acrobot-v1": O.acrobot_step, "MountainCar-v0": O.mountaincar_step,
          "MountainCarContinuous-v0": O.mountaincar_cont_step}


def _quiet(**kw):
    base = dict(outdir=None, quiet=True, stdout_freq=0, save_every=0, device="cpu", cuda_graph=False)
    base.update(kw)
    return base


def _planted(env_id, states, actions):
    """One step of a fresh bank from the given states: (state, obs, reward, done, truncated) after it, with the
    pre-reset frame in ``bank.final_obs``."""
    states = torch.as_tensor(states, dtype=torch.float32).reshape(-1, E.REGISTRY[env_id].state_dim)
    bank = E.make(env_id, states.shape[0], seed=3)
    bank.keep_final_obs = True
    bank.reset()
    bank.state.copy_(states)
    if bank.is_discrete:
        a = torch.as_tensor(actions, dtype=torch.int32).reshape(-1)
    else:
        a = torch.as_tensor(actions, dtype=torch.float32).reshape(-1, 1)
    bank.step(a, prev_obs=bank.obs.clone())
    return bank


def _random_states(env_id, n, g, vel=0.25):
    """Uniform states inside the clamp ranges. Acrobot's velocities span ``vel`` of theirs: the 1e-5 bar is an fp32
    bar only while the velocity-squared terms stay small. At the full range 0.5 * w2^2 reaches 400, one fp32 rounding
    of it (ulp 3e-5) moves the accelerations by 0.2 * 3e-5 / 0.57 = 1e-5 on its own, and fp32 against fp64 measures
    1.1e-4; at a quarter (w2^2 <= 50, 1.3e-6 per rounding) it measures 1.1e-6, the order the bar was set from."""
    u = torch.rand(n, 4, generator=g, dtype=torch.float64)
    if env_id == "Acrobot-v1":
        lo = torch.tensor([-math.pi, -math.pi, -4 * math.pi * vel, -9 * math.pi * vel])
        return (lo + u * (-2 * lo)).float()
    lo, hi = torch.tensor([-1.2, -0.07]), torch.tensor([0.6, 0.07])
    return (lo + u[:, :2] * (hi - lo)).float()


# ------------------------------------------------------------------------------------------------------ dynamics
@pytest.mark.parametrize("env_id", IDS)
def test_torch_oracle_matches_fp64_equations(env_id):
    """256 random in-range states x every action (continuous: 3 draws from +-3, so the force clamp and the unclipped
    penalty both act): the fp32 torch step against the fp64 oracle from the same fp32 state, atol 1e-5 (the bar of
    test_envs_cpu.py; numpy fp32 against fp64 differs by at most 8.4e-7 on Acrobot's observation and 6.5e-8 on
    MountainCar's state). Acrobot is compared through its observation: a wrap may land on either side of +-pi."""
    g = torch.Generator().manual_seed(11)
    states = _random_states(env_id, 256, g)
    if env_id == "MountainCarContinuous-v0":
        action_sets = [torch.rand(256, generator=g) * 6 - 3 for _ in range(3)]
        assert any(bool((a.abs() > 1).any()) for a in action_sets)
    else:
        action_sets = [torch.full((256,), a, dtype=torch.int32) for a in range(3)]
    n_term = 0
    for acts in action_sets:
        bank = _planted(env_id, states, acts)
        for i in range(256):
            s, r, term = ORACLE[env_id](states[i].double().numpy(), acts[i].item())
            if env_id == "Acrobot-v1":
                margin = abs(O.acrobot_height(s) - 1.0)
                want = O.acrobot_obs(s)
            else:
                goal = 0.5 if env_id == "MountainCar-v0" else 0.45
                margin = min(abs(s[0] - goal), abs(s[1]) if s[0] >= goal else 1.0)
                want = s
            assert np.allclose(bank.final_obs[i].double().numpy(), want, atol=1e-5), (env_id, i)
            if margin > 1e-4:   # away from the goal's edge both precisions decide alike
                assert bool(bank.done[i]) == term, (env_id, i)
                assert abs(float(bank.reward[i]) - r) <= 1e-5, (env_id, i)
                n_term += term
            assert not bool(bank.truncated[i])
    assert n_term > 0, "the random states must include goal states"


def test_acrobot_wraps_and_clamps_at_full_speed():
    """Velocities over the whole clamp range (where fp32 and fp64 part by up to 1e-4, see _random_states): the step
    agrees with the fp64 equations to rtol 1e-4 of the velocity scale, the angles come back inside [-pi, pi] and the
    velocities inside +-4 pi / +-9 pi, with states on both clamps and past both wraps among the 256."""
    g = torch.Generator().manual_seed(12)
    states = _random_states("Acrobot-v1", 256, g, vel=1.0)
    pi32 = float(torch.tensor(math.pi))
    wrapped = clamped = 0
    for a in range(3):
        bank = _planted("Acrobot-v1", states, torch.full((256,), a, dtype=torch.int32))
        for i in range(256):
            s, _, _ = O.acrobot_step(states[i].double().numpy(), a)
            assert np.allclose(bank.final_obs[i].double().numpy(), O.acrobot_obs(s), atol=1e-4 * 9 * math.pi), i
            clamped += abs(s[2]) == 4 * math.pi or abs(s[3]) == 9 * math.pi
            wrapped += abs(states[i, 1].item() + 0.2 * states[i, 3].item()) > 1.5 * math.pi
        fin = bank.final_obs
        assert (fin[:, 4].abs() <= float(torch.tensor(4 * math.pi))).all()
        assert (fin[:, 5].abs() <= float(torch.tensor(9 * math.pi))).all()
    assert clamped > 10 and wrapped > 10
    # the state itself (not reset here: nothing terminates below the bar with the tip held down) is wrapped
    b = _planted("Acrobot-v1", [[3.1, -3.1, 2.0, -25.0], [-3.1, 3.1, -12.0, 28.0]], [1, 1])
    for i in range(2):
        if not bool(b.done[i]):
            assert (b.state[i, :2].abs() <= pi32).all()


def test_acrobot_planted_swing_up():
    b = _planted("Acrobot-v1", [[2.5, 0.0, 0.0, 0.0]], [1])
    want = np.array([2.42426, 0.05893, -0.77069, 0.60548])
    assert bool(b.done[0]) and not bool(b.truncated[0]) and float(b.reward[0]) == 0.0
    assert np.allclose(b.final_obs[0].numpy(), O.acrobot_obs(want), atol=1e-4)
    assert abs(O.acrobot_height(want) - 1.54) < 0.01
    # the returned observation is the next episode's reset frame: every state component in [-0.1, 0.1)
    assert (b.state.abs() <= 0.1).all() and int(b.t[0]) == 0
    assert torch.allclose(b.obs[0, :4], torch.tensor([1.0, 0.0, 1.0, 0.0]), atol=0.1)
    assert float(b.ep_stats[1]) == 1.0 and float(b.ep_stats[0]) == 0.0 and float(b.ep_stats[2]) == 1.0


def test_mountaincar_planted_goal_and_wall():
    b = _planted("MountainCar-v0", [[0.49, 0.05], [-1.19, -0.05]], [2, 0])
    assert abs(float(b.final_obs[0, 0]) - 0.54075) < 1e-5
    assert b.done.tolist() == [1, 0] and b.truncated.tolist() == [0, 0]
    assert b.reward.tolist() == [-1.0, -1.0]
    # the left wall: the clamp bound exactly, and the velocity of a car that still moved left is zeroed
    assert float(b.state[1, 0]) == float(torch.tensor(-1.2)) and float(b.state[1, 1]) == 0.0
    assert torch.equal(b.obs[1], b.state[1]) and torch.equal(b.final_obs[1], b.state[1])
    # env 0 was reset: p in [-0.6, -0.4), v = 0
    assert -0.6 <= float(b.state[0, 0]) < -0.4 and float(b.state[0, 1]) == 0.0


def test_mountaincar_continuous_planted_goal_and_wall():
    b = _planted("MountainCarContinuous-v0", [[0.44, 0.05], [-1.19, -0.05]], [1.7, -3.0])
    assert abs(float(b.final_obs[0, 0]) - 0.49088) < 1e-5
    assert b.done.tolist() == [1, 0] and b.truncated.tolist() == [0, 0]
    # force clamped to 1 (p would be 0.49193 at 1.7), penalty from the unclipped action: 100 - 0.1 * 1.7^2
    assert abs(float(b.reward[0]) - 99.711) < 1e-4
    assert abs(float(b.reward[1]) + 0.9) < 1e-6
    assert float(b.state[1, 0]) == float(torch.tensor(-1.2)) and float(b.state[1, 1]) == 0.0
    # the discrete task's goal (0.5) is not reached from there: the two tasks differ in their threshold
    d = _planted("MountainCar-v0", [[0.44, 0.05]], [2])
    assert not bool(d.done[0])


# ------------------------------------------------------------------------------------------------------ bank mechanics
def test_registry_and_roll_params():
    want = {"Acrobot-v1": ((500, 2000), (500, 3000)), "MountainCar-v0": ((200, 800), (200, 1200)),
            "MountainCarContinuous-v0": ((999, 3000), (999, 3000))}
    for env_id, (basic, a3c) in want.items():
        assert E.get_roll_params(env_id, "basic") == basic
        assert E.get_roll_params(env_id, "a3c") == a3c
        assert E.REGISTRY[env_id].__name__ in E.__all__
    acro, car, cont = (E.make(i, 2) for i in IDS)
    assert acro.action_space.n == 3 and acro.reset().shape == (2, 6) and acro.state.shape == (2, 4)
    assert car.action_space.n == 3 and car.reset().shape == (2, 2)
    assert not cont.is_discrete and cont.action_space.shape == (1,) and cont.reset().shape == (2, 2)
    assert float(cont.action_space.low[0]) == -1.0 and float(cont.action_space.high[0]) == 1.0
    for bank in (acro, car, cont):
        assert bank.native_final_obs


@pytest.mark.parametrize("env_id", IDS)
@pytest.mark.parametrize("limit", [None, 3])
def test_time_limits_and_autoreset(env_id, limit):
    """The idle action (no torque / no push) never reaches a goal, so every episode ends at the time limit: gym's
    TimeLimit value by default, ``max_episode_steps`` when given. Resets re-draw the start state; ``ep_stats`` counts
    the finished episodes, their lengths and their returns."""
    bank = E.make(env_id, 3, seed=0, max_episode_steps=limit)
    L = LIMITS[env_id] if limit is None else limit
    assert bank.spec.max_episode_steps == L
    bank.reset()
    start = bank.state.clone()
    idle = torch.ones(3, dtype=torch.int32) if bank.is_discrete else torch.zeros(3, 1)
    for t in range(1, 2 * L + 1):
        _, r, d, info = bank.step(idle, prev_obs=bank.obs.clone())
        ends = t % L == 0
        assert d.tolist() == [int(ends)] * 3 and info["truncated"].tolist() == [int(ends)] * 3, (env_id, t)
        if ends:
            assert (bank.t == 0).all() and (bank.ep_ret == 0).all()
            assert not torch.equal(bank.state, start)          # a fresh draw, keyed on the global step
            if env_id != "Acrobot-v1":
                assert (bank.state[:, 1] == 0).all() and ((bank.state[:, 0] >= -0.6) & (bank.state[:, 0] < -0.4)).all()
            else:
                assert (bank.state.abs() <= 0.1).all()
    per_step = 0.0 if env_id == "MountainCarContinuous-v0" else -1.0
    s = bank.ep_stats
    assert int(s[1]) == 6 and float(s[2]) == 6 * L and abs(float(s[0]) - 6 * L * per_step) < 1e-3


@pytest.mark.parametrize("env_id", IDS)
def test_frame_stack_vector(env_id):
    bank = E.make(env_id, 2, seed=0, frame_stack=3, max_episode_steps=2)
    D = bank.frame_shape[0]
    o0 = bank.reset().clone()
    assert o0.shape == (2, 3 * D) and torch.equal(o0[:, :D], o0[:, 2 * D:])
    a = torch.full((2,), 2, dtype=torch.int32) if bank.is_discrete else torch.full((2, 1), 0.5)
    o1 = bank.step(a, prev_obs=o0)[0].clone()
    assert torch.equal(o1[:, :2 * D], o0[:, D:]) and not torch.equal(o1[:, 2 * D:], o0[:, 2 * D:])
    assert torch.equal(o1[:, 2 * D:], bank._frame())
    o2 = bank.step(a, prev_obs=o1)[0]          # the time limit: the stack restarts as three copies of the reset frame
    assert bank.done.all()
    assert torch.equal(o2[:, :D], o2[:, D:2 * D]) and torch.equal(o2[:, :D], o2[:, 2 * D:])
    assert torch.equal(o2[:, 2 * D:], bank._frame())


@pytest.mark.parametrize("env_id", IDS)
def test_env_partitioning_is_rank_invariant(env_id):
    """Resets keyed by the global env id: a 2-rank split reproduces the 1-rank bank, at reset and after auto-resets."""
    banks = [E.make(env_id, 4, seed=9, max_episode_steps=2), E.make(env_id, 2, seed=9, max_episode_steps=2),
             E.make(env_id, 2, seed=9, max_episode_steps=2, env_offset=2)]
    for b in banks:
        b.reset()
    full, lo, hi = banks
    assert torch.equal(full.state[:2], lo.state) and torch.equal(full.state[2:], hi.state)
    assert not torch.equal(lo.state, hi.state)
    for _ in range(3):
        for b in banks:
            a = torch.zeros(b.num_envs, dtype=torch.int32) if b.is_discrete else torch.full((b.num_envs, 1), -0.3)
            b.step(a, prev_obs=b.obs.clone())
        assert torch.equal(full.state[:2], lo.state) and torch.equal(full.state[2:], hi.state)
        assert torch.equal(full.obs[2:], hi.obs)


# ------------------------------------------------------------------------------------------------------ trainers
def test_acrobot_preset():
    cfg = preset("acrobot_ppo")
    assert (cfg.env, cfg.algo, cfg.num_envs, cfg.n_steps) == ("Acrobot-v1", "ppo", 16, 128)
    assert (cfg.ppo_epochs, cfg.ppo_minibatches, cfg.lr, cfg.critic_lr) == (4, 4, 1e-3, 1e-3)
    assert (cfg.gamma, cfg.returns, cfg.gae_lambda, cfg.norm_adv, cfg.ent_coef) == (0.99, "gae", 0.95, True, 0.0)
    assert (cfg.model_variant, cfg.dtype, cfg.device) == ("basic", "fp32", "cuda")


@pytest.mark.parametrize("env_id", IDS)
@pytest.mark.parametrize("algo", ["ppo", "a2c"])
def test_trainers_step(env_id, algo):
    cfg = preset("acrobot_ppo", **_quiet(env=env_id, algo=algo, num_envs=4, n_steps=8, ppo_epochs=2,
                                         ppo_minibatches=2))
    tr = ActorCriticTrainer(cfg)
    assert tr.env.env_id == env_id
    p0 = tr.flat.data.clone()
    for _ in range(2):
        tr.step()
    assert torch.isfinite(tr.flat.data).all() and (tr.flat.data != p0).any()
    assert tr.storage.actions.shape[1:] == ((4,) if tr.env.is_discrete else (4, 1))


def test_bootstrap_on_timeout_with_terminations_and_truncations():
    """MountainCarContinuous with a 3-step limit and two envs planted at the goal's edge: one rollout holds terminated
    steps and truncated steps. Only the truncated ones get gamma * V(terminal observation) on top of the env reward;
    a terminated step keeps its raw reward (the 100 bonus included)."""
    gamma = 0.9
    kw = dict(seed=5, max_episode_steps=3)

    def plant(b):
        b.state[0] = torch.tensor([0.449, 0.06])    # reaches 0.45 whatever the action: |dv| <= 0.004 per step
        b.state[2] = torch.tensor([0.44, 0.05])
        return b._frame()

    cfg = preset("acrobot_ppo", **_quiet(env="MountainCarContinuous-v0", num_envs=4, n_steps=7, gamma=gamma,
                                         bootstrap_on_timeout=True, norm_adv=False))
    tr = ActorCriticTrainer(cfg, env=E.make("MountainCarContinuous-v0", 4, **kw))
    st = tr.storage
    st.obs[0].copy_(plant(tr.env))               # the rollout starts from the planted states
    tr.collect()
    twin = E.make("MountainCarContinuous-v0", 4, **kw)
    twin.keep_final_obs = True
    twin.reset()
    twin.obs.copy_(plant(twin))
    n_term = n_trunc = 0
    with torch.no_grad():
        for t in range(7):
            _, r, d, info = twin.step(st.actions[t], prev_obs=twin.obs.clone())
            trunc = info["truncated"].bool()
            term = d.bool() & ~trunc
            assert torch.equal(d, st.dones[t]) and torch.equal(info["truncated"], st.truncated[t])
            boot = gamma * tr.model.value(twin.final_obs)
            assert torch.allclose(st.rewards[t][trunc], (r + boot)[trunc], atol=1e-6)
            assert torch.equal(st.rewards[t][~trunc], r[~trunc])
            assert (r[term] > 90).all()
            n_term += int(term.sum())
            n_trunc += int(trunc.sum())
    assert n_term >= 2 and n_trunc >= 4
    assert bool(st.dones[0, 0]) and not bool(st.truncated[0, 0])
