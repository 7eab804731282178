"""Acrobot-v1, MountainCar-v0 and MountainCarContinuous-v0 on an MI355X: their tasks of csrc/kernels/env_classic.hip
against their torch oracles (envs/classic.py), planted goal / wall states on the device, the native MLP engine on
the three banks against the torch engine, and the ``acrobot_ppo`` preset learning on the native engine."""
import math

import pytest
import torch

from actor_critic_algs_on_tensorflow_amd import envs as E
from actor_critic_algs_on_tensorflow_amd import preset

pytestmark = pytest.mark.gpu

IDS = ["Acrobot-v1", "MountainCar-v0", "MountainCarContinuous-v0"]


def _quiet(**kw):
    base = dict(outdir=None, quiet=True, stdout_freq=0, save_every=0, device="cuda:0")
    base.update(kw)
    return base


# ------------------------------------------------------------------------------------------------------ kernel vs oracle
@pytest.mark.parametrize("N", [16, 300])
@pytest.mark.parametrize("env_id", IDS)
def test_env_bank_matches_oracle(cuda, env_id, N):
    """The form of test_gpu_kernels.py::test_env_bank_matches_oracle: 60 random-action steps from reset, state and
    observation re-synced from the CPU bank after each. N = 300 runs a second, partly filled workgroup. No episode
    ends within 60 steps of a reset (MountainCar cannot climb out that fast; Acrobot's tip stays at least 0.036 below
    the bar under random torques), so no goal test can fall on different sides in the two banks."""
    gpu = E.make(env_id, N, device=cuda, seed=5)
    cpu = E.make(env_id, N, device="cpu", seed=5)
    gpu.reset()
    cpu.reset()
    gpu.state.copy_(cpu.state)
    gpu.obs.copy_(cpu.obs)
    g = torch.Generator().manual_seed(1)
    for t in range(60):
        a = cpu.sample_actions(generator=g)
        prev_c, prev_g = cpu.obs.clone(), gpu.obs.clone()
        oc, rc, dc, _ = cpu.step(a, prev_obs=prev_c, obs_out=cpu.obs)
        og, rg, dg, _ = gpu.step(a.to(cuda), prev_obs=prev_g, obs_out=gpu.obs)
        assert not dc.any() and not dg.any(), (env_id, t)
        assert not gpu.truncated.any()
        assert torch.allclose(rc, rg.cpu(), rtol=1e-4, atol=1e-4), (env_id, t)
        assert torch.allclose(oc, og.cpu(), rtol=1e-4, atol=1e-4), (env_id, t)
        if env_id != "Acrobot-v1":   # Acrobot is compared by its observation: a wrap may land on either side of +-pi
            assert torch.allclose(cpu.state, gpu.state.cpu(), rtol=1e-4, atol=1e-4), (env_id, t)
        gpu.state.copy_(cpu.state)  # keep chaotic dynamics from drifting apart by ulps
        gpu.obs.copy_(cpu.obs)
    assert torch.equal(cpu.t, gpu.t.cpu()) and torch.equal(cpu.tg, gpu.tg.cpu())
    assert torch.allclose(cpu.ep_ret, gpu.ep_ret.cpu(), rtol=1e-4, atol=1e-3)
    assert torch.equal(cpu.ep_stats, gpu.ep_stats.cpu()) and float(cpu.ep_stats[1]) == 0.0


@pytest.mark.parametrize("env_id", IDS)
def test_env_bank_final_obs_matches_oracle(cuda, env_id):
    """The form of test_gpu_kernels.py::test_env_bank_final_obs_matches_oracle: a 3-step time limit, so every third
    step truncates, writes the pre-reset stack to final_out and returns the reset frame."""
    N = 2
    gpu = E.make(env_id, N, device=cuda, seed=5, max_episode_steps=3)
    cpu = E.make(env_id, N, device="cpu", seed=5, max_episode_steps=3)
    assert gpu.native_final_obs
    for bank in (gpu, cpu):
        bank.keep_final_obs = True
        bank.reset()
    gpu.state.copy_(cpu.state)
    gpu.obs.copy_(cpu.obs)
    g = torch.Generator().manual_seed(1)
    resets = 0
    for t in range(7):
        a = cpu.sample_actions(generator=g)
        prev_c, prev_g = cpu.obs.clone(), gpu.obs.clone()
        oc, rc, dc, ic = cpu.step(a, prev_obs=prev_c, obs_out=cpu.obs)
        og, rg, dg, ig = gpu.step(a.to(cuda), prev_obs=prev_g, obs_out=gpu.obs)
        assert torch.equal(dc, dg.cpu()) and torch.equal(ic["truncated"], ig["truncated"].cpu()), (env_id, t)
        assert torch.allclose(cpu.final_obs, gpu.final_obs.cpu(), rtol=1e-4, atol=1e-4), (env_id, t)
        assert torch.allclose(oc, og.cpu(), rtol=1e-4, atol=1e-4), (env_id, t)
        if bool(dc.all()):   # the terminal stack is the pre-reset observation, not the reset one that follows
            resets += 1
            assert ig["truncated"].all()
            assert not torch.equal(gpu.final_obs, og), (env_id, t)
        gpu.state.copy_(cpu.state)
        gpu.obs.copy_(cpu.obs)
    assert resets >= 2
    assert torch.allclose(cpu.ep_stats, gpu.ep_stats.cpu(), rtol=1e-4, atol=1e-3) and float(cpu.ep_stats[1]) == 4.0


# ------------------------------------------------------------------------------------------------------ planted cases
# (state, action, terminated, reward, pre-reset state to atol 1e-4 or exactly); expected values from the fp64 oracle
# (tests/oracles/gym_classic_oracle.py), each with a wide margin to its goal threshold
WALL = (float(torch.tensor(-1.2)), 0.0)
PLANTED = {
    "Acrobot-v1": [((2.5, 0.0, 0.0, 0.0), 1, True, 0.0, (2.42426, 0.05893, -0.77069, 0.60548), False),
                   ((0.0, 0.0, 0.0, 0.0), 1, False, -1.0, (0.0, 0.0, 0.0, 0.0), False)],
    "MountainCar-v0": [((0.49, 0.05), 2, True, -1.0, (0.54075, 0.05075), False),
                       ((-1.19, -0.05), 0, False, -1.0, WALL, True)],
    "MountainCarContinuous-v0": [((0.44, 0.05), 1.7, True, 99.711, (0.49088, 0.05088), False),
                                 ((-1.19, -0.05), -3.0, False, -0.9, WALL, True)],
}


def _frame(env_id, s):
    s = torch.as_tensor(s, dtype=torch.float64)
    if env_id == "Acrobot-v1":
        return torch.stack([s[0].cos(), s[0].sin(), s[1].cos(), s[1].sin(), s[2], s[3]]).float()
    return s.float()


@pytest.mark.parametrize("env_id,frame_stack", [(i, 1) for i in IDS] + [("Acrobot-v1", 3)])
def test_planted_goal_and_wall_states_on_device(cuda, env_id, frame_stack):
    """Goal and wall states written into the device bank's state: done / truncated / reward, the pre-reset frame in
    final_obs, and the reset frame (the CPU bank's, same seed and tg) as the returned observation. The frame-stack
    push is one template, so frame_stack = 3 runs once, on the widest frame."""
    cases = PLANTED[env_id]
    N = len(cases)
    states = torch.tensor([c[0] for c in cases], dtype=torch.float32)
    banks = []
    for dev in (cuda, "cpu"):
        b = E.make(env_id, N, device=dev, seed=3, frame_stack=frame_stack)
        b.keep_final_obs = True
        b.reset()
        b.state.copy_(states.to(dev))
        banks.append(b)
    gpu, cpu = banks
    gpu.obs.copy_(cpu.obs)
    if gpu.is_discrete:
        a = torch.tensor([c[1] for c in cases], dtype=torch.int32)
    else:
        a = torch.tensor([[c[1]] for c in cases], dtype=torch.float32)
    prev = cpu.obs.clone()
    oc = cpu.step(a, prev_obs=prev.clone())[0]
    og = gpu.step(a.to(cuda), prev_obs=prev.to(cuda))[0].cpu()
    D = gpu.frame_shape[0]
    for i, (_, _, term, rew, after, exact) in enumerate(cases):
        assert bool(gpu.done[i]) == term and not bool(gpu.truncated[i]), (env_id, i)
        assert abs(float(gpu.reward[i]) - rew) <= 1e-4, (env_id, i)
        fin = gpu.final_obs[i].cpu()
        want = _frame(env_id, after)
        if exact:
            assert torch.equal(fin[-D:], want), (env_id, i)
        else:
            assert torch.allclose(fin[-D:], want, rtol=0, atol=1e-4), (env_id, i)
        assert torch.equal(fin[:-D], prev[i, D:])                     # pre-reset: the older frames shifted down
        if term:   # the returned observation: the reset frame for this tg, frame_stack copies of it
            assert torch.equal(og[i], og[i, :D].repeat(frame_stack))
            assert int(gpu.t[i]) == 0 and float(gpu.ep_ret[i]) == 0.0
        else:
            assert torch.equal(og[i], fin)
            assert int(gpu.t[i]) == 1
    assert torch.equal(gpu.done.cpu(), cpu.done) and torch.equal(gpu.tg.cpu(), cpu.tg)
    assert torch.allclose(og, oc, rtol=1e-4, atol=1e-4)
    assert torch.allclose(gpu.final_obs.cpu(), cpu.final_obs, rtol=1e-4, atol=1e-4)
    assert torch.allclose(gpu.ep_stats.cpu(), cpu.ep_stats, rtol=1e-4, atol=1e-3) and float(gpu.ep_stats[1]) == 1.0


# ------------------------------------------------------------------------------------------------------ native MLP engine
@pytest.mark.parametrize("env_id", IDS)
def test_native_mlp_update_matches_torch_engine(cuda, env_id):
    """PPO at 4 envs x 8 steps on the native MLP engine (its updates replay as one captured graph) against the torch
    engine from the same parameters and seed, with the tolerances of test_gpu_mlp.py (policy step: values rtol 1e-4 /
    atol 1e-5, log-probs and actions 1e-4; trainer: update direction cosine > 0.999, length within 1 %). A captured
    trainer runs one eager update first, so both the eager update and the graph's first replay are compared. A 3-step
    time limit puts auto-resets into every rollout."""
    from actor_critic_algs_on_tensorflow_amd.algos.trainer import ActorCriticTrainer
    kw = _quiet(env=env_id, num_envs=4, n_steps=8, ppo_epochs=2, ppo_minibatches=2, seed=11)

    def make(engine, graph):
        env = E.make(env_id, 4, device=cuda, seed=11, max_episode_steps=3)
        return ActorCriticTrainer(preset("acrobot_ppo", engine=engine, cuda_graph=graph, **kw), env=env)

    nat, ref = make("native", True), make("torch", False)
    assert nat.mlp is not None and ref.mlp is None
    torch.testing.assert_close(nat.flat.data, ref.flat.data, rtol=0, atol=0)
    p_nat, p_ref = nat.flat.data.clone(), ref.flat.data.clone()

    def compare(which):
        a, b = nat.storage, ref.storage
        for name in ("dones", "truncated"):
            assert torch.equal(getattr(a, name), getattr(b, name)), (which, name)
        assert int(a.dones.sum()) >= 8 and torch.equal(a.dones, a.truncated)
        if nat.env.is_discrete:
            assert torch.equal(a.actions, b.actions), which
        else:
            torch.testing.assert_close(a.actions, b.actions, rtol=1e-4, atol=1e-4, msg=which)
        torch.testing.assert_close(a.logp, b.logp, rtol=1e-4, atol=1e-4, msg=which)
        torch.testing.assert_close(a.values, b.values, rtol=1e-4, atol=1e-5, msg=which)
        torch.testing.assert_close(a.rewards, b.rewards, rtol=1e-4, atol=1e-4, msg=which)
        torch.testing.assert_close(a.obs, b.obs, rtol=1e-4, atol=1e-4, msg=which)
        d_n, d_r = nat.flat.data - p_nat, ref.flat.data - p_ref
        cos = torch.nn.functional.cosine_similarity(d_n.double(), d_r.double(), dim=0)
        assert cos > 0.999, (which, float(cos))
        assert abs(float(d_n.norm() / d_r.norm()) - 1) < 1e-2, which

    nat.capture(warmup=1)
    ref.step()
    torch.cuda.synchronize()
    assert nat.graph is not None and nat.graph[0] == "single"
    compare("eager update")
    p_nat, p_ref = nat.flat.data.clone(), ref.flat.data.clone()
    nat.step()
    ref.step()
    torch.cuda.synchronize()
    compare("graph replay")
    assert torch.isfinite(nat.flat.data).all() and torch.isfinite(nat.stats_buf).all()


def test_eval_every_on_acrobot_takes_the_native_per_step_path(cuda):
    from actor_critic_algs_on_tensorflow_amd.algos.trainer import ActorCriticTrainer
    cfg = preset("acrobot_ppo", **_quiet(num_envs=4, n_steps=8, ppo_epochs=1, ppo_minibatches=2, engine="native",
                                         cuda_graph=True, eval_every=1, eval_envs=3, eval_episodes=2))
    env = E.make("Acrobot-v1", 4, device=cuda, seed=cfg.seed, max_episode_steps=20)
    tr = ActorCriticTrainer(cfg, env=env)
    assert tr.mlp is not None and tr.evaluator.path == "native" and tr.evaluator.L == 40
    tr.train(2)
    torch.cuda.synchronize()
    assert len(tr.eval_history) == 2
    r = tr.evaluator.result()
    assert r["path"] == "native" and r["episodes"] == 6
    score = tr.eval_history[-1]["eval_ret_mean"]
    assert math.isfinite(score) and -20.0 <= score <= 0.0 and score == r["ret_mean"]


# ------------------------------------------------------------------------------------------------------ learning
def test_acrobot_ppo_learns_on_the_native_engine(cuda):
    """Preset acrobot_ppo (16 envs x 128 steps, 4 epochs x 4 minibatches) on the native MLP engine, one captured graph
    per update, seeds 1 and 7, 120 updates (246 k env steps): the mean finished-episode return over the last 20
    updates is above -150. A random policy scores -500 (it never reaches the goal); curves of both engines are in
    profiles/classic_gym_envs.txt."""
    from actor_critic_algs_on_tensorflow_amd.algos.trainer import ActorCriticTrainer
    for seed in (1, 7):
        tr = ActorCriticTrainer(preset("acrobot_ppo", **_quiet(engine="native", cuda_graph=True, seed=seed)))
        assert tr.mlp is not None
        tr.capture(warmup=1)
        assert tr.graph is not None and tr.graph[0] == "single"
        for _ in range(99):   # the capture's warm-up was update 1
            tr.step()
        first, _, _ = tr.env.drain_episode_stats()
        for _ in range(20):
            tr.step()
        last, n_ep, _ = tr.env.drain_episode_stats()
        print(f"acrobot_ppo native seed {seed}: updates 1-100 mean return {first:.1f}, 101-120 {last:.1f} "
              f"over {n_ep} episodes")
        assert n_ep > 0 and last > -150, (seed, first, last)
