"""Deterministic evaluation of the CNN model, the parts that run without a GPU: the config gate, the chunk plan of the
captured evaluation, ``api.evaluate_policy`` and the CLI on a CNN checkpoint (torch path)."""
import numpy as np
import pytest
import torch

from actor_critic_algs_on_tensorflow_amd import ckpt
from actor_critic_algs_on_tensorflow_amd import envs as E
from actor_critic_algs_on_tensorflow_amd import preset
from actor_critic_algs_on_tensorflow_amd.algos.evaluator import Evaluator, chunk_plan
from actor_critic_algs_on_tensorflow_amd.api import Agent, evaluate_policy

ENV, N, MAXS, SEED = "PongNoFrameskip-v4", 2, 6, 31


def test_config_accepts_the_cnn_presets_on_a_gpu_device():
    assert preset("pong_a2c", eval_every=2).eval_every == 2
    assert preset("breakout_ppo", eval_every=1, eval_envs=4).eval_envs == 4
    assert preset("pong_a2c", eval_every=2, engine="torch").engine == "torch"


def test_config_keeps_refusing_the_cnn_model_on_a_cpu_device():
    with pytest.raises(ValueError, match="eval_every.*CPU"):
        preset("pong_a2c", device="cpu", eval_every=2)
    for kw in (dict(algo="a3c"), dict(algo="basic_ac")):
        with pytest.raises(ValueError, match="eval_every"):
            preset("pong_a2c", eval_every=2, **kw)


@pytest.mark.parametrize("L,chunk,want", [(1, 64, (0, 1)), (5, 2, (2, 1)), (5, 64, (0, 5)), (24, 10, (2, 4)),
                                          (64, 64, (1, 0)), (10000, 64, (156, 16))])
def test_chunk_plan(L, chunk, want):
    q, tail = chunk_plan(L, chunk)
    assert (q, tail) == want
    assert q * chunk + tail == L and 0 <= tail < chunk and (q * chunk) % 2 == 0


@pytest.mark.parametrize("chunk", [1, 3, 63, 0, -2])
def test_chunk_plan_refuses_odd_chunks(chunk):
    with pytest.raises(ValueError, match="chunk_steps"):
        chunk_plan(24, chunk)
    env = E.make("CartPole-v1", 1, device="cpu", seed=1, max_episode_steps=4)
    with pytest.raises(ValueError, match="chunk_steps"):
        Evaluator(None, env, None, None, 1, chunk_steps=chunk)


@pytest.fixture(scope="module")
def cnn_checkpoint(tmp_path_factory):
    ag = Agent.for_env(ENV, seed=3)
    with torch.no_grad():   # decisive logits: random-init gaps are far below the head's own rounding
        ag.model.net.heads.kernel.copy_(0.05 * torch.randn(ag.model.net.heads.kernel.shape,
                                                           generator=torch.Generator().manual_seed(5)))
    path = str(tmp_path_factory.mktemp("cnn_ckpt") / "model-Pong")
    ckpt.save_tensors(path, ckpt.model_tensors(ag.model))
    return path, ag.model


def _act_loop(model):
    """Records of an independent ``model.act(deterministic=True)`` loop on the same bank."""
    env = E.make(ENV, N, device="cpu", seed=SEED, frame_stack=4, max_episode_steps=MAXS)
    obs = env.reset()
    ret = np.zeros(N, np.float32)
    ln = np.zeros(N, np.int32)
    ep_ret, ep_len = np.full((N, 1), np.nan, np.float32), np.full((N, 1), -1, np.int32)
    for _ in range(MAXS):
        with torch.no_grad():
            a = model.act(obs, deterministic=True)[0]
        obs, r, d, _ = env.step(a)
        ret = ret + r.numpy()
        ln += 1
        for e in range(N):
            if d[e] and ep_len[e, 0] < 0:
                ep_ret[e, 0], ep_len[e, 0] = ret[e], ln[e]
        ret[d.numpy() != 0] = 0.0
        ln[d.numpy() != 0] = 0
    return ep_ret, ep_len


def test_evaluate_policy_takes_a_cnn_checkpoint(cnn_checkpoint):
    path, model = cnn_checkpoint
    r = evaluate_policy(path, ENV, num_envs=N, episodes=1, seed=SEED, device="cpu", max_episode_steps=MAXS)
    assert r["path"] == "torch" and r["episodes"] == N
    want_ret, want_len = _act_loop(model)
    assert r["ep_ret"].tobytes() == want_ret.tobytes() and np.array_equal(r["ep_len"], want_len)
    assert r["len_mean"] == float(want_len.mean())
    with pytest.raises(ValueError, match="engine='native'"):
        evaluate_policy(path, ENV, num_envs=N, episodes=1, seed=SEED, device="cpu", engine="native",
                        max_episode_steps=MAXS)


def test_eval_policy_cli_takes_a_cnn_checkpoint(cnn_checkpoint, capsys):
    from actor_critic_algs_on_tensorflow_amd.cli import eval_policy
    path, model = cnn_checkpoint
    r = eval_policy.main([ENV, path, "--batched", str(N), "--num_episodes", "1", "--seed", str(SEED),
                          "--max_episode_steps", str(MAXS)])
    assert r["episodes"] == N and "Deterministic evaluation (torch path)" in capsys.readouterr().out
    want_ret, want_len = _act_loop(model)
    assert r["ep_ret"].tobytes() == want_ret.tobytes() and np.array_equal(r["ep_len"], want_len)
