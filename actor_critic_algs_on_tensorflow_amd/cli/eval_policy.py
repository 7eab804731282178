"""Batched deterministic evaluation CLI: restore a TF-bundle checkpoint of an MLP or CNN policy and score its mean /
arg-max actions on a bank of envs (``api.evaluate_policy``, ``algos/evaluator.py``). The reference's one-env sampled loop with
its per-episode report stays ``cli/test_model.py``.

    python -m actor_critic_algs_on_tensorflow_amd.cli.eval_policy Pendulum-v0 tests/fixtures/model-Pendulum_a3c \
        --batched 16 [--num_episodes 1] [--device cuda:0] [--max_episode_steps 1000]
"""
from __future__ import annotations

import argparse


def main(argv=None):
    p = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("env")
    p.add_argument("model_path")
    p.add_argument("--batched", default=16, type=int, metavar="N", help="envs of the evaluation bank")
    p.add_argument("--num_episodes", default=1, type=int, help="episodes per env")
    p.add_argument("--seed", default=12321, type=int)
    p.add_argument("--frames", default=1, type=int)
    p.add_argument("--device", default="cpu", help="device of the evaluation (a GPU runs the native MLP / CNN engine)")
    p.add_argument("--engine", default="auto", choices=["auto", "native", "torch"])
    p.add_argument("--max_episode_steps", default=None, type=int,
                   help="time limit of the bank (default: the env's own; the step budget is num_episodes times it)")
    a = p.parse_args(argv)
    from ..api import evaluate_policy
    from .. import ckpt
    path = a.model_path
    if not path.endswith(".index") and ckpt.latest_checkpoint(path):
        path = ckpt.latest_checkpoint(path)
    path = path[:-len(".index")] if path.endswith(".index") else path
    print("\n************Test Mode**********\nUsing model path {}\n\n".format(path))
    r = evaluate_policy(path, a.env, num_envs=a.batched, episodes=a.num_episodes, seed=a.seed, frames=a.frames,
                        device=a.device, engine=a.engine, max_episode_steps=a.max_episode_steps)
    print("Deterministic evaluation ({} path): {} episodes on {} envs".format(r["path"], r["episodes"], a.batched))
    print("Reward mean {} std {} min {} max {}".format(r["ret_mean"], r["ret_std"], r["ret_min"], r["ret_max"]))
    print("Episode Length {}".format(r["len_mean"]))
    return r


if __name__ == "__main__":
    main()
