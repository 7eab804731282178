"""Single-process trainer CLI, flag-compatible with ``Basic_AC/run_AC.py`` (``Basic_AC/run_AC.py:11-22``).

    python -m actor_critic_algs_on_tensorflow_amd.cli.run_ac --env CartPole-v0 --seed 12321 --frames 1

Default ``--algo basic_ac`` is the reference's episode-batched loop (batch-1 inference, PathAdv targets,
KL-adaptive lr, log10 regulariser schedules, reference log format). ``--algo a2c|ppo`` (with ``--preset``)
switches to the vectorised GPU-native trainers with the same flags where they apply.
"""
from __future__ import annotations

import argparse
import os


def build_parser():
    p = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("--animate", default=False, action="store_true")
    p.add_argument("--env", default="Pendulum-v0",
                   help="env id (envs.REGISTRY): CartPole-v0 / -v1, Pendulum-v0, Acrobot-v1, MountainCar-v0, "
                        "MountainCarContinuous-v0, PongNoFrameskip-v4, BreakoutNoFrameskip-v4, HalfCheetahShape-v0")
    p.add_argument("--seed", default=12321, type=int)
    p.add_argument("--tboard", default=False, action="store_true")
    p.add_argument("--save_every", default=600, type=int)
    p.add_argument("--outdir", default="log.txt")
    p.add_argument("--checkpoint_dir", default=os.path.join("tmp", "checkpoints"))
    p.add_argument("--frames", default=1, type=int)
    p.add_argument("--mode", choices=["train", "debug"], default="train")
    p.add_argument("--desired_kl", default=0.002, type=float)
    # extensions
    p.add_argument("--algo", default="basic_ac", choices=["basic_ac", "a2c", "ppo"])
    p.add_argument("--preset", default=None, help="start from a named preset (config.PRESETS)")
    p.add_argument("--iters", default=5000000, type=int, help="ITER of the reference")
    p.add_argument("--device", default=None)
    p.add_argument("--num_envs", default=None, type=int)
    p.add_argument("--metrics", default=None, help="JSONL metrics sidecar path")
    p.add_argument("--quiet", action="store_true")
    p.add_argument("--norm-obs", action="store_true",
                   help="running observation normalisation (TrainConfig.norm_obs; --algo a2c|ppo, MLP models)")
    p.add_argument("--norm-reward", action="store_true",
                   help="running return-based reward scaling (TrainConfig.norm_reward; --algo a2c|ppo, MLP models)")
    p.add_argument("--target-kl", default=None, type=float,
                   help="PPO early stopping: skip an update's remaining minibatch steps once the approximate KL "
                        "exceeds 1.5 x this (TrainConfig.target_kl; --algo ppo, one device)")
    p.add_argument("--eval-every", default=0, type=int,
                   help="deterministic evaluation on a second bank after every N-th update (TrainConfig.eval_every; "
                        "--algo a2c|ppo, MLP models, one device)")
    p.add_argument("--ep-window", default=0, type=int,
                   help="rolling window over the last K finished training episodes, kept on the device "
                        "(TrainConfig.ep_window; --algo a2c|ppo): ep_ret_mean, ... in the metrics stream")
    p.add_argument("--stop-return", default=None, type=float,
                   help="stop once the episode window is full and its mean return reaches this "
                        "(TrainConfig.stop_return; needs --ep-window, one device)")
    p.add_argument("--actor-hidden", default=None, type=_widths,
                   help="hidden widths of the actor, e.g. 64,64 (TrainConfig.actor_hidden; --algo a2c|ppo, MLP models)")
    p.add_argument("--critic-hidden", default=None, type=_widths,
                   help="hidden widths of the critic, e.g. 64,64 (TrainConfig.critic_hidden)")
    p.add_argument("--hidden-act", default=None, choices=["tanh", "relu", "lrelu"],
                   help="activation of the hidden layers of both towers (TrainConfig.hidden_act)")
    p.add_argument("--mlp-init", default=None, choices=["reference", "orthogonal"],
                   help="initialisers of the MLP towers (TrainConfig.mlp_init)")
    p.add_argument("--fused-rollout-towers", action="store_true",
                   help="one-launch rollout and evaluation for custom actors whose weights fit in LDS "
                        "(TrainConfig.fused_rollout_towers; --algo a2c|ppo, MLP models, MuJoCo-shaped bank)")
    return p


def _widths(text):
    """``"64,64"`` -> ``(64, 64)``."""
    try:
        return tuple(int(w) for w in text.split(","))
    except ValueError:
        raise argparse.ArgumentTypeError(f"expected comma-separated widths such as 64,64, got {text!r}") from None


def config_from_args(a):
    from ..config import preset
    name = a.preset or ("basic_ac" if a.algo == "basic_ac" else ("breakout_ppo" if a.algo == "ppo" else "cartpole_cpu"))
    kw = dict(env=a.env, seed=a.seed, save_every=a.save_every, outdir=a.outdir, checkpoint_dir=a.checkpoint_dir,
              frames=a.frames, mode=a.mode, desired_kl=a.desired_kl, total_updates=a.iters, tboard=a.tboard,
              metrics_path=a.metrics, quiet=a.quiet)
    if a.algo != "basic_ac":
        kw["algo"] = a.algo
    if a.device:
        kw["device"] = a.device
    if a.num_envs:
        kw["num_envs"] = a.num_envs
    if a.norm_obs:
        kw["norm_obs"] = True
    if a.norm_reward:
        kw["norm_reward"] = True
    if a.target_kl is not None:
        kw["target_kl"] = a.target_kl
    if a.eval_every:
        kw["eval_every"] = a.eval_every
    if a.ep_window:
        kw["ep_window"] = a.ep_window
    if a.stop_return is not None:
        kw["stop_return"] = a.stop_return
    if a.fused_rollout_towers:
        kw["fused_rollout_towers"] = True
    for k in ("actor_hidden", "critic_hidden", "hidden_act", "mlp_init"):
        if getattr(a, k) is not None:
            kw[k] = getattr(a, k)
    return preset(name, **kw)


def main(argv=None):
    a = build_parser().parse_args(argv)
    from ..api import train
    cfg = config_from_args(a)
    res = train(cfg)
    print("done: %d iterations, %d env steps, %.1f env-steps/s" % (res.iterations, res.env_steps,
                                                                    res.env_steps_per_sec))
    return res


if __name__ == "__main__":
    main()
