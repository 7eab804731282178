#!/usr/bin/env python3
"""Throughput of every BASELINE.json config on one device (env-steps/s, ms per update), one JSON line per config.

    python scripts/bench_configs.py [--configs pong_a2c,breakout_ppo,mujoco_ppo_dp8,cartpole_cpu] [--updates K]
                                    [--warmup W] [--engine auto|torch] [--device cuda:0] [--engine-opts JSON]
                                    [--bootstrap-on-timeout] [--norm-obs] [--norm-reward]
                                    [--target-kl X] [--ep-window K] [--fused-rollout-towers]

Each config runs with its preset (config.py PRESETS): same model, env bank, rollout length, optimiser and PPO
epochs/minibatches as BASELINE.json names; synthetic envs and random-init weights. The update is captured as a
hipGraph where the trainer supports it (single device). The 8-GPU configs (a2c_dp8, mujoco_ppo_dp8) are measured
here per device; their multi-GPU runs go through torch.distributed.run like bench.py.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def run(name, updates, warmup, engine, device, dp_world1=False, engine_opts=None, bootstrap_on_timeout=False,
        norm_obs=False, norm_reward=False, target_kl=None, ep_window=0, fused_rollout_towers=False):
    from actor_critic_algs_on_tensorflow_amd import preset
    from actor_critic_algs_on_tensorflow_amd.algos.trainer import ActorCriticTrainer
    dev = device if name != "cartpole_cpu" or device == "cpu" else device
    cfg = preset(name, device=dev, outdir=None, quiet=True, stdout_freq=0, save_every=0, engine=engine,
                 cuda_graph=dev.startswith("cuda"))
    if bootstrap_on_timeout:
        cfg.bootstrap_on_timeout = True
    if norm_obs:
        cfg = cfg.replace(norm_obs=True)   # (validated: MLP configs only)
    if norm_reward:
        cfg = cfg.replace(norm_reward=True)   # (validated: MLP configs only)
    if target_kl is not None:
        cfg = cfg.replace(target_kl=target_kl)   # (validated: PPO configs only; a CNN config runs on the torch engine)
    if ep_window:
        cfg = cfg.replace(ep_window=ep_window)   # (the rolling episode window: two launches per update)
    if fused_rollout_towers:
        cfg = cfg.replace(fused_rollout_towers=True)   # (validated: MLP configs only; custom actors that fit LDS)
    if engine_opts:
        import dataclasses
        cfg.engine_opts = dataclasses.replace(cfg.engine_opts, **engine_opts)
    dp = None
    if dp_world1:
        # the data-parallel update at world size 1 (RCCL on a GPU): every collective of the DP schedule is issued
        # (recorded in the update's graph), so the trace shows what the collectives cost on top of the compute
        import torch.distributed as dist
        from actor_critic_algs_on_tensorflow_amd.parallel import dp as DP
        if not dist.is_initialized():
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("MASTER_PORT", "29531")
            kw = dict(device_id=torch.device(dev)) if dev.startswith("cuda") else {}
            dist.init_process_group("nccl" if dev.startswith("cuda") else "gloo", rank=0, world_size=1, **kw)
        dp = DP.DataParallel()
    tr = ActorCriticTrainer(cfg, dp=dp)
    cuda = dev.startswith("cuda")
    if cuda:
        tr.capture(warmup=2)
    for _ in range(warmup):
        tr.step()
    if cuda:
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(updates):
        tr.step()
    if cuda:
        torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    steps = cfg.n_steps * tr.env.num_envs * updates
    # early stopping: the optimiser steps the last update applied and the approximate KL that ended (or closed) it
    kl = {"target_kl": cfg.target_kl, "ppo_steps": int(tr.stats["ppo_steps"]),
          "approx_kl": float(tr.stats["approx_kl"])} if cfg.target_kl is not None else {"target_kl": None}
    return {**kl, "config": name, "env_steps_per_s": round(steps / dt, 1), "ms_per_update": round(1e3 * dt / updates, 4),
            "updates": updates, "envs": tr.env.num_envs, "n_steps": cfg.n_steps, "algo": cfg.algo,
            "engine": "native-cnn" if tr.engine is not None else ("native-mlp" if tr.mlp is not None else "torch"),
            "hipgraph": bool(tr.graph), "device": dev, "dp_world1": bool(dp_world1),
            "engine_opts": engine_opts or {}, "bootstrap_on_timeout": bool(cfg.bootstrap_on_timeout),
            "norm_obs": bool(cfg.norm_obs), "norm_reward": bool(cfg.norm_reward), "ep_window": int(cfg.ep_window),
            "fused_rollout_towers": bool(cfg.fused_rollout_towers),
            "ppo": {"epochs": cfg.ppo_epochs, "minibatches": cfg.ppo_minibatches} if cfg.algo == "ppo" else None}


def run_eval(name, reps, device, norm_obs=False, eval_envs=16, eval_episodes=1, max_episode_steps=None, opts=None,
             fused_rollout_towers=False):
    """The deterministic evaluation of a config (``TrainConfig.eval_every``; algos/evaluator.py) on its own: time per
    evaluation as its captured graph replays (restore, launches, summary; the CNN path: its chain of chunk graphs),
    and, as the yardstick, the training rollout (``collect``) timed eagerly on the same trainer.
    ``max_episode_steps``: the time limit of both banks (the evaluation runs ``eval_episodes`` times as many steps)."""
    from actor_critic_algs_on_tensorflow_amd import envs as E
    from actor_critic_algs_on_tensorflow_amd import preset
    from actor_critic_algs_on_tensorflow_amd.algos.trainer import ActorCriticTrainer
    cuda = device.startswith("cuda")
    kw = dict(engine_opts=opts) if opts else {}
    if fused_rollout_towers:
        kw["fused_rollout_towers"] = True
    cfg = preset(name, device=device, outdir=None, quiet=True, stdout_freq=0, save_every=0, cuda_graph=cuda,
                 eval_every=1, eval_envs=eval_envs, eval_episodes=eval_episodes, norm_obs=norm_obs, **kw)
    env = None
    if max_episode_steps is not None:
        env = E.make(cfg.env, cfg.num_envs, device=device, seed=cfg.seed, max_episode_steps=int(max_episode_steps),
                     frame_stack=4 if ("Pong" in cfg.env or "Breakout" in cfg.env) else cfg.frames)
    tr = ActorCriticTrainer(cfg, env=env)
    ev = tr.evaluator

    def timed(fn, n):
        if cuda:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        if cuda:
            torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n

    if norm_obs:
        tr.step()   # the tables leave the identity
    ev.run()        # warm-up (+ capture on a GPU)
    res = ev.result()
    dt = timed(ev.run, reps)
    tr.collect()
    dt_roll = timed(tr.collect, max(1, reps // 2))
    return {"config": name, "eval": True, "path": ev.path, "hipgraph": ev.graph is not None, "device": device,
            "norm_obs": bool(norm_obs), "fused_rollout_towers": bool(cfg.fused_rollout_towers), "eval_envs": ev.N,
            "eval_steps": ev.L, "ms_per_eval": round(1e3 * dt, 4),
            "us_per_eval_step": round(1e6 * dt / ev.L, 3), "ret_mean": res["ret_mean"], "episodes": res["episodes"],
            "train_rollout_envs": tr.env.num_envs, "train_rollout_steps": cfg.n_steps,
            "train_collect_ms": round(1e3 * dt_roll, 4), "train_collect_us_per_step": round(1e6 * dt_roll / cfg.n_steps, 3)}


def main():
    # one JSON line per config on stdout: native libraries (RCCL's banner / warnings) write to fd 1 -> stderr
    sys.stdout.flush()
    out_fd = os.dup(1)
    os.dup2(2, 1)
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="pong_a2c,breakout_ppo,mujoco_ppo_dp8,cartpole_cpu")
    ap.add_argument("--updates", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--engine", default="auto")
    ap.add_argument("--device", default="cuda:0" if torch.cuda.is_available() else "cpu")
    ap.add_argument("--dp-world1", action="store_true", help="run the data-parallel schedule at world size 1")
    ap.add_argument("--engine-opts", default="", help='JSON EngineOpts overrides, e.g. \'{"ppo_head": false}\'')
    ap.add_argument("--bootstrap-on-timeout", action="store_true",
                    help="set TrainConfig.bootstrap_on_timeout on the chosen configs")
    ap.add_argument("--norm-obs", action="store_true",
                    help="set TrainConfig.norm_obs on the chosen configs (MLP models)")
    ap.add_argument("--norm-reward", action="store_true",
                    help="set TrainConfig.norm_reward on the chosen configs (MLP models)")
    ap.add_argument("--target-kl", type=float, default=None,
                    help="set TrainConfig.target_kl on the chosen configs (PPO; early stopping on the approximate KL)")
    ap.add_argument("--ep-window", type=int, default=0,
                    help="set TrainConfig.ep_window on the chosen configs (the rolling window over the last K episodes)")
    ap.add_argument("--fused-rollout-towers", action="store_true",
                    help="set TrainConfig.fused_rollout_towers on the chosen configs (MLP models; also under --eval)")
    ap.add_argument("--eval", action="store_true",
                    help="measure the deterministic evaluation (eval_every) of the chosen configs (the MLP presets and "
                         "pong_a2c / breakout_ppo) instead of their updates: --updates replays of the evaluation graph "
                         "(--norm-obs: with the normaliser; --engine-opts reaches the CNN engine)")
    ap.add_argument("--eval-envs", type=int, default=16, help="--eval: envs of the evaluation bank")
    ap.add_argument("--eval-max-steps", type=int, default=None,
                    help="--eval: time limit of the banks = steps of one evaluation (default: the env's own)")
    args = ap.parse_args()
    opts = json.loads(args.engine_opts) if args.engine_opts else None
    if args.eval:
        for name in args.configs.split(","):
            res = run_eval(name, args.updates, args.device, args.norm_obs, args.eval_envs,
                           max_episode_steps=args.eval_max_steps, opts=opts,
                           fused_rollout_towers=args.fused_rollout_towers)
            os.write(out_fd, (json.dumps(res) + "\n").encode())
        return
    for name in args.configs.split(","):
        res = run(name, args.updates, args.warmup, args.engine, args.device, args.dp_world1, opts,
                  args.bootstrap_on_timeout, args.norm_obs, args.norm_reward, args.target_kl, args.ep_window,
                  args.fused_rollout_towers)
        os.write(out_fd, (json.dumps(res) + "\n").encode())


if __name__ == "__main__":
    main()
