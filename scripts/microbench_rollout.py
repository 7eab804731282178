"""Phase timings of the fused MLP rollout kernel (mlp_rollout_kernel) from its s_memrealtime stamps (100 MHz):
per step, the end of each actor layer, of the parallel Gaussian head and of the env step, as seen by wave 0 of
workgroup 0 after each barrier. Median over steps 1..15 of a MuJoCo-shape config (64 envs).

    python scripts/microbench_rollout.py [PRESET] [--layers-only] [--towers]

PRESET: a config.PRESETS name (default mujoco_ppo_dp8). An actor other than the reference's runs the launch's
generic-tower chain (TrainConfig.fused_rollout_towers); ``--towers`` selects that chain for the reference actor too."""
import json
import sys
import time

import torch

sys.path.insert(0, ".")
from actor_critic_algs_on_tensorflow_amd import preset  # noqa: E402
from actor_critic_algs_on_tensorflow_amd.algos.trainer import ActorCriticTrainer, KEY_ENV_BITS  # noqa: E402


def main():
    names = [a for a in sys.argv[1:] if not a.startswith("--")]
    name = names[0] if names else "mujoco_ppo_dp8"
    cfg = preset(name, device="cuda:0", outdir=None, quiet=True, stdout_freq=0, save_every=0, cuda_graph=False)
    tr = ActorCriticTrainer(cfg)
    eng, st, env = tr.mlp, tr.storage, tr.env
    towers = "--towers" in sys.argv or not eng.supports_fused_rollout(env)
    if towers and not eng.supports_rollout_towers(env):
        raise SystemExit(f"{name}: the one-launch rollout does not take this actor / bank")
    nl = len(eng.towers[0])
    stamps = torch.zeros(256, dtype=torch.int64, device="cuda:0")
    out = {"preset": name, "towers": towers, "actor": [eng.D] + [l.out_features for l in eng.towers[0]],
           "wlds": eng.rollout_weights_in_lds(), "lds_bytes": eng.rollout_lds_bytes(True), "T": st.T, "N": env.num_envs}
    for rep in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.rollout_linear(env, st, KEY_ENV_BITS, tr.policy_seed, stamps=stamps, towers=towers)
        torch.cuda.synchronize()
        out[f"host_ms_{rep}"] = round((time.perf_counter() - t0) * 1e3, 3)
    allst = stamps.cpu().tolist()
    if "--layers-only" in sys.argv:   # diagnostics: actor layers alone in the step loop
        st2 = torch.zeros(256, dtype=torch.int64, device="cuda:0")
        st2[255] = 1
        eng.rollout_linear(env, st, KEY_ENV_BITS, tr.policy_seed, stamps=st2, towers=towers)
        torch.cuda.synchronize()
        a2 = st2.cpu().tolist()
        s2 = [a2[8 * k:8 * k + 8] for k in range(16)]
        out["layers_only_layer_us"] = [round((s2[8][i] - (s2[8][i - 1] if i else s2[7][6])) * 0.01, 2)
                                       for i in range(nl)]
    s = [allst[8 * k:8 * k + 8] for k in range(16)]
    # stamp slots: layers 0 .. nl - 1 (at most 5), then 5 = head, 6 = env step
    slots = [(f"layer{i}", i) for i in range(nl)] + [("head", 5), ("env", 6)]
    ph = {n: [] for n, _ in slots}
    for k in range(1, 16):
        prev = s[k - 1][6]
        for n, i in slots:
            ph[n].append((s[k][i] - prev) * 10 / 1000.0)   # 10 ns ticks -> us
            prev = s[k][i]
    out["phase_us_median"] = {n: round(sorted(v)[len(v) // 2], 3) for n, v in ph.items()}
    out["step_us_median"] = round(sorted((s[k][6] - s[k - 1][6]) * 0.01 for k in range(1, 16))[7], 3)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
