"""``TrainConfig.fused_rollout_towers`` without a device: config validation, the CLI flag and the preset, the LDS fit
helper against values computed by hand from the kernel's layout, and a numpy model of the run-time wave split of the
generic-tower chain (``csrc/kernels/mlp.hip`` roll_gen_plan / roll_gen_mfma / roll_gen_epilogue).

The split tests check the FORMULA (every (column, k) owned once, ``s_red`` in bounds), on a numpy restatement of it:
they would pass on any tree, and an edit to the HIP formula does not fail them. What pins the kernel to the formula is
the GPU test ``test_gpu_rollout_towers.py::test_generic_chain_is_bitwise_the_register_chain_on_the_reference_actor``
(the compile-time ``RollLayer`` split and the run-time one must issue the same MFMAs) and the per-tower comparisons
beside it. The constants here that the engine also has (envs per workgroup, LDS caps, ``ngp2``) are taken from the
engine."""
import dataclasses

import numpy as np
import pytest

from actor_critic_algs_on_tensorflow_amd.config import PRESETS, TrainConfig, preset
from actor_critic_algs_on_tensorflow_amd.ops.mlp import MLPEngine, ngp2


# ------------------------------------------------------------------------------------------------ config
def test_flag_defaults_off_and_round_trips():
    c = TrainConfig()
    assert c.fused_rollout_towers is False and c.fused_rollout is True
    d = c.to_dict()
    assert d["fused_rollout_towers"] is False
    assert TrainConfig(**d) == c
    on = c.replace(fused_rollout_towers=True)
    assert on.fused_rollout_towers and TrainConfig(**on.to_dict()) == on
    names = [f.name for f in dataclasses.fields(TrainConfig)]
    assert names.index("fused_rollout_towers") == names.index("fused_rollout") + 1


@pytest.mark.parametrize("algo", ["a3c", "basic_ac"])
def test_flag_needs_a2c_or_ppo(algo):
    with pytest.raises(ValueError, match="fused_rollout_towers=True with algo"):
        TrainConfig(algo=algo, fused_rollout_towers=True)


def test_flag_refuses_the_cnn_model_and_ignores_the_torch_engine():
    with pytest.raises(ValueError, match="fused_rollout_towers=True with model='cnn'"):
        TrainConfig(algo="ppo", model="cnn", fused_rollout_towers=True)
    for algo in ("a2c", "ppo"):
        for model in ("auto", "mlp"):
            assert TrainConfig(algo=algo, model=model, fused_rollout_towers=True).fused_rollout_towers
    assert TrainConfig(algo="ppo", engine="torch", fused_rollout_towers=True).engine == "torch"   # accepted, no effect


def test_preset_is_the_tanh64_preset_plus_the_flag():
    base, fused = dict(PRESETS["halfcheetah_ppo_tanh64"]), dict(PRESETS["halfcheetah_ppo_tanh64_fused"])
    assert "fused_rollout_towers" not in base
    assert fused.pop("fused_rollout_towers") is True and fused == base
    p, q = preset("halfcheetah_ppo_tanh64"), preset("halfcheetah_ppo_tanh64_fused")
    assert not p.fused_rollout_towers and q.fused_rollout_towers
    assert q.replace(fused_rollout_towers=False) == p
    assert (q.actor_hidden, q.critic_hidden, q.hidden_act, q.mlp_init) == ((64, 64), (64, 64), "tanh", "orthogonal")
    others = [v for k, v in PRESETS.items() if k != "halfcheetah_ppo_tanh64_fused"]
    assert all(not dict(v).get("fused_rollout_towers") for v in others)


def test_cli_flag():
    from actor_critic_algs_on_tensorflow_amd.cli.run_ac import build_parser, config_from_args
    base = "--algo ppo --preset halfcheetah_ppo_tanh64 --env HalfCheetahShape-v0"
    assert not config_from_args(build_parser().parse_args(base.split())).fused_rollout_towers
    c = config_from_args(build_parser().parse_args((base + " --fused-rollout-towers").split()))
    assert c.fused_rollout_towers and c.actor_hidden == (64, 64)
    with pytest.raises(ValueError, match="fused_rollout_towers"):   # the flag on the reference-parity trainer
        config_from_args(build_parser().parse_args("--fused-rollout-towers".split()))


# ------------------------------------------------------------------------------------------------ LDS fit helper
CAP, CAP_NORM = MLPEngine.ROLLOUT_MAX_LDS, MLPEngine.ROLLOUT_MAX_LDS - MLPEngine.ROLLOUT_NORM_LDS


@pytest.mark.parametrize("hidden,frames,nbytes,fits", [
    ((64, 64), 1, 34576, True), ((64, 64), 2, 43792, True), ((64, 64), 3, 43792, True),
    ((192, 64), 1, 106000, True),
    ((256, 64, 64), 1, 133968, True), ((256, 64, 64), 2, 167760, False), ((256, 64, 64), 3, 167760, False),
    ((128, 128, 64), 2, 149072, True), ((128, 128, 64), 3, 149072, True),
    ((256, 128), 1, 184592, False)])
def test_lds_helper_matches_the_kernel_layout(hidden, frames, nbytes, fits):
    widths = [17 * frames] + list(hidden) + [6]
    assert MLPEngine.rollout_lds_bytes_of(widths, True) == nbytes
    assert MLPEngine.rollout_towers_fit(widths) is fits
    assert MLPEngine.rollout_lds_bytes_of(widths, False) < MLPEngine.rollout_lds_bytes_of(widths, True)


def test_lds_caps():
    assert (CAP, CAP_NORM) == (153600, 151552)
    ref = [51, 128, 128, 64, 6]   # the reference widths at 3 frames: under both caps
    assert MLPEngine.rollout_lds_bytes_of(ref) == 149072 <= CAP_NORM
    assert MLPEngine.rollout_towers_fit(ref, norm_obs=True) and MLPEngine.rollout_towers_fit(ref, norm_obs=False)
    for frames in (1, 2, 3):      # (256, 128) never fits
        assert not MLPEngine.rollout_towers_fit([17 * frames, 256, 128, 6])
        assert not MLPEngine.rollout_towers_fit([17 * frames, 256, 128, 6], norm_obs=True)
    # the tables' static LDS can be what decides: a tower between the two caps
    between = [w for w in ([17, 256, 96, 6], [34, 256, 32, 6], [17, 240, 128, 6], [17, 256, 80, 16, 6])
               if CAP_NORM < MLPEngine.rollout_lds_bytes_of(w) <= CAP]
    for w in between:
        assert MLPEngine.rollout_towers_fit(w) and not MLPEngine.rollout_towers_fit(w, norm_obs=True)


# ------------------------------------------------------------------------------------------------ the run-time split
WAVES, RB = 8, MLPEngine.ROLL_RB   # MLP_THREADS / 64 waves per workgroup; envs per workgroup (= MFMA 4x4x1 rows)


def _plan(K, N):
    """roll_gen_plan: RollLayer's formula at run time."""
    K_, NP = 16 * ngp2(K), 16 * ngp2(N)
    CG = (N + 63) // 64
    S = min(WAVES // CG, K_ // 4)
    return K_, NP, CG, S, K_ // S


def _check_ownership(K_, N):
    """Every (column, k) of the padded layer [N][K_] is owned by exactly one (wave, K range); every s_red index the
    waves write and the epilogue reads stays below 8 * 4 * 64."""
    red_size = WAVES * RB * 64
    CG = (N + 63) // 64
    S = min(WAVES // CG, K_ // 4)
    kper = K_ // S
    owner = np.zeros((N, K_), dtype=np.int32)
    lanes = np.arange(64)
    for w in range(WAVES):
        if w >= CG * S:
            continue                                       # the wave sits the layer out
        cg, sp = w % CG, w // CG
        cols = cg * 64 + lanes
        live = cols < N                                    # lanes past N read a clamped column that is never summed
        owner[cols[live], sp * kper:(sp + 1) * kper] += 1
        assert ((w * RB + RB - 1) * 64 + lanes).max() < red_size
        assert sp * CG + cg == w                           # the slot the epilogue reads for (column group, split)
    assert (owner == 1).all(), (K_, N)
    for c in range(N):                                     # the epilogue's reads of column c
        cg, lane = c >> 6, c & 63
        assert cg < CG and (((S - 1) * CG + cg) * RB + RB - 1) * 64 + lane < red_size


def test_split_covers_every_column_and_k_exactly_once():
    checked = set()
    for K in range(1, 257):
        for N in range(1, 257):
            K_, NP, CG, S, kper = _plan(K, N)
            assert K <= K_ <= 256 and K_ % S == 0 and kper % 4 == 0 and kper >= 4 and 1 <= CG * S <= WAVES
            assert (kper // 4) & (kper // 4 - 1) == 0               # rounds of four float4 pairs, then <= 2 singles
            assert NP & (NP - 1) == 0 and N <= NP <= 256            # the epilogue's shift and mask
            if (K_, N) not in checked:                              # K enters the split through K_ alone
                checked.add((K_, N))
                _check_ownership(K_, N)
    assert len(checked) == 5 * 256


def test_split_is_the_register_chains_on_the_reference_actor():
    """RollLayer<K_, N_> of the four compile-time layers (N_ = 16 for the 6-wide head): CG, S, kper."""
    want = {(17, 128): (1, 2, 4, 8), (51, 128): (1, 2, 4, 16), (128, 128): (1, 2, 4, 32), (128, 64): (1, 1, 8, 16),
            (64, 6): (1, 1, 8, 8)}
    for (K, N), (_, CG, S, kper) in want.items():
        assert _plan(K, N)[2:] == (CG, S, kper), (K, N)
