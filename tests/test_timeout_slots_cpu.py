"""Host side of the fused rollout's time-limit bootstrap: the slot count per env (``ops/mlp.py`` timeout_slots) bounds
the truncations of any env of the bank, and the torch fallback of ``timeout_bootstrap_`` (the oracle of the HIP
kernel) adds ``gamma * V`` at the used slots only."""
import pytest
import torch

from actor_critic_algs_on_tensorflow_amd.ops.mlp import timeout_slots
from actor_critic_algs_on_tensorflow_amd.ops.returns import timeout_bootstrap_, timeout_bootstrap_ref_


def test_timeout_slots_bound_every_start_and_are_attained():
    """An env that enters a T-step rollout ``t0 < max_steps`` steps into its episode is truncated
    ``floor((t0 + T) / max_steps)`` times: never more than ``timeout_slots(T, max_steps)``, and exactly that for some
    ``t0`` (so no smaller slot count would do)."""
    for max_steps in range(1, 13):
        for T in range(1, 31):
            S = timeout_slots(T, max_steps)
            assert S == -(-T // max_steps)
            counts = [(t0 + T) // max_steps for t0 in range(max_steps)]
            assert max(counts) <= S, (max_steps, T, counts)
            assert max(counts) == S, (max_steps, T, counts)


def test_timeout_slots_rejects_empty_geometry():
    with pytest.raises(ValueError):
        timeout_slots(0, 5)
    with pytest.raises(ValueError):
        timeout_slots(5, 0)


def test_timeout_bootstrap_fallback_hand_example():
    """T = 3 steps, N = 2 envs, S = 2 slots. Env 0 was cut at step 2 (slot 0; slot 1 unused: its value, a NaN here,
    is never read); env 1 was cut at steps 0 and 2."""
    rewards = torch.tensor([[1.0, 2.0], [3.0, 4.0], [5.0, 6.0]])
    final_step = torch.tensor([[2, -1], [0, 2]], dtype=torch.int32)
    v_final = torch.tensor([[10.0, float("nan")], [20.0, 40.0]])
    want = torch.tensor([[1.0, 2.0 + 0.5 * 20.0], [3.0, 4.0], [5.0 + 0.5 * 10.0, 6.0 + 0.5 * 40.0]])
    for fn in (timeout_bootstrap_, timeout_bootstrap_ref_):
        r = rewards.clone()
        out = fn(r, final_step, v_final, 0.5)
        assert out is r
        assert torch.equal(r, want), r
    # all slots unused: nothing changes
    r = rewards.clone()
    timeout_bootstrap_(r, torch.full((2, 2), -1, dtype=torch.int32), torch.full((2, 2), float("nan")), 0.5)
    assert torch.equal(r, rewards)
