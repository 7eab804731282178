"""PPO early stopping on the approximate KL (``TrainConfig.target_kl``) on the CPU: the refusals, the statistic
(``losses.approx_kl``) against fp64, the torch engine against the host-break oracle of
``tests/oracles/target_kl_oracle.py`` (bit for bit), the gate reaching a ``FusedGroupStep`` built before it, the
metrics keys, and save / resume in the middle of a run. GPU side: ``tests/test_gpu_target_kl.py``."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "oracles"))

import target_kl_oracle as O  # noqa: E402

from actor_critic_algs_on_tensorflow_amd import TrainConfig, preset  # noqa: E402
from actor_critic_algs_on_tensorflow_amd.algos import losses as L  # noqa: E402
from actor_critic_algs_on_tensorflow_amd.algos.trainer import STAT_KEYS, ActorCriticTrainer  # noqa: E402

E_, M_ = 4, 2   # ppo_epochs x ppo_minibatches of the trainer tests: 8 steps per update
# a learning rate above the presets' so that the approximate KL grows inside one update
SMALL = {"pendulum": dict(num_envs=4, n_steps=24, ppo_epochs=E_, ppo_minibatches=M_, lr=1e-3),
         "cartpole": dict(env="CartPole-v1", num_envs=4, n_steps=24, ppo_epochs=E_, ppo_minibatches=M_, lr=1e-3)}


def _make(kind, **kw):
    base = dict(outdir=None, quiet=True, stdout_freq=0, save_every=0, device="cpu", cuda_graph=False)
    base.update(SMALL[kind])
    base.update(kw)
    return ActorCriticTrainer(preset("pendulum_ppo", **base))


# ------------------------------------------------------------------------------------------------ refusals
def test_config_refusals():
    for bad in (0.0, -0.01):
        with pytest.raises(ValueError, match="target_kl"):
            TrainConfig(algo="ppo", target_kl=bad)
    for algo in ("a2c", "a3c", "basic_ac"):
        with pytest.raises(ValueError, match="target_kl"):
            TrainConfig(algo=algo, target_kl=0.01)
    with pytest.raises(ValueError, match="target_kl"):
        TrainConfig(algo="ppo", target_kl=0.01, engine="native", model="cnn")
    assert TrainConfig().target_kl is None and TrainConfig(algo="ppo", target_kl=0.02).target_kl == 0.02
    for name in ("mujoco_ppo_dp8", "pendulum_ppo", "breakout_ppo"):
        assert preset(name).target_kl is None


def test_trainer_refusals():
    # data parallelism: every rank would have to take the same decision
    with pytest.raises(ValueError, match="data parallelism.*all-reduce"):
        ActorCriticTrainer(preset("pendulum_ppo", outdir=None, quiet=True, stdout_freq=0, save_every=0, device="cpu",
                                  cuda_graph=False, num_envs=2, n_steps=4, target_kl=0.01),
                           dp=SimpleNamespace(rank=0, world_size=1))
    # model="auto" resolving to the CNN family with engine="native"
    with pytest.raises(ValueError, match="target_kl with engine='native' and a CNN model"):
        ActorCriticTrainer(preset("breakout_ppo", outdir=None, quiet=True, stdout_freq=0, save_every=0, device="cpu",
                                  cuda_graph=False, model="auto", engine="native", num_envs=1, n_steps=1,
                                  target_kl=0.01))
    # the async parameter-server gradient sink replaces the optimiser step the gate would skip
    tr = _make("pendulum", target_kl=0.01)
    tr._grad_sink = lambda: None
    with pytest.raises(ValueError, match="gradient sink"):
        tr._apply_grads()


# ------------------------------------------------------------------------------------------------ statistic
@pytest.mark.parametrize("scale", [0.0, 1e-6, 1e-3, 0.3, 3.0])
def test_approx_kl_matches_fp64(scale):
    g = torch.Generator().manual_seed(int(scale * 1e6) + 5)
    lo = -torch.rand(257, generator=g) * 6.0
    lp = lo + scale * torch.randn(257, generator=g)
    got = float(L.approx_kl(lp, lo))
    want = O.approx_kl64(lp, lo)
    # per row: expm1 and the subtraction round to fp32 (a few ulp of max(|expm1 x|, |x|)), the inputs' difference x is
    # itself rounded (|d expm1(x) - x| <= |expm1 x| * ulp(x)); the fp32 mean adds n ulp of the result at the most
    x = (lp.double() - lo.double())
    row = (torch.expm1(x).abs() + x.abs()) * 4 * 2.0 ** -24 + torch.expm1(x).abs() * x.abs() * 2.0 ** -23
    bound = float(row.mean()) + 257 * 2.0 ** -24 * abs(want)
    print("scale", scale, "got", got, "fp64", want, "err", abs(got - want), "bound", bound)
    assert abs(got - want) <= bound
    assert got >= -bound, "never negative beyond rounding"


def test_approx_kl_zero_at_equal_inputs_and_plain_form_cancels():
    lo = -torch.rand(100) * 5
    assert float(L.approx_kl(lo.clone(), lo)) == 0.0
    assert float(L.approx_kl(lo.double(), lo.double())) == 0.0
    # the plain (r - 1) - log r form loses everything at small x; expm1 does not
    x = torch.full((64,), 3e-4)
    plain = float(((torch.exp(x) - 1.0) - x).mean())
    want = O.approx_kl64(x, torch.zeros(64))
    assert abs(float(L.approx_kl(x, torch.zeros(64))) - want) <= 1e-3 * want < abs(plain - want)


def test_threshold_is_one_float32():
    tr = _make("pendulum", target_kl=0.013)
    assert tr._kl_thr == O.threshold(0.013) == float(np.float32(1.5) * np.float32(0.013))
    assert _make("pendulum")._kl_thr == 0.0 and _make("pendulum")._kl_state is None


# ------------------------------------------------------------------------------------------------ torch engine
@pytest.fixture(scope="module", params=["pendulum", "cartpole"])
def probe(request):
    """One never-stopping run per env (shared, unchanged): kl_trace of update 0 -> (kind, j, thr)."""
    tr = _make(request.param)
    assert tr.mlp is None and tr.engine is None
    tr.step()
    j, thr = O.pick_threshold(tr._kl_trace.tolist())
    return request.param, j, thr


def test_torch_engine_equals_host_break_oracle(probe):
    kind, j, thr = probe
    tr = _make(kind, target_kl=thr / 1.5)
    ref = _make(kind)
    log = O.host_break(ref, tr._kl_thr)
    steps = []
    for u in range(3):
        tr.step()
        ref.step()
        steps.append(int(tr.stats["ppo_steps"]))
        O.assert_state_equal(tr, ref, f"{kind} update {u}")
        assert int(tr.update_counter) == u + 1 == int(ref.update_counter)
    print(kind, "stop step of update 0:", j, "thr", thr, "ppo_steps", steps, "oracle", log["steps"])
    assert steps == log["steps"] and steps[0] == j and 2 <= j <= E_ * M_ - 2
    for g, o in tr.opts.items():
        assert float(o.t) == sum(steps), g
    # the trace of the last update: the statistic up to the stop, -1 behind it
    n = steps[-1]
    trace = tr._kl_trace.tolist()
    assert all(v >= 0 for v in trace[:n + 1]) and all(v == -1.0 for v in trace[n + 1:])
    if n < E_ * M_:
        assert trace[n] > tr._kl_thr and float(tr.stats["approx_kl"]) == trace[n]
        assert int(tr._kl_state[0]) == 0 and int(tr._kl_state[1]) == n


def test_torch_engine_unreachable_threshold_equals_off(probe):
    kind = probe[0]
    tr, ref = _make(kind, target_kl=1e9), _make(kind)
    for _ in range(2):
        tr.step()
        ref.step()
    O.assert_state_equal(tr, ref, kind)
    assert int(tr.stats["ppo_steps"]) == E_ * M_ and float(tr.opts["actor"].t) == 2 * E_ * M_
    assert torch.equal(tr._kl_trace, ref._kl_trace) and float(tr.stats["approx_kl"]) == float(ref.stats["approx_kl"])


def test_nan_compares_false():
    tr = _make("pendulum", target_kl=0.01)
    tr._kl_rule(0, torch.tensor(float("nan")))
    assert int(tr._kl_state[0]) == 1 and int(tr._kl_state[1]) == 1
    tr._kl_rule(1, torch.tensor(1.0))
    assert int(tr._kl_state[0]) == 0 and int(tr._kl_state[1]) == 1
    tr._kl_rule(2, torch.tensor(0.0))
    assert int(tr._kl_state[0]) == 0 and int(tr._kl_state[1]) == 1 and float(tr._kl_trace[2]) == -1.0
    tr._kl_rule(0, torch.tensor(0.0))   # the next update starts armed again
    assert tr._kl_state[:2].tolist() == [1, 1]


# ------------------------------------------------------------------------------------------------ group-step gate
def test_group_step_table_gains_the_gate_set_after_construction():
    from actor_critic_algs_on_tensorflow_amd.ops.optim import FusedGroupStep
    tr = _make("pendulum")
    opts = list(tr.opts.values())
    assert len(opts) == 2 and FusedGroupStep.compatible(opts)
    first = FusedGroupStep(opts)   # an earlier group step over the same optimisers keeps following the gate too
    gs = FusedGroupStep(opts)
    assert gs._trans is None and first._trans is None
    gate = torch.ones(1, dtype=torch.int32)
    for o in opts:
        o.set_gate(gate)
    assert gs._trans is not None and tuple(gs._trans.shape) == (2, FusedGroupStep.MAXT, 5)
    for k in range(2):
        assert gs._trans[k, 0].tolist() == [0, 1, 1, -9, gate.data_ptr()], "the gate row (optim.hip table code -9)"
        assert not gs._trans[k, 1:].any()
    opts[0].set_gate(None)
    assert not gs._trans[0].any() and gs._trans[1, 0, 3] == -9
    assert torch.equal(first._trans, gs._trans)
    opts[1].set_gate(None)
    assert gs._trans is None and first._trans is None


# ------------------------------------------------------------------------------------------------ records
def test_stat_keys_are_appended():
    assert STAT_KEYS[:9] == ("pg", "kl", "entropy", "crit_loss", "clipfrac", "act_loss", "ratio", "ev_before",
                             "ev_after")
    assert STAT_KEYS[9:] == ("approx_kl", "ppo_steps")


def test_log_has_the_keys_only_when_set(tmp_path):
    for k, target in enumerate((None, 1e9)):
        tr = _make("pendulum", target_kl=target, outdir=str(tmp_path / f"log{k}.txt"))
        tr.step()
        s = tr.log(0, print_tog=False)
        tr.close()
        assert ("approx_kl" in s) == ("ppo_steps" in s) == (target is not None)
        if target is not None:
            assert s["ppo_steps"] == E_ * M_ and s["approx_kl"] == float(tr.stats["approx_kl"]) > 0


# ------------------------------------------------------------------------------------------------ checkpoints
def test_save_and_resume_mid_run_is_bitwise(probe, tmp_path):
    kind, _, thr = probe
    whole = _make(kind, target_kl=thr / 1.5)
    first = _make(kind, target_kl=thr / 1.5)
    for _ in range(3):
        whole.step()
    first.step()
    assert int(first._kl_state[0]) == 0, "saved while the flag of a stopped update (update 0) is still down"
    path = first.save_checkpoint(str(tmp_path / "model-kl-1"))
    resumed = _make(kind, target_kl=thr / 1.5)
    resumed.load_checkpoint(path)
    for _ in range(2):
        resumed.step()
    O.assert_state_equal(resumed, whole, kind)
    assert int(resumed.stats["ppo_steps"]) == int(whole.stats["ppo_steps"])
