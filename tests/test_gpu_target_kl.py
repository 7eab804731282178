"""PPO early stopping on the approximate KL (``TrainConfig.target_kl``) on the GPU, native MLP engine: the statistic of
every loss head against the fp64 oracle, the closed gate (nothing moves), the strict boundary, the trainer (captured ==
eager == the host-break oracle of ``tests/oracles/target_kl_oracle.py``, bit for bit) and the accumulating
weight-gradient path. Measured errors and bars: ``profiles/target_kl.txt``. CPU side: ``tests/test_target_kl_cpu.py``."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "oracles"))

import target_kl_oracle as O  # noqa: E402
from test_gpu_mlp import _model  # noqa: E402

from actor_critic_algs_on_tensorflow_amd.ops import distributions as D  # noqa: E402

pytestmark = pytest.mark.gpu

INF = float("inf")
NONE = 2 ** 31 - 1   # stop_at while no launch has stopped the update
HEADS = {   # (ob_dim, ac_dim, discrete, variant), SPEC train path
    "spec_gauss": ((17, 6, False, "basic"), True),      # the MuJoCo towers: the fused Gaussian head
    "generic_gauss": ((17, 6, False, "basic"), False),  # the same towers through the generic Gaussian head
    "categorical": ((4, 2, True, "basic"), True),       # 2 actions
}


def _batch(cuda, eng, ref, B, disc, seed):
    """Observations, actions sampled by the reference model, and the DEVICE's own evaluate log-probs."""
    g = torch.Generator().manual_seed(seed)
    obs = torch.randn(B, eng.D, generator=g).to(cuda)
    with torch.no_grad():
        pi, v0 = ref(obs)
        keys = torch.arange(B, device=cuda, dtype=torch.int64)
        act, _, _ = (D.categorical_sample_ref(pi, keys, 9) if disc else
                     D.gaussian_sample_ref(pi, ref.actor.log_std, keys, 9))
    lp = torch.empty(B, device=cuda)
    eng.evaluate(obs, act, lp)
    adv = torch.randn(B, generator=g).to(cuda)
    ret = v0 + torch.randn(B, generator=g).to(cuda)
    return obs, act.contiguous(), lp, adv, ret, v0.contiguous(), g


def _coefs(cuda):
    return torch.tensor(0.02, device=cuda), torch.tensor(0.3, device=cuda)   # entropy, KL-proxy coefficients


# ------------------------------------------------------------------------------------------------ 1. statistic
@pytest.mark.parametrize("B", [1, 16, 36])
@pytest.mark.parametrize("head", list(HEADS))
def test_statistic_matches_fp64(cuda, head, B):
    """B = 1: a one-row partial tile; 16: one full tile; 36: two full tiles + a 4-row partial tile. logp_old = the
    device's own evaluate log-probs + noise of scale 0, 1e-3, 0.3.

    Bar, per case (profiles/target_kl.txt): 8 x the error of the fp32 torch form against fp64 on the same inputs (the
    project's rule, tests/test_gpu_sampling.py), plus what the train launch's own log-probs add -- they differ from the
    evaluate launch's by d_i (summation order), measured as d_rms = sqrt(statistic 1) at noise 0, where statistic 1 is
    mean((logp_old - logp)^2); since expm1(x + d) - (x + d) = [expm1(x) - x] + expm1(x) d + e^x d^2 / 2 + ..., the mean
    moves by at most sqrt(mean expm1(x)^2) d_rms + max(e^x) d_rms^2 (Cauchy-Schwarz; the second-order term doubled
    for the rest of the series; at noise 0 the first-order term vanishes and this one is the whole bar). Nothing
    else is allowed: where the train launch reproduces the evaluate launch's log-probs bit for bit (d_rms = 0) the bar
    is 8 x the torch form's error alone, and 0 at noise 0."""
    case, spec = HEADS[head]
    ob, ac, disc, variant = case
    m, ref, flat, eng = _model(cuda, ob, ac, disc, variant, seed=7)
    eng.spec = spec
    obs, act, lp, adv, ret, v0, g = _batch(cuda, eng, ref, B, disc, seed=100 + B)
    ce, beta = _coefs(cuda)
    d_rms = None
    for scale in (0.0, 1e-3, 0.3):
        lo = lp + scale * torch.randn(B, generator=g).to(cuda)
        stats = torch.zeros(16, device=cuda)
        ks = torch.full((2,), -7.0, device=cuda)
        trace = torch.full((1,), -7.0, device=cuda)
        eng.train(obs, act, lo, adv, ret, ce, beta, B, v_old=v0, ppo=True, ppo_clip=0.2, stats=stats,
                  kl_stat=ks, kl_trace=trace)
        torch.cuda.synchronize()
        got = float(ks[0])
        assert float(trace[0]) == got and float(ks[1]) == -7.0, "trace = the statistic; no step count without a flag"
        want = O.approx_kl64(lp, lo)
        x32 = lp - lo
        err32 = abs(float((torch.expm1(x32) - x32).mean()) - want)
        if scale == 0.0:
            d_rms = math.sqrt(max(float(stats[1]), 0.0))
        x = lp.double().cpu() - lo.double().cpu()
        e1 = torch.expm1(x)
        shift = float(e1.pow(2).mean().sqrt()) * d_rms + float(x.exp().max()) * d_rms ** 2
        bar = 8 * err32 + shift
        print(f"{head} B={B} noise={scale}: got {got:.9e} fp64 {want:.9e} err {abs(got - want):.3e} "
              f"torch-fp32 err {err32:.3e} d_rms {d_rms:.3e} shift {shift:.3e} bar {bar:.3e}")
        assert abs(got - want) <= bar
        assert got >= -bar
    # A2C mode leaves the slot at 0
    eng.train(obs, act, lo, adv, ret, ce, beta, B, ppo=False, stats=stats, kl_stat=ks)
    torch.cuda.synchronize()
    assert float(ks[0]) == 0.0


# ------------------------------------------------------------------------------------------------ 2. / 3. the gate
class Rig:
    """Engine + the trainer's optimiser wiring (grouped Adam launch on the item path, norm partials from the
    weight-gradient launch), and one 36-row PPO minibatch. The gate is set AFTER the group step exists."""

    def __init__(self, cuda, head="spec_gauss", gate=True, B=36):
        from actor_critic_algs_on_tensorflow_amd.ops.optim import FusedGroupStep, make_optimizer
        case, spec = HEADS[head]
        ob, ac, disc, variant = case
        self.m, self.ref, self.flat, self.eng = _model(cuda, ob, ac, disc, variant, seed=3)
        self.eng.spec = spec
        self.B = B
        self.opts = [make_optimizer("adam", self.flat, grp, lr, max_grad_norm=0.5)
                     for grp, lr in (("actor", 3e-3), ("critic", 1e-2))]
        for t, o in enumerate(self.opts):
            o.zero_grad_after = True
            o.ext_parts = self.eng.parts[t]
            gen = torch.Generator().manual_seed(50 + t)
            o.m.copy_(0.01 * torch.randn(o.m.numel(), generator=gen))
            o.v.copy_(1e-4 * torch.rand(o.v.numel(), generator=gen))
            o.t.fill_(4.0)
        self.gs = FusedGroupStep(self.opts, self.eng.frag_copies())
        self.state = torch.tensor([1, 0, NONE], dtype=torch.int32, device=cuda)   # [go, steps, stop_at]
        if gate:
            for o in self.opts:
                o.set_gate(self.state[0:1])
            assert self.gs._trans is not None and int(self.gs._trans[0, 0, 3]) == -9
        obs, act, lp, adv, ret, v0, g = _batch(cuda, self.eng, self.ref, B, disc, seed=21)
        self.args = (obs, act, lp + 0.3 * torch.randn(B, generator=g).to(cuda), adv, ret) + _coefs(cuda) + (B,)
        self.v0 = v0
        self.stats = torch.zeros(16, device=cuda)
        self.ks = torch.zeros(2, device=cuda)
        self.trace = torch.zeros(4, device=cuda)
        self.bump = torch.zeros(1, dtype=torch.int64, device=cuda)

    def step(self, thr=None, j=1):
        """train + the grouped optimiser launch; ``thr`` None: without the new arguments."""
        kl = {} if thr is None else dict(kl_stat=self.ks, go=self.state, kl_thr=thr, kl_trace=self.trace[j:j + 1],
                                             kl_step=j)
        used = self.eng.train(*self.args, v_old=self.v0, ppo=True, ppo_clip=0.2, stats=self.stats, bump=self.bump,
                              **kl)
        assert used
        self.gs.step()
        torch.cuda.synchronize()

    def snapshot(self):
        e = self.eng
        out = dict(data=self.flat.data, grad=self.flat.grad, stats=self.stats[0:7], mpart=e._mpart(self.B),
                   parts0=e.parts[0], parts1=e.parts[1])
        for t, o in enumerate(self.opts):
            out.update({f"m{t}": o.m, f"v{t}": o.v, f"t{t}": o.t.reshape(1)})
        for i, lay in enumerate(l for tw in e.towers for l in tw):
            out[f"F{i}"] = e.F[id(lay)]
            if id(lay) in e.G:
                out[f"G{i}"] = e.G[id(lay)]
        return {k: v.clone() for k, v in out.items()}


def _same(a, b, skip=()):
    for k in a:
        if k not in skip:
            assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("head", ["spec_gauss", "categorical"])
def test_closed_gate_moves_nothing(cuda, head):
    r = Rig(cuda, head)
    r.state.copy_(torch.tensor([0, 0, 0], dtype=torch.int32))   # step 0 stopped the update; this is step 1
    r.flat.grad.fill_(3.0)          # (holds g_log_std too)
    r.stats.fill_(7.0)
    r.eng._mpart(r.B).fill_(5.0)
    for p in r.eng.parts:
        p.fill_(9.0)
    r.ks.fill_(-7.0)
    r.trace.fill_(-7.0)
    before = r.snapshot()
    r.step(thr=INF, j=1)
    _same(before, r.snapshot())
    if r.eng.g_log_std is not None:
        assert bool((r.eng.g_log_std == 3.0).all())
    assert r.trace.tolist() == [-7.0, -1.0, -7.0, -7.0] and r.ks.tolist() == [-7.0, -7.0]
    assert int(r.bump) == 1 and r.state.tolist() == [0, 0, 0]


@pytest.mark.parametrize("head", ["spec_gauss", "categorical"])
def test_open_gate_with_unreachable_threshold_equals_plain_calls(cuda, head):
    a, b = Rig(cuda, head), Rig(cuda, head, gate=False)
    p0 = a.flat.data.clone()
    a.step(thr=INF)
    b.step(thr=None)
    _same(a.snapshot(), b.snapshot())
    assert (a.flat.data != p0).any() and float(a.opts[0].t) == 5.0
    assert a.state.tolist() == [1, 1, NONE] and float(a.ks[1]) == 1.0 and float(a.ks[0]) == float(a.trace[1]) > 0
    assert int(a.bump) == 1 == int(b.bump)


def test_boundary_is_strict(cuda):
    probe = Rig(cuda)
    probe.step(thr=INF)
    s = float(probe.ks[0])
    assert s > 0
    at = Rig(cuda)
    before = at.snapshot()
    at.step(thr=s)          # approx_kl > thr is false at equality: the step is applied
    assert float(at.ks[0]) == s and at.state.tolist() == [1, 1, NONE] and float(at.opts[0].t) == 5.0
    assert (at.flat.data != before["data"]).any()
    _same(at.snapshot(), probe.snapshot())
    below = Rig(cuda)
    before = below.snapshot()
    below.step(thr=float(np.nextafter(np.float32(s), np.float32(0))))
    assert float(below.ks[0]) == s == float(below.trace[1]) and below.state.tolist() == [0, 0, 1]
    assert float(below.ks[1]) == 0.0
    # nothing applied: parameters, moments, step counts, fragment copies (the gradient of the stopping minibatch
    # stays in the slab: never applied, overwritten by the next storing launch)
    after = below.snapshot()
    _same(before, after, skip=("grad", "stats", "mpart", "parts0", "parts1"))
    # the launch that stops writes its gradient whole: its item workgroups do not read the flag that the bookkeeping
    # workgroup of the same launch closes, so the slab equals a plain train call's, bit for bit
    plain = Rig(cuda)
    plain.eng.train(*plain.args, v_old=plain.v0, ppo=True, ppo_clip=0.2, stats=plain.stats)
    torch.cuda.synchronize()
    full = plain.snapshot()
    for k in ("grad", "parts0", "parts1", "stats"):
        assert torch.equal(after[k], full[k]), k
    # a launch behind the stop writes nothing: items (stop_at = 1 < 2), train launch and bookkeeping (flag closed)
    below.flat.grad.fill_(3.0)
    below.step(thr=INF, j=2)
    assert bool((below.flat.grad == 3.0).all()) and float(below.trace[2]) == -1.0 and below.state.tolist() == [0, 0, 1]


# ------------------------------------------------------------------------------------------------ 4. trainer
E_, M_ = 4, 2
CONFIGS = {
    # 36-row minibatches (two full tiles + a 4-row partial one), the one-launch fused rollout
    "mujoco": ("mujoco_ppo_dp8", dict(num_envs=8, n_steps=9)),
    "pendulum": ("pendulum_ppo", dict(num_envs=4, n_steps=8)),                       # generic head (spec off below)
    "cartpole": ("pendulum_ppo", dict(env="CartPole-v1", num_envs=4, n_steps=8)),    # categorical head
}
LR = 3e-3   # above the presets' 3e-4: the approximate KL grows several-fold within one update


def _trainer(name, graph, **over):
    from actor_critic_algs_on_tensorflow_amd import preset
    from actor_critic_algs_on_tensorflow_amd.algos.trainer import ActorCriticTrainer
    pre, kw = CONFIGS[name]
    kw = dict(kw, device="cuda:0", outdir=None, quiet=True, stdout_freq=0, save_every=0, cuda_graph=graph,
              ppo_epochs=E_, ppo_minibatches=M_, lr=LR)
    kw.update(over)
    tr = ActorCriticTrainer(preset(pre, **kw))
    assert tr.mlp is not None
    if name == "pendulum":
        tr.mlp.spec = False
    if name == "mujoco":
        assert tr.cfg.fused_rollout and tr.mlp.supports_fused_rollout(tr.env)
    return tr


def _oracle(name, thr, **over):
    from actor_critic_algs_on_tensorflow_amd.config import EngineOpts
    ref = _trainer(name, False, engine_opts=EngineOpts(adam_step_offsets=False), **over)
    return ref, O.host_break(ref, thr)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_trainer_captured_equals_eager_equals_host_break(cuda, name):
    probe = _trainer(name, False)
    probe.update_body()
    torch.cuda.synchronize()
    trace = probe._kl_trace.tolist()
    j, thr = O.pick_threshold(trace)
    print(name, "probe kl_trace", ["%.3e" % v for v in trace], "-> stop at step", j, "thr", thr)
    tr, twin = _trainer(name, True, target_kl=thr / 1.5), _trainer(name, False, target_kl=thr / 1.5)
    ref, log = _oracle(name, twin._kl_thr)
    assert abs(twin._kl_thr - thr) <= 1e-6 * thr
    tr.capture(warmup=1)
    assert tr.graph is not None and tr.graph[0] == "single"
    twin.update_body()   # the capture's warm-up update
    ref.update_body()
    steps = [int(twin.stats["ppo_steps"])]
    assert int(tr.stats["ppo_steps"]) == steps[0]
    for u in range(3):
        tr.step()
        twin.step()
        ref.step()
        torch.cuda.synchronize()
        steps.append(int(twin.stats["ppo_steps"]))
        assert int(tr.stats["ppo_steps"]) == steps[-1]
        O.assert_state_equal(tr, twin, f"{name}: replay {u} vs eager")
        O.assert_state_equal(twin, ref, f"{name}: eager vs host-break oracle, update {u + 1}")
        assert torch.equal(tr._kl_trace, twin._kl_trace)
        assert torch.equal(tr.stats_buf[:7], twin.stats_buf[:7]) and torch.equal(tr.stats_buf[9:11], twin.stats_buf[9:11])
        assert int(tr.update_counter) == u + 2 == int(twin.update_counter)
    print(name, "ppo_steps per update", steps, "oracle", log["steps"])
    assert steps == log["steps"] and steps[0] == j
    assert any(2 <= s <= E_ * M_ - 2 for s in steps)
    for grp, o in twin.opts.items():
        assert float(o.t) == sum(steps) == float(tr.opts[grp].t), grp
    assert torch.isfinite(tr.flat.data).all()


def test_default_off_publishes_the_statistic_and_auto_falls_back_for_cnn(cuda):
    from actor_critic_algs_on_tensorflow_amd import preset
    from actor_critic_algs_on_tensorflow_amd.algos.trainer import ActorCriticTrainer
    tr = _trainer("mujoco", False)
    assert tr._kl_state is None and tr.opts["actor"].gate is None
    tr.update_body()
    torch.cuda.synchronize()
    trace = tr._kl_trace.tolist()
    assert all(v >= 0 for v in trace) and trace[-1] == float(tr.stats["approx_kl"]) > 0
    assert float(tr.opts["actor"].t) == E_ * M_
    cnn = ActorCriticTrainer(preset("breakout_ppo", device="cuda:0", outdir=None, quiet=True, stdout_freq=0,
                                    save_every=0, cuda_graph=False, num_envs=2, n_steps=2, target_kl=0.01))
    assert cnn.engine is None and cnn.mlp is None, "engine='auto' + CNN + target_kl runs on the torch engine"
    assert all(o.gate is not None for o in cnn.opts.values())


# ------------------------------------------------------------------------------------------------ 5. accumulating path
def test_accumulating_wgrad_path_starts_the_next_update_clean(cuda):
    """4096-row minibatches: the weight-gradient launch splits its row tiles over two workgroups per item, which ADD
    into the slab (nsplit = 2; two addends commute, so the sums are still deterministic). The stopping minibatch's
    gradient stays behind a stopped update; the next update's arming clears it."""
    from actor_critic_algs_on_tensorflow_amd.ops.mlp import MLPEngine
    over = dict(num_envs=64, n_steps=128, ppo_epochs=2, ppo_minibatches=2)
    assert MLPEngine.wgrad_nsplit(64 * 128 // 2) == 2
    probe = _trainer("mujoco", False, **over)
    probe.update_body()
    torch.cuda.synchronize()
    trace = probe._kl_trace.tolist()
    j, thr = O.pick_threshold(trace)
    print("probe kl_trace", ["%.3e" % v for v in trace], "-> stop at step", j, "thr", thr)
    tr = _trainer("mujoco", False, target_kl=thr / 1.5, **over)
    ref, log = _oracle("mujoco", tr._kl_thr, **over)
    steps = []
    for u in range(3):
        tr.step()
        ref.step()
        torch.cuda.synchronize()
        steps.append(int(tr.stats["ppo_steps"]))
        O.assert_state_equal(tr, ref, f"update {u}")
    print("ppo_steps", steps, "oracle", log["steps"])
    assert steps == log["steps"] and steps[0] == j == 2
    assert not tr.mlp.last_stores_all
    for grp, o in tr.opts.items():
        assert float(o.t) == sum(steps), grp
