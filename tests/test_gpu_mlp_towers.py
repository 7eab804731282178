"""Custom MLP towers (hidden sizes, tanh / relu / lrelu) on the native MLP engine: the generic kernels of
csrc/kernels/mlp.hip against the fp64 oracle tests/oracles/mlp_tower_oracle.py.

Bars: for every output class the error of the fp32 PyTorch autograd of the same model against the oracle is measured
at the same shapes and inputs (``mlp_tower_oracle.reference_error``, on the CPU); the kernel may be 8 x that, and never
has to be below 4 fp32 ulps of the class's largest magnitude. Classes: values, log-prob, entropy, the greedy mean, each
layer's dW / db (one class per layer; the actor head's includes ``g_log_std``), every db of at least 16 elements once
more on its own, the statistics. Each figure is printed before it is asserted
(``pytest -s``); profiles/mlp_towers.txt keeps one such run.

Not here: a trainer with ``actor_hidden=(128, 128, 64)`` / ``critic_hidden=(256, 128)`` spelled out against the
defaults -- given widths always build custom towers (``hidden_<i>`` names), they are not routed through the reference
construction.
"""
import os
import sys

import numpy as np
import pytest
import torch

from actor_critic_algs_on_tensorflow_amd import preset
from actor_critic_algs_on_tensorflow_amd.models.policy import MLPActorCritic
from actor_critic_algs_on_tensorflow_amd.ops.optim import FlatParams

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "oracles"))
import mlp_tower_cases as C  # noqa: E402
import mlp_tower_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

BETA, CENT, PCLIP, VCLIP = 0.7, 0.05, 0.2, 0.15


def _engine(cuda, m):
    from actor_critic_algs_on_tensorflow_amd.ops.mlp import MLPEngine
    m = m.to(cuda)
    flat = FlatParams(m.param_groups(), cuda)
    return m, flat, MLPEngine(m, flat)


def _report(tag, err, ref, bar):
    bad = []
    for k in sorted(err):
        print(f"  {tag} {k:14s} ref_err {ref[k]:.3e}  bar {bar[k]:.3e}  kernel_err {err[k]:.3e}"
              f"{'  <-- above the bar' if err[k] > bar[k] else ''}")
        if err[k] > bar[k]:
            bad.append((k, err[k], bar[k]))
    return bad


def _check_case(cuda, c):
    head = c["head"][0]
    disc = head == "categorical"
    A = c["head"][1]
    cpu_model = C.build(c)
    ta, tc = C.towers_of(cpu_model)
    hk = C.head_kw(cpu_model)
    m, flat, eng = _engine(cuda, cpu_model)
    assert not eng.spec
    T = lambda a: torch.as_tensor(a).to(cuda)
    bad = []
    for B in c["batches"]:
        x = C.inputs(c, B)
        fw = O.forward(ta, tc, head, x["obs"], x["act"], **hk)
        lo = (fw["logp"] + x["lo_noise"]).astype(np.float32)
        ret = (fw["value"] + x["ret_noise"]).astype(np.float32)
        vo = (fw["value"] + x["vo_noise"]).astype(np.float32)
        kw = dict(logp_old=lo, adv=x["adv"], ret=ret, v_old=vo, ppo=c["ppo"], beta=BETA, ent_coef=CENT,
                  ppo_clip=PCLIP, v_clip=VCLIP if c["ppo"] else 0.0)
        ref_err, want = O.reference_error(ta, tc, head, x["obs"], x["act"], kw, **hk)
        bar = O.bars(ref_err, want)
        obs, act = T(x["obs"]), T(x["act"])
        # ---- forward: value, evaluate, greedy policy_step
        got = {}
        v = torch.empty(B, device=cuda)
        eng.value(obs, v)
        lp, en, v2 = (torch.empty(B, device=cuda) for _ in range(3))
        eng.evaluate(obs, act, lp, en, v2)
        assert torch.equal(v, v2)
        got.update(value=v.cpu().numpy(), logp=lp.cpu().numpy(), entropy=en.cpu().numpy())
        ga = torch.empty((B,) if disc else (B, A), dtype=torch.int32 if disc else torch.float32, device=cuda)
        glp, gen, gv = (torch.empty(B, device=cuda) for _ in range(3))
        tg = torch.zeros(B, dtype=torch.int64, device=cuda)
        ids = torch.arange(B, dtype=torch.int64, device=cuda)
        eng.policy_step(obs, ga, glp, gen, gv, tg, ids, 20, 1, greedy=True)
        assert torch.equal(gv, v)
        if disc:
            g = O.forward(ta, tc, head, x["obs"], None)
            keep = g["gap"] >= C.GAP
            assert (~keep).sum() <= C.GAP_CAP * B, (B, int((~keep).sum()))
            assert np.array_equal(ga.cpu().numpy().astype(np.int64)[keep], g["argmax"][keep])
        else:
            got["mean"] = ga.cpu().numpy()
        # ---- one train + weight-gradient launch
        flat.grad.zero_()
        stats = torch.zeros(16, device=cuda)
        used = eng.train(obs, act, T(lo), T(x["adv"]), T(ret), torch.tensor(CENT, device=cuda),
                         torch.tensor(BETA, device=cuda), B, v_old=T(vo), ppo=c["ppo"], ppo_clip=PCLIP,
                         v_clip=VCLIP if c["ppo"] else 0.0, stats=stats, clips=(None, None), want_parts=True)
        torch.cuda.synchronize()
        assert used
        for t, name in enumerate(("actor", "critic")):
            for l, lay in enumerate(eng.towers[t]):
                top = t == 0 and not disc and l == len(eng.towers[t]) - 1
                got[f"grad/{name}/{l}"] = O.layer_class(eng._views(lay.kernel)[1].cpu().numpy(),
                                                        eng._views(lay.bias)[1].cpu().numpy(),
                                                        eng.g_log_std.cpu().numpy() if top else None)
                if O.own_class(lay.out_features):
                    got[f"db/{name}/{l}"] = eng._views(lay.bias)[1].cpu().numpy()
        got["stats"] = stats[:6].cpu().numpy()
        assert set(got) == set(want), sorted(set(got) ^ set(want))
        err = O.class_errors(got, want)
        bad += [(B,) + b for b in _report(f"{C.case_id(c)} B={B}", err, ref_err, bar)]
        # the partials are the sum of squares of the gradient the launch wrote (its own gradient: against the oracle's
        # they would carry twice the gradient's error; the bar of test_gpu_mlp.py's same check)
        for t, grp in enumerate(("actor", "critic")):
            s, e = flat.groups[grp]
            torch.testing.assert_close(eng.parts[t].sum(), (flat.grad[s:e] ** 2).sum(), rtol=1e-4, atol=1e-12)
    assert not bad, bad


@pytest.mark.parametrize("c", C.set_a(), ids=C.case_id)
def test_every_tower_list_tanh_with_planted_saturation(cuda, c):
    """Hidden tanh under the Gaussian head's own tanh (both sites live), first-layer columns saturated to +-1.0f."""
    _check_case(cuda, c)


@pytest.mark.parametrize("c", C.set_b(), ids=C.case_id)
def test_every_width_head_and_batch_on_48x32_tanh(cuda, c):
    _check_case(cuda, c)


@pytest.mark.parametrize("c", C.set_c(), ids=C.case_id)
def test_relu_and_lrelu_custom_towers(cuda, c):
    _check_case(cuda, c)


# ------------------------------------------------------------------------------------------------ optimiser, fragments
def _fill_grads(m, it):
    """The same seeded gradient for every parameter by name, whatever the slab's device and layout."""
    for i, (n, p) in enumerate(m.named_parameters()):
        g = torch.randn(p.shape, generator=torch.Generator().manual_seed(1000 * it + i))
        p.grad.copy_(g.to(p.device))


@pytest.mark.parametrize("actor,critic", [((48, 32), (24, 24)), ((8,), (64, 64))])
def test_grouped_adam_writes_fragment_copies_of_custom_towers(cuda, actor, critic):
    """One grouped Adam launch on custom towers: F / G of every layer are frag_f(W) / frag_g(W) of the updated slab
    bitwise (zero pad included), the parameters, moments and step counts equal the float4 sweep path's bitwise (the
    bar of test_gpu_mlp.py::test_item_path_optimizer_matches_sweep), and the parameters equal the torch FusedAdam
    reference of the same gradients."""
    from actor_critic_algs_on_tensorflow_amd.ops.mlp import frag_f, frag_g
    from actor_critic_algs_on_tensorflow_amd.ops.optim import FusedGroupStep, make_optimizer
    c = dict(actor=actor, critic=critic, act="tanh", D=17, head=("gaussian", 6), saturate=False)
    runs = []
    for items in (True, False):
        m, flat, eng = _engine(cuda, C.build(c))
        opts = [make_optimizer("adam", flat, g, lr, max_grad_norm=0.5) for g, lr in (("actor", 3e-3), ("critic", 1e-2))]
        gs = FusedGroupStep(opts, eng.frag_copies() if items else None)
        assert (gs._items[0] is not None) == items
        for it in range(2):
            _fill_grads(m, it)
            gs.step()
        torch.cuda.synchronize()
        runs.append((flat.data.clone(), [(o.m.clone(), o.v.clone(), o.t.clone()) for o in opts], eng, m))
    (p1, st1, eng1, m1), (p0, st0, _, _) = runs
    # the torch FusedAdam reference of the same gradients (the optimisers' CPU path), parameter by parameter, to the bar
    # of test_gpu_kernels.py::test_fused_optimizers
    mc = C.build(c)
    fc = FlatParams(mc.param_groups(), torch.device("cpu"))
    oc = [make_optimizer("adam", fc, g, lr, max_grad_norm=0.5) for g, lr in (("actor", 3e-3), ("critic", 1e-2))]
    for it in range(2):
        _fill_grads(mc, it)
        for o in oc:
            o.step()
    for (n, a), (n2, b) in zip(m1.named_parameters(), mc.named_parameters()):
        assert n == n2
        torch.testing.assert_close(a.detach().cpu(), b.detach(), rtol=1e-5, atol=1e-6, msg=n)
    assert torch.equal(p1, p0)
    for (a, b, cc), (x, y, z) in zip(st1, st0):
        assert torch.equal(a, x) and torch.equal(b, y) and torch.equal(cc, z)
    for tw in eng1.towers:
        for i, lay in enumerate(tw):
            W = lay.kernel.detach()
            assert torch.equal(eng1.F[id(lay)], frag_f(W)), (lay.in_features, lay.out_features)
            assert (id(lay) in eng1.G) == (i > 0)
            if i:
                assert torch.equal(eng1.G[id(lay)], frag_g(W)), (lay.in_features, lay.out_features)


# ------------------------------------------------------------------------------------------------ path selection
def _ref_width_model(act):
    g = torch.Generator().manual_seed(3)
    return MLPActorCritic(17, 6, False, np.full(6, 1.0, np.float32), "basic", generator=g,
                          actor_hidden=(128, 128, 64), critic_hidden=(256, 128), hidden_act=act)


def test_spec_and_fused_rollout_follow_widths_and_activations(cuda):
    from actor_critic_algs_on_tensorflow_amd import envs as E
    from actor_critic_algs_on_tensorflow_amd.ops.mlp import MLPEngine
    env = E.make("HalfCheetahShape-v0", 4, device=cuda, seed=1)
    g = torch.Generator().manual_seed(3)
    ref = MLPActorCritic(17, 6, False, np.full(6, 1.0, np.float32), "basic", generator=g).to(cuda)
    e_ref = MLPEngine(ref, FlatParams(ref.param_groups(), cuda))
    assert e_ref.spec and e_ref.supports_fused_rollout(env)
    _, _, e_relu = _engine(cuda, _ref_width_model("relu"))
    assert e_relu.spec                                  # reference widths, slope activations: the SPEC path is right
    assert not e_relu.supports_fused_rollout(env)       # ... and the one-launch rollout stays the reference actor's
    _, _, e_tanh = _engine(cuda, _ref_width_model("tanh"))
    assert not e_tanh.spec
    assert not e_tanh.supports_fused_rollout(env)       # the reference widths alone do not qualify
    _, _, e_cust = _engine(cuda, C.build(C.set_a()[3]))
    assert not e_cust.spec and not e_cust.supports_fused_rollout(env)


def test_relu_at_reference_widths_spec_matches_generic(cuda):
    """relu at the reference widths takes the SPEC train path (slopes are descriptor words): same gradients as the
    generic path to the bar of test_gpu_mlp.py::test_mlp_spec_train_path_matches_generic's neighbours (1e-4)."""
    B = 33
    r = np.random.RandomState(5)
    obs = torch.as_tensor(r.randn(B, 17).astype(np.float32)).to(cuda)
    act = torch.as_tensor(r.randn(B, 6).astype(np.float32)).to(cuda)
    lo, adv, ret = (torch.as_tensor(r.randn(B).astype(np.float32)).to(cuda) for _ in range(3))
    ce, beta = torch.tensor(0.01, device=cuda), torch.tensor(0.3, device=cuda)
    grads = []
    for spec in (True, False):
        m, flat, eng = _engine(cuda, _ref_width_model("relu"))
        assert eng.spec
        eng.spec = spec
        eng.train(obs, act, lo - 8.0, adv, ret, ce, beta, B, ppo=True, ppo_clip=0.2)
        torch.cuda.synchronize()
        grads.append(flat.grad.clone())
    assert float(grads[0].abs().max()) > 0
    torch.testing.assert_close(grads[0], grads[1], rtol=1e-4, atol=1e-6)


def test_launchers_refuse_hidden_tanh_on_the_reference_only_paths(cuda):
    """A hidden tanh descriptor never runs as identity on the reference-only paths: the SPEC selection falls back to
    the generic kernel, and the one-launch rollout's launcher refuses it before anything is launched."""
    m, flat, eng = _engine(cuda, _ref_width_model("tanh"))
    B = 16
    obs = torch.zeros(B, 17, device=cuda)
    act = torch.zeros(B, 6, device=cuda)
    z = torch.zeros(B, device=cuda)
    c0 = torch.tensor(0.0, device=cuda)
    eng.spec = True   # the binding sees the hidden tanh in the host descriptor and falls back to the generic kernel
    eng.train(obs, act, z, z, z, c0, c0, B)
    torch.cuda.synchronize()
    tr = _trainer(cuda, "HalfCheetahShape-v0", False, actor_hidden=(128, 128, 64), critic_hidden=(256, 128))
    assert tr.mlp.hidden_tanh == [True, True]
    with pytest.raises(RuntimeError, match="mlp_rollout launch failed"):
        tr.mlp.rollout_linear(tr.env, tr.storage, 20, 1)


# ------------------------------------------------------------------------------------------------ trainer level
def _trainer(cuda, env_id, graph, engine="auto", **kw):
    from actor_critic_algs_on_tensorflow_amd.algos.trainer import ActorCriticTrainer
    base = dict(env=env_id, num_envs=4, n_steps=8, ppo_epochs=2, ppo_minibatches=2, device="cuda:0", outdir=None,
                quiet=True, stdout_freq=0, save_every=0, cuda_graph=graph, engine=engine)
    base.update(kw)
    return ActorCriticTrainer(preset("halfcheetah_ppo_tanh64", **base))


ENVS = ["Pendulum-v0", "HalfCheetahShape-v0"]


@pytest.mark.parametrize("env_id", ENVS)
@pytest.mark.parametrize("extra", [{}, dict(norm_obs=True), dict(target_kl=1e-10)], ids=["plain", "norm_obs", "kl"])
def test_trainer_captured_equals_eager(cuda, env_id, extra):
    """3 captured-graph updates == 3 eager updates bitwise, on the per-step path (no one-launch rollout), with the
    generic-path features on custom towers: norm_obs tables, and target_kl low enough to stop after the first step."""
    g, e = _trainer(cuda, env_id, True, **extra), _trainer(cuda, env_id, False, **extra)
    for tr in (g, e):
        assert tr.mlp is not None and not tr.mlp.spec and not tr.mlp.supports_fused_rollout(tr.env)

        def boom(*a, **k):
            raise AssertionError("custom towers must not take the one-launch rollout")
        tr.mlp.rollout_linear = boom
    g.capture(warmup=1)
    assert g.graph is not None
    e.update_body()   # the capture's warm-up update
    p0 = e.flat.data.clone()
    for _ in range(3):
        g.step()
        e.step()
        torch.cuda.synchronize()
        assert torch.equal(g.flat.data, e.flat.data)
        if "target_kl" in extra:
            assert int(g.stats["ppo_steps"]) == 1 == int(e.stats["ppo_steps"])
            assert torch.equal(g._kl_trace, e._kl_trace) and bool((g._kl_trace[2:] == -1).all())
    assert torch.isfinite(e.flat.data).all() and (e.flat.data != p0).any()
    for fa, fb in zip(list(g.mlp.F.values()) + list(g.mlp.G.values()),
                      list(e.mlp.F.values()) + list(e.mlp.G.values())):
        assert torch.equal(fa, fb)


EXTRAS = [{}, dict(norm_obs=True), dict(target_kl=1e-10)]


@pytest.mark.parametrize("env_id", ENVS)
@pytest.mark.parametrize("extra", EXTRAS, ids=["plain", "norm_obs", "kl"])
def test_trainer_update_matches_torch_engine(cuda, env_id, extra):
    """The parameter change against the torch engine's on the same rollouts (same seeds, same actions), plain, with
    ``norm_obs`` (the normalised input tile of the TANH instantiations against ``ObsNormalizer.apply``) and with
    ``target_kl`` low enough that both engines apply exactly one step per update (the KL gate). Two updates: the
    normaliser's tables are the identity during the first (they are merged after its learner), so only the second one
    runs on normalised observations; each update is held to the bar on its own.

    The bar is the fixed one of test_gpu_mlp.py::test_mlp_trainer_matches_torch_engine, direction and length of the
    whole change, not the measured per-class gradient bar: an Adam step divides each element's gradient by its own
    running magnitude, so an element whose gradient is within fp32 rounding of zero legitimately steps either way in
    two fp32 implementations, by up to 2 lr. No per-element bound follows from a gradient error; what a gradient
    error of relative size d does bound is the angle (about d) and the length (about d) of the whole change
    (profiles/mlp_towers.txt section 4 keeps the measured figures)."""
    nat, ref = _trainer(cuda, env_id, False, **extra), _trainer(cuda, env_id, False, engine="torch", **extra)
    assert nat.mlp is not None and ref.mlp is None
    assert torch.equal(nat.flat.data, ref.flat.data)
    for u in range(2):
        pn, pr = nat.flat.data.clone(), ref.flat.data.clone()
        nat.step()
        ref.step()
        torch.cuda.synchronize()
        torch.testing.assert_close(nat.storage.actions, ref.storage.actions, rtol=1e-4, atol=1e-4)
        if "target_kl" in extra:
            print(env_id, "ppo_steps native", int(nat.stats["ppo_steps"]), "torch", int(ref.stats["ppo_steps"]))
            assert int(nat.stats["ppo_steps"]) == 1 == int(ref.stats["ppo_steps"])
        if "norm_obs" in extra:
            sn, sr = nat.obs_norm.state_dict(), ref.obs_norm.state_dict()
            for k in sn:
                torch.testing.assert_close(torch.as_tensor(sn[k]), torch.as_tensor(sr[k]), rtol=1e-6, atol=1e-9, msg=k)
            assert float(sn["count"]) > 0 and float(torch.as_tensor(sn["mean"]).abs().max()) > 0   # tables have moved
        d_n, d_r = (nat.flat.data - pn).double(), (ref.flat.data - pr).double()
        cos = float(torch.nn.functional.cosine_similarity(d_n, d_r, dim=0))
        print(env_id, sorted(extra), "update", u, "cos", cos, "norm ratio", float(d_n.norm() / d_r.norm()),
              "max |dp_native - dp_torch|", float((d_n - d_r).abs().max()), "max |dp_torch|", float(d_r.abs().max()))
        assert float(d_r.norm()) > 0
        assert cos > 0.999 and abs(float(d_n.norm() / d_r.norm()) - 1) < 1e-2


@pytest.mark.parametrize("env_id", ENVS)
def test_eval_every_on_custom_towers(cuda, env_id):
    on = _trainer(cuda, env_id, False, eval_every=1, eval_envs=3, eval_episodes=1)
    off = _trainer(cuda, env_id, False)
    assert on.evaluator.path == "native"   # per step: the one-launch evaluation is the reference actor's
    for tr in (on, off):
        tr.train(2)
    torch.cuda.synchronize()
    assert len(on.eval_history) == 2 and np.isfinite(on.eval_history[-1]["eval_ret_mean"])
    assert torch.equal(on.flat.data, off.flat.data)


def test_agent_acts_through_the_engine_on_custom_towers(cuda):
    from actor_critic_algs_on_tensorflow_amd.api import Agent
    m = C.build(C.set_a()[3])
    ag = Agent(m, device="cuda:0", seed=3)
    obs = np.random.RandomState(1).randn(9, 17).astype(np.float32)
    a, lp, _ = ag.act(obs)
    assert ag._eng is not None and ag._eng[0] == "mlp" and not ag._eng[1].spec
    ref = Agent(C.build(C.set_a()[3]), device="cuda:0", seed=3, engine="torch")
    a2, lp2, _ = ref.act(obs)
    np.testing.assert_allclose(a, a2, rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(lp, lp2, rtol=1e-4, atol=1e-4)


def test_agent_auto_falls_back_outside_the_engine_limits(cuda):
    """A tower the engine cannot take (width 40, trained on the torch engine): ``engine="auto"`` acts through the
    PyTorch modules, with the parameters left where they were; ``engine="native"`` names the limit."""
    from actor_critic_algs_on_tensorflow_amd.api import Agent
    mk = lambda: MLPActorCritic(17, 6, False, np.full(6, 1.0, np.float32), "basic",
                                generator=torch.Generator().manual_seed(4), actor_hidden=(40,), critic_hidden=(8,))
    obs = np.random.RandomState(2).randn(5, 17).astype(np.float32)
    ag = Agent(mk(), device="cuda:0", seed=3)
    a, lp, _ = ag.act(obs)
    assert ag._eng is None
    a2, lp2, _ = Agent(mk(), device="cuda:0", seed=3, engine="torch").act(obs)
    assert np.array_equal(a, a2) and np.array_equal(lp, lp2)
    with pytest.raises(ValueError, match="actor_hidden.*multiple of 16"):
        Agent(mk(), device="cuda:0", engine="native").act(obs)
