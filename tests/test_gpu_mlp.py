"""Fused MLP engine (csrc/kernels/mlp.hip via ops/mlp.py) against fp32 PyTorch references of the same maths.

Every check builds the reference MLP actor-critic (both the Basic and the A3C variant, Gaussian and
categorical heads), runs the HIP kernels on its flat parameter slab, and compares with autograd on an identical
copy of the model.
"""
import copy

import pytest
import torch

from actor_critic_algs_on_tensorflow_amd.algos import losses as L
from actor_critic_algs_on_tensorflow_amd.models.policy import MLPActorCritic
from actor_critic_algs_on_tensorflow_amd.ops import distributions as D
from actor_critic_algs_on_tensorflow_amd.ops.optim import FlatParams

pytestmark = pytest.mark.gpu

CASES = [  # (ob_dim, ac_dim, discrete, variant)
    (17, 6, False, "basic"),
    (17, 6, False, "a3c"),
    (3, 1, False, "a3c"),
    (4, 2, True, "basic"),
    (8, 5, True, "a3c"),
]


def _model(cuda, ob, ac, disc, variant, seed=0):
    import numpy as np
    g = torch.Generator().manual_seed(seed)
    m = MLPActorCritic(ob, ac, disc, None if disc else np.full(ac, 2.0, np.float32), variant, generator=g)
    if not disc:
        with torch.no_grad():
            m.actor.log_std.copy_(torch.linspace(-0.7, 0.4, ac))
    ref = copy.deepcopy(m).to(cuda)
    m = m.to(cuda)
    flat = FlatParams(m.param_groups(), cuda)
    from actor_critic_algs_on_tensorflow_amd.ops.mlp import MLPEngine
    return m, ref, flat, MLPEngine(m, flat)


@pytest.mark.parametrize("case", CASES)
def test_mlp_policy_step_and_evaluate(cuda, case):
    ob, ac, disc, variant = case
    m, ref, flat, eng = _model(cuda, ob, ac, disc, variant)
    N = 70
    obs = torch.randn(N, ob, device=cuda)
    tg = torch.randint(0, 1000, (N,), device=cuda, dtype=torch.int64)
    ids = torch.arange(N, device=cuda, dtype=torch.int64) + 5
    act = torch.empty((N,) if disc else (N, ac), dtype=torch.int32 if disc else torch.float32, device=cuda)
    logp, ent, v = (torch.empty(N, device=cuda) for _ in range(3))
    eng.policy_step(obs, act, logp, ent, v, tg, ids, 20, 1234)
    with torch.no_grad():
        pi, v_ref = ref(obs)
        keys = tg * (1 << 20) + ids
        a_ref, lp_ref, ent_ref = (D.categorical_sample_ref(pi, keys, 1234) if disc else
                                  D.gaussian_sample_ref(pi, ref.actor.log_std, keys, 1234))
    torch.testing.assert_close(v, v_ref, rtol=1e-4, atol=1e-5)
    if disc:
        assert (act == a_ref).float().mean() > 0.97
    else:
        torch.testing.assert_close(act, a_ref, rtol=1e-4, atol=1e-5)
        torch.testing.assert_close(logp, lp_ref, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(ent, ent_ref, rtol=1e-4, atol=1e-5)
    # evaluate given actions
    lp2, ent2, v2 = (torch.empty(N, device=cuda) for _ in range(3))
    eng.evaluate(obs, a_ref, lp2, ent2, v2)
    with torch.no_grad():
        lp_e, ent_e, v_e = ref.evaluate(obs, a_ref)
    torch.testing.assert_close(lp2, lp_e, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(ent2, ent_e, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(v2, v_e, rtol=1e-4, atol=1e-5)
    out = torch.empty(N, device=cuda)
    eng.value(obs, out)
    torch.testing.assert_close(out, v_e, rtol=1e-4, atol=1e-5)
    if disc:
        # decisive-row rule (tests/oracles/sampling_oracle.py) on top of the agreement share above: wherever the fp64
        # gap of the reference model's perturbed logits exceeds the margin (widened by 4 x the engine's measured
        # difference from that model on these rows), the engine's action is the oracle's
        import os
        import sys
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "oracles"))
        import sampling_oracle as O
        o = O.categorical(pi, keys, 1234)
        diff = max(float((v - v_ref).abs().max()), float((lp2 - lp_e).abs().max()), float((ent2 - ent_e).abs().max()))
        dec = O.decisive(o["gap"], O.MARGIN + 4 * diff)
        assert float(dec.double().mean()) >= 0.95
        assert torch.equal(act.cpu().long()[dec], o["act"][dec])
        torch.testing.assert_close(logp.cpu()[dec], o["logp"].float()[dec], rtol=1e-4, atol=1e-4)


def _ref_grads(ref, obs, act, lo, adv, ret, v_old, ppo, beta, ce, clip, vclip):
    ref.zero_grad()
    logp, ent, v = ref.evaluate(obs, act)
    if ppo:
        a_loss, pg, kl, entm, cf = L.ppo_actor_loss(logp, lo, adv, ent, clip, ce, beta)
    else:
        a_loss, pg, kl, entm = L.actor_loss(logp, lo, adv, ent, beta, ce)
        cf = torch.zeros(())
    c_loss = L.value_loss(v, ret, v_old if ppo else None, vclip if ppo else None)
    (a_loss + c_loss).backward()
    grads = {n: (p.grad.detach().clone() if p.grad is not None else torch.zeros_like(p))
             for n, p in ref.named_parameters()}
    return grads, dict(
        pg=pg, kl=kl, entropy=entm, crit_loss=c_loss, clipfrac=cf, act_loss=a_loss)


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("ppo", [False, True])
def test_mlp_train_gradients_match_autograd(cuda, case, ppo):
    ob, ac, disc, variant = case
    m, ref, flat, eng = _model(cuda, ob, ac, disc, variant, seed=3)
    # fixed inputs: an unseeded draw occasionally puts a pre-activation within rounding of the leaky-ReLU kink, where
    # the kernel and autograd legitimately take different sides (one run in ~40 failed the 2e-3 bar on one element)
    torch.manual_seed(1234)
    Bfull, B = 300, 200
    obs = torch.randn(Bfull, ob, device=cuda)
    with torch.no_grad():
        pi, v0 = ref(obs)
        keys = torch.arange(Bfull, device=cuda, dtype=torch.int64)
        act, lp0, _ = (D.categorical_sample_ref(pi, keys, 7) if disc else
                       D.gaussian_sample_ref(pi, ref.actor.log_std, keys, 7))
    lo = lp0 + 0.3 * torch.randn(Bfull, device=cuda)   # make the ratio / KL terms non-trivial
    adv = torch.randn(Bfull, device=cuda)
    ret = v0 + torch.randn(Bfull, device=cuda)
    v_old = v0 + 0.1 * torch.randn(Bfull, device=cuda)
    idx = torch.randperm(Bfull, device=cuda)[:B]
    beta, ce = torch.tensor(0.7, device=cuda), torch.tensor(0.05, device=cuda)
    stats = torch.zeros(16, device=cuda)
    used = eng.train(obs, act, lo, adv, ret, ce, beta, B, idx=idx, v_old=v_old, ppo=ppo, ppo_clip=0.2,
                     v_clip=0.15 if ppo else 0.0, stats=stats, clips=(None, None), want_parts=True)
    torch.cuda.synchronize()
    g_ref, s_ref = _ref_grads(ref, obs[idx], act[idx], lo[idx], adv[idx], ret[idx], v_old[idx], ppo, beta, ce,
                              0.2, 0.15)
    for (n, p) in m.named_parameters():
        torch.testing.assert_close(p.grad, g_ref[n], rtol=2e-3, atol=2e-5, msg=lambda s: f"{n}: {s}")
    names = ("pg", "kl", "entropy", "crit_loss", "clipfrac", "act_loss")
    slots = (0, 1, 2, 3, 4, 5)
    for nm, k in zip(names, slots):
        torch.testing.assert_close(stats[k], s_ref[nm].float().to(cuda), rtol=1e-3, atol=1e-5, msg=nm)
    assert used
    # per-tower sums of squares == the gradient norms of the actor / critic groups
    for t, grp in enumerate(("actor", "critic")):
        s, e = flat.groups[grp]
        torch.testing.assert_close(eng.parts[t].sum(), (flat.grad[s:e] ** 2).sum(), rtol=1e-4, atol=1e-9)


def test_mlp_trainer_matches_torch_engine(cuda):
    """MuJoCo-shape PPO (BASELINE config 5, scaled down): native MLP engine vs the autograd engine, same seeds."""
    from actor_critic_algs_on_tensorflow_amd import preset
    from actor_critic_algs_on_tensorflow_amd.algos.trainer import ActorCriticTrainer
    kw = dict(num_envs=16, n_steps=32, ppo_epochs=2, ppo_minibatches=4, device="cuda:0", outdir=None, quiet=True,
              stdout_freq=0, save_every=0, cuda_graph=False)
    nat = ActorCriticTrainer(preset("mujoco_ppo_dp8", engine="auto", **kw))
    ref = ActorCriticTrainer(preset("mujoco_ppo_dp8", engine="torch", **kw))
    assert nat.mlp is not None and ref.mlp is None
    torch.testing.assert_close(nat.flat.data, ref.flat.data)
    p0 = nat.flat.data.clone()
    nat.step()
    ref.step()
    torch.cuda.synchronize()
    torch.testing.assert_close(nat.storage.actions, ref.storage.actions, rtol=1e-4, atol=1e-4)
    d_n, d_r = nat.flat.data - p0, ref.flat.data - p0
    cos = torch.nn.functional.cosine_similarity(d_n.double(), d_r.double(), dim=0)
    assert cos > 0.999, float(cos)
    assert abs(float(d_n.norm() / d_r.norm()) - 1) < 1e-2


@pytest.mark.parametrize("preset_name,kw", [
    ("mujoco_ppo_dp8", dict(num_envs=16, n_steps=32, ppo_epochs=2, ppo_minibatches=4)),
    ("cartpole_cpu", dict(num_envs=8, n_steps=5)),
    ("basic_ac", dict(algo="a2c", env="Pendulum-v0", num_envs=8, n_steps=16)),
])
def test_mlp_trainer_graph_capture(cuda, preset_name, kw):
    """The whole native MLP update (rollout launches + learner launches) replays as one hipGraph."""
    from actor_critic_algs_on_tensorflow_amd import preset
    from actor_critic_algs_on_tensorflow_amd.algos.trainer import ActorCriticTrainer
    cfg = preset(preset_name, device="cuda:0", outdir=None, quiet=True, stdout_freq=0, save_every=0,
                 cuda_graph=True, **kw)
    tr = ActorCriticTrainer(cfg)
    assert tr.mlp is not None
    tr.capture(warmup=1)
    assert tr.graph is not None and tr.graph[0] == "single"
    p0 = tr.flat.data.clone()
    for _ in range(3):
        tr.step()
    torch.cuda.synchronize()
    assert torch.isfinite(tr.flat.data).all() and (tr.flat.data != p0).any()
    assert torch.isfinite(tr.stats_buf).all()


@pytest.mark.parametrize("name", ["adam", "rmsprop"])
def test_multi_group_optimizer_matches_separate_steps(cuda, name):
    """Actor + critic groups stepped by ONE opt_multi launch == each group stepped by its own kernel."""
    from actor_critic_algs_on_tensorflow_amd.ops.optim import FlatParams, FusedGroupStep, make_optimizer
    torch.manual_seed(0)
    ps = {"actor": [torch.nn.Parameter(torch.randn(37, 5)), torch.nn.Parameter(torch.randn(7))],
          "critic": [torch.nn.Parameter(torch.randn(129, 3))]}
    flats = []
    for _ in range(2):
        f = FlatParams({k: [torch.nn.Parameter(p.detach().clone()) for p in v] for k, v in ps.items()}, cuda)
        f.grad.copy_(torch.randn(f.numel, generator=torch.Generator().manual_seed(1)).to(cuda))
        flats.append(f)
    cfgs = {"actor": dict(lr=3e-3, clip_value=0.05, max_grad_norm=0.5), "critic": dict(lr=1e-2, max_grad_norm=0.3)}
    sep = [make_optimizer(name, flats[0], g, **c) for g, c in cfgs.items()]
    grp = [make_optimizer(name, flats[1], g, **c) for g, c in cfgs.items()]
    for o in sep + grp:
        o.zero_grad_after = True
    gs = FusedGroupStep(grp)
    for it in range(3):
        for o in sep:
            o.step()
        gs.step()
        g = torch.randn(flats[0].numel, generator=torch.Generator().manual_seed(10 + it)).to(cuda)
        flats[0].grad.copy_(g)
        flats[1].grad.copy_(g)
    torch.cuda.synchronize()
    torch.testing.assert_close(flats[1].data, flats[0].data, rtol=0, atol=0)
    for a, b in zip(sep, grp):
        torch.testing.assert_close(b.v, a.v, rtol=0, atol=0)


def test_prp_permutation_kernel_matches_oracle(cuda):
    from actor_critic_algs_on_tensorflow_amd import _native
    from actor_critic_algs_on_tensorflow_amd.envs import rng
    for n, uc, ep in ((16384, 3, 2), (1000, 0, 0), (4097, 12, 9), (1, 5, 1)):
        out = torch.empty(n, dtype=torch.int64, device=cuda)
        ucd = torch.tensor([uc], dtype=torch.int64, device=cuda)
        _native.require().prp_perm(out, 777, ucd, ep)
        ref = rng.prp(torch.arange(n), n, rng.minibatch_key(777, torch.tensor(uc), ep))
        assert torch.equal(out.cpu(), ref)
        assert torch.equal(torch.sort(out.cpu()).values, torch.arange(n))


def test_optimizer_writes_fragment_copies(cuda):
    """The multi-group optimiser launch keeps the MLP engine's fp32 weight fragment copies (forward F, data-gradient
    G) equal to the fragment order of W after every step, and the refresh pass rewrites them."""
    from actor_critic_algs_on_tensorflow_amd.ops.mlp import frag_f, frag_g
    from actor_critic_algs_on_tensorflow_amd import preset
    from actor_critic_algs_on_tensorflow_amd.algos.trainer import ActorCriticTrainer
    tr = ActorCriticTrainer(preset("mujoco_ppo_dp8", num_envs=8, n_steps=16, ppo_epochs=1, ppo_minibatches=2,
                                   device="cuda:0", outdir=None, quiet=True, stdout_freq=0, save_every=0,
                                   cuda_graph=False))
    for _ in range(2):
        tr.step()
    torch.cuda.synchronize()
    assert tr._group_step is not None and tr._group_step._items[0] is not None

    def check():
        for tw in tr.mlp.towers:
            for i, lay in enumerate(tw):
                W = lay.kernel.detach()
                assert torch.equal(tr.mlp.F[id(lay)], frag_f(W)), lay
                if i:
                    assert torch.equal(tr.mlp.G[id(lay)], frag_g(W)), lay
                else:
                    assert id(lay) not in tr.mlp.G
    check()
    with torch.no_grad():
        tr.flat.data.mul_(0.5)
    tr.mlp.sync_shadow()
    check()


@pytest.mark.parametrize("frames,num_envs", [(1, 20), (3, 37)])
def test_fused_rollout_matches_per_step_launches(cuda, frames, num_envs):
    """mlp_rollout_kernel (whole T-step rollout of the MuJoCo-shaped bank in one launch, 4-env workgroups on 4x4x1
    MFMAs + one batched critic launch) == T x (policy_step launch + env_step_linear launch) + value launch: the same
    resets, done flags and step counters exactly, actions, log-probs, observations, rewards, values and env state up
    to the actor's fp32 summation order (measured max |diff| ~1e-6; episode limit 7 so resets happen inside the
    rollout; partial 4-env tiles)."""
    from actor_critic_algs_on_tensorflow_amd import preset
    from actor_critic_algs_on_tensorflow_amd.algos.trainer import ActorCriticTrainer
    kw = dict(num_envs=num_envs, n_steps=24, frames=frames, ppo_epochs=1, ppo_minibatches=2, device="cuda:0",
              outdir=None, quiet=True, stdout_freq=0, save_every=0, cuda_graph=False)
    trs = [ActorCriticTrainer(preset("mujoco_ppo_dp8", fused_rollout=f, **kw)) for f in (True, False)]
    for tr in trs:
        assert tr.mlp is not None and tr.mlp.supports_fused_rollout(tr.env)
        tr.env.max_episode_steps = 7
    for _ in range(2):   # second rollout starts from the written-back env bank
        for tr in trs:
            tr.collect()
        torch.cuda.synchronize()
        a, b = (tr.storage for tr in trs)
        for name in ("dones", "truncated"):
            assert torch.equal(getattr(a, name), getattr(b, name)), name
        for name in ("obs", "actions", "logp", "entropy", "rewards", "values"):
            x, y = getattr(a, name), getattr(b, name)
            torch.testing.assert_close(x, y, rtol=1e-4, atol=1e-4, msg=name)
        ea, eb = (tr.env for tr in trs)
        for name in ("t", "tg"):
            assert torch.equal(getattr(ea, name), getattr(eb, name)), name
        for name in ("state", "ep_ret"):
            torch.testing.assert_close(getattr(ea, name), getattr(eb, name), rtol=1e-4, atol=1e-4, msg=name)
        torch.testing.assert_close(ea.ep_stats, eb.ep_stats, rtol=1e-5, atol=1e-4)
        assert int(a.dones.sum()) > 0
        for tr in trs:
            tr.storage.roll_over()


def test_seg_stats_kernel_matches_reference(cuda):
    """Per-variable mean / std / max / min (TensorBoard variable summaries) in one launch vs float64 torch."""
    from actor_critic_algs_on_tensorflow_amd.ops.stats import seg_stats, seg_stats_ref
    x = torch.randn(300000, device=cuda) * 3 + 1
    segs = torch.tensor([[0, 1], [7, 100], [1000, 65536], [70000, 229999], [5, 3]], device=cuda)
    torch.testing.assert_close(seg_stats(x, segs), seg_stats_ref(x, segs), rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("case", [(17, 6, False, "basic"), (4, 2, True, "basic"), (40, 3, False, "basic")])
def test_mlp_spec_train_path_matches_generic(cuda, case):
    """The train launch's SPEC path (reference towers, every weight fragment preloaded into registers, split-K head
    layers) == the generic layer loop: same gradients to fp32 summation-order noise, same statistics."""
    ob, ac, disc, variant = case
    m, ref, flat, eng = _model(cuda, ob, ac, disc, variant, seed=5)
    B = 512
    obs = torch.randn(B, ob, device=cuda)
    with torch.no_grad():
        pi, v0 = ref(obs)
        keys = torch.arange(B, device=cuda, dtype=torch.int64)
        act, lp0, _ = (D.categorical_sample_ref(pi, keys, 9) if disc else
                       D.gaussian_sample_ref(pi, ref.actor.log_std, keys, 9))
    lo = lp0 + 0.2 * torch.randn(B, device=cuda)
    adv, ret = torch.randn(B, device=cuda), v0 + torch.randn(B, device=cuda)
    beta, ce = torch.tensor(0.3, device=cuda), torch.tensor(0.02, device=cuda)
    out = []
    for spec in (True, False):
        eng.spec = spec
        flat.grad.zero_()
        stats = torch.zeros(16, device=cuda)
        eng.train(obs, act, lo, adv, ret, ce, beta, B, v_old=v0, ppo=True, ppo_clip=0.2, stats=stats,
                  want_parts=True)
        torch.cuda.synchronize()
        out.append((flat.grad.clone(), stats.clone(), [p.clone() for p in eng.parts]))
    (g1, s1, p1), (g0, s0, p0) = out
    scale = g0.abs().max()
    assert (g1 - g0).abs().max() <= 1e-5 * scale, float((g1 - g0).abs().max() / scale)
    torch.testing.assert_close(s1, s0, rtol=1e-5, atol=1e-7)
    for a, b in zip(p1, p0):
        torch.testing.assert_close(a.sum(), b.sum(), rtol=1e-5, atol=1e-9)


@pytest.mark.parametrize("variant", ["basic", "a3c"])
def test_item_path_optimizer_matches_sweep(cuda, variant):
    """The optimiser's item path (MLP segments: 16 x 64 weight blocks that also write the fragment copies, small
    weights, element ranges) updates every parameter, moment and step count exactly as the float4 sweep path."""
    from actor_critic_algs_on_tensorflow_amd.ops.mlp import frag_f, frag_g
    from actor_critic_algs_on_tensorflow_amd.ops.optim import FusedGroupStep, make_optimizer
    runs = []
    for items in (True, False):
        m, ref, flat, eng = _model(cuda, 17, 6, False, variant, seed=11)
        opts = [make_optimizer("adam", flat, g, lr, max_grad_norm=0.5)
                for g, lr in (("actor", 3e-3), ("critic", 1e-2))]
        gs = FusedGroupStep(opts, eng.frag_copies() if items else None)
        assert (gs._items[0] is not None) == items
        for it in range(3):
            flat.grad.copy_(torch.randn(flat.numel, generator=torch.Generator().manual_seed(20 + it)).to(cuda))
            gs.step()
        torch.cuda.synchronize()
        runs.append((flat.data.clone(), [(o.m.clone(), o.v.clone(), o.t.clone()) for o in opts], eng, m))
    (p1, st1, eng1, m1), (p0, st0, _, _) = runs
    assert torch.equal(p1, p0)
    for (a, b, c), (x, y, z) in zip(st1, st0):
        assert torch.equal(a, x) and torch.equal(b, y) and torch.equal(c, z)
    for i, lay in enumerate(l for tw in eng1.towers for l in tw):
        assert torch.equal(eng1.F[id(lay)], frag_f(lay.kernel.detach()))
        if id(lay) in eng1.G:
            assert torch.equal(eng1.G[id(lay)], frag_g(lay.kernel.detach()))
