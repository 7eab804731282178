"""Running observation normalisation on the GPU: ``obs_norm_prepare`` / ``obs_norm_merge`` (``obs_norm.hip``) against
the torch forms of ``ops/obs_norm.py`` and numpy's fp64 statistics, the in-kernel normalisation of ``mlp_fwd_kernel``'s
generic input tile (modes 0 and 1) and of ``mlp_rollout_kernel``'s NORM instantiations against ``apply`` in front of the
same launches, and the native MLP trainer with ``norm_obs=True`` (graph replay == eager, state == the statistics of the
recorded raw rollouts). Bars: ``tests/test_obs_norm_cpu.py``."""
import numpy as np
import pytest
import torch

from test_obs_norm_cpu import SIZES, _data, check_state, spy

pytestmark = pytest.mark.gpu

T = 24


def _set_tables(norm, seed=0, clip=1.5):
    """Test tables: means in +-0.5 (away from 0), stds in [0.5, 2], clip 1.5 -- so that clipping occurs."""
    g = torch.Generator().manual_seed(seed)
    D = norm.D
    sign = torch.where(torch.rand(D, generator=g) < 0.5, -1.0, 1.0)
    mean = sign * (0.1 + 0.4 * torch.rand(D, generator=g))
    std = 0.5 + 1.5 * torch.rand(D, generator=g)
    norm.mean32.copy_(mean)
    norm.istd32.copy_(1.0 / std)
    norm.clip = clip
    return norm


# ------------------------------------------------------------------------------------------------ 8. prepare
@pytest.mark.parametrize("R,D,r_stat", [(1, 4, 1), (37, 17, 30), (18, 51, 15), (1000, 17, 1000),
                                        (257 * 8, 34, 256 * 8)])
def test_prepare_matches_fallback(cuda, R, D, r_stat):
    from actor_critic_algs_on_tensorflow_amd import _native
    from actor_critic_algs_on_tensorflow_amd.ops.obs_norm import ObsNormalizer
    ops = _native.require()
    g = torch.Generator().manual_seed(R + D)
    wide = torch.randn(R, D + 3, generator=g) * 1.7   # rows with a stride of D + 3 floats
    ref = _set_tables(ObsNormalizer(D), seed=D)
    ref.mean.copy_(ref.mean32.double() + 0.01)        # statistics about a running mean that is not the data's
    ref.count.fill_(5.0)
    dev = ObsNormalizer(D, clip=1.5, device=cuda)
    dev.state.copy_(ref.state)
    dev.tables.copy_(ref.tables)
    obs_c = wide[:, :D]
    obs_g = wide.to(cuda)[:, :D]
    assert not obs_g.is_contiguous() or R == 1
    plane_c = ref.prepare(obs_c, torch.empty(R, D), r_stat)
    runs = []
    for _ in range(2):
        plane = torch.full((R, D), float("nan"), device=cuda)
        dev.prepare(obs_g, plane, r_stat)
        nparts, nb = dev._pending
        assert nparts == (R + 63) // 64 and nb == r_stat
        dev.batch.fill_(float("nan"))
        ops.obs_norm_merge(dev._part, nparts, dev.batch, nb, dev.state, dev.tables, 0, dev.eps)
        torch.cuda.synchronize()
        runs.append((plane.cpu(), dev.batch.cpu().clone()))
    assert torch.equal(runs[0][0], plane_c), "plane bitwise equal to the fallback's"
    assert (runs[0][0].abs() == 1.5).any() or R == 1
    want = ref.batch_stats(obs_c[:r_stat])
    print("batch rel err", ((runs[0][1] - want).abs() / want.abs().clamp_min(1e-300)).max().item())
    torch.testing.assert_close(runs[0][1], want, rtol=1e-12, atol=0)
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), "bitwise reproducible"
    # stage 0 touches neither the state nor the tables
    assert torch.equal(dev.state.cpu(), ref.state) and torch.equal(dev.tables.cpu(), ref.tables)


# ------------------------------------------------------------------------------------------------ 9. merge
def test_merge_three_batches_matches_numpy(cuda):
    from actor_critic_algs_on_tensorflow_amd import _native
    from actor_critic_algs_on_tensorflow_amd.ops.obs_norm import ObsNormalizer
    ops = _native.require()
    D = 17
    fused, split = ObsNormalizer(D, device=cuda), ObsNormalizer(D, device=cuda)
    seen = []
    for b in _data()[:3]:
        x = b.to(cuda)
        plane = torch.empty_like(x)
        fused.prepare(x, plane, x.shape[0])
        fused.merge()                                   # stages 0 and 1 in one launch
        split.prepare(x, plane, x.shape[0])
        nparts, nb = split._pending
        split._pending = None
        ops.obs_norm_merge(split._part, nparts, split.batch, nb, split.state, split.tables, 0, split.eps)
        ops.obs_norm_merge(None, 0, split.batch, 0.0, split.state, split.tables, 1, split.eps)
        torch.cuda.synchronize()
        seen.append(b)
        check_state(fused, torch.cat(seen), f"{len(seen)} batches")
        assert torch.equal(fused.state, split.state) and torch.equal(fused.tables, split.tables)
    assert float(fused.count[0]) == sum(SIZES[:3])
    # the torch form of the merge (the CPU path) computes the same state from the same batch vector
    cpu = ObsNormalizer(D)
    for b in _data()[:3]:
        cpu.prepare(b, torch.empty_like(b), b.shape[0])
        cpu.merge()
    np.testing.assert_allclose(fused.state.cpu().numpy(), cpu.state.numpy(), rtol=1e-10, atol=1e-12)


# ------------------------------------------------------------------------------------------------ 10. / 11. mlp_fwd
def _engine_trainer(kind, N):
    from actor_critic_algs_on_tensorflow_amd import preset
    from actor_critic_algs_on_tensorflow_amd.algos.trainer import ActorCriticTrainer
    name = {"gauss17": "mujoco_ppo_dp8", "cartpole": "cartpole_cpu", "pendulum": "pendulum_ppo"}[kind]
    tr = ActorCriticTrainer(preset(name, num_envs=N, n_steps=4, device="cuda:0", outdir=None, quiet=True, stdout_freq=0,
                                   save_every=0, cuda_graph=False))
    assert tr.mlp is not None and tr.mlp.D == {"gauss17": 17, "cartpole": 4, "pendulum": 3}[kind]
    return tr


@pytest.mark.parametrize("kind", ["gauss17", "cartpole", "pendulum"])
@pytest.mark.parametrize("N", [5, 33])
def test_policy_step_value_evaluate_normalise_in_kernel(cuda, kind, N):
    """With a normaliser attached the launches take RAW observations; every output is bitwise what the same launch
    computes from ``apply(obs)`` without one."""
    from actor_critic_algs_on_tensorflow_amd.algos.trainer import KEY_ENV_BITS
    from actor_critic_algs_on_tensorflow_amd.ops.obs_norm import ObsNormalizer
    tr = _engine_trainer(kind, N)
    eng, env = tr.mlp, tr.env
    norm = _set_tables(ObsNormalizer(eng.D, device=cuda), seed=N)
    g = torch.Generator().manual_seed(N)
    obs = (torch.randn(N, eng.D, generator=g) * 1.5).to(cuda)
    pre = norm.apply(obs)
    assert (pre.abs() == 1.5).any() and not torch.equal(pre, obs)

    def run(o, attach):
        eng.obs_norm = norm if attach else None
        st = tr.storage
        act, logp, ent, v = (torch.zeros_like(x) for x in (st.actions[0], st.logp[0], st.entropy[0], st.values[0]))
        eng.policy_step(o, act, logp, ent, v, env.tg, env.env_ids, KEY_ENV_BITS, tr.policy_seed)
        v1 = eng.value(o, torch.zeros(N, device=cuda))
        lp2, en2, v2 = (torch.zeros(N, device=cuda) for _ in range(3))
        eng.evaluate(o, act, lp2, en2, v2)
        lp3 = torch.zeros(N, device=cuda)
        eng.evaluate(o, act, lp3)   # actor tower alone
        torch.cuda.synchronize()
        eng.obs_norm = None
        return dict(act=act, logp=logp, ent=ent, v=v, v1=v1, lp2=lp2, en2=en2, v2=v2, lp3=lp3)

    a, b = run(obs, True), run(pre, False)
    raw = run(obs, False)
    for k in a:
        assert torch.isfinite(a[k].float()).all(), k
        assert torch.equal(a[k], b[k]), k
    assert not torch.equal(a["v"], raw["v"]), "the tables act"


def test_mlp_fwd_rejects_tables_in_train_mode(cuda):
    """The learner reads the pre-normalised plane: a train launch (mode 2) with tables would normalise twice, so the
    launcher refuses it before anything runs; the same operands without tables launch."""
    from actor_critic_algs_on_tensorflow_amd import _native
    from actor_critic_algs_on_tensorflow_amd.ops.obs_norm import ObsNormalizer
    ops = _native.require()
    tr = _engine_trainer("gauss17", 4)
    eng = tr.mlp
    B = 16
    desc, _ = eng.desc(B)
    norm = _set_tables(ObsNormalizer(eng.D, device=cuda))
    obs = torch.randn(B, eng.D, device=cuda)
    act = torch.randn(B, eng.A, device=cuda)
    row = lambda: torch.randn(B, device=cuda)
    logp, adv, ret = row(), row(), row()

    out = torch.zeros(B, device=cuda)

    def launch(mode, tables, hdesc):
        ntw = 2 if mode == 2 else 1   # evaluate: the actor tower alone (no v_out)
        ops.mlp_fwd(desc, 0, ntw, mode, eng.lds_bytes(mode, 0, ntw), obs, None, None, 0, 0, 0, 0, B, eng.head, eng.A,
                    eng.log_std, eng.ac_scale, None, None, 0, 0, None, out if mode == 1 else None, None, None, act,
                    logp, adv, ret, None, tr.ent_coef, tr.kl_coef, 1.0, 0.0, 0.0, False,
                    eng.g_log_std if mode == 2 else None, eng.mstats if mode == 2 else None,
                    eng._mpart(B) if mode == 2 else None, None, hdesc, tables, 1.5)

    g0 = tr.flat.grad.clone()
    for hdesc in (None, eng._hdescs[B]):   # the generic and the SPEC train path
        with pytest.raises(RuntimeError, match="mlp_fwd"):
            launch(2, norm.tables, hdesc)
    torch.cuda.synchronize()
    assert torch.equal(tr.flat.grad, g0)
    with pytest.raises(RuntimeError, match="norm_tables"):
        launch(1, norm.tables[:, :5].contiguous(), None)
    launch(1, norm.tables, None)
    launch(2, None, eng._hdescs[B])
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 12. fused rollout
def _trainer(frames=1, num_envs=5, **over):
    from actor_critic_algs_on_tensorflow_amd import preset
    from actor_critic_algs_on_tensorflow_amd.algos.trainer import ActorCriticTrainer
    kw = dict(num_envs=num_envs, n_steps=T, frames=frames, ppo_epochs=1, ppo_minibatches=2, device="cuda:0",
              outdir=None, quiet=True, stdout_freq=0, save_every=0, cuda_graph=False, norm_obs=True)
    kw.update(over)
    tr = ActorCriticTrainer(preset("mujoco_ppo_dp8", **kw))
    assert tr.mlp is not None and tr.mlp.supports_fused_rollout(tr.env) and tr.mlp.obs_norm is tr.obs_norm
    return tr


def _no_per_step(*a, **k):
    raise AssertionError("norm_obs left the one-launch rollout: policy_step was called")


@pytest.mark.parametrize("frames,num_envs,boot", [(1, 5, False), (3, 9, False), (1, 5, True), (3, 9, True)])
def test_fused_norm_rollout_matches_per_step_launches(cuda, frames, num_envs, boot):
    """NORM (x BOOT) instantiations of both KP0 widths, a partial 4-env tile, episode limit 7 with staggered episode
    clocks: flags and counters exactly, everything the actor's fp32 summation order touches to 1e-4 (the project's bar
    for fused against per-step). ``storage.obs`` stays raw on the fused side."""
    N = num_envs
    trs = [_trainer(frames, N, fused_rollout=f, bootstrap_on_timeout=boot) for f in (True, False)]
    for tr in trs:
        tr.env.max_episode_steps = 7
        tr.env.t.copy_(torch.arange(N, device=cuda) % 7)
        _set_tables(tr.obs_norm, seed=frames)
    fused, per_step = trs
    fused.mlp.policy_step = _no_per_step
    for it in range(2):   # the second rollout starts from the written-back env bank
        for tr in trs:
            tr.collect()
        torch.cuda.synchronize()
        a, b = fused.storage, per_step.storage
        for name in ("dones", "truncated"):
            assert torch.equal(getattr(a, name), getattr(b, name)), name
        assert int(a.truncated.sum()) >= 3 * N
        for name in ("obs", "actions", "logp", "entropy", "rewards", "values"):
            assert torch.isfinite(getattr(a, name)).all(), name
            torch.testing.assert_close(getattr(a, name), getattr(b, name), rtol=1e-4, atol=1e-4, msg=name)
        ea, eb = fused.env, per_step.env
        for name in ("t", "tg"):
            assert torch.equal(getattr(ea, name), getattr(eb, name)), name
        for name in ("state", "ep_ret"):
            torch.testing.assert_close(getattr(ea, name), getattr(eb, name), rtol=1e-4, atol=1e-4, msg=name)
        # raw, not the normalised values: the newest frame of every stack is the env's state row
        normed = fused.obs_norm.apply(a.obs)
        assert float((a.obs - normed).abs().max()) > 0.1
        D0 = 17 * (frames - 1)
        torch.testing.assert_close(a.obs[T][:, D0:], ea.state.view(N, 17), rtol=0, atol=0)
        if boot:
            ws = fused._boot_ws
            used = ws.final_step >= 0
            s_u = ws.final_step.long()[used]
            e_u = torch.arange(N, device=cuda)[:, None].expand_as(used)[used]
            assert int(used.sum()) == int(a.truncated.sum())
            torch.testing.assert_close(ws.final_obs[used], per_step._final_obs[s_u, e_u], rtol=1e-4, atol=1e-4)
        for tr in trs:
            tr.storage.roll_over()
    # the tables matter: the same rollout without a normaliser acts differently
    plain = _trainer(frames, N, fused_rollout=True, norm_obs=False, bootstrap_on_timeout=boot)
    plain.env.max_episode_steps = 7
    plain.env.t.copy_(torch.arange(N, device=cuda) % 7)
    plain.collect()
    again = _trainer(frames, N, fused_rollout=True, bootstrap_on_timeout=boot)
    again.env.max_episode_steps = 7
    again.env.t.copy_(torch.arange(N, device=cuda) % 7)
    _set_tables(again.obs_norm, seed=frames)
    again.collect()
    torch.cuda.synchronize()
    assert not torch.allclose(plain.storage.actions, again.storage.actions, rtol=1e-4, atol=1e-4)


# ------------------------------------------------------------------------------------------------ 13. trainer
def _rows(log, D):
    return torch.cat([r.reshape(-1, D) for r in log["rows"]])


def test_trainer_graph_replay_equals_eager_and_state_matches_rollouts(cuda):
    kw = dict(num_envs=8, n_steps=16, ppo_epochs=1, ppo_minibatches=2, fused_rollout=True)
    tr = _trainer(1, cuda_graph=True, **kw)
    twin = _trainer(1, cuda_graph=False, **kw)
    log = spy(twin)
    ratios = []
    step = twin._mlp_step

    def step_(*a, **k):
        step(*a, **k)
        ratios.append(twin.stats["ratio"].clone())

    twin._mlp_step = step_
    for t in (tr, twin):
        t.mlp.policy_step = _no_per_step
    tr.capture(warmup=1)
    assert tr.graph is not None and tr.graph[0] == "single"
    twin.update_body()   # the capture's warm-up update
    p0 = tr.flat.data.clone()
    for _ in range(3):
        tr.step()
        twin.step()
    torch.cuda.synchronize()
    assert torch.equal(tr.flat.data, twin.flat.data)
    assert torch.equal(tr.obs_norm.state, twin.obs_norm.state)
    assert torch.equal(tr.obs_norm.tables, twin.obs_norm.tables)
    assert (tr.flat.data != p0).any() and torch.isfinite(tr.flat.data).all() and torch.isfinite(tr.stats_buf).all()
    assert len(log["rows"]) == 4 and float(tr.obs_norm.count[0]) == 4 * 8 * 16
    for k in range(4):
        assert torch.equal(log["at_collect"][k], log["at_merge"][k]), "tables frozen within update %d" % k
    check_state(tr.obs_norm, _rows(log, 17), "graph replay")
    # frozen tables: PPO's ratio is exactly 1 on the first minibatch of an update whose tables are not the identity
    assert len(ratios) == 8
    print("ratio, first minibatch of update 2:", float(ratios[4]))
    assert abs(float(ratios[4]) - 1.0) <= 1e-6
    assert abs(float(ratios[6]) - 1.0) <= 1e-6


@pytest.mark.parametrize("name,over", [("mujoco_ppo_dp8", dict(fused_rollout=False)),
                                       ("cartpole_cpu", dict())])
def test_trainer_per_step_and_a2c_configs(cuda, name, over):
    from actor_critic_algs_on_tensorflow_amd import preset
    from actor_critic_algs_on_tensorflow_amd.algos.trainer import ActorCriticTrainer
    kw = dict(num_envs=8, n_steps=16, device="cuda:0", outdir=None, quiet=True, stdout_freq=0, save_every=0,
              cuda_graph=False, norm_obs=True, **over)
    if name == "mujoco_ppo_dp8":
        kw.update(ppo_epochs=1, ppo_minibatches=2)
    tr = ActorCriticTrainer(preset(name, **kw))
    assert tr.mlp is not None and tr.mlp.obs_norm is tr.obs_norm
    log = spy(tr)
    p0 = tr.flat.data.clone()
    for _ in range(2):
        tr.step()
    torch.cuda.synchronize()
    assert torch.isfinite(tr.flat.data).all() and (tr.flat.data != p0).any()
    assert torch.equal(log["at_collect"][1], log["at_merge"][1])
    assert not torch.equal(log["at_collect"][0], log["at_collect"][1])
    check_state(tr.obs_norm, _rows(log, tr.obs_norm.D), name)
