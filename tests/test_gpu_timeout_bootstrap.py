"""Time-limit bootstrap inside the one-launch MuJoCo rollout (``mlp_rollout_kernel``'s BOOT instantiation keeps the
terminal observation of every truncated step in ``ceil(T / max_steps)`` slots per env; ``timeout_bootstrap_kernel``
adds ``gamma * V(terminal observation)`` to those steps' rewards), against the per-step native path
(``policy_step`` + ``env_step_linear`` launches, terminal stacks as a ``[T, N, D]`` slab)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

T = 24


def _trainer(frames=1, num_envs=5, **over):
    from actor_critic_algs_on_tensorflow_amd import preset
    from actor_critic_algs_on_tensorflow_amd.algos.trainer import ActorCriticTrainer
    kw = dict(num_envs=num_envs, n_steps=T, frames=frames, ppo_epochs=1, ppo_minibatches=2, device="cuda:0",
              outdir=None, quiet=True, stdout_freq=0, save_every=0, cuda_graph=False, bootstrap_on_timeout=True)
    kw.update(over)
    tr = ActorCriticTrainer(preset("mujoco_ppo_dp8", **kw))
    assert tr.mlp is not None and tr.mlp.supports_fused_rollout(tr.env)
    return tr


def _no_per_step(*a, **k):
    raise AssertionError("bootstrap_on_timeout left the one-launch rollout: policy_step was called")


@pytest.mark.parametrize("frames,num_envs", [(1, 5), (3, 9)])
def test_fused_bootstrap_rollout_matches_per_step_launches(cuda, frames, num_envs):
    """Episode limit 7 and staggered episode clocks (t0 = env % 7): the envs of one 4-env tile are cut at different
    steps and fill 3 or 4 of their S = ceil(24 / 7) = 4 slots. Flags and counters exactly, everything the actor's
    fp32 summation order touches (4x4x1 tiles vs 16x16x4) to 1e-4, the project's bar for fused against per-step --
    the rewards include gamma * V(terminal observation) on both sides."""
    N = num_envs
    trs = [_trainer(frames, N, fused_rollout=f) for f in (True, False)]
    for tr in trs:
        tr.env.max_episode_steps = 7
        tr.env.t.copy_(torch.arange(N, device=cuda) % 7)
    fused, per_step = trs
    fused.mlp.policy_step = _no_per_step
    for it in range(3):   # later rollouts start from the written-back env bank; the third has envs at t0 >= 4
        t0 = fused.env.t.clone()
        for tr in trs:
            tr.collect()
        torch.cuda.synchronize()
        a, b = fused.storage, per_step.storage
        for name in ("dones", "truncated"):
            assert torch.equal(getattr(a, name), getattr(b, name)), name
        for name in ("obs", "actions", "logp", "entropy", "rewards", "values"):
            torch.testing.assert_close(getattr(a, name), getattr(b, name), rtol=1e-4, atol=1e-4, msg=name)
        ea, eb = fused.env, per_step.env
        for name in ("t", "tg"):
            assert torch.equal(getattr(ea, name), getattr(eb, name)), name
        for name in ("state", "ep_ret"):
            torch.testing.assert_close(getattr(ea, name), getattr(eb, name), rtol=1e-4, atol=1e-4, msg=name)
        # the slot table: every used slot names a truncated step of its env, every truncated step has its slot, and
        # the slot holds the per-step path's terminal stack of that step
        ws = fused._boot_ws
        assert ws.S == 4 and ws.final_step.shape == (N, 4) and ws.final_obs.shape == (N, 4, 17 * frames)
        step = ws.final_step.long()
        used = step >= 0
        assert ((step == -1) | used).all() and (step < T).all()
        env = torch.arange(N, device=cuda)[:, None].expand_as(step)
        s_u, e_u = step[used], env[used]
        assert a.truncated[s_u, e_u].all()
        assert int(used.sum()) == int(a.truncated.sum())
        assert torch.unique(s_u * N + e_u).numel() == s_u.numel()
        torch.testing.assert_close(ws.final_obs[used], per_step._final_obs[s_u, e_u], rtol=1e-4, atol=1e-4)
        # slots are filled in step order, unused ones trail; the counts follow the envs' episode clocks
        want = (t0.long() + T) // 7
        assert torch.equal(used.sum(1), want)
        for s in range(1, 4):
            assert (~used[:, s] | (used[:, s - 1] & (step[:, s] > step[:, s - 1]))).all()
        if it == 0:
            assert int((~used).sum()) > 0      # envs that started at t0 <= 3 leave a slot at -1
        assert int(used.sum(1).max()) == 4     # and some env uses all S slots
        for tr in trs:
            tr.storage.roll_over()
    assert int(fused.env.t.max()) < 7


def test_unused_slots_are_never_consumed(cuda):
    """No truncation inside the rollout (limit 1000): the launch writes -1 into every slot of a table pre-filled with
    'step 0', the NaN terminal stacks (and their NaN values) are never read, and the rewards are bitwise those of
    the same trainer without bootstrapping."""
    tr = _trainer(1, 5, fused_rollout=True)
    twin = _trainer(1, 5, fused_rollout=True, bootstrap_on_timeout=False)
    tr.mlp.policy_step = _no_per_step
    assert tr.env.max_episode_steps == 1000
    ws = tr._timeout_boot_ws()
    assert ws.S == 1
    ws.final_obs.fill_(float("nan"))
    ws.final_step.zero_()
    tr.collect()
    twin.collect()
    torch.cuda.synchronize()
    assert tr._boot_ws is ws
    assert (ws.final_step == -1).all()
    assert int(tr.storage.truncated.sum()) == 0
    assert torch.isnan(ws.final_obs).all()
    assert torch.equal(tr.storage.rewards, twin.storage.rewards)
    assert torch.equal(tr.storage.values, twin.storage.values)
    assert getattr(twin, "_boot_ws", None) is None


def test_timeout_bootstrap_kernel_matches_fallback(cuda):
    """T = 5, N = 3, S = 2 with used and unused slots (the unused ones hold NaN values): the HIP kernel against the
    torch fallback, both fp32 multiply-then-add."""
    from actor_critic_algs_on_tensorflow_amd.ops.returns import timeout_bootstrap_, timeout_bootstrap_ref_
    g = torch.Generator().manual_seed(11)
    rewards = torch.randn(5, 3, generator=g)
    v = torch.randn(3, 2, generator=g) * 7
    final_step = torch.tensor([[1, 4], [-1, -1], [3, -1]], dtype=torch.int32)
    v[final_step < 0] = float("nan")
    want = timeout_bootstrap_ref_(rewards.clone(), final_step, v, 0.97)
    got = timeout_bootstrap_(rewards.to(cuda), final_step.to(cuda), v.to(cuda), 0.97)
    torch.cuda.synchronize()
    assert torch.isfinite(got).all()
    torch.testing.assert_close(got.cpu(), want, rtol=1e-6, atol=0)
    changed = (got.cpu() != rewards)
    assert changed.sum() == 3 and changed[1, 0] and changed[4, 0] and changed[3, 2]
    # the GPU fallback path (the oracle on device tensors) agrees too
    torch.testing.assert_close(timeout_bootstrap_ref_(rewards.to(cuda), final_step.to(cuda), v.to(cuda), 0.97).cpu(),
                               want, rtol=1e-6, atol=0)


def test_rollout_launcher_rejects_too_few_slots(cuda):
    """Host-side validation only: final_obs sized for S = 1 while T = 24 and max_steps = 7 need 4 slots. The op
    raises before anything is launched: no buffer of the rollout or the env bank changes."""
    from actor_critic_algs_on_tensorflow_amd import _native
    from actor_critic_algs_on_tensorflow_amd.algos.trainer import KEY_ENV_BITS
    tr = _trainer(1, 5, fused_rollout=True)
    env, st, eng = tr.env, tr.storage, tr.mlp
    N, D = env.num_envs, eng.D
    desc, _ = eng.desc(None)
    st.rewards.fill_(-7.0)
    st.obs[1:].fill_(-7.0)
    before = {n: getattr(env, n).clone() for n in ("state", "t", "tg", "ep_ret")}

    def launch(max_steps, final_obs, final_step):
        _native.require().mlp_rollout(desc, eng.rollout_lds_bytes(True), st.obs, st.actions, st.logp, st.entropy,
                                      st.rewards, st.dones, st.truncated, eng.log_std, eng.ac_scale, KEY_ENV_BITS,
                                      tr.policy_seed, env.state, env.t, env.tg, env.ep_ret, env.ep_stats,
                                      env.env_ids, env.A, env.B, env.seed, max_steps, env.frame_stack, True, None,
                                      final_obs, final_step)

    fo = torch.zeros(N, 1, D, device=cuda)
    fs = torch.zeros(N, 1, dtype=torch.int32, device=cuda)
    with pytest.raises(RuntimeError, match="mlp_rollout"):
        launch(7, fo, fs)                                             # S = 1 < ceil(24 / 7)
    with pytest.raises(RuntimeError, match="go together"):
        launch(1000, fo, None)                                        # slots without their step table
    with pytest.raises(RuntimeError, match="final_step"):
        launch(1000, fo, torch.zeros(N, 2, dtype=torch.int32, device=cuda))
    with pytest.raises(RuntimeError, match="final_obs"):
        launch(1000, torch.zeros(N + 1, 1, D, device=cuda), torch.zeros(N + 1, 1, dtype=torch.int32, device=cuda))
    torch.cuda.synchronize()
    assert (st.rewards == -7.0).all() and (st.obs[1:] == -7.0).all() and (fs == 0).all()
    for n, v in before.items():
        assert torch.equal(getattr(env, n), v), n


def test_bootstrap_rollout_graph_capture_equals_eager(cuda):
    """The fused bootstrap rollout (rollout launch, two critic launches, fix-up launch) is part of the ONE captured
    update graph -- the slot table needs no host-side clear between replays -- and replays bit-for-bit what the
    eager update computes."""
    kw = dict(num_envs=16, n_steps=32, ppo_epochs=2, ppo_minibatches=4, fused_rollout=True)
    tr = _trainer(1, cuda_graph=True, **kw)
    twin = _trainer(1, cuda_graph=False, **kw)
    for t in (tr, twin):
        t.env.max_episode_steps = 7
        t.mlp.policy_step = _no_per_step
    tr.capture(warmup=1)
    assert tr.graph is not None and tr.graph[0] == "single"
    twin.update_body()   # the capture's warm-up update
    p0 = tr.flat.data.clone()
    for _ in range(3):
        tr.step()
        twin.step()
    torch.cuda.synchronize()
    assert tr._boot_ws.S == 5 and int((tr._boot_ws.final_step >= 0).sum()) > 0
    assert torch.equal(tr.flat.data, twin.flat.data)
    assert (tr.flat.data != p0).any() and torch.isfinite(tr.flat.data).all()
    assert torch.isfinite(tr.stats_buf).all()
