"""Running reward scaling on the GPU: ``reward_norm_scan`` / ``reward_norm_apply`` (``reward_norm.hip``) against the torch
forms of ``ops/reward_norm.py`` (bit-equal), the ``D = 1`` ``obs_norm_merge`` launch behind them (batch vector within
the bound of a reordered sum, merged state within the tolerances ``tests/test_gpu_obs_norm.py`` uses for that launch),
launcher validation, and the native MLP trainer with ``norm_reward=True`` (graph replay == eager, state == the oracle
replayed over the recorded raw rewards). Bars: ``tests/test_reward_norm_cpu.py``."""
import numpy as np
import pytest
import torch

from test_reward_norm_cpu import GAMMA, U52, _case, _primed, replay, spy

pytestmark = pytest.mark.gpu

T_KINDS = ("1", "U-1", "U", "U+1", "2U+1")


def _T(kind):
    from actor_critic_algs_on_tensorflow_amd.ops.reward_norm import scan_unroll
    U = scan_unroll()
    assert U >= 8, "RWN_UNROLL, the steps per load round, is at least 8"
    return {"1": 1, "U-1": U - 1, "U": U, "U+1": U + 1, "2U+1": 2 * U + 1}[kind]


# ------------------------------------------------------------------------------------------------ 12. kernels
@pytest.mark.parametrize("N", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("kind", T_KINDS)
def test_scan_merge_apply_match_fallbacks(cuda, N, kind):
    from actor_critic_algs_on_tensorflow_amd import _native
    ops = _native.require()
    T = _T(kind)
    r, d = _case(T, N, seed=T * 1000 + N)
    ref, dev = _primed(N, clip=0.8), _primed(N, cuda, clip=0.8)
    assert torch.equal(dev.state.cpu(), ref.state) and float(ref.count[0]) > 0 and ref.ret.any()
    r_g, d_g = r.to(cuda), d.to(cuda)
    ref.scan_torch(r, d)
    dev.part.fill_(float("nan"))
    dev.scan(r_g, d_g)
    torch.cuda.synchronize()
    assert torch.equal(r_g.cpu(), r), "the scan does not modify the rewards"
    assert torch.equal(dev.ret.cpu(), ref.ret), "ret bit-equal"
    assert torch.equal(dev.part.cpu(), ref.part), "per-env partial rows bit-equal"
    assert dev.stats._pending == (N, float(T * N))
    # stage 0 of the D = 1 merge: the N rows summed in a fixed order
    dev.batch.fill_(float("nan"))
    ops.obs_norm_merge(dev.part.view(-1), N, dev.batch, float(T * N), dev.state, dev.tables, 0, dev.eps)
    torch.cuda.synchronize()
    want = ref.batch_from_parts(T)
    bound = N * U52 * ref.part.abs().sum(0)
    err = (dev.batch.cpu()[:2] - want[:2]).abs()
    print("batch err", err.tolist(), "bound", bound.tolist())
    assert bool((err <= bound).all()) and float(dev.batch[2]) == T * N
    assert torch.equal(dev.state.cpu(), ref.state), "stage 0 leaves the state alone"
    # the whole merge (one launch) against the torch form
    dev.merge()
    ref.batch.copy_(want)
    ref.stats.merge_batch_()
    torch.cuda.synchronize()
    np.testing.assert_allclose(dev.state.cpu().numpy(), ref.state.numpy(), rtol=1e-10, atol=1e-12)
    for got, exp in ((dev.mean32.cpu().numpy(), ref.mean32.numpy()), (dev.istd32.cpu().numpy(), ref.istd32.numpy())):
        ulp = np.spacing(np.maximum(np.abs(got), np.abs(exp)).astype(np.float32))
        assert np.all(np.abs(got.astype(np.float64) - exp.astype(np.float64)) <= 2.0 * ulp), (got, exp)
    # apply with the device's tables: bit-equal
    ref.tables.copy_(dev.tables.cpu())
    dev.apply_(r_g)
    want_r = ref.apply_(r.clone())
    torch.cuda.synchronize()
    assert torch.equal(r_g.cpu(), want_r)
    if T * N >= 8:
        assert (want_r.abs() == 0.8).any() and (want_r.abs() < 0.8).any()


@pytest.mark.parametrize("T,N,off", [(7, 3, 0), (5, 130, 0), (16, 64, 0), (1, 1, 0), (9, 65, 1), (3, 1, 2)])
def test_apply_vector_body_scalar_tail_and_unaligned_base(cuda, T, N, off):
    """21, 650 and 585 elements are no multiple of 4 (the tail is taken), 1024 is (no tail), 1 and 3 are below one
    vector; a base 4 or 8 bytes past a 16-byte boundary takes the element-wise instantiation."""
    from actor_critic_algs_on_tensorflow_amd.ops.reward_norm import RewardNormalizer
    g = torch.Generator().manual_seed(T * N + off)
    x = torch.randn(T * N, generator=g) * 3.0
    norm = RewardNormalizer(N, GAMMA, clip=1.25, device=cuda)
    norm.istd32.fill_(0.37)
    buf = torch.full((T * N + off + 8,), float("nan"), device=cuda)
    view = buf[off:off + T * N].view(T, N)
    view.copy_(x.view(T, N))
    assert view.is_contiguous() and (view.data_ptr() % 16 == 0) == (off == 0)
    norm.apply_(view)
    torch.cuda.synchronize()
    want = x.view(T, N).clone().mul_(torch.tensor(0.37)).clamp_(-1.25, 1.25)
    assert torch.equal(view.cpu(), want)
    assert torch.isnan(buf[:off]).all() and torch.isnan(buf[off + T * N:]).all(), "nothing written outside"


# ------------------------------------------------------------------------------------------------ 13. validation
def test_launchers_refuse_bad_operands(cuda):
    from actor_critic_algs_on_tensorflow_amd import _native
    ops = _native.require()
    T, N = 6, 5
    norm = _primed(N, cuda)
    r, d = (x.to(cuda) for x in _case(T, N))
    ret0 = norm.ret.clone()
    norm.part.fill_(-7.0)
    scan = lambda r_, d_, ret_=norm.ret: ops.reward_norm_scan(r_, d_, ret_, norm.state, norm.part.view(-1), GAMMA)
    bad = {"fp16 rewards": lambda: scan(r.half(), d),
           "int32 dones": lambda: scan(r, d.int()),
           "transposed rewards": lambda: scan(r.t().contiguous().t(), d),
           "transposed dones": lambda: scan(r, d.t().contiguous().t()),
           "ret of the wrong length": lambda: scan(r, d, torch.zeros(N + 1, dtype=torch.float64, device=cuda)),
           "fp32 ret": lambda: scan(r, d, torch.zeros(N, device=cuda)),
           "cpu rewards": lambda: scan(r.cpu(), d),
           "apply: fp16": lambda: ops.reward_norm_apply(r.half(), norm.tables.view(-1), 10.0),
           "apply: transposed": lambda: ops.reward_norm_apply(r.t().contiguous().t(), norm.tables.view(-1), 10.0),
           "apply: clip 0": lambda: ops.reward_norm_apply(r.clone(), norm.tables.view(-1), 0.0)}
    assert r.t().contiguous().t().shape == r.shape and not r.t().contiguous().t().is_contiguous()
    for what, call in bad.items():
        with pytest.raises((RuntimeError, NotImplementedError)):
            call()
            pytest.fail(what + " was accepted")
    torch.cuda.synchronize()
    assert torch.equal(norm.ret, ret0) and bool((norm.part == -7.0).all()), "nothing was launched"
    scan(r, d)   # the same operands, well-formed, launch
    torch.cuda.synchronize()
    assert not torch.equal(norm.ret, ret0) and not bool((norm.part == -7.0).any())


@pytest.mark.parametrize("T,N", [(6, 1), (1, 5)])
def test_stride_of_a_size_one_dimension_is_ignored(cuda, T, N):
    """A ``[T, 1]`` or ``[1, N]`` view is contiguous whatever stride its size-1 dimension carries."""
    r, d = (x.to(cuda) for x in _case(T, N))
    odd = (1, 7) if N == 1 else (99, 1)
    r2, d2 = r.as_strided((T, N), odd), d.as_strided((T, N), odd)
    assert r2.is_contiguous() and r2.stride() == odd and torch.equal(r2, r)
    a, b = _primed(N, cuda), _primed(N, cuda)
    a.scan(r, d)
    b.scan(r2, d2)
    torch.cuda.synchronize()
    assert torch.equal(a.ret, b.ret) and torch.equal(a.part, b.part) and not torch.equal(a.ret, _primed(N, cuda).ret)


# ------------------------------------------------------------------------------------------------ 14. / 15. trainer
def _make(name, cuda_graph, **over):
    from actor_critic_algs_on_tensorflow_amd import preset
    from actor_critic_algs_on_tensorflow_amd.algos.trainer import ActorCriticTrainer
    kw = dict(device="cuda:0", outdir=None, quiet=True, stdout_freq=0, save_every=0, cuda_graph=cuda_graph,
              norm_reward=True)
    kw.update(over)
    tr = ActorCriticTrainer(preset(name, **kw))
    assert tr.mlp is not None and (tr.reward_norm is not None) == kw["norm_reward"]
    return tr


def _replay_equals_eager(make, boot):
    """3 captured replays == 3 eager updates (after the capture's warm-up update), bit for bit; the eager twin's state
    == the torch oracle replayed over its recorded raw rewards. -> (twin, its log)"""
    tr, twin = make(True), make(False)
    log = spy(twin)
    tr.capture(warmup=1)
    assert tr.graph is not None and tr.graph[0] == "single"
    twin.update_body()   # the capture's warm-up update
    p0 = tr.flat.data.clone()
    for _ in range(3):
        tr.step()
        twin.step()
    torch.cuda.synchronize()
    assert torch.equal(tr.flat.data, twin.flat.data)
    assert torch.equal(tr.reward_norm.ret, twin.reward_norm.ret)
    assert torch.equal(tr.reward_norm.state, twin.reward_norm.state)
    assert torch.equal(tr.reward_norm.tables, twin.reward_norm.tables)
    assert (tr.flat.data != p0).any() and torch.isfinite(tr.flat.data).all() and torch.isfinite(tr.stats_buf).all()
    st = twin.storage
    assert len(log["raw"]) == 4 and float(tr.reward_norm.count[0]) == 4 * st.T * st.N
    clip = twin.cfg.reward_clip
    _, ref = replay(log, st.N, twin.cfg.gamma, clip)   # on the CPU
    assert torch.equal(twin.reward_norm.ret.cpu(), ref.ret), "ret depends on the raw rewards alone: bit-equal"
    np.testing.assert_allclose(twin.reward_norm.state.cpu().numpy(), ref.state.numpy(), rtol=1e-10, atol=1e-12)
    for k in range(4):
        raw, scaled, tab = log["raw"][k], log["scaled"][k], log["tables"][k]
        assert torch.equal(scaled, (raw * tab.view(-1)[1]).clamp(-clip, clip)), "scaled with the merged istd32"
        assert not torch.equal(scaled, raw), "the rewards were scaled"
        if not boot:
            assert torch.equal(log["at_returns"][k], scaled)
    return twin, log


@pytest.mark.parametrize("boot", [False, True])
def test_native_mlp_trainer_fused_rollout(cuda, boot):
    def make(graph):
        tr = _make("mujoco_ppo_dp8", graph, num_envs=8, n_steps=12, ppo_epochs=1, ppo_minibatches=2,
                   fused_rollout=True, bootstrap_on_timeout=boot)
        assert tr.mlp.supports_fused_rollout(tr.env)
        tr.env.max_episode_steps = 5

        def no_per_step(*a, **k):
            raise AssertionError("norm_reward left the one-launch rollout: policy_step was called")

        tr.mlp.policy_step = no_per_step
        return tr

    twin, log = _replay_equals_eager(make, boot)
    assert all(int(d.sum()) >= 2 * 8 for d in log["dones"]), "episode boundaries occur in every rollout"
    if boot:
        # the scan saw raw env rewards; gamma V(terminal observation) is added, unscaled, after the scaling, at the
        # truncated steps and nowhere else
        for k in range(4):
            cut = log["dones"][k].bool()   # (this bank never terminates: every done is a time-limit cut)
            got, scaled = log["at_returns"][k], log["scaled"][k]
            assert torch.equal(got[~cut], scaled[~cut])
            assert bool((got[cut] != scaled[cut]).any())
        plain = _make("mujoco_ppo_dp8", False, num_envs=8, n_steps=12, ppo_epochs=1, ppo_minibatches=2,
                      fused_rollout=True, norm_reward=False)
        assert plain.reward_norm is None
        plain.env.max_episode_steps = 5
        plain.collect()
        torch.cuda.synchronize()
        torch.testing.assert_close(log["raw"][0], plain.storage.rewards, rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("algo", ["ppo", "a2c"])
def test_native_mlp_trainer_per_step_path(cuda, algo):
    def make(graph):
        tr = _make("pendulum_ppo", graph, num_envs=4, n_steps=6, ppo_epochs=1, ppo_minibatches=2, algo=algo)
        assert not (tr.cfg.fused_rollout and tr.mlp.supports_fused_rollout(tr.env)) and tr.cfg.algo == algo
        return tr

    _replay_equals_eager(make, False)
