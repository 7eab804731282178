"""Rolling episode window on the GPU: ``ep_monitor_scan`` / ``ep_monitor_commit`` (``ep_monitor.hip``) against the
independent oracle of ``tests/oracles/ep_monitor_oracle.py`` (state arrays, counts, minimum and maximum exact; means and
standard deviation within the derived bar of ``tests/test_ep_monitor_cpu.py``), run-to-run bit equality, the binding's
refusals, and the native MLP and CNN trainers with ``ep_window=100`` (state == the torch form fed the stored rewards /
dones update by update, carry == the bank's own accumulators, ring == the drained episode statistics, graph replay ==
eager, and nothing the trainer reads changes)."""
import numpy as np
import pytest
import torch

from test_ep_monitor_cpu import KS, EpMonitorOracle, _rewards, assert_matches_oracle, sequence, spy_monitor

pytestmark = pytest.mark.gpu

STATE = ("cur_ret", "cur_len", "ring_ret", "ring_len", "total")


def _shape(kind):
    from actor_critic_algs_on_tensorflow_amd.ops.ep_monitor import scan_unroll
    U = scan_unroll()
    assert U >= 8, "EPM_UNROLL, the steps per load round, is at least 8"
    return {"5x32": (5, 32), "U-1": (U - 1, 70), "U": (U, 64), "2U+5": (2 * U + 5, 70), "16x300": (16, 300)}[kind]


def _monitor(N, K, cuda):
    from actor_critic_algs_on_tensorflow_amd.ops.ep_monitor import EpisodeMonitor
    return EpisodeMonitor(N, K, cuda)


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("kind", ["5x32", "U-1", "U", "2U+5", "16x300"])
def test_kernels_equal_the_oracle(cuda, kind, K):
    """Every planted case of the CPU test (no done; corners; a step where every env is done; C = K, 0 < C < K,
    C > 2K; random), consecutively on one monitor; then the same inputs again on a fresh one: bit-identical."""
    T, N = _shape(kind)
    seq = sequence(T, N, K)
    assert any(C == K for _, _, C in seq) and seq[0][2] == 0
    assert any(C > 2 * K for _, _, C in seq) or T * N < 2 * K + 3, "every shape that can hold them wraps twice"
    ref = EpMonitorOracle(N, K)
    a, b = _monitor(N, K, cuda), _monitor(N, K, cuda)
    for u, (r, d, C) in enumerate(seq):
        r_g, d_g = r.to(cuda), d.to(cuda)
        a.update(r_g, d_g)
        b.update(r_g.clone(), d_g.clone())
        torch.cuda.synchronize()
        assert torch.equal(r_g.cpu(), r) and torch.equal(d_g.cpu(), d), "the inputs are not modified"
        ref.update(r.numpy(), d.numpy())
        assert_matches_oracle(a, ref, (kind, K, u))
        for k in STATE + ("summary",):
            assert torch.equal(getattr(a, k), getattr(b, k)), (kind, K, u, k)


@pytest.mark.parametrize("K", KS)
def test_kernels_equal_the_oracle_at_128_x_4096(cuda, K):
    """T N = 524 288 at a done density of 1/200: three consecutive calls (every one finishes more than 2K episodes)."""
    T, N = 128, 4096
    g = torch.Generator().manual_seed(K)
    ref, mon, twin = EpMonitorOracle(N, K), _monitor(N, K, cuda), _monitor(N, K, cuda)
    for u in range(3):
        r = _rewards(T, N, g)
        d = (torch.rand(T, N, generator=g) < 1.0 / 200).to(torch.uint8)
        r_g, d_g = r.to(cuda), d.to(cuda)
        mon.update(r_g, d_g)
        twin.update(r_g, d_g)
        torch.cuda.synchronize()
        ref.update(r.numpy(), d.numpy(), rows=True)
        assert ref.summary["new"] > 2 * K
        assert_matches_oracle(mon, ref, (K, u))
        for k in STATE + ("summary",):
            assert torch.equal(getattr(mon, k), getattr(twin, k)), (K, u, k)


def test_equal_window_has_zero_std_and_exact_mean(cuda):
    mon = _monitor(70, 100, cuda)
    r = torch.full((6, 70), 0.1, dtype=torch.float32, device=cuda)
    d = torch.zeros(6, 70, dtype=torch.uint8, device=cuda)
    d[2] = d[5] = 1
    mon.update(r, d)
    res = mon.result()
    x = np.float32(np.float32(np.float32(0.1) + np.float32(0.1)) + np.float32(0.1))
    assert res["filled"] == 100 and res["total"] == 140 and res["ret_std"] == 0.0 and res["ret_mean"] == float(x)
    assert res["ret_min"] == res["ret_max"] == float(x) and res["len_mean"] == 3.0 and res["new_len_mean"] == 3.0


def test_binding_refuses_bad_operands(cuda):
    from actor_critic_algs_on_tensorflow_amd import _native
    ops = _native.require()
    T, N, K = 6, 5, 4
    mon = _monitor(N, K, cuda).reserve(T)
    r, d, _ = sequence(T, N, K)[-1]
    r, d = r.to(cuda), d.to(cuda)
    mon.cur_ret.fill_(-7.0)

    def call(r_=r, d_=d, cur_ret=mon.cur_ret, cur_len=mon.cur_len, ring_ret=mon.ring_ret, ring_len=mon.ring_len,
             total=mon.total, summary=mon.summary, ep_ret=mon._ep_ret, ep_len=mon._ep_len):
        ops.ep_monitor_update(r_, d_, cur_ret, cur_len, ring_ret, ring_len, total, summary, ep_ret, ep_len)

    i32 = lambda n: torch.zeros(n, dtype=torch.int32, device=cuda)
    f32 = lambda n: torch.zeros(n, device=cuda)
    max_cells = int(ops.ep_monitor_max_cells())
    assert max_cells >= 128 * 4096
    bad = {"fp16 rewards": lambda: call(r_=r.half()),
           "int32 dones": lambda: call(d_=d.int()),
           "1-d rewards": lambda: call(r_=r.view(-1), d_=d.view(-1)),
           "dones of another shape": lambda: call(d_=d[:T - 1]),
           "transposed rewards": lambda: call(r_=r.t().contiguous().t()),
           "transposed dones": lambda: call(d_=d.t().contiguous().t()),
           "cur_ret of the wrong length": lambda: call(cur_ret=f32(N + 1)),
           "fp64 cur_ret": lambda: call(cur_ret=torch.zeros(N, dtype=torch.float64, device=cuda)),
           "int64 cur_len": lambda: call(cur_len=torch.zeros(N, dtype=torch.int64, device=cuda)),
           "K = 0": lambda: call(ring_ret=f32(0), ring_len=i32(0)),
           "K = 4097": lambda: call(ring_ret=f32(4097), ring_len=i32(4097)),
           "ring_len of another K": lambda: call(ring_len=i32(K + 1)),
           "int32 total": lambda: call(total=i32(1)),
           "short summary": lambda: call(summary=torch.zeros(9, dtype=torch.float64, device=cuda)),
           "short scratch": lambda: call(ep_ret=f32(T * N - 1)),
           "unaligned dones": lambda: call(d_=torch.zeros(T * N + 16, dtype=torch.uint8, device=cuda)[1:T * N + 1]
                                           .view(T, N)),
           "more cells than one workgroup takes": lambda: call(
               r_=torch.zeros(max_cells // 4 + 1, 4, device=cuda),
               d_=torch.zeros(max_cells // 4 + 1, 4, dtype=torch.uint8, device=cuda),
               cur_ret=f32(4), cur_len=i32(4)),
           "cpu rewards": lambda: call(r_=r.cpu()),
           "cpu state": lambda: call(cur_ret=mon.cur_ret.cpu())}
    for what, fn in bad.items():
        with pytest.raises((RuntimeError, NotImplementedError)):
            fn()
            pytest.fail(what + " was accepted")
    torch.cuda.synchronize()
    assert bool((mon.cur_ret == -7.0).all()) and int(mon.total[0]) == 0, "nothing was launched"
    call()   # the same operands, well-formed, launch
    torch.cuda.synchronize()
    assert not bool((mon.cur_ret == -7.0).any()) and int(mon.total[0]) == int(d.sum())
    from actor_critic_algs_on_tensorflow_amd.ops.ep_monitor import EpisodeMonitor
    for K_bad in (0, 4097):
        with pytest.raises(ValueError, match="window K"):
            EpisodeMonitor(N, K_bad, cuda)


# ------------------------------------------------------------------------------------------------ trainers
ENGINES = {
    "cartpole_per_step": ("cartpole_cpu", dict(num_envs=70, n_steps=5), None),
    "mujoco_fused": ("mujoco_ppo_dp8", dict(num_envs=8, n_steps=12, ppo_epochs=1, ppo_minibatches=2,
                                            fused_rollout=True), 5),
    "mujoco_fused_norm_boot": ("mujoco_ppo_dp8", dict(num_envs=8, n_steps=12, ppo_epochs=1, ppo_minibatches=2,
                                                      fused_rollout=True, norm_reward=True,
                                                      bootstrap_on_timeout=True), 5),
    "pong_fused_steps": ("pong_a2c", dict(num_envs=32, n_steps=5, seed=5), 7),
    "breakout_ppo": ("breakout_ppo", dict(num_envs=16, n_steps=16, ppo_epochs=1, ppo_minibatches=2, seed=9), 14),
}


def _make(which, cuda_graph, ep_window):
    from actor_critic_algs_on_tensorflow_amd import preset
    from actor_critic_algs_on_tensorflow_amd.algos.trainer import ActorCriticTrainer
    name, kw, limit = ENGINES[which]
    tr = ActorCriticTrainer(preset(name, device="cuda:0", outdir=None, quiet=True, stdout_freq=0, save_every=0,
                                   cuda_graph=cuda_graph, ep_window=ep_window, **kw))
    assert (tr.mlp is not None) != (tr.engine is not None), "a native engine"
    assert (tr.ep_monitor is not None) == bool(ep_window)
    if which.startswith("mujoco"):
        assert tr.mlp.supports_fused_rollout(tr.env)
    if which == "pong_fused_steps":
        assert tr.engine.fused_step_ok(tr.env.num_envs) and tr.storage.ring
    if limit is not None:
        tr.env.max_episode_steps = limit
    return tr


def _snapshot(tr):
    st = tr.storage
    out = [tr.flat.data, st.rewards, st.dones, st.values, st.logp, st.actions, tr.env.ep_ret, tr.env.t,
           tr.update_counter]
    for opt in tr.opts.values():
        out += [torch.as_tensor(v) for _, v in sorted(opt.state_dict().items())]
    if tr.reward_norm is not None:
        out += [tr.reward_norm.state, tr.reward_norm.ret, tr.reward_norm.tables]
    return [x.detach().clone() for x in out]


@pytest.mark.parametrize("which", list(ENGINES))
def test_native_trainers(cuda, which, monkeypatch):
    """Captured replays (ep_window=100) == eager updates (ep_window=100) == eager updates (ep_window=0) in everything
    the trainer reads; the window == the torch form over the eager twin's recorded rewards / dones, update by update;
    its carry == the bank's accumulators; its ring == the bank's drained episode statistics."""
    monkeypatch.setattr("actor_critic_algs_on_tensorflow_amd.ops.gemm.TUNE", False)
    from actor_critic_algs_on_tensorflow_amd.ops.ep_monitor import EpisodeMonitor
    graph, eager, off = _make(which, True, 100), _make(which, False, 100), _make(which, False, 0)
    log = spy_monitor(eager)
    graph.capture(warmup=1)
    assert graph.graph is not None and graph.graph[0] == "single"
    eager.update_body()   # the capture's warm-up update
    off.update_body()
    ref = EpisodeMonitor(eager.storage.N, 100)
    ref.update(log["raw"][0].cpu(), log["dones"][0].cpu())
    for u in range(4):
        for tr in (graph, eager, off):
            tr.step()
        torch.cuda.synchronize()
        ref.update(log["raw"][u + 1].cpu(), log["dones"][u + 1].cpu())
        for k in STATE:
            assert torch.equal(getattr(eager.ep_monitor, k).cpu(), getattr(ref, k)), (u, k)
            assert torch.equal(getattr(graph.ep_monitor, k), getattr(eager.ep_monitor, k)), (u, k)
        assert torch.equal(graph.ep_monitor.summary, eager.ep_monitor.summary), u
        got, want = eager.ep_monitor.summary.cpu(), ref.summary
        assert torch.equal(got[[0, 1, 4, 5, 7]], want[[0, 1, 4, 5, 7]]), (got, want)
        big = max(1.0, float(ref.ring_ret.abs().max()))
        assert float((got - want).abs().max()) <= 1e-12 * big * max(1.0, float(want[[6, 9]].max())), (got, want)
    assert len(log["raw"]) == 5 and int(ref.total[0]) > 0, "episodes ended within these updates"
    for i, (a, b, c) in enumerate(zip(_snapshot(graph), _snapshot(eager), _snapshot(off))):
        assert torch.equal(a, b) and torch.equal(b, c), i
    if eager.reward_norm is not None:
        assert not torch.equal(log["raw"][-1], eager.storage.rewards), "the trainer learns from scaled rewards"
    # the carry is the bank's own accumulator (a plain fp32 add of the stored reward in step order)
    mon = eager.ep_monitor
    assert torch.equal(mon.cur_ret, eager.env.ep_ret.view(-1))
    assert torch.equal(mon.cur_len.to(torch.int64), eager.env.t.view(-1).to(torch.int64))
    # K holds every episode of the run: the ring against the bank's per-wave float-atomic statistics
    mean, n, ln = eager.env.drain_episode_stats()
    res = mon.result()
    assert n == res["total"] == res["filled"] <= 100
    ring_sum, drained = float(res["returns"].astype(np.float64).sum()), mean * n
    abs_sum = float(np.abs(res["returns"].astype(np.float64)).sum())
    print(which, "episodes", n, "ring sum", ring_sum, "drained sum", drained, "diff", abs(ring_sum - drained))
    # bar: 8 x the difference the drained fp32 atomic sum shows between two identical runs (profiles/ep_monitor.txt)
    assert abs(ring_sum - drained) <= DRAIN_BAR_REL * max(abs_sum, 1.0)
    assert abs(float(res["lengths"].astype(np.float64).sum()) - ln * n) <= 1e-6 * max(1.0, ln * n)


# 8 x the largest run-to-run difference that the drained float-atomic return sum showed between two identical runs
# without ep_window, measured once on an MI355X and taken relative to the sum of the absolute episode returns
# (profiles/ep_monitor.txt: 9.8e-4 on 14 628, the MuJoCo-shaped bank at 64 x 256; 0 on the other banks)
DRAIN_BAR_REL = 8 * 6.68e-8
