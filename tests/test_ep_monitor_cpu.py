"""Rolling window over the last K finished training episodes (``TrainConfig.ep_window``, ``ops/ep_monitor.py``) on CPU:
the torch form against the independent double loop of ``tests/oracles/ep_monitor_oracle.py``, the torch-engine
trainers (the window sees raw rewards; nothing the trainer reads is written), the metrics row, ``stop_return``,
checkpoints, config refusals and gloo data parallelism.

Bars. Every state array (carry, ring, total) and the summary's counts, minimum and maximum are exact: both sides run
the same fp32 adds in the same order and move the same values. The means and the standard deviation are fp64 sums of
at most 4096 fp32 values in two different orders: they differ by at most ``(K - 1) 2^-52 max|x|`` on the mean, well
inside the ``1e-12 max(1, max|ret|)`` used here (plus ``1e-12`` relative on the standard deviation, whose two-pass form
keeps its error at the same scale)."""
import json
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "oracles"))
from ep_monitor_oracle import EpMonitorOracle   # noqa: E402

from actor_critic_algs_on_tensorflow_amd import preset   # noqa: E402
from actor_critic_algs_on_tensorflow_amd.algos.trainer import ActorCriticTrainer   # noqa: E402
from actor_critic_algs_on_tensorflow_amd.config import TrainConfig   # noqa: E402
from actor_critic_algs_on_tensorflow_amd.ops.ep_monitor import SUMMARY_KEYS, EpisodeMonitor   # noqa: E402

KS = (1, 7, 100)
EP_KEYS = ("ep_ret_mean", "ep_ret_std", "ep_ret_min", "ep_ret_max", "ep_len_mean", "ep_count", "ep_total", "ep_new")


# ------------------------------------------------------------------------------------------------ shared cases
def _rewards(T, N, g):
    """Random non-integer fp32 of a few units with an offset: the order of the adds matters."""
    return (torch.randn(T, N, generator=g) * 2.0 + 0.7).to(torch.float32)


def _exact(T, N, C, g):
    """Exactly ``min(C, T N)`` dones at random cells."""
    d = torch.zeros(T * N, dtype=torch.uint8)
    d[torch.randperm(T * N, generator=g)[:min(C, T * N)]] = 1
    return d.view(T, N)


def sequence(T, N, K, seed=0):
    """Consecutive updates ``[(rewards, dones, C)]`` for one monitor (the carry runs through all of them): no done at
    all; dones at (0, 0) and (T-1, N-1) only; a step where every env is done; exactly ``C = K``; ``0 < C < K`` (where
    K > 1); ``C > 2K`` (the ring wraps more than once; as many as the shape holds); a random 30 %."""
    g = torch.Generator().manual_seed(seed * 1000 + T * 7 + N * 3 + K)
    out = []

    def add(d):
        out.append((_rewards(T, N, g), d.contiguous(), int(d.sum())))

    add(torch.zeros(T, N, dtype=torch.uint8))
    corners = torch.zeros(T, N, dtype=torch.uint8)
    corners[0, 0] = corners[T - 1, N - 1] = 1
    add(corners)
    row = corners.clone()
    row[T // 2] = 1
    add(row)
    add(_exact(T, N, K, g))
    if K > 1:
        add(_exact(T, N, max(1, K // 2), g))
    add(_exact(T, N, 2 * K + 3, g))
    add((torch.rand(T, N, generator=g) < 0.3).to(torch.uint8))
    return out


def assert_matches_oracle(mon, ref, what=""):
    """``mon`` (an EpisodeMonitor on any device) against the oracle after the same updates."""
    for k in ("cur_ret", "cur_len", "ring_ret", "ring_len"):
        got = getattr(mon, k).cpu().numpy()
        assert got.dtype == getattr(ref, k).dtype and np.array_equal(got, getattr(ref, k)), (what, k)
    assert int(mon.total[0]) == ref.total, what
    s = dict(zip(SUMMARY_KEYS, mon.summary.cpu().tolist()))
    o = ref.summary
    for k in ("filled", "total", "new", "ret_min", "ret_max"):
        assert s[k] == o[k], (what, k, s[k], o[k])
    filled = int(o["filled"])
    big = max(1.0, float(np.abs(ref.ring_ret[:filled]).max())) if filled else 1.0
    tol = 1e-12 * big
    for k in ("ret_mean", "len_mean", "new_ret_mean", "new_len_mean"):
        scale = max(1.0, abs(o[k])) if k.startswith("new") or k == "len_mean" else 1.0
        assert abs(s[k] - o[k]) <= tol * scale, (what, k, s[k], o[k])
    assert abs(s["ret_std"] - o["ret_std"]) <= tol + 1e-12 * o["ret_std"], (what, s["ret_std"], o["ret_std"])
    if filled and float(np.ptp(ref.ring_ret[:filled])) == 0.0:
        assert s["ret_std"] == 0.0 and s["ret_mean"] == float(ref.ring_ret[0]), what
    res = mon.result()
    ret, ln = ref.chronological()
    assert np.array_equal(res["returns"], ret) and np.array_equal(res["lengths"], ln), what


# ------------------------------------------------------------------------------------------------ the torch form
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("T,N", [(5, 3), (16, 13)])
def test_torch_form_equals_the_oracle(T, N, K):
    mon, ref, rows = EpisodeMonitor(N, K), EpMonitorOracle(N, K), EpMonitorOracle(N, K)
    seen = set()
    for u, (r, d, C) in enumerate(sequence(T, N, K)):
        mon.update(r, d)
        ref.update(r.numpy(), d.numpy())
        rows.update(r.numpy(), d.numpy(), rows=True)
        assert_matches_oracle(mon, ref, (T, N, K, u))
        assert ref.summary["new"] == C
        # the oracle's large-shape form is the same loop
        for k in ("cur_ret", "cur_len", "ring_ret", "ring_len"):
            assert np.array_equal(getattr(rows, k), getattr(ref, k))
        assert rows.total == ref.total and rows.summary == ref.summary
        seen.add("0" if C == 0 else "<K" if C < K else "=K" if C == K else ">2K" if C > 2 * K else "other")
    want = {"0", "=K", ">2K"} | ({"<K"} if K > 1 else set())
    if 2 * K + 1 > T * N:   # (the shape cannot hold that many: (16, 13) holds every case of every K)
        want -= {">2K"} | ({"=K"} if K > T * N else set())
    assert want <= seen, (want, seen)


def test_equal_window_has_zero_std_and_exact_mean():
    mon = EpisodeMonitor(2, 7)
    r = torch.full((6, 2), 0.1, dtype=torch.float32)
    d = torch.zeros(6, 2, dtype=torch.uint8)
    d[2] = d[5] = 1
    mon.update(r, d)
    res = mon.result()
    x = np.float32(np.float32(np.float32(0.1) + np.float32(0.1)) + np.float32(0.1))
    assert res["filled"] == 4 and res["ret_std"] == 0.0 and res["ret_mean"] == float(x) == res["ret_min"]
    assert res["len_mean"] == 3.0 and res["new"] == 4 and res["new_len_mean"] == 3.0


def test_shape_checks_and_state_dict():
    mon = EpisodeMonitor(3, 4)
    r, d = torch.zeros(5, 3), torch.zeros(5, 3, dtype=torch.uint8)
    for bad_r, bad_d in ((torch.zeros(5, 4), torch.zeros(5, 4, dtype=torch.uint8)), (r, d[:4]), (r[0], d[0]),
                         (r.double(), d), (r, d.bool())):
        with pytest.raises(ValueError, match="EpisodeMonitor"):
            mon.update(bad_r, bad_d)
    for K in (0, 4097):
        with pytest.raises(ValueError, match="window K"):
            EpisodeMonitor(3, K)
    for rr, dd, _ in sequence(5, 3, 4)[:5]:
        mon.update(rr, dd)
    twin = EpisodeMonitor(3, 4).load_state_dict(mon.state_dict())
    for k in ("cur_ret", "cur_len", "ring_ret", "ring_len", "total"):
        assert torch.equal(getattr(twin, k), getattr(mon, k)), k
    assert torch.equal(twin.summary[:7], mon.summary[:7])
    with pytest.raises(ValueError, match="K=4"):
        EpisodeMonitor(3, 5).load_state_dict(mon.state_dict())
    with pytest.raises(KeyError, match="ring_len"):
        EpisodeMonitor(3, 4).load_state_dict({k: v for k, v in mon.state_dict().items() if k != "ring_len"})


# ------------------------------------------------------------------------------------------------ trainers
def _quiet(**kw):
    base = dict(outdir=None, quiet=True, stdout_freq=0, save_every=0, device="cpu", cuda_graph=False)
    base.update(kw)
    return base


SMALL = {"cartpole_cpu": dict(num_envs=3, n_steps=5),
         "pendulum_ppo": dict(num_envs=4, n_steps=24, ppo_epochs=2, ppo_minibatches=2)}
VARIANTS = [("cartpole_cpu", {}), ("pendulum_ppo", {}),
            ("pendulum_ppo", dict(norm_reward=True, bootstrap_on_timeout=True))]


def _trainer(name, limit=None, **kw):
    tr = ActorCriticTrainer(preset(name, **_quiet(**dict(SMALL[name], **kw))))
    if limit is not None:
        tr.env.max_episode_steps = limit   # episodes end within an update
    return tr


def spy_monitor(tr):
    """Records the rewards / dones handed to the monitor, update by update."""
    log = dict(raw=[], dones=[])
    update = tr.ep_monitor.update

    def update_(rewards, dones):
        log["raw"].append(rewards.clone())
        log["dones"].append(dones.clone())
        return update(rewards, dones)

    tr.ep_monitor.update = update_
    return log


@pytest.mark.parametrize("name,kw", VARIANTS)
def test_torch_trainer_window_is_raw_and_changes_nothing(name, kw):
    limit = 7 if name == "pendulum_ppo" else None
    on, off = _trainer(name, limit, ep_window=100, **kw), _trainer(name, limit, **kw)
    assert on.mlp is None and on.ep_monitor is not None and off.ep_monitor is None
    log = spy_monitor(on)
    ref = EpMonitorOracle(on.storage.N, 100)
    for u in range(6):
        on.step()
        off.step()
        ref.update(log["raw"][u].numpy(), log["dones"][u].numpy())
        assert_matches_oracle(on.ep_monitor, ref, (name, u))
    assert len(log["raw"]) == 6 and ref.total > 0
    # the carry is the bank's own accumulator: the window saw the raw env rewards, in step order
    assert torch.equal(on.ep_monitor.cur_ret, on.env.ep_ret)
    assert torch.equal(on.ep_monitor.cur_len.to(torch.int64), on.env.t.to(torch.int64))
    # nothing the trainer reads was written
    assert torch.equal(on.flat.data, off.flat.data)
    for k in ("rewards", "dones", "values", "logp"):
        assert torch.equal(getattr(on.storage, k), getattr(off.storage, k)), k
    for g in on.opts:
        for k, v in on.opts[g].state_dict().items():
            assert torch.equal(torch.as_tensor(v), torch.as_tensor(off.opts[g].state_dict()[k])), (g, k)
    if kw.get("norm_reward"):
        assert torch.equal(on.reward_norm.state, off.reward_norm.state)
        assert torch.equal(on.reward_norm.ret, off.reward_norm.ret)
        assert not torch.equal(log["raw"][-1], on.storage.rewards), "the trainer learns from scaled rewards"
    # episode count and return sum agree with the bank's own drained statistics
    mean, n, _ = on.env.drain_episode_stats()
    assert n == ref.total
    got = on.ep_monitor.result()
    assert abs(float(got["returns"].astype(np.float64).sum()) - mean * n) <= 1e-4 * max(1.0, abs(mean * n))


def test_metrics_row_carries_the_window(tmp_path):
    m = tmp_path / "metrics.jsonl"
    tr = _trainer("cartpole_cpu", ep_window=100, outdir=str(tmp_path / "log.txt"), metrics_path=str(m),
                  stdout_freq=2)
    hist = tr.train(7)
    tr.close()
    rows = [json.loads(line) for line in open(m)]
    assert len(rows) == 4 == len(hist) and tr.stopped_at is None
    for row in rows:
        assert set(EP_KEYS) <= set(row), sorted(row)
        assert "avg_rew" in row and "episodes" in row   # the reference columns stay
    last = tr.ep_monitor.result()
    assert rows[-1]["ep_total"] == last["total"] > 0 and rows[-1]["ep_count"] == last["filled"]
    assert rows[-1]["ep_ret_mean"] == last["ret_mean"] and rows[-1]["ep_ret_std"] == last["ret_std"]
    plain = _trainer("cartpole_cpu", outdir=str(tmp_path / "p" / "log.txt"), metrics_path=str(tmp_path / "p.jsonl"),
                     stdout_freq=2)
    plain.train(3)
    plain.close()
    for line in open(tmp_path / "p.jsonl"):
        assert not set(EP_KEYS) & set(json.loads(line)), "default off: no new column"


# ------------------------------------------------------------------------------------------------ stop_return
def _cartpole_v0(tmp_path, **kw):
    return _trainer("cartpole_cpu", env="CartPole-v0", ep_window=8, stdout_freq=1, outdir=str(tmp_path / "log.txt"),
                    total_updates=60, **kw)


def test_stop_return_stops_at_the_first_full_window(tmp_path):
    seen = []
    twin = _cartpole_v0(tmp_path / "twin")
    twin.train(60, callback=lambda t, it: seen.append(t.ep_monitor.result()))
    twin.close()
    first = next(i for i, r in enumerate(seen) if r["filled"] == 8)
    assert seen[first]["ret_mean"] >= 5 and first < 59, "the untrained policy's window already meets the threshold"
    tr = _cartpole_v0(tmp_path / "stop", stop_return=5.0)
    hist = tr.train()
    tr.close()
    assert tr.stopped_at == first and tr.iteration == first + 1 and len(hist) == first + 1
    assert hist[-1]["ep_count"] == 8 and hist[-1]["ep_ret_mean"] >= 5
    assert torch.equal(tr.flat.data, _run(twin_of=tmp_path / "again", n=first + 1).flat.data)


def _run(twin_of, n):
    tr = _cartpole_v0(twin_of)
    tr.train(n)
    tr.close()
    return tr


def test_stop_return_out_of_reach_runs_to_the_end(tmp_path):
    tr = _cartpole_v0(tmp_path, stop_return=1e9)
    tr.train(12)
    tr.close()
    assert tr.stopped_at is None and tr.iteration == 12


# ------------------------------------------------------------------------------------------------ config
def test_config_refusals():
    for algo in ("a3c", "basic_ac"):
        with pytest.raises(ValueError, match="ep_window"):
            TrainConfig(ep_window=100, algo=algo)
    for K in (-1, 4097):
        with pytest.raises(ValueError, match="ep_window"):
            TrainConfig(ep_window=K)
    with pytest.raises(ValueError, match="stop_return needs ep_window"):
        TrainConfig(stop_return=100.0)
    with pytest.raises(ValueError, match="stop_return needs stdout_freq"):
        TrainConfig(stop_return=100.0, ep_window=10, stdout_freq=0)
    assert TrainConfig().ep_window == 0 and TrainConfig().stop_return is None
    assert TrainConfig(ep_window=4096).ep_window == 4096 and TrainConfig(ep_window=1).ep_window == 1
    tr = _trainer("cartpole_cpu")
    assert tr.ep_monitor is None and tr.stopped_at is None
    # the trainer checks again (a config edited after construction)
    cfg = preset("cartpole_cpu", **_quiet(**SMALL["cartpole_cpu"]))
    object.__setattr__(cfg, "stop_return", 10.0)
    with pytest.raises(ValueError, match="stop_return needs ep_window"):
        ActorCriticTrainer(cfg)


# ------------------------------------------------------------------------------------------------ checkpoints
def _pendulum(**kw):
    return _trainer("pendulum_ppo", 7, **kw)


@pytest.fixture(scope="module")
def bundle(tmp_path_factory):
    d = tmp_path_factory.mktemp("ep_monitor_ckpt")
    tr = _pendulum(ep_window=7)
    for _ in range(3):
        tr.step()
    path = tr.save_checkpoint(str(d / "model-Pendulum-3"))
    plain = _pendulum()
    plain.step()
    return dict(path=path, trainer=tr, plain=plain.save_checkpoint(str(d / "plain" / "model-Pendulum-1")))


def test_checkpoint_tensors(bundle):
    from actor_critic_algs_on_tensorflow_amd.ckpt import load_tensors
    t, mon = load_tensors(bundle["path"]), bundle["trainer"].ep_monitor
    assert int(mon.total[0]) > 7, "the ring has wrapped"
    for k, dt in (("cur_ret", np.float32), ("cur_len", np.int32), ("ring_ret", np.float32), ("ring_len", np.int32),
                  ("total", np.int64)):
        got = np.asarray(t["_acamd/ep_monitor/" + k])
        assert got.dtype == dt and np.array_equal(got.reshape(-1), getattr(mon, k).numpy()), k
    assert not any("ep_monitor" in k for k in load_tensors(bundle["plain"]))


def test_checkpoint_resume_is_bitwise(bundle):
    whole = _pendulum(ep_window=7)
    for _ in range(5):
        whole.step()
    resumed = _pendulum(ep_window=7)
    resumed.load_checkpoint(bundle["path"])
    for k in ("cur_ret", "cur_len", "ring_ret", "ring_len", "total"):
        assert torch.equal(getattr(resumed.ep_monitor, k), getattr(bundle["trainer"].ep_monitor, k)), k
    for _ in range(2):
        resumed.step()
    assert torch.equal(resumed.flat.data, whole.flat.data)
    for k in ("cur_ret", "cur_len", "ring_ret", "ring_len", "total", "summary"):
        assert torch.equal(getattr(resumed.ep_monitor, k), getattr(whole.ep_monitor, k)), k
    a, b = resumed.ep_monitor.result(), whole.ep_monitor.result()
    assert np.array_equal(a["returns"], b["returns"]) and np.array_equal(a["lengths"], b["lengths"])


def test_checkpoint_refusals(bundle):
    with pytest.raises(KeyError, match="_acamd/ep_monitor/cur_ret"):
        _pendulum(ep_window=7).load_checkpoint(bundle["plain"])
    with pytest.raises(ValueError, match="K=7"):
        _pendulum(ep_window=8).load_checkpoint(bundle["path"])
    tr = _pendulum()
    tr.load_checkpoint(bundle["path"])   # an ep_window=0 trainer ignores the tensors
    assert tr.ep_monitor is None and torch.equal(tr.flat.data, bundle["trainer"].flat.data)


# ------------------------------------------------------------------------------------------------ gloo world 2
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


DP_KW = dict(num_envs=2, n_steps=12, ppo_epochs=2, ppo_minibatches=2, seed=5, stdout_freq=1)


def _dp_worker(rank, world, port, out_dir):
    import torch.distributed as dist
    from actor_critic_algs_on_tensorflow_amd.parallel.dp import DataParallel
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    out = {}
    for tag, K in (("on", 100), ("off", 0)):
        kw = dict(DP_KW, ep_window=K, outdir=os.path.join(out_dir, tag, "log.txt"),
                  metrics_path=os.path.join(out_dir, f"{tag}.jsonl"))
        tr = ActorCriticTrainer(preset("pendulum_ppo", **_quiet(**kw)), dp=DataParallel())
        tr.env.max_episode_steps = 5
        calls = []
        comm = tr._comm
        tr._comm = lambda fn, comm=comm, calls=calls: (calls.append(1), comm(fn))[1]
        tr.train(3)
        tr.close()
        out[tag] = dict(p=tr.flat.data.clone(), collectives=len(calls),
                        ring=None if tr.ep_monitor is None else tr.ep_monitor.ring_ret.clone(),
                        total=None if tr.ep_monitor is None else int(tr.ep_monitor.total[0]))
    torch.save(out, os.path.join(out_dir, f"r{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_dp_gloo_world2(tmp_path):
    """``ep_window`` under data parallelism: it trains, every rank keeps the window of its own envs, rank 0 logs its
    own, and neither a collective nor a parameter bit differs from the ``ep_window=0`` twin."""
    world = 2
    mp.spawn(_dp_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    out = [torch.load(tmp_path / f"r{r}.pt", weights_only=True) for r in range(world)]
    for r in range(world):
        assert out[r]["on"]["collectives"] == out[r]["off"]["collectives"] > 0
        assert torch.equal(out[r]["on"]["p"], out[r]["off"]["p"]) and torch.equal(out[r]["on"]["p"], out[0]["on"]["p"])
        assert out[r]["on"]["total"] == 3 * 12 * 2 // 5
    assert not torch.equal(out[0]["on"]["ring"], out[1]["on"]["ring"]), "each rank keeps its own window"
    rows = [json.loads(line) for line in open(tmp_path / "on.jsonl")]
    assert len(rows) == 3 and all(set(EP_KEYS) <= set(row) for row in rows)
    assert rows[-1]["ep_total"] == out[0]["on"]["total"]
    assert not any(set(EP_KEYS) & set(json.loads(line)) for line in open(tmp_path / "off.jsonl"))
    with pytest.raises(ValueError, match="stop_return under data parallelism"):
        ActorCriticTrainer(preset("pendulum_ppo", **_quiet(**dict(DP_KW, ep_window=8, stop_return=1.0))),
                           dp=type("FakeDP", (), dict(rank=0, world_size=2))())
