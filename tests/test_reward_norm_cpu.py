"""Running return-based reward scaling (``TrainConfig.norm_reward``, ``ops/reward_norm.py``) on CPU: the torch scan
against a plain numpy fp64 loop (bit-equal), splitting a rollout, reward-unit invariance, the clip, the torch-engine
trainer (the scan sees raw rewards, a time-limit bootstrap term is added unscaled after the scaling), config refusals,
checkpoints and gloo data parallelism.

Bars. Bit-equality wherever two computations run the same fp64 operations in the same order (the scan, ``ret``, a
resumed run). Where only the summation order differs (the statistics against numpy's two-pass mean / variance, data
parallel against one process), the bound of a sum of ``n`` values: ``n * 2^-52 * sum |terms|``, with the terms the
statistic is built from -- the deviations ``d`` about each update's pivot for the mean, and ``d^2`` plus the two
correction terms of the merge (``S1^2 / nb`` and ``delta^2 count nb / tot``) for the sum of squared deviations."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from actor_critic_algs_on_tensorflow_amd import preset
from actor_critic_algs_on_tensorflow_amd.algos.trainer import ActorCriticTrainer
from actor_critic_algs_on_tensorflow_amd.config import TrainConfig
from actor_critic_algs_on_tensorflow_amd.ops.reward_norm import RewardNormalizer

U52 = 2.0 ** -52
GAMMA = 0.97


class NpRef:
    """The issue's semantics as plain Python / numpy fp64 scalars, plus the sums of absolute terms behind the bars."""

    def __init__(self, N, gamma, eps=1e-8, ret=None, count=0.0, mean=0.0, m2=0.0):
        self.N, self.gamma, self.eps = N, float(gamma), eps
        self.ret = np.zeros(N) if ret is None else np.array(ret, dtype=np.float64)
        self.count, self.mean, self.m2 = float(count), float(mean), float(m2)
        self.returns = []          # every discounted return seen
        self.abs_d = 0.0           # sum |d|
        self.abs_sq = 0.0          # sum d^2 + the merge's correction terms
        self.part = None

    def scan(self, r, done):
        T, N = r.shape
        part = np.zeros((N, 2))
        for e in range(N):
            R, S1, S2 = float(self.ret[e]), 0.0, 0.0
            for t in range(T):
                R = R * self.gamma
                R = R + float(np.float64(r[t, e]))
                d = R - self.mean
                S1 = S1 + d
                S2 = S2 + d * d
                self.returns.append(R)
                self.abs_d += abs(d)
                self.abs_sq += d * d
                if done[t, e]:
                    R = 0.0
            self.ret[e] = R
            part[e] = (S1, S2)
        self.part = part
        return part

    def merge(self, S1, S2, nb):
        count, tot = self.count, self.count + nb
        delta = S1 / nb
        self.abs_sq += S1 * S1 / nb + delta * delta * count * nb / tot
        self.mean = self.mean + S1 / tot
        self.m2 = self.m2 + ((S2 - S1 * S1 / nb) + delta * delta * count * nb / tot)
        self.count = tot

    def update(self, r, done):
        part = self.scan(np.asarray(r), np.asarray(done))
        self.merge(float(part[:, 0].sum()), float(part[:, 1].sum()), float(r.shape[0] * r.shape[1]))

    def bounds(self):
        """(mean bound, m2 bound): n 2^-52 sum |terms| for the n returns seen so far."""
        n = len(self.returns)
        return n * U52 * (self.abs_d / self.count + abs(self.mean)), n * U52 * self.abs_sq


def _case(T=7, N=3, seed=0):
    """Rewards of a few units with an offset; dones at t = 0 and t = T-1 (env 0), an all-done env (1), a never-done
    env (2); further envs random."""
    g = torch.Generator().manual_seed(seed)
    r = (torch.randn(T, N, generator=g) * 2.0 + 0.7).to(torch.float32)
    d = torch.zeros(T, N, dtype=torch.uint8)
    d[0, 0] = 1
    d[T - 1, 0] = 1
    if N > 1:
        d[:, 1] = 1
    if N > 3:
        d[:, 3:] = (torch.rand(T, N - 3, generator=g) < 0.3).to(torch.uint8)
    return r, d


def _primed(N, device="cpu", clip=10.0):
    """A normaliser with a non-zero carry and count > 0, mean != 0."""
    norm = RewardNormalizer(N, GAMMA, clip, device=device)
    f64 = lambda v: torch.tensor([v], dtype=torch.float64)
    norm.load_state_dict(dict(count=f64(11.0), mean=f64(0.31), m2=f64(23.5),
                              ret=torch.linspace(-1.5, 2.5, N, dtype=torch.float64)))
    return norm


# ------------------------------------------------------------------------------------------------ 1. oracle
def test_scan_matches_numpy_loop_bitwise():
    T, N = 7, 3
    r, d = _case(T, N)
    assert d[0, 0] and d[T - 1, 0] and d[:, 1].all() and not d[:, 2].any()
    norm = _primed(N)
    ref = NpRef(N, GAMMA, ret=norm.ret.numpy(), count=11.0, mean=0.31, m2=23.5)
    raw = r.clone()
    norm.scan(r, d)
    part = ref.scan(r.numpy(), d.numpy())
    assert np.array_equal(norm.ret.numpy(), ref.ret)
    assert np.array_equal(norm.part.numpy(), part)
    assert torch.equal(r, raw), "the scan does not modify the rewards"
    assert float(norm.ret[1]) == 0.0 and float(norm.ret[2]) != 0.0
    assert float(norm.batch[2]) == T * N


# ------------------------------------------------------------------------------------------------ 2. splitting
def test_split_updates_match_one_scan_and_numpy_statistics():
    T, N = 7, 3
    r, d = _case(T, N, seed=1)
    two, one = RewardNormalizer(N, GAMMA), RewardNormalizer(N, GAMMA)
    ref = NpRef(N, GAMMA)
    for sl in (slice(0, 4), slice(4, 7)):
        two.update_(r[sl].clone(), d[sl])
        ref.update(r[sl].numpy(), d[sl].numpy())
    one.scan(r, d)
    assert torch.equal(two.ret, one.ret)
    assert np.array_equal(two.ret.numpy(), ref.ret)
    R = np.array(ref.returns)
    assert R.size == T * N and float(two.count[0]) == T * N
    b_mean, b_m2 = ref.bounds()
    err_mean = abs(float(two.mean[0]) - R.mean())
    err_m2 = abs(float(two.m2[0]) - R.var() * R.size)
    print("mean err %.3e (bound %.3e), m2 err %.3e (bound %.3e)" % (err_mean, b_mean, err_m2, b_m2))
    assert err_mean <= b_mean, ("mean: n 2^-52 (sum |d| / count + |mean|)", err_mean, b_mean, ref.abs_d, ref.mean)
    assert err_m2 <= b_m2, ("m2: n 2^-52 (sum d^2 + sum S1^2 / nb + sum delta^2 count nb / tot)", err_m2, b_m2,
                            ref.abs_sq, float((R * R).sum()))
    istd = np.float32(1.0 / np.sqrt(float(two.m2[0]) / (T * N) + 1e-8))
    assert float(two.istd32) == float(istd) and float(two.mean32) == float(np.float32(float(two.mean[0])))


# ------------------------------------------------------------------------------------------------ 3. reward unit
def test_reward_unit_invariance():
    T, N = 24, 5
    r, d = _case(T, N, seed=2)
    a, b = RewardNormalizer(N, GAMMA), RewardNormalizer(N, GAMMA)
    ra, rb = r.clone(), r * 1024.0
    a.update_(ra, d)
    b.update_(rb, d)
    var = float(a.m2[0] / a.count[0])
    assert var >= 1e-2
    tol = ra.abs().double() * (1e-8 / (2.0 * var) + 2.0 ** -22)
    err = (ra.double() - rb.double()).abs()
    print("max err / tol", float((err / tol.clamp_min(1e-300)).max()))
    assert bool((err <= tol).all())
    assert float(ra.abs().max()) < 10.0 and float(ra.std()) < 1.5, "unit scale from the first update on"


# ------------------------------------------------------------------------------------------------ 4. clip
def test_clip_and_frozen_identity():
    T, N = 24, 5
    r, d = _case(T, N, seed=3)
    r = r - 0.7   # both signs on both sides of the clip
    norm = RewardNormalizer(N, GAMMA, clip=0.5)
    x = r.clone()
    norm.update_(x, d)
    ref = np.minimum(np.maximum(r.numpy() * norm.istd32.numpy(), np.float32(-0.5)), np.float32(0.5))
    assert x.dtype == torch.float32 and np.array_equal(x.numpy(), ref)
    assert (x == 0.5).any() and (x == -0.5).any() and float(x.abs().max()) == 0.5
    fresh = RewardNormalizer(N, GAMMA, clip=1.0).freeze()
    y = r.clone()
    fresh.update_(y, d)
    assert torch.equal(y, r.clamp(-1.0, 1.0)) and (y.abs() == 1.0).any()
    assert float(fresh.count[0]) == 0.0 and not fresh.ret.any(), "a frozen normaliser never scans or merges"
    with pytest.raises(ValueError):
        RewardNormalizer(N, GAMMA, clip=0.0)


def test_load_state_dict_keeps_gamma_and_clip():
    src = _primed(3, clip=5.0)
    sd = dict(src.state_dict(), ret=src.ret)
    assert float(sd["gamma"]) == GAMMA and float(sd["clip"]) == 5.0
    dst = RewardNormalizer(3, GAMMA, clip=2.0).load_state_dict(sd)
    assert torch.equal(dst.state, src.state) and torch.equal(dst.tables, src.tables) and torch.equal(dst.ret, src.ret)
    assert dst.clip == 2.0 and dst.gamma == GAMMA
    other = RewardNormalizer(3, 0.9)
    with pytest.raises(ValueError, match="gamma"):
        other.load_state_dict(sd)
    assert float(other.count[0]) == 0.0 and not other.ret.any(), "a refused load changes nothing"


# ------------------------------------------------------------------------------------------------ 5. torch trainer
def _quiet(**kw):
    base = dict(outdir=None, quiet=True, stdout_freq=0, save_every=0, device="cpu", cuda_graph=False)
    base.update(kw)
    return base


SMALL = {"cartpole_cpu": dict(num_envs=3, n_steps=5),
         "pendulum_ppo": dict(num_envs=4, n_steps=24, ppo_epochs=2, ppo_minibatches=2)}


def spy(tr):
    """Records, per update, the rewards and dones handed to ``update_`` (before it runs), the rewards and the tables
    it leaves, and the rewards that reach ``compute_returns``."""
    log = dict(raw=[], dones=[], scaled=[], tables=[], at_returns=[])
    update_, returns = tr.reward_norm.update_, tr.compute_returns

    def update__(rewards, dones, *a, **k):
        log["raw"].append(rewards.clone())
        log["dones"].append(dones.clone())
        out = update_(rewards, dones, *a, **k)
        log["scaled"].append(rewards.clone())
        log["tables"].append(tr.reward_norm.tables.clone())
        return out

    def returns_():
        log["at_returns"].append(tr.storage.rewards.clone())
        return returns()

    tr.reward_norm.update_, tr.compute_returns = update__, returns_
    return log


def replay(log, N, gamma, clip=10.0, device="cpu"):
    """The oracle over the recorded raw rollouts: (scaled rewards per update, the normaliser after the last)."""
    ref = RewardNormalizer(N, gamma, clip, device=device)
    out = []
    for raw, dones in zip(log["raw"], log["dones"]):
        r = raw.clone().to(device)
        ref.scan_torch(r, dones.to(device))
        ref.batch.copy_(ref.batch_from_parts(r.shape[0]))
        ref.stats.merge_batch_()
        out.append(r.mul_(ref.istd32).clamp_(-clip, clip))
    return out, ref


@pytest.mark.parametrize("name", ["cartpole_cpu", "pendulum_ppo"])
def test_torch_trainer_scales_what_reaches_the_returns(name):
    tr = ActorCriticTrainer(preset(name, **_quiet(norm_reward=True, **SMALL[name])))
    twin = ActorCriticTrainer(preset(name, **_quiet(**SMALL[name])))
    assert tr.mlp is None and tr.reward_norm is not None
    log = spy(tr)
    for _ in range(3):
        tr.step()
    twin.collect()
    assert torch.equal(log["raw"][0], twin.storage.rewards), "update 0 scans what a plain trainer collects"
    assert len(log["raw"]) == 3 == len(log["at_returns"])
    N, T = tr.storage.N, tr.storage.T
    scaled, ref = replay(log, N, tr.cfg.gamma)
    for k in range(3):
        assert torch.equal(log["at_returns"][k], scaled[k]), k
        assert not torch.equal(log["at_returns"][k], log["raw"][k])
    assert torch.equal(tr.reward_norm.state, ref.state) and torch.equal(tr.reward_norm.ret, ref.ret)
    assert float(tr.reward_norm.count[0]) == 3 * T * N
    np_ref = NpRef(N, tr.cfg.gamma)
    for raw, dones in zip(log["raw"], log["dones"]):
        np_ref.update(raw.numpy(), dones.numpy())
    assert np.array_equal(tr.reward_norm.ret.numpy(), np_ref.ret)
    b_mean, b_m2 = np_ref.bounds()
    R = np.array(np_ref.returns)
    assert abs(float(tr.reward_norm.mean[0]) - R.mean()) <= b_mean
    assert abs(float(tr.reward_norm.m2[0]) - R.var() * R.size) <= b_m2
    assert torch.isfinite(tr.flat.data).all()


def test_torch_trainer_bootstrap_term_is_added_unscaled_after_scaling():
    kw = dict(SMALL["pendulum_ppo"], bootstrap_on_timeout=True)
    tr = ActorCriticTrainer(preset("pendulum_ppo", **_quiet(norm_reward=True, **kw)))
    plain = ActorCriticTrainer(preset("pendulum_ppo", **_quiet(**SMALL["pendulum_ppo"])))
    boot = ActorCriticTrainer(preset("pendulum_ppo", **_quiet(**kw)))
    for t in (tr, plain, boot):
        t.env.max_episode_steps = 5
    log = spy(tr)
    tr.step()
    plain.collect()
    boot.collect()
    raw = log["raw"][0]
    trunc = tr.storage.truncated.bool()
    assert int(trunc.sum()) >= 4 * tr.storage.N
    # the scan saw the raw env rewards: what a trainer without bootstrapping collects, bitwise
    assert torch.equal(raw, plain.storage.rewards)
    side = tr._boot_side
    assert bool((side[trunc] != 0).all()) and not side[~trunc].any()
    # the side buffer holds the very terms a norm_reward=False trainer adds to its raw rewards ...
    assert torch.equal(boot.storage.rewards, raw + side)
    # ... and they are added, unscaled, to the scaled rewards
    scaled, _ = replay(log, tr.storage.N, tr.cfg.gamma)
    assert torch.equal(log["at_returns"][0], scaled[0] + side)
    assert not torch.equal(scaled[0], raw)
    for _ in range(2):
        tr.step()
    scaled, ref = replay(log, tr.storage.N, tr.cfg.gamma)
    assert torch.equal(log["at_returns"][2], scaled[2] + tr._boot_side)
    assert torch.equal(tr.reward_norm.state, ref.state)


# ------------------------------------------------------------------------------------------------ 6. / 7. config
def test_config_refusals():
    for kw in (dict(model="cnn"), dict(algo="a3c"), dict(algo="basic_ac")):
        with pytest.raises(ValueError, match="norm_reward"):
            TrainConfig(norm_reward=True, **kw)
    for clip in (0.0, -1.0):
        with pytest.raises(ValueError, match="reward_clip"):
            TrainConfig(norm_reward=True, reward_clip=clip)
    # model="auto" resolving to the CNN family is refused by the trainer
    with pytest.raises(ValueError, match="norm_reward=True with a CNN model"):
        ActorCriticTrainer(preset("pong_a2c", **_quiet(model="auto", num_envs=1, n_steps=1, norm_reward=True)))


def test_defaults_are_off():
    assert TrainConfig().norm_reward is False and TrainConfig().reward_clip == 10.0
    tr = ActorCriticTrainer(preset("pendulum_ppo", **_quiet(**SMALL["pendulum_ppo"])))
    assert tr.reward_norm is None
    for name in ("mujoco_ppo_dp8", "pendulum_ppo"):
        assert preset(name).norm_reward is False


# ------------------------------------------------------------------------------------------------ 8. - 10. checkpoints
def _pendulum(**kw):
    return ActorCriticTrainer(preset("pendulum_ppo", **_quiet(**dict(SMALL["pendulum_ppo"], **kw))))


@pytest.fixture(scope="module")
def bundle(tmp_path_factory):
    """A norm_reward checkpoint after 2 updates (+ the trainer that wrote it) and one written without norm_reward."""
    d = tmp_path_factory.mktemp("reward_norm_ckpt")
    tr = _pendulum(norm_reward=True, reward_clip=5.0)
    for _ in range(2):
        tr.step()
    path = tr.save_checkpoint(str(d / "model-Pendulum-2"))
    plain = _pendulum()
    plain.step()
    plain_path = plain.save_checkpoint(str(d / "plain" / "model-Pendulum-1"))
    return dict(path=path, trainer=tr, plain=plain_path, plain_trainer=plain)


def test_checkpoint_tensors_are_fp64(bundle):
    from actor_critic_algs_on_tensorflow_amd.ckpt import load_tensors
    t = load_tensors(bundle["path"])
    norm = bundle["trainer"].reward_norm
    for k, ref in (("count", norm.count), ("mean", norm.mean), ("m2", norm.m2)):
        got = np.asarray(t["_acamd/reward_norm/" + k])
        assert got.dtype == np.float64 and np.array_equal(got.reshape(-1), ref.numpy().reshape(-1)), k
    assert float(t["_acamd/reward_norm/clip"]) == 5.0
    assert float(t["_acamd/reward_norm/gamma"]) == bundle["trainer"].cfg.gamma
    ret = np.asarray(t["_acamd/env/reward_ret"])
    assert ret.dtype == np.float64 and np.array_equal(ret, norm.ret.numpy()) and ret.any()
    assert float(np.abs(ret - ret.astype(np.float32)).max()) > 0, "fp32 storage would have lost bits"
    plain = load_tensors(bundle["plain"])
    assert not any("reward" in k for k in plain)


def test_checkpoint_resume_is_bitwise(bundle):
    whole = _pendulum(norm_reward=True, reward_clip=5.0)
    for _ in range(4):
        whole.step()
    resumed = _pendulum(norm_reward=True, reward_clip=5.0)
    resumed.load_checkpoint(bundle["path"])
    src = bundle["trainer"].reward_norm
    assert torch.equal(resumed.reward_norm.state, src.state) and torch.equal(resumed.reward_norm.tables, src.tables)
    assert torch.equal(resumed.reward_norm.ret, src.ret)
    for _ in range(2):
        resumed.step()
    assert torch.equal(resumed.flat.data, whole.flat.data)
    assert torch.equal(resumed.reward_norm.state, whole.reward_norm.state)
    assert torch.equal(resumed.reward_norm.tables, whole.reward_norm.tables)
    assert torch.equal(resumed.reward_norm.ret, whole.reward_norm.ret)


def test_checkpoint_without_tensors_and_ignored_tensors(bundle):
    with pytest.raises(KeyError, match="_acamd/reward_norm/count"):
        _pendulum(norm_reward=True).load_checkpoint(bundle["plain"])
    tr = _pendulum()
    tr.load_checkpoint(bundle["path"])   # a norm_reward=False trainer ignores them
    assert tr.reward_norm is None and torch.equal(tr.flat.data, bundle["trainer"].flat.data)
    from actor_critic_algs_on_tensorflow_amd.api import Agent
    agent = Agent.from_checkpoint(bundle["path"], "Pendulum-v0")
    assert not hasattr(agent, "reward_norm")


# ------------------------------------------------------------------------------------------------ 11. gloo world 2
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


DP_KW = dict(num_envs=2, n_steps=12, ppo_epochs=2, ppo_minibatches=2, seed=5, norm_reward=True)


def _dp_worker(rank, world, port, out_dir):
    import torch.distributed as dist
    from actor_critic_algs_on_tensorflow_amd.parallel.dp import DataParallel
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    tr = ActorCriticTrainer(preset("pendulum_ppo", **_quiet(**DP_KW)), dp=DataParallel())
    log = spy(tr)
    states, rets = [], []
    for _ in range(2):
        tr.step()
        states.append(tr.reward_norm.state.clone())
        rets.append(tr.reward_norm.ret.clone())
    torch.save({"p": tr.flat.data.clone(), "tables": tr.reward_norm.tables.clone(), "states": states, "rets": rets,
                "raw": log["raw"], "dones": log["dones"], "at_returns": log["at_returns"]},
               os.path.join(out_dir, f"r{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_dp_gloo_world2(tmp_path):
    """Both ranks hold bitwise-identical statistics and parameters; ``ret`` is per rank. The statistics equal, within
    the bound of a reordered sum, one normaliser fed the union of both ranks' raw rollouts update by update, and after
    update 0 (whose rollouts do not depend on the learner) a single-process trainer over the same 4 envs."""
    world = 2
    mp.spawn(_dp_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    out = [torch.load(tmp_path / f"r{r}.pt", weights_only=True) for r in range(world)]
    assert torch.equal(out[0]["p"], out[1]["p"]) and torch.equal(out[0]["tables"], out[1]["tables"])
    for u in range(2):
        assert torch.equal(out[0]["states"][u], out[1]["states"][u]), u
    assert not torch.equal(out[0]["rets"][1], out[1]["rets"][1]), "ret is local to each rank"
    n, gamma = DP_KW["num_envs"], preset("pendulum_ppo").gamma
    union = NpRef(world * n, gamma)
    one = RewardNormalizer(world * n, gamma)
    for u in range(2):
        raw = torch.cat([out[r]["raw"][u] for r in range(world)], dim=1)
        dones = torch.cat([out[r]["dones"][u] for r in range(world)], dim=1)
        union.update(raw.numpy(), dones.numpy())
        scaled = raw.clone()
        one.update_(scaled, dones)
        b_mean, b_m2 = union.bounds()
        got = out[0]["states"][u]
        assert float(got[0]) == float(one.count[0]) == (u + 1) * 12 * world * n
        assert abs(float(got[1]) - float(one.mean[0])) <= b_mean and abs(float(got[2]) - float(one.m2[0])) <= b_m2
        assert np.array_equal(torch.cat([out[r]["rets"][u] for r in range(world)]).numpy(), union.ret)
        # every rank scaled its own rewards with the shared istd32
        for r in range(world):
            torch.testing.assert_close(out[r]["at_returns"][u], scaled[:, r * n:(r + 1) * n], rtol=2.0 ** -22, atol=0)
    single = ActorCriticTrainer(preset("pendulum_ppo", **_quiet(**dict(DP_KW, num_envs=world * n))))
    single.step()
    first = NpRef(world * n, gamma)
    first.update(torch.cat([out[r]["raw"][0] for r in range(world)], dim=1).numpy(),
                 torch.cat([out[r]["dones"][0] for r in range(world)], dim=1).numpy())
    b_mean, b_m2 = first.bounds()
    got = out[0]["states"][0]
    assert abs(float(got[1]) - float(single.reward_norm.mean[0])) <= b_mean
    assert abs(float(got[2]) - float(single.reward_norm.m2[0])) <= b_m2
    assert torch.equal(torch.cat([out[r]["rets"][0] for r in range(world)]), single.reward_norm.ret)
