"""Running observation normalisation (``TrainConfig.norm_obs``, ``ops/obs_norm.py``) on CPU: the merge arithmetic
against numpy's fp64 statistics, the apply formula, the torch-engine trainer's schedule (tables frozen within an
update, the rollout's ``obs[0:T]`` merged after its learner, storage raw), config refusals, checkpoints, ``Agent`` and
gloo data parallelism.

Bars: ``|d mean| <= 1e-10 * std``, ``rtol 1e-10`` on the variance, fp32 tables within 2 ulp of the
tables derived from numpy's values."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from actor_critic_algs_on_tensorflow_amd import preset
from actor_critic_algs_on_tensorflow_amd.algos.trainer import ActorCriticTrainer
from actor_critic_algs_on_tensorflow_amd.config import TrainConfig
from actor_critic_algs_on_tensorflow_amd.ops.obs_norm import ObsNormalizer

D = 17
SIZES = (37, 137, 237, 337, 437, 537)


def _data(seed=0):
    """Six fp32 batches of 37 .. 537 rows, column scales 0.01 .. 50 (log-spaced) and offsets of alternating sign up to
    +-100. The offset of a column is twice its scale: the first merge pivots about the identity state's mean 0, so its
    ``S2 - S1^2 / nb`` loses ``(mean / std)^2`` of fp64's 1.1e-16 -- a property of additive statistics about a pivot
    every rank shares, not of an implementation. At ``|mean| / std = 2`` that leaves the bars their three orders of
    magnitude over the measured error."""
    g = torch.Generator().manual_seed(seed)
    scale = torch.logspace(-2, np.log10(50.0), D)
    off = 2.0 * scale * torch.tensor([1.0, -1.0] * D)[:D]
    return [(torch.randn(n, D, generator=g) * scale + off).to(torch.float32) for n in SIZES]


def check_state(norm, rows, what=""):
    """The normaliser's state and tables against numpy's fp64 statistics of ``rows`` (every raw row merged so far)."""
    x = np.asarray(rows.detach().cpu().numpy(), dtype=np.float64).reshape(-1, norm.D)
    mean, var = x.mean(0), x.var(0)
    std = np.sqrt(var)
    assert float(norm.count[0]) == x.shape[0], what
    got_mean = norm.mean.cpu().numpy()
    got_var = (norm.m2 / norm.count[0]).cpu().numpy()
    assert np.all(np.abs(got_mean - mean) <= 1e-10 * std + 1e-300), (what, np.abs(got_mean - mean) / std)
    np.testing.assert_allclose(got_var, var, rtol=1e-10, atol=0, err_msg=what)
    for got, ref in ((norm.mean32.cpu().numpy(), mean.astype(np.float32)),
                     (norm.istd32.cpu().numpy(), (1.0 / np.sqrt(var + norm.eps)).astype(np.float32))):
        ulp = np.spacing(np.maximum(np.abs(got), np.abs(ref)).astype(np.float32))
        assert np.all(np.abs(got.astype(np.float64) - ref.astype(np.float64)) <= 2.0 * ulp), (what, got, ref)


def _merged(clip=10.0):
    norm = ObsNormalizer(D, clip=clip)
    batches = _data()
    for i, b in enumerate(batches):
        # 1-3 parts whose statistics are added, as data-parallel ranks would
        parts = torch.tensor_split(b, 1 + i % 3)
        norm.batch.copy_(sum(norm.batch_stats(p) for p in parts))
        norm.merge_batch_()
    return norm, torch.cat(batches)


# ------------------------------------------------------------------------------------------------ 1. merge arithmetic
def test_merge_matches_numpy_fp64():
    norm = ObsNormalizer(D)
    seen = []
    for i, b in enumerate(_data()):
        parts = torch.tensor_split(b, 1 + i % 3)
        assert len(parts) == 1 + i % 3
        norm.batch.copy_(sum(norm.batch_stats(p) for p in parts))
        norm.merge_batch_()
        seen.append(b)
        check_state(norm, torch.cat(seen), f"after batch {i}")
    assert float(norm.count[0]) == sum(SIZES)


def test_prepare_merge_is_the_same_arithmetic():
    """``prepare`` + ``merge`` (the trainer's calls) == ``batch_stats`` + ``merge_batch_``; rows past ``r_stat`` are
    normalised but not counted; an empty batch changes nothing."""
    a, b = ObsNormalizer(D), ObsNormalizer(D)
    for x in _data():
        plane = torch.empty_like(x)
        a.prepare(x, plane, x.shape[0] - 5)
        assert torch.equal(plane, a.apply(x))
        a.merge()
        b.batch.copy_(b.batch_stats(x[:x.shape[0] - 5]))
        b.merge_batch_()
        assert torch.equal(a.state, b.state) and torch.equal(a.tables, b.tables)
    before = a.state.clone(), a.tables.clone()
    a.prepare(x, plane, 0)
    a.merge()
    assert torch.equal(a.state, before[0]) and torch.equal(a.tables, before[1])


# ------------------------------------------------------------------------------------------------ 2. apply
def test_apply_identity_then_clipped():
    norm = ObsNormalizer(D, clip=1.5)
    x = torch.cat(_data()).clamp(-1.5, 1.5)   # (the clamp itself holds from the start)
    assert torch.equal(norm.apply(x), x), "identity tables while count == 0"
    norm, rows = _merged(clip=1.5)
    y = norm.apply(rows)
    # exactly subtract, multiply, clamp in fp32
    m, s = norm.mean32.numpy(), norm.istd32.numpy()
    ref = np.minimum(np.maximum((rows.numpy() - m) * s, np.float32(-1.5)), np.float32(1.5))
    assert y.dtype == torch.float32 and np.array_equal(y.numpy(), ref)
    frac = float(((y == 1.5) | (y == -1.5)).float().mean())
    assert (y == 1.5).any() and (y == -1.5).any() and 0.02 < frac < 0.2, frac   # 13 % of a unit normal lies past 1.5
    assert float(y.abs().max()) == 1.5


# ------------------------------------------------------------------------------------------------ 3. torch-engine trainer
def _quiet(**kw):
    base = dict(outdir=None, quiet=True, stdout_freq=0, save_every=0, device="cpu", cuda_graph=False)
    base.update(kw)
    return base


SMALL = {"cartpole_cpu": dict(num_envs=3, n_steps=5),
         "pendulum_ppo": dict(num_envs=4, n_steps=24, ppo_epochs=2, ppo_minibatches=2)}


def spy(tr):
    """Records, per update, the raw ``obs[0:T]`` and the tables at ``collect`` and right before ``merge``."""
    log = dict(rows=[], at_collect=[], at_merge=[])
    collect, merge = tr.collect, tr.obs_norm.merge

    def collect_():
        log["at_collect"].append(tr.obs_norm.tables.clone())
        return collect()

    def merge_(*a, **k):
        st = tr.storage
        log["rows"].append(st.obs[:st.T].clone())
        log["at_merge"].append(tr.obs_norm.tables.clone())
        return merge(*a, **k)

    tr.collect, tr.obs_norm.merge = collect_, merge_
    return log


@pytest.mark.parametrize("name", ["cartpole_cpu", "pendulum_ppo"])
def test_torch_trainer_schedule(name):
    tr = ActorCriticTrainer(preset(name, **_quiet(norm_obs=True, **SMALL[name])))
    twin = ActorCriticTrainer(preset(name, **_quiet(norm_obs=False, **SMALL[name])))
    assert tr.mlp is None and tr.obs_norm is not None and twin.obs_norm is None
    log = spy(tr)
    first = tr.storage.obs[0].clone()
    assert torch.equal(first, twin.storage.obs[0])
    for k in range(3):
        tr.step()
        assert len(log["rows"]) == k + 1
        # frozen for the whole of update k: rollout, bootstrap values, every epoch, the post-update KL evaluation
        assert torch.equal(log["at_collect"][k], log["at_merge"][k])
        if k:
            assert not torch.equal(log["at_collect"][k], log["at_collect"][k - 1]), "the merge of update k-1 acts in k"
        check_state(tr.obs_norm, torch.cat([r.reshape(-1, tr.obs_norm.D) for r in log["rows"]]), f"update {k}")
        if k == 0:
            # identity tables: update 0 collects what the norm_obs=False twin collects, bitwise, and storage is raw
            twin.step()
            assert torch.equal(log["rows"][0][0], first)
            assert torch.equal(tr.storage.obs[1:], twin.storage.obs[1:])
            assert torch.equal(tr.storage.actions, twin.storage.actions)
    assert torch.isfinite(tr.flat.data).all()


def test_torch_trainer_bootstrap_on_timeout_value_is_normalised():
    """``bootstrap_on_timeout``: V(final_obs) reads the normalised terminal observation (a model that sees raw rows
    would differ once the tables are not the identity)."""
    kw = _quiet(norm_obs=True, bootstrap_on_timeout=True, **SMALL["pendulum_ppo"])
    tr = ActorCriticTrainer(preset("pendulum_ppo", **kw))
    tr.env.max_episode_steps = 7
    tr.step()
    seen = []
    value = tr.model.value
    tr.model.value = lambda o: (seen.append(o.clone()), value(o))[1]
    tr.collect()
    tr.model.value = value
    assert len(seen) >= tr.storage.T + 1   # (model(obs) values its input too)
    assert torch.equal(seen[-2], tr.obs_norm.apply(tr.env.final_obs))
    assert torch.equal(seen[-1], tr.obs_norm.apply(tr.storage.obs[tr.storage.T]))
    assert not torch.equal(seen[-1], tr.storage.obs[tr.storage.T])


# ------------------------------------------------------------------------------------------------ 4. config refusals
def test_config_refusals():
    for kw in (dict(model="cnn"), dict(algo="a3c"), dict(algo="basic_ac")):
        with pytest.raises(ValueError, match="norm_obs"):
            TrainConfig(norm_obs=True, **kw)
    with pytest.raises(ValueError, match="obs_clip"):
        TrainConfig(norm_obs=True, obs_clip=0.0)
    # model="auto" resolving to the CNN family is refused by the trainer
    with pytest.raises(ValueError, match="norm_obs=True with a CNN model"):
        ActorCriticTrainer(preset("pong_a2c", **_quiet(model="auto", num_envs=1, n_steps=1, norm_obs=True)))
    assert TrainConfig().norm_obs is False and TrainConfig().obs_clip == 10.0


# ------------------------------------------------------------------------------------------------ 5. checkpoints
def _pendulum(**kw):
    return ActorCriticTrainer(preset("pendulum_ppo", **_quiet(**dict(SMALL["pendulum_ppo"], **kw))))


@pytest.fixture(scope="module")
def bundle(tmp_path_factory):
    """A norm_obs checkpoint after 2 updates (+ the trainer that wrote it) and one written without norm_obs."""
    d = tmp_path_factory.mktemp("obs_norm_ckpt")
    tr = _pendulum(norm_obs=True, obs_clip=5.0)
    for _ in range(2):
        tr.step()
    path = tr.save_checkpoint(str(d / "model-Pendulum-2"))
    plain = _pendulum(norm_obs=False)
    plain.step()
    plain_path = plain.save_checkpoint(str(d / "plain" / "model-Pendulum-1"))
    return dict(path=path, trainer=tr, plain=plain_path, plain_trainer=plain)


def test_checkpoint_tensors_are_fp64(bundle):
    from actor_critic_algs_on_tensorflow_amd.ckpt import load_tensors
    t = load_tensors(bundle["path"])
    norm = bundle["trainer"].obs_norm
    for k, ref in (("count", norm.count), ("mean", norm.mean), ("m2", norm.m2)):
        got = np.asarray(t["_acamd/obs_norm/" + k])
        assert got.dtype == np.float64 and np.array_equal(got.reshape(-1), ref.numpy().reshape(-1)), k
    assert float(t["_acamd/obs_norm/clip"]) == 5.0
    assert not any(k.startswith("_acamd/obs_norm/") for k in load_tensors(bundle["plain"]))


def test_checkpoint_resume_is_bitwise(bundle):
    whole = _pendulum(norm_obs=True, obs_clip=5.0)
    for _ in range(4):
        whole.step()
    resumed = _pendulum(norm_obs=True, obs_clip=5.0)
    resumed.load_checkpoint(bundle["path"])
    assert torch.equal(resumed.obs_norm.state, bundle["trainer"].obs_norm.state)
    assert torch.equal(resumed.obs_norm.tables, bundle["trainer"].obs_norm.tables)
    for _ in range(2):
        resumed.step()
    assert torch.equal(resumed.flat.data, whole.flat.data)
    assert torch.equal(resumed.obs_norm.state, whole.obs_norm.state)
    assert torch.equal(resumed.obs_norm.tables, whole.obs_norm.tables)


def test_checkpoint_without_tensors(bundle):
    with pytest.raises(KeyError, match="_acamd/obs_norm/count"):
        _pendulum(norm_obs=True).load_checkpoint(bundle["plain"])
    tr = _pendulum(norm_obs=False)
    tr.load_checkpoint(bundle["plain"])
    assert tr.obs_norm is None and torch.equal(tr.flat.data, bundle["plain_trainer"].flat.data)


# ------------------------------------------------------------------------------------------------ 6. Agent
def test_agent_from_checkpoint_normalises_and_stays_frozen(bundle):
    from actor_critic_algs_on_tensorflow_amd.api import Agent
    agent = Agent.from_checkpoint(bundle["path"], "Pendulum-v0")
    norm = agent.obs_norm
    src = bundle["trainer"].obs_norm
    assert norm is not None and norm.frozen and norm.clip == 5.0
    assert torch.equal(norm.state, src.state) and torch.equal(norm.tables, src.tables)
    g = torch.Generator().manual_seed(3)
    obs = torch.randn(9, 3, generator=g) * torch.tensor([1.0, 1.0, 8.0])
    state = norm.state.clone(), norm.tables.clone()
    for _ in range(5):
        a, logp, ent = agent.act(obs.numpy(), deterministic=True)
    keys = torch.arange(9, dtype=torch.int64)
    ra, rlogp, rent, _ = agent.model.act(norm.apply(obs), keys=keys, seed=agent.seed, deterministic=True)
    assert np.array_equal(a, ra.numpy()) and np.array_equal(logp, rlogp.numpy()) and np.array_equal(ent, rent.numpy())
    with torch.no_grad():
        assert np.array_equal(agent.value(obs.numpy()), agent.model.value(norm.apply(obs)).numpy())
        assert not np.array_equal(agent.value(obs.numpy()), agent.model.value(obs).numpy())
    sampled = agent.act(obs.numpy())[0]
    assert sampled.shape == a.shape
    assert torch.equal(norm.state, state[0]) and torch.equal(norm.tables, state[1])
    norm.prepare(obs, torch.empty_like(obs), 9)
    norm.merge()
    assert torch.equal(norm.state, state[0]), "a frozen normaliser applies and never merges"
    assert Agent.from_checkpoint(bundle["plain"], "Pendulum-v0").obs_norm is None


# ------------------------------------------------------------------------------------------------ 7. gloo world 2
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


DP_KW = dict(num_envs=2, n_steps=12, ppo_epochs=2, ppo_minibatches=2, seed=5, norm_obs=True)


def _dp_worker(rank, world, port, out_dir):
    import torch.distributed as dist
    from actor_critic_algs_on_tensorflow_amd.parallel.dp import DataParallel
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    tr = ActorCriticTrainer(preset("pendulum_ppo", **_quiet(**DP_KW)), dp=DataParallel())
    log = spy(tr)
    states = []
    for _ in range(2):
        tr.step()
        states.append(tr.obs_norm.state.clone())
    torch.save({"p": tr.flat.data.clone(), "state": tr.obs_norm.state.clone(), "tables": tr.obs_norm.tables.clone(),
                "rows": log["rows"], "states": states}, os.path.join(out_dir, f"n{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_dp_gloo_world2(tmp_path):
    """Both ranks hold bitwise-identical normaliser state and parameters. The state equals one normaliser fed, update by
    update, the union of both ranks' recorded raw rollouts (and numpy's statistics of all of them); after update 0,
    whose rollouts do not depend on the learner, it also equals a single-process trainer over the same 4 envs."""
    world = 2
    mp.spawn(_dp_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    out = [torch.load(tmp_path / f"n{r}.pt", weights_only=True) for r in range(world)]
    for k in ("p", "state", "tables"):
        assert torch.equal(out[0][k], out[1][k]), k
    Dn = 3
    union = ObsNormalizer(Dn)
    seen = []
    for u in range(2):
        rows = torch.cat([out[r]["rows"][u].reshape(-1, Dn) for r in range(world)])
        union.prepare(rows, torch.empty_like(rows), rows.shape[0])
        union.merge()
        seen.append(rows)
        assert float(union.count[0]) == float(out[0]["states"][u][0])
        np.testing.assert_allclose(out[0]["states"][u].numpy(), union.state.numpy(), rtol=1e-10, atol=1e-12)
    dp_norm = ObsNormalizer(Dn)
    dp_norm.load_state_dict(dict(count=out[0]["state"][0:1], mean=out[0]["state"][1:1 + Dn],
                                 m2=out[0]["state"][1 + Dn:]))
    assert torch.equal(dp_norm.tables, out[0]["tables"])
    check_state(dp_norm, torch.cat(seen), "world 2")
    single = ActorCriticTrainer(preset("pendulum_ppo", **_quiet(**dict(DP_KW, num_envs=2 * world))))
    single.step()
    one = ObsNormalizer(Dn)
    one.load_state_dict(dict(count=out[0]["states"][0][0:1], mean=out[0]["states"][0][1:1 + Dn],
                             m2=out[0]["states"][0][1 + Dn:]))
    check_state(one, seen[0], "update 0, world 2")
    check_state(single.obs_norm, seen[0], "update 0, single process")
