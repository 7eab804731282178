"""Configurable MLP towers (TrainConfig.actor_hidden / critic_hidden / hidden_act / mlp_init) without a GPU: the model
constructions, the config's refusals, the CLI flags, checkpoints through the TF-bundle codec, the fragment layouts the
GPU test compares against, the fp64 oracle against autograd, and the torch-engine trainer."""
import os
import sys

import numpy as np
import pytest
import torch

from actor_critic_algs_on_tensorflow_amd import ckpt
from actor_critic_algs_on_tensorflow_amd import envs as E
from actor_critic_algs_on_tensorflow_amd.api import Agent
from actor_critic_algs_on_tensorflow_amd.config import PRESETS, TrainConfig, preset
from actor_critic_algs_on_tensorflow_amd.models.layers import Dense
from actor_critic_algs_on_tensorflow_amd.models.policy import MLPActorCritic, build_model
from actor_critic_algs_on_tensorflow_amd.ops.mlp import frag_f, frag_g, ngp2

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "oracles"))
import mlp_tower_cases as C  # noqa: E402
import mlp_tower_oracle as O  # noqa: E402


# ------------------------------------------------------------------------------------------------ model
def _parent_model(ob, ac, disc, variant, seed):
    """The reference towers as the code before the tower fields built them: literal layers, the same initialiser calls
    in the same order (critic first), one generator."""
    g = torch.Generator().manual_seed(seed)
    c = [Dense(ob, 256, "relu", generator=g), Dense(256, 128, "relu", generator=g),
         Dense(128, 128, "relu", generator=g), Dense(128, 1, None, generator=g)]
    a = [Dense(ob, 128, "lrelu", generator=g), Dense(128, 128, "lrelu", generator=g),
         Dense(128, 64, "lrelu", generator=g)]
    if disc:
        a.append(Dense(64, ac, None, kernel_init="xavier" if variant == "basic" else "normc", generator=g))
    else:
        a.append(Dense(64, ac, "tanh", kernel_init="xav" if variant == "basic" else "xavier", generator=g))
    names = {}
    for scope, lays, ln in (("critic", c, ["first_layer", "second_layer", "third_layer", "value"]),
                            ("actor", a, ["first_layer", "second_layer", "third_layer",
                                          "logits" if disc else "mu_layer"])):
        for lay, n in zip(lays, ln):
            names[f"{scope}.{n}.kernel"] = lay.kernel
            names[f"{scope}.{n}.bias"] = lay.bias
    return names


@pytest.mark.parametrize("disc,variant", [(False, "basic"), (False, "a3c"), (True, "basic"), (True, "a3c")])
def test_defaults_build_the_parent_model(disc, variant):
    g = torch.Generator().manual_seed(5)
    m = MLPActorCritic(11, 3, disc, None if disc else np.full(3, 2.0, np.float32), variant, generator=g)
    want = _parent_model(11, 3, disc, variant, 5)
    got = dict(m.named_parameters())
    order = [n for n in got if n != "actor.log_std"]
    assert order == list(want), order   # same names, same order (critic before actor)
    for n in want:
        assert got[n].shape == want[n].shape and torch.equal(got[n], want[n]), n
    assert ("actor.log_std" in got) == (not disc)
    assert not m.custom_towers
    assert [l.out_features for l in m.actor.hidden_layers] == [128, 128, 64]
    assert [l.out_features for l in m.critic.hidden_layers] == ([256, 128, 128] if variant == "a3c" else [256, 128])
    # the forward reads what it read: the basic critic's value takes the second layer
    x = torch.randn(4, 11)
    c = m.critic
    h = c.second_layer(c.first_layer(x))
    assert torch.equal(m.value(x), c.value(c.third_layer(h) if variant == "a3c" else h).view(-1))


def test_build_model_defaults_equal_old_signature():
    env = E.make("Pendulum-v0", 1)
    a = build_model(env, "mlp", "a3c", seed=3)
    b = build_model(env, "mlp", "a3c", seed=3, **TrainConfig().mlp_kwargs())
    assert [n for n, _ in a.named_parameters()] == [n for n, _ in b.named_parameters()]
    for (n, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
        assert torch.equal(p, q), n


def test_custom_fields_build_the_stated_layers():
    env = E.make("Pendulum-v0", 1)
    m = build_model(env, "mlp", "basic", seed=1, actor_hidden=(64, 32), critic_hidden=(48,), hidden_act="tanh",
                    mlp_init="orthogonal")
    assert m.custom_towers
    assert [(l.in_features, l.out_features, l.activation) for l in m.actor.hidden_layers] == \
        [(3, 64, "tanh"), (64, 32, "tanh")]
    assert (m.actor.out_layer.in_features, m.actor.out_layer.out_features) == (32, 1)
    assert [(l.in_features, l.out_features, l.activation) for l in m.critic.hidden_layers] == [(3, 48, "tanh")]
    # the basic critic has no dead layer when custom
    assert sorted(n for n, _ in m.critic.named_parameters()) == ["hidden_0.bias", "hidden_0.kernel", "value.bias",
                                                                 "value.kernel"]
    assert not hasattr(m.critic, "third_layer") and not hasattr(m.actor, "first_layer")
    # orthogonal: W^T W = gain^2 I on the narrow side; zero biases
    W = m.actor.hidden_0.kernel.detach().double()
    torch.testing.assert_close(W @ W.t(), 2.0 * torch.eye(3, dtype=torch.float64), atol=1e-5, rtol=0)
    Wh = m.actor.mu_layer.kernel.detach().double()
    torch.testing.assert_close(Wh.t() @ Wh, 1e-4 * torch.eye(1, dtype=torch.float64), atol=1e-9, rtol=0)
    Wv = m.critic.value.kernel.detach().double()
    torch.testing.assert_close(Wv.t() @ Wv, torch.eye(1, dtype=torch.float64), atol=1e-5, rtol=0)
    assert all(float(p.detach().abs().max()) == 0 for n, p in m.named_parameters() if n.endswith("bias"))
    # hidden_act alone: the reference widths (value path only) with that activation, hidden_<i> names
    m2 = build_model(env, "mlp", "basic", seed=1, hidden_act="relu")
    assert [l.out_features for l in m2.actor.hidden_layers] == [128, 128, 64]
    assert [l.out_features for l in m2.critic.hidden_layers] == [256, 128]
    assert {l.activation for l in m2.actor.hidden_layers + m2.critic.hidden_layers} == {"relu"}
    # actor_hidden alone: the critic stays the reference construction, and None keeps the reference activations
    m3 = build_model(env, "mlp", "basic", seed=1, actor_hidden=(16,))
    assert m3.actor.custom and not m3.critic.custom and hasattr(m3.critic, "third_layer")
    assert m3.actor.hidden_0.activation == "lrelu" and m3.critic.first_layer.activation == "relu"
    # the forward is the plain chain
    x = torch.randn(5, 3)
    h = torch.tanh(x @ m.critic.hidden_0.kernel + m.critic.hidden_0.bias)
    torch.testing.assert_close(m.value(x), (h @ m.critic.value.kernel + m.critic.value.bias).view(-1))


# ------------------------------------------------------------------------------------------------ config
@pytest.mark.parametrize("kw,match", [
    (dict(actor_hidden=(40,)), "actor_hidden.*multiple of 16"),
    (dict(critic_hidden=(40, 16)), "critic_hidden.*multiple of 16"),
    (dict(actor_hidden=(8, 8, 8, 8, 8)), "actor_hidden.*1 to 4 hidden layers"),
    (dict(actor_hidden=()), "actor_hidden"),
    (dict(critic_hidden=(257,)), "critic_hidden.*1\\.\\.256"),
    (dict(actor_hidden=(0,)), "actor_hidden"),
    (dict(actor_hidden=(256, 256)), "actor_hidden.*MLP_PARTS = 256.*256 -> 256"),
    (dict(critic_hidden=(256, 256)), "critic_hidden.*MLP_PARTS"),
    (dict(actor_hidden="64,64"), "actor_hidden"),
    (dict(hidden_act="gelu"), "hidden_act"),
    (dict(mlp_init="he"), "mlp_init"),
    (dict(algo="a3c", hidden_act="tanh"), "hidden_act.*a3c"),
    (dict(algo="basic_ac", actor_hidden=(64,)), "actor_hidden.*basic_ac"),
    (dict(model="cnn", hidden_act="tanh"), "hidden_act.*cnn"),
    (dict(model="cnn", mlp_init="orthogonal"), "mlp_init.*cnn"),
])
def test_config_refusals_name_the_field(kw, match):
    with pytest.raises(ValueError, match=match):
        TrainConfig(**{"algo": "ppo", **kw})


def test_config_accepts_round_trips_and_presets():
    c = TrainConfig(algo="ppo", actor_hidden=[64, 64], critic_hidden=[256, 16], hidden_act="tanh",
                    mlp_init="orthogonal")
    assert c.actor_hidden == (64, 64) and c.critic_hidden == (256, 16) and c.custom_mlp
    assert TrainConfig(**c.to_dict()) == c
    import json
    assert TrainConfig(**json.loads(json.dumps(c.to_dict()))) == c   # lists come back as tuples
    d = TrainConfig()
    assert (d.actor_hidden, d.critic_hidden, d.hidden_act, d.mlp_init) == (None, None, None, "reference")
    assert not d.custom_mlp
    # the widest towers the slots allow; the torch engine has no limits
    TrainConfig(algo="ppo", critic_hidden=(256, 128, 128))
    TrainConfig(algo="a2c", engine="torch", actor_hidden=(40, 300), critic_hidden=(8,) * 6)
    p = preset("halfcheetah_ppo_tanh64")
    base = dict(PRESETS["mujoco_ppo_dp8"])
    assert (p.actor_hidden, p.critic_hidden, p.hidden_act, p.mlp_init) == ((64, 64), (64, 64), "tanh", "orthogonal")
    assert all(getattr(p, k) == v for k, v in base.items())


def test_cli_flags():
    from actor_critic_algs_on_tensorflow_amd.cli.run_ac import build_parser, config_from_args
    a = build_parser().parse_args("--algo ppo --preset pendulum_ppo --actor-hidden 64,64 --critic-hidden 32 "
                                  "--hidden-act tanh --mlp-init orthogonal".split())
    c = config_from_args(a)
    assert (c.actor_hidden, c.critic_hidden, c.hidden_act, c.mlp_init) == ((64, 64), (32,), "tanh", "orthogonal")
    c = config_from_args(build_parser().parse_args("--algo ppo --preset pendulum_ppo".split()))
    assert not c.custom_mlp
    with pytest.raises(SystemExit):
        build_parser().parse_args(["--actor-hidden", "64x64"])
    with pytest.raises(SystemExit):
        build_parser().parse_args(["--hidden-act", "gelu"])


def test_engine_limits_where_the_model_meets_the_engine():
    """MLPEngine.check_towers needs no device: the whole-tower limits that the config cannot know before the env."""
    from actor_critic_algs_on_tensorflow_amd.ops.mlp import MLPEngine
    mk = lambda ob, **kw: MLPActorCritic(ob, 2, False, np.full(2, 1.0, np.float32), "basic",
                                         generator=torch.Generator().manual_seed(0), **kw)
    tw = MLPEngine.check_towers(mk(17, actor_hidden=(64, 64), critic_hidden=(8,), hidden_act="tanh"))
    assert [[l.out_features for l in t] for t in tw] == [[64, 64, 2], [8, 1]]
    # 51 observations: 4 x 12 + 12 x 16 + 16 = 256 tiles fit a critic, and not a continuous actor (+1 for log_std)
    MLPEngine.check_towers(mk(51, critic_hidden=(192, 256)))
    with pytest.raises(ValueError, match="actor_hidden.*log_std.*MLP_PARTS"):
        MLPEngine.check_towers(mk(51, actor_hidden=(192, 256)))
    with pytest.raises(ValueError, match="critic_hidden.*multiple of 16"):
        MLPEngine.check_towers(mk(17, critic_hidden=(40,)))
    with pytest.raises(ValueError, match="actor_hidden.*1 to 4"):
        MLPEngine.check_towers(mk(17, actor_hidden=(8,) * 5))


# ------------------------------------------------------------------------------------------------ checkpoints
def _cfg(tmp_path, **kw):
    base = dict(algo="ppo", env="Pendulum-v0", model="mlp", num_envs=4, n_steps=8, ppo_epochs=2, ppo_minibatches=2,
                device="cpu", engine="torch", cuda_graph=False, outdir=None, quiet=True, stdout_freq=0, save_every=0,
                checkpoint_dir=str(tmp_path), returns="gae", norm_adv=True, lr=3e-3, critic_lr=3e-3)
    base.update(kw)
    return TrainConfig(**base)


def test_custom_checkpoint_round_trip(tmp_path):
    from actor_critic_algs_on_tensorflow_amd.algos.trainer import ActorCriticTrainer
    cfg = _cfg(tmp_path, actor_hidden=(24, 16), critic_hidden=(32,), hidden_act="tanh", mlp_init="orthogonal")
    tr = ActorCriticTrainer(cfg)
    tr.step()
    path = ckpt.save_trainer(tr)
    t = ckpt.load_tensors(path)
    model_keys = sorted(k for k in t if k.startswith("acamd_mlp/"))
    assert model_keys == sorted(
        [f"acamd_mlp/actor/hidden_{i}/{w}" for i in (0, 1) for w in ("kernel", "bias")]
        + [f"acamd_mlp/actor/mu_layer/{w}" for w in ("kernel", "bias")] + ["acamd_mlp/actor/log_std"]
        + [f"acamd_mlp/critic/hidden_0/{w}" for w in ("kernel", "bias")]
        + [f"acamd_mlp/critic/value/{w}" for w in ("kernel", "bias")])
    assert not any(k.startswith(("Actor/", "Critic/", "global_")) for k in t)
    assert ckpt.detect_variant(t.keys()) == "custom"
    for k, want in (("actor_hidden", [24, 16]), ("critic_hidden", [32])):
        a = np.array(t["_acamd/mlp_arch/" + k])
        assert a.dtype == np.int32 and a.reshape(-1).tolist() == want
    assert int(np.array(t["_acamd/mlp_arch/hidden_act"]).reshape(-1)[0]) == 3
    assert int(np.array(t["_acamd/mlp_arch/mlp_init"]).reshape(-1)[0]) == 1
    assert np.array(t["_acamd/mlp_arch/hidden_act"]).dtype == np.int32
    # Agent.from_checkpoint rebuilds the towers and acts as the source model does
    ag = Agent.from_checkpoint(path, "Pendulum-v0")
    assert ag.model.arch() == tr.model.arch()
    obs = np.random.RandomState(0).randn(9, 3).astype(np.float32)
    a, lp, _ = ag.act(obs, deterministic=True)
    a0, lp0, _, _ = tr.model.act(torch.as_tensor(obs), deterministic=True)
    assert np.array_equal(a, a0.numpy()) and np.array_equal(lp, lp0.numpy())
    # resume: the same architecture restores bit for bit, another one is refused with both named
    tr2 = ActorCriticTrainer(cfg.replace(resume=None))
    ckpt.load_trainer(tr2, path)
    assert torch.equal(tr2.flat.data, tr.flat.data)
    for g in tr.opts:
        assert torch.equal(tr2.opts[g].state_dict()["m"], tr.opts[g].state_dict()["m"])
    other = ActorCriticTrainer(_cfg(tmp_path, actor_hidden=(24, 24), critic_hidden=(32,), hidden_act="tanh"))
    with pytest.raises(ValueError, match=r"actor_hidden=\(24, 16\).*actor_hidden=\(24, 24\)"):
        ckpt.load_trainer(other, path)
    ref = ActorCriticTrainer(_cfg(tmp_path))
    with pytest.raises(ValueError, match="actor_hidden"):
        ckpt.load_trainer(ref, path)


def test_reference_checkpoint_keeps_the_parent_key_set(tmp_path):
    from actor_critic_algs_on_tensorflow_amd.algos.trainer import ActorCriticTrainer
    tr = ActorCriticTrainer(_cfg(tmp_path))
    path = ckpt.save_trainer(tr)
    t = ckpt.load_tensors(path)
    lay = lambda s, ns: [f"{s}/{n}/{w}" for n in ns for w in ("kernel", "bias")]
    model = set(lay("Actor", ["first_layer", "second_layer", "third_layer", "mu_layer"])
                + ["Actor/Variable", "Actor/Variable_1", "Actor/Variable_2", "Actor/Variable_3"]
                + lay("Critic", ["first_layer", "second_layer", "third_layer", "value"]) + ["Critic/Variable"])
    pnames = [n for n, _ in tr.model.named_parameters()]
    opt = set()
    for g, grp in (("actor", "actor."), ("critic", "critic.")):
        sd = tr.opts[g].state_dict()
        for k in sd:
            if k in ("m", "v"):
                opt |= {f"_acamd/opt/{g}/{k}/{n}" for n in pnames if n.startswith(grp)}
            else:
                opt.add(f"_acamd/opt/{g}/{k}")
    rest = {"_acamd/iteration", "_acamd/env_steps", "_acamd/world_size", "_acamd/update_counter", "_acamd/ent_coef",
            "_acamd/kl_coef"} | {f"_acamd/env/{k}" for k in ("state", "t", "tg", "ep_ret", "obs")}
    assert set(t) == model | opt | rest, sorted(set(t) ^ (model | opt | rest))
    assert ckpt.detect_variant(t.keys()) == "basic"
    # a bundle without the architecture keys loads into reference towers, and only there
    cust = ActorCriticTrainer(_cfg(tmp_path, hidden_act="tanh"))
    with pytest.raises(ValueError, match="hidden_act"):
        ckpt.load_trainer(cust, path)


# ------------------------------------------------------------------------------------------------ fragment layouts
@pytest.mark.parametrize("K,N", [(8, 8), (17, 24), (24, 48), (48, 32), (64, 64), (3, 8), (64, 6), (8, 1)])
def test_fragment_layouts_pad_with_zeros(K, N):
    """frag_f / frag_g written out element by element (common.h mlp_frag_f: column tile, k-group, lane = 16 q + r, 4
    consecutive k): W wherever (k, c) is inside the matrix, zero in the pad -- what the GPU test compares F / G with."""
    W = torch.arange(1, K * N + 1, dtype=torch.float32).reshape(K, N)   # no zero inside W
    for frag, M in ((frag_f, W), (frag_g, W.t())):
        Kk, Nn = M.shape
        gk, tn = ngp2(Kk), ngp2(Nn)
        out = frag(W)
        assert out.numel() == gk * tn * 256
        want = torch.zeros(tn, gk, 4, 16, 4)
        for tile in range(tn):
            for g in range(gk):
                for q in range(4):
                    for s in range(4):
                        k = 16 * g + 4 * q + s
                        c0 = 16 * tile
                        if k < Kk and c0 < Nn:
                            n = min(16, Nn - c0)
                            want[tile, g, q, :n, s] = M[k, c0:c0 + n]
        assert torch.equal(out, want.reshape(-1))
        assert int((out != 0).sum()) == K * N   # every element of W once, zero elsewhere


# ------------------------------------------------------------------------------------------------ oracle, inputs
def _oracle_case(c, B):
    m = C.build(c)
    ta, tc = C.towers_of(m)
    x = C.inputs(c, B)
    return m, ta, tc, x, C.head_kw(m)


@pytest.mark.parametrize("c", C.set_a()[2:4] + C.set_b()[1:3] + C.set_c()[:2], ids=C.case_id)
def test_oracle_agrees_with_the_package_autograd(c):
    """The oracle was written from the maths; the package's own fp32 modules and losses, differentiated by autograd,
    land within fp32 rounding of it (a loose, fixed bar: this guards the oracle, the GPU bars are measured)."""
    from actor_critic_algs_on_tensorflow_amd.algos import losses as L
    B = 17
    m, ta, tc, x, hk = _oracle_case(c, B)
    head = c["head"][0]
    fw = O.forward(ta, tc, head, x["obs"], x["act"], **hk)
    lo = (fw["logp"] + x["lo_noise"]).astype(np.float32)
    ret = (fw["value"] + x["ret_noise"]).astype(np.float32)
    vo = (fw["value"] + x["vo_noise"]).astype(np.float32)
    kw = dict(logp_old=lo, adv=x["adv"], ret=ret, v_old=vo, ppo=c["ppo"], beta=0.7, ent_coef=0.05, ppo_clip=0.2,
              v_clip=0.15 if c["ppo"] else 0.0)
    o = O.train(ta, tc, head, x["obs"], x["act"], **kw, **hk)
    T = torch.as_tensor
    logp, ent, v = m.evaluate(T(x["obs"]), T(x["act"]))
    if c["ppo"]:
        al, pg, kl, em, cf = L.ppo_actor_loss(logp, T(lo), T(x["adv"]), ent, 0.2, 0.05, 0.7)
    else:
        al, pg, kl, em = L.actor_loss(logp, T(lo), T(x["adv"]), ent, 0.7, 0.05)
        cf = torch.zeros(())
    cl = L.value_loss(v, T(ret), T(vo) if c["ppo"] else None, 0.15 if c["ppo"] else None)
    (al + cl).backward()
    np.testing.assert_allclose(logp.detach().numpy(), fw["logp"], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(v.detach().numpy(), fw["value"], rtol=1e-4, atol=1e-5)
    for name, tower, gs in (("actor", m.actor, o["grads_actor"]), ("critic", m.critic, o["grads_critic"])):
        for lay, (dW, db) in zip(tower.hidden_layers + [tower.out_layer], gs):
            sc = max(1e-6, float(np.abs(dW).max()))
            np.testing.assert_allclose(lay.kernel.grad.numpy(), dW, rtol=0, atol=2e-4 * sc, err_msg=name)
            np.testing.assert_allclose(lay.bias.grad.numpy(), db, rtol=0,
                                       atol=2e-4 * max(1e-6, float(np.abs(db).max())), err_msg=name)
    if head == "gaussian":
        np.testing.assert_allclose(m.actor.log_std.grad.numpy(), o["g_log_std"], rtol=1e-4, atol=1e-5)
    got = dict(pg=pg, kl=kl, entropy=em, crit_loss=cl, clipfrac=cf, act_loss=al)
    for n in O.STAT_NAMES:
        np.testing.assert_allclose(float(got[n].detach()), o["stats"][n], rtol=1e-4, atol=1e-5, err_msg=n)
    # the measurement helper reports every class, and the bars are never zero
    err, want = O.reference_error(ta, tc, head, x["obs"], x["act"], kw, **hk)
    assert set(err) == set(want) and all(np.isfinite(e) for e in err.values())
    assert all(b > 0 for k, b in O.bars(err, want).items() if np.abs(want[k]).max() > 0)


def test_planted_saturation_and_argmax_gap_cap():
    """What the GPU file relies on, from the fp64 oracle alone: the saturated cases have hidden tanh outputs that round
    to exactly +-1.0f and others near 0 (|y| < 0.35: the bias, derivative above 0.87); every categorical case keeps >= 95 % of its rows above the arg-max gap."""
    for c in C.set_a():
        m, ta, tc, x, hk = _oracle_case(c, 17)
        fw = O.forward(ta, tc, "gaussian", x["obs"], x["act"], **hk)
        for hid in (fw["hidden_actor"][0], fw["hidden_critic"][0]):
            y32 = hid.astype(np.float32)
            assert (np.abs(y32) == 1.0).mean() > 0.2 and (np.abs(y32) < 0.35).mean() > 0.2, C.case_id(c)
    n = 0
    for c in C.set_b() + C.set_c():
        if c["head"][0] != "categorical":
            continue
        for B in c["batches"]:
            m, ta, tc, x, hk = _oracle_case(c, B)
            gap = O.forward(ta, tc, "categorical", x["obs"], None)["gap"]
            out = int((gap < C.GAP).sum())
            assert out <= C.GAP_CAP * B, (C.case_id(c), B, out)
            n += 1
    assert n >= 24


# ------------------------------------------------------------------------------------------------ torch-engine trainer
def test_torch_engine_trains_tanh_towers(tmp_path):
    from actor_critic_algs_on_tensorflow_amd.algos.trainer import ActorCriticTrainer
    tr = ActorCriticTrainer(_cfg(tmp_path, actor_hidden=(64, 64), critic_hidden=(64, 64), hidden_act="tanh",
                                 mlp_init="orthogonal"))
    assert tr.mlp is None and tr.model.custom_towers
    assert [l.activation for l in tr.model.actor.hidden_layers] == ["tanh", "tanh"]
    p0 = tr.flat.data.clone()
    tr.step()
    p1 = tr.flat.data.clone()
    tr.step()
    assert torch.isfinite(tr.flat.data).all()
    assert (p1 != p0).any() and (tr.flat.data != p1).any()
    for tower in (tr.model.actor, tr.model.critic):
        for lay in tower.hidden_layers + [tower.out_layer]:
            s = sum(a.numel() for a in (lay.kernel, lay.bias))
            assert s and (lay.kernel.detach() != 0).any()
    # a model handed in with custom towers works the same way
    m = build_model(tr.env, "mlp", "basic", seed=2, actor_hidden=(16,), hidden_act="relu")
    tr2 = ActorCriticTrainer(_cfg(tmp_path), model=m)
    q0 = tr2.flat.data.clone()
    tr2.step()
    assert (tr2.flat.data != q0).any()


# ------------------------------------------------------------------------------------------------ optimiser item table
@pytest.mark.parametrize("K,N", [(48, 32), (256, 16), (51, 24), (17, 240), (64, 6), (32, 16)])
def test_optimizer_item_table_covers_wide_odd_weights(K, N):
    """FusedGroupStep.item_table on weights whose N is no multiple of 64 (custom widths): the records, walked as
    optim.hip's opt_items walks them, touch every element of the segment once and send element (k, c) of the weight to
    frag_f / frag_g's place for it; no record holds more than 1024 elements."""
    from types import SimpleNamespace
    from actor_critic_algs_on_tensorflow_amd.ops.optim import FusedGroupStep
    pre, post = 20, 7
    p = torch.zeros(pre + K * N + post)
    W = p[pre:pre + K * N]
    W.copy_(torch.arange(1, K * N + 1, dtype=torch.float32))
    F = torch.zeros(ngp2(K) * ngp2(N) * 256)
    G = torch.zeros_like(F)
    recs = FusedGroupStep.item_table(SimpleNamespace(p=p), [(W, K, N, F, G)]).tolist()
    seen = torch.zeros(p.numel(), dtype=torch.int32)
    Fo, Go = torch.zeros_like(F), torch.zeros_like(G)
    for typ, e0, n, n3, fp, gp, w6, w7 in recs:
        assert typ in (0, 2)
        tot = n if (typ == 0 or w7) else n * n3
        assert 0 < tot <= 1024
        seen[e0:e0 + tot] += 1
        if typ == 2:
            assert fp == F.data_ptr() and gp == G.data_ptr() and n3 == N
            Kf = w7 if w7 else n
            assert Kf == K
            for i in range(tot):
                o = w6 + i
                k, c = o // N, o % N
                fi = (((c >> 4) * ngp2(Kf) + (k >> 4)) * 64 + ((k >> 2) & 3) * 16 + (c & 15)) * 4 + (k & 3)
                gi = (((k >> 4) * ngp2(N) + (c >> 4)) * 64 + ((c >> 2) & 3) * 16 + (k & 15)) * 4 + (c & 3)
                Fo[fi] = p[e0 + i]
                Go[gi] = p[e0 + i]
    assert bool((seen == 1).all())
    Wm = W.view(K, N)
    assert torch.equal(Fo, frag_f(Wm)) and torch.equal(Go, frag_g(Wm))


# ------------------------------------------------------------------------------------------------ hidden_act=None
@pytest.mark.parametrize("towers", [dict(actor_hidden=(16,), critic_hidden=(16,)), dict(critic_hidden=(16,)),
                                    dict(actor_hidden=(16,))], ids=["both", "critic", "actor"])
def test_checkpoint_round_trip_with_widths_given_and_no_hidden_act(tmp_path, towers):
    """Widths given, ``hidden_act=None``: the actor stays lrelu and the critic relu, a tower whose widths were not given
    stays the reference construction, and the bundle says so -- the rebuilt model is the trained one (act, value),
    resume restores it bit for bit, and resume under a named activation with the same widths is refused."""
    from actor_critic_algs_on_tensorflow_amd.algos.trainer import ActorCriticTrainer
    cfg = _cfg(tmp_path, **towers)
    tr = ActorCriticTrainer(cfg)
    tr.step()
    assert tr.model.arch() == dict(actor_hidden=towers.get("actor_hidden"), critic_hidden=towers.get("critic_hidden"),
                                   hidden_act=None, mlp_init="reference")
    path = ckpt.save_trainer(tr)
    t = ckpt.load_tensors(path)
    assert int(np.array(t["_acamd/mlp_arch/hidden_act"]).reshape(-1)[0]) == 0
    assert np.array(t["_acamd/mlp_arch/tower_acts"]).reshape(-1).tolist() == [2, 1]   # lrelu actor, relu critic
    assert np.array(t["_acamd/mlp_arch/custom"]).reshape(-1).tolist() == [int("actor_hidden" in towers),
                                                                          int("critic_hidden" in towers)]
    assert ckpt.mlp_arch(t) == tr.model.arch()
    ag = Agent.from_checkpoint(path, "Pendulum-v0")
    assert ag.model.arch() == tr.model.arch()
    assert ag.model.actor.custom == ("actor_hidden" in towers) and ag.model.critic.custom == ("critic_hidden" in towers)
    assert [l.activation for l in ag.model.actor.hidden_layers] == ["lrelu"] * len(ag.model.actor.hidden_layers)
    assert [l.activation for l in ag.model.critic.hidden_layers] == ["relu"] * len(ag.model.critic.hidden_layers)
    for (n, p), (n2, q) in zip(tr.model.named_parameters(), ag.model.named_parameters()):
        assert n == n2 and torch.equal(p.detach(), q.detach()), n   # every parameter, a dead third layer included
    obs = np.random.RandomState(0).randn(9, 3).astype(np.float32)
    a, lp, _ = ag.act(obs, deterministic=True)
    a0, lp0, _, v0 = tr.model.act(torch.as_tensor(obs), deterministic=True)
    assert np.array_equal(a, a0.numpy()) and np.array_equal(lp, lp0.numpy())
    assert np.array_equal(ag.value(obs), v0.numpy())
    tr2 = ActorCriticTrainer(cfg)
    ckpt.load_trainer(tr2, path)
    assert torch.equal(tr2.flat.data, tr.flat.data)
    # the same widths under a named activation are another network
    named = dict(towers, hidden_act="lrelu")
    named.setdefault("actor_hidden", (128, 128, 64))
    named.setdefault("critic_hidden", (256, 128))
    with pytest.raises(ValueError, match="hidden_act"):
        ckpt.load_trainer(ActorCriticTrainer(_cfg(tmp_path, **named)), path)
    with pytest.raises(ValueError, match="hidden_act"):
        ckpt.load_trainer(ActorCriticTrainer(_cfg(tmp_path, **dict(towers, hidden_act="relu"))), path)
