"""Seeded cases shared by tests/test_mlp_towers_cpu.py and tests/test_gpu_mlp_towers.py: the custom-tower models, their
inputs and the fp64 oracle's tower lists. Everything is drawn on the CPU from fixed seeds, so the CPU file can check
properties of the inputs (the arg-max gap cap, the planted saturation) that the GPU file relies on."""
import numpy as np
import torch

from actor_critic_algs_on_tensorflow_amd.models.policy import MLPActorCritic

# the smallest tower lists at which each mechanism of the generic kernel can go wrong
TOWERS = [(8,), (24, 24), (48, 32), (64, 64), (256, 16), (32, 16, 16, 8)]
HEADS = [("categorical", 2), ("categorical", 3), ("gaussian", 1), ("gaussian", 6)]
DIMS = (3, 17, 51)
BATCHES = (1, 16, 17, 33)
GAP = 1e-4          # greedy categorical rows below this fp64 top-two logit gap are left out ...
GAP_CAP = 0.05      # ... and at most this share of the rows may be


def critic_of(actor_hidden):
    """Actor and critic take different lists in every case: the critic gets the next list."""
    return TOWERS[(TOWERS.index(tuple(actor_hidden)) + 1) % len(TOWERS)]


def set_a():
    """Every tower list x tanh at one (D, head, B)."""
    return [dict(actor=t, critic=critic_of(t), act="tanh", D=17, head=("gaussian", 6), batches=(17,), ppo=True,
                 saturate=True) for t in TOWERS]


def set_b():
    """Every (D, head) x the batches, on (48, 32) tanh (one all-pad column tile)."""
    return [dict(actor=(48, 32), critic=critic_of((48, 32)), act="tanh", D=D, head=h, batches=BATCHES,
                 ppo=h[0] == "gaussian", saturate=False) for D in DIMS for h in HEADS]


def set_c():
    """relu / lrelu on two lists."""
    return [dict(actor=t, critic=critic_of(t), act=a, D=17, head=h, batches=(17,), ppo=False, saturate=False)
            for t, h in (((24, 24), ("categorical", 3)), ((64, 64), ("gaussian", 6))) for a in ("relu", "lrelu")]


def case_id(c):
    return "{}-{}-{}-D{}-{}{}".format("x".join(map(str, c["actor"])), "x".join(map(str, c["critic"])), c["act"],
                                      c["D"], c["head"][0][:3], c["head"][1])


def build(c, seed=0):
    """The case's model on the CPU: random biases (the initialisers leave them zero), a spread log-std and, with
    ``saturate``, first-layer columns scaled so that hidden tanh outputs are exactly +-1.0f in some columns (tanhf
    rounds to 1 from |z| ~ 9) and near 0 in others."""
    g = torch.Generator().manual_seed(1000 + seed)
    kind, A = c["head"]
    disc = kind == "categorical"
    m = MLPActorCritic(c["D"], A, disc, None if disc else np.full(A, 2.0, np.float32), "basic", generator=g,
                       actor_hidden=c["actor"], critic_hidden=c["critic"], hidden_act=c["act"])
    with torch.no_grad():
        for tower in (m.actor, m.critic):
            for lay in tower.hidden_layers + [tower.out_layer]:
                lay.bias.copy_(0.1 * torch.randn(lay.bias.shape, generator=g))
            if c["saturate"]:
                W = tower.hidden_layers[0].kernel
                n = W.shape[1]
                scale = torch.ones(n)
                scale[0::3] = 200.0     # |z| far above 9 on nearly every row: tanhf(z) == +-1.0f, derivative 0
                scale[1::3] = 0.01      # |z| ~ 0.01: tanh in its linear range, derivative ~ 1
                W.mul_(scale)
        if not disc:
            m.actor.log_std.copy_(torch.linspace(-0.7, 0.4, A))
    return m


def towers_of(m):
    """The oracle's tower lists of a model: fp32 parameters as numpy, the top layer's activation ``None``."""
    out = []
    for tower in (m.actor, m.critic):
        lays = tower.hidden_layers
        out.append([(l.kernel.detach().cpu().numpy(), l.bias.detach().cpu().numpy(), l.activation) for l in lays]
                   + [(tower.out_layer.kernel.detach().cpu().numpy(), tower.out_layer.bias.detach().cpu().numpy(),
                       None)])
    return out


def head_kw(m):
    if m.discrete:
        return {}
    return dict(log_std=m.actor.log_std.detach().cpu().numpy(), ac_scale=m.actor.ac_scale.cpu().numpy())


def inputs(c, B, seed=0):
    """Observations, actions and the loss inputs of one batch, as float32 / int numpy arrays."""
    r = np.random.RandomState(7000 + 131 * seed + B + 17 * c["D"])
    kind, A = c["head"]
    obs = r.randn(B, c["D"]).astype(np.float32)
    if kind == "gaussian":
        act = (2.0 * np.tanh(r.randn(B, A)) + 0.3 * r.randn(B, A)).astype(np.float32)
    else:
        act = r.randint(0, A, size=B).astype(np.int32)
    return dict(obs=obs, act=act, lo_noise=(0.3 * r.randn(B)).astype(np.float32), adv=r.randn(B).astype(np.float32),
                ret_noise=r.randn(B).astype(np.float32), vo_noise=(0.1 * r.randn(B)).astype(np.float32))
