"""fp64 oracle of the deterministic evaluation (algos/evaluator.py): fp64 copies of the actor layers plus fp64 dynamics
of the MuJoCo-shaped bank, on the identical ``envs/rng.py`` counter draws (the 24-bit uniforms are exact in fp32 and
widened), and the crafted reward / done columns the record-scan tests share. Nothing here looks at a kernel's output.

Tolerances are never fixed in advance: a GPU path is held to 8 x the measured error of the fp32 CPU torch evaluator
against this oracle on the same bank (``tests/test_gpu_sampling.py``'s rule).
"""
from __future__ import annotations

import torch

from actor_critic_algs_on_tensorflow_amd.envs import rng
from actor_critic_algs_on_tensorflow_amd.envs.mujoco import ACT_DIM, OBS_DIM, make_dynamics


# ------------------------------------------------------------------------------------------------ the actor, fp64
def actor_layers(model):
    a = model.actor
    return [a.first_layer, a.second_layer, a.third_layer, a.logits if a.discrete else a.mu_layer]


def actor_fp64(model, obs, tables=None, clip=None):
    """fp64 head input of the actor for the raw observations ``obs`` [B, D]: the logits (categorical) or the mean
    ``tanh(y) * ac_scale`` (Gaussian). ``tables`` [2, D] fp32 (mean32, istd32) + ``clip``: observation normaliser."""
    x = obs.detach().cpu().double()
    if tables is not None:
        t = tables.detach().cpu().double()
        x = ((x - t[0]) * t[1]).clamp(-float(clip), float(clip))
    for lay in actor_layers(model):
        y = x @ lay.kernel.detach().cpu().double() + lay.bias.detach().cpu().double()
        if lay.activation == "lrelu":
            y = torch.where(y > 0, y, 0.2 * y)
        elif lay.activation == "relu":
            y = y.clamp(min=0)
        elif lay.activation == "tanh":
            y = torch.tanh(y)
        x = y
    if model.discrete:
        return x
    return x * model.actor.ac_scale.detach().cpu().double()


def argmax_gap(z):
    """(first arg-max, top-1 minus top-2) of fp64 logits [B, A] (A >= 2)."""
    top = z.max(-1, keepdim=True).values
    act = (z == top).to(torch.int64).argmax(-1)
    t2 = torch.topk(z, 2, dim=-1).values
    return act, t2[:, 0] - t2[:, 1]


# ------------------------------------------------------------------------------------------------ the bank, fp64
def _u(seed, ids, tg, stream0, n):
    return torch.stack([rng.uniform(seed, ids, tg, stream0 + j) for j in range(n)], 1).double()


def run_linear(model, N, seed, frames, max_steps, E, tables=None, clip=None, dyn_seed=1234):
    """The whole evaluation of the MuJoCo-shaped bank in fp64: reset at tg = 0, ``E * max_steps`` steps of the actor's
    mean, records of the first ``E`` episodes per env. -> dict(ep_ret [N, E] fp64, ep_len [N, E], cnt [N], state
    [N, 17] fp64, t [N], tg [N])."""
    A_, B_ = make_dynamics(dyn_seed)
    A_, B_ = torch.as_tensor(A_).double(), torch.as_tensor(B_).double()
    seed = int(seed) & 0xFFFFFFFF
    ids = torch.arange(N, dtype=torch.int64)
    tg = torch.zeros(N, dtype=torch.int64)
    state = (_u(seed, ids, tg, 100, OBS_DIM) - 0.5) * 0.2
    obs = state.repeat(1, frames)
    t = torch.zeros(N, dtype=torch.int64)
    er = torch.zeros(N, dtype=torch.float64)
    ep_ret = torch.full((N, E), float("nan"), dtype=torch.float64)
    ep_len = torch.full((N, E), -1, dtype=torch.int64)
    cnt = torch.zeros(N, dtype=torch.int64)
    for _ in range(E * max_steps):
        a = actor_fp64(model, obs, tables, clip).clamp(-1.0, 1.0)
        tg = tg + 1
        state = state @ A_.t() + a @ B_.t() + (_u(seed, ids, tg, 300, OBS_DIM) - 0.5) * 0.02
        rew = state[:, 8] - 0.1 * (a * a).sum(1)
        t = t + 1
        er = er + rew
        done = t >= max_steps
        for i in torch.nonzero(done).view(-1).tolist():
            if cnt[i] < E:
                ep_ret[i, cnt[i]] = er[i]
                ep_len[i, cnt[i]] = t[i]
                cnt[i] += 1
        fresh = (_u(seed, ids, tg, 100, OBS_DIM) - 0.5) * 0.2
        state = torch.where(done.view(-1, 1), fresh, state)
        t = torch.where(done, torch.zeros_like(t), t)
        er = torch.where(done, torch.zeros_like(er), er)
        pushed = torch.cat([obs[:, OBS_DIM:], state], 1)
        obs = torch.where(done.view(-1, 1), state.repeat(1, frames), pushed)
    return dict(ep_ret=ep_ret, ep_len=ep_len, cnt=cnt, state=state, t=t, tg=tg)


# ------------------------------------------------------------------------------------------------ record scan
def scan_loop(rewards, dones, E):
    """Plain Python loop over the columns: (ep_ret [N, E] float32 with nan sentinels, ep_len [N, E] int32 with -1,
    cnt [N] int32). The adds are fp32, in step order."""
    L, N = rewards.shape
    ep_ret = torch.full((N, E), float("nan"), dtype=torch.float32)
    ep_len = torch.full((N, E), -1, dtype=torch.int32)
    cnt = torch.zeros(N, dtype=torch.int32)
    r32 = rewards.detach().cpu().to(torch.float32)
    d = dones.detach().cpu()
    for e in range(N):
        ret = torch.zeros((), dtype=torch.float32)
        ln = c = 0
        for t in range(L):
            ret = ret + r32[t, e]
            ln += 1
            if int(d[t, e]):
                if c < E:
                    ep_ret[e, c] = ret
                    ep_len[e, c] = ln
                    c += 1
                ret = torch.zeros((), dtype=torch.float32)
                ln = 0
        cnt[e] = c
    return ep_ret, ep_len, cnt


def crafted_columns(L, N, seed=0):
    """Reward / done columns [L, N] whose envs cover the record scan's edges: env 0 ends an episode at step 0 and at
    step L - 1, env 1 never finishes (cnt = 0, every slot stays a sentinel), env 2 finishes at every step (more than E
    episodes for any E < L), the others at random steps. Rewards are random with mixed magnitudes, so the fp32 sum
    depends on its order."""
    g = torch.Generator().manual_seed(1000 + 7 * L + N + seed)
    rewards = torch.randn(L, N, generator=g) * torch.tensor([1.0, 1e3, 1e-3])[torch.arange(N) % 3]
    dones = (torch.rand(L, N, generator=g) < 0.2).to(torch.uint8)
    dones[:, 0] = 0
    dones[0, 0] = 1
    dones[L - 1, 0] = 1
    if N > 1:
        dones[:, 1] = 0
    if N > 2:
        dones[:, 2] = 1
    return rewards.contiguous(), dones.contiguous()
