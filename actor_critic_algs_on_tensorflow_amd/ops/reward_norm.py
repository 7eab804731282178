"""Running return-based reward scaling for the MLP engines (``TrainConfig.norm_reward``; the reward half of Baselines'
``VecNormalize``): the rewards of a rollout are divided by the running standard deviation of the per-env discounted
return and clipped, ``r = clip(r / sqrt(var(R) + eps), +-c)``. No mean is subtracted.

State, on the device, fp64: ``ret[N]``, the per-env running discounted return (it carries across updates and is local
to each data-parallel rank), and ``count, mean, m2`` of every return seen -- exactly :class:`ObsNormalizer`'s state
with ``D = 1``, which this class composes for the state, the fp32 tables (``mean32``, ``istd32``; the identity (0, 1)
while ``count == 0``), the merge, data parallelism and ``state_dict``.

Per update, after the rollout has written the raw ``rewards [T, N]`` (fp32) and ``dones [T, N]`` (uint8; a time-limit
cut is a done):

1. :meth:`scan` -- for every env ``e``, ``t = 0 .. T-1`` in order, in fp64 without contraction: ``R = R * gamma +
   r[t, e]`` (a multiply, then an add), ``d = R - mean``, ``S1_e += d``, ``S2_e += d * d``, then ``R = 0`` where
   ``done[t, e]``. ``mean`` is the running mean from before this update; ``ret[e] = R`` is stored back; one partial row
   ``(S1_e, S2_e)`` per env; the rewards are not modified.
2. :meth:`merge` -- the ``N`` partial rows are summed in a fixed order into the additive batch vector ``[S1, S2, nb = T
   N]``, all-reduced (sum) under data parallelism, and merged by the rule of ``ops/obs_norm.py`` (Chan et al.): the
   ``obs_norm_merge`` launch with ``D = 1``.
3. :meth:`apply_` -- in place, fp32: ``r = min(max(r * istd32, -clip), clip)``; ``istd32`` is read from device memory.

The statistics include the rollout they scale, as in ``VecNormalize``, which updates before it normalises: the very
first update already trains on unit-scale rewards, and a run is invariant to the bank's reward unit up to ``eps``. This
differs from ``norm_obs``, whose tables must stay frozen while the policy acts; rewards never feed the policy, so
nothing forces that here. A bootstrap term ``gamma V(terminal observation)`` is in the critic's units, which are
already scaled: the scan sees the raw env reward only, and the trainer adds the term after step 3.

On a GPU :meth:`scan` / :meth:`apply_` are the kernels of ``csrc/kernels/reward_norm.hip`` (bit-equal to the torch
forms below, which are their oracle and the CPU / torch-engine path). Every buffer is allocated by the constructor,
outside graph capture, and nothing synchronises with the host.
"""
from __future__ import annotations

import torch

from .. import _native
from .obs_norm import ObsNormalizer


def scan_unroll():
    """Time steps per load round of ``reward_norm_scan_kernel`` (``RWN_UNROLL``): rollouts shorter than, equal to and
    longer than it take different paths through the kernel."""
    return int(_native.require().reward_norm_unroll())


class RewardNormalizer:
    def __init__(self, N, gamma, clip=10.0, eps=1e-8, device="cpu"):
        self.N, self.gamma = int(N), float(gamma)
        if self.N < 1:
            raise ValueError(f"RewardNormalizer needs N >= 1, got N={N}")
        self.stats = ObsNormalizer(1, clip, eps, device)   # (validates clip > 0)
        self.device = self.stats.device
        self.ret = torch.zeros(self.N, dtype=torch.float64, device=self.device)
        self.part = torch.zeros(self.N, 2, dtype=torch.float64, device=self.device)   # (S1_e, S2_e) of the last scan
        self.stats._part = self.part.view(-1)   # the partial rows of the D = 1 merge

    # the D = 1 statistics, by name
    clip = property(lambda self: self.stats.clip)
    eps = property(lambda self: self.stats.eps)
    frozen = property(lambda self: self.stats.frozen)
    state = property(lambda self: self.stats.state)
    tables = property(lambda self: self.stats.tables)
    batch = property(lambda self: self.stats.batch)
    count = property(lambda self: self.stats.count)
    mean = property(lambda self: self.stats.mean)
    m2 = property(lambda self: self.stats.m2)
    mean32 = property(lambda self: self.stats.mean32)
    istd32 = property(lambda self: self.stats.istd32)

    def _check(self, rewards, dones=None):
        if rewards.dim() != 2 or rewards.shape[1] != self.N or rewards.shape[0] < 1:
            raise ValueError(f"RewardNormalizer: rewards must be [T >= 1, {self.N}], got {tuple(rewards.shape)}")
        if dones is not None and tuple(dones.shape) != tuple(rewards.shape):
            raise ValueError("RewardNormalizer: dones must have the rewards' shape")

    # ------------------------------------------------------------------------------------------- the three steps
    def scan(self, rewards, dones):
        """Step 1; leaves the partial rows pending for :meth:`merge`. A frozen normaliser scans nothing."""
        self._check(rewards, dones)
        if self.frozen:
            return
        T = rewards.shape[0]
        if _native.use_native(rewards):
            _native.require().reward_norm_scan(rewards, dones, self.ret, self.state, self.part, self.gamma)
            self.stats._pending = (self.N, float(T * self.N))
            return
        self.scan_torch(rewards, dones)
        self.batch.copy_(self.batch_from_parts(T))
        self.stats._pending = (None, float(T * self.N))

    def scan_torch(self, rewards, dones):
        """The oracle of ``reward_norm_scan_kernel``: a loop over ``T`` on fp64 ``[N]`` vectors, one rounding per
        written operation (torch contracts nothing)."""
        R = self.ret.clone()
        mean = self.mean[0].clone()
        S1, S2 = torch.zeros_like(R), torch.zeros_like(R)
        zero = torch.zeros_like(R)
        for t in range(rewards.shape[0]):
            R = R * self.gamma + rewards[t].to(torch.float64)
            d = R - mean
            S1 = S1 + d
            S2 = S2 + d * d
            R = torch.where(dones[t] != 0, zero, R)
        self.ret.copy_(R)
        self.part[:, 0].copy_(S1)
        self.part[:, 1].copy_(S2)

    def batch_from_parts(self, T):
        """``[S1, S2, nb]`` of the last scan, torch (the oracle of the merge launch's stage 0 up to the summation
        order)."""
        nb = torch.full((1,), float(T * self.N), dtype=torch.float64, device=self.device)
        return torch.cat([self.part.sum(0), nb])

    def merge(self, dp=None, comm=None):
        """Step 2: :meth:`ObsNormalizer.merge` with ``D = 1`` (one launch on one rank; under data parallelism the
        batch vector is all-reduced between its two stages, through ``comm``)."""
        self.stats.merge(dp, comm)

    def apply_(self, rewards):
        """Step 3, in place."""
        self._check(rewards)
        if _native.use_native(rewards):
            _native.require().reward_norm_apply(rewards, self.tables.view(-1), self.clip)
            return rewards
        return rewards.mul_(self.istd32).clamp_(-self.clip, self.clip)

    def update_(self, rewards, dones, dp=None, comm=None):
        """The three steps in order: the statistics include the rollout they scale."""
        self.scan(rewards, dones)
        self.merge(dp, comm)
        return self.apply_(rewards)

    # ------------------------------------------------------------------------------------------- persistence
    def freeze(self):
        """The normaliser applies and never scans or merges."""
        self.stats.freeze()
        return self

    def state_dict(self):
        """``count, mean, m2, clip, gamma`` as fp64 tensors: identical on every data-parallel rank. ``ret`` is per
        rank and handled apart (checkpoints store it beside the env-bank tensors; :meth:`load_state_dict` takes it
        when given)."""
        sd = self.stats.state_dict()
        sd["gamma"] = torch.tensor(self.gamma, dtype=torch.float64)
        return sd

    def load_state_dict(self, sd):
        """The constructor's ``gamma`` and ``clip`` stay: ``gamma`` is also the discount of the trainer's returns, and
        running returns accumulated under another discount mean nothing under this one, so a stored ``gamma`` that
        differs is refused; ``clip`` shapes no state, and a stored value that differs is ignored."""
        missing = [k for k in ("count", "mean", "m2") if k not in sd]
        if missing:
            raise KeyError(f"RewardNormalizer.load_state_dict: missing {missing}")
        if "gamma" in sd:
            gamma = float(torch.as_tensor(sd["gamma"], dtype=torch.float64).reshape(-1)[0])
            if gamma != self.gamma:
                raise ValueError(f"RewardNormalizer.load_state_dict: statistics of returns discounted by gamma={gamma}, "
                                 f"this normaliser discounts by {self.gamma}")
        self.stats.load_state_dict({k: v for k, v in sd.items() if k in ("count", "mean", "m2")})
        if "ret" in sd:
            ret = torch.as_tensor(sd["ret"], dtype=torch.float64).reshape(-1)
            if ret.numel() != self.N:
                raise ValueError(f"RewardNormalizer.load_state_dict: returns of {ret.numel()} envs, this normaliser "
                                 f"has {self.N}")
            self.ret.copy_(ret)
        return self
