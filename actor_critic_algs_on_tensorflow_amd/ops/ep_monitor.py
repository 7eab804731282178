"""Rolling window over the last ``K`` finished training episodes (``TrainConfig.ep_window``): kept and summarised on the
device in a fixed order, so it repeats bit for bit and costs no host read outside log time.

State, on the device, allocated by the constructor (outside graph capture):

* ``cur_ret[N]`` fp32, ``cur_len[N]`` int32 -- the unfinished episode of each env, carried across updates;
* ``ring_ret[K]`` fp32, ``ring_len[K]`` int32 -- the window; slot ``total mod K`` is written next;
* ``total`` int64[1] -- episodes ever finished; ``filled = min(total, K)``.

Per update, after the rollout wrote the raw ``rewards [T, N]`` (fp32) and ``dones [T, N]`` (uint8; a time-limit cut is
a done), before any reward scaling or bootstrap term, :meth:`update` does, in the flattened order ``i = t N + n`` (step
first, then env index)::

    cur_ret[n] = fp32(cur_ret[n] + r[t][n]);  cur_len[n] += 1
    if done[t][n]:
        ring_ret[total % K] = cur_ret[n];  ring_len[total % K] = cur_len[n];  total += 1
        cur_ret[n] = 0;  cur_len[n] = 0

The per-env add is a plain fp32 add in step order, the bank's own ``ep_ret`` arithmetic. If an update finishes more than
``K`` episodes only the last ``K`` survive. ``summary`` (fp64[10], :data:`SUMMARY_KEYS`) is recomputed by every update
over the filled slots: sums in fp64 of the fp32 / int32 entries, the standard deviation in two passes (population),
zeros where there is nothing to average. Nothing else is read or written.

On a GPU :meth:`update` is the two launches of ``csrc/kernels/ep_monitor.hip`` (the per-env scan, then a one-workgroup
commit that compacts the done column in memory order and reduces the summary; no atomics); :meth:`update_torch` is
their oracle and the CPU path. The state arrays agree exactly, the fp64 sums up to their summation order.
"""
from __future__ import annotations

import torch

from .. import _native

MAX_K = 4096
SUMMARY_KEYS = ("filled", "total", "ret_mean", "ret_std", "ret_min", "ret_max", "len_mean", "new", "new_ret_mean",
                "new_len_mean")
STATE_KEYS = ("cur_ret", "cur_len", "ring_ret", "ring_len", "total")


def scan_unroll():
    """Time steps per load round of ``ep_monitor_scan_kernel`` (``EPM_UNROLL``): rollouts shorter than, equal to and
    longer than it take different paths through the kernel."""
    return int(_native.require().ep_monitor_unroll())


class EpisodeMonitor:
    def __init__(self, N, K, device="cpu"):
        self.N, self.K = int(N), int(K)
        if self.N < 1:
            raise ValueError(f"EpisodeMonitor needs N >= 1, got N={N}")
        if not 1 <= self.K <= MAX_K:
            raise ValueError(f"EpisodeMonitor: the window K must be in 1 .. {MAX_K}, got K={K}")
        self.device = dev = torch.device(device)
        self.cur_ret = torch.zeros(self.N, dtype=torch.float32, device=dev)
        self.cur_len = torch.zeros(self.N, dtype=torch.int32, device=dev)
        self.ring_ret = torch.zeros(self.K, dtype=torch.float32, device=dev)
        self.ring_len = torch.zeros(self.K, dtype=torch.int32, device=dev)
        self.total = torch.zeros(1, dtype=torch.int64, device=dev)
        self.summary = torch.zeros(len(SUMMARY_KEYS), dtype=torch.float64, device=dev)
        self._ep_ret = self._ep_len = None   # the kernels' [T, N] scratch (reserve)

    def _check(self, rewards, dones):
        if rewards.dim() != 2 or rewards.shape[1] != self.N or rewards.shape[0] < 1:
            raise ValueError(f"EpisodeMonitor: rewards must be [T >= 1, {self.N}], got {tuple(rewards.shape)}")
        if tuple(dones.shape) != tuple(rewards.shape):
            raise ValueError("EpisodeMonitor: dones must have the rewards' shape")
        if rewards.dtype != torch.float32 or dones.dtype != torch.uint8:
            raise ValueError(f"EpisodeMonitor: rewards must be float32 and dones uint8, got {rewards.dtype} and "
                             f"{dones.dtype}")

    def reserve(self, T):
        """The kernels' scratch for rollouts of up to ``T`` steps: call before graph capture (the trainer does)."""
        cells = int(T) * self.N
        if self.device.type == "cuda" and (self._ep_ret is None or self._ep_ret.numel() < cells):
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("EpisodeMonitor: the scratch must be reserved before graph capture")
            self._ep_ret = torch.zeros(cells, dtype=torch.float32, device=self.device)
            self._ep_len = torch.zeros(cells, dtype=torch.int32, device=self.device)
        return self

    # ------------------------------------------------------------------------------------------- the update
    def update(self, rewards, dones):
        self._check(rewards, dones)
        if _native.use_native(rewards):
            self.reserve(rewards.shape[0])
            _native.require().ep_monitor_update(rewards, dones, self.cur_ret, self.cur_len, self.ring_ret,
                                                self.ring_len, self.total, self.summary, self._ep_ret, self._ep_len)
            return
        self.update_torch(rewards, dones)

    def update_torch(self, rewards, dones):
        """The oracle of the two kernels: a loop over ``T`` on fp32 ``[N]`` vectors (one rounding per add), then the
        finished episodes in flattened ``(t, n)`` order into their slots, then the summary. Reads the episode count on
        the host."""
        self._check(rewards, dones)
        T, K = rewards.shape[0], self.K
        cur, ln = self.cur_ret.clone(), self.cur_len.clone()
        ep_ret = torch.zeros(T, self.N, dtype=torch.float32, device=self.device)
        ep_len = torch.zeros(T, self.N, dtype=torch.int32, device=self.device)
        for t in range(T):
            cur = cur + rewards[t]
            ln = ln + 1
            d = dones[t] != 0
            ep_ret[t] = cur
            ep_len[t] = ln
            cur = torch.where(d, torch.zeros_like(cur), cur)
            ln = torch.where(d, torch.zeros_like(ln), ln)
        self.cur_ret.copy_(cur)
        self.cur_len.copy_(ln)
        idx = torch.nonzero(dones.reshape(-1) != 0).reshape(-1)   # ascending: the flattened (t, n) order
        C = int(idx.numel())
        new_ret, new_len = ep_ret.reshape(-1)[idx], ep_len.reshape(-1)[idx]
        total = int(self.total[0])
        if C:
            keep = min(C, K)   # the first C - K would be overwritten by this same update
            slots = (total + torch.arange(C - keep, C, device=self.device, dtype=torch.int64)) % K
            self.ring_ret[slots] = new_ret[C - keep:]
            self.ring_len[slots] = new_len[C - keep:]
        self.total.fill_(total + C)
        self._summarise_torch(new_ret, new_len)

    def _summarise_torch(self, new_ret=None, new_len=None):
        """``summary`` from the window (and this update's finished episodes), torch fp64."""
        total, K = int(self.total[0]), self.K
        filled = min(total, K)
        C = 0 if new_ret is None else int(new_ret.numel())
        s = torch.zeros(len(SUMMARY_KEYS), dtype=torch.float64)
        s[0], s[1], s[7] = filled, total, C
        if filled:
            x = self.ring_ret[:filled].to(torch.float64).cpu()
            mean = x.sum() / filled
            s[2] = mean
            s[3] = torch.sqrt(((x - mean) ** 2).sum() / filled)
            s[4], s[5] = x.min(), x.max()
            s[6] = self.ring_len[:filled].to(torch.float64).cpu().sum() / filled
        if C:
            s[8] = new_ret.to(torch.float64).sum() / C
            s[9] = new_len.to(torch.float64).sum() / C
        self.summary.copy_(s)

    # ------------------------------------------------------------------------------------------- reading
    def result(self):
        """The summary by name plus the window in chronological order, oldest first (numpy arrays). One host read of
        the summary, one of the window."""
        s = self.summary.detach().cpu().tolist()
        out = {k: (int(v) if k in ("filled", "total", "new") else float(v)) for k, v in zip(SUMMARY_KEYS, s)}
        filled, total, K = out["filled"], out["total"], self.K
        ret, ln = self.ring_ret.detach().cpu().numpy(), self.ring_len.detach().cpu().numpy()
        # once the ring has wrapped, the oldest entry sits in the slot written next
        order = [(total + i) % K for i in range(K)] if total > K else list(range(filled))
        out["returns"] = ret[order].copy()
        out["lengths"] = ln[order].copy()
        return out

    # ------------------------------------------------------------------------------------------- persistence
    def state_dict(self):
        """The five state arrays (per data-parallel rank: every rank keeps the window of its own envs)."""
        return {k: getattr(self, k).detach().clone() for k in STATE_KEYS}

    def load_state_dict(self, sd):
        """Bitwise. A ring of another ``K`` or a carry of another ``N`` is refused; the summary is recomputed from the
        loaded window (its ``new`` slots are zero until the next update)."""
        missing = [k for k in STATE_KEYS if k not in sd]
        if missing:
            raise KeyError(f"EpisodeMonitor.load_state_dict: missing {missing}")
        t = {k: torch.as_tensor(sd[k]).reshape(-1) for k in STATE_KEYS}
        if t["ring_ret"].numel() != self.K or t["ring_len"].numel() != self.K:
            raise ValueError(f"EpisodeMonitor.load_state_dict: a window of K={t['ring_ret'].numel()} episodes, this "
                             f"monitor keeps K={self.K}")
        if t["cur_ret"].numel() != self.N or t["cur_len"].numel() != self.N:
            raise ValueError(f"EpisodeMonitor.load_state_dict: episodes of {t['cur_ret'].numel()} envs, this monitor "
                             f"has {self.N}")
        for k in STATE_KEYS:
            dst = getattr(self, k)
            dst.copy_(t[k].to(dst.dtype))
        self._summarise_torch()
        return self
