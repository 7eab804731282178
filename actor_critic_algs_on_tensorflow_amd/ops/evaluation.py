"""Episode records of a deterministic evaluation (``algos/evaluator.py``) and their summary.

Records, on the device: ``ep_ret [N, E]`` float32, ``ep_len [N, E]`` int32 and ``cnt [N]`` int32 -- the returns and
lengths of the first ``E`` episodes every env of the evaluation bank finished, and how many it finished (at most
``E``). An episode's return is the fp32 sum of its rewards in step order, the bank's own ``ep_ret`` arithmetic. Slots an
env never filled keep their sentinels (``nan``, ``-1``); :meth:`EvalRecords.clear` puts them back at the start of every
evaluation.

:func:`eval_scan` fills the records from stored ``rewards [L, N]`` / ``dones [L, N]`` columns: on a GPU the
``eval_scan`` kernel (``csrc/kernels/eval_scan.hip``), elsewhere :func:`eval_scan_ref`, the torch form that is also the
kernel's oracle (bit-equal: same adds in the same order). The fused evaluation launch (``ops/mlp.py``
``rollout_eval_linear``) writes the same records itself.

:func:`summarize` is a handful of fp64 torch ops over the records in ``[N][E]`` order (capturable, no host sync):
``[mean, population std, min, max of the returns, mean length, episodes]``.
"""
from __future__ import annotations

import torch

from .. import _native

SUMMARY_KEYS = ("ret_mean", "ret_std", "ret_min", "ret_max", "len_mean", "episodes")
RET_SENTINEL = float("nan")
LEN_SENTINEL = -1


def scan_unroll():
    """Time steps per load round of ``eval_scan_kernel`` (``EVS_UNROLL``)."""
    return int(_native.require().eval_scan_unroll())


class EvalRecords:
    """The record buffers of one evaluator, allocated once (outside any graph capture)."""

    def __init__(self, N, E, device="cpu"):
        self.N, self.E = int(N), int(E)
        if self.N < 1 or self.E < 1:
            raise ValueError(f"EvalRecords needs N >= 1 and E >= 1, got N={N}, E={E}")
        self.device = torch.device(device)
        self.ep_ret = torch.empty(self.N, self.E, dtype=torch.float32, device=self.device)
        self.ep_len = torch.empty(self.N, self.E, dtype=torch.int32, device=self.device)
        self.cnt = torch.empty(self.N, dtype=torch.int32, device=self.device)
        self.summary = torch.zeros(len(SUMMARY_KEYS), dtype=torch.float64, device=self.device)
        self.clear()

    def clear(self):
        """Sentinels everywhere (device-side fills)."""
        self.ep_ret.fill_(RET_SENTINEL)
        self.ep_len.fill_(LEN_SENTINEL)
        self.cnt.zero_()

    def summarize(self):
        self.summary.copy_(summarize(self.ep_ret, self.ep_len, self.cnt))
        return self.summary

    def tensors(self):
        return self.ep_ret, self.ep_len, self.cnt


def eval_scan_ref(rewards, dones, ep_ret, ep_len, cnt):
    """Torch form of the record scan, the oracle of ``eval_scan_kernel`` and the CPU path: a loop over ``L`` on ``[N]``
    vectors. Per env, in step order: ``ret = ret + r`` (fp32), ``len += 1``; where done, the episode goes to slot
    ``cnt`` if ``cnt < E``, ``cnt += 1`` and ``ret = len = 0``. ``cnt`` is always written; slots from ``cnt`` on are
    left as they are."""
    L, N = rewards.shape
    E = ep_ret.shape[1]
    dev = rewards.device
    ret = torch.zeros(N, dtype=torch.float32, device=dev)
    ln = torch.zeros(N, dtype=torch.int32, device=dev)
    c = torch.zeros(N, dtype=torch.int64, device=dev)
    rows = torch.arange(N, device=dev)
    for t in range(L):
        ret = ret + rewards[t].to(torch.float32)
        ln = ln + 1
        d = dones[t] != 0
        w = d & (c < E)
        if w.device.type != "cpu" or bool(w.any()):
            slot = c.clamp(max=E - 1)
            ep_ret[rows, slot] = torch.where(w, ret, ep_ret[rows, slot])
            ep_len[rows, slot] = torch.where(w, ln, ep_len[rows, slot])
        c = c + w.to(torch.int64)
        ret = torch.where(d, torch.zeros_like(ret), ret)
        ln = torch.where(d, torch.zeros_like(ln), ln)
    cnt.copy_(c.to(torch.int32))
    return ep_ret, ep_len, cnt


def eval_scan(rewards, dones, ep_ret, ep_len, cnt):
    """Records from stored columns: the kernel on a GPU, :func:`eval_scan_ref` elsewhere."""
    if rewards.dim() != 2 or tuple(dones.shape) != tuple(rewards.shape) or rewards.shape[0] < 1:
        raise ValueError(f"eval_scan: rewards and dones must be [L >= 1, N], got {tuple(rewards.shape)} and "
                         f"{tuple(dones.shape)}")
    N = rewards.shape[1]
    if ep_ret.dim() != 2 or ep_ret.shape[0] != N or tuple(ep_len.shape) != tuple(ep_ret.shape) or cnt.numel() != N:
        raise ValueError("eval_scan: records must be ep_ret / ep_len [N, E] and cnt [N]")
    if _native.use_native(rewards):
        _native.require().eval_scan(rewards, dones, ep_ret, ep_len, cnt)
        return ep_ret, ep_len, cnt
    return eval_scan_ref(rewards, dones, ep_ret, ep_len, cnt)


def summarize(ep_ret, ep_len, cnt):
    """fp64 ``[mean, population std, min, max of the returns, mean length, episodes]`` over the recorded slots in
    ``[N][E]`` order. With every slot recorded (what the evaluator's step budget guarantees and its host read
    asserts) these are plain moments of ``ep_ret``."""
    E = ep_ret.shape[1]
    valid = torch.arange(E, device=ep_ret.device).unsqueeze(0) < cnt.unsqueeze(1)
    r = torch.where(valid, ep_ret.to(torch.float64), torch.zeros((), dtype=torch.float64, device=ep_ret.device))
    n = valid.sum().to(torch.float64)
    nn = n.clamp(min=1.0)
    mean = r.sum() / nn
    dev = torch.where(valid, r - mean, torch.zeros_like(r))
    std = ((dev * dev).sum() / nn).sqrt()
    inf = torch.full_like(r, float("inf"))
    rmin = torch.where(valid, r, inf).min()
    rmax = torch.where(valid, r, -inf).max()
    ln = torch.where(valid, ep_len.to(torch.float64), torch.zeros_like(r)).sum() / nn
    return torch.stack([mean, std, rmin, rmax, ln, n])
