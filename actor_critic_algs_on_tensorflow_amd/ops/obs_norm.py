"""Running observation normalisation for the MLP engines (``TrainConfig.norm_obs``; Baselines' ``VecNormalize``,
Brax's ``normalize_observations``): a running per-feature mean and variance of the RAW observations, applied in
front of both towers as ``clip((obs - mean) / sqrt(var + eps), +-c)``.

State, per engine, on the device, fp64 (one tensor ``state`` of ``1 + 2 D``): ``count``, ``mean[D]``, ``m2[D]`` (the sum
of squared deviations). Two fp32 tables are derived from it (``tables [2, D]``): ``mean32 = (float)mean`` and ``istd32 =
(float)(1 / sqrt(m2 / count + eps))``, computed in fp64 and then rounded; the identity (0, 1) while ``count == 0``.

Apply, in fp32: ``y = min(max((x - mean32[c]) * istd32[c], -clip), clip)`` -- exactly subtract, multiply, clamp (a
subtract feeding a multiply cannot contract into an fma, so the HIP kernels and torch round alike).

Batch statistics are additive, so data parallelism sums them: ``S1[c] = sum (x - mean[c])``, ``S2[c] = sum (x -
mean[c])^2`` about the current running mean, in fp64, and the row count ``nb`` (``batch [2 D + 1]``). Merge, with
``tot = count + nb`` and ``delta = S1 / nb``: ``mean += S1 / tot``; ``m2 += (S2 - S1^2 / nb) + delta^2 count nb /
tot``; ``count = tot``.

On a GPU :meth:`ObsNormalizer.prepare` / :meth:`merge` are the kernels of ``csrc/kernels/obs_norm.hip`` (fixed
reduction order, no floating-point atomics: bitwise reproducible); everywhere else the torch forms below, which are
their oracle. Nothing here synchronises with the host, and every buffer is allocated by the constructor or by
:meth:`reserve` -- outside graph capture.
"""
from __future__ import annotations

import torch

from .. import _native


class ObsNormalizer:
    def __init__(self, D, clip=10.0, eps=1e-8, device="cpu"):
        self.D, self.clip, self.eps = int(D), float(clip), float(eps)
        if self.D < 1 or not self.clip > 0:
            raise ValueError(f"ObsNormalizer needs D >= 1 and clip > 0, got D={D}, clip={clip}")
        self.device = torch.device(device)
        D = self.D
        self.state = torch.zeros(1 + 2 * D, dtype=torch.float64, device=self.device)
        self.count, self.mean, self.m2 = self.state[0:1], self.state[1:1 + D], self.state[1 + D:]
        self.tables = torch.zeros(2, D, dtype=torch.float32, device=self.device)
        self.mean32, self.istd32 = self.tables[0], self.tables[1]
        self.istd32.fill_(1.0)
        self.batch = torch.zeros(2 * D + 1, dtype=torch.float64, device=self.device)   # S1, S2, nb
        self.frozen = False
        self._part = None       # native: per-workgroup partial rows of the last prepare
        self._pending = None    # (partial rows, nb) of a prepare not merged yet; partial rows None: batch is final

    # ------------------------------------------------------------------------------------------- apply
    def apply(self, obs):
        """Out of place, torch: the oracle of every kernel that normalises, and the CPU / torch-engine path."""
        x = obs.to(torch.float32)
        return ((x - self.mean32) * self.istd32).clamp(-self.clip, self.clip)

    def kernel_args(self):
        """(tables, clip) operands of the native MLP launches."""
        return self.tables, self.clip

    # ------------------------------------------------------------------------------------------- statistics
    def reserve(self, R):
        """Allocates the native partial rows for ``R``-row prepares (call outside graph capture)."""
        if _native.use_native(self.state):
            n = int(_native.require().obs_norm_parts(int(R))) * 2 * self.D
            if self._part is None or self._part.numel() < n:
                if torch.cuda.is_current_stream_capturing():
                    raise RuntimeError("ObsNormalizer: the partial rows must be allocated before graph capture "
                                       "(reserve(R) / a warm-up prepare)")
                self._part = torch.zeros(n, dtype=torch.float64, device=self.device)

    def prepare(self, obs_rows, plane, r_stat):
        """``plane[R, D] = apply(obs_rows[R, D])`` and the batch statistics of the first ``r_stat`` rows about the
        running mean, left pending for :meth:`merge`. ``obs_rows`` may have a row stride; ``plane`` is contiguous."""
        R, D = obs_rows.shape
        r_stat = int(r_stat)
        if D != self.D or not 0 <= r_stat <= R or tuple(plane.shape) != (R, D):
            raise ValueError(f"ObsNormalizer.prepare: obs [R, {self.D}], plane alike, 0 <= r_stat <= R")
        if _native.use_native(obs_rows):
            self.reserve(R)
            ops = _native.require()
            ops.obs_norm_prepare(obs_rows, plane, self.tables, self.state, self._part, r_stat, self.clip)
            self._pending = (int(ops.obs_norm_parts(R)), float(r_stat))
            return plane
        plane.copy_(self.apply(obs_rows))
        self.batch.copy_(self.batch_stats(obs_rows[:r_stat]))
        self._pending = (None, float(r_stat))
        return plane

    def batch_stats(self, rows):
        """``[S1, S2, nb]`` of ``rows [n, D]`` about the current running mean, fp64, torch (the oracle of the native
        partial sums). Additive: the vectors of several row sets (data-parallel ranks) sum to the vector of their
        union."""
        d = rows.to(torch.float64) - self.mean
        nb = torch.full((1,), float(rows.shape[0]), dtype=torch.float64, device=d.device)
        return torch.cat([d.sum(0), (d * d).sum(0), nb])

    def merge(self, dp=None, comm=None):
        """Merges the pending batch statistics into the state and rewrites the tables. ``dp``: every rank all-reduces
        (sum) its ``batch`` first, so all ranks hold bitwise-identical state; ``comm(fn)`` issues that collective (the
        trainer's segment-cutting ``_comm``; default: call it now). A frozen normaliser never merges."""
        if self.frozen or self._pending is None:
            self._pending = None
            return
        nparts, nb = self._pending
        self._pending = None
        native = _native.use_native(self.state)
        if native:
            ops = _native.require()
            if dp is None:
                ops.obs_norm_merge(self._part, nparts, self.batch, nb, self.state, self.tables, 2, self.eps)
                return
            ops.obs_norm_merge(self._part, nparts, self.batch, nb, self.state, self.tables, 0, self.eps)
        if dp is not None:
            batch = self.batch
            fn = lambda: dp.allreduce_sum_(batch)
            fn() if comm is None else comm(fn)
        if native:
            _native.require().obs_norm_merge(None, 0, self.batch, 0.0, self.state, self.tables, 1, self.eps)
        else:
            self.merge_batch_()

    def merge_batch_(self):
        """Stage 1 in torch (the oracle of ``obs_norm_merge``): ``batch`` into the state, tables rewritten. No host
        read: an empty batch (``nb == 0``) leaves everything as it is through ``torch.where``."""
        D = self.D
        S1, S2, nb = self.batch[:D], self.batch[D:2 * D], self.batch[2 * D]
        count = self.count[0].clone()
        ok = nb > 0
        nbs = torch.where(ok, nb, torch.ones_like(nb))
        tot = count + nbs
        delta = S1 / nbs
        mean = self.mean + S1 / tot
        m2 = self.m2 + ((S2 - S1 * S1 / nbs) + delta * delta * count * nbs / tot)
        self.mean.copy_(torch.where(ok, mean, self.mean))
        self.m2.copy_(torch.where(ok, m2, self.m2))
        self.count.copy_(torch.where(ok, tot, count).reshape(1))
        mean32 = self.mean.to(torch.float32)
        istd32 = (1.0 / torch.sqrt(self.m2 / tot + self.eps)).to(torch.float32)
        self.mean32.copy_(torch.where(ok, mean32, self.mean32))
        self.istd32.copy_(torch.where(ok, istd32, self.istd32))

    def rebuild_tables(self):
        """Tables from the state (checkpoint load); one host read of ``count``."""
        if float(self.count[0]) > 0:
            self.mean32.copy_(self.mean.to(torch.float32))
            self.istd32.copy_((1.0 / torch.sqrt(self.m2 / self.count[0] + self.eps)).to(torch.float32))
        else:
            self.mean32.zero_()
            self.istd32.fill_(1.0)

    # ------------------------------------------------------------------------------------------- persistence
    def freeze(self):
        """Evaluation: the normaliser applies and never merges."""
        self.frozen = True
        return self

    def state_dict(self):
        return {"count": self.count.detach().cpu().clone().reshape(()), "mean": self.mean.detach().cpu().clone(),
                "m2": self.m2.detach().cpu().clone(), "clip": torch.tensor(self.clip, dtype=torch.float64)}

    def load_state_dict(self, sd):
        missing = [k for k in ("count", "mean", "m2") if k not in sd]
        if missing:
            raise KeyError(f"ObsNormalizer.load_state_dict: missing {missing}")
        as64 = lambda v: torch.as_tensor(v, dtype=torch.float64).reshape(-1)
        mean, m2 = as64(sd["mean"]), as64(sd["m2"])
        if mean.numel() != self.D or m2.numel() != self.D:
            raise ValueError(f"ObsNormalizer.load_state_dict: statistics of {mean.numel()} features, this normaliser "
                             f"has {self.D}")
        self.count.copy_(as64(sd["count"])[:1])
        self.mean.copy_(mean)
        self.m2.copy_(m2)
        if "clip" in sd:
            self.clip = float(as64(sd["clip"])[0])
        self._pending = None
        self.rebuild_tables()
        return self
