"""Oracles of PPO early stopping on the approximate KL (``TrainConfig.target_kl``).

* :func:`approx_kl64` -- the statistic in fp64: ``mean(expm1(x) - x)``, ``x = logp - logp_old``.
* :func:`threshold` -- the one float32 the trainer compares against, ``float32(1.5) * float32(target_kl)``.
* :func:`host_break` -- the stop rule as a HOST decision: a trainer built with ``target_kl=None`` whose
  ``_run_optimizers`` is wrapped. Before each minibatch step it reads the published ``approx_kl`` statistic back; once
  ``float32(approx_kl) > thr`` in an update, that step and the rest of the update skip the optimiser and zero the
  gradient slab instead. Needs an eager trainer (it reads the device every step) and, on the native MLP engine,
  ``engine_opts.adam_step_offsets=False`` (the step-ticket path, bitwise equal to the offsets path, counts the applied
  steps by itself).
* :func:`pick_threshold` -- a threshold that stops an update in its middle, from a probe run's ``kl_trace``.
"""
import numpy as np
import torch


def approx_kl64(logp, logp_old):
    x = logp.detach().double().cpu() - logp_old.detach().double().cpu()
    return float((torch.expm1(x) - x).mean())


def threshold(target_kl):
    return float(np.float32(1.5) * np.float32(target_kl))


def host_break(tr, thr):
    """Wraps ``tr._run_optimizers`` (``tr.cfg.target_kl`` is None). Returns the log: ``steps[u]`` = optimiser steps
    applied in update ``u``, ``kl[u]`` = the statistic read in front of every step of it (None once stopped)."""
    assert tr.cfg.target_kl is None and tr.cfg.algo == "ppo" and tr.graph is None
    if tr.mlp is not None:
        assert not tr.cfg.engine_opts.adam_step_offsets
    per = tr.cfg.ppo_epochs * tr.cfg.ppo_minibatches
    thr = np.float32(thr)
    log = dict(steps=[], kl=[], calls=0, stopped=False)
    run = tr._run_optimizers

    def wrapped():
        if log["calls"] % per == 0:
            log["stopped"] = False
            log["steps"].append(0)
            log["kl"].append([])
        log["calls"] += 1
        if not log["stopped"]:
            akl = np.float32(float(tr.stats["approx_kl"]))
            log["kl"][-1].append(float(akl))
            if akl > thr:   # strict; NaN compares false
                log["stopped"] = True
        else:
            log["kl"][-1].append(None)
        if log["stopped"]:
            tr.flat.grad.zero_()
            return
        log["steps"][-1] += 1
        run()

    tr._run_optimizers = wrapped
    return log


def pick_threshold(trace):
    """``trace``: the ``kl_trace`` of one update of a run that never stops. The first step ``j`` in ``[2, len - 2]``
    whose value exceeds the largest earlier one by >= 20 % gives ``thr`` = the geometric mean of the two: every earlier
    step passes and step ``j`` stops, each with ~9.5 % to spare. -> (j, thr); raises if the probe offers no such j."""
    t = [float(v) for v in trace]
    for j in range(2, len(t) - 1):
        prev = max(t[:j])
        if prev > 0 and t[j] >= 1.2 * prev:
            return j, float(np.sqrt(t[j] * prev))
    raise AssertionError(f"the probe's approximate KL never grows by 20 % inside [2, {len(t) - 2}]: {t}")


def optimizer_state(tr):
    """Everything an optimiser step changes: parameters, moments, Adam step counts."""
    out = [tr.flat.data.clone()]
    for g in sorted(tr.opts):
        o = tr.opts[g]
        out += [o.m.clone(), o.v.clone(), o.t.clone().reshape(1)]
    return out


def assert_state_equal(a, b, what=""):
    sa, sb = optimizer_state(a), optimizer_state(b)
    assert len(sa) == len(sb)
    for k, (x, y) in enumerate(zip(sa, sb)):
        assert torch.equal(x, y), f"{what}: optimiser state tensor {k} differs (max |d| = {float((x - y).abs().max())})"
