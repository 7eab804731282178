"""The fp64 returns oracle (tests/oracles/returns_oracle.py) checked without a GPU, on the input sets the GPU tests of
tests/test_gpu_returns.py use: against the PyTorch oracles of ops/returns.py and the reference's ``PathAdv``; the
derived tolerances against numpy transcriptions of the kernels' own arithmetic (the six fp32 loops; the scan's
algorithm in fp64); the planted terminals against the scan geometry they are meant to sit on."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "oracles"))
import returns_oracle as O  # noqa: E402

from test_returns_scan import _emulate  # noqa: E402

from actor_critic_algs_on_tensorflow_amd.ops import returns as R  # noqa: E402


def _simple_as_cases():
    out = []
    for T, N, g, lm, dn in O.simple_cases():
        out.append((T, N, "gae", None, g, lm, dn, "randn"))
        out += [(T, N, "nstep", L, g, lm, dn, "randn") for L in O.simple_windows(T)]
    return out


def _head_as_cases():
    out = []
    for shapes in (O.HEAD_SHAPES, O.ENV_SHAPES, O.LOSS_SHAPES):
        for T, N, mode, L, g, lm, dn in O.head_cases(shapes):
            out.append((T, N, "nstep" if mode == 1 else "gae", L, g, lm, dn, "randn"))
    return list(dict.fromkeys(out))


ALL_CASES = list(dict.fromkeys(O.scan_cases() + _simple_as_cases() + _head_as_cases()))


def _max_ratio(err, tol):
    """max err / tol; an element with zero tolerance must have zero error."""
    err, tol = np.broadcast_arrays(np.asarray(err, dtype=np.float64), np.asarray(tol, dtype=np.float64))
    zero = tol == 0
    assert (err[zero] == 0).all()
    return float((err[~zero] / tol[~zero]).max()) if (~zero).any() else 0.0


def test_oracle_agrees_with_the_pytorch_oracles_on_every_input_set():
    """targets() == gae_ref / nstep_returns_ref within those refs' fp32 output rounding plus the effect of their
    unrounded gamma / lambda: a term k steps away carries gamma^k (lam^k), so rounding the two moves it by
    k (|dg| / g + |dl| / l) relatively; fp64 evaluation adds 8 roundings per step."""
    for case in ALL_CASES:
        T, N, mode, L, g, lm, dn, vs = case
        r, v, d, ret, adv, M = O.case_data(*case)
        LL = T if L is None else L
        tr, tv, td = torch.from_numpy(r.copy()), torch.from_numpy(v.copy()), torch.from_numpy(d.copy())
        ro, ao = R.gae_ref(tr, tv, td, g, lm) if mode == "gae" else R.nstep_returns_ref(tr, tv, td, g, LL)
        g32, l32 = float(np.float32(g)), float(np.float32(lm))
        rel = (abs(g - g32) / g32 if g32 else 0.0) + (abs(lm - l32) / l32 if l32 and mode == "gae" else 0.0)
        steps = O.steps_behind(mode, T, N, LL)
        for got, want, m in ((ro, ret, M["ret"]), (ao, adv, M["adv"])):
            tol = O.U32 * np.abs(want) + ((steps + 1) * rel + 8 * (steps + 1) * O.U64) * m
            assert _max_ratio(np.abs(got.double().numpy() - want), tol) <= 1.0, case


@pytest.mark.parametrize("L", [1, 5, 36, 37, 40])
@pytest.mark.parametrize("terminal", [False, True])
def test_oracle_agrees_with_path_adv_on_single_episodes(L, terminal):
    r, v, _ = O.rollout(37, 19, "none", "randn")
    g32 = float(np.float32(0.98))
    for n in (0, 7):
        d = np.zeros((37, 1), dtype=np.uint8)
        d[36, 0] = 1 if terminal else 0
        ret, adv, M = O.targets(r[:, n:n + 1], v[:, n:n + 1], d, "nstep", 0.98, 0.0, L)
        tg, ad = R.path_adv(r[:, n], v[:, n], terminal, g32, L)
        steps = O.steps_behind("nstep", 37, 1, L)
        assert _max_ratio(np.abs(np.array(tg)[:, None] - ret), 8 * (steps + 1) * O.U64 * M["ret"]) <= 1.0
        assert _max_ratio(np.abs(np.array(ad)[:, None] - adv), 8 * (steps + 1) * O.U64 * M["adv"]) <= 1.0


def test_fp32_transcriptions_stay_inside_the_derived_bound_on_every_input_set():
    """The six fp32 loops (gae_kernel, nstep_kernel, and the GAE / n-step loops of ac_loss, head_bwd, a2c_head,
    a2c_head_env) in numpy fp32, one rounding per operation: inside (6 steps + 4) u M everywhere, on every input set
    of the GPU tests. The worst fraction of the bound is printed (python -m pytest -s)."""
    worst = {}
    for case in ALL_CASES:
        T, N, mode, L, g, lm, dn, vs = case
        r, v, d, ret, adv, M = O.case_data(*case)
        LL = T if L is None else L
        steps = O.steps_behind(mode, T, N, LL)
        for head in (False, True):
            re, ae = O.emulate_fp32(r, v, d, mode, g, lm, LL, head=head)
            assert re.dtype == np.float32 and ae.dtype == np.float32
            for name, got, want, m in (("ret", re, ret, M["ret"]), ("adv", ae, adv, M["adv_head" if head else "adv"])):
                ratio = _max_ratio(np.abs(got.astype(np.float64) - want), O.tolerance("fp32", steps, m))
                assert ratio <= 1.0, (case, head, name, ratio)
                key = (mode, "head" if head else "simple")
                worst[key] = max(worst.get(key, 0.0), ratio)
    print("fp32 transcription, worst error / bound:", {k: round(x, 4) for k, x in worst.items()})
    assert max(worst.values()) > 0.0   # the transcription does round: the comparison is not vacuous


def test_scan_emulation_stays_inside_the_scan_tolerance_on_the_planted_sets():
    """The scan's algorithm (test_returns_scan._emulate: chunk maps -> suffix scan -> replay, window form) in fp64
    stays inside the fp64 part of the scan tolerance, k 2^-53 M_full, and its fp32 rounding inside the whole of it."""
    for case in O.scan_cases():
        T, N, mode, L, g, lm, dn, vs = case
        if dn != "planted":
            continue
        r, v, d, ret, adv, M = O.case_data(*case)
        LL = T if L is None else L
        CH = O.geometry(T, N)[1]
        g32, l32 = float(np.float32(g)), float(np.float32(lm))
        re, ae = _emulate(r.astype(np.float64), v.astype(np.float64), d, mode, g32, l32, LL, CH)
        for got, want, m in ((re, ret, M["scan_ret"]), (ae, adv, M["scan_adv"])):
            assert _max_ratio(np.abs(got - want), O.tolerance("scan", M=m, value=0.0 * want, T=T)) <= 1.0, case
            got32 = got.astype(np.float32).astype(np.float64)
            assert _max_ratio(np.abs(got32 - want), O.tolerance("scan", M=m, value=want, T=T)) <= 1.0, case


def test_geometry_of_the_shape_table():
    """The reasons the shape table gives for its shapes hold for the restated geometry."""
    assert O.geometry(1, 1)[1:3] == (1, 1) and O.geometry(8, 3)[1:3] == (1, 8)
    assert O.geometry(9, 5) == (128, 2, 5, 1) and O.geometry(9, 129) == (128, 2, 5, 2)   # 5 and 1 live envs of 128
    assert O.geometry(37, 19)[1:3] == (8, 5)
    assert O.geometry(2048, 2)[1:3] == (256, 8)      # the last register shape (K <= 8)
    assert O.geometry(2049, 3)[1:3] == (256, 9)      # the first global-path shape
    assert O.geometry(4100, 2)[1:3] == (256, 17)
    assert (9 * 5) % 4 and (2049 * 3) % 4 and (9 * 129) % 4       # scalar normalisation
    assert (4100 * 2) % 4 == 0 and (37 * 19) % 4                  # vector normalisation on the global path


def test_planted_sets_contain_the_terminals_they_claim():
    seen_window = 0
    shapes = {(c[0], c[1], c[3] if c[2] == "nstep" else None) for c in ALL_CASES if c[6] == "planted"}
    for T, N, L in sorted(shapes, key=str):
        d, cl = O.planted(T, N, L)
        K = O.geometry(T, N)[2]
        assert cl["K"] == K
        want = sorted({t for t in (0, K - 1, K, T - 1) if 0 <= t < T})
        assert sorted(t for t, n in cl["base"] if n == 0) == want
        assert all(d[t, n] == 1 for t, n in cl["base"])
        assert d[0, 0] == 1 and d[T - 1, 0] == 1
        if K < T:
            # the last step of chunk 0 and the first step of chunk 1 of the kernel's chunking (t0 = ch * K)
            assert d[K - 1, 0] == 1 and d[K, 0] == 1 and (K - 1) // K == 0 and K // K == 1
        for i, t in enumerate(want):
            if 3 + i < N:
                assert d[:, 3 + i].sum() == 1 and d[t, 3 + i] == 1
        if L is not None and L < T and N >= 3:
            ts = cl["tstar"]
            assert ts is not None and 0 <= ts and ts + L <= T - 1
            assert cl["inside"] == (ts + L - 1, 1) and cl["outside"] == (ts + L, 2)
            # the only terminal of env 1 is the window's last step; the only one of env 2 the first step outside it
            assert d[:, 1].sum() == 1 and d[ts + L - 1, 1] == 1
            assert d[:, 2].sum() == 1 and d[ts + L, 2] == 1
            # and the oracle does treat them differently: env 1's window is cut (no bootstrap), env 2's is not
            r, v, _ = O.rollout(T, N, "planted", "randn", L)
            ret, _, _ = O.targets(r, v, d, "nstep", 1.0, 0.0, L)
            np.testing.assert_allclose(ret[ts, 1], r[ts:ts + L, 1].astype(np.float64).sum(), rtol=1e-12)
            np.testing.assert_allclose(ret[ts, 2], r[ts:ts + L, 2].astype(np.float64).sum() + float(v[ts + L, 2]),
                                       rtol=1e-12)
            seen_window += 1
        else:
            assert cl["inside"] is None and cl["outside"] is None
    assert seen_window >= 8


def test_stats_against_numpy_and_the_torch_forms():
    r, v, d, ret, adv, M = O.case_data(37, 19, "gae", None, 0.99, 0.95, "random", "offset")
    ret32, adv32 = ret.astype(np.float32), adv.astype(np.float32)
    st = O.stats(ret32, adv32, v[:37])
    from actor_critic_algs_on_tensorflow_amd.utils.stats import var_accounted_for_tensor
    ev_t = float(var_accounted_for_tensor(torch.from_numpy(ret32), torch.from_numpy(v[:37].copy())))
    assert abs(st["ev"] - ev_t) < 1e-4                        # the fp32 torch form, at mean 100 / spread 2
    assert abs(st["ev"] - np.corrcoef(ret32.reshape(-1).astype(np.float64),
                                      v[:37].reshape(-1).astype(np.float64))[0, 1]) < 1e-12
    na = R.normalize_advantages(torch.from_numpy(adv32)).numpy().reshape(-1)
    np.testing.assert_allclose(na, st["norm"], rtol=1e-4, atol=1e-5)   # the fp32 torch form
    assert st["mom"][0] == 37 * 19 and abs(st["mom"][1] - adv32.astype(np.float64).sum()) < 1e-9
    z = O.stats(np.zeros(6, np.float32), np.zeros(6, np.float32), np.zeros(6, np.float32))
    assert np.isnan(z["ev"]) and (z["norm"] == 0).all()


@pytest.mark.parametrize("L", [0, -3])
@pytest.mark.parametrize("mode", ["nstep", "gae"])
def test_returns_scan_cpu_refuses_a_window_below_one(L, mode):
    r, v, d = (torch.from_numpy(x.copy()) for x in O.rollout(9, 5))
    ret_out, adv_out = torch.full((9, 5), 7.0), torch.full((9, 5), 7.0)
    with pytest.raises(ValueError, match="look_ahead must be >= 1"):
        R.returns_scan(r, v, d, mode, 0.99, 0.95, look_ahead=L, ret_out=ret_out, adv_out=adv_out)
    assert (ret_out == 7.0).all() and (adv_out == 7.0).all()
