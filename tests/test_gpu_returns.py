"""Every return / advantage kernel against the one fp64 oracle of tests/oracles/returns_oracle.py, at its edges.

Kernels: ``gae_kernel`` (1), ``nstep_kernel`` (2), ``returns_scan_kernel`` (3: register and global path, full and
truncated window, moments, EV, in-place normalisation, aligned / unaligned / odd sizes) of returns.hip, and the
in-kernel returns of ``ac_loss`` (4: staged and unstaged), ``head_bwd`` (5), ``a2c_head`` (6) and ``a2c_head_env`` (7)
of loss.hip -- for 4-7 only ``ret_w``, ``adv_w`` and the EV in ``stats[7]``; their loss and gradient outputs are
pinned elsewhere and must merely be finite here. Every element is compared; every tolerance is derived in the oracle
module's docstring from the kernels' rounding points, none from a kernel output. Each test prints its largest error
as a fraction of the bound (``pytest -s``). Plus: the one-workgroup ``ev`` / ``moments`` / ``normalize`` kernels and
``mb_gather``'s deferred normalisation against ``stats()`` of their inputs; no entry point accepts a look-ahead below 1.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "oracles"))
import returns_oracle as O  # noqa: E402

from actor_critic_algs_on_tensorflow_amd.ops import returns as R  # noqa: E402

pytestmark = pytest.mark.gpu


def _ops():
    from actor_critic_algs_on_tensorflow_amd import _native
    return _native.require()


def _check(name, got, want, tol, what):
    """Every element of ``got`` within ``tol`` of ``want``; returns max err / tol (zero-tolerance elements: exact)."""
    got = np.asarray(got.detach().cpu().numpy() if torch.is_tensor(got) else got, dtype=np.float64)
    want, tol = np.broadcast_arrays(np.asarray(want, dtype=np.float64), np.asarray(tol, dtype=np.float64))
    got = got.reshape(want.shape)
    assert np.isfinite(got).all(), (name, what, "non-finite output")
    err = np.abs(got - want)
    bad = err > tol
    if bad.any():
        q = np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), np.where(err > 0, np.inf, 0.0))
        i = np.unravel_index(np.argmax(q), err.shape)
        raise AssertionError(f"{name} {what}: {int(bad.sum())} of {bad.size} elements outside the bound; worst at {i}: "
                             f"got {got[i]!r}, oracle {want[i]!r}, err {err[i]:.3e}, bound {tol[i]:.3e}")
    nz = tol > 0
    ratio = float((err[nz] / tol[nz]).max()) if nz.any() else 0.0
    print(f"returns-oracle ratio {name} {what} {ratio:.4f}")
    return ratio


def _dev(cuda, *arrays):
    return [torch.tensor(np.asarray(a)).to(cuda) for a in arrays]


def _same_or_both_nan(a, b):
    return torch.equal(a, b) or (bool(torch.isnan(a).all()) and bool(torch.isnan(b).all()))


# ------------------------------------------------------------------------------------------------ scan (kernel 3)


def _scan(cuda, r, v, d, mode, g, lm, L, norm, ws, adv_out=None):
    ev = torch.full((1,), 7.0, device=cuda)
    ret, adv, mom = R.returns_scan(r, v, d, mode, g, lm, look_ahead=L, norm=norm, ws=ws, ev_out=ev, adv_out=adv_out)
    torch.cuda.synchronize()
    return ret, adv, mom.clone(), ev


def _check_scan_stats(name, T, N, ret_g, adv_g, mom, ev, v):
    """EV and moments are functions of what the kernel wrote: compared with stats() of its own fp32 outputs."""
    st = O.stats(ret_g.cpu().numpy(), adv_g.cpu().numpy(), v[:T])
    m = mom.cpu().numpy()
    assert m[0] == T * N
    _check(name, m[:8], st["mom"], O.tolerance("mom", st=st), "mom")
    if np.isnan(st["ev"]):
        assert bool(torch.isnan(ev).all()), (name, "EV of a constant series must be NaN", ev)
    else:
        _check(name, ev, st["ev"], O.tolerance("ev", st=st), "ev")
    return st


@pytest.mark.parametrize("case", O.scan_cases(), ids=lambda c: "-".join(str(x) for x in c))
def test_returns_scan_matches_oracle(cuda, case):
    T, N, mode, L, g, lm, dn, vs = case
    r, v, d, ret, adv, M = O.case_data(*case)
    assert tuple(_ops().returns_scan_geometry(T, N)) == O.geometry(T, N)
    tr, tv, td = _dev(cuda, r, v, d)
    ws = R.ScanWorkspace(cuda, T, N)
    name = f"scan[{'reg' if O.geometry(T, N)[2] <= 8 else 'glob'}]"
    ret_g, adv_g, mom, ev = _scan(cuda, tr, tv, td, mode, g, lm, L, False, ws)
    _check(name, ret_g, ret, O.tolerance("scan", M=M["scan_ret"], value=ret, T=T), "ret")
    _check(name, adv_g, adv, O.tolerance("scan", M=M["scan_adv"], value=adv, T=T), "adv")
    st = _check_scan_stats(name, T, N, ret_g, adv_g, mom, ev, v)
    # fused in-place normalisation: same targets, same pre-normalisation moments and EV, normalised advantages
    ret_n, adv_n, mom_n, ev_n = _scan(cuda, tr, tv, td, mode, g, lm, L, True, ws)
    assert torch.equal(ret_n, ret_g) and torch.equal(mom_n, mom) and _same_or_both_nan(ev_n, ev)
    _check(name, adv_n, st["norm"].reshape(T, N), O.tolerance("norm", st=st).reshape(T, N), "norm")
    # a repeat launch is bitwise the same (fixed-order reductions, self-cleaning ticket)
    ret_2, adv_2, mom_2, ev_2 = _scan(cuda, tr, tv, td, mode, g, lm, L, True, ws)
    assert torch.equal(ret_2, ret_n) and torch.equal(adv_2, adv_n) and torch.equal(mom_2, mom_n)
    assert _same_or_both_nan(ev_2, ev_n)
    if vs == "zero":
        assert (ret_g == 0).all() and (adv_g == 0).all() and (adv_n == 0).all()
        assert bool(torch.isnan(ev).all()) and float(mom[0]) == T * N
        from actor_critic_algs_on_tensorflow_amd.utils.stats import var_accounted_for_tensor
        assert bool(torch.isnan(var_accounted_for_tensor(ret_g.reshape(-1), tv[:T].reshape(-1))))


@pytest.mark.parametrize("T,N,L", O.SCAN_FULL_EQUIV)
def test_returns_scan_window_past_the_end_is_the_whole_rollout(cuda, T, N, L):
    r, v, d, _, _, _ = O.case_data(T, N, "nstep", None, 0.99, 0.95, "planted", "randn")
    tr, tv, td = _dev(cuda, r, v, d)
    ws = R.ScanWorkspace(cuda, T, N)
    full = _scan(cuda, tr, tv, td, "nstep", 0.99, 0.95, None, False, ws)
    win = _scan(cuda, tr, tv, td, "nstep", 0.99, 0.95, L, False, ws)
    for a, b in zip(full, win):
        assert torch.equal(a, b)


def test_returns_scan_unaligned_adv_takes_the_scalar_normalisation(cuda):
    """T*N % 4 == 0 but ``adv_out`` starts one float into its buffer: the float4 normalisation must not be taken (it
    would need 16-byte alignment); the result equals the aligned launch bitwise and the guard floats are untouched."""
    T, N = 2048, 2
    case = (T, N, "gae", None, 0.99, 0.95, "planted", "randn")
    r, v, d, ret, adv, M = O.case_data(*case)
    tr, tv, td = _dev(cuda, r, v, d)
    ws = R.ScanWorkspace(cuda, T, N)
    _, adv_al, _, _ = _scan(cuda, tr, tv, td, "gae", 0.99, 0.95, None, True, ws)
    raw_g, adv_raw, _, _ = _scan(cuda, tr, tv, td, "gae", 0.99, 0.95, None, False, ws)
    buf = torch.full((T * N + 8,), 7.0, device=cuda)
    view = buf[1:1 + T * N]
    assert view.is_contiguous() and view.data_ptr() % 16 == 4 and (T * N) % 4 == 0
    _, adv_un, _, _ = _scan(cuda, tr, tv, td, "gae", 0.99, 0.95, None, True, ws, adv_out=view)
    assert adv_un.data_ptr() == view.data_ptr()
    assert torch.equal(adv_un, adv_al)
    assert float(buf[0]) == 7.0 and (buf[1 + T * N:] == 7.0).all()
    st = O.stats(raw_g.cpu().numpy(), adv_raw.cpu().numpy(), v[:T])
    _check("scan[reg]", adv_un, st["norm"].reshape(T, N), O.tolerance("norm", st=st).reshape(T, N), "norm-unaligned")


@pytest.mark.parametrize("T,N", [(9, 5), (128, 128)])
def test_normalize_mom_in_place_equals_out_of_place(cuda, T, N):
    case = (T, N, "gae", None, 0.99, 0.95, "random", "randn")
    r, v, d, ret, adv, M = O.case_data(*case)
    tr, tv, td = _dev(cuda, r, v, d)
    ws = R.ScanWorkspace(cuda, T, N)
    ret_g, adv_g, mom, _ = _scan(cuda, tr, tv, td, "gae", 0.99, 0.95, None, False, ws)
    out = torch.full_like(adv_g, 7.0)
    _ops().normalize_mom(adv_g, out, mom, 1e-8)
    inplace = adv_g.clone()
    _ops().normalize_mom(inplace, inplace, mom, 1e-8)
    torch.cuda.synchronize()
    assert torch.equal(inplace, out)
    st = O.stats(ret_g.cpu().numpy(), adv_g.cpu().numpy(), v[:T])
    _check("normalize_mom", inplace, st["norm"].reshape(T, N), O.tolerance("norm", st=st).reshape(T, N), "norm")


# ------------------------------------------------------------------------------------- simple kernels (1 and 2)


@pytest.mark.parametrize("T,N,g,lm,dn", O.simple_cases())
def test_gae_and_nstep_kernels_match_oracle(cuda, T, N, g, lm, dn):
    r, v, d, ret, adv, M = O.case_data(T, N, "gae", None, g, lm, dn)
    tr, tv, td = _dev(cuda, r, v, d)
    ret_g, adv_g = R.gae(tr, tv, td, g, lm)
    steps = O.steps_behind("gae", T, N, T)
    _check("gae_kernel", ret_g, ret, O.tolerance("fp32", steps, M["ret"]), "ret")
    _check("gae_kernel", adv_g, adv, O.tolerance("fp32", steps, M["adv"]), "adv")
    for L in O.simple_windows(T):
        r, v, d, ret, adv, M = O.case_data(T, N, "nstep", L, g, lm, dn)
        tr, tv, td = _dev(cuda, r, v, d)
        ret_g, adv_g = R.nstep_returns(tr, tv, td, g, L)
        steps = O.steps_behind("nstep", T, N, L)
        _check("nstep_kernel", ret_g, ret, O.tolerance("fp32", steps, M["ret"]), f"ret L={L}")
        _check("nstep_kernel", adv_g, adv, O.tolerance("fp32", steps, M["adv"]), f"adv L={L}")


# ------------------------------------------------------------------------------------- in-kernel returns (4 - 7)


def _head_operands(cuda, T, N, A):
    """The remaining operands of the head kernels, as tests/test_gpu_r3.py / test_gpu_r5.py build them."""
    A1, B = A + 1, T * N
    g = torch.Generator(device="cpu").manual_seed(T * 100 + N + A)
    return dict(z=torch.randn(B, A1, generator=g).to(cuda),
                act=torch.randint(0, A, (B,), dtype=torch.int32, generator=g).to(cuda),
                lpo=(-torch.rand(B, generator=g) * 2).to(cuda),
                h=torch.relu(torch.randn(B, 512, generator=g)).to(torch.bfloat16).to(cuda),
                Wh=(0.05 * torch.randn(512, A1, generator=g)).to(torch.bfloat16).to(cuda),
                ent=torch.tensor([0.01], device=cuda), kl=torch.tensor([0.3], device=cuda))


def _head_outs(cuda, B, A1):
    return dict(ret=torch.full((B,), 7.0, device=cuda), adv=torch.full((B,), 7.0, device=cuda),
                dh=torch.zeros(B, 512, dtype=torch.bfloat16, device=cuda), gWh=torch.zeros(512 * A1, device=cuda),
                gbh=torch.zeros(A1, device=cuda), gbfc=torch.zeros(512, device=cuda),
                stats=torch.full((8,), 7.0, device=cuda))


def _head_case(case):
    T, N, mode, L, g, lm, dn = case
    name = "nstep" if mode == 1 else "gae"
    r, v, d, ret, adv, M = O.case_data(T, N, name, L, g, lm, dn)
    return r, v, d, ret, adv, M, O.steps_behind(name, T, N, T if L is None else L), T if L is None else L


def _check_head(kernel, T, N, o, ret, adv, M, steps, v, ev=True):
    _check(kernel, o["ret"], ret.reshape(-1), O.tolerance("fp32", steps, M["ret"]).reshape(-1), "ret_w")
    _check(kernel, o["adv"], adv.reshape(-1), O.tolerance("fp32", steps, M["adv_head"]).reshape(-1), "adv_w")
    if ev:
        st = O.stats(o["ret"].cpu().numpy(), o["adv"].cpu().numpy(), v[:T])
        _check(kernel, o["stats"][7], st["ev"], O.tolerance("ev", st=st), "ev")


def _run_head_bwd_and_a2c_head(cuda, case, A, kernels):
    T, N, mode = case[:3]
    r, v, d, ret, adv, M, steps, L = _head_case(case)
    g, lm = case[4], case[5]
    A1, B = A + 1, T * N
    op = _head_operands(cuda, T, N, A)
    tr, tv, td = _dev(cuda, r, v, d)
    ops = _ops()
    for kernel in kernels:
        first = None
        for norm_adv in (False, True):
            o = _head_outs(cuda, B, A1)
            val = tv.clone()
            args = (op["z"], op["act"], op["lpo"], op["ent"], op["kl"], 0.5, tr, val, td, L, mode, norm_adv, g, lm,
                    o["ret"], o["adv"], op["h"], op["Wh"], o["dh"], o["gWh"], o["gbh"], o["gbfc"], o["stats"])
            if kernel == "head_bwd":
                ops.head_bwd(*args)
            else:
                ops.a2c_head(*args, None, 0, None, None, None)   # V(s_T) from val: no grid barrier
            torch.cuda.synchronize()
            assert torch.equal(val, tv)
            _check_head(kernel, T, N, o, ret, adv, M, steps, v)
            for k in ("dh", "gWh", "gbh", "gbfc", "stats"):
                assert torch.isfinite(o[k].float()).all(), (kernel, k)
            if first is None:
                first = o
            else:   # adv_w is written un-normalised whatever norm_adv says
                assert torch.equal(o["adv"], first["adv"]) and torch.equal(o["ret"], first["ret"])
                assert torch.equal(o["stats"][7], first["stats"][7])


@pytest.mark.parametrize("case", O.head_cases(O.HEAD_SHAPES), ids=lambda c: "-".join(str(x) for x in c))
def test_head_bwd_and_a2c_head_returns_match_oracle(cuda, case):
    _run_head_bwd_and_a2c_head(cuda, case, 6, ("head_bwd", "a2c_head"))


@pytest.mark.parametrize("A", [2, 7])
def test_head_bwd_returns_match_oracle_at_the_head_width_ends(cuda, A):
    _run_head_bwd_and_a2c_head(cuda, (5, 32, 1, 5, 0.99, 0.95, "planted"), A, ("head_bwd",))


@pytest.mark.parametrize("case", O.head_cases(O.ENV_SHAPES), ids=lambda c: "-".join(str(x) for x in c))
def test_a2c_head_env_returns_match_oracle(cuda, case):
    T, N, mode = case[:3]
    r, v, d, ret, adv, M, steps, L = _head_case(case)
    g, lm = case[4], case[5]
    A, A1, B = 6, 7, T * N
    op = _head_operands(cuda, T, N, A)
    tr, tv, td = _dev(cuda, r, v, d)
    o = _head_outs(cuda, B, A1)
    val = tv.clone()
    pWh, pbfc, pbh = (torch.full((N * n,), float("nan"), device=cuda) for n in (512 * A1, 512, A1))
    spart = torch.full((N, 10), float("nan"), dtype=torch.float64, device=cuda)
    _ops().a2c_head_env(op["z"], op["act"], op["lpo"], op["ent"], op["kl"], 0.5, tr, val, td, L, mode, g, lm, o["ret"],
                        o["adv"], op["h"], op["Wh"], o["dh"], None, 0, None, None, pWh, pbfc, pbh, spart)
    torch.cuda.synchronize()
    assert torch.equal(val, tv)
    _check_head("a2c_head_env", T, N, o, ret, adv, M, steps, v, ev=False)
    for x in (o["dh"].float(), pWh, pbfc, pbh, spart[:, :9]):   # 9 statistics per env row (the 10th slot is spare)
        assert torch.isfinite(x).all()


def _ac_loss(cuda, op, A, tr, val, td, L, mode, g, lm, norm_adv, o, dz, gbh):
    A1, B = A + 1, tr.numel()
    z = op["z"]
    _ops().ac_loss(z, A1, z[:, A:], A1, op["act"], None, None, op["lpo"], None, None, None, op["ent"], op["kl"], 0.5,
                   0.0, 0.0, dz, A1, dz[:, A:], A1, None, o["stats"], B, A, False, mode, tr, val, td, L, g, lm,
                   norm_adv, o["ret"], o["adv"], gbh)


@pytest.mark.parametrize("case", O.head_cases(O.LOSS_SHAPES), ids=lambda c: "-".join(str(x) for x in c))
def test_ac_loss_fused_returns_match_oracle(cuda, case):
    """Staged in LDS (B <= 2048 and N <= 256) and unstaged (the global scratch re-read after the block fence)."""
    T, N, mode = case[:3]
    r, v, d, ret, adv, M, steps, L = _head_case(case)
    g, lm = case[4], case[5]
    A, A1, B = 6, 7, T * N
    op = _head_operands(cuda, T, N, A)
    tr, tv, td = _dev(cuda, r, v, d)
    first = None
    for norm_adv in (False, True):
        o = _head_outs(cuda, B, A1)
        dz = torch.zeros(B, A1, dtype=torch.bfloat16, device=cuda)
        val = tv.clone()
        _ac_loss(cuda, op, A, tr, val, td, L, mode, g, lm, norm_adv, o, dz, o["gbh"])
        torch.cuda.synchronize()
        assert torch.equal(val, tv)
        _check_head("ac_loss[%s]" % ("staged" if B <= 2048 and N <= 256 else "unstaged"), T, N, o, ret, adv, M, steps,
                    v)
        assert torch.isfinite(dz.float()).all() and torch.isfinite(o["stats"]).all() and torch.isfinite(o["gbh"]).all()
        if first is None:
            first = o
        else:
            assert torch.equal(o["adv"], first["adv"]) and torch.equal(o["ret"], first["ret"])


# ------------------------------------------------- small statistics: one-workgroup ev / moments / normalize, mb_gather


@pytest.mark.parametrize("n", [5, 1025])   # a few threads; one element past the 1024-thread workgroup
def test_one_workgroup_ev_moments_and_normalize_match_oracle(cuda, n):
    """``ev_kernel`` (``ops.ev`` without a workspace), ``moments_kernel`` and ``normalize_kernel`` against
    ``stats()`` of their inputs, with the oracle's ``ev``, ``mom`` and ``norm`` tolerances. ``moments`` returns fp32:
    its fp64 sum lies within the ``mom`` tolerance of the oracle's and is then rounded once, and rounding is
    monotonic, so the output must lie between the fp32 roundings of the two ends of that interval."""
    rng = np.random.default_rng(n)
    x = rng.standard_normal(n).astype(np.float32)
    y = (np.float32(0.5) * x + rng.standard_normal(n).astype(np.float32)).astype(np.float32)
    st = O.stats(x, x, y)   # ret = adv = x, V = y
    tx, ty = _dev(cuda, x, y)
    ops = _ops()
    ev = torch.full((1,), 7.0, device=cuda)
    ops.ev(tx, ty, ev)
    _check("ev_kernel", ev, st["ev"], O.tolerance("ev", st=st), "ev")
    mom = torch.full((5,), 7.0, device=cuda)
    ops.moments(tx, ty, mom)
    want, tol = st["mom"][3:8], O.tolerance("mom", st=st)[3:8]   # sum x, x^2, y, y^2, x*y
    got = mom.cpu().numpy()
    lo, hi = (want - tol).astype(np.float32), (want + tol).astype(np.float32)
    print("returns-oracle moments_kernel", got, lo, hi)
    assert ((lo <= got) & (got <= hi)).all(), ("moments_kernel", got, lo, hi)
    out = torch.full((n,), 7.0, device=cuda)
    ops.normalize(tx, out, 1e-8)
    _check("normalize_kernel", out, st["norm"], O.tolerance("norm", st=st), "norm")
    assert torch.equal(tx.cpu(), torch.tensor(x)) and torch.equal(ty.cpu(), torch.tensor(y))


@pytest.mark.parametrize("index_mode", [True, False], ids=["index", "copy"])
@pytest.mark.parametrize("R", [16, 20], ids=["vector", "bytes"])   # 16 B vector copies; the byte loop
def test_mb_gather_deferred_normalisation_matches_oracle(cuda, R, index_mode):
    """``mb_gather_kernel`` with a ``mom`` tensor (advantage normalisation deferred from the returns scan), both
    modes: the gather is exact against the keyed permutation of envs/rng.py, the normalised advantages lie within
    the oracle's ``norm`` tolerance of ``stats()`` of the whole batch. The minibatch ends on the last batch row."""
    from actor_critic_algs_on_tensorflow_amd.envs import rng as prng
    n, mb, off, seed, ep = 33, 7, 26, 4242, 1
    rng = np.random.default_rng(R)
    obs = torch.tensor(rng.integers(0, 256, (n, R), dtype=np.uint8)).to(cuda)
    act = torch.tensor(rng.integers(0, 6, n, dtype=np.int32)).to(cuda)
    logp, adv, ret, v = (rng.standard_normal(n).astype(np.float32) for _ in range(4))
    adv = (adv * np.float32(3.0) + np.float32(1.0)).astype(np.float32)
    st = O.stats(ret, adv, v)
    fl = _dev(cuda, logp, adv, ret, v)
    mom = torch.tensor(st["mom"][:3], dtype=torch.float64).to(cuda)   # count, sum adv, sum adv^2
    uc = torch.tensor([3], dtype=torch.int64, device=cuda)
    o_act = torch.full((mb,), 7, dtype=torch.int32, device=cuda)
    o_fl = [torch.full((mb,), 7.0, device=cuda) for _ in range(4)]
    o_obs = None if index_mode else torch.full((mb, R), 7, dtype=torch.uint8, device=cuda)
    o_idx = torch.full((mb,), -1, dtype=torch.int64, device=cuda) if index_mode else None
    _ops().mb_gather(obs, act, *fl, o_obs, o_act, *o_fl, seed, uc, ep, off, mom, 1e-8, None, o_idx)
    torch.cuda.synchronize()
    sel = prng.prp(torch.arange(off, off + mb, dtype=torch.int64), n, prng.minibatch_key(seed, torch.tensor(3), ep))
    assert sorted(sel.tolist()) == sorted(set(sel.tolist())) and 0 <= int(sel.min()) and int(sel.max()) < n
    sel_d = sel.to(cuda)
    if index_mode:
        assert torch.equal(o_idx, sel_d)
    else:
        assert torch.equal(o_obs, obs[sel_d])
    assert torch.equal(o_act, act[sel_d])
    for k in (0, 2, 3):   # logp, ret, old value: copied
        assert torch.equal(o_fl[k], fl[k][sel_d])
    s = sel.numpy()
    _check("mb_gather", o_fl[1], st["norm"][s], O.tolerance("norm", st=st)[s], "norm")
    assert int(uc) == 3


# ------------------------------------------------------------------------------------------------- rejections


@pytest.mark.parametrize("L", [0, -3])
def test_no_entry_point_takes_a_window_below_one(cuda, L):
    """h = t + L < t would read before the rollout (or before the LDS copy): every binding refuses L < 1 before any
    launch, and the outputs keep their sentinel."""
    T, N, A, A1 = 5, 32, 6, 7
    B = T * N
    r, v, d = O.rollout(T, N)
    tr, tv, td = _dev(cuda, r, v, d)
    op = _head_operands(cuda, T, N, A)
    ops = _ops()
    msg = "look_ahead must be >= 1"

    def sentinel(*ts):
        torch.cuda.synchronize()
        for t in ts:
            assert (t == 7.0).all()

    ret, adv = torch.full((T, N), 7.0, device=cuda), torch.full((T, N), 7.0, device=cuda)
    with pytest.raises(RuntimeError, match=msg):
        ops.nstep_returns(tr, tv, td, ret, adv, 0.99, L)
    ws = R.ScanWorkspace(cuda, T, N)
    for mode in (1, 2):
        with pytest.raises(RuntimeError, match=msg):
            ops.returns_scan(tr, tv, td, ret, adv, mode, 0.99, 0.95, L, True, 1e-8, ws.part, ws.ticket, ws.mom, None,
                             ws.gz)
    for mode in ("nstep", "gae"):
        with pytest.raises(ValueError, match=msg):
            R.returns_scan(tr, tv, td, mode, 0.99, 0.95, look_ahead=L, ws=ws, ret_out=ret, adv_out=adv)
    with pytest.raises(ValueError, match=msg):
        R.nstep_returns(tr, tv, td, 0.99, L)
    sentinel(ret, adv)
    assert (ws.mom == 0).all() and (ws.ticket == 0).all()

    o = _head_outs(cuda, B, A1)
    o["dh"].fill_(7.0)
    head = (op["z"], op["act"], op["lpo"], op["ent"], op["kl"], 0.5, tr, tv.clone(), td, L, 1)
    tail = (o["ret"], o["adv"], op["h"], op["Wh"], o["dh"])
    grads = (o["gWh"], o["gbh"], o["gbfc"], o["stats"])
    with pytest.raises(RuntimeError, match=msg):
        ops.head_bwd(*head, False, 0.99, 0.95, *tail, *grads)
    with pytest.raises(RuntimeError, match=msg):
        ops.a2c_head(*head, False, 0.99, 0.95, *tail, *grads, None, 0, None, None, None)
    pWh, pbfc, pbh = (torch.full((N * n,), 7.0, device=cuda) for n in (512 * A1, 512, A1))
    spart = torch.full((N, 10), 7.0, dtype=torch.float64, device=cuda)
    with pytest.raises(RuntimeError, match=msg):
        ops.a2c_head_env(*head, 0.99, 0.95, *tail, None, 0, None, None, pWh, pbfc, pbh, spart)
    dz = torch.full((B, A1), 7.0, dtype=torch.bfloat16, device=cuda)
    with pytest.raises(RuntimeError, match=msg):
        _ac_loss(cuda, op, A, tr, tv.clone(), td, L, 1, 0.99, 0.95, False, o, dz, o["gbh"])
    sentinel(o["ret"], o["adv"], o["stats"], o["dh"].float(), dz.float(), pWh, pbfc, pbh, spart)
    assert (o["gWh"] == 0).all() and (o["gbh"] == 0).all() and (o["gbfc"] == 0).all()
