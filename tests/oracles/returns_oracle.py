"""One fp64 oracle for every return / advantage kernel, with its input sets and derived tolerances.

The seven kernels it judges (csrc/kernels/returns.hip 1-3, loss.hip 4-7): ``gae_kernel``, ``nstep_kernel``,
``returns_scan_kernel``, ``ac_loss_kernel`` phase 0, ``head_bwd_kernel``, ``a2c_head_kernel``,
``a2c_head_env_kernel``. Nothing here imports ``ops/returns.py`` for its maths and nothing looks at a kernel output:
:func:`targets` is written from the definitions (``PathAdv`` of Basic_AC/run_AC.py:55-80 generalised to ``[T, N]``;
GAE(lambda)), :func:`stats` from Basic_AC/util.py:4-12 and run_AC.py:241, and every tolerance from the rounding
points of the code it bounds.

Definitions (``d[t]`` = the transition at t ended its episode, ``nd = 1 - d``; ``gamma`` / ``lam`` rounded to fp32
first, because that is what every kernel receives):

* n-step: ``h = min(t + L, T)``, ``e`` = the first terminal step in ``[t, h)`` (none: ``e = h - 1``),
  ``ret_t = sum_{k=t..e} gamma^(k-t) r_k + [no terminal in [t, h)] gamma^(h-t) V_h``, ``adv_t = ret_t - V_t``.
* GAE: ``A_t = r_t + gamma V_{t+1} nd_t - V_t + gamma lam nd_t A_{t+1}``, ``A_T = 0``, ``ret_t = A_t + V_t``.

``M`` is the same recurrence over absolute values (the sum of the magnitudes of the terms behind an element): every
rounding perturbs one term relatively, so every forward error bound below is ``(number of roundings) * u * M``.

Tolerances, with the operation counts they rest on
--------------------------------------------------
fp32 kernels (1, 2, 4-7), ``u = 2^-24``: ``(6 * steps + 4) * u * M`` with ``steps`` the recurrence steps behind the
element (``T - t`` for GAE, ``min(L, T - t)`` for n-step). Roundings per step, counted from the loops:

* GAE step (kernels 1, 4, 5, 6, 7, the same two statements in each): ``gamma * v`` 1, ``* nd`` exact, ``r +`` 1,
  ``- v`` 1, ``gamma * lam`` 1, ``* nd`` exact, ``* last`` 1, ``delta +`` 1 = 6. A term that enters at step s reaches
  step t through 3 roundings per step (coefficient, multiply, add) plus its own 3: ``3 * steps + 3``.
* n-step step (kernels 2, 4, 5, 6, 7, the same loop in each): ``disc * r`` 1, ``acc +`` 1, ``disc * gamma`` 1 = 3; the
  bootstrap ``disc * v`` 1, ``acc +`` 1. The k-th term carries the k roundings of ``disc`` plus 2, and at most
  ``steps`` additions after it: ``2 * steps + 2``.
* after the loop: ``ret = last + v`` 1 (GAE), ``adv = ret - v`` 1 -- inside the ``+ 4``.

Six per step is an upper count for each loop; FMA contraction only removes roundings. For kernels 4-7 in GAE mode
``adv`` is ``(last + v) - v``, so its ``M`` is that of ``ret`` (:func:`targets` returns it as ``M["adv_head"]``).

Scan (kernel 3): every output is ONE fp32 rounding of an fp64 value: ``u * |value| + k * 2^-53 * M_full``.
``M_full`` (``M["scan_ret"]``, ``M["scan_adv"]``) runs over the whole remaining rollout, because the prefix-sum window
form computes ``Gz_t + gamma^(h-t) (V_h - Gz_h)`` with ``Gz`` the un-bootstrapped return to the rollout's end. ``k``
counts the fp64 roundings on the longest dependent chain at that T, from the kernel:

* pass 1, per step of a chunk (K steps): the term ``r + g * vn * nd - v`` 3, ``ca = x + c * ca`` 2, ``cc = c * cc`` 1
  (``c = g * lam * nd`` is exact: two 24-bit factors) -- at most 8 with slack;
* suffix scan: log2(CH) compositions, ``na = ca + cc * s_a`` 2, ``nc = cc * s_c`` 1 -- at most 8; the carry
  ``s_a + s_c * init`` 2;
* pass 2, per step: 7 (GAE), 2 (n-step); the output ``x + vt`` or ``x - vt`` 1 -- at most 8;
* window pass: ``pow`` (taken as 4), ``v - gz`` 1, ``gh *`` 1, ``tg +`` 1, ``tg - vt`` 1 = 8.
* the coefficient ``prod c`` that multiplies a term s steps away is built from s - 1 multiplications whatever the
  association, so the chain count alone is not a bound: ``T`` roundings are added for it.

``k = 8 * (2 K + log2(CH) + 3) + T`` (:func:`scan_k`). At T = 4100 that is 4452, i.e. 5e-13 * M.

Normalised advantages (kernel 3 tail, ``normalize_mom_kernel``): mean and std are rounded to fp32 once each,
``eps + std`` 1, ``1 / (.)`` 1 (taken as 2), ``a - fm`` 1, ``* inv`` 1: c = 6 relative roundings on ``a - mean``, and
the rounding of the mean shifts every element by ``u |mean|``. The fp64 single-pass variance adds
``kappa * n * 2^-53`` relatively (``kappa = (mean^2 + var) / var``):
``(u |mean| + (6 u + kappa n 2^-53) |a - mean|) / (eps + std)``.

EV and moments are functions of what the kernel wrote, so they are compared with :func:`stats` of the kernel's own
fp32 outputs: EV ``u + kappa * n * 2^-53`` (the final fp32 cast and the single-pass fp64 variance; ``kappa`` of the
worse series; a thread's sum is at most ``n / 256`` terms plus a tree, so ``n`` roundings cover the variance and the
covariance terms together); moments ``n * 2^-53 * sum |terms|``.
"""
from __future__ import annotations

import functools
import math

import numpy as np

U32 = 2.0 ** -24
U64 = 2.0 ** -53
EPS = 1e-8

# ------------------------------------------------------------------------------------------------------ oracle


def _f32(x):
    return float(np.float32(x))


def targets(r, v, d, mode, gamma, lam, L):
    """fp64 targets / advantages of a ``[T, N]`` rollout, one env column at a time.

    ``r``, ``d`` ``[T, N]``, ``v`` ``[T + 1, N]`` (widened to fp64); ``mode`` "gae" or "nstep"; ``gamma``, ``lam`` are
    rounded to fp32 first. Returns ``(ret, adv, M)``, ``M`` a dict of absolute-value recurrences: ``ret``, ``adv``
    (the element's own terms), ``adv_head`` (kernels 4-7: ``adv = ret - v``), ``scan_ret`` / ``scan_adv`` (the whole
    remaining rollout, for the scan)."""
    r = np.asarray(r, dtype=np.float64)
    v = np.asarray(v, dtype=np.float64)
    d = np.asarray(d) != 0
    T, N = r.shape
    assert v.shape == (T + 1, N) and d.shape == (T, N) and int(L) >= 1
    g, lm = _f32(gamma), _f32(lam)
    ret, adv = np.zeros((T, N)), np.zeros((T, N))
    M = {k: np.zeros((T, N)) for k in ("ret", "adv", "adv_head", "scan_ret", "scan_adv")}
    if mode == "gae":
        for n in range(N):
            a, m = 0.0, 0.0
            for t in range(T - 1, -1, -1):
                nd = 0.0 if d[t, n] else 1.0
                a = r[t, n] + g * v[t + 1, n] * nd - v[t, n] + g * lm * nd * a
                m = abs(r[t, n]) + g * abs(v[t + 1, n]) * nd + abs(v[t, n]) + g * lm * nd * m
                adv[t, n], ret[t, n] = a, a + v[t, n]
                M["adv"][t, n], M["ret"][t, n] = m, m + abs(v[t, n])
        M["adv_head"] = M["ret"] + np.abs(v[:T])
        M["scan_ret"], M["scan_adv"] = M["ret"], M["adv"]
        return ret, adv, M
    assert mode == "nstep"
    L = int(L)
    pw = g ** np.arange(min(L, T) + 1, dtype=np.float64)
    for n in range(N):
        nxt = np.full(T + 1, T)            # first terminal step >= t (T: none)
        mz = np.zeros(T + 1)               # |.| of the un-bootstrapped return to the rollout's end
        for t in range(T - 1, -1, -1):
            nxt[t] = t if d[t, n] else nxt[t + 1]
            mz[t] = abs(r[t, n]) + (0.0 if d[t, n] else g * mz[t + 1])
        for t in range(T):
            h = min(t + L, T)
            alive = nxt[t] >= h
            e = h if alive else nxt[t] + 1   # one past the last summed step
            acc = float(np.dot(pw[:e - t], r[t:e, n]))
            m = float(np.dot(pw[:e - t], np.abs(r[t:e, n])))
            mf = mz[t]
            if alive:
                acc += pw[h - t] * v[h, n]
                m += pw[h - t] * abs(v[h, n])
                mf += pw[h - t] * (abs(v[h, n]) + (mz[h] if L < T else 0.0))
            ret[t, n], adv[t, n] = acc, acc - v[t, n]
            M["ret"][t, n], M["scan_ret"][t, n] = m, mf
    M["adv"] = M["ret"] + np.abs(v[:T])
    M["adv_head"] = M["adv"]
    M["scan_adv"] = M["scan_ret"] + np.abs(v[:T])
    return ret, adv, M


def steps_behind(mode, T, N, L):
    """Recurrence steps behind every element: ``T - t`` (GAE), ``min(L, T - t)`` (n-step); ``[T, 1]``."""
    left = np.arange(T, 0, -1, dtype=np.float64)[:, None]
    return left if mode == "gae" else np.minimum(float(L), left)


def stats(ret32, adv32, v):
    """Two-pass fp64 statistics of fp32 arrays (widened): EV correlation of (ret, v) with the population std, the
    moments in ``returns_scan``'s order ``[count, sum adv, sum adv^2, sum ret, sum ret^2, sum V, sum V^2, sum ret V]``
    with the sums of absolute terms behind each, and the fp64 normalisation ``(a - mean) / (eps + std)``."""
    x = np.asarray(ret32, dtype=np.float64).reshape(-1)
    a = np.asarray(adv32, dtype=np.float64).reshape(-1)
    y = np.asarray(v, dtype=np.float64).reshape(-1)
    n = x.size
    assert a.size == n and y.size == n
    mx, my, ma = x.mean(), y.mean(), a.mean()
    vx, vy, va = ((x - mx) ** 2).mean(), ((y - my) ** 2).mean(), ((a - ma) ** 2).mean()
    with np.errstate(invalid="ignore", divide="ignore"):
        ev = float(((x - mx) * (y - my)).mean() / math.sqrt(vx * vy)) if vx * vy > 0 else float("nan")

    def kappa(m, var):
        return (m * m + var) / var if var > 0 else float("inf")

    terms = [a, a * a, x, x * x, y, y * y, x * y]
    return dict(n=n, ev=ev, ev_kappa=max(kappa(mx, vx), kappa(my, vy)),
                mom=np.array([float(n)] + [t.sum() for t in terms]),
                mom_abs=np.array([0.0] + [np.abs(t).sum() for t in terms]),
                mean=ma, std=math.sqrt(va), adv_kappa=kappa(ma, va),
                norm=(a - ma) / (EPS + math.sqrt(va)))


# -------------------------------------------------------------------------------------------------- tolerances


def geometry(T, N):
    """``aca_returns_scan_geometry`` restated: ``(E, CH, K, blocks)``."""
    ch = 1
    while ch < 256 and ch * 8 < T:
        ch <<= 1
    E = 256 // ch
    return E, ch, -(-T // ch), -(-N // E)


def scan_k(T):
    """fp64 roundings on the longest chain of ``returns_scan_kernel`` at this T (module docstring)."""
    _, CH, K, _ = geometry(T, 1)
    return 8 * (2 * K + int(math.log2(CH)) + 3) + T


def tolerance(kind, steps=None, M=None, value=None, T=None, st=None):
    """Derived absolute tolerances (module docstring). ``kind``:

    * ``"fp32"``: ``(6 steps + 4) u M`` -- kernels 1, 2, 4-7;
    * ``"scan"``: ``u |value| + scan_k(T) 2^-53 M`` -- kernel 3 (``M`` over the whole remaining rollout);
    * ``"norm"``: per element, from ``st = stats(...)`` of the un-normalised advantages;
    * ``"ev"``: scalar, from ``st``; ``"mom"``: the 8 moments, from ``st``."""
    if kind == "fp32":
        return (6.0 * steps + 4.0) * U32 * M
    if kind == "scan":
        return U32 * np.abs(value) + scan_k(T) * U64 * M
    if kind == "norm":
        dev = np.abs(st["norm"]) * (EPS + st["std"])          # |a - mean|
        kap = st["adv_kappa"] if math.isfinite(st["adv_kappa"]) else 0.0   # a constant series: no cancellation
        return (U32 * abs(st["mean"]) + (6.0 * U32 + kap * st["n"] * U64) * dev) / (EPS + st["std"])
    if kind == "ev":
        return U32 + st["ev_kappa"] * st["n"] * U64
    if kind == "mom":
        return st["n"] * U64 * st["mom_abs"]
    raise ValueError(kind)


# -------------------------------------------------------------------------------------------------- input sets

DONES = ("none", "all", "random", "planted")
VALUES = ("randn", "offset", "zero")
GAMMAS = ((0.99, 0.95), (1.0, 1.0), (0.9, 0.0), (0.0, 0.5), (0.999, 0.99))


def window_start(T, K, L):
    """The fixed start ``t*`` whose truncated window ``[t*, t* + L)`` gets the planted edge terminals, or None when
    the window is not truncated there (``t* + L`` must be a step of the rollout)."""
    if L is None or T - 1 - L < 0:
        return None
    return min(K + 1, T - 1 - L)


def planted(T, N, L=None):
    """Terminals at the scan's edges. Returns ``(d, claims)``:

    * env 0 carries ``t in {0, K - 1, K, T - 1}`` (those inside the rollout; K from :func:`geometry`), so a terminal
      sits on a chunk's last step, on the next chunk's first step and on both ends of the rollout;
    * env ``3 + i`` (where it exists) carries the i-th of them alone;
    * for a truncated window, with ``t* = window_start(T, K, L)``: env ``1 % N`` has its only terminal at
      ``t* + L - 1`` (the last step inside the window), env ``2 % N`` its only one at ``t* + L`` (the first outside).

    ``claims = dict(K, base=[(t, n), ...], tstar, inside=(t, n) | None, outside=(t, n) | None)``."""
    K = geometry(T, N)[2]
    d = np.zeros((T, N), dtype=np.uint8)
    base_t = sorted({t for t in (0, K - 1, K, T - 1) if 0 <= t < T})
    base = [(t, 0) for t in base_t]
    for i, t in enumerate(base_t):
        if 3 + i < N:
            base.append((t, 3 + i))
    for t, n in base:
        d[t, n] = 1
    ts = window_start(T, K, L)
    inside = outside = None
    if ts is not None and N >= 3:
        inside, outside = (ts + L - 1, 1), (ts + L, 2)
        d[inside] = 1
        d[outside] = 1
    return d, dict(K=K, base=base, tstar=ts, inside=inside, outside=outside)


def _seed(T, N, dones, values):
    return T * 1000003 + N * 1009 + DONES.index(dones) * 17 + VALUES.index(values)


def rollout(T, N, dones="random", values="randn", L=None):
    """fp32 ``r [T, N]``, ``v [T + 1, N]`` and uint8 ``d [T, N]`` of one input set (deterministic in its arguments).

    dones: ``none``, ``all``, ``random`` (p = 0.1), ``planted`` (:func:`planted`); values: ``randn`` (r ~ N(0, 1),
    v ~ 2 N(0, 1)), ``offset`` (v ~ 100 + 2 N(0, 1): mean much larger than spread), ``zero`` (r = v = 0)."""
    rng = np.random.default_rng(_seed(T, N, dones, values))
    r = rng.standard_normal((T, N)).astype(np.float32)
    v = (2.0 * rng.standard_normal((T + 1, N))).astype(np.float32)
    rnd = (rng.random((T, N)) < 0.1).astype(np.uint8)
    if values == "offset":
        v = (np.float32(100.0) + v).astype(np.float32)
    elif values == "zero":
        r, v = np.zeros_like(r), np.zeros_like(v)
    if dones == "none":
        d = np.zeros((T, N), dtype=np.uint8)
    elif dones == "all":
        d = np.ones((T, N), dtype=np.uint8)
    elif dones == "random":
        d = rnd
    else:
        d = planted(T, N, L)[0]
    return r, v, d


def _case(T, N, mode, L=None, gl=GAMMAS[0], dones="planted", values="randn"):
    return (T, N, mode, L, gl[0], gl[1], dones, values)


def scan_cases():
    """``(T, N, mode, L, gamma, lam, dones, values)`` of the scan tests; L None = the whole rollout."""
    out = []
    # the shape table: one chunk; CH = 2 with odd T*N and a nearly empty last workgroup; CH = 8; the last register
    # shape; the first global-path shape (K = 9, odd T*N); K = 17 with the vector normalisation
    for T, N in ((1, 1), (8, 3), (9, 5), (9, 129), (37, 19), (2048, 2), (2049, 3), (4100, 2)):
        out += [_case(T, N, "gae"), _case(T, N, "nstep")]
    out += [_case(37, 19, "nstep", L) for L in (1, 4, 5, 6, 36)]
    out += [_case(2049, 3, "nstep", L) for L in (9, 10, 2048)]
    for T, N, Lw in ((9, 5, 5), (37, 19, 5), (2049, 3, 9)):
        for dn in DONES:
            for vs in VALUES:
                out += [_case(T, N, "gae", None, GAMMAS[0], dn, vs), _case(T, N, "nstep", None, GAMMAS[0], dn, vs),
                        _case(T, N, "nstep", Lw, GAMMAS[0], dn, vs)]
    for T, N, Lw in ((37, 19, 6), (2049, 3, 10)):
        for gl in GAMMAS:
            out += [_case(T, N, "gae", None, gl), _case(T, N, "nstep", None, gl), _case(T, N, "nstep", Lw, gl)]
    return list(dict.fromkeys(out))


SCAN_FULL_EQUIV = ((37, 19, 37), (37, 19, 38))   # windows at or past the rollout's end == the whole rollout

SIMPLE_SHAPES = ((1, 1), (37, 19), (5, 257), (7, 37))   # two workgroups of gae_kernel / of nstep_kernel


def simple_cases():
    """``(T, N, gamma, lam, dones)`` for kernels 1 and 2; each runs GAE and n-step at ``L in simple_windows(T)``."""
    return [(T, N, g, lm, dn) for T, N in SIMPLE_SHAPES for dn in DONES for g, lm in GAMMAS]


def simple_windows(T):
    return list(dict.fromkeys((1, 5, T, T + 3)))


# (T, N, mode, L): mode 1 n-step, 2 GAE (L then unused: the rollout length is passed)
HEAD_SHAPES = ((5, 32, 1, 5), (5, 32, 2, None), (16, 24, 1, 5), (16, 24, 1, 16), (1, 7, 1, 1), (2, 256, 2, None),
               (512, 1, 2, None), (512, 1, 1, 512))
ENV_SHAPES = ((5, 32, 1, 5), (5, 32, 2, None), (64, 3, 1, 5), (64, 1, 2, None), (64, 1, 1, 64), (1, 7, 1, 1))
LOSS_SHAPES = ((5, 32, 1, 5), (16, 24, 2, None), (2, 257, 2, None), (5, 410, 1, 5))   # staged x2, N > 256, B > 2048
HEAD_DONES = ("planted", "random")
HEAD_GAMMAS = ((0.99, 0.95), (1.0, 1.0))


def head_cases(shapes):
    return [(T, N, mode, L, g, lm, dn) for T, N, mode, L in shapes for dn in HEAD_DONES for g, lm in HEAD_GAMMAS]


# ------------------------------------------------------------------------- fp32 transcriptions of the kernel loops


def emulate_fp32(r, v, d, mode, gamma, lam, L, head=False):
    """numpy fp32 transcription of the six fp32 loops (one rounding per operation, no contraction), vectorised over
    the elements but in each element's own operation order: ``gae_kernel`` / ``nstep_kernel`` (``head=False``) and
    the phase-0 loops of kernels 4-7 (``head=True``: ``adv = ret - v`` also for GAE). Returns fp32 ``(ret, adv)``."""
    f = np.float32
    r, v = np.asarray(r, dtype=f), np.asarray(v, dtype=f)
    dn = np.asarray(d) != 0
    T, N = r.shape
    g, lm = f(gamma), f(lam)
    if mode == "gae":
        adv, ret = np.zeros((T, N), f), np.zeros((T, N), f)
        last = np.zeros(N, f)
        gl = f(g * lm)
        for t in range(T - 1, -1, -1):
            nd = np.where(dn[t], f(0), f(1))
            delta = (r[t] + (g * v[t + 1]) * nd) - v[t]
            last = delta + (gl * nd) * last
            adv[t], ret[t] = last, last + v[t]
        return (ret, ret - v[:T]) if head else (ret, adv)
    acc = np.zeros((T, N), f)
    alive = np.ones((T, N), bool)
    disc = np.ones((T, 1), f)              # per start t: gamma^j while the window runs, frozen at its end
    Lw = min(int(L), T)
    for j in range(Lw):
        n = T - j                          # starts t < T - j still have step t + j inside the rollout
        acc[:n] = np.where(alive[:n], acc[:n] + disc[:n] * r[j:], acc[:n])
        run = np.zeros((T, 1), bool)
        run[:n] = True
        disc = np.where(run, disc * g, disc)
        alive[:n] &= ~dn[j:]
    # disc froze at gamma^(h - t) for every start whose window ran to h; dead windows do not use it
    h = np.minimum(np.arange(T) + Lw, T)
    boot = disc * v[h]
    ret = np.where(alive, acc + boot, acc)
    return ret, ret - v[:T]



# ------------------------------------------------------------------------------------ shared, read-only case data


@functools.lru_cache(maxsize=None)
def case_data(T, N, mode, L, gamma, lam, dones, values="randn"):
    """``(r, v, d, ret, adv, M)`` of one case, computed once per process and read-only. ``L`` None = whole rollout;
    the planted window terminals follow ``L`` for n-step cases only."""
    r, v, d = rollout(T, N, dones, values, L if mode == "nstep" else None)
    ret, adv, M = targets(r, v, d, mode, gamma, lam, T if L is None else L)
    for x in (r, v, d, ret, adv, *M.values()):
        x.setflags(write=False)
    return r, v, d, ret, adv, M
