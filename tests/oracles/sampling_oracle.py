"""fp64 oracle of the policy samplers (csrc/kernels/heads.hip, cat_sample in common.h, the in-kernel samplers of
mlp.hip) and the input sets their CPU and GPU tests share.

The uniforms are formed exactly as the kernels form them -- the integer hash is exact, ``((h >> 8) + 0.5) * 2^-24`` is
evaluated in fp32 -- and then widened, so the oracle draws from the kernels' own bits and everything after the uniform
(two logs, the softmax, Box-Muller, the Gaussian density) is fp64.

Decisive rows. Gumbel-max picks ``argmax(z + g)``; a kernel that evaluates ``z + g`` in fp32 (two ``logf`` and one add,
|g| <= 17, |z| <= 32: about 1e-5 of error) may legitimately pick another action only where the two largest perturbed
logits are closer than that. A row is *decisive* when its fp64 gap (top-1 minus top-2, +inf for one action) is at least
``MARGIN``; on decisive rows the action must equal the oracle's exactly and the log-prob is compared, the entropy is
compared on every row. The input sets below are chosen so that (nearly) every row is decisive, and the CPU test
asserts that share, so a later change of inputs cannot silently empty the check.

Tolerances of the floating-point outputs are not fixed in advance: :func:`tolerance` takes the measured error of the
fp32 PyTorch reference (``ops/distributions.py`` ``*_ref``) against this oracle on the same inputs, times 8 (the GPU's
``logf`` / ``expf`` / ``cosf`` may each be an ulp or two off the host's), with a floor of 4 fp32 ulps of the largest
magnitude involved. Nothing here ever looks at a kernel's output.
"""
from __future__ import annotations

import functools
import math

import torch

from actor_critic_algs_on_tensorflow_amd.envs import rng
from actor_critic_algs_on_tensorflow_amd.ops import distributions as D

MARGIN = 1e-4            # fp32 error of z + g (about 1e-5) with a factor 10 to spare
MIN_DECISIVE = 0.99      # share of rows every input set must keep decisive
SEED = 11
KEY_U_ONE = 30897600     # (seed 11, stream 0): h >> 8 == 0xFFFFFF, u == 1.0 exactly
KEY_U_MIN = 8763087      # (seed 11, stream 0): h >> 8 == 0, u == 0.5 * 2^-24
NEG_KEYS = (-1, -(1 << 40) + 3)
HALF_LOG_2PI = 0.5 * math.log(2 * math.pi)


# ---------------------------------------------------------------------------------------------------- the oracle
def uniforms(seed, keys, streams):
    """fp64 [B, S]: the kernels' fp32 uniform of (seed, key, stream), widened. keys int64 [B], streams int64 [S]."""
    k = torch.as_tensor(keys, dtype=torch.int64).view(-1, 1)
    s = torch.as_tensor(streams, dtype=torch.int64).view(1, -1)
    h = rng.hash_u32(int(seed) & rng.M32, k & rng.M32, (k >> 32) & rng.M32, s)
    u = ((h >> 8).to(torch.float32) + 0.5) * (1.0 / 16777216.0)
    return u.double()


def categorical(logits, keys, seed):
    """dict: ``lp`` [B, A] log-softmax, ``ent`` [B], ``pert`` [B, A] = z + Gumbel, ``act`` [B] first index of the
    maximum, ``logp`` [B] = lp[act], ``gap`` [B] top-1 minus top-2 of pert (+inf for A == 1); all fp64 / int64."""
    z = logits.detach().cpu().double()
    B, A = z.shape
    lp = torch.log_softmax(z, dim=-1)
    p = lp.exp()
    ent = -torch.where(p > 0, p * lp, torch.zeros_like(p)).sum(-1)
    u = uniforms(seed, torch.as_tensor(keys).cpu(), torch.arange(A))
    pert = z + (-torch.log(-torch.log(u)))
    top = pert.max(-1, keepdim=True).values
    act = (pert == top).to(torch.int64).argmax(-1)          # first index of the maximum
    if A > 1:
        t2 = torch.topk(pert, 2, dim=-1).values
        gap = t2[:, 0] - t2[:, 1]
        gap = torch.where(torch.isnan(gap), torch.zeros_like(gap), gap)   # inf - inf: two lanes at +inf, a tie
    else:
        gap = torch.full((B,), math.inf, dtype=torch.float64)
    return dict(lp=lp, ent=ent, pert=pert, act=act, logp=lp.gather(-1, act.view(-1, 1)).squeeze(-1), gap=gap)


def gaussian(mu, log_std, keys, seed):
    """dict: ``act`` [B, A], ``logp`` [B], ``ent`` [B], ``eps`` [B, A], ``ls`` [A] (clipped), all fp64."""
    m = mu.detach().cpu().double()
    B, A = m.shape
    ls = torch.clamp(log_std.detach().cpu().double().view(A), D.LOG_STD_MIN, D.LOG_STD_MAX)
    j = torch.arange(A)
    k = torch.as_tensor(keys).cpu()
    u1, u2 = uniforms(seed, k, 2 * j), uniforms(seed, k, 2 * j + 1)
    eps = torch.sqrt(-2.0 * torch.log(u1)) * torch.cos(2 * math.pi * u2)
    act = m + torch.exp(ls) * eps
    logp = (-0.5 * eps * eps - ls - HALF_LOG_2PI).sum(-1)     # (act - mu) / sigma == eps exactly
    ent = (0.5 + HALF_LOG_2PI + ls).expand(B, A).sum(-1)
    return dict(act=act, logp=logp, ent=ent, eps=eps, ls=ls)


def decisive(gap, margin=MARGIN):
    return gap >= margin


# ---------------------------------------------------------------------------------------------------- tolerances
def ulp32(x):
    """Spacing of fp32 numbers at magnitude ``x`` (x > 0)."""
    x = max(float(x), 2.0 ** -126)
    return 2.0 ** (math.floor(math.log2(x)) - 23)


def err(got, want):
    """(max abs error, max relative error) of ``got`` against the fp64 ``want`` (relative where want != 0)."""
    g, w = got.detach().cpu().double(), want.double()
    if g.numel() == 0:
        return 0.0, 0.0
    d = (g - w).abs()
    nz = w != 0
    rel = float((d[nz] / w[nz].abs()).max()) if bool(nz.any()) else 0.0
    return float(d.max()), rel


def tolerance(ref_abs_err, magnitude):
    """Absolute tolerance for a kernel output: 8 x the fp32 reference's measured error, at least 4 ulps of the largest
    magnitude involved."""
    return max(8.0 * ref_abs_err, 4.0 * ulp32(magnitude))


# ---------------------------------------------------------------------------------------------------- input sets
def sweep_keys(B):
    """Per-row keys with a varying, non-zero high word; the last two rows (B >= 4) carry the negative keys."""
    i = torch.arange(B, dtype=torch.int64)
    k = i * 7919 + (((i % 5) * 4097) << 32) + (1 << 44)
    if B >= 4:
        k[-2], k[-1] = NEG_KEYS
    return k


CAT_SWEEP_A = (1, 2, 7, 8, 9, 16, 33, 63, 64)
CAT_SWEEP_B = 1024
CAT_SMALL_B = (1, 3, 5, 257)      # A = 6, outputs 8 rows longer than B
CAT_WIDE = ((65, 33), (200, 33))  # (A, B): beyond the kernel's 64 lanes, served by the PyTorch fallback
GAUSS_A = (1, 3, 6, 17)
GAUSS_B = (1, 127, 128, 129, 300)
PAD_ROWS = 8
SENTINEL = -777.0


def cat_inputs(A, B):
    g = torch.Generator().manual_seed(1000 * A + B)
    return torch.randn(B, A, generator=g) * 2, sweep_keys(B)


def gauss_inputs(A, B):
    """mu [B, A] with |mu| up to 3 (``a - mu`` cancels against the smallest sigma), log_std with values below -2.5,
    above 2.5, exactly -2.5 / 2.5 and 0, keys with non-zero high words; component 0 of row 0 draws the pinned smallest
    uniform (u1 == 0.5 * 2^-24: the largest Box-Muller radius, at the smallest sigma and |mu| == 3)."""
    g = torch.Generator().manual_seed(2000 * A + B)
    mu = (torch.rand(B, A, generator=g) * 6 - 3)
    mu[0, 0] = 3.0
    ls = torch.tensor([-3.0, 2.5, 0.0, -2.5, 3.5, 0.3, -1.0])[torch.arange(A) % 7].clone()
    keys = sweep_keys(B)
    keys[0] = KEY_U_MIN
    if B >= 8:
        keys[1] = KEY_U_ONE    # u1 == 1.0: radius 0, the action is the mean
    return mu, ls, keys


def tie_logits(A, S):
    z = torch.zeros(64, A)
    z[:, sorted(S)] = 2.0 ** 30      # fp32 ulp 128: absorbs every finite Gumbel value
    return z


TIES = [(64, s) for s in ((5, 37), (31, 32), (8, 9), (63,), (0, 63), tuple(range(64)))] + \
       [(8, s) for s in ((3, 7), (6,), (1, 2, 4))]


def tie_keys():
    return sweep_keys(64) + 12345


def mix_tg(N, gen):
    """Global step counters around and far beyond key 2^32 (tg 4096 at key_shift 20), mixed within one batch."""
    special = torch.tensor([0, 4095, 4096, 2 ** 32 - 1, 2 ** 32, 2 ** 36 + 5], dtype=torch.int64)
    tg = torch.randint(0, 2 ** 36, (N,), generator=gen, dtype=torch.int64)
    tg[:len(special)] = special[:N]
    return tg


# ---------------------------------------------------------------------------------------------------- measurements
@functools.lru_cache(maxsize=None)
def cat_case(A, B, seed=SEED):
    """Inputs, oracle, fp32 reference, its measured errors and the tolerances derived from them (computed once)."""
    z, keys = cat_inputs(A, B)
    return _cat_measure(z, keys, seed)


def _cat_measure(z, keys, seed):
    o = categorical(z, keys, seed)
    a_r, lp_r, e_r = D.categorical_sample_ref(z, keys, seed)
    dec = decisive(o["gap"])
    same = dec & (a_r.long() == o["act"])
    e_lp, e_en = err(lp_r[same], o["logp"][same]), err(e_r, o["ent"])
    mag = max(float(z.abs().max()), float(o["logp"].abs().max()), 1.0)
    tol = dict(logp=tolerance(e_lp[0], mag), ent=tolerance(e_en[0], max(float(o["ent"].abs().max()), 1.0)))
    return dict(z=z, keys=keys, seed=seed, oracle=o, ref=(a_r, lp_r, e_r), decisive=dec,
                ref_err=dict(logp=e_lp, ent=e_en), tol=tol)


@functools.lru_cache(maxsize=None)
def gauss_case(A, B, seed=SEED):
    mu, ls, keys = gauss_inputs(A, B)
    o = gaussian(mu, ls, keys, seed)
    r = D.gaussian_sample_ref(mu, ls, keys, seed)
    e = dict(act=err(r[0], o["act"]), logp=err(r[1], o["logp"]), ent=err(r[2], o["ent"]))
    # log-prob: the fp32 action is rounded to ulp(|a|); (a - mu) / sigma recovers eps with that error amplified by
    # 1 / sigma, and -eps^2 / 2 by |eps| again -- the largest magnitude its rounding acts on is |a| |eps| / sigma
    sig = torch.exp(o["ls"]).view(1, A)
    amp = float((o["act"].abs().max(torch.as_tensor(mu).double().abs()) * o["eps"].abs() / sig).max())
    tol = dict(act=tolerance(e["act"][0], max(float(o["act"].abs().max()), float(mu.abs().max()))),
               logp=tolerance(e["logp"][0], max(float(o["logp"].abs().max()), amp, 1.0)),
               ent=tolerance(e["ent"][0], max(float(o["ent"].abs().max()), 1.0)))
    return dict(mu=mu, ls=ls, keys=keys, seed=seed, oracle=o, ref=r, ref_err=e, tol=tol)


ENV_CASES = ((6, 20), (20, 20), (6, 12))   # (A, key_shift): one A <= 8, one A > 8, one other shift
ENV_B = 70
ENV_SEED = 77


def env_inputs(A, key_shift):
    """categorical_sample_env: logits, global step counters on both sides of key 2^32 and env ids; the keys are
    ``tg * 2^key_shift + id`` computed in int64 on the host."""
    g = torch.Generator().manual_seed(3000 * A + key_shift)
    z = torch.randn(ENV_B, A, generator=g) * 2
    value = torch.randn(ENV_B, generator=g)
    tg = mix_tg(ENV_B, g)
    ids = torch.arange(ENV_B, dtype=torch.int64) + 5
    return z, value, tg, ids, tg * (1 << key_shift) + ids


@functools.lru_cache(maxsize=None)
def env_case(A, key_shift):
    z, value, tg, ids, keys = env_inputs(A, key_shift)
    c = _cat_measure(z, keys, ENV_SEED)
    c.update(value=value, tg=tg, ids=ids, key_shift=key_shift)
    return c


def pinned_one_case(A):
    """u == 1.0 on lane 0 (+inf Gumbel noise) against a logit 50 ahead on lane 1."""
    z = torch.zeros(1, A)
    z[0, 1] = 50.0
    return _cat_measure(z, torch.tensor([KEY_U_ONE]), SEED)


def all_cat_cases():
    """(name, case) of every categorical input set the GPU tests compare against the oracle."""
    for A in CAT_SWEEP_A:
        yield f"cat A={A} B={CAT_SWEEP_B}", cat_case(A, CAT_SWEEP_B)
    for B in CAT_SMALL_B:
        yield f"cat A=6 B={B}", cat_case(6, B)
    for A, B in CAT_WIDE:
        yield f"cat A={A} B={B} (fallback)", cat_case(A, B)
    for A, ks in ENV_CASES:
        yield f"cat env A={A} B={ENV_B} key_shift={ks}", env_case(A, ks)
    for A in (4, 20):
        yield f"cat u=1 A={A} B=1", pinned_one_case(A)


def all_gauss_cases():
    for A in GAUSS_A:
        for B in GAUSS_B:
            yield f"gauss A={A} B={B}", gauss_case(A, B)


def profile_lines():
    """The measured reference errors and derived tolerances, as recorded in profiles/sampling_oracle.txt."""
    out = ["# fp32 PyTorch reference (ops/distributions.py *_ref) against the fp64 sampling oracle",
           "# (tests/oracles/sampling_oracle.py) on the input sets of tests/test_gpu_sampling.py, and the GPU tolerance",
           "# derived from each: max(8 x max abs error, 4 fp32 ulps of the largest magnitude involved).",
           "# Written by tests/test_sampling_oracle_cpu.py; columns: case, output, max abs err, max rel err, tolerance.",
           f"# margin {MARGIN:g}; decisive = share of rows whose fp64 top-1/top-2 gap is at least the margin."]
    for name, c in all_cat_cases():
        out.append(f"{name}: decisive {float(c['decisive'].double().mean()):.4f}")
        for k in ("logp", "ent"):
            a, r = c["ref_err"][k]
            out.append(f"{name}: {k} abs {a:.3e} rel {r:.3e} tol {c['tol'][k]:.3e}")
    for name, c in all_gauss_cases():
        for k in ("act", "logp", "ent"):
            a, r = c["ref_err"][k]
            out.append(f"{name}: {k} abs {a:.3e} rel {r:.3e} tol {c['tol'][k]:.3e}")
    return out
