"""The fp64 sampling oracle (tests/oracles/sampling_oracle.py) against the fp32 PyTorch references on every input set
of tests/test_gpu_sampling.py: decisive share, action equality, value agreement; the measured reference errors (they
set the GPU tolerances) are written to profiles/sampling_oracle.txt. Plus the pinned extreme uniforms, the
negative keys and the dispatch of wide action spaces."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "oracles"))
import sampling_oracle as O  # noqa: E402

from actor_critic_algs_on_tensorflow_amd.envs import rng  # noqa: E402
from actor_critic_algs_on_tensorflow_amd.ops import distributions as D  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE = os.path.join(ROOT, "profiles", "sampling_oracle.txt")


def test_oracle_matches_fp32_references_and_records_their_error():
    for name, c in O.all_cat_cases():
        o, (a_r, lp_r, e_r), dec = c["oracle"], c["ref"], c["decisive"]
        share = float(dec.double().mean())
        assert share >= O.MIN_DECISIVE, (name, share)
        assert share == 1.0, (name, share)                   # the inputs are chosen so that every row is decisive
        assert torch.equal(a_r.long()[dec], o["act"][dec]), name
        # fp32 log-softmax / entropy of up to 200 logits of magnitude <= 10: a few ulps of 10, far below 1e-4
        assert c["ref_err"]["logp"][0] < 2e-5 and c["ref_err"]["ent"][0] < 2e-5, (name, c["ref_err"])
        assert all(math.isfinite(t) and 0 < t < 2e-4 for t in c["tol"].values()), (name, c["tol"])
        if name.startswith("cat A="):                        # the explicit-key sweeps
            B = c["z"].shape[0]
            assert B < 4 or (int(c["keys"][-2]), int(c["keys"][-1])) == O.NEG_KEYS
            assert bool(((c["keys"] >> 32) != 0).all())      # the high key word is never zero there
        elif name.startswith("cat env"):                     # both sides of key 2^32 in one batch
            hi = c["keys"] >> 32
            assert bool((hi == 0).any()) and bool((hi > 0).any())
            assert c["key_shift"] != 20 or bool((hi == 1).any())
    for name, c in O.all_gauss_cases():
        o, r = c["oracle"], c["ref"]
        assert all(torch.isfinite(x).all() for x in r) and all(torch.isfinite(o[k]).all() for k in ("act", "logp", "ent"))
        # sigma <= e^2.5, radius <= 5.89: |a - mu| <= 72; fp32 log / sqrt / cos chains stay below 1e-4 of that
        assert c["ref_err"]["act"][0] < 1e-4 and c["ref_err"]["ent"][0] < 1e-5, (name, c["ref_err"])
        assert c["ref_err"]["logp"][0] < 1e-3, (name, c["ref_err"])
        assert all(math.isfinite(t) and 0 < t < 8e-3 for t in c["tol"].values()), (name, c["tol"])
        ls = c["ls"]
        if ls.numel() >= 5:
            assert (ls < -2.5).any() and (ls > 2.5).any() and (ls == 2.5).any() and (ls == -2.5).any() and (ls == 0).any()
        assert float(c["mu"].abs().max()) == 3.0
        # row 0, component 0: the pinned smallest uniform -> the largest Box-Muller radius
        assert abs(float(o["eps"][0, 0])) <= math.sqrt(-2 * math.log(2.0 ** -25)) + 1e-12
    lines = O.profile_lines()
    os.makedirs(os.path.dirname(PROFILE), exist_ok=True)
    text = "\n".join(lines) + "\n"
    try:
        with open(PROFILE) as f:
            same = f.read() == text
    except OSError:
        same = False
    if not same:
        try:
            with open(PROFILE, "w") as f:
                f.write(text)
        except OSError:      # read-only checkout: the measurements above still hold
            pass


def test_oracle_structure_on_hand_cases():
    # A == 1: always action 0, log-prob 0, entropy 0, gap +inf
    o = O.categorical(torch.tensor([[3.0], [-7.0]]), torch.tensor([5, 6]), 1)
    assert o["act"].tolist() == [0, 0] and o["logp"].tolist() == [0.0, 0.0] and o["ent"].tolist() == [0.0, 0.0]
    assert torch.isinf(o["gap"]).all()
    # first index of the maximum; an exact tie has gap 0 and is not decisive
    o = O.categorical(torch.tensor([[1.0, 1.0, 0.0]]), torch.tensor([O.KEY_U_ONE]), O.SEED)   # lane 0 at +inf
    assert int(o["act"]) == 0 and torch.isinf(o["gap"]).all()
    pert = torch.tensor([[0.5, 2.0, 2.0, 1.0]], dtype=torch.float64)
    assert int((pert == pert.max(-1, keepdim=True).values).to(torch.int64).argmax(-1)) == 1
    # forced ties (logit 2^30 in the lanes of S): the oracle's log-softmax is -log|S| there, its entropy log|S|
    for A, S in O.TIES:
        o = O.categorical(O.tie_logits(A, S), O.tie_keys(), O.SEED)
        assert (o["lp"][:, sorted(S)] + math.log(len(S))).abs().max() < 1e-12
        assert (o["ent"] - math.log(len(S))).abs().max() < 1e-12
        c = D.categorical_sample_ref(O.tie_logits(A, S), O.tie_keys(), O.SEED)
        assert bool((c[0] == min(S)).all()), (A, S)          # fp32: every finite Gumbel value is absorbed
        torch.testing.assert_close(c[1], torch.full((64,), -math.log(len(S))), rtol=0, atol=4 * O.ulp32(1.0))
        torch.testing.assert_close(c[2], torch.full((64,), math.log(len(S))), rtol=0, atol=4 * O.ulp32(1.0))
    # Gaussian: log-prob of the oracle's own action is the sum of log N(eps)
    g = O.gaussian(torch.zeros(3, 2), torch.tensor([0.0, 9.0]), torch.tensor([1, 2, 3]), 4)
    assert g["ls"].tolist() == [0.0, 2.5]
    want = (-0.5 * g["eps"] ** 2 - g["ls"] - O.HALF_LOG_2PI).sum(-1)
    torch.testing.assert_close(g["logp"], want, rtol=0, atol=0)
    torch.testing.assert_close(g["ent"], torch.full((3,), 2 * (0.5 + O.HALF_LOG_2PI) + 2.5, dtype=torch.float64))
    assert O.ulp32(1.0) == 2.0 ** -23 and O.ulp32(1.5) == 2.0 ** -23 and O.ulp32(2.0 ** 30) == 128.0
    assert O.tolerance(0.0, 1.0) == 4 * 2.0 ** -23 and O.tolerance(1e-3, 1.0) == 8e-3


def test_pinned_extreme_uniforms():
    """uniform_open / _u_open return (0, 1]: 1.0 exactly when h >> 8 == 0xFFFFFF, 0.5 * 2^-24 at the other end."""
    assert rng.hash_u32_py(O.SEED, O.KEY_U_ONE, 0, 0) >> 8 == 0xFFFFFF
    assert rng.hash_u32_py(O.SEED, O.KEY_U_MIN, 0, 0) >> 8 == 0
    u = D._u_open(O.SEED, torch.tensor([O.KEY_U_ONE, O.KEY_U_MIN]), 0)
    assert u.dtype == torch.float32 and u.tolist() == [1.0, 0.5 * 2.0 ** -24]
    assert O.uniforms(O.SEED, [O.KEY_U_ONE, O.KEY_U_MIN], [0]).view(-1).tolist() == [1.0, 0.5 * 2.0 ** -24]
    # u == 1: +inf Gumbel noise on lane 0 beats a logit 50 ahead; log-prob and entropy stay finite
    for A in (4, 20):
        z = torch.zeros(1, A)
        z[0, 1] = 50.0
        k = torch.tensor([O.KEY_U_ONE])
        o = O.categorical(z, k, O.SEED)
        a, lp, en = D.categorical_sample_ref(z, k, O.SEED)
        assert int(o["act"]) == 0 and int(a) == 0 and torch.isinf(o["gap"]).all()
        assert math.isfinite(float(lp)) and math.isfinite(float(en)) and abs(float(lp) - float(o["logp"])) < 1e-5
    # u1 == 1: Box-Muller radius 0, the action is the mean; u1 minimal: radius sqrt(50 log 2) = 5.887
    g = O.gaussian(torch.tensor([[1.25], [1.25]]), torch.tensor([0.0]), torch.tensor([O.KEY_U_ONE, O.KEY_U_MIN]), O.SEED)
    assert float(g["eps"][0, 0]) == 0.0 and float(g["act"][0, 0]) == 1.25
    assert abs(float(g["eps"][1, 0])) <= math.sqrt(50 * math.log(2.0)) + 1e-12
    r = D.gaussian_sample_ref(torch.tensor([[1.25], [1.25]]), torch.tensor([0.0]),
                              torch.tensor([O.KEY_U_ONE, O.KEY_U_MIN]), O.SEED)
    assert float(r[0][0, 0]) == 1.25 and all(torch.isfinite(x).all() for x in r)


def test_negative_keys_hash_as_twos_complement_words():
    for k in O.NEG_KEYS:
        w = k & 0xFFFFFFFFFFFFFFFF
        lo, hi = w & 0xFFFFFFFF, w >> 32
        for stream in (0, 1, 63):
            h = rng.hash_u32_py(O.SEED, lo, hi, stream)
            want = float(torch.tensor((h >> 8), dtype=torch.float32).add(0.5).mul(1.0 / 16777216.0))
            assert float(D._u_open(O.SEED, torch.tensor([k]), stream)) == want
            assert float(O.uniforms(O.SEED, [k], [stream])) == want
    # the two words are hashed separately: dropping the high word changes the draw
    k = torch.tensor([(5 << 32) + 9, 9])
    u = D._u_open(O.SEED, k, 0)
    assert float(u[0]) != float(u[1])


@pytest.mark.parametrize("A,native", [(1, True), (64, True), (65, False), (200, False)])
def test_wide_action_spaces_dispatch_to_the_reference(A, native, monkeypatch):
    """D.categorical_sample keeps the HIP kernel for GPU logits of at most 64 actions and samples wider spaces through
    the PyTorch reference on the tensor's own device. The dispatch condition alone decides, so no GPU is needed: the
    device test is patched to answer as it does for GPU logits, and the native op is replaced by a recorder."""
    monkeypatch.setattr(D._native, "use_native", lambda t: True)
    logits = torch.zeros(3, A)
    assert D._categorical_native(logits) == native
    called = {}

    class Ops:
        @staticmethod
        def categorical_sample(*a):
            called["native"] = True

    monkeypatch.setattr(D._native, "require", lambda: Ops)
    keys = torch.arange(3)
    out = D.categorical_sample(logits, keys, 5)
    assert ("native" in called) == native
    if not native:
        ref = D.categorical_sample_ref(logits, keys, 5)
        for x, y in zip(out, ref):
            assert torch.equal(x, y)
    monkeypatch.setattr(D._native, "use_native", lambda t: False)
    assert not D._categorical_native(logits)
