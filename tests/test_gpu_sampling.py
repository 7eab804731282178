"""The policy samplers against the fp64 oracle of tests/oracles/sampling_oracle.py at their edges: the 64-lane path,
keys beyond 2^32 (and negative), exact ties, strided logits, partial blocks, untouched padding, the pinned extreme
uniforms and the sampling law; the MLP engine's in-kernel samplers and the fused Pong steps across key 2^32.

Actions are compared by the decisive-row rule (the oracle's module docstring): exact equality wherever the fp64 gap
between the two largest perturbed logits is at least the margin. Floating-point tolerances come from the measured
error of the fp32 PyTorch reference against the oracle on the same inputs (x 8, floor 4 ulps), never from a kernel's
output; tests/test_sampling_oracle_cpu.py records them in profiles/sampling_oracle.txt.
"""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "oracles"))
import sampling_oracle as O  # noqa: E402

from test_gpu_mlp import CASES, _model  # noqa: E402

from actor_critic_algs_on_tensorflow_amd.ops import distributions as D  # noqa: E402

pytestmark = pytest.mark.gpu


def _ops():
    from actor_critic_algs_on_tensorflow_amd import _native
    return _native.require()


def _padded(cuda, B, pad=O.PAD_ROWS):
    act = torch.full((B + pad,), -7, dtype=torch.int32, device=cuda)
    logp = torch.full((B + pad,), O.SENTINEL, device=cuda)
    ent = torch.full((B + pad,), O.SENTINEL, device=cuda)
    return act, logp, ent


def _untouched(B, act, logp, ent):
    assert bool((act[B:] == -7).all()) and bool((logp[B:] == O.SENTINEL).all()) and bool((ent[B:] == O.SENTINEL).all())


def _check_cat(name, c, act, logp, ent):
    """Decisive-row rule of one categorical case ``c`` (oracle, decisive mask, tolerances) on kernel outputs."""
    o, dec = c["oracle"], c["decisive"]
    B = dec.numel()
    act, logp, ent = act[:B].cpu().long(), logp[:B].cpu().double(), ent[:B].cpu().double()
    share = float(dec.double().mean())
    wrong = int((act[dec] != o["act"][dec]).sum())
    e_lp = float((logp[dec] - o["logp"][dec]).abs().max()) if bool(dec.any()) else 0.0
    e_en = float((ent - o["ent"]).abs().max())
    print(f"{name}: decisive {share:.4f} wrong actions {wrong} logp err {e_lp:.3e} (tol {c['tol']['logp']:.3e}) "
          f"ent err {e_en:.3e} (tol {c['tol']['ent']:.3e})")
    assert share >= O.MIN_DECISIVE, (name, share)
    assert wrong == 0, (name, wrong)
    assert torch.isfinite(logp).all() and torch.isfinite(ent).all(), name
    assert e_lp <= c["tol"]["logp"], (name, e_lp, c["tol"]["logp"])
    assert e_en <= c["tol"]["ent"], (name, e_en, c["tol"]["ent"])


# ------------------------------------------------------------------------------------------ categorical_sample
@pytest.mark.parametrize("A", O.CAT_SWEEP_A)
def test_categorical_sweep_explicit_keys(cuda, A):
    """A on both sides of the 8-lane / 64-lane switch, keys with a varying non-zero high word and two negative ones."""
    c = O.cat_case(A, O.CAT_SWEEP_B)
    B = O.CAT_SWEEP_B
    act, logp, ent = _padded(cuda, B)
    _ops().categorical_sample(c["z"].to(cuda), c["keys"].to(cuda), c["seed"], act, logp, ent)
    _check_cat(f"A={A}", c, act, logp, ent)
    _untouched(B, act, logp, ent)


@pytest.mark.parametrize("B", O.CAT_SMALL_B)
def test_categorical_partial_blocks_leave_padding(cuda, B):
    """B not a multiple of the 4 rows per block: rows at or beyond B stay untouched."""
    c = O.cat_case(6, B)
    act, logp, ent = _padded(cuda, B)
    _ops().categorical_sample(c["z"].to(cuda), c["keys"].to(cuda), c["seed"], act, logp, ent)
    _check_cat(f"A=6 B={B}", c, act, logp, ent)
    _untouched(B, act, logp, ent)


@pytest.mark.parametrize("A,key_shift", O.ENV_CASES)
def test_categorical_sample_env_strided_logits_and_high_keys(cuda, A, key_shift):
    """Keys formed in-kernel from (tg, env id) on both sides of 2^32, logits a [:, :A] view of a wider tensor, the
    value column copied out: bitwise the explicit-key kernel on the host's int64 keys, which obeys the oracle."""
    c = O.env_case(A, key_shift)
    B = O.ENV_B
    ops = _ops()
    a0, l0, e0 = _padded(cuda, B)
    ops.categorical_sample(c["z"].to(cuda), c["keys"].to(cuda), O.ENV_SEED, a0, l0, e0)
    _check_cat(f"env A={A} shift={key_shift} (explicit keys)", c, a0, l0, e0)
    _untouched(B, a0, l0, e0)
    tg, ids = c["tg"].to(cuda), c["ids"].to(cuda)
    for extra in (1, 3):
        wide = torch.full((B, A + extra), float("nan"))
        wide[:, :A] = c["z"]
        wide[:, A] = c["value"]
        wide = wide.to(cuda)
        a1, l1, e1 = _padded(cuda, B)
        vout = torch.full((B + O.PAD_ROWS,), O.SENTINEL, device=cuda)
        ops.categorical_sample_env(wide[:, :A], tg, ids, key_shift, O.ENV_SEED, a1, l1, e1, vout)
        assert torch.equal(a1, a0) and torch.equal(l1, l0) and torch.equal(e1, e0), extra
        assert torch.equal(vout[:B], wide[:, A]) and bool((vout[B:] == O.SENTINEL).all()), extra
        # the explicit-key kernel on the same strided view
        a2, l2, e2 = _padded(cuda, B)
        ops.categorical_sample(wide[:, :A], c["keys"].to(cuda), O.ENV_SEED, a2, l2, e2)
        assert torch.equal(a2, a0) and torch.equal(l2, l0) and torch.equal(e2, e0), extra


@pytest.mark.parametrize("A,S", O.TIES)
def test_forced_ties_take_the_first_index(cuda, A, S):
    """Logit 2^30 (fp32 ulp 128, absorbs every finite Gumbel value) in the lanes of S, 0 elsewhere: over 64 keys the
    action is min(S), the log-prob -log|S| and the entropy log|S| (one logf of a small integer: 4 ulps)."""
    act, logp, ent = _padded(cuda, 64)
    _ops().categorical_sample(O.tie_logits(A, S).to(cuda), O.tie_keys().to(cuda), O.SEED, act, logp, ent)
    n = len(S)
    tol = 4 * O.ulp32(math.log(n)) if n > 1 else 0.0
    e_lp = float((logp[:64].cpu().double() + math.log(n)).abs().max())
    e_en = float((ent[:64].cpu().double() - math.log(n)).abs().max())
    print(f"ties A={A} S={S if n < 8 else 'all'}: actions {sorted(set(act[:64].tolist()))} logp err {e_lp:.3e} "
          f"ent err {e_en:.3e} tol {tol:.3e}")
    assert bool((act[:64] == min(S)).all())
    assert e_lp <= tol and e_en <= tol
    _untouched(64, act, logp, ent)


@pytest.mark.parametrize("A", [4, 20])
def test_pinned_uniform_one_wins_with_finite_outputs(cuda, A):
    """Key 30897600 / seed 11 / stream 0 draws u == 1.0: lane 0's Gumbel noise is +inf and beats a logit 50 ahead."""
    c = O.pinned_one_case(A)
    assert float(O.uniforms(O.SEED, c["keys"], [0])) == 1.0 and int(c["oracle"]["act"]) == 0
    act, logp, ent = _padded(cuda, 1)
    _ops().categorical_sample(c["z"].to(cuda), c["keys"].to(cuda), O.SEED, act, logp, ent)
    assert int(act[0]) == 0
    _check_cat(f"u=1 A={A}", c, act, logp, ent)
    assert abs(float(logp[0]) - float(c["oracle"]["lp"][0, 0])) <= c["tol"]["logp"]


def test_sampling_law_on_the_64_lane_path(cuda):
    """A = 40, 200 000 consecutive keys: every action's frequency within 5 binomial standard deviations of softmax."""
    n, A = 200000, 40
    z = torch.linspace(-2, 2, A)
    p = torch.softmax(z.double(), 0)
    a, _, _ = D.categorical_sample(z.repeat(n, 1).to(cuda), torch.arange(n, dtype=torch.int64, device=cuda), 3)
    freq = torch.bincount(a.cpu().long(), minlength=A).double() / n
    dev = ((freq - p).abs() / torch.sqrt(p * (1 - p) / n)).max()
    print(f"sampling law A=40: max deviation {float(dev):.2f} sigma")
    assert freq.numel() == A and float(dev) <= 5.0


@pytest.mark.parametrize("A,B", O.CAT_WIDE)
def test_more_than_64_actions_sample_through_the_reference(cuda, A, B):
    """D.categorical_sample on GPU logits beyond the kernel's 64 lanes: no error, the CPU reference's actions."""
    c = O.cat_case(A, B)
    act, logp, ent = D.categorical_sample(c["z"].to(cuda), c["keys"].to(cuda), c["seed"])
    assert act.is_cuda and act.dtype == torch.int32 and act.shape == (B,)
    dec = c["decisive"]
    assert torch.equal(act.cpu()[dec], c["ref"][0][dec])
    _check_cat(f"A={A} (fallback)", c, act, logp, ent)


# ------------------------------------------------------------------------------------------ gaussian_sample
@pytest.mark.parametrize("B", O.GAUSS_B)
@pytest.mark.parametrize("A", O.GAUSS_A)
def test_gaussian_sweep_strided_mu(cuda, A, B):
    """mu a [:, :A] view of a wider tensor, log_std beyond / at the clip bounds, |mu| up to 3 against the smallest
    sigma, keys with high words, the pinned smallest uniform in row 0; B around the 128-row block."""
    c = O.gauss_case(A, B)
    o, tol = c["oracle"], c["tol"]
    wide = torch.full((B, A + 3), float("nan"))
    wide[:, :A] = c["mu"]
    wide = wide.to(cuda)
    act = torch.full((B + O.PAD_ROWS, A), O.SENTINEL, device=cuda)
    _, logp, ent = _padded(cuda, B)
    _ops().gaussian_sample(wide[:, :A], c["ls"].to(cuda), c["keys"].to(cuda), c["seed"], act, logp, ent)
    errs = dict(act=float((act[:B].cpu().double() - o["act"]).abs().max()),
                logp=float((logp[:B].cpu().double() - o["logp"]).abs().max()),
                ent=float((ent[:B].cpu().double() - o["ent"]).abs().max()))
    print(f"gauss A={A} B={B}: " + " ".join(f"{k} err {errs[k]:.3e} (tol {tol[k]:.3e})" for k in errs))
    assert torch.isfinite(act[:B]).all() and torch.isfinite(logp[:B]).all() and torch.isfinite(ent[:B]).all()
    for k in errs:
        assert errs[k] <= tol[k], (k, errs[k], tol[k])
    assert bool((act[B:] == O.SENTINEL).all()) and bool((logp[B:] == O.SENTINEL).all())
    assert bool((ent[B:] == O.SENTINEL).all())


# ------------------------------------------------------------------------------------------ MLP engine
@pytest.mark.parametrize("case", CASES)
def test_mlp_policy_step_high_keys_against_oracle(cuda, case):
    """policy_step's in-kernel row_key and samplers with global step counters on both sides of key 2^32: the oracle
    is fed the reference model's logits / means; for the discrete heads the margin grows by 4 x the engine's measured
    difference from that model on the same observations."""
    ob, ac, disc, variant = case
    m, ref, flat, eng = _model(cuda, ob, ac, disc, variant)
    N = 70
    g = torch.Generator().manual_seed(41)
    obs = torch.randn(N, ob, generator=g).to(cuda)
    tg_h = torch.randint(0, 2 ** 36, (N,), generator=g, dtype=torch.int64)
    tg_h[:8] = torch.tensor([4095, 4096, 2 ** 32, 2 ** 36 + 5] * 2)
    tg = tg_h.to(cuda)
    ids = torch.arange(N, device=cuda, dtype=torch.int64) + 5
    act = torch.empty((N,) if disc else (N, ac), dtype=torch.int32 if disc else torch.float32, device=cuda)
    logp, ent, v = (torch.empty(N, device=cuda) for _ in range(3))
    eng.policy_step(obs, act, logp, ent, v, tg, ids, 20, 1234)
    keys = tg_h * (1 << 20) + ids.cpu()
    with torch.no_grad():
        pi, v_ref = ref(obs)
    torch.testing.assert_close(v, v_ref, rtol=1e-4, atol=1e-5)
    if disc:
        o = O.categorical(pi, keys, 1234)
        a_ref = o["act"].to(torch.int32).to(cuda)
    else:
        o = O.gaussian(pi, ref.actor.log_std, keys, 1234)
        a_ref = o["act"].float().to(cuda)
    lp2, ent2, v2 = (torch.empty(N, device=cuda) for _ in range(3))
    eng.evaluate(obs, a_ref, lp2, ent2, v2)
    with torch.no_grad():
        lp_e, ent_e, v_e = ref.evaluate(obs, a_ref)
    torch.testing.assert_close(lp2, lp_e, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(ent2, ent_e, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(v2, v_e, rtol=1e-4, atol=1e-5)
    if disc:
        diff = max(float((v - v_ref).abs().max()), float((lp2 - lp_e).abs().max()), float((ent2 - ent_e).abs().max()))
        margin = O.MARGIN + 4 * diff
        dec = O.decisive(o["gap"], margin)
        share = float(dec.double().mean())
        wrong = int((act.cpu().long()[dec] != o["act"][dec]).sum())
        print(f"mlp {case}: engine-reference diff {diff:.3e} margin {margin:.3e} decisive {share:.4f} wrong {wrong}")
        assert share >= 0.95, share
        assert wrong == 0
        torch.testing.assert_close(logp.cpu()[dec], o["logp"].float()[dec], rtol=1e-4, atol=1e-4)
    else:
        torch.testing.assert_close(act.cpu(), o["act"].float(), rtol=1e-4, atol=1e-5)
        torch.testing.assert_close(logp.cpu(), o["logp"].float(), rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(ent.cpu(), o["ent"].float(), rtol=1e-4, atol=1e-5)


def test_fused_mlp_rollout_carries_the_key_across_2_32(cuda):
    """test_fused_rollout_matches_per_step_launches at (frames, num_envs) = (1, 20) with every env's global step
    counter at 4090 before the first rollout: the 24 steps cross key 2^32 (tg 4096 at key_shift 20), so the one-launch
    rollout's register copy of the key carries into its high word."""
    from actor_critic_algs_on_tensorflow_amd import preset
    from actor_critic_algs_on_tensorflow_amd.algos.trainer import ActorCriticTrainer
    kw = dict(num_envs=20, n_steps=24, frames=1, ppo_epochs=1, ppo_minibatches=2, device="cuda:0",
              outdir=None, quiet=True, stdout_freq=0, save_every=0, cuda_graph=False)
    trs = [ActorCriticTrainer(preset("mujoco_ppo_dp8", fused_rollout=f, **kw)) for f in (True, False)]
    for tr in trs:
        assert tr.mlp is not None and tr.mlp.supports_fused_rollout(tr.env)
        tr.env.max_episode_steps = 7
        tr.env._sbuf["tg"].fill_(4090)    # both parity slots
    for it in range(2):   # second rollout starts from the written-back env bank
        for tr in trs:
            tr.collect()
        torch.cuda.synchronize()
        a, b = (tr.storage for tr in trs)
        for name in ("dones", "truncated"):
            assert torch.equal(getattr(a, name), getattr(b, name)), name
        for name in ("obs", "actions", "logp", "entropy", "rewards", "values"):
            x, y = getattr(a, name), getattr(b, name)
            torch.testing.assert_close(x, y, rtol=1e-4, atol=1e-4, msg=name)
        ea, eb = (tr.env for tr in trs)
        for name in ("t", "tg"):
            assert torch.equal(getattr(ea, name), getattr(eb, name)), name
        assert bool((ea.tg == 4090 + 24 * (it + 1)).all())
        for name in ("state", "ep_ret"):
            torch.testing.assert_close(getattr(ea, name), getattr(eb, name), rtol=1e-4, atol=1e-4, msg=name)
        torch.testing.assert_close(ea.ep_stats, eb.ep_stats, rtol=1e-5, atol=1e-4)
        assert int(a.dones.sum()) > 0
        for tr in trs:
            tr.storage.roll_over()


# ------------------------------------------------------------------------------------------ Pong
@pytest.mark.parametrize("tg0", [4095, 4096, 2 ** 31 + 3])
def test_fused_pong_policy_env_step_high_keys(cuda, tg0):
    """test_fused_policy_env_step_matches_separate_kernels with the env bank's global step counter at and beyond key
    2^32: all three forms sample with the key categorical_sample_env forms -- the fused kernels' own logits through
    categorical_sample_env give their actions, log-probs and entropies bit for bit, and obey the oracle."""
    from actor_critic_algs_on_tensorflow_amd import envs as E
    ops = _ops()
    N, A = 16, 6
    g = torch.Generator().manual_seed(5)
    h = torch.relu(torch.randn(N, 512, generator=g)).to(torch.bfloat16).to(cuda)
    Wh = (torch.randn(512 * (A + 1), generator=g) * 0.05).to(torch.bfloat16).to(cuda)
    bh = torch.randn(A + 1, generator=g).to(cuda)
    outs = []
    for fused in (True, False, "pre_shifted"):
        env = E.make("PongNoFrameskip-v4", N, device=cuda, seed=3)
        o0 = env.reset().clone()
        env._sbuf["tg"].fill_(tg0)
        tg_before, ids = env.tg.clone(), env.env_ids.clone()
        o1 = torch.empty_like(o0)
        act = torch.empty(N, dtype=torch.int32, device=cuda)
        lp, en, val = (torch.empty(N, device=cuda) for _ in range(3))
        z = torch.empty(N, A + 1, device=cuda)
        rew = torch.empty(N, device=cuda)
        dn, tr = (torch.empty(N, dtype=torch.uint8, device=cuda) for _ in range(2))
        if fused == "pre_shifted":
            W = [(torch.randn(n, generator=g) * 0.05).to(torch.bfloat16).to(cuda) for n in (8192, 32768, 36864)]
            bb = [torch.zeros(n, device=cuda) for n in (32, 64, 64)]
            ys = [torch.empty(N * r, c, dtype=torch.bfloat16, device=cuda) for r, c in ((400, 32), (81, 64), (49, 64))]
            ops.cnn_trunk_fwd(o0, W[0], bb[0], W[1], bb[1], W[2], bb[2], ys[0], ys[1], ys[2], 1.0 / 255.0, o1)
            ops.env_policy_step_pong(h, Wh, bh, z, act, lp, en, val, 20, 77, env.state, env.t, env.tg, env.ep_ret,
                                     env.ep_stats, env.env_ids, o0, o1, rew, dn, tr, env.seed,
                                     env.max_episode_steps, 4, True)
        elif fused:
            ops.env_policy_step_pong(h, Wh, bh, z, act, lp, en, val, 20, 77, env.state, env.t, env.tg, env.ep_ret,
                                     env.ep_stats, env.env_ids, o0, o1, rew, dn, tr, env.seed,
                                     env.max_episode_steps, 4)
        else:
            z = (h.float() @ Wh.float().view(512, A + 1)) + bh
            ops.categorical_sample_env(z[:, :A].contiguous(), env.tg, env.env_ids, 20, 77, act, lp, en, None)
            val = z[:, A].clone()
            env.step(act, prev_obs=o0, obs_out=o1, reward_out=rew, done_out=dn, trunc_out=tr)
        assert bool((env.tg == tg0 + 1).all())
        # this form's own logits through categorical_sample_env at the pre-step counter: the same key, the same bits
        a_s = torch.empty(N, dtype=torch.int32, device=cuda)
        l_s, e_s, v_s = (torch.empty(N, device=cuda) for _ in range(3))
        ops.categorical_sample_env(z[:, :A], tg_before, ids, 20, 77, a_s, l_s, e_s, v_s)
        assert torch.equal(a_s, act) and torch.equal(l_s, lp) and torch.equal(e_s, en), fused
        assert torch.equal(v_s, val), fused
        c = O._cat_measure(z[:, :A].cpu(), tg_before.cpu() * (1 << 20) + ids.cpu(), 77)
        _check_cat(f"pong tg={tg0} form={fused}", c, act, lp, en)
        outs.append((act.clone(), lp.clone(), en.clone(), val.clone(), o1.clone(), z.clone()))
    (a0, l0, e0, v0, f0, z0), (a1, l1, e1, v1, f1, z1), (a2, l2, e2, v2, f2, z2) = outs
    assert torch.equal(a0, a2) and torch.equal(f0, f2) and torch.equal(z0, z2) and torch.equal(l0, l2)
    assert torch.allclose(z0, z1, atol=2e-3)
    same = a0 == a1
    assert same.float().mean() >= 0.9
    assert torch.allclose(l0[same], l1[same], atol=2e-3) and torch.allclose(e0, e1, atol=2e-3)
    assert torch.allclose(v0, v1, atol=2e-3)
    assert torch.equal(f0[same], f1[same])


def test_fused_pong_rollout_step_crosses_key_2_32(cuda, monkeypatch):
    """test_fused_rollout_step_equals_separate_policy_and_trunk, eager, 2 updates of 5 steps from global step 4094:
    pong_fused_step crosses key 2^32 inside the first update and stays bit for bit equal to the separate launches."""
    monkeypatch.setattr("actor_critic_algs_on_tensorflow_amd.ops.gemm.TUNE", False)
    from actor_critic_algs_on_tensorflow_amd import preset
    from actor_critic_algs_on_tensorflow_amd.algos.trainer import ActorCriticTrainer
    runs = []
    for fused in ("1", "0"):
        tr = ActorCriticTrainer(preset("pong_a2c", num_envs=16, n_steps=5, device="cuda:0", outdir=None, quiet=True,
                                       stdout_freq=0, save_every=0, seed=5, engine_opts=dict(fused_step=fused == "1")))
        tr.env.max_episode_steps = 7
        tr.env._sbuf["tg"].fill_(4094)    # both parity slots
        snaps = []
        for _ in range(2):
            tr.step()
            st = tr.storage
            snaps.append([tr.flat.data.clone(), st.actions[:].clone(), st.rewards[:].clone(),
                          st.values[:].clone(), st.obs[st.T].clone(), tr.env.state.clone(), tr.env.t.clone(),
                          tr.env.tg.clone(), tr.env.ep_ret.clone(), tr.env.ep_stats.clone()])
        torch.cuda.synchronize()
        assert (getattr(tr, "_env_flips", 0) == 5) == (fused == "1")
        assert bool((tr.env.tg == 4094 + 10).all())
        runs.append(snaps)
    for k, (a, b) in enumerate(zip(*runs)):
        for j, (x, y) in enumerate(zip(a, b)):
            assert torch.equal(x, y), (k, j)
