"""fp64 oracle of an arbitrary MLP actor-critic tower pair: forward, loss and backward written from the maths.

A tower is a list of ``(W [K, N], b [N], act)`` with ``act`` in ``tanh | relu | lrelu | None`` (the top layer's is
``None``: the Gaussian head applies its own tanh to the top pre-activation ``z``). The fp32 parameters are taken as
given (converted to float64, never rounded again); nothing here calls the package.

    dense        y = act(x W + b);   relu' = [y > 0],  lrelu(0.2)' = [y > 0] + 0.2 [y <= 0],  tanh' = 1 - y^2
    Gaussian     mu = tanh(z) sc,  ls = clip(log_std, -2.5, 2.5),
                 logp = sum_j -0.5 ((a - mu) / e^ls)^2 - ls - 0.5 log 2 pi,   H = sum_j 0.5 + 0.5 log 2 pi + ls
    categorical  logp = z_a - logsumexp z,   H = -sum p log p
    A2C actor    -mean(adv logp) + beta mean((lo - logp)^2) - c_ent mean H                       (algos/losses.py)
    PPO actor    -mean(min(r adv, clip(r, 1 +- eps) adv)) + beta mean((lo - logp)^2) - c_ent mean H,  r = e^(logp - lo)
    critic       mean((v - R)^2), or mean(max((v - R)^2, (vc - R)^2)) with vc = v_old + clip(v - v_old, +-eps_v)

:func:`reference_error` is the measurement the GPU test's bars come from: the error of the fp32 PyTorch autograd of
the same model (built here from ``torch`` primitives) against this oracle, per output class.
"""
import numpy as np

HALF_LOG_2PI = 0.5 * np.log(2.0 * np.pi)
STAT_NAMES = ("pg", "kl", "entropy", "crit_loss", "clipfrac", "act_loss")
MARGIN = 8.0       # the kernel's bar: MARGIN x the fp32 autograd's measured error (another summation order, tanhf)
FLOOR_ULPS = 4.0   # ... and never below a few fp32 ulps of the class's largest magnitude (reference error zero)
EPS32 = 2.0 ** -23


def _f64(x):
    return np.asarray(x, dtype=np.float64)


def act_fwd(z, act):
    if act == "tanh":
        return np.tanh(z)
    if act == "relu":
        return np.where(z > 0, z, 0.0)
    if act == "lrelu":
        return np.where(z > 0, z, 0.2 * z)
    assert act is None, act
    return z


def act_bwd(y, act):
    if act == "tanh":
        return 1.0 - y * y
    if act == "relu":
        return (y > 0).astype(np.float64)
    if act == "lrelu":
        return np.where(y > 0, 1.0, 0.2)
    assert act is None, act
    return np.ones_like(y)


def tower_forward(tower, x):
    """-> [x, y_0, ..., y_top] (float64); y_top is the top pre-activation."""
    ys = [_f64(x)]
    for W, b, act in tower:
        ys.append(act_fwd(ys[-1] @ _f64(W) + _f64(b), act))
    return ys


def tower_backward(tower, ys, d_top):
    """dL/d(top output) -> [(dW, db)] per layer."""
    grads = [None] * len(tower)
    dp = _f64(d_top)
    for l in range(len(tower) - 1, -1, -1):
        W, _, act = tower[l]
        dp = dp * act_bwd(ys[l + 1], act)          # dL/d(pre-activation of layer l)
        grads[l] = (ys[l].T @ dp, dp.sum(0))
        dp = dp @ _f64(W).T
    return grads


def gaussian_head(z, log_std, ac_scale, actions=None):
    th = np.tanh(z)
    mu = th * _f64(ac_scale)
    ls = np.clip(_f64(log_std), -2.5, 2.5)
    a = mu if actions is None else _f64(actions)
    d = a - mu
    logp = (-0.5 * (d * np.exp(-ls)) ** 2 - ls - HALF_LOG_2PI).sum(1)
    ent = np.broadcast_to((0.5 + HALF_LOG_2PI + ls).sum(), logp.shape).copy()
    return dict(mu=mu, th=th, ls=ls, d=d, logp=logp, ent=ent)


def categorical_head(z, actions=None):
    m = z.max(1, keepdims=True)
    lse = m[:, 0] + np.log(np.exp(z - m).sum(1))
    logq = z - lse[:, None]
    p = np.exp(logq)
    ent = -(p * logq).sum(1)
    amax = z.argmax(1)   # the first index of the largest logit
    srt = np.sort(z, 1)
    gap = srt[:, -1] - srt[:, -2] if z.shape[1] > 1 else np.full(z.shape[0], np.inf)
    a = amax if actions is None else np.asarray(actions).astype(np.int64)
    logp = logq[np.arange(z.shape[0]), a]
    return dict(p=p, logq=logq, logp=logp, ent=ent, argmax=amax, gap=gap, a=a)


def forward(actor, critic, head, obs, actions=None, log_std=None, ac_scale=None):
    """Evaluate (``actions`` given) or greedy (``actions=None``: the mean / first arg-max and its log-prob)."""
    ya = tower_forward(actor, obs)
    yc = tower_forward(critic, obs)
    h = gaussian_head(ya[-1], log_std, ac_scale, actions) if head == "gaussian" else categorical_head(ya[-1], actions)
    out = dict(value=yc[-1][:, 0], logp=h["logp"], entropy=h["ent"], hidden_actor=ya[1:-1], hidden_critic=yc[1:-1])
    if head == "gaussian":
        out["mean"] = h["mu"]
    else:
        out["argmax"], out["gap"] = h["argmax"], h["gap"]
    return out


def train(actor, critic, head, obs, actions, logp_old, adv, ret, v_old=None, ppo=False, beta=0.0, ent_coef=0.0,
          ppo_clip=0.2, v_clip=0.0, log_std=None, ac_scale=None):
    """One loss + backward: -> dict(grads_actor, grads_critic, g_log_std, stats, sumsq_actor, sumsq_critic)."""
    B = obs.shape[0]
    lo, adv, ret = _f64(logp_old), _f64(adv), _f64(ret)
    ya = tower_forward(actor, obs)
    yc = tower_forward(critic, obs)
    z = ya[-1]
    h = gaussian_head(z, log_std, ac_scale, actions) if head == "gaussian" else categorical_head(z, actions)
    lp, H = h["logp"], h["ent"]
    if ppo:
        ratio = np.exp(lp - lo)
        s1 = ratio * adv
        s2 = np.clip(ratio, 1.0 - ppo_clip, 1.0 + ppo_clip) * adv
        pg = -np.minimum(s1, s2).mean()
        dsurr = np.where(s1 <= s2, ratio * adv, 0.0)   # d min(s1, s2) / d logp (inside the clip range s2 == s1)
        clipfrac = (np.abs(ratio - 1.0) > ppo_clip).mean()
    else:
        pg = -(adv * lp).mean()
        dsurr = adv
        clipfrac = 0.0
    kl = ((lo - lp) ** 2).mean()
    a_loss = pg + beta * kl - ent_coef * H.mean()
    g = (-dsurr - 2.0 * beta * (lo - lp)) / B        # dL/d logp_i
    gH = -ent_coef / B                                # dL/d H_i
    g_ls = None
    if head == "gaussian":
        ivar = np.exp(-2.0 * h["ls"])
        sc = _f64(ac_scale)
        dz = g[:, None] * h["d"] * ivar * sc * (1.0 - h["th"] ** 2)
        raw = _f64(log_std)
        inr = (raw >= -2.5) & (raw <= 2.5)
        g_ls = np.where(inr, (g[:, None] * (h["d"] ** 2 * ivar - 1.0)).sum(0) + gH * B, 0.0)
    else:
        onehot = np.zeros_like(z)
        onehot[np.arange(B), h["a"]] = 1.0
        dz = g[:, None] * (onehot - h["p"]) + gH * (-h["p"] * (h["logq"] + H[:, None]))
    v = yc[-1][:, 0]
    if ppo and v_old is not None and v_clip and v_clip > 0:
        vo = _f64(v_old)
        vc = vo + np.clip(v - vo, -v_clip, v_clip)
        e1, e2 = (v - ret) ** 2, (vc - ret) ** 2
        c_loss = np.maximum(e1, e2).mean()
        dv = np.where(e1 >= e2, 2.0 * (v - ret), 2.0 * (vc - ret) * (np.abs(v - vo) < v_clip)) / B
    else:
        c_loss = ((v - ret) ** 2).mean()
        dv = 2.0 * (v - ret) / B
    ga = tower_backward(actor, ya, dz)
    gc = tower_backward(critic, yc, dv[:, None])
    ssa = sum((dW ** 2).sum() + (db ** 2).sum() for dW, db in ga) + (0.0 if g_ls is None else (g_ls ** 2).sum())
    ssc = sum((dW ** 2).sum() + (db ** 2).sum() for dW, db in gc)
    stats = dict(pg=pg, kl=kl, entropy=H.mean(), crit_loss=c_loss, clipfrac=clipfrac, act_loss=a_loss)
    return dict(grads_actor=ga, grads_critic=gc, g_log_std=g_ls, stats=stats, sumsq_actor=ssa, sumsq_critic=ssc,
                logp=lp, value=v)


# ------------------------------------------------------------------------------------------------ classes and bars
def classes_forward(o):
    """Oracle forward -> {class: float64 array}."""
    c = dict(value=o["value"], logp=o["logp"], entropy=o["entropy"])
    if "mean" in o:
        c["mean"] = o["mean"]
    return c


def layer_class(dW, db, extra=None):
    """One class per layer: its dW and db (and, for the actor's head, ``g_log_std``) as one vector. A class is what a
    reference error is measured over, and a one-element class (the value head's db, a one-action head's db or
    log-std gradient) gives a one-sample estimate of the fp32 error that 8 x says little about."""
    parts = [np.asarray(dW).reshape(-1), np.asarray(db).reshape(-1)]
    if extra is not None:
        parts.append(np.asarray(extra).reshape(-1))
    return np.concatenate(parts)


# A bias gradient is also judged on its own (against its own reference error and magnitude, which in a layer class
# hide behind dW's on a saturated first layer) when it has at least this many elements, one column tile. The bar is
# 8 x the largest of n reference errors; if the kernel's errors are about 3 x the reference's (what the large classes
# show), the bar is missed by chance when all n reference errors fall under ~3/8 of the kernel's largest: about 10 %
# of the time at n = 2, 1 % at n = 6, 1e-4 at n = 16. Narrower arrays (and g_log_std, at most 16 and here at most 6
# numbers) stay in their layer's class only.
MIN_OWN_CLASS = 16


def own_class(n):
    """Whether a bias gradient of ``n`` elements is also a class of its own."""
    return int(n) >= MIN_OWN_CLASS


def classes_train(o):
    c = {}
    for t, gs in (("actor", o["grads_actor"]), ("critic", o["grads_critic"])):
        for l, (dW, db) in enumerate(gs):
            top = t == "actor" and l == len(gs) - 1
            c[f"grad/{t}/{l}"] = layer_class(dW, db, o["g_log_std"] if top else None)
            if own_class(np.size(db)):
                c[f"db/{t}/{l}"] = np.asarray(db).reshape(-1)
    c["stats"] = np.array([o["stats"][n] for n in STAT_NAMES])
    return c


def class_errors(got, want):
    """Largest absolute error per class; ``got``: {class: array-like} of the same shapes."""
    return {k: float(np.max(np.abs(_f64(got[k]).reshape(-1) - _f64(want[k]).reshape(-1)))) if np.size(want[k]) else 0.0
            for k in want}


def bars(ref_err, want):
    """The kernel's bar per class: ``MARGIN`` x the fp32 reference's error, at least ``FLOOR_ULPS`` fp32 ulps of the
    class's largest magnitude."""
    return {k: max(MARGIN * ref_err[k], FLOOR_ULPS * EPS32 * float(np.max(np.abs(want[k])) if np.size(want[k]) else 0))
            for k in want}


def _torch_model(actor, critic, head, log_std, ac_scale):
    import torch

    def P(x):
        return torch.tensor(np.asarray(x, dtype=np.float32), requires_grad=True)
    ta = [(P(W), P(b), act) for W, b, act in actor]
    tc = [(P(W), P(b), act) for W, b, act in critic]
    ls = P(log_std) if head == "gaussian" else None

    def run(tower, x):
        for W, b, act in tower:
            x = torch.addmm(b, x, W)
            if act == "tanh":
                x = torch.tanh(x)
            elif act == "relu":
                x = torch.relu(x)
            elif act == "lrelu":
                x = 0.8 * torch.relu(x) + 0.2 * x
        return x

    def dist(z, actions):
        if head == "gaussian":
            mu = torch.tanh(z) * torch.tensor(np.asarray(ac_scale, dtype=np.float32))
            l = torch.clamp(ls, -2.5, 2.5).expand_as(mu)
            a = mu.detach() if actions is None else torch.tensor(np.asarray(actions, dtype=np.float32))
            logp = (-0.5 * ((a - mu) * torch.exp(-l)) ** 2 - l - float(HALF_LOG_2PI)).sum(-1)
            ent = (0.5 + float(HALF_LOG_2PI) + l).sum(-1)
            return mu, logp, ent
        logq = torch.log_softmax(z, -1)
        a = z.argmax(-1) if actions is None else torch.tensor(np.asarray(actions).astype(np.int64))
        return None, logq.gather(1, a.view(-1, 1)).squeeze(1), -(logq.exp() * logq).sum(-1)
    return ta, tc, ls, run, dist


def reference_forward(actor, critic, head, obs, actions=None, log_std=None, ac_scale=None):
    """The fp32 PyTorch forward of the same model -> {class: array}."""
    import torch
    ta, tc, ls, run, dist = _torch_model(actor, critic, head, log_std, ac_scale)
    with torch.no_grad():
        x = torch.tensor(np.asarray(obs, dtype=np.float32))
        mu, logp, ent = dist(run(ta, x), actions)
        c = dict(value=run(tc, x)[:, 0].numpy(), logp=logp.numpy(), entropy=ent.numpy())
        if mu is not None:
            c["mean"] = mu.numpy()
    return c


def reference_train(actor, critic, head, obs, actions, logp_old, adv, ret, v_old=None, ppo=False, beta=0.0,
                    ent_coef=0.0, ppo_clip=0.2, v_clip=0.0, log_std=None, ac_scale=None):
    """The fp32 PyTorch autograd of the same model and losses -> {class: array} (``classes_train`` keys)."""
    import torch
    ta, tc, ls, run, dist = _torch_model(actor, critic, head, log_std, ac_scale)
    f = lambda a: torch.tensor(np.asarray(a, dtype=np.float32))
    x, lo, ad, rt = f(obs), f(logp_old), f(adv), f(ret)
    _, lp, H = dist(run(ta, x), actions)
    v = run(tc, x)[:, 0]
    kl = ((lo - lp) ** 2).mean()
    if ppo:
        ratio = torch.exp(lp - lo)
        pg = -torch.min(ratio * ad, torch.clamp(ratio, 1.0 - ppo_clip, 1.0 + ppo_clip) * ad).mean()
        cf = ((ratio - 1.0).abs() > ppo_clip).float().mean()
    else:
        pg = -(ad * lp).mean()
        cf = torch.zeros(())
    a_loss = pg + beta * kl - ent_coef * H.mean()
    if ppo and v_old is not None and v_clip and v_clip > 0:
        vo = f(v_old)
        vc = vo + torch.clamp(v - vo, -v_clip, v_clip)
        c_loss = torch.max((v - rt) ** 2, (vc - rt) ** 2).mean()
    else:
        c_loss = ((v - rt) ** 2).mean()
    (a_loss + c_loss).backward()
    c = {}
    for t, tw in (("actor", ta), ("critic", tc)):
        for l, (W, b, _) in enumerate(tw):
            top = t == "actor" and l == len(tw) - 1 and ls is not None
            c[f"grad/{t}/{l}"] = layer_class(W.grad.numpy(), b.grad.numpy(), ls.grad.numpy() if top else None)
            if own_class(b.grad.numel()):
                c[f"db/{t}/{l}"] = b.grad.numpy().reshape(-1)
    c["stats"] = np.array([float(t_.detach()) for t_ in (pg, kl, H.mean(), c_loss, cf, a_loss)])
    return c


def reference_error(actor, critic, head, obs, actions, train_kw=None, log_std=None, ac_scale=None):
    """The measurement helper: the fp32 PyTorch model's error against this oracle, per output class, for the evaluate
    forward (``value``, ``logp``, ``entropy``), the greedy forward (``mean``, Gaussian heads) and -- with ``train_kw``
    (the keyword arguments of :func:`train` after ``actions``) -- one loss + backward. -> (errors, oracle classes)."""
    hk = dict(log_std=log_std, ac_scale=ac_scale)
    want = classes_forward(forward(actor, critic, head, obs, actions, **hk))
    got = reference_forward(actor, critic, head, obs, actions, **hk)
    if head == "gaussian":
        want["mean"] = forward(actor, critic, head, obs, None, **hk)["mean"]
        got["mean"] = reference_forward(actor, critic, head, obs, None, **hk)["mean"]
    if train_kw is not None:
        want.update(classes_train(train(actor, critic, head, obs, actions, **train_kw, **hk)))
        got.update(reference_train(actor, critic, head, obs, actions, **train_kw, **hk))
    return class_errors(got, want), want
