"""The reference's MLP actor and critic, with TF-compatible variable names.

Actor (``Basic_AC/policies.py:33-89``, ``A3C/policies.py:34-104``)::

    first_layer  D->128 lrelu(0.2) -> second_layer 128->128 lrelu -> third_layer 128->64 lrelu
    continuous: mu_layer 64->A, tanh * ac_scale;  log_std [A] (init 0, clipped to [-2.5, 2.5] in forward)
    discrete:   logits 64->A

Critic (``Basic_AC/policies.py:123-149``, ``A3C/policies.py:137-170``)::

    first_layer D->256 relu -> second_layer 256->128 relu -> third_layer 128->128 relu -> value 128->1

``variant`` selects the documented divergences:
  * ``"basic"``: mu kernel init 0.1*Xavier, logits default Xavier, critic value reads the *second* layer
    (the third layer is built but unused -- bug #4, kept so checkpoints carry the same variables).
  * ``"a3c"``: mu kernel default Xavier, logits column-normalised (0.1), critic value reads the third layer.

Custom towers (``hidden`` and / or ``activation`` given; ``TrainConfig.actor_hidden`` / ``critic_hidden`` /
``hidden_act``): any 1..4 hidden widths, one of ``tanh | relu | lrelu`` on every hidden layer, the same heads. Their
layers are ``hidden_0 .. hidden_{n-1}`` plus the head; the critic's value reads its last hidden layer (no dead layer).
Both constructions expose ``hidden_layers`` (in order, the layers the forward uses) and ``out_layer``. ``init``:
``"reference"`` (the initialisers above; Xavier on custom hidden layers) or ``"orthogonal"`` (gain sqrt(2) on hidden
layers, 0.01 on the policy head, 1 on the value head; biases are zero either way).

On GPU the whole actor / critic forward can run as ONE fused kernel with the weights resident in LDS
(``ops.mlp.fused_mlp_forward``; the actor's 99 KiB of fp32 weights fit a CU's 160 KiB LDS).
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn

from .layers import Dense


HIDDEN_ACTS = ("tanh", "relu", "lrelu")
MLP_INITS = ("reference", "orthogonal")
REF_ACTOR_HIDDEN = (128, 128, 64)


def ref_critic_hidden(variant):
    """Hidden widths the reference critic's value path reads (the ``basic`` third layer is built but unused)."""
    return (256, 128, 128) if variant == "a3c" else (256, 128)


def _check_tower_args(who, hidden, activation, init):
    if hidden is not None:
        hidden = tuple(int(w) for w in hidden)
        if not hidden or any(w < 1 for w in hidden):
            raise ValueError(f"{who}: hidden={hidden!r} needs at least one hidden layer of width >= 1")
    if activation is not None and activation not in HIDDEN_ACTS:
        raise ValueError(f"{who}: activation={activation!r}, expected one of {list(HIDDEN_ACTS)}")
    if init not in MLP_INITS:
        raise ValueError(f"{who}: init={init!r}, expected one of {list(MLP_INITS)}")
    return hidden


def _hidden_init(init):
    return ("orthogonal", 2 ** 0.5) if init == "orthogonal" else "xavier"


class MLPActor(nn.Module):
    def __init__(self, ob_dim, ac_dim, discrete=False, ac_scale=2.0, variant="basic", generator=None, hidden=None,
                 activation=None, init="reference"):
        super().__init__()
        self.ob_dim, self.ac_dim, self.discrete, self.variant = ob_dim, ac_dim, discrete, variant
        hidden = _check_tower_args("MLPActor", hidden, activation, init)
        self.custom = hidden is not None or activation is not None
        self.hidden = hidden if hidden is not None else REF_ACTOR_HIDDEN
        self.activation = activation or "lrelu"
        self.init = init
        hk = _hidden_init(init)
        if self.custom:
            k = ob_dim
            for i, w in enumerate(self.hidden):
                setattr(self, f"hidden_{i}", Dense(k, w, self.activation, kernel_init=hk, generator=generator))
                k = w
            self._hidden_names = [f"hidden_{i}" for i in range(len(self.hidden))]
        else:
            self.first_layer = Dense(ob_dim, 128, "lrelu", kernel_init=hk, generator=generator)
            self.second_layer = Dense(128, 128, "lrelu", kernel_init=hk, generator=generator)
            self.third_layer = Dense(128, 64, "lrelu", kernel_init=hk, generator=generator)
            self._hidden_names = ["first_layer", "second_layer", "third_layer"]
        top = self.hidden[-1]
        head_init = ("orthogonal", 0.01) if init == "orthogonal" else None
        if discrete:
            self.logits = Dense(top, ac_dim, None,
                                kernel_init=head_init or ("xavier" if variant == "basic" else "normc"),
                                generator=generator)
        else:
            self.mu_layer = Dense(top, ac_dim, "tanh",
                                  kernel_init=head_init or ("xav" if variant == "basic" else "xavier"),
                                  generator=generator)
            self.log_std = nn.Parameter(torch.zeros(ac_dim))
            scale = np.broadcast_to(np.asarray(ac_scale if ac_scale is not None else 1.0, dtype=np.float32),
                                    (ac_dim,)).copy()
            self.register_buffer("ac_scale", torch.as_tensor(scale))

    @property
    def hidden_layers(self):
        return [getattr(self, n) for n in self._hidden_names]

    @property
    def out_layer(self):
        return self.logits if self.discrete else self.mu_layer

    def trunk(self, ob):
        for lay in self.hidden_layers:
            ob = lay(ob)
        return ob

    def forward(self, ob):
        """-> logits ``[B, A]`` (discrete) or mu ``[B, A]`` (continuous)."""
        h = self.trunk(ob.float())
        if self.discrete:
            return self.logits(h)
        return self.mu_layer(h) * self.ac_scale


class MLPCritic(nn.Module):
    def __init__(self, ob_dim, variant="basic", ob_scale=1.0, generator=None, hidden=None, activation=None,
                 init="reference"):
        super().__init__()
        self.variant = variant
        self.ob_scale = ob_scale
        hidden = _check_tower_args("MLPCritic", hidden, activation, init)
        self.custom = hidden is not None or activation is not None
        self.hidden = hidden if hidden is not None else ref_critic_hidden(variant)
        self.activation = activation or "relu"
        self.init = init
        hk = _hidden_init(init)
        vk = ("orthogonal", 1.0) if init == "orthogonal" else "xavier"
        if self.custom:
            k = ob_dim
            for i, w in enumerate(self.hidden):
                setattr(self, f"hidden_{i}", Dense(k, w, self.activation, kernel_init=hk, generator=generator))
                k = w
            self._hidden_names = [f"hidden_{i}" for i in range(len(self.hidden))]
        else:
            self.first_layer = Dense(ob_dim, 256, "relu", kernel_init=hk, generator=generator)
            self.second_layer = Dense(256, 128, "relu", kernel_init=hk, generator=generator)
            # basic: built with the TF default (glorot) initialiser and unused by the value path
            self.third_layer = Dense(128, 128, "relu", kernel_init=hk, generator=generator)
            self._hidden_names = ["first_layer", "second_layer"] + (["third_layer"] if variant == "a3c" else [])
        self.value = Dense(self.hidden[-1], 1, None, kernel_init=vk, generator=generator)

    @property
    def hidden_layers(self):
        """The hidden layers the value path reads, in order."""
        return [getattr(self, n) for n in self._hidden_names]

    @property
    def out_layer(self):
        return self.value

    def forward(self, ob):
        x1 = ob.float() * self.ob_scale
        for lay in self.hidden_layers:
            x1 = lay(x1)
        return self.value(x1).view(-1)
