"""Classic-control envs with the exact gym equations (gym itself is not installed -- SURVEY §7.5 item 8).

* ``CartPole-v0`` / ``CartPole-v1``: gym ``CartPoleEnv`` (Euler integrator, 12 deg / 2.4 thresholds, reward 1
  per step including the terminating one); TimeLimit 200 / 500.
* ``Pendulum-v0``: gym ``PendulumEnv`` v0 (``thdot += (-3g/(2l) sin(th+pi) + 3/(ml^2) u) dt`` ...);
  reward ``-(angle_normalize(th)^2 + .1 thdot^2 + .001 u^2)``; TimeLimit 200; no termination.
* ``Acrobot-v1``: gym 0.21 ``AcrobotEnv`` ("book" dynamics, one classical RK4 step of 0.2 s, angles wrapped and
  velocities clamped after the step); reward -1 per step, 0 on the step that swings the tip above the bar;
  TimeLimit 500.
* ``MountainCar-v0`` / ``MountainCarContinuous-v0``: gym ``MountainCarEnv`` / ``Continuous_MountainCarEnv`` (clamped
  velocity and position, the left wall stops the car); TimeLimit 200 / 999. The continuous task pays 100 at the
  goal minus ``0.1 u^2`` of the unclipped action.

CartPole and Pendulum are the envs the reference trains on (``README.md``, ``Basic_AC/run_AC.py:13``). Random resets
use the counter-based hash RNG (:mod:`.rng`) so the HIP kernels (``csrc/kernels/env_classic.hip``: one task struct per
env around one bank-step kernel, launched by :meth:`VecEnv._native_step` through ``native_op``) reproduce them.
"""
from __future__ import annotations

import math

import torch

from . import rng
from .base import VecEnv
from .spaces import Box, Discrete


class CartPoleVecEnv(VecEnv):
    env_id = "CartPole-v1"
    native_op = "env_step_cartpole"
    state_dim = 4
    default_max_steps = 500
    observation_space = Box(low=[-4.8, -3.4e38, -0.419, -3.4e38], high=[4.8, 3.4e38, 0.419, 3.4e38])
    action_space = Discrete(2)

    GRAVITY, MASSCART, MASSPOLE, LENGTH, FORCE_MAG, TAU = 9.8, 1.0, 0.1, 0.5, 10.0, 0.02
    THETA_LIMIT = 12 * 2 * math.pi / 360
    X_LIMIT = 2.4

    @property
    def frame_shape(self):
        return (4,)

    def _reset_state(self, mask):
        ids = self.env_ids
        for j in range(4):
            u = rng.uniform(self.seed, ids, self.tg, 100 + j)
            self.state[:, j] = torch.where(mask, u * 0.1 - 0.05, self.state[:, j])

    def _dynamics(self, actions):
        x, x_dot, th, th_dot = self.state.unbind(1)
        total_mass = self.MASSPOLE + self.MASSCART
        pml = self.MASSPOLE * self.LENGTH
        force = torch.where(actions.view(-1).long() == 1, torch.full_like(x, self.FORCE_MAG),
                            torch.full_like(x, -self.FORCE_MAG))
        c, s = torch.cos(th), torch.sin(th)
        temp = (force + pml * th_dot * th_dot * s) / total_mass
        thacc = (self.GRAVITY * s - c * temp) / (self.LENGTH * (4.0 / 3.0 - self.MASSPOLE * c * c / total_mass))
        xacc = temp - pml * thacc * c / total_mass
        x = x + self.TAU * x_dot
        x_dot = x_dot + self.TAU * xacc
        th = th + self.TAU * th_dot
        th_dot = th_dot + self.TAU * thacc
        self.state.copy_(torch.stack([x, x_dot, th, th_dot], 1))
        term = (x < -self.X_LIMIT) | (x > self.X_LIMIT) | (th < -self.THETA_LIMIT) | (th > self.THETA_LIMIT)
        return torch.ones_like(x), term

    def _frame(self):
        return self.state.clone()


class CartPoleV0VecEnv(CartPoleVecEnv):
    env_id = "CartPole-v0"
    default_max_steps = 200


def angle_normalize(x):
    return torch.remainder(x + math.pi, 2 * math.pi) - math.pi


class PendulumVecEnv(VecEnv):
    env_id = "Pendulum-v0"
    native_op = "env_step_pendulum"
    state_dim = 2
    default_max_steps = 200
    observation_space = Box(low=[-1.0, -1.0, -8.0], high=[1.0, 1.0, 8.0])
    action_space = Box(low=[-2.0], high=[2.0])

    MAX_SPEED, MAX_TORQUE, DT, G, M, L = 8.0, 2.0, 0.05, 10.0, 1.0, 1.0

    @property
    def frame_shape(self):
        return (3,)

    def _reset_state(self, mask):
        ids = self.env_ids
        th = rng.uniform(self.seed, ids, self.tg, 100) * (2 * math.pi) - math.pi
        thd = rng.uniform(self.seed, ids, self.tg, 101) * 2.0 - 1.0
        self.state[:, 0] = torch.where(mask, th, self.state[:, 0])
        self.state[:, 1] = torch.where(mask, thd, self.state[:, 1])

    def _dynamics(self, actions):
        th, thdot = self.state.unbind(1)
        u = torch.clamp(actions.reshape(self.num_envs, -1)[:, 0].float(), -self.MAX_TORQUE, self.MAX_TORQUE)
        costs = angle_normalize(th) ** 2 + 0.1 * thdot ** 2 + 0.001 * (u ** 2)
        newthdot = thdot + (-3 * self.G / (2 * self.L) * torch.sin(th + math.pi)
                            + 3.0 / (self.M * self.L ** 2) * u) * self.DT
        newth = th + newthdot * self.DT
        newthdot = torch.clamp(newthdot, -self.MAX_SPEED, self.MAX_SPEED)
        self.state.copy_(torch.stack([newth, newthdot], 1))
        return -costs, torch.zeros_like(th, dtype=torch.bool)

    def _frame(self):
        th, thdot = self.state.unbind(1)
        return torch.stack([torch.cos(th), torch.sin(th), thdot], 1)


def _f32(x):
    """The fp32 value of a constant as a Python float: comparisons against it are exact in either precision."""
    return torch.tensor(x, dtype=torch.float32).item()


def _wrap(x, lo, hi):
    """gym ``acrobot.wrap``: repeated -+(hi - lo) until lo <= x <= hi (at most WRAP_ITERS times, as the kernel; one RK4
    step from clamped velocities moves an angle by far less than 16 turns)."""
    diff = hi - lo
    for _ in range(AcrobotVecEnv.WRAP_ITERS):
        over = x > hi
        if x.device.type == "cpu" and not bool(over.any()):   # no host sync on a device bank: all iterations run
            break
        x = torch.where(over, x - diff, x)
    for _ in range(AcrobotVecEnv.WRAP_ITERS):
        under = x < lo
        if x.device.type == "cpu" and not bool(under.any()):
            break
        x = torch.where(under, x + diff, x)
    return x


class AcrobotVecEnv(VecEnv):
    env_id = "Acrobot-v1"
    native_op = "env_step_acrobot"
    state_dim = 4
    default_max_steps = 500
    observation_space = Box(low=[-1.0, -1.0, -1.0, -1.0, -4 * math.pi, -9 * math.pi],
                            high=[1.0, 1.0, 1.0, 1.0, 4 * math.pi, 9 * math.pi])
    action_space = Discrete(3)

    DT, M1, M2, L1, LC1, LC2, I1, I2, G = 0.2, 1.0, 1.0, 1.0, 0.5, 0.5, 1.0, 1.0, 9.8
    MAX_VEL_1, MAX_VEL_2 = 4 * math.pi, 9 * math.pi
    WRAP_ITERS = 16
    PI = _f32(math.pi)

    @property
    def frame_shape(self):
        return (6,)

    def _reset_state(self, mask):
        ids = self.env_ids
        for j in range(4):
            u = rng.uniform(self.seed, ids, self.tg, 100 + j)
            self.state[:, j] = torch.where(mask, u * 0.2 - 0.1, self.state[:, j])

    def _dsdt(self, th1, th2, w1, w2, a):
        """(alpha1, alpha2) of the "book" equations of motion; the kernel's ``acrobot_dsdt`` is the same sequence."""
        m1, m2, l1, lc1, lc2, i1, i2, g = self.M1, self.M2, self.L1, self.LC1, self.LC2, self.I1, self.I2, self.G
        c2, s2 = torch.cos(th2), torch.sin(th2)
        d1 = m1 * lc1 ** 2 + m2 * (l1 ** 2 + lc2 ** 2 + 2 * l1 * lc2 * c2) + i1 + i2
        d2 = m2 * (lc2 ** 2 + l1 * lc2 * c2) + i2
        phi2 = m2 * lc2 * g * torch.cos(th1 + th2 - math.pi / 2)
        phi1 = (-m2 * l1 * lc2 * w2 * w2 * s2 - 2 * m2 * l1 * lc2 * w2 * w1 * s2
                + (m1 * lc1 + m2 * l1) * g * torch.cos(th1 - math.pi / 2) + phi2)
        a2 = (a + d2 / d1 * phi1 - m2 * l1 * lc2 * w1 * w1 * s2 - phi2) / (m2 * lc2 ** 2 + i2 - d2 * d2 / d1)
        a1 = -(d2 * a2 + phi1) / d1
        return a1, a2

    def _dynamics(self, actions):
        s = self.state.unbind(1)
        a = (actions.view(-1).long() - 1).float()
        dt = self.DT

        def f(y):
            a1, a2 = self._dsdt(y[0], y[1], y[2], y[3], a)
            return (y[2], y[3], a1, a2)

        k1 = f(s)
        k2 = f(tuple(s[j] + dt / 2 * k1[j] for j in range(4)))
        k3 = f(tuple(s[j] + dt / 2 * k2[j] for j in range(4)))
        k4 = f(tuple(s[j] + dt * k3[j] for j in range(4)))
        th1, th2, w1, w2 = (s[j] + dt / 6.0 * (k1[j] + 2 * k2[j] + 2 * k3[j] + k4[j]) for j in range(4))
        th1 = _wrap(th1, -self.PI, self.PI)
        th2 = _wrap(th2, -self.PI, self.PI)
        w1 = torch.clamp(w1, -self.MAX_VEL_1, self.MAX_VEL_1)
        w2 = torch.clamp(w2, -self.MAX_VEL_2, self.MAX_VEL_2)
        self.state.copy_(torch.stack([th1, th2, w1, w2], 1))
        term = (-torch.cos(th1) - torch.cos(th2 + th1)) > 1.0
        return torch.where(term, torch.zeros_like(th1), torch.full_like(th1, -1.0)), term

    def _frame(self):
        th1, th2, w1, w2 = self.state.unbind(1)
        return torch.stack([torch.cos(th1), torch.sin(th1), torch.cos(th2), torch.sin(th2), w1, w2], 1)


class MountainCarVecEnv(VecEnv):
    env_id = "MountainCar-v0"
    native_op = "env_step_mountaincar"
    state_dim = 2
    default_max_steps = 200
    observation_space = Box(low=[-1.2, -0.07], high=[0.6, 0.07])
    action_space = Discrete(3)

    MIN_POS, MAX_POS, MAX_SPEED, GOAL_POS = _f32(-1.2), _f32(0.6), _f32(0.07), _f32(0.5)
    FORCE, GRAVITY = 0.001, 0.0025

    @property
    def frame_shape(self):
        return (2,)

    def _reset_state(self, mask):
        u = rng.uniform(self.seed, self.env_ids, self.tg, 100)
        self.state[:, 0] = torch.where(mask, u * 0.2 - 0.6, self.state[:, 0])
        self.state[:, 1] = torch.where(mask, torch.zeros_like(u), self.state[:, 1])

    def _force(self, actions):
        return (actions.view(-1).long() - 1).float()

    def _move(self, f):
        """The shared car step for a unit force ``f``: clamped velocity and position, and the left wall."""
        p, v = self.state.unbind(1)
        v = v + (f * self.FORCE + torch.cos(3 * p) * (-self.GRAVITY))
        v = torch.clamp(v, -self.MAX_SPEED, self.MAX_SPEED)
        p = torch.clamp(p + v, self.MIN_POS, self.MAX_POS)
        v = torch.where((p == self.MIN_POS) & (v < 0), torch.zeros_like(v), v)
        self.state.copy_(torch.stack([p, v], 1))
        return (p >= self.GOAL_POS) & (v >= 0)

    def _dynamics(self, actions):
        term = self._move(self._force(actions))
        return torch.full_like(self.state[:, 0], -1.0), term

    def _frame(self):
        return self.state.clone()


class MountainCarContinuousVecEnv(MountainCarVecEnv):
    env_id = "MountainCarContinuous-v0"
    native_op = "env_step_mountaincar_cont"
    default_max_steps = 999
    action_space = Box(low=[-1.0], high=[1.0])

    GOAL_POS = _f32(0.45)
    FORCE = 0.0015

    def _dynamics(self, actions):
        u = actions.reshape(self.num_envs, -1)[:, 0].float()
        term = self._move(torch.clamp(u, -1.0, 1.0))
        # the action penalty reads the unclipped action (gym Continuous_MountainCarEnv.step)
        return torch.where(term, torch.full_like(u, 100.0), torch.zeros_like(u)) - (u * u) * 0.1, term
