"""fp64 numpy step functions of gym 0.21's Acrobot-v1, MountainCar-v0 and MountainCarContinuous-v0, written from the
published equations of motion. Independent of ``envs/classic.py``: scalar maths per env, plain ``while`` wraps, no
shared constants or helpers. Each function takes one state (and action) and returns
``(next_state, reward, terminated)``.
"""
import math

import numpy as np


# ---------------------------------------------------------------------------------------------------- Acrobot-v1
def _acrobot_rhs(y, torque):
    m1 = m2 = 1.0
    l1 = 1.0
    lc1 = lc2 = 0.5
    i1 = i2 = 1.0
    g = 9.8
    theta1, theta2, dtheta1, dtheta2 = y
    d1 = m1 * lc1 ** 2 + m2 * (l1 ** 2 + lc2 ** 2 + 2 * l1 * lc2 * math.cos(theta2)) + i1 + i2
    d2 = m2 * (lc2 ** 2 + l1 * lc2 * math.cos(theta2)) + i2
    phi2 = m2 * lc2 * g * math.cos(theta1 + theta2 - math.pi / 2.0)
    phi1 = (-m2 * l1 * lc2 * dtheta2 ** 2 * math.sin(theta2)
            - 2 * m2 * l1 * lc2 * dtheta2 * dtheta1 * math.sin(theta2)
            + (m1 * lc1 + m2 * l1) * g * math.cos(theta1 - math.pi / 2.0) + phi2)
    ddtheta2 = ((torque + d2 / d1 * phi1 - m2 * l1 * lc2 * dtheta1 ** 2 * math.sin(theta2) - phi2)
                / (m2 * lc2 ** 2 + i2 - d2 ** 2 / d1))
    ddtheta1 = -(d2 * ddtheta2 + phi1) / d1
    return np.array([dtheta1, dtheta2, ddtheta1, ddtheta2], dtype=np.float64)


def _wrap(x, lo, hi):
    span = hi - lo
    while x > hi:
        x -= span
    while x < lo:
        x += span
    return x


def acrobot_step(state, action):
    y0 = np.asarray(state, dtype=np.float64)
    torque = float(int(action) - 1)
    dt = 0.2
    k1 = _acrobot_rhs(y0, torque)
    k2 = _acrobot_rhs(y0 + dt / 2.0 * k1, torque)
    k3 = _acrobot_rhs(y0 + dt / 2.0 * k2, torque)
    k4 = _acrobot_rhs(y0 + dt * k3, torque)
    y = y0 + dt / 6.0 * (k1 + 2 * k2 + 2 * k3 + k4)
    y[0] = _wrap(y[0], -math.pi, math.pi)
    y[1] = _wrap(y[1], -math.pi, math.pi)
    y[2] = min(max(y[2], -4 * math.pi), 4 * math.pi)
    y[3] = min(max(y[3], -9 * math.pi), 9 * math.pi)
    terminated = bool(-math.cos(y[0]) - math.cos(y[1] + y[0]) > 1.0)
    return y, (0.0 if terminated else -1.0), terminated


def acrobot_obs(state):
    t1, t2, w1, w2 = (float(x) for x in state)
    return np.array([math.cos(t1), math.sin(t1), math.cos(t2), math.sin(t2), w1, w2], dtype=np.float64)


def acrobot_height(state):
    """Tip height above the pivot in link lengths; the goal is ``> 1``."""
    return -math.cos(state[0]) - math.cos(state[1] + state[0])


# ---------------------------------------------------------------------------------------------------- MountainCar
def _car(position, velocity, push, goal):
    velocity += push - 0.0025 * math.cos(3 * position)
    velocity = min(max(velocity, -0.07), 0.07)
    position += velocity
    position = min(max(position, -1.2), 0.6)
    if position == -1.2 and velocity < 0:
        velocity = 0.0
    return position, velocity, bool(position >= goal and velocity >= 0)


def mountaincar_step(state, action):
    p, v, terminated = _car(float(state[0]), float(state[1]), (int(action) - 1) * 0.001, 0.5)
    return np.array([p, v], dtype=np.float64), -1.0, terminated


def mountaincar_cont_step(state, u):
    u = float(u)
    force = min(max(u, -1.0), 1.0)
    p, v, terminated = _car(float(state[0]), float(state[1]), force * 0.0015, 0.45)
    reward = (100.0 if terminated else 0.0) - 0.1 * u * u
    return np.array([p, v], dtype=np.float64), reward, terminated
