"""Scenes of the rigid-body derivative tests (tests/test_rb_derivs_*.py): the tumbling worlds of test_rigid_bodies.py
and the reference's billiard shot (python/examples/billiard_optimization.py, examples/billiard_opt_example_gui.cpp)."""
import math

import numpy as np

import tds_amd
from test_rigid_bodies import make_mixed_worlds, make_worlds  # noqa: F401  (re-exported)

# billiards: six balls in the 1-2-3 rack, the white ball at (0, -2, 0); radius 0.5, mass 1, no gravity, dt 1/60,
# 50 solver iterations, the World's default friction (0.5) and restitution (0)
BILLIARD_DT = 1.0 / 60.0
BILLIARD_TARGET_BALL = 5
BILLIARD_TARGET = np.array([3.5, 8.0, 0.0])
WHITE = 6


def billiard_model():
    bodies = [{"mass": 1.0, "sphere": 0.5} for _ in range(7)]
    return tds_amd.make_rb_model(bodies, dt=BILLIARD_DT, gravity=(0.0, 0.0, 0.0), solver_iterations=50)


def billiard_state(n=1):
    """s0 [n, 7, 13] at rest; the shot goes into the white ball's linear velocity (state entries (6, 7), (6, 8))"""
    r = 0.5
    dx, dy = math.cos(math.pi / 3) * r * 2, math.sin(math.pi / 3) * r * 2
    pos, rx, y = [], 0.0, 0.0
    for column in (1, 2, 3):
        x = rx
        for _ in range(column):
            pos.append((x, y, 0.0))
            x += 2 * r
        rx -= dx
        y += dy
    pos.append((0.0, -2.0, 0.0))
    st = np.zeros((n, 7, 13))
    st[:, :, 0:3] = np.array(pos)
    st[:, :, 6] = 1.0
    return st


def shot_velocity(force):
    """the white ball's velocity after apply_central_force(F) and one apply_force_impulse: F dt / m"""
    return np.asarray(force, dtype=np.float64) * BILLIARD_DT / 1.0


def billiard_cost(sT):
    """||p_target(T) - target||^2 per world, sT [n, 7, 13]"""
    d = sT[..., BILLIARD_TARGET_BALL, 0:3] - BILLIARD_TARGET
    return (d * d).sum(-1)

MIXED_ORDER = ["plane", "s1", "c1", "b1", "s2", "c2", "b2"]
