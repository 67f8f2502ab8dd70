"""Random kinematic trees for the step derivatives and the batched queries (tests/test_tree_derivs_*.py): a fixed,
curated list of models of tests/test_random_trees.py's generator, eight per model class of csrc/tds_diff_classes.h
plus the three class-S trees whose reverse-mode tapes overflow the class's capacity, and 16 seeded states per tree.

The list is chosen so that, per class, every joint type (fixed and the eight 1-dof ones), every shape kind the class
can hold, the three parent styles, fixed and floating bases, pgs_iterations 1 and 2, three root-chain lengths, a tree
at the class's link bound and one at its dof bound occur; every tree's joint-space inertia is positive definite at all
of its 16 states.  tests/test_tree_derivs_cpu.py asserts these facts against the host code and the C oracle."""
import functools
import os
import re

import numpy as np

import tds_amd
import oraclelib  # checker only
from test_random_trees import random_tree_model

CLASSES = ("S", "A", "L")
N_STATES = 16
POOL = 128   # states drawn per tree; the 16 are chosen from them


def case(cls, seed, tape_fits=True, **kw):
    return {"cls": cls, "seed": seed, "kw": kw, "tape_fits": tape_fits,
            "id": f"{cls}-{'floating' if kw.get('floating') else 'fixed'}{seed}"}


# (class, generator seed, generator arguments); tape_fits: every state's step-VJP tape fits the class's capacity
OVERFLOW = [case("S", 105, tape_fits=False), case("S", 113, tape_fits=False), case("S", 116, tape_fits=False)]
_S_FLOATING = dict(floating=True, links=(1, 8), p_fixed=0.6, contact_points=8)
_A_FLOATING = dict(floating=True, links=(6, 14), p_fixed=0.4, contact_points=17)
_L_FIXED = dict(links=(15, 22), p_fixed=0.3, contact_points=4, shapes=("sphere", "capsule"))
_L_FLOATING = dict(floating=True, links=(15, 22), p_fixed=0.5, contact_points=4, shapes=("sphere", "capsule"))
CASES = [
    case("S", 65), case("S", 27), case("S", 42), case("S", 11),
    case("S", 9, links=(8, 8), p_fixed=0.3, contact_points=2),            # 8 links: the link bound
    case("S", 504, **_S_FLOATING), case("S", 893, **_S_FLOATING),        # 8 dofs: the dof bound; 893 carries a box
    case("S", 503, **_S_FLOATING),
    case("A", 97), case("A", 9), case("A", 1), case("A", 6), case("A", 21),
    case("A", 858, **_A_FLOATING),                                        # 14 links, 14 dofs; a box on a floating tree
    case("A", 500, **_A_FLOATING), case("A", 726, floating=True),
    case("L", 2, **_L_FIXED), case("L", 9, **_L_FIXED), case("L", 1, **_L_FIXED),
    case("L", 3, **_L_FIXED),                                             # 18 dofs
    case("L", 858, **_L_FLOATING),                                        # 22 links, 18 dofs
    case("L", 502, **_L_FLOATING),                                        # 22 links
    case("L", 500, **_L_FLOATING), case("L", 503, **_L_FLOATING),
]
ALL = CASES + OVERFLOW


def of_class(cls, cases=None):
    return [c for c in (CASES if cases is None else cases) if c["cls"] == cls]


@functools.lru_cache(maxsize=None)
def class_bounds():
    """{class: (links, dofs, contact points, visuals)} as csrc/tds_diff_classes.h states them"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "tiny-differentiable-simulator_amd", "csrc", "tds_diff_classes.h")) as f:
        found = re.findall(r"using TdsBound([SAL]) = TdsDiffBounds<(\d+), (\d+), (\d+), (\d+)>", f.read())
    return {c: tuple(int(v) for v in b) for c, *b in found}


def contact_points(m):
    need = {tds_amd.model.GEOM_SPHERE: 1, tds_amd.model.GEOM_CAPSULE: 2, tds_amd.model.GEOM_BOX: 8}
    return sum(need.get(m.geoms[g].type, 0) for g in range(m.num_geoms)) if m.has_plane else 0


def model_class(m):
    """tds_jvp_pick restated: the first class whose bound holds the model (None: refused)"""
    ny = m.dof_q + m.dof_qd + (7 * m.num_visuals + 1 if m.pack_visuals else 0)
    for cls in CLASSES:
        nl, nd, nc, nv = class_bounds()[cls]
        if (m.num_links <= nl and m.dof_qd <= nd and contact_points(m) <= nc and m.input_dim <= 3 * nd + 4
                and (not m.pack_visuals or m.num_visuals <= nv) and ny <= 2 * nd + 2 + 7 * nv and m.output_dim >= ny):
            return cls
    return None


def tree(c):
    """(model, length of the massless root chain, parent style) of a case; a new model every call"""
    return random_tree_model(c["seed"], **c["kw"])


def draw_states(m, n_virtual, n, seed):
    """n records as tests/test_random_trees.py draws them for fixed and for floating bases"""
    rng = np.random.default_rng(seed)
    nq, nd, nj = m.dof_q, m.dof_qd, m.action_dim
    x = np.zeros((n, m.input_dim))
    if m.is_floating:
        quat = rng.normal(size=(n, 4))
        x[:, 0:4] = quat / np.linalg.norm(quat, axis=1, keepdims=True)
        x[:, 4:6] = rng.uniform(-1, 1, (n, 2))
        x[:, 6] = rng.uniform(0.0, 0.5, n)
        x[:, 7:nq] = rng.uniform(-0.6, 0.6, (n, nq - 7))
    else:
        x[:, :nd] = rng.uniform(-0.6, 0.6, (n, nd))
        if n_virtual >= 3:
            x[:, 2] = rng.uniform(0.0, 0.4, n)            # height of the virtual base above the plane
    x[:, nq:nq + nd] = rng.uniform(-1, 1, (n, nd))
    x[:, nq + nd:] = rng.uniform(-1, 1, (n, nj))
    return x


def active_contacts(m, x):
    """penetrating contact points of each record [n], by the oracle's narrowphase"""
    if not m.num_geoms:
        return np.zeros(x.shape[0], dtype=np.int64)
    return np.array([int((oraclelib.step_debug(m, xe)["contacts"][:, 9] < 0).sum()) for xe in x])


@functools.lru_cache(maxsize=None)
def states(seed, kw=()):
    """(x [16, input_dim], active contacts [16]) of the tree (seed, sorted generator arguments): the first state with
    the fewest and the first with the most active contacts among POOL seeded ones, then the first 14 of the others.
    Shared by the tests: read-only."""
    m, n_virtual, _ = random_tree_model(seed, **dict(kw))
    pool = draw_states(m, n_virtual, POOL, 7000 + seed)
    counts = active_contacts(m, pool)
    lo, hi = int(np.argmin(counts)), int(np.argmax(counts))
    rest = [i for i in range(POOL) if i not in (lo, hi)][:N_STATES - len({lo, hi})]
    idx = np.array(sorted({lo, hi}) + rest)
    x = np.ascontiguousarray(pool[idx])
    x.setflags(write=False)
    return x, counts[idx]


def states_of(c):
    return states(c["seed"], tuple(sorted(c["kw"].items())))
