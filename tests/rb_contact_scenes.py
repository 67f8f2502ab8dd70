"""Directed scenes of the rigid-body contact tests (tests/test_rb_contacts.py, oracle/gen_golden_rb.py): one scene per
branch of the reference's collision dispatcher (contact_point.hpp:444-496), per pair it skips, per guarded division,
and heaps at 10 and 16 bodies (TDS_RB_MAX_BODIES).  A scene is N worlds of one model from a fixed seed; every state
entry is float32-representable, so that one f64 reference result serves the f64 and the f32 kernel ("the f32-rounded
state" is the state).  The model values are ordinary decimals (dt 1/60, g 9.81, masses 0.7 ...): each path rounds them
itself.

Velocities are the ones the solver sees: the builder subtracts the gravity impulse g dt that World::step adds first."""
import hashlib

import numpy as np

import tds_amd

N = 32
DT = 1.0 / 60.0
G = (0.0, 0.0, -9.81)
PLANE = (0.51, -0.34, 1.7, 0.25)              # tilted, non-unit normal, non-zero constant
S1, S2 = {"mass": 0.7, "sphere": 0.15}, {"mass": 1.3, "sphere": 0.22}
CAP = {"mass": 1.2, "capsule": (0.08, 0.40)}
CAP2 = {"mass": 0.9, "capsule": (0.10, 0.25)}
BOX = {"mass": 2.0, "box": (0.30, 0.20, 0.25)}
BOX2 = {"mass": 1.5, "box": (0.20, 0.20, 0.20)}
BOX_RADIUS = 1e-2                             # contact_point.hpp:181-182 (a Box's own radius is 0)


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _rand_dir(rng, n):
    return _unit(rng.normal(size=(n, 3)))


def _rand_quat(rng, n):
    return _unit(rng.normal(size=(n, 4)))


def quat_rot(q, v):
    """q v q^-1, q [n, 4] as (x, y, z, w), v [3] or [n, 3]"""
    u, w = q[:, :3], q[:, 3:4]
    v = np.broadcast_to(v, u.shape)
    t = 2.0 * np.cross(u, v)
    return v + w * t + np.cross(u, t)


def _plane_frame(plane):
    nh = np.array(plane[:3]) / np.linalg.norm(plane[:3])
    t1 = _unit(np.cross(nh, [1.0, 0.0, 0.0]))
    return nh, t1, np.cross(nh, t1), plane[3]


def _lateral(rng, n, axis, speed):
    """[n, 3] orthogonal to axis [n, 3] (or [3]), of length speed ([n] or scalar)"""
    axis = np.broadcast_to(axis, (n, 3))
    r = rng.normal(size=(n, 3))
    r = _unit(r - (r * axis).sum(-1, keepdims=True) * axis)
    return r * np.broadcast_to(np.asarray(speed, dtype=np.float64), (n,))[:, None]


def _spheres_of(body, q):
    """centres of a body's collision spheres relative to its position [n, k, 3], and their radius"""
    n = q.shape[0]
    if "sphere" in body:
        return np.zeros((n, 1, 3)), body["sphere"]
    if "capsule" in body:
        r, ln = body["capsule"]
        return np.stack([quat_rot(q, np.array([0, 0, s * 0.5 * ln])) for s in (1, -1)], 1), r
    ex = np.array(body["box"]) * 0.5 - BOX_RADIUS
    offs = [np.array([sx, sy, sz]) * ex for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)]
    return np.stack([quat_rot(q, o) for o in offs], 1), BOX_RADIUS


def _lat_speed(rng, n, variant):
    return {"slide": rng.uniform(2.8, 3.2, n), "stick": rng.uniform(0.008, 0.012, n)}.get(variant, rng.uniform(0.3, 1.5, n))


def _blank(n, nb):
    st = np.zeros((n, nb, 13))
    st[:, :, 6] = 1.0
    return st


def _put(st, b, pos, q, lin, ang, dynamic=True):
    st[:, b, 0:3], st[:, b, 3:7], st[:, b, 10:13] = pos, q, ang
    st[:, b, 7:10] = lin - (np.array(G) * DT if dynamic else 0.0)


def _on_plane(rng, n, body, plane, variant=None):
    """pose and velocity of a body pressed into the plane and approaching it"""
    nh, t1, t2, c = _plane_frame(plane)
    q = _rand_quat(rng, n)
    offs, rad = _spheres_of(body, q)
    low = (offs @ nh).min(1)                                       # lowest collision sphere, along the normal
    depth = rng.uniform(-0.03, 0.008, n) if "box" in body else rad * rng.uniform(0.5, 0.9, n)
    h = c + depth - low
    pos = rng.uniform(-0.5, 0.5, (n, 1)) * t1 + rng.uniform(-0.5, 0.5, (n, 1)) * t2 + h[:, None] * nh
    if "sphere" in body:
        lin = -nh * rng.uniform(0.5, 2.0, (n, 1)) + _lateral(rng, n, nh, _lat_speed(rng, n, variant))
        # the contact point lies along the normal: spin about it adds no lateral velocity to the "stick" variant
        ang = nh * rng.uniform(-2, 2, (n, 1)) if variant == "stick" else rng.uniform(-2, 2, (n, 3))
    else:
        lin = -nh * rng.uniform(1.0, 2.5, (n, 1)) + _lateral(rng, n, nh, _lat_speed(rng, n, variant))
        ang = rng.uniform(-1.5, 1.5, (n, 3))
    return pos, q, lin, ang


def _plane_pair(rng, n, body, plane_first, variant=None):
    st = _blank(n, 2)
    _put(st, 1 if plane_first else 0, *_on_plane(rng, n, body, PLANE, variant))
    pl = {"mass": 0.0, "plane": PLANE}
    return ([pl, body] if plane_first else [body, pl]), st


def _sphere_pair(rng, n, a, b, variant=None, coincident=False):
    """two overlapping spheres approaching along the line of centres; a or b may be static (mass 0)"""
    st = _blank(n, 2)
    d = _rand_dir(rng, n)                                          # from a to b
    pa = rng.uniform(-0.5, 0.5, (n, 3))
    pb = pa if coincident else pa + d * ((a["sphere"] + b["sphere"]) * rng.uniform(0.6, 0.95, (n, 1)))
    drift = rng.uniform(-0.5, 0.5, (n, 3))
    lat = _lateral(rng, n, d, _lat_speed(rng, n, variant))
    spin = (lambda: d * rng.uniform(-3, 3, (n, 1))) if variant == "stick" else (lambda: rng.uniform(-3, 3, (n, 3)))
    va = drift + d * rng.uniform(0.8, 2.0, (n, 1)) + lat
    vb = drift - d * rng.uniform(0.8, 2.0, (n, 1))
    if a["mass"] == 0.0:
        va, vb = np.zeros((n, 3)), vb - va
    if b["mass"] == 0.0:
        va, vb = va - vb, np.zeros((n, 3))
    _put(st, 0, pa, _rand_quat(rng, n), va, spin(), a["mass"] != 0.0)
    _put(st, 1, pb, _rand_quat(rng, n), vb, spin(), b["mass"] != 0.0)
    return [a, b], st


def _capsule_sphere(rng, n, capsule_first):
    """a sphere pressed into one end cap of a capsule"""
    st = _blank(n, 2)
    r, ln = CAP["capsule"]
    q = _rand_quat(rng, n)
    pc = rng.uniform(-0.5, 0.5, (n, 3))
    end = quat_rot(q, np.array([0.0, 0.0, 0.5 * ln])) * rng.choice([-1.0, 1.0], (n, 1))
    d = _unit(_unit(end) + 0.8 * _rand_dir(rng, n))               # outwards from the cap, give or take
    ps = pc + end + d * ((r + S1["sphere"]) * rng.uniform(0.6, 0.95, (n, 1)))
    vc = d * rng.uniform(0.3, 1.0, (n, 1)) + rng.uniform(-0.3, 0.3, (n, 3))
    vs = -d * rng.uniform(1.0, 2.5, (n, 1)) + _lateral(rng, n, d, rng.uniform(0.3, 1.5, n))
    c, s = (0, 1) if capsule_first else (1, 0)
    _put(st, c, pc, q, vc, rng.uniform(-1.5, 1.5, (n, 3)))
    _put(st, s, ps, _rand_quat(rng, n), vs, rng.uniform(-3, 3, (n, 3)))
    return ([CAP, S1] if capsule_first else [S1, CAP]), st


def _skipped(rng, n, a, b):
    """two bodies the dispatcher has no function for, overlapping and approaching"""
    st = _blank(n, 2)
    d = _rand_dir(rng, n)
    pa = rng.uniform(-0.5, 0.5, (n, 3))
    for i, (body, pos, s) in enumerate(((a, pa, 1.0), (b, pa + 0.05 * d, -1.0))):
        _put(st, i, pos, _rand_quat(rng, n), s * d * rng.uniform(0.5, 2.0, (n, 1)), rng.uniform(-2, 2, (n, 3)),
             body["mass"] != 0.0)
    return [a, b], st


def _heap(rng, n, count, plane_at):
    """`count` mixed bodies dropped into a heap on the tilted plane, the plane at index plane_at of the body order"""
    kinds = [S1, CAP, BOX, S2, CAP2, BOX2, S1, S2]
    bodies = [dict(kinds[i % len(kinds)], mass=round(0.5 + 0.1 * i, 1)) for i in range(count)]
    pl = {"mass": 0.0, "plane": PLANE}
    order = bodies[:plane_at] + [pl] + bodies[plane_at:]
    st = _blank(n, count + 1)
    nh, t1, t2, c = _plane_frame(PLANE)
    for i, body in enumerate(order):
        if "plane" in body:
            continue
        pos, q, lin, ang = _on_plane(rng, n, body, PLANE)
        if i % 3:                                                  # two in three sit higher up in the heap
            pos = pos + nh * rng.uniform(0.05, 0.45, (n, 1))
        pos = pos - (pos @ t1)[:, None] * t1 * 0.6 - (pos @ t2)[:, None] * t2 * 0.6      # pull the heap together
        _put(st, i, pos, q, lin, ang)
    return order, st


def _drop(rng, n):
    """a sphere falling straight onto a horizontal plane, no spin: the lateral velocity is exactly 0"""
    st = _blank(n, 2)
    st[:, 1, 0:2] = rng.uniform(-0.5, 0.5, (n, 2))
    st[:, 1, 2] = S1["sphere"] * rng.uniform(0.5, 0.9, n)
    st[:, 1, 9] = -rng.uniform(0.5, 2.0, n)
    return [{"mass": 0.0, "plane": (0.0, 0.0, 1.0, 0.0)}, S1], st


def _three(rng, n):
    """sphere | plane | capsule, both pressed into the plane (the plane in the middle: one pair runs swapped)"""
    st = _blank(n, 3)
    _put(st, 0, *_on_plane(rng, n, S1, PLANE))
    _put(st, 2, *_on_plane(rng, n, CAP, PLANE))
    return [S1, {"mass": 0.0, "plane": PLANE}, CAP], st


_PL = {"mass": 0.0, "plane": PLANE}
_STATIC = {"mass": 0.0, "sphere": 0.22}
# name -> (builder(rng, n), solver_iterations, kind); kind: "hit" (the pair collides), "skip" (the dispatcher skips it),
# "edge", "heap".  The seed of a scene is its position in this table.
TABLE = [
    ("plane_sphere", lambda r, n: _plane_pair(r, n, S1, True), 1, "hit"),
    ("sphere_plane", lambda r, n: _plane_pair(r, n, S1, False), 1, "hit"),
    ("plane_capsule", lambda r, n: _plane_pair(r, n, CAP, True), 1, "hit"),
    ("capsule_plane", lambda r, n: _plane_pair(r, n, CAP, False), 1, "hit"),
    ("plane_box", lambda r, n: _plane_pair(r, n, BOX, True), 1, "hit"),
    ("box_plane", lambda r, n: _plane_pair(r, n, BOX, False), 1, "hit"),
    ("sphere_sphere", lambda r, n: _sphere_pair(r, n, S1, S2), 1, "hit"),
    ("capsule_sphere", lambda r, n: _capsule_sphere(r, n, True), 1, "hit"),
    ("sphere_capsule", lambda r, n: _capsule_sphere(r, n, False), 1, "hit"),
    ("static_sphere_sphere", lambda r, n: _sphere_pair(r, n, _STATIC, S1), 1, "hit"),
    ("sphere_static_sphere", lambda r, n: _sphere_pair(r, n, S1, _STATIC), 1, "hit"),
    ("sphere_plane_it4", lambda r, n: _plane_pair(r, n, S2, False), 4, "hit"),
    ("plane_box_it4", lambda r, n: _plane_pair(r, n, BOX2, True), 4, "hit"),
    ("sphere_sphere_it4", lambda r, n: _sphere_pair(r, n, S2, S1), 4, "hit"),
    ("capsule_sphere_it4", lambda r, n: _capsule_sphere(r, n, True), 4, "hit"),
    ("plane_sphere_slide", lambda r, n: _plane_pair(r, n, S1, True, "slide"), 1, "hit"),
    ("plane_sphere_stick", lambda r, n: _plane_pair(r, n, S1, True, "stick"), 1, "hit"),
    ("sphere_plane_slide", lambda r, n: _plane_pair(r, n, S2, False, "slide"), 1, "hit"),
    ("sphere_plane_stick", lambda r, n: _plane_pair(r, n, S2, False, "stick"), 1, "hit"),
    ("sphere_sphere_slide", lambda r, n: _sphere_pair(r, n, S1, S2, "slide"), 1, "hit"),
    ("sphere_sphere_stick", lambda r, n: _sphere_pair(r, n, S1, S2, "stick"), 1, "hit"),
    ("capsule_capsule", lambda r, n: _skipped(r, n, CAP, CAP2), 2, "skip"),
    ("box_sphere", lambda r, n: _skipped(r, n, BOX, S1), 2, "skip"),
    ("box_capsule", lambda r, n: _skipped(r, n, BOX, CAP), 2, "skip"),
    ("box_box", lambda r, n: _skipped(r, n, BOX, BOX2), 2, "skip"),
    ("plane_plane", lambda r, n: _skipped(r, n, _PL, {"mass": 1.0, "plane": (0.0, 0.3, 1.0, 0.1)}), 2, "skip"),
    ("coincident_spheres", lambda r, n: _sphere_pair(r, n, S1, S2, coincident=True), 2, "edge"),
    ("straight_drop", _drop, 2, "edge"),
    ("no_iterations", _three, 0, "edge"),
    ("heap10_plane_first", lambda r, n: _heap(r, n, 9, 0), 3, "heap"),
    ("heap10_plane_mid", lambda r, n: _heap(r, n, 9, 4), 3, "heap"),
    ("heap16_plane_first", lambda r, n: _heap(r, n, 15, 0), 3, "heap"),
    ("heap16_plane_mid", lambda r, n: _heap(r, n, 15, 8), 3, "heap"),
    ("three_bodies", _three, 2, "hit"),
]
NAMES = [t[0] for t in TABLE]
KIND = {t[0]: t[3] for t in TABLE}
HEAPS = [n for n in NAMES if KIND[n] == "heap"]
SEED0 = 20260


def scene(name, n=N, iters=None):
    """(model, state [n, nb, 13], bodies) of a scene; iters overrides its solver_iterations"""
    idx = NAMES.index(name)
    _, builder, its, _ = TABLE[idx]
    bodies, st = builder(np.random.default_rng(SEED0 + idx), n)
    st = st.astype(np.float32).astype(np.float64)
    m = tds_amd.make_rb_model(bodies, dt=DT, gravity=G, solver_iterations=its if iters is None else iters,
                              friction=0.5, restitution=0.2)
    return m, st, bodies


def digest(m, st):
    """hash of a scene's inputs: the model struct's bytes and the state"""
    return hashlib.sha256(bytes(m) + np.ascontiguousarray(st).tobytes()).hexdigest()


def perturbation_spread(step, m, st, eps, draws=16, seed=4242):
    """U of a scene for a number format with machine epsilon eps: the largest change of step(m, .)'s result over all
    worlds and `draws` draws in which every state entry is multiplied by 1 + d eps, d random in {-1, 0, 1}"""
    rng = np.random.default_rng(seed)
    y0 = step(m, st, 1)
    u = 0.0
    for _ in range(draws):
        d = rng.integers(-1, 2, st.shape).astype(np.float64)
        u = max(u, float(np.abs(step(m, st * (1.0 + d * eps), 1) - y0).max()))
    return u
