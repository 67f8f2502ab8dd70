"""Synthetic stars for the 8- and the 16-lane step kernels (csrc/tds_oct.hip, csrc/tds_quad.hip;
tests/test_star_kernels_*.py): a generator that perturbs the Ant and Laikago in everything the kernels' detection leaves
free (tds_oct_detect, the quad block of csrc/tds_device_model.h), a fixed, curated list of stars per kind with the
unmodified models as its known-good end, and 67 seeded states per star.

What the detection fixes stays: the closed-form root chain on links 0..4 and link 5's joint, four legs of two jointed
links (oct) or three jointed links and a fixed toe (quad), PD actuation on leg joints only, one capsule per leg link and
the root sphere (oct) or one sphere per toe (quad), visuals 0 or one per link from link 5 on.  What the kernels read from
their constant tables moves: joint types and axes, leg X_T, masses, centres of mass, full inertias, springs and dampers,
initial poses, the shapes' sizes and frames, the plane, cfm / erp / friction / restitution, pgs_iterations, action_limit,
the reward rule, the visuals and their frames and, for quad, where the PD loop starts.

The list is chosen so that, per kind, the facts of tests/test_star_kernels_cpu.py's coverage test hold; that test asserts
them against this file, with the oracle's largest |y| per star (MAX_ABS_Y below: the inputs' conditioning, below 1e3)."""
import functools

import numpy as np

import tds_amd
import oraclelib  # checker only
from test_oct import _contact_states

J = tds_amd.model
KINDS = ("oct", "quad")
BASE = {"oct": "ant", "quad": "laikago"}
KERNEL = {"oct": "oct8", "quad": "quad16"}
N_STATES = 67   # a ragged last workgroup for 8, for 4 and for 32 environments per workgroup
POOL = 384      # states drawn per star; the 67 are chosen from them
JOINT_KINDS = [J.JOINT_REVOLUTE_X, J.JOINT_REVOLUTE_Y, J.JOINT_REVOLUTE_Z, J.JOINT_REVOLUTE_AXIS, J.JOINT_PRISMATIC_X,
               J.JOINT_PRISMATIC_Y, J.JOINT_PRISMATIC_Z, J.JOINT_PRISMATIC_AXIS]
REVOLUTE = JOINT_KINDS[:4]
PRISMATIC = JOINT_KINDS[4:]
REWARDS = (J.TDS_REWARD_NONE, J.TDS_REWARD_ANT, J.TDS_REWARD_LAIKAGO)  # (the humanoid rule needs a spherical root joint)
# penetrating contact points a star's states must show, as (lo, hi) bins, both ends included
CONTACT_BINS = {"oct": [(0, 0), (1, 1), (2, 2), (3, 3), (4, 4), (5, 8), (9, 12), (13, 17)],
                "quad": [(0, 0), (1, 1), (2, 2), (3, 3), (4, 4)]}


def leg_joint_links(kind):
    """links with a leg joint, in link order"""
    return list(range(6, 14)) if kind == "oct" else [6 + 4 * k + j for k in range(4) for j in range(3)]


def hip_links(kind):
    return [6 + 2 * k for k in range(4)] if kind == "oct" else [6 + 4 * k for k in range(4)]


def last_joint_links(kind):
    return [7 + 2 * k for k in range(4)] if kind == "oct" else [8 + 4 * k for k in range(4)]


def toe_links():
    return [9 + 4 * k for k in range(4)]


def _rot(axis, a):
    axis = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K


def _get3x3(a):
    return np.array([a[k] for k in range(9)]).reshape(3, 3)


def _set(arr, values):
    for k, v in enumerate(np.asarray(values, dtype=np.float64).reshape(-1)):
        arr[k] = float(v)


def _body(l, rng, full_inertia):
    """mass, centre of mass and inertia of a link: scaled, shifted, and a random positive-definite term of the size of
    the link's own inertia added"""
    l.mass = l.mass * rng.uniform(0.7, 1.4)
    _set(l.com, np.array([l.com[k] for k in range(3)]) + rng.uniform(-0.05, 0.05, 3))
    I0 = _get3x3(l.inertia)
    A = rng.uniform(-1, 1, (3, 3))
    extra = A @ A.T if full_inertia else np.diag(rng.uniform(0.1, 1.0, 3))
    _set(l.inertia, I0 + extra * 0.3 * np.trace(I0) / 3.0)


def _frame(l, rng, xt_rot):
    if xt_rot == "random":   # never the identity: at least 0.2 rad
        R = _rot(rng.uniform(-1, 1, 3), rng.choice([-1.0, 1.0]) * rng.uniform(0.2, 0.8)) @ _get3x3(l.X_T_rot)
        _set(l.X_T_rot, R)
    elif xt_rot == "identity":
        _set(l.X_T_rot, np.eye(3))
    _set(l.X_T_trans, np.array([l.X_T_trans[k] for k in range(3)]) + rng.uniform(-0.05, 0.05, 3))


def synthetic_star(kind, seed, joints="cycle", joint_offset=0, xt_rot="random", springs=True, full_inertia=True,
                   root_com=True, tilt=0.1, plane_constant=0.0, restitution=0.0, pgs_iterations=1, reward_mode=None,
                   visuals=True, pd_start_link=6, plain=False):
    """A star of `kind` ("oct": the Ant's structure, "quad": Laikago's), a new model every call.
    joints: "cycle" (the eight 1-dof kinds along the leg joints, starting at joint_offset), "revolute", "prismatic"
    (cycles of the four kinds of each) or "keep"; xt_rot: "random" (a rotation of 0.2 .. 0.8 rad on every leg link's X_T),
    "identity" or "keep"; springs: stiffness and damping on the leg joints; full_inertia: off-diagonal inertia terms;
    root_com: a centre of mass of link 5 away from its origin; tilt: the plane normal's angle to e_z; visuals: 9 / 17
    visuals with random frames, or none; pd_start_link (quad): the first link of the PD loop; plain: the model as loaded."""
    assert kind in KINDS
    m = tds_amd.load_model(BASE[kind]).copy()
    if plain:
        return m
    rng = np.random.default_rng(seed)
    legs = leg_joint_links(kind)
    pools = {"cycle": JOINT_KINDS, "revolute": REVOLUTE, "prismatic": PRISMATIC}
    for n, i in enumerate(legs):
        l = m.links[i]
        if joints != "keep":
            jt = pools[joints][(n + joint_offset) % len(pools[joints])]
            l.joint_type = jt
            S = np.zeros(6)
            if jt in (J.JOINT_REVOLUTE_X, J.JOINT_REVOLUTE_Y, J.JOINT_REVOLUTE_Z):
                S[jt - J.JOINT_REVOLUTE_X] = 1.0
            elif jt == J.JOINT_REVOLUTE_AXIS:
                S[:3] = rng.uniform(0.3, 1, 3) * rng.choice([-1.0, 1.0], 3) * 1.7   # (not normalised)
            elif jt in (J.JOINT_PRISMATIC_X, J.JOINT_PRISMATIC_Y, J.JOINT_PRISMATIC_Z):
                S[3 + jt - J.JOINT_PRISMATIC_X] = 1.0
            else:
                S[3:] = rng.uniform(0.3, 1, 3) * rng.choice([-1.0, 1.0], 3)          # (not normalised)
            _set(l.S, S)
        _frame(l, rng, xt_rot)
        _body(l, rng, full_inertia)
        l.stiffness = rng.uniform(0.2, 2.0) if springs else 0.0
        l.damping = rng.uniform(0.05, 0.5) if springs else 0.0
    if kind == "quad":
        for i in toe_links():
            _frame(m.links[i], rng, xt_rot)
            _body(m.links[i], rng, full_inertia)
    root = m.links[5]
    keep = [root.com[k] for k in range(3)]
    _body(root, rng, full_inertia)
    if not root_com:
        _set(root.com, keep)
    # shapes
    for g in range(m.num_geoms):
        G = m.geoms[g]
        if G.type == J.GEOM_CAPSULE:
            G.radius = rng.uniform(0.05, 0.11)
            G.length = G.length * rng.uniform(0.7, 1.3)
            _set(G.X_rot, _rot(rng.uniform(-1, 1, 3), rng.uniform(-0.5, 0.5)) @ _get3x3(G.X_rot))
            _set(G.X_trans, np.array([G.X_trans[k] for k in range(3)]) + rng.uniform(-0.03, 0.03, 3))
        elif kind == "oct":   # the root sphere
            G.radius = rng.uniform(0.18, 0.3)
            _set(G.X_trans, rng.uniform(-0.05, 0.05, 3))
        else:                 # a toe sphere
            G.radius = rng.uniform(0.02, 0.05)
            _set(G.X_trans, rng.uniform(-0.02, 0.02, 3))
    # the world
    t, p = rng.uniform(0.03, 1.0) * tilt, rng.uniform(-np.pi, np.pi)
    _set(m.plane_normal, [np.sin(t) * np.cos(p), np.sin(t) * np.sin(p), np.cos(t)] if tilt else [0.0, 0.0, 1.0])
    m.plane_constant = plane_constant
    m.cfm = float(10.0 ** rng.uniform(-5, -3))
    m.erp = rng.uniform(0.05, 0.3)
    m.friction = rng.uniform(0.3, 1.0)
    m.restitution = restitution
    m.pgs_iterations = pgs_iterations
    m.action_limit = rng.uniform(0.2, 0.6)
    if reward_mode is not None:
        m.reward_mode = reward_mode
    nqd = m.dof_q + m.dof_qd
    if visuals:
        for v in range(m.num_visuals):
            V = m.visuals[v]
            _set(V.X_rot, _rot(rng.uniform(-1, 1, 3), rng.uniform(-3, 3)))   # (large angles: every branch of matrix_to_quat)
            _set(V.X_trans, rng.uniform(-0.2, 0.2, 3))
    else:
        m.num_visuals, m.pack_visuals, m.output_dim = 0, 0, nqd
    if pd_start_link != 6:
        assert kind == "quad" and pd_start_link > 6
        m.pd_start_link = pd_start_link
        m.action_dim = sum(1 for i in legs if i >= pd_start_link)
        m.input_dim = nqd + m.action_dim + 3
    for a in range(m.action_dim):
        m.initial_poses[a] = m.initial_poses[a] + rng.uniform(-0.2, 0.2)
    m.name = f"{kind}star{seed}".encode()
    return m


def case(kind, tag, seed=0, z=None, **kw):
    """z: the range of the root's height the star's states are drawn from (None: the kind's own)"""
    return {"kind": kind, "id": f"{kind}-{tag}", "seed": seed, "z": z, "kw": kw}


_R = J.TDS_REWARD_NONE, J.TDS_REWARD_ANT, J.TDS_REWARD_LAIKAGO
CASES = [
    case("oct", "ant", plain=True),
    # every joint kind on the even lanes (hips) and on the odd ones: offsets 0 and 1; X_T rotated on every leg link
    case("oct", "cycle0", 1, joint_offset=0, tilt=0.1, plane_constant=0.03, restitution=0.2, pgs_iterations=2, reward_mode=_R[1]),
    case("oct", "cycle1", 2, joint_offset=1, xt_rot="identity", springs=False, tilt=0.0, pgs_iterations=3, reward_mode=_R[2],
         visuals=False),
    case("oct", "prismatic", 3, joints="prismatic", tilt=0.07, plane_constant=-0.02, pgs_iterations=1, reward_mode=_R[0]),
    case("oct", "revolute", 4, joints="revolute", xt_rot="identity", springs=False, full_inertia=False, root_com=False,
         tilt=0.1, restitution=0.3, pgs_iterations=2, reward_mode=_R[1]),
    case("oct", "cycle3", 5, joint_offset=3, springs=True, tilt=0.0, plane_constant=0.03, restitution=0.1, pgs_iterations=3,
         reward_mode=_R[1], visuals=False),
    case("oct", "keep", 6, joints="keep", xt_rot="random", tilt=0.05, pgs_iterations=1, reward_mode=_R[2]),
    case("oct", "cycle6", 7, joint_offset=6, xt_rot="keep", springs=True, tilt=0.1, restitution=0.2, pgs_iterations=2,
         reward_mode=_R[0]),
    case("quad", "laikago", plain=True),
    case("quad", "cycle0", 11, joint_offset=0, tilt=0.1, plane_constant=0.03, restitution=0.2, pgs_iterations=2, reward_mode=_R[2]),
    case("quad", "cycle1", 12, joint_offset=1, xt_rot="identity", springs=False, tilt=0.0, pgs_iterations=3, reward_mode=_R[1],
         visuals=False),
    case("quad", "prismatic", 13, z=(0.4, 1.0), joints="prismatic", tilt=0.07, plane_constant=-0.02, pgs_iterations=1, reward_mode=_R[0]),
    case("quad", "revolute", 14, z=(0.15, 0.4), joints="revolute", xt_rot="identity", springs=False, full_inertia=False, root_com=False,
         tilt=0.1, restitution=0.3, pgs_iterations=2, reward_mode=_R[2]),
    case("quad", "pd10", 35, z=(0.2, 0.5), joint_offset=4, tilt=0.0, plane_constant=0.03, restitution=0.1, pgs_iterations=3,
         reward_mode=_R[2], visuals=False, pd_start_link=10),
    case("quad", "keep", 16, joints="keep", xt_rot="random", tilt=0.05, pgs_iterations=1, reward_mode=_R[1]),
    case("quad", "cycle5", 17, joint_offset=5, xt_rot="keep", springs=True, tilt=0.1, restitution=0.2, pgs_iterations=2,
         reward_mode=_R[0], pd_start_link=15),
]
# the oracle's largest |y| over a star's 67 states (tests/test_star_kernels_cpu.py asserts each: below 1e3)
MAX_ABS_Y = {
    "oct-ant": 30.08717551, "oct-cycle0": 9.35195772, "oct-cycle1": 8.255946671, "oct-prismatic": 26.06747844,
    "oct-revolute": 25.82351877, "oct-cycle3": 18.28672425, "oct-keep": 12.75631739, "oct-cycle6": 21.65994805,
    "quad-laikago": 276.4232669, "quad-cycle0": 413.6329411, "quad-cycle1": 388.9680799, "quad-prismatic": 206.5786559,
    "quad-revolute": 396.6278068, "quad-pd10": 686.137093, "quad-keep": 261.6703592, "quad-cycle5": 182.7345324,
}


def of_kind(kind, cases=None):
    return [c for c in (CASES if cases is None else cases) if c["kind"] == kind]


def by_id(cid):
    return next(c for c in CASES if c["id"] == cid)


def star(c):
    """the model of a case; a new model every call"""
    return synthetic_star(c["kind"], c["seed"], **c["kw"])


def xt_is_identity(m, i):
    return [m.links[i].X_T_rot[k] for k in range(9)] == [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]


def mixed_cases(kind):
    """the two stars the float-record test runs: X_T rotated on every leg link, and prismatic on all leg joints"""
    legs = leg_joint_links(kind)
    everywhere = next(c for c in of_kind(kind) if not any(xt_is_identity(star(c), i) for i in legs))
    prismatic = next(c for c in of_kind(kind) if all(star(c).links[i].joint_type in PRISMATIC for i in legs))
    assert everywhere["id"] != prismatic["id"]
    return [everywhere, prismatic]


def draw_states(kind, m, n, rng, z=None):
    """oct: tests/test_oct.py's contact states; quad: those of tests/test_quad.py's contact patterns"""
    if kind == "oct":
        lo, hi = z or (0.05, 0.75)
        return _contact_states(m, n, rng, lo=lo, hi=hi)
    nq, nd, adim = m.dof_q, m.dof_qd, m.action_dim
    lo, hi = z or (0.30, 0.50)
    x = np.zeros((n, m.input_dim))
    # the pose of every leg joint: of the PD loop's where it has one, the unmodified model's otherwise
    ip = np.array([tds_amd.load_model(BASE[kind]).initial_poses[i] for i in range(nq - 6)])
    ip[nq - 6 - adim:] = [m.initial_poses[i] for i in range(adim)]
    x[:, 0:2] = rng.uniform(-2, 2, (n, 2))
    x[:, 2] = rng.uniform(lo, hi, n)                  # from well inside the plane to airborne
    x[:, 3:5] = rng.uniform(-0.4, 0.4, (n, 2))        # roll / pitch: some toes down, some up
    x[:, 5] = rng.uniform(-3, 3, n)
    x[:, 6:nq] = ip + rng.uniform(-0.5, 0.5, (n, nq - 6))
    x[:, nq:nq + nd] = rng.uniform(-1.5, 1.5, (n, nd))
    x[:, nq + nd:nq + nd + adim] = rng.uniform(-0.4, 0.4, (n, adim))
    x[:, -3:] = [100, 2, 50]
    return x


def active_contacts(m, x):
    """penetrating contact points of each record [n], by the oracle's narrowphase"""
    return np.array([int((oraclelib.step_debug(m, xe)["contacts"][:, 9] < 0).sum()) for xe in x])


@functools.lru_cache(maxsize=None)
def _states(cid):
    c = by_id(cid)
    m = star(c)
    pool = draw_states(c["kind"], m, POOL, np.random.default_rng(9000 + c["seed"]), c["z"])
    counts = active_contacts(m, pool)
    chosen = []
    for lo, hi in CONTACT_BINS[c["kind"]]:   # the first three states of every bin, then the first of the others
        chosen += [i for i in range(POOL) if lo <= counts[i] <= hi][:3]
    chosen = sorted(set(chosen))
    rest = [i for i in range(POOL) if i not in set(chosen)][:N_STATES - len(chosen)]
    idx = np.array(sorted(chosen + rest))
    x = np.ascontiguousarray(pool[idx])
    x.setflags(write=False)
    cnt = counts[idx]
    cnt.setflags(write=False)
    return x, cnt


def states_of(c):
    """(x [67, input_dim], penetrating contact points [67]) of a star.  Shared by the tests: read-only."""
    return _states(c["id"])


@functools.lru_cache(maxsize=None)
def _oracle_y(cid):
    c = by_id(cid)
    y = oraclelib.step(star(c), states_of(c)[0])
    y.setflags(write=False)
    return y


def oracle_y(c):
    """the oracle's step of the star's 67 states [67, output_dim].  Computed once, shared: read-only."""
    return _oracle_y(c["id"])
