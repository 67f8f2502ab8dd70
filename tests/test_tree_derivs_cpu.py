"""CPU: the second statement of the step (tds_diff_step.h, tds_dyn.h, tds_contact.h in their host instantiations) on the
curated random trees of tests/tree_cases.py, against references that share no code with it: the C oracle's step and
step_debug, central differences of the oracle (step h = 1e-6 max(1, |x_j|), tests/diff_states.py), and forward against
reverse mode.  Also the proof that the generator's new arguments leave the models of tests/test_random_trees.py as they
were (digests recorded from the generator before it had them), and the facts the curated list promises.

A state whose penetrating contact set (the oracle's narrowphase) changes at x +- h e_j for some column j is left out of
the comparisons with central differences; every tree keeps at least 8 of its 16 states and every class three quarters.

Measured maxima over the trees of a class, metric max |a - b| / max(|b|, 1); BOUND is 10 x each:
                                                          S         A         L
  step_host, jacobian_host's y vs oracle step          3.2e-13   6.1e-14   4.0e-13
  jacobian_host vs central differences                 3.7e-07   1.1e-07   1.0e-06
  vjp_host vs w^T jacobian_host (k = 1, 3)             2.0e-12   1.8e-13   1.6e-12
  theta columns vs central differences                 4.5e-07   7.3e-07   6.3e-07
  vjp_params_host vs forward mode                      3.7e-12   8.5e-14   1.5e-12
  dynamics_host vs step_debug (x_world, M, qdd)        7.4e-14   5.4e-14   1.2e-13
  inverse_dynamics_host(qdd_oracle) vs tau - Kq - Dqd  3.7e-14   2.6e-14   4.5e-14
  point_jacobian_host vs central differences           4.7e-10   5.9e-10   6.3e-10
  contacts_host vs step_debug (points, jac, A, b, p)   1.1e-12   3.7e-14   1.9e-12
  qd_post vs step_host                                 7.5e-14   5.0e-16   2.7e-15
  dynamics_jvp_host vs central differences             6.4e-08   3.7e-08   1.8e-07
  inverse_dynamics_jvp_host vs central differences     6.5e-09   2.2e-08   5.3e-08
  contacts_jvp_host vs central differences             2.6e-07   5.6e-07   2.5e-06
  states left out by the contact-set rule              0 / 176   0 / 128   0 / 128
No entry came within a factor of 100 of WRONG_TERM.  The three overflowing trees record 21 442 (seed 105), 22 762 (113)
and 20 268 (116) entries at their longest state against class S's 16 384."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import tds_amd
from tds_amd import hip_backend as hb
import diff_states as ds
import oraclelib  # checker only
import tree_cases as tc
from test_dynamics_cpu import spring_terms
from test_random_trees import random_tree_model

M = tds_amd.model
H_REL = 1e-6   # the central differences' step, as tests/diff_states.py
IDS = [c["id"] for c in tc.ALL]
FIT_IDS = [c["id"] for c in tc.CASES]
BY_ID = {c["id"]: c for c in tc.ALL}

# 10 x the measured maxima of the docstring, per class
BOUND = {
    "step": {"S": 10 * 3.2e-13, "A": 10 * 6.1e-14, "L": 10 * 4.0e-13},
    "jacobian": {"S": 10 * 3.7e-07, "A": 10 * 1.1e-07, "L": 10 * 1.0e-06},
    "vjp": {"S": 10 * 2.0e-12, "A": 10 * 1.8e-13, "L": 10 * 1.6e-12},
    "theta": {"S": 10 * 4.5e-07, "A": 10 * 7.3e-07, "L": 10 * 6.3e-07},
    "vjp_params": {"S": 10 * 3.7e-12, "A": 10 * 8.5e-14, "L": 10 * 1.5e-12},
    "dynamics": {"S": 10 * 7.4e-14, "A": 10 * 5.4e-14, "L": 10 * 1.2e-13},
    "inverse_dynamics": {"S": 10 * 3.7e-14, "A": 10 * 2.6e-14, "L": 10 * 4.5e-14},
    "point_jacobian": {"S": 10 * 4.7e-10, "A": 10 * 5.9e-10, "L": 10 * 6.3e-10},
    "contacts": {"S": 10 * 1.1e-12, "A": 10 * 3.7e-14, "L": 10 * 1.9e-12},
    "qd_post": {"S": 10 * 7.5e-14, "A": 10 * 5.0e-16, "L": 10 * 2.7e-15},
    "dynamics_jvp": {"S": 10 * 6.4e-08, "A": 10 * 3.7e-08, "L": 10 * 1.8e-07},
    "inverse_dynamics_jvp": {"S": 10 * 6.5e-09, "A": 10 * 2.2e-08, "L": 10 * 5.3e-08},
    "contacts_jvp": {"S": 10 * 2.6e-07, "A": 10 * 5.6e-07, "L": 10 * 2.5e-06},
}
WRONG_TERM = 1e-3   # an entry further than this from its central difference is a wrong term, not truncation


def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1.0))) if a.size else 0.0


def check(what, cls, err, extra=""):
    """print the figure, then hold it against its bound"""
    bound = BOUND[what][cls]
    print(f"{what} [{cls}]: {err:.3e} (bound {bound:.1e}){extra}")
    assert err <= bound, (what, cls, err, bound)


def load(cid):
    c = BY_ID[cid]
    m, n_virtual, style = tc.tree(c)
    x, counts = tc.states_of(c)
    return c, m, x, counts


def penetrating(m, xe):
    return tuple(oraclelib.step_debug(m, xe)["contacts"][:, 9] < 0) if m.num_geoms else ()


_KEPT = {}


def kept(cid):
    """[16] bool: the penetrating set of the state is the same at x +- h e_j for every column j"""
    if cid not in _KEPT:
        _, m, x, _ = load(cid)
        ok = np.ones(x.shape[0], dtype=bool)
        for e in range(x.shape[0] if m.num_geoms else 0):
            base = penetrating(m, x[e])
            for j in range(m.input_dim):
                h = H_REL * max(1.0, abs(x[e, j]))
                for s in (h, -h):
                    xe = x[e].copy()
                    xe[j] += s
                    ok[e] &= penetrating(m, xe) == base
        _KEPT[cid] = ok
    return _KEPT[cid]


def split(m, x):
    nq, nd = m.dof_q, m.dof_qd
    return x[:, :nq].copy(), x[:, nq:nq + nd].copy(), x[:, nq + nd:nq + nd + hb.dyn_tau_dim(m)].copy()


def every_param(m):
    return hb.all_params(m) + hb.contact_params(m)


# ---------------------------------------------------------------- the generator and the list
def test_default_arguments_draw_the_models_the_random_tree_tests_have_always_seen(built):
    """every seed tests/test_random_trees.py uses, against digests of the model blobs recorded from the generator as it
    was before it had the arguments links, p_fixed, contact_points and shapes"""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "random_tree_digests.json")) as f:
        want = json.load(f)
    seeds = {"plain": (range(0, 40), {}), "floating": (range(500, 530), {"floating": True}),
             "spherical": ([*range(900, 930), *range(1700, 1730)], {"spherical": True})}
    for key, (rng, kw) in seeds.items():
        assert sorted(want[key], key=int) == [str(s) for s in rng]
        for s in rng:
            m, n_virtual, style = random_tree_model(s, **kw)
            assert [hashlib.sha256(bytes(m)).hexdigest(), int(n_virtual), int(style)] == want[key][str(s)], (key, s)
    # and the arguments act
    m, _, _ = random_tree_model(3, links=(15, 22), p_fixed=0.5, contact_points=4, shapes=("sphere", "capsule"))
    assert 15 <= m.num_links <= 22 and tc.contact_points(m) <= 4
    assert all(m.geoms[g].type != M.GEOM_BOX for g in range(m.num_geoms))
    assert sum(m.links[i].joint_type == M.JOINT_FIXED for i in range(m.num_links)) >= 4


def test_curated_list_holds_what_it_promises(built):
    assert len(IDS) == len(set(IDS)) == 27
    assert [(c["seed"], c["kw"]) for c in tc.OVERFLOW] == [(105, {}), (113, {}), (116, {})]
    no_contact = {cls: 0 for cls in tc.CLASSES}
    for cls in tc.CLASSES:
        cases = tc.of_class(cls)
        assert len(cases) == 8
        nl_max, nd_max, nc_max, _ = tc.class_bounds()[cls]
        joints, kinds, styles, bases, pgs, chains, nls, nds = set(), set(), set(), set(), set(), set(), set(), set()
        for c in cases + ([c for c in tc.OVERFLOW if c["cls"] == cls]):
            m, n_virtual, style = tc.tree(c)
            x, counts = tc.states_of(c)
            assert x.shape == (tc.N_STATES, m.input_dim) and len({xe.tobytes() for xe in x}) == tc.N_STATES
            # the class: tds_jvp_pick restated over the bounds read from csrc/tds_diff_classes.h, and what the library
            # shows of its pick (K = 4 in S, 2 in A and L, which share every figure the C ABI reports)
            assert tc.model_class(m) == cls == c["cls"], c["id"]
            assert hb.jacobian_tangents(m) == (4 if cls == "S" else 2)
            assert m.num_links <= nl_max and m.dof_qd <= nd_max and tc.contact_points(m) <= nc_max
            # positive definite at every state, by the oracle's Cholesky and by the host's
            y = oraclelib.step(m, x)
            assert np.isfinite(y).all()
            Mq = hb.dynamics_host(m, x[:, :m.dof_q], want=("mass_matrix",))["mass_matrix"]
            assert all(np.linalg.eigvalsh(Mq[e]).min() > 0 for e in range(tc.N_STATES))
            # contacts: the host's narrowphase counts what the oracle's does; shapes touch the plane somewhere
            if tc.contact_points(m):
                host = (hb.contacts_host(m, x, want=("contacts",))["contacts"][:, :, 9] < 0).sum(axis=1)
                np.testing.assert_array_equal(host, counts)
                assert counts.max() > 0, c["id"]
            else:
                assert counts.max() == 0
            no_contact[cls] += int((counts == 0).sum())
            # the tape
            w = np.zeros((tc.N_STATES, m.output_dim))
            if c["tape_fits"]:
                _, lens = hb.vjp_host(m, x, w, tape_len=True)
                assert np.all(lens > 0)
                sel = every_param(m)
                _, lens_p = hb.vjp_params_host(m, x, hb.params_get(m, sel), sel, w, tape_len=True)
                assert np.all(lens_p > lens)
            else:
                with pytest.raises(hb.TdsHipError, match="error 2: .*tape exceeds the capacity"):
                    hb.vjp_host(m, x, w, tape_len=True)
                _, lens = hb.vjp_host(m, x, w, tape_len=True, tape_cap=1 << 18)
                print(f"{c['id']}: {m.num_links} links, {m.dof_qd} dofs, {tc.contact_points(m)} contact points, "
                      f"pgs_iterations {m.pgs_iterations}: longest tape {lens.max()}")
                continue   # (the overflowing trees are extra: the coverage below is the eight's)
            joints |= {int(m.links[i].joint_type) for i in range(m.num_links)}
            kinds |= {int(m.geoms[g].type) for g in range(m.num_geoms)}
            styles.add(int(style))
            bases.add(bool(m.is_floating))
            pgs.add(int(m.pgs_iterations))
            if not m.is_floating:
                chains.add(int(n_virtual))
            nls.add(m.num_links)
            nds.add(m.dof_qd)
        assert joints == set(range(-1, 8)), (cls, joints)
        assert kinds == ({M.GEOM_SPHERE, M.GEOM_CAPSULE} | ({M.GEOM_BOX} if nc_max >= 8 else set())), (cls, kinds)
        assert styles == {0, 1, 2} and bases == {False, True} and pgs == {1, 2}, (cls, styles, bases, pgs)
        assert len(chains) >= 3, (cls, chains)
        assert nl_max in nls and nd_max in nds, (cls, nls, nds)
        assert no_contact[cls] > 0


@pytest.mark.parametrize("cls", tc.CLASSES)
def test_contact_set_rule_keeps_enough_states(cls, built):
    cases = [c for c in tc.ALL if c["cls"] == cls]
    k = np.stack([kept(c["id"]) for c in cases])
    print(f"class {cls}: the contact-set rule leaves out {(~k).sum()} of {k.size} states")
    assert k.mean() >= 0.75 and k.sum(axis=1).min() >= 8


# ---------------------------------------------------------------- step and Jacobian
@pytest.mark.parametrize("cid", IDS)
def test_step_and_jacobian_match_the_oracle(cid, built):
    """the overflowing trees too: forward mode knows no tape"""
    c, m, x, counts = load(cid)
    y_ref = oraclelib.step(m, x)
    jac, yj = hb.jacobian_host(m, x, want_y=True)
    check("step", c["cls"], max(rel(hb.step_host(m, x), y_ref), rel(yj, y_ref)))
    ok = kept(cid)
    J_fd, _ = ds.central_jacobian(m, x[ok], h_rel=H_REL)
    err = rel(jac[ok], J_fd)
    assert err <= WRONG_TERM, "a wrong term"
    check("jacobian", c["cls"], err, f" over {ok.sum()} states with {sorted(set(counts[ok].tolist()))} active contacts")


# ---------------------------------------------------------------- reverse mode
@pytest.mark.parametrize("cid", FIT_IDS)
def test_vjp_is_w_times_the_jacobian(cid, built):
    c, m, x, _ = load(cid)
    jac, yj = hb.jacobian_host(m, x, want_y=True)
    rng = np.random.default_rng(c["seed"])
    err = 0.0
    for k in (1, 3):
        w = rng.normal(size=(x.shape[0], k, m.output_dim))
        wj, y = hb.vjp_host(m, x, w, want_y=True)
        err = max(err, rel(wj, np.einsum("nko,noi->nki", w, jac)), rel(y, yj))
    check("vjp", c["cls"], err)


@pytest.mark.parametrize("cid", [c["id"] for c in tc.OVERFLOW])
def test_overflowing_trees_raise_the_capacity_error(cid, built):
    """TDS_ERR_UNSUPPORTED with NaN rows for the environments that overflowed, in plain and in parameter mode"""
    c, m, x, _ = load(cid)
    w = np.ones((x.shape[0], m.output_dim))
    with pytest.raises(hb.TdsHipError, match="error 2: .*tape exceeds the capacity"):
        hb.vjp_host(m, x, w)
    sel = every_param(m)
    with pytest.raises(hb.TdsHipError, match="error 2: .*tape exceeds the capacity"):
        hb.vjp_params_host(m, x, hb.params_get(m, sel), sel, w)
    _, lens = hb.vjp_host(m, x, w, tape_len=True, tape_cap=1 << 18)
    wj, y, got = np.zeros((x.shape[0], m.input_dim)), np.zeros((x.shape[0], m.output_dim)), np.zeros(x.shape[0], np.int32)
    rc = hb.lib().tds_hip_vjp_host_tape(C.byref(m), x.shape[0], x.ctypes.data, 1, w.ctypes.data, y.ctypes.data,
                                        wj.ctypes.data, 0, got.ctypes.data)
    assert rc == 2
    over = got < 0
    assert over.any() and np.array_equal(got[~over], lens[~over])
    assert np.all(np.isnan(wj[over])) and np.all(np.isnan(y[over]))
    jac = hb.jacobian_host(m, x)
    assert rel(wj[~over], np.einsum("no,noi->ni", w, jac)[~over]) <= BOUND["vjp"]["S"]


# ---------------------------------------------------------------- parameters
def theta_central(m, x, sel, theta):
    """central differences of the oracle's step over the selected scalars on params_apply'd models, h = 1e-6
    max(1, |theta_j|) (tests/test_param_derivs_cpu.py; cfm apart), and per (state, scalar) whether the penetrating set
    held"""
    J = np.zeros((x.shape[0], m.output_dim, len(sel)))
    same = np.ones((x.shape[0], len(sel)), dtype=bool)
    base = [penetrating(m, xe) for xe in x]
    for j in range(len(sel)):
        # (cfm is 1e-5 and y' in it reaches 1e5: a step of 1e-6 is a tenth of it, so it takes 1e-3 of its own size)
        h = 1e-3 * theta[j] if sel[j] == ("cfm",) else H_REL * max(1.0, abs(theta[j]))
        ys = []
        for s in (h, -h):
            t = theta.copy()
            t[j] += s
            mm = hb.params_apply(m, sel, t)
            ys.append(oraclelib.step(mm, x))
            if sel[j][0].startswith("geom_"):   # (the other scalars do not move a contact point)
                same[:, j] &= [penetrating(mm, xe) == b for xe, b in zip(x, base)]
        J[:, :, j] = (ys[0] - ys[1]) / (2 * h)
    return J, same


@pytest.mark.parametrize("cid", FIT_IDS)
def test_parameter_derivatives(cid, built):
    """every selectable parameter, the contact model's included, at the first six states (the fewest and the most
    active contacts are the first two)"""
    c, m, x, _ = load(cid)
    x = x[:6]
    sel = every_param(m)
    theta = hb.params_get(m, sel)
    n, nin, p = x.shape[0], m.input_dim, len(sel)
    v = np.zeros((n, p, nin + p))
    v[:, np.arange(p), nin + np.arange(p)] = 1.0
    Jt = hb.jvp_params_host(m, x, theta, sel, v).transpose(0, 2, 1)
    J_fd, same = theta_central(m, x, sel, theta)
    ok = same & kept(cid)[:6, None]
    assert ok.any(axis=0).all() or not m.num_geoms
    err = max((rel(Jt[e][:, ok[e]], J_fd[e][:, ok[e]]) for e in range(n)), default=0.0)
    assert err <= WRONG_TERM, "a wrong term"
    check("theta", c["cls"], err, f" over {p} parameters, {ok.sum()} of {ok.size} (state, parameter) pairs")
    assert np.count_nonzero(Jt) > 0
    rng = np.random.default_rng(c["seed"])
    w = rng.normal(size=(n, 2, m.output_dim))
    jac = hb.jacobian_host(m, x)
    wj = hb.vjp_params_host(m, x, theta, sel, w)
    check("vjp_params", c["cls"], rel(wj, np.einsum("nko,noi->nki", w, np.concatenate([jac, Jt], axis=2))))


# ---------------------------------------------------------------- dynamics queries
@pytest.mark.parametrize("cid", IDS)
def test_dynamics_queries_match_step_debug(cid, built):
    c, m, x, _ = load(cid)
    q, qd, tau = split(m, x)
    d = hb.dynamics_host(m, q, qd, tau, want=("x_world", "mass_matrix", "qdd"))
    dbg = [oraclelib.step_debug(m, xe) for xe in x]
    err = max(rel(d["x_world"], np.stack([g["X_world"] for g in dbg])), rel(d["qdd"], np.stack([g["qdd"] for g in dbg])))
    if tc.contact_points(m):   # (the oracle forms M for its contact solve only)
        err = max(err, rel(d["mass_matrix"], np.stack([g["M"] for g in dbg])))
    check("dynamics", c["cls"], err)
    if m.is_floating:
        with pytest.raises(hb.TdsHipError, match="error 2: .*no floating-base inverse dynamics"):
            hb.dynamics_host(m, q, qd, tau, want=("bias",))
    else:
        got = hb.inverse_dynamics_host(m, q, qd, np.stack([g["qdd"] for g in dbg]))
        check("inverse_dynamics", c["cls"], rel(got, tau - spring_terms(m, q, qd)))
    # point Jacobians of a local point on every link against central differences of x_world
    # (a revolute joint about a free axis turns about the normalised axis by q and moves with S qd, S as given: SURVEY
    # quirk 7; the generator's axes are not unit vectors, so that joint's column is |S| times the derivative in q)
    rng = np.random.default_rng(c["seed"])
    speed = np.ones(m.dof_qd)
    for i in range(m.num_links):
        if m.links[i].joint_type == M.JOINT_REVOLUTE_AXIS:
            speed[m.links[i].qd_index] = np.linalg.norm(m.links[i].S[:3])
    err = 0.0
    for link in range(m.num_links):
        pl = rng.normal(0, 0.2, 3)
        J = hb.point_jacobian_host(m, q, link, np.broadcast_to(pl, (q.shape[0], 3)).copy(), local=True)
        J_fd = np.zeros_like(J)
        for j in range(m.dof_qd):
            # (a fixed base: q and qd share their indices; a floating base's six come by its own velocity, left to
            # tests/test_dynamics_cpu.py)
            if m.is_floating and j < 6:
                J_fd[:, :, j] = J[:, :, j]
                continue
            jq = j + (1 if m.is_floating else 0)
            pts = []
            for s in (H_REL, -H_REL):
                qq = q.copy()
                qq[:, jq] += s
                X = hb.dynamics_host(m, qq, want=("x_world",))["x_world"][:, link]
                pts.append(X[:, :9].reshape(-1, 3, 3) @ pl + X[:, 9:])
            J_fd[:, :, j] = (pts[0] - pts[1]) / (2 * H_REL) * speed[j]
        err = max(err, rel(J, J_fd))
    assert err <= WRONG_TERM, "a wrong term"
    check("point_jacobian", c["cls"], err)


# ---------------------------------------------------------------- contact query
@pytest.mark.parametrize("cid", IDS)
def test_contact_query_matches_step_debug(cid, built):
    """oracle -> query: contacts -> contacts, jac -> jac, lcp_A -> delassus, lcp_b -> rhs, lcp_p -> impulse"""
    c, m, x, counts = load(cid)
    d = hb.contacts_host(m, x)
    check("qd_post", c["cls"], rel(d["qd_post"], hb.step_host(m, x)[:, m.dof_q:m.dof_q + m.dof_qd]))
    nc = tc.contact_points(m)
    assert d["contacts"].shape == (x.shape[0], nc, 10)
    if not nc:
        return
    err = 0.0
    for e in range(x.shape[0]):
        g = oraclelib.step_debug(m, x[e])
        assert g["contacts"].shape == (nc, 10)
        err = max(err, rel(d["contacts"][e], g["contacts"]), rel(d["jac"][e], g["jac"]),
                  rel(d["delassus"][e], g["lcp_A"]), rel(d["rhs"][e], g["lcp_b"]), rel(d["impulse"][e], g["lcp_p"]))
    check("contacts", c["cls"], err, f" at {sorted(set(counts.tolist()))} active contacts")
    assert np.abs(d["impulse"]).max() > 0


# ---------------------------------------------------------------- query derivatives
def query_selection(m, contact):
    heavy = max(range(m.num_links), key=lambda i: m.links[i].mass)
    sel = [("mass", heavy), ("com", heavy, 1), ("inertia", heavy, 3), ("xt_trans", m.num_links - 1, 0), ("gravity", 2)]
    if m.is_floating:
        sel += [("base_mass",), ("base_com", 0)]
    if contact:
        sel += [("friction",), ("restitution",), ("erp",), ("cfm",)]
        sel += [q for q in hb.contact_params(m) if q[0].startswith("geom_")][:5]
    return sel


def theta_scale(theta):
    """a direction's theta part moves every scalar by its own size (cfm is 1e-5: a step of h would change it by a tenth,
    and the solve of a nearly singular A is far from linear over that)"""
    return np.where(theta != 0, np.abs(theta), 1.0)


@pytest.mark.parametrize("cid", IDS)
def test_query_derivatives_match_central_differences(cid, built):
    """three directions in [z | theta]: the tangents against (f(z + h v) - f(z - h v)) / 2h of the primal host query on
    params_apply'd models; states whose penetrating set differs at either end are left out of the contact query's"""
    c, m, x, _ = load(cid)
    n = x.shape[0]
    rng = np.random.default_rng(c["seed"] + 1)
    h = H_REL
    # dynamics
    q, qd, tau = split(m, x)
    sel = query_selection(m, False)
    theta = hb.params_get(m, sel)
    want = ("x_world", "mass_matrix", "qdd") if m.is_floating else hb.DYN_OUTPUTS
    nq, nd, nt, p = m.dof_q, m.dof_qd, hb.dyn_tau_dim(m), len(sel)
    v = rng.normal(size=(n, 3, nq + nd + nt + p))
    v[:, :, nq + nd + nt:] *= theta_scale(theta)
    tan = hb.dynamics_jvp_host(m, q, qd, tau, v, want=want, params=sel, theta=theta)
    err = 0.0
    for k in range(3):
        ends = []
        for s in (h, -h):
            per_state = []
            for e in range(n):   # (theta moves along its own direction in every state: a model per state)
                mm = hb.params_apply(m, sel, theta + s * v[e, k, nq + nd + nt:])
                z = v[e, k]
                per_state.append(hb.dynamics_host(mm, q[e:e + 1] + s * z[:nq], qd[e:e + 1] + s * z[nq:nq + nd],
                                                  tau[e:e + 1] + s * z[nq + nd:nq + nd + nt], want=want))
            ends.append({name: np.concatenate([d[name] for d in per_state]) for name in want})
        for name in want:
            err = max(err, rel(tan[name][:, k], (ends[0][name] - ends[1][name]) / (2 * h)))
    assert err <= WRONG_TERM, "a wrong term"
    check("dynamics_jvp", c["cls"], err)
    if not m.is_floating:
        qdd = rng.normal(size=(n, nd))
        vi = rng.normal(size=(n, 3, nq + 2 * nd + p))
        vi[:, :, nq + 2 * nd:] *= theta_scale(theta)
        dtau = hb.inverse_dynamics_jvp_host(m, q, qd, qdd, vi, params=sel, theta=theta)
        err = 0.0
        for k in range(3):
            ends = []
            for s in (h, -h):
                ends.append(np.concatenate([hb.inverse_dynamics_host(
                    hb.params_apply(m, sel, theta + s * vi[e, k, nq + 2 * nd:]), q[e:e + 1] + s * vi[e, k, :nq],
                    qd[e:e + 1] + s * vi[e, k, nq:nq + nd], qdd[e:e + 1] + s * vi[e, k, nq + nd:nq + 2 * nd])
                    for e in range(n)]))
            err = max(err, rel(dtau[:, k], (ends[0] - ends[1]) / (2 * h)))
        assert err <= WRONG_TERM, "a wrong term"
        check("inverse_dynamics_jvp", c["cls"], err)
    # contacts
    sel = query_selection(m, True)
    theta = hb.params_get(m, sel)
    nin, p = m.input_dim, len(sel)
    v = rng.normal(size=(n, 3, nin + p))
    v[:, :, nin:] *= theta_scale(theta)
    tan = hb.contacts_jvp_host(m, x, v, params=sel, theta=theta)
    ok = kept(cid).copy()
    err, used = 0.0, 0
    for k in range(3):
        ends, same = [], ok.copy()
        for s in (h, -h):
            per_state = []
            for e in range(n):
                mm = hb.params_apply(m, sel, theta + s * v[e, k, nin:])
                xe = x[e] + s * v[e, k, :nin]
                same[e] &= penetrating(mm, xe) == penetrating(m, x[e])
                per_state.append(hb.contacts_host(mm, xe[None]))
            ends.append({name: np.concatenate([d[name] for d in per_state]) for name in hb.CONTACT_OUTPUTS})
        assert same.sum() >= 8
        used += int(same.sum())
        for name in hb.CONTACT_OUTPUTS:
            err = max(err, rel(tan[name][same, k], ((ends[0][name] - ends[1][name]) / (2 * h))[same]))
    assert err <= WRONG_TERM, "a wrong term"
    check("contacts_jvp", c["cls"], err, f" over {used} of {3 * n} (state, direction) pairs")
