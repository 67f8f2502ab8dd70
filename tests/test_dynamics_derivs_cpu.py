"""Forward-mode derivatives of the batched dynamics queries on the CPU (tds_hip_dynamics_jvp_host /
tds_hip_inverse_dynamics_jvp_host: the host instantiation of csrc/tds_dyn.h over duals and a parameter overlay): against
central differences of the host queries, against the reference where it is built, and against identities of rigid-body
dynamics everywhere.  z = [q | qd | tau | theta] for the dynamics call, [q | qd | qdd | theta] for inverse dynamics."""
import functools

import numpy as np
import pytest

import tds_amd
from tds_amd import hip_backend as hb

from test_dynamics_cpu import FIXED, rel, split, spring_terms, states, wanted
from test_jacobian_cpu import REFUSED, SUPPORTED, make_ref, needs_ref

H_REL, FD_BOUND = 1e-6, 1e-5  # test_jacobian_cpu.central_diff's step and the bound of its tests
# what test_tangents_match_central_differences_of_the_host_query measures per model (its worst output, relative to
# max(1, max |J|) of a state): the differences' own error, which the autograd checks on the GPU take their atol from
MEASURED_FD = {"ant": 5.3e-9, "ant_floating": 3.7e-9, "laikago": 4.0e-9, "laikago_floating": 5.2e-10,
               "laikago_floating_env": 4.4e-10, "laikago_soft": 3.4e-9, "cartpole": 1.2e-9, "cartpole_plane": 1.2e-9,
               "pendulum5": 2.2e-8, "pendulum5_plane": 4.7e-8, "cube_floating": 5.5e-10}
CONTACT_KINDS =[("friction",), ("restitution",), ("cfm",), ("erp",)]


@functools.lru_cache(maxsize=None)
def inputs(name):
    """the model, q, qd of test_dynamics_cpu.states and seeded tau, qdd ~ N(0, 1)"""
    m, x = states(name)
    q, qd, _ = split(m, x)
    rng = np.random.default_rng(7)
    tau = rng.normal(0, 1.0, (x.shape[0], hb.dyn_tau_dim(m)))
    qdd = rng.normal(0, 1.0, (x.shape[0], m.dof_qd))
    return m, q, qd, tau, qdd


def selection(m, name):
    """masses, a COM component, an inertia component (off-diagonal: two entries of the blob), gravity z, the base's where
    there is one, and on the pendulum a spring stiffness and damping"""
    sel = []
    if m.num_links:
        last = m.num_links - 1
        sel += [("mass", 0), ("com", last, 2), ("inertia", 0, 3), ("inertia", last, 1)]
        if last:
            sel += [("mass", last)]
    if m.is_floating:
        sel += [("base_mass",), ("base_com", 0), ("base_inertia", 4)]
    sel += [("gravity", 2)]
    if name.startswith("pendulum5"):
        sel += [("stiffness", 1), ("damping", 2)]
    return sel


def thetas(m, sel, n, seed=3):
    """per-environment values near the model's (entries that are zero in the model move off zero)"""
    rng = np.random.default_rng(seed)
    base = hb.params_get(m, sel)
    return base * (1 + 0.1 * rng.uniform(-1, 1, (n, len(sel)))) + 1e-3 * np.abs(rng.normal(size=(n, len(sel))))


def flat(d, names):
    return np.concatenate([d[k].reshape(d[k].shape[0], -1) for k in names], axis=1)


def eye_dirs(n, width):
    return np.ascontiguousarray(np.broadcast_to(np.eye(width), (n, width, width)))


def query(m, z, sel, names, inverse):
    """the host query at one z = [q | qd | u | theta] (theta through params_apply), outputs flattened"""
    nq, nd = m.dof_q, m.dof_qd
    nu = nd if inverse else hb.dyn_tau_dim(m)
    q, qd, u, th = np.split(z, [nq, nq + nd, nq + nd + nu])
    mm = hb.params_apply(m, sel, th) if sel else m
    if inverse:
        return hb.inverse_dynamics_host(mm, q[None], qd[None], u[None])[0]
    return flat(hb.dynamics_host(mm, q[None], qd[None], u[None], want=names), names)[0]


def central(m, z, sel, names, inverse):
    y0 = query(m, z, sel, names, inverse)
    J = np.zeros((y0.shape[0], z.shape[0]))
    for j in range(z.shape[0]):
        h = H_REL * max(1.0, abs(z[j]))
        zp, zm = z.copy(), z.copy()
        zp[j] += h
        zm[j] -= h
        J[:, j] = (query(m, zp, sel, names, inverse) - query(m, zm, sel, names, inverse)) / (2 * h)
    return J


# ---------------------------------------------------------------- primal
@pytest.mark.parametrize("name", SUPPORTED)
def test_primal_without_theta_is_the_query_bit_for_bit(name, built):
    m, q, qd, tau, qdd = inputs(name)
    names = wanted(m)
    ref = hb.dynamics_host(m, q, qd, tau, want=names)
    k0 = hb.dynamics_jvp_host(m, q, qd, tau, None, want=names)
    v = np.random.default_rng(0).normal(size=(q.shape[0], 3, hb.dyn_input_dim(m)))
    _, prim = hb.dynamics_jvp_host(m, q, qd, tau, v, want=names, want_primal=True)
    for k in names:
        np.testing.assert_array_equal(k0[k], ref[k], err_msg=k)
        np.testing.assert_array_equal(prim[k], ref[k], err_msg=k)
    if not m.is_floating:
        t = hb.inverse_dynamics_host(m, q, qd, qdd)
        np.testing.assert_array_equal(hb.inverse_dynamics_jvp_host(m, q, qd, qdd), t)
        vi = np.random.default_rng(0).normal(size=(q.shape[0], 2, hb.dyn_input_dim(m, True)))
        np.testing.assert_array_equal(hb.inverse_dynamics_jvp_host(m, q, qd, qdd, vi, want_primal=True)[1], t)
    # NULL qd / tau / qdd: zeros in value
    z = hb.dynamics_jvp_host(m, q, None, None, None, want=names)
    zr = hb.dynamics_host(m, q, None, None, want=names)
    for k in names:
        np.testing.assert_array_equal(z[k], zr[k], err_msg=k)


@pytest.mark.parametrize("name", SUPPORTED)
def test_primal_at_theta_is_the_query_on_the_applied_model(name, built):
    m, q, qd, tau, qdd = inputs(name)
    names, sel = wanted(m), selection(m, name)
    th = thetas(m, sel, q.shape[0])
    got = hb.dynamics_jvp_host(m, q, qd, tau, None, want=names, params=sel, theta=th)
    v = np.random.default_rng(0).normal(size=(q.shape[0], 2, hb.dyn_input_dim(m) + len(sel)))
    _, prim = hb.dynamics_jvp_host(m, q, qd, tau, v, want=names, params=sel, theta=th, want_primal=True)
    worst = 0.0
    for e in range(q.shape[0]):
        me = hb.params_apply(m, sel, th[e])
        ref = hb.dynamics_host(me, q[e:e + 1], qd[e:e + 1], tau[e:e + 1], want=names)
        worst = max([worst] + [rel(got[k][e], ref[k][0]) for k in names] + [rel(prim[k][e], ref[k][0]) for k in names])
        if not m.is_floating:
            t = hb.inverse_dynamics_jvp_host(m, q[e:e + 1], qd[e:e + 1], qdd[e:e + 1], params=sel, theta=th[e])
            worst = max(worst, rel(t, hb.inverse_dynamics_host(me, q[e:e + 1], qd[e:e + 1], qdd[e:e + 1])))
    print(f"{name}: primal at theta vs params_apply max rel = {worst:.3e}")
    assert worst <= 1e-12


# ---------------------------------------------------------------- against central differences of the host query
@pytest.mark.parametrize("name", SUPPORTED)
def test_tangents_match_central_differences_of_the_host_query(name, built):
    """every column of z (theta's through params_apply) and every output, each output with its own scale"""
    m, q, qd, tau, qdd = inputs(name)
    names, sel = wanted(m), selection(m, name)
    n, p = q.shape[0], len(sel)
    th = thetas(m, sel, n)
    nz = hb.dyn_input_dim(m) + p
    tan = hb.dynamics_jvp_host(m, q, qd, tau, eye_dirs(n, nz), want=names, params=sel, theta=th)
    worst = {}
    for e in (0, n // 2, n - 1):
        J_fd = central(m, np.concatenate([q[e], qd[e], tau[e], th[e]]), sel, names, False)
        o = 0
        for k in names:
            J = tan[k][e].reshape(nz, -1).T
            if not J.size:  # a base without links has no x_world
                continue
            err = float(np.max(np.abs(J - J_fd[o:o + J.shape[0]])) / max(1.0, np.max(np.abs(J))))
            worst[k] = max(worst.get(k, 0.0), err)
            o += J.shape[0]
            assert np.max(np.abs(J)) > 0, k
    if not m.is_floating:
        nzi = hb.dyn_input_dim(m, True) + p
        dt = hb.inverse_dynamics_jvp_host(m, q, qd, qdd, eye_dirs(n, nzi), params=sel, theta=th)
        for e in (0, n // 2, n - 1):
            J_fd = central(m, np.concatenate([q[e], qd[e], qdd[e], th[e]]), sel, None, True)
            J = dt[e].T
            worst["tau"] = max(worst.get("tau", 0.0), float(np.max(np.abs(J - J_fd)) / max(1.0, np.max(np.abs(J)))))
    print(f"{name}: tangents vs central differences: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert max(worst.values()) <= FD_BOUND


# ---------------------------------------------------------------- against the reference
def ref_fd(r, m, x, cols):
    """central differences of RefSim.debug's M and qdd over the record's columns `cols`"""
    JM, Jq = [], []
    for j in cols:
        h = H_REL * max(1.0, abs(x[j]))
        xp, xm = x.copy(), x.copy()
        xp[j] += h
        xm[j] -= h
        a, b = r.debug(xp, m), r.debug(xm, m)
        JM.append((a["M"] - b["M"]).ravel() / (2 * h))
        Jq.append((a["qdd"] - b["qdd"]) / (2 * h))
    return np.stack(JM), np.stack(Jq)


@needs_ref
@pytest.mark.parametrize("name", SUPPORTED)
def test_mass_matrix_and_qdd_tangents_match_the_reference(name, built):
    """every q and qd column, a floating base's four quaternion entries included (M and the base-frame qdd do not move
    with them, in the reference or here: no column is left out)"""
    m, x = states(name)
    q, qd, tau = split(m, x)
    cols = list(range(m.dof_q + m.dof_qd))
    r = make_ref(name)
    worst = 0.0
    try:
        for e in (0, x.shape[0] - 1):
            v = np.zeros((1, len(cols), hb.dyn_input_dim(m)))
            v[0, np.arange(len(cols)), cols] = 1.0
            tan = hb.dynamics_jvp_host(m, q[e:e + 1], qd[e:e + 1], tau[e:e + 1], v, want=("mass_matrix", "qdd"))
            JM, Jq = ref_fd(r, m, x[e], cols)
            for J, J_fd in ((tan["mass_matrix"][0].reshape(len(cols), -1), JM), (tan["qdd"][0], Jq)):
                worst = max(worst, float(np.max(np.abs(J - J_fd)) / max(1.0, np.max(np.abs(J)))))
    finally:
        r.close()
    print(f"{name}: dM, dqdd vs central differences of the reference = {worst:.3e}")
    assert worst <= FD_BOUND


@needs_ref
def test_gravity_and_spring_tangents_match_the_reference(built):
    """pendulum5: gravity z through set_gravity, link 2's stiffness and damping through set_link_spring"""
    m, x = states("pendulum5")
    for i in range(m.num_links):
        m.links[i].stiffness, m.links[i].damping = 3.0 + i, 0.2 + 0.1 * i
    q, qd, tau = split(m, x)
    sel = [("gravity", 2), ("stiffness", 2), ("damping", 2)]
    th = hb.params_get(m, sel)
    n, nx = x.shape[0], hb.dyn_input_dim(m)
    v = np.zeros((n, 3, nx + 3))
    v[:, np.arange(3), nx + np.arange(3)] = 1.0
    tan = hb.dynamics_jvp_host(m, q, qd, tau, v, want=("qdd",), params=sel)["qdd"]

    def ref_qdd(theta):
        r = make_ref("pendulum5")
        try:
            for i in range(m.num_links):
                r.set_link_spring(i, m.links[i].stiffness, m.links[i].damping)
            r.set_gravity([m.gravity[0], m.gravity[1], theta[0]])
            r.set_link_spring(2, theta[1], theta[2])
            return np.stack([r.debug(x[e], m)["qdd"] for e in range(n)])
        finally:
            r.close()

    worst = 0.0
    for j in range(3):
        h = H_REL * max(1.0, abs(th[j]))
        tp, tm = th.copy(), th.copy()
        tp[j] += h
        tm[j] -= h
        J_fd = (ref_qdd(tp) - ref_qdd(tm)) / (2 * h)
        assert np.max(np.abs(tan[:, j])) > 1e-3
        worst = max(worst, float(np.max(np.abs(tan[:, j] - J_fd)) / max(1.0, np.max(np.abs(tan[:, j])))))
    print(f"pendulum5: dqdd / d(gravity z, stiffness, damping) vs the reference = {worst:.3e}")
    assert worst <= FD_BOUND


# ---------------------------------------------------------------- identities
@pytest.mark.parametrize("name", FIXED)
def test_inverse_dynamics_in_qdd_is_the_mass_matrix(name, built):
    m, q, qd, tau, qdd = inputs(name)
    n, nq, nd = q.shape[0], m.dof_q, m.dof_qd
    v = np.zeros((n, nd, nq + 2 * nd))
    v[:, np.arange(nd), nq + nd + np.arange(nd)] = 1.0
    dt = hb.inverse_dynamics_jvp_host(m, q, qd, qdd, v)  # [n][j][i] = d tau_i / d qdd_j
    M = hb.dynamics_host(m, q, want=("mass_matrix",))["mass_matrix"]
    assert rel(dt, M.transpose(0, 2, 1)) <= 1e-12


@pytest.mark.parametrize("name", FIXED)
def test_qdd_in_tau_is_the_inverse_mass_matrix(name, built):
    m, q, qd, tau, qdd = inputs(name)
    n, nq, nd = q.shape[0], m.dof_q, m.dof_qd
    v = np.zeros((n, nd, nq + 2 * nd))
    v[:, np.arange(nd), nq + nd + np.arange(nd)] = 1.0
    tan, prim = hb.dynamics_jvp_host(m, q, qd, tau, v, want=("qdd", "mass_matrix"), want_primal=True)
    prod = np.einsum("nab,njb->nja", prim["mass_matrix"], tan["qdd"])
    assert rel(prod, np.broadcast_to(np.eye(nd), prod.shape)) <= 1e-10


@pytest.mark.parametrize("name", FIXED)
def test_tangents_of_one_call_satisfy_the_equation_of_motion(name, built):
    """M dqdd + dM qdd + dbias + K dq + D dqd = dtau along random directions"""
    m, q, qd, tau, qdd = inputs(name)
    n, nq, nd = q.shape[0], m.dof_q, m.dof_qd
    v = np.random.default_rng(5).normal(size=(n, 5, nq + 2 * nd))
    tan, prim = hb.dynamics_jvp_host(m, q, qd, tau, v, want=hb.DYN_OUTPUTS, want_primal=True)
    lhs = np.einsum("nab,nkb->nka", prim["mass_matrix"], tan["qdd"]) + \
        np.einsum("nkab,nb->nka", tan["mass_matrix"], prim["qdd"]) + tan["bias"]
    for k in range(v.shape[1]):
        lhs[:, k] += spring_terms(m, v[:, k, :nq], v[:, k, nq:nq + nd])
    assert rel(lhs, v[:, :, nq + nd:]) <= 1e-10


@pytest.mark.parametrize("name", SUPPORTED)
def test_mass_matrix_tangent_is_symmetric(name, built):
    m, q, qd, tau, qdd = inputs(name)
    v = np.random.default_rng(6).normal(size=(q.shape[0], 3, hb.dyn_input_dim(m)))
    dM = hb.dynamics_jvp_host(m, q, qd, tau, v, want=("mass_matrix",))["mass_matrix"]
    assert np.max(np.abs(dM)) > 0 or m.num_links == 0
    assert rel(dM, dM.transpose(0, 1, 3, 2)) <= 1e-10


@pytest.mark.parametrize("name", FIXED)
def test_coriolis_power_is_half_the_mass_matrix_rate(name, built):
    """gravity selected and set to zero: bias = C(q, qd) qd, and qd^T C qd = 1/2 qd^T Mdot qd with Mdot = dM[dq = qd]
    (fixed base, 1-DoF joints: dof_q = dof_qd).  The identity needs joint transforms that are the rigid motions S
    generates, so unit joint axes.  The Ant's ankle axes are (0.7071067, 0.7071067, 0) as the reference has them,
    |S|^2 = 1 - 2.4e-7, and the model as it is misses the identity by that much (measured 1.2e-7, printed below); the
    check runs on a copy with the axes scaled to unit length (measured 1.3e-15), the same copy for every model."""
    m, q, qd, tau, qdd = inputs(name)
    raw, m = m, m.copy()
    for i in range(m.num_links):
        s = np.array(m.links[i].S)
        for k in range(6):
            m.links[i].S[k] = s[k] / (np.linalg.norm(s) or 1.0)  # (a fixed joint's S is zero)
    n, nq, nd = q.shape[0], m.dof_q, m.dof_qd
    assert nq == nd
    qd = qd + np.random.default_rng(8).normal(size=qd.shape)  # the golden records are close to rest
    sel = [("gravity", 0), ("gravity", 1), ("gravity", 2)]
    v = np.zeros((n, 1, nq + 2 * nd + 3))
    v[:, 0, :nq] = qd
    tan, prim = hb.dynamics_jvp_host(m, q, qd, None, v, want=("mass_matrix", "bias"), params=sel, theta=np.zeros(3),
                                     want_primal=True)
    lhs = np.einsum("na,na->n", qd, prim["bias"])
    rhs = 0.5 * np.einsum("na,nab,nb->n", qd, tan["mass_matrix"][:, 0], qd)
    t_raw, p_raw = hb.dynamics_jvp_host(raw, q, qd, None, v, want=("mass_matrix", "bias"), params=sel, theta=np.zeros(3),
                                        want_primal=True)
    miss = rel(np.einsum("na,na->n", qd, p_raw["bias"]), 0.5 * np.einsum("na,nab,nb->n", qd, t_raw["mass_matrix"][:, 0], qd))
    print(f"{name}: qd^T bias against 1/2 qd^T Mdot qd: {rel(lhs, rhs):.3e} (axes as the model has them: {miss:.3e})")
    assert np.max(np.abs(lhs)) > 1e-3
    assert rel(lhs, rhs) <= 1e-10


@pytest.mark.parametrize("name", FIXED)
def test_gravity_torques_are_linear_in_gravity(name, built):
    """qd = qdd = 0: ID is linear in g, so its tangent along theta_gravity = g is ID itself"""
    m, q, qd, tau, qdd = inputs(name)
    n, nq, nd = q.shape[0], m.dof_q, m.dof_qd
    sel = [("gravity", 0), ("gravity", 1), ("gravity", 2)]
    v = np.zeros((n, 1, nq + 2 * nd + 3))
    v[:, 0, nq + 2 * nd:] = hb.params_get(m, sel)
    dt, t = hb.inverse_dynamics_jvp_host(m, q, None, None, v, params=sel, want_primal=True)
    assert np.max(np.abs(t)) > 0 or name.startswith("cartpole")
    assert rel(dt[:, 0], t) <= 1e-12


@pytest.mark.parametrize("name", SUPPORTED)
def test_contact_model_parameters_give_exact_zeros(name, built):
    m, q, qd, tau, qdd = inputs(name)
    sel = CONTACT_KINDS + ([("geom_trans", 0, 2)] if m.num_geoms else [])
    n, nx, p = q.shape[0], hb.dyn_input_dim(m), len(sel)
    v = np.zeros((n, p, nx + p))
    v[:, np.arange(p), nx + np.arange(p)] = 1.0
    tan = hb.dynamics_jvp_host(m, q, qd, tau, v, want=wanted(m), params=sel, theta=hb.params_get(m, sel) + 0.1)
    for k, t in tan.items():
        assert not t.any(), k
    if not m.is_floating:
        vi = np.zeros((n, p, hb.dyn_input_dim(m, True) + p))
        vi[:, np.arange(p), hb.dyn_input_dim(m, True) + np.arange(p)] = 1.0
        assert not hb.inverse_dynamics_jvp_host(m, q, qd, qdd, vi, params=sel).any()


@pytest.mark.parametrize("name", SUPPORTED)
def test_tangents_are_linear_in_the_directions(name, built):
    m, q, qd, tau, qdd = inputs(name)
    names, sel = wanted(m), selection(m, name)
    n, nz = q.shape[0], hb.dyn_input_dim(m) + len(sel)
    rng = np.random.default_rng(9)
    a, b = rng.normal(size=(n, 1, nz)), rng.normal(size=(n, 1, nz))
    v = np.concatenate([a, b, 2.0 * a - 3.0 * b, np.zeros_like(a)], axis=1)
    tan = hb.dynamics_jvp_host(m, q, qd, tau, v, want=names, params=sel)
    for k in names:
        t = tan[k]
        assert rel(t[:, 2], 2.0 * t[:, 0] - 3.0 * t[:, 1]) <= 1e-10, k
        assert not t[:, 3].any(), k


# ---------------------------------------------------------------- the regressor of inverse-dynamics identification
def test_mass_regressor_identifies_the_link_masses(built):
    """tau is affine in the link masses: Y = dID / dtheta is exact for any step, and least squares on it recovers them"""
    m = tds_amd.load_model("pendulum5")
    rng = np.random.default_rng(11)
    n, nq, nd = 64, m.dof_q, m.dof_qd
    q, qd, qdd = rng.uniform(-1, 1, (n, nq)), rng.normal(size=(n, nd)), rng.normal(size=(n, nd))
    sel = [("mass", i) for i in range(5)]
    th = hb.params_get(m, sel)
    v = np.zeros((n, 5, nq + 2 * nd + 5))
    v[:, np.arange(5), nq + 2 * nd + np.arange(5)] = 1.0
    Y, t0 = hb.inverse_dynamics_jvp_host(m, q, qd, qdd, v, params=sel, want_primal=True)  # Y [n][5][nd]
    t1 = hb.inverse_dynamics_host(hb.params_apply(m, sel, 1.3 * th), q, qd, qdd)
    assert rel(t1, t0 + np.einsum("njd,j->nd", Y, 0.3 * th)) <= 1e-11
    A = Y.transpose(0, 2, 1).reshape(n * nd, 5)
    cond = np.linalg.cond(A)
    print(f"cond(Y) = {cond:.3e}")
    assert cond < 1e8
    # tau(theta) = tau(theta0) + Y (theta - theta0): solve for theta from the torques of the heavier model
    est = th + np.linalg.lstsq(A, (t1 - t0).ravel(), rcond=None)[0]
    assert rel(est, 1.3 * th) <= 1e-9


# ---------------------------------------------------------------- refusals and arguments
@pytest.mark.parametrize("name", REFUSED)
def test_unsupported_models_are_refused(name, built):
    m = tds_amd.load_model(name)
    q = np.zeros((1, m.dof_q))
    with pytest.raises(hb.TdsHipError, match="not supported"):
        hb.dynamics_jvp_host(m, q, want=("mass_matrix",))
    with pytest.raises(hb.TdsHipError, match="not supported"):
        hb.inverse_dynamics_jvp_host(m, q)
    with pytest.raises(hb.TdsHipError, match="not supported"):
        hb.dynamics_jvp_tangents(m)


def test_floating_base_bias_and_inverse_dynamics_are_refused(built):
    m, q, qd, tau, qdd = inputs("ant_floating")
    v = np.zeros((q.shape[0], 1, hb.dyn_input_dim(m)))
    with pytest.raises(hb.TdsHipError, match="need a fixed base"):
        hb.dynamics_jvp_host(m, q, qd, tau, v, want=("bias",))
    with pytest.raises(hb.TdsHipError, match="need a fixed base"):
        hb.dynamics_jvp_host(m, q, qd, tau, None, want=("bias",))
    with pytest.raises(hb.TdsHipError, match="need a fixed base"):
        hb.inverse_dynamics_jvp_host(m, q)
    assert hb.dynamics_jvp_tangents(m) >= 1


def test_bad_selections_and_arguments(built):
    import ctypes as C

    m, q, qd, tau, qdd = inputs("pendulum5")
    n, nx = q.shape[0], hb.dyn_input_dim(m)
    with pytest.raises(hb.TdsHipError, match="link index out of range"):
        hb.dynamics_jvp_host(m, q, params=[("mass", 99)])
    with pytest.raises(hb.TdsHipError, match="duplicate parameter"):
        hb.inverse_dynamics_jvp_host(m, q, params=[("mass", 1), ("mass", 1)])
    with pytest.raises(hb.TdsHipError, match="need a floating base"):
        hb.dynamics_jvp_host(m, q, params=[("base_mass",)])
    L, out = hb.lib(), np.zeros((n, m.dof_qd))
    o = hb.DynOut(qdd=out.ctypes.data)
    v = np.zeros((n, 1, nx))
    args = (C.byref(m), n, q.ctypes.data, None, None, 0, None, None)
    assert L.tds_hip_dynamics_jvp_host(*args, -1, v.ctypes.data, C.byref(o), C.byref(o)) == 1  # k < 0
    assert L.tds_hip_dynamics_jvp_host(*args, 1, None, C.byref(o), C.byref(o)) == 1  # k > 0, v NULL
    assert "NULL or empty argument" in L.tds_hip_last_error().decode()
    assert L.tds_hip_dynamics_jvp_host(*args, 1, v.ctypes.data, C.byref(o), None) == 1  # no tangent requested
    assert "no output requested" in L.tds_hip_last_error().decode()
    assert L.tds_hip_dynamics_jvp_host(*args, 0, None, C.byref(hb.DynOut()), None) == 1  # no output requested
    assert L.tds_hip_dynamics_jvp_host(*args, 0, None, None, None) == 1
    assert L.tds_hip_inverse_dynamics_jvp_host(*args, 1, v.ctypes.data, out.ctypes.data, None) == 1
    assert "no output requested" in L.tds_hip_last_error().decode()
    assert L.tds_hip_inverse_dynamics_jvp_host(*args, 0, None, None, None) == 1
    assert L.tds_hip_dynamics_jvp_host(*args, 0, None, C.byref(o), None) == 0
    assert L.tds_hip_dynamics_jvp_host(*args, 1, v.ctypes.data, None, C.byref(o)) == 0


def test_a_singular_mass_matrix_gives_nan_in_qdd_and_its_tangents_only(built):
    """massless links: M is not positive definite; every output is written, then the call fails"""
    m = tds_amd.load_model("pendulum5")
    sel = [("mass", i) for i in range(5)] + [("inertia", i, c) for i in range(5) for c in range(3)]
    th = np.zeros(len(sel))
    q = np.full((2, m.dof_q), 0.3)
    v = np.ones((2, 1, hb.dyn_input_dim(m) + len(sel)))
    tan = {k: np.full(s, 7.0) for k, s in hb.dyn_tangent_shapes(m, 2, 1).items()}
    prim = {k: np.full(s, 7.0) for k, s in hb.dyn_shapes(m, 2).items()}
    with pytest.raises(hb.TdsHipError, match="not positive definite"):
        hb.dynamics_jvp_host(m, q, None, None, v, params=sel, theta=th, want_primal=True, out=tan, out_primal=prim)
    for d in (tan, prim):
        assert np.isnan(d["qdd"]).all()
        for k in ("x_world", "mass_matrix", "bias"):
            assert np.isfinite(d[k]).all() and not (d[k] == 7.0).all(), k
