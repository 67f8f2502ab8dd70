"""Batched dynamics queries on the CPU (tds_hip_dynamics_host / _inverse_dynamics_host / _point_jacobian_host: the host
instantiation of csrc/tds_dyn.h): against the reference where it is built, and against each other everywhere."""
import numpy as np
import pytest

import tds_amd
from tds_amd import hip_backend as hb

from test_jacobian_cpu import REFUSED, SUPPORTED, golden, make_ref, needs_ref

FIXED = [n for n in SUPPORTED if not tds_amd.load_model(n).is_floating]
FLOATING = [n for n in SUPPORTED if tds_amd.load_model(n).is_floating]

# qdd and inverse dynamics against the reference go through a solve: the bound is 10 x the largest host-vs-reference
# difference measured on the CPU over states(name) of every model (relative, denominator max(|ref|, 1)):
#   qdd   ant 2.1e-14, ant_floating 1.1e-14, laikago 1.9e-14, laikago_floating 8.7e-15, laikago_floating_env 1.8e-15,
#         laikago_soft 4.1e-14, cartpole 7.8e-16, cartpole_plane 4.3e-16, pendulum5 1.4e-13, pendulum5_plane 4.6e-13,
#         cube_floating 0; with springs set on pendulum5: 2.3e-13                          -> maximum 4.6e-13
#   ID(q, qd, qdd_ref) against tau - K q - D qd: ant 1.3e-15, laikago 4.0e-14, laikago_soft 5.9e-14, cartpole 4.4e-16,
#         cartpole_plane 1.8e-15, pendulum5 1.4e-14, pendulum5_plane 6.4e-15               -> maximum 5.9e-14
# (both far below the project's gate of 1e-6; each test prints its figure before it asserts)
QDD_BOUND = 10 * 4.6e-13
ID_BOUND = 10 * 5.9e-14


def rel(a, b):
    """largest |a - b| / max(|b|, 1) (the denominator of test_double_instantiation_matches_reference)"""
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1.0))) if a.size else 0.0


def states(name, k=6, seed=1):
    """records of the model: k golden ones, then the same with seeded perturbations of q | qd (unit base quaternion)"""
    m = tds_amd.load_model(name)
    x, _ = golden(name, k)
    rng = np.random.default_rng(seed)
    xp = x + rng.normal(0, 1e-3, x.shape) * (np.arange(x.shape[1]) < m.dof_q + m.dof_qd)
    x = np.concatenate([x, xp])
    if m.is_floating:
        x[:, 0:4] /= np.linalg.norm(x[:, 0:4], axis=1, keepdims=True)
    return m, x


def split(m, x):
    """q, qd and the torques the reference's forward_dynamics sees: zero for locomotion models (initialize() clears
    them), the record's action slots for torque models"""
    nq, nd = m.dof_q, m.dof_qd
    loco = m.step_mode == tds_amd.TDS_STEP_LOCOMOTION
    nt = hb.dyn_tau_dim(m)
    tau = np.zeros((x.shape[0], nt)) if loco else x[:, nq + nd:nq + nd + nt].copy()
    return x[:, :nq].copy(), x[:, nq:nq + nd].copy(), tau


def spring_terms(m, q, qd):
    """K q + D qd per dof"""
    out = np.zeros((q.shape[0], m.dof_qd))
    for i in range(m.num_links):
        l = m.links[i]
        if l.qd_index >= 0 and l.joint_type != tds_amd.JOINT_FIXED:
            out[:, l.qd_index] = l.stiffness * q[:, l.q_index] + l.damping * qd[:, l.qd_index]
    return out


def wanted(m):
    return ("x_world", "mass_matrix", "qdd") if m.is_floating else hb.DYN_OUTPUTS


# ---------------------------------------------------------------- against the reference
@needs_ref
@pytest.mark.parametrize("name", SUPPORTED)
def test_kinematics_mass_matrix_and_point_jacobians_match_reference(name, built):
    m, x = states(name)
    q, qd, tau = split(m, x)
    d = hb.dynamics_host(m, q, qd, tau, want=("x_world", "mass_matrix"))
    r = make_ref(name)
    rows = 0
    try:
        for e in range(x.shape[0]):
            dbg = r.debug(x[e], m)
            assert rel(d["x_world"][e], dbg["X_world"]) <= 1e-9
            assert rel(d["mass_matrix"][e], dbg["M"]) <= 1e-9
            for c in range(len(dbg["links"])):
                J = hb.point_jacobian_host(m, q[e:e + 1], int(dbg["links"][c]), dbg["contacts"][c, 3:6])[0]
                assert rel(J, dbg["jac"][c]) <= 1e-9
                rows += 3
    finally:
        r.close()
    print(f"{name}: {rows} Jacobian rows checked")
    if name in ("ant", "laikago", "cartpole_plane", "pendulum5_plane"):
        assert rows > 0


@needs_ref
@pytest.mark.parametrize("name", SUPPORTED)
def test_forward_dynamics_matches_reference(name, built):
    m, x = states(name)
    q, qd, tau = split(m, x)
    qdd = hb.dynamics_host(m, q, qd, tau, want=("qdd",))["qdd"]
    r = make_ref(name)
    try:
        err = max(rel(qdd[e], r.debug(x[e], m)["qdd"]) for e in range(x.shape[0]))
    finally:
        r.close()
    print(f"{name}: qdd host vs reference max rel = {err:.3e} (bound {QDD_BOUND:.1e})")
    assert err <= QDD_BOUND <= 1e-6


@needs_ref
def test_forward_dynamics_with_springs_matches_reference(built):
    """joint stiffness and damping set on the reference and in the blob (laikago_soft, whose blob carries springs, is
    one of the models of test_forward_dynamics_matches_reference)"""
    m, x = states("pendulum5")
    q, qd, tau = split(m, x)
    r = make_ref("pendulum5")
    try:
        for i in range(m.num_links):
            k, dmp = 3.0 + i, 0.2 + 0.1 * i
            r.set_link_spring(i, k, dmp)
            m.links[i].stiffness, m.links[i].damping = k, dmp
        qdd = hb.dynamics_host(m, q, qd, tau, want=("qdd",))["qdd"]
        plain = hb.dynamics_host(tds_amd.load_model("pendulum5"), q, qd, tau, want=("qdd",))["qdd"]
        err = max(rel(qdd[e], r.debug(x[e], m)["qdd"]) for e in range(x.shape[0]))
    finally:
        r.close()
    print(f"pendulum5 with springs: qdd host vs reference max rel = {err:.3e}")
    assert err <= QDD_BOUND
    assert np.max(np.abs(qdd - plain)) > 1e-3  # the springs act


@needs_ref
@pytest.mark.parametrize("name", FIXED)
def test_inverse_dynamics_of_reference_accelerations(name, built):
    """ID(q, qd, qdd_ref) = tau - K q - D qd with the reference's forward dynamics"""
    m, x = states(name)
    q, qd, tau = split(m, x)
    r = make_ref(name)
    try:
        qdd_ref = np.stack([r.debug(x[e], m)["qdd"] for e in range(x.shape[0])])
    finally:
        r.close()
    got = hb.inverse_dynamics_host(m, q, qd, qdd_ref)
    err = rel(got, tau - spring_terms(m, q, qd))
    print(f"{name}: ID(qdd_ref) vs tau - Kq - Dqd max rel = {err:.3e} (bound {ID_BOUND:.1e})")
    assert err <= ID_BOUND <= 1e-6


# ---------------------------------------------------------------- without the reference
@pytest.mark.parametrize("name", SUPPORTED)
def test_mass_matrix_is_symmetric_and_positive_definite(name, built):
    m, x = states(name)
    q, _, _ = split(m, x)
    M = hb.dynamics_host(m, q, want=("mass_matrix",))["mass_matrix"]
    if m.is_floating:  # the base's 6 x 6 block is the composite inertia's I and M blocks as the sweep leaves them (the
        assert np.max(np.abs(M - M.transpose(0, 2, 1))) <= 1e-14  # reference's too): symmetric to round-off only
        np.testing.assert_array_equal(M[:, 6:, :], M[:, :, 6:].transpose(0, 2, 1))
    else:  # both triangles are written with the same value
        np.testing.assert_array_equal(M, M.transpose(0, 2, 1))
    assert M.shape == (x.shape[0], m.dof_qd, m.dof_qd)
    for e in range(M.shape[0]):
        assert np.min(np.linalg.eigvalsh(M[e])) > 0.0


@pytest.mark.parametrize("name", FIXED)
def test_rnea_columns_are_the_crba_mass_matrix(name, built):
    """two independent algorithms: ID(q, 0, e_j) - ID(q, 0, 0) = M e_j"""
    m, x = states(name)
    q, _, _ = split(m, x)
    nd = m.dof_qd
    M = hb.dynamics_host(m, q, want=("mass_matrix",))["mass_matrix"]
    g = hb.inverse_dynamics_host(m, q)
    for j in range(nd):
        col = hb.inverse_dynamics_host(m, q, None, np.eye(nd)[j]) - g
        assert np.max(np.abs(col - M[:, :, j])) <= 1e-11, j


@pytest.mark.parametrize("name", FIXED)
def test_bias_mass_matrix_and_inverse_dynamics_agree(name, built):
    m, x = states(name)
    q, qd, tau = split(m, x)
    d = hb.dynamics_host(m, q, qd, tau)
    np.testing.assert_array_equal(d["bias"], hb.inverse_dynamics_host(m, q, qd, None))  # bias = ID(q, qd, 0)
    np.testing.assert_array_equal(d["bias"], hb.inverse_dynamics_host(m, q, qd, np.zeros_like(qd)))
    Mqdd = np.einsum("nij,nj->ni", d["mass_matrix"], d["qdd"])
    tid = hb.inverse_dynamics_host(m, q, qd, d["qdd"])
    assert rel(Mqdd + d["bias"], tid) <= 1e-11
    assert np.max(np.abs(d["bias"])) > 0.0


@pytest.mark.parametrize("name", FIXED)
def test_forward_dynamics_inverts_inverse_dynamics(name, built):
    """forward_dynamics(q, qd, ID(q, qd, a) + K q + D qd) = a, to the measured bound of the solve"""
    m, x = states(name)
    q, qd, _ = split(m, x)
    a = np.random.default_rng(5).normal(0, 2.0, qd.shape)
    tau = hb.inverse_dynamics_host(m, q, qd, a) + spring_terms(m, q, qd)
    back = hb.dynamics_host(m, q, qd, tau, want=("qdd",))["qdd"]
    err = rel(back, a)
    print(f"{name}: FD(ID(a)) vs a max rel = {err:.3e}")
    assert err <= QDD_BOUND


def link_points(m, q, rng):
    """a non-fixed link per model (the last one) and a link-local point per state"""
    link = max(i for i in range(m.num_links) if m.links[i].joint_type != tds_amd.JOINT_FIXED)
    return link, rng.normal(0, 0.2, (q.shape[0], 3))


def world_of_local(m, q, link, p_local):
    X = hb.dynamics_host(m, q, want=("x_world",))["x_world"][:, link]
    return np.einsum("nij,nj->ni", X[:, :9].reshape(-1, 3, 3), p_local) + X[:, 9:]


@pytest.mark.parametrize("name", FIXED)
def test_point_jacobian_times_qd_is_the_points_velocity(name, built):
    """J qd = d/dh of the world position of a link-local point along q + h qd (central differences)"""
    m, x = states(name)
    q, qd, _ = split(m, x)
    link, pl = link_points(m, q, np.random.default_rng(3))
    J = hb.point_jacobian_host(m, q, link, pl, local=True)
    h = 1e-6
    fd = (world_of_local(m, q + h * qd, link, pl) - world_of_local(m, q - h * qd, link, pl)) / (2 * h)
    assert np.max(np.abs(np.einsum("nij,nj->ni", J, qd) - fd)) <= 1e-6
    assert np.count_nonzero(J) > 0


@pytest.mark.parametrize("name", [n for n in SUPPORTED if tds_amd.load_model(n).num_links > 0])
def test_point_jacobian_local_and_world_flags_agree(name, built):
    m, x = states(name)
    q, _, _ = split(m, x)
    link, pl = link_points(m, q, np.random.default_rng(4))
    Jl = hb.point_jacobian_host(m, q, link, pl, local=True)
    Jw = hb.point_jacobian_host(m, q, link, world_of_local(m, q, link, pl), local=False)
    assert rel(Jl, Jw) <= 1e-12
    assert Jl.shape == (x.shape[0], 3, m.dof_qd)


@pytest.mark.parametrize("name", ["ant", "laikago_floating", "pendulum5_plane"])
def test_want_subsets_are_slices_of_the_full_call(name, built):
    m, x = states(name)
    q, qd, tau = split(m, x)
    full = hb.dynamics_host(m, q, qd, tau, want=wanted(m))
    for k in wanted(m):
        np.testing.assert_array_equal(hb.dynamics_host(m, q, qd, tau, want=(k,))[k], full[k])
    pair = hb.dynamics_host(m, q, qd, tau, want=("qdd", "x_world"))
    assert sorted(pair) == ["qdd", "x_world"]
    np.testing.assert_array_equal(pair["qdd"], full["qdd"])


def test_any_number_of_states(built):
    m, x = states("ant")
    q, qd, tau = split(m, x)
    full = hb.dynamics_host(m, q, qd, tau)
    for n in (1, 5):
        part = hb.dynamics_host(m, q[:n], qd[:n], tau[:n])
        for k in full:
            np.testing.assert_array_equal(part[k], full[k][:n])
    big = hb.dynamics_host(m, np.tile(q, (9, 1)), np.tile(qd, (9, 1)), np.tile(tau, (9, 1)), want=("qdd",))["qdd"]
    np.testing.assert_array_equal(big, np.tile(full["qdd"], (9, 1)))


@pytest.mark.parametrize("name", REFUSED)
def test_models_out_of_scope_are_refused(name, built):
    """the refusals (and messages) of tds_hip_jacobian"""
    m = tds_amd.load_model(name)
    q = np.zeros((1, m.dof_q))
    with pytest.raises(hb.TdsHipError, match="error 2: step Jacobians: .* not supported"):
        hb.dynamics_host(m, q)
    with pytest.raises(hb.TdsHipError, match="error 2: step Jacobians: .* not supported"):
        hb.inverse_dynamics_host(m, q)
    with pytest.raises(hb.TdsHipError, match="error 2: step Jacobians: .* not supported"):
        hb.point_jacobian_host(m, q, 0, np.zeros(3))


@pytest.mark.parametrize("name", FLOATING)
def test_floating_base_inverse_dynamics_is_refused(name, built):
    m, x = states(name)
    q, qd, tau = split(m, x)
    with pytest.raises(hb.TdsHipError, match="error 2: .*no floating-base inverse dynamics"):
        hb.dynamics_host(m, q, qd, tau, want=("bias",))
    with pytest.raises(hb.TdsHipError, match="error 2: .*no floating-base inverse dynamics"):
        hb.inverse_dynamics_host(m, q, qd, None)
    d = hb.dynamics_host(m, q, qd, tau, want=wanted(m))  # the rest is served
    assert all(np.all(np.isfinite(v)) for v in d.values())


def test_invalid_arguments(built):
    import ctypes as C

    m, x = states("ant")
    q, _, _ = split(m, x)
    for link in (m.num_links, -2):
        with pytest.raises(hb.TdsHipError, match="error 1: .*link index out of range"):
            hb.point_jacobian_host(m, q, link, np.zeros(3))
    L = hb.lib()
    out = hb.DynOut()
    M = np.zeros((1, m.dof_qd, m.dof_qd))
    assert L.tds_hip_dynamics_host(C.byref(m), 1, q.ctypes.data, None, None, C.byref(out)) == 1  # nothing requested
    out.mass_matrix = M.ctypes.data
    assert L.tds_hip_dynamics_host(C.byref(m), 0, q.ctypes.data, None, None, C.byref(out)) == 1  # n < 1
    assert L.tds_hip_dynamics_host(C.byref(m), 1, None, None, None, C.byref(out)) == 1  # NULL q
    assert L.tds_hip_dynamics_host(C.byref(m), 1, q.ctypes.data, None, None, None) == 1  # NULL out
    assert L.tds_hip_dynamics_host(C.byref(m), 1, q.ctypes.data, None, None, C.byref(out)) == 0
    assert L.tds_hip_inverse_dynamics_host(C.byref(m), 1, q.ctypes.data, None, None, None) == 1
    assert L.tds_hip_point_jacobian_host(C.byref(m), 1, q.ctypes.data, 0, None, 0, M.ctypes.data) == 1
    with pytest.raises(ValueError, match="unknown dynamics output"):
        hb.dynamics_host(m, q, want=("jacobian",))
