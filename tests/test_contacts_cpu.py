"""The batched contact query on the CPU (tds_hip_contacts_host: the host instantiation of csrc/tds_contact.h): against
the reference where it is built, against the double step (step_host) and against plain numpy restatements everywhere."""
import functools

import numpy as np
import pytest

import tds_amd
from tds_amd import hip_backend as hb

import diff_states as ds
from test_dynamics_cpu import rel
from test_jacobian_cpu import REFUSED, SUPPORTED, golden, make_ref, needs_ref

PLANE = [n for n in SUPPORTED if tds_amd.load_model(n).has_plane]
NO_PLANE = [n for n in SUPPORTED if not tds_amd.load_model(n).has_plane]

# The momentum identities against the reference go through its M and its stepped qd: the bound is 10 x the largest
# host-vs-reference difference measured on the CPU over states(name) of every model (relative, denominator
# max(|ref|, 1); each test prints its figures before it asserts):
#   M_ref (qd_pre - qd_post_ref) = rows^T impulse, and sum_c jac_c^T force_c dt = M_ref (qd_post_ref - qd_pre), the
#   larger of the two: ant 3.0e-15, ant_floating 2.7e-15, laikago 1.3e-14, laikago_floating 2.2e-14,
#         laikago_floating_env 6.2e-15, laikago_soft 6.9e-15, cartpole_plane 5.7e-16, pendulum5_plane 2.3e-12,
#         cube_floating 2.1e-14                                                            -> maximum 2.3e-12
MOMENTUM_BOUND = 10 * 2.3e-12
# Without the reference (relative, denominator max(|value|, 1)):
#   delassus against rows M^-1 rows^T + cfm 1 (M from dynamics_host, numpy's solve):
#         ant 1.4e-14, ant_floating 1.7e-14, laikago 2.0e-15, laikago_floating 2.6e-15, laikago_floating_env 1.7e-15,
#         laikago_soft 2.0e-15, cartpole_plane 3.3e-16, pendulum5_plane 4.2e-14, cube_floating 1.1e-16
#                                                                                          -> maximum 4.2e-14
#   impulse against numpy's solve_pgs on the returned delassus and rhs:
#         ant 5.9e-16, ant_floating 5.8e-16, laikago 1.8e-15, laikago_floating 7.2e-15, laikago_floating_env 2.6e-15,
#         laikago_soft 1.4e-15, cartpole_plane 5.0e-14, pendulum5_plane 4.1e-14, cube_floating 4.8e-14
#                                                                                          -> maximum 5.0e-14
DELASSUS_BOUND = 10 * 4.2e-14
PGS_BOUND = 10 * 5.0e-14


@functools.lru_cache(maxsize=None)
def states(name):
    """the model and its records: 6 golden ones and, for the models of diff_states, 48 seeded states that span every
    penetrating contact count (shared by the tests: treat as read-only)"""
    m = tds_amd.load_model(name)
    x, _ = golden(name, 6)
    if name in ds.MODELS:
        x = np.concatenate([x, ds.states(name, 48)])
    x = np.ascontiguousarray(x)
    x.setflags(write=False)
    return m, x


@functools.lru_cache(maxsize=None)
def query(name):
    m, x = states(name)
    return hb.contacts_host(m, x)


def qd_of_step(m, y):
    return y[:, m.dof_q:m.dof_q + m.dof_qd]


def solve_pgs(A, b, nc, mu, iterations):
    """mb_constraint_solver.hpp:101-142 with the bounds of :417-436: normal rows in [0, 1e5], friction rows within
    +- mu max(p_normal, 0) of their point's normal row"""
    nr = 3 * nc
    p = np.zeros(nr)
    for _ in range(iterations):
        for i in range(nr):
            delta = A[i, :i] @ p[:i] + A[i, i + 1:] @ p[i + 1:]
            v = (b[i] - delta) / A[i, i]
            if i < nc:
                v = min(max(v, 0.0), 1e5)
            else:
                s = max(p[i % nc], 0.0)
                v = min(max(v, -mu * s), mu * s)
            p[i] = v
    return p


# ---------------------------------------------------------------- against the reference
@needs_ref
@pytest.mark.parametrize("name", PLANE)
def test_contacts_links_and_jacobians_match_reference(name, built):
    m, x = states(name)
    d = query(name)
    lay = hb.contact_layout(m)
    r = make_ref(name)
    try:
        for e in range(x.shape[0]):
            dbg = r.debug(x[e], m)
            assert dbg["contacts"].shape == (lay["n_c"], 10)
            np.testing.assert_array_equal(dbg["links"], lay["link"])
            assert rel(d["contacts"][e], dbg["contacts"]) <= 1e-9
            assert rel(d["jac"][e], dbg["jac"]) <= 1e-9
    finally:
        r.close()


@needs_ref
@pytest.mark.parametrize("name", PLANE)
def test_penetrating_count_is_the_references(name, built):
    """for every state, none left out; the states spread over the counts the model can have"""
    m, x = states(name)
    counts = ds.contact_counts(name, m, x)
    np.testing.assert_array_equal((query(name)["contacts"][:, :, 9] < 0).sum(axis=1), counts)
    if name in ds.MODELS and name != "cartpole_plane":  # (whose boxes lie in the plane at every state)
        assert counts.min() == 0 and counts.max() >= ds.MAX_CONTACTS[name] - 1 and len(set(counts)) >= 4


@needs_ref
@pytest.mark.parametrize("name", SUPPORTED)
def test_qd_post_is_the_reference_steps(name, built):
    m, x = states(name)
    r = make_ref(name)
    try:
        y_ref = r.step(x)
    finally:
        r.close()
    d = hb.contacts_host(m, x, want=("qd_post",))
    err = rel(d["qd_post"], qd_of_step(m, y_ref))
    print(f"{name}: qd_post host vs reference step max rel = {err:.3e}")
    assert err <= 1e-10


@needs_ref
@pytest.mark.parametrize("name", SUPPORTED)
def test_qd_pre_is_qd_plus_dt_times_the_references_qdd(name, built):
    """RefSim.debug takes tau = 0 on locomotion models (max_force = 0 gives that) and the record's action slots on
    torque models"""
    m, x = states(name)
    x = x.copy()
    if m.step_mode == tds_amd.TDS_STEP_LOCOMOTION:
        x[:, m.dof_q + m.dof_qd + m.action_dim + 2] = 0.0
    qd_pre = hb.contacts_host(m, x, want=("qd_pre",))["qd_pre"]
    r = make_ref(name)
    try:
        want = np.stack([x[e, m.dof_q:m.dof_q + m.dof_qd] + m.dt * r.debug(x[e], m)["qdd"] for e in range(x.shape[0])])
    finally:
        r.close()
    err = rel(qd_pre, want)
    print(f"{name}: qd_pre host vs reference max rel = {err:.3e}")
    assert err <= 1e-10


@needs_ref
@pytest.mark.parametrize("name", PLANE)
def test_momentum_identities_against_reference(name, built):
    m, x = states(name)
    d = query(name)
    r = make_ref(name)
    try:
        qd_post_ref = qd_of_step(m, r.step(x))
        M = np.stack([r.debug(x[e], m)["M"] for e in range(x.shape[0])])
    finally:
        r.close()
    lhs = np.einsum("eij,ej->ei", M, d["qd_pre"] - qd_post_ref)
    by_rows = np.einsum("erd,er->ed", d["rows"], d["impulse"])
    by_force = np.einsum("ecki,eck->ei", d["jac"], d["force"]) * m.dt
    e1, e2 = rel(by_rows, lhs), rel(by_force, -lhs)
    print(f"{name}: M_ref (qd_pre - qd_post_ref) vs rows^T impulse {e1:.3e}, vs -sum jac^T force dt {e2:.3e} "
          f"(bound {MOMENTUM_BOUND:.1e})")
    assert max(e1, e2) <= MOMENTUM_BOUND <= 1e-8
    assert np.abs(d["impulse"]).max() > 0


# ---------------------------------------------------------------- without the reference
@pytest.mark.parametrize("name", SUPPORTED)
def test_qd_post_is_the_double_steps(name, built):
    m, x = states(name)
    d = hb.contacts_host(m, x, want=("qd_post",))
    assert rel(d["qd_post"], qd_of_step(m, hb.step_host(m, x))) <= 1e-10
    _, y = golden(name, 6)
    assert rel(d["qd_post"][:6], qd_of_step(m, y)) <= 1e-10


@pytest.mark.parametrize("name", PLANE)
def test_delassus_is_rows_minv_rowsT_plus_cfm(name, built):
    m, x = states(name)
    d = query(name)
    M = hb.dynamics_host(m, x[:, :m.dof_q], want=("mass_matrix",))["mass_matrix"]
    nr = d["rows"].shape[1]
    A = np.stack([d["rows"][e] @ np.linalg.solve(M[e], d["rows"][e].T) for e in range(x.shape[0])]) + m.cfm * np.eye(nr)
    err = rel(d["delassus"], A)
    print(f"{name}: delassus vs rows M^-1 rows^T + cfm 1 max rel = {err:.3e} (bound {DELASSUS_BOUND:.1e})")
    assert err <= DELASSUS_BOUND <= 1e-8
    np.testing.assert_array_equal(d["delassus"], d["delassus"].transpose(0, 2, 1))


@pytest.mark.parametrize("name", PLANE)
def test_impulse_is_solve_pgs_on_the_returned_system(name, built):
    m, x = states(name)
    d = query(name)
    nc = d["contacts"].shape[1]
    p = np.stack([solve_pgs(d["delassus"][e], d["rhs"][e], nc, m.friction, m.pgs_iterations) for e in range(x.shape[0])])
    err = rel(d["impulse"], p)
    print(f"{name}: impulse vs numpy solve_pgs max rel = {err:.3e} (bound {PGS_BOUND:.1e})")
    assert err <= PGS_BOUND <= 1e-8


@pytest.mark.parametrize("name", PLANE)
def test_bounds_separated_points_and_geometry(name, built):
    m, x = states(name)
    d = query(name)
    lay = hb.contact_layout(m)
    nc = lay["n_c"]
    assert nc > 0 and d["contacts"].shape == (x.shape[0], nc, 10)
    pn, pf1, pf2 = d["impulse"][:, :nc], d["impulse"][:, nc:2 * nc], d["impulse"][:, 2 * nc:]
    assert np.all(pn >= 0) and np.all(pn <= 1e5)
    for pf in (pf1, pf2):
        assert np.all(np.abs(pf) <= m.friction * np.maximum(pn, 0.0))
    sep = d["contacts"][:, :, 9] >= 0
    assert sep.any() and (~sep).any()
    sep3 = np.concatenate([sep, sep, sep], axis=1)
    assert np.all(d["rows"][sep3] == 0) and np.all(d["rhs"][sep3] == 0) and np.all(d["impulse"][sep3] == 0)
    assert np.all(d["force"][sep] == 0)
    assert np.all(np.diagonal(d["delassus"], axis1=1, axis2=2)[sep3] == m.cfm)
    # point_on_a - point_on_b = distance normal; the normal is the layout's, the plane's turned round
    c = d["contacts"]
    assert rel(c[:, :, 6:9] - c[:, :, 3:6], c[:, :, 9:10] * c[:, :, 0:3]) <= 1e-12
    np.testing.assert_array_equal(c[:, :, 0:3], np.broadcast_to(lay["normal"], c[:, :, 0:3].shape))
    np.testing.assert_array_equal(lay["normal"], -np.array(m.plane_normal[:]))
    # rows are the Jacobians along the layout's directions, the force is the impulses along them
    for k, t in enumerate(("normal", "t1", "t2")):
        want = np.einsum("ecki,k->eci", d["jac"], lay[t]) * ~sep[:, :, None]
        assert rel(d["rows"][:, k * nc:(k + 1) * nc], want) <= 1e-12
    f = -(pn[..., None] * lay["normal"] + pf1[..., None] * lay["t1"] + pf2[..., None] * lay["t2"]) / m.dt
    assert rel(d["force"], f) <= 1e-12
    assert [int(g) for g in lay["geom"]] == sorted(int(g) for g in lay["geom"])
    assert all(m.geoms[int(g)].link == int(li) for g, li in zip(lay["geom"], lay["link"]))


@pytest.mark.parametrize("setting", [{"pgs_iterations": 3}, {"friction": 0.5}, {"restitution": 0.3}])
@pytest.mark.parametrize("name", ["ant", "laikago", "pendulum5_plane", "cube_floating"])
def test_solver_settings_on_model_copies(name, setting, built):
    _, x = states(name)
    m = tds_amd.load_model(name)
    for k, v in setting.items():
        setattr(m, k, v)
    d = hb.contacts_host(m, x, want=("qd_post", "impulse"))
    assert rel(d["qd_post"], qd_of_step(m, hb.step_host(m, x))) <= 1e-10
    assert not np.array_equal(d["impulse"], query(name)["impulse"])


def test_want_subsets_leave_the_other_buffers_untouched(built):
    m, x = states("ant")
    full = query("ant")
    shapes = hb.contact_shapes(m, x.shape[0])
    for want in [("force",), ("contacts", "jac"), ("qd_pre",), ("rows", "rhs"), ("delassus",), ("impulse", "qd_post")]:
        out = {k: np.full(shapes[k], 7.25) for k in hb.CONTACT_OUTPUTS}
        o = hb.ContactOut(**{k: out[k].ctypes.data for k in want})
        assert hb.lib().tds_hip_contacts_host(m, x.shape[0], x.ctypes.data, o) == 0
        for k in hb.CONTACT_OUTPUTS:
            np.testing.assert_array_equal(out[k], full[k] if k in want else np.full(shapes[k], 7.25))
    res = hb.contacts_host(m, x, want="force")
    assert list(res) == ["force"]
    with pytest.raises(ValueError):
        hb.contacts_host(m, x, want=("forces",))
    assert hb.lib().tds_hip_contacts_host(m, 1, x.ctypes.data, hb.ContactOut()) == 1  # no output: TDS_ERR_INVALID_ARG


@pytest.mark.parametrize("name", NO_PLANE)
def test_models_without_a_plane_have_no_contact_points(name, built):
    m, x = states(name)
    assert hb.contact_layout(m)["n_c"] == 0
    d = hb.contacts_host(m, x)
    for k in ("contacts", "jac", "rows", "rhs", "delassus", "impulse", "force"):
        assert d[k].size == 0
    assert rel(d["qd_post"], qd_of_step(m, hb.step_host(m, x))) <= 1e-10
    np.testing.assert_array_equal(d["qd_post"], d["qd_pre"])
    assert hb.contacts_host(m, x, want=("force",))["force"].shape == (x.shape[0], 0, 3)


@pytest.mark.parametrize("name", REFUSED)
def test_models_out_of_scope_are_refused(name, built):
    """the refusals (and messages) of tds_hip_jacobian"""
    m = tds_amd.load_model(name)
    x = np.zeros((1, m.input_dim))
    with pytest.raises(hb.TdsHipError, match="error 2: step Jacobians: .* not supported"):
        hb.contact_layout(m)
    with pytest.raises(hb.TdsHipError, match="error 2: step Jacobians: .* not supported"):
        hb.contacts_host(m, x)
    q = np.zeros(m.dof_qd)
    o = hb.ContactOut(qd_post=q.ctypes.data)
    assert hb.lib().tds_hip_contacts_host(m, 1, x.ctypes.data, o) == 2
    assert "not supported" in hb.lib().tds_hip_last_error().decode()


def test_singular_mass_matrix_gives_nan_and_an_error(built):
    """a massless chain: M is not positive definite.  contacts and jac stay valid, rows .. qd_post are NaN for that
    call, and the call returns TDS_ERR_INVALID_ARG after writing everything"""
    m, x = states("pendulum5_plane")
    good = query("pendulum5_plane")
    m = tds_amd.load_model("pendulum5_plane")
    for i in range(m.num_links):
        m.links[i].mass = 0.0
        for k in range(9):
            m.links[i].inertia[k] = 0.0
    shapes = hb.contact_shapes(m, x.shape[0])
    out = {k: np.zeros(shapes[k]) for k in hb.CONTACT_OUTPUTS}
    with pytest.raises(hb.TdsHipError, match="error 1: contact query: joint-space inertia not positive definite"):
        hb.contacts_host(m, x, out=out)
    np.testing.assert_array_equal(out["contacts"], good["contacts"])
    np.testing.assert_array_equal(out["jac"], good["jac"])
    for k in ("rows", "rhs", "delassus", "impulse", "force", "qd_pre", "qd_post"):
        assert np.all(np.isnan(out[k])), k
