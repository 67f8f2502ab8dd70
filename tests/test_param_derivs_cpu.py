"""CPU: the parameter derivatives' host instantiations (tds_hip_jvp_params_host, tds_hip_vjp_params_host) — at the
blob's values against the plain derivatives, J_theta against central differences of the double step, of the C oracle
and of the reference on perturbed models, per-environment theta, and what is refused."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

import tds_amd
from tds_amd import hip_backend as hb

sys.path.insert(0, os.path.join(ROOT, "oracle"))
import oraclelib  # noqa: E402  (checker only)
import reflib  # noqa: E402  (checker only)

SUPPORTED = ["ant", "ant_floating", "laikago", "laikago_floating", "laikago_floating_env", "laikago_soft",
             "cartpole", "cartpole_plane", "pendulum5", "pendulum5_plane", "cube_floating"]
REFUSED = ["humanoid", "humanoid_spherical", "pendulum5_spherical", "two_cubes_floating", "pendulum_and_cube"]
INERTIA_IDX = [(0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)]


def golden(name, k=6):
    return np.load(os.path.join(ROOT, "tests", "golden", f"{name}.npz"))["x"][:k]


def set_param(m, q, value):
    """a copy of model m with the selected scalar q (a param_spec tuple) set to value"""
    m = m.copy()
    name = q[0]
    code, on_link, nc = hb.PARAM_KINDS[name]
    rest = list(q[1:])
    link = rest.pop(0) if on_link else 0
    comp = rest.pop(0) if rest else 0
    l = m.links[link]
    if name in ("mass", "stiffness", "damping"):
        setattr(l, name, value)
    elif name == "com":
        l.com[comp] = value
    elif name == "xt_trans":
        l.X_T_trans[comp] = value
    elif name in ("inertia", "base_inertia"):
        r, c = INERTIA_IDX[comp]
        arr = l.inertia if name == "inertia" else m.base_inertia
        arr[3 * r + c] = value
        arr[3 * c + r] = value
    elif name == "base_mass":
        m.base_mass = value
    elif name == "base_com":
        m.base_com[comp] = value
    elif name == "gravity":
        m.gravity[comp] = value
    else:
        setattr(m, name, value)
    return m


def j_theta(m, x, sel):
    """J_theta [N, output_dim, p] at the blob's values, by forward mode over unit theta directions"""
    n, nin, p = x.shape[0], m.input_dim, len(sel)
    v = np.zeros((n, p, nin + p))
    v[:, np.arange(p), nin + np.arange(p)] = 1.0
    return hb.jvp_params_host(m, x, hb.params_get(m, sel), sel, v).transpose(0, 2, 1)


def central_diff_theta(step, m, x, sel, h_rel=1e-6):
    """central differences of step(model, x) [N, output_dim] over each selected scalar, and a flag per environment
    and scalar: the two one-sided differences agree (no branch switches within +- h)"""
    theta = hb.params_get(m, sel)
    y0 = step(m, x)
    J = np.zeros((x.shape[0], y0.shape[1], len(sel)))
    smooth = np.ones((x.shape[0], len(sel)), dtype=bool)
    for j, q in enumerate(sel):
        h = h_rel * max(1.0, abs(theta[j]))
        yp, ym = step(set_param(m, q, theta[j] + h), x), step(set_param(m, q, theta[j] - h), x)
        J[:, :, j] = (yp - ym) / (2 * h)
        fwd, bwd = (yp - y0) / h, (y0 - ym) / h
        scale = np.maximum(1.0, np.max(np.abs(J[:, :, j]), axis=1))
        smooth[:, j] = np.max(np.abs(fwd - bwd), axis=1) / scale <= 1e-3
    return J, smooth


def rel(a, b):
    return float(np.max(np.abs(a - b)) / max(1.0, np.max(np.abs(b))))


@pytest.mark.parametrize("name", SUPPORTED)
def test_at_blob_values_equal_the_plain_derivatives(name, built):
    """theta = the blob's values of every selectable parameter: y and the x columns are those of vjp_host and
    jacobian_host, bit for bit"""
    m = tds_amd.load_model(name)
    x = golden(name, 3)
    sel = hb.all_params(m)
    theta = hb.params_get(m, sel)
    nin, p = m.input_dim, len(sel)
    w = np.random.default_rng(2).normal(size=(3, 2, m.output_dim))
    wj, y = hb.vjp_params_host(m, x, theta, sel, w, want_y=True)
    wj0, y0 = hb.vjp_host(m, x, w, want_y=True)
    assert wj.shape == (3, 2, nin + p)
    np.testing.assert_array_equal(y, y0)
    np.testing.assert_array_equal(wj[:, :, :nin], wj0)
    v = np.zeros((3, nin, nin + p))
    v[:, :, :nin] = np.eye(nin)
    jv, yj = hb.jvp_params_host(m, x, theta, sel, v, want_y=True)
    jac, yj0 = hb.jacobian_host(m, x, want_y=True)
    np.testing.assert_array_equal(yj, yj0)
    np.testing.assert_array_equal(jv.transpose(0, 2, 1), jac)
    np.testing.assert_array_equal(hb.jvp_params_host(m, x, theta, sel), yj0)


@pytest.mark.parametrize("name", SUPPORTED)
def test_theta_adjoints_are_w_times_j_theta_and_match_central_differences(name, built):
    m = tds_amd.load_model(name)
    x = golden(name, 4)
    sel = hb.all_params(m)
    nin = m.input_dim
    J = j_theta(m, x, sel)
    w = np.random.default_rng(3).normal(size=(x.shape[0], 2, m.output_dim))
    wj = hb.vjp_params_host(m, x, hb.params_get(m, sel), sel, w)
    assert rel(wj[:, :, nin:], np.einsum("nko,nop->nkp", w, J)) <= 1e-11
    assert np.count_nonzero(wj[:, :, nin:]) > 0
    J_fd, smooth = central_diff_theta(hb.step_host, m, x, sel)
    checked = 0
    for e in range(x.shape[0]):
        cols = np.flatnonzero(smooth[e])
        scale = max(1.0, np.max(np.abs(J[e][:, cols])))
        assert np.max(np.abs(J[e][:, cols] - J_fd[e][:, cols])) / scale <= 1e-6, name
        checked += cols.size
    assert checked >= len(sel), (checked, len(sel))


# mass, COM, inertia, X_T translation and the base's inertia against the plain-C restatement of the step
ORACLE_CASES = {
    "ant": [("mass", 0), ("mass", 5), ("com", 3, 0), ("inertia", 2, 0), ("inertia", 4, 3), ("xt_trans", 1, 0),
            ("xt_trans", 6, 2)],
    "pendulum5_plane": [("mass", 2), ("com", 4, 1), ("inertia", 3, 2), ("inertia", 1, 5), ("xt_trans", 2, 1)],
    "ant_floating": [("base_mass",), ("base_com", 2), ("base_inertia", 0), ("base_inertia", 4), ("mass", 3),
                     ("xt_trans", 2, 1)],
    "cube_floating": [("base_mass",), ("base_com", 0), ("base_inertia", 1), ("base_inertia", 3)],
}


@pytest.mark.parametrize("name", list(ORACLE_CASES))
def test_j_theta_matches_central_differences_of_the_oracle(name, built):
    m = tds_amd.load_model(name)
    x = golden(name, 4)
    sel = ORACLE_CASES[name]
    J = j_theta(m, x, sel)
    J_fd, smooth = central_diff_theta(lambda mm, xx: oraclelib.step(mm, xx), m, x, sel)
    checked = 0
    for e in range(x.shape[0]):
        cols = np.flatnonzero(smooth[e])
        if cols.size:
            assert np.max(np.abs(J[e][:, cols] - J_fd[e][:, cols])) / max(1.0, np.max(np.abs(J[e]))) <= 1e-5
            checked += cols.size
    assert checked >= len(sel)
    assert np.count_nonzero(J) > 0


needs_ref = pytest.mark.skipif(not reflib.available(), reason="the reference library is not built here")


def ref_diff(name, x, setter, value, h):
    """central difference of the reference's step over a setting applied by setter(r, value)"""
    import gen_golden  # noqa: E402  (checker only: the table of reference constructors)

    out = []
    for v in (value + h, value - h):
        r, _ = gen_golden.make_ref(name)
        try:
            setter(r, v)
            out.append(r.step(x))
        finally:
            r.close()
    return (out[0] - out[1]) / (2 * h)


@needs_ref
@pytest.mark.parametrize("name", ["pendulum5_plane", "ant"])
def test_gravity_friction_restitution_match_the_reference(name, built):
    m = tds_amd.load_model(name)
    x = golden(name, 4)
    sel = [("gravity", 0), ("gravity", 2), ("friction",), ("restitution",)]
    J = j_theta(m, x, sel)
    _, smooth = central_diff_theta(hb.step_host, m, x, sel)
    g = list(m.gravity)

    def set_g(k):
        return lambda r, v: r.set_gravity([v if i == k else g[i] for i in range(3)])

    setters = [set_g(0), set_g(2),
               lambda r, v: r.set_solver(m.cfm, m.erp, m.pgs_iterations, v, m.restitution),
               lambda r, v: r.set_solver(m.cfm, m.erp, m.pgs_iterations, m.friction, v)]
    values = [g[0], g[2], m.friction, m.restitution]
    for j, (setter, val) in enumerate(zip(setters, values)):
        h = 1e-6 * max(1.0, abs(val))
        fd = ref_diff(name, x, setter, val, h)
        envs = np.flatnonzero(smooth[:, j])
        assert envs.size >= 1, sel[j]  # every parameter is compared on at least one environment
        for e in envs:
            assert np.max(np.abs(J[e][:, j] - fd[e])) / max(1.0, np.max(np.abs(J[e][:, j]))) <= 1e-5, sel[j]
    assert np.count_nonzero(J[:, :, 2:]) > 0  # friction and restitution act through the golden states' contacts


@needs_ref
def test_springs_match_the_reference(built):
    name = "pendulum5"
    m = tds_amd.load_model(name)
    x = golden(name, 3)
    sel = [("stiffness", 1), ("damping", 1), ("stiffness", 4), ("damping", 3)]
    J = j_theta(m, x, sel)
    for j, q in enumerate(sel):
        link = q[1]
        k0, d0 = m.links[link].stiffness, m.links[link].damping
        h = 1e-6
        if q[0] == "stiffness":
            fd = ref_diff(name, x, lambda r, v: r.set_link_spring(link, v, d0), k0, h)
        else:
            fd = ref_diff(name, x, lambda r, v: r.set_link_spring(link, k0, v), d0, h)
        assert np.max(np.abs(J[:, :, j] - fd)) / max(1.0, np.max(np.abs(J[:, :, j]))) <= 1e-5, q
        assert np.count_nonzero(J[:, :, j]) > 0


@pytest.mark.parametrize("name", ["ant", "ant_floating", "laikago", "pendulum5_plane", "cube_floating"])
def test_per_environment_theta_is_the_step_of_that_model(name, built):
    m = tds_amd.load_model(name)
    x = golden(name, 5)
    sel = hb.all_params(m)
    base = hb.params_get(m, sel)
    rng = np.random.default_rng(4)
    shape = (x.shape[0], len(sel))
    additive = np.array([not q[0].endswith("inertia") for q in sel])  # (zero inertia products stay zero: M stays SPD)
    theta = base * (1.0 + 0.05 * rng.uniform(-1, 1, shape)) + 0.01 * rng.uniform(-1, 1, shape) * additive
    y = hb.jvp_params_host(m, x, theta, sel)
    _, y_rev = hb.vjp_params_host(m, x, theta, sel, np.zeros((x.shape[0], m.output_dim)), want_y=True)
    for e in range(x.shape[0]):
        me = m
        for j, q in enumerate(sel):
            me = set_param(me, q, theta[e, j])
        y_e = hb.step_host(me, x[e:e + 1])[0]
        np.testing.assert_array_equal(y[e], y_e)
        assert rel(y_rev[e], y_e) <= 1e-12
        assert np.max(np.abs(y_e - hb.step_host(m, x[e:e + 1])[0])) > 0  # theta does move the step


def test_param_spec_and_params_get(built):
    m = tds_amd.load_model("ant_floating")
    sel = [("mass", 3), ("com", 3, 2), ("inertia", 2, 4), ("xt_trans", 1, 0), ("stiffness", 0), ("damping", 5),
           ("base_mass",), ("base_com", 1), ("base_inertia", 5), ("gravity", 2), ("friction",), ("restitution",)]
    arr = hb.param_spec(sel)
    assert [(arr[j].kind, arr[j].link, arr[j].comp) for j in range(len(sel))] == [
        (0, 3, 0), (1, 3, 2), (2, 2, 4), (3, 1, 0), (4, 0, 0), (5, 5, 0), (6, 0, 0), (7, 0, 1), (8, 0, 5), (9, 0, 2),
        (10, 0, 0), (11, 0, 0)]
    theta = hb.params_get(m, sel)
    assert list(theta) == [m.links[3].mass, m.links[3].com[2], m.links[2].inertia[2], m.links[1].X_T_trans[0],
                           m.links[0].stiffness, m.links[5].damping, m.base_mass, m.base_com[1], m.base_inertia[5],
                           m.gravity[2], m.friction, m.restitution]
    with pytest.raises(ValueError):
        hb.param_spec([("length", 1)])
    for bad in ([("mass",)], [("com",)], [("mass", 1, 0, 0)]):
        with pytest.raises(ValueError):
            hb.param_spec(bad)


@pytest.mark.parametrize("sel,match", [
    ([hb.Param(12, 0, 0, 0)], "unknown parameter kind"),
    ([hb.Param(-1, 0, 0, 0)], "unknown parameter kind"),
    ([("mass", 14)], "link index out of range"),
    ([("mass", -1)], "link index out of range"),
    ([("com", 2, 3)], "component index out of range"),
    ([("inertia", 2, 6)], "component index out of range"),
    ([("mass", 2, 1)], "component index out of range"),
    ([("gravity", 3)], "component index out of range"),
    ([hb.Param(10, 1, 0, 0)], "link index out of range"),
    ([("mass", 2), ("com", 2, 0), ("mass", 2)], "duplicate parameter"),
    ([("base_mass",)], "floating base"),
    ([("base_inertia", 1)], "floating base"),
])
def test_bad_selections_are_invalid_arguments(sel, match, built):
    m = tds_amd.load_model("ant")  # fixed base, 14 links
    x = golden("ant", 1)
    th = np.zeros(len(sel))
    for call in (lambda: hb.params_get(m, sel),
                 lambda: hb.jvp_params_host(m, x, th, sel),
                 lambda: hb.vjp_params_host(m, x, th, sel, np.zeros((1, m.output_dim)))):
        with pytest.raises(hb.TdsHipError, match=match) as e:
            call()
        assert "tds_hip error 1:" in str(e.value)  # TDS_ERR_INVALID_ARG


@pytest.mark.parametrize("name", REFUSED)
def test_unsupported_models_are_refused_with_the_jacobians_message(name, built):
    m = tds_amd.load_model(name)
    x = np.zeros((1, m.input_dim))
    sel = [("mass", 0)]
    with pytest.raises(hb.TdsHipError) as e_jac:
        hb.jacobian_host(m, x)
    for call in (lambda: hb.jvp_params_host(m, x, [1.0], sel),
                 lambda: hb.vjp_params_host(m, x, [1.0], sel, np.zeros((1, m.output_dim)))):
        with pytest.raises(hb.TdsHipError, match="not supported") as e:
            call()
        assert str(e.value) == str(e_jac.value)


def test_tape_lengths_fit_the_parameter_capacity(built):
    """every golden record of every supported model, every selectable parameter selected: no overflow"""
    for name in SUPPORTED:
        m = tds_amd.load_model(name)
        x = np.load(os.path.join(ROOT, "tests", "golden", f"{name}.npz"))["x"]
        sel = hb.all_params(m)
        _, lens = hb.vjp_params_host(m, x, hb.params_get(m, sel), sel, np.zeros((x.shape[0], m.output_dim)),
                                     tape_len=True)
        assert np.all(lens > 0), name


def test_tape_overflow_is_an_error_with_nan_outputs(built):
    m = tds_amd.load_model("pendulum5_plane")
    x = np.ascontiguousarray(golden("pendulum5_plane", 2))
    sel = hb.all_params(m)
    theta = hb.params_get(m, sel)
    w = np.ones((2, m.output_dim))
    _, lens = hb.vjp_params_host(m, x, theta, sel, w, tape_len=True)
    with pytest.raises(hb.TdsHipError, match="tape exceeds the capacity"):
        hb.vjp_params_host(m, x, theta, sel, w, tape_cap=int(lens.min()) - 1)
    p = len(sel)
    wj = np.zeros((2, m.input_dim + p))
    y = np.zeros((2, m.output_dim))
    th = np.ascontiguousarray(np.broadcast_to(theta, (2, p)))
    rc = hb.lib().tds_hip_vjp_params_host(C.byref(m), 2, x.ctypes.data, p, hb.param_spec(sel), th.ctypes.data, 1,
                                          w.ctypes.data, y.ctypes.data, wj.ctypes.data, int(lens.min()) - 1, None)
    assert rc == 2  # TDS_ERR_UNSUPPORTED
    assert np.all(np.isnan(wj)) and np.all(np.isnan(y))
