"""CPU: the articulated trajectories' host instantiation (tds_hip_trajectory_jvp_host) — one step against the parameter
JVP, the primal against chained steps, js against the chain rule of the per-step [x | theta] Jacobians, the states and
columns against the reference, linearity, errors, refusals and NaN records."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

import tds_amd
from tds_amd import hip_backend as hb

sys.path.insert(0, os.path.join(ROOT, "oracle"))
import reflib  # noqa: E402  (checker only)
import diff_states  # noqa: E402
from test_param_derivs_cpu import SUPPORTED, REFUSED, set_param  # noqa: E402

# parameters of every kind the models carry: a link's mass, COM, inertia, X_T, springs, gravity, friction
SEL = {"ant": [("mass", 3), ("com", 5, 2), ("inertia", 4, 0), ("gravity", 2), ("friction",)],
       "laikago": [("mass", 2), ("xt_trans", 3, 1), ("gravity", 0), ("friction",)],
       "pendulum5_plane": [("mass", 2), ("stiffness", 1), ("damping", 3), ("gravity", 2), ("restitution",)],
       "cube_floating": [("base_mass",), ("base_inertia", 1), ("friction",)]}


def golden(name, k=4):
    return np.ascontiguousarray(np.load(os.path.join(ROOT, "tests", "golden", f"{name}.npz"))["x"][:k])


def starts(name, k=4):
    """golden records, and contact-sweep states where diff_states has a recipe for the model"""
    x = golden(name, k)
    if name in diff_states.MODELS:
        x = np.concatenate([x, diff_states.states(name, k, seed=3)])
    return np.ascontiguousarray(x)


def sel_of(name, m):
    return SEL.get(name) or [("mass", min(1, m.num_links - 1)), ("gravity", 2)]


def thetas(m, sel, n, seed):
    base = hb.params_get(m, sel)
    rng = np.random.default_rng(seed)
    return base * (1.0 + 0.02 * rng.uniform(-1, 1, (n, len(sel))))


def rel(a, b):
    return float(np.max(np.abs(a - b)) / max(1.0, np.max(np.abs(b))))


@pytest.mark.parametrize("name", SUPPORTED)
def test_one_step_is_the_parameter_jvp(name, built):
    """both are host code built without FMA: bit for bit"""
    m = tds_amd.load_model(name)
    x = starts(name)
    n, nin, nsd = x.shape[0], m.input_dim, m.dof_q + m.dof_qd
    sel = sel_of(name, m)
    rng = np.random.default_rng(1)
    for params, th in (((), None), (sel, thetas(m, sel, n, 2))):
        p = len(params)
        v = rng.normal(size=(n, 3, nin + p))
        s, js = hb.trajectory_jvp_host(m, x, v, steps=1, params=params, theta=th)
        th_p = th if th is not None else np.zeros((n, 0))
        jv, y = hb.jvp_params_host(m, x, th_p, params, v, want_y=True)
        assert s.shape == (n, 1, nsd) and js.shape == (n, 3, 1, nsd)
        np.testing.assert_array_equal(s[:, 0], y[:, :nsd])
        np.testing.assert_array_equal(js[:, :, 0], jv[:, :, :nsd])


def chained(m, x0, steps, u=None, params=(), theta=None):
    """q | qd of every step of a Python loop of step_host (jvp_params_host where theta is given)"""
    nsd = m.dof_q + m.dof_qd
    x, out = x0.copy(), []
    for t in range(steps):
        if t > 0:
            x[:, :nsd] = out[-1]
            if u is not None:
                x[:, nsd:nsd + u.shape[2]] = u[:, t - 1]
        y = hb.step_host(m, x) if theta is None else hb.jvp_params_host(m, x, theta, params)
        out.append(y[:, :nsd])
    return np.stack(out, axis=1)


@pytest.mark.parametrize("name", SUPPORTED)
def test_primal_is_the_chained_step(name, built):
    m = tds_amd.load_model(name)
    x = starts(name, 3)
    n, steps = x.shape[0], 10
    nsd, n_act, _ = hb.trajectory_dims(m, steps)
    sel = sel_of(name, m)
    th = thetas(m, sel, n, 4)
    u = np.random.default_rng(5).uniform(-0.3, 0.3, (n, steps - 1, n_act))
    for uu in (None, u):
        s, _ = hb.trajectory_jvp_host(m, x, steps=steps, u=uu)
        np.testing.assert_array_equal(s, chained(m, x, steps, uu))
        s_th, _ = hb.trajectory_jvp_host(m, x, steps=steps, u=uu, params=sel, theta=th)
        np.testing.assert_array_equal(s_th, chained(m, x, steps, uu, sel, th))
        s2, js = hb.trajectory_jvp_host(m, x, np.ones((n, 2, m.input_dim + len(sel))), steps=steps, every=2, u=uu,
                                        params=sel, theta=th)
        np.testing.assert_array_equal(s2, s_th[:, 1::2])
        assert np.all(np.isfinite(js))


@pytest.mark.parametrize("name", ["ant", "laikago", "pendulum5_plane", "cube_floating"])
def test_chain_rule_of_the_step_jacobians(name, built):
    """js over T = 12 steps = the product of the per-step [x | theta] Jacobians along the trajectory (numpy)"""
    m = tds_amd.load_model(name)
    x0 = starts(name, 3)
    n, nin, T = x0.shape[0], m.input_dim, 12
    nsd, n_act, _ = hb.trajectory_dims(m, T)
    sel = SEL[name]
    p = len(sel)
    th = thetas(m, sel, n, 6)
    rng = np.random.default_rng(7)
    v = rng.normal(size=(n, 4, nin + p))
    for u in (None, rng.uniform(-0.2, 0.2, (n, T - 1, n_act))):
        s, js = hb.trajectory_jvp_host(m, x0, v, steps=T, u=u, params=sel, theta=th)
        eye = np.broadcast_to(np.eye(nin + p), (n, nin + p, nin + p))
        D = np.array(eye[:, :nin])  # d x_t / d [x0 | theta], [n, nin, nin + p]
        x = x0.copy()
        ref = []
        for t in range(T):
            if t > 0:
                x[:, :nsd] = s[:, t - 1]
                if u is not None:
                    x[:, nsd:nsd + n_act] = u[:, t - 1]
                    D[:, nsd:nsd + n_act] = 0.0
            J = hb.jvp_params_host(m, x, th, sel, np.ascontiguousarray(eye))[:, :, :nsd].transpose(0, 2, 1)
            S = np.einsum("nij,njk->nik", J[:, :, :nin], D) + np.concatenate(
                [np.zeros((n, nsd, nin)), J[:, :, nin:]], axis=2)
            D[:, :nsd] = S
            ref.append(np.einsum("nik,ndk->ndi", S, v))
        ref = np.stack(ref, axis=2)  # [n, k, T, nsd]
        for e in range(n):
            assert rel(js[e], ref[e]) <= 1e-12, (name, e, rel(js[e], ref[e]))
        assert np.count_nonzero(js[:, :, :, :]) > 0


needs_ref = pytest.mark.skipif(not reflib.available(), reason="the reference library is not built here")


def ref_loop(r, x0, steps, nsd):
    x, out = x0.copy(), []
    for t in range(steps):
        if t > 0:
            x[:, :nsd] = out[-1]
        out.append(r.step(x)[:, :nsd])
    return np.stack(out, axis=1)


def make_ref(name):
    import gen_golden  # noqa: E402  (checker only: the table of reference constructors)

    return gen_golden.make_ref(name)[0]


@needs_ref
@pytest.mark.parametrize("name", ["ant", "laikago", "pendulum5_plane", "pendulum5", "cartpole"])
def test_states_match_the_reference_loop(name, built):
    m = tds_amd.load_model(name)
    x = golden(name, 4)
    T = 20
    r = make_ref(name)
    try:
        s_ref = ref_loop(r, x, T, m.dof_q + m.dof_qd)
    finally:
        r.close()
    s, _ = hb.trajectory_jvp_host(m, x, steps=T)
    assert rel(s, s_ref) <= 1e-9, rel(s, s_ref)


@needs_ref
@pytest.mark.parametrize("name", ["pendulum5_plane", "ant"])
def test_columns_match_central_differences_of_the_reference(name, built):
    """x0's q | qd columns and gravity / friction / restitution against central differences of the reference's loop,
    on entries whose one-sided differences agree (diff_states' kink filter)"""
    m = tds_amd.load_model(name)
    x = golden(name, 3)
    n, nin, nsd, T = x.shape[0], m.input_dim, m.dof_q + m.dof_qd, 8
    g = list(m.gravity)
    kinds = [("gravity", 2), ("friction",), ("restitution",)]
    setters = [lambda r, v: r.set_gravity([g[0], g[1], v]),
               lambda r, v: r.set_solver(m.cfm, m.erp, m.pgs_iterations, v, m.restitution),
               lambda r, v: r.set_solver(m.cfm, m.erp, m.pgs_iterations, m.friction, v)]
    cols = list(range(0, nsd, 3))
    v = np.zeros((n, len(cols) + len(kinds), nin + len(kinds)))
    v[:, np.arange(len(cols)), cols] = 1.0
    v[:, len(cols) + np.arange(len(kinds)), nin + np.arange(len(kinds))] = 1.0
    _, js = hb.trajectory_jvp_host(m, x, v, steps=T, params=kinds)
    js = js.reshape(n, v.shape[1], -1)
    r = make_ref(name)
    checked = 0
    try:
        def loop(z):
            return ref_loop(r, z, T, nsd).reshape(z.shape[0], -1)

        J, kink = diff_states.central_jacobian(m, x, cols=np.array(cols), step=loop)
        for e in range(n):
            if not kink[e]:
                scale = max(1.0, np.max(np.abs(js[e, :len(cols)])))
                assert np.max(np.abs(js[e, :len(cols)].T - J[e])) / scale <= 1e-6, (name, e)
                checked += len(cols)
        theta = [g[2], m.friction, m.restitution]
        for j, (setter, val) in enumerate(zip(setters, theta)):
            h = 1e-6 * max(1.0, abs(val))
            ys = []
            for s_ in (1, -1, 2, -2, 0):
                setter(r, val + s_ * h)
                ys.append(loop(x)[:, None])
            setter(r, val)
            Jt, kt = diff_states._central_and_kink(ys[4], ys[0], ys[1], ys[2], ys[3], h, 1e-5)
            for e in np.flatnonzero(~kt):
                col = js[e, len(cols) + j]
                assert np.max(np.abs(col - Jt[e][:, 0])) / max(1.0, np.max(np.abs(col))) <= 1e-6, (name, kinds[j], e)
                checked += 1
    finally:
        r.close()
    assert checked >= 4, checked


def test_linearity_in_v(built):
    m = tds_amd.load_model("ant")
    x = starts("ant", 2)
    n, sel = x.shape[0], SEL["ant"]
    rng = np.random.default_rng(8)
    v1, v2 = rng.normal(size=(2, n, m.input_dim + len(sel)))
    th = thetas(m, sel, n, 9)
    _, j1 = hb.trajectory_jvp_host(m, x, v1, steps=6, params=sel, theta=th)
    _, j2 = hb.trajectory_jvp_host(m, x, v2, steps=6, params=sel, theta=th)
    _, j12 = hb.trajectory_jvp_host(m, x, 2.0 * v1 - 0.5 * v2, steps=6, params=sel, theta=th)
    assert rel(j12, 2.0 * j1 - 0.5 * j2) <= 1e-12


def test_invalid_steps_every_and_selection(built):
    m = tds_amd.load_model("pendulum5")
    x = golden("pendulum5", 1)
    for steps, every in ((0, 1), (-2, 1), (6, 4), (6, 0), (6, -3)):
        with pytest.raises(hb.TdsHipError, match="tds_hip error 1:"):
            hb.trajectory_jvp_host(m, x, steps=steps, every=every)
    for sel in ([("mass", 9)], [("base_mass",)], [("mass", 1), ("mass", 1)]):
        with pytest.raises(hb.TdsHipError, match="tds_hip error 1:"):
            hb.trajectory_jvp_host(m, x, steps=2, params=sel, theta=np.ones(len(sel)))


@pytest.mark.parametrize("name", REFUSED)
def test_refused_models_give_the_jacobians_message(name, built):
    m = tds_amd.load_model(name)
    x = np.zeros((1, m.input_dim))
    with pytest.raises(hb.TdsHipError) as e_jac:
        hb.jacobian_host(m, x)
    with pytest.raises(hb.TdsHipError, match="not supported") as e:
        hb.trajectory_jvp_host(m, x, steps=3)
    assert str(e.value) == str(e_jac.value)


def test_not_positive_definite_from_some_step_gives_nan_records_from_that_step(built):
    """the base link's mass negative: M is factored where contacts are active, and is not positive definite once the
    pendulum reaches the plane (environment 1 only)"""
    name = "pendulum5_plane"
    m = tds_amd.load_model(name)
    x = np.ascontiguousarray(np.repeat(np.load(os.path.join(ROOT, "tests", "golden", f"{name}.npz"))["x"][5:6], 2, 0))
    sel = [("mass", 0)]
    T = 12
    theta = np.array([[m.links[0].mass], [-0.1 * m.links[0].mass]])
    # where the first NaN record lies: the step whose inertia is not positive definite
    s_ok = chained(m, x[:1], T, None, sel, theta[:1])
    first = None
    xx = x[1:2].copy()
    for t in range(T):
        if t > 0:
            xx[:, :m.dof_q + m.dof_qd] = y[:, :m.dof_q + m.dof_qd]
        try:
            y = hb.jvp_params_host(m, xx, theta[1:], sel)
        except hb.TdsHipError:
            first = t
            break
    assert first is not None and first > 0
    nsd, nin = m.dof_q + m.dof_qd, m.input_dim
    s = np.zeros((2, T, nsd))
    js = np.zeros((2, 1, T, nsd))
    v = np.ones((2, 1, nin + 1))
    rc = hb.lib().tds_hip_trajectory_jvp_host(C.byref(m), 2, T, 1, x.ctypes.data, None, 1, hb.param_spec(sel),
                                              np.ascontiguousarray(theta).ctypes.data, 1, v.ctypes.data,
                                              s.ctypes.data, js.ctypes.data)
    assert rc == 1  # TDS_ERR_INVALID_ARG
    np.testing.assert_array_equal(s[0], s_ok[0])
    assert np.all(np.isfinite(js[0]))
    assert np.all(np.isfinite(s[1, :first])) and np.all(np.isfinite(js[1, :, :first]))
    assert np.all(np.isnan(s[1, first:])) and np.all(np.isnan(js[1, :, first:]))
