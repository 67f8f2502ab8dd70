"""CPU: the trajectory VJP's host instantiation (tds_hip_trajectory_vjp_host) — one step against the parameter VJP,
[gx0 | gtheta] against forward mode, gu against the lambda-recursion over per-step VJPs and against central
differences, zero and linear cotangents, tape lengths, overflowing tapes, NaN environments, errors and refusals."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from conftest import ROOT

import tds_amd
from tds_amd import hip_backend as hb

import diff_states
from test_param_derivs_cpu import REFUSED
from test_traj_derivs_cpu import sel_of

MODELS = ["ant", "laikago", "cube_floating", "pendulum5", "pendulum5_plane", "ant_floating"]
N, T = 6, 12


def rel(a, b):
    return float(np.max(np.abs(a - b)) / max(1.0, np.max(np.abs(b)))) if a.size else 0.0


@functools.lru_cache(maxsize=None)
def case(name, n=N, steps=T):
    """(m, sel, x0, u, theta, gs at every = 1); the arrays are shared between the tests: read only"""
    m = tds_amd.load_model(name)
    if name in diff_states.MODELS or name == "cube_floating":
        x0 = diff_states.states(name, n, 11, m)
    else:
        g = np.load(os.path.join(ROOT, "tests", "golden", f"{name}.npz"))["x"]
        x0 = g[np.random.default_rng(11).integers(0, g.shape[0], n)]
    x0 = np.ascontiguousarray(x0)
    nsd, n_act, _ = hb.trajectory_dims(m, steps)
    u = np.random.default_rng(12).uniform(-0.2, 0.2, (n, steps - 1, n_act))
    sel = sel_of(name, m)
    th = hb.params_get(m, sel) * (1.0 + 0.01 * np.random.default_rng(13).uniform(-1, 1, (n, len(sel))))
    gs = np.random.default_rng(14).normal(size=(n, steps, nsd))
    for a in (x0, u, th, gs):
        a.setflags(write=False)
    return m, sel, x0, u, th, gs


def gs_of(gs, every):
    return np.ascontiguousarray(gs[:, every - 1::every])


@functools.lru_cache(maxsize=None)
def recursion(name):
    """(gx0, gu, gtheta, tape lengths [n, T]) of the explicit lambda-recursion over vjp_params_host, u given, every 1"""
    m, sel, x0, u, th, gs = case(name)
    nsd, n_act, _ = hb.trajectory_dims(m, T)
    nin = m.input_dim
    s, _ = hb.trajectory_jvp_host(m, x0, steps=T, u=u, params=sel, theta=th)
    lam = np.zeros((N, nsd))
    gx0, gu, gth = np.zeros((N, nin)), np.zeros((N, T - 1, n_act)), np.zeros((N, len(sel)))
    lens = np.zeros((N, T), dtype=np.int32)
    for t in range(T - 1, -1, -1):
        x = x0.copy()
        if t > 0:
            x[:, :nsd] = s[:, t - 1]
            x[:, nsd:nsd + n_act] = u[:, t - 1]
        w = np.zeros((N, m.output_dim))
        w[:, :nsd] = lam + gs[:, t]
        wj, lens[:, t] = hb.vjp_params_host(m, x, th, sel, w, tape_len=True)
        lam = wj[:, :nsd]
        if t > 0:
            gu[:, t - 1] = wj[:, nsd:nsd + n_act]
        else:
            gx0[:, :nsd + n_act] = wj[:, :nsd + n_act]
        gx0[:, nsd + n_act:] += wj[:, nsd + n_act:nin]
        gth += wj[:, nin:]
    return gx0, gu, gth, lens


@pytest.mark.parametrize("name", MODELS)
def test_one_step_is_the_parameter_vjp(name, built):
    """both are host code built without FMA, over the same tape: bit for bit"""
    m, sel, x0, _, th, gs = case(name)
    nsd = m.dof_q + m.dof_qd
    g1 = np.ascontiguousarray(gs[:, :1])
    s, gx0, gu, gth = hb.trajectory_vjp_host(m, x0, g1, 1, params=sel, theta=th)
    w = np.zeros((N, m.output_dim))
    w[:, :nsd] = g1[:, 0]
    wj = hb.vjp_params_host(m, x0, th, sel, w)
    np.testing.assert_array_equal(np.concatenate([gx0, gth], axis=1), wj)
    np.testing.assert_array_equal(s, hb.trajectory_jvp_host(m, x0, steps=1, params=sel, theta=th)[0])
    assert gu.shape == (N, 0, hb.trajectory_dims(m, 1)[1]) and np.count_nonzero(wj) > 0


@pytest.mark.parametrize("with_u", [True, False])
@pytest.mark.parametrize("every", [1, 3])
@pytest.mark.parametrize("name", MODELS)
def test_gx0_and_gtheta_match_forward_mode(name, every, with_u, built):
    m, sel, x0, u, th, gs = case(name)
    nall = m.input_dim + len(sel)
    uu = u if with_u else None
    g = gs_of(gs, every)
    s, gx0, _, gth = hb.trajectory_vjp_host(m, x0, g, T, every, uu, sel, th)
    v = np.ascontiguousarray(np.broadcast_to(np.eye(nall), (N, nall, nall)))
    s_f, js = hb.trajectory_jvp_host(m, x0, v, T, every, uu, sel, th)
    np.testing.assert_array_equal(s, s_f)
    assert np.all(np.abs(s) < 1e3)  # no environment is excluded
    ref = np.einsum("nrs,nkrs->nk", g, js)
    got = np.concatenate([gx0, gth], axis=1)
    worst = max(rel(got[e], ref[e]) for e in range(N))
    print(name, every, with_u, "reverse against forward", worst)
    assert worst <= 1e-11, worst
    assert np.count_nonzero(got) > 0


@pytest.mark.parametrize("name", MODELS)
def test_gu_matches_the_lambda_recursion(name, built):
    m, sel, x0, u, th, gs = case(name)
    gx0_r, gu_r, gth_r, lens_r = recursion(name)
    s, gx0, gu, gth, lens = hb.trajectory_vjp_host(m, x0, gs, T, 1, u, sel, th, tape_len=True)
    worst = max(max(rel(a[e], b[e]) for e in range(N)) for a, b in ((gu, gu_r), (gx0, gx0_r), (gth, gth_r)))
    print(name, "against the recursion", worst)
    assert worst <= 1e-11, worst
    assert lens.shape == (N, T) and lens.dtype == np.int32
    np.testing.assert_array_equal(lens, lens_r)
    if gu.size:
        assert np.count_nonzero(gu) > 0


@pytest.mark.parametrize("name", ["ant", "laikago", "pendulum5", "pendulum5_plane", "ant_floating"])
def test_gu_matches_central_differences(name, built):
    m, sel, x0, u, th, gs = case(name)
    n_act = hb.trajectory_dims(m, T)[1]
    _, _, gu, _ = hb.trajectory_vjp_host(m, x0, gs, T, 1, u, sel, th)
    h = 1e-6

    def loss(uu):
        s, _ = hb.trajectory_jvp_host(m, x0, steps=T, u=uu, params=sel, theta=th)
        return np.einsum("nrs,nrs->n", gs, s)

    for t, i in ((0, 0), (T // 2, n_act - 1), (T - 2, n_act // 2)):
        up, um = u.copy(), u.copy()
        up[:, t, i] += h
        um[:, t, i] -= h
        fd = (loss(up) - loss(um)) / (2 * h)
        err = np.abs(fd - gu[:, t, i]) / np.maximum(1.0, np.abs(gu[:, t, i]))
        print(name, (t, i), "central differences", err.max())
        assert err.max() <= 1e-6, (name, t, i, err)


def test_zero_and_linear_cotangents(built):
    m, sel, x0, u, th, gs = case("ant")
    ga, gb = gs_of(gs, 3), np.random.default_rng(15).normal(size=(N, T // 3, gs.shape[2]))
    run = lambda g: hb.trajectory_vjp_host(m, x0, g, T, 3, u, sel, th)[1:]  # noqa: E731
    for out in run(np.zeros_like(ga)):
        assert np.all(out == 0.0)
    for oa, ob, oab in zip(run(ga), run(gb), run(2.0 * ga - 0.5 * gb)):
        assert rel(oab, 2.0 * oa - 0.5 * ob) <= 1e-12


def raw(m, x0, gs, steps, u, sel, th, tape_cap=0):
    """the C call itself: (rc, s, gx0, gu, gtheta, tape lengths)"""
    n, p = x0.shape[0], len(sel)
    nsd, n_act, n_rec = hb.trajectory_dims(m, steps)
    s = np.zeros((n, n_rec, nsd))
    gx0, gu, gth = np.ones((n, m.input_dim)), np.ones((n, steps - 1, n_act)), np.ones((n, p))
    lens = np.zeros((n, steps), dtype=np.int32)
    arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in (x0, u, th, gs)]
    rc = hb.lib().tds_hip_trajectory_vjp_host(C.byref(m), n, steps, 1, arrs[0].ctypes.data, arrs[1].ctypes.data, p,
                                              hb.param_spec(sel), arrs[2].ctypes.data, arrs[3].ctypes.data,
                                              s.ctypes.data, gx0.ctypes.data, gu.ctypes.data, gth.ctypes.data,
                                              int(tape_cap), lens.ctypes.data)
    return rc, s, gx0, gu, gth, lens


def test_a_small_tape_capacity_gives_nan_gradients_for_the_overflowing_environments(built):
    m, sel, x0, u, th, gs = case("ant")
    _, gx0_r, gu_r, gth_r, lens_r = hb.trajectory_vjp_host(m, x0, gs, T, 1, u, sel, th, tape_len=True)
    longest = lens_r.max(axis=1)
    cap = int(np.sort(longest)[N // 2 - 1])
    over = longest > cap
    assert 0 < over.sum() < N, longest
    rc, s, gx0, gu, gth, lens = raw(m, x0, gs, T, u, sel, th, tape_cap=cap)
    assert rc == 2  # TDS_ERR_UNSUPPORTED
    np.testing.assert_array_equal(lens, np.where(lens_r > cap, -1, lens_r))
    for got, ref in ((gx0, gx0_r), (gu, gu_r), (gth, gth_r)):
        assert np.all(np.isnan(got[over]))
        np.testing.assert_array_equal(got[~over], ref[~over])
    assert np.all(np.isfinite(s))
    with pytest.raises(hb.TdsHipError, match="tape exceeds the capacity"):
        hb.trajectory_vjp_host(m, x0, gs, T, 1, u, sel, th, tape_cap=cap)


def test_not_positive_definite_gives_nan_gradients_for_that_environment_only(built):
    """test_traj_derivs_cpu's case: the base link's mass negative in environment 1, whose inertia is not positive
    definite once the pendulum reaches the plane"""
    name = "pendulum5_plane"
    m = tds_amd.load_model(name)
    x = np.ascontiguousarray(np.repeat(np.load(os.path.join(ROOT, "tests", "golden", f"{name}.npz"))["x"][5:6], 2, 0))
    sel = [("mass", 0)]
    theta = np.array([[m.links[0].mass], [-0.1 * m.links[0].mass]])
    nsd, n_act, _ = hb.trajectory_dims(m, T)
    u = np.random.default_rng(16).uniform(-0.2, 0.2, (2, T - 1, n_act))
    gs = np.random.default_rng(17).normal(size=(2, T, nsd))
    rc, s, gx0, gu, gth, _ = raw(m, x, gs, T, u, sel, theta)
    assert rc == 1  # TDS_ERR_INVALID_ARG
    rc1, s1, gx1, gu1, gth1, _ = raw(m, x[:1], gs[:1], T, u[:1], sel, theta[:1])
    assert rc1 == 0
    for got, ref in ((s, s1), (gx0, gx1), (gu, gu1), (gth, gth1)):
        np.testing.assert_array_equal(got[:1], ref)
        assert np.all(np.isfinite(ref))
    assert np.all(np.isnan(gx0[1])) and np.all(np.isnan(gu[1])) and np.all(np.isnan(gth[1]))
    nan_rec = np.isnan(s[1]).all(axis=1)
    first = int(np.argmax(nan_rec))
    assert first > 0 and np.all(nan_rec[first:]) and np.all(np.isfinite(s[1, :first]))


def test_invalid_steps_every_and_selection(built):
    m, sel, x0, u, th, gs = case("pendulum5")
    x = x0[:1]
    for steps, every in ((0, 1), (-2, 1), (6, 4), (6, 0), (6, -3)):
        with pytest.raises(hb.TdsHipError) as e_jvp:
            hb.trajectory_jvp_host(m, x, steps=steps, every=every)
        with pytest.raises(hb.TdsHipError, match="tds_hip error 1:") as e:
            hb.trajectory_vjp_host(m, x, np.zeros((1, 1, gs.shape[2])), steps, every)
        assert str(e.value) == str(e_jvp.value).replace("trajectory_jvp", "trajectory_vjp")
    for bad in ([("mass", 9)], [("base_mass",)], [("mass", 1), ("mass", 1)]):
        with pytest.raises(hb.TdsHipError) as e_jvp:
            hb.trajectory_jvp_host(m, x, steps=2, params=bad, theta=np.ones(len(bad)))
        with pytest.raises(hb.TdsHipError, match="tds_hip error 1:") as e:
            hb.trajectory_vjp_host(m, x, np.zeros((1, 2, gs.shape[2])), 2, params=bad, theta=np.ones(len(bad)))
        assert str(e.value) == str(e_jvp.value)
    # malformed arrays are refused in Python, before the library is called: N = 2, K = 2, steps = 2
    x, th = x0[:2], th[:2]
    nin, nout, p, nsd = m.input_dim, m.output_dim, len(sel), gs.shape[2]
    n_act = hb.trajectory_dims(m, 2)[1]
    P = hb.policy_network_spec(m)[4]
    z = np.zeros
    for bad_theta, got in ((th[:, :-1], f"({2}, {p - 1})"), (th[:1], f"(1, {p})"), (th[0, :-1], f"({p - 1},)")):
        for call in (lambda t: hb.jvp_params_host(m, x, t, sel),
                     lambda t: hb.vjp_params_host(m, x, t, sel, z((2, nout))),
                     lambda t: hb.trajectory_jvp_host(m, x, steps=2, params=sel, theta=t),
                     lambda t: hb.trajectory_vjp_host(m, x, z((2, 2, nsd)), 2, params=sel, theta=t),
                     lambda t: hb.policy_trajectory_vjp_host(m, x, z(P), z((2, 2, nsd)), 2, params=sel, theta=t)):
            with pytest.raises(ValueError, match=rf"theta: expected \[{p}\] or \[2, {p}\], got " + got.replace("(", r"\(").replace(")", r"\)")):
                call(bad_theta)
    for v in (z((2, 2, nin + p + 1)), z((3, 2, nin + p)), z((2, nin + p + 1)), z((2, 2, 1, nin + p))):
        with pytest.raises(ValueError, match=rf"v: expected \[2, K, {nin + p}\]"):
            hb.jvp_params_host(m, x, th, sel, v)
        with pytest.raises(ValueError, match=rf"v: expected \[2, K, {nin + p}\]"):
            hb.trajectory_jvp_host(m, x, v, 2, params=sel, theta=th)
    for w in (z((2, 2, nout + 1)), z((3, 2, nout)), z((2, nout + 1)), z((2, 2, 1, nout))):
        with pytest.raises(ValueError, match=rf"w: expected \[2, K, {nout}\] or \[2, {nout}\], got "):
            hb.vjp_params_host(m, x, th, sel, w)
        with pytest.raises(ValueError, match=rf"w: expected \[2, K, {nout}\] or \[2, {nout}\], got "):
            hb.vjp_host(m, x, w)
    for bad_u in (z((2, 2, n_act)), z((2, 1, n_act + 1)), z((1, 1, n_act))):
        with pytest.raises(ValueError, match=rf"u: expected \[2, 1, {n_act}\], got "):
            hb.trajectory_jvp_host(m, x, steps=2, u=bad_u)
        with pytest.raises(ValueError, match=rf"u: expected \[2, 1, {n_act}\], got "):
            hb.trajectory_vjp_host(m, x, z((2, 2, nsd)), 2, u=bad_u)
    for bad_gs in (z((2, 1, nsd)), z((2, 2, nsd + 1)), z((1, 2, nsd))):
        with pytest.raises(ValueError, match=rf"gs: expected \[2, 2, {nsd}\], got "):
            hb.trajectory_vjp_host(m, x, bad_gs, 2)
        with pytest.raises(ValueError, match=rf"gs: expected \[2, 2, {nsd}\], got "):
            hb.policy_trajectory_vjp_host(m, x, z(P), bad_gs, 2)
    for bad_ga in (z((2, 1, n_act)), z((2, 2, n_act + 1)), z((1, 2, n_act))):
        with pytest.raises(ValueError, match=rf"ga: expected \[2, 2, {n_act}\], got "):
            hb.policy_trajectory_vjp_host(m, x, z(P), None, 2, ga=bad_ga)
    for bad_pol, got in ((z(P + 1), rf"\({P + 1},\)"), (z((1, P)), rf"\(1, {P}\)"), (z((2, P - 1)), rf"\(2, {P - 1}\)")):
        with pytest.raises(ValueError, match=rf"policy: expected \[{P}\] or \[2, {P}\], got " + got):
            hb.policy_trajectory_vjp_host(m, x, bad_pol, z((2, 2, nsd)), 2)


@pytest.mark.parametrize("name", REFUSED)
def test_refused_models_give_the_trajectory_jvp_message(name, built):
    m = tds_amd.load_model(name)
    x = np.zeros((1, m.input_dim))
    with pytest.raises(hb.TdsHipError) as e_jvp:
        hb.trajectory_jvp_host(m, x, steps=3)
    with pytest.raises(hb.TdsHipError, match="not supported") as e:
        hb.trajectory_vjp_host(m, x, np.zeros((1, 3, m.dof_q + m.dof_qd)), 3)
    assert str(e.value) == str(e_jvp.value)
