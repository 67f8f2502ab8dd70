"""CPU: closed-loop policy gradients on the host (tds_hip_policy_trajectory_vjp_host) — the degenerate policy against
the open-loop trajectory VJP, the primal against a numpy policy, the open-loop primal and the reference's loop, the
gradients against the explicit lambda-recursion with a numpy backward pass and against central differences of the
reference's closed loop, the observation mask, zero and linear cotangents, overflowing tapes, NaN environments, errors
and refusals.

Weight scale: the policies are drawn as SCALE * normal / sqrt(fan_in) (biases SCALE * normal) with SCALE = 0.3, seed 21.
With it every environment of the reference's closed loop of every model below stays below |s| = 1e3 over the T = 12
steps (asserted in test_states_match_the_reference_loop; measured maxima are printed there)."""
import ctypes as C
import functools
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
from test_param_derivs_cpu import REFUSED  # noqa: E402
from test_traj_vjp_cpu import case  # noqa: E402

MODELS = ["ant", "laikago", "ant_floating", "pendulum5_plane", "pendulum5", "cartpole"]
RAW = {"pendulum5": True, "cartpole": True}  # fixed bases: q[0], q[1] are joints
KINDS = ["linear", "mlp"]
N, T = 6, 12
SCALE, SEED = 0.3, 21
TANH, RELU, IDENTITY = 0, 2, -1
needs_ref = pytest.mark.skipif(not reflib.available(), reason="the reference library is not built here")


def rel(a, b):
    return float(np.max(np.abs(a - b)) / max(1.0, np.max(np.abs(b)))) if a.size else 0.0


def worst(a, b):
    return max(rel(a[e], b[e]) for e in range(a.shape[0]))


def net_of(m, kind):
    """(layer_sizes, activations, use_bias) as numpy sees them: the linear policy spelled out as a network"""
    od, ad = m.dof_q + m.dof_qd, m.action_dim
    if kind == "linear":
        return [od, ad], [IDENTITY], [0, 1]
    return [od, 16, 16, ad], [TANH, RELU, IDENTITY], [1, 1, 1, 1]


def net_args(m, kind):
    """the network as the call takes it: None for the linear policy"""
    if kind == "linear":
        return {}
    ls, act, ub = net_of(m, kind)
    return dict(layer_sizes=ls, activations=act, use_bias=ub)


def offsets(ls, ub):
    """(weight offset per layer >= 1, bias offset per layer or None), biases behind all weights"""
    wo, w = {}, 0
    for i in range(1, len(ls)):
        wo[i] = w
        w += ls[i - 1] * ls[i]
    bo, b = {}, w
    for i in range(len(ls)):
        bo[i] = b if ub[i] else None
        b += ls[i] if ub[i] else 0
    return wo, bo, b


def draw_policy(m, kind, n=N, seed=SEED):
    ls, act, ub = net_of(m, kind)
    wo, bo, P = offsets(ls, ub)
    rng = np.random.default_rng(seed)
    pol = np.zeros((n, P))
    for i in range(1, len(ls)):
        pol[:, wo[i]:wo[i] + ls[i - 1] * ls[i]] = SCALE * rng.normal(size=(n, ls[i - 1] * ls[i])) / np.sqrt(ls[i - 1])
    for i in range(len(ls)):
        if ub[i]:
            pol[:, bo[i]:bo[i] + ls[i]] = SCALE * rng.normal(size=(n, ls[i]))
    return pol


def act_f(kind, v):
    return np.tanh(v) if kind == TANH else np.maximum(v, 0.0) if kind == RELU else v


def act_d(kind, v):
    return 1.0 - np.tanh(v) ** 2 if kind == TANH else (v > 0.0).astype(float) if kind == RELU else np.ones_like(v)


def np_forward(net, pol, obs, raw):
    """(actions [n, act], the layers' values a, pre-activations v) of the network per environment"""
    ls, act, ub = net
    wo, bo, _ = offsets(ls, ub)
    o = obs.copy()
    if not raw:
        o[:, :2] = 0.0
    if ub[0]:
        o = o + pol[:, bo[0]:bo[0] + ls[0]]
    a, vs = [o], [None]
    for i in range(1, len(ls)):
        W = pol[:, wo[i]:wo[i] + ls[i - 1] * ls[i]].reshape(-1, ls[i], ls[i - 1])
        v = np.einsum("ncp,np->nc", W, a[-1])
        if ub[i]:
            v = v + pol[:, bo[i]:bo[i] + ls[i]]
        vs.append(v)
        a.append(act_f(act[i - 1], v))
    return a[-1], a, vs


def np_backward(net, pol, a, vs, ubar, raw):
    """(gpolicy [n, P], masked observation adjoint [n, obs])"""
    ls, act, ub = net
    wo, bo, P = offsets(ls, ub)
    g = np.zeros((pol.shape[0], P))
    d = ubar
    for i in range(len(ls) - 1, 0, -1):
        d = d * act_d(act[i - 1], vs[i])
        if ub[i]:
            g[:, bo[i]:bo[i] + ls[i]] = d
        g[:, wo[i]:wo[i] + ls[i - 1] * ls[i]] = np.einsum("nc,np->ncp", d, a[i - 1]).reshape(pol.shape[0], -1)
        W = pol[:, wo[i]:wo[i] + ls[i - 1] * ls[i]].reshape(-1, ls[i], ls[i - 1])
        d = np.einsum("ncp,nc->np", W, d)
    if ub[0]:
        g[:, bo[0]:bo[0] + ls[0]] = d
    d = d.copy()
    if not raw:
        d[:, :2] = 0.0
    return g, d


def raw_of(name, t, first_raw=False):
    return bool(RAW.get(name)) or (first_raw and t == 0)


@functools.lru_cache(maxsize=None)
def setup(name, kind):
    """(m, sel, x0, theta, gs at every = 1, ga, policy); shared between the tests: read only"""
    m, sel, x0, _, th, gs = case(name)
    ga = np.random.default_rng(18).normal(size=(N, T, m.action_dim))
    pol = draw_policy(m, kind)
    for a in (ga, pol):
        a.setflags(write=False)
    return m, sel, x0, th, gs, ga, pol


def call(name, kind, gs, ga, every=1, steps=T, pol=None, theta="case", params="case", **kw):
    m, sel, x0, th, _, _, p0 = setup(name, kind)
    return hb.policy_trajectory_vjp_host(m, x0, p0 if pol is None else pol, gs, steps, every, ga,
                                         params=sel if params == "case" else params,
                                         theta=th if theta == "case" else theta, obs_raw=bool(RAW.get(name)),
                                         **net_args(m, kind), **kw)


def gs_of(gs, every):
    return np.ascontiguousarray(gs[:, every - 1::every])


@functools.lru_cache(maxsize=None)
def primal(name, kind):
    m, sel, x0, th, gs, ga, pol = setup(name, kind)
    s, u = call(name, kind, None, None)
    s.setflags(write=False), u.setflags(write=False)
    return s, u


def recursion(name, kind, every, with_ga, first_raw=False):
    """(gpolicy, gx0, gtheta, ubar [n, T, act]) of the explicit lambda-recursion over vjp_params_host and np_backward
    along the primal of the call"""
    m, sel, x0, th, gs, ga, pol = setup(name, kind)
    net = net_of(m, kind)
    nsd, nact, nin = m.dof_q + m.dof_qd, m.action_dim, m.input_dim
    if first_raw:
        s, u = hb.policy_trajectory_vjp_host(m, x0, pol, None, T, params=sel, theta=th, first_obs_raw=True,
                                             **net_args(m, kind))
    else:
        s, u = primal(name, kind)
    lam = np.zeros((N, nsd))
    gpol, gx0, gth = np.zeros_like(pol), np.zeros((N, nin)), np.zeros((N, len(sel)))
    ubars = np.zeros((N, T, nact))
    for t in range(T - 1, -1, -1):
        x = x0.copy()
        if t > 0:
            x[:, :nsd] = s[:, t - 1]
        x[:, nsd:nsd + nact] = u[:, t]
        w = np.zeros((N, m.output_dim))
        w[:, :nsd] = lam
        if (t + 1) % every == 0:
            w[:, :nsd] += gs[:, t]
        wj = hb.vjp_params_host(m, x, th, sel, w)
        ubar = wj[:, nsd:nsd + nact] + (ga[:, t] if with_ga else 0.0)
        ubars[:, t] = ubar
        gx0[:, nsd + nact:] += wj[:, nsd + nact:nin]
        gth += wj[:, nin:]
        raw = raw_of(name, t, first_raw)
        _, a, vs = np_forward(net, pol, x[:, :nsd], raw)
        g, dobs = np_backward(net, pol, a, vs, ubar, raw)
        gpol += g
        lam = wj[:, :nsd] + dobs
    gx0[:, :nsd] = lam
    return gpol, gx0, gth, ubars


# ---------------------------------------------------------------- the degenerate policy
@pytest.mark.parametrize("name", MODELS)
def test_zero_weights_are_the_open_loop_trajectory(name, built):
    m, sel, x0, th, gs, _, pol = setup(name, "linear")
    nsd, nact = m.dof_q + m.dof_qd, m.action_dim
    b = np.random.default_rng(19).uniform(-0.2, 0.2, (N, nact))
    deg = np.zeros_like(pol)
    deg[:, nsd * nact:] = b
    s, u, gpol, gx0, gth = call(name, "linear", gs, None, pol=deg)
    xb = x0.copy()
    xb[:, nsd:nsd + nact] = b
    s_o, gx0_o, _, gth_o = hb.trajectory_vjp_host(m, xb, gs, T, 1, None, sel, th)
    np.testing.assert_array_equal(s, s_o)
    np.testing.assert_array_equal(u, np.broadcast_to(b[:, None], u.shape))
    assert worst(gpol[:, nsd * nact:], gx0_o[:, nsd:nsd + nact]) <= 1e-12
    assert np.all(gx0[:, nsd:nsd + nact] == 0.0)
    for got, ref in ((gx0[:, :nsd], gx0_o[:, :nsd]), (gx0[:, nsd + nact:], gx0_o[:, nsd + nact:]), (gth, gth_o)):
        assert worst(got, ref) <= 1e-12
    # the weight block: sum_t ubar_t (x) obs_t, ubar_t from the open loop with the actions as a sequence
    ub = np.ascontiguousarray(np.broadcast_to(b[:, None], (N, T - 1, nact)))
    _, gx0_u, gu, _ = hb.trajectory_vjp_host(m, xb, gs, T, 1, ub, sel, th)
    ubar = np.concatenate([gx0_u[:, None, nsd:nsd + nact], gu], axis=1)
    obs = np.concatenate([x0[:, None, :nsd], s[:, :-1]], axis=1).copy()
    if not RAW.get(name):
        obs[:, :, :2] = 0.0
    ref_w = np.einsum("nta,nto->nao", ubar, obs).reshape(N, -1)
    assert worst(gpol[:, :nsd * nact], ref_w) <= 1e-12
    assert np.count_nonzero(gpol) > 0


# ---------------------------------------------------------------- the primal
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", MODELS)
def test_actions_and_states_of_the_primal(name, kind, built):
    m, sel, x0, th, gs, ga, pol = setup(name, kind)
    nsd = m.dof_q + m.dof_qd
    s, u = primal(name, kind)
    assert s.shape == (N, T, nsd) and u.shape == (N, T, m.action_dim)
    obs = np.concatenate([x0[:, None, :nsd], s[:, :-1]], axis=1)
    for t in range(T):
        u_np = np_forward(net_of(m, kind), pol, obs[:, t], raw_of(name, t))[0]
        assert worst(u[:, t], u_np) <= 1e-12, (t, worst(u[:, t], u_np))
    xu = x0.copy()
    xu[:, nsd:nsd + m.action_dim] = u[:, 0]
    s_open, _ = hb.trajectory_jvp_host(m, xu, steps=T, u=np.ascontiguousarray(u[:, 1:]), params=sel, theta=th)
    np.testing.assert_array_equal(s, s_open)
    # with a cotangent the primal is the same, and `every` selects from it
    s3, u3 = call(name, kind, gs_of(gs, 3), None, every=3)[:2]
    np.testing.assert_array_equal(s3, s[:, 2::3])
    np.testing.assert_array_equal(u3, u)


def make_ref(name):
    import gen_golden  # noqa: E402  (checker only: the table of reference constructors)

    return gen_golden.make_ref(name)[0]


def ref_closed_loop(r, m, net, x0, pol, name, steps=T):
    """(s [n, steps, nsd], u [n, steps, act]) of the reference's step under the numpy policy"""
    nsd, nact = m.dof_q + m.dof_qd, m.action_dim
    x, ss, us = x0.copy(), [], []
    for t in range(steps):
        u = np_forward(net, pol, x[:, :nsd], raw_of(name, t))[0]
        x[:, nsd:nsd + nact] = u
        y = r.step(x)[:, :nsd]
        x[:, :nsd] = y
        ss.append(y), us.append(u)
    return np.stack(ss, axis=1), np.stack(us, axis=1)


@needs_ref
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", MODELS)
def test_states_match_the_reference_loop(name, kind, built):
    m, sel, x0, th, gs, ga, pol = setup(name, kind)
    s, u = hb.policy_trajectory_vjp_host(m, x0, pol, None, T, obs_raw=bool(RAW.get(name)), **net_args(m, kind))
    r = make_ref(name)
    try:
        s_ref, u_ref = ref_closed_loop(r, m, net_of(m, kind), x0, pol, name)
    finally:
        r.close()
    print(name, kind, "max |s| of the reference's closed loop", np.abs(s_ref).max(), "against it", rel(s, s_ref))
    assert np.all(np.abs(s_ref) < 1e3)  # no environment is excluded
    assert rel(s, s_ref) <= 1e-9, rel(s, s_ref)
    assert rel(u, u_ref) <= 1e-9


# ---------------------------------------------------------------- the gradients
@pytest.mark.parametrize("with_ga", [False, True])
@pytest.mark.parametrize("every", [1, 3])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", MODELS)
def test_gradients_match_the_lambda_recursion(name, kind, every, with_ga, built):
    m, sel, x0, th, gs, ga, pol = setup(name, kind)
    s, u, gpol, gx0, gth = call(name, kind, gs_of(gs, every), ga if with_ga else None, every=every)
    np.testing.assert_array_equal(s, primal(name, kind)[0][:, every - 1::every])
    gpol_r, gx0_r, gth_r, _ = recursion(name, kind, every, with_ga)
    w = max(worst(gpol, gpol_r), worst(gx0, gx0_r), worst(gth, gth_r))
    print(name, kind, every, with_ga, "against the recursion", w)
    assert w <= 1e-10, w
    assert np.count_nonzero(gpol) > 0 and np.count_nonzero(gx0) > 0 and np.count_nonzero(gth) > 0
    assert np.all(gx0[:, m.dof_q + m.dof_qd:m.dof_q + m.dof_qd + m.action_dim] == 0.0)


def test_only_ga_is_a_cotangent_too(built):
    name, kind = "pendulum5_plane", "mlp"
    m, sel, x0, th, gs, ga, pol = setup(name, kind)
    s, u, gpol, gx0, gth = call(name, kind, None, ga)
    z = call(name, kind, np.zeros_like(gs), ga)
    for a, b in zip((s, u, gpol, gx0, gth), z):
        np.testing.assert_array_equal(a, b)
    assert np.count_nonzero(gpol) > 0


def fd_entries(m, kind):
    """policy entries in different layers (linear: two weights and a bias)"""
    ls, act, ub = net_of(m, kind)
    wo, bo, P = offsets(ls, ub)
    if kind == "linear":
        return [wo[1] + 3, wo[1] + ls[0] * (ls[1] - 1) + ls[0] - 2, bo[1] + ls[1] // 2]
    return [wo[1] + 2 * ls[0] + 4, wo[2] + 5 * 16 + 3, wo[3] + 7, bo[2] + 1, bo[3] + ls[3] - 1]


@needs_ref
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", MODELS)
def test_gradients_match_central_differences_of_the_reference(name, kind, built):
    """loss <gs, s> + <ga, u> of the reference's closed loop, h = 1e-6, on entries whose one-sided differences agree"""
    m, _, x0, _, gs, ga, pol = setup(name, kind)
    net = net_of(m, kind)
    g = list(m.gravity)
    sel = [("gravity", 2)]
    _, _, gpol, _, gth = call(name, kind, gs, ga, params=sel, theta=np.array([g[2]]))
    r = make_ref(name)
    h, checked, per_entry = 1e-6, 0, []

    cot = np.concatenate([gs.reshape(N, -1), ga.reshape(N, -1)], axis=1)

    def loss(p):
        """the trajectory the loss is linear in, [n, T (nsd + act)]: the differences below are taken on it BEFORE the
        dot product with the cotangent, so that the sum's round-off (terms of up to 245 |gs|) is not divided by h"""
        s, u = ref_closed_loop(r, m, net, x0, p, name)
        return np.concatenate([s.reshape(N, -1), u.reshape(N, -1)], axis=1)

    def compare(f, got, what):
        """f(step) -> trajectory; got [n]; the environments whose one-sided differences agree are compared.  The two
        second-order one-sided differences are the reference's own estimates of the derivative: where they disagree
        by more than the bound asserted below (a branch switch within +- 2h, or the reference's round-off at |s| up
        to 245 over h = 1e-6: the disagreement grows as 1 / h there), the central difference cannot certify that bound
        and the environment is left out; the counts are asserted"""
        y0, yp, ym, yp2, ym2 = f(0.0), f(h), f(-h), f(2 * h), f(-2 * h)
        dot = lambda y: np.einsum("nk,nk->n", y, cot)  # noqa: E731
        fd = dot(yp - ym) / (2 * h)
        fwd, bwd = dot(4 * (yp - y0) - (yp2 - y0)) / (2 * h), dot(4 * (y0 - ym) - (y0 - ym2)) / (2 * h)
        ok = np.abs(fwd - bwd) <= 1e-6 * np.maximum(1.0, np.abs(fd))
        # ... and the reference's round-off: it enters a central difference as 1 / h (measured on pendulum5_plane and
        # laikago: 1e-8, 2e-7, 3e-6, 3e-5 at h = 1e-4 .. 1e-7 for losses of several hundred), the truncation as h^2, so
        # the central difference over 10 h shows what that of h carries: an environment is compared where the two agree
        # to half the bound, i.e. where the reference's derivative is known to better than what is asserted
        fd10 = dot(f(10 * h) - f(-10 * h)) / (20 * h)
        ok &= np.abs(fd - fd10) <= 0.5e-6 * np.maximum(1.0, np.abs(fd))
        err = np.abs(fd - got) / np.maximum(1.0, np.abs(got))
        print(name, kind, what, "checked", int(ok.sum()), "worst", err[ok].max() if ok.any() else None)
        assert np.all(err[ok] <= 1e-6), (name, kind, what, err, ok)
        return int(ok.sum())

    try:
        for j in fd_entries(m, kind):
            def f(d, j=j):
                p = pol.copy()
                p[:, j] += d
                return loss(p)
            per_entry.append(compare(f, gpol[:, j], ("policy", j)))

        def f_g(d):
            r.set_gravity([g[0], g[1], g[2] + d])
            try:
                return loss(pol)
            finally:
                r.set_gravity(g)
        per_entry.append(compare(f_g, gth[:, 0], "gravity z"))
    finally:
        r.close()
    checked = sum(per_entry)
    assert len(per_entry) >= 4 and min(per_entry) >= 1 and checked >= 2 * len(per_entry), per_entry


# ---------------------------------------------------------------- the observation mask
def test_masked_observation_entries_pass_nothing_back(built):
    name, kind = "ant", "linear"
    m, sel, x0, th, gs, ga, pol = setup(name, kind)
    nsd, nact = m.dof_q + m.dof_qd, m.action_dim
    run = lambda **kw: hb.policy_trajectory_vjp_host(m, x0, pol, gs, T, 1, ga, params=sel, theta=th, **kw)  # noqa: E731
    s0, u0, gp0, gx0, _ = run()
    s1, u1, gp1, gx1, _ = run(first_obs_raw=True)
    s2, u2, gp2, gx2, _ = run(obs_raw=True)
    cols = lambda gp: gp[:, :nsd * nact].reshape(N, nact, nsd)[:, :, :2]  # noqa: E731
    assert np.all(cols(gp0) == 0.0)
    # bits clear: gx0[0:2] is the physical part alone (the recursion masks the policy's term)
    _, gx0_r, _, _ = recursion(name, kind, 1, True)
    assert worst(gx0[:, :2], gx0_r[:, :2]) <= 1e-10
    # bit 0: step 0 alone sees the raw entries: its columns are ubar_0 (x) obs_0[0:2], and gx0[0:2] gains W^T ubar_0
    gp_r, gx1_r, _, ubars = recursion(name, kind, 1, True, first_raw=True)
    assert worst(cols(gp1), np.einsum("na,no->nao", ubars[:, 0], x0[:, :2])) <= 1e-10
    assert worst(gx1, gx1_r) <= 1e-10 and worst(gp1, gp_r) <= 1e-10
    assert np.any(u1[:, 0] != u0[:, 0]) and np.count_nonzero(cols(gp1)) > 0
    W01 = pol[:, :nsd * nact].reshape(N, nact, nsd)[:, :, :2]
    assert np.all(np.abs(np.einsum("nao,na->no", W01, ubars[:, 0])) > 0)
    # bit 1: every step does
    obs2 = np.concatenate([x0[:, None, :nsd], s2[:, :-1]], axis=1)
    for t in (0, 1, T - 1):
        assert worst(u2[:, t], np_forward(net_of(m, kind), pol, obs2[:, t], True)[0]) <= 1e-12
    assert np.any(u2[:, 1:] != u1[:, 1:]) and np.any(cols(gp2) != cols(gp1))


# ---------------------------------------------------------------- edge cases
def test_zero_and_linear_cotangents(built):
    name, kind = "ant", "mlp"
    m, sel, x0, th, gs, ga, pol = setup(name, kind)
    rng = np.random.default_rng(15)
    g1, a1 = gs_of(gs, 3), ga
    g2, a2 = rng.normal(size=g1.shape), rng.normal(size=a1.shape)
    run = lambda g, a: call(name, kind, g, a, every=3)[2:]  # noqa: E731
    for out in run(np.zeros_like(g1), np.zeros_like(a1)):
        assert np.all(out == 0.0)
    for oa, ob, oab in zip(run(g1, a1), run(g2, a2), run(2.0 * g1 - 0.5 * g2, 2.0 * a1 - 0.5 * a2)):
        assert rel(oab, 2.0 * oa - 0.5 * ob) <= 1e-12


def raw_call(m, x0, pol, gs, ga, steps, sel, th, every=1, flags=0, net=(0, None, None, None), tape_cap=0):
    """the C call itself: (rc, s, u, gpolicy, gx0, gtheta, tape lengths)"""
    n, p = x0.shape[0], len(sel)
    nsd, n_act, n_rec = hb.trajectory_dims(m, steps, every)
    s, u = np.zeros((n, max(n_rec, 1), nsd)), np.zeros((n, max(steps, 1), max(n_act, 1)))
    gpol, gx0, gth = np.ones_like(pol), np.ones((n, m.input_dim)), np.ones((n, max(p, 1)))
    lens = np.zeros((n, max(steps, 1)), dtype=np.int32)
    arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in (x0, pol, th, gs, ga)]
    ints = [None if a is None else np.ascontiguousarray(a, dtype=np.int32) for a in net[1:]]
    ip = [None if a is None else a.ctypes.data for a in ints]
    rc = hb.lib().tds_hip_policy_trajectory_vjp_host(
        C.byref(m), n, steps, every, flags, arrs[0].ctypes.data, arrs[1].ctypes.data, net[0], ip[0], ip[1], ip[2], p,
        hb.param_spec(sel), arrs[2].ctypes.data, arrs[3].ctypes.data, arrs[4].ctypes.data, s.ctypes.data, u.ctypes.data,
        gpol.ctypes.data, gx0.ctypes.data, gth.ctypes.data, int(tape_cap), lens.ctypes.data)
    return rc, s, u, gpol, gx0, gth[:, :p], lens


def test_a_small_tape_capacity_gives_nan_gradients_for_the_overflowing_environments(built):
    name, kind = "ant", "linear"
    m, sel, x0, th, gs, ga, pol = setup(name, kind)
    ref = call(name, kind, gs, ga, tape_len=True)
    longest = ref[5].max(axis=1)
    cap = int(np.sort(longest)[N // 2 - 1])
    over = longest > cap
    assert 0 < over.sum() < N, longest
    rc, s, u, gpol, gx0, gth, lens = raw_call(m, x0, pol, gs, ga, T, sel, th, tape_cap=cap)
    assert rc == 2  # TDS_ERR_UNSUPPORTED
    np.testing.assert_array_equal(lens, np.where(ref[5] > cap, -1, ref[5]))
    for got, want in ((gpol, ref[2]), (gx0, ref[3]), (gth, ref[4])):
        assert np.all(np.isnan(got[over]))
        np.testing.assert_array_equal(got[~over], want[~over])
    np.testing.assert_array_equal(s, ref[0])
    np.testing.assert_array_equal(u, ref[1])
    with pytest.raises(hb.TdsHipError, match="tape exceeds the capacity"):
        call(name, kind, gs, ga, tape_cap=cap)


def test_not_positive_definite_gives_nan_gradients_for_that_environment_only(built):
    """test_traj_vjp_cpu's case: the base link's mass negative in environment 1"""
    name = "pendulum5_plane"
    m = tds_amd.load_model(name)
    x = np.ascontiguousarray(np.repeat(np.load(os.path.join(ROOT, "tests", "golden", f"{name}.npz"))["x"][5:6], 2, 0))
    sel = [("mass", 0)]
    theta = np.array([[m.links[0].mass], [-0.1 * m.links[0].mass]])
    nsd, n_act, _ = hb.trajectory_dims(m, T)
    pol = np.repeat(draw_policy(m, "linear", 1, 22), 2, 0)
    pol[:, :nsd * n_act] *= 1e-3  # weak feedback: the pendulum falls to the plane as it does in the open loop
    gs = np.random.default_rng(17).normal(size=(2, T, nsd))
    ga = np.random.default_rng(18).normal(size=(2, T, n_act))
    rc, s, u, gpol, gx0, gth, _ = raw_call(m, x, pol, gs, ga, T, sel, theta)
    assert rc == 1  # TDS_ERR_INVALID_ARG
    rc1, s1, u1, gpol1, gx1, gth1, _ = raw_call(m, x[:1], pol[:1], gs[:1], ga[:1], T, sel, theta[:1])
    assert rc1 == 0
    for got, ref in ((s, s1), (u, u1), (gpol, gpol1), (gx0, gx1), (gth, gth1)):
        np.testing.assert_array_equal(got[:1], ref)
        assert np.all(np.isfinite(ref))
    assert np.all(np.isnan(gpol[1])) and np.all(np.isnan(gx0[1])) and np.all(np.isnan(gth[1]))
    nan_rec = np.isnan(s[1]).all(axis=1)
    first = int(np.argmax(nan_rec))
    assert first > 0 and np.all(nan_rec[first:]) and np.all(np.isfinite(s[1, :first]))


def test_invalid_network_steps_and_every(built):
    name = "pendulum5"
    m, sel, x0, th, gs, ga, pol = setup(name, "linear")
    od, ad = m.dof_q + m.dof_qd, m.action_dim
    x, g = x0[:1], np.zeros((1, 1, od))
    for steps, every in ((0, 1), (-2, 1), (6, 4), (6, 0), (6, -3)):
        with pytest.raises(hb.TdsHipError, match="tds_hip error 1:"):
            hb.policy_trajectory_vjp_host(m, x, pol[:1], g, steps, every)
    big = np.zeros((1, 4096 * 8))
    for ls, act, ub in (([od + 1, ad], [IDENTITY], [0, 1]), ([od, ad + 1], [IDENTITY], [0, 1]),
                        ([od, 0, ad], [TANH, IDENTITY], [0, 1, 1]), ([od, 257, ad], [TANH, IDENTITY], [0, 1, 1]),
                        ([od, 8, ad], [7, IDENTITY], [0, 1, 1]), ([od, 8, ad], [-2, IDENTITY], [0, 1, 1]),
                        ([od], [IDENTITY], [0]), ([od] + [4] * 7 + [ad], [TANH] * 8, [0] * 9)):
        P = hb.policy_network_spec(m, ls, act, ub)[4]
        rc = raw_call(m, x, big[:, :max(P, 1)], np.zeros((1, 2, od)), np.zeros((1, 2, max(ad, 1))), 2, [],
                      np.zeros((1, 1)), net=(len(ls), ls, act, ub))[0]
        assert rc == 1, (ls, act, ub)
    rc = raw_call(m, x, pol[:1], np.zeros((1, 2, od)), np.zeros((1, 2, ad)), 2, [], np.zeros((1, 1)), flags=4)[0]
    assert rc == 1
    rc = raw_call(m, x, pol[:1], np.zeros((1, 2, od)), np.zeros((1, 2, ad)), 2, [], np.zeros((1, 1)), flags=2)[0]
    assert rc == 0


def test_a_model_without_actions_is_an_invalid_argument(built):
    m = tds_amd.load_model("cube_floating")
    assert m.action_dim < 1
    x = diff_states.states("cube_floating", 1, 11, m)
    with pytest.raises(hb.TdsHipError, match="tds_hip error 1:.*no actions"):
        hb.policy_trajectory_vjp_host(m, x, np.zeros((1, hb.policy_network_spec(m)[4])),
                                      np.zeros((1, 3, m.dof_q + m.dof_qd)), 3)


@pytest.mark.parametrize("name", REFUSED)
def test_refused_models_give_the_trajectory_jvp_message(name, built):
    m = tds_amd.load_model(name)
    x = np.zeros((1, m.input_dim))
    with pytest.raises(hb.TdsHipError) as e_jvp:
        hb.trajectory_jvp_host(m, x, steps=3)
    P = hb.policy_network_spec(m)[4]
    with pytest.raises(hb.TdsHipError, match="not supported") as e:
        hb.policy_trajectory_vjp_host(m, x, np.zeros((1, P)), np.zeros((1, 3, m.dof_q + m.dof_qd)), 3)
    assert str(e.value) == str(e_jvp.value)
