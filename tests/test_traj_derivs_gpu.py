"""GPU: the articulated trajectories' kernels (tds_traj.hip) against their host instantiation, chunked launches,
consistency with the step derivatives on the same handle, trajectory_fn (gradcheck, against chained
param_step_fn(mode="reverse")), and the pendulum system identification through one trajectory call per loss."""
import os

import numpy as np
import pytest

from conftest import ROOT

import tds_amd
from tds_amd import hip_backend as hb
import diff_states

pytestmark = pytest.mark.gpu

# device against host: the step's transcendental functions are the device's and the host's own (sin, cos); every
# other operation rounds alike (no FP contraction on either side).  Measured maximum: DESIGN 7a.
DEV_TOL = 1e-10
SEL = {"ant": [("gravity", 2), ("friction",), ("mass", 3)], "laikago": [("mass", 2), ("gravity", 0)],
       "pendulum5": [("mass", 2), ("stiffness", 1)], "cube_floating": [("base_mass",), ("friction",)]}


def records(name, n, seed=0):
    g = np.load(os.path.join(ROOT, "tests", "golden", f"{name}.npz"))
    rng = np.random.default_rng(seed)
    return g["x"][rng.integers(0, g["x"].shape[0], n)]


def starts(name, n, seed=0):
    m = tds_amd.load_model(name)
    return diff_states.states(name, n, seed, m) if name in diff_states.MODELS else records(name, n, seed)


def rel(a, b):
    return float(np.max(np.abs(a - b)) / max(1.0, np.max(np.abs(b))))


def inputs(name, n, T, k, seed):
    m = tds_amd.load_model(name)
    sel = SEL[name]
    x = np.ascontiguousarray(starts(name, n, seed))
    base = hb.params_get(m, sel)
    rng = np.random.default_rng(seed + 1)
    th = base * (1.0 + 0.01 * rng.uniform(-1, 1, (n, len(sel))))
    v = rng.normal(size=(n, k, m.input_dim + len(sel)))
    _, n_act, _ = hb.trajectory_dims(m, T)
    u = rng.uniform(-0.2, 0.2, (n, T - 1, n_act))
    return m, sel, x, th, v, u


def device(sim, x, v, T, u, sel, th, every=1):
    import torch

    c = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    s, js = sim.trajectory_jvp(c(x), c(v), T, every, c(u), sel, c(th))
    return s.cpu().numpy(), (None if js is None else js.cpu().numpy())


@pytest.mark.parametrize("n", [1, 7, 4096])
@pytest.mark.parametrize("name", ["ant", "laikago", "pendulum5", "cube_floating"])
def test_device_matches_host(name, n, built):
    T = 48
    m, sel, x, th, v, u = inputs(name, n, T, 3, 0)
    sim = hb.HipSim(m, min(n, 64), device=0, dtype="f64")
    s, js = device(sim, x, v, T, u, sel, th)
    s0, _ = device(sim, x, None, T, u, sel, th)  # k = 0: the double kernel
    idx = np.arange(n) if n <= 64 else np.random.default_rng(1).choice(n, 64, replace=False)
    s_h, js_h = hb.trajectory_jvp_host(m, x[idx], v[idx], T, 1, u[idx], sel, th[idx])
    # some contact-sweep states (lying inside the plane) diverge within T on host and device alike: those are not
    # compared, where rounding differences grow without bound
    bounded = [e for e in range(len(idx)) if np.all(np.abs(s_h[e]) < 1e3)]
    assert len(bounded) >= 0.75 * len(idx), len(bounded)
    for e_h in bounded:
        e_d = idx[e_h]
        assert rel(s[e_d], s_h[e_h]) <= DEV_TOL, (name, e_d, rel(s[e_d], s_h[e_h]))
        assert rel(js[e_d], js_h[e_h]) <= DEV_TOL, (name, e_d, rel(js[e_d], js_h[e_h]))
    print(name, n, "max rel device-host", max(max(rel(s[idx[e]], s_h[e]), rel(js[idx[e]], js_h[e])) for e in bounded))
    np.testing.assert_array_equal(s0, s)  # the dual's values are the double step's (NaN where both are)


@pytest.mark.parametrize("name", ["ant", "pendulum5"])
def test_chunking_is_invisible(name, built):
    T = 48
    m, sel, x, th, v, u = inputs(name, 9, T, 3, 2)
    sim = hb.HipSim(m, 9, device=0, dtype="f64")
    out = {}
    for chunk in (1, 5):
        sim.set_option("traj_steps", chunk)
        out[chunk] = [device(sim, x, v, T, u, sel, th, every=4), device(sim, x, None, T, None, sel, th, every=3)]
    sim2 = hb.HipSim(m, 9, device=0, dtype="f64")  # the default: T / 16 = 3 launches
    out["default"] = [device(sim2, x, v, T, u, sel, th, every=4), device(sim2, x, None, T, None, sel, th, every=3)]
    for key in (5, "default"):
        for (s_a, j_a), (s_b, j_b) in zip(out[1], out[key]):
            np.testing.assert_array_equal(s_a, s_b)
            if j_a is not None:
                np.testing.assert_array_equal(j_a, j_b)


def test_consistency_with_the_step_derivatives_and_the_handle(built):
    import torch

    name, n = "ant", 16
    m, sel, x, th, v, _ = inputs(name, n, 1, 2, 3)
    sim = hb.HipSim(m, n, device=0, dtype="f64")
    xd, thd, vd = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (x, th, v))
    resident = sim.x.clone() if hasattr(sim, "x") else None
    y_b, jv_b = sim.jvp_params(xd, thd, sel, vd)
    jac_b = sim.jacobian(xd)
    s, js = sim.trajectory_jvp(xd, vd, 1, 1, None, sel, thd)
    nsd = m.dof_q + m.dof_qd
    assert rel(s[:, 0].cpu().numpy(), y_b[:, :nsd].cpu().numpy()) <= 1e-12
    assert rel(js[:, :, 0].cpu().numpy(), jv_b[:, :, :nsd].cpu().numpy()) <= 1e-12
    sim.trajectory_jvp(xd, vd, 40, 8, None, sel, thd)  # a longer call grows and reuses the shared work buffer
    y_a, jv_a = sim.jvp_params(xd, thd, sel, vd)
    assert torch.equal(y_a, y_b) and torch.equal(jv_a, jv_b)
    assert torch.equal(sim.jacobian(xd), jac_b)
    if resident is not None:
        assert torch.equal(sim.x, resident)
    for dt in ("f32", "mix"):
        try:
            s32 = hb.HipSim(m, 4, device=0, dtype=dt)
        except (hb.TdsHipError, ValueError, KeyError):
            continue
        with pytest.raises(hb.TdsHipError, match="f64"):
            s32.trajectory_jvp(xd[:4], None, 3)
    with pytest.raises(hb.TdsHipError, match="tds_hip error 1:"):
        sim.trajectory_jvp(xd, None, 6, 4)
    with pytest.raises(hb.TdsHipError, match="spherical"):
        s2 = hb.HipSim(tds_amd.load_model("pendulum5_spherical"), 2, device=0, dtype="f64")
        s2.trajectory_jvp(torch.from_numpy(records("pendulum5_spherical", 2)).cuda(), None, 3)


def test_gradcheck_of_trajectory_fn(built):
    import torch

    m = tds_amd.load_model("pendulum5")
    n, sel = 2, SEL["pendulum5"]
    sim = hb.HipSim(m, n, device=0, dtype="f64")
    x0 = torch.from_numpy(records("pendulum5", n, 4)).cuda()
    wrt = [0, 3, 6]
    f = tds_amd.trajectory_fn(sim, 6, wrt, sel, every=2)
    z = x0[:, wrt].clone().requires_grad_(True)
    base = hb.params_get(m, sel) + np.array([0.0, 0.5])
    th1 = torch.from_numpy(base).cuda().requires_grad_(True)
    thn = torch.from_numpy(np.stack([base, base * 1.01])).cuda().requires_grad_(True)
    for th in (thn, th1):
        assert torch.autograd.gradcheck(lambda zz, tt: f(x0, zz, tt), (z, th), eps=1e-6, atol=1e-5, rtol=1e-4)
    with pytest.raises(ValueError, match="wrt"):
        f(x0.clone().requires_grad_(True))
    u = torch.zeros((n, 5, m.dof_qd), dtype=torch.float64, device="cuda", requires_grad=True)
    with pytest.raises(ValueError, match="reverse"):
        f(x0, u=u)


def test_trajectory_loss_gradient_matches_chained_reverse_mode_on_the_ant(built):
    import torch

    name, n, T = "ant", 256, 16
    m = tds_amd.load_model(name)
    sel = [("gravity", 2), ("friction",), ("mass", 2), ("mass", 5)]
    sim = hb.HipSim(m, n, device=0, dtype="f64")
    x0 = torch.from_numpy(np.ascontiguousarray(starts(name, n, 5))).cuda()
    nsd = m.dof_q + m.dof_qd
    theta0 = torch.from_numpy(hb.params_get(m, sel)).cuda()
    w = torch.from_numpy(np.random.default_rng(6).normal(size=(n, T, nsd))).cuda()
    th = theta0.clone().requires_grad_(True)
    s = tds_amd.trajectory_fn(sim, T, (), sel)(x0, None, th)
    (g_traj,) = torch.autograd.grad((w * s).sum(), th)
    th2 = theta0.clone().requires_grad_(True)
    f = tds_amd.param_step_fn(sim, sel, mode="reverse")
    x, loss = x0, 0.0
    for t in range(T):
        y = f(x, th2)
        loss = loss + (w[:, t] * y[:, :nsd]).sum()
        x = torch.cat([y[:, :nsd], x0[:, nsd:]], dim=1)
    (g_rev,) = torch.autograd.grad(loss, th2)
    assert rel(g_traj.cpu().numpy(), g_rev.cpu().numpy()) <= 1e-10, (g_traj, g_rev)
    assert torch.count_nonzero(g_traj) == len(sel)
    counts = diff_states.contact_counts(name, m, x0.cpu().numpy()[:32], reference=False)
    assert counts.max() > 0  # contacts are active


def test_system_identification_through_one_trajectory_call(built):
    """test_param_derivs_gpu's pendulum5 identification (SYSID_SEL, seed, T = 60), one trajectory_fn call per loss"""
    import torch
    from test_param_derivs_gpu import SYSID_SEL, SYSID_T, SYSID_N, sysid_setup, host_rollout

    m, base, true, s0, taus = sysid_setup()
    nq = m.dof_q
    target = torch.from_numpy(host_rollout(m, true, s0, taus)).cuda()
    sim = hb.HipSim(m, SYSID_N, device=0, dtype="f64")
    x0 = torch.from_numpy(np.concatenate([s0, taus[0]], axis=1)).cuda()
    u = torch.from_numpy(np.ascontiguousarray(taus[1:].transpose(1, 0, 2))).cuda()
    base_d = torch.from_numpy(base).cuda()
    traj = tds_amd.trajectory_fn(sim, SYSID_T, (), SYSID_SEL)
    f = tds_amd.param_step_fn(sim, SYSID_SEL, mode="reverse")
    taus_d = torch.from_numpy(taus).cuda()

    def loss_of(scale):
        s = traj(x0, None, base_d * scale, u)  # [N, T, 2 nq]
        return ((s[:, :, :nq].transpose(0, 1) - target) ** 2).sum()

    def chained_loss(scale):
        theta, s, loss = base_d * scale, x0[:, :2 * nq], 0.0
        for t in range(SYSID_T):
            s = f(torch.cat([s, taus_d[t]], dim=1), theta)[:, :2 * nq]
            loss = loss + ((s[:, :nq] - target[t]) ** 2).sum()
        return loss

    sc = torch.ones(len(SYSID_SEL), dtype=torch.float64, device="cuda", requires_grad=True)
    (g,) = torch.autograd.grad(loss_of(sc), sc)
    sc2 = torch.ones(len(SYSID_SEL), dtype=torch.float64, device="cuda", requires_grad=True)
    (g_rev,) = torch.autograd.grad(chained_loss(sc2), sc2)
    assert rel(g.cpu().numpy(), g_rev.cpu().numpy()) <= 1e-10, (g, g_rev)

    sc = torch.ones(len(SYSID_SEL), dtype=torch.float64, device="cuda", requires_grad=True)
    opt = torch.optim.LBFGS([sc], lr=1.0, max_iter=200, tolerance_grad=1e-14, tolerance_change=1e-16,
                            history_size=20, line_search_fn="strong_wolfe")

    def closure():
        opt.zero_grad()
        loss = loss_of(sc)
        loss.backward()
        return loss

    for _ in range(3):
        opt.step(closure)
    theta = (base_d * sc).detach().cpu().numpy()
    assert np.max(np.abs(theta - true) / np.abs(true)) <= 1e-3, (theta, true)
