"""GPU: the trajectory VJP's kernels (tds_traj_vjp.hip) against their host instantiation, windows and chunks,
the lane budget, consistency with the step and trajectory derivatives on one handle, trajectory_fn(mode="reverse")
(gradcheck, against chained param_step_fn(mode="reverse"), against forward mode), refusals and the tape bound."""
import ctypes as C
import functools

import numpy as np
import pytest

import tds_amd
from tds_amd import hip_backend as hb
import diff_states
from test_traj_derivs_gpu import DEV_TOL, SEL, records, starts, rel

pytestmark = pytest.mark.gpu

T = 12


def cuda(a):
    import torch

    return None if a is None else torch.from_numpy(np.array(a, dtype=np.float64, order="C")).cuda()  # (a writable copy)


@functools.lru_cache(maxsize=None)
def inputs(name, n, steps=T, every=1, seed=11):
    """(m, sel, x0, theta, u, gs): shared between the tests, read only"""
    m = tds_amd.load_model(name)
    sel = SEL[name]
    x = np.ascontiguousarray(starts(name, n, seed))
    rng = np.random.default_rng(seed + 1)
    th = hb.params_get(m, sel) * (1.0 + 0.01 * rng.uniform(-1, 1, (n, len(sel))))
    nsd, n_act, n_rec = hb.trajectory_dims(m, steps, every)
    u = rng.uniform(-0.2, 0.2, (n, steps - 1, n_act))
    gs = rng.normal(size=(n, n_rec, nsd))
    for a in (x, th, u, gs):
        a.setflags(write=False)
    return m, sel, x, th, u, gs


def device(sim, x, gs, steps, every, u, sel, th):
    return tuple(t.cpu().numpy() for t in sim.trajectory_vjp(cuda(x), cuda(gs), steps, every, cuda(u), sel, cuda(th)))


def worst_rel(dev, host, idx=None):
    """the largest per-environment relative difference over (s, gx0, gu, gtheta)"""
    worst = 0.0
    for d, h in zip(dev, host):
        d = d if idx is None else d[idx]
        for e in range(h.shape[0]):
            if h[e].size:
                worst = max(worst, rel(d[e], h[e]))
    return worst


@pytest.mark.parametrize("n", [1, 7, 130])
@pytest.mark.parametrize("name", ["ant", "laikago", "cube_floating", "pendulum5"])
def test_device_matches_host(name, n, built):
    m, sel, x, th, u, gs = inputs(name, n)
    sim = hb.HipSim(m, min(n, 64), device=0, dtype="f64")
    dev = device(sim, x, gs, T, 1, u, sel, th)
    host = hb.trajectory_vjp_host(m, x, gs, T, 1, u, sel, th)
    worst = worst_rel(dev, host)
    print(name, n, "max rel device-host", worst)
    assert worst <= DEV_TOL, worst
    s0 = sim.trajectory_jvp(cuda(x), None, T, 1, cuda(u), sel, cuda(th))[0].cpu().numpy()
    np.testing.assert_array_equal(dev[0], s0)
    assert np.count_nonzero(dev[1]) > 0 and np.all(np.isfinite(dev[1]))


def test_device_matches_host_without_u_every_3(built):
    name, n = "ant", 7
    m, sel, x, th, _, gs = inputs(name, n, T, 3)
    sim = hb.HipSim(m, n, device=0, dtype="f64")
    dev = device(sim, x, gs, T, 3, None, sel, th)
    host = hb.trajectory_vjp_host(m, x, gs, T, 3, None, sel, th)
    worst = worst_rel(dev, host)
    print(name, n, "u NULL, every 3: max rel device-host", worst)
    assert worst <= DEV_TOL, worst
    np.testing.assert_array_equal(dev[0], sim.trajectory_jvp(cuda(x), None, T, 3, None, sel, cuda(th))[0].cpu().numpy())
    nsd, n_act, _ = hb.trajectory_dims(m, T, 3)
    assert np.count_nonzero(dev[1][:, nsd:nsd + n_act]) > 0 and np.all(dev[2] == 0.0)


@functools.lru_cache(maxsize=None)
def default_plan_result(name):
    """trajectory_vjp of the windows-and-chunks case on a handle with both options unset: one chunk, the default window"""
    m, sel, x, th, u, gs = inputs(name, 130, T, 3)
    sim = hb.HipSim(m, 64, device=0, dtype="f64")
    return device(sim, x, gs, T, 3, u, sel, th)


@pytest.mark.parametrize("traj_steps", [1, 5, None])
@pytest.mark.parametrize("name", ["ant", "pendulum5"])
def test_windows_and_chunks_are_invisible(name, traj_steps, built):
    """traj_vjp_lanes 64, 128, unset: 3 chunks, 2 chunks, one chunk of the 130 environments; traj_steps 1, 5, unset:
    windows of 1, of 5 | 5 | 2 and the default where the lane budget has room for them"""
    m, sel, x, th, u, gs = inputs(name, 130, T, 3)
    ref = default_plan_result(name)
    sim = hb.HipSim(m, 64, device=0, dtype="f64")
    sim.set_option("traj_steps", traj_steps)
    for lanes in (64, 128, None):
        sim.set_option("traj_vjp_lanes", lanes)
        for a, b in zip(ref, device(sim, x, gs, T, 3, u, sel, th)):
            np.testing.assert_array_equal(a, b, err_msg=str((traj_steps, lanes)))


def test_past_the_default_lane_budget(built):
    name, n, steps = "pendulum5", 4166, 3
    m, sel, x, th, u, gs = inputs(name, n, steps)
    sim = hb.HipSim(m, 64, device=0, dtype="f64")
    dev = device(sim, x, gs, steps, 1, u, sel, th)
    idx = np.sort(np.concatenate([np.random.default_rng(1).choice(n, 60, replace=False), [0, 4095, 4096, n - 1]]))[:64]
    host = hb.trajectory_vjp_host(m, x[idx], gs[idx], steps, 1, u[idx], sel, th[idx])
    worst = worst_rel(dev, host, idx)
    print(name, n, "max rel device-host", worst)
    assert worst <= DEV_TOL, worst
    assert all(np.all(np.isfinite(d)) for d in dev)


def test_consistency_on_one_handle(built):
    import torch

    name, n = "ant", 16
    m, sel, x, th, u, gs = inputs(name, n)
    nsd, nin = m.dof_q + m.dof_qd, m.input_dim
    xd, thd, ud, gsd = (cuda(a) for a in (x, th, u, gs))
    sim = hb.HipSim(m, n, device=0, dtype="f64")
    # one step: the parameter VJP of the cotangent [gs | 0]
    w = torch.zeros((n, m.output_dim), dtype=torch.float64, device="cuda")
    w[:, :nsd] = gsd[:, 0]
    y, wj_x, wj_th = sim.vjp_params(xd, thd, sel, w)
    s1, gx1, _, gth1 = sim.trajectory_vjp(xd, gsd[:, :1].contiguous(), 1, 1, None, sel, thd)
    assert rel(gx1.cpu().numpy(), wj_x.cpu().numpy()) <= 1e-12
    assert rel(gth1.cpu().numpy(), wj_th.cpu().numpy()) <= 1e-12
    assert rel(s1[:, 0].cpu().numpy(), y[:, :nsd].cpu().numpy()) <= 1e-12
    # the whole trajectory: gs^T (d s / d [x0 | theta]) from forward mode
    s, gx0, gu, gth = sim.trajectory_vjp(xd, gsd, T, 1, ud, sel, thd)
    jac = sim.trajectory_jacobian(xd, T, range(nin), sel, thd, 1, ud)  # [n, T nsd, nin + p]
    ref = torch.bmm(gsd.reshape(n, 1, -1), jac).squeeze(1).cpu().numpy()
    got = torch.cat([gx0, gth], dim=1).cpu().numpy()
    worst = max(rel(got[e], ref[e]) for e in range(n))
    print("reverse against forward on the device", worst)
    assert worst <= 1e-10, worst
    # interleaved on one handle (one work buffer) = fresh handles
    wj_a = sim.vjp(xd, w)
    wj_a = wj_a[1] if isinstance(wj_a, tuple) else wj_a
    again = sim.trajectory_vjp(xd, gsd, T, 1, ud, sel, thd)
    s_j, js_j = sim.trajectory_jvp(xd, jac.new_ones((n, 2, nin + len(sel))), T, 1, ud, sel, thd)
    again2 = sim.trajectory_vjp(xd, gsd, T, 1, ud, sel, thd)
    fresh = [hb.HipSim(m, n, device=0, dtype="f64") for _ in range(3)]
    wj_f = fresh[0].vjp(xd, w)
    wj_f = wj_f[1] if isinstance(wj_f, tuple) else wj_f
    assert torch.equal(wj_a, wj_f)
    for a, b, c in zip(again, again2, fresh[1].trajectory_vjp(xd, gsd, T, 1, ud, sel, thd)):
        assert torch.equal(a, c) and torch.equal(b, c)
    s_f, js_f = fresh[2].trajectory_jvp(xd, jac.new_ones((n, 2, nin + len(sel))), T, 1, ud, sel, thd)
    assert torch.equal(s_j, s_f) and torch.equal(js_j, js_f) and torch.equal(s, s_f)


def test_gradcheck_of_reverse_mode_trajectory_fn(built):
    import torch

    m = tds_amd.load_model("pendulum5")
    n, sel, steps = 2, SEL["pendulum5"], 6
    sim = hb.HipSim(m, n, device=0, dtype="f64")
    x0 = torch.from_numpy(records("pendulum5", n, 4)).cuda()
    wrt = [0, 3, 6]
    f = tds_amd.trajectory_fn(sim, steps, wrt, sel, every=2, mode="reverse")
    z = x0[:, wrt].clone().requires_grad_(True)
    base = hb.params_get(m, sel) + np.array([0.0, 0.5])
    th1 = torch.from_numpy(base).cuda().requires_grad_(True)
    thn = torch.from_numpy(np.stack([base, base * 1.01])).cuda().requires_grad_(True)
    n_act = hb.trajectory_dims(m, steps)[1]
    u = torch.from_numpy(np.random.default_rng(5).uniform(-0.2, 0.2, (n, steps - 1, n_act))).cuda().requires_grad_(True)
    for th in (thn, th1):
        assert torch.autograd.gradcheck(lambda zz, tt, uu: f(x0, zz, tt, uu), (z, th, u), eps=1e-6, atol=1e-5,
                                        rtol=1e-4)
    with pytest.raises(ValueError, match="wrt"):
        f(x0.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="mode"):
        tds_amd.trajectory_fn(sim, steps, wrt, sel, mode="adjoint")


def test_action_and_parameter_gradients_match_chained_reverse_mode_on_the_ant(built):
    import torch

    name, n, steps = "ant", 64, 16
    m = tds_amd.load_model(name)
    sel = [("gravity", 2), ("friction",), ("mass", 2), ("mass", 5)]
    sim = hb.HipSim(m, n, device=0, dtype="f64")
    x0 = torch.from_numpy(np.ascontiguousarray(starts(name, n, 5))).cuda()
    nsd, n_act, _ = hb.trajectory_dims(m, steps)
    theta0 = torch.from_numpy(hb.params_get(m, sel)).cuda()
    rng = np.random.default_rng(6)
    w = torch.from_numpy(rng.normal(size=(n, steps, nsd))).cuda()
    u0 = torch.from_numpy(rng.uniform(-0.2, 0.2, (n, steps - 1, n_act))).cuda()
    th, u = theta0.clone().requires_grad_(True), u0.clone().requires_grad_(True)
    s = tds_amd.trajectory_fn(sim, steps, (), sel, mode="reverse")(x0, None, th, u)
    g_th, g_u = torch.autograd.grad((w * s).sum(), (th, u))
    th2, u2 = theta0.clone().requires_grad_(True), u0.clone().requires_grad_(True)
    f = tds_amd.param_step_fn(sim, sel, mode="reverse")
    x, loss = x0, 0.0
    for t in range(steps):
        y = f(x, th2)
        loss = loss + (w[:, t] * y[:, :nsd]).sum()
        if t + 1 < steps:
            x = torch.cat([y[:, :nsd], u2[:, t], x0[:, nsd + n_act:]], dim=1)
    r_th, r_u = torch.autograd.grad(loss, (th2, u2))
    e_th, e_u = rel(g_th.cpu().numpy(), r_th.cpu().numpy()), rel(g_u.cpu().numpy(), r_u.cpu().numpy())
    print("ant x 64, T = 16: fused against chained reverse mode, theta", e_th, "u", e_u)
    assert e_th <= 1e-10 and e_u <= 1e-10, (e_th, e_u)
    assert torch.count_nonzero(g_th) == len(sel) and torch.count_nonzero(g_u) > 0
    counts = diff_states.contact_counts(name, m, x0.cpu().numpy()[:32], reference=False)
    assert counts.max() > 0  # contacts are active


def test_forward_and_reverse_mode_trajectory_fn_agree(built):
    import torch

    name, n = "ant", 7
    m, sel, x, th, u, gs = inputs(name, n, T, 3)
    sim = hb.HipSim(m, n, device=0, dtype="f64")
    x0, ud, w = cuda(x), cuda(u), cuda(gs)
    wrt = [0, 2, 9, m.input_dim - 1]
    grads = {}
    for mode in ("forward", "reverse"):
        z = x0[:, wrt].clone().requires_grad_(True)
        thd = cuda(th).requires_grad_(True)
        s = tds_amd.trajectory_fn(sim, T, wrt, sel, every=3, mode=mode)(x0, z, thd, ud)
        grads[mode] = [g.cpu().numpy() for g in torch.autograd.grad((w * s).sum(), (z, thd))]
    for a, b in zip(grads["forward"], grads["reverse"]):
        assert rel(a, b) <= 1e-10, rel(a, b)
        assert np.count_nonzero(b) > 0


def test_refusals_and_the_tape_bound(built):
    import torch
    from test_diff_sweep_cpu import ANT_PGS_OVERFLOW

    name, n = "ant", 16
    m, sel, x, th, u, gs = inputs(name, n)
    xd, gsd = cuda(x), cuda(gs)
    sim = hb.HipSim(m, n, device=0, dtype="f64")
    for dt in ("f32", "mix"):
        try:
            s32 = hb.HipSim(m, 4, device=0, dtype=dt)
        except (hb.TdsHipError, ValueError, KeyError):
            continue
        with pytest.raises(hb.TdsHipError, match="f64"):
            s32.trajectory_vjp(xd[:4], gsd[:4, :3].contiguous(), 3)
    with pytest.raises(hb.TdsHipError, match="tds_hip error 1:"):
        sim.trajectory_vjp(xd, gsd[:, :1].contiguous(), 6, 4)
    with pytest.raises(hb.TdsHipError, match="tds_hip error 1:"):
        sim.trajectory_vjp(xd, gsd[:, :1].contiguous(), 0, 1)
    with pytest.raises(hb.TdsHipError, match="spherical"):
        ms = tds_amd.load_model("pendulum5_spherical")
        s2 = hb.HipSim(ms, 2, device=0, dtype="f64")
        s2.trajectory_vjp(torch.from_numpy(records("pendulum5_spherical", 2)).cuda(),
                          torch.zeros((2, 3, ms.dof_q + ms.dof_qd), dtype=torch.float64, device="cuda"), 3)
    # malformed tensors are refused in Python, before the library is called: N = 2, K = 2, steps = 2
    mp, selp, xp, thp, up, gp = inputs("pendulum5", 2, 2)
    sp = hb.HipSim(mp, 2, device=0, dtype="f64")
    nin, nout, p, nsd = mp.input_dim, mp.output_dim, len(selp), gp.shape[2]
    n_act, P = up.shape[2], hb.policy_network_spec(mp)[4]
    z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")  # noqa: E731
    xg, tg, pol = cuda(xp), cuda(thp), z(P)
    bad_x = (z(2, nin + 1), z(2, 1, nin), xg.float(), xg.cpu())
    bad_th = (z(2, p + 1), z(1, p), tg.float(), tg.cpu())
    bad_v = (z(2, 2, nin + p + 1), z(3, 2, nin + p), z(2, nin + p + 1), z(2, 2, nin + p).float(), z(2, 2, nin + p).cpu())
    bad_w = (z(2, 2, nout + 1), z(3, 2, nout), z(2, nout + 1), z(2, 2, nout).float(), z(2, 2, nout).cpu())
    bad_u = (z(2, 2, n_act), z(2, 1, n_act + 1), z(1, 1, n_act), z(2, 1, n_act).float(), z(2, 1, n_act).cpu())
    bad_gs = (z(2, 1, nsd), z(2, 2, nsd + 1), z(1, 2, nsd), z(2, 2, nsd).float(), z(2, 2, nsd).cpu())
    bad_ga = (z(2, 1, n_act), z(2, 2, n_act + 1), z(1, 2, n_act), z(2, 2, n_act).float(), z(2, 2, n_act).cpu())
    bad_pol = (z(P + 1), z(1, P), z(2, P - 1), pol.float(), pol.cpu())
    bad_y = (z(2, nout + 1), z(1, nout), z(2, nout).float(), z(2, nout).cpu(), z(nout, 2).t())
    refused = [lambda b=b: sp.jvp(b, z(2, 2, nin)) for b in bad_x]
    refused += [lambda b=b: sp.jacobian(b) for b in bad_x]
    refused += [lambda b=b: sp.vjp(b, z(2, 2, nout)) for b in bad_x]
    refused += [lambda b=b: sp.jvp_params(b, tg, selp) for b in bad_x]
    refused += [lambda b=b: sp.vjp_params(b, tg, selp, z(2, 2, nout)) for b in bad_x]
    refused += [lambda b=b: sp.trajectory_jvp(b, None, 2) for b in bad_x]
    refused += [lambda b=b: sp.trajectory_vjp(b, z(2, 2, nsd), 2) for b in bad_x]
    refused += [lambda b=b: sp.policy_trajectory_vjp(b, pol, z(2, 2, nsd), 2) for b in bad_x]
    refused += [lambda b=b: sp.jacobian(xg, y=b) for b in bad_y]
    refused += [lambda b=b: sp.vjp(xg, z(2, 2, nout), y=b) for b in bad_y]
    refused += [lambda b=b: sp.jvp(xg, b) for b in (z(2, 2, nin + 1), z(3, 2, nin), z(2, nin + 1), z(2, 2, nin).float())]
    refused += [lambda b=b: sp.jvp_params(xg, tg, selp, b) for b in bad_v]
    refused += [lambda b=b: sp.trajectory_jvp(xg, b, 2, params=selp, theta=tg) for b in bad_v]
    refused += [lambda b=b: sp.vjp(xg, b) for b in bad_w]
    refused += [lambda b=b: sp.vjp_params(xg, tg, selp, b) for b in bad_w]
    refused += [lambda b=b: sp.jvp_params(xg, b, selp) for b in bad_th]
    refused += [lambda b=b: sp.vjp_params(xg, b, selp, z(2, 2, nout)) for b in bad_th]
    refused += [lambda b=b: sp.trajectory_jvp(xg, None, 2, params=selp, theta=b) for b in bad_th]
    refused += [lambda b=b: sp.trajectory_vjp(xg, z(2, 2, nsd), 2, params=selp, theta=b) for b in bad_th]
    refused += [lambda b=b: sp.policy_trajectory_vjp(xg, pol, z(2, 2, nsd), 2, params=selp, theta=b) for b in bad_th]
    refused += [lambda b=b: sp.trajectory_jvp(xg, None, 2, u=b) for b in bad_u]
    refused += [lambda b=b: sp.trajectory_vjp(xg, z(2, 2, nsd), 2, u=b) for b in bad_u]
    refused += [lambda b=b: sp.trajectory_vjp(xg, b, 2) for b in bad_gs]
    refused += [lambda b=b: sp.policy_trajectory_vjp(xg, pol, b, 2) for b in bad_gs]
    refused += [lambda b=b: sp.policy_trajectory_vjp(xg, pol, None, 2, ga=b) for b in bad_ga]
    refused += [lambda b=b: sp.policy_trajectory_vjp(xg, b, z(2, 2, nsd), 2) for b in bad_pol]
    for i, call in enumerate(refused):
        with pytest.raises(AssertionError):
            call()
            pytest.fail(f"refused[{i}] was accepted")
    # one PGS iteration past class A's range, every parameter selected: some tapes of the contact sweep exceed the bound
    mo = m.copy()
    mo.pgs_iterations = ANT_PGS_OVERFLOW
    so = hb.HipSim(mo, n, device=0, dtype="f64")
    so.set_option("traj_steps", 1)  # two windows: the later step's gu row is written before the earlier step overflows
    sel_all = hb.all_params(mo)
    p = len(sel_all)
    tha = hb.params_get(mo, sel_all)
    with pytest.raises(hb.TdsHipError, match="tds_hip error 2:.*tape exceeds the capacity"):
        so.trajectory_vjp(xd, gsd[:, :2].contiguous(), 2, 1, cuda(u[:, :1]), sel_all, cuda(tha))
    # the raw call: NaN gradients for exactly the environments whose tapes overflow on the host, the rest as the host's
    nsd, n_act, _ = hb.trajectory_dims(mo, 2)
    g2, u1, thd = gsd[:, :2].contiguous(), cuda(u[:, :1]), cuda(np.broadcast_to(tha, (n, p)))
    sd = torch.zeros((n, 2, nsd), dtype=torch.float64, device="cuda")
    gx0, gu, gth = (torch.zeros(shape, dtype=torch.float64, device="cuda")
                    for shape in ((n, mo.input_dim), (n, 1, n_act), (n, p)))
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    rc = hb.lib().tds_hip_trajectory_vjp(so.h, n, 2, 1, vp(xd), vp(u1), p, hb.param_spec(sel_all), vp(thd), vp(g2),
                                         vp(sd), vp(gx0), vp(gu), vp(gth))
    assert rc == 2  # TDS_ERR_UNSUPPORTED
    # (the host's tape lengths at the class's bound, by the raw call: -1 where a step's tape overflows)
    hs, hgx, hgu, hgt = np.zeros((n, 2, nsd)), np.zeros((n, mo.input_dim)), np.zeros((n, 1, n_act)), np.zeros((n, p))
    lens = np.zeros((n, 2), dtype=np.int32)
    tha_n, g2_h, u1_h = (np.ascontiguousarray(a) for a in (np.broadcast_to(tha, (n, p)), gs[:, :2], u[:, :1]))
    rc = hb.lib().tds_hip_trajectory_vjp_host(C.byref(mo), n, 2, 1, x.ctypes.data, u1_h.ctypes.data, p,
                                              hb.param_spec(sel_all), tha_n.ctypes.data, g2_h.ctypes.data,
                                              hs.ctypes.data, hgx.ctypes.data, hgu.ctypes.data, hgt.ctypes.data, 0,
                                              lens.ctypes.data)
    assert rc == 2
    over = (lens < 0).any(axis=1)
    assert 0 < over.sum() < n, lens
    fit = np.flatnonzero(~over)
    host = hb.trajectory_vjp_host(mo, x[fit], gs[fit, :2], 2, 1, u[fit, :1], sel_all, tha)
    for k, (d, h) in enumerate(zip((sd, gx0, gu, gth), host)):
        d = d.cpu().numpy()
        assert np.all(np.isfinite(d[fit])) and max(rel(d[e], h[i]) for i, e in enumerate(fit)) <= DEV_TOL
        assert np.all(np.isnan(d[over])) if k > 0 else np.all(np.isfinite(d[over]))  # the states stay
