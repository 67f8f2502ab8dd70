"""GPU: the parameter derivatives' kernels (tds_dparam.hip) against their host instantiations, at the blob's values
against forward_zero / HipSim.vjp / HipSim.jacobian, param_step_fn (gradcheck, both modes), and system
identification of a pendulum's link masses and lengths through chained steps (examples/pendulum_sys_id.cpp)."""
import os
import time

import numpy as np
import pytest

from conftest import ROOT

import tds_amd
from tds_amd import hip_backend as hb

pytestmark = pytest.mark.gpu

MODELS = ["ant", "laikago", "ant_floating", "pendulum5_plane"]


def records(name, n, seed=0):
    g = np.load(os.path.join(ROOT, "tests", "golden", f"{name}.npz"))
    rng = np.random.default_rng(seed)
    return g["x"][rng.integers(0, g["x"].shape[0], n)]


def rel(a, b):
    return float(np.max(np.abs(a - b)) / max(1.0, np.max(np.abs(b))))


def thetas(m, sel, n, seed):
    """per-environment theta near the blob's values (inertias scaled only: M stays positive definite)"""
    base = hb.params_get(m, sel)
    rng = np.random.default_rng(seed)
    additive = np.array([not q[0].endswith("inertia") for q in sel])
    return base * (1.0 + 0.02 * rng.uniform(-1, 1, (n, len(sel)))) + 0.005 * rng.uniform(-1, 1, (n, len(sel))) * additive


def check_device_against_host(name, n, k, seed):
    import torch

    m = tds_amd.load_model(name)
    sel = hb.all_params(m)
    nin, p = m.input_dim, len(sel)
    x = records(name, n, seed)
    th = thetas(m, sel, n, seed + 1)
    rng = np.random.default_rng(seed + 2)
    v = rng.normal(size=(n, k, nin + p))
    w = rng.normal(size=(n, k, m.output_dim))
    sim = hb.HipSim(m, n, device=0, dtype="f64")
    xd, thd = torch.from_numpy(x).cuda(), torch.from_numpy(th).cuda()
    y_f, jv = sim.jvp_params(xd, thd, sel, torch.from_numpy(v).cuda())
    y_r, wjx, wjt = sim.vjp_params(xd, thd, sel, torch.from_numpy(w).cuda())
    y_f, jv, y_r = y_f.cpu().numpy(), jv.cpu().numpy(), y_r.cpu().numpy()
    wj = np.concatenate([wjx.cpu().numpy(), wjt.cpu().numpy()], axis=2)
    assert jv.shape == (n, k, m.output_dim) and wj.shape == (n, k, nin + p)
    assert np.all(np.isfinite(jv)) and np.all(np.isfinite(wj))
    idx = np.arange(n) if n <= 33 else np.r_[np.arange(8), np.arange(n - 8, n), np.arange(8, n, 509)]
    jv_h, y_h = hb.jvp_params_host(m, x[idx], th[idx], sel, v[idx], want_y=True)
    wj_h = hb.vjp_params_host(m, x[idx], th[idx], sel, w[idx])
    assert rel(jv[idx], jv_h) <= 1e-12
    assert rel(wj[idx], wj_h) <= 1e-12
    for y in (y_f, y_r):
        assert rel(y[idx], y_h) <= 1e-12
    y_only = sim.jvp_params(xd, thd, sel).cpu().numpy()  # k = 0: the double step over a double overlay
    assert rel(y_only[idx], y_h) <= 1e-12
    assert rel(y_only, y_f) <= 1e-12


@pytest.mark.parametrize("n", [1, 7, 4096])
@pytest.mark.parametrize("name", MODELS)
def test_device_matches_host(name, n, built):
    check_device_against_host(name, n, 1, 0)


@pytest.mark.parametrize("name", MODELS)
def test_device_matches_host_several_directions(name, built):
    check_device_against_host(name, 33, 3, 1)


def test_more_environments_than_lanes(built):
    """n = 4096 + 70: two chunks of the reverse mode"""
    check_device_against_host("cartpole_plane", 4096 + 70, 1, 3)


@pytest.mark.parametrize("name", MODELS)
def test_at_blob_values_equal_the_plain_paths(name, built):
    import torch

    n, k = 40, 2
    m = tds_amd.load_model(name)
    sel = hb.all_params(m)
    nin, p = m.input_dim, len(sel)
    sim = hb.HipSim(m, n, device=0, dtype="f64")
    x = torch.from_numpy(records(name, n, 5)).cuda()
    theta = torch.from_numpy(hb.params_get(m, sel)).cuda()  # [p]: every environment
    w = torch.from_numpy(np.random.default_rng(6).normal(size=(n, k, m.output_dim))).cuda()

    def close(a, b, tol=1e-12):
        return (torch.abs(a - b).max() / torch.clamp(torch.abs(b).max(), min=1.0)).item() <= tol

    y = sim.jvp_params(x, theta, sel)
    y_r, wjx, _ = sim.vjp_params(x, theta, sel, w)
    y_v, wj0 = sim.vjp(x, w)
    assert close(y, y_v) and close(y_r, y_v) and close(wjx, wj0)
    # forward_zero runs the step kernels (pendulum5_plane: the serial-chain kernel), which round differently from
    # the template: the bound of the plain derivatives' primal checks
    y_fz = sim.forward_zero(x)
    assert (torch.abs(y - y_fz) / torch.clamp(torch.abs(y_fz), min=1.0)).max().item() <= 1e-10
    v = torch.zeros((n, nin, nin + p), dtype=torch.float64, device="cuda")
    v[:, :, :nin] = torch.eye(nin, dtype=torch.float64, device="cuda")
    _, jv = sim.jvp_params(x, theta, sel, v)
    assert close(jv.transpose(1, 2), sim.jacobian(x))


def test_selection_errors_and_refusals(built):
    import torch

    sim = hb.HipSim(tds_amd.load_model("ant"), 4, device=0, dtype="f64")
    x = torch.from_numpy(records("ant", 4)).cuda()
    th = torch.zeros(1, dtype=torch.float64, device="cuda")
    w = torch.zeros((4, sim.output_dim), dtype=torch.float64, device="cuda")
    for sel in ([("base_mass",)], [("mass", 14)], [("com", 1, 3)]):
        with pytest.raises(hb.TdsHipError, match="tds_hip error 1:"):
            sim.jvp_params(x, th, sel)
        with pytest.raises(hb.TdsHipError, match="tds_hip error 1:"):
            sim.vjp_params(x, th, sel, w)
    with pytest.raises(hb.TdsHipError, match="tds_hip error 1:.*duplicate"):
        sim.vjp_params(x, torch.zeros(2, dtype=torch.float64, device="cuda"), [("mass", 1), ("mass", 1)], w)
    for name, match in (("pendulum5_spherical", "spherical"), ("two_cubes_floating", "several bodies")):
        s2 = hb.HipSim(tds_amd.load_model(name), 2, device=0, dtype="f64")
        x2 = torch.from_numpy(records(name, 2)).cuda()
        w2 = torch.zeros((2, s2.output_dim), dtype=torch.float64, device="cuda")
        with pytest.raises(hb.TdsHipError, match=match):
            s2.vjp_params(x2, th, [("mass", 0)], w2)
        with pytest.raises(hb.TdsHipError, match=match):
            s2.jvp_params(x2, th, [("mass", 0)])
    s3 = hb.HipSim(tds_amd.load_model("ant"), 4, device=0, dtype="f32")
    with pytest.raises(hb.TdsHipError, match="f64"):
        s3.jvp_params(x, th, [("mass", 0)])


GRAD_SEL = [("mass", 1), ("mass", 3), ("com", 2, 1), ("inertia", 4, 2), ("xt_trans", 3, 1), ("stiffness", 2),
            ("damping", 4), ("gravity", 2)]


@pytest.mark.parametrize("mode", ["reverse", "forward"])
def test_gradcheck_of_param_step_fn(mode, built):
    """pendulum5: no plane, no contacts; theta [N, p] and theta [p] shared by the environments"""
    import torch

    n = 2
    m = tds_amd.load_model("pendulum5")
    sim = hb.HipSim(m, n, device=0, dtype="f64")
    f = tds_amd.param_step_fn(sim, GRAD_SEL, mode=mode)
    x = torch.from_numpy(records("pendulum5", n, 7)).cuda().requires_grad_(True)
    base = hb.params_get(m, GRAD_SEL) + np.array([0, 0, 0, 0, 0, 0.5, 0.1, 0])  # nonzero springs
    th1 = torch.from_numpy(base).cuda().requires_grad_(True)
    thn = torch.from_numpy(np.stack([base, base * 1.01])).cuda().requires_grad_(True)
    for th in (thn, th1):
        assert torch.autograd.gradcheck(f, (x, th), eps=1e-6, atol=1e-5, rtol=1e-4, nondet_tol=0.0)


def test_forward_and_reverse_modes_agree_on_ant(built):
    import torch

    n = 16
    m = tds_amd.load_model("ant")
    sel = hb.all_params(m)
    sim = hb.HipSim(m, n, device=0, dtype="f64")
    x = torch.from_numpy(records("ant", n, 8)).cuda()
    th = torch.from_numpy(hb.params_get(m, sel)).cuda()
    g_out = torch.from_numpy(np.random.default_rng(9).normal(size=(n, m.output_dim))).cuda()
    grads = {}
    for mode in ("reverse", "forward"):
        xr, tr = x.clone().requires_grad_(True), th.clone().requires_grad_(True)
        y = tds_amd.param_step_fn(sim, sel, mode=mode)(xr, tr)
        grads[mode] = torch.autograd.grad(y, [xr, tr], g_out)
    for a, b in zip(grads["reverse"], grads["forward"]):
        assert (torch.abs(a - b).max() / torch.clamp(torch.abs(b).max(), min=1.0)).item() <= 1e-11
    assert torch.count_nonzero(grads["reverse"][1]) > 0


def test_param_step_fn_mode_is_checked(built):
    sim = hb.HipSim(tds_amd.load_model("cartpole"), 1, device=0, dtype="f64")
    with pytest.raises(ValueError):
        tds_amd.param_step_fn(sim, [("mass", 0)], mode="backward")


# ---------------------------------------------------------------- system identification (pendulum_sys_id.cpp)
SYSID_SEL = [("mass", i) for i in range(5)] + [("xt_trans", i, 1) for i in range(1, 5)]  # masses, link lengths
SYSID_T, SYSID_N = 60, 8


def sysid_setup():
    m = tds_amd.load_model("pendulum5")
    base = hb.params_get(m, SYSID_SEL)
    true = base * np.array([1.3, 0.8, 1.2, 0.9, 1.1, 1.15, 0.85, 1.1, 0.9])
    rng = np.random.default_rng(11)
    nq = m.dof_q
    s0 = np.concatenate([rng.uniform(-1.0, 1.0, (SYSID_N, nq)), rng.uniform(-2.0, 2.0, (SYSID_N, nq))], axis=1)
    taus = rng.uniform(-3.0, 3.0, (SYSID_T, SYSID_N, nq))  # torques: the masses are identifiable
    return m, base, true, s0, taus


def host_rollout(m, theta, s0, taus):
    """q of every step of the host template's rollout at theta"""
    s, qs = s0, []
    nq = m.dof_q
    for t in range(SYSID_T):
        y = hb.jvp_params_host(m, np.concatenate([s, taus[t]], axis=1), theta, SYSID_SEL)
        s = y[:, :2 * nq]
        qs.append(s[:, :nq])
    return np.stack(qs)


def test_system_identification_of_a_pendulum(built):
    import torch

    t_start = time.time()
    m, base, true, s0, taus = sysid_setup()
    nq = m.dof_q
    target = torch.from_numpy(host_rollout(m, true, s0, taus)).cuda()
    sim = hb.HipSim(m, SYSID_N, device=0, dtype="f64")
    f = tds_amd.param_step_fn(sim, SYSID_SEL, mode="reverse")
    s0_d, taus_d, base_d = torch.from_numpy(s0).cuda(), torch.from_numpy(taus).cuda(), torch.from_numpy(base).cuda()

    def loss_of(scale):  # theta = base * scale: the unknowns are of order one
        theta, s, loss = base_d * scale, s0_d, 0.0
        for t in range(SYSID_T):
            y = f(torch.cat([s, taus_d[t]], dim=1), theta)
            s = y[:, :2 * nq]
            loss = loss + ((s[:, :nq] - target[t]) ** 2).sum()
        return loss

    def host_loss(scale):
        return float(((host_rollout(m, base * scale, s0, taus) - target.cpu().numpy()) ** 2).sum())

    # the rollout loss's gradient against central differences of host rollouts
    scale0 = np.ones(len(SYSID_SEL))
    sc = torch.from_numpy(scale0).cuda().requires_grad_(True)
    (g,) = torch.autograd.grad(loss_of(sc), sc)
    g = g.cpu().numpy()
    g_fd = np.zeros_like(g)
    for j in range(len(g)):
        h = 1e-6
        e = np.zeros_like(scale0)
        e[j] = h
        g_fd[j] = (host_loss(scale0 + e) - host_loss(scale0 - e)) / (2 * h)
    assert np.max(np.abs(g - g_fd)) / np.max(np.abs(g_fd)) <= 1e-6, (g, g_fd)

    # a plain torch optimiser recovers theta*
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
    assert time.time() - t_start < 60.0
