"""GPU: the step VJPs' kernel (tds_vjp.hip) against the host instantiation of the same template and against w^T J of
the forward-mode kernel, the primal against forward_zero, step_fn(mode="reverse") (gradcheck, a chain of steps),
sharing of the handle's work buffer, and what is refused."""
import os

import numpy as np
import pytest

from conftest import ROOT

import tds_amd
from tds_amd import hip_backend as hb

pytestmark = pytest.mark.gpu

SUPPORTED = ["ant", "ant_floating", "laikago", "laikago_floating", "laikago_floating_env", "laikago_soft",
             "cartpole", "cartpole_plane", "pendulum5", "pendulum5_plane", "cube_floating"]


def records(name, n, seed=0):
    g = np.load(os.path.join(ROOT, "tests", "golden", f"{name}.npz"))
    rng = np.random.default_rng(seed)
    return g["x"][rng.integers(0, g["x"].shape[0], n)]


def sim_for(name, n, dtype="f64"):
    return hb.HipSim(tds_amd.load_model(name), n, device=0, dtype=dtype)


def rel(a, b):
    return float(np.max(np.abs(a - b)) / max(1.0, np.max(np.abs(b))))


def check_device_against_host(name, n, k, seed):
    import torch

    m = tds_amd.load_model(name)
    x = records(name, n, seed)
    w = np.random.default_rng(seed + 100).normal(size=(n, k, m.output_dim))
    sim = sim_for(name, n)
    xd = torch.from_numpy(x).cuda()
    y, wj = sim.vjp(xd, torch.from_numpy(w).cuda())
    y, wj = y.cpu().numpy(), wj.cpu().numpy()
    assert wj.shape == (n, k, m.input_dim) and np.all(np.isfinite(wj))
    idx = np.arange(n) if n <= 33 else np.r_[np.arange(8), np.arange(n - 8, n), np.arange(8, n, 509)]
    wj_h, y_h = hb.vjp_host(m, x[idx], w[idx], want_y=True)
    assert rel(wj[idx], wj_h) <= 1e-12
    assert np.max(np.abs(y[idx] - y_h) / np.maximum(np.abs(y_h), 1.0)) <= 1e-12
    y_fz = sim.forward_zero(xd).cpu().numpy()
    assert np.max(np.abs(y - y_fz) / np.maximum(np.abs(y_fz), 1.0)) <= 1e-10


@pytest.mark.parametrize("n", [1, 7, 4096])
@pytest.mark.parametrize("name", SUPPORTED)
def test_device_vjp_matches_host(name, n, built):
    check_device_against_host(name, n, 1, 0)


@pytest.mark.parametrize("name", SUPPORTED)
def test_device_vjp_matches_host_several_cotangents(name, built):
    check_device_against_host(name, 33, 3, 1)


@pytest.mark.parametrize("name", ["ant", "laikago", "cartpole_plane", "cube_floating"])
def test_device_vjp_is_w_times_device_jacobian(name, built):
    import torch

    n, k = 64, 2
    m = tds_amd.load_model(name)
    sim = sim_for(name, n)
    x = torch.from_numpy(records(name, n, 2)).cuda()
    w = torch.from_numpy(np.random.default_rng(4).normal(size=(n, k, m.output_dim))).cuda()
    _, wj = sim.vjp(x, w)
    ref = torch.einsum("nko,noi->nki", w, sim.jacobian(x))
    assert (torch.abs(wj - ref).max() / torch.clamp(torch.abs(ref).max(), min=1.0)).item() <= 1e-11
    y1, wj1 = sim.vjp(x, w[:, 0])
    assert wj1.shape == (n, m.input_dim)
    assert (torch.abs(wj1 - wj[:, 0]).max() / torch.clamp(torch.abs(wj[:, 0]).max(), min=1.0)).item() <= 1e-14


@pytest.mark.parametrize("name", ["cartpole", "ant"])
def test_gradcheck_of_step_fn_reverse(name, built):
    import torch

    n = 2
    m = tds_amd.load_model(name)
    sim = sim_for(name, n)
    x = torch.from_numpy(records(name, n, 7)).cuda()
    if m.step_mode == tds_amd.TDS_STEP_LOCOMOTION:  # actions well inside the clamp: a smooth state
        nq, nd = m.dof_q, m.dof_qd
        x[:, nq + nd:nq + nd + m.action_dim] *= 0.1
    x.requires_grad_(True)
    f = tds_amd.step_fn(sim, mode="reverse")
    assert torch.autograd.gradcheck(f, (x,), eps=1e-6, atol=1e-5, rtol=1e-4, nondet_tol=0.0)
    g_out = torch.from_numpy(np.random.default_rng(5).normal(size=(n, m.output_dim))).cuda()
    (g_rev,) = torch.autograd.grad(f(x), x, g_out)
    (g_fwd,) = torch.autograd.grad(tds_amd.step_fn(sim)(x), x, g_out)
    assert (torch.abs(g_rev - g_fwd).max() / torch.clamp(torch.abs(g_fwd).max(), min=1.0)).item() <= 1e-11


def test_step_fn_mode_is_checked(built):
    sim = sim_for("cartpole", 1)
    with pytest.raises(ValueError):
        tds_amd.step_fn(sim, mode="backward")


def test_backprop_through_a_chain_of_steps(built):
    """8 steps of ant x 256, chained by step_fn: next x = y's q | qd, fresh actions, the record's kp kd max_force"""
    import torch

    n, steps = 256, 8
    m = tds_amd.load_model("ant")
    nq, nd, na = m.dof_q, m.dof_qd, m.action_dim
    sim = sim_for("ant", n)
    x0_np = records("ant", n, 9)
    gains = torch.from_numpy(x0_np[:, nq + nd + na:]).cuda()
    rng = np.random.default_rng(12)
    acts_np = [0.3 * rng.normal(size=(n, na)) for _ in range(steps)]
    w_np = rng.normal(size=(n, nq + nd))

    def run(mode):
        f = tds_amd.step_fn(sim, mode=mode)
        x0 = torch.from_numpy(x0_np[:, :nq + nd].copy()).cuda().requires_grad_(True)
        acts = [torch.from_numpy(a).cuda().requires_grad_(True) for a in acts_np]
        s = x0
        for t in range(steps):
            y = f(torch.cat([s, acts[t], gains], dim=1))
            s = y[:, :nq + nd]
        loss = (s * torch.from_numpy(w_np).cuda()).sum() + (s[:, :nq] ** 2).sum()
        return torch.autograd.grad(loss, [x0] + acts)

    g_rev, g_fwd = run("reverse"), run("forward")
    for a, b in zip(g_rev, g_fwd):
        assert torch.isfinite(a).all()
        assert (torch.abs(a - b).max() / torch.clamp(torch.abs(b).max(), min=1.0)).item() <= 1e-9
    assert torch.count_nonzero(g_rev[0]) > 0 and torch.count_nonzero(g_rev[-1]) > 0


def test_work_buffer_is_shared_with_the_jacobians(built):
    import torch

    name, n = "ant", 40
    m = tds_amd.load_model(name)
    x = torch.from_numpy(records(name, n, 6)).cuda()
    w = torch.from_numpy(np.random.default_rng(8).normal(size=(n, 2, m.output_dim))).cuda()
    fresh_j = sim_for(name, n).jacobian(x)
    fresh_v = sim_for(name, n).vjp(x, w)
    sim = sim_for(name, n)
    j1 = sim.jacobian(x)
    y2, v2 = sim.vjp(x, w)
    j3 = sim.jacobian(x)
    assert torch.equal(j1, fresh_j) and torch.equal(j3, fresh_j)
    assert torch.equal(v2, fresh_v[1]) and torch.equal(y2, fresh_v[0])
    # n other than num_envs: more and fewer environments than the handle has
    for n2 in (n + 100, 5):
        x2 = torch.from_numpy(records(name, n2, 13)).cuda()
        w2 = torch.from_numpy(np.random.default_rng(n2).normal(size=(n2, 1, m.output_dim))).cuda()
        y_a, v_a = sim.vjp(x2, w2)
        y_b, v_b = sim_for(name, n2).vjp(x2, w2)
        assert torch.equal(v_a, v_b) and torch.equal(y_a, y_b)


def test_more_environments_than_lanes(built):
    """n = 4096 + 70: the lanes of the launch walk the environments twice"""
    import torch

    name, n = "cartpole_plane", 4096 + 70
    m = tds_amd.load_model(name)
    x = records(name, n, 14)
    w = np.random.default_rng(15).normal(size=(n, 1, m.output_dim))
    _, wj = sim_for(name, 8).vjp(torch.from_numpy(x).cuda(), torch.from_numpy(w).cuda())
    wj = wj.cpu().numpy()
    idx = np.r_[np.arange(4), np.arange(4090, 4100), np.arange(n - 4, n)]
    assert rel(wj[idx], hb.vjp_host(m, x[idx], w[idx])) <= 1e-12


def test_f32_handles_and_unsupported_models_are_refused(built):
    import torch

    for dtype in ("f32", "mixed"):
        sim = sim_for("ant", 4, dtype)
        x = torch.zeros((4, sim.input_dim), dtype=torch.float64, device="cuda")
        w = torch.zeros((4, sim.output_dim), dtype=torch.float64, device="cuda")
        with pytest.raises(hb.TdsHipError, match="f64"):
            sim.vjp(x, w)
    for name in ("humanoid_spherical", "pendulum5_spherical"):
        sim = sim_for(name, 4)
        x = torch.from_numpy(records(name, 4)).cuda()
        w = torch.zeros((4, sim.output_dim), dtype=torch.float64, device="cuda")
        with pytest.raises(hb.TdsHipError, match="spherical"):
            sim.vjp(x, w)
