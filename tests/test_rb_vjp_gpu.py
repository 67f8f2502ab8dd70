"""Reverse-mode derivatives of rigid-body rollouts on the MI355X (tds_rb_vjp): device against the host templates over
windows and passes, the primal, autograd in u, theta and s0, and the billiard shot: every input's gradient from one
reverse call, and the descent of test_rb_derivs_gpu.py driven through it."""
import numpy as np
import pytest

from conftest import rel_err
from rb_scenes import (BILLIARD_TARGET, BILLIARD_TARGET_BALL, MIXED_ORDER, WHITE, billiard_model, billiard_state,
                       make_mixed_worlds, make_worlds, shot_velocity)
from test_rb_vjp_cpu import REV_FWD_BOUND

import tds_amd
from tds_amd import hip_backend as hb

pytestmark = pytest.mark.gpu
PARAMS = [("mass", 2), ("gravity", 2), ("friction",), ("restitution",)]


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def budget_for(m, n, steps, p, cap, chunk, W):
    """the smallest work_bytes at which a call takes passes of `chunk` worlds and windows of W steps"""
    def reaches(b):
        try:
            return hb.rb_vjp_plan(m, n, steps, p, cap, b)[1:3] >= (chunk, W)
        except hb.TdsHipError:
            return False
    lo, hi = 1, hb.rb_vjp_plan(m, n, steps, p, cap)[3]
    while lo < hi:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if reaches(mid) else (mid + 1, hi)
    assert hb.rb_vjp_plan(m, n, steps, p, cap, lo)[1:3] == (chunk, W)
    return lo


@pytest.mark.parametrize("n", [1, 7, 70])
def test_rb_vjp_device_matches_host_over_windows_and_passes(n, built):
    import torch
    steps = 7
    m, s0 = make_worlds(n, 7)
    ns = m.num_bodies * 13
    sim = hb.RigidBodySim(m, 16)
    n64 = (n + 63) // 64 * 64
    for use_theta in (False, True):
        sel = PARAMS if use_theta else ()
        p = len(sel)
        th = hb.rb_params_get(m, sel) * (1 + 0.05 * np.random.default_rng(2).random((n, p))) if use_theta else None
        gs = np.random.default_rng(n).normal(size=(n, steps, ns))
        s_h, g0_h, gt_h = hb.rb_vjp_host(m, s0, steps, gs, sel, th, every=1)
        cap = hb.rb_vjp_plan(m, n, steps, p)[0]
        assert hb.rb_vjp_plan(m, n, steps, p)[1:3] == (n64, steps)          # the default: one pass, one window
        results = []
        for chunk, W in ((None, None), (n64, 3), (64, 1)):                    # windows 3, 3, 1; two passes at n = 70
            wb = 0 if chunk is None else budget_for(m, n, steps, p, cap, chunk, W)
            s_d, g0_d, gt_d = sim.vjp(_cuda(s0), _cuda(gs), steps, sel, None if th is None else _cuda(th), every=1,
                                      tape_cap=0 if chunk is None else cap, work_bytes=wb)
            results.append((s_d, g0_d, gt_d))
        s_d, g0_d, gt_d = results[0]
        for other in results[1:]:
            assert all(torch.equal(a, b) for a, b in zip(results[0], other))  # bit for bit
        e_s = rel_err(s_d.cpu().numpy(), s_h, 1e-2)
        e_g = rel_err(g0_d.cpu().numpy(), g0_h, 1e-2)
        e_t = rel_err(gt_d.cpu().numpy(), gt_h, 1e-2) if use_theta else 0.0
        print(f"n={n} theta={use_theta}: s {e_s:.2e}, gs0 {e_g:.2e}, gtheta {e_t:.2e}")
        assert e_s <= 1e-12 and e_g <= 1e-12 and e_t <= 1e-12
        assert gt_d.shape == (n, p)


def test_rb_vjp_one_step_and_mixed_scene(built):
    for m, s0, steps, sel in ((*make_worlds(7, 7), 1, PARAMS),
                              (*make_mixed_worlds(7, 21, MIXED_ORDER), 5,
                               [("mass", 3), ("gravity", 2), ("friction",), ("restitution",)])):
        n, ns = s0.shape[0], m.num_bodies * 13
        sim = hb.RigidBodySim(m, 4)
        th = hb.rb_params_get(m, sel) * (1 + 0.05 * np.random.default_rng(3).random((n, len(sel))))
        gs = np.random.default_rng(steps).normal(size=(n, 1, ns))
        s_h, g0_h, gt_h = hb.rb_vjp_host(m, s0, steps, gs, sel, th)
        s_d, g0_d, gt_d = sim.vjp(_cuda(s0), _cuda(gs), steps, sel, _cuda(th))
        errs = [rel_err(d.cpu().numpy(), h, 1e-2) for d, h in ((s_d, s_h), (g0_d, g0_h), (gt_d, gt_h))]
        print(f"{m.num_bodies} bodies, {steps} steps: s {errs[0]:.2e}, gs0 {errs[1]:.2e}, gtheta {errs[2]:.2e}")
        assert max(errs) <= 1e-12


def test_rb_vjp_primal_resident_state_and_refusals(built):
    import torch
    m, s0 = make_worlds(64, 7)
    ns = m.num_bodies * 13
    sim = hb.RigidBodySim(m, 64)
    sim.state.copy_(_cuda(s0))
    before = sim.state.clone()
    steps = 12
    s, g0, gt = sim.vjp(_cuda(s0), torch.zeros((64, 1, ns), dtype=torch.float64, device="cuda"), steps)
    assert torch.equal(s[:, 0], sim.jvp(_cuda(s0), None, steps)[0])
    assert torch.equal(sim.state, before)                # the resident state is not touched
    assert not g0.any() and gt.shape == (64, 0)          # a zero cotangent gives exact zeros
    s4 = sim.vjp(_cuda(s0), torch.zeros((64, 3, ns), dtype=torch.float64, device="cuda"), steps, every=4)[0]
    assert torch.equal(s4[:, 2], s[:, 0]) and torch.equal(s4[:, 0], sim.jvp(_cuda(s0), None, 4)[0])
    f32 = hb.RigidBodySim(m, 4, dtype="f32")
    with pytest.raises(hb.TdsHipError, match="f32"):
        f32.vjp(_cuda(s0[:4]), torch.zeros((4, 1, ns), dtype=torch.float64, device="cuda"), 1)
    with pytest.raises(hb.TdsHipError, match="every must divide steps"):
        sim.vjp(_cuda(s0), torch.zeros((64, 1, ns), dtype=torch.float64, device="cuda"), 6, every=4)
    with pytest.raises(hb.TdsHipError, match="one step of 64 worlds needs"):
        sim.vjp(_cuda(s0), torch.zeros((64, 1, ns), dtype=torch.float64, device="cuda"), 6, tape_cap=20000,
                work_bytes=1 << 20)
    # an overflowing capacity: NaN gradients, the states stand
    with pytest.raises(hb.TdsHipError, match="tape exceeds the capacity"):
        sim.vjp(_cuda(s0), torch.ones((64, 1, ns), dtype=torch.float64, device="cuda"), 6, tape_cap=100)
    # malformed tensors are refused in Python, before the library is called: N = 2, K = 2, steps = 2
    z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")  # noqa: E731
    s2, sel = _cuda(s0[:2]), [("mass", 1), ("friction",)]
    bad_s = (s2.float(), s2.cpu())
    bad_th = (z(2, 1), z(1, 2), z(2, 2).float(), z(2, 2).cpu())
    bad_v = (z(2, 2, ns + 3), z(3, 2, ns + 2), z(2, ns + 3), z(2, 2, 1, ns + 2), z(2, 2, ns + 2).float(),
             z(2, 2, ns + 2).cpu())
    bad_gs = (z(2, 2, ns), z(2, ns - 1), z(1, 1, ns), z(2, 1, ns).float(), z(2, 1, ns).cpu())
    refused = [lambda b=b: sim.jvp(b, None, 2) for b in bad_s]
    refused += [lambda b=b: sim.vjp(b, z(2, 1, ns), 2) for b in bad_s]
    refused += [lambda b=b: sim.jvp(s2, None, 2, sel, b) for b in bad_th]
    refused += [lambda b=b: sim.vjp(s2, z(2, 1, ns), 2, sel, b) for b in bad_th]
    refused += [lambda b=b: sim.jvp(s2, b, 2, sel) for b in bad_v]
    refused += [lambda b=b: sim.vjp(s2, b, 2) for b in bad_gs]
    refused.append(lambda: sim.vjp(s2, z(2, 1, ns), 2, every=1))
    for i, call in enumerate(refused):
        with pytest.raises(AssertionError):
            call()
            pytest.fail(f"refused[{i}] was accepted")


def test_rb_rollout_fn_reverse_gradcheck(built):
    import torch
    m, s0 = make_worlds(3, 7)
    sim = hb.RigidBodySim(m, 3)
    wrt = [(1, 7), (1, 8), (2, 9), (3, 2)]
    params = [("mass", 2), ("friction",)]
    f = tds_amd.rb_rollout_fn(sim, 10, wrt, params, mode="reverse")
    fwd = tds_amd.rb_rollout_fn(sim, 10, wrt, params)
    s = _cuda(s0)
    u = torch.stack([s[:, b, c] for b, c in wrt], 1).clone().requires_grad_(True)
    th = torch.tensor(hb.rb_params_get(m, params), dtype=torch.float64, device="cuda", requires_grad=True)
    assert torch.autograd.gradcheck(lambda uu, tt: f(s, uu, tt), (u, th), eps=1e-6, atol=1e-5, rtol=1e-4)
    thn = th.detach().expand(3, 2).clone().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda uu, tt: f(s, uu, tt), (u, thn), eps=1e-6, atol=1e-5, rtol=1e-4)
    sg = s.clone().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda ss, uu: f(ss, uu), (sg, u), eps=1e-6, atol=1e-5, rtol=1e-4)
    # both modes give the same gradients
    w = torch.from_numpy(np.random.default_rng(6).normal(size=(3, m.num_bodies, 13))).cuda()
    for theta in (th, thn):
        g_rev = torch.autograd.grad((f(s, u, theta) * w).sum(), (u, theta))
        g_fwd = torch.autograd.grad((fwd(s, u, theta) * w).sum(), (u, theta))
        for a, b in zip(g_rev, g_fwd):
            assert float((a - b).abs().max() / b.abs().max()) <= REV_FWD_BOUND
    assert torch.equal(f(s, u, th), fwd(s, u, th))
    # every: the intermediate states, differentiable
    f5 = tds_amd.rb_rollout_fn(sim, 10, wrt, params, mode="reverse", every=5)
    s5 = f5(s, u, th)
    assert s5.shape == (3, 2, m.num_bodies, 13) and torch.equal(s5[:, 1], f(s, u, th))
    (g5,) = torch.autograd.grad((s5[:, 1] * w).sum(), u)
    assert torch.equal(g5, g_rev[0])
    with pytest.raises(ValueError, match="mode"):
        tds_amd.rb_rollout_fn(sim, 10, wrt, params, mode="adjoint")


def test_billiard_every_gradient_from_one_reverse_call(built):
    import torch
    m = billiard_model()
    steps = 300
    sim = hb.RigidBodySim(m, 1)
    s0 = billiard_state(1)
    s0[:, WHITE, 7:9] = shot_velocity([[10.0, 600.0]])
    params = [("mass", b) for b in range(7)]
    s = _cuda(s0)
    sT = sim.jvp(s, None, steps)[0]
    gs = torch.zeros_like(sT)
    gs[0, BILLIARD_TARGET_BALL, :3] = 2 * (sT[0, BILLIARD_TARGET_BALL, :3] - _cuda(BILLIARD_TARGET))
    s_rec, gs0, gth = sim.vjp(s, gs, steps, params)                     # 91 + 7 gradients, one call
    assert torch.equal(s_rec[:, 0], sT)
    wrt = [(b, c) for b in range(7) for c in range(13)]
    J = sim.jacobian(s, steps, wrt, params)                             # [1, 91, 98]: 98 forward columns
    ref = (J[0] * gs.reshape(-1, 1)).sum(0)
    got = torch.cat([gs0.reshape(-1), gth.reshape(-1)])
    e = float((got - ref).abs().max() / ref.abs().max())
    print(f"billiard, 300 steps: 98 gradients of the cost, reverse against forward {e:.2e}")
    assert e <= REV_FWD_BOUND


def test_billiard_descent_through_reverse_mode(built):
    import torch
    m = billiard_model()
    steps = 300
    sim = hb.RigidBodySim(m, 1)
    # one world per shot; world 0 is the fixed shot, which moves ball 5 (test_billiard_gradient_and_descent's)
    rng = np.random.default_rng(0)
    forces = np.concatenate([[[10.0, 600.0]], rng.uniform([-100, 400], [100, 800], (63, 2))])
    n = forces.shape[0]
    s0 = billiard_state(n)
    s0[:, WHITE, 7:9] = shot_velocity(forces)
    wrt = [(WHITE, 7), (WHITE, 8)]
    f = tds_amd.rb_rollout_fn(sim, steps, wrt, mode="reverse")
    s = _cuda(s0)
    u = s[:, WHITE, 7:9].clone()
    tgt = torch.tensor([3.5, 8.0, 0.0], dtype=torch.float64, device="cuda")

    def cost(uu):
        return ((f(s, uu)[:, BILLIARD_TARGET_BALL, :3] - tgt) ** 2).sum(1)

    c0 = cost(u)[0].item()
    lr = torch.full((n, 1), 1.0, dtype=torch.float64, device="cuda")
    for _ in range(10):
        uu = u.clone().requires_grad_(True)
        c = cost(uu)
        (g,) = torch.autograd.grad(c.sum(), uu)
        with torch.no_grad():
            done = torch.zeros(n, dtype=torch.bool, device="cuda")
            for _ in range(8):                                      # backtracking per world
                cand = u - lr * g
                better = (cost(cand) < c) & ~done
                u = torch.where(better[:, None], cand, u)
                done |= better
                if bool(done.all()):
                    break
                lr = torch.where(done[:, None], lr, lr * 0.5)
    c1 = cost(u)[0].item()
    print(f"billiard descent through reverse mode, fixed shot: cost {c0:.4f} -> {c1:.4f}")
    assert c1 < 0.5 * c0
