"""Forward-mode derivatives of rigid-body rollouts on the MI355X (tds_rb_jvp): device against the host template,
primal against RigidBodySim.step, autograd, and the reference's billiard shot optimised on the GPU gradient."""
import numpy as np
import pytest

import reflib
from conftest import rel_err
from rb_scenes import (BILLIARD_TARGET_BALL, MIXED_ORDER, WHITE, billiard_cost, billiard_model, billiard_state,
                       make_mixed_worlds, make_worlds, shot_velocity)

import tds_amd
from tds_amd import hip_backend as hb

pytestmark = pytest.mark.gpu
SHOT = (6 * 13 + 7, 6 * 13 + 8)


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("scene", ["plane_first", "plane_last", "mixed"])
def test_rb_jvp_device_matches_host_tumbling(scene, built):
    import torch
    steps = 40 if scene == "mixed" else 120             # test_rigid_bodies.py's horizons: 40 and 120 steps
    for n in (1, 7, 1000):
        if scene == "mixed":
            m, s0 = make_mixed_worlds(n, 21, MIXED_ORDER)
            params = [("mass", 3), ("gravity", 2), ("friction",), ("restitution",)]
        else:
            m, s0 = make_worlds(n, 7, plane_last=scene == "plane_last")
            params = [("mass", 2), ("gravity", 2), ("friction",), ("restitution",)]
        ns = m.num_bodies * 13
        sim = hb.RigidBodySim(m, 16)
        for use_theta in (False, True):
            p = len(params) if use_theta else 0
            sel = params if use_theta else ()
            v = np.random.default_rng(n).normal(size=(n, 5, ns + p))
            th = hb.rb_params_get(m, sel) * (1 + 0.05 * np.random.default_rng(2).random((n, p))) if use_theta else None
            sT_h, jv_h = hb.rb_jvp_host(m, s0, steps, v, sel, th)
            sT_d, jv_d = sim.jvp(_cuda(s0), _cuda(v), steps, sel, None if th is None else _cuda(th))
            torch.cuda.synchronize()
            e_s = rel_err(sT_d.cpu().numpy(), sT_h, 1e-2)
            e_j = rel_err(jv_d.cpu().numpy(), jv_h, 1e-2)
            print(f"{scene} n={n} theta={use_theta}: s_T {e_s:.2e}, jv {e_j:.2e}")
            assert e_s <= 1e-12 and e_j <= 1e-12


def test_rb_jvp_primal_and_resident_state(built):
    import torch
    m, s0 = make_worlds(64, 7)
    sim = hb.RigidBodySim(m, 64)
    sim.state.copy_(_cuda(s0))
    before = sim.state.clone()
    sT, jv = sim.jvp(_cuda(s0), None, 120)
    assert jv is None
    torch.cuda.synchronize()
    assert torch.equal(sim.state, before)                # the resident state is not touched
    sim.step(120)
    e = rel_err(sT.cpu().numpy(), sim.state.cpu().numpy(), 1e-2)
    print(f"jvp primal against RigidBodySim.step (120 steps): {e:.2e}")
    assert e <= 1e-9                                     # tds_rb_step contracts products into FMAs, tds_rb_jvp does not
    sT2, _ = sim.jvp(_cuda(s0), _cuda(np.ones((64, 2, m.num_bodies * 13))), 120)
    assert torch.equal(sT, sT2)
    f32 = hb.RigidBodySim(m, 4, dtype="f32")
    with pytest.raises(hb.TdsHipError, match="f32"):
        f32.jvp(_cuda(s0[:4]), None, 1)


def test_rb_rollout_fn_gradcheck(built):
    import torch
    m, s0 = make_worlds(3, 7)
    sim = hb.RigidBodySim(m, 3)
    wrt = [(1, 7), (1, 8), (2, 9), (3, 2)]
    params = [("mass", 2), ("friction",)]
    f = tds_amd.rb_rollout_fn(sim, 10, wrt, params)
    s = _cuda(s0)
    u = torch.stack([s[:, b, c] for b, c in wrt], 1).clone().requires_grad_(True)
    th = torch.tensor(hb.rb_params_get(m, params), dtype=torch.float64, device="cuda", requires_grad=True)
    assert torch.autograd.gradcheck(lambda uu, tt: f(s, uu, tt), (u, th), eps=1e-6, atol=1e-5, rtol=1e-4)
    thn = th.detach().expand(3, 2).clone().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda uu, tt: f(s, uu, tt), (u, thn), eps=1e-6, atol=1e-5, rtol=1e-4)
    with pytest.raises(ValueError, match="s0"):
        f(s.clone().requires_grad_(True), u)


def test_billiard_gradient_and_descent(built):
    import torch
    m = billiard_model()
    steps = 300
    sim = hb.RigidBodySim(m, 1)
    # one world per shot; world 0 is the fixed shot, which moves ball 5
    rng = np.random.default_rng(0)
    forces = np.concatenate([[[10.0, 600.0]], rng.uniform([-100, 400], [100, 800], (63, 2))])
    n = forces.shape[0]
    s0 = billiard_state(n)
    s0[:, WHITE, 7:9] = shot_velocity(forces)
    # device gradient of the cost in (vx, vy) against central differences of the reference
    v = np.zeros((1, 2, 91))
    v[0, 0, SHOT[0]] = v[0, 1, SHOT[1]] = 1.0
    sT, jv = sim.jvp(_cuda(s0[:1]), _cuda(v), steps)
    sT, jv = sT.cpu().numpy(), jv.cpu().numpy()
    d = sT[0, BILLIARD_TARGET_BALL, :3] - np.array([3.5, 8.0, 0.0])
    grad = 2 * jv[0, :, BILLIARD_TARGET_BALL, :3] @ d
    assert billiard_cost(sT)[0] < billiard_cost(s0)[0] - 1.0       # the shot moves ball 5
    if reflib.available():
        h = 1e-6
        for c in range(2):
            a, b = s0[:1].copy(), s0[:1].copy()
            a[0, WHITE, 7 + c] += h
            b[0, WHITE, 7 + c] -= h
            fd = (billiard_cost(reflib.rb_step(m, a, steps)) - billiard_cost(reflib.rb_step(m, b, steps)))[0] / (2 * h)
            print(f"billiard d cost / d v{'xy'[c]}: device {grad[c]:.9f}, reference central difference {fd:.9f}")
            assert abs(grad[c] - fd) <= 1e-5 * max(abs(fd), 1.0)
    # gradient descent with backtracking on the GPU gradient, every shot a world
    wrt = [(WHITE, 7), (WHITE, 8)]
    f = tds_amd.rb_rollout_fn(sim, steps, wrt)
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
    print(f"billiard descent, fixed shot: cost {c0:.4f} -> {c1:.4f}")
    assert c1 < 0.5 * c0
