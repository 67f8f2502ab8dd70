"""GPU: closed-loop policy gradients (tds_policy_grad.hip, tds_hip_policy_trajectory_vjp) against their host
instantiation, plan independence, the lane budget, a shared handle, the rollout, policy_trajectory_fn (gradcheck, the
shared policy, against the chained param_step_fn(mode="reverse") with a torch module), a descent that uses the gradient,
and refusals."""
import functools

import numpy as np
import pytest

import tds_amd
from tds_amd import hip_backend as hb
import diff_states
from test_traj_derivs_gpu import DEV_TOL, SEL, records, starts, rel
from test_policy_grad_cpu import RAW, draw_policy, net_args, net_of, offsets

pytestmark = pytest.mark.gpu

T = 12
KINDS = ["linear", "mlp"]


def cuda(a):
    import torch

    return None if a is None else torch.from_numpy(np.array(a, dtype=np.float64, order="C")).cuda()  # (a writable copy)


@functools.lru_cache(maxsize=None)
def inputs(name, kind, n, steps=T, every=1, seed=11):
    """(m, sel, x0, theta, policy, gs, ga): shared between the tests, read only"""
    m = tds_amd.load_model(name)
    sel = SEL[name] if name in SEL else [("mass", 1), ("gravity", 2)]
    x = np.ascontiguousarray(starts(name, n, seed))
    rng = np.random.default_rng(seed + 1)
    th = hb.params_get(m, sel) * (1.0 + 0.01 * rng.uniform(-1, 1, (n, len(sel))))
    nsd, n_act, n_rec = hb.trajectory_dims(m, steps, every)
    gs = rng.normal(size=(n, n_rec, nsd))
    ga = rng.normal(size=(n, steps, n_act))
    pol = draw_policy(m, kind, n)
    for a in (x, th, pol, gs, ga):
        a.setflags(write=False)
    return m, sel, x, th, pol, gs, ga


def device(sim, name, kind, x, pol, gs, ga, steps, every, sel, th):
    out = sim.policy_trajectory_vjp(cuda(x), cuda(pol), cuda(gs), steps, every, cuda(ga), params=sel, theta=cuda(th),
                                    obs_raw=bool(RAW.get(name)), **net_args(sim.model, kind))
    return tuple(t.cpu().numpy() for t in out)


def host(m, name, kind, x, pol, gs, ga, steps, every, sel, th):
    return hb.policy_trajectory_vjp_host(m, x, pol, gs, steps, every, ga, params=sel, theta=th,
                                         obs_raw=bool(RAW.get(name)), **net_args(m, kind))


def worst_rel(dev, hst, idx=None):
    """the largest per-environment relative difference over (s, u, gpolicy, gx0, gtheta)"""
    worst = 0.0
    for d, h in zip(dev, hst):
        d = d if idx is None else d[idx]
        for e in range(h.shape[0]):
            if h[e].size:
                worst = max(worst, rel(d[e], h[e]))
    return worst


@pytest.mark.parametrize("n", [1, 7, 130])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["ant", "laikago", "pendulum5", "cartpole"])
def test_device_matches_host(name, kind, n, built):
    m, sel, x, th, pol, gs, ga = inputs(name, kind, n)
    sim = hb.HipSim(m, min(n, 64), device=0, dtype="f64")
    dev = device(sim, name, kind, x, pol, gs, ga, T, 1, sel, th)
    hst = host(m, name, kind, x, pol, gs, ga, T, 1, sel, th)
    worst = worst_rel(dev, hst)
    print(name, kind, n, "max rel device-host", worst)
    assert worst <= DEV_TOL, worst
    assert all(np.all(np.isfinite(d)) for d in dev) and np.count_nonzero(dev[2]) > 0
    nsd = m.dof_q + m.dof_qd
    assert np.all(dev[3][:, nsd:nsd + m.action_dim] == 0.0)
    # the primal alone is the same trajectory
    s, u = sim.policy_trajectory(cuda(x), cuda(pol), T, params=sel, theta=cuda(th), obs_raw=bool(RAW.get(name)),
                                 **net_args(m, kind))
    np.testing.assert_array_equal(s.cpu().numpy(), dev[0])
    np.testing.assert_array_equal(u.cpu().numpy(), dev[1])


@functools.lru_cache(maxsize=None)
def default_plan_result(name, kind):
    m, sel, x, th, pol, gs, ga = inputs(name, kind, 130, T, 3)
    sim = hb.HipSim(m, 64, device=0, dtype="f64")
    return device(sim, name, kind, x, pol, gs, ga, T, 3, sel, th)


@pytest.mark.parametrize("traj_steps", [1, 5, None])
@pytest.mark.parametrize("name,kind", [("ant", "mlp"), ("pendulum5", "linear")])
def test_windows_and_chunks_are_invisible(name, kind, traj_steps, built):
    m, sel, x, th, pol, gs, ga = inputs(name, kind, 130, T, 3)
    ref = default_plan_result(name, kind)
    sim = hb.HipSim(m, 64, device=0, dtype="f64")
    sim.set_option("traj_steps", traj_steps)
    for lanes in (64, 128, None):
        sim.set_option("traj_vjp_lanes", lanes)
        for a, b in zip(ref, device(sim, name, kind, x, pol, gs, ga, T, 3, sel, th)):
            np.testing.assert_array_equal(a, b, err_msg=str((traj_steps, lanes)))


def test_past_the_default_lane_budget(built):
    name, kind, n, steps = "pendulum5", "mlp", 4166, 3
    m, sel, x, th, pol, gs, ga = inputs(name, kind, n, steps)
    sim = hb.HipSim(m, 64, device=0, dtype="f64")
    dev = device(sim, name, kind, x, pol, gs, ga, steps, 1, sel, th)
    idx = np.sort(np.concatenate([np.random.default_rng(1).choice(n, 60, replace=False), [0, 4095, 4096, n - 1]]))[:64]
    hst = host(m, name, kind, x[idx], pol[idx], gs[idx], ga[idx], steps, 1, sel, th[idx])
    worst = worst_rel(dev, hst, idx)
    print(name, n, "max rel device-host", worst)
    assert worst <= DEV_TOL, worst
    assert all(np.all(np.isfinite(d)) for d in dev)


def test_interleaved_on_one_handle(built):
    import torch

    name, kind, n = "ant", "mlp", 16
    m, sel, x, th, pol, gs, ga = inputs(name, kind, n)
    nsd, n_act, _ = hb.trajectory_dims(m, T)
    xd, thd, pd, gsd, gad = (cuda(a) for a in (x, th, pol, gs, ga))
    ud = cuda(np.random.default_rng(3).uniform(-0.2, 0.2, (n, T - 1, n_act)))
    w = torch.zeros((n, m.output_dim), dtype=torch.float64, device="cuda")
    w[:, :nsd] = gsd[:, 0]
    kw = dict(params=sel, theta=thd, **net_args(m, kind))
    sim = hb.HipSim(m, n, device=0, dtype="f64")
    a1 = sim.policy_trajectory_vjp(xd, pd, gsd, T, 1, gad, **kw)
    v1 = sim.vjp(xd, w)
    a2 = sim.policy_trajectory_vjp(xd, pd, gsd, T, 1, gad, **kw)
    t1 = sim.trajectory_vjp(xd, gsd, T, 1, ud, sel, thd)
    a3 = sim.policy_trajectory_vjp(xd, pd, gsd, T, 1, gad, **kw)
    fresh = [hb.HipSim(m, n, device=0, dtype="f64") for _ in range(3)]
    af = fresh[0].policy_trajectory_vjp(xd, pd, gsd, T, 1, gad, **kw)
    vf = fresh[1].vjp(xd, w)
    tf = fresh[2].trajectory_vjp(xd, gsd, T, 1, ud, sel, thd)
    for a, b, c, f in zip(a1, a2, a3, af):
        assert torch.equal(a, f) and torch.equal(b, f) and torch.equal(c, f)
    for a, f in zip(v1 if isinstance(v1, tuple) else (v1,), vf if isinstance(vf, tuple) else (vf,)):
        assert torch.equal(a, f)
    for a, f in zip(t1, tf):
        assert torch.equal(a, f)


def test_actions_and_states_match_the_rollout(built):
    """Ant x 64, the linear policy, 8 steps, no auto-reset: u and the [q | qd] part of the rollout's trajectory records
    within the project's 1e-6 parity gate (both sides are pinned to the reference within it), environments not done"""
    import torch

    name, n, steps = "ant", 64, 8
    m = tds_amd.load_model(name)
    nsd, nact = m.dof_q + m.dof_qd, m.action_dim
    x = np.ascontiguousarray(records(name, n, 7))
    pol = 0.1 * draw_policy(m, "linear", n, 5)
    sim = hb.HipSim(m, n, device=0, dtype="f64")
    sim.x.copy_(cuda(x))
    before = sim.x.clone()
    s, u = sim.policy_trajectory(cuda(x), cuda(pol), steps)
    assert torch.equal(sim.x, before)  # the resident state is untouched
    _, counted, traj, _ = sim.rollout_ex(cuda(pol), steps, want_traj=True)
    traj = traj.cpu().numpy()
    alive = counted.cpu().numpy() == steps  # never done
    assert alive.sum() >= n // 2, alive.sum()
    s, u = s.cpu().numpy(), u.cpu().numpy()
    err_s = rel(s[alive], traj[alive][:, :, :nsd])
    print("ant x 64 against the rollout: states", err_s)
    assert err_s <= 1e-6, err_s
    # the actions: the linear policy on the rollout's own states, masked as the rollout masks them
    W = pol[:, :nsd * nact].reshape(n, nact, nsd)
    b = pol[:, nsd * nact:]
    for t in range(steps):
        o = (traj[:, t - 1, :nsd] if t > 0 else x[:, :nsd]).copy()
        o[:, :2] = 0.0
        u_r = np.einsum("nao,no->na", W, o) + b
        assert rel(u[alive, t], u_r[alive]) <= 1e-6


def test_gradcheck_and_the_shared_policy(built):
    import torch

    for name, kind, raw in (("cartpole", "mlp", True), ("pendulum5", "linear", True)):
        m = tds_amd.load_model(name)
        n, steps = 2, 4
        sel = [("mass", 1), ("gravity", 2)]
        sim = hb.HipSim(m, n, device=0, dtype="f64")
        f = tds_amd.policy_trajectory_fn(sim, steps, params=sel, every=2, obs_raw=raw, **net_args(m, kind))
        x0 = torch.from_numpy(records(name, n, 4)).cuda().requires_grad_(True)
        pol_n = cuda(draw_policy(m, kind, n, 31)).requires_grad_(True)
        pol_1 = cuda(draw_policy(m, kind, 1, 32)[0]).requires_grad_(True)
        base = hb.params_get(m, sel)
        th_1 = cuda(base).requires_grad_(True)
        th_n = cuda(np.stack([base, base * 1.01])).requires_grad_(True)
        for pol, th in ((pol_n, th_n), (pol_1, th_1)):
            assert torch.autograd.gradcheck(lambda xx, pp, tt: f(xx, pp, tt), (x0, pol, th), eps=1e-6, atol=1e-5,
                                            rtol=1e-4)
        # one policy for every environment: the sum of the per-environment gradients
        w_s = cuda(np.random.default_rng(8).normal(size=(n, steps // 2, m.dof_q + m.dof_qd)))
        w_u = cuda(np.random.default_rng(9).normal(size=(n, steps, m.action_dim)))
        loss = lambda su: (w_s * su[0]).sum() + (w_u * su[1]).sum()  # noqa: E731
        (g_1,) = torch.autograd.grad(loss(f(x0, pol_1, th_1)), (pol_1,))
        rows = pol_1.detach().unsqueeze(0).repeat(n, 1).requires_grad_(True)
        (g_n,) = torch.autograd.grad(loss(f(x0, rows, th_1)), (rows,))
        assert rel(g_1.cpu().numpy(), g_n.sum(0).cpu().numpy()) <= 1e-12 and torch.count_nonzero(g_1) > 0
        with pytest.raises(ValueError, match="theta"):
            tds_amd.policy_trajectory_fn(sim, steps)(x0, pol_1, th_1)


def torch_policy(net, pol, obs, raw):
    """the network in torch (float64), per environment, differentiable in pol"""
    import torch

    ls, act, ub = net
    wo, bo, _ = offsets(ls, ub)
    o = obs if raw else torch.cat([torch.zeros_like(obs[:, :2]), obs[:, 2:]], dim=1)
    if ub[0]:
        o = o + pol[:, bo[0]:bo[0] + ls[0]]
    for i in range(1, len(ls)):
        W = pol[:, wo[i]:wo[i] + ls[i - 1] * ls[i]].reshape(-1, ls[i], ls[i - 1])
        v = torch.bmm(W, o.unsqueeze(2)).squeeze(2)
        if ub[i]:
            v = v + pol[:, bo[i]:bo[i] + ls[i]]
        o = torch.tanh(v) if act[i - 1] == 0 else torch.relu(v) if act[i - 1] == 2 else v
    return o


def test_policy_and_parameter_gradients_match_the_chain_on_the_ant(built):
    import torch

    name, kind, n, steps = "ant", "mlp", 64, 16
    m = tds_amd.load_model(name)
    net = net_of(m, kind)
    sel = [("gravity", 2), ("friction",), ("mass", 2), ("mass", 5)]
    sim = hb.HipSim(m, n, device=0, dtype="f64")
    x0 = torch.from_numpy(np.ascontiguousarray(starts(name, n, 5))).cuda()
    nsd, n_act, _ = hb.trajectory_dims(m, steps)
    theta0 = torch.from_numpy(hb.params_get(m, sel)).cuda()
    rng = np.random.default_rng(6)
    w = torch.from_numpy(rng.normal(size=(n, steps, nsd))).cuda()
    wu = torch.from_numpy(rng.normal(size=(n, steps, n_act))).cuda()
    pol0 = cuda(draw_policy(m, kind, n, 33))
    th, pol = theta0.clone().requires_grad_(True), pol0.clone().requires_grad_(True)
    s, u = tds_amd.policy_trajectory_fn(sim, steps, params=sel, **net_args(m, kind))(x0, pol, th)
    g_th, g_pol = torch.autograd.grad((w * s).sum() + (wu * u).sum(), (th, pol))
    th2, pol2 = theta0.clone().requires_grad_(True), pol0.clone().requires_grad_(True)
    f = tds_amd.param_step_fn(sim, sel, mode="reverse")
    state, loss = x0[:, :nsd], 0.0
    for t in range(steps):
        ut = torch_policy(net, pol2, state, False)
        y = f(torch.cat([state, ut, x0[:, nsd + n_act:]], dim=1), th2)
        state = y[:, :nsd]
        loss = loss + (w[:, t] * state).sum() + (wu[:, t] * ut).sum()
    r_th, r_pol = torch.autograd.grad(loss, (th2, pol2))
    e_th = rel(g_th.cpu().numpy(), r_th.cpu().numpy())
    e_pol = max(rel(g_pol[e].cpu().numpy(), r_pol[e].cpu().numpy()) for e in range(n))
    print("ant x 64, T = 16: fused against the chain, theta", e_th, "policy", e_pol)
    assert e_th <= 1e-10 and e_pol <= 1e-10, (e_th, e_pol)
    assert torch.count_nonzero(g_th) == len(sel) and torch.count_nonzero(g_pol) > 0
    counts = diff_states.contact_counts(name, m, x0.cpu().numpy()[:32], reference=False)
    assert counts.max() > 0  # contacts are active


def test_descent_along_the_gradient(built):
    """pendulum5 x 64, the linear policy, T = 30, loss sum |q|^2 + 1e-3 sum |u|^2: ten iterations of backtracking
    descent along -gpolicy each accept a step under the Armijo condition"""
    import torch

    name, n, steps = "pendulum5", 64, 30
    m = tds_amd.load_model(name)
    nq = m.dof_q
    sim = hb.HipSim(m, n, device=0, dtype="f64")
    x0 = torch.from_numpy(records(name, n, 2)).cuda()
    f = tds_amd.policy_trajectory_fn(sim, steps, obs_raw=True)
    pol = cuda(0.1 * draw_policy(m, "linear", 1, 41)[0])

    def loss_of(p):
        s, u = f(x0, p)
        return (s[:, :, :nq] ** 2).sum() + 1e-3 * (u ** 2).sum()

    losses = []
    for it in range(10):
        p = pol.clone().requires_grad_(True)
        loss = loss_of(p)
        (g,) = torch.autograd.grad(loss, (p,))
        loss = loss.detach()
        losses.append(float(loss))
        step, accepted = 1.0 / max(float(g.norm()), 1e-12), False
        for _ in range(30):
            with torch.no_grad():
                trial = float(loss_of(pol - step * g))
            if trial <= float(loss) - 1e-4 * step * float(g.dot(g)):
                accepted = True
                break
            step *= 0.5
        assert accepted, (it, losses)
        pol = pol - step * g
    print("descent", losses[0], "->", trial)
    assert trial < losses[0]


def test_refusals(built):
    import torch

    m = tds_amd.load_model("ant")
    n = 4
    x = cuda(records("ant", n, 1))
    pol = cuda(draw_policy(m, "linear", n))
    gs = torch.zeros((n, 3, m.dof_q + m.dof_qd), dtype=torch.float64, device="cuda")
    for dt in ("f32", "mix"):
        try:
            s32 = hb.HipSim(m, n, device=0, dtype=dt)
        except (hb.TdsHipError, ValueError, KeyError):
            continue
        with pytest.raises(hb.TdsHipError, match="f64"):
            s32.policy_trajectory_vjp(x, pol, gs, 3)
    sim = hb.HipSim(m, n, device=0, dtype="f64")
    with pytest.raises(hb.TdsHipError, match="tds_hip error 1:"):
        sim.policy_trajectory_vjp(x, pol, gs[:, :1].contiguous(), 6, 4)
    with pytest.raises(hb.TdsHipError, match="spherical"):
        ms = tds_amd.load_model("pendulum5_spherical")
        s2 = hb.HipSim(ms, 2, device=0, dtype="f64")
        P = hb.policy_network_spec(ms)[4]
        s2.policy_trajectory_vjp(torch.from_numpy(records("pendulum5_spherical", 2)).cuda(),
                                 torch.zeros((2, P), dtype=torch.float64, device="cuda"),
                                 torch.zeros((2, 3, ms.dof_q + ms.dof_qd), dtype=torch.float64, device="cuda"), 3)
    with pytest.raises(hb.TdsHipError, match="tds_hip error 1:.*no actions"):
        mc = tds_amd.load_model("cube_floating")
        s3 = hb.HipSim(mc, 2, device=0, dtype="f64")
        s3.policy_trajectory_vjp(cuda(diff_states.states("cube_floating", 2, 1, mc)),
                                 torch.zeros((2, 1), dtype=torch.float64, device="cuda")[:, :0],
                                 torch.zeros((2, 3, mc.dof_q + mc.dof_qd), dtype=torch.float64, device="cuda"), 3)
