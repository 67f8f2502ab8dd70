"""GPU: the contact model's parameters (cfm, erp, the collision shapes' radius, length, extents and X_trans) through the
parameter derivatives' kernels and through the per-environment model variants of the general step kernel.

Derivatives: device against the host instantiations (1e-12), forward against reverse, gradcheck of param_step_fn and
the trajectory VJP against its host checker.  Variants: N = 70 environments, each under its own contact model, against
step_host of the applied models, jvp_params on the device, ordinary handles of the applied models and the reference.
The states come from the contact sweep of tests/diff_states.py, so that the contact model acts on most of them."""
import functools
import os

import numpy as np
import pytest

from conftest import rel_err

import tds_amd
from tds_amd import hip_backend as hb

import diff_states

pytestmark = pytest.mark.gpu

DERIV_MODELS = ["ant", "laikago_soft", "cartpole_plane", "cube_floating"]
VARIANT_MODELS = ["ant", "laikago", "cartpole_plane", "cube_floating"]
N = 70
TOL = 1e-9  # tests/test_variants_gpu.py: two separately compiled builds of one step
GENERAL = {"oct": 0, "quad": 0, "chain": 0}
SPHERE, BOX = 0, 4


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def rel(a, b):
    return float(np.max(np.abs(a - b)) / max(1.0, np.max(np.abs(b))))


def draw_theta(m, sel, n, seed):
    """+- 5 % relative and + [0, 0.004) additive on the contact kinds (cfm and radii stay positive, a box's zero radius
    below the clamp at 1e-2); the old kinds as tests/test_variants_gpu.py draws them"""
    base = hb.params_get(m, sel)
    rng = np.random.default_rng(seed)
    new = np.array([q[0] in hb.CONTACT_PARAM_KINDS for q in sel])
    additive = np.array([not q[0].endswith("inertia") for q in sel])
    u = rng.uniform(-1, 1, (n, len(sel)))
    return base * (1.0 + 0.05 * rng.uniform(-1, 1, (n, len(sel)))) + np.where(new, 0.002 * (u + 1.0), 0.01 * u * additive)


@functools.lru_cache(maxsize=None)
def deriv_case(name, n):
    """(model, selection: every contact parameter, x [n] of the contact sweep, theta [n, p]); read only"""
    m = tds_amd.load_model(name)
    if name == "cartpole_plane":  # one box above the clamp of the radius: a nonzero derivative
        g = next(g for g in range(m.num_geoms) if m.geoms[g].type == BOX)
        m = hb.params_apply(m, [("geom_radius", g)], [0.03])
    sel = hb.contact_params(m)
    x = np.ascontiguousarray(diff_states.states(name, n, 5, m))
    th = draw_theta(m, sel, n, 6)
    return m, sel, x, th


# ------------------------------------------------------------------------------------------------ derivatives
@pytest.mark.parametrize("n,k", [(1, 1), (7, 1), (65, 1), (33, 3)])
@pytest.mark.parametrize("name", DERIV_MODELS)
def test_device_matches_host(name, n, k, built):
    """jvp_params (k = 0: y alone; k directions over [x | theta]) and vjp_params (k cotangents) against the host
    instantiations, 1e-12; n = 65: one lane past a wavefront"""
    torch = _torch()
    m, sel, x, th = deriv_case(name, n)
    nin, p = m.input_dim, len(sel)
    rng = np.random.default_rng(n + k)
    kf = 3 if k == 1 else k  # forward mode: three directions over [x | theta] in every case
    v = rng.normal(size=(n, kf, nin + p))
    w = rng.normal(size=(n, k, m.output_dim))
    sim = hb.HipSim(m, n, device=0, dtype="f64")
    xd, thd = torch.from_numpy(x).cuda(), torch.from_numpy(th).cuda()
    y0 = sim.jvp_params(xd, thd, sel).cpu().numpy()
    y_f, jv = sim.jvp_params(xd, thd, sel, torch.from_numpy(v).cuda())
    y_r, wjx, wjt = sim.vjp_params(xd, thd, sel, torch.from_numpy(w).cuda())
    sim.close()
    wj = np.concatenate([wjx.cpu().numpy(), wjt.cpu().numpy()], axis=2)
    jv_h, y_h = hb.jvp_params_host(m, x, th, sel, v, want_y=True)
    wj_h = hb.vjp_params_host(m, x, th, sel, w)
    errs = dict(y0=rel(y0, y_h), y_f=rel(y_f.cpu().numpy(), y_h), y_r=rel(y_r.cpu().numpy(), y_h),
                jv=rel(jv.cpu().numpy(), jv_h), wj=rel(wj, wj_h))
    print(name, n, k, {a: f"{e:.1e}" for a, e in errs.items()})
    assert max(errs.values()) <= 1e-12, errs
    assert np.count_nonzero(wj_h[:, :, nin:]) > 0 and np.max(np.abs(y_h - hb.step_host(m, x))) > 0


def test_forward_and_reverse_modes_agree_on_ant(built):
    torch = _torch()
    n = 16
    m, sel, x, th = deriv_case("ant", n)
    sel = hb.all_params(m) + sel
    th = np.concatenate([np.tile(hb.params_get(m, hb.all_params(m)), (n, 1)), th], axis=1)
    sim = hb.HipSim(m, n, device=0, dtype="f64")
    g_out = torch.from_numpy(np.random.default_rng(9).normal(size=(n, m.output_dim))).cuda()
    grads = {}
    for mode in ("reverse", "forward"):
        xr = torch.from_numpy(x).cuda().requires_grad_(True)
        tr = torch.from_numpy(th).cuda().requires_grad_(True)
        y = tds_amd.param_step_fn(sim, sel, mode=mode)(xr, tr)
        grads[mode] = torch.autograd.grad(y, [xr, tr], g_out)
    sim.close()
    for a, b in zip(grads["reverse"], grads["forward"]):
        e = (torch.abs(a - b).max() / torch.clamp(torch.abs(b).max(), min=1.0)).item()
        print("ant, reverse against forward:", e)
        assert e <= 1e-11
    assert torch.count_nonzero(grads["reverse"][1][:, -len(hb.contact_params(m)):]) > 0


def smooth_states(m, sel, x, theta):
    """the states whose one-sided differences over every selected entry agree (no contact switches within reach of
    gradcheck's steps), by the host step"""
    from test_contact_params_cpu import set_param

    mm = hb.params_apply(m, sel, theta)
    _, kink = diff_states.central_theta(mm, x, sel, hb.step_host, set_param, h_rel=1e-5)
    _, kink_x = diff_states.central_jacobian(mm, x, h_rel=1e-5, step=lambda z: hb.step_host(mm, z))
    return np.flatnonzero(~kink.any(axis=1) & ~kink_x)


@pytest.mark.parametrize("mode", ["reverse", "forward"])
def test_gradcheck_of_param_step_fn(mode, built):
    """laikago_soft, theta = [cfm, erp, a foot's radius], shared [p] and per environment [N, p], on two states of the
    contact sweep with toes down and no switch nearby.  The 156 outputs go through a fixed random projection onto
    four: gradcheck takes one backward call per output element, and a reverse-mode call records a whole tape."""
    torch = _torch()
    m = tds_amd.load_model("laikago_soft")
    foot = next(g for g in range(m.num_geoms) if m.geoms[g].type == SPHERE)
    sel = [("cfm",), ("erp",), ("geom_radius", foot)]
    base = hb.params_get(m, sel)
    xs = diff_states.states("laikago_soft", 24, 5, m)
    J = hb.jvp_params_host(m, xs, base, sel, np.tile(np.eye(m.input_dim + 3)[m.input_dim:], (24, 1, 1)))
    live = np.flatnonzero(np.abs(J).max(axis=2).min(axis=1) > 0)  # every entry acts on the state
    keep = live[np.isin(live, smooth_states(m, sel, xs, base))][:2]
    assert keep.size == 2, (live, keep)
    n = 2
    sim = hb.HipSim(m, n, device=0, dtype="f64")
    step = tds_amd.param_step_fn(sim, sel, mode=mode)
    proj = torch.from_numpy(np.random.default_rng(10).normal(size=(m.output_dim, 4))).cuda()
    f = lambda xx, tt: step(xx, tt) @ proj  # noqa: E731
    x = torch.from_numpy(np.ascontiguousarray(xs[keep])).cuda().requires_grad_(True)
    th1 = torch.from_numpy(base).cuda().requires_grad_(True)
    thn = torch.from_numpy(np.stack([base, base * 1.01])).cuda().requires_grad_(True)
    for th in (thn, th1):
        # (eps 1e-7: small against cfm = 9.1e-3 and the foot's radius 0.03, large against the step's round-off)
        assert torch.autograd.gradcheck(f, (x, th), eps=1e-7, atol=1e-5, rtol=1e-4, nondet_tol=0.0)
    sim.close()


def test_trajectory_vjp_matches_its_host_checker(built):
    torch = _torch()
    name, steps, n = "laikago_soft", 5, 7
    m = tds_amd.load_model(name)
    foot = next(g for g in range(m.num_geoms) if m.geoms[g].type == SPHERE)
    sel = [("cfm",), ("erp",), ("geom_radius", foot), ("geom_trans", foot, 2), ("friction",)]
    x0 = np.ascontiguousarray(diff_states.states(name, n, 11, m))
    nsd, n_act, _ = hb.trajectory_dims(m, steps)
    th = draw_theta(m, sel, n, 13)
    u = np.random.default_rng(12).uniform(-0.2, 0.2, (n, steps - 1, n_act))
    gs = np.random.default_rng(14).normal(size=(n, steps, nsd))
    sim = hb.HipSim(m, n, device=0, dtype="f64")
    out = sim.trajectory_vjp(torch.from_numpy(x0).cuda(), torch.from_numpy(gs).cuda(), steps, 1,
                             torch.from_numpy(u).cuda(), sel, torch.from_numpy(th).cuda())
    out = [o.cpu().numpy() for o in out]
    sim.close()
    ref = hb.trajectory_vjp_host(m, x0, gs, steps, 1, u, sel, th)
    for what, a, b in zip(("s", "gx0", "gu", "gtheta"), out, ref):
        e = max(rel(a[e_], b[e_]) for e_ in range(n))
        print("trajectory_vjp", what, f"{e:.2e}")
        assert e <= 1e-11, (what, e)  # (tests/test_traj_vjp_gpu.py's bound on the gradients of chained steps)
    assert np.count_nonzero(ref[3]) > 0


# ------------------------------------------------------------------------------------------------ variants
def variant_sel(name, m):
    """cfm, erp, and per shape kind one entry of each geometry kind the model has, + two old kinds"""
    sel = [("cfm",), ("erp",)]
    seen = set()
    for g in range(m.num_geoms):
        t = m.geoms[g].type
        if t in seen or t not in (0, 2, 4):
            continue
        seen.add(t)
        sel += [("geom_radius", g), ("geom_trans", g, 2), ("geom_trans", g, 0)]
        if t == 2:
            sel.append(("geom_length", g))
        if t == 4:
            sel += [("geom_extent", g, 0), ("geom_extent", g, 2)]
    last = next(g for g in range(m.num_geoms - 1, -1, -1) if m.geoms[g].type in (0, 2, 4))
    if ("geom_radius", last) not in sel:
        sel += [("geom_radius", last), ("geom_trans", last, 1)]
    return sel + [("gravity", 2), ("friction",)]


@functools.lru_cache(maxsize=None)
def variant_case(name):
    m = tds_amd.load_model(name)
    sel = variant_sel(name, m)
    x = np.ascontiguousarray(diff_states.states(name, N, 12, m))
    theta = draw_theta(m, sel, N, 7)
    map3 = np.random.default_rng(12).permutation(np.arange(N) % 3).astype(np.int32)
    ref_own = np.stack([hb.step_host(hb.params_apply(m, sel, theta[e]), x[e:e + 1])[0] for e in range(N)])
    ref_3 = np.stack([hb.step_host(hb.params_apply(m, sel, theta[v]), x) for v in range(3)])
    assert np.max(np.abs(ref_own - hb.step_host(m, x))) > 0
    return dict(m=m, sel=sel, x=x, theta=theta, map3=map3, ref_own=ref_own, ref_3=ref_3)


@pytest.mark.parametrize("name", VARIANT_MODELS)
def test_each_environment_steps_its_own_contact_model(name, built):
    torch = _torch()
    c = variant_case(name)
    m, sel, theta, map3 = c["m"], c["sel"], c["theta"], c["map3"]
    x = torch.from_numpy(c["x"]).cuda()
    sim = hb.HipSim(m, N)
    own = sim.single_step_kernel()[0]
    y_before = sim.forward_zero(x).clone()
    for v, ev, th_rows, ref in ((N, None, theta, c["ref_own"]),
                                (3, map3, theta[map3], c["ref_3"][map3, np.arange(N)]),
                                (1, np.zeros(N, dtype=np.int32), np.tile(theta[:1], (N, 1)), c["ref_3"][0])):
        sim.set_model_variants(sel, theta[:v], ev)
        assert sim.num_model_variants == v and sim.single_step_kernel()[0] == "general"
        y = sim.forward_zero(x).clone()
        y_par = sim.jvp_params(x, torch.from_numpy(np.ascontiguousarray(th_rows)).cuda(), sel)
        e_host = rel_err(y.cpu().numpy(), ref)
        e_par = rel_err(y.cpu().numpy(), y_par.cpu().numpy())
        print(f"{name} V={v}: vs step_host of the applied models {e_host:.2e}, vs jvp_params on the device {e_par:.2e}")
        assert e_host <= TOL and e_par <= TOL, (name, v, e_host, e_par)
        if v == 3:
            for k in range(3):
                ordinary = hb.HipSim(hb.params_apply(m, sel, theta[k]), N, options=GENERAL)
                rows = np.flatnonzero(map3 == k)
                e_ord = rel_err(y[rows].cpu().numpy(), ordinary.forward_zero(x)[rows].cpu().numpy())
                print(f"{name} V=3 variant {k}: vs an ordinary handle of the applied model {e_ord:.2e}")
                assert e_ord <= TOL, (name, k, e_ord)
                ordinary.close()
    sim.clear_model_variants()
    assert sim.num_model_variants == 0 and sim.single_step_kernel()[0] == own
    assert torch.equal(sim.forward_zero(x), y_before)
    sim.close()


@pytest.mark.parametrize("loop", [1, 0])
def test_step_many_runs_the_contact_variants(loop, built):
    """three steps in one step_many call (the step-loop build, and chained graphs) against three forward_zero calls"""
    torch = _torch()
    c = variant_case("ant")
    m, sel, theta, map3 = c["m"], c["sel"], c["theta"], c["map3"]
    nqd, steps = m.dof_q + m.dof_qd, 3
    x0 = torch.from_numpy(c["x"]).cuda()
    acts = torch.from_numpy(np.random.default_rng(21).uniform(-0.4, 0.4, (steps, N, m.action_dim))).cuda().contiguous()
    sim = hb.HipSim(m, N)
    sim.set_option("step_many_loop", loop)

    def run():
        sim.x.copy_(x0)
        sim.step_many(acts, steps)
        return sim.y.clone()

    before = run()
    sim.set_model_variants(sel, theta[:3], map3)
    x, y = x0.clone(), None
    for k in range(steps):
        x[:, nqd:nqd + m.action_dim] = acts[k]
        y = sim.forward_zero(x).clone()
        x[:, :nqd] = y[:, :nqd]
    assert sim.step_many_is_loop(steps) == bool(loop)
    got = run()
    e = rel_err(got.cpu().numpy(), y.cpu().numpy())
    print(f"step_many under contact variants, step_many_loop = {loop}: {e:.2e}")
    assert e <= TOL and rel_err(got.cpu().numpy(), before.cpu().numpy()) > 1e-6
    sim.clear_model_variants()
    assert torch.equal(run(), before)
    sim.close()


def test_ant_softness_variants_against_the_reference(built):
    """one reference simulator per variant with set_solver(cfm_v, erp_v, ...): each variant's rows within the
    project's gate"""
    import reflib
    if not reflib.available():
        pytest.skip("the reference library is not built here")
    import gen_golden

    torch = _torch()
    c = variant_case("ant")
    m, x, map3 = c["m"], c["x"], c["map3"]
    sel = [("cfm",), ("erp",)]
    theta = hb.params_get(m, sel) * np.array([[0.5, 1.2], [1.0, 0.8], [20.0, 1.0]])
    sim = hb.HipSim(m, N)
    sim.set_model_variants(sel, theta, map3)
    y = sim.forward_zero(torch.from_numpy(x).cuda()).cpu().numpy()
    sim.close()
    for v in range(3):
        r, _ = gen_golden.make_ref("ant")
        try:
            r.set_solver(theta[v, 0], theta[v, 1], m.pgs_iterations, m.friction, m.restitution)
            rows = np.flatnonzero(map3 == v)
            y_ref = r.step(x[rows])
        finally:
            r.close()
        err = rel_err(y[rows], y_ref)
        print(f"ant variant {v} (cfm {theta[v, 0]:.1e}, erp {theta[v, 1]:.2f}; {rows.size} rows) vs the reference: {err:.2e}")
        assert err <= 1e-6, (v, err)


def test_recovery_of_softness_and_a_foot_radius(built):
    """laikago_soft: cfm, erp and a foot's radius fitted to a 6-step trajectory of 16 states of the contact sweep with
    torch's LBFGS over trajectory_fn(mode="reverse"), from 10 % / -10 % / 5 % off; theta* to 1e-3, the bound of
    tests/test_param_derivs_gpu.py's recovery (the same optimisation on the host checkers ends at 4e-10)"""
    torch = _torch()
    name, steps, n = "laikago_soft", 6, 16
    m = tds_amd.load_model(name)
    foot = next(g for g in range(m.num_geoms) if m.geoms[g].type == SPHERE)
    sel = [("cfm",), ("erp",), ("geom_radius", foot)]
    true = hb.params_get(m, sel)
    x0 = np.ascontiguousarray(diff_states.states(name, n, 11, m))
    n_act = hb.trajectory_dims(m, steps)[1]
    u = np.random.default_rng(12).uniform(-0.2, 0.2, (n, steps - 1, n_act))
    target = torch.from_numpy(hb.trajectory_jvp_host(m, x0, steps=steps, u=u, params=sel, theta=true)[0]).cuda()
    sim = hb.HipSim(m, n, device=0, dtype="f64")
    f = tds_amd.trajectory_fn(sim, steps, params=sel, mode="reverse")
    x0_d, u_d, true_d = torch.from_numpy(x0).cuda(), torch.from_numpy(u).cuda(), torch.from_numpy(true).cuda()
    sc = torch.tensor([1.1, 0.9, 1.05], dtype=torch.float64, device="cuda", requires_grad=True)  # theta = theta* scale
    opt = torch.optim.LBFGS([sc], lr=1.0, max_iter=100, tolerance_grad=1e-14, tolerance_change=1e-16,
                            line_search_fn="strong_wolfe")
    calls = [0]

    def closure():
        opt.zero_grad()
        loss = ((f(x0_d, None, true_d * sc, u_d) - target) ** 2).sum()
        loss.backward()
        calls[0] += 1
        return loss

    first = float(closure().detach())
    opt.step(closure)
    last = float(closure().detach())
    sim.close()
    err = float(torch.abs(sc.detach() - 1.0).max())
    print(f"recovery: loss {first:.3e} -> {last:.3e} in {calls[0]} evaluations, theta* to {err:.2e}")
    assert first > 1.0 and err <= 1e-3, (first, last, err)
