"""GPU: the step-derivative and query kernels (tds_jvp.hip, tds_vjp.hip, tds_dparam.hip, tds_traj.hip, tds_dyn.hip,
tds_dyn_jvp.hip, tds_contact.hip, tds_contact_jvp.hip) on the curated random trees of tests/tree_cases.py, f64, against
the host instantiation of the same templates (which tests/test_tree_derivs_cpu.py holds against the C oracle).

Every tree gets one handle over 70 records, its 16 states tiled: the one-lane-per-environment tape kernels end in a
partial wavefront, and 3 and 5 directions leave partial direction blocks (K = 4 in class S, 2 in A and L).  Every output
the bindings allocate, and every one handed to them, lies in front of poisoned padding that must come back untouched.

Device against host: the project's 1e-12, metric rel() of tests/test_diff_sweep_gpu.py (both sides are one template and
differ by contraction only).  Measured maxima on an MI355X, each the largest over a class's trees and every call:
  S 3.8e-13 (the primals; derivatives 1.1e-13), A 2.9e-14 (derivatives 1.1e-14), L 5.0e-13 (derivatives 8.8e-14),
  trajectories over three steps 1.3e-14.  No tree needed a bound of its own.
The jvp kernel's primal against forward_zero of the handle's own step kernel (the general kernel on every tree: another
statement of the step on the device), metric max |a - b| / max(|b|, 1): measured S 3.4e-13, A 7.7e-14, L 4.3e-13;
FORWARD_ZERO_BOUND is 10 x the largest, far inside the 1e-6 per-step contract.
The file takes 6 s of wall time on an MI355X."""
import numpy as np
import pytest

import tds_amd
from tds_amd import hip_backend as hb
import tree_cases as tc
from test_diff_sweep_gpu import rel as sweep_rel, step_rel

pytestmark = pytest.mark.gpu

N = 70
PAD = 64
POISON = -7.25
DEVICE_BOUND = 1e-12
FORWARD_ZERO_BOUND = 10 * 4.4e-13
BY_ID = {c["id"]: c for c in tc.ALL}
# one fixed and one floating tree per class
TRAJECTORY_IDS = ["S-fixed65", "S-floating504", "A-fixed1", "A-floating858", "L-fixed3", "L-floating858"]


class Poisoned:
    """The allocator of the bindings' device outputs (hb._DevArrays.new) with PAD poisoned entries behind each"""

    def __init__(self):
        self.buffers = []

    def new(self, shape, like=None, dtype="float64", zero=False):
        import torch

        shape = tuple(int(d) for d in shape)
        n = int(np.prod(shape)) if shape else 1
        self.fill = POISON if dtype.startswith("float") else -7
        flat = torch.full((n + PAD,), self.fill, dtype=getattr(torch, dtype), device="cuda")
        if zero:
            flat[:n] = 0
        self.buffers.append((flat, n, self.fill))
        return flat[:n].view(shape)

    def check(self):
        import torch

        torch.cuda.synchronize()
        for flat, n, fill in self.buffers:
            assert bool((flat[n:] == fill).all()), (tuple(flat.shape), n)
        count, self.buffers = len(self.buffers), []
        return count


@pytest.fixture
def poisoned(monkeypatch):
    p = Poisoned()
    monkeypatch.setattr(hb._DevArrays, "new", staticmethod(p.new))
    return p


def rel(a, b):
    """test_diff_sweep_gpu's; an output without extent (a tree without shapes) agrees"""
    return sweep_rel(a, b) if np.size(b) else 0.0


def cu(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def tiled(c):
    m, _, _ = tc.tree(c)
    x, counts = tc.states_of(c)
    idx = np.arange(N) % tc.N_STATES
    return m, np.ascontiguousarray(x[idx]), counts[idx]


def every_param(m):
    return hb.all_params(m) + hb.contact_params(m)


def split(m, x):
    nq, nd = m.dof_q, m.dof_qd
    return x[:, :nq].copy(), x[:, nq:nq + nd].copy(), x[:, nq + nd:nq + nd + hb.dyn_tau_dim(m)].copy()


def seen(figures, what, err):
    figures[what] = max(figures.get(what, 0.0), err)


def forward_mode(sim, m, x, xd, rng, poisoned, figures):
    nin = m.input_dim
    jac_h, y_h = hb.jacobian_host(m, x, want_y=True)
    y_fz = sim.forward_zero(xd).cpu().numpy()
    for k in (3, 5):
        v = rng.normal(size=(N, k, nin))
        y, jv = sim.jvp(xd, cu(v), y=poisoned.new((N, m.output_dim)))
        y, jv = y.cpu().numpy(), jv.cpu().numpy()
        seen(figures, "jvp", rel(jv, np.einsum("noi,nki->nko", jac_h, v)))
        seen(figures, "jvp primal", step_rel(y, y_h))
        seen(figures, "forward_zero", step_rel(y, y_fz))
    y = poisoned.new((N, m.output_dim))
    jac = sim.jacobian(xd, y=y)
    seen(figures, "jacobian", rel(jac.cpu().numpy(), jac_h))
    seen(figures, "jvp primal", step_rel(y.cpu().numpy(), y_h))
    return jac_h, y_h


@pytest.mark.parametrize("cid", [c["id"] for c in tc.CASES])
def test_device_matches_host_on_a_tree(cid, built, poisoned):
    c = BY_ID[cid]
    m, x, counts = tiled(c)
    nin, nout = m.input_dim, m.output_dim
    rng = np.random.default_rng(c["seed"] + 2)
    figures = {}
    sim = hb.HipSim(m, N, device=0, dtype="f64")
    try:
        kernel = sim.single_step_kernel()[0]
        xd = cu(x)
        jac_h, y_h = forward_mode(sim, m, x, xd, rng, poisoned, figures)
        # reverse mode
        for k in (1, 3):
            w = rng.normal(size=(N, k, nout))
            y, wj = sim.vjp(xd, cu(w), y=poisoned.new((N, nout)))
            seen(figures, "vjp", rel(wj.cpu().numpy(), hb.vjp_host(m, x, w)))
            seen(figures, "vjp primal", step_rel(y.cpu().numpy(), y_h))
        # [x | theta], every selectable parameter
        sel = every_param(m)
        p = len(sel)
        theta = hb.params_get(m, sel)
        thd = cu(theta)
        v = rng.normal(size=(N, 3, nin + p))
        y, jv = sim.jvp_params(xd, thd, sel, cu(v))
        seen(figures, "jvp_params", rel(jv.cpu().numpy(), hb.jvp_params_host(m, x, theta, sel, v)))
        seen(figures, "jvp primal", step_rel(y.cpu().numpy(), y_h))
        w = rng.normal(size=(N, 2, nout))
        y, wj_x, wj_t = sim.vjp_params(xd, thd, sel, cu(w))
        wj = np.concatenate([wj_x.cpu().numpy(), wj_t.cpu().numpy()], axis=-1)
        seen(figures, "vjp_params", rel(wj, hb.vjp_params_host(m, x, theta, sel, w)))
        seen(figures, "vjp primal", step_rel(y.cpu().numpy(), y_h))
        # the queries, every output the base allows
        q, qd, tau = split(m, x)
        qdev, qdd_, taud = cu(q), cu(qd), cu(tau)
        want = ("x_world", "mass_matrix", "qdd") if m.is_floating else hb.DYN_OUTPUTS
        out = {k: poisoned.new(s) for k, s in hb.dyn_shapes(m, N).items() if k in want}
        d = sim.dynamics(qdev, qdd_, taud, want=want, out=out)
        d_h = hb.dynamics_host(m, q, qd, tau, want=want)
        for k in want:
            seen(figures, "dynamics", rel(d[k].cpu().numpy(), d_h[k]))
        out = {k: poisoned.new(s) for k, s in hb.contact_shapes(m, N).items()}
        d = sim.contacts(xd, out=out)
        d_h = hb.contacts_host(m, x)
        for k in hb.CONTACT_OUTPUTS:
            seen(figures, "contacts", rel(d[k].cpu().numpy(), d_h[k]))
        link = max(i for i in range(m.num_links) if m.links[i].joint_type != tds_amd.JOINT_FIXED)
        pts = rng.normal(0, 0.2, (N, 3))
        seen(figures, "point_jacobian", rel(sim.point_jacobian(qdev, link, cu(pts), local=True).cpu().numpy(),
                                            hb.point_jacobian_host(m, q, link, pts, local=True)))
        # their derivatives, three directions in [z | theta]
        dsel = hb.all_params(m)
        dth = hb.params_get(m, dsel)
        v = rng.normal(size=(N, 3, hb.dyn_input_dim(m) + len(dsel)))
        out = {k: poisoned.new(s) for k, s in hb.dyn_tangent_shapes(m, N, 3).items() if k in want}
        t = sim.dynamics_jvp(qdev, qdd_, taud, cu(v), want=want, params=dsel, theta=cu(dth), out=out)
        t_h = hb.dynamics_jvp_host(m, q, qd, tau, v, want=want, params=dsel, theta=dth)
        for k in want:
            seen(figures, "dynamics_jvp", rel(t[k].cpu().numpy(), t_h[k]))
        v = rng.normal(size=(N, 3, nin + p))
        out = {k: poisoned.new(s) for k, s in hb.contact_tangent_shapes(m, N, 3).items()}
        t = sim.contacts_jvp(xd, cu(v), params=sel, theta=thd, out=out)
        t_h = hb.contacts_jvp_host(m, x, v, params=sel, theta=theta)
        for k in hb.CONTACT_OUTPUTS:
            seen(figures, "contacts_jvp", rel(t[k].cpu().numpy(), t_h[k]))
        if m.is_floating:
            with pytest.raises(hb.TdsHipError, match="error 2: .*no floating-base inverse dynamics"):
                sim.dynamics(qdev, qdd_, taud, want=("bias",))
            with pytest.raises(hb.TdsHipError, match="error 2: .*no floating-base inverse dynamics"):
                sim.inverse_dynamics(qdev, qdd_, None)
        else:
            acc = rng.normal(size=(N, m.dof_qd))
            seen(figures, "inverse_dynamics", rel(sim.inverse_dynamics(qdev, qdd_, cu(acc)).cpu().numpy(),
                                                  hb.inverse_dynamics_host(m, q, qd, acc)))
            v = rng.normal(size=(N, 3, hb.dyn_input_dim(m, True) + len(dsel)))
            dtau = sim.inverse_dynamics_jvp(qdev, qdd_, cu(acc), cu(v), params=dsel, theta=cu(dth))
            seen(figures, "inverse_dynamics_jvp",
                 rel(dtau.cpu().numpy(), hb.inverse_dynamics_jvp_host(m, q, qd, acc, v, params=dsel, theta=dth)))
        buffers = poisoned.check()
    finally:
        sim.close()
    fz = figures.pop("forward_zero")
    print(f"{cid}: {m.num_links} links, {m.dof_qd} dofs, {tc.contact_points(m)} contact points (active "
          f"{sorted(set(counts.tolist()))}), {p} parameters, step kernel {kernel}, {buffers} padded buffers; "
          f"device vs host " + ", ".join(f"{k} {v:.2e}" for k, v in figures.items()) + f"; jvp primal vs forward_zero {fz:.2e}")
    assert buffers >= 20
    assert max(figures.values()) <= DEVICE_BOUND, figures
    assert fz <= FORWARD_ZERO_BOUND <= 1e-6


@pytest.mark.parametrize("cid", [c["id"] for c in tc.OVERFLOW])
def test_overflowing_tree_is_refused_and_the_handle_lives_on(cid, built, poisoned):
    """the capacity error of the host call in plain and in parameter mode; forward mode on the same handle afterwards"""
    c = BY_ID[cid]
    m, x, _ = tiled(c)
    rng = np.random.default_rng(c["seed"] + 2)
    figures = {}
    sim = hb.HipSim(m, N, device=0, dtype="f64")
    try:
        xd = cu(x)
        w = cu(rng.normal(size=(N, m.output_dim)))
        with pytest.raises(hb.TdsHipError, match="error 2: .*tape exceeds the capacity"):
            sim.vjp(xd, w)
        sel = every_param(m)
        with pytest.raises(hb.TdsHipError, match="error 2: .*tape exceeds the capacity"):
            sim.vjp_params(xd, cu(hb.params_get(m, sel)), sel, w)
        forward_mode(sim, m, x, xd, rng, poisoned, figures)
        poisoned.check()
    finally:
        sim.close()
    fz = figures.pop("forward_zero")
    print(f"{cid}: device vs host " + ", ".join(f"{k} {v:.2e}" for k, v in figures.items()) +
          f"; jvp primal vs forward_zero {fz:.2e}")
    assert max(figures.values()) <= DEVICE_BOUND, figures
    assert fz <= FORWARD_ZERO_BOUND <= 1e-6


@pytest.mark.parametrize("cid", TRAJECTORY_IDS)
def test_trajectory_derivatives_on_a_tree(cid, built, poisoned):
    """three steps, a record each, in [x0 | theta] with a link's mass, gravity and friction; against the host twins"""
    c = BY_ID[cid]
    m, x, _ = tiled(c)
    rng = np.random.default_rng(c["seed"] + 3)
    steps = 3
    nsd, n_act, n_rec = hb.trajectory_dims(m, steps)
    sel = [("mass", m.num_links - 1), ("gravity", 2), ("friction",)]
    theta = hb.params_get(m, sel)
    u = rng.uniform(-1, 1, (N, steps - 1, n_act))
    figures = {}
    sim = hb.HipSim(m, N, device=0, dtype="f64")
    try:
        xd, ud, thd = cu(x), cu(u), cu(theta)
        v = rng.normal(size=(N, 3, m.input_dim + len(sel)))
        s, js = sim.trajectory_jvp(xd, cu(v), steps, u=ud, params=sel, theta=thd)
        s_h, js_h = hb.trajectory_jvp_host(m, x, v, steps, u=u, params=sel, theta=theta)
        seen(figures, "trajectory_jvp", rel(js.cpu().numpy(), js_h))
        seen(figures, "trajectory", rel(s.cpu().numpy(), s_h))
        gs = rng.normal(size=(N, n_rec, nsd))
        s, gx0, gu, gth = sim.trajectory_vjp(xd, cu(gs), steps, u=ud, params=sel, theta=thd)
        s_h, gx0_h, gu_h, gth_h = hb.trajectory_vjp_host(m, x, gs, steps, u=u, params=sel, theta=theta)
        seen(figures, "trajectory", rel(s.cpu().numpy(), s_h))
        for got, host in ((gx0, gx0_h), (gu, gu_h), (gth, gth_h)):
            seen(figures, "trajectory_vjp", rel(got.cpu().numpy(), host))
        poisoned.check()
    finally:
        sim.close()
    print(f"{cid}: device vs host " + ", ".join(f"{k} {v:.2e}" for k, v in figures.items()))
    assert np.abs(js_h).max() > 0 and np.abs(gx0_h).max() > 0
    assert max(figures.values()) <= DEVICE_BOUND, figures
