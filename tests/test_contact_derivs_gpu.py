"""Forward-mode derivatives of the contact query on the GPU (tds_hip_contacts_jvp, csrc/tds_contact_jvp.hip) against
their host instantiation, plus what a handle owes its other users (untouched outputs, the shared work buffer, the
stream, the refusals) and the autograd function tds_amd.contact_fn."""
import functools

import numpy as np
import pytest

import tds_amd
from tds_amd import hip_backend as hb

import diff_states as ds
from test_contact_derivs_cpu import MEASURED_X, identity, theta_sel
from test_dynamics_gpu import records, rel

pytestmark = pytest.mark.gpu

# Device against host: the same template without FP contraction on either side; only sin / cos are each side's own.
# The metric is test_contacts_gpu.py's (|a - b| / max(|b|, 1), the maximum over an output).  Measured on the MI355X over
# every case of test_device_matches_host, primal outputs and tangents: 3.91e-12 on cartpole_plane (sixteen active points
# on two dofs; the primal query's own maximum is 9.6e-13 there), ant 2.2e-13, laikago 5.5e-13, ant_floating 1.2e-12,
# pendulum5_plane 3.6e-13, cube_floating 0.  The tests assert 10 x the largest.
DEV_MEASURED = 3.91e-12
DEV_TOL = 10 * DEV_MEASURED
MODELS = ["ant", "laikago", "ant_floating", "cartpole_plane", "pendulum5_plane", "cube_floating"]


@functools.lru_cache(maxsize=None)
def sweep(name, n):
    x = np.ascontiguousarray(ds.states(name, n))
    x.setflags(write=False)
    return x


def cu(a):
    import torch

    return torch.from_numpy(np.array(a, dtype=np.float64, order="C")).cuda()  # (a copy: the sweeps are read-only)


def host(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def directions(rng, n, k, width):
    """k directions: the whole identity where k == width, random ones otherwise"""
    return identity(n, k, 0, width) if k == width else rng.normal(size=(n, k, width))


def compare(name, m, x, sel, th, v, idx=None):
    """device tangents and primal of every output against the host's, on the environments idx; the worst error"""
    sim = hb.HipSim(m, 8, device=0, dtype="f64")
    tan, prim = sim.contacts_jvp(cu(x), cu(v), params=sel, theta=None if th is None else cu(th), want_primal=True)
    tan, prim = host(tan), host(prim)
    idx = np.arange(x.shape[0]) if idx is None else idx
    ht, hp = hb.contacts_jvp_host(m, x[idx], v[idx], params=sel, theta=None if th is None else th[idx], want_primal=True)
    worst = 0.0
    for k in hb.CONTACT_OUTPUTS:
        assert tan[k].shape == hb.contact_tangent_shapes(m, x.shape[0], v.shape[1])[k]
        for got, ref in ((tan[k][idx], ht[k]), (prim[k][idx], hp[k])):
            assert np.all(np.isfinite(got)), (name, k)
            e = rel(got, ref)
            worst = max(worst, e)
            assert e <= DEV_TOL, (name, k, e)
    sep = hp["contacts"][:, :, 9] >= 0
    sep3 = np.concatenate([sep, sep, sep], axis=1)
    for k in ("rows", "rhs", "impulse"):
        assert not np.any(np.moveaxis(tan[k][idx], 1, -1)[sep3]), (name, k)
    assert not np.any(np.moveaxis(tan["force"][idx], 1, -1)[sep]), name
    print(f"{name} n {x.shape[0]} k {v.shape[1]}: max rel device-host {worst:.2e}")
    return worst


@pytest.mark.parametrize("n", [1, 7, 65])
@pytest.mark.parametrize("name", MODELS)
def test_device_matches_host(name, n, built):
    """[x | theta] with the selection of the CPU tests at per-environment theta; k: one direction, a full block, a
    partial last block, and the whole Jacobian"""
    m = tds_amd.load_model(name)
    x = sweep(name, 65)[:n]
    sel = theta_sel(m)
    nall, K = m.input_dim + len(sel), hb.contacts_jvp_tangents(m)
    rng = np.random.default_rng(7)
    th = hb.params_get(m, sel) * (1.0 + 0.05 * rng.uniform(size=(n, len(sel))))
    for k in (1, K, K + 1, nall):
        compare(name, m, x, sel, th, directions(rng, n, k, nall))
    compare(name, m, x, [], None, directions(rng, n, K + 1, m.input_dim))  # p = 0: the model's values


def test_grid_stride_walk(built):
    """2100 environments x 9 blocks = 18 900 items on at most 16 384 lanes; the sample holds the last environments"""
    m = tds_amd.load_model("pendulum5_plane")
    n, K = 2100, hb.contacts_jvp_tangents(m)
    x = sweep("pendulum5_plane", n)
    sel = [("friction",), ("erp",)]
    k = 8 * K + 1
    assert n * ((k + K - 1) // K) > 16384
    rng = np.random.default_rng(8)
    v = rng.normal(size=(n, k, m.input_dim + 2))
    idx = np.concatenate([rng.choice(n - 16, 48, replace=False), np.arange(n - 16, n)])
    compare("pendulum5_plane", m, x, sel, None, v, idx)


def test_only_requested_outputs_are_written_and_out_buffers_are_reused(built):
    import torch

    m = tds_amd.load_model("ant")
    n, k = 33, 3  # not the handle's num_envs
    x = cu(sweep("ant", 65)[:n])
    sel = [("friction",)]
    v = cu(np.random.default_rng(9).normal(size=(n, k, m.input_dim + 1)))
    sim = hb.HipSim(m, 8, device=0, dtype="f64")
    full, fullp = sim.contacts_jvp(x, v, params=sel, want_primal=True)
    shapes, pshapes = hb.contact_tangent_shapes(m, n, k), hb.contact_shapes(m, n)
    for want in (("force",), ("contacts", "jac"), ("qd_pre",), ("rows", "rhs"), ("delassus",), ("impulse", "qd_post")):
        bufs = {o: torch.full(shapes[o], -7.25, dtype=torch.float64, device="cuda") for o in hb.CONTACT_OUTPUTS}
        res = sim.contacts_jvp(x, v, want=want, params=sel, out=bufs)
        torch.cuda.synchronize()
        for o in hb.CONTACT_OUTPUTS:
            if o in want:
                assert res[o] is bufs[o] and torch.equal(bufs[o], full[o]), o
            else:
                assert o not in res and bool((bufs[o] == -7.25).all()), o
        # the raw entry point: primal and tangent sets chosen apart, the others poisoned
        pb = {o: torch.full(pshapes[o], -7.25, dtype=torch.float64, device="cuda") for o in hb.CONTACT_OUTPUTS}
        po = hb.ContactOut(**{o: pb[o].data_ptr() for o in want})
        to = hb.ContactOut(force=bufs["force"].data_ptr())
        assert hb.lib().tds_hip_contacts_jvp(sim.h, n, x.data_ptr(), 1, hb.param_spec(sel), None, k, v.data_ptr(), po,
                                             to) == 0
        torch.cuda.synchronize()
        for o in hb.CONTACT_OUTPUTS:
            assert torch.equal(pb[o], fullp[o]) if o in want else bool((pb[o] == -7.25).all()), o
        assert torch.equal(bufs["force"], full["force"])
    prim = sim.contacts_jvp(x, None, params=sel)  # k = 0: the primal at theta
    for o in hb.CONTACT_OUTPUTS:
        assert torch.equal(prim[o], fullp[o]), o
    J = sim.contacts_jacobian(x, "force", params=sel)
    cols = sim.contacts_jvp(x, cu(identity(n, m.input_dim + 1, 0, m.input_dim + 1)), want=("force",), params=sel)["force"]
    assert J.shape == (n, 17, 3, m.input_dim + 1) and torch.equal(J, cols.movedim(1, -1))
    some = sim.contacts_jacobian(x, "force", cols=[3, m.input_dim], params=sel)
    assert torch.equal(some, J[..., [3, m.input_dim]])


def test_work_buffer_is_shared_with_the_other_calls(built):
    import torch

    m = tds_amd.load_model("ant")
    n = 16
    xn = sweep("ant", 65)[:n]
    rng = np.random.default_rng(4)
    xd, v = cu(xn), cu(rng.normal(size=(n, 2, m.input_dim)))
    w = cu(rng.normal(size=(n, 2, m.output_dim)))
    q, qd = cu(xn[:, :m.dof_q]), cu(xn[:, m.dof_q:m.dof_q + m.dof_qd])
    tgt = cu(rng.normal(0, 0.3, (n, 1, 3)))
    sel = [("friction",), ("cfm",)]
    vc = cu(rng.normal(size=(n, 5, m.input_dim + 2)))

    def others(sim):
        y, jv = sim.jvp(xd, v)
        _, wj = sim.vjp(xd, w)
        d = sim.dynamics(q, qd, want=("mass_matrix", "qdd"))
        c = sim.contacts(xd, want=("impulse", "force"))
        ik = sim.inverse_kinematics(q, [m.num_links - 1], tgt, max_iterations=3)
        return [y, jv, wj, d["mass_matrix"], d["qdd"], c["impulse"], c["force"], ik["q"], ik["residual"]]

    def mine(sim):
        t = sim.contacts_jvp(xd, vc, params=sel)
        return [t[k] for k in hb.CONTACT_OUTPUTS]

    def same(a, b):
        return all(torch.equal(s, t) for s, t in zip(a, b))

    sim = hb.HipSim(m, n, device=0, dtype="f64")
    before, mine_before = others(sim), mine(sim)
    big = cu(np.tile(xn, (300, 1)))
    sim.contacts_jvp(big, cu(rng.normal(size=(big.shape[0], 3, m.input_dim + 2))), params=sel)  # grows the shared buffer
    assert same(others(sim), before) and same(mine(sim), mine_before)
    fresh = hb.HipSim(m, n, device=0, dtype="f64")  # the other way round: the derivatives first, another call grows
    first = mine(fresh)
    fresh.dynamics(cu(np.tile(xn[:, :m.dof_q], (3000, 1))), want=("mass_matrix",))
    assert same(others(fresh), before)
    assert same(first, mine_before) and same(mine(fresh), mine_before)


def test_runs_on_the_handles_stream(built):
    """ordered after earlier work on the stream given with tds_hip_set_stream: its inputs are filled there, behind a
    long-running kernel"""
    import torch

    m = tds_amd.load_model("ant")
    n = 256
    x = sweep("ant", 4096)[:n]
    sel = [("friction",)]
    v = np.random.default_rng(5).normal(size=(n, 3, m.input_dim + 1))
    sim = hb.HipSim(m, n, device=0, dtype="f64")
    names = ("impulse", "force", "qd_post")
    want = sim.contacts_jvp(cu(x), cu(v), want=names, params=sel)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    x_src, v_src = cu(x), cu(v)
    x_dev, v_dev = torch.zeros_like(x_src), torch.zeros_like(v_src)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        sim.use_current_stream()
        torch.cuda._sleep(200_000_000)  # ~0.1 s of device time ahead of the copies
        x_dev.copy_(x_src, non_blocking=True)
        v_dev.copy_(v_src, non_blocking=True)
        got = sim.contacts_jvp(x_dev, v_dev, want=names, params=sel)
    side.synchronize()
    sim.use_current_stream()
    for k in want:
        assert torch.equal(got[k], want[k]), k


def test_refusals_on_the_device(built):
    m = tds_amd.load_model("ant")
    x = cu(records("ant", 4))
    v = cu(np.zeros((4, 1, m.input_dim)))
    for dt in ("f32", "mix"):
        try:
            s32 = hb.HipSim(m, 4, device=0, dtype=dt)
        except (hb.TdsHipError, ValueError, KeyError):
            continue
        with pytest.raises(hb.TdsHipError, match="error 2: step Jacobians: f64 handles only"):
            s32.contacts_jvp(x, v)
    for name, why in (("pendulum5_spherical", "spherical joints"), ("pendulum_and_cube", "worlds of several bodies")):
        mr = tds_amd.load_model(name)
        sr = hb.HipSim(mr, 2, device=0, dtype="f64")
        with pytest.raises(hb.TdsHipError, match=f"error 2: step Jacobians: {why} are not supported"):
            sr.contacts_jvp(cu(np.zeros((2, mr.input_dim))), cu(np.zeros((2, 1, mr.input_dim))))
    sim = hb.HipSim(m, 4, device=0, dtype="f64")
    with pytest.raises(hb.TdsHipError) as e1:
        hb.params_get(m, [("mass", 99)])
    with pytest.raises(hb.TdsHipError) as e2:
        sim.contacts_jvp(x, cu(np.zeros((4, 1, m.input_dim + 1))), params=[("mass", 99)])
    assert str(e1.value) == str(e2.value)
    assert hb.lib().tds_hip_contacts_jvp(sim.h, 4, x.data_ptr(), 0, None, None, 1, v.data_ptr(), None,
                                         hb.ContactOut()) == 1  # no tangent requested


# ---------------------------------------------------------------- autograd
def kink_free_states(name, n):
    """the first n states of the sweep whose central differences see no branch switch within +- 2h"""
    m = tds_amd.load_model(name)
    x = sweep(name, 65)
    want = ("force", "qd_post")
    q = lambda z: np.concatenate([r.reshape(z.shape[0], -1) for r in hb.contacts_host(m, z, want=want).values()], axis=1)  # noqa: E731
    _, kink = ds.central_jacobian(m, x, step=q)
    hit = (hb.contacts_host(m, x, want=("contacts",))["contacts"][:, :, 9] < 0).any(axis=1)
    return x[~kink & hit][:n]


@pytest.mark.parametrize("shared", [True, False])
def test_gradcheck_of_contact_fn(shared, built):
    import torch

    name = "pendulum5_plane"
    m = tds_amd.load_model(name)
    g = int(hb.contact_layout(m)["geom"][0])
    sel = [("friction",), ("geom_radius", g)]
    xs = kink_free_states(name, 3)
    assert xs.shape[0] == 3
    sim = hb.HipSim(m, 3, device=0, dtype="f64")
    fn = tds_amd.contact_fn(sim, ("force", "qd_post"), params=sel)
    x = cu(xs).requires_grad_(True)
    th0 = cu(hb.params_get(m, sel))
    theta = (th0 if shared else th0.expand(3, 2).contiguous()).clone().requires_grad_(True)
    # atol: the error of such central differences measured on the CPU (MEASURED_X, relative to max(1, max |J|) of a
    # state), times ten, at the scale of this Jacobian
    J = torch.cat([sim.contacts_jacobian(x.detach(), k, params=sel).reshape(3, -1) for k in ("force", "qd_post")], 1)
    atol = 10 * MEASURED_X[name] * max(1.0, float(J.abs().max()))
    assert torch.autograd.gradcheck(fn, (x, theta), eps=1e-6, atol=atol, rtol=0.0, nondet_tol=0.0)


def test_friction_descent_on_the_ant(built):
    """six steps of gradient descent on the Ant's friction towards forces generated at another value: the loss falls
    at every step"""
    import torch

    m = tds_amd.load_model("ant")
    x = cu(sweep("ant", 65))
    sim = hb.HipSim(m, 65, device=0, dtype="f64")
    fn = tds_amd.contact_fn(sim, "force", params=[("friction",)])
    with torch.no_grad():
        target = fn(x, cu([0.6 * m.friction]))
    theta = cu([m.friction]).requires_grad_(True)
    losses = []
    for _ in range(7):
        loss = ((fn(x, theta) - target) ** 2).mean()
        (g,) = torch.autograd.grad(loss, theta)
        losses.append(float(loss.detach()))
        with torch.no_grad():
            theta -= 0.5 * loss / g  # half a Newton step on the loss's root
    print("friction descent:", ["%.4e" % v for v in losses], "theta", float(theta.detach()), "target", 0.6 * m.friction)
    assert all(b < a for a, b in zip(losses, losses[1:])) and losses[-1] < 0.5 * losses[0]
