"""Forward-mode derivatives of the dynamics queries on the GPU (tds_hip_dynamics_jvp / tds_hip_inverse_dynamics_jvp,
csrc/tds_dyn_jvp.hip) against their host instantiation, plus what a handle owes its other users (untouched outputs, the
shared work buffer, the stream, the refusals) and the autograd functions tds_amd.dynamics_fn / inverse_dynamics_fn."""
import numpy as np
import pytest

import tds_amd
from tds_amd import hip_backend as hb

from test_dynamics_cpu import split, wanted
from test_dynamics_derivs_cpu import MEASURED_FD, selection, thetas
from test_dynamics_gpu import MODELS, records, rel

pytestmark = pytest.mark.gpu

# Device against host: the same template without FP contraction on either side; only sin / cos are each side's own.
# The metric is test_dynamics_gpu.py's (|a - b| / max(|b|, 1), the maximum over an output).  Measured on the MI355X over
# every case of test_device_matches_host, primal outputs and tangents of both calls:
#   ant 1.30e-12, laikago 1.87e-13, ant_floating 1.15e-13, cartpole 4.26e-15, pendulum5_plane 2.35e-13,
#   cube_floating 0 (and 2.24e-13 over test_grid_stride_walk's pendulum5 sample); the largest figures are qdd's tangents.
# The tests assert 10 x the largest, which may not exceed 1e-9 (the bound the primal queries hold against the reference).
DEV_MEASURED = 1.30e-12
DEV_TOL = 10 * DEV_MEASURED
assert DEV_TOL <= 1e-9


def cu(a):
    import torch

    return None if a is None else torch.from_numpy(np.array(a, dtype=np.float64, order="C")).cuda()


def state(name, n, seed=0):
    """q, qd from the golden records, tau and qdd ~ N(0, 1)"""
    m = tds_amd.load_model(name)
    q, qd, _ = split(m, records(name, n, seed))
    rng = np.random.default_rng(2)
    return m, q, qd, rng.normal(0, 1.0, (n, hb.dyn_tau_dim(m))), rng.normal(0, 1.0, (n, m.dof_qd))


def directions(rng, n, k, width):
    """k directions: the whole identity where k == width, random ones otherwise"""
    if k == width:
        return np.ascontiguousarray(np.broadcast_to(np.eye(width), (n, width, width)))
    return rng.normal(size=(n, k, width))


def compare(name, sim, st, sel, th, k, rng, idx=None):
    """device tangents and primal of every output of both calls against the host's, on the environments idx (k None:
    every column of z); the worst error"""
    m, q, qd, tau, qdd = st
    n, p = q.shape[0], len(sel)
    idx = np.arange(n) if idx is None else idx
    pick = lambda a: None if a is None else a[idx]  # noqa: E731
    worst = 0.0

    def check(what, got, ref):
        nonlocal worst
        assert got.shape[1:] == ref.shape[1:] and np.all(np.isfinite(got)), (name, what)
        e = rel(got[idx], ref)
        print(f"{name} n {n} k {k} p {p} {what}: rel device-host {e:.2e}")
        worst = max(worst, e)
        assert e <= DEV_TOL, (name, what, e)

    width = hb.dyn_input_dim(m) + p
    v = directions(rng, n, width if k is None else k, width)
    tan, prim = sim.dynamics_jvp(cu(q), cu(qd), cu(tau), cu(v), want=wanted(m), params=sel, theta=cu(th), want_primal=True)
    ht, hp = hb.dynamics_jvp_host(m, q[idx], qd[idx], tau[idx], v[idx], want=wanted(m), params=sel, theta=pick(th),
                                  want_primal=True)
    for o in wanted(m):
        assert tuple(tan[o].shape) == hb.dyn_tangent_shapes(m, n, v.shape[1])[o]
        check("d " + o, tan[o].cpu().numpy(), ht[o])
        check(o, prim[o].cpu().numpy(), hp[o])
    if not m.is_floating:
        width = hb.dyn_input_dim(m, True) + p
        v = directions(rng, n, width if k is None else k, width)
        dt, t = sim.inverse_dynamics_jvp(cu(q), cu(qd), cu(qdd), cu(v), params=sel, theta=cu(th), want_primal=True)
        hdt, ht = hb.inverse_dynamics_jvp_host(m, q[idx], qd[idx], qdd[idx], v[idx], params=sel, theta=pick(th),
                                               want_primal=True)
        check("d tau", dt.cpu().numpy(), hdt)
        check("tau", t.cpu().numpy(), ht)
    return worst


@pytest.mark.parametrize("n", [1, 7, 65])
@pytest.mark.parametrize("name", MODELS)
def test_device_matches_host(name, n, built):
    """z = [q | qd | tau or qdd | theta] with the selection of the CPU tests at per-environment theta, and p = 0; k: one
    direction, a full block, a partial last block (zero-filled), and every column"""
    st = state(name, n)
    m = st[0]
    sel, K = selection(m, name), hb.dynamics_jvp_tangents(m)
    th = thetas(m, sel, n)
    rng = np.random.default_rng(7)
    sim = hb.HipSim(m, 8, device=0, dtype="f64")
    worst = 0.0
    for k in (1, K, K + 1, None):
        worst = max(worst, compare(name, sim, st, sel, th, k, rng))
    worst = max(worst, compare(name, sim, st, [], None, K + 1, rng))  # p = 0: the model's values
    print(f"{name} n {n}: max rel device-host {worst:.2e}")


def test_grid_stride_walk(built):
    """2100 environments x 9 blocks = 18 900 items on at most 16 384 lanes; the sample holds the last environments"""
    st = state("pendulum5", 2100)
    m = st[0]
    n, K = 2100, hb.dynamics_jvp_tangents(m)
    k = 8 * K + 1
    assert n * ((k + K - 1) // K) > 16384
    rng = np.random.default_rng(8)
    idx = np.concatenate([rng.choice(n - 16, 48, replace=False), np.arange(n - 16, n)])
    sim = hb.HipSim(m, 8, device=0, dtype="f64")
    compare("pendulum5", sim, st, [("mass", 1), ("gravity", 2)], None, k, rng, idx)


def test_only_requested_outputs_are_written_and_out_buffers_are_reused(built):
    import torch

    m, q, qd, tau, qdd = state("ant", 33)  # not the handle's num_envs
    n, k = 33, 3
    sel = [("mass", 5), ("gravity", 2)]
    nz = hb.dyn_input_dim(m) + 2
    q, qd, tau = cu(q), cu(qd), cu(tau)
    v = cu(np.random.default_rng(9).normal(size=(n, k, nz)))
    th = thetas(m, sel, n)
    sim = hb.HipSim(m, 8, device=0, dtype="f64")
    full, fullp = sim.dynamics_jvp(q, qd, tau, v, params=sel, theta=cu(th), want_primal=True)
    shapes, pshapes = hb.dyn_tangent_shapes(m, n, k), hb.dyn_shapes(m, n)
    poison = lambda s: {o: torch.full(s[o], -7.25, dtype=torch.float64, device="cuda") for o in hb.DYN_OUTPUTS}  # noqa: E731
    for want in (("mass_matrix",), ("qdd", "x_world"), ("bias",)):
        bufs = poison(shapes)
        res = sim.dynamics_jvp(q, qd, tau, v, want=want, params=sel, theta=cu(th), out=bufs)
        torch.cuda.synchronize()
        for o in hb.DYN_OUTPUTS:
            if o in want:
                assert res[o] is bufs[o] and torch.equal(bufs[o], full[o]), o
            else:
                assert o not in res and bool((bufs[o] == -7.25).all()), o
        # the raw entry point: primal and tangent sets chosen apart, the others poisoned
        pb = poison(pshapes)
        po = hb.DynOut(**{o: pb[o].data_ptr() for o in want})
        to = hb.DynOut(qdd=bufs["qdd"].data_ptr())
        assert hb.lib().tds_hip_dynamics_jvp(sim.h, n, q.data_ptr(), qd.data_ptr(), tau.data_ptr(), 2, hb.param_spec(sel),
                                             cu(th).data_ptr(), k, v.data_ptr(), po, to) == 0
        torch.cuda.synchronize()
        for o in hb.DYN_OUTPUTS:
            assert torch.equal(pb[o], fullp[o]) if o in want else bool((pb[o] == -7.25).all()), o
        assert torch.equal(bufs["qdd"], full["qdd"])
    # k = 0 at theta: the primal query on a handle created from the params_apply model
    prim = sim.dynamics_jvp(q, qd, tau, None, params=sel, theta=cu(th))
    for e in (0, 17, 32):
        other = hb.HipSim(hb.params_apply(m, sel, th[e]), 8, device=0, dtype="f64")
        ref = other.dynamics(q[e:e + 1], qd[e:e + 1], tau[e:e + 1])
        for o in hb.DYN_OUTPUTS:
            assert torch.equal(prim[o][e], ref[o][0]), (o, rel(prim[o][e].cpu().numpy(), ref[o][0].cpu().numpy()))
            assert torch.equal(prim[o][e], fullp[o][e]), o
    J = sim.dynamics_jacobian(q, qd, tau, "qdd", params=sel, theta=cu(th))
    eye = cu(np.broadcast_to(np.eye(nz), (n, nz, nz)))
    cols = sim.dynamics_jvp(q, qd, tau, eye, want=("qdd",), params=sel, theta=cu(th))["qdd"]
    assert J.shape == (n, m.dof_qd, nz) and torch.equal(J, cols.movedim(1, -1))
    some = sim.dynamics_jacobian(q, qd, tau, "qdd", cols=[3, nz - 1], params=sel, theta=cu(th))
    assert torch.equal(some, J[..., [3, nz - 1]])


def test_work_buffer_is_shared_with_the_other_calls(built):
    import torch

    m = tds_amd.load_model("ant")
    n = 16
    xn = records("ant", n)
    rng = np.random.default_rng(4)
    xd, v = cu(xn), cu(rng.normal(size=(n, 2, m.input_dim)))
    w = cu(rng.normal(size=(n, 2, m.output_dim)))
    q, qd = cu(xn[:, :m.dof_q]), cu(xn[:, m.dof_q:m.dof_q + m.dof_qd])
    sel = [("mass", 5), ("gravity", 2)]
    vc = cu(rng.normal(size=(n, 5, m.input_dim + 2)))
    vd = cu(rng.normal(size=(n, 5, hb.dyn_input_dim(m) + 2)))

    def others(sim):
        y, jv = sim.jvp(xd, v)
        _, wj = sim.vjp(xd, w)
        d = sim.dynamics(q, qd, want=("mass_matrix", "qdd"))
        c = sim.contacts_jvp(xd, vc, want=("impulse", "force"), params=sel)
        return [y, jv, wj, d["mass_matrix"], d["qdd"], c["impulse"], c["force"]]

    def mine(sim):
        t = sim.dynamics_jvp(q, qd, None, vd, params=sel)
        return [t[k] for k in hb.DYN_OUTPUTS] + [sim.inverse_dynamics_jvp(q, qd, None, vd, params=sel)]

    def same(a, b):
        return all(torch.equal(s, t) for s, t in zip(a, b))

    sim = hb.HipSim(m, n, device=0, dtype="f64")
    before, mine_before = others(sim), mine(sim)
    big = cu(np.tile(xn[:, :m.dof_q], (300, 1)))
    sim.dynamics_jvp(big, None, None, cu(rng.normal(size=(big.shape[0], 3, hb.dyn_input_dim(m) + 2))), want=("qdd",),
                     params=sel)  # grows the shared buffer
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

    m, q, qd, tau, qdd = state("ant", 256)
    n = 256
    sel = [("mass", 5)]
    v = np.random.default_rng(5).normal(size=(n, 3, hb.dyn_input_dim(m) + 1))
    sim = hb.HipSim(m, n, device=0, dtype="f64")
    names = ("mass_matrix", "qdd")
    want = sim.dynamics_jvp(cu(q), cu(qd), cu(tau), cu(v), want=names, params=sel)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    q_src, v_src, qd_dev, tau_dev = cu(q), cu(v), cu(qd), cu(tau)
    q_dev, v_dev = torch.zeros_like(q_src), torch.zeros_like(v_src)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        sim.use_current_stream()
        torch.cuda._sleep(200_000_000)  # ~0.1 s of device time ahead of the copies
        q_dev.copy_(q_src, non_blocking=True)
        v_dev.copy_(v_src, non_blocking=True)
        got = sim.dynamics_jvp(q_dev, qd_dev, tau_dev, v_dev, want=names, params=sel)
    side.synchronize()
    sim.use_current_stream()
    for k in want:
        assert torch.equal(got[k], want[k]), k


def test_refusals_on_the_device(built):
    m = tds_amd.load_model("ant")
    q = cu(records("ant", 4)[:, :m.dof_q])
    v = cu(np.zeros((4, 1, hb.dyn_input_dim(m))))
    for dt in ("f32", "mix"):
        try:
            s32 = hb.HipSim(m, 4, device=0, dtype=dt)
        except (hb.TdsHipError, ValueError, KeyError):
            continue
        with pytest.raises(hb.TdsHipError, match="error 2: step Jacobians: f64 handles only"):
            s32.dynamics_jvp(q, v=v)
        with pytest.raises(hb.TdsHipError, match="error 2: step Jacobians: f64 handles only"):
            s32.inverse_dynamics_jvp(q, v=v)
    for name, why in (("pendulum5_spherical", "spherical joints"), ("pendulum_and_cube", "worlds of several bodies")):
        mr = tds_amd.load_model(name)
        sr = hb.HipSim(mr, 2, device=0, dtype="f64")
        with pytest.raises(hb.TdsHipError, match=f"error 2: step Jacobians: {why} are not supported"):
            sr.dynamics_jvp(cu(np.zeros((2, mr.dof_q))), want=("mass_matrix",))
    mf = tds_amd.load_model("ant_floating")
    sf = hb.HipSim(mf, 2, device=0, dtype="f64")
    qf = cu(records("ant_floating", 2)[:, :mf.dof_q])
    vf = cu(np.zeros((2, 1, hb.dyn_input_dim(mf))))
    with pytest.raises(hb.TdsHipError, match="need a fixed base"):
        sf.dynamics_jvp(qf, v=vf, want=("bias",))
    with pytest.raises(hb.TdsHipError, match="need a fixed base"):
        sf.inverse_dynamics_jvp(qf)
    sim = hb.HipSim(m, 4, device=0, dtype="f64")
    with pytest.raises(hb.TdsHipError) as e1:
        hb.params_get(m, [("mass", 99)])
    with pytest.raises(hb.TdsHipError) as e2:
        sim.dynamics_jvp(q, v=cu(np.zeros((4, 1, hb.dyn_input_dim(m) + 1))), params=[("mass", 99)])
    assert str(e1.value) == str(e2.value)
    assert hb.lib().tds_hip_dynamics_jvp(sim.h, 4, q.data_ptr(), None, None, 0, None, None, 1, v.data_ptr(), None,
                                         hb.DynOut()) == 1  # no tangent requested


# ---------------------------------------------------------------- autograd
@pytest.mark.parametrize("shared", [True, False])
def test_gradcheck_of_dynamics_fn_and_inverse_dynamics_fn(shared, built):
    import torch

    m, q, qd, tau, qdd = state("pendulum5", 3)
    sel = [("mass", 2), ("gravity", 2)]
    sim = hb.HipSim(m, 3, device=0, dtype="f64")
    th0 = cu(hb.params_get(m, sel))
    theta = (th0 if shared else th0.expand(3, 2).contiguous()).clone().requires_grad_(True)
    q, qd, tau, qdd = (cu(a).requires_grad_(True) for a in (q, qd, tau, qdd))
    # atol: the error of such central differences measured on the CPU (MEASURED_FD, relative to max(1, max |J|) of a
    # state), times ten, at the scale of this Jacobian
    J = torch.cat([sim.dynamics_jacobian(q.detach(), qd.detach(), tau.detach(), k, params=sel).reshape(3, -1)
                   for k in ("qdd", "mass_matrix")], 1)
    atol = 10 * MEASURED_FD["pendulum5"] * max(1.0, float(J.abs().max()))
    fn = tds_amd.dynamics_fn(sim, ("qdd", "mass_matrix"), params=sel)
    assert torch.autograd.gradcheck(fn, (q, qd, tau, theta), eps=1e-6, atol=atol, rtol=0.0, nondet_tol=0.0)
    Ji = sim.inverse_dynamics_jvp(q.detach(), qd.detach(), qdd.detach(), cu(np.broadcast_to(np.eye(17), (3, 17, 17))),
                                  params=sel)
    atol = 10 * MEASURED_FD["pendulum5"] * max(1.0, float(Ji.abs().max()))
    fi = tds_amd.inverse_dynamics_fn(sim, params=sel)
    assert torch.autograd.gradcheck(fi, (q, qd, qdd, theta), eps=1e-6, atol=atol, rtol=0.0, nondet_tol=0.0)
