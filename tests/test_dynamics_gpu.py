"""Batched dynamics queries on the GPU (tds_hip_dynamics / _inverse_dynamics / _point_jacobian, csrc/tds_dyn.hip)
against their host instantiation, plus what a handle owes its other users: untouched outputs, the shared work buffer,
the stream, the refusals."""
import os

import numpy as np
import pytest

from conftest import ROOT

import tds_amd
from tds_amd import hip_backend as hb

from test_dynamics_cpu import spring_terms, split, wanted
from test_jacobian_cpu import needs_ref, make_ref

pytestmark = pytest.mark.gpu

# device against host: the same template, no FP contraction on either side; only sin / cos are the device's and the
# host's own.  The bound asked of every query is 1e-12; the measured maximum over the cases below is printed by the
# test (DESIGN 7b quotes it).
DEV_TOL = 1e-12
MODELS = ["ant", "laikago", "ant_floating", "cartpole", "pendulum5_plane", "cube_floating"]


def records(name, n, seed=0):
    g = np.load(os.path.join(ROOT, "tests", "golden", f"{name}.npz"))
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(g["x"][rng.integers(0, g["x"].shape[0], n)])


def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1.0))) if a.size else 0.0


def cu(a):
    import torch

    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def some_link(m):
    joints = [i for i in range(m.num_links) if m.links[i].joint_type != tds_amd.JOINT_FIXED]
    return max(joints) if joints else -1


# n: one lane, a ragged wave, one lane past a wave (more than one workgroup), a full grid; and on the smallest model
# 16 384 + 37 environments, past the lanes of a launch: the grid's stride and its ragged tail
LANE_CAP = 16384
CASES = [(name, n) for name in MODELS for n in (1, 7, 65, 4096)] + [("cartpole", LANE_CAP + 37)]


@pytest.mark.parametrize("name,n", CASES)
def test_device_matches_host(name, n, built):
    m = tds_amd.load_model(name)
    x = records(name, n)
    q, qd, _ = split(m, x)
    rng = np.random.default_rng(2)
    tau = rng.normal(0, 1.0, (n, hb.dyn_tau_dim(m)))
    pts = rng.normal(0, 0.3, (n, 3))
    link = some_link(m)
    sim = hb.HipSim(m, min(n, 64), device=0, dtype="f64")
    d = {k: v.cpu().numpy() for k, v in sim.dynamics(cu(q), cu(qd), cu(tau), want=wanted(m)).items()}
    jw = sim.point_jacobian(cu(q), link, cu(pts)).cpu().numpy()
    jl = sim.point_jacobian(cu(q), link, cu(pts), local=True).cpu().numpy()
    if n <= 65:
        idx = np.arange(n)
    elif n <= LANE_CAP:
        idx = np.random.default_rng(1).choice(n, 64, replace=False)
    else:  # every row past the cap and a sample below it
        idx = np.concatenate([np.random.default_rng(1).choice(LANE_CAP, 27, replace=False), np.arange(LANE_CAP, n)])
    h = hb.dynamics_host(m, q[idx], qd[idx], tau[idx], want=wanted(m))
    worst = 0.0
    for k in wanted(m):
        e = rel(d[k][idx], h[k])
        worst = max(worst, e)
        assert e <= DEV_TOL, (name, k, e)
    for got, loc in ((jw, False), (jl, True)):
        e = rel(got[idx], hb.point_jacobian_host(m, q[idx], link, pts[idx], local=loc))
        worst = max(worst, e)
        assert e <= DEV_TOL, (name, "jac", loc, e)
    if not m.is_floating:
        a = rng.normal(0, 2.0, qd.shape)
        t = sim.inverse_dynamics(cu(q), cu(qd), cu(a)).cpu().numpy()
        e = rel(t[idx], hb.inverse_dynamics_host(m, q[idx], qd[idx], a[idx]))
        worst = max(worst, e)
        assert e <= DEV_TOL, (name, "id", e)
    print(name, n, "max rel device-host", worst)


def test_only_requested_outputs_are_written(built):
    import torch

    m = tds_amd.load_model("ant")
    n = 33
    q, qd, _ = split(m, records("ant", n))
    sim = hb.HipSim(m, 8, device=0, dtype="f64")
    full = sim.dynamics(cu(q), cu(qd))
    shapes = hb.dyn_shapes(m, n)
    for want in (("mass_matrix",), ("qdd", "x_world"), ("bias",)):
        bufs = {k: torch.full(shapes[k], -7.25, dtype=torch.float64, device="cuda") for k in hb.DYN_OUTPUTS}
        sim.dynamics(cu(q), cu(qd), want=want, out=bufs)
        torch.cuda.synchronize()
        for k in hb.DYN_OUTPUTS:
            if k in want:
                assert torch.equal(bufs[k], full[k]), k
            else:
                assert bool((bufs[k] == -7.25).all()), k


def test_work_buffer_is_shared_with_the_step_derivatives(built):
    import torch

    m = tds_amd.load_model("ant")
    n = 16
    x = records("ant", n)
    q, qd, _ = split(m, x)
    rng = np.random.default_rng(4)
    xd, v = cu(x), cu(rng.normal(size=(n, 2, m.input_dim)))
    w = cu(rng.normal(size=(n, 2, m.output_dim)))
    sim = hb.HipSim(m, n, device=0, dtype="f64")
    y_b, jv_b = sim.jvp(xd, v)
    _, wj_b = sim.vjp(xd, w)
    d_b = sim.dynamics(cu(q), cu(qd))
    big = np.tile(q, (300, 1))  # a larger query grows the shared buffer
    sim.dynamics(cu(big), want=("mass_matrix",))
    y_a, jv_a = sim.jvp(xd, v)
    _, wj_a = sim.vjp(xd, w)
    assert torch.equal(y_a, y_b) and torch.equal(jv_a, jv_b) and torch.equal(wj_a, wj_b)
    d_a = sim.dynamics(cu(q), cu(qd))
    for k in d_b:
        assert torch.equal(d_a[k], d_b[k]), k
    fresh = hb.HipSim(m, n, device=0, dtype="f64").dynamics(cu(q), cu(qd))  # a handle that never ran a derivative
    for k in d_b:
        assert torch.equal(fresh[k], d_b[k]), k


def test_refusals_on_the_device(built):
    m = tds_amd.load_model("ant")
    q, qd, _ = split(m, records("ant", 4))
    for dt in ("f32", "mix"):
        try:
            s32 = hb.HipSim(m, 4, device=0, dtype=dt)
        except (hb.TdsHipError, ValueError, KeyError):
            continue
        with pytest.raises(hb.TdsHipError, match="error 2: step Jacobians: f64 handles only"):
            s32.dynamics(cu(q), cu(qd))
        with pytest.raises(hb.TdsHipError, match="f64 handles only"):
            s32.inverse_dynamics(cu(q), cu(qd))
        with pytest.raises(hb.TdsHipError, match="f64 handles only"):
            s32.point_jacobian(cu(q), 0, cu(np.zeros((4, 3))))
    ms = tds_amd.load_model("pendulum5_spherical")
    s2 = hb.HipSim(ms, 2, device=0, dtype="f64")
    with pytest.raises(hb.TdsHipError, match="error 2: step Jacobians: spherical joints are not supported"):
        s2.dynamics(cu(np.zeros((2, ms.dof_q))))
    sim = hb.HipSim(m, 4, device=0, dtype="f64")
    with pytest.raises(hb.TdsHipError, match="error 1: .*link index out of range"):
        sim.point_jacobian(cu(q), m.num_links, cu(np.zeros((4, 3))))
    mf = tds_amd.load_model("ant_floating")
    qf, qdf, _ = split(mf, records("ant_floating", 4))
    sf = hb.HipSim(mf, 4, device=0, dtype="f64")
    with pytest.raises(hb.TdsHipError, match="error 2: .*no floating-base inverse dynamics"):
        sf.dynamics(cu(qf), cu(qdf), want=("bias",))
    with pytest.raises(hb.TdsHipError, match="error 2: .*no floating-base inverse dynamics"):
        sf.inverse_dynamics(cu(qf), cu(qdf))


def test_query_runs_on_the_handles_stream(built):
    """the query is ordered after earlier work on the stream given with tds_hip_set_stream: its input is filled there,
    behind a long-running kernel, and the call is made without any host wait"""
    import torch

    m = tds_amd.load_model("ant")
    n = 256
    q, qd, _ = split(m, records("ant", n))
    sim = hb.HipSim(m, n, device=0, dtype="f64")
    want = sim.dynamics(cu(q), cu(qd), want=("mass_matrix", "qdd"))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    q_src, qd_dev, q_dev = cu(q), cu(qd), torch.zeros((n, m.dof_q), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        sim.use_current_stream()
        torch.cuda._sleep(200_000_000)  # ~0.1 s of device time ahead of the copy
        q_dev.copy_(q_src, non_blocking=True)
        got = sim.dynamics(q_dev, qd_dev, want=("mass_matrix", "qdd"))
    side.synchronize()
    sim.use_current_stream()
    for k in want:
        assert torch.equal(got[k], want[k]), k


@needs_ref
def test_device_matches_reference_on_the_ant(built):
    m = tds_amd.load_model("ant")
    n = 64
    x = records("ant", n, seed=3)
    q, qd, _ = split(m, x)
    sim = hb.HipSim(m, n, device=0, dtype="f64")
    d = {k: v.cpu().numpy() for k, v in sim.dynamics(cu(q), cu(qd), want=("x_world", "mass_matrix")).items()}
    r = make_ref("ant")
    try:
        for e in range(n):
            dbg = r.debug(x[e], m)
            assert rel(d["x_world"][e], dbg["X_world"]) <= 1e-9
            assert rel(d["mass_matrix"][e], dbg["M"]) <= 1e-9
    finally:
        r.close()


def test_computed_torque_reaches_the_commanded_acceleration(built):
    """tau = ID(q, qd, a*) + K q + D qd makes forward_dynamics return a*, for 4096 pendulum states"""
    m = tds_amd.load_model("pendulum5")
    n = 4096
    rng = np.random.default_rng(7)
    q, qd = rng.uniform(-np.pi, np.pi, (n, m.dof_q)), rng.normal(0, 2.0, (n, m.dof_qd))
    a_star = rng.normal(0, 3.0, (n, m.dof_qd))
    sim = hb.HipSim(m, 64, device=0, dtype="f64")
    tau = sim.inverse_dynamics(cu(q), cu(qd), cu(a_star)) + cu(spring_terms(m, q, qd))
    a = sim.forward_dynamics(cu(q), cu(qd), tau).cpu().numpy()
    err = rel(a, a_star)
    print("computed torque: max rel |a - a*| =", err)
    # the solve's bound: 10 x the largest difference measured for qdd on the CPU (tests/test_dynamics_cpu.py)
    from test_dynamics_cpu import QDD_BOUND

    assert err <= QDD_BOUND
