"""Batched iLQR on the GPU (csrc/tds_lqr.hip): lqr_backward and feedback_rollout against their host statements, the
driver on the device against the driver on the host checkers, and what a handle owes its other users: untouched
memory, the shared work buffer, the stream, the refusals.

Bounds are 10 x the maximum measured over the cases below (largest |a - b| / max(|b|, 1), printed by each test):
  lqr_backward device vs host: 0 (every sum is one lane's, in the host's order, without contraction: bit for bit)
  feedback_rollout device vs host over T = 5 steps (the step kernels contract products, the host step does not):
    cartpole 2.22e-16, pendulum5_plane 8.80e-12, ant 8.83e-13, ant_floating 2.04e-13
  (pendulum5_plane: the seeded feedback drives the chain into the ground at several hundred rad/s, where a step
  amplifies the last places most)
  ilqr(sim) vs ilqr(model), cartpole, the costs of 4 iterations: 5.62e-16; with the default alphas, costs and
  trajectory after 2 iterations: 1.23e-15"""
import ctypes as C

import numpy as np
import pytest
import torch

import tds_amd
from tds_amd import hip_backend as hb

from test_ilqr_cpu import FB_MODELS, err, golden_x, lq_problem, quadratic_cost

pytestmark = pytest.mark.gpu

LQR_DEV_BOUND = 10 * 0.0
FB_DEV_BOUND = {"cartpole": 10 * 2.22e-16, "pendulum5_plane": 10 * 8.80e-12, "ant": 10 * 8.83e-13,
                "ant_floating": 10 * 2.04e-13}
ILQR_COST_BOUND = 10 * 5.62e-16
ILQR_DEFAULT_BOUND = 10 * 1.23e-15
POISON = -7.25


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def cartpole_sim(built):
    return hb.HipSim(tds_amd.load_model("cartpole"), 16, device=0, dtype="f64")


def lqr_case(n, T, nx, nu):
    """the CPU file's well-conditioned problems, an indefinite luu in the middle of the batch (n >= 3)"""
    P = lq_problem(100 * n + nx, n, T, nx, nu)
    bad = None
    if n >= 3:
        bad = (n // 2, T // 2)
        P[5][bad] = -50.0 * np.eye(nu)
    return P, bad


def lqr_raw(sim, P, pad=64):
    """tds_hip_lqr_backward into buffers with `pad` poisoned entries behind what is due"""
    n, T, nx, nu = P[1].shape
    dev = [cu(a) for a in P]
    sizes = {"k": n * T * nu, "K": n * T * nu * nx, "dv": n * 2}
    out = {key: torch.full((sz + pad,), POISON, dtype=torch.float64, device="cuda") for key, sz in sizes.items()}
    status = torch.full((n + pad,), -7, dtype=torch.int32, device="cuda")
    hb._check(hb.lib().tds_hip_lqr_backward(sim.h, n, T, nx, nu, *(C.c_void_p(t.data_ptr()) for t in dev),
                                            *(C.c_void_p(out[key].data_ptr()) for key in ("k", "K", "dv")),
                                            C.c_void_p(status.data_ptr())))
    torch.cuda.synchronize()
    for key, sz in sizes.items():
        assert bool((out[key][sz:] == POISON).all()), key
    assert bool((status[n:] == -7).all())
    return (out["k"][:n * T * nu].reshape(n, T, nu).cpu().numpy(), out["K"][:n * T * nu * nx].reshape(n, T, nu, nx).cpu().numpy(),
            out["dv"][:2 * n].reshape(n, 2).cpu().numpy(), status[:n].cpu().numpy())


@pytest.mark.parametrize("n,T,nx,nu", [(1, 1, 1, 1), (7, 3, 5, 2), (65, 9, 37, 12), (130, 2, 40, 16)])
def test_lqr_backward_matches_host(n, T, nx, nu, cartpole_sim):
    """(65, 9, 37, 12) and (130, 2, 40, 16) run the 40 x 16 build with more workgroups than one per compute unit pair,
    the others the 28 x 8 build; T = 1 has no prefetch, T = 2 one"""
    P, bad = lqr_case(n, T, nx, nu)
    want = hb.lqr_backward_host(*P)
    got = lqr_raw(cartpole_sim, P)
    e = max(err(g, w) for g, w in zip(got[:3], want[:3]))
    print(f"lqr_backward device vs host n={n} T={T} nx={nx} nu={nu}: {e:.3e}")
    np.testing.assert_array_equal(got[3], want[3])
    if bad:
        assert want[3][bad[0]] == bad[1] + 1 and int((want[3] != 0).sum()) == 1
        assert not got[0][bad[0]].any() and not got[1][bad[0]].any() and not got[2][bad[0]].any()
    assert e <= LQR_DEV_BOUND
    # the python call returns the same
    k, K, dv, status = cartpole_sim.lqr_backward(*(cu(a) for a in P))
    for a, b in zip((k, K, dv, status), got):
        np.testing.assert_array_equal(a.cpu().numpy(), b)


def test_lqr_backward_runs_on_the_handles_stream(cartpole_sim):
    """ordered after earlier work on the stream set with tds_hip_set_stream: an input is filled there, behind a
    long-running kernel, and the call is made without any host wait"""
    sim = cartpole_sim
    P, _ = lqr_case(7, 3, 5, 2)
    dev = [cu(a) for a in P]
    want = sim.lqr_backward(*dev)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    A_late = torch.zeros_like(dev[0])
    torch.cuda.synchronize()
    try:
        with torch.cuda.stream(side):
            sim.use_current_stream()
            torch.cuda._sleep(200_000_000)  # ~0.1 s of device time ahead of the copy
            A_late.copy_(dev[0], non_blocking=True)
            got = sim.lqr_backward(A_late, *dev[1:])
        side.synchronize()
    finally:
        sim.use_current_stream()
    for g, w in zip(got, want):
        assert torch.equal(g, w)


def fb_inputs(name, rows, mapped, T=5):
    m = tds_amd.load_model(name)
    nsd, n_act, _ = hb.trajectory_dims(m, 1)
    rng = np.random.default_rng(rows + 7)
    P = max(1, rows // 2) if mapped else rows
    por = np.arange(rows)[::-1] % P if mapped else None
    x0 = golden_x(name, rng.integers(0, 48, rows))
    own = por if mapped else np.arange(rows)
    first = np.zeros(P, dtype=np.int64)
    first[own[::-1]] = np.arange(rows)[::-1]
    s_nom = x0[first, None, :nsd] + 0.05 * rng.normal(size=(P, T + 1, nsd))
    u_nom = rng.uniform(-0.3, 0.3, (P, T, n_act))
    k, K = 0.1 * rng.normal(size=(P, T, n_act)), 0.05 * rng.normal(size=(P, T, n_act, nsd))
    alpha = rng.uniform(0.1, 1.0, rows)
    return m, (x0, s_nom, u_nom, k, K, alpha), por


@pytest.fixture(scope="module")
def fb_sims(built):
    """handles of 16 environments: 65 rows are served in five launches of the step kernel, the last of one row"""
    return {name: hb.HipSim(tds_amd.load_model(name), 16, device=0, dtype="f64") for name in FB_MODELS}


@pytest.mark.parametrize("mapped", [False, True])
@pytest.mark.parametrize("rows", [1, 7, 65])
@pytest.mark.parametrize("name", FB_MODELS)
def test_feedback_rollout_matches_host(name, rows, mapped, fb_sims):
    m, P, por = fb_inputs(name, rows, mapped)
    ws, wu = hb.feedback_rollout_host(m, *P, problem_of_row=por)
    gs, gu = fb_sims[name].feedback_rollout(*(cu(a) for a in P),
                                            problem_of_row=None if por is None else cu(por.astype(np.int32)))
    torch.cuda.synchronize()
    e = max(err(gs.cpu().numpy(), ws), err(gu.cpu().numpy(), wu))
    print(f"feedback_rollout device vs host {name} rows={rows} mapped={mapped}: {e:.3e}")
    np.testing.assert_array_equal(gs[:, 0].cpu().numpy(), P[0][:, :ws.shape[2]])
    assert np.isfinite(ws).all() and e <= FB_DEV_BOUND[name]


def test_ilqr_on_the_device_follows_the_host_driver(cartpole_sim):
    """alphas without the full step: four iterations stay far from convergence, where the choice of alpha would be
    decided by the last places of the costs"""
    m = cartpole_sim.model
    nsd, n_act, _ = hb.trajectory_dims(m, 1)
    N, T = 3, 40
    x0 = golden_x("cartpole", [0, 5, 9])
    u0 = np.random.default_rng(41).uniform(-2.0, 2.0, (N, T, n_act))
    cost = quadratic_cost(m)
    kw = dict(iterations=4, alphas=(0.5, 0.25, 0.125))
    host = tds_amd.ilqr(m, x0, u0, cost, **kw)
    dev = tds_amd.ilqr(cartpole_sim, x0, u0, cost, **kw)
    torch.cuda.synchronize()
    assert dev["s"].is_cuda and tuple(dev["cost"].shape) == (5, N)
    e = err(dev["cost"].cpu().numpy(), host["cost"].numpy())
    print(f"ilqr device vs host: alphas {dev['alpha'].cpu().numpy().tolist()}, costs {e:.3e}")
    assert torch.equal(dev["alpha"].cpu(), host["alpha"]) and bool((host["alpha"] > 0).all())
    assert torch.equal(dev["status"].cpu(), host["status"]) and torch.equal(dev["mu"].cpu(), host["mu"])
    assert e <= ILQR_COST_BOUND


def test_ilqr_on_the_device_with_the_default_alphas(cartpole_sim):
    """what users call: the default line search, alpha = 1 included, for the two iterations in which the choice is
    clear-cut (the host takes the full step in both)"""
    m = cartpole_sim.model
    nsd, n_act, _ = hb.trajectory_dims(m, 1)
    N, T = 3, 40
    x0 = golden_x("cartpole", [0, 5, 9])
    u0 = np.random.default_rng(41).uniform(-2.0, 2.0, (N, T, n_act))
    cost = quadratic_cost(m)
    host = tds_amd.ilqr(m, x0, u0, cost, iterations=2)
    dev = tds_amd.ilqr(cartpole_sim, x0, u0, cost, iterations=2)
    torch.cuda.synchronize()
    e = max(err(dev["cost"].cpu().numpy(), host["cost"].numpy()), err(dev["s"].cpu().numpy(), host["s"].numpy()),
            err(dev["u"].cpu().numpy(), host["u"].numpy()))
    print(f"ilqr device vs host, default alphas: {dev['alpha'].cpu().numpy().tolist()}, costs and trajectory {e:.3e}")
    assert bool((host["alpha"] == 1.0).all()) and torch.equal(dev["alpha"].cpu(), host["alpha"])
    assert torch.equal(dev["status"].cpu(), host["status"]) and torch.equal(dev["mu"].cpu(), host["mu"])
    assert e <= ILQR_DEFAULT_BOUND


def test_the_handle_serves_its_other_calls_as_before(built):
    """jvp, vjp, dynamics and contacts on the same handle are identical before and after the new calls (a larger
    feedback rollout grows the shared work buffer), and the new calls after them"""
    name = "ant"
    m, P, por = fb_inputs(name, 7, False)
    n = 7
    x = cu(P[0])
    v = cu(np.random.default_rng(3).normal(size=(n, 2, m.input_dim)))
    w = cu(np.random.default_rng(4).normal(size=(n, m.output_dim)))
    q, qd = x[:, :m.dof_q].contiguous(), x[:, m.dof_q:m.dof_q + m.dof_qd].contiguous()
    sim = hb.HipSim(m, 16, device=0, dtype="f64")

    def others():
        y, jv = sim.jvp(x, v)
        y2, wj = sim.vjp(x, w)
        d = sim.dynamics(q, qd)
        c = sim.contacts(x)
        torch.cuda.synchronize()
        return [y, jv, y2, wj] + [d[k] for k in sorted(d)] + [c[k] for k in sorted(c)]

    dev = [cu(a) for a in P]
    fb_first = sim.feedback_rollout(*dev)  # a handle that has run nothing else
    lq, _ = lqr_case(7, 3, 5, 2)
    lq_first = sim.lqr_backward(*(cu(a) for a in lq))
    before = others()
    mb, Pb, _ = fb_inputs(name, 65, False)
    sim.feedback_rollout(*(cu(np.tile(a, (40,) + (1,) * (a.ndim - 1))) for a in Pb))  # 2600 rows: a larger buffer
    sim.lqr_backward(*(cu(a) for a in lq))
    after = others()
    for a, b in zip(before, after):
        assert torch.equal(a, b)
    for a, b in zip(fb_first, sim.feedback_rollout(*dev)):
        assert torch.equal(a, b)
    for a, b in zip(lq_first, sim.lqr_backward(*(cu(a) for a in lq))):
        assert torch.equal(a, b)


def test_refusals_on_the_device(cartpole_sim):
    for nx, nu, word in ((41, 2, "40 state entries"), (3, 17, "16 controls")):
        P = lq_problem(1, 1, 2, nx, nu)
        with pytest.raises(hb.TdsHipError, match=f"error 2: tds_hip_lqr_backward: .*{word}"):
            cartpole_sim.lqr_backward(*(cu(a) for a in P))
    m, P, _ = fb_inputs("cartpole", 3, False)
    dev = [cu(a) for a in P]
    with pytest.raises(ValueError, match="problem_of_row: entries outside"):
        cartpole_sim.feedback_rollout(*dev, problem_of_row=cu(np.array([0, 3, 1], dtype=np.int32)))
    with pytest.raises(ValueError, match="K: expected"):
        cartpole_sim.feedback_rollout(*dev[:4], dev[4][..., :3], dev[5])
    # the refusals no case above reaches: n = 2, T = 2, nx = 4, nu = 1; a feedback rollout of 3 rows
    L = [cu(a) for a in lq_problem(3, 2, 2, 4, 1)]
    one = torch.ones((2, 2, 1), dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match=r"A: expected \[n, T, nx, nx\] and B \[n, T, nx, nu\], got \(2, 2, 4, 4\) and \(2, 1, 4, 1\)"):
        cartpole_sim.lqr_backward(L[0], L[1][:, :1], *L[2:])
    with pytest.raises(ValueError, match=r"A: expected \[n, T, nx, nx\] and B"):
        cartpole_sim.lqr_backward_box(L[0][:, :, :3], *L[1:], -one, one)
    for bad in (L[6][..., :3], L[6].float(), L[6].cpu()):
        with pytest.raises(ValueError, match=r"lux: expected a CUDA float64 tensor \[2, 2, 1, 4\], got "):
            cartpole_sim.lqr_backward(*L[:6], bad, L[7])
        with pytest.raises(ValueError, match=r"lux: expected a CUDA float64 tensor \[2, 2, 1, 4\], got "):
            cartpole_sim.lqr_backward_box(*L[:6], bad, L[7], -one, one)
    for bad in (one[:, :1], one.float(), one.cpu()):
        with pytest.raises(ValueError, match=r"dhi: expected a CUDA float64 tensor \[2, 2, 1\], got "):
            cartpole_sim.lqr_backward_box(*L, -one, bad)
    with pytest.raises(ValueError, match=rf"x0: expected \[rows, {m.input_dim}\], got \[3, {m.input_dim - 1}\]"):
        cartpole_sim.feedback_rollout(dev[0][:, :-1], *dev[1:])
    with pytest.raises(ValueError, match=r"s_nom: expected \[P, T \+ 1, 4\] with T >= 1, got \[3, 6, 3\]"):
        cartpole_sim.feedback_rollout(dev[0], dev[1][..., :3], *dev[2:])
    with pytest.raises(ValueError, match=r"x0: expected a CUDA float64 tensor \[3, "):
        cartpole_sim.feedback_rollout(dev[0].float(), *dev[1:])
    with pytest.raises(ValueError, match=r"alpha: expected a CUDA float64 tensor \[3\], got \[2\]"):
        cartpole_sim.feedback_rollout(*dev[:5], dev[5][:2])
    with pytest.raises(ValueError, match=r"one row per problem \(3\), got 2"):
        cartpole_sim.feedback_rollout(dev[0][:2], *dev[1:5], dev[5][:2])
    por = cu(np.array([0, 2, 1], dtype=np.int32))
    for bad in (por[:2], por.long(), por.cpu()):
        with pytest.raises(ValueError, match=r"problem_of_row: expected a CUDA int32 tensor \[3\]"):
            cartpole_sim.feedback_rollout(*dev, problem_of_row=bad)
    lo, hi = -torch.ones_like(dev[2]), torch.ones_like(dev[2])
    for bad in (hi[:, :3], hi.float(), hi.cpu()):
        with pytest.raises(ValueError, match=rf"u_hi: expected a CUDA float64 tensor \[3, 5, {lo.shape[2]}\], got "):
            cartpole_sim.feedback_rollout(*dev, u_lo=lo, u_hi=bad)
    refused = 0
    for dt in ("f32", "mixed"):  # float arithmetic; double arithmetic over float records
        s32 = hb.HipSim(m, 4, device=0, dtype=dt)
        with pytest.raises(hb.TdsHipError, match="error 2: step Jacobians: f64 handles only"):
            s32.feedback_rollout(*dev)
        with pytest.raises(hb.TdsHipError, match="error 2: step Jacobians: f64 handles only"):
            tds_amd.ilqr(s32, P[0], P[2], quadratic_cost(m), iterations=1)
        refused += 1
    assert refused == 2
    z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")  # noqa: E731
    for name, why in (("pendulum5_spherical", "spherical joints are not supported"), ("two_cubes_floating", ".* not supported")):
        mr = tds_amd.load_model(name)
        nsd, n_act, _ = hb.trajectory_dims(mr, 1)
        sr = hb.HipSim(mr, 2, device=0, dtype="f64")
        with pytest.raises(hb.TdsHipError, match=f"error 2: step Jacobians: {why}"):
            sr.feedback_rollout(z(2, mr.input_dim), z(2, 3, nsd), z(2, 2, n_act), z(2, 2, n_act), z(2, 2, n_act, nsd), z(2))
        with pytest.raises(hb.TdsHipError, match=f"error 2: step Jacobians: {why}"):
            tds_amd.ilqr(sr, z(2, mr.input_dim), z(2, 2, n_act), quadratic_cost(mr), iterations=1)
