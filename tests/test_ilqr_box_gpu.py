"""Control-limited iLQR on the GPU (csrc/tds_lqr.hip): lqr_backward_box and the clamped feedback_rollout against their
host statements, the driver with u_limits on the device against the driver on the host checkers, and the handle's other
calls after a box call.

Bounds are 10 x the maximum measured over the cases below (largest |a - b| / max(|b|, 1), printed by each test):
  lqr_backward_box device vs host: 0 (every sum is one lane's, in the host's order, without contraction; every
    decision of the QP is formed from those sums: bit for bit, the clamped sets and iteration counts included)
  clamped feedback_rollout device vs host over T = 5 steps: the bounds recorded for the unclamped call in
    test_ilqr_gpu.py (measured with limits: cartpole 2.22e-16, ant 6.54e-13)
  ilqr(sim, u_limits) vs ilqr(model, u_limits), costs and trajectory after two iterations: cartpole, |u| <= 1: 2.442e-15;
    ant, "model" limits, N = 2, T = 8: 5.669e-14; alphas, clamped sets and status are equal"""
import ctypes as C

import numpy as np
import pytest
import torch

import tds_amd
from tds_amd import hip_backend as hb

from test_ilqr_cpu import err, golden_x, lq_problem, quadratic_cost
from test_ilqr_gpu import FB_DEV_BOUND, POISON, cu, fb_inputs, lqr_case, lqr_raw
from test_ilqr_box_cpu import bits, contact_case, fb_bounds

pytestmark = pytest.mark.gpu

LQR_BOX_DEV_BOUND = 10 * 0.0
ILQR_BOX_CARTPOLE_BOUND = 10 * 2.442e-15
ILQR_ANT_BOUND = 10 * 5.669e-14


@pytest.fixture(scope="module")
def cartpole_sim(built):
    return hb.HipSim(tds_amd.load_model("cartpole"), 16, device=0, dtype="f64")


def box_case(n, T, nx, nu):
    """the CPU file's bounds on the plain GPU test's problems: problem 0 without limits, control 0 of the last problem
    pinned, the middle problem (n >= 3) not positive definite, its indefinite step left free"""
    P, bad = lqr_case(n, T, nx, nu)
    rng = np.random.default_rng(100 * n + nx + 500000)
    dlo, dhi = -rng.uniform(0.0, 1.0, (n, T, nu)), rng.uniform(0.0, 1.0, (n, T, nu))
    if n >= 2:
        dlo[0], dhi[0] = -np.inf, np.inf
        dlo[-1, :, 0] = dhi[-1, :, 0] = rng.uniform(-0.5, 0.5, T)
    if bad:
        dlo[bad], dhi[bad] = -np.inf, np.inf
    return P, bad, dlo, dhi


def lqr_box_raw(sim, P, dlo, dhi, pad=64):
    """tds_hip_lqr_backward_box into buffers with `pad` poisoned entries behind what is due"""
    n, T, nx, nu = P[1].shape
    dev = [cu(a) for a in (*P, dlo, dhi)]
    sizes = {"k": n * T * nu, "K": n * T * nu * nx, "dv": n * 2}
    out = {key: torch.full((sz + pad,), POISON, dtype=torch.float64, device="cuda") for key, sz in sizes.items()}
    isizes = {"status": n, "clamped": n * T, "its": n * T}
    iout = {key: torch.full((sz + pad,), -7, dtype=torch.int32, device="cuda") for key, sz in isizes.items()}
    hb._check(hb.lib().tds_hip_lqr_backward_box(
        sim.h, n, T, nx, nu, *(C.c_void_p(t.data_ptr()) for t in dev),
        *(C.c_void_p(out[key].data_ptr()) for key in ("k", "K", "dv")),
        *(C.c_void_p(iout[key].data_ptr()) for key in ("status", "clamped", "its"))))
    torch.cuda.synchronize()
    for key, sz in sizes.items():
        assert bool((out[key][sz:] == POISON).all()), key
    for key, sz in isizes.items():
        assert bool((iout[key][sz:] == -7).all()), key
    return (out["k"][:n * T * nu].reshape(n, T, nu).cpu().numpy(),
            out["K"][:n * T * nu * nx].reshape(n, T, nu, nx).cpu().numpy(), out["dv"][:2 * n].reshape(n, 2).cpu().numpy(),
            iout["status"][:n].cpu().numpy(), iout["clamped"][:n * T].reshape(n, T).cpu().numpy(),
            iout["its"][:n * T].reshape(n, T).cpu().numpy())


@pytest.mark.parametrize("n,T,nx,nu", [(1, 1, 1, 1), (7, 3, 5, 2), (65, 9, 37, 12), (130, 2, 40, 16)])
def test_lqr_backward_box_matches_host(n, T, nx, nu, cartpole_sim):
    """both builds (28 x 8; 40 x 16 with more workgroups than one per compute unit pair), odd extents, T = 1 without a
    prefetch and T = 2 with one"""
    P, bad, dlo, dhi = box_case(n, T, nx, nu)
    want = hb.lqr_backward_box_host(*P, dlo, dhi)
    got = lqr_box_raw(cartpole_sim, P, dlo, dhi)
    e = max(err(g, w) for g, w in zip(got[:3], want[:3]))
    cl = bits(want[4], nu).sum(axis=-1)
    print(f"lqr_backward_box device vs host n={n} T={T} nx={nx} nu={nu}: {e:.3e}; {int(((cl > 0) & (cl < nu)).sum())} "
          f"of {cl.size} steps mixed, QP iterations <= {want[5].max()}")
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)
    assert e <= LQR_BOX_DEV_BOUND
    if bad:
        assert want[3][bad[0]] == bad[1] + 1 and int((want[3] != 0).sum()) == 1
        assert not any(g[bad[0]].any() for g in got[:3]) and not got[4][bad[0]].any() and not got[5][bad[0]].any()
    if n >= 2:
        assert not got[4][0].any() and bits(got[4][-1], nu)[:, 0].all() and not got[1][-1][:, 0].any()
        np.testing.assert_array_equal(got[0][-1][:, 0], dlo[-1, :, 0])
    if n >= 7:
        assert ((cl > 0) & (cl < nu)).any()
    # the python call returns the same
    res = cartpole_sim.lqr_backward_box(*(cu(a) for a in (*P, dlo, dhi)))
    for a, b in zip(res, got):
        np.testing.assert_array_equal(a.cpu().numpy(), b)


@pytest.mark.parametrize("n,T,nx,nu", [(1, 1, 1, 1), (7, 3, 5, 2), (65, 9, 37, 12), (130, 2, 40, 16)])
def test_infinite_bounds_on_the_device_are_the_devices_plain_pass(n, T, nx, nu, cartpole_sim):
    P, bad = lqr_case(n, T, nx, nu)
    inf = np.full((n, T, nu), np.inf)
    got = lqr_box_raw(cartpole_sim, P, -inf, inf)
    for g, w in zip(got[:4], lqr_raw(cartpole_sim, P)):
        np.testing.assert_array_equal(g, w)
    ok = got[3] == 0
    assert not got[4].any() and (got[5][ok] == 2).all() and not got[5][~ok].any()


def test_bounds_out_of_order_are_refused_by_the_wrapper(cartpole_sim):
    P, _, dlo, dhi = box_case(7, 3, 5, 2)
    bad = dhi.copy()
    bad[5, 1, 1] = -2.0
    with pytest.raises(ValueError, match="dlo > dhi"):
        cartpole_sim.lqr_backward_box(*(cu(a) for a in (*P, dlo, bad)))
    bad[5, 1, 1] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        cartpole_sim.lqr_backward_box(*(cu(a) for a in (*P, dlo, bad)))
    for nx, nu, word in ((41, 2, "40 state entries"), (3, 17, "16 controls")):
        Q = lq_problem(1, 1, 2, nx, nu)
        one = np.ones((1, 2, nu))
        with pytest.raises(hb.TdsHipError, match=f"error 2: tds_hip_lqr_backward_box: .*{word}"):
            cartpole_sim.lqr_backward_box(*(cu(a) for a in (*Q, -one, one)))
    m, F, _ = fb_inputs("cartpole", 3, False)
    lo, hi = fb_bounds(F[2])
    dev = [cu(a) for a in F]
    with pytest.raises(ValueError, match="u_lo > u_hi"):
        cartpole_sim.feedback_rollout(*dev, u_lo=cu(hi), u_hi=cu(lo))
    with pytest.raises(ValueError, match="together"):
        cartpole_sim.feedback_rollout(*dev, u_lo=cu(lo))


@pytest.fixture(scope="module")
def fb_sims(built):
    """handles of 16 environments: 65 rows are served in five launches of the step kernel, the last of one row"""
    return {name: hb.HipSim(tds_amd.load_model(name), 16, device=0, dtype="f64") for name in ("cartpole", "ant")}


@pytest.mark.parametrize("mapped", [False, True])
@pytest.mark.parametrize("rows", [1, 7, 65])
@pytest.mark.parametrize("name", ["cartpole", "ant"])
def test_clamped_feedback_rollout_matches_host(name, rows, mapped, fb_sims):
    m, P, por = fb_inputs(name, rows, mapped)
    lo, hi = fb_bounds(P[2], seed=rows)
    ws, wu = hb.feedback_rollout_host(m, *P, problem_of_row=por, u_lo=lo, u_hi=hi)
    pd = None if por is None else cu(por.astype(np.int32))
    gs, gu = fb_sims[name].feedback_rollout(*(cu(a) for a in P), problem_of_row=pd, u_lo=cu(lo), u_hi=cu(hi))
    torch.cuda.synchronize()
    gs, gu = gs.cpu().numpy(), gu.cpu().numpy()
    e = max(err(gs, ws), err(gu, wu))
    own = np.arange(rows) if por is None else por
    at_lo, at_hi = gu == lo[own], gu == hi[own]
    print(f"clamped feedback_rollout device vs host {name} rows={rows} mapped={mapped}: {e:.3e}; "
          f"{int((at_lo | at_hi).sum())} of {gu.size} actions at a bound")
    assert (gu >= lo[own]).all() and (gu <= hi[own]).all()
    # clamped entries are exactly at the bound, and the same entries as on the host
    np.testing.assert_array_equal(at_lo, wu == lo[own])
    np.testing.assert_array_equal(at_hi, wu == hi[own])
    assert (at_lo | at_hi).any() and not (at_lo | at_hi).all()
    assert np.isfinite(ws).all() and e <= FB_DEV_BOUND[name]
    # limits beyond reach: the call without limits
    inf = cu(np.full(lo.shape, np.inf))
    for a, b in zip(fb_sims[name].feedback_rollout(*(cu(a) for a in P), problem_of_row=pd, u_lo=-inf, u_hi=inf),
                    fb_sims[name].feedback_rollout(*(cu(a) for a in P), problem_of_row=pd)):
        assert torch.equal(a, b)


def test_ilqr_with_limits_on_the_device_follows_the_host_driver(cartpole_sim):
    """the CPU file's cartpole case, two iterations (the host takes the full step in both)"""
    m = cartpole_sim.model
    nsd, n_act, _ = hb.trajectory_dims(m, 1)
    N, T = 3, 40
    x0 = golden_x("cartpole", [0, 5, 9])
    u0 = np.random.default_rng(41).uniform(-2.0, 2.0, (N, T, n_act))
    cost = quadratic_cost(m)
    host = tds_amd.ilqr(m, x0, u0, cost, iterations=2, u_limits=(-1.0, 1.0))
    dev = tds_amd.ilqr(cartpole_sim, x0, u0, cost, iterations=2, u_limits=(-1.0, 1.0))
    torch.cuda.synchronize()
    e = max(err(dev[key].cpu().numpy(), host[key].numpy()) for key in ("cost", "s", "u"))
    print(f"ilqr with limits, device vs host, cartpole: alphas {dev['alpha'].cpu().numpy().tolist()}, costs and "
          f"trajectory {e:.3e}, clamped steps {int((host['clamped'] != 0).sum())} of {N * T}")
    assert dev["clamped"].is_cuda and bool((host["alpha"] > 0).all())
    assert torch.equal(dev["alpha"].cpu(), host["alpha"]) and torch.equal(dev["status"].cpu(), host["status"])
    assert torch.equal(dev["clamped"].cpu(), host["clamped"]) and bool((host["clamped"] != 0).any())
    assert bool((dev["u"].abs() <= 1.0).all())
    assert e <= ILQR_BOX_CARTPOLE_BOUND


def test_ilqr_with_model_limits_on_the_ant_follows_the_host_driver(built):
    m, x0, u0 = contact_case("ant")
    sim = hb.HipSim(m, 16, device=0, dtype="f64")
    cost = quadratic_cost(m)
    host = tds_amd.ilqr(m, x0, u0, cost, iterations=2, mu0=0.01, u_limits="model")
    dev = tds_amd.ilqr(sim, x0, u0, cost, iterations=2, mu0=0.01, u_limits="model")
    torch.cuda.synchronize()
    e = max(err(dev[key].cpu().numpy(), host[key].numpy()) for key in ("cost", "s", "u"))
    print(f"ilqr with model limits, device vs host, ant: alphas {dev['alpha'].cpu().numpy().tolist()}, costs and "
          f"trajectory {e:.3e}, clamped steps {int((host['clamped'] != 0).sum())} of {host['clamped'].numel()}")
    assert torch.equal(dev["alpha"].cpu(), host["alpha"]) and bool((host["alpha"] > 0).all())
    assert torch.equal(dev["status"].cpu(), host["status"])
    assert torch.equal(dev["clamped"].cpu(), host["clamped"]) and bool((host["clamped"] != 0).any())
    assert bool((dev["u"].abs() <= m.action_limit).all())
    assert e <= ILQR_ANT_BOUND


def test_the_handle_serves_its_other_calls_after_a_box_call(built):
    """plain lqr_backward, feedback_rollout and step give unchanged results after the box calls"""
    name = "ant"
    m, F, _ = fb_inputs(name, 7, False)
    sim = hb.HipSim(m, 7, device=0, dtype="f64")
    dev = [cu(a) for a in F]
    lq, _, dlo, dhi = box_case(7, 3, 5, 2)
    lqd = [cu(a) for a in lq]
    x = cu(F[0])

    def others():
        out = list(sim.lqr_backward(*lqd)) + list(sim.feedback_rollout(*dev)) + [sim.forward_zero(x)]
        torch.cuda.synchronize()
        return out

    before = others()
    lo, hi = fb_bounds(F[2])
    box_first = list(sim.lqr_backward_box(*lqd, cu(dlo), cu(dhi))) + \
        list(sim.feedback_rollout(*dev, u_lo=cu(lo), u_hi=cu(hi)))
    mb, Fb, _ = fb_inputs(name, 65, False)
    lob, hib = fb_bounds(Fb[2])
    tile = lambda a: cu(np.tile(a, (40,) + (1,) * (a.ndim - 1)))  # noqa: E731  (2600 rows: a larger work buffer)
    sim.feedback_rollout(*(tile(a) for a in Fb), u_lo=tile(lob), u_hi=tile(hib))
    after = others()
    for a, b in zip(before, after):
        assert torch.equal(a, b)
    box_again = list(sim.lqr_backward_box(*lqd, cu(dlo), cu(dhi))) + \
        list(sim.feedback_rollout(*dev, u_lo=cu(lo), u_hi=cu(hi)))
    for a, b in zip(box_first, box_again):
        assert torch.equal(a, b)
