"""Batched system identification on the GPU (csrc/tds_lm.hip): lm_step against its host statement, the driver on the
device against the driver on the host checkers, and what a handle owes its other users: untouched memory, the shared
work buffer, the stream, the refusals.

Bounds are 10 x the maximum measured over the cases below (largest |a - b| / max(|b|, 1), printed by each test):
  lm_step device vs host, every output, and the cost-only mode: 0 (every sum is one lane's, in the host's order,
    without contraction: bit for bit)
  sysid(sim) vs sysid(model), case (a), two iterations: costs 1.31e-18 (they are 3e-3, 4e-5, 6e-9: the
    denominator is 1), theta 4.35e-15 (the trajectory kernels' sin / cos differ from the host's in the last places)
  sysid(sim) to convergence: case (a) and case (b) T = 6 within the CPU file's bounds"""
import ctypes as C

import numpy as np
import pytest
import torch

import tds_amd
from tds_amd import hip_backend as hb

from test_param_derivs_gpu import SYSID_SEL, SYSID_T
from test_sysid_cpu import ANT_SEL, CASE_A_BOUND, CASE_B_BOUND, case_a, case_b, check_run, err, lm_case

pytestmark = pytest.mark.gpu

LM_DEV_BOUND = 10 * 0.0
DEV_COST_BOUND, DEV_THETA_BOUND = 10 * 1.31e-18, 10 * 4.35e-15
POISON = -7.25
INPUTS = ("s", "s_obs", "w", "js", "dlo", "dhi", "lam")


def cu(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def cartpole_sim(built):
    return hb.HipSim(tds_amd.load_model("cartpole"), 16, device=0, dtype="f64")


def device_case(n, counts, m, p, L):
    """the CPU file's problems; the largest shape carries an empty problem (its counts), a problem with a NaN entry,
    a pinned parameter and a problem without bounds"""
    case = {k: None if v is None else v.copy() for k, v in lm_case(500 + n + p, n, counts, m, p, L).items()}
    marks = {}
    if n >= 100:
        rs = case["row_start"]
        marks = {"empty": counts.index(0), "nan": 17, "pinned": 40, "free": 99}
        case["s"][rs[17], 11], case["w"][rs[17], 11] = np.nan, 1.0
        case["dlo"][40, 3] = case["dhi"][40, 3] = 0.0
        case["dlo"][99], case["dhi"][99] = -np.inf, np.inf
    return case, marks


def lm_raw(sim, case, pad=64):
    """tds_hip_lm_step into buffers with `pad` poisoned entries behind what is due"""
    n, (rows, p, m), L = len(case["row_start"]) - 1, case["js"].shape, case["lam"].shape[1]
    dev = [cu(case[k]) for k in INPUTS]
    rs = cu(case["row_start"])
    shapes = {"cost": (n,), "g": (n, p), "H": (n, p, p), "delta": (n, L, p), "pred": (n, L), "clamped": (n, L),
              "qp_iterations": (n, L), "status": (n, L)}
    out = {}
    for k in hb.LM_OUTPUTS:
        ints = k in hb.LM_OUTPUTS[5:]
        out[k] = torch.full((int(np.prod(shapes[k])) + pad,), -7 if ints else POISON,
                            dtype=torch.int32 if ints else torch.float64, device="cuda")
    hb._check(hb.lib().tds_hip_lm_step(sim.h, n, rows, m, p, L, C.c_void_p(rs.data_ptr()),
                                       *(C.c_void_p(t.data_ptr()) for t in dev),
                                       *(C.c_void_p(out[k].data_ptr()) for k in hb.LM_OUTPUTS)))
    torch.cuda.synchronize()
    res = {}
    for k in hb.LM_OUTPUTS:
        size = int(np.prod(shapes[k]))
        assert bool((out[k][size:] == (-7 if k in hb.LM_OUTPUTS[5:] else POISON)).all()), k
        res[k] = out[k][:size].reshape(shapes[k]).cpu().numpy()
    return res


@pytest.mark.parametrize("n,counts,m,p,L", [(1, (1,), 1, 1, 1), (7, (1, 2, 3, 1, 3, 2, 1), 37, 2, 3),
                                            (65, (2,) * 65, 130, 12, 2), (130, (1,) * 60 + (0,) + (1,) * 69, 64, 16, 5)])
def test_lm_step_matches_host(n, counts, m, p, L, cartpole_sim):
    """m = 1: one entry a tile; 37: a tile that spans rows; 130: three tiles a row, the last of two entries; 64: a full
    tile exactly.  p = 12 and 16 give two and three sums a lane, 65 and 130 problems more workgroups than a wave of them"""
    case, marks = device_case(n, counts, m, p, L)
    want = hb.lm_step_host(**case)
    got = lm_raw(cartpole_sim, case)
    finite = lambda a: np.where(np.isfinite(a), a, 0.0)  # noqa: E731  (cost = +inf of the NaN problem: compared below)
    e = max(err(finite(got[k]), finite(want[k])) for k in hb.LM_OUTPUTS[:5])
    print(f"lm_step device vs host n={n} m={m} p={p} L={L}: {e:.3e}")
    for k in hb.LM_OUTPUTS:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    if marks:
        assert not want["H"][marks["empty"]].any() and want["cost"][marks["empty"]] == 0
        assert (want["status"][marks["nan"]] == 2).all() and want["cost"][marks["nan"]] == np.inf
        assert int((want["status"] != 0).sum()) == L
        assert not want["delta"][marks["pinned"], :, 3].any() and want["delta"][marks["pinned"]].any()
        assert not want["clamped"][marks["free"]].any() and want["clamped"].any()
    assert e <= LM_DEV_BOUND
    # the python call returns the same
    py = cartpole_sim.lm_step(cu(case["row_start"]), *(cu(case[k]) for k in ("s", "s_obs", "js", "lam", "w", "dlo", "dhi")))
    for k in hb.LM_OUTPUTS:
        np.testing.assert_array_equal(py[k].cpu().numpy(), got[k], err_msg=k)


@pytest.mark.parametrize("n,counts,m", [(1, (1,), 1), (5, (3, 0, 2, 1, 4), 130), (200, (2,) * 200, 63)])
def test_cost_only_mode_matches_host(n, counts, m, cartpole_sim):
    case = lm_case(900 + n, n, counts, m, 1, 1)
    want = hb.lm_step_host(case["row_start"], case["s"], case["s_obs"], None, None, case["w"])
    got = cartpole_sim.lm_step(cu(case["row_start"]), cu(case["s"]), cu(case["s_obs"]), None, None, cu(case["w"]))
    assert list(got) == ["cost"]
    np.testing.assert_array_equal(got["cost"].cpu().numpy(), want["cost"])
    full = hb.lm_step_host(**case)
    np.testing.assert_array_equal(want["cost"], full["cost"])
    # without weights
    want1 = hb.lm_step_host(case["row_start"], case["s"], np.nan_to_num(case["s_obs"]), None)
    got1 = cartpole_sim.lm_step(cu(case["row_start"]), cu(case["s"]), cu(np.nan_to_num(case["s_obs"])), None)
    np.testing.assert_array_equal(got1["cost"].cpu().numpy(), want1["cost"])


@pytest.fixture(scope="module")
def pendulum_sim(built):
    return hb.HipSim(case_a()[0], 8, device=0, dtype="f64")


def test_sysid_on_the_device_follows_the_host_driver(pendulum_sim):
    """two iterations of case (a): the costs (3e-3, 4e-5, 6e-9) are far above the noise of the device's sin / cos, so
    the decisions are the host's"""
    m, base, true, x0, u, s_obs, weights = case_a()
    kw = dict(u=u, weights=weights, iterations=2)
    host = tds_amd.sysid(m, x0, s_obs, SYSID_SEL, base, SYSID_T, **kw)
    dev = tds_amd.sysid(pendulum_sim, x0, s_obs, SYSID_SEL, base, SYSID_T, **kw)
    torch.cuda.synchronize()
    assert dev["theta"].is_cuda and dev["s"].is_cuda and tuple(dev["cost_trace"].shape) == (3, 1)
    e_cost = err(dev["cost_trace"].cpu().numpy(), host["cost_trace"].numpy())
    e_theta = err(dev["theta"].cpu().numpy(), host["theta"].numpy())
    print(f"sysid device vs host, case (a), 2 iterations: picks {dev['pick_trace'].cpu().tolist()}, costs {e_cost:.3e}, "
          f"theta {e_theta:.3e}")
    assert torch.equal(dev["pick_trace"].cpu(), host["pick_trace"]) and bool((host["pick_trace"] >= 0).all())
    assert torch.equal(dev["reason"].cpu(), host["reason"])
    assert e_cost <= DEV_COST_BOUND and e_theta <= DEV_THETA_BOUND


def test_sysid_on_the_device_converges(pendulum_sim):
    m, base, true, x0, u, s_obs, weights = case_a()
    res = tds_amd.sysid(pendulum_sim, x0, s_obs, SYSID_SEL, base, SYSID_T, u=u, weights=weights, iterations=6)
    cpu = {k: v.cpu() for k, v in res.items()}
    check_run(cpu)
    e = float(np.max(np.abs(cpu["theta"][0].numpy() - true) / np.abs(true)))
    print(f"sysid(sim) case (a): costs {cpu['cost_trace'][:, 0].tolist()}, theta* relative error {e:.3e}")
    assert e <= CASE_A_BOUND
    mb, base_b, true_b, lo, hi, x0_b, s_obs_b = case_b(6)
    ant = hb.HipSim(mb, 4, device=0, dtype="f64")
    res = tds_amd.sysid(ant, x0_b, s_obs_b, ANT_SEL, base_b, 6, bounds=(lo, hi), iterations=8, ftol=0.0, ptol=0.0)
    cpu = {k: v.cpu() for k, v in res.items()}
    check_run(cpu)
    e = float(np.max(np.abs(cpu["theta"][0].numpy() - true_b) / np.abs(true_b)))
    print(f"sysid(sim) case (b) T=6: costs {cpu['cost_trace'][:, 0].tolist()}, theta* relative error {e:.3e}")
    assert e <= CASE_B_BOUND


def test_lm_step_runs_on_the_handles_stream(cartpole_sim):
    """ordered after earlier work on the stream set with tds_hip_set_stream: an input is filled there, behind a
    long-running kernel, and the call is made without any host wait"""
    sim = cartpole_sim
    case, _ = device_case(7, (1, 2, 3, 1, 3, 2, 1), 37, 2, 3)
    rs = cu(case["row_start"])
    dev = [cu(case[k]) for k in ("s", "s_obs", "js", "lam", "w", "dlo", "dhi")]
    want = sim.lm_step(rs, *dev, check=False)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    js_late = torch.zeros_like(dev[2])
    torch.cuda.synchronize()
    try:
        with torch.cuda.stream(side):
            sim.use_current_stream()
            torch.cuda._sleep(200_000_000)  # ~0.1 s of device time ahead of the copy
            js_late.copy_(dev[2], non_blocking=True)
            got = sim.lm_step(rs, dev[0], dev[1], js_late, *dev[3:], check=False)
        side.synchronize()
    finally:
        sim.use_current_stream()
    for k in hb.LM_OUTPUTS:
        assert torch.equal(got[k], want[k]), k


def test_the_handle_serves_its_other_calls_as_before(built):
    """jacobian, jvp and trajectory_jvp on the same handle are identical before and after lm_step and sysid (whose
    candidate rollout grows the shared work buffer), and lm_step after them; n is independent of num_envs"""
    m, base, true, x0, u, s_obs, weights = case_a()
    sim = hb.HipSim(m, 4, device=0, dtype="f64")  # (8 rows, 40 candidate rows: several launches of 4 environments)
    x = cu(x0)
    v = cu(np.random.default_rng(3).normal(size=(8, 2, m.input_dim)))

    def others():
        jac = sim.jacobian(x)
        y, jv = sim.jvp(x, v)
        s, js = sim.trajectory_jvp(x, v, 5)
        torch.cuda.synchronize()
        return [jac, y, jv, s, js]

    case, _ = device_case(65, (2,) * 65, 130, 12, 2)
    args = [cu(case["row_start"])] + [cu(case[k]) for k in ("s", "s_obs", "js", "lam", "w", "dlo", "dhi")]
    first = sim.lm_step(*args)  # a handle that has run nothing else; 65 problems on a handle of 4 environments
    before = others()
    res = tds_amd.sysid(sim, x0, s_obs, SYSID_SEL, base, SYSID_T, u=u, weights=weights, iterations=1)
    sim.lm_step(*args)
    after = others()
    for a, b in zip(before, after):
        assert torch.equal(a, b)
    again = sim.lm_step(*args)
    for k in hb.LM_OUTPUTS:
        assert torch.equal(first[k], again[k]), k
    assert float(res["cost"][0]) < float(res["cost_trace"][0, 0])


def test_refusals_on_the_device(cartpole_sim):
    case = lm_case(3, 2, (1, 2), 9, 3, 2)
    rs = cu(case["row_start"])
    dev = {k: cu(case[k]) for k in INPUTS}
    call = lambda **kw: cartpole_sim.lm_step(**{"row_start": rs, **dev, **kw})  # noqa: E731
    with pytest.raises(hb.TdsHipError, match="error 2: tds_hip_lm_step: p exceeds the bound of 16 parameters"):
        call(js=torch.ones((3, 17, 9), dtype=torch.float64, device="cuda"), dlo=None, dhi=None)
    with pytest.raises(hb.TdsHipError, match="error 2: tds_hip_lm_step: n_lambda exceeds the bound of 8 candidates"):
        call(lam=torch.ones((2, 9), dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError, match="row_start: not non-decreasing from 0 to rows = 3"):
        call(row_start=cu(np.array([0, 2, 1], dtype=np.int32)))
    with pytest.raises(ValueError, match="row_start: not non-decreasing from 0 to rows = 3"):
        call(row_start=cu(np.array([0, 1, 2], dtype=np.int32)))
    with pytest.raises(ValueError, match="dlo > dhi somewhere, or a NaN bound"):
        call(dhi=dev["dlo"] - 1.0)
    with pytest.raises(ValueError, match="lam: a lambda that is not positive and finite"):
        call(lam=-dev["lam"])
    with pytest.raises(ValueError, match="lam: a lambda that is not positive and finite"):
        call(lam=dev["lam"] * float("inf"))
    with pytest.raises(ValueError, match="dlo and dhi are given together or not at all"):
        call(dhi=None)
    for bad in (rs.long(), rs.cpu()):
        with pytest.raises(ValueError, match="row_start: expected"):
            call(row_start=bad)
    for bad in (dev["w"][:, :8], dev["w"].float(), dev["w"].cpu()):
        with pytest.raises(ValueError, match=r"w: expected a CUDA float64 tensor \[3, 9\], got "):
            call(w=bad)
    with pytest.raises(ValueError, match=r"js: expected \[3, p, m\]"):
        call(js=dev["js"][:2])
    # what trajectory_jvp refuses reaches the caller of sysid unchanged
    m, base, true, x0, u, s_obs, weights = case_a()
    for dt in ("f32", "mixed"):
        s32 = hb.HipSim(m, 4, device=0, dtype=dt)
        with pytest.raises(hb.TdsHipError, match="error 2: .*f64 handles only"):
            tds_amd.sysid(s32, x0, s_obs, SYSID_SEL, base, SYSID_T, u=u, iterations=1)
    ms = tds_amd.load_model("pendulum5_spherical")
    nsd = ms.dof_q + ms.dof_qd
    ss = hb.HipSim(ms, 2, device=0, dtype="f64")
    with pytest.raises(hb.TdsHipError, match="error 2: .*spherical joints are not supported"):
        tds_amd.sysid(ss, np.zeros((2, ms.input_dim)), np.zeros((2, 3, nsd)), [("gravity", 2)], [-9.81], 3, iterations=1)
