"""Batched inverse kinematics on the GPU (tds_hip_inverse_kinematics, csrc/tds_ik.hip) against its host instantiation,
environments of one wave that stop at different iterations, the reference's four-feet cases, and what a handle owes
its other users: untouched outputs, the shared work buffer, the stream, the refusals.

Device against host: the same statement without FP contraction on either side; only sin / cos are the device's and the
host's own, and up to 20 iterations carry that difference.  Iterations and status must be equal; q and the residual
agree within 10 x the maximum measured over the cases below (largest |a - b| / max(|b|, 1), printed by the test):
  transpose 1.25e-14 (pendulum5 x 16500),  pinv 1.14e-9 (pendulum5 x 4096),  damped LM 7.43e-14 (ant x 65)
Every other pinv figure is at most 1.5e-13; the pendulum's maximum is one sampled environment whose two targets on the
planar chain leave J close to a further rank loss, where a step carries eps cond(J)^2 (tests/test_ik_cpu.py).
"""
import numpy as np
import pytest

import tds_amd
from tds_amd import hip_backend as hb

from test_ik_cpu import DEFAULTS, METHODS, NAMES, fixture, fixture_case, rel, world_points
from test_dynamics_gpu import cu, records

pytestmark = pytest.mark.gpu

DEV_BOUND = {"transpose": 10 * 1.25e-14, "pinv": 10 * 1.14e-9, "damped_lm": 10 * 7.43e-14}
TOES = np.array([3, 7, 11, 15], dtype=np.int32)  # laikago_floating's toe links (fixed joints)
TARGET_LINKS = {"pendulum5": [2, 4], "ant": [7, 9, 11, 13], "laikago_floating": TOES, "ant_floating": [1, 3, 5, 7]}


def options(method):
    return dict(DEFAULTS, alpha=0.3 if method == hb.IK_TRANSPOSE else 0.5)


def draw(m, name, n, rng):
    """n environments: q_init from golden records, targets = the body points at a perturbed configuration"""
    q0 = np.ascontiguousarray(records(name, n, seed=int(rng.integers(1 << 30)))[:, :m.dof_q])
    qo = 7 if m.is_floating else 0
    if m.is_floating:
        q0[:, :4] /= np.linalg.norm(q0[:, :4], axis=1, keepdims=True)
    q1 = q0.copy()
    q1[:, qo:] += rng.normal(0, 0.15, (n, m.dof_q - qo))
    return q0, q1


def clean_rows(m, q0, links, pts, tgt, qref, method, o):
    """the generator's branch-margin rule on the HOST's own residuals and steps, per environment: at every iteration the
    residual is more than 1e-6 (relative) away from target_tolerance and sum delta^2 from step_tolerance^2; and no
    iteration moves a coordinate by more than one radian (beyond that the iteration map itself amplifies the last-place
    difference of the device's sin / cos: tests/test_ik_cpu.py).  Run i of the host with max_iterations = i ends with the
    q after i iterations and the residual of iteration i - 1."""
    ok = np.ones(q0.shape[0], dtype=bool)
    prev = q0
    tt, st2 = o["target_tolerance"], o["step_tolerance"] ** 2
    for i in range(1, o["max_iterations"] + 1):
        r = hb.inverse_kinematics_host(m, q0, links, tgt, pts, qref, method=method, **dict(o, max_iterations=i))
        ok &= np.abs(r["residual"] - tt) > 1e-6 * tt
        w = o["weight_reference"]  # q' = (1 - w) (q + alpha delta) + w q_ref
        step = (r["q"] if qref is None else (r["q"] - w * qref) / (1 - w)) - prev
        sq = np.sum((step / o["alpha"]) ** 2, axis=1)
        ok &= (np.abs(sq - st2) > 1e-6 * st2) & (np.abs(step).max(axis=1) <= 1.0)
        prev = r["q"]
    return ok


@pytest.mark.parametrize("name,n", [(name, n) for name in ("pendulum5", "ant", "laikago_floating", "ant_floating")
                                    for n in (1, 7, 65, 4096)] + [("pendulum5", 16500)])
def test_device_matches_host(name, n, built):
    """65 crosses a wave and a workgroup, 4096 runs in 256 workgroups of 16 lanes, 16500 walks the grid's stride past
    the 16 384 lanes of a launch (on the smallest model)"""
    m = tds_amd.load_model(name)
    links = np.asarray(TARGET_LINKS[name], dtype=np.int32)
    rng = np.random.default_rng(11)
    pts = rng.normal(0, 0.03, (len(links), 3))
    sim = hb.HipSim(m, min(n, 64), device=0, dtype="f64")
    worst = {k: 0.0 for k in METHODS}
    for method in METHODS.values():
        o = options(method)
        q0, q1 = draw(m, name, n, rng)
        tgt = world_points(m, q1, links, pts)
        qref = None
        if method == hb.IK_PINV:  # one method with a reference configuration
            qref, o["weight_reference"] = 0.5 * (q0 + q1), 0.1
            if m.is_floating:
                qref[:, :7] = q0[:, :7]
        idx = np.arange(n) if n <= 65 else np.sort(rng.choice(n, 64, replace=False))
        for _ in range(20):  # redraw the compared environments that sit on a threshold
            bad = idx[~clean_rows(m, q0[idx], links, pts, tgt[idx], None if qref is None else qref[idx], method, o)]
            if not len(bad):
                break
            q0[bad], q1b = draw(m, name, len(bad), rng)
            tgt[bad] = world_points(m, q1b, links, pts)
            if qref is not None:
                qref[bad] = 0.5 * (q0[bad] + q1b)
                qref[bad, :7 if m.is_floating else 0] = q0[bad, :7 if m.is_floating else 0]
        else:
            raise AssertionError("no clean draw")
        d = {k: v.cpu().numpy() for k, v in
             sim.inverse_kinematics(cu(q0), links, cu(tgt), pts, cu(qref), method=method, **o).items()}
        h = hb.inverse_kinematics_host(m, q0[idx], links, tgt[idx], pts, None if qref is None else qref[idx],
                                       method=method, **o)
        np.testing.assert_array_equal(d["iterations"][idx], h["iterations"])
        np.testing.assert_array_equal(d["status"][idx], h["status"])
        worst[NAMES[method]] = max(rel(d["q"][idx], h["q"]), rel(d["residual"][idx], h["residual"]))
        assert np.all(np.isin(d["status"], (hb.IK_FAILED, hb.IK_CONVERGED, hb.IK_REACHED)))
    print(name, n, "max rel device-host per method:", worst)
    for k in METHODS:
        assert worst[k] <= DEV_BOUND[k], (name, n, k, worst[k])


def test_lanes_of_one_wave_stop_at_different_iterations(built):
    """neighbouring environments stop at iterations 0, 3 and 12 and never; each equals its own single-environment call"""
    import torch

    name = "laikago_floating"
    m = tds_amd.load_model(name)
    o = dict(DEFAULTS, alpha=0.3, weight_reference=0.0)
    q0 = records(name, 1, seed=5)[:, :m.dof_q]
    q0[:, :4] /= np.linalg.norm(q0[:, :4])
    here = world_points(m, q0, TOES, np.zeros((4, 3)))[0]
    scales = np.concatenate([[0.0], np.geomspace(2e-4, 0.08, 120), [5.0]])
    cand = here[None] + scales[:, None, None] * np.array([1.0, 0.0, 0.0])
    h = hb.inverse_kinematics_host(m, np.repeat(q0, len(scales), axis=0), TOES, cand, method="pinv", **o)
    pick = []
    for want, status in ((0, hb.IK_REACHED), (3, hb.IK_REACHED), (12, hb.IK_REACHED), (20, hb.IK_FAILED)):
        hit = np.flatnonzero((h["iterations"] == want) & (h["status"] == status))
        assert len(hit), (want, status)
        pick.append(hit[len(hit) // 2])  # the middle of the range: away from the neighbouring counts
    tgt = np.tile(cand[pick], (16, 1, 1))
    sim = hb.HipSim(m, 64, device=0, dtype="f64")
    big = sim.inverse_kinematics(cu(np.repeat(q0, 64, axis=0)), TOES, cu(tgt), method="pinv", **o)
    assert big["iterations"].cpu().tolist() == [0, 3, 12, 20] * 16
    assert big["status"].cpu().tolist() == [hb.IK_REACHED, hb.IK_REACHED, hb.IK_REACHED, hb.IK_FAILED] * 16
    for j in range(4):
        one = sim.inverse_kinematics(cu(q0), TOES, cu(tgt[j:j + 1]), method="pinv", **o)
        for k in one:
            assert torch.equal(big[k][j::4], one[k].expand_as(big[k][j::4])), (j, k)
    assert torch.equal(big["q"][0], cu(q0)[0])


def test_fixture_four_feet_cases_on_the_device(built):
    g = fixture()
    rows = [i for i in range(int(g["kept"])) if str(g["model"][i]) == "laikago_floating" and int(g["k"][i]) == 4]
    assert len(rows) >= 4
    sim = hb.HipSim(tds_amd.load_model("laikago_floating"), 1, device=0, dtype="f64")
    from test_ik_cpu import FIXTURE_BOUND

    for i in rows:
        m, a, ref = fixture_case(g, i)
        kw = {k: v for k, v in a.items() if k not in ("q_init", "links", "targets", "body_points", "q_reference")}
        r = sim.inverse_kinematics(cu(a["q_init"]), a["links"], cu(a["targets"]), a["body_points"], cu(a["q_reference"]), **kw)
        assert (int(r["iterations"][0]), int(r["status"][0])) == (ref["iterations"], ref["status"]), i
        e = max(rel(r["q"][0].cpu().numpy(), ref["q"]), rel(float(r["residual"][0]), ref["residual"]))
        print("fixture case", i, NAMES[a["method"]], "device vs reference", e)
        assert e <= FIXTURE_BOUND[NAMES[a["method"]]] + DEV_BOUND[NAMES[a["method"]]]


def ant_batch(n, seed=3):
    m = tds_amd.load_model("ant")
    rng = np.random.default_rng(seed)
    links = np.asarray(TARGET_LINKS["ant"], dtype=np.int32)
    q0, q1 = draw(m, "ant", n, rng)
    return m, links, q0, world_points(m, q1, links, np.zeros((4, 3)))


def test_only_requested_outputs_are_written(built):
    import torch

    n = 33
    m, links, q0, tgt = ant_batch(n)
    sim = hb.HipSim(m, 8, device=0, dtype="f64")
    full = sim.inverse_kinematics(cu(q0), links, cu(tgt), alpha=0.5)
    poison = {"q": -7.25, "iterations": -7, "status": -7, "residual": -7.25}
    for want in (("q",), ("q", "status"), ("q", "iterations", "residual")):
        bufs = {k: torch.full_like(full[k], poison[k]) for k in full}
        got = sim.inverse_kinematics(cu(q0), links, cu(tgt), alpha=0.5, out={k: bufs[k] for k in want})
        torch.cuda.synchronize()
        assert set(got) == set(want)  # the others went in as NULL
        for k in full:
            if k in want:
                assert torch.equal(bufs[k], full[k]), k
            else:
                assert bool((bufs[k] == poison[k]).all()), k


def test_work_buffer_is_shared_with_the_other_calls(built):
    import torch
    from test_dynamics_cpu import split

    n = 16
    m, links, q0, tgt = ant_batch(n)
    x = records("ant", n)
    q, qd, _ = split(m, x)
    rng = np.random.default_rng(4)
    xd, v = cu(x), cu(rng.normal(size=(n, 2, m.input_dim)))
    sim = hb.HipSim(m, n, device=0, dtype="f64")
    ik_b = sim.inverse_kinematics(cu(q0), links, cu(tgt), alpha=0.5)  # a handle that has run nothing else
    y_b, jv_b = sim.jvp(xd, v)
    d_b = sim.dynamics(cu(q), cu(qd))
    big = 6000  # a larger call grows the shared buffer
    sim.inverse_kinematics(cu(np.tile(q0, (big // n, 1))), links, cu(np.tile(tgt, (big // n, 1, 1))), alpha=0.5)
    y_a, jv_a = sim.jvp(xd, v)
    d_a = sim.dynamics(cu(q), cu(qd))
    assert torch.equal(y_a, y_b) and torch.equal(jv_a, jv_b)
    for k in d_b:
        assert torch.equal(d_a[k], d_b[k]), k
    sim.dynamics(cu(np.tile(q, (1000, 1))), want=("mass_matrix",))  # and the other way round
    ik_a = sim.inverse_kinematics(cu(q0), links, cu(tgt), alpha=0.5)
    for k in ik_b:
        assert torch.equal(ik_a[k], ik_b[k]), k


def test_call_runs_on_the_handles_stream(built):
    """the call is ordered after earlier work on the stream given with tds_hip_set_stream: its input is filled there,
    behind a long-running kernel, and the call is made without any host wait"""
    import torch

    n = 256
    m, links, q0, tgt = ant_batch(n)
    sim = hb.HipSim(m, n, device=0, dtype="f64")
    want = sim.inverse_kinematics(cu(q0), links, cu(tgt), alpha=0.5)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    q_src, t_dev, q_dev = cu(q0), cu(tgt), torch.zeros((n, m.dof_q), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        sim.use_current_stream()
        torch.cuda._sleep(200_000_000)  # ~0.1 s of device time ahead of the copy
        q_dev.copy_(q_src, non_blocking=True)
        got = sim.inverse_kinematics(q_dev, links, t_dev, alpha=0.5)
    side.synchronize()
    sim.use_current_stream()
    for k in want:
        assert torch.equal(got[k], want[k]), k


def test_refusals_on_the_device(built):
    m, links, q0, tgt = ant_batch(4)
    for dt in ("f32", "mix"):
        try:
            s32 = hb.HipSim(m, 4, device=0, dtype=dt)
        except (hb.TdsHipError, ValueError, KeyError):
            continue
        with pytest.raises(hb.TdsHipError, match="error 2: step Jacobians: f64 handles only"):
            s32.inverse_kinematics(cu(q0), links, cu(tgt))
    ms = tds_amd.load_model("pendulum5_spherical")
    s2 = hb.HipSim(ms, 2, device=0, dtype="f64")
    with pytest.raises(hb.TdsHipError, match="error 2: step Jacobians: spherical joints are not supported"):
        s2.inverse_kinematics(cu(np.zeros((2, ms.dof_q))), [0], cu(np.zeros((2, 1, 3))))
    mb = tds_amd.load_model("two_cubes_floating")
    s3 = hb.HipSim(mb, 2, device=0, dtype="f64")
    with pytest.raises(hb.TdsHipError, match="error 2: step Jacobians: .* not supported"):
        s3.inverse_kinematics(cu(np.zeros((2, mb.dof_q))), [0], cu(np.zeros((2, 1, 3))))
    sim = hb.HipSim(m, 4, device=0, dtype="f64")
    with pytest.raises(hb.TdsHipError, match="error 1: inverse kinematics: link index out of range"):
        sim.inverse_kinematics(cu(q0), [m.num_links], cu(tgt[:, :1]))
    with pytest.raises(hb.TdsHipError, match="error 1: inverse kinematics: 1 to 4 targets"):
        sim.inverse_kinematics(cu(q0), [0] * 5, cu(np.zeros((4, 5, 3))))
    with pytest.raises(hb.TdsHipError, match="error 1: inverse kinematics: damped LM needs lambda != 0"):
        sim.inverse_kinematics(cu(q0), links, cu(tgt), method="damped_lm", lam=0.0)
    with pytest.raises(hb.TdsHipError, match="error 1: inverse kinematics: negative max_iterations"):
        sim.inverse_kinematics(cu(q0), links, cu(tgt), max_iterations=-2)
    # malformed tensors are refused in Python, before the library is called: N = 2, K = 2
    import torch

    q, t, l2 = cu(q0[:2]), cu(np.zeros((2, 2, 3))), [0, 1]
    for bad in (q[:, :-1], q.float(), q.cpu(), q[0]):
        with pytest.raises(AssertionError, match="q_init"):
            sim.inverse_kinematics(bad, l2, t)
    for bad in (t[:, :1], t[:1], t[..., :2], t.float(), t.cpu()):
        with pytest.raises(AssertionError, match="targets"):
            sim.inverse_kinematics(q, l2, bad)
    for bad in (q[:1], q[:, :-1], q.float(), q.cpu()):
        with pytest.raises(AssertionError, match="q_reference"):
            sim.inverse_kinematics(q, l2, t, q_reference=bad)
    with pytest.raises(ValueError, match=r"body_points must be \[2, 3\]"):
        sim.inverse_kinematics(q, l2, t, body_points=np.zeros((1, 3)))
    with pytest.raises(AssertionError, match="out must hold q"):
        sim.inverse_kinematics(q, l2, t, out={"status": torch.zeros(2, dtype=torch.int32, device="cuda")})
    for key, bad in (("q", torch.zeros_like(q)[:, :-1]), ("q", torch.zeros_like(q).float()), ("q", torch.zeros_like(q).cpu()),
                     ("q", torch.zeros_like(q).t().contiguous().t()), ("status", torch.zeros(2, dtype=torch.int64, device="cuda")),
                     ("residual", torch.zeros(3, dtype=torch.float64, device="cuda"))):
        with pytest.raises(AssertionError, match=key):
            sim.inverse_kinematics(q, l2, t, out={"q": torch.zeros_like(q), key: bad})
