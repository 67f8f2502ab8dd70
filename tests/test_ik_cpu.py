"""Batched inverse kinematics on the CPU (tds_hip_inverse_kinematics_host: the host instantiation of csrc/tds_ik.h):
against the reference's TinyInverseKinematics::compute (the fixture tests/golden/ik_reference.npz, written by
tools/ik_golden.py), against the same iteration composed in NumPy from the existing host queries, and properties that
need no reference.

Bounds on q and the residual (largest |a - b| / max(|b|, 1), 10 x the maximum measured on the CPU; each test prints its
figure before it asserts):
  against the fixture (61 cases)      transpose 3.8e-16 -> 3.8e-15,  pinv 2.32e-12 -> 2.32e-11,  damped LM 4.95e-15 -> 4.95e-14
  against the NumPy recomputation     transpose 1.67e-16 -> 1.67e-15,  pinv 1.08e-12 -> 1.08e-11,  damped LM 1.65e-14 -> 1.65e-13
The pinv maxima are the cases with the worst-conditioned Jacobians (fixture: four targets on the Ant, cond(J) 3e3;
NumPy: four on Laikago, 2e2), where Eigen's complete orthogonal decomposition, LAPACK's SVD and the pivoted Cholesky of
J J^T here each carry eps cond(J)^2; everywhere else the three agree to 1e-14.
"""
import os

import numpy as np
import pytest

from conftest import ROOT

import tds_amd
from tds_amd import hip_backend as hb

from test_jacobian_cpu import REFUSED, SUPPORTED

METHODS = {"transpose": hb.IK_TRANSPOSE, "pinv": hb.IK_PINV, "damped_lm": hb.IK_DAMPED_LM}
NAMES = {v: k for k, v in METHODS.items()}
FIXTURE_BOUND = {"transpose": 10 * 3.8e-16, "pinv": 10 * 2.32e-12, "damped_lm": 10 * 4.95e-15}
NUMPY_BOUND = {"transpose": 10 * 1.67e-16, "pinv": 10 * 1.08e-12, "damped_lm": 10 * 1.65e-14}
OPTS = ("max_iterations", "lambda_", "target_tolerance", "step_tolerance", "alpha", "weight_reference")
DEFAULTS = dict(max_iterations=20, lambda_=0.02, target_tolerance=1e-3, step_tolerance=1e-8, alpha=5.0,
                weight_reference=0.2)


def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1.0))) if a.size else 0.0


def fixture():
    return np.load(os.path.join(ROOT, "tests", "golden", "ik_reference.npz"))


def fixture_case(g, i):
    """case i of the fixture: model, the arguments of inverse_kinematics_host, the reference's answers"""
    m = tds_amd.load_model(str(g["model"][i]))
    k, nq = int(g["k"][i]), m.dof_q
    o = dict(zip(OPTS, g["options"][i]))
    o["max_iterations"] = int(o["max_iterations"])
    args = dict(q_init=g["q_init"][i, :nq][None], links=g["links"][i, :k], targets=g["targets"][i, :k][None],
                body_points=g["body_points"][i, :k], q_reference=g["q_ref"][i, :nq][None] if g["have_ref"][i] else None,
                method=int(g["method"][i]), **o)
    ref = dict(q=g["q"][i, :nq], iterations=int(g["iterations"][i]), status=int(g["status"][i]),
               residual=float(g["residual"][i]))
    return m, args, ref


def world_points(m, q, links, pts):
    """[N, K, 3]: the body points pts [K, 3] of links [K] at q [N, dof_q], from the host kinematics"""
    xw = hb.dynamics_host(m, q, want=("x_world",))["x_world"][:, np.asarray(links)]
    return np.einsum("nkij,kj->nki", xw[..., :9].reshape(xw.shape[0], -1, 3, 3), np.asarray(pts)) + xw[..., 9:]


def numpy_ik(m, q_init, links, targets, body_points, q_reference, method, o):
    """one environment's iteration from dynamics_host, point_jacobian_host and numpy.linalg; also whether every
    iteration kept its branch margins and, for pinv, its rank gap (the rules of tools/ik_golden.cpp) and took a step of
    at most one radian"""
    q = np.array(q_init, dtype=float)
    qo, vo = (7, 6) if m.is_floating else (0, 0)
    res, clean = -1.0, True
    for it in range(o["max_iterations"]):
        pos = world_points(m, q[None], links, body_points)[0]
        J = np.concatenate([hb.point_jacobian_host(m, q[None], int(l), p[None], local=True)[0]
                            for l, p in zip(links, body_points)])
        J[:, :vo] = 0.0
        e = (targets - pos).reshape(-1)
        res = float(np.sqrt(np.sum(e * e)))
        clean &= abs(res - o["target_tolerance"]) > 1e-6 * o["target_tolerance"]
        if res < o["target_tolerance"]:
            return q, it, hb.IK_REACHED, res, clean
        if method == hb.IK_TRANSPOSE:
            d = J.T @ e
        elif method == hb.IK_PINV:
            sv = np.linalg.svd(J, compute_uv=False)
            clean &= not np.any((sv <= 1e-6 * sv[0]) & (sv >= 1e-12 * sv[0]))
            d = np.linalg.pinv(J, rcond=1e-9) @ e
        else:
            d = J.T @ np.linalg.solve(J @ J.T + o["lambda_"] ** 2 * np.eye(J.shape[0]), e)
        d = d[vo:]
        # a step of more than one radian (or metre) is no local correction any more: the iteration map then amplifies
        # round-off by itself (the reference and NumPy part by 1e-7 in 20 such iterations), and the case measures nothing
        clean &= float(np.max(np.abs(o["alpha"] * d), initial=0.0)) <= 1.0
        q[qo:] += o["alpha"] * d
        if q_reference is not None:
            q[qo:] += o["weight_reference"] * (q_reference[qo:] - q[qo:])
        sq = float(np.sum(d * d))
        clean &= abs(sq - o["step_tolerance"] ** 2) > 1e-6 * o["step_tolerance"] ** 2
        if sq < o["step_tolerance"] ** 2:
            return q, it, hb.IK_CONVERGED, res, clean
    return q, o["max_iterations"], hb.IK_FAILED, res, clean


def random_case(name, method, seed, k=None, with_ref=None):
    """a seeded case of one environment: q_init from the model's golden records, targets = the points' positions at a
    perturbed configuration"""
    m = tds_amd.load_model(name)
    rng = np.random.default_rng(seed)
    g = np.load(os.path.join(ROOT, "tests", "golden", f"{name}.npz"))["x"]
    q0 = g[rng.integers(0, g.shape[0]), :m.dof_q].copy()
    qo = 7 if m.is_floating else 0
    if m.is_floating:
        if seed % 2:
            q0[:4] = rng.normal(size=4)
        q0[:4] /= np.linalg.norm(q0[:4])
    k = int(rng.integers(1, 5)) if k is None else k
    links = rng.integers(0, m.num_links, k).astype(np.int32)
    pts = rng.normal(0, 0.05, (k, 3)) * (seed % 3 > 0)
    q1 = q0.copy()
    q1[qo:] += rng.normal(0, 0.15, m.dof_q - qo)
    tgt = world_points(m, q1[None], links, pts)[0]
    o = dict(DEFAULTS, alpha=0.3 if method == hb.IK_TRANSPOSE else 0.5)
    qref = None
    if (seed % 2 == 0) if with_ref is None else with_ref:
        qref = q0 + np.concatenate([np.zeros(qo), rng.normal(0, 0.05, m.dof_q - qo)])
        o["weight_reference"] = 0.1
    return m, dict(q_init=q0, links=links, targets=tgt, body_points=pts, q_reference=qref, method=method, o=o)


def host(m, c, **over):
    o = dict(c["o"], **over)
    qr = None if c["q_reference"] is None else c["q_reference"][None]
    return hb.inverse_kinematics_host(m, c["q_init"][None], c["links"], c["targets"][None], c["body_points"], qr,
                                      method=c["method"], **o)


MOVING = [n for n in SUPPORTED if tds_amd.load_model(n).num_links > 0 and
          tds_amd.load_model(n).dof_qd > (6 if tds_amd.load_model(n).is_floating else 0)]


# ---------------------------------------------------------------- against the reference's answers
def test_host_matches_the_reference_fixture(built):
    g = fixture()
    n = int(g["kept"])
    assert n == len(g["model"]) >= 36
    worst = {k: 0.0 for k in METHODS}
    seen = set()
    for i in range(n):
        m, args, ref = fixture_case(g, i)
        r = hb.inverse_kinematics_host(m, **args)
        name = NAMES[args["method"]]
        assert int(r["iterations"][0]) == ref["iterations"], (i, str(g["model"][i]), name)
        assert int(r["status"][0]) == ref["status"], (i, str(g["model"][i]), name)
        worst[name] = max(worst[name], rel(r["q"][0], ref["q"]), rel(r["residual"][0], ref["residual"]))
        seen.add(ref["status"])
    print("host vs fixture, max rel per method:", worst)
    assert seen == {hb.IK_FAILED, hb.IK_CONVERGED, hb.IK_REACHED}
    for k in METHODS:
        assert worst[k] <= FIXTURE_BOUND[k], (k, worst[k])


# ---------------------------------------------------------------- against the same iteration in NumPy
@pytest.mark.parametrize("name", MOVING)
def test_host_matches_numpy_recomputation(name, built):
    worst = {k: 0.0 for k in METHODS}
    for method in METHODS.values():
        done, seed = 0, 0
        while done < 4:
            seed += 1
            assert seed < 60
            m, c = random_case(name, method, 100 * method + seed)
            q, it, st, res, clean = numpy_ik(m, c["q_init"], c["links"], c["targets"], c["body_points"],
                                             c["q_reference"], method, c["o"])
            if not clean or not np.all(np.isfinite(q)):
                continue
            done += 1
            r = host(m, c)
            assert (int(r["iterations"][0]), int(r["status"][0])) == (it, st), (name, method, seed)
            worst[NAMES[method]] = max(worst[NAMES[method]], rel(r["q"][0], q), rel(r["residual"][0], res))
    print(name, "host vs numpy, max rel per method:", worst)
    for k in METHODS:
        assert worst[k] <= NUMPY_BOUND[k], (name, k, worst[k])


# ---------------------------------------------------------------- properties
@pytest.mark.parametrize("name", ["pendulum5", "ant", "laikago_floating", "ant_floating"])
def test_reached_means_within_tolerance_and_the_base_stays(name, built):
    reached = 0
    for seed in range(12):
        m, c = random_case(name, hb.IK_PINV, seed)
        r = host(m, c, max_iterations=40)
        if m.is_floating:
            np.testing.assert_array_equal(r["q"][0, :7], c["q_init"][:7])
        if r["status"][0] == hb.IK_REACHED:
            reached += 1
            pos = world_points(m, r["q"], c["links"], c["body_points"])[0]
            dist = np.sqrt(np.sum((pos - c["targets"]) ** 2))
            assert dist < c["o"]["target_tolerance"]
            assert abs(dist - r["residual"][0]) < 1e-12
    assert reached >= 4


@pytest.mark.parametrize("method", METHODS.values())
def test_no_iterations_and_targets_already_met(method, built):
    m, c = random_case("ant", method, 5, k=2)
    r = host(m, c, max_iterations=0)
    np.testing.assert_array_equal(r["q"][0], c["q_init"])
    assert (r["iterations"][0], r["status"][0], r["residual"][0]) == (0, hb.IK_FAILED, -1.0)
    c["targets"] = world_points(m, c["q_init"][None], c["links"], c["body_points"])[0]
    r = host(m, c)
    np.testing.assert_array_equal(r["q"][0], c["q_init"])
    assert (r["iterations"][0], r["status"][0]) == (0, hb.IK_REACHED) and 0 <= r["residual"][0] < 1e-12


@pytest.mark.parametrize("name", ["pendulum5", "laikago_floating"])
def test_a_target_given_twice(name, built):
    """K = 2 with the same link, point and target twice: J has two equal blocks of rows; the Moore-Penrose step halves
    the doubled error's share, so the K = 1 iterates come back"""
    m, c = random_case(name, hb.IK_PINV, 3, k=1, with_ref=False)
    one = host(m, c, max_iterations=3)
    c2 = dict(c, links=np.repeat(c["links"], 2), targets=np.repeat(c["targets"], 2, axis=0),
              body_points=np.repeat(c["body_points"], 2, axis=0))
    two = host(m, c2, max_iterations=3)
    print(name, "twice vs once:", rel(two["q"], one["q"]))
    assert rel(two["q"], one["q"]) <= 1e-10
    assert abs(two["residual"][0] - np.sqrt(2) * one["residual"][0]) <= 1e-10
    lm = host(m, dict(c2, method=hb.IK_DAMPED_LM), max_iterations=3)
    assert np.all(np.isfinite(lm["q"])) and np.isfinite(lm["residual"][0])


@pytest.mark.parametrize("method", METHODS.values())
def test_a_batch_row_equals_its_own_call(method, built):
    name = "laikago_floating"
    cases = [random_case(name, method, s, k=2, with_ref=True)[1] for s in range(9)]
    m = tds_amd.load_model(name)
    stack = lambda key: np.stack([c[key] for c in cases])  # noqa: E731
    c0 = cases[0]
    big = hb.inverse_kinematics_host(m, stack("q_init"), c0["links"], stack("targets"), c0["body_points"],
                                     stack("q_reference"), method=method, **c0["o"])
    for i, c in enumerate(cases):
        r = host(m, dict(c, links=c0["links"], body_points=c0["body_points"]))
        for key in ("q", "iterations", "status", "residual"):
            np.testing.assert_array_equal(big[key][i], r[key][0])


def test_a_non_finite_environment_fails_alone(built):
    m, c = random_case("ant", hb.IK_PINV, 2, k=2, with_ref=False)
    q = np.stack([c["q_init"], c["q_init"], c["q_init"]])
    q[1] = np.nan
    r = hb.inverse_kinematics_host(m, q, c["links"], c["targets"], c["body_points"], method=hb.IK_PINV, **c["o"])
    assert r["status"][1] == hb.IK_FAILED and r["iterations"][1] == c["o"]["max_iterations"]
    for key in ("q", "iterations", "status", "residual"):
        np.testing.assert_array_equal(r[key][0], r[key][2])
    assert np.all(np.isfinite(r["q"][0]))


# ---------------------------------------------------------------- refusals
@pytest.mark.parametrize("name", REFUSED)
def test_models_out_of_scope_are_refused(name, built):
    m = tds_amd.load_model(name)
    with pytest.raises(hb.TdsHipError, match="error 2: step Jacobians: .* not supported"):
        hb.inverse_kinematics_host(m, np.zeros((1, m.dof_q)), [0], np.zeros((1, 1, 3)))


def test_invalid_arguments(built):
    import ctypes as C

    m, c = random_case("ant", hb.IK_PINV, 1, k=1)
    q, t = c["q_init"][None], np.zeros((1, 1, 3))
    for k in (0, 5):
        with pytest.raises(hb.TdsHipError, match="error 1: inverse kinematics: 1 to 4 targets"):
            hb.inverse_kinematics_host(m, q, np.zeros(k, dtype=np.int32), np.zeros((1, k, 3)))
    for link in (-1, m.num_links):
        with pytest.raises(hb.TdsHipError, match="error 1: inverse kinematics: link index out of range"):
            hb.inverse_kinematics_host(m, q, [link], t)
    with pytest.raises(hb.TdsHipError, match="error 1: inverse kinematics: negative max_iterations"):
        hb.inverse_kinematics_host(m, q, [0], t, max_iterations=-1)
    with pytest.raises(hb.TdsHipError, match="error 1: inverse kinematics: unknown method"):
        hb.inverse_kinematics_host(m, q, [0], t, method=3)
    with pytest.raises(hb.TdsHipError, match="error 1: inverse kinematics: damped LM needs lambda != 0"):
        hb.inverse_kinematics_host(m, q, [0], t, method="damped_lm", lam=0.0)
    with pytest.raises(ValueError, match="unknown inverse-kinematics method"):
        hb.inverse_kinematics_host(m, q, [0], t, method="newton")
    with pytest.raises(ValueError, match="unknown inverse-kinematics option"):
        hb.inverse_kinematics_host(m, q, [0], t, beta=1.0)
    # malformed arrays are refused in Python, before the library is called: N = 2, K = 2
    q2, t2 = np.repeat(q, 2, axis=0), np.zeros((2, 2, 3))
    with pytest.raises(ValueError, match=r"body_points must be \[2, 3\]"):
        hb.inverse_kinematics_host(m, q2, [0, 1], t2, body_points=np.zeros((1, 3)))
    with pytest.raises(ValueError, match="cannot reshape"):
        hb.inverse_kinematics_host(m, q2, [0, 1], np.zeros((2, 2, 2)))
    with pytest.raises(ValueError, match="broadcast"):
        hb.inverse_kinematics_host(m, q2, [0, 1], np.zeros((3, 2, 3)))
    with pytest.raises(ValueError, match="cannot reshape"):
        hb.inverse_kinematics_host(m, q2[:, :-1], [0, 1], t2)
    with pytest.raises(ValueError, match="broadcast"):
        hb.inverse_kinematics_host(m, q2, [0, 1], t2, q_reference=np.zeros((3, m.dof_q)))
    with pytest.raises(ValueError, match="cannot reshape"):
        hb.inverse_kinematics_host(m, q2, [0, 1], t2, q_reference=np.zeros((2, m.dof_q - 1)))
    L = hb.lib()
    links = (C.c_int32 * 1)(0)
    out = np.zeros((1, m.dof_q))
    call = lambda n, qp, tp, op: L.tds_hip_inverse_kinematics_host(  # noqa: E731
        C.byref(m), n, qp, 1, links, None, tp, None, None, op, None, None, None)
    assert call(0, q.ctypes.data, t.ctypes.data, out.ctypes.data) == 1  # n < 1
    assert call(1, None, t.ctypes.data, out.ctypes.data) == 1
    assert call(1, q.ctypes.data, None, out.ctypes.data) == 1
    assert call(1, q.ctypes.data, t.ctypes.data, None) == 1
    assert call(1, q.ctypes.data, t.ctypes.data, out.ctypes.data) == 0  # NULL options, points and the three outputs


def test_defaults_are_the_references(built):
    o = hb.ik_options()
    assert o.method == hb.IK_PINV
    assert {k: getattr(o, k) for k in OPTS} == DEFAULTS
    assert (hb.IK_TRANSPOSE, hb.IK_PINV, hb.IK_DAMPED_LM) == (0, 1, 2)
    assert (hb.IK_FAILED, hb.IK_CONVERGED, hb.IK_REACHED) == (0, 1, 2)
