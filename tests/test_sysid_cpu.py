"""Batched system identification without a GPU (csrc/tds_lm.hip's host statement, sysid.py over the host checkers):
lm_step_host against a numpy restatement of its rules, the box QP's properties, a linear model against lstsq, the
gradient against reverse mode, the isolation of a problem that fails, the argument errors, and the driver on Models.

Bounds are 10 x the maximum measured over the cases below (largest |a - b| / max(|b|, 1), printed by each test):
  lm_step_host vs numpy (np.linalg, compact free sub-matrices), all of LM_SHAPES: cost, g, H 9.96e-15 (p = 16,
    260 entries a sum: numpy's sums are pairwise, the statement's sequential); delta, pred 7.81e-16
  infinite bounds, delta vs np.linalg.solve: 1.67e-16
  delta vs the best of all 3^p active sets (p <= 5): 1.11e-16
  one step at lambda = 1e-12 on a linear model vs np.linalg.lstsq: 1.78e-12 (the damping itself: lambda D against H)
  g vs trajectory_vjp_host's gtheta: pendulum5 6.94e-18, ant 6.66e-16
  driver, case (a) pendulum5: costs 3.2e-3 -> 4.0e-5 -> 6.2e-9 -> 8.1e-18, theta* relative error 3.68e-08 after three
    accepted steps (bound: 10 x that, below the 1e-6 the case allows); case (b) ant through contacts, after four
    accepted steps: T = 6 2.85e-15, T = 8 2.07e-15 (bound 10 x the larger)
KKT conditions are asserted to 1e-8 |A|: the QP's own stop rule is |g_free|_2 < 1e-8 (tds_hip.h, rule 4)."""
import functools
import itertools
import os

import numpy as np
import pytest
import torch

import tds_amd
from tds_amd import hip_backend as hb

from conftest import ROOT
from test_param_derivs_gpu import SYSID_SEL, SYSID_T, sysid_setup

SUMS_BOUND = 10 * 9.96e-15
STEP_BOUND = 10 * 7.81e-16
SOLVE_BOUND = 10 * 1.67e-16
ACTIVE_SET_BOUND = 10 * 1.11e-16
LSTSQ_BOUND = 10 * 1.78e-12
VJP_BOUND = {"pendulum5": 10 * 6.94e-18, "ant": 10 * 6.66e-16}
CASE_A_BOUND = 10 * 3.68e-08
CASE_B_BOUND = 10 * 2.85e-15
KKT_TOL = 1e-8

# (n, rows per problem, m, p, L)
LM_SHAPES = [(1, (1,), 1, 1, 1), (3, (2, 0, 3), 63, 2, 3), (2, (1, 2), 64, 5, 2), (4, (3, 1, 0, 2), 65, 4, 5),
             (2, (2, 2), 130, 16, 8), (3, (1, 1, 1), 37, 3, 1)]


def err(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1.0))) if a.size else 0.0


def lm_case(seed, n, counts, m, p, L, bounds="box"):
    """a call's arguments by name (read only): residuals of order one, weights in [0.5, 1.5] with zeros over NaN
    observations, lambdas from 1e-6 to 10, and bounds that cut some steps ("box"), none ("inf") or no arrays (None)"""
    rng = np.random.default_rng(seed)
    rows = int(sum(counts))
    row_start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    s, s_obs = rng.normal(size=(rows, m)), rng.normal(size=(rows, m))
    js = rng.normal(size=(rows, p, m))
    w = rng.uniform(0.5, 1.5, (rows, m))
    skip = rng.uniform(size=(rows, m)) < 0.2
    w[skip], s_obs[skip] = 0.0, np.nan
    js[skip.nonzero()[0], :, skip.nonzero()[1]] = 1e300  # (not counted either)
    lam = np.tile(np.logspace(-6, 1, L)[None], (n, 1)) if L > 1 else np.full((n, 1), 1e-2)
    dlo = dhi = None
    if bounds == "box":
        scale = 0.3 / np.sqrt(max(rows // n, 1) * m)
        dlo, dhi = -rng.uniform(0.0, 1.0, (n, p)) * scale, rng.uniform(0.0, 1.0, (n, p)) * scale
        dlo[:, ::3], dhi[:, 1::4] = -np.inf, np.inf
    elif bounds == "inf":
        dlo, dhi = np.full((n, p), -np.inf), np.full((n, p), np.inf)
    return dict(row_start=row_start, s=s, s_obs=s_obs, js=js, lam=lam, w=w, dlo=dlo, dhi=dhi)


def np_box_qp(A, g, lo, hi):
    """tds_hip.h's rules 1-7 over compact free sub-matrices: (x, clamped bits, iterations, status)"""
    p = g.shape[0]
    x = np.clip(np.zeros(p), lo, hi)
    cl, factored, it = np.zeros(p, dtype=bool), None, 1
    for it in range(1, 101):
        grad = g + A @ x
        cl = ((x == lo) & (grad > 0)) | ((x == hi) & (grad < 0))
        f = ~cl
        if cl.all():
            break
        if factored is None or (cl != factored).any():
            try:
                np.linalg.cholesky(A[np.ix_(f, f)])
            except np.linalg.LinAlgError:
                return np.zeros(p), 0, 0, 1
            factored = cl
        if np.sqrt((grad[f] ** 2).sum()) < 1e-8:
            break
        y = x.copy()
        y[f] = -np.linalg.solve(A[np.ix_(f, f)], g[f] + A[np.ix_(f, cl)] @ x[cl])
        sd = (y - x) @ grad
        if not sd < 0:
            break
        value = lambda v: v @ (0.5 * (A @ v) + g)  # noqa: E731
        fx, step, taken = value(x), 1.0, False
        while True:
            c = np.clip(y if step == 1.0 else x + step * (y - x), lo, hi)
            if (value(c) - fx) / (step * sd) >= 0.1:
                taken = True
                break
            step *= 0.6
            if step < 1e-22:
                break
        if not taken:
            break
        x = c
    return x, int(sum(1 << a for a in range(p) if cl[a])), min(it, 100), 0


def np_lm_step(row_start, s, s_obs, js, lam, w, dlo, dhi):
    n, (rows, p, m), L = len(row_start) - 1, js.shape, lam.shape[1]
    out = {"cost": np.zeros(n), "g": np.zeros((n, p)), "H": np.zeros((n, p, p)), "delta": np.zeros((n, L, p)),
           "pred": np.zeros((n, L)), "clamped": np.zeros((n, L), dtype=np.int32),
           "qp_iterations": np.zeros((n, L), dtype=np.int32), "status": np.zeros((n, L), dtype=np.int32)}
    for i in range(n):
        sl = slice(row_start[i], row_start[i + 1])
        keep = w[sl] != 0
        a = np.where(keep, w[sl] * np.where(keep, s[sl] - s_obs[sl], 0.0), 0.0).reshape(-1)
        c = np.where(keep[:, None, :], w[sl][:, None, :] * js[sl], 0.0).transpose(1, 0, 2).reshape(p, -1)
        H, g = c @ c.T, c @ a
        out["cost"][i], out["g"][i], out["H"][i] = 0.5 * a @ a, g, H
        D = np.clip(np.diag(H), 1e-6, 1e32)
        lo = np.full(p, -np.inf) if dlo is None else dlo[i]
        hi = np.full(p, np.inf) if dhi is None else dhi[i]
        for l in range(L):
            x, bits, its, status = np_box_qp(H + lam[i, l] * np.diag(D), g, lo, hi)
            out["delta"][i, l], out["clamped"][i, l], out["qp_iterations"][i, l], out["status"][i, l] = x, bits, its, status
            out["pred"][i, l] = -(g @ x + 0.5 * x @ H @ x)
    return out


@functools.lru_cache(maxsize=None)
def lm_pair(shape, bounds="box"):
    case = lm_case(1000 + 7 * LM_SHAPES.index(shape), *shape, bounds=bounds)
    return case, hb.lm_step_host(**case)


@pytest.mark.parametrize("shape", LM_SHAPES)
def test_lm_step_host_matches_the_numpy_statement(shape, built):
    case, got = lm_pair(shape)
    want = np_lm_step(**case)
    e_sums = max(err(got[k], want[k]) for k in ("cost", "g", "H"))
    e_step = max(err(got[k], want[k]) for k in ("delta", "pred"))
    print(f"lm_step_host vs numpy {shape}: sums {e_sums:.3e}, step {e_step:.3e}")
    for k in ("clamped", "qp_iterations", "status"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    assert not got["status"].any() and np.isfinite(got["delta"]).all()
    np.testing.assert_array_equal(got["H"], got["H"].transpose(0, 2, 1))
    for i, c in enumerate(np.diff(case["row_start"])):
        if c == 0:  # an empty problem
            assert got["cost"][i] == 0 and not got["H"][i].any() and not got["g"][i].any() and not got["delta"][i].any()
    assert e_sums <= SUMS_BOUND and e_step <= STEP_BOUND
    # pred is the model's exact decrease at the step returned
    g, H, d = got["g"], got["H"], got["delta"]
    dec = -(np.einsum("np,nlp->nl", g, d) + 0.5 * np.einsum("nlp,npq,nlq->nl", d, H, d))
    assert err(got["pred"], dec) <= STEP_BOUND
    # the cost-only mode prices the same residuals
    only = hb.lm_step_host(case["row_start"], case["s"], case["s_obs"], None, None, case["w"])
    assert list(only) == ["cost"]
    np.testing.assert_array_equal(only["cost"], got["cost"])


@pytest.mark.parametrize("shape", LM_SHAPES)
def test_infinite_bounds_give_the_damped_gauss_newton_step(shape, built):
    case, got = lm_pair(shape, "inf")
    none = hb.lm_step_host(**{**case, "dlo": None, "dhi": None})
    for k in hb.LM_OUTPUTS:
        np.testing.assert_array_equal(got[k], none[k], err_msg=k)
    worst = 0.0
    for i in range(shape[0]):
        D = np.clip(np.diag(got["H"][i]), 1e-6, 1e32)
        for l in range(shape[4]):
            x = -np.linalg.solve(got["H"][i] + case["lam"][i, l] * np.diag(D), got["g"][i])
            if np.linalg.norm(got["g"][i]) < 1e-8:
                x = np.zeros_like(x)  # (rule 4: the empty problem)
            worst = max(worst, err(got["delta"][i, l], x))
    print(f"lm_step_host, infinite bounds vs np.linalg.solve {shape}: {worst:.3e}")
    assert not got["clamped"].any() and worst <= SOLVE_BOUND


def kkt_violation(A, g, x, lo, hi):
    grad = g + A @ x
    at_lo, at_hi = x == lo, x == hi
    free = ~at_lo & ~at_hi
    v = np.abs(grad[free]).max(initial=0.0)
    v = max(v, (-grad[at_lo & ~at_hi]).max(initial=0.0), grad[at_hi & ~at_lo].max(initial=0.0))
    return v / max(np.abs(A).max(), 1.0)


@pytest.mark.parametrize("shape", LM_SHAPES)
def test_box_qp_properties(shape, built):
    case, got = lm_pair(shape)
    n, _, _, p, L = shape
    worst_kkt = worst_set = 0.0
    for i in range(n):
        H, g, lo, hi = got["H"][i], got["g"][i], case["dlo"][i], case["dhi"][i]
        D = np.clip(np.diag(H), 1e-6, 1e32)
        for l in range(L):
            A, x = H + case["lam"][i, l] * np.diag(D), got["delta"][i, l]
            assert (x >= lo).all() and (x <= hi).all()
            worst_kkt = max(worst_kkt, kkt_violation(A, g, x, lo, hi))
            bits = got["clamped"][i, l]
            for a in range(p):
                if bits >> a & 1:
                    assert x[a] in (lo[a], hi[a])
            if p <= 5:  # the minimiser over all 3^p active sets
                best, best_f = None, np.inf
                for kind in itertools.product((0, 1, 2), repeat=p):
                    kind = np.array(kind)
                    if ((kind == 1) & np.isinf(lo)).any() or ((kind == 2) & np.isinf(hi)).any():
                        continue
                    y = np.where(kind == 1, lo, np.where(kind == 2, hi, 0.0))
                    f = kind == 0
                    if f.any():
                        y[f] = -np.linalg.solve(A[np.ix_(f, f)], g[f] + A[np.ix_(f, ~f)] @ y[~f])
                    if (y < lo).any() or (y > hi).any():
                        continue
                    fy = y @ (0.5 * A @ y + g)
                    if fy < best_f:
                        best, best_f = y, fy
                worst_set = max(worst_set, err(x, best))
    print(f"lm_step_host box QP {shape}: KKT {worst_kkt:.3e}, vs the best active set {worst_set:.3e}")
    assert got["clamped"].any() or shape[2] == 1
    assert worst_kkt <= KKT_TOL and worst_set <= ACTIVE_SET_BOUND


def test_a_pinned_parameter_keeps_its_value(built):
    case = dict(lm_case(5, 2, (2, 1), 40, 4, 3))
    case["dlo"], case["dhi"] = case["dlo"].copy(), case["dhi"].copy()
    case["dlo"][:, 2] = case["dhi"][:, 2] = 0.0
    got = hb.lm_step_host(**case)
    assert not got["status"].any() and not got["delta"][:, :, 2].any() and got["delta"].any()
    free = np_lm_step(**case)
    assert err(got["delta"], free["delta"]) <= STEP_BOUND


def test_one_step_on_a_linear_model_is_the_least_squares_solution(built):
    rng = np.random.default_rng(21)
    rows, m, p = 3, 50, 6
    J = rng.normal(size=(rows, p, m))
    theta0, b, s_obs = rng.normal(size=p), rng.normal(size=(rows, m)), rng.normal(size=(rows, m))
    s = np.einsum("rpm,p->rm", J, theta0) + b
    got = hb.lm_step_host([0, rows], s, s_obs, J, np.array([[1e-12]]))
    A = J.transpose(0, 2, 1).reshape(rows * m, p)
    want = np.linalg.lstsq(A, (s_obs - b).reshape(-1), rcond=None)[0]
    e = err(theta0 + got["delta"][0, 0], want)
    print(f"one LM step at lambda = 1e-12 vs lstsq: {e:.3e}")
    assert got["status"][0, 0] == 0 and e <= LSTSQ_BOUND


def golden_x(name, idx):
    return np.ascontiguousarray(np.load(os.path.join(ROOT, "tests", "golden", f"{name}.npz"))["x"][list(idx)])


ANT_SEL = [("friction",), ("mass", 5), ("gravity", 2)]


@pytest.mark.parametrize("name", ["pendulum5", "ant"])
def test_gradient_matches_reverse_mode(name, built):
    """g against gtheta of trajectory_vjp_host with gs = w^2 (s - s_obs): reverse mode shares no code with lm_step"""
    m = tds_amd.load_model(name)
    sel = SYSID_SEL if name == "pendulum5" else ANT_SEL
    rng = np.random.default_rng(8)
    rows, T, p = 4, 6, len(sel)
    x0 = golden_x(name, rng.integers(0, 48, rows))
    theta = hb.params_get(m, sel) * rng.uniform(0.9, 1.1, p)
    V = hb.trajectory_directions(m.input_dim, (), p).numpy()[None].repeat(rows, axis=0)
    s, js = hb.trajectory_jvp_host(m, x0, V, T, 1, None, sel, theta)
    s_obs = s + 0.01 * rng.normal(size=s.shape)
    w = rng.uniform(0.5, 1.5, s.shape)
    got = hb.lm_step_host([0, 1, rows], s, s_obs, js, np.ones((2, 1)), w)
    _, _, _, gth = hb.trajectory_vjp_host(m, x0, w * w * (s - s_obs), T, 1, None, sel, theta)
    want = np.stack([gth[:1].sum(axis=0), gth[1:].sum(axis=0)])
    e = err(got["g"], want)
    print(f"lm_step_host g vs trajectory_vjp_host {name}: {e:.3e}")
    assert np.abs(want).max() > 1e-3 and e <= VJP_BOUND[name]


def alone(case, i):
    """problem i of a call as a call of its own"""
    r0, r1 = case["row_start"][i], case["row_start"][i + 1]
    cut = lambda a, sl: None if a is None else a[sl]  # noqa: E731
    return dict(row_start=np.array([0, r1 - r0], dtype=np.int32), lam=case["lam"][i:i + 1],
                dlo=cut(case["dlo"], slice(i, i + 1)), dhi=cut(case["dhi"], slice(i, i + 1)),
                **{k: case[k][r0:r1] for k in ("s", "s_obs", "js", "w")})


@pytest.mark.parametrize("status", [1, 2])
def test_a_failing_problem_leaves_the_others_untouched(status, built):
    case = {k: None if v is None else v.copy() for k, v in lm_case(77, 4, (2, 1, 2, 1), 70, 3, 3).items()}
    bad = 1
    r0 = case["row_start"][bad]
    if status == 2:
        case["s"][r0, 5] = np.nan  # one counted entry
        case["w"][r0, 5] = 1.0
    else:  # two equal directions (one entry, 2) and a lambda that rounds away: the second pivot is 4 - (4 / 2)^2 = 0
        case["js"][r0, :, :], case["w"][r0, :] = 0.0, 0.0
        case["js"][r0, :2, 0], case["js"][r0, 2, 2], case["w"][r0, :3], case["s_obs"][r0, :3] = 2.0, 1.0, 1.0, 0.25
        case["lam"][bad, 0] = 1e-17
        case["dlo"][bad], case["dhi"][bad] = -np.inf, np.inf
    got = hb.lm_step_host(**case)
    if status == 2:
        assert (got["status"][bad] == 2).all() and got["cost"][bad] == np.inf
        for k in ("g", "H", "delta", "pred", "clamped", "qp_iterations"):
            assert not got[k][bad].any(), k
    else:
        assert got["status"][bad].tolist() == [1, 0, 0] and np.isfinite(got["cost"][bad])
        assert not got["delta"][bad, 0].any() and got["pred"][bad, 0] == 0 and got["delta"][bad, 1:].any()
    for i in range(4):
        if i != bad:
            one = hb.lm_step_host(**alone(case, i))
            assert not one["status"].any()
            for k in hb.LM_OUTPUTS:
                np.testing.assert_array_equal(got[k][i], one[k][0], err_msg=k)


def test_every_argument_error_is_named(built):
    case = lm_case(3, 2, (1, 2), 9, 3, 2)
    call = lambda **kw: hb.lm_step_host(**{**case, **kw})  # noqa: E731
    with pytest.raises(hb.TdsHipError, match="error 1: tds_hip_lm_step_host: row_start does not run from 0 to rows"):
        call(row_start=[1, 2, 3])
    with pytest.raises(hb.TdsHipError, match="error 1: tds_hip_lm_step_host: row_start does not run from 0 to rows"):
        call(row_start=[0, 1, 2])
    with pytest.raises(hb.TdsHipError, match="error 1: tds_hip_lm_step_host: row_start decreases"):
        call(row_start=[0, 4, 3])
    hi = case["dhi"].copy()
    hi[1, 1] = case["dlo"][1, 1] - 1.0
    with pytest.raises(hb.TdsHipError, match="error 1: tds_hip_lm_step_host: dlo > dhi or a NaN bound"):
        call(dhi=hi)
    hi[1, 1] = np.nan
    with pytest.raises(hb.TdsHipError, match="error 1: tds_hip_lm_step_host: dlo > dhi or a NaN bound"):
        call(dhi=hi)
    for bad in (0.0, -1.0, np.inf, np.nan):
        lam = case["lam"].copy()
        lam[1, 0] = bad
        with pytest.raises(hb.TdsHipError, match="error 1: tds_hip_lm_step_host: a lambda that is not positive and finite"):
            call(lam=lam)
    with pytest.raises(ValueError, match="dlo and dhi are given together or not at all"):
        call(dhi=None)
    with pytest.raises(hb.TdsHipError, match="error 2: tds_hip_lm_step_host: p exceeds the bound of 16 parameters"):
        hb.lm_step_host([0, 1], np.zeros((1, 4)), np.zeros((1, 4)), np.ones((1, 17, 4)), np.ones((1, 1)))
    with pytest.raises(hb.TdsHipError, match="error 2: tds_hip_lm_step_host: n_lambda exceeds the bound of 8 candidates"):
        hb.lm_step_host([0, 1], np.zeros((1, 4)), np.zeros((1, 4)), np.ones((1, 2, 4)), np.ones((1, 9)))
    with pytest.raises(hb.TdsHipError, match="error 1: tds_hip_lm_step_host: m must be at least 1"):
        hb.lm_step_host([0, 1], np.zeros((1, 0)), np.zeros((1, 0)), np.ones((1, 2, 0)), np.ones((1, 1)))
    with pytest.raises(ValueError, match=r"js: expected \[3, p, m\]"):
        call(js=case["js"][:2])
    with pytest.raises(ValueError, match=r"s_obs: expected \[3, 9\]"):
        call(s_obs=case["s_obs"][:, :8])
    with pytest.raises(ValueError, match=r"lam: expected \[2, 2\]"):
        call(lam=case["lam"][:1])
    with pytest.raises(ValueError, match=r"row_start: expected \[n \+ 1\] with n >= 1"):
        call(row_start=[0])


# ---------------------------------------------------------------------------------------------- the driver on Models
@functools.lru_cache(maxsize=None)
def case_a():
    """pendulum5, nine parameters, 8 rows of T = 60 as ONE problem, only q weighted (read only):
    (m, base, true, x0, u, s_obs, weights)"""
    m, base, true, s0, taus = sysid_setup()
    x0 = np.concatenate([s0, taus[0]], axis=1)
    u = np.ascontiguousarray(taus[1:].transpose(1, 0, 2))
    s_obs, _ = hb.trajectory_jvp_host(m, x0, None, SYSID_T, 1, u, SYSID_SEL, true)
    weights = np.concatenate([np.ones(m.dof_q), np.zeros(m.dof_qd)])
    return m, base, true, x0, u, s_obs, weights


@functools.lru_cache(maxsize=None)
def case_b(T):
    """ant through contacts: (m, base, true, lo, hi, x0, s_obs)"""
    m = tds_amd.load_model("ant")
    g = np.load(os.path.join(ROOT, "tests", "golden", "ant.npz"))["x"]
    x0 = np.ascontiguousarray(g[np.random.default_rng(3).integers(0, g.shape[0], 4)])
    base = hb.params_get(m, ANT_SEL)
    true = base * np.array([0.8, 1.3, 1.05])
    lo, hi = np.minimum(0.5 * base, 1.5 * base), np.maximum(0.5 * base, 1.5 * base)
    s_obs, _ = hb.trajectory_jvp_host(m, x0, None, T, 1, None, ANT_SEL, true)
    return m, base, true, lo, hi, x0, s_obs


@functools.lru_cache(maxsize=None)
def run_a(**kw):
    m, base, true, x0, u, s_obs, weights = case_a()
    return tds_amd.sysid(m, x0, s_obs, SYSID_SEL, base, SYSID_T, u=u, weights=weights, **kw)


def check_run(res, eta=1e-3):
    """what holds of every run, exactly: the cost never rises; each pick is the rule's, recomputed from the traces;
    a problem takes no step once it is frozen (after iterations_used iterations, where reason is not 0)"""
    cost, pick = res["cost_trace"].numpy(), res["pick_trace"].numpy()
    rho, pred, cc, st = (res[k].numpy() for k in ("rho_trace", "pred_trace", "cand_cost_trace", "status_trace"))
    used, reason = res["iterations_used"].numpy(), res["reason"].numpy()
    assert (cost[1:] <= cost[:-1]).all()
    its, N = pick.shape
    for it in range(its):
        with np.errstate(invalid="ignore", divide="ignore"):
            np.testing.assert_array_equal(rho[it], (cost[it][:, None] - cc[it]) / pred[it])
            ok = (st[it] == 0) & (pred[it] > 0) & np.isfinite(cc[it]) & (rho[it] >= eta)
        for i in range(N):
            if pick[it, i] >= 0:
                assert it < used[i] and ok[i, pick[it, i]]
                assert cc[it, i, pick[it, i]] == np.where(ok[i], cc[it, i], np.inf).min() == cost[it + 1, i]
            else:
                assert cost[it + 1, i] == cost[it, i]
                # (not taken: nothing qualified, or the problem was frozen, or froze here on reason 2)
                assert not ok[i].any() or it >= used[i] or (reason[i] == 2 and it == used[i] - 1)
    th = res["theta_trace"].numpy()
    np.testing.assert_array_equal(th[-1], res["theta"].numpy())
    for i in range(N):
        assert used[i] == its if reason[i] == 0 else (pick[used[i]:, i] == -1).all()
        assert (th[used[i]:, i] == th[used[i], i]).all()
        for it in range(its):
            assert (th[it + 1, i] != th[it, i]).any() == (pick[it, i] >= 0)


def test_sysid_recovers_the_pendulums_parameters(built):
    m, base, true, *_ = case_a()
    res = run_a(iterations=6)
    e = float(np.max(np.abs(res["theta"][0].numpy() - true) / np.abs(true)))
    print(f"sysid case (a): costs {res['cost_trace'][:, 0].tolist()}, picks {res['pick_trace'][:, 0].tolist()}, "
          f"reason {res['reason'].tolist()}, theta* relative error {e:.3e}")
    check_run(res)
    assert res["cost_trace"][0, 0] > 1e-3 and res["cost"][0] < 1e-15
    assert int(res["best"]) == 0 and tuple(res["s"].shape) == (8, SYSID_T, 2 * m.dof_q)
    assert e <= CASE_A_BOUND <= 1e-6


@pytest.mark.parametrize("T", [6, 8])
def test_sysid_recovers_the_ants_parameters_through_contacts(T, built):
    """the tolerances are off: gravity's 9.81 dominates |theta|, so the default ptol freezes T = 6 (reason 2) with the
    friction still 9e-8 off, which is that rule's meaning and not this test's subject"""
    m, base, true, lo, hi, x0, s_obs = case_b(T)
    res = tds_amd.sysid(m, x0, s_obs, ANT_SEL, base, T, bounds=(lo, hi), iterations=8, ftol=0.0, ptol=0.0)
    e = float(np.max(np.abs(res["theta"][0].numpy() - true) / np.abs(true)))
    print(f"sysid case (b) T={T}: costs {res['cost_trace'][:, 0].tolist()}, theta* relative error {e:.3e}")
    check_run(res)
    assert e <= CASE_B_BOUND


def test_sysid_in_a_tight_box_ends_on_its_bounds(built):
    m, base, true, x0, u, s_obs, weights = case_a()
    lo, hi = 0.9 * base, 1.1 * base
    res = tds_amd.sysid(m, x0, s_obs, SYSID_SEL, base, SYSID_T, u=u, weights=weights, bounds=(lo, hi), iterations=12)
    check_run(res)
    theta, g = res["theta"][0].numpy(), res["g"][0].numpy()
    at_lo, at_hi = theta == lo, theta == hi
    print(f"sysid in [0.9, 1.1] model: costs {res['cost_trace'][[0, -1], 0].tolist()}, at a bound "
          f"{int((at_lo | at_hi).sum())} of 9, reason {res['reason'].tolist()}")
    assert res["cost"][0] < res["cost_trace"][0, 0] and (theta >= lo).all() and (theta <= hi).all()
    assert (at_lo | at_hi).any() and not (at_lo | at_hi).all()
    # the gradient of the last linearisation pushes outwards where theta sits on a bound ...
    final = tds_amd.sysid(m, x0, s_obs, SYSID_SEL, theta, SYSID_T, u=u, weights=weights, bounds=(lo, hi), iterations=1)
    g = final["g"][0].numpy()
    assert (g[at_lo] > 0).all() and (g[at_hi] < 0).all()
    # ... and the QP's clamped set there is those parameters
    bits = int(final["clamped"][0])
    assert [bool(bits >> a & 1) for a in range(9)] == (at_lo | at_hi).tolist()


def test_zero_tolerances_never_freeze(built):
    res = run_a(iterations=8, ftol=0.0, ptol=0.0)
    check_run(res)
    assert res["reason"].tolist() in ([0], [3]) and res["reason"].tolist() != [1] and res["reason"].tolist() != [2]
    frozen = run_a(iterations=8)
    assert frozen["reason"].tolist() in ([1], [2]) and int(frozen["iterations_used"][0]) < 8
    check_run(frozen)


def test_data_that_are_not_finite_do_not_read_as_convergence(built):
    """a problem at status 2 (here: an infinite weight) has delta = 0 everywhere; that is not reason 2"""
    m, base, true, x0, u, s_obs, weights = case_a()
    bad = weights.copy()
    bad[0] = np.inf
    res = tds_amd.sysid(m, x0, s_obs, SYSID_SEL, base, SYSID_T, u=u, weights=bad, iterations=3)
    check_run(res)
    assert bool((res["status_trace"] == 2).all()) and res["cost"][0] == np.inf
    assert res["reason"].tolist() == [0] and res["pick_trace"].tolist() == [[-1]] * 3
    assert torch.equal(res["theta"][0], torch.from_numpy(base))
    assert bool((res["lambda_trace"][1:, 0] > res["lambda_trace"][:-1, 0]).all())


def test_multi_start_takes_the_best_of_its_starts(built):
    m, base, true, x0, u, s_obs, weights = case_a()
    lo, hi = 0.5 * base, 1.5 * base
    starts = tds_amd.sysid_starts(base, lo, hi, 6, seed=5)
    assert tuple(starts.shape) == (6, 9) and torch.equal(starts[0], torch.from_numpy(base))
    assert bool((starts >= torch.from_numpy(lo)).all()) and bool((starts <= torch.from_numpy(hi)).all())
    assert torch.equal(starts, tds_amd.sysid_starts(base, lo, hi, 6, seed=5))
    with pytest.raises(ValueError, match="finite bounds"):
        tds_amd.sysid_starts(base, lo, np.inf, 6)
    rep = lambda a: np.tile(a, (6,) + (1,) * (a.ndim - 1))  # noqa: E731
    kw = dict(u=rep(u), weights=weights, bounds=(lo, hi), iterations=5)
    many = tds_amd.sysid(m, rep(x0), rep(s_obs), SYSID_SEL, starts, SYSID_T, **kw)
    one = tds_amd.sysid(m, x0, s_obs, SYSID_SEL, starts[:1], SYSID_T, **{**kw, "u": u})
    check_run(many)
    for k in ("theta", "cost", "reason", "iterations_used", "H", "g", "clamped", "cost_trace", "lambda_trace",
              "pick_trace", "rho_trace", "pred_trace"):
        first = (lambda t: t[:, 0]) if k.endswith("_trace") else (lambda t: t[0])  # noqa: E731
        np.testing.assert_array_equal(first(many[k]).numpy(), first(one[k]).numpy(), err_msg=k)  # (NaN equals NaN)
    assert torch.equal(many["s"][:8], one["s"])
    assert int(many["best"]) == int(many["cost"].argmin()) and float(many["cost"].min()) == float(many["cost"][many["best"]])
    print(f"multi-start: final costs {many['cost'].tolist()}, best {int(many['best'])}")


def test_sysid_refuses_what_does_not_fit(built):
    m, base, true, x0, u, s_obs, weights = case_a()
    with pytest.raises(ValueError, match="sysid: theta0"):
        tds_amd.sysid(m, x0, s_obs, SYSID_SEL, base[:8], SYSID_T, u=u)
    with pytest.raises(ValueError, match="sysid: expected x0"):
        tds_amd.sysid(m, x0, s_obs[:, :50], SYSID_SEL, base, SYSID_T, u=u)
    with pytest.raises(ValueError, match="sysid: the problems' rows"):
        tds_amd.sysid(m, x0, s_obs, SYSID_SEL, base, SYSID_T, u=u, row_start=[0, 7])
    with pytest.raises(ValueError, match="sysid: weights do not broadcast"):
        tds_amd.sysid(m, x0, s_obs, SYSID_SEL, base, SYSID_T, u=u, weights=np.ones(3))
    with pytest.raises(ValueError, match="sysid: bounds: lo > hi"):
        tds_amd.sysid(m, x0, s_obs, SYSID_SEL, base, SYSID_T, u=u, bounds=(base, 0.5 * base))
    zero = tds_amd.sysid(m, x0, s_obs, SYSID_SEL, base, SYSID_T, u=u, weights=weights, iterations=0)
    assert tuple(zero["cost_trace"].shape) == (1, 1) and zero["cost"][0] == run_a(iterations=6)["cost_trace"][0, 0]
