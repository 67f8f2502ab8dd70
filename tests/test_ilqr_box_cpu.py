"""CPU: control-limited iLQR's host statements — lqr_backward_box_host with infinite bounds against the plain pass
(bit for bit), against a numpy restatement with compact free sub-matrices, its QP against brute force over the active
sets and against the KKT conditions, the structure of the feedback gains, the clamped feedback_rollout_host against a
python loop with np.clip, the ilqr driver with u_limits over the host checkers, argument errors and refusals.

Bounds that are not exact are 10 x the maximum measured on this file's seeded inputs (printed by each test before it
asserts), largest |a - b| / max(|b|, 1):
  lqr_backward_box_host vs the numpy restatement over the 45 shapes: 3.553e-15 (k, K, dv); the clamped sets are
    equal; of the 540 (problem, step) pairs 273 have free and clamped controls, 50 all clamped, 217 none; at most 10
    QP iterations
  k of one step vs the minimiser over all 3^nu active sets, nu = 1, 2, 3, 5, 50 problems each: 6.661e-16
  cartpole ilqr with |u| <= 1, six iterations: projected |grad_U J|_inf after / before = 1.201e-8 (bound: 1e-6, about
    seventy-fold room for another summation order); with |u| <= 0.5: 1.379e-8
The clamped rollout equals the python loop exactly, as the unclamped one does in test_ilqr_cpu.py."""
import functools
import os

import numpy as np
import pytest
import torch

from conftest import ROOT

import tds_amd
from tds_amd import hip_backend as hb

from test_ilqr_cpu import FB_MODELS, err, fb_case, golden_x, grad_u, lq_problem, quadratic_cost
from test_param_derivs_cpu import REFUSED

BOX_VS_NUMPY = 3.553e-14
QP_VS_BRUTE_FORCE = 6.661e-15
PROJECTED_GRAD_RATIO = 1e-6  # (fixed in advance, not 10 x the measured)
SHAPES = [(nx, nu, T) for nx in (1, 2, 5, 37, 40) for nu in (1, 3, 16) for T in (1, 2, 9)]


def shape_problem(nx, nu, T):
    """the plain test's problem of this shape, and dlo = -U(0, 1), dhi = U(0, 1) seeded by the shape"""
    seed = 1000 * nx + 10 * nu + T
    P = lq_problem(seed, 3, T, nx, nu)
    rng = np.random.default_rng(seed + 500000)
    return P, -rng.uniform(0.0, 1.0, (3, T, nu)), rng.uniform(0.0, 1.0, (3, T, nu))


# ---- the numpy restatement -----------------------------------------------------------------------------------------
def box_qp_numpy(H, q, lo, hi, x0):
    """projected Newton with compact free sub-matrices; (x, clamped mask, iterations, the factorised free mask or
    None where the loop stopped with nothing free)"""
    f = lambda v: 0.5 * v @ H @ v + q @ v  # noqa: E731
    x = np.clip(x0, lo, hi)
    prev, Hff = None, None
    for it in range(1, 101):
        g = q + H @ x
        cl = ((x == lo) & (g > 0)) | ((x == hi) & (g < 0))
        fr = ~cl
        if not fr.any():
            return x, cl, it, None
        if prev is None or (cl != prev).any():
            Hff = H[np.ix_(fr, fr)]
            np.linalg.cholesky(Hff)  # (raises where it is not positive definite: no such step in this file's use)
            prev = cl
        if np.linalg.norm(g[fr]) < 1e-8:
            break
        y = x.copy()
        y[fr] = -np.linalg.solve(Hff, q[fr] + H[np.ix_(fr, cl)] @ x[cl])
        s = y - x
        sd = s @ g
        if sd >= 0:
            break
        step, fx, taken = 1.0, f(x), False
        while True:
            c = np.clip(y if step == 1.0 else x + step * s, lo, hi)
            if (f(c) - fx) / (step * sd) >= 0.1:
                taken = True
                break
            step *= 0.6
            if step < 1e-22:
                break
        if not taken:
            break
        x = c
    return x, cl, it, ~prev


def lqr_box_numpy(A, B, lx, lu, lxx, luu, lux, mu, dlo, dhi):
    """the control-limited recursion with numpy products; also Q_u and Q_uu of every step (for the KKT conditions)"""
    n, T, nx, nu = B.shape
    k, K, dv = np.zeros((n, T, nu)), np.zeros((n, T, nu, nx)), np.zeros((n, 2))
    clamped, its = np.zeros((n, T), dtype=np.int32), np.zeros((n, T), dtype=np.int32)
    Qus, Quus = np.zeros((n, T, nu)), np.zeros((n, T, nu, nu))
    for p in range(n):
        Vx, Vxx = lx[p, T], lxx[p, T]
        start = np.zeros(nu)
        for t in range(T - 1, -1, -1):
            a, b = A[p, t], B[p, t]
            Qx, Qu = lx[p, t] + a.T @ Vx, lu[p, t] + b.T @ Vx
            Qxx, Qux, Quu = lxx[p, t] + a.T @ Vxx @ a, lux[p, t] + b.T @ Vxx @ a, luu[p, t] + b.T @ Vxx @ b
            H = Quu + mu[p] * np.eye(nu)
            kk, cl, it, free = box_qp_numpy(H, Qu, dlo[p, t], dhi[p, t], start)
            KK = np.zeros((nu, nx))
            if free is not None:
                KK[free] = -np.linalg.solve(H[np.ix_(free, free)], Qux[free])
            Vx = Qx + KK.T @ Quu @ kk + KK.T @ Qu + Qux.T @ kk
            Vxx = Qxx + KK.T @ Quu @ KK + KK.T @ Qux + Qux.T @ KK
            Vxx = 0.5 * (Vxx + Vxx.T)
            dv[p, 0] += kk @ Qu
            dv[p, 1] += 0.5 * kk @ Quu @ kk
            k[p, t], K[p, t], start = kk, KK, kk
            clamped[p, t], its[p, t] = int(sum(1 << i for i in np.flatnonzero(cl))), it
            Qus[p, t], Quus[p, t] = Qu, Quu
    return k, K, dv, clamped, its, Qus, Quus


@functools.lru_cache(maxsize=None)
def shape_results(nx, nu, T):
    """(problem, dlo, dhi, the library's six outputs, the restatement's); computed once, read only"""
    P, dlo, dhi = shape_problem(nx, nu, T)
    got = hb.lqr_backward_box_host(*P, dlo, dhi)
    want = lqr_box_numpy(*P, dlo, dhi)
    for a in (*P, dlo, dhi, *got, *want):
        a.setflags(write=False)
    return P, dlo, dhi, got, want


def bits(clamped, nu):
    """[.., nu] bool from the int32 masks"""
    return (clamped[..., None] >> np.arange(nu)) & 1 == 1


# ---- 1. infinite bounds ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx,nu,T", SHAPES)
def test_infinite_bounds_reproduce_the_plain_pass_exactly(nx, nu, T, built):
    P = lq_problem(1000 * nx + 10 * nu + T, 3, T, nx, nu)
    inf = np.full((3, T, nu), np.inf)
    k, K, dv, status, clamped, its = hb.lqr_backward_box_host(*P, -inf, inf)
    for got, want in zip((k, K, dv, status), hb.lqr_backward_host(*P)):
        np.testing.assert_array_equal(got, want)
    assert (status == 0).all() and (clamped == 0).all() and (its == 2).all()


# ---- 2. against the numpy restatement ------------------------------------------------------------------------------
@pytest.mark.parametrize("nx,nu,T", SHAPES)
def test_lqr_backward_box_host_against_numpy(nx, nu, T, built):
    P, dlo, dhi, (k, K, dv, status, clamped, its), (rk, rK, rdv, rcl, rits, _, _) = shape_results(nx, nu, T)
    e = max(err(k, rk), err(K, rK), err(dv, rdv))
    print(f"lqr_backward_box_host vs numpy nx={nx} nu={nu} T={T}: {e:.3e}, QP iterations <= {its.max()}")
    assert (status == 0).all()
    np.testing.assert_array_equal(clamped, rcl)
    assert (k >= dlo).all() and (k <= dhi).all()
    assert e <= BOX_VS_NUMPY


def test_the_restatement_test_is_not_vacuous(built):
    mixed = none = every = pairs = top = 0
    for nx, nu, T in SHAPES:
        _, _, _, (_, _, _, _, clamped, its), _ = shape_results(nx, nu, T)
        count = bits(clamped, nu).sum(axis=-1)
        pairs += count.size
        mixed += int(((count > 0) & (count < nu)).sum())
        none += int((count == 0).sum())
        every += int((count == nu).sum())
        top = max(top, int(its.max()))
    print(f"{pairs} (problem, step) pairs: {mixed} mixed, {every} all clamped, {none} none clamped; QP iterations <= {top}")
    assert pairs == 540 and 4 * mixed >= pairs and none > 0 and every > 0 and top < 100


# ---- 3. the QP against brute force and the KKT conditions --------------------------------------------------------
@pytest.mark.parametrize("nu", [1, 2, 3, 5])
def test_the_qp_against_all_active_sets(nu, built):
    """T = 1: k minimises k^T H k / 2 + q^T k in the box, H = luu + B^T lxx_T B + mu I, q = lu + B^T lx_T.  Brute
    force: every control free, at its lower or at its upper bound (3^nu sets); the free ones solve their linear
    system; the feasible point of least value is the minimiser (the problem is convex)."""
    n, nx = 50, 4
    A, B, lx, lu, lxx, luu, lux, mu = lq_problem(900 + nu, n, 1, nx, nu)
    rng = np.random.default_rng(nu)
    dlo, dhi = -rng.uniform(0.0, 1.0, (n, 1, nu)), rng.uniform(0.0, 1.0, (n, 1, nu))
    k, K, dv, status, clamped, its = hb.lqr_backward_box_host(A, B, lx, lu, lxx, luu, lux, mu, dlo, dhi)
    assert (status == 0).all()
    worst, sets = 0.0, set()
    for p in range(n):
        b = B[p, 0]
        H, q = luu[p, 0] + b.T @ lxx[p, 1] @ b + mu[p] * np.eye(nu), lu[p, 0] + b.T @ lx[p, 1]
        best, best_f = None, np.inf
        for code in range(3 ** nu):
            kind = (code // 3 ** np.arange(nu)) % 3  # 0 free, 1 lower, 2 upper
            fr = kind == 0
            x = np.where(kind == 1, dlo[p, 0], dhi[p, 0])
            if fr.any():
                x[fr] = -np.linalg.solve(H[np.ix_(fr, fr)], q[fr] + H[np.ix_(fr, ~fr)] @ x[~fr])
            if (x >= dlo[p, 0]).all() and (x <= dhi[p, 0]).all():
                f = 0.5 * x @ H @ x + q @ x
                if f < best_f:
                    best, best_f = x, f
        worst = max(worst, err(k[p, 0], best))
        sets.add(int(clamped[p, 0]))
    print(f"QP vs brute force, nu={nu}: {worst:.3e} over {n} problems, {len(sets)} different clamped sets")
    assert len(sets) >= min(3, 2 ** nu - 1)
    assert worst <= QP_VS_BRUTE_FORCE


@pytest.mark.parametrize("nx,nu,T", SHAPES)
def test_k_satisfies_the_kkt_conditions(nx, nu, T, built):
    """g = Q_u + (Q_uu + mu I) k with Q_u, Q_uu recomputed in numpy: zero on the free controls (to the statement's own
    stop), pointing into the box on the clamped ones"""
    P, dlo, dhi, (k, _, _, _, clamped, _), (_, _, _, _, _, Qu, Quu) = shape_results(nx, nu, T)
    H = Quu + P[7][:, None, None, None] * np.eye(nu)
    g = Qu + (H @ k[..., None])[..., 0]
    cl = bits(clamped, nu)
    assert (np.abs(g[~cl]) < 1e-8).all()
    assert ((k == dlo) | (k == dhi))[cl].all()
    assert (g[cl & (k == dlo)] >= 0).all() and (g[cl & (k == dhi)] <= 0).all()


# ---- 4. feedback structure -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx,nu,T", SHAPES)
def test_rows_of_K_at_clamped_controls_are_exactly_zero(nx, nu, T, built):
    _, _, _, (_, K, _, _, clamped, _), _ = shape_results(nx, nu, T)
    cl = bits(clamped, nu)
    assert not K[cl].any()
    assert (np.abs(K[~cl]).max(axis=-1) > 0).all()


def test_a_pinned_control_takes_its_value_and_no_feedback(built):
    n, T, nx, nu, pin = 3, 4, 5, 3, 1
    P = lq_problem(6, n, T, nx, nu)
    rng = np.random.default_rng(6)
    dlo, dhi = -rng.uniform(0.0, 1.0, (n, T, nu)), rng.uniform(0.0, 1.0, (n, T, nu))
    dlo[..., pin] = dhi[..., pin] = rng.uniform(-0.5, 0.5, (n, T))
    k, K, dv, status, clamped, its = hb.lqr_backward_box_host(*P, dlo, dhi)
    assert (status == 0).all()
    np.testing.assert_array_equal(k[..., pin], dlo[..., pin])
    assert not K[:, :, pin].any() and bits(clamped, nu)[..., pin].all()
    assert K[:, :, [0, 2]].any()


@pytest.mark.parametrize("t_bad", [0, 2, 3])
def test_a_problem_that_is_not_positive_definite_is_reported_and_left_nominal(t_bad, built):
    n, T, nx, nu, bad = 4, 4, 5, 3, 2
    A, B, lx, lu, lxx, luu, lux, mu = lq_problem(5, n, T, nx, nu, mu=(0.0,))
    luu[bad, t_bad] = np.diag([1.0, -200.0, 1.0])
    rng = np.random.default_rng(55)
    dlo, dhi = -rng.uniform(0.0, 1.0, (n, T, nu)), rng.uniform(0.0, 1.0, (n, T, nu))
    dlo[bad, t_bad], dhi[bad, t_bad] = -np.inf, np.inf  # (the indefinite control stays free: the pivot is met)
    out = hb.lqr_backward_box_host(A, B, lx, lu, lxx, luu, lux, mu, dlo, dhi)
    assert out[3].tolist() == [0, 0, t_bad + 1, 0]
    assert not any(a[bad].any() for a in out[:3]) and not out[4][bad].any() and not out[5][bad].any()
    for p in (0, 1, 3):
        alone = hb.lqr_backward_box_host(*(a[p:p + 1] for a in (A, B, lx, lu, lxx, luu, lux, mu, dlo, dhi)))
        for got, one in zip(out, alone):
            np.testing.assert_array_equal(got[p], one[0])
        assert out[0][p].any() and out[1][p].any() and out[4][p].any()


# ---- 5. the clamped rollout ----------------------------------------------------------------------------------------
def chained_clipped(m, x0, s_nom, u_nom, k, K, alpha, por, lo, hi):
    """a python loop of step_host with the feedback law and np.clip; the law's sum runs in index order"""
    nsd, n_act, _ = hb.trajectory_dims(m, 1)
    rows, T = x0.shape[0], u_nom.shape[1]
    s, u = np.zeros((rows, T + 1, nsd)), np.zeros((rows, T, n_act))
    x = x0.copy()
    s[:, 0] = x0[:, :nsd]
    for t in range(T):
        d = np.zeros((rows, n_act))
        for j in range(nsd):
            d += K[por, t, :, j] * (s[:, t, j] - s_nom[por, t, j])[:, None]
        u[:, t] = np.clip((u_nom[por, t] + alpha[:, None] * k[por, t]) + d, lo[por, t], hi[por, t])
        x[:, :nsd], x[:, nsd:nsd + n_act] = s[:, t], u[:, t]
        s[:, t + 1] = hb.step_host(m, x)[:, :nsd]
    return s, u


def fb_bounds(u_nom, seed=3):
    rng = np.random.default_rng(seed)
    return -rng.uniform(0.05, 0.3, u_nom.shape), rng.uniform(0.05, 0.3, u_nom.shape)


@pytest.mark.parametrize("name", FB_MODELS)
def test_clamped_feedback_rollout_host_is_the_python_loop_with_clip(name, built):
    m, x0, s_nom, u_nom, k, K, alpha = fb_case(name)
    lo, hi = fb_bounds(u_nom)
    s, u = hb.feedback_rollout_host(m, x0, s_nom, u_nom, k, K, alpha, u_lo=lo, u_hi=hi)
    rs, ru = chained_clipped(m, x0, s_nom, u_nom, k, K, alpha, np.arange(3), lo, hi)
    np.testing.assert_array_equal(u, ru)
    np.testing.assert_array_equal(s, rs)
    assert (u >= lo).all() and (u <= hi).all()
    at = (u == lo) | (u == hi)
    assert at.any() and not at.all()
    s_free, u_free = hb.feedback_rollout_host(m, x0, s_nom, u_nom, k, K, alpha)
    assert np.abs(u - u_free).max() > 1e-3 and np.abs(s - s_free).max() > 0


@pytest.mark.parametrize("name", FB_MODELS)
def test_infinite_limits_are_the_rollout_without_limits(name, built):
    m, x0, s_nom, u_nom, k, K, alpha = fb_case(name)
    inf = np.full(u_nom.shape, np.inf)
    for got, want in zip(hb.feedback_rollout_host(m, x0, s_nom, u_nom, k, K, alpha, u_lo=-inf, u_hi=inf),
                         hb.feedback_rollout_host(m, x0, s_nom, u_nom, k, K, alpha)):
        np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("name", FB_MODELS)
def test_problem_of_row_indexes_the_limits(name, built):
    m, x0, s_nom, u_nom, k, K, alpha = fb_case(name, rows=3, P=2)
    lo, hi = fb_bounds(u_nom)
    por = np.array([1, 0, 1])
    s, u = hb.feedback_rollout_host(m, x0, s_nom, u_nom, k, K, alpha, problem_of_row=por, u_lo=lo, u_hi=hi)
    rs, ru = hb.feedback_rollout_host(m, x0, s_nom[por], u_nom[por], k[por], K[por], alpha, u_lo=lo[por], u_hi=hi[por])
    np.testing.assert_array_equal(s, rs)
    np.testing.assert_array_equal(u, ru)
    assert (u >= lo[por]).all() and (u <= hi[por]).all() and ((u == lo[por]) | (u == hi[por])).any()


# ---- 6. the driver on the cartpole ---------------------------------------------------------------------------------
def armijo_holds_box(m, cost, x0, s, u, mu, alpha, J_new, lo, hi, armijo=1e-4):
    """one iteration's model recomputed from the host pieces; the accepted steps' inequality"""
    N, T = u.shape[:2]
    nsd, n_act, _ = hb.trajectory_dims(m, 1)
    jac = hb.jacobian_host(m, hb.trajectory_records(m, x0, s, u), rows=range(nsd), cols=range(nsd + n_act))
    jac = jac.reshape(N, T, nsd, nsd + n_act)
    J, lx, lu, lxx, luu, lux = [t.numpy() for t in cost.expand(torch.from_numpy(s), torch.from_numpy(u))]
    k, K, dv, status, _, _ = hb.lqr_backward_box_host(
        np.ascontiguousarray(jac[..., :nsd]), np.ascontiguousarray(jac[..., nsd:]), lx, lu, lxx, luu, lux, mu,
        lo - u, hi - u)
    sa, ua = hb.feedback_rollout_host(m, x0, s, u, k, K, alpha, u_lo=lo, u_hi=hi)
    Ja = cost.value(torch.from_numpy(sa), torch.from_numpy(ua)).numpy()
    took = alpha > 0
    np.testing.assert_array_equal(Ja[took], J_new[took])
    assert (status[took] == 0).all()
    assert ((J - Ja)[took] >= (armijo * -(alpha * dv[:, 0] + alpha ** 2 * dv[:, 1]))[took]).all()
    return sa, ua, took


def cartpole_case():
    m = tds_amd.load_model("cartpole")
    nsd, n_act, _ = hb.trajectory_dims(m, 1)
    N, T = 3, 40
    x0 = golden_x("cartpole", [0, 5, 9])
    u0 = np.random.default_rng(41).uniform(-2.0, 2.0, (N, T, n_act))
    return m, x0, u0, quadratic_cost(m)


@pytest.mark.parametrize("limit", [1.0, 0.5])
def test_ilqr_with_limits_on_the_cartpole(limit, built):
    """|u| <= 1 cuts the unconstrained solution (max |u| 2.4, 4.25, 1.11) in all three problems; 0.5 is tighter"""
    m, x0, u0, cost = cartpole_case()
    nsd, n_act, _ = hb.trajectory_dims(m, 1)
    N, T, iters = 3, 40, 6
    r = tds_amd.ilqr(m, x0, u0, cost, iterations=iters, u_limits=(-limit, limit))
    c, al, u = r["cost"].numpy(), r["alpha"].numpy(), r["u"].numpy()
    assert c.shape == (iters + 1, N) and tuple(r["clamped"].shape) == (N, T) and tuple(r["qp_iterations"].shape) == (N, T)
    assert (np.abs(u) <= limit).all()
    assert (c[1:] <= c[:-1]).all() and (c[-1] < c[0]).all()
    at = np.abs(u) == limit
    print(f"cartpole |u| <= {limit}: cost {c[0]} -> {c[-1]}, controls at a bound {at.sum(axis=(1, 2)).tolist()} of {T * n_act}")
    assert at.any(axis=(1, 2)).all() and (~at).any(axis=(1, 2)).all()
    # every accepted step satisfies the Armijo inequality, recomputed from the pieces along the driver's own path
    lo, hi = np.full((N, T, n_act), -limit), np.full((N, T, n_act), limit)
    z = np.zeros
    s0, uc0 = hb.feedback_rollout_host(m, x0, z((N, T + 1, nsd)), u0, z((N, T, n_act)), z((N, T, n_act, nsd)), 0.0,
                                       u_lo=lo, u_hi=hi)
    np.testing.assert_array_equal(uc0, np.clip(u0, lo, hi))
    s, uu = s0, uc0
    for i in range(iters):
        sa, ua, took = armijo_holds_box(m, cost, x0, s, uu, r["mu_trace"][i].numpy(), al[i], c[i + 1], lo, hi)
        s, uu = np.where(took[:, None, None], sa, s), np.where(took[:, None, None], ua, uu)
    np.testing.assert_array_equal(s, r["s"].numpy())
    np.testing.assert_array_equal(uu, u)

    def projected(s_, u_):
        """|grad_U J|_inf with the entries zeroed where u is at a bound and the gradient points outward"""
        _, lx, lu, *_ = [t.numpy() for t in cost.expand(torch.from_numpy(s_), torch.from_numpy(u_))]
        g = grad_u(m, x0, s_, u_, lx, lu)
        g[((u_ == lo) & (g > 0)) | ((u_ == hi) & (g < 0))] = 0.0
        return np.abs(g).max(axis=(1, 2))

    ratio = float((projected(s, uu) / projected(s0, uc0)).max())
    print(f"cartpole |u| <= {limit}: projected |grad_U J|_inf ratio {ratio:.3e}")
    assert ratio < PROJECTED_GRAD_RATIO


def test_no_limits_is_the_call_without_the_keyword(built):
    m, x0, u0, cost = cartpole_case()
    a = tds_amd.ilqr(m, x0, u0, cost, iterations=2)
    b = tds_amd.ilqr(m, x0, u0, cost, iterations=2, u_limits=None)
    assert a.keys() == b.keys() and "clamped" not in a
    for key in a:
        assert torch.equal(a[key], b[key]), key


def test_limits_beyond_reach_change_nothing_but_the_two_new_entries(built):
    m, x0, u0, cost = cartpole_case()
    a = tds_amd.ilqr(m, x0, u0, cost, iterations=2)
    b = tds_amd.ilqr(m, x0, u0, cost, iterations=2, u_limits=(-np.inf, np.inf))
    for key in a:
        assert torch.equal(a[key], b[key]), key
    assert not b["clamped"].any() and bool((b["qp_iterations"] == 2).all())


# ---- 7. "model" limits, argument errors, refusals ------------------------------------------------------------------
def contact_case(name, N=2, T=8):
    """records of the golden file that stand on the ground, actions beyond the model's action_limit"""
    m = tds_amd.load_model(name)
    nsd, n_act, _ = hb.trajectory_dims(m, 1)
    g = np.load(os.path.join(ROOT, "tests", "golden", f"{name}.npz"))
    down = np.flatnonzero(g["active_contacts"] > 0)[:N]
    assert down.size == N
    x0 = np.ascontiguousarray(g["x"][down])
    u0 = np.random.default_rng(42).uniform(-0.5, 0.5, (N, T, n_act))
    assert (np.abs(u0) > m.action_limit).any()
    return m, x0, u0


def test_model_limits_on_a_locomotion_model_through_contacts(built):
    """the Ant clamps its actions to +-action_limit inside the step: "model" takes that limit"""
    m, x0, u0 = contact_case("ant")
    assert m.step_mode == tds_amd.model.TDS_STEP_LOCOMOTION
    r = tds_amd.ilqr(m, x0, u0, quadratic_cost(m), iterations=3, mu0=0.01, u_limits="model")
    c, u = r["cost"].numpy(), r["u"].numpy()
    print(f"ant, model limits {m.action_limit}: cost {c[0]} -> {c[-1]}, alphas {r['alpha'].numpy().tolist()}")
    assert (np.abs(u) <= m.action_limit).all()
    assert (c[1:] <= c[:-1]).all() and (c[-1] < c[0]).all()
    same = tds_amd.ilqr(m, x0, u0, quadratic_cost(m), iterations=3, mu0=0.01, u_limits=(-m.action_limit, m.action_limit))
    for key in r:
        assert torch.equal(r[key], same[key]), key


def test_limits_through_contacts_on_pendulum5_plane(built):
    """the inputs of test_ilqr_through_contacts_and_rejected_steps with the honest cost and |u| <= 0.4.  The model
    steps on torques (TDS_STEP_TAU: nothing clamps them inside the step), so "model" is refused for it, as for the
    cartpole, and the limit is given in numbers."""
    m, x0, u0 = contact_case("pendulum5_plane")
    cost = quadratic_cost(m)
    with pytest.raises(ValueError, match="locomotion model"):
        tds_amd.ilqr(m, x0, u0, cost, iterations=1, u_limits="model")
    r = tds_amd.ilqr(m, x0, u0, cost, iterations=5, mu0=0.01, u_limits=(-0.4, 0.4))
    c, u = r["cost"].numpy(), r["u"].numpy()
    print(f"pendulum5_plane, |u| <= 0.4: cost {c[0]} -> {c[-1]}, alphas {r['alpha'].numpy().tolist()}")
    assert (np.abs(u) <= 0.4).all()
    assert (c[1:] <= c[:-1]).all() and (c[-1] < c[0]).all()
    assert (r["status_trace"].numpy() == 0).all()


def test_argument_errors(built):
    m, x0, u0, cost = cartpole_case()
    N, T, n_act = u0.shape
    with pytest.raises(ValueError, match="locomotion model"):
        tds_amd.ilqr(m, x0, u0, cost, iterations=1, u_limits="model")
    with pytest.raises(ValueError, match="u_limits is None"):
        tds_amd.ilqr(m, x0, u0, cost, iterations=1, u_limits="ant")
    with pytest.raises(ValueError, match="lo > hi"):
        tds_amd.ilqr(m, x0, u0, cost, iterations=1, u_limits=(1.0, -1.0))
    with pytest.raises(ValueError, match="lo > hi"):
        tds_amd.ilqr(m, x0, u0, cost, iterations=1, u_limits=(-1.0, float("nan")))
    with pytest.raises(ValueError, match="do not broadcast"):
        tds_amd.ilqr(m, x0, u0, cost, iterations=1, u_limits=(-np.ones((N, T + 1, n_act)), 1.0))
    with pytest.raises(ValueError, match="u_limits is None"):
        tds_amd.ilqr(m, x0, u0, cost, iterations=1, u_limits=(-1.0, 0.0, 1.0))
    P = lq_problem(2, 2, 3, 4, 2)
    ok = np.ones((2, 3, 2))
    with pytest.raises(ValueError, match="dhi: expected"):
        hb.lqr_backward_box_host(*P, -ok, ok[:, :2])
    with pytest.raises(ValueError, match="lux"):
        hb.lqr_backward_box_host(*P[:6], P[6][..., :3], P[7], -ok, ok)
    bad = ok.copy()
    bad[1, 2, 0] = -2.0
    with pytest.raises(ValueError, match="dlo > dhi"):
        hb.lqr_backward_box_host(*P, -ok, bad)
    bad[1, 2, 0] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        hb.lqr_backward_box_host(*P, -ok, bad)
    # the C function's own check (the wrapper's is in front of it)
    out = [np.zeros((2, 3, 2)), np.zeros((2, 3, 2, 4)), np.zeros((2, 2)), np.zeros(2, dtype=np.int32),
           np.zeros((2, 3), dtype=np.int32), np.zeros((2, 3), dtype=np.int32)]
    arrays = [np.ascontiguousarray(a) for a in (*P, -ok, bad)]
    rc = hb.lib().tds_hip_lqr_backward_box_host(2, 3, 4, 2, *(a.ctypes.data for a in arrays), *(a.ctypes.data for a in out))
    assert rc == 1
    with pytest.raises(hb.TdsHipError, match="error 1: tds_hip_lqr_backward_box_host: dlo > dhi or a NaN bound"):
        hb._check(rc)
    for nx, nu, word in ((41, 2, "40 state entries"), (3, 17, "16 controls")):
        Q = lq_problem(1, 1, 2, nx, nu)
        with pytest.raises(hb.TdsHipError) as e:
            hb.lqr_backward_box_host(*Q, -np.ones((1, 2, nu)), np.ones((1, 2, nu)))
        assert "tds_hip error 2" in str(e.value) and word in str(e.value)
    fm, fx0, s_nom, u_nom, k, K, alpha = fb_case("cartpole")
    lo, hi = fb_bounds(u_nom)
    with pytest.raises(ValueError, match="together"):
        hb.feedback_rollout_host(fm, fx0, s_nom, u_nom, k, K, alpha, u_lo=lo)
    with pytest.raises(ValueError, match="u_hi: expected"):
        hb.feedback_rollout_host(fm, fx0, s_nom, u_nom, k, K, alpha, u_lo=lo, u_hi=hi[:, :3])
    with pytest.raises(ValueError, match="u_lo > u_hi"):
        hb.feedback_rollout_host(fm, fx0, s_nom, u_nom, k, K, alpha, u_lo=hi, u_hi=lo)
    nan = hi.copy()
    nan[0, 0, 0] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        hb.feedback_rollout_host(fm, fx0, s_nom, u_nom, k, K, alpha, u_lo=lo, u_hi=nan)
    rows, T = fx0.shape[0], u_nom.shape[1]
    s_out, u_out = np.zeros((rows, T + 1, s_nom.shape[2])), np.zeros(u_nom.shape)
    arrays = [np.ascontiguousarray(a) for a in (fx0, s_nom, u_nom, k, K, alpha)]
    rc = hb.lib().tds_hip_feedback_rollout_box_host(hb.C.byref(fm), rows, T, rows, *(a.ctypes.data for a in arrays), None,
                                                    lo.ctypes.data, nan.ctypes.data, s_out.ctypes.data,
                                                    u_out.ctypes.data)
    with pytest.raises(hb.TdsHipError, match="error 1: tds_hip_feedback_rollout_box_host: u_lo > u_hi or a NaN bound"):
        hb._check(rc)


@pytest.mark.parametrize("name", REFUSED)
def test_unsupported_models_are_refused_with_the_jacobians_message(name, built):
    m = tds_amd.load_model(name)
    nsd, n_act, _ = hb.trajectory_dims(m, 1)
    with pytest.raises(hb.TdsHipError) as e_jac:
        hb.jacobian_host(m, np.zeros((1, m.input_dim)))
    z = np.zeros
    with pytest.raises(hb.TdsHipError) as e:
        hb.feedback_rollout_host(m, z((1, m.input_dim)), z((1, 3, nsd)), z((1, 2, n_act)), z((1, 2, n_act)),
                                 z((1, 2, n_act, nsd)), 1.0, u_lo=-np.ones((1, 2, n_act)), u_hi=np.ones((1, 2, n_act)))
    assert str(e.value) == str(e_jac.value)
    with pytest.raises(hb.TdsHipError) as e:
        tds_amd.ilqr(m, z((1, m.input_dim)), z((1, 2, n_act)), quadratic_cost(m), iterations=1, u_limits=(-1.0, 1.0))
    assert str(e.value) == str(e_jac.value)
