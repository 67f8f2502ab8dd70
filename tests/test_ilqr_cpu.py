"""CPU: batched iLQR's host statements — lqr_backward_host against a numpy restatement and against the whole-horizon
QP, the non-PD refusal, feedback_rollout_host against chained step_host, the three pieces against independent
derivative paths, the ilqr driver over the host checkers, argument errors and refusals.

Bounds are 10 x the maximum measured on this file's seeded inputs (printed by each test before it asserts):
  lqr_backward_host vs numpy, max |a - b| / max(|b|, 1) over the 45 shapes: 6.44e-15 (a value above 1e-10 is a bug)
  gains rolled out vs the dense QP's minimiser: 9.4e-16;  -(dV1 + dV2) vs the QP's optimal decrease: 6.2e-16 relative
  dV1 vs the central difference in alpha of the closed-loop cost: cartpole 5.07e-12, pendulum5 4.33e-12 relative
  dV1 of the feedback-free pass vs k . grad_U J: cartpole 3.2e-16, pendulum5 3.7e-16 relative
  k of that pass vs -luu^-1 grad_U J: cartpole 6.26e-16, pendulum5 4.94e-15
  cartpole ilqr: max_problem |grad_U J|_inf(result) / |grad_U J|_inf(u0) = 4.7e-10"""
import functools
import os

import numpy as np
import pytest
import torch

from conftest import ROOT

import tds_amd
from tds_amd import hip_backend as hb

from test_param_derivs_cpu import REFUSED

LQR_VS_NUMPY = 6.44e-14
QP_GAINS, QP_VALUE = 9.4e-15, 6.2e-15
DV1_VS_FD = {"cartpole": 5.07e-11, "pendulum5": 4.33e-11}
DV1_VS_GRAD = {"cartpole": 3.2e-15, "pendulum5": 3.7e-15}
GRAD_RATIO = 4.7e-9
K_VS_GRAD = {"cartpole": 6.26e-15, "pendulum5": 4.94e-14}


def err(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1.0))) if a.size else 0.0


def spd(rng, lead, d):
    """[*lead, d, d] symmetric with eigenvalues in [0.5, 2]"""
    q = np.linalg.qr(rng.normal(size=lead + (d, d)))[0]
    e = rng.uniform(0.5, 2.0, lead + (d,))
    a = (q * e[..., None, :]) @ np.swapaxes(q, -1, -2)
    return 0.5 * (a + np.swapaxes(a, -1, -2))


def lq_problem(seed, n, T, nx, nu, mu=(0.0, 0.3)):
    """well conditioned by construction: lxx, luu SPD in [0.5, 2], |A|_2 <= 1"""
    rng = np.random.default_rng(seed)
    A = rng.normal(size=(n, T, nx, nx))
    A /= np.maximum(1.0, np.linalg.norm(A, 2, axis=(-2, -1)))[..., None, None]
    B = rng.normal(size=(n, T, nx, nu))
    lx, lu = rng.normal(size=(n, T + 1, nx)), rng.normal(size=(n, T, nu))
    lxx, luu = spd(rng, (n, T + 1), nx), spd(rng, (n, T), nu)
    lux = 0.1 * rng.normal(size=(n, T, nu, nx))
    return A, B, lx, lu, lxx, luu, lux, np.resize(np.asarray(mu, dtype=np.float64), n)


def lqr_numpy(A, B, lx, lu, lxx, luu, lux, mu):
    """the recursion restated with numpy products and np.linalg.solve"""
    n, T, nx, nu = B.shape
    k, K, dv = np.zeros((n, T, nu)), np.zeros((n, T, nu, nx)), np.zeros((n, 2))
    for p in range(n):
        Vx, Vxx = lx[p, T], lxx[p, T]
        for t in range(T - 1, -1, -1):
            a, b = A[p, t], B[p, t]
            Qx, Qu = lx[p, t] + a.T @ Vx, lu[p, t] + b.T @ Vx
            Qxx, Qux, Quu = lxx[p, t] + a.T @ Vxx @ a, lux[p, t] + b.T @ Vxx @ a, luu[p, t] + b.T @ Vxx @ b
            Qt = Quu + mu[p] * np.eye(nu)
            kk, KK = -np.linalg.solve(Qt, Qu), -np.linalg.solve(Qt, Qux)
            Vx = Qx + KK.T @ Quu @ kk + KK.T @ Qu + Qux.T @ kk
            Vxx = Qxx + KK.T @ Quu @ KK + KK.T @ Qux + Qux.T @ KK
            Vxx = 0.5 * (Vxx + Vxx.T)
            dv[p, 0] += kk @ Qu
            dv[p, 1] += 0.5 * kk @ Quu @ kk
            k[p, t], K[p, t] = kk, KK
    return k, K, dv


@pytest.mark.parametrize("T", [1, 2, 9])
@pytest.mark.parametrize("nu", [1, 3, 16])
@pytest.mark.parametrize("nx", [1, 2, 5, 37, 40])
def test_lqr_backward_host_against_numpy(nx, nu, T, built):
    P = lq_problem(1000 * nx + 10 * nu + T, 3, T, nx, nu)
    k, K, dv, status = hb.lqr_backward_host(*P)
    rk, rK, rdv = lqr_numpy(*P)
    e = max(err(k, rk), err(K, rK), err(dv, rdv))
    print(f"lqr_backward_host vs numpy nx={nx} nu={nu} T={T}: {e:.3e}")
    assert (status == 0).all()
    assert e <= LQR_VS_NUMPY


def test_gains_are_the_minimiser_of_the_whole_horizon_qp(built):
    """mu = 0: du_t = k_t + K_t dx_t rolled through dx_{t+1} = A dx_t + B du_t from dx_0 = 0 is the minimiser of
    sum_t lx.dx + lu.du + dx lxx dx / 2 + du luu du / 2 + du lux dx (+ the terminal terms), found here by eliminating
    the states (X = S U) and solving the dense normal equations.  dV1 + dV2 is the change of the cost the recursion
    expects at alpha = 1, a negative number: the QP's optimal value.  Read as the optimal DECREASE (what the line
    search compares with), the QP's figure is -(dV1 + dV2)."""
    T, nx, nu, n = 9, 5, 2, 2
    A, B, lx, lu, lxx, luu, lux, _ = lq_problem(77, n, T, nx, nu)
    mu = np.zeros(n)
    k, K, dv, status = hb.lqr_backward_host(A, B, lx, lu, lxx, luu, lux, mu)
    assert (status == 0).all()
    worst_u = worst_v = 0.0
    for p in range(n):
        S = np.zeros(((T + 1) * nx, T * nu))
        for t in range(T):  # X_{t+1} = A_t X_t + B_t U_t
            S[(t + 1) * nx:(t + 2) * nx] = A[p, t] @ S[t * nx:(t + 1) * nx]
            S[(t + 1) * nx:(t + 2) * nx, t * nu:(t + 1) * nu] += B[p, t]
        Lxx, Luu, Lux = np.zeros(((T + 1) * nx,) * 2), np.zeros((T * nu,) * 2), np.zeros((T * nu, (T + 1) * nx))
        for t in range(T + 1):
            Lxx[t * nx:(t + 1) * nx, t * nx:(t + 1) * nx] = lxx[p, t]
        for t in range(T):
            Luu[t * nu:(t + 1) * nu, t * nu:(t + 1) * nu] = luu[p, t]
            Lux[t * nu:(t + 1) * nu, t * nx:(t + 1) * nx] = lux[p, t]
        H = S.T @ Lxx @ S + Luu + Lux @ S + S.T @ Lux.T
        g = S.T @ lx[p].reshape(-1) + lu[p].reshape(-1)
        U = -np.linalg.solve(H, g)
        decrease = -0.5 * g @ U
        dx, du = np.zeros(nx), np.zeros((T, nu))
        for t in range(T):
            du[t] = k[p, t] + K[p, t] @ dx
            dx = A[p, t] @ dx + B[p, t] @ du[t]
        worst_u = max(worst_u, err(du.reshape(-1), U))
        worst_v = max(worst_v, abs(-(dv[p, 0] + dv[p, 1]) - decrease) / max(abs(decrease), 1.0))
        assert decrease > 0 and dv[p, 0] < 0 < dv[p, 1]
    print(f"QP: gains {worst_u:.3e}, value {worst_v:.3e}")
    assert worst_u <= QP_GAINS and worst_v <= QP_VALUE


@pytest.mark.parametrize("t_bad", [0, 2, 3])
def test_a_problem_that_is_not_positive_definite_is_reported_and_left_nominal(t_bad, built):
    n, T, nx, nu, bad = 4, 4, 5, 3, 2
    A, B, lx, lu, lxx, luu, lux, mu = lq_problem(5, n, T, nx, nu, mu=(0.0,))
    luu[bad, t_bad] = np.diag([1.0, -200.0, 1.0])
    k, K, dv, status = hb.lqr_backward_host(A, B, lx, lu, lxx, luu, lux, mu)
    assert status.tolist() == [0, 0, t_bad + 1, 0]
    assert not k[bad].any() and not K[bad].any() and not dv[bad].any()
    for p in (0, 1, 3):
        alone = hb.lqr_backward_host(*(a[p:p + 1] for a in (A, B, lx, lu, lxx, luu, lux, mu)))
        for got, one in zip((k, K, dv, status), alone):
            np.testing.assert_array_equal(got[p], one[0])
        assert k[p].any() and K[p].any()


# ---- feedback_rollout_host ---------------------------------------------------------------------------------------
FB_MODELS = ["cartpole", "pendulum5_plane", "ant", "ant_floating"]


def golden_x(name, idx):
    return np.ascontiguousarray(np.load(os.path.join(ROOT, "tests", "golden", f"{name}.npz"))["x"][list(idx)])


@functools.lru_cache(maxsize=None)
def fb_case(name, rows=3, T=5, P=None):
    """(m, x0 [rows], s_nom, u_nom, k, K [P], alpha [rows]); read only"""
    m = tds_amd.load_model(name)
    nsd, n_act, _ = hb.trajectory_dims(m, 1)
    P = rows if P is None else P
    rng = np.random.default_rng(21)
    x0 = golden_x(name, rng.integers(0, 48, rows))
    u_nom = rng.uniform(-0.3, 0.3, (P, T, n_act))
    s_nom = x0[np.arange(P) % rows, None, :nsd] + 0.05 * rng.normal(size=(P, T + 1, nsd))
    k, K = 0.1 * rng.normal(size=(P, T, n_act)), 0.05 * rng.normal(size=(P, T, n_act, nsd))
    alpha = rng.uniform(0.1, 1.0, rows)
    for a in (x0, s_nom, u_nom, k, K, alpha):
        a.setflags(write=False)
    return m, x0, s_nom, u_nom, k, K, alpha


def chained(m, x0, s_nom, u_nom, k, K, alpha, por):
    """a python loop of step_host with the feedback law in numpy; the law's sum runs in index order, as the library's"""
    nsd, n_act, _ = hb.trajectory_dims(m, 1)
    rows, T = x0.shape[0], u_nom.shape[1]
    s, u = np.zeros((rows, T + 1, nsd)), np.zeros((rows, T, n_act))
    x = x0.copy()
    s[:, 0] = x0[:, :nsd]
    for t in range(T):
        d = np.zeros((rows, n_act))
        for j in range(nsd):
            d += K[por, t, :, j] * (s[:, t, j] - s_nom[por, t, j])[:, None]
        u[:, t] = (u_nom[por, t] + alpha[:, None] * k[por, t]) + d
        x[:, :nsd], x[:, nsd:nsd + n_act] = s[:, t], u[:, t]
        s[:, t + 1] = hb.step_host(m, x)[:, :nsd]
    return s, u


@pytest.mark.parametrize("name", FB_MODELS)
def test_feedback_rollout_host_without_gains_is_chained_step_host(name, built):
    m, x0, s_nom, u_nom, k, K, alpha = fb_case(name)
    s, u = hb.feedback_rollout_host(m, x0, s_nom, u_nom, np.zeros_like(k), np.zeros_like(K), alpha)
    rs, ru = chained(m, x0, s_nom, u_nom, np.zeros_like(k), np.zeros_like(K), alpha, np.arange(3))
    np.testing.assert_array_equal(u, u_nom)
    np.testing.assert_array_equal(s, rs)
    assert np.isfinite(s).all() and np.abs(s[:, -1] - s[:, 0]).max() > 0


@pytest.mark.parametrize("name", FB_MODELS)
def test_feedback_rollout_host_with_gains_is_the_python_loop(name, built):
    m, x0, s_nom, u_nom, k, K, alpha = fb_case(name)
    s, u = hb.feedback_rollout_host(m, x0, s_nom, u_nom, k, K, alpha)
    rs, ru = chained(m, x0, s_nom, u_nom, k, K, alpha, np.arange(3))
    np.testing.assert_array_equal(u, ru)
    np.testing.assert_array_equal(s, rs)
    assert np.abs(u - u_nom).max() > 1e-3


@pytest.mark.parametrize("name", FB_MODELS)
def test_problem_of_row_is_replicated_gains(name, built):
    m, x0, s_nom, u_nom, k, K, alpha = fb_case(name, rows=3, P=2)
    por = np.array([1, 0, 1])
    s, u = hb.feedback_rollout_host(m, x0, s_nom, u_nom, k, K, alpha, problem_of_row=por)
    rs, ru = hb.feedback_rollout_host(m, x0, s_nom[por], u_nom[por], k[por], K[por], alpha)
    np.testing.assert_array_equal(s, rs)
    np.testing.assert_array_equal(u, ru)


# ---- the three pieces against independent paths ------------------------------------------------------------------
def quadratic_cost(m, N=None, R=0.05):
    nsd, n_act, _ = hb.trajectory_dims(m, 1)
    w = np.linspace(1.0, 2.0, nsd)
    return tds_amd.QuadraticCost(np.diag(w), R * np.eye(n_act), 10.0 * np.diag(w))


@functools.lru_cache(maxsize=None)
def pieces(name, T=12, N=3):
    """(m, cost, x0, s, u, A, B, expansion) at the open-loop trajectory of seeded actions"""
    m = tds_amd.load_model(name)
    nsd, n_act, _ = hb.trajectory_dims(m, 1)
    rng = np.random.default_rng(31)
    x0 = golden_x(name, [1, 7, 20][:N])
    u0 = rng.uniform(-1.0, 1.0, (N, T, n_act))
    s, u = hb.feedback_rollout_host(m, x0, np.zeros((N, T + 1, nsd)), u0, np.zeros((N, T, n_act)),
                                    np.zeros((N, T, n_act, nsd)), 0.0)
    cost = quadratic_cost(m)
    jac = hb.jacobian_host(m, hb.trajectory_records(m, x0, s, u), rows=range(nsd), cols=range(nsd + n_act))
    jac = jac.reshape(N, T, nsd, nsd + n_act)
    A, B = np.ascontiguousarray(jac[..., :nsd]), np.ascontiguousarray(jac[..., nsd:])
    ex = [t.numpy() for t in cost.expand(torch.from_numpy(s), torch.from_numpy(u))]
    return m, cost, x0, s, u, A, B, ex


@pytest.mark.parametrize("name", ["cartpole", "pendulum5"])
def test_dv1_is_the_slope_of_the_closed_loop_cost_in_alpha(name, built):
    m, cost, x0, s, u, A, B, (J, lx, lu, lxx, luu, lux) = pieces(name)
    N = x0.shape[0]
    k, K, dv, status = hb.lqr_backward_host(A, B, lx, lu, lxx, luu, lux, np.zeros(N))
    assert (status == 0).all()
    h = 1e-4
    Jh = []
    for a in (h, -h):
        sa, ua = hb.feedback_rollout_host(m, x0, s, u, k, K, a)
        Jh.append(cost.value(torch.from_numpy(sa), torch.from_numpy(ua)).numpy())
    slope = (Jh[0] - Jh[1]) / (2 * h)
    e = float(np.max(np.abs(slope - dv[:, 0]) / np.maximum(np.abs(dv[:, 0]), 1.0)))
    print(f"{name}: dV1 {dv[:, 0]} vs central difference {slope}: {e:.3e}")
    assert (dv[:, 0] < 0).all()
    assert e <= DV1_VS_FD[name]


@pytest.mark.parametrize("name", ["cartpole", "pendulum5"])
def test_dv1_without_feedback_is_k_dot_the_gradient_in_u(name, built):
    """Identity: run the backward pass with lxx = 0 and lux = 0 (mu = 0).  Then V_xx stays 0 at every step, so
    Q_ux = 0, K = 0 and V_x = Q_x = lx + A^T V_x is the plain costate lambda_t; Q_u,t = lu_t + B_t^T lambda_{t+1} is
    the gradient of the total cost in u_t, k_t = -luu^-1 Q_u,t, and dV1 = sum_t k_t . dJ/du_t.  The gradient comes
    from the reverse-mode trajectory derivative (cotangent lx on the states) plus the cost's own lu."""
    m, cost, x0, s, u, A, B, (J, lx, lu, lxx, luu, lux) = pieces(name)
    N, T = u.shape[:2]
    nsd, n_act, _ = hb.trajectory_dims(m, 1)
    k, K, dv, status = hb.lqr_backward_host(A, B, lx, lu, np.zeros_like(lxx), luu, np.zeros_like(lux), np.zeros(N))
    assert (status == 0).all() and not K.any()
    grad = grad_u(m, x0, s, u, lx, lu)
    ek = err(k, -np.linalg.solve(luu, grad[..., None])[..., 0])
    print(f"{name}: k vs -luu^-1 grad_U J: {ek:.3e}")
    assert ek <= K_VS_GRAD[name]
    want = (k * grad).sum(axis=(1, 2))
    e = float(np.max(np.abs(dv[:, 0] - want) / np.maximum(np.abs(want), 1.0)))
    print(f"{name}: dV1 {dv[:, 0]} vs k . grad {want}: {e:.3e}")
    assert e <= DV1_VS_GRAD[name]


def grad_u(m, x0, s, u, lx, lu):
    """dJ/du [N, T, n_act] from trajectory_vjp_host: the cotangent on s_1 .. s_T is lx, the direct term is lu"""
    nsd, n_act, _ = hb.trajectory_dims(m, 1)
    T = u.shape[1]
    x = x0.copy()
    x[:, nsd:nsd + n_act] = u[:, 0]
    _, gx0, gu, _ = hb.trajectory_vjp_host(m, x, np.ascontiguousarray(lx[:, 1:]), T, u=np.ascontiguousarray(u[:, 1:]))
    return np.concatenate([gx0[:, None, nsd:nsd + n_act], gu], axis=1) + lu


# ---- the driver ----------------------------------------------------------------------------------------------------
def armijo_holds(m, cost, x0, s, u, mu, alpha, J_new, armijo=1e-4):
    """recompute one iteration's model from the host pieces and check the accepted steps' inequality"""
    N, T = u.shape[:2]
    nsd, n_act, _ = hb.trajectory_dims(m, 1)
    jac = hb.jacobian_host(m, hb.trajectory_records(m, x0, s, u), rows=range(nsd), cols=range(nsd + n_act))
    jac = jac.reshape(N, T, nsd, nsd + n_act)
    J, lx, lu, lxx, luu, lux = [t.numpy() for t in cost.expand(torch.from_numpy(s), torch.from_numpy(u))]
    k, K, dv, status = hb.lqr_backward_host(np.ascontiguousarray(jac[..., :nsd]), np.ascontiguousarray(jac[..., nsd:]),
                                            lx, lu, lxx, luu, lux, mu)
    sa, ua = hb.feedback_rollout_host(m, x0, s, u, k, K, alpha)
    Ja = cost.value(torch.from_numpy(sa), torch.from_numpy(ua)).numpy()
    took = alpha > 0
    np.testing.assert_array_equal(Ja[took], J_new[took])
    assert (status[took] == 0).all()
    assert ((J - Ja)[took] >= (armijo * -(alpha * dv[:, 0] + alpha ** 2 * dv[:, 1]))[took]).all()
    return sa, ua, took


def test_ilqr_on_the_cartpole(built):
    m = tds_amd.load_model("cartpole")
    nsd, n_act, _ = hb.trajectory_dims(m, 1)
    N, T, iters = 3, 40, 4
    x0 = golden_x("cartpole", [0, 5, 9])
    u0 = np.random.default_rng(41).uniform(-2.0, 2.0, (N, T, n_act))
    cost = quadratic_cost(m)
    r = tds_amd.ilqr(m, x0, u0, cost, iterations=iters)
    c, al = r["cost"].numpy(), r["alpha"].numpy()
    assert c.shape == (iters + 1, N) and al.shape == (iters, N) and tuple(r["s"].shape) == (N, T + 1, nsd)
    assert (c[1:] <= c[:-1]).all() and (c[-1] < c[0]).all()
    assert (al[0] > 0).all() and (r["status"].numpy() == 0).all()
    # every accepted step satisfies the Armijo inequality, recomputed from the pieces along the driver's own path
    s, u = hb.feedback_rollout_host(m, x0, np.zeros((N, T + 1, nsd)), u0, np.zeros((N, T, n_act)),
                                    np.zeros((N, T, n_act, nsd)), 0.0)
    for i in range(iters):
        sa, ua, took = armijo_holds(m, cost, x0, s, u, r["mu_trace"][i].numpy(), al[i], c[i + 1])
        s, u = np.where(took[:, None, None], sa, s), np.where(took[:, None, None], ua, u)
    np.testing.assert_array_equal(s, r["s"].numpy())
    np.testing.assert_array_equal(u, r["u"].numpy())

    def gnorm(s_, u_):
        _, lx, lu, *_ = [t.numpy() for t in cost.expand(torch.from_numpy(s_), torch.from_numpy(u_))]
        return np.abs(grad_u(m, x0, s_, u_, lx, lu)).max(axis=(1, 2))

    s0, _ = hb.feedback_rollout_host(m, x0, np.zeros((N, T + 1, nsd)), u0, np.zeros((N, T, n_act)),
                                     np.zeros((N, T, n_act, nsd)), 0.0)
    ratio = float((gnorm(s, u) / gnorm(s0, u0)).max())
    print(f"cartpole ilqr: cost {c[0]} -> {c[-1]}, |grad_U J|_inf ratio {ratio:.3e}")
    assert ratio <= GRAD_RATIO and ratio < 1.0


def test_ilqr_through_contacts_and_rejected_steps(built):
    """pendulum5_plane with spheres on the ground.  Problem 0 has an honest cost; problem 1's R is indefinite, so its
    Q_uu + mu I is not positive definite until mu has grown past it: those iterations are rejected (status != 0,
    alpha 0, the cost and the trajectory kept, mu multiplied), the later ones accepted (mu divided)."""
    name = "pendulum5_plane"
    m = tds_amd.load_model(name)
    nsd, n_act, _ = hb.trajectory_dims(m, 1)
    N, T, iters = 2, 8, 5
    g = np.load(os.path.join(ROOT, "tests", "golden", f"{name}.npz"))
    down = np.flatnonzero(g["active_contacts"] > 0)[:N]
    assert down.size == N
    x0 = np.ascontiguousarray(g["x"][down])
    u0 = np.random.default_rng(42).uniform(-0.5, 0.5, (N, T, n_act))
    w = np.linspace(1.0, 2.0, nsd)
    R = np.stack([0.05 * np.eye(n_act), -0.5 * np.eye(n_act)])[:, None]
    cost = tds_amd.QuadraticCost(np.diag(w), R, 10.0 * np.diag(w))
    r = tds_amd.ilqr(m, x0, u0, cost, iterations=iters, mu0=0.01, mu_factor=10.0, mu_min=1e-9)
    c, al, mu, st = r["cost"].numpy(), r["alpha"].numpy(), r["mu_trace"].numpy(), r["status_trace"].numpy()
    assert (c[1:] <= c[:-1]).all() and c[-1, 0] < c[0, 0]
    assert (st[:, 0] == 0).all() and (al[0, 0] > 0)
    # problem 1: mu = 0.01, 0.1 cannot lift -0.5; 1.0 does
    assert (st[:2, 1] != 0).all() and (al[:2, 1] == 0).all() and (c[:3, 1] == c[0, 1]).all()
    np.testing.assert_allclose(mu[:3, 1], [0.01, 0.1, 1.0], rtol=1e-12)
    assert st[2, 1] == 0
    for i in range(iters):
        grew = (al[i] == 0)
        np.testing.assert_allclose(mu[i + 1], np.where(grew, mu[i] * 10.0, np.maximum(mu[i] / 10.0, 1e-9)), rtol=1e-12)
        assert ((st[i] == 0) | grew).all()
    np.testing.assert_array_equal(r["mu"].numpy(), mu[-1])
    np.testing.assert_array_equal(r["status"].numpy(), st[-1])


# ---- argument errors and refusals ----------------------------------------------------------------------------------
def test_dimensions_beyond_the_bounds_are_refused(built):
    for nx, nu, word in ((41, 2, "40 state entries"), (3, 17, "16 controls")):
        P = lq_problem(1, 1, 2, nx, nu)
        with pytest.raises(hb.TdsHipError) as e:
            hb.lqr_backward_host(*P)
        assert "tds_hip error 2" in str(e.value) and word in str(e.value)


def test_argument_errors(built):
    A, B, lx, lu, lxx, luu, lux, mu = lq_problem(2, 2, 3, 4, 2)
    with pytest.raises(ValueError, match="lux"):
        hb.lqr_backward_host(A, B, lx, lu, lxx, luu, lux[:, :, :, :3], mu)
    with pytest.raises(ValueError, match="lx"):
        hb.lqr_backward_host(A, B, lx[:, :3], lu, lxx, luu, lux, mu)
    with pytest.raises(ValueError, match=r"A: expected"):
        hb.lqr_backward_host(A[:, :, :3], B, lx, lu, lxx, luu, lux, mu)
    m, x0, s_nom, u_nom, k, K, alpha = fb_case("cartpole")
    with pytest.raises(ValueError, match="K"):
        hb.feedback_rollout_host(m, x0, s_nom, u_nom, k, K[..., :3], alpha)
    with pytest.raises(ValueError, match="one row per problem"):
        hb.feedback_rollout_host(m, x0[:2], s_nom, u_nom, k, K, alpha[:2])
    with pytest.raises(hb.TdsHipError, match="problem_of_row outside"):
        hb.feedback_rollout_host(m, x0, s_nom, u_nom, k, K, alpha, problem_of_row=[0, 3, 1])
    with pytest.raises(ValueError, match="T >= 1"):
        hb.feedback_rollout_host(m, x0, s_nom[:, :1], u_nom[:, :0], k[:, :0], K[:, :0], alpha)
    with pytest.raises(ValueError, match="ilqr: expected"):
        tds_amd.ilqr(m, x0, u_nom[:2], quadratic_cost(m))
    # the refusals no case above reaches: n = 2, T = 2, nx = 4, nu = 1
    P = lq_problem(3, 2, 2, 4, 1)
    with pytest.raises(ValueError, match=r"A: expected \[n, T, nx, nx\] and B \[n, T, nx, nu\], got \(2, 2, 4, 4\) and \(2, 1, 4, 1\)"):
        hb.lqr_backward_host(P[0], P[1][:, :1], *P[2:])
    with pytest.raises(ValueError, match="broadcast"):
        hb.lqr_backward_host(*P[:7], np.zeros(3))
    with pytest.raises(ValueError, match=rf"x0: expected \[rows, {m.input_dim}\], got \[3, {m.input_dim - 1}\]"):
        hb.feedback_rollout_host(m, x0[:, :-1], s_nom, u_nom, k, K, alpha)
    with pytest.raises(ValueError, match=r"s_nom: expected \[P, T \+ 1, 4\] with T >= 1, got \[3, 6, 3\]"):
        hb.feedback_rollout_host(m, x0, s_nom[..., :3], u_nom, k, K, alpha)
    with pytest.raises(ValueError, match=r"problem_of_row: expected \[3\], got \[2\]"):
        hb.feedback_rollout_host(m, x0, s_nom, u_nom, k, K, alpha, problem_of_row=[0, 1])
    with pytest.raises(ValueError, match="broadcast"):
        hb.feedback_rollout_host(m, x0, s_nom, u_nom, k, K, alpha[:2])


@pytest.mark.parametrize("name", REFUSED)
def test_unsupported_models_are_refused_with_the_jacobians_message(name, built):
    m = tds_amd.load_model(name)
    nsd, n_act, _ = hb.trajectory_dims(m, 1)
    with pytest.raises(hb.TdsHipError) as e_jac:
        hb.jacobian_host(m, np.zeros((1, m.input_dim)))
    z = np.zeros
    with pytest.raises(hb.TdsHipError) as e:
        hb.feedback_rollout_host(m, z((1, m.input_dim)), z((1, 3, nsd)), z((1, 2, n_act)), z((1, 2, n_act)),
                                 z((1, 2, n_act, nsd)), 1.0)
    assert str(e.value) == str(e_jac.value)
    with pytest.raises(hb.TdsHipError) as e:
        tds_amd.ilqr(m, z((1, m.input_dim)), z((1, 2, n_act)), quadratic_cost(m), iterations=1)
    assert str(e.value) == str(e_jac.value)
