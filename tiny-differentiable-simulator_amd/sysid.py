"""Batched system identification: N nonlinear least-squares problems over the model's parameters at once
(Levenberg-Marquardt with box bounds, after the reference's CeresEstimator; N random starts are its
BasinHoppingEstimator's workers).

Per iteration: ONE ``trajectory_jvp`` with the p unit directions on theta (the states and their derivatives in the
parameters), ONE ``lm_step`` (cost, gradient, Gauss-Newton matrix and the damped, box-constrained step for every
damping of a ladder), ONE k = 0 trajectory call over every candidate of every problem, and ONE cost-only ``lm_step``
that prices them.  Given a ``HipSim`` the loop runs on the device; given a ``Model`` the same driver runs over the
``_host`` checkers on CPU tensors, so it can be tested without a GPU.  Every decision is a ``torch.where`` per problem:
the driver itself never waits for the device.

Out of scope: robust losses, x0 as an unknown, rigid-body worlds, and what ``trajectory_jvp`` refuses (spherical
joints, worlds of several bodies, f32 handles)."""
from . import hip_backend
from . import model as _model

LAMBDA_MIN, LAMBDA_MAX = 1e-16, 1e32
DEFAULT_LADDER = (1.0 / 9.0, 1.0 / 3.0, 1.0, 3.0, 9.0)
REASON_RUNNING, REASON_FTOL, REASON_PTOL, REASON_LAMBDA = 0, 1, 2, 3


class _DeviceOps:
    """the two native calls on a HipSim (CUDA tensors)"""

    def __init__(self, sim):
        self.sim, self.model = sim, sim.model
        self.device = f"cuda:{sim.device}"

    def trajectory(self, x0, v, steps, every, u, params, theta):
        return self.sim.trajectory_jvp(x0, v, steps, every, u, params, theta)

    def lm_step(self, row_start, s, s_obs, js, lam, w, dlo, dhi):
        return self.sim.lm_step(row_start, s, s_obs, js, lam, w, dlo, dhi, check=False)  # (built below)


class _HostOps:
    """the same calls over the _host checkers (CPU tensors in and out)"""

    def __init__(self, m):
        self.model, self.device = m, "cpu"

    def trajectory(self, x0, v, steps, every, u, params, theta):
        import torch

        np_ = lambda t: None if t is None else t.numpy()  # noqa: E731
        s, js = hip_backend.trajectory_jvp_host(self.model, np_(x0), np_(v), steps, every, np_(u), params, np_(theta))
        return torch.from_numpy(s), None if js is None else torch.from_numpy(js)

    def lm_step(self, row_start, s, s_obs, js, lam, w, dlo, dhi):
        import torch

        np_ = lambda t: None if t is None else t.numpy()  # noqa: E731
        out = hip_backend.lm_step_host(np_(row_start), np_(s), np_(s_obs), np_(js), np_(lam), np_(w), np_(dlo), np_(dhi))
        return {k: torch.from_numpy(a) for k, a in out.items()}


def sysid_starts(theta0, lo, hi, starts: int, seed: int = 0):
    """[starts, p] initial guesses for ``sysid``: row 0 is theta0 (clamped into the box), the others are uniform in
    [lo, hi] (numpy's default_rng(seed)).  lo, hi broadcast to [p] and must be finite."""
    import numpy as np
    import torch

    theta0 = np.asarray(theta0, dtype=np.float64).reshape(-1)
    lo, hi = (np.broadcast_to(np.asarray(b, dtype=np.float64), theta0.shape) for b in (lo, hi))
    if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (lo <= hi).all()):
        raise ValueError("sysid_starts: needs finite bounds lo <= hi")
    if starts < 1:
        raise ValueError("sysid_starts: needs at least one start")
    out = np.random.default_rng(seed).uniform(lo, hi, (int(starts), theta0.shape[0]))
    out[0] = np.clip(theta0, lo, hi)
    return torch.from_numpy(out)


def sysid(sim_or_model, x0, s_obs, params, theta0, steps: int, every: int = 1, u=None, rows_per_problem=None,
          row_start=None, weights=None, bounds=None, iterations: int = 20, lambda0: float = 1e-4,
          ladder=DEFAULT_LADDER, eta: float = 1e-3, ftol: float = 1e-6, ptol: float = 1e-8):
    """Identify the model parameters ``params`` (a selection as for ``jvp_params``) of N problems at once from
    observed trajectories: minimise cost = 1/2 sum (w (s(theta) - s_obs))^2 per problem.

    x0 [rows, input_dim] are the first records of the rows' trajectories, u None or [rows, steps - 1, n_act] their
    later actions, s_obs [rows, n_rec, nsd] the observed states after every, 2 every, .. steps (n_rec = steps //
    every; NaN: a missing measurement, weight 0).  Problem i owns rows_per_problem consecutive rows (default: rows /
    N), or the rows row_start[i] .. row_start[i + 1] - 1 (row_start [N + 1] host ints); its rows share its theta.
    theta0 [N, p] (or [p]: N = 1) are the starts.  weights broadcast from [nsd], [n_rec, nsd] or [rows, n_rec, nsd]
    (None: 1).  bounds None or (lo, hi), each broadcasting to [N, p] (+-inf: none on that side); theta0 is clamped into
    the box first and every iterate stays inside it.

    Per iteration and problem, ``lm_step`` solves the damped step for lambda times every entry of ``ladder``; the
    candidates theta_c = clamp(theta + delta_l) are rolled out and priced, rho_l = (cost - cost_l) / pred_l is their
    gain ratio, and among those with status 0, pred_l > 0, a finite cost and rho_l >= eta the one of lowest cost is
    taken: lambda <- lambda_l max(1/3, 1 - (2 rho - 1)^3), nu <- 2 (Ceres's trust-region rule with lambda = 1 /
    radius).  Where none qualifies theta is kept, lambda <- lambda max(ladder) nu and nu <- 2 nu.  lambda stays in
    [1e-16, 1e32].  A problem freezes (its theta no longer moves) with reason 1 after an accepted step with cost -
    cost_new <= ftol cost, reason 2 where every candidate has |delta| <= ptol (|theta| + ptol), reason 3 where
    lambda reached its upper end; a tolerance of 0 switches its test off.  A problem whose data are not finite at its
    theta (status 2: cost = inf, every delta 0) is not taken for stalled: it keeps its theta, its lambda grows and it
    ends on reason 3 with cost = inf.

    Returns a dict: theta [N, p], cost [N], reason [N] (0: still running), iterations_used [N], best (the index of
    the lowest cost), H [N, p, p], g [N, p], clamped [N] (bit a: parameter a at a bound in the step that was taken, or
    in the first candidate's where none was) of the LAST linearisation (H^-1 is what the parameters' covariance is read
    from), s [rows, n_rec, nsd] at theta, and per iteration cost_trace [it + 1, N], lambda_trace [it + 1, N], theta_trace [it + 1, N, p],
    pick_trace [it, N] (the candidate taken, -1: none), rho_trace, pred_trace, cand_cost_trace, status_trace
    [it, N, L].  Tensors on the handle's device (a HipSim) or the CPU (a Model).

    Memory: js is materialised, rows p n_rec nsd doubles per iteration (T = 1000 steps of the Ant, 512 rows, p = 9:
    1 GB); ``every`` is the lever for it."""
    import torch

    ops = _HostOps(sim_or_model) if isinstance(sim_or_model, _model.Model) else _DeviceOps(sim_or_model)
    m, dev = ops.model, ops.device
    nsd, n_act, n_rec = hip_backend.trajectory_dims(m, steps, every)
    f64 = lambda a: (a if isinstance(a, torch.Tensor) else torch.tensor(a)).to(dev, torch.float64)  # noqa: E731
    x0 = f64(x0).contiguous()
    s_obs = f64(s_obs).contiguous()
    theta = f64(theta0)
    theta = (theta[None] if theta.dim() == 1 else theta).contiguous()
    rows, (N, p) = int(x0.shape[0]), (int(d) for d in theta.shape)
    if p != len(params) or not 1 <= p <= hip_backend.LM_MAX_P:
        raise ValueError(f"sysid: theta0 [N, {len(params)}] with 1 <= p <= {hip_backend.LM_MAX_P}, got {list(theta.shape)}")
    if n_rec < 1 or tuple(x0.shape) != (rows, m.input_dim) or tuple(s_obs.shape) != (rows, n_rec, nsd):
        raise ValueError(f"sysid: expected x0 [rows, {m.input_dim}] and s_obs [rows, {n_rec}, {nsd}], got "
                         f"{list(x0.shape)} and {list(s_obs.shape)}")
    u = None if u is None else f64(u).contiguous()
    ladder = [float(a) for a in ladder]
    L, lad_max = len(ladder), max(ladder, default=0.0)  # (host numbers: the loop below touches device tensors only)
    lad = torch.tensor(ladder, dtype=torch.float64, device=dev)
    if not 1 <= L <= hip_backend.LM_MAX_LAMBDA or not all(a > 0 for a in ladder) or iterations < 0:
        raise ValueError(f"sysid: needs 1 .. {hip_backend.LM_MAX_LAMBDA} positive ladder entries and iterations >= 0")
    # the rows of the problems (host integers: part of the call's shape, not of its data)
    if row_start is None:
        per = rows // N if rows_per_problem is None else int(rows_per_problem)
        starts_h = [i * per for i in range(N + 1)]
    elif rows_per_problem is not None:
        raise ValueError("sysid: rows_per_problem or row_start, not both")
    else:
        starts_h = [int(r) for r in row_start]
    if len(starts_h) != N + 1 or starts_h[0] != 0 or starts_h[-1] != rows or \
            any(b < a for a, b in zip(starts_h, starts_h[1:])):
        raise ValueError(f"sysid: the problems' rows must run from 0 to rows = {rows} without gaps, got {starts_h}")
    counts = [b - a for a, b in zip(starts_h, starts_h[1:])]
    row_start_t = torch.tensor(starts_h, dtype=torch.int32, device=dev)
    prob_of_row = torch.repeat_interleave(torch.arange(N, device=dev), torch.tensor(counts, device=dev))
    # the candidates' layout: problem i L + l holds the rows of problem i once more
    cand_src, cand_counts = [], []
    for i in range(N):
        for _ in range(L):
            cand_src.extend(range(starts_h[i], starts_h[i + 1]))
            cand_counts.append(counts[i])
    cand_src = torch.tensor(cand_src, dtype=torch.long, device=dev)
    cand_start_h = [0]
    for c in cand_counts:
        cand_start_h.append(cand_start_h[-1] + c)
    cand_row_start = torch.tensor(cand_start_h, dtype=torch.int32, device=dev)
    cand_prob_of_row = torch.repeat_interleave(torch.arange(N * L, device=dev), torch.tensor(cand_counts, device=dev))
    # row r of problem i under candidate l sits at cand_first[i] + l counts[i] + (r - starts[i])
    first = torch.tensor([cand_start_h[i * L] for i in range(N)], dtype=torch.long, device=dev)[prob_of_row]
    cnt_r = torch.tensor(counts, dtype=torch.long, device=dev)[prob_of_row]
    within = torch.arange(rows, device=dev) - torch.tensor(starts_h[:-1], dtype=torch.long, device=dev)[prob_of_row]
    # weights; a missing observation counts for nothing
    try:
        W = torch.ones((rows, n_rec, nsd), dtype=torch.float64, device=dev) if weights is None else \
            f64(weights).expand(rows, n_rec, nsd)
    except RuntimeError:
        raise ValueError(f"sysid: weights do not broadcast to {[rows, n_rec, nsd]}") from None
    W = torch.where(torch.isnan(s_obs), torch.zeros_like(s_obs), W).contiguous()
    lo = hi = None
    if bounds is not None:
        try:
            lo, hi = (f64(b).expand(N, p).contiguous() for b in bounds)
        except (RuntimeError, ValueError, TypeError):
            raise ValueError(f"sysid: bounds is None or (lo, hi) that broadcast to [N, p] = {[N, p]}") from None
        if not bool((lo <= hi).all()):
            raise ValueError("sysid: bounds: lo > hi somewhere, or a NaN bound")
        theta = torch.minimum(torch.maximum(theta, lo), hi)
    V = hip_backend.trajectory_directions(m.input_dim, (), p, device=dev)[None].expand(rows, -1, -1).contiguous()
    x0_c, W_c, obs_c = x0[cand_src], W[cand_src], s_obs[cand_src]
    u_c = None if u is None else u[cand_src]

    lam = torch.full((N,), float(lambda0), dtype=torch.float64, device=dev).clamp(LAMBDA_MIN, LAMBDA_MAX)
    nu = torch.full((N,), 2.0, dtype=torch.float64, device=dev)
    reason = torch.zeros(N, dtype=torch.int32, device=dev)
    used = torch.zeros(N, dtype=torch.int32, device=dev)
    J = s = None
    H = torch.zeros((N, p, p), dtype=torch.float64, device=dev)
    g = torch.zeros((N, p), dtype=torch.float64, device=dev)
    clamped = torch.zeros(N, dtype=torch.int32, device=dev)
    costs, lams, thetas, picks, rhos, preds, ccosts, stats = [], [lam], [theta], [], [], [], [], []
    for _ in range(int(iterations)):
        s_lin, js = ops.trajectory(x0, V, steps, every, u, params, theta[prob_of_row].contiguous())
        lams_l = (lam[:, None] * lad[None, :]).clamp(LAMBDA_MIN, LAMBDA_MAX).contiguous()
        st = ops.lm_step(row_start_t, s_lin, s_obs, js, lams_l, W, None if lo is None else lo - theta,
                         None if hi is None else hi - theta)
        if J is None:  # (later iterations carry the cost their candidate was priced at: the trace cannot rise)
            J, s = st["cost"], s_lin
            costs.append(J)
        H, g = st["H"], st["g"]
        delta, pred, status = st["delta"], st["pred"], st["status"]
        cand = theta[:, None, :] + delta
        if lo is not None:
            cand = torch.minimum(torch.maximum(cand, lo[:, None, :]), hi[:, None, :])
        th_c = cand.reshape(N * L, p)[cand_prob_of_row].contiguous()
        s_c, _ = ops.trajectory(x0_c, None, steps, every, u_c, params, th_c)
        Jc = ops.lm_step(cand_row_start, s_c, obs_c, None, None, W_c, None, None)["cost"].reshape(N, L)
        rho = (J[:, None] - Jc) / pred
        ok = (status == 0) & (pred > 0) & torch.isfinite(Jc) & (rho >= eta)
        live = reason == 0
        # reason 2: no candidate moves theta
        # (a problem whose data are not finite, status 2, has delta = 0 by definition: that is no convergence)
        small = delta.norm(dim=2) <= ptol * (theta.norm(dim=1) + ptol)[:, None]
        stalled = live & small.all(dim=1) & (status != 2).all(dim=1) & (ptol > 0)
        score = torch.where(ok, Jc, torch.full_like(Jc, float("inf")))
        best = score.argmin(dim=1)
        accept = ok.any(dim=1) & live & ~stalled
        rho_b = rho.gather(1, best[:, None])[:, 0]
        J_b = Jc.gather(1, best[:, None])[:, 0]
        theta = torch.where(accept[:, None], cand.gather(1, best[:, None, None].expand(N, 1, p))[:, 0], theta)
        taken_rows = first + best[prob_of_row] * cnt_r + within
        s = torch.where(accept[prob_of_row][:, None, None], s_c[taken_rows], s)
        converged = accept & (J - J_b <= ftol * J) & (ftol > 0)
        J = torch.where(accept, J_b, J)
        lam_acc = lams_l.gather(1, best[:, None])[:, 0] * torch.clamp(1.0 - (2.0 * rho_b - 1.0) ** 3, min=1.0 / 3.0)
        lam_new = torch.where(accept, lam_acc, lam * lad_max * nu).clamp(LAMBDA_MIN, LAMBDA_MAX)
        moving = live & ~stalled
        lam = torch.where(moving, lam_new, lam)
        nu = torch.where(moving, torch.where(accept, torch.full_like(nu, 2.0), 2.0 * nu), nu)
        reason = torch.where(stalled, torch.full_like(reason, REASON_PTOL), reason)
        reason = torch.where(converged, torch.full_like(reason, REASON_FTOL), reason)
        reason = torch.where(moving & ~converged & (lam >= LAMBDA_MAX), torch.full_like(reason, REASON_LAMBDA), reason)
        used = used + live.to(torch.int32)
        clamped = st["clamped"].gather(1, torch.where(accept, best, torch.zeros_like(best))[:, None])[:, 0]
        costs.append(J)
        lams.append(lam)
        thetas.append(theta)
        picks.append(torch.where(accept, best, torch.full_like(best, -1)))
        rhos.append(rho)
        preds.append(pred)
        ccosts.append(Jc)
        stats.append(status)
    if J is None:  # iterations = 0: the cost at the start
        s, _ = ops.trajectory(x0, None, steps, every, u, params, theta[prob_of_row].contiguous())
        J = ops.lm_step(row_start_t, s, s_obs, None, None, W, None, None)["cost"]
        costs.append(J)
    hist = lambda a, shape, dt: torch.stack(a) if a else torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
    return {"theta": theta, "cost": J, "reason": reason, "iterations_used": used, "best": J.argmin(), "H": H, "g": g,
            "clamped": clamped, "s": s, "cost_trace": torch.stack(costs), "lambda_trace": torch.stack(lams),
            "theta_trace": torch.stack(thetas),
            "pick_trace": hist(picks, (0, N), torch.long), "rho_trace": hist(rhos, (0, N, L), torch.float64),
            "pred_trace": hist(preds, (0, N, L), torch.float64),
            "cand_cost_trace": hist(ccosts, (0, N, L), torch.float64),
            "status_trace": hist(stats, (0, N, L), torch.int32)}
