"""Batched iLQR over the contact step: N trajectory-optimisation problems at once.

Per iteration: the step Jacobians of the N T records of the nominal trajectories (``jacobian``: [A_t | B_t]), the
cost's quadratic expansion, the Riccati backward pass (``lqr_backward``, one launch), ONE closed-loop rollout over
every line-search candidate of every problem (``feedback_rollout``), and a per-problem Armijo choice.  Given a
``HipSim`` the loop runs on the device; given a ``Model`` the same driver runs over the ``_host`` checkers on CPU
tensors, so it can be tested without a GPU.  Every decision is a ``torch.where`` per problem.

With ``u_limits`` the iteration is control-limited (Tassa, Mansard, Todorov, ICRA 2014): the backward pass solves a
box-constrained QP per step and keeps feedback only on the controls it left free (``lqr_backward_box``), and every
rollout clamps its actions, so each nominal trajectory is feasible and the cost is charged for the actions executed.

Out of scope: second-order dynamics terms (DDP), state constraints."""
from . import hip_backend
from . import model as _model


class QuadraticCost:
    """J = sum_t 1/2 (s_t - s_ref)^T Q (s_t - s_ref) + 1/2 (u_t - u_ref)^T R (u_t - u_ref)
         + 1/2 (s_T - s_ref)^T Qf (s_T - s_ref).

    Q, Qf [.., nsd, nsd] and R [.., n_act, n_act] broadcast over problems and time ([nsd, nsd], [T, nsd, nsd] or
    [N, T, nsd, nsd]; Qf [nsd, nsd] or [N, nsd, nsd]); s_ref [.., nsd] broadcasts to [N, T + 1, nsd], u_ref to
    [N, T, n_act] (None: zero).  The weights are used as given (symmetric, R positive definite: the caller's part)."""

    def __init__(self, Q, R, Qf, s_ref=None, u_ref=None):
        import torch

        as64 = lambda a: None if a is None else torch.as_tensor(a, dtype=torch.float64)  # noqa: E731
        self.Q, self.R, self.Qf, self.s_ref, self.u_ref = as64(Q), as64(R), as64(Qf), as64(s_ref), as64(u_ref)

    def _terms(self, s, u):
        import torch

        N, T, nsd, n_act = u.shape[0], u.shape[1], s.shape[2], u.shape[2]
        on = lambda a: a.to(s.device)  # noqa: E731
        Q = on(self.Q).expand(N, T, nsd, nsd)
        Qf = on(self.Qf).expand(N, nsd, nsd)
        R = on(self.R).expand(N, T, n_act, n_act)
        ds = s if self.s_ref is None else s - on(self.s_ref).expand(N, T + 1, nsd)
        du = u if self.u_ref is None else u - on(self.u_ref).expand(N, T, n_act)
        lxx = torch.cat([Q, Qf[:, None]], dim=1)
        lx = torch.matmul(lxx, ds[..., None])[..., 0]
        lu = torch.matmul(R, du[..., None])[..., 0]
        return ds, du, lx, lu, lxx, R

    def value(self, s, u):
        """J [..]: s [.., T + 1, nsd], u [.., T, n_act] with the problems in the FIRST dimension (any dimensions
        between it and the last two are candidates of the same problem)"""
        lead = s.shape[:-2]
        N = lead[0]
        s3, u3 = s.reshape(N, -1, *s.shape[-2:]), u.reshape(N, -1, *u.shape[-2:])
        out = []
        for c in range(s3.shape[1]):
            ds, du, lx, lu, _, _ = self._terms(s3[:, c], u3[:, c])
            out.append(0.5 * ((ds * lx).sum(dim=(1, 2)) + (du * lu).sum(dim=(1, 2))))
        import torch

        return torch.stack(out, dim=1).reshape(lead)

    def expand(self, s, u):
        """(value [N], lx [N, T + 1, nsd], lu [N, T, n_act], lxx [N, T + 1, nsd, nsd], luu [N, T, n_act, n_act],
        lux [N, T, n_act, nsd]) at s [N, T + 1, nsd], u [N, T, n_act]"""
        import torch

        ds, du, lx, lu, lxx, R = self._terms(s, u)
        value = 0.5 * ((ds * lx).sum(dim=(1, 2)) + (du * lu).sum(dim=(1, 2)))
        N, T, n_act, nsd = u.shape[0], u.shape[1], u.shape[2], s.shape[2]
        lux = torch.zeros((N, T, n_act, nsd), dtype=torch.float64, device=s.device)
        return value, lx, lu, lxx.contiguous(), R.contiguous(), lux


class _DeviceOps:
    """the three native calls on a HipSim (CUDA tensors)"""

    def __init__(self, sim):
        self.sim, self.model = sim, sim.model
        self.device = f"cuda:{sim.device}"

    def jacobian(self, x, rows, cols):
        return self.sim.jacobian(x, rows=rows, cols=cols)

    def lqr_backward(self, *a):
        return self.sim.lqr_backward(*a)

    def lqr_backward_box(self, *a):
        return self.sim.lqr_backward_box(*a, check=False)  # (the bounds: lo - u <= 0 <= hi - u of a feasible u)

    def feedback_rollout(self, x0, s_nom, u_nom, k, K, alpha, por, u_lo=None, u_hi=None):
        return self.sim.feedback_rollout(x0, s_nom, u_nom, k, K, alpha, por, check=False,  # (por: built below)
                                         u_lo=u_lo, u_hi=u_hi)


class _HostOps:
    """the same calls over the _host checkers (CPU tensors in and out)"""

    def __init__(self, m):
        self.model, self.device = m, "cpu"

    def jacobian(self, x, rows, cols):
        import torch

        return torch.from_numpy(hip_backend.jacobian_host(self.model, x.numpy(), rows=rows, cols=cols))

    def lqr_backward(self, *a):
        import torch

        return tuple(torch.from_numpy(r) for r in hip_backend.lqr_backward_host(*(t.numpy() for t in a)))

    def lqr_backward_box(self, *a):
        import torch

        return tuple(torch.from_numpy(r) for r in hip_backend.lqr_backward_box_host(*(t.numpy() for t in a)))

    def feedback_rollout(self, x0, s_nom, u_nom, k, K, alpha, por, u_lo=None, u_hi=None):
        import torch

        lim = {} if u_lo is None else {"u_lo": u_lo.numpy(), "u_hi": u_hi.numpy()}
        s, u = hip_backend.feedback_rollout_host(self.model, x0.numpy(), s_nom.numpy(), u_nom.numpy(), k.numpy(),
                                                 K.numpy(), alpha.numpy(), None if por is None else por.numpy(), **lim)
        return torch.from_numpy(s), torch.from_numpy(u)


DEFAULT_ALPHAS = tuple(2.0 ** -i for i in range(8))


def ilqr(sim_or_model, x0, u0, cost, iterations: int = 10, alphas=DEFAULT_ALPHAS, armijo: float = 1e-4,
         mu0=1e-6, mu_min: float = 1e-9, mu_max: float = 1e9, mu_factor: float = 10.0, u_limits=None):
    """iLQR for N problems of horizon T from x0 [N, input_dim] (the first record of each problem: its state, and the
    gains every later record keeps) and the action sequences u0 [N, T, n_act].

    cost: an object with ``expand(s [N, T + 1, nsd], u [N, T, n_act]) -> (value [N], lx, lu, lxx, luu, lux)`` (and,
    optionally, ``value(s [N, C, T + 1, nsd], u [N, C, T, n_act]) -> [N, C]``), e.g. QuadraticCost.  Per iteration and
    problem the largest alpha of ``alphas`` with J_old - J_new >= armijo (-(alpha dV1 + alpha^2 dV2)) is taken and the
    regularisation mu (added to Q_uu's diagonal) divided by mu_factor (not below mu_min); where none qualifies, or
    the backward pass met a Q_uu + mu I that is not positive definite (status != 0), the nominal trajectory is kept
    and mu multiplied by mu_factor (not above mu_max).  The constants are algorithm settings.

    Returns a dict: s [N, T + 1, nsd], u [N, T, n_act], k [N, T, n_act], K [N, T, n_act, nsd] (the last backward
    pass's gains), cost [iterations + 1, N], alpha [iterations, N] (0: rejected), mu [N], status [N] (of the last
    backward pass); and per iteration mu_trace [iterations + 1, N] (the mu each backward pass ran with, then the
    final one), status_trace [iterations, N], dv_trace [iterations, N, 2].  mu0 may be a [N] tensor (a mu per problem).
    Tensors on the handle's device (a HipSim) or the CPU (a Model).

    u_limits: None (no limits: the calls above), a pair (lo, hi) that broadcasts to [N, T, n_act] (+-inf: no limit on
    that side), or "model": -+action_limit of a locomotion model, which clamps its actions inside the step (a torque
    model has no limit of its own: ValueError).  With limits the first open-loop rollout and every candidate's rollout
    clamp their actions to [lo, hi], the backward pass is ``lqr_backward_box`` with the bounds lo - u, hi - u on the
    step, and the result gains clamped [N, T] (int32, bit a: control a clamped in the last pass's QP) and
    qp_iterations [N, T].  The line search, the mu schedule and the traces are the same."""
    import torch

    ops = _HostOps(sim_or_model) if isinstance(sim_or_model, _model.Model) else _DeviceOps(sim_or_model)
    m, dev = ops.model, ops.device
    nsd, n_act, _ = hip_backend.trajectory_dims(m, 1)
    own = lambda a: a if isinstance(a, torch.Tensor) else torch.tensor(a)  # noqa: E731  (a copy of an array)
    x0 = own(x0).to(dev, torch.float64).contiguous()
    u = own(u0).to(dev, torch.float64).contiguous()
    N, T = int(u.shape[0]), int(u.shape[1])
    if tuple(x0.shape) != (N, m.input_dim) or tuple(u.shape) != (N, T, n_act):
        raise ValueError(f"ilqr: expected x0 [N, {m.input_dim}] and u0 [N, T, {n_act}], got {list(x0.shape)} and "
                         f"{list(u.shape)}")
    al = torch.tensor([float(a) for a in alphas], dtype=torch.float64, device=dev)
    C = int(al.shape[0])
    if C < 1 or iterations < 0:
        raise ValueError("ilqr: needs at least one alpha and iterations >= 0")
    lo = hi = None
    if u_limits is not None:
        if isinstance(u_limits, str):
            if u_limits != "model":
                raise ValueError(f'ilqr: u_limits is None, (lo, hi) or "model", got {u_limits!r}')
            if m.step_mode != _model.TDS_STEP_LOCOMOTION:
                raise ValueError('ilqr: u_limits="model" needs a locomotion model (a torque model has no action limit)')
            u_limits = (-float(m.action_limit), float(m.action_limit))
        if len(u_limits) != 2:
            raise ValueError(f'ilqr: u_limits is None, (lo, hi) or "model", got {u_limits!r}')
        try:
            lo, hi = (torch.as_tensor(b, dtype=torch.float64).to(dev).expand(N, T, n_act).contiguous() for b in u_limits)
        except RuntimeError:
            raise ValueError(f"ilqr: u_limits do not broadcast to [N, T, {n_act}] = {[N, T, n_act]}") from None
        if not bool((lo <= hi).all()):
            raise ValueError("ilqr: u_limits: lo > hi somewhere, or a NaN bound")
    rows_sel, cols_sel = list(range(nsd)), list(range(nsd + n_act))
    value_of = getattr(cost, "value", None)
    # the candidates' rows: row p C + c is problem p under alpha[c]
    por = torch.arange(N, dtype=torch.int32, device=dev).repeat_interleave(C)
    alpha_rows = al.repeat(N)
    x0_rows = x0.repeat_interleave(C, dim=0)
    # the nominal trajectory of u0: the open-loop rollout
    zk = torch.zeros((N, T, n_act), dtype=torch.float64, device=dev)
    zK = torch.zeros((N, T, n_act, nsd), dtype=torch.float64, device=dev)
    lim = {} if lo is None else {"u_lo": lo, "u_hi": hi}
    s, u = ops.feedback_rollout(x0, torch.zeros((N, T + 1, nsd), dtype=torch.float64, device=dev), u, zk, zK,
                                torch.zeros(N, dtype=torch.float64, device=dev), None, **lim)
    mu = torch.as_tensor(mu0, dtype=torch.float64).to(dev).expand(N).contiguous()
    costs, taken, mus, stats, dvs = [], [], [mu], [], []
    k, K, status = zk, zK, torch.zeros(N, dtype=torch.int32, device=dev)
    clamped = qp_its = torch.zeros((N, T), dtype=torch.int32, device=dev)
    J = cost.expand(s, u)[0]
    costs.append(J)
    for _ in range(int(iterations)):
        jac = ops.jacobian(hip_backend.trajectory_records(m, x0, s, u), rows_sel, cols_sel)
        jac = jac.reshape(N, T, nsd, nsd + n_act)
        A, B = jac[..., :nsd].contiguous(), jac[..., nsd:].contiguous()
        J, lx, lu, lxx, luu, lux = cost.expand(s, u)
        ex = (A, B, lx.contiguous(), lu.contiguous(), lxx.contiguous(), luu.contiguous(), lux.contiguous(), mu)
        if lo is None:
            k, K, dv, status = ops.lqr_backward(*ex)
        else:
            k, K, dv, status, clamped, qp_its = ops.lqr_backward_box(*ex, lo - u, hi - u)
        sc, uc = ops.feedback_rollout(x0_rows, s, u, k, K, alpha_rows, por, **lim)
        sc, uc = sc.reshape(N, C, T + 1, nsd), uc.reshape(N, C, T, n_act)
        if value_of is not None:
            Jc = value_of(sc, uc)
        else:
            Jc = cost.expand(sc.reshape(N * C, T + 1, nsd), uc.reshape(N * C, T, n_act))[0].reshape(N, C)
        expected = -(al[None, :] * dv[:, :1] + al[None, :] ** 2 * dv[:, 1:])
        ok = torch.isfinite(Jc) & (J[:, None] - Jc >= armijo * expected) & (status == 0)[:, None]
        # the largest qualifying alpha: the first one, where the alphas are given in falling order
        score = torch.where(ok, al[None, :].expand(N, C), torch.full_like(Jc, -1.0))
        best = score.argmax(dim=1)
        accept = ok.any(dim=1)
        pick = best[:, None, None, None]
        s_new = sc.gather(1, pick.expand(N, 1, T + 1, nsd))[:, 0]
        u_new = uc.gather(1, pick.expand(N, 1, T, n_act))[:, 0]
        s = torch.where(accept[:, None, None], s_new, s)
        u = torch.where(accept[:, None, None], u_new, u)
        J = torch.where(accept, Jc.gather(1, best[:, None])[:, 0], J)
        mu = torch.where(accept, torch.clamp(mu / mu_factor, min=mu_min), torch.clamp(mu * mu_factor, max=mu_max))
        taken.append(torch.where(accept, al[best], torch.zeros_like(J)))
        costs.append(J)
        mus.append(mu)
        stats.append(status)
        dvs.append(dv)
    hist = lambda a, shape, dt: torch.stack(a) if a else torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
    res = {"s": s, "u": u, "k": k, "K": K, "cost": torch.stack(costs),
           "alpha": hist(taken, (0, N), torch.float64), "mu": mu, "status": status,
           "mu_trace": torch.stack(mus), "status_trace": hist(stats, (0, N), torch.int32),
           "dv_trace": hist(dvs, (0, N, 2), torch.float64)}
    if lo is not None:
        res.update({"clamped": clamped, "qp_iterations": qp_its})
    return res
