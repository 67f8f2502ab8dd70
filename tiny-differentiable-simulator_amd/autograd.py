"""torch.autograd through one step: ``step_fn(sim)(x)`` is forward_zero of a HipSim, differentiable in x.

The forward pass is the step kernels' forward_zero.  Where ``x.requires_grad``, it also computes the step Jacobian J
[N, output_dim, input_dim] with the forward-mode kernel (HipSim.jacobian), and the backward pass returns J^T grad_y
by bmm.  With ``step_fn(sim, mode="reverse")`` the forward pass keeps only x, and the backward pass returns
grad_y^T J from the reverse-mode kernel (HipSim.vjp): no Jacobian is formed.  The derivative is that of the algorithm
as executed (clamps, PGS projections and contact activation follow the branch the primal takes; quaternion entries
differentiated raw): see DESIGN.md, "Step Jacobians".

``param_step_fn(sim, params)(x, theta)`` is the step at the model parameters theta (the selection ``params``,
hip_backend.param_spec), differentiable in x and theta: see DESIGN.md, "Parameter derivatives".

``rb_rollout_fn(sim, steps, wrt, params)(s0, u, theta)`` is a rollout of a rigid-body world (RigidBodySim), differentiable
in the state entries ``wrt`` (overwritten by u) and the parameters theta: see DESIGN.md, "Rigid-body rollouts".

``trajectory_fn(sim, steps, wrt, params, every)(x0, z, theta, u)`` is an articulated-body trajectory (forward_zero
chained), differentiable in the record entries ``wrt`` (overwritten by z) and the parameters theta: see DESIGN.md,
"Articulated trajectories".

``contact_fn(sim, want, params)(x, theta)`` is the contact query (impulses, forces, ...), differentiable in x and theta:
see DESIGN.md, "Derivatives of the contact query".

``dynamics_fn(sim, want, params)(q, qd, tau, theta)`` and ``inverse_dynamics_fn(sim, params)(q, qd, qdd, theta)`` are the
batched dynamics queries (qdd, the mass matrix, ...; tau = ID), differentiable in every argument: see DESIGN.md,
"Derivatives of the dynamics queries"."""

_StepFunction = None
_StepFunctionReverse = None
_ParamStepFunction = None
_RbRolloutFunction = None
_RbRolloutReverseFunction = None
_TrajectoryFunction = None
_TrajectoryReverseFunction = None
_ContactFunction = None
_DynamicsFunction = None


def _function():
    """the autograd.Function, built on first use (the package itself does not import torch)"""
    global _StepFunction
    if _StepFunction is None:
        import torch

        class StepFunction(torch.autograd.Function):
            @staticmethod
            def forward(ctx, x, sim):
                xd = x.detach().contiguous()
                y = sim.forward_zero(xd)
                if ctx.needs_input_grad[0]:
                    ctx.save_for_backward(sim.jacobian(xd))
                return y

            @staticmethod
            def backward(ctx, grad_y):
                (jac,) = ctx.saved_tensors
                grad_x = torch.bmm(jac.transpose(1, 2), grad_y.to(jac.dtype).unsqueeze(2)).squeeze(2)
                return grad_x, None

        _StepFunction = StepFunction
    return _StepFunction


def _function_reverse():
    """the reverse-mode autograd.Function, built on first use"""
    global _StepFunctionReverse
    if _StepFunctionReverse is None:
        import torch
        from torch.autograd.function import once_differentiable

        class StepFunctionReverse(torch.autograd.Function):
            @staticmethod
            def forward(ctx, x, sim):
                xd = x.detach().contiguous()
                y = sim.forward_zero(xd)
                ctx.sim = sim
                if ctx.needs_input_grad[0]:
                    ctx.save_for_backward(xd)
                return y

            @staticmethod
            @once_differentiable
            def backward(ctx, grad_y):
                (xd,) = ctx.saved_tensors
                _, grad_x = ctx.sim.vjp(xd, grad_y.to(xd.dtype).contiguous())
                return grad_x, None

        _StepFunctionReverse = StepFunctionReverse
    return _StepFunctionReverse


def step_fn(sim, mode: str = "forward"):
    """x [num_envs, input_dim] (float64, on the sim's device) -> y = forward_zero(x), differentiable in x.

    mode "forward": the forward pass computes the dense Jacobian where x requires grad, backward is J^T grad_y.
    mode "reverse": the forward pass saves x, backward is one VJP per call (HipSim.vjp)."""
    if mode == "forward":
        fn = _function()
    elif mode == "reverse":
        fn = _function_reverse()
    else:
        raise ValueError(f"step_fn: mode must be 'forward' or 'reverse', not {mode!r}")

    def f(x):
        return fn.apply(x, sim)

    return f


def _param_function():
    """the autograd.Function of param_step_fn, built on first use"""
    global _ParamStepFunction
    if _ParamStepFunction is None:
        import torch
        from torch.autograd.function import once_differentiable

        class ParamStepFunction(torch.autograd.Function):
            @staticmethod
            def forward(ctx, x, theta, sim, params, mode):
                xd, th = x.detach().contiguous(), theta.detach().contiguous()
                n, nin, p = xd.shape[0], sim.input_dim, len(params)
                ctx.sim, ctx.params, ctx.mode, ctx.shared = sim, params, mode, th.dim() == 1
                if not (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]):
                    return sim.jvp_params(xd, th, params)
                if mode == "forward":  # J^T [N, input_dim + p, output_dim] from one unit direction per input
                    eye = torch.eye(nin + p, dtype=torch.float64, device=xd.device)
                    y, jt = sim.jvp_params(xd, th, params, eye.expand(n, nin + p, nin + p).contiguous())
                    ctx.save_for_backward(jt)
                else:
                    y = sim.jvp_params(xd, th, params)
                    ctx.save_for_backward(xd, th)
                return y

            @staticmethod
            @once_differentiable
            def backward(ctx, grad_y):
                nin = ctx.sim.input_dim
                if ctx.mode == "forward":
                    (jt,) = ctx.saved_tensors
                    g = torch.bmm(jt, grad_y.to(jt.dtype).unsqueeze(2)).squeeze(2)
                    gx, gth = g[:, :nin], g[:, nin:]
                else:
                    xd, th = ctx.saved_tensors
                    _, gx, gth = ctx.sim.vjp_params(xd, th, ctx.params, grad_y.to(xd.dtype).contiguous())
                if ctx.shared:  # one theta for every environment: its gradient sums over them
                    gth = gth.sum(0)
                return gx, gth, None, None, None

        _ParamStepFunction = ParamStepFunction
    return _ParamStepFunction


def param_step_fn(sim, params, mode: str = "reverse"):
    """(x, theta) -> y: the step of x [num_envs, input_dim] at the model parameters theta, differentiable in both.

    params: the selection (tuples such as ("mass", 3), ("com", 3, 2), ("xt_trans", 1, 2), ("friction",), or
    tds_param_t; hip_backend.param_spec).  theta: [p], shared by every environment (its gradient is summed over
    them), or [N, p].  The forward pass computes y at theta with the parameter kernel (HipSim.jvp_params).
    mode "reverse": backward is one VJP per call (HipSim.vjp_params).  mode "forward": where an input requires grad,
    the forward pass forms J over [x | theta] (input_dim + p directions) and backward is J^T grad_y."""
    from . import hip_backend

    if mode not in ("forward", "reverse"):
        raise ValueError(f"param_step_fn: mode must be 'forward' or 'reverse', not {mode!r}")
    sel = hip_backend.param_spec(params)
    p = len(params)
    fn = _param_function()
    spec = [sel[j] for j in range(p)]  # checked tds_param_t entries (param_spec passes them through)

    def f(x, theta):
        return fn.apply(x, theta, sim, spec, mode)

    return f


def _rb_rollout_function():
    global _RbRolloutFunction
    if _RbRolloutFunction is None:
        import torch
        from torch.autograd.function import once_differentiable

        class RbRolloutFunction(torch.autograd.Function):
            @staticmethod
            def forward(ctx, u, theta, s0, sim, steps, idx, dirs, params):
                n, nb = s0.shape[0], sim.model.num_bodies
                s = s0.detach().reshape(n, -1).clone()
                s[:, idx] = u.detach().to(s.dtype)
                s = s.reshape(n, nb, -1)
                th = None if theta is None else theta.detach()
                ctx.shared = th is not None and th.dim() == 1
                ctx.has_theta = th is not None
                if not any(ctx.needs_input_grad[:2]):
                    return sim.jvp(s, None, steps, params, th)[0]
                # only the len(wrt) + p columns that are needed: J [N, nb * 13, len(wrt) + p]
                sT, jv = sim.jvp(s, dirs.expand(n, -1, -1), steps, params, th)
                ctx.save_for_backward(jv.reshape(n, dirs.shape[0], -1))
                ctx.nu = len(idx)
                return sT

            @staticmethod
            @once_differentiable
            def backward(ctx, grad_sT):
                (jt,) = ctx.saved_tensors  # [N, len(wrt) + p, nb * 13] = J^T
                n = jt.shape[0]
                g = torch.bmm(jt, grad_sT.reshape(n, -1, 1).to(jt.dtype)).squeeze(2)
                gu, gth = g[:, :ctx.nu], g[:, ctx.nu:]
                if ctx.shared:
                    gth = gth.sum(0)
                return gu, (gth if ctx.has_theta else None), None, None, None, None, None, None

        _RbRolloutFunction = RbRolloutFunction
    return _RbRolloutFunction


def _rb_rollout_reverse_function():
    global _RbRolloutReverseFunction
    if _RbRolloutReverseFunction is None:
        import torch
        from torch.autograd.function import once_differentiable

        class RbRolloutReverseFunction(torch.autograd.Function):
            @staticmethod
            def forward(ctx, u, theta, s0, sim, steps, every, idx, params):
                n, nb = s0.shape[0], sim.model.num_bodies
                s = s0.detach().reshape(n, -1).clone()
                s[:, idx] = u.detach().to(s.dtype)
                s = s.reshape(n, nb, -1)
                th = None if theta is None else theta.detach()
                ctx.shared = th is not None and th.dim() == 1
                ctx.has_theta = th is not None
                ctx.sim, ctx.steps, ctx.every, ctx.idx, ctx.params = sim, steps, every, idx, params
                ctx.save_for_backward(*(t for t in (s, th) if t is not None))
                if every is None:
                    return sim.jvp(s, None, steps, params, th)[0]
                # the records: the primal kernel chained, `every` steps per launch (the same steps, bit for bit)
                out, cur = [], s
                for _ in range(steps // every):
                    cur = sim.jvp(cur, None, every, params, th)[0]
                    out.append(cur)
                return torch.stack(out, 1)

            @staticmethod
            @once_differentiable
            def backward(ctx, grad_s):
                saved = list(ctx.saved_tensors)
                s = saved.pop(0)
                th = saved.pop(0) if ctx.has_theta else None
                _, gs0, gth = ctx.sim.vjp(s, grad_s.to(s.dtype).contiguous(), ctx.steps, ctx.params, th, ctx.every)
                n = s.shape[0]
                if ctx.shared:  # one theta for every world: its gradient sums over them
                    gth = gth.sum(0)
                gu = gs0.reshape(n, -1)[:, ctx.idx]
                # the entries wrt were overwritten by u: s0's own gradient is zero there
                g0 = gs0.reshape(n, -1).clone()
                g0[:, ctx.idx] = 0.0
                return gu, (gth if ctx.has_theta else None), g0.reshape(gs0.shape), None, None, None, None, None

        _RbRolloutReverseFunction = RbRolloutReverseFunction
    return _RbRolloutReverseFunction


def rb_rollout_fn(sim, steps: int, wrt, params=(), mode: str = "forward", every=None):
    """(s0, u, theta=None) -> s_T: `steps` World::steps of a RigidBodySim (f64) from s0 [N, num_bodies, 13] with the
    state entries wrt (a list of (body, comp), comp 0..12 of position | quaternion xyzw | linear | angular velocity)
    overwritten by u [N, len(wrt)], differentiable in u and theta.

    params: a selection of ("mass", body), ("gravity", comp), ("friction",), ("restitution",) (hip_backend.param_spec);
    theta: None (the model's values), [p] shared by every world (its gradient is summed over them) or [N, p].  Where u
    or theta requires grad, the forward pass computes the len(wrt) + p needed columns of d s_T / d [u | theta] with
    RigidBodySim.jvp and backward is J^T grad.  s0 itself is not differentiated: s0.requires_grad raises.

    mode "reverse": the forward pass keeps only its inputs and backward is one RigidBodySim.vjp, whatever the number of
    inputs: differentiable in u, in theta and in s0 itself (its entries wrt excepted: u overwrites them).  With `every`
    given (reverse mode only) the result is the states after every, 2 every, .., steps steps, [N, n_rec, num_bodies, 13],
    so that a loss may read intermediate states of the roll."""
    from . import hip_backend

    if mode not in ("forward", "reverse"):
        raise ValueError(f"rb_rollout_fn: mode must be 'forward' or 'reverse', not {mode!r}")
    if every is not None and mode != "reverse":
        raise ValueError("rb_rollout_fn: every needs mode='reverse' (forward mode returns the final state alone)")
    if every is not None and (int(every) < 1 or int(steps) % int(every)):
        raise ValueError(f"rb_rollout_fn: every ({every}) must divide steps ({steps})")
    nb = sim.model.num_bodies
    p = len(params)
    sel = hip_backend.param_spec(params)
    spec = [sel[j] for j in range(p)]
    idx = [b * 13 + c for b, c in wrt]
    fn = _rb_rollout_function()
    cache = {}

    def check(u, theta):
        if u.dim() != 2 or u.shape[1] != len(idx):
            raise ValueError(f"rb_rollout_fn: u must be [N, {len(idx)}], got {tuple(u.shape)}")
        if theta is not None and p == 0:
            raise ValueError("rb_rollout_fn: theta given but no params selected")

    if mode == "reverse":
        rev = _rb_rollout_reverse_function()

        def fr(s0, u, theta=None):
            import torch

            check(u, theta)
            ix = torch.tensor(idx, dtype=torch.long, device=s0.device)
            return rev.apply(u, theta, s0, sim, int(steps), None if every is None else int(every), ix, spec)

        return fr

    def f(s0, u, theta=None):
        import torch

        if s0.requires_grad:
            raise ValueError("rb_rollout_fn: s0 is not differentiated (only the entries wrt, through u): detach s0 "
                             "or list the entries in wrt")
        check(u, theta)
        key = str(s0.device)
        if key not in cache:
            cache[key] = hip_backend.rb_directions(nb, wrt, p, device=s0.device)
        ix = torch.tensor(idx, dtype=torch.long, device=s0.device)
        return fn.apply(u, theta, s0, sim, int(steps), ix, cache[key], spec)

    return f


def _trajectory_function():
    global _TrajectoryFunction
    if _TrajectoryFunction is None:
        import torch
        from torch.autograd.function import once_differentiable

        class TrajectoryFunction(torch.autograd.Function):
            @staticmethod
            def forward(ctx, z, theta, x0, u, sim, steps, every, idx, dirs, params):
                x = x0.detach().clone()
                if z is not None:
                    x[:, idx] = z.detach().to(x.dtype)
                th = None if theta is None else theta.detach()
                ud = None if u is None else u.detach()
                ctx.shared = th is not None and th.dim() == 1
                ctx.has_z, ctx.has_theta = z is not None, th is not None
                if not any(ctx.needs_input_grad[:2]):
                    return sim.trajectory_jvp(x, None, steps, every, ud, params, th)[0]
                # only the len(wrt) + p columns that are needed: J^T [N, len(wrt) + p, n_rec (nq + nd)]
                n = x.shape[0]
                s, js = sim.trajectory_jvp(x, dirs.expand(n, -1, -1), steps, every, ud, params, th)
                ctx.save_for_backward(js.reshape(n, dirs.shape[0], -1))
                ctx.nz = len(idx)
                return s

            @staticmethod
            @once_differentiable
            def backward(ctx, grad_s):
                (jt,) = ctx.saved_tensors
                n = jt.shape[0]
                g = torch.bmm(jt, grad_s.reshape(n, -1, 1).to(jt.dtype)).squeeze(2)
                gz, gth = g[:, :ctx.nz], g[:, ctx.nz:]
                if ctx.shared:  # one theta for every environment: its gradient sums over them
                    gth = gth.sum(0)
                return ((gz if ctx.has_z else None), (gth if ctx.has_theta else None)) + (None,) * 8

        _TrajectoryFunction = TrajectoryFunction
    return _TrajectoryFunction


def _trajectory_reverse_function():
    global _TrajectoryReverseFunction
    if _TrajectoryReverseFunction is None:
        import torch
        from torch.autograd.function import once_differentiable

        class TrajectoryReverseFunction(torch.autograd.Function):
            @staticmethod
            def forward(ctx, z, theta, u, x0, sim, steps, every, idx, params):
                x = x0.detach().clone()
                if z is not None:
                    x[:, idx] = z.detach().to(x.dtype)
                th = None if theta is None else theta.detach()
                ud = None if u is None else u.detach()
                ctx.shared = th is not None and th.dim() == 1
                ctx.has = (z is not None, th is not None, ud is not None)
                ctx.sim, ctx.steps, ctx.every, ctx.idx, ctx.params = sim, steps, every, idx, params
                ctx.save_for_backward(*(t for t in (x, th, ud) if t is not None))
                return sim.trajectory_jvp(x, None, steps, every, ud, params, th)[0]

            @staticmethod
            @once_differentiable
            def backward(ctx, grad_s):
                saved = list(ctx.saved_tensors)
                x = saved.pop(0)
                th = saved.pop(0) if ctx.has[1] else None
                ud = saved.pop(0) if ctx.has[2] else None
                _, gx0, gu, gth = ctx.sim.trajectory_vjp(x, grad_s.to(x.dtype).contiguous(), ctx.steps, ctx.every, ud,
                                                         ctx.params, th)
                if ctx.shared:  # one theta for every environment: its gradient sums over them
                    gth = gth.sum(0)
                return ((gx0[:, ctx.idx] if ctx.has[0] else None), (gth if ctx.has[1] else None),
                        (gu if ctx.has[2] else None)) + (None,) * 6

        _TrajectoryReverseFunction = TrajectoryReverseFunction
    return _TrajectoryReverseFunction


def trajectory_fn(sim, steps: int, wrt=(), params=(), every: int = 1, mode: str = "forward"):
    """(x0, z=None, theta=None, u=None) -> s [N, n_rec, nq + nd]: the states after steps every, 2 every, .., steps of
    forward_zero chained from x0 [N, input_dim] (a HipSim, f64), with x0's entries wrt (indices into its input_dim
    entries) overwritten by z [N, len(wrt)], differentiable in z and theta.

    params: the selection (hip_backend.param_spec); theta: None (the model's values), [p] shared by every environment
    (its gradient is summed over them) or [N, p].  u: None (x0's actions every step) or [N, steps - 1, n_act], the
    actions of steps 1 .. (HipSim.trajectory_jvp).  Where z or theta requires grad, the forward pass computes the
    len(wrt) + p needed columns of d s / d [z | theta] in forward mode and backward is J^T grad.  x0 and u are not
    differentiated: x0.requires_grad and u.requires_grad raise.

    mode "reverse": the forward pass is the primal alone and backward is one HipSim.trajectory_vjp, differentiable in
    z, theta and the actions u (trajectory optimisation, policy gradients through the rollout); x0.requires_grad still
    raises."""
    from . import hip_backend

    if mode not in ("forward", "reverse"):
        raise ValueError(f"trajectory_fn: mode must be 'forward' or 'reverse', not {mode!r}")
    p = len(params)
    sel = hip_backend.param_spec(params)
    spec = [sel[j] for j in range(p)]
    idx = [int(i) for i in wrt]
    fn = _trajectory_function()
    cache = {}

    def f(x0, z=None, theta=None, u=None):
        import torch

        if x0.requires_grad:
            raise ValueError("trajectory_fn: x0 is not differentiated: list the entries to differentiate in wrt and "
                             "pass them as z")
        if mode == "forward" and u is not None and u.requires_grad:
            raise ValueError("trajectory_fn: the actions u are not differentiated: for gradients in an action sequence "
                             "chain step_fn(sim, mode='reverse')")
        if z is None and idx:
            z = x0[:, idx]
        if z is not None and (z.dim() != 2 or z.shape[1] != len(idx)):
            raise ValueError(f"trajectory_fn: z must be [N, {len(idx)}], got {tuple(z.shape)}")
        if theta is not None and p == 0:
            raise ValueError("trajectory_fn: theta given but no params selected")
        ix = torch.tensor(idx, dtype=torch.long, device=x0.device)
        if mode == "reverse":
            return _trajectory_reverse_function().apply(z, theta, u, x0, sim, int(steps), int(every), ix, spec)
        key = str(x0.device)
        if key not in cache:
            cache[key] = hip_backend.trajectory_directions(sim.input_dim, idx, p, device=x0.device)
        return fn.apply(z, theta, x0, u, sim, int(steps), int(every), ix, cache[key], spec)

    return f


_PolicyTrajectoryFunction = None


def _policy_trajectory_function():
    global _PolicyTrajectoryFunction
    if _PolicyTrajectoryFunction is None:
        import torch
        from torch.autograd.function import once_differentiable

        class PolicyTrajectoryFunction(torch.autograd.Function):
            @staticmethod
            def forward(ctx, x0, policy, theta, sim, steps, every, net, params, obs_raw):
                x = x0.detach()
                pol = policy.detach()
                th = None if theta is None else theta.detach()
                ctx.shared_policy = pol.dim() == 1
                ctx.shared_theta = th is not None and th.dim() == 1
                ctx.has_theta = th is not None
                ctx.sim, ctx.steps, ctx.every, ctx.net, ctx.params, ctx.obs_raw = sim, steps, every, net, params, obs_raw
                ctx.save_for_backward(*(t for t in (x, pol, th) if t is not None))
                return sim.policy_trajectory(x, pol, steps, every, *net, params=params, theta=th, obs_raw=obs_raw)

            @staticmethod
            @once_differentiable
            def backward(ctx, grad_s, grad_u):
                saved = list(ctx.saved_tensors)
                x, pol = saved[0], saved[1]
                th = saved[2] if ctx.has_theta else None
                gs = None if grad_s is None else grad_s.to(x.dtype).contiguous()
                ga = None if grad_u is None else grad_u.to(x.dtype).contiguous()
                if gs is None and ga is None:
                    return (None,) * 9
                _, _, gpol, gx0, gth = ctx.sim.policy_trajectory_vjp(
                    x, pol, gs, ctx.steps, ctx.every, ga, *ctx.net, params=ctx.params, theta=th, obs_raw=ctx.obs_raw)
                if ctx.shared_policy:  # one policy for every environment: its gradient sums over them
                    gpol = gpol.sum(0)
                if ctx.shared_theta:
                    gth = gth.sum(0)
                return (gx0, gpol, (gth if ctx.has_theta else None)) + (None,) * 6

        _PolicyTrajectoryFunction = PolicyTrajectoryFunction
    return _PolicyTrajectoryFunction


def policy_trajectory_fn(sim, steps: int, layer_sizes=None, activations=None, use_bias=None, params=(), every: int = 1,
                         obs_raw: bool = False):
    """(x0, policy, theta=None) -> (s, u): the closed-loop trajectory u_t = pi(obs_t) of HipSim.policy_trajectory (a
    HipSim, f64): the states s [N, n_rec, nq + nd] after steps every, 2 every, .., steps and the actions taken u
    [N, steps, n_act], differentiable in policy, theta and x0 through the dynamics and the policy network in one
    HipSim.policy_trajectory_vjp per backward pass.  Losses and rewards are the caller's torch code on s and u.

    policy [P] shared by every environment (its gradient is summed over them) or [N, P]; the network as for
    hip_backend.policy_network_spec (layer_sizes None: the linear policy); params and theta as for trajectory_fn.  x0's
    action slots are not read and get a zero gradient; its gain slots get theirs."""
    from . import hip_backend

    p = len(params)
    sel = hip_backend.param_spec(params)
    spec = [sel[j] for j in range(p)]
    net = (layer_sizes, activations, use_bias)

    def f(x0, policy, theta=None):
        if theta is not None and p == 0:
            raise ValueError("policy_trajectory_fn: theta given but no params selected")
        return _policy_trajectory_function().apply(x0, policy, theta, sim, int(steps), int(every), net, spec,
                                                   bool(obs_raw))

    return f


def _contact_function():
    """the autograd.Function of contact_fn, built on first use"""
    global _ContactFunction
    if _ContactFunction is None:
        import torch
        from torch.autograd.function import once_differentiable

        class ContactFunction(torch.autograd.Function):
            @staticmethod
            def forward(ctx, x, theta, sim, want, params):
                xd = x.detach().contiguous()
                th = None if theta is None else theta.detach().contiguous()
                n, nin, p = xd.shape[0], sim.input_dim, len(params)
                need_x, need_th = ctx.needs_input_grad[0], theta is not None and ctx.needs_input_grad[1]
                ctx.need, ctx.shared, ctx.nin = (need_x, need_th), th is not None and th.dim() == 1, nin
                if not (need_x or need_th):
                    res = sim.contacts_jvp(xd, None, want=want, params=params, theta=th)
                    return tuple(res[k] for k in want)
                # one unit direction per input that requires grad: the columns of J over [x | theta]
                cols = list(range(nin) if need_x else ()) + list(range(nin, nin + p) if need_th else ())
                v = torch.zeros((n, len(cols), nin + p), dtype=torch.float64, device=xd.device)
                v[:, torch.arange(len(cols)), torch.tensor(cols)] = 1.0
                tan, res = sim.contacts_jvp(xd, v, want=want, params=params, theta=th, want_primal=True)
                ctx.save_for_backward(*[tan[k].reshape(n, len(cols), -1) for k in want])  # J^T per output
                return tuple(res[k] for k in want)

            @staticmethod
            @once_differentiable
            def backward(ctx, *grads):
                g = None
                for jt, gy in zip(ctx.saved_tensors, grads):
                    if gy is None:
                        continue
                    t = torch.bmm(jt, gy.to(jt.dtype).reshape(jt.shape[0], -1, 1)).squeeze(2)
                    g = t if g is None else g + t
                need_x, need_th = ctx.need
                gx = g[:, :ctx.nin] if need_x and g is not None else None
                gth = g[:, (ctx.nin if need_x else 0):] if need_th and g is not None else None
                if gth is not None and ctx.shared:  # one theta for every environment: its gradient sums over them
                    gth = gth.sum(0)
                return gx, gth, None, None, None

        _ContactFunction = ContactFunction
    return _ContactFunction


def contact_fn(sim, want=("force",), params=()):
    """(x, theta=None) -> the contact query's outputs `want` (hip_backend.CONTACT_OUTPUTS; a tensor for one name, a
    tuple for several) at the records x [N, input_dim] and the model parameters theta, differentiable in both.

    params: the selection (hip_backend.param_spec, the contact kinds ("cfm",), ("erp",), ("geom_radius", g), ...
    included).  theta: [p], shared by every environment (its gradient is summed over them), or [N, p]; None: the
    model's values.  Forward mode, as step_fn / param_step_fn(mode="forward"): where an input requires grad the forward
    pass forms the needed columns of J over [x | theta] with HipSim.contacts_jvp and backward is J^T grad by bmm, so a
    forward pass that is differentiated costs ceil((input_dim + p) / K) blocks of K = contacts_jvp_tangents(model)
    directions per environment (input_dim or p of them where only x or only theta requires grad) and one backward
    costs no further launch.  Reverse mode is not built for the query."""
    from . import hip_backend

    names = hip_backend._contact_want(want)
    sel = hip_backend.param_spec(params)
    spec = [sel[j] for j in range(len(params))]
    fn = _contact_function()

    def f(x, theta=None):
        out = fn.apply(x, theta, sim, names, spec)
        return out[0] if len(names) == 1 else out

    return f


def _dynamics_function():
    """the autograd.Function of dynamics_fn and inverse_dynamics_fn, built on first use"""
    global _DynamicsFunction
    if _DynamicsFunction is None:
        import torch
        from torch.autograd.function import once_differentiable

        class DynamicsFunction(torch.autograd.Function):
            @staticmethod
            def forward(ctx, q, qd, u, theta, sim, want, params, inverse):
                from . import hip_backend

                det = lambda t: None if t is None else t.detach().contiguous()  # noqa: E731
                qv, qdv, uv, th = det(q), det(qd), det(u), det(theta)
                m, n, p = sim.model, q.shape[0], len(params)
                widths = (m.dof_q, m.dof_qd, m.dof_qd if inverse else hip_backend.dyn_tau_dim(m), p)
                need = tuple(t is not None and ctx.needs_input_grad[i] for i, t in enumerate((q, qd, u, theta)))
                ctx.need, ctx.widths, ctx.shared = need, widths, th is not None and th.dim() == 1

                def call(v):
                    if inverse:
                        r = sim.inverse_dynamics_jvp(qv, qdv, uv, v, params=params, theta=th, want_primal=True)
                        return r if v is None else ({"tau": r[0]}, {"tau": r[1]})
                    return sim.dynamics_jvp(qv, qdv, uv, v, want=want, params=params, theta=th, want_primal=True)

                if not any(need):
                    res = call(None)
                    return (res,) if inverse else tuple(res[k] for k in want)
                # one unit direction per input that requires grad: the columns of J over [q | qd | u | theta]
                starts = [sum(widths[:i]) for i in range(4)]
                cols = [c for i in range(4) if need[i] for c in range(starts[i], starts[i] + widths[i])]
                v = torch.zeros((n, len(cols), sum(widths)), dtype=torch.float64, device=qv.device)
                v[:, torch.arange(len(cols)), torch.tensor(cols)] = 1.0
                tan, res = call(v)
                ctx.save_for_backward(*[tan[k].reshape(n, len(cols), -1) for k in want])  # J^T per output
                return tuple(res[k] for k in want)

            @staticmethod
            @once_differentiable
            def backward(ctx, *grads):
                g = None
                for jt, gy in zip(ctx.saved_tensors, grads):
                    if gy is None:
                        continue
                    t = torch.bmm(jt, gy.to(jt.dtype).reshape(jt.shape[0], -1, 1)).squeeze(2)
                    g = t if g is None else g + t
                out, o = [], 0
                for need, width in zip(ctx.need, ctx.widths):
                    out.append(g[:, o:o + width] if need and g is not None else None)
                    o += width if need else 0
                if out[3] is not None and ctx.shared:  # one theta for every environment: its gradient sums over them
                    out[3] = out[3].sum(0)
                return (*out, None, None, None, None)

        _DynamicsFunction = DynamicsFunction
    return _DynamicsFunction


def _dynamics_fn(sim, names, params, inverse):
    from . import hip_backend

    sel = hip_backend.param_spec(params)
    spec = [sel[j] for j in range(len(params))]
    fn = _dynamics_function()

    def f(q, qd, u, theta):
        if theta is not None and not spec:
            raise ValueError("dynamics_fn: theta given but no params selected")
        out = fn.apply(q, qd, u, theta, sim, names, spec, inverse)
        return out[0] if len(names) == 1 else out

    return f


def dynamics_fn(sim, want=("qdd",), params=()):
    """(q, qd=None, tau=None, theta=None) -> the dynamics queries' outputs `want` (hip_backend.DYN_OUTPUTS; a tensor for
    one name, a tuple for several) at the states q [N, dof_q], qd [N, dof_qd], the torques tau [N, dyn_tau_dim(model)]
    (None: zero) and the model parameters theta, differentiable in all four.

    params: the selection (hip_backend.param_spec).  theta: [p], shared by every environment (its gradient is summed
    over them), or [N, p]; None: the model's values.  Forward mode, as contact_fn: where an input requires grad the
    forward pass forms the needed columns of J over [q | qd | tau | theta] with HipSim.dynamics_jvp and backward is
    J^T grad by bmm, so a forward pass that is differentiated costs ceil(columns / K) blocks of
    K = dynamics_jvp_tangents(model) directions per environment and one backward costs no further launch.  Reverse mode
    is not built for the queries."""
    from . import hip_backend

    g = _dynamics_fn(sim, hip_backend._dyn_want(want), params, False)

    def f(q, qd=None, tau=None, theta=None):
        return g(q, qd, tau, theta)

    return f


def inverse_dynamics_fn(sim, params=()):
    """(q, qd=None, qdd=None, theta=None) -> tau [N, dof_qd] = ID(q, qd, qdd) (HipSim.inverse_dynamics; fixed base only)
    at the model parameters theta, differentiable in all four; params, theta and the cost as for dynamics_fn, through
    HipSim.inverse_dynamics_jvp."""
    g = _dynamics_fn(sim, ("tau",), params, True)

    def f(q, qd=None, qdd=None, theta=None):
        return g(q, qd, qdd, theta)

    return f
