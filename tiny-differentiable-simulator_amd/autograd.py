"""torch.autograd through one step: ``step_fn(sim)(x)`` is forward_zero of a HipSim, differentiable in x.

The forward pass is the step kernels' forward_zero.  Where ``x.requires_grad``, it also computes the step Jacobian J
[N, output_dim, input_dim] with the forward-mode kernel (HipSim.jacobian), and the backward pass returns J^T grad_y
by bmm.  With ``step_fn(sim, mode="reverse")`` the forward pass keeps only x, and the backward pass returns
grad_y^T J from the reverse-mode kernel (HipSim.vjp): no Jacobian is formed.  The derivative is that of the algorithm
as executed (clamps, PGS projections and contact activation follow the branch the primal takes; quaternion entries
differentiated raw): see DESIGN.md, "Step Jacobians"."""

_StepFunction = None
_StepFunctionReverse = None


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
