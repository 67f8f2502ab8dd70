"""torch.autograd through one step: ``step_fn(sim)(x)`` is forward_zero of a HipSim, differentiable in x.

The forward pass is the step kernels' forward_zero.  Where ``x.requires_grad``, it also computes the step Jacobian J
[N, output_dim, input_dim] with the forward-mode kernel (HipSim.jacobian), and the backward pass returns J^T grad_y
by bmm.  The derivative is that of the algorithm as executed (clamps, PGS projections and contact activation follow
the branch the primal takes; quaternion entries differentiated raw): see DESIGN.md, "Step Jacobians"."""

_StepFunction = None


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


def step_fn(sim):
    """x [num_envs, input_dim] (float64, on the sim's device) -> y = forward_zero(x), differentiable in x"""
    fn = _function()

    def f(x):
        return fn.apply(x, sim)

    return f
