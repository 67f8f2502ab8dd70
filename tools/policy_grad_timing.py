"""Times the closed-loop policy gradient (HipSim.policy_trajectory_vjp) on the Ant over T = 100 steps, n = 256 and 4096,
for the linear policy and an [obs, 64, 64, act] tanh network, against
  (b) HipSim.trajectory_vjp, open loop on the action sequence that (a) returns: the same physics without the policy
      kernels and with the sweeps of a window in one launch (the floor), and
  (c) the chain a user writes without the fused call: param_step_fn(mode="reverse") plus a float64 torch module per step.
The loss is <w, s> + <wu, u>; the gradients are in the policy's parameters and in p = 2 model parameters (gravity z,
friction).  One process, device-synchronised wall clock, one warm-up of every variant first, then three rounds that
alternate between the variants, medians.  Run it under `rocprofv3 --kernel-trace --stats -- python
tools/policy_grad_timing.py` for the kernel times (the gradients' equality is checked by
tests/test_policy_grad_gpu.py)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402

import tds_amd  # noqa: E402
from tds_amd import hip_backend as hb  # noqa: E402

TANH = 0


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def draw(ls, n, rng, scale=0.1):
    """[n, P] parameters of the network ls, biases on every layer but the input: weights scale / sqrt(fan_in)"""
    w = [scale * rng.normal(size=(n, ls[i - 1] * ls[i])) / np.sqrt(ls[i - 1]) for i in range(1, len(ls))]
    b = [scale * rng.normal(size=(n, ls[i])) for i in range(1, len(ls))]
    return np.concatenate(w + b, axis=1)


def torch_policy(ls, tanh, pol, obs):
    o = torch.cat([torch.zeros_like(obs[:, :2]), obs[:, 2:]], dim=1)
    wo = 0
    bo = sum(ls[i - 1] * ls[i] for i in range(1, len(ls)))
    for i in range(1, len(ls)):
        W = pol[:, wo:wo + ls[i - 1] * ls[i]].reshape(-1, ls[i], ls[i - 1])
        o = torch.bmm(W, o.unsqueeze(2)).squeeze(2) + pol[:, bo:bo + ls[i]]
        if tanh and i + 1 < len(ls):
            o = torch.tanh(o)
        wo += ls[i - 1] * ls[i]
        bo += ls[i]
    return o


def case(label, n, T, rounds, kind):
    m = tds_amd.load_model("ant")
    g = np.load(os.path.join(ROOT, "tests", "golden", "ant.npz"))["x"]
    x0 = torch.from_numpy(g[np.random.default_rng(0).integers(0, g.shape[0], n)]).cuda()
    sim = hb.HipSim(m, n, device=0, dtype="f64")
    nsd, n_act, _ = hb.trajectory_dims(m, T)
    rng = np.random.default_rng(1)
    w = torch.from_numpy(rng.normal(size=(n, T, nsd))).cuda()
    wu = torch.from_numpy(rng.normal(size=(n, T, n_act))).cuda()
    ls = [nsd, n_act] if kind == "linear" else [nsd, 64, 64, n_act]
    net = {} if kind == "linear" else dict(layer_sizes=ls, activations=[TANH, TANH, -1], use_bias=[0, 1, 1, 1])
    pol0 = torch.from_numpy(draw(ls, n, rng)).cuda()
    sel = [("gravity", 2), ("friction",)]
    th0 = torch.from_numpy(hb.params_get(m, sel)).cuda()
    f = tds_amd.param_step_fn(sim, sel, mode="reverse")
    out = {}

    def fused():
        _, u, gpol, _, gth = sim.policy_trajectory_vjp(x0, pol0, w, T, 1, wu, params=sel, theta=th0, **net)
        out["fused"] = (gpol, gth.sum(0), u)

    fused()
    u_taken = out["fused"][2]
    xu = x0.clone()
    xu[:, nsd:nsd + n_act] = u_taken[:, 0]
    u_rest = u_taken[:, 1:].contiguous()

    def open_loop():
        out["open"] = sim.trajectory_vjp(xu, w, T, 1, u_rest, sel, th0)

    def chain():
        th, pol = th0.clone().requires_grad_(True), pol0.clone().requires_grad_(True)
        state, loss = x0[:, :nsd], 0.0
        for t in range(T):
            ut = torch_policy(ls, kind != "linear", pol, state)
            y = f(torch.cat([state, ut, x0[:, nsd + n_act:]], dim=1), th)
            state = y[:, :nsd]
            loss = loss + (w[:, t] * state).sum() + (wu[:, t] * ut).sum()
        gth, gpol = torch.autograd.grad(loss, (th, pol))
        out["chain"] = (gpol, gth)

    variants = {"(a) policy_trajectory_vjp": fused, "(b) trajectory_vjp, open loop on (a)'s actions": open_loop,
                "(c) chained param_step_fn reverse + torch policy": chain}
    for fn in variants.values():  # warm-up: the work buffer grows, the kernels are loaded
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            times[k].append(wall_ms(fn))
    print(f"case {label}: ant x {n}, T = {T}, {kind} policy {ls}, P = {pol0.shape[1]}")
    for k, ts in times.items():
        print(f"  {k:50s} " + " ".join(f"{t:10.2f}" for t in ts) + f"   median {np.median(ts):10.2f} ms per gradient")
    # per environment, relative to the chain's largest entry; environments whose closed loop is unbounded over T steps
    # (NaN, or gradients past 1e6 where rounding decides) are counted, not compared
    gp_c, gp_f = out["chain"][0], out["fused"][0]
    big = gp_c.abs().amax(dim=1)
    ok = torch.isfinite(big) & (big < 1e6)
    err = (gp_f[ok] - gp_c[ok]).abs().amax(dim=1) / big[ok].clamp(min=1.0)
    print(f"  (a) against (c), gpolicy per environment: max {float(err.max()):.2e}, median {float(err.median()):.2e} "
          f"over {int(ok.sum())} of {n} bounded environments")
    del sim
    torch.cuda.empty_cache()


def main():
    T = int(os.environ.get("TRAJ_STEPS", 100))
    rounds = int(os.environ.get("TRAJ_ROUNDS", 3))
    for label, n in (("A", 256), ("B", 4096)):
        for kind in ("linear", "mlp"):
            if os.environ.get("TRAJ_CASE", label) == label and os.environ.get("TRAJ_POLICY", kind) == kind:
                case(f"{label} {kind}", n, T, rounds, kind)


if __name__ == "__main__":
    main()
