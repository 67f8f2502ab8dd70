"""Times the trajectory VJP (HipSim.trajectory_vjp) on the Ant over T = 100 steps against the same gradient through T
chained param_step_fn(mode="reverse") calls: the gradient of a trajectory loss <w, s> in the action sequence u
(T - 1 steps x 8 actions per environment) and in p = 2 parameters (gravity z, friction).  Case A: Ant x 256, case B:
Ant x 4096; the fused call at option traj_vjp_lanes unset (4096) and 16384.  One process, device-synchronised wall
clock, one warm-up of every variant first, then three rounds that alternate between the variants.  Run it under
`rocprofv3 --kernel-trace --stats -- python tools/traj_vjp_timing.py` for the kernel times (the gradients' equality is
checked by tests/test_traj_vjp_gpu.py)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402

import tds_amd  # noqa: E402
from tds_amd import hip_backend as hb  # noqa: E402


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def case(label, n, T, rounds):
    m = tds_amd.load_model("ant")
    g = np.load(os.path.join(ROOT, "tests", "golden", "ant.npz"))["x"]
    x0 = torch.from_numpy(g[np.random.default_rng(0).integers(0, g.shape[0], n)]).cuda()
    sim = hb.HipSim(m, n, device=0, dtype="f64")
    nsd, n_act, _ = hb.trajectory_dims(m, T)
    rng = np.random.default_rng(1)
    w = torch.from_numpy(rng.normal(size=(n, T, nsd))).cuda()
    u0 = torch.from_numpy(rng.uniform(-0.2, 0.2, (n, T - 1, n_act))).cuda()
    sel = [("gravity", 2), ("friction",)]
    th0 = torch.from_numpy(hb.params_get(m, sel)).cuda()
    f = tds_amd.param_step_fn(sim, sel, mode="reverse")
    out = {}

    def fused(lanes):
        def run():
            sim.set_option("traj_vjp_lanes", lanes)
            _, _, gu, gth = sim.trajectory_vjp(x0, w, T, 1, u0, sel, th0)
            out[lanes] = (gu, gth.sum(0))
        return run

    def chain():
        th, u = th0.clone().requires_grad_(True), u0.clone().requires_grad_(True)
        x, loss = x0, 0.0
        for t in range(T):
            y = f(x, th)
            loss = loss + (w[:, t] * y[:, :nsd]).sum()
            if t + 1 < T:
                x = torch.cat([y[:, :nsd], u[:, t], x0[:, nsd + n_act:]], dim=1)
        gth, gu = torch.autograd.grad(loss, (th, u))
        out["chain"] = (gu, gth)

    variants = {"trajectory_vjp, traj_vjp_lanes unset": fused(None), "trajectory_vjp, traj_vjp_lanes 16384": fused(16384),
                "chained param_step_fn reverse": chain}
    for fn in variants.values():  # warm-up: the work buffer grows, the kernels are loaded
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            times[k].append(wall_ms(fn))
    print(f"case {label}: ant x {n}, T = {T}, traj_steps = {sim.get_option('traj_steps') or 'default'}")
    for k, ts in times.items():
        print(f"  {k:40s} " + " ".join(f"{t:10.2f}" for t in ts) + f"   median {np.median(ts):10.2f} ms per gradient")
    # per environment, relative to the chain's largest entry; random actions from golden records over T steps leave
    # some rollouts unbounded (NaN, or gradients past 1e6 where rounding decides): those are counted, not compared
    gu_c, gth_c = out["chain"]
    big = gu_c.abs().amax(dim=(1, 2))
    ok = torch.isfinite(big) & (big < 1e6)
    for lanes in (None, 16384):
        gu_f = out[lanes][0]
        same = bool((torch.isfinite(gu_f).all(dim=2).all(dim=1) == torch.isfinite(big)).all())
        err = (gu_f[ok] - gu_c[ok]).abs().amax(dim=(1, 2)) / big[ok].clamp(min=1.0)
        print(f"  fused ({lanes or 'unset'}) against chain, gu per environment: max {float(err.max()):.2e}, median "
              f"{float(err.median()):.2e} over {int(ok.sum())} of {n} bounded environments (NaN in the same "
              f"environments: {same})")
    del sim
    torch.cuda.empty_cache()


def main():
    T = int(os.environ.get("TRAJ_STEPS", 100))
    rounds = int(os.environ.get("TRAJ_ROUNDS", 3))
    for label, n in (("A", 256), ("B", 4096)):
        if os.environ.get("TRAJ_CASE", label) == label:
            case(label, n, T, rounds)


if __name__ == "__main__":
    main()
