"""Times the articulated trajectory derivatives on Ant x 4096 over T = 100 steps against one loss gradient through
chained param_step_fn, in forward and in reverse mode.  Run it under `rocprofv3 --kernel-trace --stats -- python
tools/traj_jvp_timing.py` for the kernel times; it prints the wall clock per call (HIP events) itself.  Cases: the
states alone (k = 0); the gradient of a trajectory loss in p = 2 parameters (gravity z, friction: one direction block)
and in the 14 link masses (tools/param_vjp_timing.py's selection), each through trajectory_fn and through T chained
param_step_fn calls in both modes (the gradients' equality is checked by tests/test_traj_derivs_gpu.py)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402

import tds_amd  # noqa: E402
from tds_amd import hip_backend as hb  # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    n, T = int(os.environ.get("TRAJ_N", 4096)), int(os.environ.get("TRAJ_STEPS", 100))
    m = tds_amd.load_model("ant")
    g = np.load(os.path.join(ROOT, "tests", "golden", "ant.npz"))["x"]
    x0 = torch.from_numpy(g[np.random.default_rng(0).integers(0, g.shape[0], n)]).cuda()
    sim = hb.HipSim(m, n, device=0, dtype="f64")
    nsd = m.dof_q + m.dof_qd
    w = torch.from_numpy(np.random.default_rng(1).normal(size=(n, T, nsd))).cuda()
    sels = {"p = 2": [("gravity", 2), ("friction",)], "14 masses": [("mass", i) for i in range(m.num_links)]}
    print(f"ant x {n}, T = {T}, traj_steps = {sim.get_option('traj_steps') or 'default'}")
    print(f"trajectory_jvp k = 0:                  {timed(lambda: sim.trajectory_jvp(x0, None, T), 3):10.2f} ms per call")
    grads = {}
    for name, sel in sels.items():
        th0 = torch.from_numpy(hb.params_get(m, sel)).cuda()
        traj = tds_amd.trajectory_fn(sim, T, (), sel)

        def g_traj():
            th = th0.clone().requires_grad_(True)
            grads[name, "traj"] = torch.autograd.grad((w * traj(x0, None, th)).sum(), th)[0]

        def g_chain(mode):
            f = tds_amd.param_step_fn(sim, sel, mode=mode)

            def run():
                th = th0.clone().requires_grad_(True)
                x, loss = x0, 0.0
                for t in range(T):
                    y = f(x, th)
                    loss = loss + (w[:, t] * y[:, :nsd]).sum()
                    x = torch.cat([y[:, :nsd], x0[:, nsd:]], dim=1)
                grads[name, mode] = torch.autograd.grad(loss, th)[0]
            return run

        print(f"{name}: trajectory_fn gradient:        {timed(g_traj, 2):10.2f} ms per call")
        print(f"{name}: chained param_step_fn reverse: {timed(g_chain('reverse'), 1):10.2f} ms per call")
        if name == "p = 2" or os.environ.get("TRAJ_FORWARD_ALL"):
            print(f"{name}: chained param_step_fn forward: {timed(g_chain('forward'), 1):10.2f} ms per call")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
