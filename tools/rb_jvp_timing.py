"""Times the rigid-body rollout derivatives on the billiard scene (tests/rb_scenes.py): N = 4096 worlds, 300 steps, 50
solver iterations.  Run it under `rocprofv3 --kernel-trace --stats -- python tools/rb_jvp_timing.py` for the kernel
times; it prints the wall clock per call (HIP events) itself.  Cases: tds_rb_step; tds_rb_jvp at k = 2 (one shot
gradient); tds_rb_jvp with the full 91-column state Jacobian (7 bodies)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402

from rb_scenes import WHITE, billiard_model, billiard_state, shot_velocity  # noqa: E402
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
    n, steps = int(os.environ.get("RB_N", 4096)), int(os.environ.get("RB_STEPS", 300))
    m = billiard_model()
    s0 = billiard_state(n)
    s0[:, WHITE, 7:9] = shot_velocity(np.random.default_rng(0).uniform([-100, 400], [100, 800], (n, 2)))
    sim = hb.RigidBodySim(m, n)
    x = torch.from_numpy(s0).cuda()
    sim.state.copy_(x)
    ns = m.num_bodies * 13
    v2 = torch.zeros((n, 2, ns), dtype=torch.float64, device="cuda")
    v2[:, 0, WHITE * 13 + 7] = 1.0
    v2[:, 1, WHITE * 13 + 8] = 1.0
    vfull = torch.eye(ns, dtype=torch.float64, device="cuda").expand(n, ns, ns).contiguous()
    print(f"billiards x {n}, {steps} steps, {m.solver_iterations} solver iterations")
    print(f"tds_rb_step:               {timed(lambda: sim.step(steps), 3):10.2f} ms per call")
    print(f"tds_rb_jvp k = 0:          {timed(lambda: sim.jvp(x, None, steps), 3):10.2f} ms per call")
    print(f"tds_rb_jvp k = 2:          {timed(lambda: sim.jvp(x, v2, steps), 3):10.2f} ms per call")
    print(f"tds_rb_jvp k = {ns} (full): {timed(lambda: sim.jvp(x, vfull, steps), 1):10.2f} ms per call")


if __name__ == "__main__":
    main()
