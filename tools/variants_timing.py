"""Times the step loop with per-environment model variants installed: Ant x 4096 in double, option oct = 0 (the general
kernel), tds_hip_step_many_rings of 1000 steps with obs and y rings, HIP events around each call.  Cases, alternated
round by round on ONE handle so that they share whatever else runs on the machine: no variants (the baseline: the
handle's ordinary step-loop build, two wavefronts per workgroup at this size), no variants with option loop_w2 = 0 (the
ordinary ONE-wavefront step-loop build: the form the variant builds have), V = 1, V = 16, V = 4096.  Prints us per step per case: the median over the rounds
and the spread (min .. max).  VARIANTS_N / VARIANTS_STEPS / VARIANTS_ROUNDS override the sizes; VARIANTS_BASELINE_ONLY=1
runs the first case alone and calls nothing of the variants' interface (a library from before it: the same handle's rate
on the parent commit)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

import torch  # noqa: E402

import tds_amd  # noqa: E402
from tds_amd import hip_backend as hb  # noqa: E402

SEL = [("mass", 7), ("com", 8, 1), ("inertia", 9, 3), ("xt_trans", 10, 0), ("stiffness", 11), ("damping", 12),
       ("gravity", 2), ("friction",), ("restitution",)]


def main():
    n = int(os.environ.get("VARIANTS_N", 4096))
    steps = int(os.environ.get("VARIANTS_STEPS", 1000))
    rounds = int(os.environ.get("VARIANTS_ROUNDS", 5))
    m = tds_amd.load_model("ant")
    g = np.load(os.path.join(ROOT, "tests", "golden", "ant.npz"))["x"]
    rng = np.random.default_rng(0)
    x0 = torch.from_numpy(g[rng.integers(0, g.shape[0], n)]).cuda()
    blocks, slots = 16, 8
    acts = torch.from_numpy(rng.uniform(-0.4, 0.4, (blocks, n, m.action_dim))).cuda().contiguous()
    sim = hb.HipSim(m, n, options={"oct": 0})
    obs_ring = torch.zeros((slots, n, sim.obs_dim + 2), dtype=torch.float64, device="cuda")
    y_ring = torch.zeros((slots, n, m.output_dim), dtype=torch.float64, device="cuda")
    base = hb.params_get(m, SEL)
    baseline_only = os.environ.get("VARIANTS_BASELINE_ONLY", "0") == "1"
    cases = [("no variants", 0)] + ([] if baseline_only else [("no variants, loop_w2 = 0", -1)] + [(f"V = {v}", v) for v in (1, 16, n)])
    theta = base * (1.0 + 0.05 * rng.uniform(-1, 1, (n, len(SEL))))
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {name: [] for name, _ in cases}
    print(f"ant x {n}, f64, oct = 0, step_many_rings of {steps} steps, {rounds} rounds (+ 1 warm-up round)")
    if not baseline_only:
        print(f"device model: {hb.model_variants_host(m, SEL, theta[:1], np.zeros(n), n)} B per variant")
    for r in range(rounds + 1):
        for name, v in cases:
            if v <= 0:
                if not baseline_only:
                    sim.clear_model_variants()
                    sim.set_option("loop_w2", 0 if v < 0 else None)
            else:
                sim.set_model_variants(SEL, theta[:v], None if v == n else rng.permutation(np.arange(n) % v))
            assert sim.step_many_is_loop(steps) and sim.single_step_kernel()[0] == "general"
            sim.x.copy_(x0)
            sim.step_many_rings(acts, 20, obs_ring=obs_ring, y_ring=y_ring)  # (warm: code object, rings)
            sim.x.copy_(x0)
            torch.cuda.synchronize()
            a.record()
            sim.step_many_rings(acts, steps, obs_ring=obs_ring, y_ring=y_ring)
            b.record()
            torch.cuda.synchronize()
            if r > 0:
                times[name].append(1e3 * a.elapsed_time(b) / steps)
    for name, _ in cases:
        t = np.array(times[name])
        print(f"{name:24s}: {np.median(t):8.3f} us per step (min {t.min():.3f} .. max {t.max():.3f}), "
              f"{n / np.median(t):8.1f} M env-steps/s")


if __name__ == "__main__":
    main()
