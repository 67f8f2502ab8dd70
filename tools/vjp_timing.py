"""Times, in one process, the step derivatives of Ant x 4096: the dense Jacobian (forward mode, HipSim.jacobian) and
the VJP (reverse mode, HipSim.vjp) at k = 1 and k = 8 cotangents.  Prints one line per case: the wall time per call
(torch.cuda events around `--reps` calls, after one warm-up call that also sizes the handle's work buffer).

Run it under `rocprofv3 --kernel-trace --stats -d <dir> -o vjp -- python tools/vjp_timing.py` for the kernels' own
durations (DESIGN 7a quotes both)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--model", default="ant")
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()

    import numpy as np
    import torch

    import tds_amd
    from tds_amd import hip_backend as hb

    m = tds_amd.load_model(args.model)
    g = np.load(os.path.join(ROOT, "tests", "golden", f"{args.model}.npz"))
    rng = np.random.default_rng(0)
    x = torch.from_numpy(g["x"][rng.integers(0, g["x"].shape[0], args.n)]).cuda()
    sim = hb.HipSim(m, args.n, device=0, dtype="f64")
    w8 = torch.from_numpy(rng.normal(size=(args.n, 8, m.output_dim))).cuda()
    cases = {
        "jacobian": lambda: sim.jacobian(x),
        "vjp_k1": lambda: sim.vjp(x, w8[:, :1]),
        "vjp_k8": lambda: sim.vjp(x, w8),
    }
    for name, fn in cases.items():
        fn()  # warm-up: module load, work buffer
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(args.reps):
            fn()
        t1.record()
        torch.cuda.synchronize()
        print(json.dumps({"case": name, "model": args.model, "n": args.n, "reps": args.reps,
                          "ms_per_call": round(t0.elapsed_time(t1) / args.reps, 3),
                          "device_used_bytes": device_used()}), flush=True)
    # the two modes agree (a check of the run, not a test)
    _, wj = sim.vjp(x, w8[:, :1])
    ref = torch.einsum("no,noi->ni", w8[:, 0], sim.jacobian(x))
    print(json.dumps({"check": "vjp_k1 vs w^T jacobian",
                      "max_rel": float((wj[:, 0] - ref).abs().max() / max(1.0, float(ref.abs().max())))}))


def device_used():
    """bytes in use on the device (the handle's work buffer is most of it; the C ABI does not expose its size)"""
    import torch

    free, total = torch.cuda.mem_get_info()
    return int(total - free)


if __name__ == "__main__":
    main()
