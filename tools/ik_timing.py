"""Times, in one process, batched inverse kinematics for Laikago's four feet (laikago_floating x 4096, targets a 3 cm
step of every toe from the pose, alpha 0.3) next to the yardstick it is held to: the same pinv iteration composed from
the public calls that existed before it (forward_kinematics, four point_jacobian, torch.linalg.pinv, the update), run
for as many iterations as the fused call's slowest environment takes.  Prints one line per case: the wall time per call
(a synchronise around `--reps` calls, after one warm-up call that also sizes the handle's work buffer).  --widths
64,32,16 repeats the pinv call with workgroups of that many lanes (TDS_HIP_DYN_WIDTH).

Run it under `rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o ik -- python tools/ik_timing.py` for the
kernel's own durations, then `python tools/ik_timing.py --summarise <dir>/ik_kernel_trace.csv` (same --reps, --widths)
for the table of profiles/ik_laikago4096_kernel_trace.txt (DESIGN 7c quotes both)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TOES = [3, 7, 11, 15]
METHODS = ("pinv", "damped_lm", "transpose")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--widths", default="64,32,16")
    ap.add_argument("--summarise", metavar="KERNEL_TRACE_CSV", help="print the kernel's durations per case of a traced run")
    args = ap.parse_args()
    if args.summarise:
        return summarise(args)

    import numpy as np
    import torch

    import tds_amd
    from tds_amd import hip_backend as hb

    m = tds_amd.load_model("laikago_floating")
    g = np.load(os.path.join(ROOT, "tests", "golden", "laikago_floating.npz"))
    rng = np.random.default_rng(0)
    q0 = g["x"][rng.integers(0, g["x"].shape[0], args.n), :m.dof_q].copy()
    q0[:, :4] /= np.linalg.norm(q0[:, :4], axis=1, keepdims=True)
    q0 = torch.from_numpy(q0).cuda()
    n, nd = args.n, m.dof_qd
    sim = hb.HipSim(m, n, device=0, dtype="f64")
    zero = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
    xw = sim.forward_kinematics(q0)[:, TOES]
    tgt = (xw[..., 9:] + torch.tensor([0.03, 0.0, 0.0], dtype=torch.float64, device="cuda")).contiguous()
    opts = dict(alpha=0.3, weight_reference=0.0)

    def timed(name, fn, **extra):
        fn()  # warm-up: module load, work buffer
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            fn()
        torch.cuda.synchronize()
        print(json.dumps(dict({"case": name, "n": n, "reps": args.reps,
                               "ms_per_call": round((time.perf_counter() - t0) * 1e3 / args.reps, 4)}, **extra)), flush=True)

    res = sim.inverse_kinematics(q0, TOES, tgt, method="pinv", **opts)
    iters = int(res["iterations"].max())
    print(json.dumps({"fused pinv": {"iterations_max": iters, "iterations_mean": float(res["iterations"].double().mean()),
                                     "status_counts": torch.bincount(res["status"], minlength=3).tolist()}}), flush=True)

    def composed():
        q = q0.clone()
        for _ in range(iters):
            x = sim.forward_kinematics(q)[:, TOES]
            J = torch.cat([sim.point_jacobian(q, l, zero, local=True) for l in TOES], dim=1)
            J[:, :, :6] = 0.0
            e = (tgt - x[..., 9:]).reshape(n, 12, 1)
            q[:, 7:] += 0.3 * (torch.linalg.pinv(J) @ e)[:, 6:, 0]
        return q

    for method in METHODS:
        timed(f"fused {method}", lambda method=method: sim.inverse_kinematics(q0, TOES, tgt, method=method, **opts))
    timed(f"composed pinv, {iters} iterations (the yardstick)", composed)
    for w in [int(s) for s in args.widths.split(",") if s]:
        os.environ["TDS_HIP_DYN_WIDTH"] = str(w)
        timed("fused pinv", lambda: sim.inverse_kinematics(q0, TOES, tgt, method="pinv", **opts), lanes_per_workgroup=w)
    os.environ.pop("TDS_HIP_DYN_WIDTH", None)
    # a check of the run, not a test: the composition without stopping rules ends where the fused call ends, up to the
    # iterations the fused call saves its early finishers
    print(json.dumps({"check": "max |q_fused - q_composed| over the environments that ran all iterations",
                      "max_abs": float((res["q"] - composed())[res["iterations"] == iters].abs().max())}))


def summarise(args):
    """kernel durations (ms) per case from a rocprofv3 kernel trace of this tool: tds_ik_kernel's dispatches in call
    order (one untimed call, then a warm-up and `reps` timed calls per case)"""
    import csv

    widths = [int(s) for s in args.widths.split(",") if s]
    rows = [r for r in csv.DictReader(open(args.summarise)) if "tds_ik_kernel" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    ms = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6  # noqa: E731
    per = args.reps + 1
    names = [f"fused {k}" for k in METHODS] + [f"fused pinv, {w} lanes per workgroup" for w in widths]
    line = "{:<40s} tds_ik_kernel wg {:>3s} x {:>4s}  calls {:d} mean {:7.3f} min {:7.3f} max {:7.3f}"
    for i, name in enumerate(names):
        grp = rows[1 + i * per:1 + (i + 1) * per][1:]
        t = [ms(r) for r in grp]
        wg = grp[0]["Workgroup_Size_X"]
        print(line.format(name, wg, str(int(grp[0]["Grid_Size_X"]) // int(wg)), len(t), sum(t) / len(t), min(t), max(t)))


if __name__ == "__main__":
    main()
