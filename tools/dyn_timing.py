"""Times, in one process, the batched dynamics queries of Ant x 4096 (HipSim.dynamics with all four outputs, each
output alone, inverse_dynamics, point_jacobian) next to the yardstick they are held to: the double step kernel
tds_param_y_kernel, reached through jvp_params with k = 0 and one parameter selected.  Prints one line per case: the
wall time per call (torch.cuda events around `--reps` calls, after one warm-up call that also sizes the handle's work
buffer).  --widths 64,32,16 repeats the full query with workgroups of that many lanes (TDS_HIP_DYN_WIDTH), the
occupancy choice of csrc/tds_dyn.hip.

Run it under `rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o dyn -- python tools/dyn_timing.py` for the
kernels' own durations, then `python tools/dyn_timing.py --summarise <dir>/dyn_kernel_trace.csv` (same --reps, --widths)
for the per-case table of profiles/dyn_ant4096_kernel_trace.txt (DESIGN 7b quotes both)."""
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--widths", default="64,32,16")
    ap.add_argument("--summarise", metavar="KERNEL_TRACE_CSV", help="print the kernels' durations per case of a traced run")
    args = ap.parse_args()
    if args.summarise:
        return summarise(args)

    import numpy as np
    import torch

    import tds_amd
    from tds_amd import hip_backend as hb

    m = tds_amd.load_model(args.model)
    g = np.load(os.path.join(ROOT, "tests", "golden", f"{args.model}.npz"))
    rng = np.random.default_rng(0)
    x = torch.from_numpy(g["x"][rng.integers(0, g["x"].shape[0], args.n)]).cuda()
    nq, nd = m.dof_q, m.dof_qd
    q, qd = x[:, :nq].contiguous(), x[:, nq:nq + nd].contiguous()
    tau = torch.from_numpy(rng.normal(size=(args.n, hb.dyn_tau_dim(m)))).cuda()
    qdd = torch.from_numpy(rng.normal(size=(args.n, nd))).cuda()
    pts = torch.from_numpy(rng.normal(0, 0.3, size=(args.n, 3))).cuda()
    sim = hb.HipSim(m, args.n, device=0, dtype="f64")
    sel = [("gravity", 2)]
    theta = torch.from_numpy(hb.params_get(m, sel)).cuda()
    full = ("x_world", "mass_matrix", "qdd") if m.is_floating else hb.DYN_OUTPUTS
    link = max(i for i in range(m.num_links) if m.links[i].joint_type != tds_amd.JOINT_FIXED)
    out = {k: torch.empty(hb.dyn_shapes(m, args.n)[k], dtype=torch.float64, device="cuda") for k in full}
    cases = {"step_y (tds_param_y_kernel, the yardstick)": lambda: sim.jvp_params(x, theta, sel),
             "dynamics_all": lambda: sim.dynamics(q, qd, tau, want=full, out=out)}
    for k in full:
        cases[f"dynamics_{k}"] = (lambda k=k: sim.dynamics(q, qd, tau, want=(k,), out=out))
    if not m.is_floating:
        cases["inverse_dynamics"] = lambda: sim.inverse_dynamics(q, qd, qdd)
    cases["point_jacobian"] = lambda: sim.point_jacobian(q, link, pts)

    def timed(name, fn, **extra):
        fn()  # warm-up: module load, work buffer
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(args.reps):
            fn()
        t1.record()
        torch.cuda.synchronize()
        print(json.dumps(dict({"case": name, "model": args.model, "n": args.n, "reps": args.reps,
                               "ms_per_call": round(t0.elapsed_time(t1) / args.reps, 4)}, **extra)), flush=True)

    for name, fn in cases.items():
        timed(name, fn)
    for w in [int(s) for s in args.widths.split(",") if s]:
        os.environ["TDS_HIP_DYN_WIDTH"] = str(w)
        timed("dynamics_all", cases["dynamics_all"], lanes_per_workgroup=w)
    os.environ.pop("TDS_HIP_DYN_WIDTH", None)
    # a check of the run, not a test: M qdd + bias = tau on a fixed base
    if not m.is_floating:
        d = sim.dynamics(q, qd, tau)
        res = torch.einsum("nij,nj->ni", d["mass_matrix"], d["qdd"]) + d["bias"] - tau
        print(json.dumps({"check": "M qdd + bias - tau (no springs in this model)" if not any(
            m.links[i].stiffness or m.links[i].damping for i in range(m.num_links)) else "M qdd + bias - tau + K q + D qd",
            "max_abs": float(res.abs().max())}))


def case_names(floating, widths):
    full = ("x_world", "mass_matrix", "qdd") if floating else ("x_world", "mass_matrix", "bias", "qdd")
    names = ["dynamics, all outputs"] + [f"dynamics, {k} only" for k in full]
    names += ([] if floating else ["inverse_dynamics"]) + ["point_jacobian"]
    return names + [f"dynamics, all outputs, {w} lanes per workgroup" for w in widths]


def summarise(args):
    """kernel durations (ms) per case from a rocprofv3 kernel trace of this tool: the dispatches in call order, a warm-up
    and `reps` timed calls per case"""
    import csv

    widths = [int(s) for s in args.widths.split(",") if s]
    rows = [r for r in csv.DictReader(open(args.summarise)) if "tds_dyn_kernel" in r["Kernel_Name"]
            or "tds_param_y_kernel" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    ms = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6  # noqa: E731
    per = args.reps + 1
    yard = [ms(r) for r in rows if "tds_param_y_kernel" in r["Kernel_Name"]]
    dyn = [r for r in rows if "tds_dyn_kernel" in r["Kernel_Name"]]
    floating = len(dyn) // per < len(case_names(False, widths))
    line = "{:<52s} {:<22s} wg {:>3s} x {:>4s}  calls {:d} mean {:7.3f} min {:7.3f} max {:7.3f}"
    print(line.format("step y, k = 0, one parameter (the yardstick)", "tds_param_y_kernel", "64", "-", len(yard),
                      sum(yard) / len(yard), min(yard), max(yard)))
    for i, name in enumerate(case_names(floating, widths)):
        grp = dyn[i * per:(i + 1) * per]
        t = [ms(r) for r in grp]
        wg = grp[0]["Workgroup_Size_X"]
        print(line.format(name, "tds_dyn_kernel", wg, str(int(grp[0]["Grid_Size_X"]) // int(wg)), len(t), sum(t) / len(t),
                          min(t), max(t)))


if __name__ == "__main__":
    main()
