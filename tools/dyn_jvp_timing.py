"""Times, in one process, the forward-mode derivatives of the dynamics queries (HipSim.dynamics_jvp /
inverse_dynamics_jvp) of `--model` x `--n` from golden records: the dense derivative of qdd in [q | qd | tau] (every
column, one launch) alternated with the yardstick it is held to, what a user did before: central differences through
HipSim.dynamics(want=qdd), two launches per column.  Also, without a requirement, the same directions with all four
outputs, and inverse_dynamics_jvp in [q | qd | qdd | the first five link masses].  Prints one line per case: the median
and the mean wall time per call (torch.cuda events around each of `--reps` calls, after one warm-up call of every case
that also sizes the handle's work buffer).

Run it under `rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o dj -- python tools/dyn_jvp_timing.py`
for the kernels' own durations, then `python tools/dyn_jvp_timing.py --summarise <dir>/dj_kernel_trace.csv` for the
per-kernel table (DESIGN 7b quotes both)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = ("tds_dyn_jvp_kernel", "tds_dyn_kernel")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--model", default="ant")
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--summarise", metavar="KERNEL_TRACE_CSV", help="print the kernels' durations of a traced run")
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
    n, nq, nd, nt = args.n, m.dof_q, m.dof_qd, hb.dyn_tau_dim(m)
    x = g["x"][rng.integers(0, g["x"].shape[0], n)]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    q, qd = dev(x[:, :nq]), dev(x[:, nq:nq + nd])
    tau, qdd = dev(rng.normal(size=(n, nt))), dev(rng.normal(size=(n, nd)))
    sim = hb.HipSim(m, n, device=0, dtype="f64")
    K, nx = hb.dynamics_jvp_tangents(m), nq + nd + nt
    eye = dev(np.broadcast_to(np.eye(nx), (n, nx, nx)))
    shapes = hb.dyn_tangent_shapes(m, n, nx)
    out = {o: torch.empty(shapes[o], dtype=torch.float64, device="cuda") for o in hb.DYN_OUTPUTS}
    fd = torch.empty((n, nd, nx), dtype=torch.float64, device="cuda")
    plus, minus = ({"qdd": torch.empty((n, nd), dtype=torch.float64, device="cuda")} for _ in range(2))

    def central_differences(h=1e-6):
        """d qdd / d [q | qd | tau] as a user of the primal query forms it: two launches per column"""
        col = 0
        for z in (q, qd, tau):
            for j in range(z.shape[1]):
                z[:, j] += h
                sim.dynamics(q, qd, tau, want=("qdd",), out=plus)
                z[:, j] -= 2 * h
                sim.dynamics(q, qd, tau, want=("qdd",), out=minus)
                z[:, j] += h
                fd[:, :, col] = (plus["qdd"] - minus["qdd"]) / (2 * h)
                col += 1
        return fd

    cases = {
        f"dynamics_jvp qdd, k={nx}": lambda: sim.dynamics_jvp(q, qd, tau, eye, want=("qdd",), out=out),
        f"central differences of dynamics(qdd), {2 * nx} launches (the yardstick)": central_differences,
        f"dynamics_jvp all outputs, k={nx}": lambda: sim.dynamics_jvp(q, qd, tau, eye, want=hb.DYN_OUTPUTS, out=out),
    }
    if not m.is_floating:
        sel = [("mass", i) for i in range(min(5, m.num_links))]
        ni = nq + 2 * nd + len(sel)
        eye_i = dev(np.broadcast_to(np.eye(ni), (n, ni, ni)))
        cases[f"inverse_dynamics_jvp, k={ni}, p={len(sel)}"] = \
            lambda: sim.inverse_dynamics_jvp(q, qd, qdd, eye_i, params=sel)
    for fn in cases.values():  # warm-up: module load, the work buffer at its largest
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name in cases}
    for _ in range(args.reps):  # alternated: a case and its yardstick see the same clocks
        for name, fn in cases.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            torch.cuda.synchronize()
            times[name].append(t0.elapsed_time(t1))
    err = float(((sim.dynamics_jvp(q, qd, tau, eye, want=("qdd",))["qdd"].movedim(1, -1) - central_differences()).abs().max()
                 / out["qdd"].abs().max().clamp(min=1.0)).cpu())
    for name, t in times.items():
        print(json.dumps({"case": name, "model": args.model, "n": n, "K": K, "reps": args.reps,
                          "ms_median": round(statistics.median(t), 4), "ms_mean": round(sum(t) / len(t), 4),
                          "ms_min": round(min(t), 4), "ms_max": round(max(t), 4)}), flush=True)
    print(json.dumps({"jvp_against_central_differences_rel": err}), flush=True)


def summarise(args):
    """kernel durations (ms) per kernel and grid from a rocprofv3 kernel trace of this tool, in dispatch order"""
    import collections
    import csv

    rows = [r for r in csv.DictReader(open(args.summarise)) if any(k in r["Kernel_Name"] for k in KERNELS)]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    groups = collections.OrderedDict()
    for r in rows:
        name = next(k for k in KERNELS if k in r["Kernel_Name"])
        key = (name, r["Workgroup_Size_X"], r["Grid_Size_X"])
        groups.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6)
    for (name, wg, grid), t in groups.items():
        print("{:<20s} wg {:>3s} x {:>5d}  launches {:4d} mean {:8.3f} median {:8.3f} min {:8.3f} max {:8.3f} sum {:9.3f}"
              .format(name, wg, int(grid) // int(wg), len(t), sum(t) / len(t), statistics.median(t), min(t), max(t), sum(t)))
        if name == "tds_dyn_jvp_kernel":  # the cases share a grid: each launch, in the order of the cases
            print("    each (ms): " + " ".join(f"{v:.3f}" for v in t))


if __name__ == "__main__":
    main()
