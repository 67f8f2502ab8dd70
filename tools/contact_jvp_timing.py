"""Times, in one process, the forward-mode derivatives of the contact query (HipSim.contacts_jvp: outputs impulse |
force | qd_post, one parameter selected) of `--model` x `--n` from golden records, at k = K (one block of directions)
and k = input_dim + p (the whole Jacobian), each alternated with the yardstick it is held to: the step's own forward
mode in [x | theta], HipSim.jvp_params, at the same n, k and p.  Also the primal query at theta (k = 0) beside
HipSim.contacts.  Prints one line per case: the wall time per call (torch.cuda events around `--reps` calls, after one
warm-up call of every case that also sizes the handle's work buffer), as tools/contact_timing.py does.

Run it under `rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o cj -- python tools/contact_jvp_timing.py`
for the kernels' own durations, then `python tools/contact_jvp_timing.py --summarise <dir>/cj_kernel_trace.csv` for the
per-kernel table (DESIGN 7d quotes both)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WANT = ("impulse", "force", "qd_post")
KERNELS = ("tds_contact_jvp_kernel", "tds_jvp_param_kernel", "tds_contact_kernel", "tds_param_y_kernel")


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
    n = args.n
    x = torch.from_numpy(g["x"][rng.integers(0, g["x"].shape[0], n)]).cuda()
    sim = hb.HipSim(m, n, device=0, dtype="f64")
    sel = [("friction",)]
    nall, K = m.input_dim + 1, hb.contacts_jvp_tangents(m)
    theta = torch.from_numpy(hb.params_get(m, sel)).cuda()
    cases = {}
    for k in (K, nall):
        v = torch.from_numpy(rng.normal(size=(n, k, nall))).cuda()
        out = {o: torch.empty(hb.contact_tangent_shapes(m, n, k)[o], dtype=torch.float64, device="cuda") for o in WANT}
        cases[f"contacts_jvp k={k}"] = (lambda v=v, out=out: sim.contacts_jvp(x, v, want=WANT, params=sel, theta=theta, out=out))
        cases[f"jvp_params k={k} (the yardstick)"] = (lambda v=v: sim.jvp_params(x, theta, sel, v))
    cases["contacts_jvp k=0 (the primal at theta)"] = lambda: sim.contacts_jvp(x, None, want=WANT, params=sel, theta=theta)
    cases["contacts (the primal query)"] = lambda: sim.contacts(x, want=WANT)
    for fn in cases.values():  # warm-up: module load, the work buffer at its largest
        fn()
    torch.cuda.synchronize()
    total = dict.fromkeys(cases, 0.0)
    for _ in range(args.reps):  # alternated: a case and its yardstick see the same clocks
        for name, fn in cases.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            torch.cuda.synchronize()
            total[name] += t0.elapsed_time(t1)
    for name in cases:
        print(json.dumps({"case": name, "model": args.model, "n": n, "p": 1, "K": K, "reps": args.reps,
                          "ms_per_call": round(total[name] / args.reps, 4)}), flush=True)


def summarise(args):
    """kernel durations (ms) per kernel and grid from a rocprofv3 kernel trace of this tool: the warm-up call of each
    case is its first dispatch and is left out"""
    import collections
    import csv

    rows = [r for r in csv.DictReader(open(args.summarise)) if any(k in r["Kernel_Name"] for k in KERNELS)]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    groups = collections.OrderedDict()
    for r in rows:
        name = next(k for k in KERNELS if k in r["Kernel_Name"])
        full = r["Kernel_Name"]  # (mangled or demangled, as the profiler writes it)
        primal = name == "tds_contact_jvp_kernel" and ("Li0EE" in full or ", 0>" in full or ",0>" in full)
        key = (name, "k = 0" if primal else "", r["Workgroup_Size_X"], r["Grid_Size_X"])
        groups.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6)
    for (name, kind, wg, grid), t in groups.items():
        t = t[1:] or t
        print("{:<24s} {:<7s} wg {:>3s} x {:>5d}  calls {:d} mean {:8.3f} min {:8.3f} max {:8.3f}".format(
            name, kind, wg, int(grid) // int(wg), len(t), sum(t) / len(t), min(t), max(t)))


if __name__ == "__main__":
    main()
