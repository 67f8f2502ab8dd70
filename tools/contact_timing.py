"""Times, in one process, the batched contact query of Ant x 4096 (HipSim.contacts: what the step itself forms, all nine
outputs, each output alone) next to the yardstick it is held to: the double step kernel tds_param_y_kernel, reached
through jvp_params with k = 0 and one parameter selected, exactly as tools/dyn_timing.py times it.  Prints one line per
case: the wall time per call (torch.cuda events around `--reps` calls, after one warm-up call that also sizes the
handle's work buffer).

Run it under `rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o ct -- python tools/contact_timing.py` for
the kernels' own durations, then `python tools/contact_timing.py --summarise <dir>/ct_kernel_trace.csv` (same --reps) for
the per-case table of profiles/contact_ant4096_kernel_trace.txt (DESIGN 7d quotes both)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OUTPUTS = ("contacts", "jac", "rows", "rhs", "delassus", "impulse", "force", "qd_pre", "qd_post")
STEP_FORMS = ("contacts", "rows", "rhs", "impulse", "force", "qd_pre", "qd_post")  # everything the step itself forms


def case_names():
    return ["contacts, what the step forms (7 outputs)", "contacts, all nine outputs"] + [f"contacts, {k} only" for k in OUTPUTS]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--model", default="ant")
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--summarise", metavar="KERNEL_TRACE_CSV", help="print the kernels' durations per case of a traced run")
    args = ap.parse_args()
    if args.summarise:
        return summarise(args)

    import numpy as np
    import torch

    import tds_amd
    from tds_amd import hip_backend as hb

    assert OUTPUTS == hb.CONTACT_OUTPUTS
    m = tds_amd.load_model(args.model)
    g = np.load(os.path.join(ROOT, "tests", "golden", f"{args.model}.npz"))
    rng = np.random.default_rng(0)
    x = torch.from_numpy(g["x"][rng.integers(0, g["x"].shape[0], args.n)]).cuda()
    sim = hb.HipSim(m, args.n, device=0, dtype="f64")
    sel = [("gravity", 2)]
    theta = torch.from_numpy(hb.params_get(m, sel)).cuda()
    out = {k: torch.empty(hb.contact_shapes(m, args.n)[k], dtype=torch.float64, device="cuda") for k in OUTPUTS}
    cases = {"step_y (tds_param_y_kernel, the yardstick)": lambda: sim.jvp_params(x, theta, sel),
             "contacts_step_forms": lambda: sim.contacts(x, want=STEP_FORMS, out=out),
             "contacts_all": lambda: sim.contacts(x, want=OUTPUTS, out=out)}
    for k in OUTPUTS:
        cases[f"contacts_{k}"] = (lambda k=k: sim.contacts(x, want=(k,), out=out))

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
                          "ms_per_call": round(t0.elapsed_time(t1) / args.reps, 4)}), flush=True)
    # a check of the run, not a test: qd_post against the step's own qd, and the penetrating points of the batch
    sim.contacts(x, want=OUTPUTS, out=out)
    y = sim.jvp_params(x, theta, sel)
    nq, nd = m.dof_q, m.dof_qd
    print(json.dumps({"check": "qd_post - qd of the step", "max_abs": float((out["qd_post"] - y[:, nq:nq + nd]).abs().max()),
                      "penetrating_points_per_env": float((out["contacts"][:, :, 9] < 0).sum(dim=1).double().mean())
                      if out["contacts"].numel() else 0.0}))


def summarise(args):
    """kernel durations (ms) per case from a rocprofv3 kernel trace of this tool: the dispatches in call order, a warm-up
    and `reps` timed calls per case"""
    import csv

    rows = [r for r in csv.DictReader(open(args.summarise)) if "tds_contact_kernel" in r["Kernel_Name"]
            or "tds_param_y_kernel" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    ms = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6  # noqa: E731
    per = args.reps + 1
    yard = [ms(r) for r in rows if "tds_param_y_kernel" in r["Kernel_Name"]][:per]
    ct = [r for r in rows if "tds_contact_kernel" in r["Kernel_Name"]]
    line = "{:<52s} {:<22s} wg {:>3s} x {:>4s}  calls {:d} mean {:7.3f} min {:7.3f} max {:7.3f}"
    print(line.format("step y, k = 0, one parameter (the yardstick)", "tds_param_y_kernel", "64", "-", len(yard),
                      sum(yard) / len(yard), min(yard), max(yard)))
    for i, name in enumerate(case_names()):
        grp = ct[i * per:(i + 1) * per]
        t = [ms(r) for r in grp]
        wg = grp[0]["Workgroup_Size_X"]
        print(line.format(name, "tds_contact_kernel", wg, str(int(grp[0]["Grid_Size_X"]) // int(wg)), len(t),
                          sum(t) / len(t), min(t), max(t)))


if __name__ == "__main__":
    main()
