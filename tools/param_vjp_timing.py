"""Times, in one process, the parameter derivatives of Ant x 4096 against the plain ones: vjp (k = 1, the baseline),
vjp_params with the 14 link masses, with every parameter of all_params and with those plus every contact parameter
(contact_params: cfm, erp, the shapes), jvp_params over [x | the 14 masses] (one
unit direction per input: the dense Jacobian in [x | theta]), and the dense Jacobian.  Prints one line per case: the
wall time per call (torch.cuda events around `--reps` calls, after one warm-up call that also sizes the handle's work
buffer), then the tape lengths the host template records for a sample of the records (parameter mode, every
parameter selected; plain mode).  The y-only cases compare jvp_params at k = 0 (the double step over a double
overlay) with one tangent direction (the dual kernel) and with forward_zero.

Run it under `rocprofv3 --kernel-trace --stats -d <dir> -o param_vjp -- python tools/param_vjp_timing.py` for the
kernels' own durations (DESIGN 7a quotes both)."""
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
    x_np = g["x"][rng.integers(0, g["x"].shape[0], args.n)]
    x = torch.from_numpy(x_np).cuda()
    sim = hb.HipSim(m, args.n, device=0, dtype="f64")
    masses = [("mass", i) for i in range(m.num_links)]
    every = hb.all_params(m)
    th_m = torch.from_numpy(hb.params_get(m, masses)).cuda()
    th_a = torch.from_numpy(hb.params_get(m, every)).cuda()
    every_c = every + hb.contact_params(m)
    th_c = torch.from_numpy(hb.params_get(m, every_c)).cuda()
    w = torch.from_numpy(rng.normal(size=(args.n, 1, m.output_dim))).cuda()
    nall = m.input_dim + len(masses)
    eye = torch.eye(nall, dtype=torch.float64, device="cuda").expand(args.n, nall, nall).contiguous()
    v1 = torch.from_numpy(rng.normal(size=(args.n, 1, m.input_dim + len(every)))).cuda()
    cases = {
        "vjp_k1": lambda: sim.vjp(x, w),
        "vjp_params_masses": lambda: sim.vjp_params(x, th_m, masses, w),
        "vjp_params_every": lambda: sim.vjp_params(x, th_a, every, w),
        "vjp_params_every_and_contact": lambda: sim.vjp_params(x, th_c, every_c, w),
        "jvp_params_masses_dense": lambda: sim.jvp_params(x, th_m, masses, eye),
        "jacobian": lambda: sim.jacobian(x),
        # y at theta: k = 0 runs the double step over a double overlay; one direction runs the dual kernel
        "jvp_params_y_only_every": lambda: sim.jvp_params(x, th_a, every),
        "jvp_params_k1_every": lambda: sim.jvp_params(x, th_a, every, v1),
        "forward_zero": lambda: sim.forward_zero(x),
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
    # the two modes agree on the masses' columns (a check of the run, not a test)
    _, _, wjt = sim.vjp_params(x, th_m, masses, w)
    _, jv = sim.jvp_params(x, th_m, masses, eye[:, m.input_dim:])
    ref = torch.einsum("no,npo->np", w[:, 0], jv)
    print(json.dumps({"check": "vjp_params vs w^T jvp_params (masses)",
                      "max_rel": float((wjt[:, 0] - ref).abs().max() / max(1.0, float(ref.abs().max())))}))
    sample = x_np[:64]
    zeros = np.zeros((sample.shape[0], m.output_dim))
    _, lens_p = hb.vjp_params_host(m, sample, hb.params_get(m, every), every, zeros, tape_len=True)
    _, lens_m = hb.vjp_params_host(m, sample, hb.params_get(m, masses), masses, zeros, tape_len=True)
    _, lens_c = hb.vjp_params_host(m, sample, hb.params_get(m, every_c), every_c, zeros, tape_len=True)
    _, lens = hb.vjp_host(m, sample, zeros, tape_len=True)
    print(json.dumps({"tape_len_max": {"plain": int(lens.max()), "masses": int(lens_m.max()),
                                       "every": int(lens_p.max()), "every_and_contact": int(lens_c.max())},
                      "p_every": len(every), "p_every_and_contact": len(every_c)}))


def device_used():
    """bytes in use on the device (the handle's work buffer is most of it; the C ABI does not expose its size)"""
    import torch

    free, total = torch.cuda.mem_get_info()
    return int(total - free)


if __name__ == "__main__":
    main()
