"""Do two builds of libtds_hip.so compute the same reverse-mode rollout derivatives, bit for bit?

    python tools/rollout_vjp_ab.py <parent libtds_hip.so> [--device] [-o report]

Runs the trajectory VJP, the closed-loop policy gradient and the rigid-body rollout VJP once under the parent's library
and once under this tree's (TDS_HIP_LIB), each entry point and library in a fresh child process, and compares every
output of every case with array_equal (NaN equal to NaN: the overflowing cases).  Without --device the host entry points
run (no GPU needed): test_traj_vjp_cpu.py's models at 7 steps with every 1 and at 6 steps with every 3 (every divides
steps), with and without u; a linear and an MLP policy with gs only, ga only and both; the mixed and billiard scenes of
test_rb_vjp_cpu.py; one overflowing tape_cap each.  With --device the device calls run on shapes that cross every
boundary of the chained sweep's loops: ant and pendulum5 at n = 130 (two full wavefronts and a ragged one), 7 steps,
traj_vjp_lanes 64 and unset x traj_steps 1, 5 and unset, open loop and closed loop with both policy kinds; the mixed
scene at n = 70 with work_bytes that force windows shorter than the rollout and two passes.  Exit status 0: every output
equal."""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]

STEPS = 7
ENTRIES = ["traj", "policy", "rb"]


def host_traj(hb):
    from test_traj_vjp_cpu import MODELS, case, gs_of, raw

    for name in MODELS:
        for steps, every in ((STEPS, 1), (STEPS - 1, 3)):  # every divides steps: 3 goes with 6 steps
            m, sel, x0, u, th, gs = case(name, 6, steps)
            for with_u in (True, False):
                yield f"{name} steps={steps} every={every} u={with_u}", hb.trajectory_vjp_host(
                    m, x0, gs_of(gs, every), steps, every, u if with_u else None, sel, th, tape_len=True)
    m, sel, x0, u, th, gs = case("ant", 6, STEPS)
    lens = hb.trajectory_vjp_host(m, x0, gs, STEPS, 1, u, sel, th, tape_len=True)[4]
    cap = int(np.sort(lens.max(axis=1))[2])
    yield f"ant tape_cap={cap} (overflows)", raw(m, x0, gs, STEPS, u, sel, th, tape_cap=cap)


def host_policy(hb):
    from test_policy_grad_cpu import draw_policy, net_args, net_of, raw_call
    from test_traj_vjp_cpu import case

    m, sel, x0, _, th, gs = case("ant", 6, STEPS)
    ga = np.random.default_rng(15).normal(size=(6, STEPS, m.action_dim))
    for kind in ("linear", "mlp"):
        pol = draw_policy(m, kind, 6)
        for label, g, a in (("gs", gs, None), ("ga", None, ga), ("gs+ga", gs, ga)):
            yield f"ant {kind} {label}", hb.policy_trajectory_vjp_host(m, x0, pol, g, STEPS, 1, a, params=sel, theta=th,
                                                                       tape_len=True, **net_args(m, kind))
    pol = draw_policy(m, "mlp", 6)
    lens = hb.policy_trajectory_vjp_host(m, x0, pol, gs, STEPS, 1, ga, params=sel, theta=th, tape_len=True,
                                         **net_args(m, "mlp"))[5]
    cap = int(np.sort(lens.max(axis=1))[2])
    ls, act, ub = net_of(m, "mlp")
    yield f"ant mlp tape_cap={cap} (overflows)", raw_call(m, x0, pol, gs, ga, STEPS, sel, th,
                                                          net=(len(ls), ls, act, ub), tape_cap=cap)


def host_rb(hb):
    from rb_scenes import WHITE, billiard_model, billiard_state, shot_velocity
    from test_rb_vjp_cpu import raw, scene

    for name in ("mixed", "billiard"):
        m, s0, steps, params, th = scene(name)
        for every in (1, steps):
            gs = np.random.default_rng(steps + every).normal(size=(s0.shape[0], steps // every, m.num_bodies * 13))
            yield f"{name} steps={steps} every={every}", hb.rb_vjp_host(m, s0, steps, gs, params, th, every)
    m = billiard_model()
    s0 = billiard_state(2)
    s0[0, WHITE, 7:9] = shot_velocity([10.0, 600.0])
    s0[1, :, 0], s0[1, :, 1] = 10.0 * np.arange(7), 0.0
    gs = np.random.default_rng(4).normal(size=(2, 1, 91))
    yield "billiard tape_cap=1000 (overflows)", raw(m, s0, 40, gs, [("mass", 5), ("friction",)], tape_cap=1000)


PLANS = [(lanes, ts) for lanes in (64, None) for ts in (1, 5, None)]


def device_traj(hb):
    from test_traj_vjp_gpu import device, inputs

    for name in ("ant", "pendulum5"):
        m, sel, x, th, u, gs = inputs(name, 130, STEPS)
        sim = hb.HipSim(m, 64, device=0, dtype="f64")
        for lanes, ts in PLANS:
            sim.set_option("traj_vjp_lanes", lanes)
            sim.set_option("traj_steps", ts)
            yield f"{name} n=130 traj_vjp_lanes={lanes} traj_steps={ts}", device(sim, x, gs, STEPS, 1, u, sel, th)


def device_policy(hb):
    from test_policy_grad_gpu import device, inputs

    for name in ("ant", "pendulum5"):
        for kind in ("linear", "mlp"):
            m, sel, x, th, pol, gs, ga = inputs(name, kind, 130, STEPS)
            sim = hb.HipSim(m, 64, device=0, dtype="f64")
            for lanes, ts in PLANS:
                sim.set_option("traj_vjp_lanes", lanes)
                sim.set_option("traj_steps", ts)
                yield (f"{name} {kind} n=130 traj_vjp_lanes={lanes} traj_steps={ts}",
                       device(sim, name, kind, x, pol, gs, ga, STEPS, 1, sel, th))


def device_rb(hb):
    import torch
    from rb_scenes import MIXED_ORDER, make_mixed_worlds
    from test_rb_vjp_gpu import budget_for

    n, params = 70, [("mass", 3), ("gravity", 2), ("friction",), ("restitution",)]
    m, s0 = make_mixed_worlds(n, 21, MIXED_ORDER)
    th = hb.rb_params_get(m, params) + 0.05 * (1 + np.random.default_rng(2).random((n, len(params))))
    gs = np.random.default_rng(3).normal(size=(n, STEPS, m.num_bodies * 13))
    cap = hb.rb_vjp_plan(m, n, STEPS, len(params))[0]
    # one pass with windows of 3, 3 and 1 steps; two passes (64 + 6 worlds) with windows of one step
    bounds = [budget_for(m, n, STEPS, len(params), cap, chunk, W) for chunk, W in ((128, 3), (64, 1))]
    sim = hb.RigidBodySim(m, 1)
    for label, b in [("default", 0)] + [(f"work_bytes={wb}", wb) for wb in bounds]:
        plan = hb.rb_vjp_plan(m, n, STEPS, len(params), cap, b)
        out = sim.vjp(torch.from_numpy(s0).cuda(), torch.from_numpy(gs).cuda(), STEPS, params,
                      torch.from_numpy(th).cuda(), every=1, tape_cap=cap, work_bytes=b)
        yield f"mixed n={n} {label}: {plan[1]} worlds x {plan[2]} steps", tuple(t.cpu().numpy() for t in out)


def child(entry, device, out):
    from tds_amd import hip_backend as hb

    cases = globals()[("device_" if device else "host_") + entry](hb)
    np.savez(out, **{f"{label}|{i}": np.asarray(a) for label, outs in cases for i, a in enumerate(outs)})


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("parent_lib")
    ap.add_argument("--device", action="store_true")
    ap.add_argument("-o", "--output")
    ap.add_argument("--child", nargs=2, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.child[0], args.device, args.child[1])
    lines, bad = [f"# {'device' if args.device else 'host'} calls under {args.parent_lib} (parent) and under this tree's "
                  "library, every output compared with array_equal"], 0
    with tempfile.TemporaryDirectory() as tmp:
        for entry in ENTRIES:
            got = []
            for side, libpath in (("parent", os.path.abspath(args.parent_lib)), ("tree", None)):
                env = dict(os.environ)
                env.pop("TDS_HIP_LIB", None)
                if libpath:
                    env["TDS_HIP_LIB"] = libpath
                out = os.path.join(tmp, f"{entry}_{side}.npz")
                cmd = [sys.executable, os.path.abspath(__file__), args.parent_lib, "--child", entry, out]
                subprocess.run(cmd + (["--device"] if args.device else []), env=env, check=True, timeout=600)
                got.append(np.load(out))
            a, b = got
            assert sorted(a.files) == sorted(b.files), (a.files, b.files)
            for label in dict.fromkeys(k.split("|")[0] for k in a.files):
                keys = [k for k in a.files if k.split("|")[0] == label]
                ne = [k.split("|")[1] for k in keys if not np.array_equal(a[k], b[k], equal_nan=True)]
                nans = sum(int(np.isnan(a[k]).sum()) for k in keys if a[k].dtype.kind == "f")
                lines.append(f"{entry:7s} {label:60s} {len(keys)} outputs" + (f", {nans} NaN" if nans else "") + ": " +
                             ("equal" if not ne else f"NOT EQUAL (outputs {', '.join(ne)})"))
                bad += bool(ne)
    lines.append(f"# {len(lines) - 1} cases, {'all equal' if bad == 0 else f'{bad} differ'}")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.output:
        with open(args.output, "w") as f:
            f.write(text)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
