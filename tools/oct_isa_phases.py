#!/usr/bin/env python3
"""Instructions between the OCTMARK comments of the 8-lane kernel's assembly (built with -DTDS_OCT_MARKS), per kernel.

A lone wavefront issues an instruction every ~4 (moves, DPP, scalar) to ~5.2 (f64) cycles whatever it depends on
(tools/ubench/lone_wave_latency.hip), so a phase that only issues runs at ~4.6 cycles per slot; what a phase takes above that is
LDS latency it has nothing to cover with (~70 cycles per dependent read).  Two columns show it:

  exposed   s_waitcnt lgkmcnt(n) with fewer than EXPOSED_SLOTS instruction slots since the youngest LDS / scalar read it
            waits for (the (n + 1)-th youngest outstanding operation: they return in order) — a round trip the wavefront sits out;
  cyc/slot  with --phases FILE (the output of tools/oct_profile.py): the stamped cycles of the main wavefront's phases over
            their slots, in a second table.

usage: tools/oct_isa_phases.py [kernel substring, default IddLb1ELi3 = f64 step-loop two-wavefront build]
                               [--phases profiles/oct_lds_before.txt] [--src other/tds_oct.hip]
                               [--define NAME=VALUE ...: further -D flags of an experiment build] [--asm marks.s: an assembly compiled before, not compiled here]"""
import argparse
import collections
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CS = os.path.join(ROOT, "tiny-differentiable-simulator_amd", "csrc")
EXPOSED_SLOTS = 12
# the stamped phases of the main wavefront (tools/oct_profile.py prints them in this order) and the marks they span
# (a mark with no instruction behind it in a build — main_FC, main_rootvel in some — has no line in the first table)
PHASES = [("PD, jcalc, root sincos, kinematics", ["main_top", "main_jcalc", "main_rootsincos", "main_rootvel", "main_legs", "main_publish_kin"]),
          ("D rigid inertias", ["main_rigid"]),
          ("E totals, G, H leg LDL^T", ["main_totals", "main_FC", "main_legldl"]),
          ("Schur sums, root block, 6 x 6 LDL^T", ["main_schur", "main_wait_schur", "main_Rblock", "main_ldl6"])]


def phase_cycles(path):
    """the first four phase lines of an oct_profile.py output: '  3708  PD, jcalc, ...'"""
    cyc = []
    for l in open(path):
        m = re.match(r"\s+(\d+)\s+(PD, jcalc|D rigid|E totals|Schur sums)", l)
        if m:
            cyc.append(int(m.group(1)))
    return cyc[:4]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("kernel", nargs="?", default="IddLb1ELi3")
    ap.add_argument("--phases", default=None)
    ap.add_argument("--src", default=os.path.join(CS, "tds_oct.hip"))
    ap.add_argument("--define", action="append", default=[], metavar="NAME=VALUE")
    ap.add_argument("--asm", default=None)
    args = ap.parse_args()
    if args.asm:
        txt = open(args.asm).read()
    else:
        with tempfile.TemporaryDirectory() as tmp:
            out = os.path.join(tmp, "oct_marks.s")
            subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"), "-I" + CS,
                                   "-Wno-unused-function", "-mllvm", "-disable-machine-licm", "-ffp-contract=on", "-DTDS_OCT_MARKS"] + ["-D" + d for d in args.define] +
                                  ["--cuda-device-only", "-S", "-o", out, args.src], stderr=subprocess.DEVNULL)
            txt = open(out).read()
    m = re.search(r"^(_Z\w*tds_oct_kernel" + args.kernel + r"\w*):.*?\n(.*?)^\.Lfunc_end\d+:", txt, re.S | re.M)
    body = m.group(2).split("\n")
    cur, counts = "(prologue)", collections.OrderedDict()
    slot = 0
    pending = []  # outstanding LDS / scalar-memory operations, oldest first: (slot, is a read)
    for l in body:
        t = l.strip()
        mm = re.match(r";\s*OCTMARK\s+(\S+)", t)
        if mm:
            cur = mm.group(1)
            continue
        if not l.startswith("\t"):  # a label: another path may join here, nothing is known to be outstanding
            if t.endswith(":"):
                pending = []
            continue
        if not t or t.startswith((".", ";")):
            continue
        op = t.split()[0]
        c = counts.setdefault(cur, collections.Counter())
        slot += 1
        c["total"] += 1
        c["valu"] += op.startswith("v_")
        c["ds"] += op.startswith("ds_")
        c["salu"] += op.startswith("s_")
        c["mem"] += op.startswith(("global_", "flat_", "scratch_"))
        c["dpp"] += ("dpp" in t or "quad_perm" in t or "row_" in t)
        c["wait"] += op == "s_waitcnt"
        if op.startswith("ds_") or op.startswith(("s_load", "s_buffer_load", "s_memtime", "s_memrealtime")):
            pending.append((slot, not op.startswith("ds_write")))
        elif op == "s_waitcnt":
            w = re.search(r"lgkmcnt\((\d+)\)", t)
            if w:
                n = int(w.group(1))
                done, pending = (pending[:len(pending) - n], pending[len(pending) - n:]) if n < len(pending) else ([], pending)
                reads = [s for s, rd in done if rd]
                if reads and slot - reads[-1] < EXPOSED_SLOTS:
                    c["exposed"] += 1
    print(m.group(1))
    print(f"{'after mark':22s} {'total':>6s} {'valu':>6s} {'ds':>5s} {'salu':>5s} {'mem':>4s} {'dpp':>4s} {'waits':>5s} {'exposed':>7s}")
    for k, c in counts.items():
        print(f"{k:22s} {c['total']:6d} {c['valu']:6d} {c['ds']:5d} {c['salu']:5d} {c['mem']:4d} {c['dpp']:4d} {c['wait']:5d} {c['exposed']:7d}")
    cyc = phase_cycles(args.phases) if args.phases else []
    print()
    print(f"{'main wavefront phase':38s} {'slots':>6s} {'waits':>5s} {'exposed':>7s} {'cycles':>7s} {'cyc/slot':>8s}")
    for i, (name, marks) in enumerate(PHASES):
        tot = sum(counts.get(k, {}).get("total", 0) for k in marks)
        wt = sum(counts.get(k, {}).get("wait", 0) for k in marks)
        ex = sum(counts.get(k, {}).get("exposed", 0) for k in marks)
        if i < len(cyc) and tot:
            print(f"{name:38s} {tot:6d} {wt:5d} {ex:7d} {cyc[i]:7d} {cyc[i] / tot:8.2f}")
        else:
            print(f"{name:38s} {tot:6d} {wt:5d} {ex:7d} {'-':>7s} {'-':>8s}")


if __name__ == "__main__":
    main()
