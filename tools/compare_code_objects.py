#!/usr/bin/env python3
"""Are two builds of libtds_hip.so's objects the same DEVICE code?  tools/compare_code_objects.py <obj dir A> <obj dir B> [-o report]

For every *.o of either directory the gfx950 code object is taken out of the fat binary (llvm-objcopy --dump-section
.hip_fatbin, clang-offload-bundler --unbundle: handles the compressed bundle) and compared PER KERNEL SYMBOL:
  * the disassembly (llvm-objdump -d --no-leading-addr; instruction text, encoding words and branch labels — the absolute
    address in the trailing comment and the zero padding that aligns the next function are dropped: emission order
    inside an object may differ), and
  * the kernel's entry in the metadata notes (llvm-readelf --notes: register counts, scratch, LDS, kernarg size, spills).
The sets of kernel names must be equal.  Functions that are no kernels (a lambda's ordinal may be renamed) are compared as
a multiset of bodies.  File hashes are NOT compared: they differ where the code does not.  No GPU, nothing is built here.
Exit status 0: every kernel of every unit equal."""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def code_object(obj, tmp):
    """path of the unbundled gfx950 code object of obj, or None where the object holds no device code"""
    fat = os.path.join(tmp, "fatbin")
    if os.path.exists(fat):
        os.remove(fat)
    subprocess.run([f"{LLVM}/llvm-objcopy", "--dump-section", f".hip_fatbin={fat}", obj, os.devnull],
                   capture_output=True, text=True)
    if not os.path.exists(fat) or os.path.getsize(fat) == 0:
        return None
    if TARGET not in run(f"{LLVM}/clang-offload-bundler", "--list", "--type=o", f"--input={fat}").split():
        return None
    co = os.path.join(tmp, "co")
    run(f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--targets={TARGET}", f"--input={fat}", f"--output={co}")
    return co


def functions(co):
    """{symbol: [instruction lines]} of the code object's .text"""
    out, cur = {}, None
    for line in run(f"{LLVM}/llvm-objdump", "-d", "--no-leading-addr", co).splitlines():
        m = re.match(r"^<(.+)>:$", line)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and line.strip():
            # "insn   // 000000001900: C00200C0 0000010C <label>" -> the address goes, the rest stays
            cur.append(re.sub(r"\s*//\s*[0-9A-Fa-f]+:", " //", line.strip()))
    # the zero words that align the NEXT function are no code of this one (objdump shows them as "..." or decodes a lone
    # zero dword; the last function of .text has none): they depend on the emission order only
    for body in out.values():
        while body and (body[-1] == "..." or re.search(r"// (00000000 ?)+$", body[-1])):
            body.pop()
    return out


def kernel_notes(co):
    """{kernel name: its entry of amdhsa.kernels, as text}"""
    text = run(f"{LLVM}/llvm-readelf", "--notes", co)
    out = {}
    if "amdhsa.kernels:" not in text:
        return out
    body = text.split("amdhsa.kernels:", 1)[1].split("amdhsa.target:", 1)[0]
    for entry in re.split(r"(?m)^  - ", body)[1:]:
        name = re.search(r"(?m)^\s*\.name:\s*(\S+)", entry).group(1)
        out[name] = entry
    return out


def compare_unit(a, b, tmp):
    """(kernels compared, [differences]) of the objects a and b"""
    sides = []
    for obj in (a, b):
        co = code_object(obj, tmp)
        sides.append((functions(co), kernel_notes(co)) if co else ({}, {}))
    (fa, na), (fb, nb) = sides
    diffs = []
    for k in sorted(set(na) - set(nb)):
        diffs.append(f"kernel only in A: {k}")
    for k in sorted(set(nb) - set(na)):
        diffs.append(f"kernel only in B: {k}")
    common = sorted(set(na) & set(nb))
    for k in common:
        if fa.get(k) != fb.get(k):
            la, lb = fa.get(k, []), fb.get(k, [])
            at = next((i for i, (x, y) in enumerate(zip(la, lb)) if x != y), min(len(la), len(lb)))
            diffs.append(f"disassembly differs: {k} ({len(la)} / {len(lb)} instructions, first at {at})")
        if na[k] != nb[k]:
            diffs.append(f"notes differ: {k}")
    # what is no kernel: equal as a multiset of bodies, whatever the names
    rest = [collections.Counter("\n".join(v) for s, v in f.items() if s not in n) for f, n in ((fa, na), (fb, nb))]
    if rest[0] != rest[1]:
        diffs.append(f"non-kernel functions differ ({sum(rest[0].values())} / {sum(rest[1].values())})")
    return len(common), diffs


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("dir_a")
    ap.add_argument("dir_b")
    ap.add_argument("-o", "--output")
    args = ap.parse_args()
    units = lambda d: {f for f in os.listdir(d) if f.endswith(".o")}
    ua, ub = units(args.dir_a), units(args.dir_b)
    lines, bad, total = [f"# device code of {args.dir_a} (A) against {args.dir_b} (B), per kernel symbol: disassembly + metadata notes"], 0, 0
    with tempfile.TemporaryDirectory() as tmp:
        for u in sorted(ua | ub):
            if u not in ua or u not in ub:
                # (a unit without device code may come or go: host code is not this tool's business)
                only = os.path.join(args.dir_a if u in ua else args.dir_b, u)
                co = code_object(only, tmp)
                n = len(kernel_notes(co)) if co else 0
                lines.append(f"{u:28s} only in {'A' if u in ua else 'B'}: {n} kernels" + ("" if n == 0 else "  NOT EQUAL"))
                bad += n != 0
                continue
            n, diffs = compare_unit(os.path.join(args.dir_a, u), os.path.join(args.dir_b, u), tmp)
            total += n
            lines.append(f"{u:28s} {n:4d} kernels compared: " + ("equal" if not diffs else "NOT EQUAL"))
            lines += [f"    {d}" for d in diffs]
            bad += bool(diffs)
    lines.append(f"# {total} kernels compared, {'all equal' if bad == 0 else f'{bad} units differ'}")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.output:
        with open(args.output, "w") as f:
            f.write(text)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
