#!/usr/bin/env python3
"""TEST INFRASTRUCTURE.  Generates tests/golden/rb_contacts.npz from the REAL reference (oracle/_ref/libtds_ref.so) for
the directed rigid-body scenes of tests/rb_contact_scenes.py.  Per scene:
  y64_<s>      the reference's double World::step, 1 step                                   float64 [N, nb, 13]
  y64x10_<s>   ... 10 steps (the heap scenes only)                                           float64
  y32_<s>      the reference's own float World::step (oracle/ref_harness_f32.cpp), 1 step    float32
  fired64_<s>, fired32_<s>   per world: the result differs from the same model with solver_iterations = 0
  u64_<s>, u32_<s>           the spread U of the C oracle's one-step result under input roundings of that format
                             (rb_contact_scenes.perturbation_spread)
  hash_<s>     sha256 of the scene's inputs (model struct and state)
and C, the factor of the tests' bounds C * U:  C = 2 * max over scenes and compared worlds of |y32 - y64| / U_32, rounded
up to a power of two — how many input roundings the reference's own float arithmetic is worth, times 2 for another
operation order (FMA contraction, reciprocal-multiply).  A world whose fired mask differs between the float and the
double reference sits on a branch threshold and is left out of float comparisons; at most 10 % of a scene.
Run where the reference tree exists:  python oracle/gen_golden_rb.py"""
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oraclelib  # noqa: E402
import reflib  # noqa: E402
import rb_contact_scenes as sc  # noqa: E402

EPS32, EPS64 = float(np.finfo(np.float32).eps), float(np.finfo(np.float64).eps)


def fired(step, name, y):
    m0, st, _ = sc.scene(name, iters=0)
    return np.any(step(m0, st, 1) != y, axis=(1, 2))


def main():
    out, worst = {}, 0.0
    for name in sc.NAMES:
        m, st, _ = sc.scene(name)
        y64 = reflib.rb_step(m, st, 1)
        y32 = reflib.rb_step_f32(m, st, 1)
        assert y32.dtype == np.float32 and np.isfinite(y64).all() and np.isfinite(y32).all(), name
        assert np.array_equal(oraclelib.rb_step(m, st, 1), y64), name      # the C oracle IS the reference, bit for bit
        f64, f32 = fired(reflib.rb_step, name, y64), fired(reflib.rb_step_f32, name, y32)
        u64 = sc.perturbation_spread(oraclelib.rb_step, m, st, EPS64)
        u32 = sc.perturbation_spread(oraclelib.rb_step, m, st, EPS32)
        keep = f64 == f32
        ratio = float(np.abs(y32.astype(np.float64) - y64)[keep].max() / u32)
        worst = max(worst, ratio)
        out.update({"y64_" + name: y64, "y32_" + name: y32, "fired64_" + name: f64, "fired32_" + name: f32,
                    "u64_" + name: u64, "u32_" + name: u32, "hash_" + name: sc.digest(m, st)})
        if name in sc.HEAPS:
            out["y64x10_" + name] = reflib.rb_step(m, st, 10)
            assert np.array_equal(oraclelib.rb_step(m, st, 10), out["y64x10_" + name]), name
        excl = 1.0 - keep.mean()
        print(f"{name:22s} {sc.KIND[name]:4s} fired {f64.mean():5.0%}  excluded {excl:5.1%}  U_64 {u64:.2e}  U_32 {u32:.2e}"
              f"  |ref_f32 - ref_f64| / U_32 {ratio:6.2f}")
        assert excl <= 0.10, (name, excl)
        assert f64.mean() >= 0.5 if sc.KIND[name] in ("hit", "heap") else True, (name, f64.mean())
        assert not f64.any() if sc.KIND[name] == "skip" else True, name
    c = 2.0 ** math.ceil(math.log2(2.0 * worst))
    out["C"] = c
    print(f"C = {c:g}  (2 x {worst:.2f}, rounded up to a power of two)")
    path = os.path.join(ROOT, "tests", "golden", "rb_contacts.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
