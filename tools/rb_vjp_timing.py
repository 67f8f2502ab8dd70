"""Times the reverse-mode rigid-body rollout derivative on the billiard scene (tests/rb_scenes.py): N = 4096 worlds,
300 steps, 50 solver iterations.  HIP events around every call, a warm-up call and then five calls per case:
tds_rb_vjp (one cotangent on s_T: every input's gradient), and in the same process tds_rb_step, tds_rb_jvp at k = 2 (one
shot gradient) and at k = 91 (the full state Jacobian).

    python tools/rb_vjp_timing.py [parent library]

With the path of a libtds_hip.so built from the parent commit, every call is timed from that library as well,
alternated call by call with this tree's: the columns show whether they have moved, and the parent's own spread over
its five calls is the margin.  RB_N, RB_STEPS, RB_TAPE_CAP (default 32768: the fixed shot's longest step
records 11 765 entries, the hardest of the random shots more) and RB_WORK_GIB (a comma-separated list of work-buffer bounds, default "8,32") change the run."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402

from rb_scenes import BILLIARD_TARGET_BALL, WHITE, billiard_model, billiard_state, shot_velocity  # noqa: E402
from tds_amd import hip_backend as hb  # noqa: E402

REPS = 5


class Handle:
    """a rigid-body handle of library L through the C ABI alone"""

    def __init__(self, L, m, n, s0):
        self.L, self.n = L, n
        L.tds_rb_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.tds_rb_set_stream.argtypes = [C.c_void_p, C.c_void_p]
        L.tds_rb_set_state.argtypes = [C.c_void_p, C.c_void_p]
        L.tds_rb_step.argtypes = [C.c_void_p, C.c_int]
        L.tds_rb_jvp.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                 C.c_void_p, C.c_void_p, C.c_void_p]
        L.tds_rb_vjp.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_size_t]
        L.tds_rb_last_error.restype = C.c_char_p
        self.h = C.c_void_p()
        self.check(L.tds_rb_create(C.byref(m), n, 0, 0, C.byref(self.h)))
        self.check(L.tds_rb_set_stream(self.h, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        self.check(L.tds_rb_set_state(self.h, np.ascontiguousarray(s0).ctypes.data))

    def check(self, rc):
        if rc != 0:
            raise RuntimeError(self.L.tds_rb_last_error().decode())

    def step(self, steps):
        self.check(self.L.tds_rb_step(self.h, steps))

    def jvp(self, x, v, steps, sT, jv):
        self.check(self.L.tds_rb_jvp(self.h, self.n, steps, x.data_ptr(), 0, None, None, v.shape[1], v.data_ptr(),
                                     sT.data_ptr(), jv.data_ptr()))


    def vjp(self, x, gs, steps, sT, gs0, cap, work_bytes):
        """one cotangent on the final state, no parameters"""
        self.check(self.L.tds_rb_vjp(self.h, self.n, steps, steps, x.data_ptr(), 0, None, None, gs.data_ptr(),
                                     sT.data_ptr(), gs0.data_ptr(), None, cap, work_bytes))


def one(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def timed(fns):
    """REPS calls of every function after a warm-up call each, alternated call by call: [ms] per function"""
    for fn in fns:
        one(fn)
    t = [[] for _ in fns]
    for _ in range(REPS):
        for i, fn in enumerate(fns):
            t[i].append(one(fn))
    return t


def show(name, t):
    t = sorted(t)
    print(f"{name:42s} median {t[len(t) // 2]:9.2f} ms   min {t[0]:9.2f}   max {t[-1]:9.2f}   "
          f"[{' '.join(f'{x:.2f}' for x in t)}]", flush=True)
    return t[len(t) // 2]


def main():
    n, steps = int(os.environ.get("RB_N", 4096)), int(os.environ.get("RB_STEPS", 300))
    cap = int(os.environ.get("RB_TAPE_CAP", 32768))
    budgets = [int(float(g) * (1 << 30)) for g in os.environ.get("RB_WORK_GIB", "8,32").split(",")]
    m = billiard_model()
    s0 = billiard_state(n)
    s0[:, WHITE, 7:9] = shot_velocity(np.random.default_rng(0).uniform([-100, 400], [100, 800], (n, 2)))
    ns = m.num_bodies * 13
    x = torch.from_numpy(s0).cuda()
    v2 = torch.zeros((n, 2, ns), dtype=torch.float64, device="cuda")
    v2[:, 0, WHITE * 13 + 7] = 1.0
    v2[:, 1, WHITE * 13 + 8] = 1.0
    vfull = torch.eye(ns, dtype=torch.float64, device="cuda").expand(n, ns, ns).contiguous()
    sT = torch.empty_like(x)
    jv2, jvf = torch.empty((n, 2, ns), dtype=torch.float64, device="cuda"), torch.empty_like(vfull)
    print(f"billiards x {n}, {steps} steps, {m.solver_iterations} solver iterations; {REPS} calls after a warm-up call")
    libs = [("this tree", Handle(hb.lib(), m, n, s0))]
    if len(sys.argv) > 1:
        libs.append(("parent", Handle(C.CDLL(os.path.abspath(sys.argv[1])), m, n, s0)))
    med = {}
    for case, call in (("tds_rb_step", lambda h: h.step(steps)),
                       ("tds_rb_jvp k = 2", lambda h: h.jvp(x, v2, steps, sT, jv2)),
                       (f"tds_rb_jvp k = {ns}", lambda h: h.jvp(x, vfull, steps, sT, jvf))):
        ts = timed([(lambda h=h: call(h)) for _, h in libs])
        for (name, _), t in zip(libs, ts):
            med[case, name] = show(f"{case}, {name}", t)
    gs = torch.zeros((n, 1, ns), dtype=torch.float64, device="cuda")
    gs[:, 0, BILLIARD_TARGET_BALL * 13:BILLIARD_TARGET_BALL * 13 + 3] = 1.0
    gs0 = torch.empty_like(x)
    best = None
    for wb in budgets:
        plan = hb.rb_vjp_plan(m, n, steps, 0, cap, wb)
        ts = timed([(lambda h=h: h.vjp(x, gs, steps, sT, gs0, cap, wb)) for _, h in libs])
        for (name, _), t in zip(libs, ts):
            v = show(f"tds_rb_vjp, {wb / (1 << 30):g} GiB: {plan[1]} worlds x {plan[2]} steps, {name}", t)
            if name == "this tree":
                best = v if best is None else min(best, v)
        print(f"    work buffer {plan[3] / 1e9:.2f} GB, tape capacity {plan[0]}")
    k2, kf = med["tds_rb_jvp k = 2", "this tree"], med[f"tds_rb_jvp k = {ns}", "this tree"]
    per_col = (kf - k2) / (ns - 2)
    print(f"forward mode costs {per_col:.2f} ms per further column past k = 2; one tds_rb_vjp ({best:.2f} ms) costs as "
          f"much as tds_rb_jvp at k = {2 + (best - k2) / per_col:.0f}")


if __name__ == "__main__":
    main()
