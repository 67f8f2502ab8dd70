#!/usr/bin/env python3
"""Draws the inverse-kinematics cases, runs the reference on them through tools/ik_golden (built from
tools/ik_golden.cpp as tools/README.md says) and writes tests/golden/ik_reference.npz.

    python tools/ik_golden.py <path to the ik_golden binary> <reference root>

A case whose branch margins or rank gap fail (see ik_golden.cpp) is dropped and drawn again with the next seed; the
file records how many were drawn and kept.  Targets are the body points' positions at a second, perturbed configuration
(reachable), computed with the project's own host kinematics; the unreachable cases are shifted on purpose: out of
the pendulum's plane by 5 cm, and beyond reach for the Ant and Laikago.  (A pendulum target metres away makes the pinv
iteration a chaotic map, steps of several radians, in which the reference and NumPy themselves part by 1e-7 in 20
iterations; such a case measures nothing.)"""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tds_amd  # noqa: E402
from tds_amd import hip_backend as hb  # noqa: E402

# model -> (urdf under the reference's data/, floating): what oracle/gen_golden.py's constructors load
URDF = {
    "pendulum5": ("pendulum5.urdf", 0), "cartpole": ("cartpole.urdf", 0), "ant": ("gym/ant_org_xyz_xyzrot.urdf", 0),
    "laikago": ("laikago/laikago_toes_zup_xyz_xyzrot.urdf", 0),
    "laikago_floating": ("laikago/laikago_toes_zup.urdf", 1), "ant_floating": ("gym/ant_org.urdf", 1),
}
METHODS = (hb.IK_TRANSPOSE, hb.IK_PINV, hb.IK_DAMPED_LM)
QMAX = 25  # q is padded to this many entries in the file
TOES = (3, 7, 11, 15)  # laikago_floating's toe links (fixed joints)


def world_points(m, q, links, pts):
    xw = hb.dynamics_host(m, q[None], want=("x_world",))["x_world"][0]
    return np.stack([xw[l, :9].reshape(3, 3) @ p + xw[l, 9:] for l, p in zip(links, pts)])


def draw(name, method, variant, seed):
    """one case as a dict; variant: 0 one target, 1 two targets + q_reference + off-origin points, 2 four targets,
    3 unreachable, 4 the feet of Laikago, 5 divergent transpose"""
    m = tds_amd.load_model(name)
    rng = np.random.default_rng(seed)
    g = np.load(os.path.join(ROOT, "tests", "golden", f"{name}.npz"))["x"]
    q0 = g[rng.integers(0, g.shape[0]), :m.dof_q].copy()
    qo = 7 if m.is_floating else 0
    if m.is_floating:
        if variant in (1, 2):  # a base rotated well away from the identity
            q0[:4] = rng.normal(size=4)
        q0[:4] /= np.linalg.norm(q0[:4])
    c = dict(model=name, method=method, max_it=20, lam=0.02, ttol=1e-3, stol=1e-8, alpha=0.5, wref=0.2, q_ref=None)
    nl = m.num_links
    k = {0: 1, 1: 2, 2: 4, 3: 1, 4: 4, 5: 1}[variant]
    if variant == 4:
        links = np.array(TOES if method != hb.IK_TRANSPOSE else TOES[:1])
        k = len(links)
    else:
        moving = [i for i in range(nl) if i >= min(nl - 1, 2)]
        links = rng.choice(moving, k, replace=len(moving) < k) if k > 1 else np.array([nl - 1])
    pts = np.zeros((k, 3)) if variant in (0, 4, 5) else rng.normal(0, 0.05, (k, 3))
    q1 = q0.copy()
    q1[qo:] += rng.normal(0, 0.15, m.dof_q - qo)
    tgt = world_points(m, q1, links, pts)
    if variant == 1:
        c["q_ref"] = q0 + np.concatenate([np.zeros(qo), rng.normal(0, 0.05, m.dof_q - qo)])
        c["wref"] = 0.1
    if variant == 3:
        if name == "pendulum5":  # out of the chain's plane: the axis along which no joint moves the point
            jac = hb.point_jacobian_host(m, q0[None], int(links[0]), pts[:1], local=True)[0]
            tgt = tgt + 0.05 * (np.abs(jac).sum(axis=1) < 1e-12)
        else:  # beyond the limbs' reach
            tgt = tgt + np.array([3.0, 2.0, 4.0])
        c["stol"] = 1e-2
    if variant == 4:  # a 3 cm step of every foot from the pose
        tgt = world_points(m, q0, links, pts) + np.array([0.03, 0.0, 0.0])
        c.update(alpha=0.3, wref=0.0)
    if method == hb.IK_TRANSPOSE:
        c["alpha"] = 5.0 if variant == 5 else 0.3
    c.update(k=k, links=np.asarray(links, dtype=np.int32), pts=pts, tgt=tgt, q0=q0)
    return c


def case_text(c):
    urdf, fl = URDF[c["model"]]
    nq = c["q0"].shape[0]
    f = lambda a: " ".join(repr(float(v)) for v in np.asarray(a).reshape(-1))  # noqa: E731
    s = (f"{urdf} {fl} {c['method']} {c['k']} {c['max_it']} {c['lam']!r} {c['ttol']!r} {c['stol']!r} {c['alpha']!r} "
         f"{c['wref']!r} {int(c['q_ref'] is not None)} {nq} {f(c['q0'])} ")
    if c["q_ref"] is not None:
        s += f(c["q_ref"]) + " "
    for j in range(c["k"]):
        s += f"{int(c['links'][j])} {f(c['pts'][j])} {f(c['tgt'][j])} "
    return s + "\n"


def main(binary, ref_root):
    plan = []
    for name in URDF:
        m = tds_amd.load_model(name)
        for method in METHODS:
            for variant in (0, 1, 2, 3):
                if variant == 3 and (name, method) not in (("pendulum5", hb.IK_PINV), ("ant", hb.IK_DAMPED_LM),
                                                           ("laikago_floating", hb.IK_TRANSPOSE)):
                    continue
                plan.append((name, method, variant))
            if name == "laikago_floating":
                plan.append((name, method, 4))
        del m
    plan.append(("pendulum5", hb.IK_TRANSPOSE, 5))
    kept, drawn = [], 0
    for i, (name, method, variant) in enumerate(plan):
        for attempt in range(20):
            c = draw(name, method, variant, 1000 * i + attempt)
            drawn += 1
            out = subprocess.run([binary, ref_root], input=case_text(c), capture_output=True, text=True, check=True).stdout
            out = [ln for ln in out.splitlines() if ln.startswith("IK ")][-1].split()[1:]
            nq = c["q0"].shape[0]
            c.update(status=int(out[0]), iter=int(out[1]), residual=float(out[2]), q=np.array(out[3:3 + nq], dtype=float))
            if out[3 + nq] == "1" and out[4 + nq] == "1" and np.all(np.isfinite(c["q"])):
                kept.append(c)
                break
        else:
            raise SystemExit(f"no case kept for {name} {method} {variant}")
        print(name, method, variant, "attempts", attempt + 1, "status", c["status"], "iter", c["iter"], "res %.3g" % c["residual"])
    n = len(kept)

    def pad(key, shape):
        a = np.zeros((n,) + shape)
        for i, c in enumerate(kept):
            v = np.asarray(c[key] if c[key] is not None else 0.0, dtype=float)
            a[(i,) + tuple(slice(0, s) for s in v.shape)] = v
        return a

    np.savez_compressed(
        os.path.join(ROOT, "tests", "golden", "ik_reference.npz"),
        model=np.array([c["model"] for c in kept]), method=np.array([c["method"] for c in kept], dtype=np.int32),
        k=np.array([c["k"] for c in kept], dtype=np.int32), links=pad("links", (4,)).astype(np.int32),
        body_points=pad("pts", (4, 3)), targets=pad("tgt", (4, 3)), q_init=pad("q0", (QMAX,)),
        have_ref=np.array([c["q_ref"] is not None for c in kept]), q_ref=pad("q_ref", (QMAX,)),
        # max_iterations, lambda, target_tolerance, step_tolerance, alpha, weight_reference
        options=np.array([[c["max_it"], c["lam"], c["ttol"], c["stol"], c["alpha"], c["wref"]] for c in kept]),
        q=pad("q", (QMAX,)), iterations=np.array([c["iter"] for c in kept], dtype=np.int32),
        status=np.array([c["status"] for c in kept], dtype=np.int32), residual=np.array([c["residual"] for c in kept]),
        drawn=np.int32(drawn), kept=np.int32(n))
    print("kept", n, "of", drawn, "drawn; status counts", np.bincount([c["status"] for c in kept], minlength=3))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
