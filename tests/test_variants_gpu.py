"""GPU: per-environment model variants (HipSim.set_model_variants) — every environment steps under its own variant of the
model, through every stepping path: forward_zero, step, step_many (loop and graphs), the record rings, the rollout, the
forced reset; in double, float-record and pure float handles; and what is refused.

N = 70 environments: a partial last wavefront at 16 lanes (4 environments per wavefront) and at 32 (2), and no multiple
of 8 for the kernels that decline.  "The model of variant v" is params_apply(m, SEL, theta[v]): the checkers are the
double step on the CPU (hb.step_host), the parameter derivatives' y on the device (sim.jvp_params), ordinary handles
created from the applied models, and the reference."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, rel_err

import tds_amd
from tds_amd import hip_backend as hb

pytestmark = pytest.mark.gpu

N = 70
# two separately compiled builds of one step: agreement to round-off (tests/test_general_builds.py: LOOP_TOL)
TOL = 1e-9
GENERAL = {"oct": 0, "quad": 0, "chain": 0}

# a handful of entries per model: link mass, com, inertia (diagonal and off-diagonal), xt_trans, stiffness, damping,
# gravity, friction, restitution, + the base kinds on the floating models.  Links outside the root chain of the Ant and
# Laikago (a mass or a spring there changes the model's structure: tests/test_variants_cpu.py)
SEL = {
    "ant": [("mass", 7), ("com", 8, 1), ("inertia", 9, 3), ("xt_trans", 10, 0), ("stiffness", 11), ("damping", 12),
            ("gravity", 2), ("friction",), ("restitution",)],
    "laikago": [("mass", 6), ("com", 7, 1), ("inertia", 8, 3), ("xt_trans", 10, 0), ("xt_trans", 9, 2), ("stiffness", 11),
                ("damping", 12), ("gravity", 2), ("friction",), ("restitution",)],
    "cartpole": [("mass", 1), ("com", 1, 0), ("inertia", 1, 1), ("xt_trans", 1, 2), ("stiffness", 1), ("damping", 0),
                 ("gravity", 2), ("friction",), ("restitution",)],
    "pendulum5_plane": [("mass", 2), ("com", 4, 1), ("inertia", 3, 2), ("xt_trans", 2, 1), ("stiffness", 1), ("damping", 3),
                        ("gravity", 0), ("gravity", 2), ("friction",), ("restitution",)],
    "ant_floating": [("base_mass",), ("base_com", 1), ("base_inertia", 4), ("mass", 2), ("com", 3, 1), ("inertia", 4, 3),
                     ("xt_trans", 5, 0), ("stiffness", 6), ("damping", 7), ("gravity", 2), ("friction",), ("restitution",)],
    "cube_floating": [("base_mass",), ("base_com", 0), ("base_inertia", 1), ("base_inertia", 3), ("gravity", 2),
                      ("friction",), ("restitution",)],
}
OWN_KERNEL = {"ant": "oct8", "laikago": "quad16", "cartpole": "chain8", "pendulum5_plane": "general",
              "ant_floating": "general", "cube_floating": "general"}


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def draw_theta(m, sel, n, seed=7):
    """+- 5 % relative, + +- 0.01 additive except on inertias (as tests/test_param_derivs_cpu.py)"""
    base = hb.params_get(m, sel)
    rng = np.random.default_rng(seed)
    additive = np.array([not q[0].endswith("inertia") for q in sel])
    return base * (1.0 + 0.05 * rng.uniform(-1, 1, (n, len(sel)))) + 0.01 * rng.uniform(-1, 1, (n, len(sel))) * additive


_CASES = {}


def case(name):
    """per model, computed once: the model, N golden states, theta [N, p], a shuffled map onto three variants, and the
    CPU references — ref_own[e] = environment e under theta[e]; ref_3[v] = every environment under theta[v], v < 3"""
    if name not in _CASES:
        m = tds_amd.load_model(name)
        g = np.load(os.path.join(GOLDEN, name + ".npz"))["x"]
        rng = np.random.default_rng(12)
        x = np.ascontiguousarray(g[rng.integers(0, g.shape[0], N)])
        sel = SEL[name]
        theta = draw_theta(m, sel, N)
        map3 = rng.permutation(np.arange(N) % 3).astype(np.int32)
        ref_own = np.stack([hb.step_host(hb.params_apply(m, sel, theta[e]), x[e:e + 1])[0] for e in range(N)])
        ref_3 = np.stack([hb.step_host(hb.params_apply(m, sel, theta[v]), x) for v in range(3)])
        assert np.max(np.abs(ref_own - hb.step_host(m, x))) > 0  # (theta does move the step)
        _CASES[name] = dict(m=m, x=x, sel=sel, theta=theta, map3=map3, ref_own=ref_own, ref_3=ref_3)
    return _CASES[name]


def rows_of(ref_3, map3):
    return ref_3[map3, np.arange(map3.shape[0])]


@pytest.mark.parametrize("name", list(SEL))
def test_each_environment_steps_its_own_model(name, built):
    torch = _torch()
    c = case(name)
    m, sel, theta, map3 = c["m"], c["sel"], c["theta"], c["map3"]
    x = torch.from_numpy(c["x"]).cuda()
    sim = hb.HipSim(m, N)
    assert sim.single_step_kernel()[0] == OWN_KERNEL[name] and sim.num_model_variants == 0
    y_before = sim.forward_zero(x).clone()
    for v, ev, th_rows, ref in ((N, None, theta, c["ref_own"]),
                                (3, map3, theta[map3], rows_of(c["ref_3"], map3)),
                                (1, np.zeros(N, dtype=np.int32), np.tile(theta[:1], (N, 1)), c["ref_3"][0])):
        # (theta as a numpy array, and as a device tensor)
        sim.set_model_variants(sel, theta[:v] if v != 3 else torch.from_numpy(theta[:3]).cuda(), ev)
        assert sim.num_model_variants == v and sim.single_step_kernel()[0] == "general"
        y = sim.forward_zero(x).clone()
        y_par = sim.jvp_params(x, torch.from_numpy(np.ascontiguousarray(th_rows)).cuda(), sel)
        e_host = rel_err(y.cpu().numpy(), ref)
        e_par = rel_err(y.cpu().numpy(), y_par.cpu().numpy())
        print(f"{name} V={v}: vs step_host of the applied models {e_host:.2e}, vs jvp_params on the device {e_par:.2e}")
        assert e_host <= TOL and e_par <= TOL, (name, v, e_host, e_par)
        if v == 3:  # three ordinary handles created from the applied models, on the general kernel
            for k in range(3):
                ordinary = hb.HipSim(hb.params_apply(m, sel, theta[k]), N, options=GENERAL)
                assert ordinary.single_step_kernel()[0] == "general"
                rows = np.flatnonzero(map3 == k)
                e_ord = rel_err(y[rows].cpu().numpy(), ordinary.forward_zero(x)[rows].cpu().numpy())
                print(f"{name} V=3 variant {k}: vs an ordinary handle of the applied model {e_ord:.2e}")
                assert e_ord <= TOL, (name, k, e_ord)
                ordinary.close()
    sim.clear_model_variants()
    assert sim.num_model_variants == 0 and sim.single_step_kernel()[0] == OWN_KERNEL[name]
    assert torch.equal(sim.forward_zero(x), y_before)
    sim.close()


def test_ant_variants_against_the_reference(built):
    """one reference simulator per variant with gravity, friction, restitution and a link's spring set to theta_v: the
    Ant rows of each variant stay within the project's gate"""
    import reflib
    if not reflib.available():
        pytest.skip("the reference library is not built here")
    import gen_golden

    torch = _torch()
    c = case("ant")
    m, x = c["m"], c["x"]
    sel = [("gravity", 2), ("friction",), ("restitution",), ("stiffness", 11), ("damping", 11)]
    theta = draw_theta(m, sel, 3, seed=9)
    theta[:, 2] = np.abs(theta[:, 2])  # (a restitution in [0, 1))
    map3 = c["map3"]
    sim = hb.HipSim(m, N)
    sim.set_model_variants(sel, theta, map3)
    y = sim.forward_zero(torch.from_numpy(x).cuda()).cpu().numpy()
    sim.close()
    for v in range(3):
        r, _ = gen_golden.make_ref("ant")
        try:
            r.set_gravity([m.gravity[0], m.gravity[1], theta[v, 0]])
            r.set_solver(m.cfm, m.erp, m.pgs_iterations, theta[v, 1], theta[v, 2])
            r.set_link_spring(11, theta[v, 3], theta[v, 4])
            rows = np.flatnonzero(map3 == v)
            err = rel_err(y[rows], r.step(x[rows]))
        finally:
            r.close()
        print(f"ant variant {v} ({rows.size} rows) vs the reference: {err:.2e}")
        assert err <= 1e-6, (v, err)


def chained(sim, x0, acts, nqd):
    """three chained forward_zero steps from x0 with the action block of each step: the y of every step"""
    x, ys = x0.clone(), []
    adim = acts.shape[2]
    for k in range(acts.shape[0]):
        x[:, nqd:nqd + adim] = acts[k]
        y = sim.forward_zero(x).clone()
        x[:, :nqd] = y[:, :nqd]
        ys.append(y)
    return ys


def test_every_launch_form_runs_the_variants(built):
    torch = _torch()
    c = case("ant")
    m, sel, theta, map3 = c["m"], c["sel"], c["theta"], c["map3"]
    nqd, steps = m.dof_q + m.dof_qd, 3
    x0 = torch.from_numpy(c["x"]).cuda()
    rng = np.random.default_rng(21)
    acts = torch.from_numpy(rng.uniform(-0.4, 0.4, (steps, N, m.action_dim))).cuda().contiguous()
    same = acts[:1].expand(steps, N, m.action_dim).contiguous()
    sim = hb.HipSim(m, N)

    def run_step_many(loop):
        sim.set_option("step_many_loop", loop)
        assert sim.step_many_is_loop(steps) == bool(loop)
        sim.x.copy_(x0)
        sim.step_many(acts, steps)
        return sim.y.clone()

    # ---- before installing: the handle's own kernel, graphs cached
    before = {loop: run_step_many(loop) for loop in (1, 0)}
    ref0 = chained(sim, x0, acts, nqd)
    for loop in (1, 0):
        assert rel_err(before[loop].cpu().numpy(), ref0[-1].cpu().numpy()) <= TOL
    # ---- installed
    sim.set_model_variants(sel, theta[:3], map3)
    ref = chained(sim, x0, acts, nqd)
    ref_same = chained(sim, x0, same, nqd)
    # (forward_zero under the variants is what test_each_environment_steps_its_own_model holds to the CPU step)
    assert rel_err(ref[-1].cpu().numpy(), ref0[-1].cpu().numpy()) > 1e-6  # (the variants do move three steps)
    sim.x.copy_(x0)
    sim.step(acts[0], substeps=steps)
    e = rel_err(sim.y.cpu().numpy(), ref_same[-1].cpu().numpy())
    print(f"step(substeps=3): {e:.2e}")
    assert e <= TOL and rel_err(sim.x[:, :nqd].cpu().numpy(), ref_same[-1][:, :nqd].cpu().numpy()) <= TOL
    for loop in (1, 0):  # step_many as one step-loop launch, and as chained graphs of single steps
        e = rel_err(run_step_many(loop).cpu().numpy(), ref[-1].cpu().numpy())
        print(f"step_many, step_many_loop = {loop}: {e:.2e}")
        assert e <= TOL, (loop, e)
        # per-step rings: every slot
        obs_ring = torch.zeros((steps, N, nqd + 2), dtype=torch.float64, device="cuda")
        y_ring = torch.zeros((steps, N, m.output_dim), dtype=torch.float64, device="cuda")
        sim.x.copy_(x0)
        sim.step_many_rings(acts, steps, obs_ring=obs_ring, y_ring=y_ring)
        torch.cuda.synchronize()
        for k in range(steps):
            e = rel_err(y_ring[k].cpu().numpy(), ref[k].cpu().numpy())
            e_obs = rel_err(obs_ring[k][:, 2:nqd].cpu().numpy(), ref[k][:, 2:nqd].cpu().numpy())
            print(f"step_many_rings, step_many_loop = {loop}, slot {k}: y {e:.2e}, obs {e_obs:.2e}")
            assert e <= TOL and e_obs <= TOL, (loop, k, e, e_obs)
        # ... reward and done included: against ordinary handles of the applied models, each variant's own rows
        for v in range(3):
            ordinary = hb.HipSim(hb.params_apply(m, sel, theta[v]), N, options=GENERAL)
            ordinary.set_option("step_many_loop", loop)
            o_ring = torch.zeros_like(obs_ring)
            ordinary.x.copy_(x0)
            ordinary.step_many_rings(acts, steps, obs_ring=o_ring)
            torch.cuda.synchronize()
            rows = np.flatnonzero(map3 == v)
            e = rel_err(obs_ring[:, rows].cpu().numpy(), o_ring[:, rows].cpu().numpy())
            assert e <= TOL, (loop, v, e)
            ordinary.close()
    # ---- cleared: the cached graphs of the variants must not survive either
    sim.clear_model_variants()
    for loop in (1, 0):
        assert torch.equal(run_step_many(loop), before[loop]), loop
    sim.close()


def test_rollout_and_forced_reset_under_the_variants(built):
    torch = _torch()
    c = case("ant")
    m, sel, theta, map3 = c["m"], c["sel"], c["theta"], c["map3"]
    nqd, steps = m.dof_q + m.dof_qd, 3
    x0 = torch.from_numpy(c["x"]).cuda()
    rng = np.random.default_rng(22)
    sim = hb.HipSim(m, N)
    sim.set_model_variants(sel, theta[:3], map3)
    policy = torch.from_numpy(0.05 * rng.normal(size=(N, sim.policy_num_parameters))).cuda().contiguous()
    mask = torch.from_numpy((rng.uniform(size=N) < 0.5).astype(np.uint8)).cuda()
    assert 0 < int(mask.sum()) < N and m.settle_steps > 0

    def run(s):
        """(return, steps, state after the rollout), (state, observation after a forced reset of the masked ones)"""
        s.x.copy_(x0)
        ret, cnt = s.rollout(policy, steps)
        after = s.x.clone()
        obs = torch.zeros((N, nqd + 2), dtype=torch.float64, device="cuda")
        s.reset(mask, obs)
        torch.cuda.synchronize()
        return ret, cnt, after, s.x.clone(), obs

    got = run(sim)
    base = hb.HipSim(m, N, options=GENERAL)
    plain = run(base)
    base.close()
    assert rel_err(got[2].cpu().numpy(), plain[2].cpu().numpy()) > 1e-6  # (the variants do move the rollout)
    for v in range(3):
        ordinary = hb.HipSim(hb.params_apply(m, sel, theta[v]), N, options=GENERAL)  # (same seed, same reset counts)
        want = run(ordinary)
        ordinary.close()
        rows = np.flatnonzero(map3 == v)
        assert torch.equal(got[1][rows], want[1][rows])
        errs = [rel_err(a[rows].cpu().numpy(), b[rows].cpu().numpy()) for a, b in zip(got, want) if a.dtype == torch.float64]
        print(f"variant {v}: return / state after the rollout / state, obs after the reset: {['%.2e' % e for e in errs]}")
        assert max(errs) <= TOL, (v, errs)
    sim.close()


# float records: double arithmetic that agrees to TOL, rounded to float — one unit in the last place of a float where the
# two doubles straddle a rounding boundary (2^-23 relative).  Pure float: the gate tests/test_f32.py holds an f32 build
# to, 4 x the reference's own float-against-double error on the model + 1e-6 (tests/golden/f32_reference.npz: the Ant).
MIXED_TOL = 2.0 ** -23 + TOL


@pytest.mark.parametrize("name", ["ant", "ant_floating"])
@pytest.mark.parametrize("dtype", ["f32", "mixed"])
def test_float_handles_step_the_variants(name, dtype, built):
    torch = _torch()
    c = case(name)
    m, sel, theta, map3 = c["m"], c["sel"], c["theta"], c["map3"]
    f = np.load(os.path.join(GOLDEN, "f32_reference.npz"))
    tol = MIXED_TOL if dtype == "mixed" else 4.0 * rel_err(f["ant_y32"], f["ant_y64"]) + 1e-6
    x = torch.from_numpy(c["x"].astype(np.float32)).cuda()
    sim = hb.HipSim(m, N, dtype=dtype)
    sim.set_model_variants(sel, theta[:3], map3)
    assert sim.single_step_kernel()[0] == "general"
    y = sim.forward_zero(x).clone()
    assert y.dtype == torch.float32
    sim.close()
    for v in range(3):
        ordinary = hb.HipSim(hb.params_apply(m, sel, theta[v]), N, dtype=dtype, options=GENERAL)
        rows = np.flatnonzero(map3 == v)
        e = rel_err(y[rows].double().cpu().numpy(), ordinary.forward_zero(x)[rows].double().cpu().numpy())
        print(f"{name} {dtype} variant {v}: vs an ordinary {dtype} handle of the applied model {e:.2e} (bound {tol:.2e})")
        assert e <= tol, (name, dtype, v, e)
        ordinary.close()


def test_refusals(built):
    _torch()
    c = case("ant")
    m, sel, theta, map3 = c["m"], c["sel"], c["theta"], c["map3"]
    sim = hb.HipSim(m, N)
    sim.set_auto_reset(True, seed=3)
    with pytest.raises(hb.TdsHipError, match="auto-reset") as e:
        sim.set_model_variants(sel, theta[:3], map3)
    assert "tds_hip error 2:" in str(e.value) and sim.num_model_variants == 0
    sim.set_auto_reset(False)
    sim.set_model_variants(sel, theta[:3], map3)
    with pytest.raises(hb.TdsHipError, match="auto-reset") as e:
        sim.set_auto_reset(True, seed=3)
    assert "tds_hip error 2:" in str(e.value)
    bad = map3.copy()
    bad[N - 1] = 3
    for th, ev, match in ((theta[:3], bad, "maps to variant"), (theta[:3], None, "no environment map"),
                          (np.tile(theta, (2, 1)), np.zeros(N), "variants for 70 environments")):
        with pytest.raises(hb.TdsHipError, match=match) as e:
            sim.set_model_variants(sel, th, ev)
        assert "tds_hip error 1:" in str(e.value) and sim.num_model_variants == 3  # (a refused call changes nothing)
    with pytest.raises(hb.TdsHipError, match=r"variant 1 .*\(field root_last\)") as e:
        sim.set_model_variants([("mass", 2)], np.array([[0.0], [0.3]]), np.arange(N) % 2)
    assert "tds_hip error 1:" in str(e.value)
    sim.close()
    for name in ("pendulum5_spherical", "three_pendulums_plane"):
        mm = tds_amd.load_model(name)
        s = hb.HipSim(mm, 8)
        with pytest.raises(hb.TdsHipError, match="not supported") as e:
            s.set_model_variants([("mass", 0)], np.ones((8, 1)))
        assert "tds_hip error 2:" in str(e.value)
        s.close()
