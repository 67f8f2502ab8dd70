"""Reverse-mode derivatives of rigid-body rollouts on the CPU (tds_rb_vjp_host, the checker of the device path): against
forward mode column by column, against central differences of the reference, the primal, the cotangent's handling,
tape overflow, refusals, and the host code under the sanitizers (tools/rb_vjp_sanitize.cpp)."""
import ctypes as C
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import reflib
from conftest import ROOT
from rb_scenes import (BILLIARD_TARGET, BILLIARD_TARGET_BALL, MIXED_ORDER, WHITE, billiard_cost, billiard_model,
                       billiard_state, make_mixed_worlds, make_worlds, shot_velocity)

from tds_amd import hip_backend as hb

# Reverse and forward mode are exact derivatives of one executed algorithm and differ in summation order only.  The
# worst error measured on the CPU, relative to the world's largest entry: 2.2e-15 over test_reverse_matches_forward's
# scenes (billiard, 40 steps, every = 40) and 7.7e-15 on the 300-step billiard roll of
# test_billiard_300_steps_all_inputs.  The bound is ten times the worst, far inside the 1e-9 it may not be looser than.
REV_FWD_BOUND = 8e-14
N = 3


@functools.lru_cache(maxsize=None)
def scene(name):
    """(model, s0 [N], steps, params, theta [N, p]): one selection of each of the four kinds, theta per world"""
    if name == "billiard":
        m = billiard_model()
        s0 = billiard_state(N)
        s0[:, WHITE, 7:9] = shot_velocity([[10.0, 600.0], [-40.0, 550.0], [25.0, 700.0]])
        steps, params = 40, [("mass", 6), ("gravity", 1), ("friction",), ("restitution",)]
    elif name == "mixed":
        m, s0 = make_mixed_worlds(N, 21, MIXED_ORDER)
        steps, params = 8, [("mass", 3), ("gravity", 2), ("friction",), ("restitution",)]
    else:
        m, s0 = make_worlds(N, 7, plane_last=name == "plane_last")
        steps, params = 12, [("mass", 1 if name == "plane_last" else 2), ("gravity", 2), ("friction",),
                             ("restitution",)]
    th = hb.rb_params_get(m, params) + 0.05 * (1 + np.random.default_rng(2).random((N, len(params))))
    return m, s0, steps, params, th


@functools.lru_cache(maxsize=None)
def forward_jacobians(name):
    """J_r [N, ns + p, ns] = d s_r / d [s0 | theta] for r = 1 .. steps, from rb_jvp_host over all unit directions"""
    m, s0, steps, params, th = scene(name)
    ns, p = m.num_bodies * 13, len(params)
    v = np.broadcast_to(np.eye(ns + p), (N, ns + p, ns + p))
    return [hb.rb_jvp_host(m, s0, r, v, params, th)[1].reshape(N, ns + p, ns) for r in range(1, steps + 1)]


def world_err(got, ref):
    """max over worlds of max |got - ref| / the world's largest |ref|"""
    got, ref = got.reshape(N, -1), ref.reshape(N, -1)
    return float((np.abs(got - ref).max(1) / np.abs(ref).max(1)).max())


@pytest.mark.parametrize("name", ["plane_first", "plane_last", "mixed", "billiard"])
def test_reverse_matches_forward(name, built):
    m, s0, steps, params, th = scene(name)
    ns, p = m.num_bodies * 13, len(params)
    J = forward_jacobians(name)
    for every in (1, steps):
        n_rec = steps // every
        gs = np.random.default_rng(steps + every).normal(size=(N, n_rec, ns))
        s, gs0, gth = hb.rb_vjp_host(m, s0, steps, gs, params, th, every)
        ref = sum(np.einsum("nkj,nj->nk", J[(r + 1) * every - 1], gs[:, r]) for r in range(n_rec))
        e = world_err(np.concatenate([gs0.reshape(N, ns), gth], 1), ref)
        print(f"{name} every={every}: reverse against forward {e:.2e}")
        assert e <= REV_FWD_BOUND, (name, every, e)
        assert np.all(np.abs(gth).max(0) > 0)                        # every selected kind reaches the states


def test_billiard_300_steps_all_inputs(built):
    """the gradient of the cost in all 91 initial-state entries and the seven masses, one reverse call against the 98
    forward columns"""
    m = billiard_model()
    steps, params = 300, [("mass", b) for b in range(7)]
    s0 = billiard_state(1)
    s0[:, WHITE, 7:9] = shot_velocity([[10.0, 600.0]])
    sT, jv = hb.rb_jvp_host(m, s0, steps, np.eye(98)[None], params)
    for gs in (np.random.default_rng(1).normal(size=(1, 91)), None):
        if gs is None:
            gs = np.zeros((1, 7, 13))
            gs[0, BILLIARD_TARGET_BALL, :3] = 2 * (sT[0, BILLIARD_TARGET_BALL, :3] - BILLIARD_TARGET)
        _, gs0, gth = hb.rb_vjp_host(m, s0, steps, gs, params)
        ref = jv[0].reshape(98, 91) @ gs.reshape(-1)
        got = np.concatenate([gs0.reshape(-1), gth.reshape(-1)])
        e = np.abs(got - ref).max() / np.abs(ref).max()
        print(f"billiard, 300 steps, 98 inputs: reverse against forward {e:.2e}")
        assert e <= REV_FWD_BOUND


@pytest.mark.skipif(not reflib.available(), reason="reference library not built (oracle/_ref)")
def test_billiard_shot_gradient_matches_reference_differences(built):
    m = billiard_model()
    steps = 300
    s0 = billiard_state(1)
    s0[:, WHITE, 7:9] = shot_velocity([[10.0, 600.0]])
    sT = hb.rb_jvp_host(m, s0, steps)
    gs = np.zeros((1, 7, 13))
    gs[0, BILLIARD_TARGET_BALL, :3] = 2 * (sT[0, BILLIARD_TARGET_BALL, :3] - BILLIARD_TARGET)   # d cost / d s_T
    _, gs0, _ = hb.rb_vjp_host(m, s0, steps, gs)
    h = 1e-6
    for c in range(2):
        a, b = s0.copy(), s0.copy()
        a[0, WHITE, 7 + c] += h
        b[0, WHITE, 7 + c] -= h
        fd = (billiard_cost(reflib.rb_step(m, a, steps)) - billiard_cost(reflib.rb_step(m, b, steps)))[0] / (2 * h)
        print(f"billiard d cost / d v{'xy'[c]}: reverse {gs0[0, WHITE, 7 + c]:.9f}, reference difference {fd:.9f}")
        assert abs(gs0[0, WHITE, 7 + c] - fd) <= 1e-5 * max(abs(fd), 1.0)


@pytest.mark.parametrize("name", ["plane_first", "billiard"])
def test_primal_is_the_forward_calls(name, built):
    m, s0, steps, params, th = scene(name)
    ns = m.num_bodies * 13
    s_T, _, _ = hb.rb_vjp_host(m, s0, steps, np.zeros((N, 1, ns)), params, th)
    assert s_T.shape == (N, 1, m.num_bodies, 13)
    assert np.array_equal(s_T[:, 0], hb.rb_jvp_host(m, s0, steps, None, params, th))
    s_all, _, _ = hb.rb_vjp_host(m, s0, steps, np.zeros((N, steps, ns)), params, th, every=1)
    assert np.array_equal(s_all[:, -1], s_T[:, 0])
    s_4, _, _ = hb.rb_vjp_host(m, s0, steps, np.zeros((N, steps // 4, ns)), params, th, every=4)
    assert np.array_equal(s_4, s_all[:, 3::4])
    assert np.array_equal(s_all[:, 4], hb.rb_jvp_host(m, s0, 5, None, params, th))


def test_zero_cotangent_and_linearity(built):
    m, s0, steps, params, th = scene("plane_first")
    ns = m.num_bodies * 13
    _, g0, gt = hb.rb_vjp_host(m, s0, steps, np.zeros((N, steps, ns)), params, th, every=1)
    assert not g0.any() and not gt.any()                 # exact zeros
    rng = np.random.default_rng(8)
    ga, gb = rng.normal(size=(2, N, steps, ns))
    a, b = 0.7, -1.3
    _, g0a, gta = hb.rb_vjp_host(m, s0, steps, ga, params, th, every=1)
    _, g0b, gtb = hb.rb_vjp_host(m, s0, steps, gb, params, th, every=1)
    _, g0c, gtc = hb.rb_vjp_host(m, s0, steps, a * ga + b * gb, params, th, every=1)
    assert world_err(g0c, a * g0a + b * g0b) <= 1e-12
    assert world_err(gtc, a * gta + b * gtb) <= 1e-12


def raw(m, s0, steps, gs, sel=(), tape_cap=0):
    """the C call itself: (rc, gs0, gtheta)"""
    n, p = s0.shape[0], len(sel)
    gs0, gth = np.ones_like(s0), np.ones((n, max(p, 1)))
    s0, gs = np.ascontiguousarray(s0), np.ascontiguousarray(gs)
    rc = hb.lib().tds_rb_vjp_host(C.byref(m), n, steps, steps, s0.ctypes.data, p, hb.param_spec(sel), None,
                                  gs.ctypes.data, None, gs0.ctypes.data, gth.ctypes.data, int(tape_cap))
    return rc, gs0, gth[:, :p]


def test_a_small_tape_capacity_gives_nan_gradients_for_the_overflowing_world_only(built):
    """World 0 is the fixed shot: the steps in which its balls collide record up to 11 765 entries.  World 1 is at rest
    with the balls far apart: a sphere that ends without an impulse leaves no entries, so its steps hold 350 (gravity
    and integrate).  A capacity of 1000 holds the second world and not the first; 100 holds neither."""
    m = billiard_model()
    steps, sel = 40, [("mass", 5), ("friction",)]
    s0 = billiard_state(2)
    s0[0, WHITE, 7:9] = shot_velocity([10.0, 600.0])
    s0[1, :, 0] = 10.0 * np.arange(7)
    s0[1, :, 1] = 0.0
    gs = np.random.default_rng(4).normal(size=(2, 1, 91))
    rc, g0, gt = raw(m, s0, steps, gs, sel, tape_cap=1000)
    assert rc == 2                                       # TDS_ERR_UNSUPPORTED
    assert np.all(np.isnan(g0[0])) and np.all(np.isnan(gt[0]))
    _, g0_own, gt_own = hb.rb_vjp_host(m, s0[1:], steps, gs[1:], sel)
    assert np.all(np.isfinite(g0[1])) and np.all(np.isfinite(gt[1]))
    assert np.array_equal(g0[1], g0_own[0]) and np.array_equal(gt[1], gt_own[0])
    with pytest.raises(hb.TdsHipError, match="tape exceeds the capacity"):
        hb.rb_vjp_host(m, s0, steps, gs, sel, tape_cap=1000)
    rc, g0, gt = raw(m, s0, steps, gs, sel, tape_cap=100)
    assert rc == 2 and np.all(np.isnan(g0)) and np.all(np.isnan(gt))
    rc, g0, gt = raw(m, s0, steps, gs, sel, tape_cap=20000)             # above the longest step: as the default
    _, g0_d, gt_d = hb.rb_vjp_host(m, s0, steps, gs, sel)
    assert rc == 0 and np.array_equal(g0, g0_d) and np.array_equal(gt, gt_d)


def test_the_default_capacity_holds_every_step_in_full_contact(built):
    """tumbling boxes and capsules on a plane with 8 iterations: every collision sphere in contact"""
    m, s0 = make_mixed_worlds(2, 21, MIXED_ORDER)
    ns = m.num_bodies * 13
    cap = hb.rb_vjp_plan(m, 2, 60, 4)[0]
    _, g0, _ = hb.rb_vjp_host(m, s0, 60, np.ones((2, 1, ns)), tape_cap=cap)
    assert np.all(np.isfinite(g0))


def test_plan(built):
    m = billiard_model()
    cap, chunk, W, total = hb.rb_vjp_plan(m, 4096, 300)
    assert cap == 21 * 50 * 320 + 7 * 64 and chunk % 64 == 0 and W >= 1 and total <= 8 << 30
    cap2, chunk2, W2, total2 = hb.rb_vjp_plan(m, 70, 7, 4, tape_cap=5000, work_bytes=1 << 30)
    assert (cap2, chunk2, W2) == (5000, 128, 7) and total2 <= 1 << 30
    # a budget that holds exactly that plan holds it, one byte less does not
    assert hb.rb_vjp_plan(m, 70, 7, 4, tape_cap=5000, work_bytes=total2)[1:3] == (128, 7)
    assert hb.rb_vjp_plan(m, 70, 7, 4, tape_cap=5000, work_bytes=total2 - 1)[1:3] == (128, 6)
    need = hb.rb_vjp_plan(m, 64, 1, 4, tape_cap=5000, work_bytes=1 << 30)[3]
    with pytest.raises(hb.TdsHipError, match=f"one step of 64 worlds needs [0-9]+ B"):
        hb.rb_vjp_plan(m, 70, 7, 4, tape_cap=5000, work_bytes=need // 2)
    # the default capacity is capped by the budget
    assert 0 < hb.rb_vjp_plan(m, 70, 7, work_bytes=64 << 20)[0] < cap


def test_refusals(built):
    m, s0 = make_worlds(2, 7)              # body 0 is the plane (static)
    ns = m.num_bodies * 13
    gs = np.zeros((2, 1, ns))
    for steps, every, why in ((0, 1, "steps must be at least 1"), (-2, 1, "steps must be at least 1"),
                              (6, 4, "every must divide steps"), (6, 0, "every must divide steps"),
                              (6, -3, "every must divide steps")):
        with pytest.raises(hb.TdsHipError, match="tds_rb error 1: tds_rb_vjp_host: " + why):
            hb.rb_vjp_host(m, s0, steps, gs, every=every)
    for bad in ([("mass", 0)], [("mass", 6)], [("mass", 1), ("mass", 1)], [("gravity", 3)], [("com", 1, 0)],
                [("friction",), ("friction",)], [("inertia", 1, 0)]):
        with pytest.raises(hb.TdsHipError) as e_jvp:
            hb.rb_jvp_host(m, s0, 1, np.zeros((2, 1, ns + len(bad))), bad)
        with pytest.raises(hb.TdsHipError, match="tds_rb error 1:") as e:
            hb.rb_vjp_host(m, s0, 1, gs, bad)
        assert str(e.value) == str(e_jvp.value)
    # malformed arrays are refused in Python, before the library is called: N = 2, K = 2, steps = 2
    sel = [("mass", 1), ("friction",)]
    z = np.zeros
    for bad_gs in (z((2, 2, ns)), z((2, ns - 1)), z((1, 1, ns))):
        with pytest.raises(ValueError, match=rf"gs: expected \[2, 1, {ns}\], got "):
            hb.rb_vjp_host(m, s0, 2, bad_gs)
    with pytest.raises(ValueError, match=rf"gs: expected \[2, 2, {ns}\], got "):
        hb.rb_vjp_host(m, s0, 2, gs, every=1)
    for bad_theta, got in ((z((2, 1)), r"\(2, 1\)"), (z((1, 2)), r"\(1, 2\)"), (z(3), r"\(3,\)")):
        with pytest.raises(ValueError, match=r"theta: expected \[2\] or \[2, 2\], got " + got):
            hb.rb_vjp_host(m, s0, 2, gs, sel, bad_theta)
        with pytest.raises(ValueError, match=r"theta: expected \[2\] or \[2, 2\], got " + got):
            hb.rb_jvp_host(m, s0, 2, None, sel, bad_theta)
    for v in (z((2, 2, ns + 3)), z((3, 2, ns + 2)), z((2, ns + 3)), z((2, 2, 1, ns + 2))):
        with pytest.raises(ValueError, match=rf"v: expected \[2, K, {ns + 2}\]"):
            hb.rb_jvp_host(m, s0, 2, v, sel)
    with pytest.raises(ValueError, match="cannot reshape"):
        hb.rb_jvp_host(m, np.zeros((2, ns - 1)), 2)
    with pytest.raises(ValueError, match="cannot reshape"):
        hb.rb_vjp_host(m, np.zeros((2, ns - 1)), 2, gs)
    L = hb.lib()
    st, out = np.ascontiguousarray(s0), np.zeros_like(s0)
    nul = (hb.Param * 1)()
    args = lambda **k: [k.get("m", C.byref(m)), k.get("n", 2), 1, 1, k.get("s0", st.ctypes.data), k.get("p", 0),
                        k.get("sel", nul), None, k.get("gs", gs.ctypes.data), None, out.ctypes.data, None,
                        k.get("cap", 0)]
    assert L.tds_rb_vjp_host(*args()) == 0
    for k in ({"m": None}, {"n": 0}, {"s0": None}, {"gs": None}, {"p": 1, "sel": None}, {"p": -1}, {"cap": -1}):
        assert L.tds_rb_vjp_host(*args(**k)) == 1, k


def test_host_code_is_clean_under_the_sanitizers(built, tmp_path):
    """tools/rb_vjp_sanitize.cpp: tds_rb_vjp_host on the tumbling and billiard scenes, default and overflowing capacity,
    as a program of its own built with -fsanitize=address,undefined (no Python, no GPU).  A check of the build machine:
    sanitizer runs stay off the machines that hold a GPU."""
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present: the sanitizer program runs where the library is built")
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "rb_vjp_sanitize")
    csrc = os.path.join(ROOT, "tiny-differentiable-simulator_amd", "csrc")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-ffp-contract=off",
                           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                           "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
                           os.path.join(ROOT, "tools", "rb_vjp_sanitize.cpp"), os.path.join(csrc, "tds_rb_vjp.hip"),
                           "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "rb_vjp_sanitize: ok" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr
