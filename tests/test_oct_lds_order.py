"""The 8-lane kernel's LDS regions that serve twice within a step (csrc/tds_oct.hip), across the steps of ONE launch.

The main wavefront requests LDS reads ahead of their use (the operands of the Schur sums a pass ahead, the sums in one batch:
main_dyn2).  A read that moved over the sync that orders it would see a stale or a foreign value in a region that is reused:
  * the impulses' slots hold W = L_c D until the sweep and the impulses from then on;
  * the Schur sums' slots hold the sums until every lane has read them and the root block's factors for the helper afterwards;
  * the second row window doubles as the kinematics' hand-over and as the root's sines and cosines;
  * the x record is rewritten at the integration (and by the reset pool) and read by the helper's records behind barrier (0).
What such a value would be depends on the contact count and on what the step before left, so the states are those of
tests/test_oct_sweep_windows.py — 93 environments, every wavefront built for one largest contact count among 0, 1, 2, 3, 4, 5, 6,
8, 11, 16, 17, a ragged last workgroup — stepped 6 times in one ring launch (a fresh action block per step, 2 obs slots) and
held against the same steps as single launches of the same build and against the general kernel (option oct = 0).

Loop and single launches of a build do the same arithmetic per step, term by term, on the same bits (the step-loop form of the
build for one wavefront per SIMD orders its Schur reads differently from its straight-line form — not its sums): their
records are compared bit for bit, as they were equal on the commit before the reorder (measured there: f64, every build, both
batches of states).  The general kernel sums in another order: 1e-9 relative, the bound of the suite's other
8-lane-against-general comparisons.  Auto-reset against single steps: 1e-9 as tests/test_oct.py (measured: equal).

Measured (MI355X): loop vs single launches 0 everywhere; vs the general kernel y 1.1e-10 (contact counts), 3.0e-11 (landing);
float records against the rounded double records 5.9e-8."""
import functools

import numpy as np
import pytest

import tds_amd
from tds_amd import hip_backend
from conftest import rel_err
import diff_states
from test_oct_sweep_windows import N, TARGETS, _batch

pytestmark = pytest.mark.gpu

STEPS, SLOTS, BLOCKS = 6, 2, 4
BUILDS = [1, 3, 0]  # option oct_w2


def _torch():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch


@functools.lru_cache(maxsize=None)
def _actions(n):
    a = np.random.default_rng(21).uniform(-0.4, 0.4, (BLOCKS, n, 8))
    a.setflags(write=False)
    return a


def _loop_launch(torch, m, x, dtype, opts, auto_reset=None, float_inputs=False):
    """STEPS steps as one ring launch: (y ring [STEPS], obs ring [SLOTS], final state), as float64 numpy
    (float_inputs: state and actions rounded to float first — what a launch with float records is given)"""
    n = x.shape[0]
    acts = np.array(_actions(n))
    if float_inputs:
        x, acts = np.array(x).astype(np.float32).astype(np.float64), acts.astype(np.float32).astype(np.float64)
    a = hip_backend.HipSim(m, n, dtype=dtype, options=dict(opts, step_many_loop=1))
    assert a.step_many_is_loop(STEPS) and a.single_step_kernel()[0] == "oct8"
    tdt = a.torch_dtype
    if auto_reset is not None:
        a.set_auto_reset(True, auto_reset)
    a.x.copy_(torch.from_numpy(np.array(x)).to(tdt).cuda())
    actions = torch.from_numpy(acts).to(tdt).cuda().contiguous()
    obs_ring = torch.zeros((SLOTS, n, a.obs_dim + 2), dtype=tdt, device="cuda")
    y_ring = torch.zeros((STEPS, n, m.output_dim), dtype=tdt, device="cuda")
    a.step_many_rings(actions, STEPS, obs_ring, y_ring, first_block=1, obs_first=1)
    return y_ring.double().cpu().numpy(), obs_ring.double().cpu().numpy(), a.x.double().cpu().numpy()


def _single_launches(torch, m, x, opts, auto_reset=None, float_inputs=False):
    """the same steps as single launches: (y [STEPS], obs [STEPS], final state)"""
    n = x.shape[0]
    acts = np.array(_actions(n))
    if float_inputs:
        x, acts = np.array(x).astype(np.float32).astype(np.float64), acts.astype(np.float32).astype(np.float64)
    b = hip_backend.HipSim(m, n, options=dict(opts, step_many_loop=0))
    if auto_reset is not None:
        b.set_auto_reset(True, auto_reset)
    b.x.copy_(torch.from_numpy(np.array(x)).cuda())
    actions = torch.from_numpy(acts).cuda().contiguous()
    obs = torch.zeros((n, b.obs_dim + 2), dtype=torch.float64, device="cuda")
    ys, os_ = [], []
    for k in range(STEPS):
        b.step(actions[(1 + k) % BLOCKS], 1, obs)
        ys.append(b.y.cpu().numpy().copy())
        os_.append(obs.cpu().numpy().copy())
    return np.array(ys), np.array(os_), b.x.cpu().numpy()


def _obs_of_ring(obs_ring):
    """(step, record) of the ring's slots after STEPS steps from slot 1: the last SLOTS steps"""
    return [(k, obs_ring[(1 + k) % SLOTS]) for k in range(STEPS - SLOTS, STEPS)]


def _check_equal(tag, loop, single):
    y_ring, obs_ring, x_a = loop
    ys, os_, x_b = single
    e_y, e_x = rel_err(y_ring, ys), rel_err(x_a, x_b)
    e_o = max(rel_err(o, os_[k]) for k, o in _obs_of_ring(obs_ring))
    same = np.array_equal(y_ring, ys) and np.array_equal(x_a, x_b) and all(np.array_equal(o, os_[k]) for k, o in _obs_of_ring(obs_ring))
    print(f"{tag}: loop vs single launches y {e_y:.3e} obs {e_o:.3e} state {e_x:.3e}, bit-equal {same}")
    assert np.isfinite(y_ring).all()
    assert same


def _check_close(tag, loop, single, tol=1e-9):
    y_ring, obs_ring, x_a = loop
    ys, os_, x_b = single
    e_y, e_x = rel_err(y_ring, ys), rel_err(x_a, x_b)
    e_o = max(rel_err(o, os_[k]) for k, o in _obs_of_ring(obs_ring))
    print(f"{tag}: y {e_y:.3e} obs {e_o:.3e} state {e_x:.3e}")
    assert e_y < tol and e_o < tol and e_x < tol


@functools.lru_cache(maxsize=None)
def _general_single_launches():
    torch = _torch()
    return _single_launches(torch, tds_amd.load_model("ant"), _batch()[0], {"oct": 0})


@pytest.mark.parametrize("w2", BUILDS)
def test_six_steps_in_one_launch_per_contact_count(w2):
    """every largest contact count of a wavefront among TARGETS, 6 steps in one launch: against single launches of the same build
    (bit for bit) and against the general kernel's single launches (1e-9)"""
    torch = _torch()
    m = tds_amd.load_model("ant")
    x, cx = _batch()
    assert x.shape[0] == N and sorted({int(cx[8 * g:8 * g + 8].max()) for g in range(len(TARGETS))}) == TARGETS
    loop = _loop_launch(torch, m, x, "f64", {"oct_w2": w2})
    _check_equal(f"oct_w2 {w2}", loop, _single_launches(torch, m, x, {"oct_w2": w2}))
    gen = _general_single_launches()
    assert hip_backend.HipSim(m, N, options={"oct": 0}).single_step_kernel()[0] == "general"
    _check_close(f"oct_w2 {w2} vs general kernel", loop, gen)


def test_six_steps_in_one_launch_with_float_records():
    """float records: the launch keeps its state in double between the steps — its records are the rounded records of the same
    launch with double records (2e-6: float round-off of a record, as tests/test_oct_sweep_windows.py)"""
    torch = _torch()
    m = tds_amd.load_model("ant")
    x, _ = _batch()
    f = _loop_launch(torch, m, x, "mixed", {"oct_w2": 1}, float_inputs=True)
    d = _loop_launch(torch, m, x, "f64", {"oct_w2": 1}, float_inputs=True)
    e_y, e_o = rel_err(f[0], d[0]), rel_err(f[1], d[1])
    print(f"float records: y {e_y:.3e} obs {e_o:.3e}")
    assert np.isfinite(f[0]).all()
    assert e_y < 2e-6 and e_o < 2e-6
    # (both launches above run the step-loop form: a stale LDS value would show in both.  The double one is therefore held
    #  against single launches — the straight-line form — from the same rounded inputs, bit for bit)
    _check_equal("double records from float inputs", d, _single_launches(torch, m, x, {"oct_w2": 1}, float_inputs=True))


def test_six_steps_in_one_launch_with_auto_reset():
    """the reset pool rewrites a done environment's x record at the end of its step, inside the launch: the batch's low states
    (z < 0.26 after a step) are done from the first step on.  Against single auto-reset steps through the same pool."""
    torch = _torch()
    m = tds_amd.load_model("ant")
    x, _ = _batch()
    loop = _loop_launch(torch, m, x, "f64", {}, auto_reset=5)
    single = _single_launches(torch, m, x, {}, auto_reset=5)
    dones = int(sum((o[:, -1] != 0).sum() for o in single[1]))
    print(f"auto-reset: {dones} done records in {STEPS} steps x {N} environments")
    assert dones >= STEPS  # (resets did happen, in every step's worth)
    for k, o in _obs_of_ring(loop[1]):
        assert (o[:, -1] == single[1][k][:, -1]).all(), k
    _check_close("auto-reset", loop, single)


@functools.lru_cache(maxsize=None)
def _landing():
    """64 environments a hand's breadth above the plane, falling at 6 m/s: no contact in step 0, one or two in step 1, at least
    three in every wavefront from step 2 on (checked here on the host oracle's own trajectory) — the W values that borrow the
    impulses' slots meet impulses within the launch, from empty slots on"""
    m = tds_amd.load_model("ant")
    n, nq, nd, ad = 64, m.dof_q, m.dof_qd, m.action_dim
    rng = np.random.default_rng(11)
    ip = np.array([m.initial_poses[i] for i in range(ad)])
    x = np.zeros((n, m.input_dim))
    x[:, 0:2] = rng.uniform(-1, 1, (n, 2))
    x[:, 3:5] = rng.uniform(-0.05, 0.05, (n, 2))
    x[:, 5] = rng.uniform(-3, 3, n)
    x[:, 6:nq] = ip + rng.uniform(-0.1, 0.1, (n, nq - 6))
    x[:, 2] = 0.46
    x[:, nq + 2] = -6.0
    x[:, -3:] = [15, 0.3, 3]
    acts = _actions(n)
    step = diff_states.oracle_step(m)
    z, counts = x.copy(), []
    for k in range(STEPS):
        z[:, nq + nd:nq + nd + ad] = acts[(1 + k) % BLOCKS]
        counts.append(diff_states.contact_counts("ant", m, z, reference=False).reshape(8, 8).max(axis=1))
        z[:, :nq + nd] = step(z)[:, :nq + nd]
    counts = np.array(counts)
    assert (counts[0] == 0).all() and (counts[2:] >= 3).all(), counts
    x.setflags(write=False)
    return x


@pytest.mark.parametrize("w2", BUILDS)
def test_landing_from_no_contact_to_three_and_more_within_one_launch(w2):
    torch = _torch()
    m = tds_amd.load_model("ant")
    x = _landing()
    loop = _loop_launch(torch, m, x, "f64", {"oct_w2": w2})
    _check_equal(f"landing, oct_w2 {w2}", loop, _single_launches(torch, m, x, {"oct_w2": w2}))
    _check_close(f"landing, oct_w2 {w2} vs general kernel", loop, _single_launches(torch, m, x, {"oct": 0}))
