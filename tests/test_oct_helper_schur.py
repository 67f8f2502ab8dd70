"""The 8-lane kernel's split of the work between barriers (1b) and (2) (csrc/tds_oct.hip, step-loop build for one wavefront per SIMD).

In that build the HELPER sums the 21 entries of the Schur complement behind barrier (1b) and hands them over at a barrier of its
own, (1c); the main wavefront computes the root block and the head of the forward dynamics meanwhile; and the visual poses go
out behind the helper's last row window, from transforms the helper keeps in registers across the windows (the hand-over
slots they came from are row slots by then).  Only the schedule changes, no expression: every comparison here is BIT FOR BIT.
The one-wavefront build (option oct_w2 = 0) takes none of it and is the yardstick; launches of ONE step pass through every
barrier once from a freshly loaded record, launches of twelve carry registers and LDS regions from step to step.

  * 67 environments (nine workgroups, the last one ragged): wavefronts whose largest contact count NA is 0, 1, 3, 4, 5, 6, 8, 17
    — no row window; one; the long first window (9 and 12 rows); two windows; three and more — of tests/test_oct_sweep_windows.py's
    batch; 8 environments: one wavefront that falls from no contact to three and more within the launch (checked on the host);
  * pgs_iterations 1 and 3; 12 steps into y and [obs | reward | done] rings of 5 slots (the rings wrap twice; the last step
    lands in the handle's y as well);
  * float records, 16 environments x 6 steps.  A launch keeps its state in double from step to step, but BETWEEN launches the
    state is the float x record: six launches of one step and one launch of six steps are different computations from the
    second step on (on any commit).  What is exact, and asserted: the first step of the two; the six-step launch against the
    one-wavefront build's six-step launch; the six one-step launches against the one-wavefront build's six one-step launches;
  * the reset pool: three environments of every wavefront end their first step done and take a pool state inside the launch.
    The terminal step's y record carries the poses of the state BEFORE that step: held against a straight-line single step
    of the one-wavefront build from that state.

Measured (MI355X): 0 differing values in every comparison; 33 resets in the reset-pool launch, 27 of them in the first step."""
import functools

import numpy as np
import pytest

import tds_amd
from tds_amd import hip_backend
import diff_states
from test_oct_sweep_windows import TARGETS, _batch

pytestmark = pytest.mark.gpu

K, SLOTS, BLOCKS = 12, 5, 16
WAVES = [0, 1, 3, 4, 5, 6, 8, 17]  # the largest contact count of wavefronts 0 .. 7 of the 67


def _torch():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch


def _model(iters):
    m = tds_amd.load_model("ant").copy()
    m.pgs_iterations = iters
    return m


@functools.lru_cache(maxsize=None)
def _states(case):
    """read-only states [n, input_dim]: "counts" 67, "landing" 8, "low" 67 (three environments per wavefront below the
    termination height), "float" 16"""
    m = tds_amd.load_model("ant")
    if case in ("counts", "low", "float"):
        x, cx = _batch()
        rows = np.concatenate([np.arange(8 * TARGETS.index(t), 8 * TARGETS.index(t) + 8) for t in WAVES] + [np.arange(88, 91)])
        assert [int(cx[rows[8 * g:8 * g + 8]].max()) for g in range(8)] == WAVES
        x = np.array(x[rows])
        if case == "float":
            x = x[np.r_[16:24, 40:48]]  # (the wavefronts of 3 and 6 contacts)
        if case == "low":
            rng = np.random.default_rng(17)
            sel = (np.arange(x.shape[0]) % 8) < 3
            x[sel, 2] = rng.uniform(0.20, 0.25, int(sel.sum()))
    else:
        n, nq, nd, ad = 8, m.dof_q, m.dof_qd, m.action_dim
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
        for k in range(4):
            z[:, nq + nd:nq + nd + ad] = acts[k % BLOCKS]
            counts.append(int(diff_states.contact_counts("ant", m, z, reference=False).max()))
            z[:, :nq + nd] = step(z)[:, :nq + nd]
        assert counts[0] == 0 and max(counts) >= 3, counts
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _actions(n):
    a = np.random.default_rng(31 + n).uniform(-0.4, 0.4, (BLOCKS, n, 8))
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _run(case, iters, w2, one_step_launches, dtype="f64", steps=K, slots=SLOTS, reset_seed=None):
    """`steps` steps from the case's states as ONE ring launch or as `steps` ring launches of one step:
    (y ring [slots], obs ring [slots], the handle's y, final state) as float64 numpy, read-only"""
    torch = _torch()
    m = _model(iters)
    x = np.array(_states(case))
    n = x.shape[0]
    acts = np.array(_actions(n))
    if dtype == "mixed":
        x, acts = x.astype(np.float32).astype(np.float64), acts.astype(np.float32).astype(np.float64)
    sim = hip_backend.HipSim(m, n, dtype=dtype, options={"step_many_loop": 1, "oct_w2": w2})
    assert sim.single_step_kernel()[0] == "oct8" and sim.step_many_is_loop(steps)
    if reset_seed is not None:
        sim.set_auto_reset(True, reset_seed)
    tdt = sim.torch_dtype
    sim.x.copy_(torch.from_numpy(x).to(tdt).cuda())
    actions = torch.from_numpy(acts).to(tdt).cuda().contiguous()
    obs_ring = torch.zeros((slots, n, sim.obs_dim + 2), dtype=tdt, device="cuda")
    y_ring = torch.zeros((slots, n, m.output_dim), dtype=tdt, device="cuda")
    if one_step_launches:
        for k in range(steps):
            sim.step_many_rings(actions, 1, obs_ring, y_ring, first_block=k, obs_first=k, y_first=k)
    else:
        sim.step_many_rings(actions, steps, obs_ring, y_ring)
    torch.cuda.synchronize()
    out = tuple(t.double().cpu().numpy() for t in (y_ring, obs_ring, sim.y, sim.x))
    for a in out:
        a.setflags(write=False)
    return out


POSES = slice(28, 28 + 7 * 9)  # q (14) | qd (14) | nine visual poses | ...
NAMES = ("y ring", "obs ring", "handle's y", "state")


def _assert_equal(tag, a, b, steps=K):
    diff = [int((p != q).sum()) for p, q in zip(a, b)]
    print(f"{tag}: differing values " + ", ".join(f"{nm} {d}" for nm, d in zip(NAMES, diff)))
    for nm, p in zip(NAMES, a):
        assert np.isfinite(p).all(), nm
    assert np.abs(a[0]).max() > 0 and np.abs(a[1][:, :, 2:-2]).max() > 0
    assert np.abs(a[0][:, :, POSES]).max() > 0
    assert diff == [0, 0, 0, 0]
    # the last step's record is in its ring slot and in the handle's y
    assert np.array_equal(a[0][(steps - 1) % a[0].shape[0]], a[2])


CASES = [("counts", 1), ("counts", 3), ("landing", 1), ("landing", 3)]


@pytest.mark.parametrize("case,iters", CASES)
def test_twelve_steps_in_one_launch_equal_twelve_launches_of_one_step(case, iters):
    one = _run(case, iters, 1, False)
    many = _run(case, iters, 1, True)
    _assert_equal(f"{case}, pgs_iterations {iters}: one launch vs {K} launches", one, many)


@pytest.mark.parametrize("one_step_launches", [False, True])
@pytest.mark.parametrize("case,iters", CASES)
def test_two_wavefront_build_equals_the_one_wavefront_build(case, iters, one_step_launches):
    two = _run(case, iters, 1, one_step_launches)
    one = _run(case, iters, 0, one_step_launches)
    _assert_equal(f"{case}, pgs_iterations {iters}, {'one-step launches' if one_step_launches else 'one launch'}: "
                  f"two wavefronts vs one", two, one)


def test_float_records():
    steps = 6
    ring = _run("float", 1, 1, False, "mixed", steps, steps)
    many = _run("float", 1, 1, True, "mixed", steps, steps)
    ring1 = _run("float", 1, 0, False, "mixed", steps, steps)
    many1 = _run("float", 1, 0, True, "mixed", steps, steps)
    d0 = [int((ring[i][0] != many[i][0]).sum()) for i in (0, 1)]
    d_ring = [int((p != q).sum()) for p, q in zip(ring, ring1)]
    d_many = [int((p != q).sum()) for p, q in zip(many, many1)]
    print(f"float records: first step, one launch vs one-step launch {d0}; six-step launch, two wavefronts vs one {d_ring}; "
          f"six one-step launches, two wavefronts vs one {d_many}")
    assert np.isfinite(ring[0]).all() and np.abs(ring[0][:, :, POSES]).max() > 0
    assert d0 == [0, 0]
    assert d_ring == [0, 0, 0, 0]
    assert d_many == [0, 0, 0, 0]


def test_reset_pool_replaces_environments_inside_the_launch():
    torch = _torch()
    one = _run("low", 1, 1, False, "f64", K, K, 7)
    many = _run("low", 1, 1, True, "f64", K, K, 7)
    done = one[1][:, :, -1] != 0  # [step, environment]
    low = (np.arange(done.shape[1]) % 8) < 3
    print(f"reset pool: {int(done.sum())} resets in {K} steps; first step: {int(done[0].sum())} of {int(low.sum())} low environments")
    per_wave = done[0, :64].reshape(8, 8)
    assert done[0][low].any() and (per_wave.any(axis=1) & ~per_wave.all(axis=1)).any()  # (reset and carried environments side by side)
    assert not done.all(axis=0).all()
    diff = [int((p != q).sum()) for p, q in zip(one, many)]
    print("reset pool: differing values, one launch vs launches of one step: " + ", ".join(f"{nm} {d}" for nm, d in zip(NAMES, diff)))
    assert np.isfinite(one[0]).all()
    assert diff == [0, 0, 0, 0]
    # the terminal step's poses are those of the state before it: a straight-line single step of the one-wavefront build
    m = _model(1)
    x = np.array(_states("low"))
    x[:, 28:36] = _actions(x.shape[0])[0]
    ref = hip_backend.HipSim(m, x.shape[0], options={"oct_w2": 0})
    y0 = ref.forward_zero(torch.from_numpy(x).cuda()).cpu().numpy()
    assert np.abs(y0[:, POSES]).max() > 0
    assert np.array_equal(one[0][0][done[0]][:, POSES], y0[done[0]][:, POSES])
