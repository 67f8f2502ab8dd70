"""The 8-lane kernel's first Gauss-Seidel sweep specialised for the wavefront's contact count (csrc/tds_oct.hip: main_sweep with
NA as a template constant; step-loop build for one wavefront per SIMD; run-time option oct_sweep_na).

With NA = 1 .. 4 contacts at most among a wavefront's environments the first sweep of a step runs straight-line: every row's
kind static, the normal rows' impulses handed to their friction rows in registers, the long window's second barrier where the
generic chain has it.  Same expressions row by row in the same order, so every comparison between builds, launch forms and
option values is BIT FOR BIT; the one-wavefront build (option oct_w2 = 0) has no such instantiation and is the yardstick.

What can go wrong depends on the wavefront's largest contact count NA — no window (0), the specialised sweep of one window
(1, 2) and of the long window with its barrier inside (3, 4), the generic chain (5; 9: four windows) — and on where the
environments sit in the workgroups.  So: Ants dropped from chosen heights at chosen tilts (the counts come from the oracle's
narrowphase and are asserted on the host, before anything runs on a GPU), one batch per (batch size, NA):

  5 environments: a partial workgroup | 8: exactly one | 9: a full one and a partial one | 24: three, with mixed counts inside
  every wavefront; the first wavefront's largest count is the batch's NA.

Twelve steps into y and [obs | reward | done] rings of five slots (they wrap twice), double and float records.  Float records:
a launch keeps its state in double from step to step, between launches the state is the float record — twelve launches of one
step and one launch of twelve are different computations from the second step on; what is exact there, and asserted, is the
first step of the two and each form against the one-wavefront build's.  Option oct_sweep_na 1 against 0: also with two
Gauss-Seidel iterations (a model copy: the second iteration's generic sweep reads the impulses the specialised one stored) and
with the reset pool replacing environments inside the launch (every batch size, double and float records).  Against the
oracle: the first step of every batch, within tests/test_oct.py's bounds (1e-6 with double records, 1e-3 with float
records).  Every handle's launches are checked to take the build under test (the host launch plan)."""
import functools

import numpy as np
import pytest

import tds_amd
from tds_amd import hip_backend
from conftest import rel_err
import diff_states
from test_launch_plan import MI355X

pytestmark = pytest.mark.gpu

K, SLOTS, BLOCKS = 12, 5, 16
COUNTS = [0, 1, 2, 3, 4, 5, 9]  # the first wavefront's largest contact count (9: the ">= 6" case, four windows)
SIZES = [5, 8, 9, 24]
CASES = [(n, na) for n in SIZES for na in COUNTS]
NAMES = ("y ring", "obs ring", "handle's y", "state")
POSES = slice(28, 28 + 7 * 9)  # q (14) | qd (14) | nine visual poses | ...


def _torch():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch


@functools.lru_cache(maxsize=None)
def _pool():
    """(x [n, input_dim], contact counts [n]) of Ants dropped from a grid of heights and tilts — read-only"""
    m = tds_amd.load_model("ant")
    nq, nd, ad = m.dof_q, m.dof_qd, m.action_dim
    ip = np.array([m.initial_poses[i] for i in range(ad)])
    rng = np.random.default_rng(23)
    heights = np.linspace(-0.06, 0.66, 19)
    tilts = [(0.0, 0.0), (0.35, 0.0), (0.0, -0.4), (0.6, 0.5), (-0.9, 0.3), (0.2, 1.1)]
    x = np.zeros((len(heights) * len(tilts), m.input_dim))
    k = 0
    for h in heights:
        for roll, pitch in tilts:
            x[k, 0:2] = rng.uniform(-1, 1, 2)
            x[k, 2] = h
            x[k, 3:5] = [roll, pitch]
            x[k, 5] = rng.uniform(-3, 3)
            x[k, 6:nq] = ip + rng.uniform(-0.3, 0.3, nq - 6)
            x[k, nq:nq + nd] = rng.uniform(-0.5, 0.5, nd)
            x[k, nq + 2] = -1.5  # falling
            k += 1
    x[:, -3:] = [15, 0.3, 3]
    c = diff_states.contact_counts("ant", m, x, reference=False)
    for na in COUNTS:
        assert (c == na).any(), (na, diff_states.histogram(c, 17))
    x.setflags(write=False)
    c.setflags(write=False)
    return x, c


@functools.lru_cache(maxsize=None)
def _states(n, na):
    """read-only states [n, input_dim]: the first wavefront's largest count is `na` (one state with exactly that many, a state
    without contact where na > 0, the others with at most as many, shuffled); the wavefronts behind it hold any counts"""
    x, c = _pool()
    rng = np.random.default_rng(100 * n + na)
    first = min(n, 8)
    pick = [np.flatnonzero(c == na)[0]]
    if na > 0:
        pick.append(np.flatnonzero(c == 0)[na % 3])
    pick.extend(rng.choice(np.flatnonzero(c <= na), first - len(pick)))
    pick = list(rng.permutation(pick[:first]))
    pick.extend(rng.choice(x.shape[0], n - first))
    pick = np.array(pick)
    cx = c[pick]
    assert pick.shape[0] == n and int(cx[:first].max()) == na
    if n == 24:  # mixed counts inside every wavefront behind the first
        assert all(len(set(cx[8 * g:8 * g + 8])) > 1 for g in range(1, 3))
    out = np.array(x[pick])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _actions(n):
    a = np.random.default_rng(31 + n).uniform(-0.4, 0.4, (BLOCKS, n, 8))
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _run(n, na, w2, one_step_launches, dtype="f64", steps=K, sweep_na=1, iters=1, reset_seed=None):
    """`steps` steps from the batch's states as ONE ring launch or as ring launches of one step:
    (y ring [SLOTS], obs ring [SLOTS], the handle's y, final state) as float64 numpy, read-only"""
    torch = _torch()
    m = tds_amd.load_model("ant").copy()
    m.pgs_iterations = iters
    x = np.array(_states(n, na))
    if reset_seed is not None:
        # three environments of every wavefront sunk so far that they end their first step below the termination height (from
        # 0.20 - 0.25 the contacts lift most of them back above it within the step: the oracle's step, on the host).  Sunk, they
        # have many contacts: the wavefront's first step is no longer one of `na` contacts — the steps behind it are, with the
        # pool's standing states beside the carried environments.
        x[(np.arange(n) % 8) < 3, 2] = np.random.default_rng(17).uniform(0.05, 0.15, int(((np.arange(n) % 8) < 3).sum()))
    acts = np.array(_actions(n))
    if dtype == "mixed":
        x, acts = x.astype(np.float32).astype(np.float64), acts.astype(np.float32).astype(np.float64)
    sim = hip_backend.HipSim(m, n, dtype=dtype, options={"step_many_loop": 1, "oct_w2": w2, "oct_sweep_na": sweep_na})
    assert sim.single_step_kernel()[0] == "oct8" and sim.step_many_is_loop(K)  # (a ring launch of one step is the step-loop form too)
    assert sim.get_option("oct_sweep_na") == sweep_na
    # the build the launches take (the host plan for a device of the MI355X's shape, which the handle follows:
    # tests/test_launch_plan.py): the build for one wavefront per SIMD — the only one with the specialised sweep — or the
    # one-wavefront build.  Without this every comparison below would also pass on another build, the new code never run.
    if torch.cuda.get_device_properties(sim.device).multi_processor_count == MI355X["num_cus"]:
        with hip_backend.default_options(step_many_loop=1, oct_w2=w2, oct_sweep_na=sweep_na):
            for nsub in sorted({1, steps}):
                plan = hip_backend.launch_plan_host(m, dtype, n, nsub=nsub, rings=1, auto_reset=int(reset_seed is not None), **MI355X)
                assert (plan["kernel"], plan["build"], plan["refused"]) == ("oct8", 3 if w2 == 1 else 1, False), plan
    if reset_seed is not None:
        sim.set_auto_reset(True, reset_seed)
    tdt = sim.torch_dtype
    sim.x.copy_(torch.from_numpy(x).to(tdt).cuda())
    actions = torch.from_numpy(acts).to(tdt).cuda().contiguous()
    obs_ring = torch.zeros((SLOTS, n, sim.obs_dim + 2), dtype=tdt, device="cuda")
    y_ring = torch.zeros((SLOTS, n, m.output_dim), dtype=tdt, device="cuda")
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


def _assert_equal(tag, a, b, steps=K):
    diff = [int((p != q).sum()) for p, q in zip(a, b)]
    print(f"{tag}: differing values " + ", ".join(f"{nm} {d}" for nm, d in zip(NAMES, diff)))
    for nm, p in zip(NAMES, a):
        assert np.isfinite(p).all(), nm
    assert np.abs(a[0]).max() > 0 and np.abs(a[1][:, :, 2:-2]).max() > 0
    assert np.abs(a[0][:, :, POSES]).max() > 0
    assert diff == [0, 0, 0, 0]
    # the last step's record is in its ring slot and in the handle's y
    assert np.array_equal(a[0][(steps - 1) % SLOTS], a[2])


@pytest.mark.parametrize("n,na", CASES)
def test_twelve_steps_in_one_launch_equal_twelve_launches_of_one_step(n, na):
    _assert_equal(f"{n} environments, NA {na}: one launch vs {K} launches", _run(n, na, 1, False), _run(n, na, 1, True))


@pytest.mark.parametrize("one_step_launches", [False, True])
@pytest.mark.parametrize("n,na", CASES)
def test_two_wavefront_build_equals_the_one_wavefront_build(n, na, one_step_launches):
    _assert_equal(f"{n} environments, NA {na}, {'one-step launches' if one_step_launches else 'one launch'}: two wavefronts vs one",
                  _run(n, na, 1, one_step_launches), _run(n, na, 0, one_step_launches))


@pytest.mark.parametrize("n,na", CASES)
def test_float_records(n, na):
    ring, many = _run(n, na, 1, False, "mixed"), _run(n, na, 1, True, "mixed")
    _assert_equal(f"float records, {n} environments, NA {na}, one launch: two wavefronts vs one", ring, _run(n, na, 0, False, "mixed"))
    _assert_equal(f"float records, {n} environments, NA {na}, one-step launches: two wavefronts vs one", many, _run(n, na, 0, True, "mixed"))
    # the first step of the two forms: one step from the same float record is the same computation
    one, two = _run(n, na, 1, True, "mixed", 1), _run(n, na, 1, False, "mixed", 2)
    d0 = [int((one[i][0] != two[i][0]).sum()) for i in (0, 1)]
    print(f"float records, {n} environments, NA {na}, first step: a launch of one step vs the first of two: differing values {d0}")
    assert np.abs(one[0][0][:, POSES]).max() > 0
    assert d0 == [0, 0]


@pytest.mark.parametrize("dtype", ["f64", "mixed"])
@pytest.mark.parametrize("n,na", CASES)
def test_option_oct_sweep_na_changes_no_bit(n, na, dtype):
    _assert_equal(f"{n} environments, NA {na}, {dtype}: oct_sweep_na 1 vs 0", _run(n, na, 1, False, dtype), _run(n, na, 1, False, dtype, K, 0))
    _assert_equal(f"{n} environments, NA {na}, {dtype}, pgs_iterations 2: oct_sweep_na 1 vs 0",
                  _run(n, na, 1, False, dtype, K, 1, 2), _run(n, na, 1, False, dtype, K, 0, 2))


@pytest.mark.parametrize("dtype", ["f64", "mixed"])
@pytest.mark.parametrize("n,na", CASES)
def test_option_oct_sweep_na_changes_no_bit_with_the_reset_pool(n, na, dtype):
    on, off = _run(n, na, 1, False, dtype, K, 1, 1, 7), _run(n, na, 1, False, dtype, K, 0, 1, 7)
    done = on[1][:, :, -1] != 0  # [slot, environment]: the last SLOTS steps
    many = _run(n, na, 1, True, dtype, 1, 1, 1, 7)  # (the first step alone: its done flags)
    first = many[1][0, :, -1] != 0
    print(f"reset pool, {dtype}, {n} environments, NA {na}: done in the first step {int(first.sum())}, in the last {SLOTS} steps {int(done.sum())}")
    # every sunk environment is replaced at the end of the first step, inside the launch; replaced and carried environments
    # stand side by side (in the first step, or — 5 environments that all end it done — in the steps behind it)
    assert first[(np.arange(n) % 8) < 3].all() and not (first.all() and done.all())
    _assert_equal(f"reset pool, {dtype}, {n} environments, NA {na}: oct_sweep_na 1 vs 0", on, off)


@pytest.mark.parametrize("dtype", ["f64", "mixed"])
@pytest.mark.parametrize("n,na", CASES)
def test_first_step_against_the_oracle(n, na, dtype):
    """tests/test_oct.py's bounds: 1e-6 with double records, 1e-3 with float records (the oracle steps the float-rounded
    state and actions the launch was given)"""
    m = tds_amd.load_model("ant")
    x = np.array(_states(n, na))
    x[:, 28:36] = _actions(n)[0]
    if dtype == "mixed":
        x = x.astype(np.float32).astype(np.float64)
    y_ref = diff_states.oracle_step(m)(x)
    y0 = _run(n, na, 1, False, dtype, 2)[0][0]  # (slot 0 of the y ring: the first of two steps in one launch)
    e = rel_err(y0, y_ref)
    print(f"{dtype}, {n} environments, NA {na}: first step of a two-step ring launch vs the oracle {e:.3e}")
    assert np.isfinite(y0).all() and e < (1e-6 if dtype == "f64" else 1e-3)
