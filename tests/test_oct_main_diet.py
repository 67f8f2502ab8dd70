"""The 8-lane kernel's main wavefront without the instructions its result does not need (csrc/tds_oct.hip, every build of the
unit: main_kin's one sincos evaluation, the root chain's oct_*_0 helpers, main_dyn's totals).

What these tests guard, part by part:
  * tds_sincos2 (csrc/tds_step_shared.h): the joint's and the root angles' sines and cosines in one interleaved evaluation —
    both Cody-Waite reductions (quadrant boundaries: angles at k pi / 2 +- 1e-9, k = -3 .. 3; angles up to +- 50 rad) and the
    per-argument fallback (an angle beyond 1e5 takes the library routine for that argument of that lane only: the environment's
    wavefront-mates must not see it);
  * the root chain without its structural zeros (root_frame, the root's velocities and bias accelerations, the root dofs' bias
    forces, couplings and 6 x 6 block): every term that remains multiplies a root coordinate or velocity, so the states hold all
    six root coordinates and all six root velocities away from zero;
  * the totals' 8-lane sums without their pinning copy.
No expression that remains is rounded differently, in any build: among the kernel's forms every comparison is BIT FOR BIT
(int64 views: the sign of a zero counts) — a ring launch of twelve steps against twelve launches of one step, and against the
one-wavefront build (option oct_w2 = 0), over the wavefront's largest contact count 0 .. 9, pgs_iterations 1 and 3, double and
float records, and with the reset pool replacing environments inside the launch.  The states, batches (5, 8, 9, 24 environments)
and the runner are tests/test_oct_behind2.py's, whose runs are shared.  With float records a launch keeps its state in double
from step to step and between launches the state is the float record: twelve launches of one step and one launch of twelve are
different computations from the second step on — what is exact there, and asserted, is the first step of the two forms and each
form against the one-wavefront build's (tests/test_oct_behind2.py, tests/test_oct_root_helper.py).

Against the general kernel (create-time option oct = 0), which shares none of the changed code: single steps within relative
1e-9, tests/test_oct.py's bound for that comparison."""
import functools

import numpy as np
import pytest

import tds_amd
from tds_amd import hip_backend
from conftest import rel_err
from test_oct_behind2 import K, SLOTS, NAMES, POSES, SIZES, _run, _torch

pytestmark = pytest.mark.gpu

COUNTS = list(range(10))  # the first wavefront's largest contact count
CASES = [(n, na) for n in SIZES for na in COUNTS]


def _assert_same_bits(tag, a, b, steps=K):
    diff = [int((np.ascontiguousarray(p).view(np.int64) != np.ascontiguousarray(q).view(np.int64)).sum()) for p, q in zip(a, b)]
    print(f"{tag}: values that differ in a bit " + ", ".join(f"{nm} {d}" for nm, d in zip(NAMES, diff)))
    for nm, p in zip(NAMES, a):
        assert np.isfinite(p).all(), nm
    assert np.abs(a[0]).max() > 0 and np.abs(a[1][:, :, 2:-2]).max() > 0
    assert np.abs(a[0][:, :, POSES]).max() > 0
    assert diff == [0, 0, 0, 0]
    assert np.array_equal(a[0][(steps - 1) % SLOTS], a[2])


@pytest.mark.parametrize("iters", [1, 3])
@pytest.mark.parametrize("n,na", CASES)
def test_ring_launch_equals_one_step_launches_and_the_one_wavefront_build(n, na, iters):
    ring = _run(n, na, 1, False, "f64", K, 1, iters)
    tag = f"{n} environments, NA {na}, pgs_iterations {iters}"
    _assert_same_bits(f"{tag}: one launch vs {K} launches", ring, _run(n, na, 1, True, "f64", K, 1, iters))
    _assert_same_bits(f"{tag}: two wavefronts vs one", ring, _run(n, na, 0, False, "f64", K, 1, iters))


@pytest.mark.parametrize("iters", [1, 3])
@pytest.mark.parametrize("n,na", CASES)
def test_float_records(n, na, iters):
    ring, many = _run(n, na, 1, False, "mixed", K, 1, iters), _run(n, na, 1, True, "mixed", K, 1, iters)
    tag = f"float records, {n} environments, NA {na}, pgs_iterations {iters}"
    _assert_same_bits(f"{tag}, one launch: two wavefronts vs one", ring, _run(n, na, 0, False, "mixed", K, 1, iters))
    _assert_same_bits(f"{tag}, one-step launches: two wavefronts vs one", many, _run(n, na, 0, True, "mixed", K, 1, iters))
    # the first step of the two forms: one step from the same float record is the same computation (runs of their own: after
    # twelve steps slot 0 of the five-slot rings holds the eleventh)
    one, two = _run(n, na, 1, True, "mixed", 1, 1, iters), _run(n, na, 1, False, "mixed", 2, 1, iters)
    d0 = [int((np.ascontiguousarray(one[i][0]).view(np.int64) != np.ascontiguousarray(two[i][0]).view(np.int64)).sum()) for i in (0, 1)]
    print(f"{tag}, first step: a launch of one step vs the first of two: values that differ in a bit {d0}")
    assert np.abs(one[0][0][:, POSES]).max() > 0
    assert d0 == [0, 0]


@pytest.mark.parametrize("dtype", ["f64", "mixed"])
@pytest.mark.parametrize("n", SIZES)
def test_reset_pool_replaces_environments_inside_the_launch(n, dtype):
    na = 3
    two, one = _run(n, na, 1, False, dtype, K, 1, 1, 7), _run(n, na, 0, False, dtype, K, 1, 1, 7)
    first = _run(n, na, 1, True, dtype, 1, 1, 1, 7)[1][0, :, -1] != 0  # (the first step alone: its done flags)
    done = two[1][:, :, -1] != 0  # [slot, environment]: the last SLOTS steps
    print(f"reset pool, {dtype}, {n} environments: done in the first step {int(first.sum())}, in the last {SLOTS} steps {int(done.sum())}")
    # every sunk environment is replaced at the end of the first step, inside the launch, beside environments that are carried
    assert first[(np.arange(n) % 8) < 3].all() and not (first.all() and done.all())
    _assert_same_bits(f"reset pool, {dtype}, {n} environments: two wavefronts vs one", two, one)


# ---- against the general kernel: states that exercise what changed ----
N_KIND = 56  # per kind of state: seven wavefronts of the 8-lane kernel
QUADRANT = np.array([k * (np.pi / 2) + s * 1e-9 for k in range(-3, 4) for s in (-1.0, 1.0)])  # k pi / 2 +- 1e-9
# The root's second angle (x[4]) at an ODD multiple of pi / 2 is the gimbal lock of the Ant's root chain: its third revolute axis
# (sin y, -sin x cos y, cos x cos y) falls onto the first, e_x, and the root block of the mass matrix loses a rank — 1e-9 beside
# it no two factorisations agree (nor did they before this change).  There the comparison is on what does not pass through the
# factorisation: the visual poses, i.e. the kinematics of the sines and cosines under test (kind "pitch at the gimbal lock").
ODD = np.array([k * (np.pi / 2) + s * 1e-9 for k in (-3, -1, 1, 3) for s in (-1.0, 1.0)])
EVEN = np.array([k * (np.pi / 2) + s * 1e-9 for k in (-2, 0, 2) for s in (-1.0, 1.0)])
KINDS = ["full root motion", "quadrant boundaries", "angles up to 50 rad", "pitch at the gimbal lock"]


def _base(m, n, rng):
    """all six root coordinates and all six root velocities away from zero: roll, pitch, yaw up to +- 1 rad, angular velocities
    of a few rad/s; from lying inside the plane to airborne, as tests/test_oct.py's contact patterns"""
    nq, nd, adim = m.dof_q, m.dof_qd, m.action_dim
    ip = np.array([m.initial_poses[i] for i in range(adim)])
    sign = lambda shape: rng.choice([-1.0, 1.0], shape)
    x = np.zeros((n, m.input_dim))
    x[:, 0:2] = sign((n, 2)) * rng.uniform(0.2, 2, (n, 2))
    x[:, 2] = rng.uniform(0.05, 0.75, n)
    x[:, 3:6] = sign((n, 3)) * rng.uniform(0.05, 1.0, (n, 3))
    x[:, 6:nq] = ip + rng.uniform(-0.6, 0.6, (n, nq - 6))
    x[:, nq:nq + 3] = sign((n, 3)) * rng.uniform(0.2, 1.5, (n, 3))
    x[:, nq + 3:nq + 6] = sign((n, 3)) * rng.uniform(0.5, 4.0, (n, 3))
    x[:, nq + 6:nq + nd] = rng.uniform(-1.5, 1.5, (n, nd - 6))
    x[:, nq + nd:nq + nd + adim] = rng.uniform(-0.5, 0.5, (n, adim))
    x[:, -3:] = [15, 0.3, 3]
    return x


@functools.lru_cache(maxsize=None)
def _general_states():
    """read-only [4 N_KIND, input_dim], in the order of KINDS"""
    m = tds_amd.load_model("ant")
    rng = np.random.default_rng(41)
    full = _base(m, N_KIND, rng)
    quad = _base(m, N_KIND, rng)
    quad[:, 3:14] = rng.choice(QUADRANT, (N_KIND, 11))
    for e in range(len(QUADRANT)):  # every boundary on a joint, on the roll and on the yaw at least once, whatever the draw
        quad[e, 6 + e % 8] = QUADRANT[e]
        quad[e + 14, 3] = QUADRANT[e]
        quad[e + 28, 5] = QUADRANT[e]
    quad[:, 4] = EVEN[np.arange(N_KIND) % len(EVEN)]
    lock = _base(m, N_KIND, rng)
    lock[:, 3:14] = rng.choice(QUADRANT, (N_KIND, 11))
    lock[:, 4] = ODD[np.arange(N_KIND) % len(ODD)]
    far = _base(m, N_KIND, rng)
    far[:, 3:14] = rng.uniform(-50, 50, (N_KIND, 11))
    far[0, 3:14] = 50.0
    far[1, 3:14] = -50.0
    while (np.abs(np.cos(far[:, 4])) < 0.3).any():  # (away from the gimbal lock, see above)
        bad = np.abs(np.cos(far[:, 4])) < 0.3
        far[bad, 4] = rng.uniform(-50, 50, int(bad.sum()))
    x = np.concatenate([full, quad, far, lock])
    assert (np.abs(x[:, 0:6]) > 0).all() and (np.abs(x[:, m.dof_q:m.dof_q + 6]) > 0).all()
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _single_steps(iters, oct_):
    """(y, [obs | reward | done], state) after one single step of every state of _general_states(), as read-only numpy"""
    torch = _torch()
    m = tds_amd.load_model("ant").copy()
    m.pgs_iterations = iters
    x = _general_states()
    sim = hip_backend.HipSim(m, x.shape[0], options={} if oct_ else {"oct": 0})
    assert sim.single_step_kernel()[0] == ("oct8" if oct_ else "general")
    xd = torch.from_numpy(np.array(x)).cuda()
    y = sim.forward_zero(xd).cpu().numpy()
    obs = torch.zeros((x.shape[0], sim.obs_dim + 2), dtype=torch.float64, device="cuda")
    sim.x.copy_(xd)
    sim.step(None, 1, obs)
    out = (y, obs.cpu().numpy(), sim.x.cpu().numpy())
    for a in out:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("iters", [1, 3])
def test_visual_poses_at_the_gimbal_lock_against_the_general_kernel(iters):
    k = KINDS.index("pitch at the gimbal lock")
    rows = slice(k * N_KIND, (k + 1) * N_KIND)
    a, b = _single_steps(iters, 1)[0][rows][:, POSES], _single_steps(iters, 0)[0][rows][:, POSES]
    e = rel_err(a, b)
    print(f"ant (pgs_iterations {iters}), pitch at odd multiples of pi / 2 +- 1e-9: visual poses, oct8 vs general {e:.3e}")
    assert np.isfinite(a).all() and np.abs(a).max() > 0
    assert e < 1e-9


@pytest.mark.parametrize("kind", KINDS[:3])
@pytest.mark.parametrize("iters", [1, 3])
def test_single_steps_against_the_general_kernel(iters, kind):
    k = KINDS.index(kind)
    rows = slice(k * N_KIND, (k + 1) * N_KIND)
    oct8, gen = _single_steps(iters, 1), _single_steps(iters, 0)
    e = [rel_err(a[rows], b[rows]) for a, b in zip(oct8, gen)]
    print(f"ant (pgs_iterations {iters}), {kind}: oct8 vs general, y {e[0]:.3e}, obs record {e[1]:.3e}, state {e[2]:.3e}")
    for a in oct8:
        assert np.isfinite(a[rows]).all()
    assert np.abs(oct8[0][rows][:, POSES]).max() > 0
    assert max(e) < 1e-9
    assert (oct8[1][rows][:, -1] == gen[1][rows][:, -1]).all()


@pytest.mark.parametrize("which", ["joint", "root yaw"])
@pytest.mark.parametrize("form", ["single step", "ring launch"])
def test_an_angle_beyond_1e5_leaves_its_wavefront_mates_alone(form, which):
    """One environment of a wavefront holds a joint angle (or, the fallback's other argument, a root angle) beyond 1e5 rad: that
    lane takes the library routine for that argument.  Its wavefront-mates' results are bit for bit those of a run in which the
    environment holds an ordinary angle; its own are finite and, for the single step, the general kernel's within 1e-9."""
    torch = _torch()
    m = tds_amd.load_model("ant")
    n, env = 24, 11  # (the second wavefront of three, neither its first nor its last environment)
    x_far = _base(m, n, np.random.default_rng(43))
    x_far[:, 2] = np.maximum(x_far[:, 2], 0.3)
    x_near = np.array(x_far)
    col = 6 + 5 if which == "joint" else 5
    x_far[env, col] = 1.0e5 + 1234.5678
    others = np.arange(n) != env
    outs = []
    for x in (x_far, x_near):
        sim = hip_backend.HipSim(m, n, options={"step_many_loop": 1})
        assert sim.single_step_kernel()[0] == "oct8"
        xd = torch.from_numpy(x).cuda()
        if form == "single step":
            outs.append(sim.forward_zero(xd).cpu().numpy())
        else:
            sim.x.copy_(xd)
            acts = torch.from_numpy(np.random.default_rng(44).uniform(-0.4, 0.4, (4, n, 8))).cuda().contiguous()
            y_ring = torch.zeros((3, n, m.output_dim), dtype=torch.float64, device="cuda")
            obs_ring = torch.zeros((3, n, sim.obs_dim + 2), dtype=torch.float64, device="cuda")
            sim.step_many_rings(acts, 3, obs_ring, y_ring)
            torch.cuda.synchronize()
            outs.append(np.concatenate([y_ring.cpu().numpy(), obs_ring.cpu().numpy()], axis=2).transpose(1, 0, 2).reshape(n, -1))
    far, near = outs
    d = int((np.ascontiguousarray(far[others]).view(np.int64) != np.ascontiguousarray(near[others]).view(np.int64)).sum())
    own = int((far[env] != near[env]).sum())
    print(f"{which} beyond 1e5, {form}: wavefront-mates' values that differ in a bit {d}; the environment's own values that differ {own}")
    assert np.isfinite(far).all() and np.abs(far[:, POSES]).max() > 0
    assert own > 0  # (the angle reached the kernel)
    assert d == 0
    if form == "single step":
        gen = hip_backend.HipSim(m, n, options={"oct": 0})
        assert gen.single_step_kernel()[0] == "general"
        yg = gen.forward_zero(torch.from_numpy(x_far).cuda()).cpu().numpy()
        e = rel_err(far, yg)
        print(f"{which} beyond 1e5: oct8 vs general {e:.3e}")
        assert e < 1e-9
