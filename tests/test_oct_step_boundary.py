"""The 8-lane kernel's step boundary (csrc/tds_oct.hip: main_fin -> barrier (0) -> main_kin of the next step).

In the step-loop build for one wavefront per SIMD the main wavefront carries its state — its dof's q and qd, the root's
coordinates and velocities — from the integration into the next step's kinematics in registers, and holds the constants of the
top of the step across barrier (0); it reads the LDS record again only in the first step of a launch and where the reset pool
replaced the state of one of its environments.  A launch of ONE step reads everything from the record, so K steps in one ring
launch are held against K ring launches of one step each of the same build, BIT FOR BIT: every slot of the y ring and of the
[obs | reward | done] ring, and the final state.

  * option oct_w2 = 2 is the build for one wavefront per SIMD (carried state, early constants), oct_w2 = 3 the 256-register
    build (neither): both are compared, n = 8 (one workgroup), 13 (a ragged last workgroup), 64;
  * with the reset pool on, environments that end a step with done take a fresh state inside the launch: the carried registers
    of that wavefront are dropped for a reload.  Three environments of every wavefront start low (base z 0.20 .. 0.25: done
    after the first step); the test asserts that resets happened and that a wavefront mixed reset and non-reset environments
    in one step.

Measured on the parent commit (MI355X), the same comparisons: 0 differing values in every case — the bound is equality."""
import functools
import os

import numpy as np
import pytest

import tds_amd
from tds_amd import hip_backend

pytestmark = pytest.mark.gpu

K = 12
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ant.npz")


def _torch():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch


@functools.lru_cache(maxsize=None)
def _inputs(n, low):
    """(states [n, input_dim], actions [K, n, 8]) — read-only.  low: environments 0 .. 2 of every wavefront start below the
    termination height"""
    m = tds_amd.load_model("ant")
    rng = np.random.default_rng(100 + n)
    g = np.load(GOLDEN)["x"]
    x = g[rng.integers(0, g.shape[0], n)].copy()
    if low:
        sel = (np.arange(n) % 8) < 3
        x[sel, 2] = rng.uniform(0.20, 0.25, int(sel.sum()))
        x[~sel, 2] = np.maximum(x[~sel, 2], 0.45)
    a = rng.uniform(-0.4, 0.4, (K, n, m.action_dim))
    x.setflags(write=False)
    a.setflags(write=False)
    return x, a


def _sim(torch, n, w2, reset_seed):
    m = tds_amd.load_model("ant")
    sim = hip_backend.HipSim(m, n, options={"step_many_loop": 1, "oct_w2": w2})
    assert sim.single_step_kernel()[0] == "oct8" and sim.step_many_is_loop(K)
    if reset_seed is not None:
        sim.set_auto_reset(True, reset_seed)
    return m, sim


def _one_launch(torch, n, w2, low, reset_seed):
    """K steps as one ring launch: (y ring [K], obs ring [K], final state)"""
    m, sim = _sim(torch, n, w2, reset_seed)
    x, a = _inputs(n, low)
    sim.x.copy_(torch.from_numpy(np.array(x)).cuda())
    actions = torch.from_numpy(np.array(a)).cuda().contiguous()
    obs_ring = torch.zeros((K, n, sim.obs_dim + 2), dtype=torch.float64, device="cuda")
    y_ring = torch.zeros((K, n, m.output_dim), dtype=torch.float64, device="cuda")
    sim.step_many_rings(actions, K, obs_ring, y_ring)
    torch.cuda.synchronize()
    return y_ring.cpu().numpy(), obs_ring.cpu().numpy(), sim.x.cpu().numpy()


def _k_launches(torch, n, w2, low, reset_seed):
    """the same K steps as K ring launches of one step each (every launch reads the LDS record it has just filled)"""
    m, sim = _sim(torch, n, w2, reset_seed)
    x, a = _inputs(n, low)
    sim.x.copy_(torch.from_numpy(np.array(x)).cuda())
    actions = torch.from_numpy(np.array(a)).cuda().contiguous()
    obs_ring = torch.zeros((K, n, sim.obs_dim + 2), dtype=torch.float64, device="cuda")
    y_ring = torch.zeros((K, n, m.output_dim), dtype=torch.float64, device="cuda")
    for k in range(K):
        sim.step_many_rings(actions, 1, obs_ring, y_ring, first_block=k, obs_first=k, y_first=k)
    torch.cuda.synchronize()
    return y_ring.cpu().numpy(), obs_ring.cpu().numpy(), sim.x.cpu().numpy()


def _assert_equal(tag, one, many):
    diff = [int((a != b).sum()) for a, b in zip(one, many)]
    print(f"{tag}: differing values, one launch vs {K} launches: y ring {diff[0]}, obs ring {diff[1]}, state {diff[2]}")
    for name, a in zip(("y ring", "obs ring", "state"), one):
        assert np.isfinite(a).all(), name
    assert np.abs(one[0]).max() > 0 and np.abs(one[1][:, :, 2:-2]).max() > 0
    assert diff == [0, 0, 0]


@pytest.mark.parametrize("n", [8, 13, 64])
@pytest.mark.parametrize("w2", [2, 3])
def test_twelve_steps_in_one_launch_equal_twelve_launches_of_one_step(w2, n):
    torch = _torch()
    one = _one_launch(torch, n, w2, False, None)
    many = _k_launches(torch, n, w2, False, None)
    _assert_equal(f"oct_w2 {w2}, n {n}", one, many)


@pytest.mark.parametrize("n", [13, 64])
@pytest.mark.parametrize("w2", [2, 3])
def test_twelve_steps_in_one_launch_with_the_reset_pool_equal_twelve_launches(w2, n):
    torch = _torch()
    one = _one_launch(torch, n, w2, True, 7)
    many = _k_launches(torch, n, w2, True, 7)
    done = one[1][:, :, -1] != 0  # [step, environment]
    full = (n // 8) * 8  # (whole wavefronts)
    per_wave = done[:, :full].reshape(K, full // 8, 8)
    mixed = int((per_wave.any(axis=2) & ~per_wave.all(axis=2)).sum())
    print(f"oct_w2 {w2}, n {n}, reset pool: {int(done.sum())} resets in {K} steps, {mixed} (step, wavefront) pairs with reset and "
          f"non-reset environments side by side")
    assert done.sum() >= 1 and mixed >= 1
    assert not done.all(axis=0).all()  # (not every environment is reset in every step: the carried path is taken as well)
    _assert_equal(f"oct_w2 {w2}, n {n}, reset pool", one, many)
