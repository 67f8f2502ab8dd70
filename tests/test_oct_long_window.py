"""The 8-lane kernel's long first window (csrc/tds_oct.hip: main_sweep; csrc/tds_oct_windows.h; option oct_long_window).

With 9 .. 12 constraint rows (NA = 3 or 4 contacts at most among a wavefront's environments) the main wavefront of a
two-wavefront workgroup does not start a second row window of one to four rows in the first Gauss-Seidel iteration: its
unrolled chain runs on through positions 8 .. 11 and takes the second window's barrier inside the chain.  Same operations per
row in the same order as window by window (option oct_long_window = 0), so the two are compared BIT FOR BIT, on the
93-environment batch of test_oct_sweep_windows.py: wavefronts of NA = 0, 1, 2, 3, 4, 5, 6, 8, 11, 16, 17 — both sides of both
boundaries (6 | 9 rows, 12 | 15 rows), the one-row tail (NA = 3), the full tail (NA = 4) — and a ragged last workgroup; under
1, 2 and 3 iterations (what follows the long window: the next step, or an ordinary first window of iteration 1 whose rows the
helper writes into the first buffer right behind the barrier inside the chain).

Measured on an MI355X (the last test; its bound is the suite's for that comparison, 1e-9): option 1 against the general
kernel after one step, y / obs / x alike and the same for oct_w2 1 and 3:  2.370e-12 (1 iteration), 4.170e-12 (2),
1.994e-12 (3).  The test prints them."""
import functools

import numpy as np
import pytest

import tds_amd
from tds_amd import hip_backend
from conftest import rel_err
from test_oct_sweep_windows import N, TARGETS, _batch

pytestmark = pytest.mark.gpu

STEPS, OBS_SLOTS = 6, 2


def _model(iters):
    m = tds_amd.load_model("ant").copy()
    m.pgs_iterations = iters
    return m


def _torch():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch


def test_the_batch_holds_long_and_ordinary_windows(built):
    """host side: which of the batch's wavefronts take the long window, and that both kinds are there"""
    long_ = [na for na in TARGETS if hip_backend.oct_window_plan_host(na, 1, 1)["long_window"]]
    assert long_ == [3, 4] and {2, 5}.issubset(TARGETS)


@functools.lru_cache(maxsize=None)
def _ring_launch(dtype, w2, iters, lw):
    """(y ring [6], obs ring [2 slots: it wraps], final state) of 6 steps in one ring launch — read-only"""
    torch = _torch()
    m = _model(iters)
    sim = hip_backend.HipSim(m, N, dtype=dtype, options={"step_many_loop": 1, "oct_w2": w2, "oct_long_window": lw})
    assert sim.single_step_kernel()[0] == "oct8" and sim.step_many_is_loop(STEPS) and sim.get_option("oct_long_window") == lw
    tdt = sim.torch_dtype
    sim.x.copy_(torch.from_numpy(np.array(_batch()[0])).to(tdt).cuda())
    actions = torch.from_numpy(np.random.default_rng(8).uniform(-0.4, 0.4, (5, N, m.action_dim))).to(tdt).cuda().contiguous()
    obs_ring = torch.zeros((OBS_SLOTS, N, sim.obs_dim + 2), dtype=tdt, device="cuda")
    y_ring = torch.zeros((STEPS, N, m.output_dim), dtype=tdt, device="cuda")
    sim.step_many_rings(actions, STEPS, obs_ring, y_ring, first_block=2, obs_first=1)
    torch.cuda.synchronize()
    out = tuple(t.cpu().numpy() for t in (y_ring, obs_ring, sim.x))
    for a in out:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("dtype,w2,iters", [("f64", w2, it) for it in (1, 2, 3) for w2 in (1, 3)] + [("f64", 0, 1), ("mixed", 1, 2)])
def test_ring_launch_is_bit_for_bit_the_same_with_and_without_the_long_window(dtype, w2, iters, built):
    """oct_w2 = 0 (one wavefront per workgroup) has no long window: the option changes nothing there either"""
    on, off = _ring_launch(dtype, w2, iters, 1), _ring_launch(dtype, w2, iters, 0)
    for name, a, b in zip(("y ring", "obs ring", "state"), on, off):
        assert np.isfinite(a).all(), name
        assert np.array_equal(a, b), (name, int((a != b).sum()))
    assert np.abs(on[0]).max() > 0 and np.abs(on[1]).max() > 0


@functools.lru_cache(maxsize=None)
def _single_step(w2, iters, options):
    """(y of forward_zero, obs record and state after one step) — read-only"""
    torch = _torch()
    m = _model(iters)
    opts = dict(options)
    if w2 is not None:
        opts["oct_w2"] = w2
    sim = hip_backend.HipSim(m, N, options=opts)
    assert sim.single_step_kernel()[0] == ("general" if opts.get("oct") == 0 else "oct8")
    xd = torch.from_numpy(np.array(_batch()[0])).cuda()
    y = sim.forward_zero(xd).cpu().numpy()
    obs = torch.zeros((N, sim.obs_dim + 2), dtype=torch.float64, device="cuda")
    sim.x.copy_(xd)
    sim.step(None, 1, obs)
    torch.cuda.synchronize()
    out = (y, obs.cpu().numpy(), sim.x.cpu().numpy())
    for a in out:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("w2", [1, 3])
def test_single_step_launch_is_bit_for_bit_the_same_with_and_without_the_long_window(w2, built):
    on = _single_step(w2, 1, (("oct_long_window", 1),))
    off = _single_step(w2, 1, (("oct_long_window", 0),))
    for name, a, b in zip(("y", "obs", "state"), on, off):
        assert np.isfinite(a).all(), name
        assert np.array_equal(a, b), (name, int((a != b).sum()))


@pytest.mark.parametrize("w2", [1, 3])
@pytest.mark.parametrize("iters", [1, 2, 3])
def test_one_step_with_the_long_window_against_the_general_kernel(iters, w2, built):
    on = _single_step(w2, iters, (("oct_long_window", 1),))
    gen = _single_step(None, iters, (("oct", 0),))
    e_y, e_o, e_x = (rel_err(a, b) for a, b in zip(on, gen))
    print(f"pgs_iterations {iters}, oct_w2 {w2}, long window: vs general kernel y {e_y:.3e} obs {e_o:.3e} x {e_x:.3e}")
    assert e_y < 1e-9 and e_o < 1e-9 and e_x < 1e-9
