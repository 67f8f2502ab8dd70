"""The 8-lane kernel's contact sweep, window by window (csrc/tds_oct.hip: main_sweep and the helper's row stages).

The sweep visits the 3 NA constraint rows of a wavefront (NA = the largest contact count among its eight environments) in
windows of eight: the window's positions are unrolled with a compile-time row index, and both wavefronts of a workgroup carry
the window's first position and its row buffer along two nested loops (Gauss-Seidel iterations, windows) with one barrier per
window.  What can go wrong there depends on NA alone, so every wavefront of the batch is built for one NA:

  0 rows | under one window: 1, 2, 4, 5, 6 | one window and a second of a single row: 3 (9 rows), 11 (33 rows) |
  exactly filled windows: 8 (24 rows), 16 (48 rows) | the maximum: 17 (51 rows, seven windows)

one state with exactly that many penetrating points and seven with at most as many (a 0 among them) at shuffled positions,
and five more states behind them: 93 environments, a ragged last workgroup.  With pgs_iterations 1, 2, 3 (the first and the
later iterations are different instances of the sweep; the row buffers take turns across an odd and an even number of
windows), on the two-wavefront builds and on the one-wavefront build (create-time option oct_w2: 1 the build for one
wavefront per SIMD, 3 the one for two, 0 one wavefront per workgroup)."""
import functools

import numpy as np
import pytest

import tds_amd
from tds_amd import hip_backend
from conftest import rel_err
import diff_states

pytestmark = pytest.mark.gpu

TARGETS = [0, 1, 2, 3, 4, 5, 6, 8, 11, 16, 17]
N = 8 * len(TARGETS) + 5
ITERS = [1, 2, 3]
BUILDS = [1, 3, 0]  # option oct_w2


def _model(iters):
    m = tds_amd.load_model("ant").copy()
    m.pgs_iterations = iters
    return m


@functools.lru_cache(maxsize=None)
def _batch():
    """(x [93, input_dim], contact counts [93]) — read-only"""
    m = tds_amd.load_model("ant")
    pool = diff_states.states("ant", 512, seed=0)
    c = diff_states.contact_counts("ant", m, pool, reference=False)
    assert diff_states.histogram(c, 17).min() >= 3, diff_states.histogram(c, 17)
    rng = np.random.default_rng(5)
    pick = []
    for t in TARGETS:
        top = np.flatnonzero(c == t)[0]
        zero = np.flatnonzero(c == 0)[t % 3]
        rest = rng.choice(np.flatnonzero(c <= t), 6)
        pick.extend(rng.permutation(np.r_[top, zero, rest]))
    pick.extend(np.flatnonzero(c >= 3)[:5])
    pick = np.array(pick)
    x, cx = pool[pick], c[pick]
    # the batch holds every case: checked on the host, before anything is stepped
    assert x.shape[0] == N
    assert [int(cx[8 * g:8 * g + 8].max()) for g in range(len(TARGETS))] == TARGETS
    assert all(int(cx[8 * g:8 * g + 8].min()) == 0 for g in range(len(TARGETS)))
    x.setflags(write=False)
    return x, cx


@functools.lru_cache(maxsize=None)
def _oracle_y(iters):
    y = diff_states.oracle_step(_model(iters))(np.array(_batch()[0]))
    y.setflags(write=False)
    return y


def _torch():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch


@pytest.mark.parametrize("w2", BUILDS)
@pytest.mark.parametrize("iters", ITERS)
def test_one_step_per_window_count_against_the_general_kernel_and_the_oracle(iters, w2):
    torch = _torch()
    m = _model(iters)
    x, _ = _batch()
    sim = hip_backend.HipSim(m, N, options={"oct_w2": w2})
    gen = hip_backend.HipSim(m, N, options={"oct": 0})
    assert sim.single_step_kernel()[0] == "oct8" and gen.single_step_kernel()[0] == "general"
    xd = torch.from_numpy(np.array(x)).cuda()
    y, yg = sim.forward_zero(xd).cpu().numpy(), gen.forward_zero(xd).cpu().numpy()
    assert np.isfinite(y).all()
    o1 = torch.zeros((N, sim.obs_dim + 2), dtype=torch.float64, device="cuda")
    o2 = torch.zeros_like(o1)
    for s_, o_ in ((sim, o1), (gen, o2)):
        s_.x.copy_(xd)
        s_.step(None, 1, o_)
    e_y, e_o, e_x = rel_err(y, yg), rel_err(o1.cpu().numpy(), o2.cpu().numpy()), rel_err(sim.x.cpu().numpy(), gen.x.cpu().numpy())
    e_ref = rel_err(y, _oracle_y(iters))
    print(f"pgs_iterations {iters}, oct_w2 {w2}: vs general kernel y {e_y:.3e} obs {e_o:.3e} x {e_x:.3e}; vs oracle {e_ref:.3e}")
    assert e_y < 1e-9 and e_o < 1e-9 and e_x < 1e-9
    assert e_ref < 1e-6


@pytest.mark.parametrize("dtype,w2,iters", [("f64", w2, it) for it in ITERS for w2 in BUILDS] + [("mixed", 1, 2)])
def test_seven_steps_in_one_launch_equal_single_steps(dtype, w2, iters):
    """7 steps as one step-loop launch (a fresh action block per step from block 2 on, 3 obs slots: the ring wraps twice) against
    the same steps as single launches: every y slot, the last three obs records, the final state.  Float records once: against
    the rounded records of the same launch with double records, as test_oct_step_loop_form_equals_single_steps."""
    torch = _torch()
    m = _model(iters)
    x, _ = _batch()
    steps, slots = 7, 3
    rng = np.random.default_rng(8)
    a = hip_backend.HipSim(m, N, dtype=dtype, options={"step_many_loop": 1, "oct_w2": w2})
    assert a.step_many_is_loop(steps) and a.single_step_kernel()[0] == "oct8"
    tdt = a.torch_dtype
    x0 = torch.from_numpy(np.array(x)).to(tdt).cuda()
    actions = torch.from_numpy(rng.uniform(-0.4, 0.4, (5, N, m.action_dim))).to(tdt).cuda().contiguous()
    a.x.copy_(x0)
    obs_ring = torch.zeros((slots, N, a.obs_dim + 2), dtype=tdt, device="cuda")
    y_ring = torch.zeros((steps, N, m.output_dim), dtype=tdt, device="cuda")
    a.step_many_rings(actions, steps, obs_ring, y_ring, first_block=2, obs_first=1)
    if dtype != "f64":
        a64 = hip_backend.HipSim(m, N, dtype="f64", options={"step_many_loop": 1, "oct_w2": w2})
        a64.x.copy_(x0.double())
        y64 = torch.zeros((steps, N, m.output_dim), dtype=torch.float64, device="cuda")
        o64 = torch.zeros((slots, N, a.obs_dim + 2), dtype=torch.float64, device="cuda")
        a64.step_many_rings(actions.double().contiguous(), steps, o64, y64, first_block=2, obs_first=1)
        e_y, e_o = rel_err(y_ring.double().cpu().numpy(), y64.cpu().numpy()), rel_err(obs_ring.double().cpu().numpy(), o64.cpu().numpy())
        print(f"float records, pgs_iterations {iters}: y {e_y:.3e} obs {e_o:.3e}")
        assert e_y < 2e-6 and e_o < 2e-6
        return
    b = hip_backend.HipSim(m, N, dtype=dtype, options={"step_many_loop": 0, "oct_w2": w2})
    b.x.copy_(x0)
    obs = torch.zeros((N, b.obs_dim + 2), dtype=tdt, device="cuda")
    worst = 0.0
    for k in range(steps):
        b.step(actions[(2 + k) % 5], 1, obs)
        e = rel_err(y_ring[k].cpu().numpy(), b.y.cpu().numpy())
        if k >= steps - slots:
            e = max(e, rel_err(obs_ring[(1 + k) % slots].cpu().numpy(), obs.cpu().numpy()))
        worst = max(worst, e)
        assert e < 1e-9, k
    e_x = rel_err(a.x.cpu().numpy(), b.x.cpu().numpy())
    print(f"pgs_iterations {iters}, oct_w2 {w2}: {steps} steps in one launch vs single steps: records {worst:.3e} state {e_x:.3e}")
    assert e_x < 1e-9
