"""GPU: every build the general step kernel's build table holds for a key (csrc/tds_kernels.hip: tds_builds_of —
straight-line / step loop / phase stamps, each as one- and as two-wavefront workgroups) is reached through the public
API, launches, and computes what its neighbours compute.  The Ant with its own kernel switched off is the key (16 lanes,
14 padded dof) at 16 workgroups; the cartpole with its own kernel switched off the keys of up to 8 padded dof on 16, 32 and
64 lanes.  (The keys and kinds these two do not reach are run by tests/test_hip_parity.py.)"""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN, rel_err

import tds_amd
from tds_amd import hip_backend

pytestmark = pytest.mark.gpu

N = 64
STEPS = 3
# straight-line against step-loop build: two separately compiled kernels, agreement to round-off —
# the bound of tests/test_hip_parity.py: test_substeps_in_kernel_equal_repeated_steps
LOOP_TOL = 1e-9
NSTAMPS = 14

# (id, model, what keeps it on the general kernel, lanes per environment, what asks for the two-wavefront form: the
#  default rule takes it for a world with contact points at this size; without contact points it has to be asked for)
KEYS = [("ant_16x14", "ant", {"oct": 0}, None, {}),
        ("cartpole_16x8", "cartpole", {"chain": 0}, 16, {"w2": 1}),
        ("cartpole_32x8", "cartpole", {"chain": 0}, 32, {"w2": 1}),
        ("cartpole_64x8", "cartpole", {"chain": 0}, 64, {"w2": 1})]


def _stamps(sim, two_waves):
    """the raw stamps of one stamped step from sim.x into sim.y: [main wavefront's 14], [helper's 1 .. 8] (or None)"""
    epb = sim.kernel_info()["envs_per_block"]
    n = 2 * NSTAMPS + 2 * ((sim.num_envs + epb - 1) // epb) if two_waves else NSTAMPS
    buf = (C.c_longlong * n)()
    rc = hip_backend.lib().tds_hip_profile_phases(sim.h, buf, n)
    assert rc == 0, rc
    st = list(buf)
    return st[:NSTAMPS], (st[NSTAMPS + 1:NSTAMPS + 9] if two_waves else None)


def _nondecreasing(v):
    return all(b >= a for a, b in zip(v, v[1:]))


@pytest.mark.parametrize("key", KEYS, ids=[k[0] for k in KEYS])
def test_every_build_of_a_key_launches_and_agrees(key, built):
    import torch

    _, name, general, lanes, ask_w2 = key
    m = tds_amd.load_model(name)
    has_contacts = name == "ant"  # (the golden Ant states drawn below stand on the plane; the cartpole has no contact points)
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    rng = np.random.default_rng(5)
    x = torch.from_numpy(g["x"][rng.integers(0, g["x"].shape[0], N)]).cuda().contiguous()
    acts = None
    if m.action_dim > 0:
        acts = torch.from_numpy(rng.uniform(-0.4, 0.4, (STEPS, N, m.action_dim))).cuda().contiguous()

    for two_waves in (False, True):
        opts = dict(general, **(ask_w2 if two_waves else {"w2": 0}))
        sim = hip_backend.HipSim(m, N, dtype="f64", lanes_per_env=lanes, options=opts)
        assert sim.single_step_kernel()[0] == "general"
        assert lanes is None or sim.kernel_info()["lanes_per_env"] == lanes
        # ---- straight-line build, and its stamped twin: the same y, bit for bit; the stamps in order
        y = sim.forward_zero(x).clone()
        sim.x.copy_(x)
        main, helper = _stamps(sim, two_waves)
        print(f"{key[0]} two_waves={two_waves}: main {[v - main[0] for v in main]}"
              + (f" helper {[v - main[0] for v in helper]}" if helper else ""))
        assert torch.equal(sim.y.view(torch.int64), y.view(torch.int64)), (key[0], two_waves)
        # (stamps nobody takes: 10 / 11 close the Jacobian rows and the row solves, which a wavefront without contacts
        #  skips; in the two-wavefront form those are the helper's phases, and 10 is the slot of the optional probe)
        skipped = {10} if two_waves else set()
        if not has_contacts:
            skipped |= {10, 11}
        taken = [v for k, v in enumerate(main) if k not in skipped]
        assert all(v != 0 for v in taken) and _nondecreasing(taken), main
        if two_waves:
            # (the two-wavefront form was the one stamped: the helper wavefront's stamps exist)
            assert all(v != 0 for v in helper) and _nondecreasing(helper), helper
        # ---- step-loop builds against chained single steps of the straight-line build
        sim.x.copy_(x)
        for k in range(STEPS):
            sim.step(None if acts is None else acts[k], 1)
        ref_x, ref_y = sim.x.clone().cpu().numpy(), sim.y.clone().cpu().numpy()
        # (a two-wavefront handle: its two-wavefront loop build, then — option loop_w2 = 0 — the one-wavefront one)
        for loop_w2 in ((None, 0) if two_waves else (None,)):
            if loop_w2 is not None:
                sim.set_option("loop_w2", loop_w2)
            sim.x.copy_(x)
            assert sim.step_many_is_loop(STEPS)
            sim.step_many(acts, STEPS)
            torch.cuda.synchronize()
            ex, ey = rel_err(sim.x.cpu().numpy(), ref_x), rel_err(sim.y.cpu().numpy(), ref_y)
            print(f"{key[0]} two_waves={two_waves} loop_w2={loop_w2}: {STEPS}-step loop vs {STEPS} launches: x {ex:.2e}, y {ey:.2e}")
            assert ex < LOOP_TOL and ey < LOOP_TOL, (key[0], two_waves, loop_w2, ex, ey)
        sim.close()
