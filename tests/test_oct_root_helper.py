"""The 8-lane kernel's helper wavefront without its exposed waits (csrc/tds_oct.hip, step-loop build for one wavefront per
SIMD — the unit's SOLO trait: the helper's control-block copy and rows_geom's batched reads).

What these tests guard, part by part:
  * the helper's copy of the control block (`hc`, read through OCT_HC): which rings a launch has, where they are, their strides
    and the two count-in pointers come from a copy made once per launch — ring launches, launches of one step (another ring
    position per launch), double and float records, and the shard layer's launches (peer stores: the copy decides the path,
    the peer table is still read per step) must store every record where the parent stored it;
  * rows_geom's two batches: a row window's operands are requested ahead of their uses, the root's velocities and the two
    constants with the first batch — every window of every Gauss-Seidel iteration passes through it, so the wavefront's largest
    contact count NA runs over no window (0), one (1, 2), the long window (3, 4), two (5), three (6 .. 8) and four (9), with
    pgs_iterations 1 and 3;
  * the visual poses and the count-in of the step before read the rings through the same copy: every pose of every step must be
    in its y record, also in a step without a row window (NA = 0) and for an environment the reset pool replaces.
Only the schedule changes, no expression: every comparison here is BIT FOR BIT.  The one-wavefront build (option oct_w2 = 0)
takes none of it and is the yardstick; launches of ONE step pass through every barrier once from a freshly loaded record,
launches of twelve carry registers and LDS regions from step to step.

The states, batches (5 environments: a partly filled wavefront | 8: exactly one | 9: one and a lane group | 24: three) and the
runner are tests/test_oct_behind2.py's, whose runs are shared (see there for what is exact with float records).  The shard
layer on one rank: every step's gathered record against ring launches of the one-wavefront build."""
import numpy as np
import pytest

import tds_amd
from tds_amd import hip_backend
from test_launch_plan import MI355X
from test_oct_behind2 import K, SLOTS, POSES, SIZES, _actions, _assert_equal, _run, _states, _torch

pytestmark = pytest.mark.gpu

COUNTS = list(range(10))  # the first wavefront's largest contact count
CASES = [(n, na) for n in SIZES for na in COUNTS]


@pytest.mark.parametrize("iters", [1, 3])
@pytest.mark.parametrize("n,na", CASES)
def test_ring_launch_equals_one_step_launches_and_the_one_wavefront_build(n, na, iters):
    ring = _run(n, na, 1, False, "f64", K, 1, iters)
    _assert_equal(f"{n} environments, NA {na}, pgs_iterations {iters}: one launch vs {K} launches", ring, _run(n, na, 1, True, "f64", K, 1, iters))
    _assert_equal(f"{n} environments, NA {na}, pgs_iterations {iters}: two wavefronts vs one", ring, _run(n, na, 0, False, "f64", K, 1, iters))


@pytest.mark.parametrize("iters", [1, 3])
@pytest.mark.parametrize("n,na", CASES)
def test_float_records(n, na, iters):
    ring, many = _run(n, na, 1, False, "mixed", K, 1, iters), _run(n, na, 1, True, "mixed", K, 1, iters)
    tag = f"float records, {n} environments, NA {na}, pgs_iterations {iters}"
    _assert_equal(f"{tag}, one launch: two wavefronts vs one", ring, _run(n, na, 0, False, "mixed", K, 1, iters))
    _assert_equal(f"{tag}, one-step launches: two wavefronts vs one", many, _run(n, na, 0, True, "mixed", K, 1, iters))
    # the first step of the two forms: one step from the same float record is the same computation (runs of their own: after
    # twelve steps slot 0 of the five-slot rings holds the eleventh)
    one, two = _run(n, na, 1, True, "mixed", 1, 1, iters), _run(n, na, 1, False, "mixed", 2, 1, iters)
    d0 = [int((one[i][0] != two[i][0]).sum()) for i in (0, 1)]
    print(f"{tag}, first step: a launch of one step vs the first of two: differing values {d0}")
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
    _assert_equal(f"reset pool, {dtype}, {n} environments: two wavefronts vs one", two, one)


def test_shard_layer_on_one_rank(built):
    """tds_hip_shard_step_many with the peer-store exchange and three loopback peers: the helper stores every step's record
    into four gathered rings and counts the slots in — pointers, strides and counters of the control block"""
    torch = _torch()
    m = tds_amd.load_model("ant")
    n, na, steps = 24, 3, K
    x, acts = np.array(_states(n, na)), np.array(_actions(n))
    a = torch.from_numpy(acts).cuda().contiguous()
    sh = hip_backend.HipShard(m, n, wire_dtype="f64", options={"shard_chunk": 64, "shard_peer": 2, "shard_peer_loopback": 3})
    ref = hip_backend.HipSim(m, n, options={"step_many_loop": 1, "oct_w2": 0})
    assert sh.sim.single_step_kernel()[0] == ref.single_step_kernel()[0] == "oct8"
    if torch.cuda.get_device_properties(sh.sim.device).multi_processor_count == MI355X["num_cus"]:
        plan = hip_backend.launch_plan_host(m, "f64", n, nsub=steps, rings=1, **MI355X)
        assert (plan["kernel"], plan["build"], plan["refused"]) == ("oct8", 3, False), plan
    for s in (sh.sim, ref):
        s.x.copy_(torch.from_numpy(x).cuda())
    ring = torch.zeros((steps, n, ref.obs_dim + 2), dtype=torch.float64, device="cuda")
    for rep in range(2):
        sh.step_many(a, steps, first_block=rep)
        assert sh.exchange_form() == "peer_stores" and sh.peer_count() == 3
        ref.step_many_rings(a, steps, ring, None, first_block=rep)
        torch.cuda.synchronize()
        for back in range(steps):
            got = sh.gathered_step(back)
            assert torch.equal(got[0].view(torch.int64), ring[steps - 1 - back].view(torch.int64)), (rep, back)
        sh.flush()
        assert torch.equal(sh.sim.x.view(torch.int64), ref.x.view(torch.int64)), rep
        assert torch.equal(sh.sim.y.view(torch.int64), ref.y.view(torch.int64)), rep
        assert sh.sim.y[:, POSES].abs().max() > 0
    sh.close()
