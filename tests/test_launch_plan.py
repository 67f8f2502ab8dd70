"""The launch planner (csrc/tds_launch_plan.h) asked on the CPU (tds_hip_launch_plan_host): which kernel, build, LDS layout
and workgroup shape every kind of launch takes, pinned for an MI355X (256 compute units, 160 KiB of LDS each) and for a
smaller device.  No GPU.

TABLE reproduces, row by row, the rules of the code the planner replaced (launch(), tds_launch_step, step_many_as_loop,
the 8-lane range split, the chain launcher, the shard layer's exchange form) over models x dtypes x batch sizes on both
sides of the residency boundaries x the options that force a form."""
import pytest

import tds_amd
from tds_amd import hip_backend

MI355X = dict(num_cus=256, lds_per_cu=160 * 1024)
SMALL = dict(num_cus=80, lds_per_cu=64 * 1024)


def plan(name, n, dtype="f64", options=None, num_envs=None, device=MI355X, **req):
    with hip_backend.default_options(**(options or {})):
        return hip_backend.launch_plan_host(tds_amd.load_model(name), dtype, num_envs or n, n=n, **device, **req)


def host_plan_agrees(sim, m, n, dtype="f64", options=None, steps=8):
    """GPU tests: the handle's kernel choice and step_many form are the host plan's (on a device of the MI355X's shape)"""
    import torch

    if torch.cuda.get_device_properties(sim.device).multi_processor_count != MI355X["num_cus"]:
        return  # (the host plan is asked for 256 compute units)
    with hip_backend.default_options(**(options or {})):
        single = hip_backend.launch_plan_host(m, dtype, n, **MI355X)
        many = hip_backend.launch_plan_host(m, dtype, n, nsub=steps, **MI355X)
    assert sim.single_step_kernel()[0] == single["kernel"] and sim.step_many_is_loop(steps) == many["loop"]


# launch kinds: a single step, a step loop with record rings, an auto-reset step, an exchange launch (rings with progress
# counters), a refill pass of the reset pool
KINDS = (dict(), dict(nsub=8, rings=1), dict(reset_mode=1), dict(nsub=8, rings=1, progress=1), dict(nsub=4, pool_pass=1))
# (model, dtype, environments, options, "kernel/build[/layout of the general kernel]" per launch kind,
#  step_many(8) as one step-loop launch, environment range of the 8-lane kernel's calls, exchange after the launch)
TABLE = [
    ('ant', 'f64', 4096, {}, 'oct8/3 oct8/3 general/0/0 oct8/3 oct8/4', 1, 0, 1),
    ('ant', 'f64', 4097, {}, 'oct8/2 oct8/2 general/0/0 oct8/2 oct8/2', 1, 0, 1),
    ('ant', 'f64', 8192, {}, 'oct8/2 oct8/2 general/0/0 oct8/2 oct8/2', 1, 0, 1),
    ('ant', 'f64', 8193, {}, 'oct8/1 oct8/1 general/0/0 oct8/1 oct8/1', 1, 8192, 0),
    ('ant', 'f64', 16384, {}, 'oct8/1 oct8/1 general/0/0 oct8/1 oct8/1', 1, 8192, 0),
    ('ant', 'mixed', 4096, {}, 'oct8/3 oct8/3 general/0/0 oct8/3 oct8/4', 1, 0, 1),
    ('ant', 'f32', 4096, {}, 'general/1/1 general/1/1 general/0/0 general/1/1 general/0/2', 1, 0, 1),
    ('laikago_soft', 'f64', 6144, {}, 'quad16/1 quad16/1 general/0/0 general/0/0 quad16/1', 1, 0, 0),
    ('laikago_soft', 'f64', 6145, {}, 'quad16/8 quad16/8 general/0/0 general/0/0 quad16/8', 1, 0, 0),
    ('laikago_soft', 'f64', 8192, {}, 'quad16/8 quad16/8 general/0/0 general/0/0 quad16/8', 1, 0, 0),
    ('laikago_soft', 'f64', 8193, {}, 'quad16/1 quad16/1 general/0/0 general/0/0 quad16/1', 0, 0, 0),
    ('laikago_soft', 'mixed', 8192, {}, 'quad16/8 quad16/8 general/0/0 general/0/0 quad16/8', 1, 0, 0),
    ('laikago', 'f64', 4096, {}, 'quad16/1 quad16/1 general/0/0 general/0/0 quad16/1', 1, 0, 0),
    ('laikago', 'f64', 8193, {}, 'quad16/1 quad16/1 general/0/0 general/0/0 quad16/1', 0, 0, 0),
    ('pendulum5', 'f64', 4096, {}, 'chain8/0 chain8/2 general/0/0 chain8/2 chain8/0', 1, 0, 0),
    ('pendulum5', 'f64', 4097, {}, 'chain8/0 chain8/1 general/0/0 chain8/1 chain8/0', 1, 0, 0),
    ('pendulum5', 'f64', 8192, {}, 'chain8/0 chain8/1 general/0/0 chain8/1 chain8/0', 1, 0, 0),
    ('pendulum5', 'f64', 8193, {}, 'chain8/0 chain8/0 general/0/0 chain8/0 chain8/0', 1, 0, 0),
    ('pendulum5', 'mixed', 4096, {}, 'chain8/0 chain8/2 general/0/0 chain8/2 chain8/0', 1, 0, 0),
    ('pendulum5', 'f32', 4096, {}, 'general/0/0 general/0/0 general/0/0 general/0/0 general/0/2', 1, 0, 0),
    ('cartpole', 'f64', 4096, {}, 'chain8/0 chain8/2 general/0/0 chain8/2 chain8/0', 1, 0, 0),
    ('cartpole', 'f64', 8193, {}, 'chain8/0 chain8/0 general/0/0 chain8/0 chain8/0', 1, 0, 0),
    ('ant_floating', 'f64', 2048, {}, 'general/0/0 general/0/0 general/0/0 general/0/0 general/0/2', 0, 0, 0),
    ('ant_floating', 'f64', 16384, {}, 'general/0/0 general/0/0 general/0/0 general/0/0 general/0/2', 0, 0, 0),
    ('ant_floating', 'f32', 2048, {}, 'general/0/0 general/0/0 general/0/0 general/0/0 general/0/2', 0, 0, 0),
    ('humanoid', 'f64', 2048, {}, 'general/0/0 general/0/0 general/0/0 general/0/0 general/0/2', 0, 0, 0),
    ('humanoid', 'mixed', 4096, {}, 'general/0/0 general/0/0 general/0/0 general/0/0 general/0/2', 0, 0, 0),
    ('pendulum5_plane', 'f64', 4096, {}, 'general/1/1 general/1/1 general/0/0 general/1/1 general/0/2', 1, 0, 1),
    ('pendulum5_plane', 'f64', 4097, {}, 'general/0/0 general/0/0 general/0/0 general/0/0 general/0/2', 1, 0, 0),
    ('pendulum5_plane', 'f64', 12288, {}, 'general/0/0 general/0/0 general/0/0 general/0/0 general/0/2', 1, 0, 0),
    ('pendulum5_plane', 'f64', 12289, {}, 'general/0/0 general/0/0 general/0/0 general/0/0 general/0/2', 0, 0, 0),
    ('pendulum5_plane', 'f32', 4096, {}, 'general/1/1 general/1/1 general/0/0 general/1/1 general/0/2', 1, 0, 1),
    ('two_pendulums_plane', 'f64', 64, {}, 'general/0/0 general/0/0 general/0/0 general/0/0 general/0/2', 0, 0, 0),
    ('two_pendulums_plane', 'mixed', 4096, {}, 'general/0/0 general/0/0 general/0/0 general/0/0 general/0/2', 0, 0, 0),
    ('two_cubes_floating', 'f64', 4096, {}, 'general/0/0 general/0/0 general/0/0 general/0/0 general/0/2', 0, 0, 0),
    ('ant', 'f64', 4096, {'oct_w2': 0}, 'oct8/1 oct8/1 general/0/0 oct8/1 oct8/1', 1, 0, 1),
    ('ant', 'f64', 4096, {'oct_w2': 2}, 'oct8/3 oct8/3 general/0/0 oct8/3 oct8/4', 1, 0, 1),
    ('ant', 'f64', 4096, {'oct_w2': 3}, 'oct8/2 oct8/2 general/0/0 oct8/2 oct8/2', 1, 0, 1),
    ('ant', 'f64', 4096, {'pool_beside': 0}, 'oct8/3 oct8/3 general/0/0 oct8/3 oct8/3', 1, 0, 1),
    ('ant', 'f64', 4096, {'step_many_loop': 0}, 'oct8/3 oct8/3 general/0/0 oct8/3 oct8/4', 0, 0, 1),
    ('ant', 'f64', 16384, {'oct_w2': 2}, 'oct8/2 oct8/2 general/0/0 oct8/2 oct8/2', 1, 0, 0),
    ('pendulum5', 'f64', 8193, {'chain_w2': 0}, 'chain8/0 chain8/0 general/0/0 chain8/0 chain8/0', 1, 0, 0),
    ('pendulum5', 'f64', 8193, {'chain_w2': 2}, 'chain8/0 chain8/1 general/0/0 chain8/1 chain8/0', 1, 0, 0),
    ('pendulum5', 'f64', 8193, {'w2': 1}, 'chain8/0 chain8/0 general/0/0 chain8/0 chain8/0', 1, 0, 0),
    ('laikago_soft', 'f64', 8192, {'quad_wide': 0}, 'quad16/1 quad16/1 general/0/0 general/0/0 quad16/1', 0, 0, 0),
    ('laikago_soft', 'f64', 8192, {'quad_wide': 2}, 'quad16/8 quad16/8 general/0/0 general/0/0 quad16/8', 1, 0, 0),
    ('laikago_soft', 'f64', 8192, {'step_many_loop': 1}, 'quad16/8 quad16/8 general/0/0 general/0/0 quad16/8', 1, 0, 0),
    ('pendulum5_plane', 'f64', 4096, {'loop_w2': 0}, 'general/1/1 general/0/0 general/0/0 general/0/0 general/0/2', 1, 0, 0),
    ('pendulum5_plane', 'f64', 4096, {'loop_w2': 2}, 'general/1/1 general/1/1 general/0/0 general/1/1 general/0/2', 1, 0, 1),
    ('pendulum5_plane', 'f64', 4096, {'w2': 0}, 'general/0/0 general/0/0 general/0/0 general/0/0 general/0/2', 1, 0, 0),
    ('pendulum5_plane', 'f64', 4096, {'w2': 2}, 'general/1/1 general/1/1 general/0/0 general/1/1 general/0/2', 1, 0, 1),
    ('pendulum5_plane', 'f64', 4096, {'loop_occ': 1}, 'general/3/1 general/3/1 general/2/0 general/3/1 general/2/2', 1, 0, 1),
    ('pendulum5_plane', 'f64', 4096, {'loop_occ': 2}, 'general/5/1 general/5/1 general/4/0 general/5/1 general/4/2', 1, 0, 1),
    ('pendulum5_plane', 'f64', 4096, {'exchange_w2': 0}, 'general/1/1 general/1/1 general/0/0 general/0/0 general/0/2', 1, 0, 0),
    ('pendulum5_plane', 'f64', 16384, {'w2': 2}, 'general/1/1 general/1/1 general/0/0 general/1/1 general/0/2', 0, 0, 1),
]


@pytest.mark.parametrize("name,dtype,n,options,kinds,loop,env_range,after", TABLE)
def test_table_of_the_mi355x(name, dtype, n, options, kinds, loop, env_range, after, built):
    cells = []
    for req in KINDS:
        p = plan(name, n, dtype, options, **req)
        cells.append(f'{p["kernel"]}/{p["build"]}' + (f'/{p["layout"]}' if p["kernel"] == "general" else ""))
    many = plan(name, n, dtype, options, nsub=8)
    exchange = plan(name, n, dtype, options, nsub=8, rings=1, progress=1)
    assert " ".join(cells) == kinds
    assert (many["loop"], many["env_range"], exchange["exchange_after"]) == (bool(loop), env_range, bool(after))


def test_laikago_soft_step_loop_forms(built):
    # narrow workgroups up to 6144 environments, wide up to 8192, chained graphs beyond (tests/test_quad.py)
    for n, waves, loop in ((6144, 1, True), (6145, 8, True), (8192, 8, True), (8193, 1, False)):
        p = plan("laikago_soft", n, nsub=8, rings=1)
        assert (p["kernel"], p["build"], p["loop"]) == ("quad16", waves, loop), n
    assert plan("laikago_soft", 8192, nsub=8, rings=1)["threads_per_wg"] == 512
    assert not plan("laikago_soft", 8192, nsub=8, options={"quad_wide": 0})["loop"]
    # its exchange launches run on the general kernel, and its shards keep per-step launches
    assert plan("laikago_soft", 4096, nsub=8, rings=1, progress=1)["kernel"] == "general"


def test_ant_builds_and_ranges(built):
    # one-wavefront-per-SIMD build up to 4096, two-wavefront build up to 8192, ranges of 8192 beyond
    for n, build, rng in ((4096, 3, 0), (4097, 2, 0), (8192, 2, 0), (8193, 1, 8192), (16384, 1, 8192)):
        p = plan("ant", n, nsub=8, rings=1)
        assert (p["kernel"], p["build"], p["loop"], p["env_range"]) == ("oct8", build, True, rng), n
    # ... which the call never launches whole: each range launch is resident, the two-wavefront build
    assert plan("ant", 8192, nsub=8, rings=1, num_envs=16384)["build"] == 2
    # the exchange's launches stay whole
    assert plan("ant", 16384, nsub=8, rings=1, progress=1)["env_range"] == 0
    # refill passes of the reset pool beside one-wavefront-per-SIMD chunks: the 240-register build
    assert plan("ant", 64, nsub=4, pool_pass=1, num_envs=4096)["build"] == 4
    assert plan("ant", 64, nsub=4, pool_pass=1, num_envs=4097)["build"] == 3
    assert plan("ant", 4096, nsub=8, options={"oct_w2": 0})["build"] == 1
    assert plan("ant", 4096, reset_mode=1)["kernel"] == "general"


def test_chain_builds(built):
    # constants-in-registers recorder build up to 4096 environments, recorder build up to 8192, no recorder beyond
    for n, build in ((4096, 2), (4097, 1), (8192, 1), (8193, 0)):
        p = plan("pendulum5", n, nsub=8, rings=1)
        assert (p["kernel"], p["build"], p["loop"]) == ("chain8", build, True), n
    assert plan("pendulum5", 4096, nsub=8)["build"] == 0  # (no rings: nothing to record)
    assert plan("pendulum5", 16384, nsub=8, rings=1, options={"chain_w2": 2})["build"] == 1
    assert plan("cartpole", 64, nsub=8, rings=1, options={"chain_w2": 0})["build"] == 0


def test_general_kernel_forms(built):
    # pendulum5 on a plane: the two-wavefront build up to 4 workgroups per compute unit
    p = plan("pendulum5_plane", 4096)
    assert (p["kernel"], p["gen_build"] & 1, p["layout"], p["threads_per_wg"]) == ("general", 1, 1, 128)
    assert plan("pendulum5_plane", 4096, reset_mode=1)["layout"] == 0
    assert plan("pendulum5_plane", 4096, nsub=8, rings=1, progress=1, options={"exchange_w2": 0})["layout"] == 0
    assert plan("pendulum5_plane", 4096, nsub=8, rings=1, progress=1)["exchange_after"]
    assert plan("pendulum5_plane", 4096, prof=1)["layout"] == 0 and plan("pendulum5_plane", 4096, prof=2)["layout"] == 1
    assert plan("humanoid", 64)["kind"] == 2 and plan("ant_floating", 64)["kind"] == 1
    assert plan("two_pendulums_plane", 64)["kind"] == 3 and plan("two_cubes_floating", 64)["kind"] == 4
    assert plan("pendulum5_plane", 64, nsub=8, options={"loop_occ": 1, "w2": 0})["refused"]


def test_rules_follow_a_smaller_device(built):
    # the chain kernel's residency: 4 SIMDs per compute unit of THIS device (80 CUs: 320 SIMDs)
    for n, build in ((1280, 2), (1281, 1), (2560, 1), (2561, 0)):
        assert plan("pendulum5", n, nsub=8, rings=1, device=SMALL)["build"] == build, n
    # the general kernel's two-wavefront rule: workgroups per compute unit from this device's LDS and compute units
    big = [plan("pendulum5_plane", n)["layout"] for n in (512, 1024, 4096, 4097)]
    small = [plan("pendulum5_plane", n, device=SMALL)["layout"] for n in (512, 1024, 4096, 4097)]
    assert big == [1, 1, 1, 0] and small == [1, 0, 0, 0]
    # the Ant's builds and ranges
    assert plan("ant", 8192, nsub=8, rings=1, device=SMALL)["env_range"] > 0
    assert plan("ant", 8192, nsub=8, rings=1)["env_range"] == 0


def test_bad_arguments(built):
    m = tds_amd.load_model("ant")
    with pytest.raises(hip_backend.TdsHipError):
        hip_backend.launch_plan_host(m, "f64", 0)
    with pytest.raises(hip_backend.TdsHipError):
        hip_backend.launch_plan_host(tds_amd.load_model("humanoid"), "f32", 64)  # (no pure-float build of spherical joints)
