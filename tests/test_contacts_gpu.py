"""The batched contact query on the GPU (tds_hip_contacts, csrc/tds_contact.hip) against its host instantiation, plus
what a handle owes its other users: untouched outputs, the shared work buffer, the stream, the refusals."""
import functools

import numpy as np
import pytest

import tds_amd
from tds_amd import hip_backend as hb

import diff_states as ds
from test_dynamics_gpu import records, rel
from test_jacobian_cpu import make_ref, needs_ref

pytestmark = pytest.mark.gpu

# device against host: the same template, no FP contraction on either side; only sin / cos (and sqrt's neighbours in
# libm) are the device's and the host's own.  The bound asked of every output is 1e-12; each test prints its maximum.
# Measured on the MI355X: ant 2.5e-14, laikago 4.8e-14, ant_floating 4.9e-14, pendulum5_plane 1.9e-13, cube_floating 0,
# cartpole_plane 9.6e-13 (sixteen active points on two dofs).
DEV_TOL = 1e-12
MODELS = ["ant", "laikago", "ant_floating", "cartpole_plane", "pendulum5_plane", "cube_floating"]


@functools.lru_cache(maxsize=None)
def sweep(name, n):
    """n seeded states spanning the model's contact counts (read-only, shared)"""
    x = np.ascontiguousarray(ds.states(name, n))
    x.setflags(write=False)
    return x


def cu(a):
    import torch

    return torch.from_numpy(np.array(a, dtype=np.float64, order="C")).cuda()  # (a copy: the sweeps are read-only)


def device_query(sim, x, want=hb.CONTACT_OUTPUTS):
    return {k: v.cpu().numpy() for k, v in sim.contacts(cu(x), want=want).items()}


def compare(name, got, m, x, idx):
    host = hb.contacts_host(m, x[idx])
    worst = 0.0
    for k in hb.CONTACT_OUTPUTS:
        assert got[k].shape == hb.contact_shapes(m, x.shape[0])[k]
        e = rel(got[k][idx], host[k])
        worst = max(worst, e)
        assert e <= DEV_TOL, (name, k, e)
    # a separated point's rows, right-hand side, impulse and force are exactly zero here too
    sep = host["contacts"][:, :, 9] >= 0
    sep3 = np.concatenate([sep, sep, sep], axis=1)
    for k in ("rows", "rhs", "impulse"):
        assert np.all(got[k][idx][sep3] == 0), (name, k)
    assert np.all(got["force"][idx][sep] == 0), name
    print(name, x.shape[0], "max rel device-host", worst)


@pytest.mark.parametrize("n", [1, 7, 65])
@pytest.mark.parametrize("name", MODELS)
def test_device_matches_host(name, n, built):
    """every state compared; 65: a partial wave and a partial second workgroup.  The states reach every contact count
    between none and all of the model's points"""
    m = tds_amd.load_model(name)
    x = sweep(name, 65)[:n]
    sim = hb.HipSim(m, 8, device=0, dtype="f64")
    got = device_query(sim, x)
    compare(name, got, m, x, np.arange(n))
    if n == 65 and name != "cartpole_plane":
        counts = (got["contacts"][:, :, 9] < 0).sum(axis=1)
        assert counts.min() == 0 and counts.max() >= ds.MAX_CONTACTS[name] - 1 and len(set(counts)) >= 4


@pytest.mark.parametrize("name", ["ant", "laikago"])
def test_device_matches_host_at_4096(name, built):
    m = tds_amd.load_model(name)
    x = sweep(name, 4096)
    sim = hb.HipSim(m, 64, device=0, dtype="f64")
    compare(name, device_query(sim, x), m, x, np.random.default_rng(1).choice(4096, 64, replace=False))


def test_device_matches_host_past_the_lane_cap(built):
    """16 384 + 37 environments: the grid's stride; the sample holds the last 37"""
    m = tds_amd.load_model("pendulum5_plane")
    n = 16384 + 37
    x = sweep("pendulum5_plane", n)
    sim = hb.HipSim(m, 64, device=0, dtype="f64")
    idx = np.concatenate([np.random.default_rng(1).choice(16384, 27, replace=False), np.arange(16384, n)])
    compare("pendulum5_plane", device_query(sim, x), m, x, idx)


def test_only_requested_outputs_are_written_and_out_buffers_are_reused(built):
    import torch

    m = tds_amd.load_model("ant")
    n = 33  # not the handle's num_envs
    x = cu(sweep("ant", 65)[:n])
    sim = hb.HipSim(m, 8, device=0, dtype="f64")
    full = sim.contacts(x)
    shapes = hb.contact_shapes(m, n)
    for want in (("force",), ("contacts", "jac"), ("qd_pre",), ("rows", "rhs"), ("delassus",), ("impulse", "qd_post")):
        bufs = {k: torch.full(shapes[k], -7.25, dtype=torch.float64, device="cuda") for k in hb.CONTACT_OUTPUTS}
        res = sim.contacts(x, want=want, out=bufs)
        torch.cuda.synchronize()
        for k in hb.CONTACT_OUTPUTS:
            if k in want:
                assert res[k] is bufs[k] and torch.equal(bufs[k], full[k]), k
            else:
                assert k not in res and bool((bufs[k] == -7.25).all()), k
    assert torch.equal(sim.contact_forces(x), full["force"])


def test_work_buffer_is_shared_with_the_other_queries(built):
    import torch

    m = tds_amd.load_model("ant")
    n = 16
    xn = sweep("ant", 65)[:n]
    rng = np.random.default_rng(4)
    xd, v = cu(xn), cu(rng.normal(size=(n, 2, m.input_dim)))
    w = cu(rng.normal(size=(n, 2, m.output_dim)))
    q, qd = cu(xn[:, :m.dof_q]), cu(xn[:, m.dof_q:m.dof_q + m.dof_qd])
    link = m.num_links - 1
    tgt = cu(rng.normal(0, 0.3, (n, 1, 3)))

    def others(sim):
        y, jv = sim.jvp(xd, v)
        _, wj = sim.vjp(xd, w)
        d = sim.dynamics(q, qd, want=("mass_matrix", "qdd"))
        ik = sim.inverse_kinematics(q, [link], tgt, max_iterations=3)
        return [y, jv, wj, d["mass_matrix"], d["qdd"], ik["q"], ik["residual"]]

    def same(a, b):
        return all(torch.equal(s, t) for s, t in zip(a, b))

    sim = hb.HipSim(m, n, device=0, dtype="f64")
    before = others(sim)
    c_before = sim.contacts(xd)
    sim.contacts(cu(np.tile(xn, (300, 1))))  # a larger query, with the Delassus matrix, grows the shared buffer
    assert same(others(sim), before)
    c_after = sim.contacts(xd)
    for k in c_before:
        assert torch.equal(c_after[k], c_before[k]), k
    fresh = hb.HipSim(m, n, device=0, dtype="f64")  # the other way round: the contact query first, the others grow
    c_fresh = fresh.contacts(xd)
    fresh.dynamics(cu(np.tile(xn[:, :m.dof_q], (600, 1))), want=("mass_matrix",))
    assert same(others(fresh), before)
    c_again = fresh.contacts(xd)
    for k in c_before:
        assert torch.equal(c_fresh[k], c_before[k]) and torch.equal(c_again[k], c_before[k]), k


def test_query_runs_on_the_handles_stream(built):
    """the query is ordered after earlier work on the stream given with tds_hip_set_stream: its input is filled there,
    behind a long-running kernel, and the call is made without any host wait"""
    import torch

    m = tds_amd.load_model("ant")
    n = 256
    x = sweep("ant", 4096)[:n]
    sim = hb.HipSim(m, n, device=0, dtype="f64")
    names = ("contacts", "impulse", "force", "qd_post")
    want = sim.contacts(cu(x), want=names)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    x_src, x_dev = cu(x), torch.zeros((n, m.input_dim), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        sim.use_current_stream()
        torch.cuda._sleep(200_000_000)  # ~0.1 s of device time ahead of the copy
        x_dev.copy_(x_src, non_blocking=True)
        got = sim.contacts(x_dev, want=names)
    side.synchronize()
    sim.use_current_stream()
    for k in want:
        assert torch.equal(got[k], want[k]), k


def test_refusals_on_the_device(built):
    m = tds_amd.load_model("ant")
    x = cu(records("ant", 4))
    for dt in ("f32", "mix"):
        try:
            s32 = hb.HipSim(m, 4, device=0, dtype=dt)
        except (hb.TdsHipError, ValueError, KeyError):
            continue
        with pytest.raises(hb.TdsHipError, match="error 2: step Jacobians: f64 handles only"):
            s32.contacts(x)
    for name, why in (("pendulum5_spherical", "spherical joints"), ("pendulum_and_cube", "worlds of several bodies")):
        mr = tds_amd.load_model(name)
        sr = hb.HipSim(mr, 2, device=0, dtype="f64")
        with pytest.raises(hb.TdsHipError, match=f"error 2: step Jacobians: {why} are not supported"):
            sr.contacts(cu(np.zeros((2, mr.input_dim))))
        out = cu(np.zeros((2, mr.dof_qd)))
        o = hb.ContactOut(qd_post=out.data_ptr())
        assert hb.lib().tds_hip_contacts(sr.h, 2, cu(np.zeros((2, mr.input_dim))).data_ptr(), o) == 2
    sim = hb.HipSim(m, 4, device=0, dtype="f64")
    assert hb.lib().tds_hip_contacts(sim.h, 4, x.data_ptr(), hb.ContactOut()) == 1  # no output requested


def test_model_without_a_plane(built):
    m = tds_amd.load_model("cartpole")
    x = records("cartpole", 9)
    sim = hb.HipSim(m, 4, device=0, dtype="f64")
    got = device_query(sim, x)
    assert got["contacts"].shape == (9, 0, 10) and got["force"].shape == (9, 0, 3)
    host = hb.contacts_host(m, x)
    assert rel(got["qd_post"], host["qd_post"]) <= DEV_TOL and rel(got["qd_pre"], host["qd_pre"]) <= DEV_TOL
    assert sim.contact_forces(cu(x)).shape == (9, 0, 3)


@needs_ref
def test_device_matches_reference_on_the_ant(built):
    """contacts, jac and the momentum identity against the reference built under oracle/_ref"""
    from test_contacts_cpu import MOMENTUM_BOUND

    m = tds_amd.load_model("ant")
    n = 64
    x = sweep("ant", 65)[:n]
    sim = hb.HipSim(m, n, device=0, dtype="f64")
    d = device_query(sim, x)
    r = make_ref("ant")
    try:
        qd_post_ref = r.step(x)[:, m.dof_q:m.dof_q + m.dof_qd]
        M = np.zeros((n, m.dof_qd, m.dof_qd))
        for e in range(n):
            dbg = r.debug(x[e], m)
            M[e] = dbg["M"]
            assert rel(d["contacts"][e], dbg["contacts"]) <= 1e-9
            assert rel(d["jac"][e], dbg["jac"]) <= 1e-9
    finally:
        r.close()
    lhs = np.einsum("eij,ej->ei", M, d["qd_pre"] - qd_post_ref)
    e1 = rel(np.einsum("erd,er->ed", d["rows"], d["impulse"]), lhs)
    e2 = rel(np.einsum("ecki,eck->ei", d["jac"], d["force"]) * m.dt, -lhs)
    print(f"ant x 64 on the device: momentum identities {e1:.3e}, {e2:.3e} (bound {MOMENTUM_BOUND:.1e})")
    assert max(e1, e2) <= MOMENTUM_BOUND


def test_contact_forces_of_settled_ants(built):
    """4096 Ants after 200 steps of HipSim.step on the resident records: the vertical forces are non-negative, and
    non-zero only where the point penetrates"""
    import torch

    m = tds_amd.load_model("ant")
    n = 4096
    sim = hb.HipSim(m, n, device=0, dtype="f64")
    sim.x.copy_(cu(records("ant", n)))
    for _ in range(200):
        sim.step()
    x = sim.x.clone()
    force = sim.contact_forces(x)
    dist = sim.contacts(x, want=("contacts",))["contacts"][:, :, 9]
    torch.cuda.synchronize()
    assert bool(torch.isfinite(force).all())
    up = torch.tensor(list(m.plane_normal[:]), dtype=torch.float64, device="cuda")
    vertical = force @ up
    assert bool((vertical >= 0).all())
    assert bool((force[dist >= 0] == 0).all())
    assert bool((vertical > 0).any()) and bool((dist < 0).any())
    # a settled Ant is carried: the vertical forces of an environment add up to the order of its weight
    weight = 9.81 * (m.base_mass + sum(m.links[i].mass for i in range(m.num_links)))
    total = vertical.sum(dim=1)
    print(f"settled ants: mean total vertical force {float(total.mean()):.3f} N, weight {weight:.3f} N, "
          f"{int((dist < 0).sum())} penetrating points")
