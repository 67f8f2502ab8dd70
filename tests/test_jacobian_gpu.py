"""GPU: the step Jacobians' kernel (tds_jvp.hip) against the host instantiation of the same template, the primal
against forward_zero, selections and accumulation, the autograd Function, and what is refused."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

import tds_amd
from tds_amd import hip_backend as hb

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(ROOT, "oracle"))
import reflib  # noqa: E402  (checker only)

SUPPORTED = ["ant", "ant_floating", "laikago", "laikago_floating", "laikago_floating_env", "laikago_soft",
             "cartpole", "cartpole_plane", "pendulum5", "pendulum5_plane", "cube_floating"]


def records(name, n, seed=0):
    g = np.load(os.path.join(ROOT, "tests", "golden", f"{name}.npz"))
    rng = np.random.default_rng(seed)
    return g["x"][rng.integers(0, g["x"].shape[0], n)]


def sim_for(name, n, dtype="f64"):
    return hb.HipSim(tds_amd.load_model(name), n, device=0, dtype=dtype)


@pytest.mark.parametrize("n", [1, 7, 4096])
@pytest.mark.parametrize("name", SUPPORTED)
def test_device_jacobian_matches_host(name, n, built):
    import torch

    m = tds_amd.load_model(name)
    x = records(name, n)
    sim = sim_for(name, n)
    y = torch.empty((n, m.output_dim), dtype=torch.float64, device="cuda")
    jac = sim.jacobian(torch.from_numpy(x).cuda(), y=y).cpu().numpy()
    # the host instantiation on a sample of environments (all of them for the small batches)
    idx = np.arange(n) if n <= 7 else np.r_[np.arange(8), np.arange(n - 8, n), np.arange(8, n, 509)]
    jac_h, y_h = hb.jacobian_host(m, x[idx], want_y=True)
    assert np.max(np.abs(jac[idx] - jac_h)) / max(1.0, np.max(np.abs(jac_h))) <= 1e-12
    assert np.max(np.abs(y.cpu().numpy()[idx] - y_h) / np.maximum(np.abs(y_h), 1.0)) <= 1e-12
    assert np.all(np.isfinite(jac))


@pytest.mark.parametrize("name", SUPPORTED)
def test_jvp_primal_is_forward_zero_and_jvp_is_J_v(name, built):
    import torch

    n, k = 33, 3
    m = tds_amd.load_model(name)
    sim = sim_for(name, n)
    x = torch.from_numpy(records(name, n, 1)).cuda()
    v = torch.from_numpy(np.random.default_rng(2).normal(size=(n, k, m.input_dim))).cuda()
    y, jv = sim.jvp(x, v)
    y_fz = sim.forward_zero(x)
    torch.cuda.synchronize()
    assert (torch.abs(y - y_fz) / torch.clamp(torch.abs(y_fz), min=1.0)).max().item() <= 1e-10
    J = sim.jacobian(x)
    jv_ref = torch.bmm(v, J.transpose(1, 2))
    assert (torch.abs(jv - jv_ref).max() / torch.clamp(torch.abs(jv_ref).max(), min=1.0)).item() <= 1e-12
    y1, jv1 = sim.jvp(x, v[:, 0])
    assert torch.equal(jv1, jv[:, 0]) and torch.equal(y1, y)


def test_selection_and_accumulation_are_slices_of_the_dense_result(built):
    import torch

    n = 257
    m = tds_amd.load_model("ant")
    sim = sim_for("ant", n)
    x = torch.from_numpy(records("ant", n, 3)).cuda()
    dense = sim.jacobian(x)
    nq, nd = m.dof_q, m.dof_qd
    rows = list(range(nq + nd))  # [q | qd] rows
    cols = [38, 0, 17, 29, 5]
    assert torch.equal(sim.jacobian(x, rows=rows), dense[:, rows])
    assert torch.equal(sim.jacobian(x, cols=cols), dense[:, :, cols])
    assert torch.equal(sim.jacobian(x, rows=rows, cols=cols), dense[:, rows][:, :, cols])
    d = dense.cpu().numpy()
    s = d[0].copy()
    for i in range(1, n):  # the emitter's host loop order
        s += d[i]
    np.testing.assert_array_equal(sim.jacobian(x, accumulate="sum").cpu().numpy(), s)
    np.testing.assert_array_equal(sim.jacobian(x, accumulate="mean").cpu().numpy(), s / n)
    np.testing.assert_array_equal(sim.jacobian(x, rows=rows, cols=cols, accumulate="mean").cpu().numpy(),
                                  s[rows][:, cols] / n)


@pytest.mark.parametrize("name", ["ant", "laikago"])
def test_jacobian_matches_central_differences_of_reference(name, built):
    if not reflib.available():
        pytest.fail("oracle/_ref (built by build()) is missing")
    import torch

    r = reflib.RefSim(name)
    try:
        m = tds_amd.load_model(name)
        x = records(name, 4, 5)
        sim = sim_for(name, 4)
        jac = sim.jacobian(torch.from_numpy(x).cuda()).cpu().numpy()
        checked = 0
        for e in range(4):
            r.step(x[e:e + 1])
            base = r.last_penetrating_contacts()
            J_fd = np.zeros_like(jac[e])
            same = True
            for j in range(m.input_dim):
                h = 1e-6 * max(1.0, abs(x[e, j]))
                xp, xm = x[e].copy(), x[e].copy()
                xp[j] += h
                xm[j] -= h
                yp = r.step(xp[None])[0]
                same &= r.last_penetrating_contacts() == base
                ym = r.step(xm[None])[0]
                same &= r.last_penetrating_contacts() == base
                J_fd[:, j] = (yp - ym) / (2 * h)
            if not same:
                continue
            assert np.max(np.abs(jac[e] - J_fd)) / max(1.0, np.max(np.abs(jac[e]))) <= 1e-5
            checked += 1
        assert checked >= 1
    finally:
        r.close()


@pytest.mark.parametrize("name", ["cartpole", "ant"])
def test_gradcheck_of_step_fn(name, built):
    import torch

    n = 2
    m = tds_amd.load_model(name)
    sim = sim_for(name, n)
    x = torch.from_numpy(records(name, n, 7)).cuda()
    if m.step_mode == tds_amd.TDS_STEP_LOCOMOTION:  # actions well inside the clamp: a smooth state
        nq, nd = m.dof_q, m.dof_qd
        x[:, nq + nd:nq + nd + m.action_dim] *= 0.1
    x.requires_grad_(True)
    f = tds_amd.step_fn(sim)
    assert torch.autograd.gradcheck(f, (x,), eps=1e-6, atol=1e-5, rtol=1e-4, nondet_tol=0.0)
    y = f(x)
    (g,) = torch.autograd.grad(y.sum(), x)
    J = sim.jacobian(x.detach())
    assert torch.allclose(g, J.sum(1), rtol=1e-12, atol=1e-12)


def test_f32_handles_and_unsupported_models_are_refused(built):
    import torch

    for dtype in ("f32", "mixed"):
        sim = sim_for("ant", 4, dtype)
        x = torch.zeros((4, sim.input_dim), dtype=torch.float64, device="cuda")
        with pytest.raises(hb.TdsHipError, match="f64"):
            sim.jacobian(x)
    for name in ("humanoid_spherical", "pendulum5_spherical"):
        sim = sim_for(name, 4)
        x = torch.from_numpy(records(name, 4)).cuda()
        with pytest.raises(hb.TdsHipError, match="spherical"):
            sim.jacobian(x)
        with pytest.raises(hb.TdsHipError, match="spherical"):
            sim.jvp(x, x)


def test_cudalib_jacobian_through_ctypes_like_cuda_function(built):
    """cudalib_ant.so's <model>_jacobian, called the way CudaFunction<double> calls it (src/utils/cuda/
    cuda_function.hpp:78-140): meta, allocate, send_global, send_local, the call, deallocate.  Slot 0 is the MEAN of
    the per-environment Jacobians tds_hip_jacobian returns (cuda_codegen.hpp:218-228), slots i >= 1 are those."""
    import ctypes as C

    import torch

    L = C.CDLL(os.path.join(ROOT, "tiny-differentiable-simulator_amd", "cudalib_ant.so"))

    class Meta(C.Structure):
        _fields_ = [("output_dim", C.c_int), ("local_input_dim", C.c_int),
                    ("global_input_dim", C.c_int), ("accumulated_output", C.c_bool)]

    names = C.POINTER(C.c_char_p)()
    count = C.c_int(0)
    L.model_info(C.byref(names), C.byref(count))
    base = names[0].decode() + "_jacobian"
    fn = getattr(L, base)
    meta = getattr(L, base + "_meta")
    meta.restype = Meta
    alloc, dealloc = getattr(L, base + "_allocate"), getattr(L, base + "_deallocate")
    send_local, send_global = getattr(L, base + "_send_local"), getattr(L, base + "_send_global")
    send_local.restype = send_global.restype = C.c_bool
    send_local.argtypes = [C.c_int, C.c_void_p]
    send_global.argtypes = [C.c_void_p]
    fn.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p]

    m = tds_amd.load_model("ant")
    md = meta()
    assert (md.output_dim, md.local_input_dim, md.global_input_dim, md.accumulated_output) == \
        (m.output_dim * m.input_dim, m.input_dim, 0, True)
    n = 37
    x = np.ascontiguousarray(records("ant", n, 11))
    out = np.zeros((n, md.output_dim))
    alloc(n)
    try:
        assert send_global(x.ctypes.data)
        assert send_local(n, x.ctypes.data)
        fn(n, 1, n, out.ctypes.data)
    finally:
        dealloc()
    sim = sim_for("ant", n)
    J = sim.jacobian(torch.from_numpy(x).cuda()).cpu().numpy()  # [n][output_dim][input_dim]
    flat = J.reshape(n, -1)  # output-major rows
    np.testing.assert_array_equal(out[1:], flat[1:])
    s = flat[0].copy()
    for i in range(1, n):
        s += flat[i]
    np.testing.assert_array_equal(out[0], s / n)
    np.testing.assert_allclose(out[0], flat.mean(0), rtol=1e-12, atol=1e-12)
