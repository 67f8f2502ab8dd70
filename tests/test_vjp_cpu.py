"""CPU: the step VJPs' host instantiation (tds_diff_step.h over TdsRev, tds_hip_vjp_host) against w^T J of the
forward-mode host Jacobian, its primal against the double step, cotangents on entries the step does not write, tape
overflow and what is refused."""
import os

import numpy as np
import pytest

from conftest import ROOT

import tds_amd
from tds_amd import hip_backend as hb

SUPPORTED = ["ant", "ant_floating", "laikago", "laikago_floating", "laikago_floating_env", "laikago_soft",
             "cartpole", "cartpole_plane", "pendulum5", "pendulum5_plane", "cube_floating"]
REFUSED = ["humanoid", "humanoid_spherical", "pendulum5_spherical", "two_cubes_floating", "pendulum_and_cube"]


def golden(name, k=6):
    g = np.load(os.path.join(ROOT, "tests", "golden", f"{name}.npz"))
    return g["x"][:k]


def n_written(m):
    """entries of y the step writes (tds_diff_ny): q | qd | 7 per visual | up . z"""
    return m.dof_q + m.dof_qd + (7 * m.num_visuals + 1 if m.pack_visuals else 0)


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("name", SUPPORTED)
def test_vjp_host_is_w_times_jacobian_host(name, k, built):
    m = tds_amd.load_model(name)
    x = golden(name)
    w = np.random.default_rng(10 + k).normal(size=(x.shape[0], k, m.output_dim))
    wj = hb.vjp_host(m, x, w)
    assert wj.shape == (x.shape[0], k, m.input_dim)
    ref = np.einsum("nko,noi->nki", w, hb.jacobian_host(m, x))
    assert np.max(np.abs(wj - ref)) / max(1.0, np.max(np.abs(ref))) <= 1e-11
    assert np.count_nonzero(wj) > 0


@pytest.mark.parametrize("name", SUPPORTED)
def test_primal_of_vjp_host_is_the_double_step(name, built):
    m = tds_amd.load_model(name)
    x = golden(name, 3)
    w = np.random.default_rng(1).normal(size=(3, m.output_dim))
    wj, y = hb.vjp_host(m, x, w, want_y=True)
    assert wj.shape == (3, m.input_dim)
    y_ref = hb.step_host(m, x)
    assert np.max(np.abs(y - y_ref) / np.maximum(np.abs(y_ref), 1.0)) <= 1e-12


@pytest.mark.parametrize("name", ["ant", "laikago", "laikago_soft", "laikago_floating_env"])
def test_cotangent_on_unwritten_outputs_gives_zero(name, built):
    m = tds_amd.load_model(name)
    ny = n_written(m)
    assert ny < m.output_dim
    x = golden(name, 2)
    w = np.zeros((2, 2, m.output_dim))
    w[:, :, ny:] = np.random.default_rng(3).normal(size=(2, 2, m.output_dim - ny))
    wj = hb.vjp_host(m, x, w)
    assert np.all(wj == 0.0)


def test_one_cotangent_per_row_gives_the_jacobian(built):
    m = tds_amd.load_model("pendulum5_plane")
    x = golden("pendulum5_plane", 2)
    w = np.broadcast_to(np.eye(m.output_dim), (2, m.output_dim, m.output_dim))
    jac = hb.jacobian_host(m, x)
    assert np.max(np.abs(hb.vjp_host(m, x, w) - jac)) / max(1.0, np.max(np.abs(jac))) <= 1e-13


@pytest.mark.parametrize("name", REFUSED)
def test_unsupported_models_are_refused(name, built):
    m = tds_amd.load_model(name)
    with pytest.raises(hb.TdsHipError, match="not supported") as e_vjp:
        hb.vjp_host(m, np.zeros((1, m.input_dim)), np.zeros((1, m.output_dim)))
    with pytest.raises(hb.TdsHipError) as e_jac:
        hb.jacobian_host(m, np.zeros((1, m.input_dim)))
    assert str(e_vjp.value) == str(e_jac.value)


def test_tape_lengths_fit_the_class_capacity(built):
    """every golden record of every supported model records within its class's capacity (no -1)"""
    for name in SUPPORTED:
        m = tds_amd.load_model(name)
        x = np.load(os.path.join(ROOT, "tests", "golden", f"{name}.npz"))["x"]
        _, lens = hb.vjp_host(m, x, np.zeros((x.shape[0], m.output_dim)), tape_len=True)
        assert np.all(lens > 0), name


def test_tape_overflow_is_an_error_with_nan_outputs(built):
    import ctypes as C

    m = tds_amd.load_model("ant")
    x_all = np.load(os.path.join(ROOT, "tests", "golden", "ant.npz"))["x"]
    _, lens = hb.vjp_host(m, x_all, np.zeros((x_all.shape[0], m.output_dim)), tape_len=True)
    short, long_ = int(np.argmin(lens)), int(np.argmax(lens))
    assert lens[short] < lens[long_]
    x = np.ascontiguousarray(x_all[[short, long_]])
    w = np.ones((2, m.output_dim))
    with pytest.raises(hb.TdsHipError, match="tape exceeds the capacity"):
        hb.vjp_host(m, x, w, tape_cap=int(lens[short]) - 1)
    # a capacity between the two: NaN for the environment that overflows, the exact result for the one that fits
    wj = np.zeros((2, m.input_dim))
    y = np.zeros((2, m.output_dim))
    got = np.zeros(2, dtype=np.int32)
    rc = hb.lib().tds_hip_vjp_host_tape(C.byref(m), 2, x.ctypes.data, 1, w.ctypes.data, y.ctypes.data,
                                        wj.ctypes.data, int(lens[short]), got.ctypes.data)
    assert rc == 2  # TDS_ERR_UNSUPPORTED
    assert got[0] == lens[short] and got[1] == -1
    assert np.all(np.isnan(wj[1])) and np.all(np.isnan(y[1]))
    np.testing.assert_array_equal(wj[0], hb.vjp_host(m, x[:1], w[:1])[0])


def test_bad_cotangent_shape_is_rejected(built):
    m = tds_amd.load_model("cartpole")
    with pytest.raises(ValueError):
        hb.vjp_host(m, np.zeros((2, m.input_dim)), np.zeros((2, m.output_dim + 1)))
