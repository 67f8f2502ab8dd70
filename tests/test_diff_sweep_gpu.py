"""GPU: the step-derivative kernels (tds_jvp.hip, tds_vjp.hip, tds_dparam.hip) over 4096-state contact sweeps of the Ant,
Laikago and the floating cube (tests/diff_states.py), laid out so that one wavefront alternates minimum- and
maximum-contact states (the shortest and the longest tapes side by side) and the next holds maximum-contact states only;
against the host instantiation of the same template, and the primal against forward_zero of the handle's own step
kernel (a second statement of the step on the device)."""
import numpy as np
import pytest

import tds_amd
from tds_amd import hip_backend as hb
import diff_states as ds

pytestmark = pytest.mark.gpu

N = 4096
MODELS = ["ant", "laikago", "cube_floating"]


def rel(a, b):
    return float(np.max(np.abs(a - b)) / max(1.0, np.max(np.abs(b))))


def step_rel(y, y_ref):
    return float(np.max(np.abs(y - y_ref) / np.maximum(np.abs(y_ref), 1.0)))


def arranged_states(name, m, seed):
    """N sweep states: wavefront 0 alternates the fewest and the most penetrating contacts, wavefront 1 holds the most
    only, the rest as drawn.  Returns (x, contact counts of the first 128)."""
    x = ds.states(name, N, seed=seed, m=m)
    pool = np.arange(0, N, 4)  # (the recipes put their sunk bands first)
    c = ds.contact_counts(name, m, x[pool], reference=False)
    lo, hi = pool[c == c.min()], pool[c == c.max()]
    assert c.min() == 0 and c.max() == ds.MAX_CONTACTS[name], (c.min(), c.max())
    head = np.empty(128, dtype=np.int64)
    head[0:64:2] = lo[np.arange(32) % lo.size]
    head[1:64:2] = hi[np.arange(32) % hi.size]
    head[64:128] = hi[(32 + np.arange(64)) % hi.size]
    out = x.copy()
    out[:128] = x[head]
    return out, ds.contact_counts(name, m, out[:128], reference=False)


def sampled(n):
    """both arranged wavefronts and check_device_against_host's sample of the rest"""
    return np.unique(np.r_[np.arange(128), np.arange(n - 8, n), np.arange(128, n, 509)])


def check_model(m, name, x, seed):
    import torch

    sim = hb.HipSim(m, N, device=0, dtype="f64")
    try:
        kernel = sim.single_step_kernel()[0]
        assert kernel in ("oct8", "quad16", "general"), kernel
        rng = np.random.default_rng(seed)
        n, nin, nout = x.shape[0], m.input_dim, m.output_dim
        idx = sampled(n)
        xd = torch.from_numpy(x).cuda()
        y_fz = sim.forward_zero(xd).cpu().numpy()
        jac_h, y_h = hb.jacobian_host(m, x[idx], want_y=True)
        # forward mode, K = 2
        v = rng.normal(size=(n, 2, nin))
        y, jv = sim.jvp(xd, torch.from_numpy(v).cuda())
        y, jv = y.cpu().numpy(), jv.cpu().numpy()
        assert np.all(np.isfinite(jv)) and np.all(np.isfinite(y))
        assert rel(jv[idx], np.einsum("noi,nki->nko", jac_h, v[idx])) <= 1e-12
        assert step_rel(y[idx], y_h) <= 1e-12
        e_fz = step_rel(y, y_fz)
        print(f"{name} (pgs_iterations {m.pgs_iterations}): jvp primal vs {kernel} forward_zero {e_fz:.2e}")
        assert e_fz <= 1e-10
        # reverse mode, k = 1 and 3
        for k in (1, 3):
            w = rng.normal(size=(n, k, nout))
            y, wj = sim.vjp(xd, torch.from_numpy(w).cuda())
            y, wj = y.cpu().numpy(), wj.cpu().numpy()
            assert np.all(np.isfinite(wj)) and np.all(np.isfinite(y))
            assert rel(wj[idx], hb.vjp_host(m, x[idx], w[idx])) <= 1e-12
            assert step_rel(y[idx], y_h) <= 1e-12
        # [x | theta], every selectable parameter
        sel = hb.all_params(m)
        p = len(sel)
        theta = hb.params_get(m, sel)
        thd = torch.from_numpy(theta).cuda()
        v = rng.normal(size=(n, nin + p))
        y, jv = sim.jvp_params(xd, thd, sel, torch.from_numpy(v).cuda())
        jv = jv.cpu().numpy()
        assert np.all(np.isfinite(jv))
        assert rel(jv[idx], hb.jvp_params_host(m, x[idx], theta, sel, v[idx])) <= 1e-12
        w = rng.normal(size=(n, 2, nout))
        y, wj_x, wj_t = sim.vjp_params(xd, thd, sel, torch.from_numpy(w).cuda())
        wj = np.concatenate([wj_x.cpu().numpy(), wj_t.cpu().numpy()], axis=-1)
        assert np.all(np.isfinite(wj))
        assert rel(wj[idx], hb.vjp_params_host(m, x[idx], theta, sel, w[idx])) <= 1e-12
        assert step_rel(y.cpu().numpy()[idx], y_h) <= 1e-12
    finally:
        sim.close()


@pytest.mark.parametrize("name", MODELS)
def test_device_derivatives_over_a_contact_sweep(name, built):
    m = tds_amd.load_model(name)
    x, c = arranged_states(name, m, seed=21)
    print(f"{name}: wavefront 0 contacts {sorted(set(c[:64].tolist()))}, wavefront 1 {sorted(set(c[64:].tolist()))}")
    check_model(m, name, x, seed=22)


def test_device_derivatives_of_the_ant_at_three_pgs_iterations(built):
    m = tds_amd.load_model("ant").copy()
    m.pgs_iterations = 3
    x, _ = arranged_states("ant", m, seed=23)
    check_model(m, "ant", x, seed=24)
