"""Forward-mode derivatives of rigid-body rollouts on the CPU (tds_rb_jvp_host, the checker of the device path):
primal against the C oracle, tangents against central differences of the reference, chain rule, linearity, refusals."""
import ctypes as C

import numpy as np
import pytest

import oraclelib
import reflib
from conftest import rel_err
from rb_scenes import MIXED_ORDER, billiard_model, billiard_state, make_mixed_worlds, make_worlds, shot_velocity

from tds_amd import hip_backend as hb

PARAMS = [("mass", 2), ("gravity", 2), ("friction",), ("restitution",)]


def scenes():
    """(name, model, s0, steps, params); masses index a dynamic body of the scene"""
    ma, sa = make_worlds(3, 7)
    mb, sb = make_worlds(3, 7, plane_last=True)
    mc, sc = make_mixed_worlds(3, 21, MIXED_ORDER)
    md = billiard_model()
    sd = billiard_state(2)
    sd[:, 6, 7:9] = shot_velocity([[10.0, 600.0], [-40.0, 550.0]])
    return [("plane_first", ma, sa, 40, [("mass", 2), ("gravity", 2), ("friction",), ("restitution",)]),
            ("plane_last", mb, sb, 40, [("mass", 1), ("gravity", 0), ("friction",), ("restitution",)]),
            ("mixed", mc, sc, 30, [("mass", 3), ("gravity", 2), ("friction",), ("restitution",)]),
            ("billiard", md, sd, 120, [("mass", 6), ("mass", 5), ("friction",)])]


def perturbed(m, q, d):
    m2 = type(m).from_buffer_copy(m)
    if q[0] == "mass":
        m2.bodies[q[1]].mass += d
    elif q[0] == "gravity":
        m2.gravity[q[1]] += d
    elif q[0] == "friction":
        m2.friction += d
    else:
        m2.restitution += d
    return m2


@pytest.mark.parametrize("idx", range(4))
def test_rb_primal_matches_oracle(idx, built):
    name, m, s0, steps, params = scenes()[idx]
    sT = hb.rb_jvp_host(m, s0, steps)
    assert rel_err(sT, oraclelib.rb_step(m, s0, steps), 1e-2) < 1e-9, name
    ns = m.num_bodies * 13 + len(params)
    v = np.random.default_rng(3).normal(size=(s0.shape[0], 3, ns))
    sT2, _ = hb.rb_jvp_host(m, s0, steps, v, params)
    assert np.array_equal(sT, sT2)                       # the value part of the dual run is the double run
    th = hb.rb_params_get(m, params)
    sT3, _ = hb.rb_jvp_host(m, s0, steps, v, params, th)
    assert np.array_equal(sT, sT3)


@pytest.mark.skipif(not reflib.available(), reason="reference library not built (oracle/_ref)")
@pytest.mark.parametrize("idx", range(4))
def test_rb_tangents_match_reference_differences(idx, built):
    name, m, s0, steps, params = scenes()[idx]
    s0 = s0[:1]
    nb = m.num_bodies
    ns = nb * 13
    rng = np.random.default_rng(11)
    dyn = [b for b in range(nb) if m.bodies[b].mass > 0]
    cols = [b * 13 + c for b in dyn for c in (0, 1, 2, 7, 8, 10)]
    cols = list(rng.choice(cols, size=min(8, len(cols)), replace=False)) + [ns + j for j in range(len(params))]
    v = np.zeros((1, len(cols), ns + len(params)))
    v[0, np.arange(len(cols)), cols] = 1.0
    _, jv = hb.rb_jvp_host(m, s0, steps, v, params)
    h = 1e-6
    checked = 0
    for j, col in enumerate(cols):
        def run(d):
            if col < ns:
                s = s0.copy().reshape(1, -1)
                s[0, col] += d
                return reflib.rb_step(m, s.reshape(s0.shape), steps)[0]
            return reflib.rb_step(perturbed(m, params[col - ns], d), s0, steps)[0]
        y0, yp, ym = run(0.0), run(h), run(-h)
        fwd, bwd, cd = (yp - y0) / h, (y0 - ym) / h, (yp - ym) / (2 * h)
        ok = np.abs(fwd - bwd) <= 1e-4 * np.maximum(np.abs(cd), 1.0)   # no branch switch within +-h
        err = np.abs(jv[0, j] - cd) / np.maximum(np.abs(cd), 1.0)
        assert err[ok].max(initial=0.0) < 1e-6, (name, col, err[ok].max())
        checked += int(ok.sum())
    assert checked >= 13 * nb * len(cols) // 2, (name, checked)


def test_rb_chain_rule_and_linearity(built):
    _, m, s0, _, params = scenes()[0]
    ns = m.num_bodies * 13 + len(params)
    rng = np.random.default_rng(5)
    v = rng.normal(size=(s0.shape[0], 2, ns))
    th = hb.rb_params_get(m, params)
    sT, jv = hb.rb_jvp_host(m, s0, 30, v, params, th)
    s1, j1 = hb.rb_jvp_host(m, s0, 18, v, params, th)
    v2 = np.concatenate([j1.reshape(s0.shape[0], 2, -1), v[:, :, -len(params):]], axis=2)
    s2, j2 = hb.rb_jvp_host(m, s1, 12, v2, params, th)
    assert rel_err(s2, sT, 1.0) <= 1e-12
    assert rel_err(j2, jv, 1.0) <= 1e-12
    a, b = 0.7, -1.3
    _, jab = hb.rb_jvp_host(m, s0, 30, a * v[:, :1] + b * v[:, 1:], params, th)
    assert rel_err(jab[:, 0], a * jv[:, 0] + b * jv[:, 1], 1.0) <= 1e-12


def test_rb_refusals(built):
    m, s0 = make_worlds(2, 7)              # body 0 is the plane (static)
    ns = m.num_bodies * 13
    for bad in ([("mass", 0)], [("mass", 6)], [("mass", 1), ("mass", 1)], [("gravity", 3)], [("com", 1, 0)],
                [("friction",), ("friction",)], [("inertia", 1, 0)]):
        with pytest.raises(hb.TdsHipError):
            hb.rb_params_get(m, bad)
        with pytest.raises(hb.TdsHipError):
            hb.rb_jvp_host(m, s0, 1, np.zeros((2, 1, ns + len(bad))), bad)
    with pytest.raises(hb.TdsHipError, match="steps"):
        hb.rb_jvp_host(m, s0, 0)
    L = hb.lib()
    st = np.ascontiguousarray(s0)
    out = np.zeros_like(st)
    v = np.zeros((2, 1, ns))
    jv = np.zeros((2, 1, ns))
    nul = (hb.Param * 1)()
    assert L.tds_rb_jvp_host(C.byref(m), 2, 1, st.ctypes.data, 0, nul, None, -1, None, out.ctypes.data, None) != 0
    assert L.tds_rb_jvp_host(None, 2, 1, st.ctypes.data, 0, nul, None, 0, None, out.ctypes.data, None) != 0
    assert L.tds_rb_jvp_host(C.byref(m), 2, 1, None, 0, nul, None, 0, None, out.ctypes.data, None) != 0
    assert L.tds_rb_jvp_host(C.byref(m), 2, 1, st.ctypes.data, 0, nul, None, 0, None, None, None) != 0
    assert L.tds_rb_jvp_host(C.byref(m), 2, 1, st.ctypes.data, 0, nul, None, 1, None, out.ctypes.data,
                             jv.ctypes.data) != 0
    assert L.tds_rb_jvp_host(C.byref(m), 2, 1, st.ctypes.data, 0, nul, None, 1, v.ctypes.data, out.ctypes.data,
                             None) != 0
    assert L.tds_rb_jvp_host(C.byref(m), 0, 1, st.ctypes.data, 0, nul, None, 0, None, out.ctypes.data, None) != 0
    assert L.tds_rb_jvp_host(C.byref(m), 2, 1, st.ctypes.data, 1, None, None, 0, None, out.ctypes.data, None) != 0
    assert L.tds_rb_params_get(C.byref(m), 1, None, out.ctypes.data) != 0
