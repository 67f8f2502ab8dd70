"""CPU: forward-mode derivatives of the contact query (tds_contact.h over TdsDual and an overlay of parameters, the
host instantiation tds_hip_contacts_jvp_host) over the seeded sweeps of tests/diff_states.py, which span every contact
count each model can reach: the primal against contacts_host, the tangents in x and in theta against central
differences of contacts_host, d qd_post against the step derivatives (another statement: tds_diff_step.h), and the
structure of the call."""
import functools
import os

import numpy as np
import pytest

import tds_amd
from tds_amd import hip_backend as hb
import diff_states as ds
import reflib  # checker only

SWEEP = {"ant": 400}  # states per model; others: 300 (tests/test_diff_sweep_cpu.py)
GROUP_A = ("contacts", "rhs", "impulse", "force", "qd_pre", "qd_post")
GROUP_B = ("jac", "rows", "delassus")
# Worst error of a kink-free state against the central differences, measured on the sweeps per model (tangents in x:
# the larger of the two output groups and of every output on its own; in theta: over the selection); the tests assert
# 10 x these.  Central differences of h = 1e-6 max(1, |x|) carry the query's round-off over 2h and h^2 f''' / 6.
MEASURED_X = {"ant": 9.11e-09, "ant_floating": 4.52e-09, "laikago": 5.07e-09, "laikago_soft": 5.07e-09,
              "laikago_floating": 2.12e-09, "laikago_floating_env": 2.71e-09, "cube_floating": 3.08e-10,
              "pendulum5_plane": 5.14e-08, "cartpole_plane": 9.00e-09}
# In theta (h = 1e-4 |theta|, 1e-4 where theta = 0) the maxima above 1e-7 are the differences' own error, not the
# tangents': every other parameter of every model is below 2e-7.
#   geom_trans z (theta = 0, so h = 1e-4 m of penetration depth into a stiff contact): truncation.  On laikago_floating
#     the error falls with h^2: 1.2e-5 at h = 1e-4, 1.2e-7 at 1e-5, 1.2e-9 at 1e-6.
#   cfm (theta = 1e-5, so h = 1e-9): round-off of the query over 2h.  On ant_floating the error GROWS as h shrinks:
#     4.2e-8 at h_rel = 1e-2, 6.0e-7 at 1e-3, 5.1e-6 at 1e-4.
MEASURED_THETA = {"ant": 2.55e-06, "ant_floating": 5.05e-06, "laikago": 1.10e-06, "laikago_soft": 1.03e-06,
                  "laikago_floating": 1.17e-05, "laikago_floating_env": 7.56e-07, "cube_floating": 5.49e-08,
                  "pendulum5_plane": 3.60e-07, "cartpole_plane": 4.41e-08}
# d qd_post against the step derivatives, every state, kinks included (round-off of two statements of the same
# arithmetic): the largest over the models, in x and in theta
MEASURED_STEP = 9.12e-13  # pendulum5_plane, theta; the Ant: 6.4e-14


def model(name, **settings):
    m = tds_amd.load_model(name).copy()
    for k, v in settings.items():
        setattr(m, k, v)
    return m


@functools.lru_cache(maxsize=None)
def sweep(name):
    m = tds_amd.load_model(name)
    x = ds.states(name, SWEEP.get(name, 300), seed=1, m=m)
    x.setflags(write=False)
    return x, ds.contact_counts(name, m, x, reference=False)


def state_rel(a, b):
    """per state: max |a - b| / max(1, max |b|)  (tests/test_diff_sweep_cpu.py)"""
    ax = tuple(range(1, a.ndim))
    return np.abs(a - b).max(axis=ax) / np.maximum(1.0, np.abs(b).max(axis=ax))


def rel(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1.0))) if a.size else 0.0


def flat(d, want, n):
    return np.concatenate([d[k].reshape(n, -1) for k in want], axis=1)


def widths(m, want):
    return [int(np.prod(hb.contact_shapes(m, 1)[k])) for k in want]


def query_of(want):
    return lambda mm, z: flat(hb.contacts_host(mm, z, want=want), want, z.shape[0])


def identity(n, k, off, width):
    v = np.zeros((n, k, width))
    v[:, np.arange(k), off + np.arange(k)] = 1.0
    return v


def jac_x(m, x, want):
    """[n, features, input_dim] from identity directions"""
    n, nin = x.shape[0], m.input_dim
    t = hb.contacts_jvp_host(m, x, identity(n, nin, 0, nin), want=want)
    return np.concatenate([t[k].reshape(n, nin, -1) for k in want], axis=2).transpose(0, 2, 1)


def theta_sel(m, friction=True):
    """friction, restitution, gravity z, the heaviest link's mass, cfm, erp, the first contact shape's radius and the z
    of its frame"""
    heavy = max(range(m.num_links), key=lambda i: m.links[i].mass) if m.num_links else None
    g = int(hb.contact_layout(m)["geom"][0])
    sel = [("restitution",), ("gravity", 2), ("mass", heavy) if m.num_links else ("base_mass",), ("cfm",), ("erp",),
           ("geom_radius", g), ("geom_trans", g, 2)]
    return ([("friction",)] if friction else []) + sel


def apply_param(m, q, value):
    return hb.params_apply(m, [q], [value])


# ---------------------------------------------------------------- 1. primal
@pytest.mark.parametrize("name", ds.MODELS)
def test_primal_is_the_query(name, built):
    """The value part of the dual instantiation, and the double instantiation over an overlay (k = 0), against
    contacts_host.  Bitwise in fact: the overlay holds the blob's doubles and the expressions are the same, which the
    second assertion states; the issue's bound is 1e-12."""
    m = model(name)
    x = sweep(name)[0][:96]
    n = x.shape[0]
    ref = hb.contacts_host(m, x)
    sel = theta_sel(m)
    v = np.zeros((n, 1, m.input_dim))
    cases = [hb.contacts_jvp_host(m, x, None),
             hb.contacts_jvp_host(m, x, None, params=sel, theta=hb.params_get(m, sel)),
             hb.contacts_jvp_host(m, x, v, want_primal=True)[1]]
    for d in cases:
        for k in hb.CONTACT_OUTPUTS:
            assert rel(d[k], ref[k]) <= 1e-12, k
            np.testing.assert_array_equal(d[k], ref[k])


# ---------------------------------------------------------------- 2. tangents in x
def central(m, x, want):
    """central differences of contacts_host over every input column, one call on [x | x +- h e_j | x +- 2h e_j]
    (diff_states.central_jacobian), judged for the concatenation `want` and for every output on its own: a dict name
    (or "all") -> (J [n, features, input_dim], kink [n])"""
    out, o = {}, 0
    n, nin = x.shape
    h = 1e-6 * np.maximum(1.0, np.abs(x))
    batch = np.repeat(x[:, None, :], 1 + 4 * nin, axis=1)
    idx = np.arange(nin)
    for s, mult in enumerate((1.0, -1.0, 2.0, -2.0)):
        batch[:, 1 + s * nin + idx, idx] += mult * h
    y = query_of(want)(m, batch.reshape(-1, nin)).reshape(n, 1 + 4 * nin, -1)
    for k, wd in [("all", y.shape[2])] + list(zip(want, widths(m, want))):
        ys = y if k == "all" else y[:, :, o:o + wd]
        o += 0 if k == "all" else wd
        if not wd:
            continue
        out[k] = ds._central_and_kink(ys[:, :1], ys[:, 1:1 + nin], ys[:, 1 + nin:1 + 2 * nin],
                                      ys[:, 1 + 2 * nin:1 + 3 * nin], ys[:, 1 + 3 * nin:], h[:, :, None], 1e-5)
    return out


@pytest.mark.parametrize("group", ["a", "b"])
@pytest.mark.parametrize("name", ds.MODELS)
def test_tangents_in_x_match_central_differences(name, group, built):
    m = model(name)
    x, counts = sweep(name)
    want = GROUP_A if group == "a" else GROUP_B
    if group == "b" and name == "ant":  # (for time: the Delassus matrix of 17 points over 37 columns)
        x, counts = x[::4], counts[::4]
    J = jac_x(m, x, want)
    fd = central(m, x, want)
    present = np.bincount(counts, minlength=counts.max() + 1) > 0
    worst, o = 0.0, 0
    for k, wd in [("all", J.shape[1])] + list(zip(want, widths(m, want))):
        Jk = J if k == "all" else J[:, o:o + wd]
        o += 0 if k == "all" else wd
        J_fd, kink = fd[k]
        ok = ~kink
        err = state_rel(Jk[ok], J_fd[ok]) if wd else np.zeros(1)
        checked = np.bincount(counts[ok], minlength=counts.max() + 1)
        print(f"{name} {k}: kink-free {ok.mean():.3f}, worst tangent error {err.max():.2e}")
        assert ok.mean() >= 0.9, k
        assert np.all(checked[present] >= 1), k
        worst = max(worst, float(err.max()))
    print(f"{name} group {group}: MEASURED_X {worst:.2e}")
    assert worst <= 10 * MEASURED_X[name]


# ---------------------------------------------------------------- 3. tangents in theta
@pytest.mark.parametrize("name", ds.MODELS)
def test_tangents_in_theta_match_central_differences(name, built):
    m = model(name)
    x = sweep(name)[0][::3]
    n, nin = x.shape[0], m.input_dim
    want = GROUP_A + GROUP_B
    sel = theta_sel(m)
    p = len(sel)
    t = hb.contacts_jvp_host(m, x, identity(n, p, nin, nin + p), want=want, params=sel)
    Jt = np.concatenate([t[k].reshape(n, p, -1) for k in want], axis=2).transpose(0, 2, 1)
    Jt_fd, kink = ds.central_theta(m, x, sel, query_of(want), apply_param, h_rel=1e-4)
    worst = 0.0
    for j, q in enumerate(sel):
        ok = ~kink[:, j]
        e = state_rel(Jt[ok][:, :, j], Jt_fd[ok][:, :, j])
        print(f"{name} {q}: kink-free {ok.mean():.3f}, worst error {e.max():.2e}")
        assert ok.mean() >= 0.9, q
        worst = max(worst, float(e.max()))
    assert np.count_nonzero(Jt) > 0
    print(f"{name}: MEASURED_THETA {worst:.2e}")
    assert worst <= 10 * MEASURED_THETA[name]


# ---------------------------------------------------------------- 4. against the step derivatives
@pytest.mark.parametrize("name", ds.MODELS)
def test_qd_post_tangents_are_the_step_derivatives(name, built):
    """every state, kinks included: both follow the primal's branch"""
    m = model(name)
    x = sweep(name)[0][::2]
    n, nin, nq, nd = x.shape[0], m.input_dim, m.dof_q, m.dof_qd
    Jx = jac_x(m, x, ("qd_post",))
    J = hb.jacobian_host(m, x)[:, nq:nq + nd]
    ex = rel(Jx, J)
    sel = theta_sel(m)
    p = len(sel)
    v = identity(n, p, nin, nin + p)
    th = hb.params_get(m, sel)
    Jt = hb.contacts_jvp_host(m, x, v, want=("qd_post",), params=sel, theta=th)["qd_post"]
    Js = hb.jvp_params_host(m, x, th, sel, v)[:, :, nq:nq + nd]
    et = rel(Jt, Js)
    print(f"{name}: d qd_post against the step derivatives: x {ex:.2e}, theta {et:.2e}")
    assert max(ex, et) <= 10 * MEASURED_STEP


# ---------------------------------------------------------------- 6. structure
def test_linearity_zero_directions_and_k0(built):
    m = model("ant")
    x = sweep("ant")[0][:40]
    n, nin = x.shape[0], m.input_dim
    sel = [("friction",), ("geom_radius", int(hb.contact_layout(m)["geom"][0]))]
    rng = np.random.default_rng(3)
    v = rng.normal(size=(n, 3, nin + 2))
    v[:, 2] = 2.0 * v[:, 0] - 0.5 * v[:, 1]
    t = hb.contacts_jvp_host(m, x, v, params=sel)
    for k in hb.CONTACT_OUTPUTS:
        lin = 2.0 * t[k][:, 0] - 0.5 * t[k][:, 1]
        assert np.max(np.abs(t[k][:, 2] - lin)) <= 1e-9 * max(1.0, np.max(np.abs(lin))), k
    z = hb.contacts_jvp_host(m, x, np.zeros((n, 2, nin + 2)), params=sel)
    for k in hb.CONTACT_OUTPUTS:
        assert not np.any(z[k]), k
    prim = hb.contacts_jvp_host(m, x, None, params=sel)
    assert set(prim) == set(hb.CONTACT_OUTPUTS) and prim["force"].shape == (n, 17, 3)


def test_separated_points_have_zero_tangents_and_forces_follow_impulses(built):
    m = model("ant")
    x = sweep("ant")[0][:120]
    n, nin = x.shape[0], m.input_dim
    lay = hb.contact_layout(m)
    nc = lay["n_c"]
    sel = [("friction",), ("erp",)]
    t, prim = hb.contacts_jvp_host(m, x, identity(n, nin + 2, 0, nin + 2), params=sel, want_primal=True)
    sep = prim["contacts"][:, :, 9] >= 0.0                     # [n, nc]
    assert sep.any() and (~sep).any()
    sep3 = np.tile(sep, (1, 3))                                 # rows: normal | t1 | t2
    for k in ("rows", "rhs", "impulse"):
        a = np.moveaxis(t[k], 1, -1)                            # [n, 3 nc, ..., k]
        assert not np.any(a[sep3]), k
    assert not np.any(np.moveaxis(t["force"], 1, -1)[sep])
    assert np.any(t["contacts"][:, :, :, 9][np.broadcast_to(sep[:, None], t["contacts"].shape[:3])])  # the distance moves
    dp = t["impulse"]                                            # [n, k, 3 nc]
    f = -(dp[..., :nc, None] * lay["normal"] + dp[..., nc:2 * nc, None] * lay["t1"]
          + dp[..., 2 * nc:, None] * lay["t2"]) / m.dt
    assert np.max(np.abs(f - t["force"])) <= 1e-12 * max(1.0, np.max(np.abs(f)))


def test_want_subsets_jacobian_columns_and_per_environment_theta(built):
    m = model("laikago")
    x = sweep("laikago")[0][:12]
    n, nin = x.shape[0], m.input_dim
    sel = [("friction",), ("cfm",)]
    rng = np.random.default_rng(4)
    v = rng.normal(size=(n, 5, nin + 2))
    th = hb.params_get(m, sel) * (1.0 + 0.2 * rng.uniform(size=(n, 2)))
    full, fullp = hb.contacts_jvp_host(m, x, v, params=sel, theta=th, want_primal=True)
    for want in [("force",), ("contacts", "jac"), ("rows", "rhs"), ("delassus",), ("impulse", "qd_post"), ("qd_pre",)]:
        sub, subp = hb.contacts_jvp_host(m, x, v, want=want, params=sel, theta=th, want_primal=True)
        assert list(sub) == list(want)
        for k in want:
            np.testing.assert_array_equal(sub[k], full[k])
            np.testing.assert_array_equal(subp[k], fullp[k])
    for e in range(n):  # per-environment theta: the model copy with that theta
        me = hb.params_apply(m, sel, th[e])
        one, onep = hb.contacts_jvp_host(me, x[e:e + 1], v[e:e + 1], params=sel, want_primal=True)
        ref = hb.contacts_host(me, x[e:e + 1])
        for k in hb.CONTACT_OUTPUTS:
            assert rel(one[k], full[k][e:e + 1]) <= 1e-12, k
            assert rel(fullp[k][e:e + 1], ref[k]) <= 1e-12, k
    with pytest.raises(ValueError):
        hb.contacts_jvp_host(m, x, v, want=("forces",), params=sel)


@pytest.mark.parametrize("settings", [{"pgs_iterations": 3}, {"friction": 0.5, "restitution": 0.3}])
def test_settings_copies(settings, built):
    m = model("ant", **settings)
    x = sweep("ant")[0][::8]
    want = ("impulse", "force", "qd_post")
    J = jac_x(m, x, want)
    J_fd, kink = ds.central_jacobian(m, x, step=lambda z: query_of(want)(m, z))
    ok = ~kink
    err = state_rel(J[ok], J_fd[ok])
    print(f"ant {settings}: kink-free {ok.mean():.3f}, worst {err.max():.2e}")
    assert ok.mean() >= 0.9 and err.max() <= 10 * MEASURED_X["ant"]


@pytest.mark.parametrize("name", ["cartpole", "pendulum5"])
def test_models_without_a_plane(name, built):
    m = model(name)
    rng = np.random.default_rng(2)
    x = rng.uniform(-0.5, 0.5, size=(8, m.input_dim))
    nin, nq, nd = m.input_dim, m.dof_q, m.dof_qd
    t = hb.contacts_jvp_host(m, x, identity(8, nin, 0, nin))
    for k in ("contacts", "jac", "rows", "rhs", "delassus", "impulse", "force"):
        assert t[k].size == 0
    np.testing.assert_array_equal(t["qd_pre"], t["qd_post"])
    J = hb.jacobian_host(m, x)[:, nq:nq + nd]
    assert rel(t["qd_post"].transpose(0, 2, 1), J) <= 1e-10


def test_singular_mass_matrix_gives_nan_and_an_error(built):
    m = model("pendulum5_plane")
    x = sweep("pendulum5_plane")[0][:6]
    n, nin = x.shape[0], m.input_dim
    v = identity(n, 3, 0, nin)
    good, goodp = hb.contacts_jvp_host(m, x, v, want_primal=True)
    for i in range(m.num_links):
        m.links[i].mass = 0.0
        for k in range(9):
            m.links[i].inertia[k] = 0.0
    out = {k: np.zeros(s) for k, s in hb.contact_tangent_shapes(m, n, 3).items()}
    outp = {k: np.zeros(s) for k, s in hb.contact_shapes(m, n).items()}
    with pytest.raises(hb.TdsHipError, match="error 1: contact query: joint-space inertia not positive definite"):
        hb.contacts_jvp_host(m, x, v, want_primal=True, out=out, out_primal=outp)
    for k in ("contacts", "jac"):
        np.testing.assert_array_equal(out[k], good[k])
        np.testing.assert_array_equal(outp[k], goodp[k])
    for k in ("rows", "rhs", "delassus", "impulse", "force", "qd_pre", "qd_post"):
        assert np.all(np.isnan(out[k])) and np.all(np.isnan(outp[k])), k


def test_refusals_and_selection_errors_keep_their_messages(built):
    for name in ("pendulum5_spherical", "two_pendulums_plane"):
        m = tds_amd.load_model(name)
        x = np.zeros((1, m.input_dim))
        with pytest.raises(hb.TdsHipError, match="error 2: step Jacobians: .* not supported"):
            hb.contacts_jvp_host(m, x, np.zeros((1, 1, m.input_dim)))
        with pytest.raises(hb.TdsHipError, match="error 2: step Jacobians: .* not supported"):
            hb.contacts_jvp_tangents(m)
    m = model("ant")
    x = sweep("ant")[0][:2]
    for bad in ([("mass", 99)], [("friction",), ("friction",)], [("geom_radius", 99)]):
        with pytest.raises(hb.TdsHipError) as e1:
            hb.params_get(m, bad)
        with pytest.raises(hb.TdsHipError) as e2:
            hb.contacts_jvp_host(m, x, np.zeros((2, 1, m.input_dim + len(bad))), params=bad)
        assert str(e1.value) == str(e2.value)
    assert hb.contacts_jvp_tangents(m) >= 1
    assert hb.lib().tds_hip_contacts_jvp_host(m, 2, x.ctypes.data, 0, None, None, 0, None, hb.ContactOut(), None) == 1


# ---------------------------------------------------------------- 5. against the reference
# worst error over the six golden records (all six pass the two filters) against central differences of the reference,
# relative to max(1, max |J|) of a record; asserted x 10
REF_MEASURED = {"ant": 6.18e-10, "laikago": 1.66e-10}


def active_set_constant(r, x, h_rel=1e-6):
    """the reference's penetrating-contact set is the same at x and at every x +- h e_j (tests/test_jacobian_cpu.py)"""
    r.step(x[None])
    base = r.last_penetrating_contacts()
    for j in range(x.shape[0]):
        h = h_rel * max(1.0, abs(x[j]))
        for s in (h, -h):
            z = x.copy()
            z[j] += s
            r.step(z[None])
            if r.last_penetrating_contacts() != base:
                return False
    return True


def clamps_inactive(m, x, margin=1e-4):
    """no PD clamp sits within `margin` of its switch (tests/test_jacobian_cpu.py)"""
    if m.step_mode != tds_amd.TDS_STEP_LOCOMOTION:
        return True
    nq, nd, na = m.dof_q, m.dof_qd, m.action_dim
    a = x[nq + nd:nq + nd + na]
    return bool(np.all(np.abs(np.abs(a) - m.action_limit) > margin))


@pytest.mark.skipif(not reflib.available(), reason="the reference library is not built here")
@pytest.mark.parametrize("name", ["ant", "laikago"])
def test_tangents_match_central_differences_of_the_reference(name, built):
    """d contacts (points, distance) against RefSim.debug and d qd_post against RefSim.step, at golden records whose
    active set is constant over +- h"""
    import gen_golden  # checker only: the table of reference constructors

    m = model(name)
    x = np.load(os.path.join(os.path.dirname(__file__), "golden", f"{name}.npz"))["x"][:6]
    nin, nq, nd = m.input_dim, m.dof_q, m.dof_qd
    r, _ = gen_golden.make_ref(name)
    try:
        checked, worst = 0, 0.0
        for e in range(x.shape[0]):
            if not active_set_constant(r, x[e]) or not clamps_inactive(m, x[e]):
                continue
            t = hb.contacts_jvp_host(m, x[e:e + 1], identity(1, nin, 0, nin), want=("contacts", "qd_post"))
            J = np.concatenate([t["contacts"].reshape(nin, -1), t["qd_post"].reshape(nin, -1)], axis=1).T
            f = lambda z: np.concatenate([r.debug(z, m)["contacts"].ravel(), r.step(z[None])[0, nq:nq + nd]])  # noqa: E731
            J_fd = np.zeros_like(J)
            for j in range(nin):
                h = 1e-6 * max(1.0, abs(x[e, j]))
                zp, zm = x[e].copy(), x[e].copy()
                zp[j] += h
                zm[j] -= h
                J_fd[:, j] = (f(zp) - f(zm)) / (2 * h)
            worst = max(worst, float(np.max(np.abs(J - J_fd)) / max(1.0, np.max(np.abs(J_fd)))))
            checked += 1
        print(f"{name}: {checked} records against the reference, REF_MEASURED {worst:.2e}")
        assert checked >= 1
        assert worst <= 10 * REF_MEASURED[name]
    finally:
        r.close()
