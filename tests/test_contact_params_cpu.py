"""CPU: the contact model's parameters in the parameter vocabulary — cfm, erp, and per collision shape its radius, a
capsule's length, a box's extents and the translation of its frame (kinds 16..21, hip_backend.CONTACT_PARAM_KINDS).
Spec and round trip, selection errors, the blob-value identity against the plain derivatives, per-environment theta,
J_theta against central differences of the double step, of the C oracle (shapes) and of the reference (cfm, erp), the
tape lengths with every old and every new parameter selected, and a short trajectory."""
import functools
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

import tds_amd
from tds_amd import hip_backend as hb

sys.path.insert(0, os.path.join(ROOT, "oracle"))
import oraclelib  # noqa: E402  (checker only)
import reflib  # noqa: E402  (checker only)

import diff_states  # noqa: E402

MODELS = ["ant", "laikago_soft", "cartpole_plane", "pendulum5_plane", "cube_floating", "ant_floating"]
# parameter-mode tape capacity per class and the models of each
CAPACITY = {"S": 18432, "A": 86016, "L": 81920}
CLASS_OF = {"pendulum5_plane": "S", "cube_floating": "S", "pendulum5": "S", "cartpole": "S",
            "ant": "A", "ant_floating": "A", "cartpole_plane": "A",
            "laikago": "L", "laikago_soft": "L", "laikago_floating": "L", "laikago_floating_env": "L"}
# the longest golden-record tapes of the old selection as DESIGN 7a has recorded them since the parameter derivatives
OLD_GOLDEN = {"pendulum5_plane": 14248, "cube_floating": 5499, "pendulum5": 6099, "cartpole": 1760, "ant": 72101,
              "ant_floating": 39201, "cartpole_plane": 6406, "laikago_soft": 70347, "laikago": 70345}
N_SWEEP = 16
BOX = 4  # TDS_GEOM_BOX


def rel(a, b):
    return float(np.max(np.abs(a - b)) / max(1.0, np.max(np.abs(b)))) if np.size(a) else 0.0


def set_param(m, q, value):
    """a copy of model m with the contact parameter q (a param_spec tuple) set by plain field assignment"""
    m = m.copy()
    name = q[0]
    if name in ("cfm", "erp"):
        setattr(m, name, value)
    elif name == "geom_radius":
        m.geoms[q[1]].radius = value
    elif name == "geom_length":
        m.geoms[q[1]].length = value
    elif name == "geom_extent":
        m.geoms[q[1]].extents[q[2]] = value
    else:
        assert name == "geom_trans", q
        m.geoms[q[1]].X_trans[q[2]] = value
    return m


@functools.lru_cache(maxsize=None)
def sweep(name, n=N_SWEEP):
    """(model, n states of the contact sweep: penetrating contacts on most of them); read only"""
    m = tds_amd.load_model(name)
    x = np.ascontiguousarray(diff_states.states(name, n, 5, m))
    x.setflags(write=False)
    return m, x


def j_theta(m, x, sel, theta=None):
    """J_theta [N, output_dim, p] by forward mode over unit theta directions"""
    n, nin, p = x.shape[0], m.input_dim, len(sel)
    v = np.zeros((n, p, nin + p))
    v[:, np.arange(p), nin + np.arange(p)] = 1.0
    return hb.jvp_params_host(m, x, hb.params_get(m, sel) if theta is None else theta, sel, v).transpose(0, 2, 1)


def raised_box(m):
    """cartpole_plane with the radius of the pole's box raised above the 1e-2 of the clamp"""
    g = next(g for g in range(m.num_geoms - 1, -1, -1) if m.geoms[g].type == BOX)
    return set_param(m, ("geom_radius", g), 0.03), g


def inert(name, m, q):
    """entries the step cannot feel, by the mechanism's symmetry — their derivative is exactly zero:
    pendulum5_plane: the chain swings in the y-z plane about x axes, nothing depends on a sphere's x;
    cartpole_plane: the cart (geom 0) slides along x — the plane's normal impulse does no work on it and its friction
    rows stay inside their bounds, so its shape is not felt at all; the pole swings in the x-z plane: its box's y
    extent and y translation are not felt"""
    if name == "pendulum5_plane":
        return q[0] == "geom_trans" and q[2] == 0
    if name == "cartpole_plane":
        return q[0].startswith("geom_") and (q[1] == 0 or (q[0] in ("geom_extent", "geom_trans") and q[2] == 1))
    return False


# ------------------------------------------------------------------------------------------------ vocabulary
def test_param_spec_round_trip_and_all_params_unchanged(built):
    ant, cart = tds_amd.load_model("ant"), tds_amd.load_model("cartpole_plane")
    assert list(hb.CONTACT_PARAM_KINDS) == ["cfm", "erp", "geom_radius", "geom_length", "geom_extent", "geom_trans"]
    assert not set(hb.CONTACT_PARAM_KINDS) & set(hb.PARAM_KINDS)
    sel = [("cfm",), ("erp",), ("geom_radius", 0), ("geom_length", 3), ("geom_trans", 2, 1)]
    arr = hb.param_spec(sel)
    assert [(arr[j].kind, arr[j].link, arr[j].comp) for j in range(len(sel))] == [
        (16, 0, 0), (17, 0, 0), (18, 0, 0), (19, 3, 0), (21, 2, 1)]
    assert list(hb.params_get(ant, sel)) == [ant.cfm, ant.erp, ant.geoms[0].radius, ant.geoms[3].length,
                                             ant.geoms[2].X_trans[1]]
    gb = next(g for g in range(cart.num_geoms) if cart.geoms[g].type == BOX)
    bsel = [("geom_extent", gb, 2), ("geom_radius", gb), ("geom_trans", gb, 0)]
    assert [(q.kind, q.link, q.comp) for q in hb.param_spec(bsel)[:3]] == [(20, gb, 2), (18, gb, 0), (21, gb, 0)]
    assert list(hb.params_get(cart, bsel)) == [cart.geoms[gb].extents[2], cart.geoms[gb].radius, cart.geoms[gb].X_trans[0]]
    # apply == plain field assignment, one entry at a time and all at once; and back
    for m, s in ((ant, sel), (cart, bsel)):
        base = hb.params_get(m, s)
        theta = base * 1.07 + 0.003
        want = m
        for j, q in enumerate(s):
            want = set_param(want, q, theta[j])
            assert bytes(hb.params_apply(m, [q], [theta[j]])) == bytes(set_param(m, q, theta[j]))
        got = hb.params_apply(m, s, theta)
        assert bytes(got) == bytes(want) and bytes(got) != bytes(m)
        np.testing.assert_array_equal(hb.params_get(got, s), theta)
        assert bytes(hb.params_apply(got, s, base)) == bytes(m)
    # the old table and all_params are what they were (p = 215, 335); the bare name stays unknown
    assert len(hb.all_params(ant)) == 215 and len(hb.all_params(tds_amd.load_model("laikago_soft"))) == 335
    assert all(q[0] in hb.PARAM_KINDS for q in hb.all_params(ant))
    for bad in ([("length", 1)], [("geom_radius",)], [("cfm", 0, 0)], [("geom_trans", 1, 0, 0)]):
        with pytest.raises(ValueError):
            hb.param_spec(bad)
    # contact_params: every new-kind entry valid for the model
    assert hb.contact_params(ant) == [("cfm",), ("erp",), ("geom_radius", 0)] + [("geom_trans", 0, c) for c in range(3)] + [
        q for g in range(1, 9) for q in [("geom_radius", g), ("geom_length", g)] + [("geom_trans", g, c) for c in range(3)]]
    assert len(hb.contact_params(cart)) == 2 + 2 * (1 + 3 + 3)
    for name in MODELS:
        m = tds_amd.load_model(name)
        hb.params_get(m, hb.all_params(m) + hb.contact_params(m))  # (valid, no duplicates)


@pytest.mark.parametrize("sel,match", [
    ([("geom_radius", 9)], "geom index out of range"),
    ([("geom_radius", -1)], "geom index out of range"),
    ([("geom_trans", 32, 0)], "geom index out of range"),
    ([("geom_trans", 1, 3)], "component index out of range"),
    ([("geom_trans", 1, -1)], "component index out of range"),
    ([("geom_radius", 1, 1)], "component index out of range"),
    ([hb.Param(16, 0, 1, 0)], "component index out of range"),
    ([hb.Param(17, 1, 0, 0)], "link index out of range"),
    ([("geom_length", 0)], "a length needs a capsule"),
    ([("geom_extent", 1, 0)], "an extent needs a box"),
    ([("cfm",), ("erp",), ("cfm",)], "duplicate parameter"),
    ([("geom_trans", 2, 1), ("mass", 2), ("geom_trans", 2, 1)], "duplicate parameter"),
    ([hb.Param(12, 0, 0, 0)], "unknown parameter kind"),
    ([hb.Param(13, 0, 0, 0)], "unknown parameter kind"),
    ([hb.Param(14, 0, 0, 0)], "unknown parameter kind"),
    ([hb.Param(15, 0, 0, 0)], "unknown parameter kind"),
    ([hb.Param(22, 0, 0, 0)], "unknown parameter kind"),
])
def test_bad_selections_are_invalid_arguments(sel, match, built):
    m = tds_amd.load_model("ant")  # geom 0: the torso's sphere, 1..8: the legs' capsules
    x = sweep("ant")[1][:1]
    th = np.zeros(len(sel))
    for call in (lambda: hb.params_get(m, sel),
                 lambda: hb.jvp_params_host(m, x, th, sel),
                 lambda: hb.vjp_params_host(m, x, th, sel, np.zeros((1, m.output_dim)))):
        with pytest.raises(hb.TdsHipError, match=match) as e:
            call()
        assert "tds_hip error 1:" in str(e.value)  # TDS_ERR_INVALID_ARG


def test_a_length_on_a_box_and_an_extent_on_a_sphere_are_refused(built):
    cart, cube = tds_amd.load_model("cartpole_plane"), tds_amd.load_model("cube_floating")
    gb = next(g for g in range(cart.num_geoms) if cart.geoms[g].type == BOX)
    with pytest.raises(hb.TdsHipError, match="a length needs a capsule"):
        hb.params_get(cart, [("geom_length", gb)])
    with pytest.raises(hb.TdsHipError, match="an extent needs a box"):
        hb.params_get(cube, [("geom_extent", 0, 0)])


def test_a_geom_of_a_model_without_a_plane_has_a_zero_derivative(built):
    m = tds_amd.load_model("cartpole")
    assert not m.has_plane and m.num_geoms > 0
    sel = hb.contact_params(m)
    x = np.load(os.path.join(ROOT, "tests", "golden", "cartpole.npz"))["x"][:3]
    J = j_theta(m, x, sel)
    w = np.random.default_rng(1).normal(size=(3, m.output_dim))
    wj, y = hb.vjp_params_host(m, x, hb.params_get(m, sel), sel, w, want_y=True)
    assert np.all(J == 0.0) and np.all(wj[:, m.input_dim:] == 0.0)
    np.testing.assert_array_equal(y, hb.step_host(m, x))
    np.testing.assert_array_equal(wj[:, :m.input_dim], hb.vjp_host(m, x, w))


# ------------------------------------------------------------------------------------------------ identities
@pytest.mark.parametrize("name", MODELS)
def test_at_blob_values_equal_the_plain_derivatives(name, built):
    """theta = the blob's values of every contact parameter (and of every old one beside them): y and the x columns
    are those of vjp_host and jacobian_host, bit for bit — on golden records and on states in contact"""
    m, xs = sweep(name)
    x = np.concatenate([np.load(os.path.join(ROOT, "tests", "golden", f"{name}.npz"))["x"][:2], xs[:4]])
    n, nin = x.shape[0], m.input_dim
    w = np.random.default_rng(2).normal(size=(n, 2, m.output_dim))
    wj0, y0 = hb.vjp_host(m, x, w, want_y=True)
    jac, yj0 = hb.jacobian_host(m, x, want_y=True)
    np.testing.assert_array_equal(y0, yj0)
    for sel in (hb.contact_params(m), hb.all_params(m) + hb.contact_params(m)):
        theta, p = hb.params_get(m, sel), len(sel)
        wj, y = hb.vjp_params_host(m, x, theta, sel, w, want_y=True)
        np.testing.assert_array_equal(y, y0)
        np.testing.assert_array_equal(wj[:, :, :nin], wj0)
        v = np.zeros((n, nin, nin + p))
        v[:, :, :nin] = np.eye(nin)
        jv, yj = hb.jvp_params_host(m, x, theta, sel, v, want_y=True)
        np.testing.assert_array_equal(yj, y0)
        np.testing.assert_array_equal(jv.transpose(0, 2, 1), jac)
        np.testing.assert_array_equal(hb.jvp_params_host(m, x, theta, sel), y0)


def draw_theta(m, sel, n, seed=4):
    """+- 5 % relative and + [0, 0.004) additive (a box's zero radius stays below the clamp, cfm and radii positive)"""
    base = hb.params_get(m, sel)
    rng = np.random.default_rng(seed)
    return base * (1.0 + 0.05 * rng.uniform(-1, 1, (n, len(sel)))) + 0.004 * rng.uniform(0, 1, (n, len(sel)))


@pytest.mark.parametrize("name", MODELS)
def test_per_environment_theta_is_the_step_of_that_model(name, built):
    m, x = sweep(name)
    sel = hb.contact_params(m)
    theta = draw_theta(m, sel, x.shape[0])
    y = hb.jvp_params_host(m, x, theta, sel)
    _, y_rev = hb.vjp_params_host(m, x, theta, sel, np.zeros((x.shape[0], m.output_dim)), want_y=True)
    y_m = hb.step_host(m, x)
    moved = 0
    for e in range(x.shape[0]):
        y_e = hb.step_host(hb.params_apply(m, sel, theta[e]), x[e:e + 1])[0]
        np.testing.assert_array_equal(y[e], y_e)
        np.testing.assert_array_equal(y_rev[e], y_e)
        moved += np.max(np.abs(y_e - y_m[e])) > 0
    assert moved >= x.shape[0] // 2, moved  # (the airborne states of the sweep do not feel the contact model)


@pytest.mark.parametrize("name", MODELS)
def test_every_entry_moves_the_step_on_some_state(name, built):
    """one entry at a time: value * 1.05 + 0.013 (a box's radius passes the clamp at 1e-2); 64 states, so that every
    shape of the Ant is down on one of them.  The entries of inert() leave the step where it was."""
    m, x = sweep(name, 64)
    y0 = hb.step_host(m, x)
    sel = hb.contact_params(m)
    base = hb.params_get(m, sel)
    for j, q in enumerate(sel):
        y = hb.jvp_params_host(m, x, [base[j] * 1.05 + 0.013], [q])
        np.testing.assert_array_equal(y, hb.step_host(set_param(m, q, base[j] * 1.05 + 0.013), x))
        assert (np.max(np.abs(y - y0)) > 0) == (not inert(name, m, q)), (name, q)


@pytest.mark.parametrize("name", MODELS)
def test_theta_adjoints_are_w_times_j_theta(name, built):
    m, x = sweep(name, 64)
    if name == "cartpole_plane":
        m, _ = raised_box(m)
    sel = hb.contact_params(m)
    J = j_theta(m, x, sel)
    w = np.random.default_rng(3).normal(size=(x.shape[0], 2, m.output_dim))
    wj = hb.vjp_params_host(m, x, hb.params_get(m, sel), sel, w)
    worst = rel(wj[:, :, m.input_dim:], np.einsum("nko,nop->nkp", w, J))
    print(name, "wj_theta against einsum(w, J_theta):", worst)
    assert worst <= 1e-11
    for q, a in zip(sel, np.abs(J).max(axis=(0, 1))):
        assert (a > 0) == (not inert(name, m, q)), (q, a)


# ------------------------------------------------------------------------------------------------ differences
CFM_H = 1e-7  # the absolute difference step of cfm (the blobs' cfm: 1e-5 .. 2e-3)


def fd_theta(m, x, sel, step_of_model):
    """diff_states.central_theta with its kink check; cfm with the absolute step CFM_H, every other entry with the
    existing kinds' h = 1e-6 max-free relative step (1e-6 where the value is 0)"""
    J = np.zeros((x.shape[0], m.output_dim, len(sel)))
    kink = np.zeros((x.shape[0], len(sel)), dtype=bool)
    for j, q in enumerate(sel):
        h_rel = CFM_H / m.cfm if q[0] == "cfm" else 1e-6
        Jj, kj = diff_states.central_theta(m, x, [q], step_of_model, set_param, h_rel=h_rel)
        J[:, :, j], kink[:, j] = Jj[:, :, 0], kj[:, 0]
    return J, kink


def worst_smooth(J, J_fd, kink):
    """(the worst error over the states without a kink, relative to max(1, max |J| of the state), entries compared)"""
    worst, checked = 0.0, np.zeros(J.shape[2], dtype=np.int64)
    for e in range(J.shape[0]):
        cols = np.flatnonzero(~kink[e])
        if cols.size:
            worst = max(worst, np.max(np.abs(J[e][:, cols] - J_fd[e][:, cols])) / max(1.0, np.max(np.abs(J[e]))))
            checked[cols] += 1
    return worst, checked


@pytest.mark.parametrize("name", MODELS + ["cartpole_plane_raised"])
def test_j_theta_matches_central_differences_of_the_double_step(name, built):
    """J_theta of every contact parameter against central differences of hb.step_host on blobs with the entry set, on
    the states of the contact sweep whose one-sided differences agree; bound 1e-6, the existing kinds'.
    cfm takes the absolute step CFM_H = 1e-7 (1 % of the smallest cfm, 1e-5: the relative 1e-6 would be 1e-11, below
    the step's round-off over h).  Measured maxima (host, this file's states): ant 9.0e-10, laikago_soft 8.0e-10,
    cartpole_plane 6.9e-10 (raised box radius: 1.6e-09), pendulum5_plane 9.6e-10, cube_floating 2.1e-10,
    ant_floating 1.3e-09.
    cartpole_plane's boxes carry radius 0: the clamp's constant branch, derivative exactly 0 (asserted);
    cartpole_plane_raised has one box at radius 0.03: a nonzero derivative (asserted)."""
    raised = name.endswith("_raised")
    m, x = sweep(name[:-len("_raised")] if raised else name)
    g_raised = None
    if raised:
        m, g_raised = raised_box(m)
    sel = hb.contact_params(m)
    J = j_theta(m, x, sel)
    J_fd, kink = fd_theta(m, x, sel, hb.step_host)
    worst, checked = worst_smooth(J, J_fd, kink)
    print(name, "J_theta against central differences of step_host:", f"{worst:.2e}", "states per entry:", checked.min())
    assert worst <= 1e-6, worst
    assert checked.min() >= 1, [q for q, c in zip(sel, checked) if c == 0]
    for j, q in enumerate(sel):
        if q[0] == "geom_radius" and m.geoms[q[1]].type == BOX:
            if q[1] == g_raised:
                assert np.max(np.abs(J[:, :, j])) > 0
            else:
                assert m.geoms[q[1]].radius <= 1e-2 and np.all(J[:, :, j] == 0.0) and np.all(J_fd[:, :, j] == 0.0)


@pytest.mark.parametrize("name", ["ant", "cartpole_plane_raised", "pendulum5_plane", "cube_floating", "ant_floating"])
def test_shapes_match_central_differences_of_the_oracle(name, built):
    """the shapes' kinds against central differences of the plain-C restatement of the step on applied blobs (the
    reference's setters do not reach shapes); 1e-6, the bound of the differences of the double step above"""
    raised = name.endswith("_raised")
    m, x = sweep(name[:-len("_raised")] if raised else name)
    if raised:
        m, _ = raised_box(m)
    sel = [q for q in hb.contact_params(m) if q[0].startswith("geom_")]
    J = j_theta(m, x, sel)
    J_fd, kink = fd_theta(m, x, sel, lambda mm, xx: oraclelib.step(mm, xx))
    worst, checked = worst_smooth(J, J_fd, kink)
    print(name, "shapes against central differences of the oracle:", f"{worst:.2e}", "states per entry:", checked.min())
    assert worst <= 1e-6, worst
    assert checked.min() >= 1 and np.count_nonzero(J) > 0


needs_ref = pytest.mark.skipif(not reflib.available(), reason="the reference library is not built here")


@needs_ref
@pytest.mark.parametrize("name", ["ant", "laikago_soft", "pendulum5_plane"])
def test_cfm_and_erp_match_the_reference(name, built):
    """central differences of the reference's step under set_solver(cfm, erp, ...), h = 1e-6 as the existing reference
    checks take it (cfm: CFM_H), bound 1e-6, on the sweep's states without a kink"""
    import gen_golden  # noqa: E402  (checker only: the table of reference constructors)

    m, x = sweep(name)
    sel = [("cfm",), ("erp",)]
    J = j_theta(m, x, sel)
    _, kink = fd_theta(m, x, sel, hb.step_host)

    def ref_step(cfm, erp):
        r, _ = gen_golden.make_ref(name)
        try:
            r.set_solver(cfm, erp, m.pgs_iterations, m.friction, m.restitution)
            return r.step(x)
        finally:
            r.close()

    for j, h in ((0, CFM_H), (1, 1e-6)):
        d = [h if j == 0 else 0.0, h if j == 1 else 0.0]
        fd = (ref_step(m.cfm + d[0], m.erp + d[1]) - ref_step(m.cfm - d[0], m.erp - d[1])) / (2 * h)
        envs = np.flatnonzero(~kink[:, j])
        assert envs.size >= 1 and np.count_nonzero(J[envs][:, :, j]) > 0, sel[j]
        worst = max(np.max(np.abs(J[e][:, j] - fd[e])) / max(1.0, np.max(np.abs(J[e][:, j]))) for e in envs)
        print(name, sel[j], "against central differences of the reference:", f"{worst:.2e}", f"({envs.size} states)")
        assert worst <= 1e-6, (sel[j], worst)


# ------------------------------------------------------------------------------------------------ tapes
def test_tape_lengths_fit_the_capacity_with_every_old_and_new_parameter(built):
    """the longest tape per model with all_params + contact_params selected, over the golden records and over the
    contact sweep of tests/diff_states.py (DESIGN 7a's table: its last column), beside the old selection's: every
    class's longest is at or below its capacity"""
    longest = {c: 0 for c in CAPACITY}
    print()
    for name, cls in CLASS_OF.items():
        m = tds_amd.load_model(name)
        rows = []
        for x in (np.load(os.path.join(ROOT, "tests", "golden", f"{name}.npz"))["x"],
                  # (the sweep of tests/test_diff_sweep_cpu.py, over which DESIGN's table was counted)
                  diff_states.states(name, 400 if name == "ant" else 300, 1, m) if name in diff_states.MODELS else None):
            if x is None:
                rows.append((None, None))
                continue
            w = np.zeros((x.shape[0], m.output_dim))
            out = []
            for sel in (hb.all_params(m), hb.all_params(m) + hb.contact_params(m)):
                _, lens = hb.vjp_params_host(m, x, hb.params_get(m, sel), sel, w, tape_len=True, tape_cap=1 << 22)
                assert np.all(lens > 0), name
                out.append(int(lens.max()))
            rows.append(tuple(out))
            longest[cls] = max(longest[cls], out[1])
        if name in OLD_GOLDEN:  # an old-kind selection records what it recorded: unselected, the new reads add no entry
            assert rows[0][0] == OLD_GOLDEN[name], (name, rows[0][0])
        p_old, p_new = len(hb.all_params(m)), len(hb.contact_params(m))
        print(f"class {cls} {name:22s} p = {p_old} + {p_new}: golden {rows[0][0]} -> {rows[0][1]}, "
              f"sweep {rows[1][0]} -> {rows[1][1]}")
    for cls, cap in CAPACITY.items():
        print(f"class {cls}: longest {longest[cls]}, capacity {cap}, margin {100.0 * (cap - longest[cls]) / cap:.0f} %")
        assert 0 < longest[cls] <= cap, (cls, longest[cls], cap)


# ------------------------------------------------------------------------------------------------ trajectory
def test_trajectory_vjp_matches_central_differences_of_chained_steps(built):
    """laikago_soft, 5 steps, theta = [cfm, erp, a foot's radius]: gtheta of trajectory_vjp_host against central
    differences of chained step_host rollouts on applied blobs, 1e-6 (cfm: CFM_H)"""
    name, steps, n = "laikago_soft", 5, 6
    m = tds_amd.load_model(name)
    x0 = np.ascontiguousarray(diff_states.states(name, n, 11, m))
    nsd, n_act, _ = hb.trajectory_dims(m, steps)
    foot = next(g for g in range(m.num_geoms) if m.geoms[g].type == 0)
    sel = [("cfm",), ("erp",), ("geom_radius", foot)]
    theta = hb.params_get(m, sel)
    u = np.random.default_rng(12).uniform(-0.2, 0.2, (n, steps - 1, n_act))
    gs = np.random.default_rng(14).normal(size=(n, steps, nsd))
    s, gx0, gu, gth = hb.trajectory_vjp_host(m, x0, gs, steps, 1, u, sel, theta)

    def rollout(th):
        mm = hb.params_apply(m, sel, th)
        x, out = x0.copy(), []
        for t in range(steps):
            if t > 0:
                x[:, nsd:nsd + n_act] = u[:, t - 1]
            y = hb.step_host(mm, x)
            x[:, :nsd] = y[:, :nsd]
            out.append(y[:, :nsd].copy())
        return np.stack(out, axis=1)

    np.testing.assert_array_equal(s, rollout(theta))
    loss = lambda th: np.einsum("nrs,nrs->n", gs, rollout(th))  # noqa: E731
    assert np.count_nonzero(gth) > 0
    for j, h in enumerate((CFM_H, 1e-6, 1e-6)):
        d = np.zeros(3)
        d[j] = h
        l0, lp, lm, lp2, lm2 = (loss(theta + k * d) for k in (0, 1, -1, 2, -2))
        fd = (lp - lm) / (2 * h)
        smooth = np.abs((-3 * l0 + 4 * lp - lp2) - (3 * l0 - 4 * lm + lm2)) / (2 * h) <= 1e-5 * np.maximum(1.0, np.abs(fd))
        err = np.abs(fd - gth[:, j]) / np.maximum(1.0, np.abs(gth[:, j]))
        print(sel[j], "trajectory gtheta against central differences:", err[smooth].max(), f"({smooth.sum()} of {n})")
        assert smooth.sum() >= n // 2 and err[smooth].max() <= 1e-6, (sel[j], err, smooth)
