"""The synthetic stars of tests/star_cases.py, checked without a GPU: the curated list's coverage facts, the launch planner
(every star plans onto its kind's kernel, every near miss — one property off — onto the general kernel), and the control
that the stars' states are well conditioned: the two CPU statements of the step, the C oracle and hip_backend.step_host,
agree on every star and state.  That control measures the references against each other, never the kernels; the kernels
are tests/test_star_kernels_gpu.py's.  (oracle/_ref, the compiled reference, cannot express a synthetic model: there is no
third statement.)

Measured over the curated list (rel_err, floor 1e-3): step_host against the oracle at most 1.0e-11 on the oct stars
(oct-cycle0; 1.3e-12 on the Ant itself) and 2.2e-12 on the quad stars (quad-revolute; 4.6e-13 on Laikago); the bound is
ten times the larger, 1.0e-10.  The oracle's largest |y| per star is 8.3 .. 30 (oct) and 183 .. 686 (quad)."""
import ctypes as C

import numpy as np
import pytest

import tds_amd
from tds_amd import hip_backend
from conftest import rel_err
from test_launch_plan import MI355X
import star_cases as sc

J = tds_amd.model
# the largest step_host-vs-oracle error over the curated list, per kind (measured; the bound below is 10 x the larger)
HOST_VS_ORACLE_MEASURED = {"oct": 1.0e-11, "quad": 2.2e-12}
HOST_VS_ORACLE_BOUND = 10 * max(HOST_VS_ORACLE_MEASURED.values())
IDS = [c["id"] for c in sc.CASES]


def _plan(m):
    return hip_backend.launch_plan_host(m, "f64", 64, **MI355X)["kernel"]


def _rotx(a):
    return [1.0, 0.0, 0.0, 0.0, np.cos(a), -np.sin(a), 0.0, np.sin(a), np.cos(a)]


@pytest.mark.parametrize("kind", sc.KINDS)
def test_the_list_covers_what_the_kernels_read(kind, built):
    cases = sc.of_kind(kind)
    assert len(cases) >= 6 + 1
    models = [sc.star(c) for c in cases]
    legs, hips, lasts = sc.leg_joint_links(kind), sc.hip_links(kind), sc.last_joint_links(kind)
    # the unmodified model is a member
    plain = tds_amd.load_model(sc.BASE[kind])
    assert any(bytes(m) == bytes(plain) for m in models)
    # every 1-dof joint type on a hip and on a last actuated leg link (oct: an even and an odd lane)
    assert {m.links[i].joint_type for m in models for i in hips} == set(sc.JOINT_KINDS)
    assert {m.links[i].joint_type for m in models for i in lasts} == set(sc.JOINT_KINDS)
    # an unnormalised free axis of both kinds
    for jt, part in ((J.JOINT_REVOLUTE_AXIS, slice(0, 3)), (J.JOINT_PRISMATIC_AXIS, slice(3, 6))):
        norms = [np.linalg.norm([m.links[i].S[k] for k in range(6)][part]) for m in models for i in legs
                 if m.links[i].joint_type == jt]
        assert norms and max(abs(n - 1.0) for n in norms) > 0.1
    # both values of XT_IDENT: identity on all leg links, and a rotation on every leg link
    ident = [[sc.xt_is_identity(m, i) for i in legs] for m in models]
    assert any(all(row) for row in ident) and any(not any(row) for row in ident)
    assert any(all(m.links[i].joint_type in sc.PRISMATIC for i in legs) for m in models)
    assert any(all(m.links[i].joint_type in sc.REVOLUTE for i in legs) for m in models)
    for present in (True, False):   # springs and dampers on some stars, none on others
        assert any(all((m.links[i].stiffness > 0 and m.links[i].damping > 0) == present for i in legs) for m in models)
    assert any(abs(m.links[i].inertia[k]) > 0 for m in models for i in range(5, m.num_links) for k in (1, 2, 5))
    assert any(abs(m.links[5].inertia[1]) > 0 for m in models)
    assert any(any(m.links[5].com[k] != 0 for k in range(3)) for m in models)
    tilted = [m.plane_normal[2] != 1.0 for m in models]
    assert any(tilted) and not all(tilted)
    for m in models:
        assert abs(np.linalg.norm([m.plane_normal[k] for k in range(3)]) - 1.0) < 1e-15
        assert np.arccos(min(1.0, m.plane_normal[2])) <= 0.1 + 1e-12
        assert 0.3 <= m.friction <= 1.0
        for i in range(5, m.num_links):   # symmetric, positive definite inertias
            I = np.array([m.links[i].inertia[k] for k in range(9)]).reshape(3, 3)
            assert np.array_equal(I, I.T) or np.allclose(I, I.T, rtol=0, atol=1e-18)
            assert np.linalg.eigvalsh((I + I.T) / 2).min() > 0
    assert any(m.plane_constant != 0 for m in models)
    assert any(m.restitution == 0 for m in models) and any(m.restitution > 0 for m in models)
    assert {m.pgs_iterations for m in models} == {1, 2, 3}
    full = 9 if kind == "oct" else 17
    assert {m.num_visuals if m.pack_visuals else 0 for m in models} == {0, full}
    for m in models:
        nv = m.num_visuals if m.pack_visuals else 0
        assert m.output_dim >= m.dof_q + m.dof_qd + (7 * nv + 1 if nv else 0)
    assert {m.reward_mode for m in models} == set(sc.REWARDS)
    if kind == "quad":
        assert any(m.pd_start_link > 6 and m.action_dim < 12 and m.input_dim == 36 + m.action_dim + 3 for m in models)
        assert any(m.pd_start_link == 6 and m.action_dim == 12 for m in models)
    # the float-record test's two stars exist and differ
    assert len({c["id"] for c in sc.mixed_cases(kind)}) == 2


@pytest.mark.parametrize("cid", IDS)
def test_every_star_plans_onto_its_kernel(cid, built):
    c = sc.by_id(cid)
    m = sc.star(c)
    hip_backend.model_check(m)
    assert _plan(m) == sc.KERNEL[c["kind"]]
    with hip_backend.default_options(**{c["kind"]: 0}):
        assert _plan(m) == "general"
    # every build is reachable at 64 environments by option
    if c["kind"] == "oct":
        for w2, build in ((0, 1), (2, 3), (3, 2)):
            with hip_backend.default_options(oct_w2=w2):
                p = hip_backend.launch_plan_host(m, "f64", 64, nsub=12, rings=1, **MI355X)
            assert (p["kernel"], p["build"]) == ("oct8", build)
    else:
        for wide, build in ((0, 1), (2, 8)):
            with hip_backend.default_options(quad_wide=wide):
                p = hip_backend.launch_plan_host(m, "f64", 64, nsub=12, rings=1, **MI355X)
            assert (p["kernel"], p["build"]) == ("quad16", build)


# ---- near misses: one property off, the rule of the detection it trips (csrc/tds_device_model.h: euler_root,
#      star_actuation, the quad block; csrc/tds_oct_model.h: tds_oct_detect) ----
def _spring_on_a_root_link(m, kind):
    m.links[3].stiffness = 1.0


def _damper_on_link_5(m, kind):
    m.links[5].damping = 0.1


def _rotated_base_frame(m, kind):
    sc._set(m.base_X_world_rot, _rotx(0.3))


def _rotated_xt_on_a_root_link(m, kind):
    sc._set(m.links[4].X_T_rot, _rotx(0.2))


def _visual_below_link_5(m, kind):
    m.visuals[0].link = 4


def _geometry_below_link_5(m, kind):
    m.geoms[0].link = 4   # (oct: the root sphere; quad: the first toe's sphere)


def _capsule_on_another_link(m, kind):
    m.geoms[1].link = 7


def _no_root_sphere(m, kind):
    for g in range(1, m.num_geoms):
        C.memmove(C.byref(m.geoms[g - 1]), C.byref(m.geoms[g]), C.sizeof(m.geoms[g]))
    m.num_geoms -= 1
    assert m.num_contacts == 16


def _five_visuals(m, kind):
    m.num_visuals = 5


def _nine_visuals(m, kind):
    m.num_visuals = 9


def _ankle_on_the_root(m, kind):
    m.links[7].parent = 5


def _tau_mode(m, kind):
    m.step_mode = J.TDS_STEP_TAU
    m.action_dim = m.dof_qd
    m.input_dim = m.dof_q + m.dof_qd + m.action_dim


def _pd_loop_from_link_5(m, kind):
    m.pd_start_link = 5
    m.action_dim += 1
    m.input_dim += 1


def _toe_with_a_joint(m, kind):
    l = m.links[9]
    l.joint_type = J.JOINT_REVOLUTE_X
    sc._set(l.S, [1.0, 0, 0, 0, 0, 0])
    l.q_index = l.qd_index = 9
    for i in range(10, m.num_links):
        if m.links[i].joint_type != J.JOINT_FIXED:
            m.links[i].q_index += 1
            m.links[i].qd_index += 1
    m.dof_q += 1
    m.dof_qd += 1
    m.action_dim += 1
    m.input_dim = m.dof_q + m.dof_qd + m.action_dim + 3


def _toe_sphere_on_the_shin(m, kind):
    m.geoms[0].link = 8


NEAR_MISSES = [
    # (kinds, change, the rule it trips)
    (sc.KINDS, _spring_on_a_root_link, "euler_root: links 0..5 carry no spring or damper"),
    (sc.KINDS, _damper_on_link_5, "euler_root: links 0..5 carry no spring or damper"),
    (sc.KINDS, _rotated_base_frame, "euler_root: the base frame is the world frame"),
    (sc.KINDS, _rotated_xt_on_a_root_link, "euler_root: identity X_T on links 0..5"),
    (sc.KINDS, _visual_below_link_5, "euler_root: nothing hangs on links 0..4"),
    (sc.KINDS, _geometry_below_link_5, "euler_root: nothing hangs on links 0..4"),
    (("oct",), _capsule_on_another_link, "oct: contact points 1 + 2 l and 2 + 2 l belong to leg link 6 + l"),
    (("oct",), _no_root_sphere, "oct: 17 contact points, the first on link 5"),
    (("oct",), _five_visuals, "oct: 0 or 9 visuals"),
    (("oct",), _ankle_on_the_root, "oct: an odd leg link's parent is the link in front of it"),
    (("oct",), _tau_mode, "star_actuation: the env step with PD control"),
    (("oct",), _pd_loop_from_link_5, "star_actuation: no action on links 0..5"),
    (("quad",), _toe_with_a_joint, "quad: 22 links, 18 dofs, every fourth leg link fixed"),
    (("quad",), _toe_sphere_on_the_shin, "quad: contact point k belongs to toe 9 + 4 k"),
    (("quad",), _nine_visuals, "quad: 0 or 17 visuals"),
    (("quad",), _tau_mode, "star_actuation: the env step with PD control"),
    (("quad",), _pd_loop_from_link_5, "star_actuation: no action on links 0..5"),
]


@pytest.mark.parametrize("kind,change,rule", [(k, f, r) for ks, f, r in NEAR_MISSES for k in ks],
                         ids=[f"{k}-{f.__name__[1:]}" for ks, f, _ in NEAR_MISSES for k in ks])
def test_near_misses_plan_onto_the_general_kernel(kind, change, rule, built):
    """on the unmodified model and on a star with every free property moved"""
    for c in (sc.of_kind(kind)[0], sc.of_kind(kind)[1]):
        m = sc.star(c)
        assert _plan(m) == sc.KERNEL[kind]
        change(m, kind)
        hip_backend.model_check(m)
        assert _plan(m) == "general", (c["id"], rule)


def test_near_misses_the_model_check_refuses(built):
    m = sc.star(sc.by_id("oct-cycle0"))
    m.links[7].joint_type = J.JOINT_FIXED   # a fixed ankle
    with pytest.raises(hip_backend.TdsHipError, match="q/qd indices must be dense in link order"):
        hip_backend.model_check(m)
    m = sc.star(sc.by_id("quad-cycle0"))
    m.links[8].joint_type = J.JOINT_FIXED   # a fixed shin: two fixed links per leg
    with pytest.raises(hip_backend.TdsHipError, match="q/qd indices must be dense in link order"):
        hip_backend.model_check(m)
    m = sc.star(sc.by_id("quad-pd10"))
    m.action_dim -= 1                       # a PD loop longer than the action record
    m.input_dim -= 1
    with pytest.raises(hip_backend.TdsHipError, match="more PD links than action_dim"):
        hip_backend.model_check(m)


@pytest.mark.parametrize("cid", IDS)
def test_states_cover_the_contact_counts_and_are_well_conditioned(cid, built):
    c = sc.by_id(cid)
    m = sc.star(c)
    x, counts = sc.states_of(c)
    y = sc.oracle_y(c)
    assert x.shape == (sc.N_STATES, m.input_dim) and y.shape == (sc.N_STATES, m.output_dim)
    assert not x.flags.writeable and not y.flags.writeable
    assert len(np.unique(x, axis=0)) == sc.N_STATES          # no state left out or repeated: the share skipped is 0
    assert np.isfinite(y).all()
    seen = sorted(set(int(v) for v in counts))
    for lo, hi in sc.CONTACT_BINS[c["kind"]]:
        assert any(lo <= v <= hi for v in seen), (cid, (lo, hi), seen)
    top = float(np.abs(y).max())
    print(f"{cid}: contact counts {seen}, oracle max |y| {top:.4g}")
    assert top < 1e3
    assert abs(top - sc.MAX_ABS_Y[cid]) <= 1e-6 * top       # (the recorded figure is this list's)


@pytest.mark.parametrize("cid", IDS)
def test_host_and_oracle_agree_on_every_star(cid, built):
    c = sc.by_id(cid)
    m = sc.star(c)
    x, _ = sc.states_of(c)
    y = hip_backend.step_host(m, np.array(x))
    e = rel_err(y, sc.oracle_y(c))
    print(f"{cid}: step_host vs oracle {e:.3e} (bound {HOST_VS_ORACLE_BOUND:.1e})")
    assert e < HOST_VS_ORACLE_BOUND
