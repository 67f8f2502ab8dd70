"""CPU: per-environment model variants, the host side — params_apply (the inverse of params_get: "the model of variant
v"), against the per-environment theta of the parameter derivatives' double step, the checks of
tds_hip_model_variants_host (sizes, maps, structure, refusals), and the stand-alone sanitizer program of
tools/variants_sanitize.cpp."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import tds_amd
from tds_amd import hip_backend as hb

INERTIA_IDX = [(0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)]
# golden rows per model on which EVERY selectable kind moves the step (friction and restitution need an active
# contact; the Ant's first rows are the ones tests/test_param_derivs_cpu.py compares with the reference)
ROWS = {"ant": [0, 1, 2, 3, 4, 5], "ant_floating": [0, 1, 2, 3, 4, 5], "laikago": [0, 1, 2, 20, 35],
        "pendulum5_plane": [0, 1, 2, 3, 4, 5], "cube_floating": [0, 1, 2, 4, 5, 6]}


def golden(name):
    return np.load(os.path.join(ROOT, "tests", "golden", f"{name}.npz"))["x"][ROWS[name]]


def blob(m):
    return C.string_at(C.byref(m), C.sizeof(m))


def assign(m, q, value):
    """field-by-field: a copy of m with the scalar a param_spec tuple names set to value"""
    m = m.copy()
    name = q[0]
    _, on_link, _ = hb.PARAM_KINDS[name]
    rest = list(q[1:])
    link = rest.pop(0) if on_link else 0
    comp = rest.pop(0) if rest else 0
    if name in ("mass", "stiffness", "damping"):
        setattr(m.links[link], name, value)
    elif name == "com":
        m.links[link].com[comp] = value
    elif name == "xt_trans":
        m.links[link].X_T_trans[comp] = value
    elif name in ("inertia", "base_inertia"):
        r, c = INERTIA_IDX[comp]
        arr = m.links[link].inertia if name == "inertia" else m.base_inertia
        arr[3 * r + c] = value
        arr[3 * c + r] = value
    elif name == "base_mass":
        m.base_mass = value
    elif name == "base_com":
        m.base_com[comp] = value
    elif name == "gravity":
        m.gravity[comp] = value
    else:
        setattr(m, name, value)
    return m


def draw_theta(m, sel, n, seed=4):
    """+- 5 % relative, + +- 0.01 additive except on inertias (zero inertia products stay zero: M stays SPD)"""
    base = hb.params_get(m, sel)
    rng = np.random.default_rng(seed)
    additive = np.array([not q[0].endswith("inertia") for q in sel])
    return base * (1.0 + 0.05 * rng.uniform(-1, 1, (n, len(sel)))) + 0.01 * rng.uniform(-1, 1, (n, len(sel))) * additive


def test_params_apply_round_trips_and_equals_field_assignment(built):
    m = tds_amd.load_model("ant_floating")
    sel = hb.all_params(m)
    theta = draw_theta(m, sel, 1)[0]
    m2 = hb.params_apply(m, sel, theta)
    np.testing.assert_array_equal(hb.params_get(m2, sel), theta)
    assert blob(hb.params_apply(m2, sel, hb.params_get(m, sel))) == blob(m)  # ... and back
    assert blob(hb.params_apply(m, [], [])) == blob(m)
    assert tds_amd.params_apply is hb.params_apply
    # one entry of each of the twelve kinds (an off-diagonal inertia comp sets both mirror entries)
    one_each = [("mass", 3), ("com", 3, 2), ("inertia", 2, 4), ("xt_trans", 1, 0), ("stiffness", 0), ("damping", 5),
                ("base_mass",), ("base_com", 1), ("base_inertia", 5), ("gravity", 2), ("friction",), ("restitution",)]
    assert sorted(hb.PARAM_KINDS[q[0]][0] for q in one_each) == list(range(12))
    for j, q in enumerate(one_each):
        value = 0.125 + 0.01 * j
        got, want = hb.params_apply(m, [q], [value]), assign(m, q, value)
        assert blob(got) == blob(want), q
        assert blob(got) != blob(m), q
    values = 0.2 + 0.01 * np.arange(12)
    want = m
    for q, v in zip(one_each, values):
        want = assign(want, q, v)
    assert blob(hb.params_apply(m, one_each, values)) == blob(want)


@pytest.mark.parametrize("sel,match", [
    ([hb.Param(12, 0, 0, 0)], "unknown parameter kind"),
    ([("mass", 14)], "link index out of range"),
    ([("com", 2, 3)], "component index out of range"),
    ([("mass", 2), ("mass", 2)], "duplicate parameter"),
    ([("base_mass",)], "floating base"),
])
def test_params_apply_refuses_what_params_get_refuses(sel, match, built):
    m = tds_amd.load_model("ant")
    for call in (lambda: hb.params_get(m, sel), lambda: hb.params_apply(m, sel, np.zeros(len(sel)))):
        with pytest.raises(hb.TdsHipError, match=match) as e:
            call()
        assert "tds_hip error 1:" in str(e.value)


@pytest.mark.parametrize("name", list(ROWS))
def test_applied_model_steps_as_the_per_environment_theta(name, built):
    """step_host of the applied model == the parameter derivatives' double step at that theta, bit for bit; and every
    kind of the selection moves the step on at least one environment of the batch"""
    m = tds_amd.load_model(name)
    x = golden(name)
    sel = hb.all_params(m)
    theta = draw_theta(m, sel, x.shape[0])
    y = hb.jvp_params_host(m, x, theta, sel)
    for e in range(x.shape[0]):
        np.testing.assert_array_equal(hb.step_host(hb.params_apply(m, sel, theta[e]), x[e:e + 1])[0], y[e])
    base = hb.params_get(m, sel)
    y0 = hb.step_host(m, x)
    for kind in sorted(set(q[0] for q in sel)):
        only = np.array([q[0] == kind for q in sel])
        th = np.where(only, theta, base)
        moved = [np.any(hb.step_host(hb.params_apply(m, sel, th[e]), x[e:e + 1])[0] != y0[e]) for e in range(x.shape[0])]
        assert any(moved), (name, kind)


ANT_SEL = [("mass", 7), ("com", 8, 1), ("inertia", 9, 3), ("xt_trans", 10, 0), ("stiffness", 11), ("damping", 12),
           ("gravity", 2), ("friction",), ("restitution",)]


def test_model_variants_host_sizes(built):
    m = tds_amd.load_model("ant")
    n = 70
    dev64 = hb.model_variants_host(m, ANT_SEL, draw_theta(m, ANT_SEL, 1), env_variant=np.zeros(n), num_envs=n)
    dev32 = hb.model_variants_host(m, ANT_SEL, draw_theta(m, ANT_SEL, 1), env_variant=np.zeros(n), num_envs=n, dtype="f32")
    # the device model is integers + scalars: the float one is smaller, but more than half of the double one
    assert dev64 // 2 < dev32 < dev64 and dev64 % 8 == 0
    for v, ev in ((1, np.zeros(n)), (3, np.arange(n) % 3), (n, None), (n, np.arange(n)[::-1])):
        theta = draw_theta(m, ANT_SEL, v)
        assert hb.model_variants_host(m, ANT_SEL, theta, env_variant=ev, num_envs=n) == v * dev64
        assert hb.model_variants_host(m, ANT_SEL, theta, env_variant=ev, num_envs=n, dtype="mixed") == v * dev64
        assert hb.model_variants_host(m, ANT_SEL, theta, env_variant=ev, num_envs=n, dtype="f32") == v * dev32
    mf = tds_amd.load_model("ant_floating")
    self = [("base_mass",), ("base_com", 1), ("base_inertia", 4), ("mass", 2), ("friction",)]
    assert hb.model_variants_host(mf, self, draw_theta(mf, self, 5)) == 5 * dev64


@pytest.mark.parametrize("sel,match", [
    ([hb.Param(12, 0, 0, 0)], "unknown parameter kind"),
    ([("mass", 14)], "link index out of range"),
    ([("mass", 7), ("mass", 7)], "duplicate parameter"),
    ([("base_mass",)], "floating base"),
])
def test_model_variants_host_refuses_bad_selections(sel, match, built):
    m = tds_amd.load_model("ant")
    with pytest.raises(hb.TdsHipError, match=match) as e:
        hb.model_variants_host(m, sel, np.ones((2, len(sel))))
    assert "tds_hip error 1:" in str(e.value)


def test_model_variants_host_refuses_bad_maps_and_structure(built):
    m = tds_amd.load_model("ant")
    n = 8
    theta = draw_theta(m, ANT_SEL, 3)
    for ev in (np.array([0, 1, 2, 3, 0, 1, 2, 0]), np.array([0, 1, 2, -1, 0, 1, 2, 0])):  # out of [0, V)
        with pytest.raises(hb.TdsHipError, match="maps to variant") as e:
            hb.model_variants_host(m, ANT_SEL, theta, env_variant=ev, num_envs=n)
        assert "tds_hip error 1:" in str(e.value)
    with pytest.raises(hb.TdsHipError, match="9 variants for 8 environments") as e:  # V > num_envs
        hb.model_variants_host(m, ANT_SEL, draw_theta(m, ANT_SEL, 9), env_variant=np.zeros(n), num_envs=n)
    assert "tds_hip error 1:" in str(e.value)
    with pytest.raises(hb.TdsHipError, match="no environment map") as e:  # NULL map, V != N
        hb.model_variants_host(m, ANT_SEL, theta, num_envs=n)
    assert "tds_hip error 1:" in str(e.value)
    # a mass on a massless link of the Ant's root chain: the chain is no longer ONE joint of the torso
    sel = [("mass", 7), ("mass", 2)]
    th = np.array([[0.04, 0.0], [0.05, 0.0], [0.04, 0.3]])
    with pytest.raises(hb.TdsHipError, match=r"variant 2 differs from the base model in structure \(field root_last\)") as e:
        hb.model_variants_host(m, sel, th, env_variant=np.arange(n) % 3, num_envs=n)
    assert "tds_hip error 1:" in str(e.value)
    assert hb.model_variants_host(m, sel, th[:2], env_variant=np.arange(n) % 2, num_envs=n) > 0
    # a joint spring on a root link: the root chain leaves its closed form
    with pytest.raises(hb.TdsHipError, match=r"variant 0 .*\(field euler_root\)"):
        hb.model_variants_host(m, [("stiffness", 2)], np.array([[0.5]]), env_variant=np.zeros(n), num_envs=n)


@pytest.mark.parametrize("name", ["pendulum5_spherical", "three_pendulums_plane"])
def test_model_variants_host_refuses_what_the_parameter_functions_refuse(name, built):
    m = tds_amd.load_model(name)
    with pytest.raises(hb.TdsHipError) as e_par:
        hb.jvp_params_host(m, np.zeros((1, m.input_dim)), [1.0], [("mass", 0)])
    with pytest.raises(hb.TdsHipError, match="not supported") as e:
        hb.model_variants_host(m, [("mass", 0)], np.array([[1.0]]))
    assert "tds_hip error 2:" in str(e.value) and str(e.value) == str(e_par.value)


def test_variant_symbols_are_declared_and_exported(built):
    hdr = open(os.path.join(ROOT, "include", "tds_hip.h")).read()
    for s in ("tds_hip_params_apply", "tds_hip_set_model_variants", "tds_hip_model_variants", "tds_hip_model_variants_host"):
        assert s + "(" in hdr and s in hb.EXPORTED_SYMBOLS and hb.lib_has_symbol(s), s
    assert tds_amd.TDS_HIP_ABI_VERSION == 5


def test_stand_alone_program_under_the_host_sanitizers(built, tmp_path):
    """tools/variants_sanitize.cpp + csrc/tds_variants.hip compiled with -fsanitize=address,undefined into a program of
    its own (no Python, no GPU): tds_hip_params_apply and tds_hip_model_variants_host on the Ant blob.  A check of the
    build machine: sanitizer runs stay off the machines that hold a GPU."""
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present: the sanitizer program runs where the library is built")
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    csrc = os.path.join(ROOT, "tiny-differentiable-simulator_amd", "csrc")
    blob_file = tmp_path / "ant.blob"
    blob_file.write_bytes(blob(tds_amd.load_model("ant")))
    exe = tmp_path / "variants_sanitize"
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host",
                           "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
                           os.path.join(ROOT, "tools", "variants_sanitize.cpp"), os.path.join(csrc, "tds_variants.hip"),
                           "-o", str(exe)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe), str(blob_file)], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "variants_sanitize: ok" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr
