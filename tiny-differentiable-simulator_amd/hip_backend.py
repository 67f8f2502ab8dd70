"""ctypes binding of libtds_hip.so (C ABI: include/tds_hip.h).

PyTorch is used for what it is good at here — device memory, streams, torch.distributed —
never for the arithmetic: every step goes through the hand-written HIP kernel.  If the
shared library is missing or no HIP device is visible the constructors raise; there is no
CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import functools
import os

from . import model as _model

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TDS_HIP_LIB", os.path.join(_HERE, "libtds_hip.so"))

TDS_OK = 0

_lib = None


class TdsHipError(RuntimeError):
    pass


def lib():
    """Load libtds_hip.so (raises if it has not been built: run __graft_entry__.build())."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise TdsHipError(f"{LIB_PATH} not built — run `python -c 'import __graft_entry__ as g; g.build()'`")
        # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64.  Import torch
        # first so that libtds_hip.so binds to the runtime torch already loaded (same streams,
        # same device contexts) instead of pulling a second copy from /opt/rocm.
        import torch  # noqa: F401
        L = C.CDLL(LIB_PATH)
        P = C.POINTER(_model.Model)
        L.tds_hip_last_error.restype = C.c_char_p
        L.tds_hip_model_check.argtypes = [P]
        L.tds_hip_create.argtypes = [P, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        L.tds_hip_destroy.argtypes = [C.c_void_p]
        L.tds_hip_set_stream.argtypes = [C.c_void_p, C.c_void_p]
        for f in ("tds_hip_num_envs", "tds_hip_input_dim", "tds_hip_output_dim", "tds_hip_dtype"):
            getattr(L, f).argtypes = [C.c_void_p]
        L.tds_hip_x_device.restype = C.c_void_p
        L.tds_hip_x_device.argtypes = [C.c_void_p]
        L.tds_hip_y_device.restype = C.c_void_p
        L.tds_hip_y_device.argtypes = [C.c_void_p]
        L.tds_hip_set_inputs.argtypes = [C.c_void_p, C.c_void_p]
        L.tds_hip_get_inputs.argtypes = [C.c_void_p, C.c_void_p]
        L.tds_hip_get_outputs.argtypes = [C.c_void_p, C.c_void_p]
        L.tds_hip_forward_zero_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.tds_hip_step.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.tds_hip_step_obs.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.tds_hip_obs_dim.argtypes = [C.c_void_p]
        L.tds_hip_set_auto_reset.argtypes = [C.c_void_p, C.c_int, C.c_ulonglong]
        L.tds_hip_reset.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.tds_hip_rollout.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_void_p,
                                      C.c_void_p, C.c_void_p]
        L.tds_hip_forward_zero_host.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.tds_hip_rollout_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_int] + [C.c_void_p] * 6
        L.tds_rb_last_error.restype = C.c_char_p
        L.tds_rb_create.argtypes = [C.POINTER(_model.RbModel), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        L.tds_rb_destroy.argtypes = [C.c_void_p]
        L.tds_rb_set_stream.argtypes = [C.c_void_p, C.c_void_p]
        L.tds_rb_state_device.argtypes = [C.c_void_p]
        L.tds_rb_state_device.restype = C.c_void_p
        L.tds_rb_set_state.argtypes = [C.c_void_p, C.c_void_p]
        L.tds_rb_get_state.argtypes = [C.c_void_p, C.c_void_p]
        L.tds_rb_step.argtypes = [C.c_void_p, C.c_int]
        L.tds_hip_set_timing.argtypes = [C.c_void_p, C.c_int]
        L.tds_hip_last_kernel_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        L.tds_hip_profile_phases.argtypes = [C.c_void_p, C.POINTER(C.c_longlong), C.c_int]
        L.tds_hip_kernel_info.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
        for f in ("tds_hip_device", "tds_hip_record_bytes", "tds_hip_sync", "tds_hip_forward_zero_host_end"):
            getattr(L, f).argtypes = [C.c_void_p]
        L.tds_hip_forward_zero_host_begin.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        for f in ("tds_hip_step_many_prepare", "tds_hip_step_many"):
            getattr(L, f).argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.tds_hip_set_graph_chains.argtypes = [C.c_void_p, C.c_int]
        for f in ("tds_hip_step_many_rings", "tds_hip_step_many_rings_prepare"):
            getattr(L, f).argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(Rings)]
        L.tds_hip_step_many_rings_blocks.argtypes = [C.c_void_p]
        L.tds_hip_step_many_is_loop.argtypes = [C.c_void_p, C.c_int]
        L.tds_hip_debug_poison_lds.argtypes = [C.c_void_p, C.c_int]
        L.tds_hip_step_many_tune.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_int)]
        # multi-GPU shards (RCCL all-gather of the observation records)
        L.tds_hip_shard_unique_id.argtypes = [C.c_void_p]
        L.tds_hip_shard_create.argtypes = [P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                           C.POINTER(C.c_void_p)]
        L.tds_hip_shard_create_all.argtypes = [P, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int,
                                               C.POINTER(C.c_void_p)]
        L.tds_hip_shard_sim.restype = C.c_void_p
        for f in ("tds_hip_shard_destroy", "tds_hip_shard_sim", "tds_hip_shard_rank", "tds_hip_shard_world",
                  "tds_hip_shard_local_envs", "tds_hip_shard_first_env", "tds_hip_shard_wire_bytes",
                  "tds_hip_shard_flush"):
            getattr(L, f).argtypes = [C.c_void_p]
        L.tds_hip_shard_set_block.argtypes = [C.c_void_p, C.c_int]
        L.tds_hip_shard_step.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.tds_hip_shard_step_many.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
        L.tds_hip_shard_step_many_prepare.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
        L.tds_hip_shard_group_step.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_void_p), C.c_int]
        L.tds_hip_shard_gathered.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int)]
        L.tds_hip_shard_ring_plan.argtypes = [C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int]
        L.tds_hip_shard_gathered_offset.argtypes = [C.c_int, C.c_int, C.c_int]
        L.tds_hip_launch_plan_host.argtypes = [P, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int,
                                               C.POINTER(C.c_int), C.c_int]
        L.tds_hip_oct_window_plan_host.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int]
        L.tds_hip_shard_gathered_offset.restype = C.c_longlong
        L.tds_hip_default_option.argtypes = [C.c_char_p, C.c_longlong]
        L.tds_hip_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_longlong]
        L.tds_hip_get_option.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_longlong), C.POINTER(C.c_int)]
        L.tds_hip_option_name.argtypes = [C.c_int]
        L.tds_hip_option_name.restype = C.c_char_p
        L.tds_hip_jvp.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        # a device call and its host twin share a tail: the handle or the model in front, the host's tape arguments
        # (tape_cap, the tape_len pointer) behind
        tape = [C.c_int, C.c_void_p]
        jac_tail = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.tds_hip_jacobian.argtypes = [C.c_void_p] + jac_tail
        L.tds_hip_jacobian_host.argtypes = [P] + jac_tail
        L.tds_hip_jacobian_tangents.argtypes = [P]
        vjp_tail = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.tds_hip_vjp.argtypes = [C.c_void_p] + vjp_tail
        L.tds_hip_vjp_host.argtypes = [P] + vjp_tail
        L.tds_hip_vjp_host_tape.argtypes = [P] + vjp_tail + tape
        PP = C.POINTER(Param)
        L.tds_hip_params_get.argtypes = [P, C.c_int, PP, C.c_void_p]
        L.tds_hip_params_apply.argtypes = [P, C.c_int, PP, C.c_void_p, P]
        L.tds_hip_set_model_variants.argtypes = [C.c_void_p, C.c_int, C.c_int, PP, C.c_void_p, C.c_void_p]
        L.tds_hip_model_variants.argtypes = [C.c_void_p]
        L.tds_hip_model_variants_host.argtypes = [P, C.c_int, C.c_int, C.c_int, C.c_int, PP, C.c_void_p, C.c_void_p,
                                                  C.POINTER(C.c_int64)]
        dp_tail = [C.c_int, C.c_void_p, C.c_int, PP, C.c_void_p, C.c_int] + [C.c_void_p] * 3
        L.tds_hip_jvp_params.argtypes = L.tds_hip_vjp_params.argtypes = [C.c_void_p] + dp_tail
        L.tds_hip_jvp_params_host.argtypes = [P] + dp_tail
        L.tds_hip_vjp_params_host.argtypes = [P] + dp_tail + tape
        tj_tail = [C.c_int] * 3 + [C.c_void_p] * 2 + [C.c_int, PP, C.c_void_p, C.c_int] + [C.c_void_p] * 3
        L.tds_hip_trajectory_jvp.argtypes = [C.c_void_p] + tj_tail
        L.tds_hip_trajectory_jvp_host.argtypes = [P] + tj_tail
        tv_tail = [C.c_int] * 3 + [C.c_void_p] * 2 + [C.c_int, PP] + [C.c_void_p] * 6
        L.tds_hip_trajectory_vjp.argtypes = [C.c_void_p] + tv_tail
        L.tds_hip_trajectory_vjp_host.argtypes = [P] + tv_tail + tape
        pv_tail = [C.c_int] * 4 + [C.c_void_p] * 2 + [C.c_int] + [C.c_void_p] * 3 + [C.c_int, PP] + [C.c_void_p] * 8
        L.tds_hip_policy_trajectory_vjp.argtypes = [C.c_void_p] + pv_tail
        L.tds_hip_policy_trajectory_vjp_host.argtypes = [P] + pv_tail + tape
        RP = C.POINTER(_model.RbModel)
        L.tds_rb_params_get.argtypes = [RP, C.c_int, PP, C.c_void_p]
        rj_tail = [C.c_int, C.c_int, C.c_void_p, C.c_int, PP, C.c_void_p, C.c_int] + [C.c_void_p] * 3
        L.tds_rb_jvp.argtypes = [C.c_void_p] + rj_tail
        L.tds_rb_jvp_host.argtypes = [RP] + rj_tail
        rv_tail = [C.c_int] * 3 + [C.c_void_p, C.c_int, PP] + [C.c_void_p] * 5 + [C.c_int]   # (.., tape_cap)
        L.tds_rb_vjp.argtypes = [C.c_void_p] + rv_tail + [C.c_size_t]                        # (.., work_bytes)
        L.tds_rb_vjp_host.argtypes = [RP] + rv_tail
        L.tds_rb_vjp_plan.argtypes = [RP] + [C.c_int] * 4 + [C.c_size_t, C.POINTER(C.c_longlong)]
        DP = C.POINTER(DynOut)
        L.tds_hip_dynamics.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 3 + [DP]
        L.tds_hip_inverse_dynamics.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 4
        L.tds_hip_point_jacobian.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        L.tds_hip_dynamics_host.argtypes = [P, C.c_int] + [C.c_void_p] * 3 + [DP]
        L.tds_hip_inverse_dynamics_host.argtypes = [P, C.c_int] + [C.c_void_p] * 4
        L.tds_hip_point_jacobian_host.argtypes = [P, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        CP = C.POINTER(ContactOut)
        L.tds_hip_contacts.argtypes = [C.c_void_p, C.c_int, C.c_void_p, CP]
        L.tds_hip_contacts_host.argtypes = [P, C.c_int, C.c_void_p, CP]
        L.tds_hip_contact_layout.argtypes = [P, C.c_void_p, C.c_void_p, C.c_void_p]
        cj_tail = [C.c_int, C.c_void_p, C.c_int, PP, C.c_void_p, C.c_int, C.c_void_p, CP, CP]
        L.tds_hip_contacts_jvp.argtypes = [C.c_void_p] + cj_tail
        L.tds_hip_contacts_jvp_host.argtypes = [P] + cj_tail
        L.tds_hip_contacts_jvp_tangents.argtypes = [P]
        dj_tail = [C.c_int] + [C.c_void_p] * 3 + [C.c_int, PP, C.c_void_p, C.c_int, C.c_void_p]
        L.tds_hip_dynamics_jvp.argtypes = [C.c_void_p] + dj_tail + [DP, DP]
        L.tds_hip_inverse_dynamics_jvp.argtypes = [C.c_void_p] + dj_tail + [C.c_void_p] * 2
        L.tds_hip_dynamics_jvp_host.argtypes = [P] + dj_tail + [DP, DP]
        L.tds_hip_inverse_dynamics_jvp_host.argtypes = [P] + dj_tail + [C.c_void_p] * 2
        L.tds_hip_dynamics_jvp_tangents.argtypes = [P]
        IP = C.POINTER(IkOptions)
        L.tds_hip_ik_default_options.argtypes = [IP]
        L.tds_hip_ik_default_options.restype = None
        ik_tail = [C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.c_void_p, C.c_void_p, IP] + \
            [C.c_void_p] * 4
        L.tds_hip_inverse_kinematics.argtypes = [C.c_void_p] + ik_tail
        L.tds_hip_inverse_kinematics_host.argtypes = [P] + ik_tail
        # (the box forms: two bounds more among the inputs; the Riccati pass two outputs more as well.  The host's
        # Riccati pass takes no model, its rollout the number of problems P)
        for box, lq_tail, fb_tail in (("", [C.c_int] * 4 + [C.c_void_p] * 12, [C.c_void_p] * 9),
                                      ("_box", [C.c_int] * 4 + [C.c_void_p] * 16, [C.c_void_p] * 11)):
            getattr(L, f"tds_hip_lqr_backward{box}").argtypes = [C.c_void_p] + lq_tail
            getattr(L, f"tds_hip_lqr_backward{box}_host").argtypes = lq_tail
            getattr(L, f"tds_hip_feedback_rollout{box}").argtypes = [C.c_void_p, C.c_int, C.c_int] + fb_tail
            getattr(L, f"tds_hip_feedback_rollout{box}_host").argtypes = [P, C.c_int, C.c_int, C.c_int] + fb_tail
        lm_tail = [C.c_int] * 5 + [C.c_void_p] * 16
        L.tds_hip_lm_step.argtypes = [C.c_void_p] + lm_tail
        L.tds_hip_lm_step_host.argtypes = lm_tail
        _lib = L
    return _lib


class DynOut(C.Structure):
    """tds_dyn_out_t: the outputs of a dynamics query, each pointer NULL where the output is not wanted"""
    _fields_ = [("x_world", C.c_void_p), ("mass_matrix", C.c_void_p), ("bias", C.c_void_p), ("qdd", C.c_void_p)]


DYN_OUTPUTS = ("x_world", "mass_matrix", "bias", "qdd")


CONTACT_OUTPUTS = ("contacts", "jac", "rows", "rhs", "delassus", "impulse", "force", "qd_pre", "qd_post")


class ContactOut(C.Structure):
    """tds_contact_out_t: the outputs of a contact query, each pointer NULL where the output is not wanted"""
    _fields_ = [(k, C.c_void_p) for k in CONTACT_OUTPUTS]


class IkOptions(C.Structure):
    """tds_ik_options_t: the settings of an inverse-kinematics call (defaults: tds_hip_ik_default_options)"""
    _fields_ = [("method", C.c_int32), ("max_iterations", C.c_int32), ("lambda_", C.c_double),
                ("target_tolerance", C.c_double), ("step_tolerance", C.c_double), ("alpha", C.c_double),
                ("weight_reference", C.c_double)]


IK_MAX_TARGETS = 4
IK_TRANSPOSE, IK_PINV, IK_DAMPED_LM = 0, 1, 2    # TDS_IK_*: the reference's TinyIKMethod
IK_FAILED, IK_CONVERGED, IK_REACHED = 0, 1, 2    # the reference's TinyIKStatus
IK_METHODS = {"transpose": IK_TRANSPOSE, "pinv": IK_PINV, "damped_lm": IK_DAMPED_LM}
IK_OPTIONS = ("max_iterations", "lambda_", "target_tolerance", "step_tolerance", "alpha", "weight_reference")


def ik_options(method="pinv", **options) -> IkOptions:
    """the library's defaults with `method` (a name of IK_METHODS or a TDS_IK_* code) and the given IK_OPTIONS set
    (`lambda` is spelled lambda_ or lam)"""
    o = IkOptions()
    lib().tds_hip_ik_default_options(C.byref(o))
    if isinstance(method, str):
        if method not in IK_METHODS:
            raise ValueError(f"unknown inverse-kinematics method {method!r} (one of {tuple(IK_METHODS)})")
        method = IK_METHODS[method]
    o.method = int(method)
    if "lam" in options:
        options["lambda_"] = options.pop("lam")
    for k, v in options.items():
        if k not in IK_OPTIONS:
            raise ValueError(f"unknown inverse-kinematics option {k!r} (one of {IK_OPTIONS})")
        setattr(o, k, v)
    return o


_IK_DTYPES = {"iterations": "int32", "status": "int32"}  # of an inverse-kinematics call's outputs, the others float64


def _ik_shapes(m, n):
    return {"q": (n, m.dof_q), "iterations": (n,), "status": (n,), "residual": (n,)}


def _ik_targets(links, body_points):
    """links [K] and body_points [K, 3] (None: the links' origins) as the C arrays of an inverse-kinematics call"""
    import numpy as np

    links = np.ascontiguousarray(np.asarray(links, dtype=np.int32).reshape(-1))
    k = links.shape[0]
    pts = np.zeros((k, 3)) if body_points is None else np.ascontiguousarray(body_points, dtype=np.float64)
    if pts.shape != (k, 3):
        raise ValueError(f"body_points must be [{k}, 3]")
    return k, links, pts, links.ctypes.data_as(C.POINTER(C.c_int32)), pts.ctypes.data_as(C.POINTER(C.c_double))


def dyn_shapes(m: _model.Model, n: int) -> dict:
    """shapes of the outputs of a dynamics query over n states"""
    nd = m.dof_qd
    return {"x_world": (n, m.num_links, 12), "mass_matrix": (n, nd, nd), "bias": (n, nd), "qdd": (n, nd)}


def dyn_tau_dim(m: _model.Model) -> int:
    """entries of a dynamics query's tau: the actuated dofs (a floating base's six are not actuated)"""
    return m.dof_qd - (6 if m.is_floating else 0)


def _dyn_want(want):
    want = (want,) if isinstance(want, str) else tuple(want)
    for k in want:
        if k not in DYN_OUTPUTS:
            raise ValueError(f"unknown dynamics output {k!r} (one of {DYN_OUTPUTS})")
    return want


def contact_layout(m: _model.Model) -> dict:
    """The model's plane contact points (tds_hip_contact_layout): n_c, per point its link [n_c] (-1: the base) and
    the index of its geometry [n_c] (int32), and the directions of the solver's rows: normal, t1, t2 [3] each"""
    import numpy as np

    nc = lib().tds_hip_contact_layout(C.byref(m), None, None, None)
    if nc < 0:
        _check(-nc)
    link, geom, dirs = np.zeros(nc, dtype=np.int32), np.zeros(nc, dtype=np.int32), np.zeros(9)
    lib().tds_hip_contact_layout(C.byref(m), link.ctypes.data, geom.ctypes.data, dirs.ctypes.data)
    return {"n_c": nc, "link": link, "geom": geom, "normal": dirs[0:3], "t1": dirs[3:6], "t2": dirs[6:9]}


def contact_shapes(m: _model.Model, n: int) -> dict:
    """shapes of the outputs of a contact query over n records"""
    nd, nc = m.dof_qd, contact_layout(m)["n_c"]
    return {"contacts": (n, nc, 10), "jac": (n, nc, 3, nd), "rows": (n, 3 * nc, nd), "rhs": (n, 3 * nc),
            "delassus": (n, 3 * nc, 3 * nc), "impulse": (n, 3 * nc), "force": (n, nc, 3), "qd_pre": (n, nd),
            "qd_post": (n, nd)}


def _contact_want(want):
    want = (want,) if isinstance(want, str) else tuple(want)
    for k in want:
        if k not in CONTACT_OUTPUTS:
            raise ValueError(f"unknown contact output {k!r} (one of {CONTACT_OUTPUTS})")
    return want


class Param(C.Structure):
    """tds_param_t (include/tds_hip.h): one selected model scalar"""
    _fields_ = [("kind", C.c_int32), ("link", C.c_int32), ("comp", C.c_int32), ("pad_", C.c_int32)]


# parameter kinds (TDS_PARAM_*): name -> (code, on a link, number of components)
PARAM_KINDS = {
    "mass": (0, True, 1), "com": (1, True, 3), "inertia": (2, True, 6), "xt_trans": (3, True, 3),
    "stiffness": (4, True, 1), "damping": (5, True, 1), "base_mass": (6, False, 1), "base_com": (7, False, 3),
    "base_inertia": (8, False, 6), "gravity": (9, False, 3), "friction": (10, False, 1), "restitution": (11, False, 1),
}
# the contact model's kinds, in a table of their own (all_params lists PARAM_KINDS only): name -> (code, on a GEOM,
# number of components).  The index of the geom kinds is the geom's, not a link's.
CONTACT_PARAM_KINDS = {
    "cfm": (16, False, 1), "erp": (17, False, 1), "geom_radius": (18, True, 1), "geom_length": (19, True, 1),
    "geom_extent": (20, True, 3), "geom_trans": (21, True, 3),
}
GEOM_SPHERE, GEOM_CAPSULE, GEOM_BOX = 0, 2, 4  # TDS_GEOM_*: the shapes that give contact points


def param_spec(params):
    """a parameter selection as a tds_param_t array: entries are tds_param_t, or tuples (kind name, link[, comp]) for
    the link kinds and (kind name[, comp]) for the others, e.g. ("mass", 3), ("com", 3, 2), ("gravity", 2),
    ("friction",).  Inertia comps 0..5 = xx, yy, zz, xy, xz, yz.  The contact model's kinds (CONTACT_PARAM_KINDS):
    ("cfm",), ("erp",), and with a GEOM index ("geom_radius", g), ("geom_length", g), ("geom_extent", g, comp),
    ("geom_trans", g, comp).  The library checks ranges, shapes and duplicates."""
    if isinstance(params, C.Array) and params._type_ is Param:
        return params
    out = (Param * max(len(params), 1))()
    for j, q in enumerate(params):
        if isinstance(q, Param):
            out[j] = q
            continue
        name, rest = q[0], list(q[1:])
        if name not in PARAM_KINDS and name not in CONTACT_PARAM_KINDS:
            raise ValueError(f"unknown parameter kind {name!r} (one of {', '.join([*PARAM_KINDS, *CONTACT_PARAM_KINDS])})")
        code, on_link, nc = PARAM_KINDS[name] if name in PARAM_KINDS else CONTACT_PARAM_KINDS[name]
        if on_link and not rest:
            raise ValueError(f"parameter {q!r}: kind {name!r} needs a {'link' if name in PARAM_KINDS else 'geom'} index")
        link = rest.pop(0) if on_link else 0
        comp = rest.pop(0) if rest else 0
        if rest:
            raise ValueError(f"parameter {q!r}: too many indices")
        out[j] = Param(code, int(link), int(comp), 0)
    return out


def all_params(m: _model.Model):
    """every selectable parameter of a model: per link mass, com, inertia, xt_trans, stiffness, damping; the base's
    (floating base); gravity, friction, restitution"""
    sel = []
    for name, (_, on_link, nc) in PARAM_KINDS.items():
        if name.startswith("base_") and not m.is_floating:
            continue
        for link in (range(m.num_links) if on_link else [None]):
            for c in range(nc):
                sel.append((name,) + ((link,) if on_link else ()) + ((c,) if nc > 1 else ()))
    return sel


def contact_params(m: _model.Model):
    """every selectable parameter of a model's contact model: cfm, erp, and per collision shape (sphere, capsule, box)
    its radius, a capsule's length, a box's extents, and the translation of its frame"""
    sel = [("cfm",), ("erp",)]
    for g in range(m.num_geoms):
        t = m.geoms[g].type
        if t not in (GEOM_SPHERE, GEOM_CAPSULE, GEOM_BOX):
            continue
        sel.append(("geom_radius", g))
        if t == GEOM_CAPSULE:
            sel.append(("geom_length", g))
        if t == GEOM_BOX:
            sel += [("geom_extent", g, c) for c in range(3)]
        sel += [("geom_trans", g, c) for c in range(3)]
    return sel


class Rings(C.Structure):
    """tds_hip_rings_t (include/tds_hip.h): per-step record rings of tds_hip_step_many_rings"""
    _fields_ = [("obs_ring", C.c_void_p), ("obs_slots", C.c_int32), ("obs_first", C.c_int32), ("obs_f32", C.c_int32),
                ("y_stride", C.c_int32), ("y_ring", C.c_void_p), ("y_slots", C.c_int32), ("y_first", C.c_int32),
                ("progress", C.c_void_p), ("obs_slot_envs", C.c_int32), ("pad1_", C.c_int32)]


EXPORTED_SYMBOLS = [
    "tds_hip_last_error", "tds_hip_abi_version", "tds_hip_device_count", "tds_hip_model_check",
    "tds_hip_create", "tds_hip_destroy", "tds_hip_set_stream", "tds_hip_num_envs",
    "tds_hip_input_dim", "tds_hip_output_dim", "tds_hip_dtype", "tds_hip_x_device",
    "tds_hip_y_device", "tds_hip_set_inputs", "tds_hip_get_inputs", "tds_hip_get_outputs",
    "tds_hip_forward_zero_device", "tds_hip_step", "tds_hip_step_obs", "tds_hip_obs_dim",
    "tds_hip_set_auto_reset", "tds_hip_reset", "tds_hip_rollout", "tds_hip_rollout_ex",
    "tds_hip_set_policy_network", "tds_hip_policy_num_parameters",
    "tds_hip_forward_zero_host", "tds_hip_send_local", "tds_hip_forward_zero_fetch",
    "tds_hip_set_timing", "tds_hip_last_kernel_ms", "tds_hip_kernel_info", "tds_hip_profile_phases",
    "tds_hip_device", "tds_hip_record_bytes", "tds_hip_sync", "tds_hip_forward_zero_host_begin",
    "tds_hip_forward_zero_host_end", "tds_hip_step_many_prepare", "tds_hip_step_many",
    "tds_hip_set_graph_chains", "tds_hip_step_many_tune", "tds_hip_step_many_is_loop", "tds_hip_debug_poison_lds",
    "tds_hip_step_many_rings", "tds_hip_step_many_rings_prepare", "tds_hip_step_many_rings_blocks",
    "tds_hip_default_option", "tds_hip_set_option", "tds_hip_get_option", "tds_hip_option_count", "tds_hip_option_name",
    "tds_hip_profile_zones", "tds_hip_step_host", "tds_hip_reset_host", "tds_hip_set_states", "tds_hip_device_alloc", "tds_hip_device_free",
    "tds_hip_device_upload", "tds_hip_device_download",
    "tds_hip_shard_rccl_version", "tds_hip_shard_unique_id", "tds_hip_shard_create", "tds_hip_shard_create_all",
    "tds_hip_shard_destroy", "tds_hip_shard_sim", "tds_hip_shard_rank", "tds_hip_shard_world",
    "tds_hip_shard_local_envs", "tds_hip_shard_first_env", "tds_hip_shard_wire_bytes", "tds_hip_shard_set_block",
    "tds_hip_shard_step", "tds_hip_shard_step_many", "tds_hip_shard_step_many_prepare", "tds_hip_shard_group_step", "tds_hip_shard_flush", "tds_hip_shard_gathered", "tds_hip_shard_gathered_step",
    "tds_hip_shard_ring_plan", "tds_hip_shard_gathered_offset", "tds_hip_shard_exchange_form", "tds_hip_shard_peer_count",
    "tds_hip_single_step_kernel", "tds_hip_launch_plan_host", "tds_hip_oct_window_plan_host", "tds_hip_oct_sweep_na_plan_host",
    "tds_hip_jvp", "tds_hip_jacobian", "tds_hip_jacobian_host", "tds_hip_jacobian_tangents",
    "tds_hip_vjp", "tds_hip_vjp_host", "tds_hip_vjp_host_tape",
    "tds_hip_params_get", "tds_hip_params_apply", "tds_hip_set_model_variants", "tds_hip_model_variants",
    "tds_hip_model_variants_host", "tds_hip_jvp_params", "tds_hip_vjp_params", "tds_hip_jvp_params_host",
    "tds_hip_vjp_params_host", "tds_hip_trajectory_jvp", "tds_hip_trajectory_jvp_host",
    "tds_hip_trajectory_vjp", "tds_hip_trajectory_vjp_host",
    "tds_hip_policy_trajectory_vjp", "tds_hip_policy_trajectory_vjp_host",
    "tds_hip_dynamics", "tds_hip_inverse_dynamics", "tds_hip_point_jacobian",
    "tds_hip_dynamics_host", "tds_hip_inverse_dynamics_host", "tds_hip_point_jacobian_host",
    "tds_hip_ik_default_options", "tds_hip_inverse_kinematics", "tds_hip_inverse_kinematics_host",
    "tds_hip_lqr_backward", "tds_hip_lqr_backward_host", "tds_hip_feedback_rollout", "tds_hip_feedback_rollout_host",
    "tds_hip_lqr_backward_box", "tds_hip_lqr_backward_box_host", "tds_hip_feedback_rollout_box",
    "tds_hip_feedback_rollout_box_host", "tds_hip_lm_step", "tds_hip_lm_step_host",
    "tds_hip_contacts", "tds_hip_contacts_host", "tds_hip_contact_layout",
    "tds_hip_contacts_jvp", "tds_hip_contacts_jvp_host", "tds_hip_contacts_jvp_tangents",
    "tds_hip_dynamics_jvp", "tds_hip_inverse_dynamics_jvp", "tds_hip_dynamics_jvp_host",
    "tds_hip_inverse_dynamics_jvp_host", "tds_hip_dynamics_jvp_tangents",
    "tds_rb_last_error", "tds_rb_create", "tds_rb_destroy", "tds_rb_set_stream", "tds_rb_state_device",
    "tds_rb_set_state", "tds_rb_get_state", "tds_rb_step", "tds_rb_jvp", "tds_rb_jvp_host", "tds_rb_params_get",
    "tds_rb_vjp", "tds_rb_vjp_host", "tds_rb_vjp_plan",
]


def lib_has_symbol(name: str) -> bool:
    """whether libtds_hip.so exports `name` (e.g. the entry point of an experiment slot, tools/build_alt.sh)"""
    return hasattr(lib(), name)


def shard_ring_plan(chunks_done: int, n_steps: int, act_first: int = 0, act_blocks: int = 1, n_blocks: int = 1):
    """the step-loop launches a tds_hip_shard_step_many call is cut into (tds_hip_shard_ring_plan; no device needed):
    list of dicts half / steps / step0 / act_first / slot0 / first_wait"""
    cap = 80
    out = (C.c_int * (6 * cap))()
    n = lib().tds_hip_shard_ring_plan(int(chunks_done), int(n_steps), int(act_first), int(act_blocks), int(n_blocks), out, cap)
    if n < 0:
        raise TdsHipError("tds_hip_shard_ring_plan: bad arguments")
    keys = ("half", "steps", "step0", "act_first", "slot0", "first_wait")
    return [dict(zip(keys, out[6 * i:6 * i + 6])) for i in range(n)]


PLAN_KERNELS = {0: "general", 1: "quad16", 2: "oct8", 3: "chain8"}
_PLAN_REQ = ("n", "env_total", "nsub", "reset_mode", "rollout", "rings", "progress", "peers", "pool_states", "pool_pass",
             "prof", "auto_reset")
_PLAN_OUT = ("kernel", "kind", "build", "gen_build", "layout", "envs_per_wg", "threads_per_wg", "blocks", "refused", "loop",
             "env_range", "exchange_after")


def launch_plan_host(m: _model.Model, dtype: str = "f64", num_envs: int = 1, num_cus: int = 256, lds_per_cu: int = 160 * 1024,
                     **req):
    """which kernel and build a launch takes (tds_hip_launch_plan_host; no device needed): the plan of a handle of
    `num_envs` environments on a device of `num_cus` compute units with `lds_per_cu` bytes of LDS each, under the process's
    default options.  req: n (default num_envs), env_total, nsub (1), reset_mode, rollout, rings, progress, peers,
    pool_states, pool_pass, prof, auto_reset.  Returns a dict of the plan; "kernel" is named as in single_step_kernel()."""
    unknown = set(req) - set(_PLAN_REQ)
    if unknown:
        raise TypeError(f"launch_plan_host: unknown request fields {sorted(unknown)}")
    vals = dict(n=num_envs, nsub=1)
    vals.update(req)
    r = (C.c_int * len(_PLAN_REQ))(*[int(vals.get(k, 0)) for k in _PLAN_REQ])
    out = (C.c_int * len(_PLAN_OUT))()
    rc = lib().tds_hip_launch_plan_host(C.byref(m), dtype_code(dtype), int(num_envs), int(num_cus), int(lds_per_cu), r,
                                        len(_PLAN_REQ), out, len(_PLAN_OUT))
    if rc != len(_PLAN_OUT):
        _check(rc)
    plan = dict(zip(_PLAN_OUT, out))
    plan["kernel"] = PLAN_KERNELS[plan["kernel"]]
    for k in ("refused", "loop", "exchange_after"):
        plan[k] = bool(plan[k])
    return plan


def oct_window_plan_host(max_contacts: int, pgs_iterations: int, long_window: int = 1):
    """the window barriers of one step of the 8-lane kernel's two-wavefront builds (tds_hip_oct_window_plan_host; no device
    needed): dict main_barriers / help_barriers / long_window for a wavefront with at most `max_contacts` contacts per
    environment"""
    out = (C.c_int * 3)()
    rc = lib().tds_hip_oct_window_plan_host(int(max_contacts), int(pgs_iterations), int(long_window), out, 3)
    if rc != 3:
        _check(rc)
    return dict(main_barriers=out[0], help_barriers=out[1], long_window=bool(out[2]))


def oct_sweep_na_plan_host(max_contacts: int, pgs_iterations: int, long_window: int = 1, sweep_na: int = 1):
    """the same walk with the main wavefront's first sweep specialised for the contact count where option oct_sweep_na sends it
    there (tds_hip_oct_sweep_na_plan_host; no device needed): dict main_barriers / help_barriers / specialised"""
    out = (C.c_int * 3)()
    lib().tds_hip_oct_sweep_na_plan_host.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int]
    rc = lib().tds_hip_oct_sweep_na_plan_host(int(max_contacts), int(pgs_iterations), int(long_window), int(sweep_na), out, 3)
    if rc != 3:
        _check(rc)
    return dict(main_barriers=out[0], help_barriers=out[1], specialised=bool(out[2]))


def default_option(key: str, value) -> None:
    """process-wide default of a library option for handles created from now on (tds_hip_default_option;
    None: back to "unset" = environment variable TDS_HIP_<KEY>, else the library's own rule)"""
    v = -(1 << 63) if value is None else int(value)
    _check(lib().tds_hip_default_option(key.encode(), v))


def option_names():
    L = lib()
    return [L.tds_hip_option_name(i).decode() for i in range(L.tds_hip_option_count())]


class default_options:
    """``with default_options(w2=0, no_chain=1): sim = HipSim(...)`` — create-time options for the handles made inside"""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        for k, v in self.kv.items():
            default_option(k, v)
        return self

    def __exit__(self, *exc):
        for k in self.kv:
            default_option(k, None)
        return False


def _check(rc):
    if rc != TDS_OK:
        raise TdsHipError(f"tds_hip error {rc}: {lib().tds_hip_last_error().decode()}")


def model_check(m: _model.Model) -> None:
    _check(lib().tds_hip_model_check(C.byref(m)))


# step Jacobians: accumulation methods (the reference's CudaAccumulationMethod)
JAC_ACCUMULATE = {None: 0, "none": 0, "sum": 1, "mean": 2}


def _index_array(idx):
    """None (dense) or a host int32 array of indices, kept alive by the caller"""
    import numpy as np

    if idx is None:
        return None, 0, None
    a = np.ascontiguousarray(np.asarray(idx, dtype=np.int64).reshape(-1).astype(np.int32))
    return a, a.shape[0], C.c_void_p(a.ctypes.data)


def jacobian_host(m: _model.Model, x, rows=None, cols=None, accumulate=None, want_y: bool = False):
    """The step Jacobian on the CPU (tds_hip_jacobian_host; the checker of the device path, needs no GPU).

    x: [N, input_dim] float64.  Returns jac [N, n_rows, n_cols] (accumulate None) or [n_rows, n_cols] ("sum",
    "mean"); with want_y also forward_zero's y [N, output_dim] from the double instantiation of the same template."""
    call = functools.partial(lib().tds_hip_jacobian_host, C.byref(m))
    jac, y = _jacobian(_HostArrays, call, m, x, rows, cols, accumulate, want_y)
    return (jac, y) if want_y else jac


def _host_outputs(shapes, want, out=None, struct=None, dtypes={}):
    """The wanted outputs of a host query: C-contiguous arrays of `shapes` (float64 where `dtypes` names no other),
    those `out` holds and new zeros for the rest; with them `struct` (a ctypes class, optional) filled with their
    addresses"""
    import numpy as np

    res = {}
    for k in want:
        dt = np.dtype(dtypes.get(k, "float64"))
        a = out[k] if out is not None and k in out else np.zeros(shapes[k], dtype=dt)
        assert a.dtype == dt and a.flags.c_contiguous and a.shape == shapes[k], k
        res[k] = a
    return res, struct and struct(**{k: a.ctypes.data for k, a in res.items()})


def _dev_outputs(shapes, want, out, device, struct=None, dtypes={}):
    """The wanted outputs of a device query: contiguous CUDA tensors of `shapes` (float64 where `dtypes` names no
    other), those `out` holds and new ones on `device` for the rest; with them `struct` (a ctypes class, optional)
    filled with their addresses"""
    import torch

    res = {}
    for k in want:
        dt = getattr(torch, dtypes.get(k, "float64"))
        t = out[k] if out is not None and k in out else torch.empty(shapes[k], dtype=dt, device=device)
        assert t.is_cuda and t.dtype == dt and t.is_contiguous() and tuple(t.shape) == shapes[k], k
        res[k] = t
    # (an output without extent, n_c = 0, has no storage: it still counts as asked for)
    nothing = None if all(t.numel() for t in res.values()) else torch.empty(1, dtype=torch.float64, device=device)
    return res, struct and struct(**{k: (t if t.numel() else nothing).data_ptr() for k, t in res.items()})


def _entries(shape):
    n = 1
    for d in shape:
        n *= int(d)
    return n


class _HostArrays:
    """How a call marshals its arguments and results over numpy arrays (the *_host functions); _DevArrays: the same
    over CUDA tensors (HipSim's and RigidBodySim's methods).  A call written on either is written once (_vjp,
    _dynamics_jvp ...).  The host side takes array-likes and refuses with ValueError; the device side demands CUDA
    tensors of the dtype and refuses with AssertionError, or with `error` where a call names another."""

    @staticmethod
    def ptr(a, empty=None):
        return None if a is None else a.ctypes.data

    @staticmethod
    def records(a, width, what):
        import numpy as np

        return np.ascontiguousarray(a, dtype=np.float64).reshape(-1, width)

    @staticmethod
    def rows(a, n, width, what):
        import numpy as np

        if a is None or width == 0:
            return None, None
        a = np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.float64).reshape(-1, width), (n, width)))
        return a, a.ctypes.data

    @staticmethod
    def directions(v, n, width, width_text=None):
        import numpy as np

        v = np.ascontiguousarray(v, dtype=np.float64)
        if v.ndim != 3 or v.shape[0] != n or v.shape[2] != width or v.shape[1] < 1:
            raise ValueError(f"v: expected [{n}, k >= 1, {width}], got {tuple(v.shape)}")
        return v

    @staticmethod
    def tangents(v, n, width, name):
        """v [n, width] (K = 1) or [n, K, width] as (the contiguous [n, K, width] array, whether to squeeze K out of
        the result)"""
        import numpy as np

        v = np.asarray(v, dtype=np.float64)
        squeeze = v.ndim == 2
        v3 = np.ascontiguousarray(v[:, None] if squeeze else v)
        if v3.ndim != 3 or v3.shape[0] != n or v3.shape[2] != width:
            raise ValueError(f"{name}: expected [{n}, K, {width}] or [{n}, {width}], got {tuple(v.shape)}")
        return v3, squeeze

    @staticmethod
    def exact(a, shape, name, dtype="float64", by_count=False, error=ValueError):
        """a as a contiguous array of `shape` (None: any; by_count: anything of that many entries)"""
        import numpy as np

        a = np.ascontiguousarray(a, dtype=dtype)
        if shape is not None and (_entries(a.shape) != _entries(shape) if by_count else a.shape != tuple(shape)):
            raise ValueError(f"{name}: expected {list(shape)}, got {list(a.shape)}")
        return a

    @staticmethod
    def once(a, n, width, name):
        """a [width] (every environment) or [n, width] as a contiguous [n, width] array"""
        import numpy as np

        t = np.asarray(a, dtype=np.float64)
        if t.ndim == 1:
            t = np.broadcast_to(t, (n, t.shape[0]))
        if t.shape != (n, width):
            raise ValueError(f"{name}: expected [{width}] or [{n}, {width}], got {tuple(np.shape(a))}")
        return np.ascontiguousarray(t)

    @staticmethod
    def theta(theta, n, p):
        th = None if theta is None else _HostArrays.once(theta, n, p, "theta")
        return th, None if p == 0 else _HostArrays.ptr(th)

    @staticmethod
    def new(shape, like, dtype="float64", zero=False):
        import numpy as np

        return np.zeros(shape, dtype=dtype)

    @staticmethod
    def outputs(shapes, want, out, like, struct=None, dtypes={}):
        return _host_outputs(shapes, want, out, struct, dtypes)


class _DevArrays:
    @staticmethod
    def ptr(t, empty=None):
        """the address of t; of a tensor without extent NULL, or that of `empty` where the library wants a buffer"""
        if t is not None and t.numel() == 0:
            t = empty
        return None if t is None else C.c_void_p(t.data_ptr())

    @staticmethod
    def records(a, width, what, n=None):
        import torch

        assert a.is_cuda and a.dtype == torch.float64 and a.dim() == 2 and a.shape[1] == width, what
        assert n is None or a.shape[0] == n, what
        return a.contiguous()

    @staticmethod
    def rows(a, n, width, what):
        a = None if a is None or width == 0 else _DevArrays.records(a, width, what, n)
        return a, _DevArrays.ptr(a)

    @staticmethod
    def directions(v, n, width, width_text=None):
        import torch

        assert v.is_cuda and v.dtype == torch.float64 and v.dim() == 3 and v.shape[1] >= 1 and \
            tuple(v.shape[::2]) == (n, width), f"v: expected [N, k >= 1, {width_text or width}]"
        return v.contiguous()

    @staticmethod
    def tangents(v, n, width, name):
        import torch

        squeeze = v.dim() == 2
        v3 = v.unsqueeze(1) if squeeze else v
        assert v3.is_cuda and v3.dtype == torch.float64 and v3.dim() == 3 and tuple(v3.shape[::2]) == (n, width), \
            f"{name}: expected a CUDA float64 tensor [{n}, K, {width}] or [{n}, {width}], got {tuple(v.shape)} {v.dtype}"
        return v3.contiguous(), squeeze

    @staticmethod
    def exact(t, shape, name, dtype="float64", by_count=False, error=AssertionError):
        import torch

        ok = t.is_cuda and t.dtype == getattr(torch, dtype)
        if ok and shape is not None:
            ok = t.numel() == _entries(shape) if by_count else tuple(t.shape) == tuple(shape)
        if not ok:
            raise error(f"{name}: expected a CUDA {dtype} tensor {'of any shape' if shape is None else list(shape)}, "
                        f"got {list(t.shape)} {t.dtype}")
        return t.contiguous()

    @staticmethod
    def once(t, n, width, name):
        import torch

        assert t.is_cuda and t.dtype == torch.float64, name
        if t.dim() == 1:
            t = t.unsqueeze(0).expand(n, -1)
        assert tuple(t.shape) == (n, width), (name, tuple(t.shape), n, width)
        return t.contiguous()

    @staticmethod
    def theta(theta, n, p):
        th = None if theta is None or p == 0 else _DevArrays.once(theta, n, p, "theta")
        return th, _DevArrays.ptr(th)

    @staticmethod
    def new(shape, like, dtype="float64", zero=False):
        import torch

        return (torch.zeros if zero else torch.empty)(shape, dtype=getattr(torch, dtype), device=like.device)

    @staticmethod
    def outputs(shapes, want, out, like, struct=None, dtypes={}):
        return _dev_outputs(shapes, want, out, like.device, struct, dtypes)


def _tape(A, tape, shape, like):
    """(lens, the two trailing arguments) of a host call that takes tape = (tape_cap, tape_len): lens int32 of `shape`
    where tape_len asks for the recorded entries; tape None (the device calls): no such arguments"""
    if tape is None:
        return None, ()
    lens = A.new(shape, like, "int32") if tape[1] else None
    return lens, (int(tape[0]), A.ptr(lens))


def _jacobian(A, call, m, x, rows, cols, accumulate, want_y, y=None, want_jac=True):
    """(jac, y) of tds_hip_jacobian[_host]; y: a buffer to write forward_zero's output into (None with want_y: a new
    one); want_jac False: the step alone"""
    x = A.records(x, m.input_dim, "x")
    n = x.shape[0]
    ra, nr, rp = _index_array(rows)
    ca, nc, cp = _index_array(cols)
    nr = nr if rows is not None else m.output_dim
    nc = nc if cols is not None else m.input_dim
    acc = JAC_ACCUMULATE[accumulate]
    jac = A.new((n, nr, nc) if acc == 0 else (nr, nc), x) if want_jac else None
    y = A.outputs({"y": (n, m.output_dim)}, ("y",) if want_y else (), None if y is None else {"y": y}, x)[0].get("y")
    _check(call(n, A.ptr(x), nr if want_jac else 0, rp, nc if want_jac else 0, cp, acc, A.ptr(y), A.ptr(jac)))
    return jac, y


def _vjp(A, call, m, x, w, want_y, y=None, params=None, theta=None, tape=None):
    """(y, wj, lens) of the step VJPs: tds_hip_vjp[_host_tape], and with a selection `params` (theta [p] or [N, p])
    tds_hip_vjp_params[_host], wj then over [x | theta]"""
    x = A.records(x, m.input_dim, "x")
    n, p = x.shape[0], 0 if params is None else len(params)
    w3, squeeze = A.tangents(w, n, m.output_dim, "w")
    k = w3.shape[1]
    th = None if params is None else A.once(theta, n, p, "theta")
    y = A.outputs({"y": (n, m.output_dim)}, ("y",) if want_y else (), None if y is None else {"y": y}, x)[0].get("y")
    wj = A.new((n, k, m.input_dim + p), x)
    lens, extra = _tape(A, tape, (n,), x)
    selection = () if params is None else (p, param_spec(params), A.ptr(th))
    _check(call(n, A.ptr(x), *selection, k, A.ptr(w3), A.ptr(y), A.ptr(wj), *extra))
    return y, (wj[:, 0] if squeeze else wj), lens


def _jvp_params(A, call, m, x, theta, params, v):
    """(y, jv) of tds_hip_jvp_params[_host]; v None: jv None"""
    x = A.records(x, m.input_dim, "x")
    n, p = x.shape[0], len(params)
    sel = param_spec(params)
    th = A.once(theta, n, p, "theta")
    y = A.new((n, m.output_dim), x)
    k, v3, jv, squeeze = 0, None, None, False
    if v is not None:
        v3, squeeze = A.tangents(v, n, m.input_dim + p, "v")
        k = v3.shape[1]
        jv = A.new((n, k, m.output_dim), x)
    _check(call(n, A.ptr(x), p, sel, A.ptr(th), k, A.ptr(v3), A.ptr(y), A.ptr(jv)))
    return y, (jv[:, 0] if squeeze else jv)


def _trajectory_inputs(A, m, x0, steps, every, u, params, theta):
    """what the trajectory calls share in front: (x0, n, p, (nsd, n_act, n_rec), u, selection, theta, its pointer, s)"""
    x0 = A.records(x0, m.input_dim, "x0")
    n, p = x0.shape[0], len(params)
    dims = trajectory_dims(m, steps, every)
    sel = param_spec(params)
    th, thp = A.theta(theta, n, p)
    u = None if u is None else A.exact(u, (n, max(int(steps) - 1, 0), dims[1]), "u")
    s = A.new((n, max(dims[2], 1), dims[0]), x0)
    return x0, n, p, dims, u, sel, th, thp, s


def _trajectory_jvp(A, call, m, x0, v, steps, every, u, params, theta):
    """(s, js) of tds_hip_trajectory_jvp[_host]; v None: js None"""
    x0, n, p, (nsd, n_act, n_rec), u, sel, th, thp, s = _trajectory_inputs(A, m, x0, steps, every, u, params, theta)
    k, v3, js, squeeze = 0, None, None, False
    if v is not None:
        v3, squeeze = A.tangents(v, n, m.input_dim + p, "v")
        k = v3.shape[1]
        js = A.new((n, k, max(n_rec, 1), nsd), x0)
    _check(call(n, int(steps), int(every), A.ptr(x0), A.ptr(u), p, sel, thp, k, A.ptr(v3), A.ptr(s), A.ptr(js)))
    return s, (js[:, 0] if squeeze else js)


def _trajectory_vjp(A, call, m, x0, gs, steps, every, u, params, theta, tape=None):
    """(s, gx0, gu, gtheta, lens) of tds_hip_trajectory_vjp[_host]"""
    x0, n, p, (nsd, n_act, n_rec), u, sel, th, thp, s = _trajectory_inputs(A, m, x0, steps, every, u, params, theta)
    gs = A.exact(gs, (n, n_rec, nsd) if n_rec > 0 else None, "gs")  # (a bad steps / every is the library's to refuse)
    gx0 = A.new((n, m.input_dim), x0)
    gu = A.new((n, max(int(steps) - 1, 0), max(n_act, 0)), x0, zero=True)
    gth = A.new((n, p), x0)
    lens, extra = _tape(A, tape, (n, max(int(steps), 1)), x0)
    # (the library wants a buffer behind every output: one without extent gets s's address)
    _check(call(n, int(steps), int(every), A.ptr(x0), A.ptr(u), p, sel, thp, A.ptr(gs), A.ptr(s), A.ptr(gx0),
                A.ptr(gu, s), A.ptr(gth, s), *extra))
    return s, gx0, gu, gth, lens


def _policy_trajectory_vjp(A, call, m, x0, policy, gs, steps, every, ga, network, params, theta, first_obs_raw, obs_raw,
                           tape=None):
    """(s, u, gpolicy, gx0, gtheta, lens) of tds_hip_policy_trajectory_vjp[_host]; network: (layer_sizes, activations,
    use_bias); gs and ga both None: the primal alone, the gradients None"""
    x0, n, p, (nsd, n_act, n_rec), _, sel, th, thp, s = _trajectory_inputs(A, m, x0, steps, every, None, params, theta)
    nl, ls, act, ub, P = policy_network_spec(m, *network)
    policy = A.once(policy, n, P, "policy")
    T = max(int(steps), 0)
    gs = None if gs is None else A.exact(gs, (n, n_rec, nsd) if n_rec > 0 else None, "gs")
    ga = None if ga is None else A.exact(ga, (n, T, n_act) if T > 0 else None, "ga")
    grad = gs is not None or ga is not None
    # (a model without actions is refused by the library, not here: u and gtheta have an entry at least, and an
    # argument without extent, the policy of such a model, gets s's address)
    u = A.new((n, max(T, 1), max(n_act, 1)), x0)
    gpol, gx0, gth = (A.new(shape, x0) for shape in ((n, P), (n, m.input_dim), (n, max(p, 1)))) if grad else (None,) * 3
    lens, extra = _tape(A, tape, (n, max(T, 1)), x0)
    flags = (1 if first_obs_raw else 0) | (2 if obs_raw else 0)
    host = _HostArrays.ptr  # (the network's int32 arrays live on the host for either call)
    ptrs = [A.ptr(t, s) for t in (gs, ga, s, u, gpol, gx0, gth)]
    _check(call(n, int(steps), int(every), flags, A.ptr(x0, s), A.ptr(policy, s), nl, host(ls), host(act), host(ub), p,
                sel, thp, *ptrs, *extra))
    return s, u[:, :T, :max(n_act, 0)], gpol, gx0, (gth[:, :p] if grad else None), lens


def _rb_jvp(A, call, m, s0, steps, v, params, theta):
    """(s_T, jv) of tds_rb_jvp[_host]; v None: jv None"""
    nb, nc = m.num_bodies, _model.TDS_RB_STATE
    s0 = A.exact(s0, None, "s0").reshape(-1, nb, nc)
    n, p = s0.shape[0], len(params)
    sel = param_spec(params)
    th, thp = A.theta(theta, n, p)
    sT = A.new(tuple(s0.shape), s0)
    k, v3, jv, squeeze = 0, None, None, False
    if v is not None:
        v3, squeeze = A.tangents(v, n, nb * nc + p, "v")
        k = v3.shape[1]
        jv = A.new((n, k, nb, nc), s0)
    _rb_check(call(n, int(steps), A.ptr(s0), p, sel, thp, k, A.ptr(v3), A.ptr(sT), A.ptr(jv)))
    return sT, (jv[:, 0] if squeeze else jv)


def _rb_vjp(A, call, m, s0, steps, gs, params, theta, every, *budget):
    """(s, gs0, gtheta) of tds_rb_vjp[_host]; budget: tape_cap, and on the device work_bytes"""
    nb, nc = m.num_bodies, _model.TDS_RB_STATE
    s0 = A.exact(s0, None, "s0").reshape(-1, nb, nc)
    n, p = s0.shape[0], len(params)
    every = int(steps) if every is None else int(every)  # (None: the final state alone)
    n_rec = int(steps) // every if every >= 1 and steps >= 1 else 1
    gs = A.exact(gs, (n, n_rec, nb * nc), "gs", by_count=True)
    sel = param_spec(params)
    th, thp = A.theta(theta, n, p)
    s, gs0, gth = A.new((n, n_rec, nb, nc), s0), A.new(tuple(s0.shape), s0), A.new((n, p), s0)
    _rb_check(call(n, int(steps), every, A.ptr(s0), p, sel, thp, A.ptr(gs), A.ptr(s), A.ptr(gs0), A.ptr(gth),
                   *(int(b) for b in budget)))
    return s, gs0, gth


def _dynamics(A, call, m, q, qd, tau, want, out):
    want = _dyn_want(want)
    q = A.records(q, m.dof_q, "q")
    n = q.shape[0]
    qd, qdp = A.rows(qd, n, m.dof_qd, "qd")
    tau, taup = A.rows(tau, n, dyn_tau_dim(m), "tau")
    res, o = A.outputs(dyn_shapes(m, n), want, out, q, DynOut)
    _check(call(n, A.ptr(q), qdp, taup, C.byref(o)))
    return res


def _inverse_dynamics(A, call, m, q, qd, qdd):
    q = A.records(q, m.dof_q, "q")
    n = q.shape[0]
    qd, qdp = A.rows(qd, n, m.dof_qd, "qd")
    qdd, qddp = A.rows(qdd, n, m.dof_qd, "qdd")
    res, _ = A.outputs({"tau": (n, m.dof_qd)}, ("tau",), None, q)
    _check(call(n, A.ptr(q), qdp, qddp, A.ptr(res["tau"])))
    return res["tau"]


def _point_jacobian(A, call, m, q, link, point, local):
    q = A.records(q, m.dof_q, "q")
    n = q.shape[0]
    point, ptp = A.rows(point, n, 3, "point")
    res, _ = A.outputs({"jac": (n, 3, m.dof_qd)}, ("jac",), None, q)
    _check(call(n, A.ptr(q), int(link), ptp, int(bool(local)), A.ptr(res["jac"])))
    return res["jac"]


def _query_jvp(A, call, like, width, params, theta, v, want_primal, want, shapes, struct, out=None, out_primal=None,
               width_text=None):
    """What the derivative calls of the queries share behind their records (`like`: the first of them).  call(p,
    selection, theta, k, v, primal, tangents) is the library's entry point with the records bound; width: the columns of
    v before theta; shapes: the primal outputs', the tangents' are [n, k, ...] of them; struct: the ctypes class of the
    output pointers (None: the one output is passed and returned bare).  A dict handed in is checked even where it is
    not written."""
    n, p = like.shape[0], len(params)
    sel = param_spec(params)
    th, thp = A.theta(theta, n, p)

    def made(shapes, wanted, given):  # (the outputs, their C argument)
        res, s = A.outputs(shapes, want if wanted or given is not None else (), given, like, struct)
        if struct is not None:
            return res, C.byref(s)
        one = next(iter(res.values()), None)
        return one, A.ptr(one)

    primal, po = made(shapes, want_primal or v is None, out_primal)
    if v is None:
        _check(call(p, sel, thp, 0, None, po, None))
        return primal
    v = A.directions(v, n, width + p, width_text)
    k = v.shape[1]
    tan, to = made({name: (n, k) + s[1:] for name, s in shapes.items()}, True, out)
    _check(call(p, sel, thp, k, A.ptr(v), po if want_primal else None, to))
    return (tan, primal) if want_primal else tan


def _dynamics_jvp(A, fn, m, q, qd, tau, v, want, params, theta, want_primal, out, out_primal):
    want = _dyn_want(want)
    q = A.records(q, m.dof_q, "q")
    n = q.shape[0]
    qd, qdp = A.rows(qd, n, m.dof_qd, "qd")
    tau, taup = A.rows(tau, n, dyn_tau_dim(m), "tau")
    return _query_jvp(A, functools.partial(fn, n, A.ptr(q), qdp, taup), q, dyn_input_dim(m), params, theta, v,
                      want_primal, want, dyn_shapes(m, n), DynOut, out, out_primal)


def _inverse_dynamics_jvp(A, fn, m, q, qd, qdd, v, params, theta, want_primal):
    q = A.records(q, m.dof_q, "q")
    n, nd = q.shape[0], m.dof_qd
    qd, qdp = A.rows(qd, n, nd, "qd")
    qdd, qddp = A.rows(qdd, n, nd, "qdd")
    return _query_jvp(A, functools.partial(fn, n, A.ptr(q), qdp, qddp), q, dyn_input_dim(m, True), params, theta, v,
                      want_primal, ("tau",), {"tau": (n, nd)}, None)


def _contacts_jvp(A, fn, m, x, v, want, params, theta, want_primal, out, out_primal):
    want = _contact_want(want)
    x = A.records(x, m.input_dim, "x")
    n = x.shape[0]
    return _query_jvp(A, functools.partial(fn, n, A.ptr(x)), x, m.input_dim, params, theta, v, want_primal, want,
                      contact_shapes(m, n), ContactOut, out, out_primal, "input_dim + p")


def _identity_directions(n, nall, cols, device):
    """v [n, n_cols, nall]: direction j is the unit vector of column cols[j] (None: every column)"""
    import torch

    cols = torch.arange(nall, device=device) if cols is None else torch.as_tensor(cols, device=device).long()
    v = torch.zeros((n, cols.numel(), nall), dtype=torch.float64, device=device)
    v[:, torch.arange(cols.numel(), device=device), cols] = 1.0
    return v


def dynamics_host(m: _model.Model, q, qd=None, tau=None, want=DYN_OUTPUTS):
    """The dynamics queries on the CPU (tds_hip_dynamics_host; the checker of HipSim.dynamics, needs no GPU).

    q [N, dof_q], qd [N, dof_qd] (None: zero), tau [N, dyn_tau_dim(m)] (None: zero), float64.  Returns a dict of the
    wanted outputs: x_world [N, num_links, 12], mass_matrix [N, dof_qd, dof_qd], bias [N, dof_qd], qdd [N, dof_qd]."""
    call = functools.partial(lib().tds_hip_dynamics_host, C.byref(m))
    return _dynamics(_HostArrays, call, m, q, qd, tau, want, None)


def inverse_dynamics_host(m: _model.Model, q, qd=None, qdd=None):
    """tau [N, dof_qd] = ID(q, qd, qdd) on the CPU (tds_hip_inverse_dynamics_host; None: zero); fixed base only"""
    call = functools.partial(lib().tds_hip_inverse_dynamics_host, C.byref(m))
    return _inverse_dynamics(_HostArrays, call, m, q, qd, qdd)


def point_jacobian_host(m: _model.Model, q, link: int, point, local: bool = False):
    """The world-frame Jacobian [N, 3, dof_qd] of a point [N, 3] (or [3]) on link `link` (-1: the base) on the CPU
    (tds_hip_point_jacobian_host); local: the point is given in the link's own frame"""
    call = functools.partial(lib().tds_hip_point_jacobian_host, C.byref(m))
    return _point_jacobian(_HostArrays, call, m, q, link, point, local)


def contacts_host(m: _model.Model, x, want=CONTACT_OUTPUTS, out=None):
    """The contact query on the CPU (tds_hip_contacts_host; the checker of HipSim.contacts, needs no GPU).

    x [N, input_dim] float64: the records of step_host.  Returns a dict of the wanted CONTACT_OUTPUTS (shapes:
    contact_shapes).  out: a dict of arrays to write into.  An environment whose M is not positive definite has NaN in
    rows .. qd_post; the call then raises after writing (pass `out` to see what it wrote)."""
    import numpy as np

    want = _contact_want(want)
    x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, m.input_dim)
    n = x.shape[0]
    res, o = _host_outputs(contact_shapes(m, n), want, out, struct=ContactOut)
    _check(lib().tds_hip_contacts_host(C.byref(m), n, x.ctypes.data, C.byref(o)))
    return res


def contacts_jvp_tangents(m: _model.Model) -> int:
    """K: the directions a work item of HipSim.contacts_jvp carries for this model (tds_hip_contacts_jvp_tangents)"""
    k = lib().tds_hip_contacts_jvp_tangents(C.byref(m))
    if k < 0:
        _check(-k)
    return k


def contact_tangent_shapes(m: _model.Model, n: int, k: int) -> dict:
    """shapes of the tangents of a contact query over n records and k directions: [n, k, *output shape]"""
    return {name: (n, k) + s[1:] for name, s in contact_shapes(m, n).items()}


def contacts_jvp_host(m: _model.Model, x, v, want=CONTACT_OUTPUTS, params=(), theta=None, want_primal: bool = False,
                      out=None, out_primal=None):
    """Forward-mode derivatives of the contact query in [x | theta] on the CPU (tds_hip_contacts_jvp_host; the checker
    of HipSim.contacts_jvp, needs no GPU).

    x [N, input_dim]; v [N, k, input_dim + p]: directions over the record and the selection `params` (param_spec; the
    contact kinds included); theta [p] or [N, p]: the selection's values (None: the model's).  Returns a dict of the
    wanted outputs' tangents [N, k, *shape] (contact_tangent_shapes), with want_primal (tangents, primal): the outputs
    themselves at theta as well.  v None: the primal dict alone (k = 0).  An environment whose M is not positive
    definite has NaN in rows .. qd_post and their tangents; the call then raises after writing (pass out / out_primal,
    dicts of arrays to write the tangents / the primal into, to see what it wrote)."""
    call = functools.partial(lib().tds_hip_contacts_jvp_host, C.byref(m))
    return _contacts_jvp(_HostArrays, call, m, x, v, want, params, theta, want_primal, out, out_primal)


def dynamics_jvp_tangents(m: _model.Model) -> int:
    """K: the directions a work item of HipSim.dynamics_jvp / inverse_dynamics_jvp carries for this model
    (tds_hip_dynamics_jvp_tangents)"""
    k = lib().tds_hip_dynamics_jvp_tangents(C.byref(m))
    if k < 0:
        _check(-k)
    return k


def dyn_tangent_shapes(m: _model.Model, n: int, k: int) -> dict:
    """shapes of the tangents of a dynamics query over n states and k directions: [n, k, *output shape]"""
    return {name: (n, k) + s[1:] for name, s in dyn_shapes(m, n).items()}


def dyn_input_dim(m: _model.Model, inverse: bool = False) -> int:
    """columns of z without theta: [q | qd | tau] of dynamics_jvp, [q | qd | qdd] of inverse_dynamics_jvp"""
    return m.dof_q + m.dof_qd + (m.dof_qd if inverse else dyn_tau_dim(m))


def dynamics_jvp_host(m: _model.Model, q, qd=None, tau=None, v=None, want=DYN_OUTPUTS, params=(), theta=None,
                      want_primal: bool = False, out=None, out_primal=None):
    """Forward-mode derivatives of the dynamics queries in z = [q | qd | tau | theta] on the CPU
    (tds_hip_dynamics_jvp_host; the checker of HipSim.dynamics_jvp, needs no GPU).

    q [N, dof_q], qd [N, dof_qd], tau [N, dyn_tau_dim(m)] (None: zero in value); v [N, k, dyn_input_dim(m) + p]:
    directions over z, theta the selection `params` (param_spec); theta [p] or [N, p]: the selection's values (None: the
    model's).  Returns a dict of the wanted DYN_OUTPUTS' tangents [N, k, *shape] (dyn_tangent_shapes), with want_primal
    (tangents, primal): the outputs themselves at theta as well.  v None: the primal dict alone (k = 0).  An environment
    whose M is not positive definite has NaN in qdd and its tangents; the call then raises after writing (pass out /
    out_primal, dicts of arrays to write the tangents / the primal into, to see what it wrote)."""
    call = functools.partial(lib().tds_hip_dynamics_jvp_host, C.byref(m))
    return _dynamics_jvp(_HostArrays, call, m, q, qd, tau, v, want, params, theta, want_primal, out, out_primal)


def inverse_dynamics_jvp_host(m: _model.Model, q, qd=None, qdd=None, v=None, params=(), theta=None,
                              want_primal: bool = False):
    """Forward-mode derivatives of tau = ID(q, qd, qdd) in z = [q | qd | qdd | theta] on the CPU
    (tds_hip_inverse_dynamics_jvp_host; the checker of HipSim.inverse_dynamics_jvp): dtau [N, k, dof_qd] for
    directions v [N, k, dof_q + 2 dof_qd + p], with want_primal (dtau, tau); v None: tau [N, dof_qd] at theta alone.
    Arguments as for dynamics_jvp_host; fixed base only."""
    call = functools.partial(lib().tds_hip_inverse_dynamics_jvp_host, C.byref(m))
    return _inverse_dynamics_jvp(_HostArrays, call, m, q, qd, qdd, v, params, theta, want_primal)


def inverse_kinematics_host(m: _model.Model, q_init, links, targets, body_points=None, q_reference=None,
                            method="pinv", **options):
    """Batched inverse kinematics on the CPU (tds_hip_inverse_kinematics_host; the checker of
    HipSim.inverse_kinematics, needs no GPU).

    q_init [N, dof_q], links [K] (1 <= K <= 4), targets [N, K, 3] in world coordinates, body_points [K, 3] in the
    links' own frames (None: their origins), q_reference [N, dof_q] or None, method "transpose" / "pinv" / "damped_lm",
    options of IK_OPTIONS.  Returns a dict: q [N, dof_q] float64, iterations [N] and status [N] int32 (IK_FAILED /
    IK_CONVERGED / IK_REACHED), residual [N] float64."""
    import numpy as np

    q_init = _HostArrays.records(q_init, m.dof_q, "q_init")
    n, k = q_init.shape[0], np.size(links)
    targets = np.broadcast_to(np.asarray(targets, dtype=np.float64).reshape((-1, k, 3) if k else (n, 0, 3)), (n, k, 3))
    call = functools.partial(lib().tds_hip_inverse_kinematics_host, C.byref(m))
    return _inverse_kinematics(_HostArrays, call, m, q_init, links, targets, body_points, q_reference, None,
                               ik_options(method, **options))


def _inverse_kinematics(A, call, m, q_init, links, targets, body_points, q_reference, out, options):
    """the dict of tds_hip_inverse_kinematics[_host]'s outputs; out: a dict of buffers to write into, and one that
    leaves iterations, status or residual out has those not computed"""
    q_init = A.records(q_init, m.dof_q, "q_init")
    n = q_init.shape[0]
    k, links, pts, lp, pp = _ik_targets(links, body_points)
    targets = A.exact(targets, (n, k, 3), "targets")
    q_reference, qrp = A.rows(q_reference, n, m.dof_q, "q_reference")
    assert out is None or "q" in out, "out must hold q"
    shapes = _ik_shapes(m, n)
    res, _ = A.outputs(shapes, [name for name in shapes if out is None or name in out], out, q_init, dtypes=_IK_DTYPES)
    _check(call(n, A.ptr(q_init), k, lp, pp, A.ptr(targets), qrp, C.byref(options), A.ptr(res["q"]),
                A.ptr(res.get("iterations")), A.ptr(res.get("status")), A.ptr(res.get("residual"))))
    return res


# -- batched iLQR: the Riccati backward pass and the closed-loop rollout (csrc/tds_lqr.hip) -----------------------
LQR_MAX_NX, LQR_MAX_NU = 40, 16


def _lqr_shapes(A, B):
    """(n, T, nx, nu) from A [n, T, nx, nx] and B [n, T, nx, nu], and the shapes of a backward pass's inputs by name,
    in the order the library takes them"""
    if len(A.shape) != 4 or len(B.shape) != 4 or A.shape[2] != A.shape[3] or tuple(B.shape[:3]) != tuple(A.shape[:3]):
        raise ValueError(f"A: expected [n, T, nx, nx] and B [n, T, nx, nu], got {tuple(A.shape)} and {tuple(B.shape)}")
    n, T, nx, nu = int(A.shape[0]), int(A.shape[1]), int(A.shape[2]), int(B.shape[3])
    return (n, T, nx, nu), {"A": (n, T, nx, nx), "B": (n, T, nx, nu), "lx": (n, T + 1, nx), "lu": (n, T, nu),
                            "lxx": (n, T + 1, nx, nx), "luu": (n, T, nu, nu), "lux": (n, T, nu, nx), "mu": (n,),
                            "dlo": (n, T, nu), "dhi": (n, T, nu)}


def _lqr_backward(X, call, check, A, B, lx, lu, lxx, luu, lux, mu, dlo=None, dhi=None):
    """(k, K, dv, status) of tds_hip_lqr_backward[_host]; with the bounds dlo, dhi the box form `call` then is: its two
    inputs more, and (.., clamped, qp_iterations).  check: dlo <= dhi is verified here (on the device a host wait)"""
    (n, T, nx, nu), shapes = _lqr_shapes(A, B)
    arg = {"A": A, "B": B, "lx": lx, "lu": lu, "lxx": lxx, "luu": luu, "lux": lux, "mu": mu}
    if dlo is not None:
        arg.update(dlo=dlo, dhi=dhi)
    arg = {key: X.exact(a, shapes[key], key, error=ValueError) for key, a in arg.items()}
    if dlo is not None and check:
        _bounds_ordered(arg["dlo"], arg["dhi"], ("dlo", "dhi"))
    out = [X.new((n, T, nu), A), X.new((n, T, nu, nx), A), X.new((n, 2), A), X.new((n,), A, "int32")]
    if dlo is not None:
        out += [X.new((n, T), A, "int32"), X.new((n, T), A, "int32")]
    _check(call(n, T, nx, nu, *(X.ptr(a) for a in arg.values()), *(X.ptr(t) for t in out)))
    return tuple(out)


def lqr_backward_host(A, B, lx, lu, lxx, luu, lux, mu):
    """The backward pass of n time-varying LQ problems on the CPU (tds_hip_lqr_backward_host; the checker of
    HipSim.lqr_backward, needs no GPU).  A [n, T, nx, nx], B [n, T, nx, nu], lx [n, T + 1, nx], lu [n, T, nu],
    lxx [n, T + 1, nx, nx], luu [n, T, nu, nu], lux [n, T, nu, nx], mu [n] (or a scalar).  Returns (k [n, T, nu],
    K [n, T, nu, nx], dv [n, 2], status [n] int32): status t + 1 where the Cholesky of Q_uu + mu I failed at step t
    (that problem's gains and dv are zero), else 0."""
    A, B, mu = _lqr_host_arrays(A, B, mu)
    return _lqr_backward(_HostArrays, lib().tds_hip_lqr_backward_host, True, A, B, lx, lu, lxx, luu, lux, mu)


def _lqr_host_arrays(A, B, mu):
    """what the host forms accept beyond the device's: array-likes, and a scalar mu"""
    import numpy as np

    A, B = np.ascontiguousarray(A, dtype=np.float64), np.ascontiguousarray(B, dtype=np.float64)
    return A, B, np.broadcast_to(np.asarray(mu, dtype=np.float64), A.shape[:1])


def _bounds_ordered(lo, hi, names):
    """ValueError unless lo <= hi in every entry (a NaN fails the comparison); numpy arrays or torch tensors"""
    if not bool((lo <= hi).all()):
        raise ValueError(f"{names[0]} > {names[1]} somewhere, or a NaN bound")


def lqr_backward_box_host(A, B, lx, lu, lxx, luu, lux, mu, dlo, dhi):
    """The backward pass under control limits on the CPU (tds_hip_lqr_backward_box_host; the checker of
    HipSim.lqr_backward_box, needs no GPU).  Arguments as lqr_backward_host, and dlo <= dhi [n, T, nu]: the bounds on
    the step k_t (lo - u_nom, hi - u_nom; +-inf: none).  Per step a box-constrained QP by projected Newton in place of
    the unconstrained solve, feedback gains on the controls it left free (include/tds_hip.h states it).  Returns
    (k, K, dv, status, clamped [n, T] int32 -- bit a set: control a clamped in the QP's final set --, qp_iterations
    [n, T] int32).  Infinite bounds give lqr_backward_host's k, K, dv, status bit for bit."""
    A, B, mu = _lqr_host_arrays(A, B, mu)
    return _lqr_backward(_HostArrays, lib().tds_hip_lqr_backward_box_host, True, A, B, lx, lu, lxx, luu, lux, mu, dlo, dhi)


def _feedback_rollout(X, calls, check_map, check_bounds, m, x0, s_nom, u_nom, k, K, alpha, problem_of_row, u_lo, u_hi):
    """(s, u) of tds_hip_feedback_rollout[_host], and with the limits u_lo, u_hi of its box form: calls = (the plain
    entry point, the box one), each taking (rows, T, P, the pointers).  check_map: the entries of problem_of_row are
    verified here, check_bounds: u_lo <= u_hi is (on the device a host wait each)"""
    nsd, n_act, _ = trajectory_dims(m, 1)
    if len(x0.shape) != 2 or x0.shape[1] != m.input_dim:
        raise ValueError(f"x0: expected [rows, {m.input_dim}], got {list(x0.shape)}")
    if len(s_nom.shape) != 3 or s_nom.shape[1] < 2 or s_nom.shape[2] != nsd:
        raise ValueError(f"s_nom: expected [P, T + 1, {nsd}] with T >= 1, got {list(s_nom.shape)}")
    rows, P, T = int(x0.shape[0]), int(s_nom.shape[0]), int(s_nom.shape[1]) - 1
    if (u_lo is None) != (u_hi is None):
        raise ValueError("u_lo and u_hi are given together or not at all")
    arg = {"x0": (x0, (rows, m.input_dim)), "s_nom": (s_nom, (P, T + 1, nsd)), "u_nom": (u_nom, (P, T, n_act)),
           "k": (k, (P, T, n_act)), "K": (K, (P, T, n_act, nsd)), "alpha": (alpha, (rows,))}
    if u_lo is not None:
        arg.update(u_lo=(u_lo, (P, T, n_act)), u_hi=(u_hi, (P, T, n_act)))
    arg = {key: X.exact(a, shape, key, error=ValueError) for key, (a, shape) in arg.items()}
    if problem_of_row is not None:
        problem_of_row = X.exact(problem_of_row, (rows,), "problem_of_row", "int32", error=ValueError)
        if check_map and not (0 <= int(problem_of_row.min()) and int(problem_of_row.max()) < P):
            raise ValueError(f"problem_of_row: entries outside [0, {P})")
    elif rows != P:
        raise ValueError(f"problem_of_row is None: x0 needs one row per problem ({P}), got {rows}")
    if u_lo is not None and check_bounds:
        _bounds_ordered(arg["u_lo"], arg["u_hi"], ("u_lo", "u_hi"))
    s, u = X.new((rows, T + 1, nsd), x0), X.new((rows, T, n_act), x0)
    inputs = [X.ptr(a) for a in arg.values()]
    _check(calls[u_lo is not None](rows, T, P, *inputs[:6], X.ptr(problem_of_row), *inputs[6:], X.ptr(s), X.ptr(u)))
    return s, u


def feedback_rollout_host(m: _model.Model, x0, s_nom, u_nom, k, K, alpha=1.0, problem_of_row=None, u_lo=None,
                          u_hi=None):
    """The closed-loop rollout on the CPU over step_host (tds_hip_feedback_rollout_host; the checker of
    HipSim.feedback_rollout, needs no GPU).  x0 [rows, input_dim], s_nom [P, T + 1, nsd], u_nom and k [P, T, n_act],
    K [P, T, n_act, nsd], alpha [rows] (or a scalar), problem_of_row [rows] ints in [0, P) or None (row r follows
    problem r: rows == P).  u_t = (u_nom + alpha k) + K (s_t - s_nom), s_{t+1} = the step of [s_t | u_t | the rest of
    x0's record].  u_lo, u_hi [P, T, n_act] (both or neither): u_t is clamped to [u_lo, u_hi] of its problem and step
    (tds_hip_feedback_rollout_box_host); None is the call without limits.  Returns (s [rows, T + 1, nsd],
    u [rows, T, n_act])."""
    import numpy as np

    # (what the host form accepts beyond the device's: array-likes, a scalar alpha, any integers in problem_of_row,
    # whose range the library checks)
    x0, s_nom = np.ascontiguousarray(x0, dtype=np.float64), np.ascontiguousarray(s_nom, dtype=np.float64)
    alpha = np.broadcast_to(np.asarray(alpha, dtype=np.float64), x0.shape[:1])
    if problem_of_row is not None:
        problem_of_row = np.asarray(problem_of_row, dtype=np.int64).reshape(-1).astype(np.int32)
    calls = [functools.partial(f, C.byref(m)) for f in (lib().tds_hip_feedback_rollout_host,
                                                        lib().tds_hip_feedback_rollout_box_host)]
    return _feedback_rollout(_HostArrays, calls, False, True, m, x0, s_nom, u_nom, k, K, alpha, problem_of_row, u_lo, u_hi)


# -- batched system identification: the Levenberg-Marquardt step (csrc/tds_lm.hip) -----------------------------------
LM_MAX_P, LM_MAX_LAMBDA = 16, 8
LM_OUTPUTS = ("cost", "g", "H", "delta", "pred", "clamped", "qp_iterations", "status")


def _lm_step(X, call, check, row_start, s, s_obs, js, lam, w, dlo, dhi):
    """the outputs of tds_hip_lm_step[_host] by name (LM_OUTPUTS; js None, the cost-only mode: cost alone).  check:
    row_start, dlo <= dhi and lam > 0 are verified here (on the device a host wait each)"""
    if len(s.shape) < 2:
        raise ValueError(f"s: expected [rows, m] (or [rows, n_rec, nsd]), got {list(s.shape)}")
    rows, m = int(s.shape[0]), _entries(s.shape[1:])
    row_start = X.exact(row_start, None, "row_start", "int32", error=ValueError)
    n = _entries(row_start.shape) - 1
    if len(row_start.shape) != 1 or n < 1:
        raise ValueError(f"row_start: expected [n + 1] with n >= 1, got {list(row_start.shape)}")
    p = 0 if js is None else int(js.shape[1]) if len(js.shape) >= 3 and js.shape[0] == rows else -1
    if p < 0:
        raise ValueError(f"js: expected [{rows}, p, m] (or [{rows}, p, n_rec, nsd]), got {list(js.shape)}")
    L = 0 if p == 0 or lam is None else int(lam.shape[-1])
    if (dlo is None) != (dhi is None):
        raise ValueError("dlo and dhi are given together or not at all")
    arg = {"s": (s, (rows, m)), "s_obs": (s_obs, (rows, m)), "w": (w, (rows, m)), "js": (js, (rows, p, m)),
           "dlo": (dlo, (n, p)), "dhi": (dhi, (n, p)), "lam": (lam, (n, L))}
    arg = {key: None if a is None or (p == 0 and key in ("js", "dlo", "dhi", "lam")) else
           X.exact(a, shape, key, by_count=key in ("s", "s_obs", "w", "js"), error=ValueError)
           for key, (a, shape) in arg.items()}
    if p > 0 and arg["lam"] is None:
        raise ValueError(f"lam: expected [{n}, n_lambda]")
    if check:
        if not (int(row_start[0]) == 0 and int(row_start[-1]) == rows and bool((row_start[1:] >= row_start[:-1]).all())):
            raise ValueError(f"row_start: not non-decreasing from 0 to rows = {rows}")
        if arg["dlo"] is not None:
            _bounds_ordered(arg["dlo"], arg["dhi"], ("dlo", "dhi"))
        if arg["lam"] is not None and not bool(((arg["lam"] > 0) & (arg["lam"] < float("inf"))).all()):
            raise ValueError("lam: a lambda that is not positive and finite")
    shapes = {"cost": (n,), "g": (n, p), "H": (n, p, p), "delta": (n, L, p), "pred": (n, L), "clamped": (n, L),
              "qp_iterations": (n, L), "status": (n, L)}
    out = {k: X.new(shapes[k], row_start, "int32" if k in LM_OUTPUTS[5:] else "float64")
           for k in (LM_OUTPUTS if p > 0 else LM_OUTPUTS[:1])}
    _check(call(n, rows, m, p, L, X.ptr(row_start), *(X.ptr(a) for a in arg.values()),
                *(X.ptr(out.get(k)) for k in LM_OUTPUTS)))
    return out


def lm_step_host(row_start, s, s_obs, js, lam=None, w=None, dlo=None, dhi=None):
    """One Levenberg-Marquardt step of n least-squares problems on the CPU (tds_hip_lm_step_host; the checker of
    HipSim.lm_step, needs no GPU; include/tds_hip.h states it).  Problem i owns the rows row_start[i] ..
    row_start[i + 1] - 1 (row_start [n + 1] ints); s, s_obs [rows, m] (or [rows, n_rec, nsd]: trajectory_jvp_host's s),
    w the same shape or None (weights 1; an entry of weight 0 is skipped, whatever its observation), js [rows, p, m]
    (trajectory_jvp_host's js for the p unit directions on theta, as it comes), lam [n, n_lambda] > 0, dlo <= dhi [n, p]
    or both None: the bounds on the step.  Returns a dict: cost [n], g [n, p], H [n, p, p], delta [n, n_lambda, p],
    pred [n, n_lambda], and int32 [n, n_lambda]: clamped, qp_iterations, status (0 valid, 1 that candidate's system not
    positive definite, 2 the problem's data not finite).  js None is the cost-only mode: {"cost": [n]}."""
    import numpy as np

    # (what the host form accepts beyond the device's: array-likes; the library itself verifies the arguments)
    row_start = np.asarray(row_start, dtype=np.int64).astype(np.int32)
    f64 = lambda a: None if a is None else np.asarray(a, dtype=np.float64)  # noqa: E731
    return _lm_step(_HostArrays, lib().tds_hip_lm_step_host, False, row_start, f64(s), s_obs, f64(js), f64(lam), w,
                    dlo, dhi)


def trajectory_records(m: _model.Model, x0, s, u):
    """The [N T, input_dim] records of a trajectory, problem-major (what jacobian / jacobian_host linearise): record
    (n, t) = [s[n, t] | u[n, t] | the rest of x0[n]].  x0 [N, input_dim], s [N, T + 1, nsd] (or [N, T, nsd]),
    u [N, T, n_act]; numpy arrays or torch tensors alike."""
    nsd, n_act, _ = trajectory_dims(m, 1)
    N, T = int(u.shape[0]), int(u.shape[1])
    if tuple(x0.shape) != (N, m.input_dim) or tuple(u.shape) != (N, T, n_act) or s.shape[0] != N or \
            s.shape[1] < T or s.shape[2] != nsd:
        raise ValueError(f"trajectory_records: x0 {list(x0.shape)}, s {list(s.shape)}, u {list(u.shape)} do not match "
                         f"[N, {m.input_dim}], [N, T + 1, {nsd}], [N, T, {n_act}]")
    import numpy as np

    if isinstance(x0, np.ndarray):
        rest = np.broadcast_to(x0[:, None, nsd + n_act:], (N, T, m.input_dim - nsd - n_act))
        return np.ascontiguousarray(np.concatenate([s[:, :T], u, rest], axis=2).reshape(N * T, m.input_dim))
    import torch

    rest = x0[:, None, nsd + n_act:].expand(N, T, m.input_dim - nsd - n_act)
    return torch.cat([s[:, :T], u, rest], dim=2).reshape(N * T, m.input_dim).contiguous()


def step_host(m: _model.Model, x):
    """forward_zero through the double instantiation of the step Jacobians' template (CPU)"""
    call = functools.partial(lib().tds_hip_jacobian_host, C.byref(m))
    return _jacobian(_HostArrays, call, m, x, None, None, None, True, want_jac=False)[1]


def vjp_host(m: _model.Model, x, w, want_y: bool = False, tape_cap: int = 0, tape_len: bool = False):
    """The step VJP on the CPU (tds_hip_vjp_host: reverse mode, the checker of the device path, needs no GPU).

    x: [N, input_dim], w: [N, K, output_dim] or [N, output_dim] (K = 1) float64.  Returns wj = w^T J [N, K, input_dim]
    (or [N, input_dim]); with want_y also forward_zero's y [N, output_dim].  tape_cap > 0 replaces the model class's
    tape capacity, and tape_len adds the entries each environment recorded (-1: overflowed) to what is returned
    (tds_hip_vjp_host_tape)."""
    call = functools.partial(lib().tds_hip_vjp_host_tape, C.byref(m))
    y, wj, lens = _vjp(_HostArrays, call, m, x, w, want_y, tape=(tape_cap, tape_len))
    out = (wj,) + ((y,) if want_y else ()) + ((lens,) if tape_len else ())
    return out if len(out) > 1 else out[0]


def params_get(m: _model.Model, params):
    """theta [p]: the model blob's values of a parameter selection (tds_hip_params_get; checks the selection)"""
    import numpy as np

    sel = param_spec(params)
    p = len(params)
    theta = np.zeros(max(p, 1), dtype=np.float64)
    _check(lib().tds_hip_params_get(C.byref(m), p, sel, theta.ctypes.data))
    return theta[:p]


def params_apply(m: _model.Model, params, theta) -> _model.Model:
    """a copy of the model blob with the selected scalars set to theta [p] (tds_hip_params_apply: the inverse of
    params_get, same checks; an off-diagonal inertia comp sets both mirror entries).  The model of a variant."""
    import numpy as np

    sel = param_spec(params)
    p = len(params)
    t = np.ascontiguousarray(np.asarray(theta, dtype=np.float64).reshape(-1))
    if t.shape[0] != p:
        raise ValueError(f"theta: expected [{p}], got {tuple(np.shape(theta))}")
    out = m.copy()
    _check(lib().tds_hip_params_apply(C.byref(m), p, sel, t.ctypes.data if p else None, C.byref(out)))
    return out


def _variant_args(params, theta, env_variant, num_envs):
    """(selection, p, theta [V, p] float64, V, map int32 [num_envs] or None) of a set of model variants; theta may be a
    numpy array or a tensor on any device"""
    import numpy as np

    sel = param_spec(params)
    p = len(params)
    if hasattr(theta, "detach"):
        theta = theta.detach().cpu().numpy()
    t = np.ascontiguousarray(np.asarray(theta, dtype=np.float64))
    if t.ndim != 2 or t.shape[1] != p:
        raise ValueError(f"theta: expected [V, {p}], got {tuple(t.shape)}")
    ev = None
    if env_variant is not None:
        if hasattr(env_variant, "detach"):
            env_variant = env_variant.detach().cpu().numpy()
        ev = np.ascontiguousarray(np.asarray(env_variant).astype(np.int32).reshape(-1))
        if ev.shape[0] != num_envs:
            raise ValueError(f"env_variant: expected [{num_envs}], got {tuple(np.shape(env_variant))}")
    return sel, p, t, t.shape[0], ev


def model_variants_host(m: _model.Model, params, theta, env_variant=None, num_envs: int | None = None, dtype: str = "f64"):
    """the checks of HipSim.set_model_variants on the CPU (tds_hip_model_variants_host; needs no GPU) for a handle of
    num_envs environments (default: one per variant); returns the bytes of the device array of the variants' models"""
    import numpy as np

    n = int(np.shape(theta)[0] if num_envs is None else num_envs)
    sel, p, t, nv, ev = _variant_args(params, theta, env_variant, n)
    nbytes = C.c_int64(0)
    _check(lib().tds_hip_model_variants_host(C.byref(m), dtype_code(dtype), n, nv, p, sel, t.ctypes.data if t.size else None,
                                             None if ev is None else ev.ctypes.data, C.byref(nbytes)))
    return int(nbytes.value)


def jvp_params_host(m: _model.Model, x, theta, params, v=None, want_y: bool = False):
    """Forward mode in [x | theta] on the CPU (tds_hip_jvp_params_host; needs no GPU).

    x [N, input_dim], theta [p] or [N, p] (the selected parameters' values), v [N, K, input_dim + p] or
    [N, input_dim + p] (K = 1).  Returns jv = J v [N, K, output_dim] (or [N, output_dim]), with want_y also y
    [N, output_dim]; v None: y alone."""
    call = functools.partial(lib().tds_hip_jvp_params_host, C.byref(m))
    y, jv = _jvp_params(_HostArrays, call, m, x, theta, params, v)
    return y if v is None else (jv, y) if want_y else jv


def vjp_params_host(m: _model.Model, x, theta, params, w, want_y: bool = False, tape_cap: int = 0,
                    tape_len: bool = False):
    """Reverse mode in [x | theta] on the CPU (tds_hip_vjp_params_host; needs no GPU).

    x [N, input_dim], theta [p] or [N, p], w [N, K, output_dim] or [N, output_dim].  Returns wj = w^T J
    [N, K, input_dim + p] (or [N, input_dim + p]), the x part first; want_y, tape_cap and tape_len as for vjp_host."""
    call = functools.partial(lib().tds_hip_vjp_params_host, C.byref(m))
    y, wj, lens = _vjp(_HostArrays, call, m, x, w, want_y, None, params, theta, (tape_cap, tape_len))
    out = (wj,) + ((y,) if want_y else ()) + ((lens,) if tape_len else ())
    return out if len(out) > 1 else out[0]


def trajectory_dims(m: _model.Model, steps: int, every: int = 1):
    """(nsd, n_act, n_rec) of a trajectory: state entries q | qd, action slots of a step's record, recorded states"""
    nsd = m.dof_q + m.dof_qd
    n_act = m.input_dim - nsd - (3 if m.step_mode == _model.TDS_STEP_LOCOMOTION else 0)
    return nsd, n_act, (int(steps) // int(every) if int(every) > 0 else 0)


def trajectory_jvp_host(m: _model.Model, x0, v=None, steps: int = 1, every: int = 1, u=None, params=(), theta=None):
    """Forward-mode trajectory derivative on the CPU (tds_hip_trajectory_jvp_host; the checker of
    HipSim.trajectory_jvp, needs no GPU).

    x0 [N, input_dim], u None or [N, steps - 1, n_act], theta None (the model's values), [p] or [N, p], v
    [N, K, input_dim + p] (or [N, input_dim + p]: K = 1).  Returns (s, js): s [N, n_rec, nq + nd], js
    [N, K, n_rec, nq + nd] (or [N, n_rec, nq + nd]); v None: js None."""
    call = functools.partial(lib().tds_hip_trajectory_jvp_host, C.byref(m))
    return _trajectory_jvp(_HostArrays, call, m, x0, v, steps, every, u, params, theta)


def trajectory_vjp_host(m: _model.Model, x0, gs, steps: int, every: int = 1, u=None, params=(), theta=None,
                        tape_cap: int = 0, tape_len: bool = False):
    """Reverse-mode trajectory derivative on the CPU (tds_hip_trajectory_vjp_host; the checker of
    HipSim.trajectory_vjp, needs no GPU).

    x0, u, params and theta as for trajectory_jvp_host; gs [N, n_rec, nq + nd], the cotangent on the recorded states.
    Returns (s, gx0, gu, gtheta): s [N, n_rec, nq + nd], gx0 [N, input_dim], gu [N, steps - 1, n_act] (zeros where u is
    None) and gtheta [N, p]; with tape_len also the entries each step recorded [N, steps] (-1: overflowed).  tape_cap
    as for vjp_host."""
    call = functools.partial(lib().tds_hip_trajectory_vjp_host, C.byref(m))
    out = _trajectory_vjp(_HostArrays, call, m, x0, gs, steps, every, u, params, theta, (tape_cap, tape_len))
    return out if tape_len else out[:4]


def policy_network_spec(m: _model.Model, layer_sizes=None, activations=None, use_bias=None):
    """(num_layers, layer_sizes, activations, use_bias, P): a policy network as the C ABI takes it (int32 arrays, kept
    alive by the caller) and its parameter count; layer_sizes None: the default linear policy (num_layers 0).
    activations: one TDS_NN_ACT_* per layer after the input (default: identity); use_bias: one flag per layer, the input
    layer's included (default: every layer but the input)."""
    import numpy as np

    od, ad = m.dof_q + m.dof_qd, m.action_dim
    if layer_sizes is None:
        return 0, None, None, None, ad * od + ad
    ls = np.ascontiguousarray(layer_sizes, dtype=np.int32)
    nl = int(ls.shape[0])
    act = np.full(max(nl - 1, 1), -1, dtype=np.int32) if activations is None else \
        np.ascontiguousarray(activations, dtype=np.int32)
    ub = np.array([0] + [1] * (nl - 1), dtype=np.int32) if use_bias is None else \
        np.ascontiguousarray(use_bias, dtype=np.int32)
    if act.shape[0] < nl - 1 or ub.shape[0] != nl:
        raise ValueError(f"policy network: {nl} layers need {nl - 1} activations and {nl} bias flags")
    nw = int(sum(int(ls[i - 1]) * int(ls[i]) for i in range(1, nl)))
    nb = int(sum(int(ls[i]) for i in range(nl) if ub[i]))
    return nl, ls, act, ub, nw + nb


def policy_trajectory_vjp_host(m: _model.Model, x0, policy, gs, steps: int, every: int = 1, ga=None, layer_sizes=None,
                               activations=None, use_bias=None, params=(), theta=None, first_obs_raw: bool = False,
                               obs_raw: bool = False, tape_cap: int = 0, tape_len: bool = False):
    """Closed-loop policy gradients on the CPU (tds_hip_policy_trajectory_vjp_host; the checker of
    HipSim.policy_trajectory_vjp, needs no GPU).

    x0 [N, input_dim] (its action slots are not read), policy [P] (every environment) or [N, P], gs None or
    [N, n_rec, nq + nd], ga None or [N, steps, n_act]; the network as for policy_network_spec; params and theta as for
    trajectory_vjp_host.  Returns (s, u, gpolicy, gx0, gtheta), with tape_len also the entries each step recorded
    [N, steps]; gs and ga both None: (s, u), the primal alone."""
    call = functools.partial(lib().tds_hip_policy_trajectory_vjp_host, C.byref(m))
    out = _policy_trajectory_vjp(_HostArrays, call, m, x0, policy, gs, steps, every, ga, (layer_sizes, activations, use_bias),
                                 params, theta, first_obs_raw, obs_raw, (tape_cap, tape_len))
    return out[:2] if gs is None and ga is None else out if tape_len else out[:5]


def trajectory_directions(input_dim: int, wrt, p: int = 0, device=None):
    """unit directions [len(wrt) + p, input_dim + p]: one per entry of x0 in wrt, then one per parameter"""
    import torch

    cols = [int(i) for i in wrt]
    for i in cols:
        if not 0 <= i < input_dim:
            raise ValueError(f"wrt entry {i} out of range (input_dim {input_dim})")
    cols += [input_dim + j for j in range(p)]
    v = torch.zeros((len(cols), input_dim + p), dtype=torch.float64, device=device)
    if cols:
        v[torch.arange(len(cols)), torch.tensor(cols)] = 1.0
    return v


def _rb_check(rc):
    if rc != TDS_OK:
        raise TdsHipError(f"tds_rb error {rc}: {lib().tds_rb_last_error().decode()}")


def rb_params_get(m: _model.RbModel, params):
    """theta [p]: the rigid-body model's values of a parameter selection (tds_rb_params_get; checks the selection).
    Kinds: ("mass", body), ("gravity", comp), ("friction",), ("restitution",)."""
    import numpy as np

    sel = param_spec(params)
    p = len(params)
    theta = np.zeros(max(p, 1), dtype=np.float64)
    _rb_check(lib().tds_rb_params_get(C.byref(m), p, sel, theta.ctypes.data))
    return theta[:p]


def rb_jvp_host(m: _model.RbModel, s0, steps: int, v=None, params=(), theta=None):
    """Forward-mode rollout derivative on the CPU (tds_rb_jvp_host; the checker of RigidBodySim.jvp, needs no GPU).

    s0 [N, num_bodies, 13], v [N, K, num_bodies * 13 + p] (or [N, num_bodies * 13 + p]: K = 1), theta None (the model's
    values), [p] or [N, p].  Returns s_T [N, num_bodies, 13] (v None) or (s_T, jv), jv [N, K, num_bodies, 13] (or
    [N, num_bodies, 13])."""
    sT, jv = _rb_jvp(_HostArrays, functools.partial(lib().tds_rb_jvp_host, C.byref(m)), m, s0, steps, v, params, theta)
    return sT if v is None else (sT, jv)


def rb_vjp_host(m: _model.RbModel, s0, steps: int, gs, params=(), theta=None, every=None, tape_cap: int = 0):
    """Reverse-mode rollout derivative on the CPU (tds_rb_vjp_host; the checker of RigidBodySim.vjp, needs no GPU).

    s0 [N, num_bodies, 13]; the state after every `every`-th step is recorded (None: the final state alone), gs
    [N, n_rec, num_bodies * 13] (or anything of that many entries: [N, num_bodies, 13] for one record) is the cotangent on
    the records; theta None (the model's values), [p] or [N, p].  Returns (s [N, n_rec, num_bodies, 13], gs0
    [N, num_bodies, 13], gtheta [N, p]).  tape_cap: entries one step's tape may hold (0: the model's bound); a world
    that overflows gets NaN gradients and the call raises."""
    call = functools.partial(lib().tds_rb_vjp_host, C.byref(m))
    return _rb_vjp(_HostArrays, call, m, s0, steps, gs, params, theta, every, tape_cap)


def rb_vjp_plan(m: _model.RbModel, n: int, steps: int, p: int = 0, tape_cap: int = 0, work_bytes: int = 0):
    """(tape capacity, worlds per pass, steps per window W, bytes of work buffer) a RigidBodySim.vjp call would choose
    (tds_rb_vjp_plan; needs no GPU)"""
    out = (C.c_longlong * 4)()
    _rb_check(lib().tds_rb_vjp_plan(C.byref(m), int(n), int(steps), int(p), int(tape_cap), int(work_bytes), out))
    return tuple(int(x) for x in out)


def jacobian_tangents(m: _model.Model) -> int:
    """tangents one device lane carries for this model (0: the model is refused)"""
    return int(lib().tds_hip_jacobian_tangents(C.byref(m)))


def wrap_device_pointer(ptr: int, shape, torch_dtype, device: int, owner=None):
    """zero-copy torch view of library-owned device memory"""
    import torch

    class _Holder:
        pass

    hld = _Holder()
    hld.__cuda_array_interface__ = {
        "shape": tuple(shape), "typestr": "<f8" if torch_dtype == torch.float64 else "<f4",
        "data": (int(ptr), False), "version": 2, "strides": None,
    }
    t = torch.as_tensor(hld, device=f"cuda:{device}")
    t._tds_owner = owner
    return t


def dtype_code(dtype) -> int:
    """"f64": double arithmetic + double records; "mixed": double arithmetic + FLOAT records (the reference's float
    record ABI, parity-gated); "f32": pure float (measured only)."""
    if isinstance(dtype, int):
        return dtype
    return {"f64": _model.TDS_DTYPE_F64, "float64": _model.TDS_DTYPE_F64, "f32": _model.TDS_DTYPE_F32,
            "float32": _model.TDS_DTYPE_F32, "mixed": _model.TDS_DTYPE_F64_REC32,
            "f64r32": _model.TDS_DTYPE_F64_REC32}[dtype]


class HipSim:
    """N resident environments of one model on one GPU.

    ``x`` / ``y`` are torch views (no copy) of the library-owned env-major records
    [N, input_dim] / [N, output_dim] in the RECORD dtype (``torch_dtype``: float64 for "f64", float32 for "mixed"
    and "f32").
    """

    def __init__(self, m: _model.Model, num_envs: int, device: int = 0, dtype: str = "f64",
                 lanes_per_env: int | None = None, na_cap: int | None = None, _handle=None, _owner=None,
                 options: dict | None = None):
        import torch

        if not torch.cuda.is_available():
            raise TdsHipError("no HIP device visible (the HIP path has no CPU fallback)")
        self.model = m.copy()
        self.num_envs = int(num_envs)
        self.device = int(device)
        self.dtype = dtype_code(dtype)
        self.torch_dtype = torch.float64 if self.dtype == _model.TDS_DTYPE_F64 else torch.float32
        self._owner = _owner  # a HipShard owns the handle of its sim
        if _handle is not None:
            self.h = _handle
            self.input_dim = self.model.input_dim
            self.output_dim = self.model.output_dim
            self.x = self._wrap(lib().tds_hip_x_device(self.h), (self.num_envs, self.input_dim))
            self.y = self._wrap(lib().tds_hip_y_device(self.h), (self.num_envs, self.output_dim))
            self.use_current_stream()
            return
        create_opts = {}
        if lanes_per_env is not None:
            create_opts["lanes_per_env"] = lanes_per_env
        if na_cap is not None:
            create_opts["na_cap"] = na_cap
        if options:  # create-time options go through the process defaults, run-time ones are set on the new handle
            ct = ("lanes_per_env", "na_cap", "w2", "gram", "no_chain", "no_rootjoint", "no_kinchain", "no_eulerroot",
                  "no_legscan", "fold_fixed", "quad", "oct", "chain")
            create_opts.update({k: v for k, v in options.items() if k in ct})
        h = C.c_void_p()
        with default_options(**create_opts):
            _check(lib().tds_hip_create(C.byref(self.model), self.num_envs, self.device, self.dtype, C.byref(h)))
        self.h = h
        if options:
            for k, v in options.items():
                if k not in create_opts:
                    self.set_option(k, v)
        self.input_dim = self.model.input_dim
        self.output_dim = self.model.output_dim
        self.x = self._wrap(lib().tds_hip_x_device(self.h), (self.num_envs, self.input_dim))
        self.y = self._wrap(lib().tds_hip_y_device(self.h), (self.num_envs, self.output_dim))
        self.use_current_stream()

    # -- zero-copy torch view of library-owned device memory -------------------------------
    def _wrap(self, ptr, shape):
        import torch

        n = 1
        for s in shape:
            n *= s
        itemsize = 8 if getattr(self, "dtype", _model.TDS_DTYPE_F64) == _model.TDS_DTYPE_F64 else 4
        typestr = "<f8" if itemsize == 8 else "<f4"

        class _Holder:
            pass

        hld = _Holder()
        hld.__cuda_array_interface__ = {
            "shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False), "version": 2,
            "strides": None,
        }
        t = torch.as_tensor(hld, device=f"cuda:{self.device}")
        t._tds_owner = self  # keep the handle alive as long as the view lives
        return t

    def set_option(self, key: str, value) -> None:
        """run-time option of this handle (tds_hip_set_option; csrc/tds_options.h lists the keys)"""
        _check(lib().tds_hip_set_option(self.h, key.encode(), -(1 << 63) if value is None else int(value)))

    def get_option(self, key: str):
        """the option's value, or None while it is unset (library rule)"""
        v, st = C.c_longlong(0), C.c_int(0)
        _check(lib().tds_hip_get_option(self.h, key.encode(), C.byref(v), C.byref(st)))
        return int(v.value) if st.value else None

    def use_current_stream(self):
        import torch

        st = torch.cuda.current_stream(self.device)
        _check(lib().tds_hip_set_stream(self.h, C.c_void_p(st.cuda_stream)))

    def close(self):
        if getattr(self, "h", None):
            if getattr(self, "_owner", None) is None:
                lib().tds_hip_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def step_many_prepare(self, actions, n_steps: int, obs=None, first_block: int = 0):
        """Capture + instantiate the hipGraph of ``n_steps`` closed-loop steps without running anything."""
        ap, nb, op = self._many_args(actions, obs)
        _check(lib().tds_hip_step_many_prepare(self.h, ap, nb, int(first_block), int(n_steps), op))

    def step_many(self, actions, n_steps: int, obs=None, first_block: int = 0):
        """``n_steps`` closed-loop steps per host call (tds_hip_step_many: chained hipGraphs or one step-loop launch,
        see step_many_is_loop): step k takes the action block ``actions[(first_block + k) % len(actions)]``
        ([B, N, action_dim] device tensor, or None).  With auto-reset on, every step resets what it ends with done."""
        ap, nb, op = self._many_args(actions, obs)
        _check(lib().tds_hip_step_many(self.h, ap, nb, int(first_block), int(n_steps), op))

    def _rings(self, obs_ring, y_ring, obs_first, y_first, progress=None):
        import torch

        r = Rings()
        if obs_ring is not None:
            assert obs_ring.is_cuda and obs_ring.is_contiguous() and obs_ring.dim() == 3
            assert tuple(obs_ring.shape[1:]) == (self.num_envs, self.obs_dim + 2)
            assert obs_ring.dtype in (self.torch_dtype, torch.float32)
            r.obs_ring, r.obs_slots, r.obs_first = obs_ring.data_ptr(), int(obs_ring.shape[0]), int(obs_first)
            r.obs_f32 = 1 if (obs_ring.dtype == torch.float32 and self.torch_dtype != torch.float32) else 0
        if y_ring is not None:
            assert y_ring.is_cuda and y_ring.is_contiguous() and y_ring.dim() == 3 and y_ring.dtype == self.torch_dtype
            # (a last dimension beyond output_dim: a padded record stride, tds_hip_rings_t::y_stride)
            assert int(y_ring.shape[1]) == self.num_envs and int(y_ring.shape[2]) >= self.output_dim
            r.y_ring, r.y_slots, r.y_first = y_ring.data_ptr(), int(y_ring.shape[0]), int(y_first)
            r.y_stride = int(y_ring.shape[2]) if int(y_ring.shape[2]) != self.output_dim else 0
        if progress is not None:
            # (one counter per slot of the obs ring, tds_hip_rings_t::progress)
            assert progress.is_cuda and progress.dtype == torch.int64 and obs_ring is not None
            assert progress.numel() >= int(obs_ring.shape[0])
            r.progress = progress.data_ptr()
        return r

    def step_many_rings(self, actions, n_steps: int, obs_ring=None, y_ring=None, first_block: int = 0,
                        obs_first: int = 0, y_first: int = 0, progress=None, prepare_only: bool = False):
        """``n_steps`` closed-loop steps per host call WITH per-step records (tds_hip_step_many_rings): step k leaves its
        [obs | reward | done] record in ``obs_ring[(obs_first + k) % len(obs_ring)]`` ([S, N, obs_dim + 2]) and its y
        record in ``y_ring[(y_first + k) % len(y_ring)]`` ([S', N, output_dim]) — what the reference's
        VectorizedEnvironment::step hands out every step.  One step-loop launch where step_many_is_loop holds."""
        ap, nb, _ = self._many_args(actions, None)
        r = self._rings(obs_ring, y_ring, obs_first, y_first, progress)
        f = lib().tds_hip_step_many_rings_prepare if prepare_only else lib().tds_hip_step_many_rings
        _check(f(self.h, ap, nb, int(first_block), int(n_steps), C.byref(r)))

    def prepared_step_many_rings(self, actions, n_steps: int, obs_ring=None, y_ring=None, first_block: int = 0,
                                 obs_first: int = 0, y_first: int = 0):
        """step_many_rings with every argument marshalled NOW: returns a callable whose body is the one C call (a
        20-step timed region is 0.3 ms — tens of microseconds of Python argument checking inside it are a tenth of it).
        Builds the graphs of the graph form as well (tds_hip_step_many_rings_prepare)."""
        ap, nb, _ = self._many_args(actions, None)
        r = self._rings(obs_ring, y_ring, obs_first, y_first, None)
        L, h, fb, ns, rr = lib(), self.h, int(first_block), int(n_steps), C.byref(r)
        _check(L.tds_hip_step_many_rings_prepare(h, ap, nb, fb, ns, rr))
        keep = (actions, obs_ring, y_ring, r)  # (the tensors and the struct must outlive the callable)

        def call(_f=L.tds_hip_step_many_rings, _keep=keep):
            if _f(h, ap, nb, fb, ns, rr) != TDS_OK:
                _check(-1)

        return call

    def step_many_rings_raw(self, actions, n_steps: int, rings: "Rings", first_block: int = 0):
        """tds_hip_step_many_rings with a hand-filled tds_hip_rings_t (obs_slot_envs, strides ...)"""
        ap, nb, _ = self._many_args(actions, None)
        _check(lib().tds_hip_step_many_rings(self.h, ap, nb, int(first_block), int(n_steps), C.byref(rings)))

    def profile_zones(self) -> dict:
        """one instrumented step, reported through the SubmitProfileTiming-shaped callback (tds_hip_profile_zones):
        {zone name: microseconds}"""
        out = {}
        FN = C.CFUNCTYPE(None, C.c_char_p, C.c_double, C.c_void_p)

        def cb(name, us, _user):
            out[name.decode()] = float(us)

        f = FN(cb)
        lib().tds_hip_profile_zones.argtypes = [C.c_void_p, FN, C.c_void_p]
        _check(lib().tds_hip_profile_zones(self.h, f, None))
        return out

    def rings_blocks(self) -> int:
        """increments of a rings progress counter per completed step (= workgroups of the step-loop launch)"""
        return int(lib().tds_hip_step_many_rings_blocks(self.h))

    def debug_poison_lds(self, byte_pattern: int = 0xFF):
        """Test aid: every compute unit's LDS filled with the byte pattern (0xFF: NaN in every scalar type)."""
        _check(lib().tds_hip_debug_poison_lds(self.h, int(byte_pattern)))

    def step_many_is_loop(self, n_steps: int) -> bool:
        """True if step_many(n_steps) runs as launches of the step-loop kernel (worlds without contact points; narrow
        kernels with contacts up to three rounds of workgroups, or at any batch size with auto-reset on)."""
        return bool(lib().tds_hip_step_many_is_loop(self.h, int(n_steps)))

    def set_graph_chains(self, chains: int):
        """Environment chains of the step_many graphs (0: library default); see tds_hip_step_many in tds_hip.h."""
        _check(lib().tds_hip_set_graph_chains(self.h, int(chains)))

    def tune_step_many(self, actions, probe_steps: int = 64, obs=None) -> int:
        """Measure 1, 2 and 3 chains on ``probe_steps`` steps each (the simulation ADVANCES by 6 x probe_steps steps),
        keep the fastest for later step_many calls and return it."""
        ap, nb, op = self._many_args(actions, obs)
        c = C.c_int()
        _check(lib().tds_hip_step_many_tune(self.h, ap, nb, int(probe_steps), op, C.byref(c)))
        return c.value

    def _many_args(self, actions, obs):
        ap, nb, op = None, 1, None
        if actions is not None:
            assert actions.is_cuda and actions.dtype == self.torch_dtype and actions.is_contiguous()
            assert actions.dim() == 3 and tuple(actions.shape[1:]) == (self.num_envs, self.model.action_dim)
            ap, nb = C.c_void_p(actions.data_ptr()), int(actions.shape[0])
        if obs is not None:
            assert obs.is_cuda and obs.dtype == self.torch_dtype and obs.is_contiguous()
            assert tuple(obs.shape) == (self.num_envs, self.obs_dim + 2)
            op = C.c_void_p(obs.data_ptr())
        return ap, nb, op

    def sync(self):
        _check(lib().tds_hip_sync(self.h))

    # -- the hot path -----------------------------------------------------------------------
    def forward_zero(self, x, y=None):
        """y = f(x) on device tensors [N, input_dim] -> [N, output_dim] (async)."""
        import torch

        assert x.is_cuda and x.dtype == self.torch_dtype and x.is_contiguous()
        assert tuple(x.shape) == (self.num_envs, self.input_dim)
        if y is None:
            y = torch.empty((self.num_envs, self.output_dim), dtype=self.torch_dtype, device=x.device)
        assert y.is_cuda and y.dtype == self.torch_dtype and y.is_contiguous()
        _check(lib().tds_hip_forward_zero_device(self.h, C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr())))
        return y

    # -- step Jacobians (forward mode, a kernel of its own) ------------------------------------
    def jvp(self, x, v, y=None):
        """(y, jv): y = f(x) [N, output_dim] and the directional derivatives jv = J(x) v [N, K, output_dim] for
        v [N, K, input_dim] (or [N, input_dim]: K = 1, jv [N, output_dim]).  Any N; f64 handles only (async)."""
        A = _DevArrays
        x = A.records(x, self.input_dim, "x")
        n = x.shape[0]
        v3, squeeze = A.tangents(v, n, self.input_dim, "v")
        y = A.new((n, self.output_dim), x) if y is None else y
        jv = A.new((n, v3.shape[1], self.output_dim), x)
        _check(lib().tds_hip_jvp(self.h, n, A.ptr(x), v3.shape[1], A.ptr(v3), A.ptr(y), A.ptr(jv)))
        return y, (jv[:, 0] if squeeze else jv)

    def jacobian(self, x, rows=None, cols=None, accumulate=None, y=None):
        """J = dy/dx at x [N, input_dim]: [N, n_rows, n_cols] (accumulate None) or [n_rows, n_cols] ("sum", "mean");
        rows / cols: index lists into y / x (None: dense).  With y (a [N, output_dim] tensor) forward_zero's output is
        written too.  Any N; f64 handles only."""
        call = functools.partial(lib().tds_hip_jacobian, self.h)
        return _jacobian(_DevArrays, call, self.model, x, rows, cols, accumulate, y is not None, y)[0]

    def vjp(self, x, w, y=None):
        """(y, wj): y = f(x) [N, output_dim] and the vector-Jacobian products wj = w^T J(x) [N, K, input_dim] for
        cotangents w [N, K, output_dim] (or [N, output_dim]: K = 1, wj [N, input_dim]).  Reverse mode: one tape per
        environment, swept back once per cotangent.  Any N; f64 handles only.  The call waits for its kernels."""
        return _vjp(_DevArrays, functools.partial(lib().tds_hip_vjp, self.h), self.model, x, w, True, y)[:2]

    # -- parameter derivatives: [x | theta], theta the selected model scalars per environment ---------------------
    def jvp_params(self, x, theta, params, v=None):
        """y = f(x; theta) [N, output_dim] (v None), else (y, jv): jv = J v [N, K, output_dim] for directions v
        [N, K, input_dim + p] over [x | theta] (or [N, input_dim + p]: K = 1, jv [N, output_dim]).  theta [p] (every
        environment) or [N, p], the values of the selection `params` (tuples or tds_param_t, see param_spec).  Any N;
        f64 handles only (async)."""
        call = functools.partial(lib().tds_hip_jvp_params, self.h)
        y, jv = _jvp_params(_DevArrays, call, self.model, x, theta, params, v)
        return y if v is None else (y, jv)

    def vjp_params(self, x, theta, params, w):
        """(y, wj_x, wj_theta): y = f(x; theta) and w^T J split into its x part [N, (K,) input_dim] and its theta part
        [N, (K,) p], for cotangents w [N, K, output_dim] (or [N, output_dim]: K = 1).  theta and params as for
        jvp_params.  Reverse mode; the call waits for its kernels."""
        call = functools.partial(lib().tds_hip_vjp_params, self.h)
        y, wj, _ = _vjp(_DevArrays, call, self.model, x, w, True, None, params, theta)
        return y, wj[..., :self.input_dim], wj[..., self.input_dim:]

    # -- articulated trajectories: forward_zero chained, forward mode in [x0 | theta] ----------------------------------
    def trajectory_jvp(self, x0, v=None, steps: int = 1, every: int = 1, u=None, params=(), theta=None):
        """(s, js): the states s [N, n_rec, nq + nd] after steps every, 2 every, .., steps of forward_zero chained from
        x0 [N, input_dim] (any N), and js = (d s / d [x0 | theta]) v [N, K, n_rec, nq + nd] for directions v
        [N, K, input_dim + p] (or [N, input_dim + p]: K = 1, js [N, n_rec, nq + nd]); v None: js None.  u None (x0's
        actions every step) or [N, steps - 1, n_act], the actions of steps 1 ..; not differentiated.  params and theta
        as for jvp_params; theta None: the model's values.  The resident state is not touched.  f64 handles only
        (async)."""
        # (k = 0 directions: v and js have no extent, their pointers are NULL, and the call is the primal one)
        call = functools.partial(lib().tds_hip_trajectory_jvp, self.h)
        return _trajectory_jvp(_DevArrays, call, self.model, x0, v, steps, every, u, params, theta)

    def trajectory_vjp(self, x0, gs, steps: int, every: int = 1, u=None, params=(), theta=None):
        """(s, gx0, gu, gtheta): the states s of trajectory_jvp's trajectory and the gradients of <gs, s> for the
        cotangent gs [N, n_rec, nq + nd] on them: gx0 [N, input_dim] in x0, gu [N, steps - 1, n_act] in the actions u of
        steps 1 .. (zeros where u is None: x0's action slots then feed every step, and gx0 holds their gradient) and
        gtheta [N, p] in theta.  Reverse mode: one primal pass, then the steps' tapes recorded several at a time
        (option traj_vjp_lanes) and swept back in turn; the call waits for its kernels.  f64 handles only."""
        call = functools.partial(lib().tds_hip_trajectory_vjp, self.h)
        return _trajectory_vjp(_DevArrays, call, self.model, x0, gs, steps, every, u, params, theta)[:4]

    # -- closed loop: the policy network between the steps, gradients through dynamics and policy -----------------
    def policy_trajectory_vjp(self, x0, policy, gs, steps: int, every: int = 1, ga=None, layer_sizes=None,
                              activations=None, use_bias=None, params=(), theta=None, first_obs_raw: bool = False,
                              obs_raw: bool = False):
        """(s, u, gpolicy, gx0, gtheta) of the closed-loop trajectory u_t = pi(obs_t) (tds_hip_policy_trajectory_vjp):
        the recorded states s [N, n_rec, nq + nd], the actions taken u [N, steps, n_act], and the gradients of
        <gs, s> + <ga, u> in the policy's parameters [N, P], in x0 [N, input_dim] (action slots zero) and in theta
        [N, p].  policy [P] (every environment) or [N, P]; the network as for hip_backend.policy_network_spec
        (layer_sizes None: the linear policy); gs [N, n_rec, nq + nd] or None, ga [N, steps, n_act] or None (both None:
        the primal alone, the gradients come back as None).  obs_raw: the policy sees obs[0], obs[1] as they are at
        every step (fixed-base models), first_obs_raw: at step 0 only.  The call waits for its kernels where a
        cotangent is given.  f64 handles only."""
        call = functools.partial(lib().tds_hip_policy_trajectory_vjp, self.h)
        return _policy_trajectory_vjp(_DevArrays, call, self.model, x0, policy, gs, steps, every, ga,
                                      (layer_sizes, activations, use_bias), params, theta, first_obs_raw, obs_raw)[:5]

    def policy_trajectory(self, x0, policy, steps: int, every: int = 1, layer_sizes=None, activations=None,
                          use_bias=None, params=(), theta=None, first_obs_raw: bool = False, obs_raw: bool = False):
        """(s, u): the closed-loop trajectory of policy_trajectory_vjp alone (async)"""
        return self.policy_trajectory_vjp(x0, policy, None, steps, every, None, layer_sizes, activations, use_bias,
                                          params, theta, first_obs_raw, obs_raw)[:2]

    # -- dynamics queries: kinematics, mass matrix, bias, forward and inverse dynamics, point Jacobians -----------
    def dynamics(self, q, qd=None, tau=None, want=DYN_OUTPUTS, out=None):
        """The wanted ones of x_world [N, num_links, 12], mass_matrix [N, dof_qd, dof_qd], bias [N, dof_qd] and
        qdd [N, dof_qd] at the states q [N, dof_q], qd [N, dof_qd] (None: zero), as a dict of tensors on the handle's
        device.  tau [N, dyn_tau_dim(model)] (None: zero) are the torques of qdd, the unconstrained forward dynamics.
        out: a dict of tensors to write into.  Any N; f64 handles only; only the wanted outputs are computed (async)."""
        call = functools.partial(lib().tds_hip_dynamics, self.h)
        return _dynamics(_DevArrays, call, self.model, q, qd, tau, want, out)

    def forward_kinematics(self, q):
        """x_world [N, num_links, 12]: rotation (9, row-major) and translation (3) of every link"""
        return self.dynamics(q, want=("x_world",))["x_world"]

    def mass_matrix(self, q):
        """the joint-space inertia M(q) [N, dof_qd, dof_qd]"""
        return self.dynamics(q, want=("mass_matrix",))["mass_matrix"]

    def forward_dynamics(self, q, qd=None, tau=None):
        """qdd [N, dof_qd] without contacts or PD control: M^-1 (tau - K q - D qd - bias)"""
        return self.dynamics(q, qd, tau, want=("qdd",))["qdd"]

    def inverse_dynamics(self, q, qd=None, qdd=None):
        """tau [N, dof_qd] = ID(q, qd, qdd) (None: zero), without springs or dampers; fixed base only (async)"""
        call = functools.partial(lib().tds_hip_inverse_dynamics, self.h)
        return _inverse_dynamics(_DevArrays, call, self.model, q, qd, qdd)

    def point_jacobian(self, q, link: int, point, local: bool = False):
        """The world-frame Jacobian [N, 3, dof_qd] of the points [N, 3] on link `link` (-1: the base); local: the points
        are given in the link's own frame (async)"""
        call = functools.partial(lib().tds_hip_point_jacobian, self.h)
        return _point_jacobian(_DevArrays, call, self.model, q, link, point, local)

    # -- forward-mode derivatives of the dynamics queries in [q | qd | tau or qdd | theta] -------------------------
    def dynamics_jvp(self, q, qd=None, tau=None, v=None, want=DYN_OUTPUTS, params=(), theta=None, out=None,
                     want_primal: bool = False):
        """Forward-mode derivatives of the dynamics queries in z = [q | qd | tau | theta] (tds_hip_dynamics_jvp): for
        directions v [N, k, dyn_input_dim(model) + p] over the states, the torques and the selection `params`
        (param_spec) the tangents of the wanted DYN_OUTPUTS, a dict of tensors [N, k, *shape] (dyn_tangent_shapes);
        with want_primal (tangents, primal): the outputs themselves as well.  qd, tau None: zero in value (their
        columns of v still count).  theta [p] or [N, p]: the selection's values (None: the model's).  v None: the
        primal dict at theta alone.  out: a dict of tangent tensors to write into.  Any N; f64 handles only; one launch
        over (environment, block of dynamics_jvp_tangents(model) directions) items (async)."""
        call = functools.partial(lib().tds_hip_dynamics_jvp, self.h)
        return _dynamics_jvp(_DevArrays, call, self.model, q, qd, tau, v, want, params, theta, want_primal, out, None)

    def inverse_dynamics_jvp(self, q, qd=None, qdd=None, v=None, params=(), theta=None, want_primal: bool = False):
        """Forward-mode derivatives of tau = ID(q, qd, qdd) in z = [q | qd | qdd | theta]
        (tds_hip_inverse_dynamics_jvp): dtau [N, k, dof_qd] for directions v [N, k, dof_q + 2 dof_qd + p], with
        want_primal (dtau, tau); v None: tau [N, dof_qd] at theta alone.  Arguments as for dynamics_jvp; fixed base
        only (async)."""
        call = functools.partial(lib().tds_hip_inverse_dynamics_jvp, self.h)
        return _inverse_dynamics_jvp(_DevArrays, call, self.model, q, qd, qdd, v, params, theta, want_primal)

    def dynamics_jacobian(self, q, qd=None, tau=None, want="qdd", cols=None, params=(), theta=None):
        """The dense derivative of one dynamics output: [N, *shape, n_cols], columns `cols` indexing into
        z = [q | qd | tau | theta] (None: all dyn_input_dim(model) + p), from identity directions through
        dynamics_jvp."""
        nall = dyn_input_dim(self.model) + len(params)
        (name,) = _dyn_want(want)
        v = _identity_directions(q.shape[0], nall, cols, q.device)
        return self.dynamics_jvp(q, qd, tau, v, want=(name,), params=params, theta=theta)[name].movedim(1, -1).contiguous()

    # -- the contact query: points, Jacobians, rows, Delassus matrix, impulses, forces -----------------------------
    def contacts(self, x, want=CONTACT_OUTPUTS, out=None):
        """What the step forward_zero(x) does about its plane contacts at the records x [N, input_dim]: the wanted
        CONTACT_OUTPUTS (shapes: contact_shapes(model, N)) as a dict of tensors on the handle's device.  out: a dict of
        tensors to write into.  Any N; f64 handles only; only the wanted outputs are computed (async)."""
        want = _contact_want(want)
        x = _DevArrays.records(x, self.input_dim, "x")
        n = x.shape[0]
        res, o = _dev_outputs(contact_shapes(self.model, n), want, out, x.device, struct=ContactOut)
        _check(lib().tds_hip_contacts(self.h, n, C.c_void_p(x.data_ptr()), C.byref(o)))
        return res

    def contacts_jvp(self, x, v, want=CONTACT_OUTPUTS, params=(), theta=None, out=None, want_primal: bool = False):
        """Forward-mode derivatives of the contact query in [x | theta] (tds_hip_contacts_jvp): for directions v
        [N, k, input_dim + p] over the record and the selection `params` (param_spec, the contact kinds included) the
        tangents of the wanted CONTACT_OUTPUTS, a dict of tensors [N, k, *shape] (contact_tangent_shapes); with
        want_primal (tangents, primal): the outputs themselves as well.  theta [p] or [N, p]: the selection's values
        (None: the model's).  v None: the primal dict at theta alone.  out: a dict of tangent tensors to write into.
        The derivative of the algorithm as executed (contact activation, PGS projections and the actuation clamps
        follow the primal's branch; a separated point has zero tangents).  Any N; f64 handles only; one launch over
        (environment, block of contacts_jvp_tangents(model) directions) items (async)."""
        call = functools.partial(lib().tds_hip_contacts_jvp, self.h)
        return _contacts_jvp(_DevArrays, call, self.model, x, v, want, params, theta, want_primal, out, None)

    def contacts_jacobian(self, x, want, cols=None, params=(), theta=None):
        """The dense derivative of one contact output: [N, *shape, n_cols], columns `cols` indexing into [x | theta]
        (None: all input_dim + p), from identity directions through contacts_jvp."""
        nall = self.input_dim + len(params)
        (name,) = _contact_want(want)
        v = _identity_directions(x.shape[0], nall, cols, x.device)
        return self.contacts_jvp(x, v, want=(name,), params=params, theta=theta)[name].movedim(1, -1).contiguous()

    def contact_forces(self, x):
        """force [N, n_c, 3]: the world-frame contact force on the robot at each contact point of the step from x"""
        return self.contacts(x, want=("force",))["force"]

    def inverse_kinematics(self, q_init, links, targets, body_points=None, q_reference=None, method="pinv", out=None,
                           **options):
        """Batched inverse kinematics (tds_hip_inverse_kinematics: the reference's TinyInverseKinematics::compute for
        every environment, one launch): from q_init [N, dof_q], move the actuated coordinates until the points
        body_points [K, 3] (the links' own frames; None: their origins) of links [K] (1 <= K <= 4) reach
        targets [N, K, 3] (world coordinates).  q_reference [N, dof_q] (optional) pulls towards a configuration;
        method "transpose" / "pinv" / "damped_lm"; options of IK_OPTIONS.  Returns a dict of tensors on the handle's
        device: q [N, dof_q] float64, iterations [N] and status [N] int32 (IK_FAILED / IK_CONVERGED / IK_REACHED),
        residual [N] float64.  out: a dict of tensors to write into; one that names q but leaves out iterations,
        status or residual has those not computed.  Any N; f64 handles only (async)."""
        call = functools.partial(lib().tds_hip_inverse_kinematics, self.h)
        return _inverse_kinematics(_DevArrays, call, self.model, q_init, links, targets, body_points, q_reference, out,
                                   ik_options(method, **options))

    # -- batched iLQR (csrc/tds_lqr.hip) ----------------------------------------------------------------------
    def lqr_backward(self, A, B, lx, lu, lxx, luu, lux, mu):
        """The backward pass of n time-varying LQ problems as one launch (tds_hip_lqr_backward; arguments and results
        as hip_backend.lqr_backward_host, CUDA float64 tensors; mu [n]).  The handle's model is not read.  Async."""
        call = functools.partial(lib().tds_hip_lqr_backward, self.h)
        return _lqr_backward(_DevArrays, call, False, A, B, lx, lu, lxx, luu, lux, mu)

    def lqr_backward_box(self, A, B, lx, lu, lxx, luu, lux, mu, dlo, dhi, check: bool = True):
        """The backward pass under control limits as one launch (tds_hip_lqr_backward_box; arguments and results as
        hip_backend.lqr_backward_box_host, CUDA tensors).  check: dlo <= dhi without NaN is verified before the launch
        (the one host wait of the call); a caller that built the bounds itself passes False and the call is
        asynchronous.  The handle's model is not read."""
        call = functools.partial(lib().tds_hip_lqr_backward_box, self.h)
        return _lqr_backward(_DevArrays, call, check, A, B, lx, lu, lxx, luu, lux, mu, dlo, dhi)

    def feedback_rollout(self, x0, s_nom, u_nom, k, K, alpha, problem_of_row=None, check: bool = True, u_lo=None,
                         u_hi=None):
        """The closed-loop rollout under u_t = (u_nom + alpha k) + K (s_t - s_nom) (tds_hip_feedback_rollout; arguments
        and results as hip_backend.feedback_rollout_host, CUDA float64 tensors; alpha [rows]; problem_of_row a CUDA
        int32 tensor [rows] with entries in [0, P), or None).  Any number of rows.  check: the entries of problem_of_row
        are verified before the launch (the one host wait of the call); a caller that built the map itself passes
        False and the call is asynchronous.  u_lo, u_hi [P, T, n_act] (both or neither): u_t is clamped to them
        (tds_hip_feedback_rollout_box; u_lo <= u_hi without NaN is verified under check); None is the call without
        limits."""
        # (P is an argument of the host entry points alone)
        calls = [lambda rows, T, P, *ptrs, f=f: f(self.h, rows, T, *ptrs)
                 for f in (lib().tds_hip_feedback_rollout, lib().tds_hip_feedback_rollout_box)]
        return _feedback_rollout(_DevArrays, calls, check, check, self.model, x0, s_nom, u_nom, k, K, alpha, problem_of_row,
                                 u_lo, u_hi)

    # -- batched system identification (csrc/tds_lm.hip) --------------------------------------------------------
    def lm_step(self, row_start, s, s_obs, js, lam=None, w=None, dlo=None, dhi=None, check: bool = True):
        """One Levenberg-Marquardt step of n least-squares problems as one launch, a wavefront per problem
        (tds_hip_lm_step; arguments and results as hip_backend.lm_step_host, CUDA float64 tensors; row_start a CUDA
        int32 tensor [n + 1]).  Any n, independent of num_envs; the handle's model is not read.  check: row_start,
        dlo <= dhi without NaN and lam > 0 are verified before the launch (the host waits of the call); a caller that
        built them itself passes False and the call is asynchronous."""
        call = functools.partial(lib().tds_hip_lm_step, self.h)
        return _lm_step(_DevArrays, call, check, row_start, s, s_obs, js, lam, w, dlo, dhi)

    def trajectory_jacobian(self, x0, steps: int, wrt, params=(), theta=None, every: int = 1, u=None):
        """dense d s / d [x0 entries wrt | theta]: [N, n_rec (nq + nd), len(wrt) + p] from unit directions (wrt: indices
        into x0's input_dim entries)"""
        n, p = x0.shape[0], len(params)
        v = trajectory_directions(self.input_dim, wrt, p, device=x0.device).expand(n, -1, -1)
        _, js = self.trajectory_jvp(x0, v, steps, every, u, params, theta)
        return js.reshape(n, v.shape[1], -1).transpose(1, 2)

    def step(self, actions=None, substeps: int = 1, obs=None):
        """Closed-loop step on the resident records (async): x[:, act] <- actions, y = f(x),
        x[:, :nq+nd] <- y[:, :nq+nd].  ``obs`` (optional) [N, obs_dim+2] receives
        [observation | reward | done] from the same launch."""
        ap = None
        if actions is not None:
            assert actions.is_cuda and actions.dtype == self.torch_dtype and actions.is_contiguous()
            assert tuple(actions.shape) == (self.num_envs, self.model.action_dim)
            ap = C.c_void_p(actions.data_ptr())
        op = None
        if obs is not None:
            assert obs.is_cuda and obs.dtype == self.torch_dtype and obs.is_contiguous()
            assert tuple(obs.shape) == (self.num_envs, self.obs_dim + 2)
            op = C.c_void_p(obs.data_ptr())
        _check(lib().tds_hip_step_obs(self.h, ap, int(substeps), op))

    def set_model_variants(self, params, theta, env_variant=None):
        """per-environment model variants (tds_hip_set_model_variants): variant v is params_apply(model, params,
        theta[v]), theta [V, p] a numpy array or a tensor on any device, params anything param_spec takes; environment e
        steps under variant env_variant[e] (None with V == num_envs: its own).  Every stepping path then runs the
        general kernel's variant builds; the derivative and query methods ignore the variants."""
        sel, p, t, nv, ev = _variant_args(params, theta, env_variant, self.num_envs)
        if nv == 0:
            raise ValueError("theta: no variants (clear_model_variants() removes them)")
        _check(lib().tds_hip_set_model_variants(self.h, nv, p, sel, t.ctypes.data if t.size else None,
                                                None if ev is None else ev.ctypes.data))

    def clear_model_variants(self):
        """back to the handle's own model and kernel"""
        _check(lib().tds_hip_set_model_variants(self.h, 0, 0, None, None, None))

    @property
    def num_model_variants(self) -> int:
        return int(lib().tds_hip_model_variants(self.h))

    def set_auto_reset(self, enable: bool, seed: int = 0):
        """Reset (+ settle) environments whose step ends with done inside the step launch."""
        _check(lib().tds_hip_set_auto_reset(self.h, 1 if enable else 0, C.c_ulonglong(seed & (2 ** 64 - 1))))

    def reset(self, mask=None, obs=None):
        """Re-initialise + settle the environments selected by ``mask`` (uint8 [N] device tensor,
        None = all) on device; optionally write their observation into ``obs``."""
        mp = None
        if mask is not None:
            import torch

            assert mask.is_cuda and mask.dtype == torch.uint8 and mask.is_contiguous() and mask.numel() == self.num_envs
            mp = C.c_void_p(mask.data_ptr())
        op = None
        if obs is not None:
            assert obs.is_cuda and obs.dtype == self.torch_dtype and obs.is_contiguous()
            assert tuple(obs.shape) == (self.num_envs, self.obs_dim + 2)
            op = C.c_void_p(obs.data_ptr())
        _check(lib().tds_hip_reset(self.h, mp, op))

    def set_policy_network(self, layer_sizes=None, activations=None, use_bias=None):
        """the policy NETWORK of the rollouts (tds_hip_set_policy_network; the reference's NeuralNetworkSpecification):
        layer_sizes incl. the input (obs_dim) and output (action_dim) layers, activations[i - 1] (TDS_NN_ACT_*: -1
        identity, 0 tanh, 1 sin, 2 relu, 3 soft_relu, 4 elu, 5 sigmoid, 6 softsign) for layer i >= 1, use_bias per layer;
        None restores the default linear policy.  Returns the number of parameters per environment."""
        if layer_sizes is None:
            _check(lib().tds_hip_set_policy_network(self.h, 0, None, None, None))
        else:
            n = len(layer_sizes)
            assert len(activations) == n - 1 and len(use_bias) == n
            arr = lambda v: (C.c_int * len(v))(*[int(a) for a in v])
            lib().tds_hip_set_policy_network.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
            _check(lib().tds_hip_set_policy_network(self.h, n, arr(layer_sizes), arr(activations), arr(use_bias)))
        return self.policy_num_parameters

    @property
    def policy_num_parameters(self) -> int:
        lib().tds_hip_policy_num_parameters.argtypes = [C.c_void_p]
        return int(lib().tds_hip_policy_num_parameters(self.h))

    def rollout_ex(self, policy, n_steps: int, shift: float = 0.0, first_obs_raw: bool = False, stats=None,
                   want_traj: bool = False):
        """rollout + the by-products of Worker::rollouts (tds_hip_rollout_ex): ``stats`` [N, obs_dim, 3] device tensor
        of (count, mean, S) updated in place (None: skipped), trajectories [N, n_steps, output_dim] + lengths [N]
        when ``want_traj``.  Returns (return_sum, steps, traj, traj_len)."""
        import torch

        adim, od = self.model.action_dim, self.obs_dim
        assert policy.is_cuda and policy.dtype == self.torch_dtype and policy.is_contiguous()
        ret = torch.zeros(self.num_envs, dtype=self.torch_dtype, device=policy.device)
        steps = torch.zeros(self.num_envs, dtype=torch.int32, device=policy.device)
        sp = None
        if stats is not None:
            assert stats.is_cuda and stats.dtype == self.torch_dtype and stats.is_contiguous()
            assert tuple(stats.shape) == (self.num_envs, od, 3)
            sp = C.c_void_p(stats.data_ptr())
        traj = tlen = None
        tp = lp = None
        if want_traj:
            traj = torch.zeros((self.num_envs, n_steps, self.output_dim), dtype=self.torch_dtype, device=policy.device)
            tlen = torch.zeros(self.num_envs, dtype=torch.int32, device=policy.device)
            tp, lp = C.c_void_p(traj.data_ptr()), C.c_void_p(tlen.data_ptr())
        _check(lib().tds_hip_rollout_ex(self.h, C.c_void_p(policy.data_ptr()), int(n_steps), C.c_double(shift),
                                        1 if first_obs_raw else 0, C.c_void_p(ret.data_ptr()),
                                        C.c_void_p(steps.data_ptr()), None, sp, tp, lp))
        return ret, steps, traj, tlen

    def rollout(self, policy, n_steps: int, shift: float = 0.0, first_obs_raw: bool = False, obs=None, mode=None):
        """n_steps of { action = W obs + b (per-environment linear policy); step; reward/done } on device
        (tds_hip_rollout): in ONE launch, or — from two wavefronts per SIMD on, without auto-reset — as one
        straight-line step launch per step with a small policy + bookkeeping kernel in between
        (mode "per_step" / "single" forces either).  ``policy``: [N, action_dim*obs_dim + action_dim] device
        tensor in NeuralNetwork parameter order.  Returns (return_sum [N], steps [N] int32) device tensors."""
        import torch

        adim, od = self.model.action_dim, self.obs_dim
        assert policy.is_cuda and policy.dtype == self.torch_dtype and policy.is_contiguous()
        assert tuple(policy.shape) == (self.num_envs, self.policy_num_parameters)
        ret = torch.zeros(self.num_envs, dtype=self.torch_dtype, device=policy.device)
        steps = torch.zeros(self.num_envs, dtype=torch.int32, device=policy.device)
        op = None
        if obs is not None:
            assert obs.is_cuda and obs.dtype == self.torch_dtype and obs.is_contiguous()
            assert tuple(obs.shape) == (self.num_envs, od + 2)
            op = C.c_void_p(obs.data_ptr())
        _check(lib().tds_hip_rollout(self.h, C.c_void_p(policy.data_ptr()), int(n_steps), C.c_double(shift),
                                     (1 if first_obs_raw else 0) | {None: 0, "per_step": 2, "single": 4}[mode],
                                     C.c_void_p(ret.data_ptr()),
                                     C.c_void_p(steps.data_ptr()), op))
        return ret, steps

    @property
    def obs_dim(self) -> int:
        return self.model.dof_q + self.model.dof_qd

    def forward_zero_host(self, x_np):
        """Blocking host-buffer call with the reference's <model>_forward_zero semantics."""
        import numpy as np

        x_np = np.ascontiguousarray(x_np, dtype=np.float64).reshape(-1, self.input_dim)
        y_np = np.zeros((x_np.shape[0], self.output_dim), dtype=np.float64)
        _check(lib().tds_hip_forward_zero_host(self.h, x_np.shape[0], x_np.ctypes.data, y_np.ctypes.data))
        return y_np

    def set_timing(self, on: bool):
        _check(lib().tds_hip_set_timing(self.h, 1 if on else 0))

    def last_kernel_ms(self) -> float:
        ms = C.c_float()
        _check(lib().tds_hip_last_kernel_ms(self.h, C.byref(ms)))
        return float(ms.value)

    PHASES = ["A load+PD", "B jcalc", "C kinematics sweep", "I narrowphase + visuals + D inertias",
              "E composite inertia + bias force sweep", "G mass matrix rows", "H LDLt",
              "F forward dynamics solve", "(barrier)",
              "J jacobian rows", "K row solves", "L PGS", "M/N pack"]

    def profile_phases(self):
        """Shader-clock cycles spent by workgroup 0 in each phase of one step (diagnostic)."""
        buf = (C.c_longlong * 14)()
        _check(lib().tds_hip_profile_phases(self.h, buf, 14))
        st = list(buf)
        return {name: st[i + 1] - st[i] for i, name in enumerate(self.PHASES)}

    def profile_phases_two_waves(self):
        """Raw stamp timelines (shader-clock cycles since the main wavefront's first stamp) of both wavefronts of
        workgroup 0 in the two-wavefront form; None when that form does not serve this grid."""
        nb = (self.num_envs + self.kernel_info()["envs_per_block"] - 1) // self.kernel_info()["envs_per_block"]
        buf = (C.c_longlong * (28 + 2 * nb))()
        _check(lib().tds_hip_profile_phases(self.h, buf, 28 + 2 * nb))
        st = list(buf)
        if st[14] == 0:
            return None
        t0 = st[0]
        # 23, 24: 100 MHz wall clock at workgroup 0's first / last stamp; 25, 26: shader clock at the LAST workgroup's
        # first / last stamp; 27: wall clock at its last stamp
        extra = dict(wg0_wall_us=(st[24] - st[23]) / 100.0, last_wg_start=st[25] - t0, last_wg_end=st[26] - t0,
                     last_wg_end_wall_us=(st[27] - st[23]) / 100.0,
                     wg_start_us=[(v - st[23]) / 100.0 for v in st[28::2]], wg_end_us=[(v - st[23]) / 100.0 for v in st[29::2]])
        return [v - t0 for v in st[:14]], [v - t0 for v in st[14:23]], extra

    def single_step_kernel(self):
        """which kernel a plain single step runs: ("general" | "quad16" | "oct8" | "chain8", lanes per environment, LDS bytes per environment)"""
        a, b = C.c_int(), C.c_int()
        lib().tds_hip_single_step_kernel.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        k = lib().tds_hip_single_step_kernel(self.h, C.byref(a), C.byref(b))
        return {1: "quad16", 2: "oct8", 3: "chain8"}.get(k, "general"), a.value, b.value

    def kernel_info(self):
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        _check(lib().tds_hip_kernel_info(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return dict(lds_bytes_per_env=a.value, lanes_per_env=b.value, envs_per_block=c.value)


class HipShard:
    """This rank's shard of a global batch of environments + the per-policy-step RCCL all-gather of the
    [obs | reward | done] records (tds_hip_shard_*).  ``sim`` is the shard's HipSim (state upload, reset,
    auto-reset ... as usual); ``step(actions)`` steps the shard and submits the exchange on the library's
    communication stream; ``gathered()`` returns the most recently exchanged records as a zero-copy tensor
    [world, block, n_local, obs_dim + 2] in the wire dtype (the current torch stream waits for the exchange)."""

    def __init__(self, m: _model.Model, global_envs: int, rank: int = 0, world: int = 1, device: int = 0,
                 dtype: str = "f64", unique_id: bytes | None = None, wire_dtype: str = "f32", block: int = 1,
                 options: dict | None = None):
        import torch

        if not torch.cuda.is_available():
            raise TdsHipError("no HIP device visible (the HIP path has no CPU fallback)")
        self._model = m.copy()
        h = C.c_void_p()
        idbuf = None
        if unique_id is not None:
            assert len(unique_id) == 128
            idbuf = C.create_string_buffer(bytes(unique_id), 128)
        wire = _model.TDS_DTYPE_F64 if wire_dtype in ("f64", "float64") else _model.TDS_DTYPE_F32
        _check(lib().tds_hip_shard_create(C.byref(self._model), int(global_envs), int(rank), int(world), int(device),
                                          dtype_code(dtype), idbuf, wire, C.byref(h)))
        self.h = h
        self.rank, self.world, self.device = int(rank), int(world), int(device)
        self.n_local = lib().tds_hip_shard_local_envs(self.h)
        self.wire_torch_dtype = torch.float64 if lib().tds_hip_shard_wire_bytes(self.h) == 8 else torch.float32
        self.sim = HipSim(m, self.n_local, device=device, dtype=dtype,
                          _handle=C.c_void_p(lib().tds_hip_shard_sim(self.h)), _owner=self)
        self.block = 1
        for k, v in (options or {}).items():  # (run-time options of the shard live in its sim handle)
            self.sim.set_option(k, v)
        if block != 1:
            self.set_block(block)

    @staticmethod
    def unique_id() -> bytes:
        buf = C.create_string_buffer(128)
        _check(lib().tds_hip_shard_unique_id(buf))
        return bytes(buf.raw)

    @staticmethod
    def rccl_version() -> int:
        return int(lib().tds_hip_shard_rccl_version())

    def set_block(self, steps_per_exchange: int):
        _check(lib().tds_hip_shard_set_block(self.h, int(steps_per_exchange)))
        self.block = int(steps_per_exchange)

    def step(self, actions=None, substeps: int = 1):
        ap = None
        if actions is not None:
            assert actions.is_cuda and actions.dtype == self.sim.torch_dtype and actions.is_contiguous()
            assert tuple(actions.shape) == (self.n_local, self.sim.model.action_dim)
            ap = C.c_void_p(actions.data_ptr())
        _check(lib().tds_hip_shard_step(self.h, ap, int(substeps)))

    def step_many(self, actions, n_steps: int, first_block: int = 0, prepare_only: bool = False):
        """n_steps steps + their exchanges as one hipGraph launch; ``actions`` [B, n_local, action_dim] or None.
        prepare_only: capture + instantiate the graph, run nothing."""
        ap, nb = None, 1
        if actions is not None:
            assert actions.is_cuda and actions.dtype == self.sim.torch_dtype and actions.is_contiguous()
            assert actions.dim() == 3 and tuple(actions.shape[1:]) == (self.n_local, self.sim.model.action_dim)
            ap, nb = C.c_void_p(actions.data_ptr()), int(actions.shape[0])
        f = lib().tds_hip_shard_step_many_prepare if prepare_only else lib().tds_hip_shard_step_many
        _check(f(self.h, ap, nb, int(first_block), int(n_steps)))

    def flush(self):
        _check(lib().tds_hip_shard_flush(self.h))

    EXCHANGE_FORMS = {0: "none", 1: "rccl_per_step", 2: "rccl_group_after_launch", 3: "rccl_per_slot", 4: "peer_stores", 5: "peer_copy"}

    def exchange_form(self) -> str:
        """which exchange the most recent step / step_many ran (tds_hip_shard_exchange_form)"""
        lib().tds_hip_shard_exchange_form.argtypes = [C.c_void_p]
        return self.EXCHANGE_FORMS.get(int(lib().tds_hip_shard_exchange_form(self.h)), "?")

    def peer_count(self) -> int:
        """ranks this shard stores its records to under the peer-store exchange; -1: not in use"""
        lib().tds_hip_shard_peer_count.argtypes = [C.c_void_p]
        return int(lib().tds_hip_shard_peer_count(self.h))

    def gathered(self):
        import torch

        ptr, blk = C.c_void_p(), C.c_int()
        st = torch.cuda.current_stream(self.device)
        _check(lib().tds_hip_shard_gathered(self.h, C.c_void_p(st.cuda_stream), C.byref(ptr), C.byref(blk)))
        shape = (self.world, blk.value, self.n_local, self.sim.obs_dim + 2)

        class _Holder:
            pass

        hld = _Holder()
        hld.__cuda_array_interface__ = {
            "shape": shape, "typestr": "<f8" if self.wire_torch_dtype == torch.float64 else "<f4",
            "data": (int(ptr.value), False), "version": 2, "strides": None,
        }
        t = torch.as_tensor(hld, device=f"cuda:{self.device}")
        t._tds_owner = self
        return t

    def gathered_step(self, steps_back: int):
        """ring exchange: gathered records [world, n_local, obs_dim + 2] of the step ``steps_back`` before the most recently
        submitted one, while it is still in the ring (tds_hip_shard_gathered_step)"""
        import torch

        ptr = C.c_void_p()
        st = torch.cuda.current_stream(self.device)
        lib().tds_hip_shard_gathered_step.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]
        _check(lib().tds_hip_shard_gathered_step(self.h, int(steps_back), C.c_void_p(st.cuda_stream), C.byref(ptr)))
        return wrap_device_pointer(ptr.value, (self.world, self.n_local, self.sim.obs_dim + 2), self.wire_torch_dtype,
                                   self.device, owner=self)

    def close(self):
        if getattr(self, "h", None):
            self.sim.h = None
            lib().tds_hip_shard_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class RigidBodySim:
    """N independent worlds of free rigid bodies (spheres, planes) on one GPU — World::step of the
    reference for tds::RigidBody objects.  ``state`` is a zero-copy torch view
    [N, num_bodies, 13]: position | quaternion xyzw | linear velocity | angular velocity."""

    def __init__(self, m: _model.RbModel, num_worlds: int, device: int = 0, dtype: str = "f64"):
        import torch

        if not torch.cuda.is_available():
            raise TdsHipError("no HIP device visible (the HIP path has no CPU fallback)")
        self.model, self.num_worlds, self.device = m, int(num_worlds), int(device)
        self.dtype = _model.TDS_DTYPE_F64 if dtype in ("f64", "float64") else _model.TDS_DTYPE_F32
        self.torch_dtype = torch.float64 if self.dtype == _model.TDS_DTYPE_F64 else torch.float32
        h = C.c_void_p()
        rc = lib().tds_rb_create(C.byref(m), self.num_worlds, self.device, self.dtype, C.byref(h))
        if rc != TDS_OK:
            raise TdsHipError(f"tds_rb_create error {rc}: {lib().tds_rb_last_error().decode()}")
        self.h = h
        lib().tds_rb_set_stream(self.h, C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream))
        self.state = HipSim._wrap(self, lib().tds_rb_state_device(self.h),
                                  (self.num_worlds, m.num_bodies, _model.TDS_RB_STATE))

    def jvp(self, s0, v=None, steps: int = 1, params=(), theta=None):
        """(s_T, jv): `steps` World::steps from s0 [N, num_bodies, 13] (any N) and jv = (d s_T / d [s0 | theta]) v
        [N, K, num_bodies, 13] for directions v [N, K, num_bodies * 13 + p] (or [N, num_bodies * 13 + p]: K = 1, jv
        [N, num_bodies, 13]); v None: jv None.  params: a selection of ("mass", body), ("gravity", comp), ("friction",),
        ("restitution",) (hip_backend.param_spec); theta None (the model's values), [p] or [N, p].  The resident state
        is not touched.  f64 handles only (async on the handle's stream)."""
        # (k = 0 directions: v and jv have no extent, their pointers are NULL, and the call is the primal one)
        return _rb_jvp(_DevArrays, functools.partial(lib().tds_rb_jvp, self.h), self.model, s0, steps, v, params, theta)

    def vjp(self, s0, gs, steps: int, params=(), theta=None, every=None, tape_cap: int = 0, work_bytes: int = 0):
        """(s, gs0, gtheta): `steps` World::steps from s0 [N, num_bodies, 13] (any N), the state after every `every`-th
        step recorded in s [N, n_rec, num_bodies, 13] (every None: the final state alone), and the gradients of
        sum(gs * s) in s0 (gs0 [N, num_bodies, 13]) and theta (gtheta [N, p]) in reverse mode (tds_rb_vjp).  gs: the
        cotangent on the records, [N, n_rec, num_bodies * 13] or any shape of that many entries.  params, theta: as
        jvp's.  tape_cap: entries one step's tape of one world may hold (0: the model's bound); work_bytes: the bound on
        the work buffer (0: 8 GiB): it decides windows and passes, never the results (hip_backend.rb_vjp_plan).  A world
        that overflows its tape gets NaN gradients and the call raises.  The resident state is not touched.  f64
        handles only; the call waits for its launches."""
        call = functools.partial(lib().tds_rb_vjp, self.h)
        return _rb_vjp(_DevArrays, call, self.model, s0, steps, gs, params, theta, every, tape_cap, work_bytes)

    def jacobian(self, s0, steps: int, wrt, params=(), theta=None):
        """dense d s_T / d [s0 entries wrt | theta]: [N, num_bodies * 13, len(wrt) + p] from unit directions.  wrt: a
        list of (body, comp) entries of the state (comp 0..12: position, quaternion xyzw, linear, angular velocity)."""
        import torch

        nb = self.model.num_bodies
        ns = nb * _model.TDS_RB_STATE
        s0 = s0.reshape(-1, nb, _model.TDS_RB_STATE)
        n, p = s0.shape[0], len(params)
        v = rb_directions(nb, wrt, p, device=s0.device).expand(n, -1, -1)
        _, jv = self.jvp(s0, v, steps, params, theta)
        return jv.reshape(n, -1, ns).transpose(1, 2)

    def step(self, steps: int = 1):
        rc = lib().tds_rb_step(self.h, int(steps))
        if rc != TDS_OK:
            raise TdsHipError(f"tds_rb_step error {rc}: {lib().tds_rb_last_error().decode()}")

    def close(self):
        if getattr(self, "h", None):
            lib().tds_rb_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def rb_directions(num_bodies: int, wrt, p: int = 0, device=None):
    """unit directions [len(wrt) + p, num_bodies * 13 + p]: one per state entry (body, comp) of wrt, then one per
    parameter"""
    import torch

    ns = num_bodies * _model.TDS_RB_STATE
    cols = []
    for b, c in wrt:
        if not (0 <= b < num_bodies and 0 <= c < _model.TDS_RB_STATE):
            raise ValueError(f"wrt entry {(b, c)} out of range ({num_bodies} bodies, {_model.TDS_RB_STATE} comps)")
        cols.append(b * _model.TDS_RB_STATE + c)
    cols += [ns + j for j in range(p)]
    v = torch.zeros((len(cols), ns + p), dtype=torch.float64, device=device)
    if cols:
        v[torch.arange(len(cols)), torch.tensor(cols)] = 1.0
    return v
