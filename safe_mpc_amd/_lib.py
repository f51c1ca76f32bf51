"""Loads the HIP engine (csrc/libsmpc_hip.so) through ctypes and declares the C ABI of include/smpc.h.

There is no CPU fallback: if the library is missing or no MI355X is visible, creating a solver raises.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

from .problem import Joint, KalmanParams, NodeEval, ProblemDesc

_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'csrc')
# SMPC_HIP_LIB selects another build of the SAME engine (diagnostic builds of scripts/qp_phase_profile.py)
LIB_PATH = os.environ.get('SMPC_HIP_LIB') or os.path.join(_CSRC, 'libsmpc_hip.so')

SYMBOLS = ['smpc_create', 'smpc_destroy', 'smpc_abi_version', 'smpc_last_error', 'smpc_set_mlp', 'smpc_set_horizon',
           'smpc_set_stage_bounds', 'smpc_set_slack_weights', 'smpc_set_instance_bounds', 'smpc_solve_batch', 'smpc_eval_nodes', 'smpc_guess_correction',
           'smpc_provide_control', 'smpc_check_trajectory', 'smpc_plant_step', 'smpc_rollout_batch', 'smpc_sync', 'smpc_stream',
           'smpc_enable_timing', 'smpc_get_timing', 'smpc_get_qp_timing', 'smpc_get_qp_wave_stats', 'smpc_policy_step', 'smpc_loop_pre',
           'smpc_loop_post', 'smpc_loop_apply_backup', 'smpc_loop_classify_aborts', 'smpc_get_timing_history',
           'smpc_accumulate_stats', 'smpc_set_mlp_activation', 'smpc_set_qp_mode', 'smpc_set_qp_crew', 'smpc_merit_terms', 'smpc_sqp_batch', 'smpc_check_guess',
           'smpc_score_rollout', 'smpc_set_instance_scene', 'smpc_ik_batch', 'smpc_ray_update', 'smpc_set_instance_curves',
           'smpc_set_instance_scene_track', 'smpc_set_scene_clock', 'smpc_set_mlp_context', 'smpc_set_instance_context',
           'smpc_set_instance_models', 'smpc_set_instance_context_track', 'smpc_set_instance_world_track', 'smpc_forecast_scene',
           'smpc_set_instance_observed_track', 'smpc_forecast_scene_fit', 'smpc_forecast_scene_poly', 'smpc_set_instance_row_bounds',
           'smpc_forecast_row_margin', 'smpc_get_instance_row_bounds', 'smpc_forecast_scene_kalman', 'smpc_kalman_row_margin']


class EngineError(RuntimeError):
    pass


_vp = C.c_void_p


class PolicyParams(C.Structure):
    """smpc_policy_params (include/smpc.h)"""
    _fields_ = [('kind', C.c_int32), ('abort_flag', C.c_int32), ('collision_first_node', C.c_int32), ('reserved0', C.c_int32),
                ('tol_x', C.c_double), ('alpha', C.c_double), ('tol_safe', C.c_double), ('tube', C.c_double),
                ('x_min', _vp), ('x_max', _vp), ('row_lb_chk', _vp), ('row_ub_chk', _vp), ('stage_lo', _vp), ('stage_hi', _vp)]


class PolicyState(C.Structure):
    """smpc_policy_state"""
    _fields_ = [(k, _vp) for k in ('x_guess', 'u_guess', 'x_temp', 'u_temp', 'p', 'x_viable', 'fails', 'current_step', 'r',
                                   'status', 'qp_iter', 'traj')] + [('traj_len', C.c_int64)]


class LoopState(C.Structure):
    """smpc_loop_state"""
    _fields_ = [(k, _vp) for k in ('x_cur', 'alive', 'sa', 'collided', 'ja', 'last_x', 'last_u', 'x_abort', 'u_abort', 'step',
                                   'x_log', 'u_log', 'r_log', 'resumed')]


class SqpOpts(C.Structure):
    """smpc_sqp_opts; the defaults are those of closed_loop.generate_guess"""
    _fields_ = [('max_iter', C.c_int32), ('reserved0', C.c_int32), ('tol', C.c_double), ('armijo', C.c_double),
                ('alpha_reduction', C.c_double), ('alpha_min', C.c_double), ('mu0', C.c_double), ('mu_max', C.c_double)]

    def __init__(self, max_iter=1, tol=1e-6, armijo=1e-4, alpha_reduction=0.7, alpha_min=0.05, mu0=10.0, mu_max=1e8):
        super().__init__(int(max_iter), 0, float(tol), float(armijo), float(alpha_reduction), float(alpha_min), float(mu0), float(mu_max))


class SqpState(C.Structure):
    """smpc_sqp_state: per-instance arrays [B]"""
    FIELDS = (('mu', 'f8'), ('done', 'u1'), ('status', 'i4'), ('alpha', 'f8'), ('merit_before', 'f8'), ('merit', 'f8'),
              ('violation', 'f8'), ('updated', 'u1'), ('iters', 'i4'), ('qp_iter_total', 'i4'))
    _fields_ = [(k, _vp) for k, _ in FIELDS]


class GuessCheck(C.Structure):
    """smpc_guess_check: tolerances, the two node choices and HOST pointers to the bounds of smpc_check_guess"""
    _fields_ = [('tol_x', C.c_double), ('tol_tau', C.c_double), ('tol_dyn', C.c_double), ('tol_safe', C.c_double), ('alpha', C.c_double),
                ('collision_first_node', C.c_int32), ('safe_node', C.c_int32),
                ('x_min', _vp), ('x_max', _vp), ('tau_min', _vp), ('tau_max', _vp), ('row_lb_chk', _vp), ('row_ub_chk', _vp)]


class ScoreParams(C.Structure):
    """smpc_score_params: what smpc_score_rollout scores against; the small arrays are HOST pointers, traj follows on_device"""
    _fields_ = [('alpha', C.c_double), ('tol_safe', C.c_double), ('want_safe', C.c_int32), ('reserved0', C.c_int32),
                ('x_min', _vp), ('x_max', _vp), ('row_lb_chk', _vp), ('row_ub_chk', _vp), ('ee_ref', _vp), ('traj', _vp),
                ('traj_len', C.c_int64)]


class IkParams(C.Structure):
    """smpc_ik_params: iteration settings and HOST pointers to the bounds of smpc_ik_batch"""
    _fields_ = [('max_iter', C.c_int32), ('reserved0', C.c_int32), ('tol_ee', C.c_double), ('push', C.c_double), ('damping', C.c_double),
                ('damping_accept', C.c_double), ('damping_reject', C.c_double), ('damping_min', C.c_double), ('damping_max', C.c_double),
                ('q_lo', _vp), ('q_hi', _vp), ('row_lb', _vp), ('row_ub', _vp)]


class RayOpts(C.Structure):
    """smpc_ray_opts"""
    _fields_ = [('bisect', C.c_int32), ('budget', C.c_int32), ('tol_term', C.c_double), ('mu0', C.c_double)]


class RayState(C.Structure):
    """smpc_ray_state: per-ray arrays [B] (q, d: [B, nq]; x_cert, u_cert: a trajectory per ray)"""
    FIELDS = (('q', 'f8'), ('d', 'f8'), ('lo', 'f8'), ('hi', 'f8'), ('s', 'f8'), ('trial', 'i4'), ('kind', 'i4'), ('open', 'u1'),
              ('x_cert', 'f8'), ('u_cert', 'f8'), ('iters_total', 'i4'))
    _fields_ = [(k, _vp) for k, _ in FIELDS]


RAY_OPEN, RAY_DEAD, RAY_SATURATED, RAY_BRACKETED = 0, 1, 2, 3      # SMPC_RAY_* of include/smpc.h


def build(force=False):
    """Compile the engine for gfx950 with hipcc (cross-compiles without a GPU)."""
    srcs = [os.path.join(_CSRC, f) for f in os.listdir(_CSRC) if f.endswith(('.hip', '.hpp'))]
    srcs.append(os.path.join(_CSRC, '..', '..', 'include', 'smpc.h'))
    if not force and os.path.exists(LIB_PATH) and all(os.path.getmtime(LIB_PATH) >= os.path.getmtime(s) for s in srcs):
        return LIB_PATH
    subprocess.check_call(['make', '-C', _CSRC, '-B', 'libsmpc_hip.so'])
    return LIB_PATH


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise EngineError(f'{LIB_PATH} not found: run `python -c "import __graft_entry__ as g; g.build()"` '
                          f'(or make -C safe_mpc_amd/csrc); the engine has no CPU fallback')
    L = C.CDLL(LIB_PATH)
    vp, i32p, dp = C.c_void_p, C.POINTER(C.c_int32), C.c_void_p
    L.smpc_create.argtypes = [C.POINTER(ProblemDesc), C.c_int, C.POINTER(vp)]
    L.smpc_destroy.argtypes = [vp]
    L.smpc_destroy.restype = None
    L.smpc_last_error.argtypes = [vp]
    L.smpc_last_error.restype = C.c_char_p
    L.smpc_set_mlp.argtypes = [vp, C.c_int, i32p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int]
    L.smpc_set_horizon.argtypes = [vp, C.c_int]
    L.smpc_set_stage_bounds.argtypes = [vp, dp, dp]
    L.smpc_set_slack_weights.argtypes = [vp, dp]
    L.smpc_set_instance_bounds.argtypes = [vp, C.c_int, dp, dp, C.c_int]
    L.smpc_set_instance_row_bounds.argtypes = [vp, C.c_int, dp, dp, C.c_int]
    L.smpc_set_instance_scene.argtypes = [vp, C.c_int, dp, C.c_int]
    L.smpc_set_instance_scene_track.argtypes = [vp, C.c_int, C.c_int64, dp, C.c_int]
    L.smpc_set_scene_clock.argtypes = [vp, dp]
    L.smpc_set_instance_world_track.argtypes = [vp, C.c_int, C.c_int64, dp, C.c_int]
    L.smpc_forecast_scene.argtypes = [vp, C.c_int, C.c_int, C.c_int, dp]
    L.smpc_set_instance_observed_track.argtypes = [vp, C.c_int, C.c_int64, dp, C.c_int]
    L.smpc_forecast_scene_fit.argtypes = [vp, C.c_int, C.c_int, C.c_int, dp]
    L.smpc_forecast_scene_poly.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, dp]
    L.smpc_forecast_row_margin.argtypes = [vp, C.c_int, C.c_int, C.c_int] + [C.c_double] * 5
    L.smpc_get_instance_row_bounds.argtypes = [vp, C.c_int, dp, dp, C.c_int]
    if hasattr(L, 'smpc_forecast_scene_kalman'):      # (an older build named by SMPC_HIP_LIB: the solver's methods raise)
        L.smpc_forecast_scene_kalman.argtypes = [vp, C.c_int, C.POINTER(KalmanParams), dp, C.c_int, C.c_int, dp]
        L.smpc_kalman_row_margin.argtypes = [vp, C.c_int, C.POINTER(KalmanParams), dp] + [C.c_double] * 4
    L.smpc_set_instance_curves.argtypes = [vp, C.c_int, C.c_int64, dp, C.c_int]
    L.smpc_solve_batch.argtypes = [vp, C.c_int, dp, dp, dp, dp, dp, dp, dp, dp, C.c_int]
    L.smpc_eval_nodes.argtypes = [vp, C.c_int, dp, dp, dp, dp, C.c_int]
    L.smpc_guess_correction.argtypes = [vp, C.c_int, dp, dp, C.c_int]
    L.smpc_provide_control.argtypes = [vp, C.c_int, dp, dp, dp, dp, dp, dp, C.c_int]
    L.smpc_check_trajectory.argtypes = [vp, C.c_int, C.c_int, dp, dp, dp, C.c_double, dp, dp, C.c_double, C.c_double,
                                        dp, dp, C.c_int]
    L.smpc_plant_step.argtypes = [vp, C.c_int, dp, dp, dp, dp, dp, dp, C.c_int]
    L.smpc_rollout_batch.argtypes = [vp, C.c_int, C.c_int, dp, dp, dp, dp, dp, dp, dp, dp, dp, dp, C.c_int]
    L.smpc_sync.argtypes = [vp]
    L.smpc_stream.argtypes = [vp]
    L.smpc_stream.restype = C.c_void_p
    L.smpc_enable_timing.argtypes = [vp, C.c_int]
    L.smpc_get_timing.argtypes = [vp, C.POINTER(C.c_float)]
    L.smpc_get_qp_timing.argtypes = [vp, C.POINTER(C.c_float)]
    L.smpc_get_qp_wave_stats.argtypes = [vp, C.POINTER(C.c_double)]
    L.smpc_policy_step.argtypes = [vp, C.c_int, C.POINTER(PolicyParams), C.POINTER(PolicyState), dp, dp, dp, dp, dp, dp]
    L.smpc_loop_pre.argtypes = [vp, C.c_int, C.c_int, C.POINTER(LoopState), dp, dp, dp, dp]
    L.smpc_loop_apply_backup.argtypes = [vp, C.c_int, C.c_int, C.POINTER(LoopState), C.c_int, dp, dp, dp, dp, dp, dp, dp]
    L.smpc_loop_post.argtypes = [vp, C.c_int, C.POINTER(PolicyParams), C.POINTER(LoopState), dp, dp, dp]
    L.smpc_loop_classify_aborts.argtypes = [vp, C.c_int, C.POINTER(LoopState), C.c_int, dp, dp]
    L.smpc_get_timing_history.argtypes = [vp, C.c_int, C.POINTER(C.c_float)]
    L.smpc_accumulate_stats.argtypes = [vp, C.c_int, dp, dp, dp]
    L.smpc_set_mlp_activation.argtypes = [vp, C.c_int]
    L.smpc_set_mlp_context.argtypes = [vp, C.c_int, dp, dp, dp, dp, C.c_int]
    L.smpc_set_instance_context.argtypes = [vp, C.c_int, dp, C.c_int]
    L.smpc_set_instance_context_track.argtypes = [vp, C.c_int, C.c_int64, dp, C.c_int]
    L.smpc_set_instance_models.argtypes = [vp, C.c_int, dp, C.c_int]
    L.smpc_set_qp_mode.argtypes = [vp, C.c_int]
    if hasattr(L, 'smpc_set_qp_crew'):      # (an older build named by SMPC_HIP_LIB, in an A/B run: a wavefront per pair, no setter)
        L.smpc_set_qp_crew.argtypes = [vp, C.c_double, C.c_int]
    L.smpc_merit_terms.argtypes = [vp, C.c_int, dp, dp, dp, dp, dp, dp, dp, dp, dp, C.c_int]
    L.smpc_sqp_batch.argtypes = [vp, C.c_int, C.POINTER(SqpOpts), dp, dp, dp, dp, C.POINTER(SqpState), C.c_int]
    L.smpc_check_guess.argtypes = [vp, C.c_int, dp, dp, C.POINTER(GuessCheck), dp, dp, dp, C.c_int]
    L.smpc_score_rollout.argtypes = [vp, C.c_int, C.c_int, dp, dp, dp, dp, C.POINTER(ScoreParams), dp, dp, dp, C.c_int]
    L.smpc_ik_batch.argtypes = [vp, C.c_int, C.c_int, dp, dp, C.POINTER(IkParams), dp, dp, dp, dp, C.c_int]
    L.smpc_ray_update.argtypes = [vp, C.c_int, C.POINTER(RayOpts), C.POINTER(RayState), C.POINTER(SqpState), dp, dp, dp, dp, dp, C.c_int]
    _lib = L
    return L
