"""Shared inputs of the per-instance reference curves' tests (test_curves_host.py, test_curves_gpu.py).

Shapes: N = 10 and n_steps_tracking = 12, so a curve has L = 23 columns and k_policy_traj serves 11 threads per instance -- B = 5 is
55 threads (less than a wavefront, instances straddling inside it), B = 13 is 143 threads (instances straddling wavefronts and blocks,
and an odd batch for the two-instances-per-wavefront interior point).  Three distinct curves are dealt round-robin over the
instances; ``current_step`` differs per instance, with one instance at 0 and one at L + 3 (clamped to the last column), and the
stepping mask has holes."""
import functools

import numpy as np

N, STEPS_TRACKING = 10, 12
L = STEPS_TRACKING + 1 + N


def params(**over):
    from safe_mpc_amd.parser import Parameters
    par = Parameters({}, 'z1')
    par.nq, par.n_dof_safe_set, par.net_size, par.N, par.nlp_max_iter, par.back_hor = 6, 6, [12, 256, 1], N, 200, 10
    par.n_steps_tracking = par.n_steps = STEPS_TRACKING
    for k, v in over.items():
        setattr(par, k, v)
    return par


@functools.lru_cache(maxsize=None)
def three_curves():
    """[3, 3, L]: the "8" at its shipped place, a larger one moved by centimetres, a smaller and faster one moved the other way"""
    from safe_mpc_amd.tracking import tracking_curves
    par = params()
    off = np.asarray(par.offset_traj, float)
    c = tracking_curves(par, '8', offsets=off + np.array([[0.0, 0.0, 0.0], [-0.04, 0.03, 0.05], [0.03, -0.05, 0.02]]),
                        sizes=par.dim_shape_8 * np.array([1.0, 1.2, 0.8]), v_max=par.vel_max_traj * np.array([1.0, 1.0, 1.5]))
    assert c.shape == (3, 3, L)
    c.setflags(write=False)
    return c


def owner(B):
    return np.arange(B) % 3


def dealt(B):
    return np.ascontiguousarray(three_curves()[owner(B)])


def current_steps(B):
    """different per instance; instance 1 at 0, the last one at L + 3"""
    cs = (3 + 5 * np.arange(B)) % (L - 2)
    cs[1], cs[B - 1] = 0, L + 3
    return cs.astype(np.int64)


def stepping(B):
    m = np.ones(B, bool)
    m[[2, B - 2]] = False
    if B > 8:
        m[7] = False
    return m


def p_statement(curves, cs, n_nodes=N + 1):
    """p[b, i, :3] = curves[b, :, clamp(cs[b] + i, 0, L - 1)]"""
    col = np.clip(cs[:, None] + np.arange(n_nodes)[None, :], 0, curves.shape[2] - 1)
    return np.stack([curves[b][:, col[b]].T for b in range(len(cs))])


@functools.lru_cache(maxsize=None)
def loop_curves():
    """[2, 3, L] for the closed loops: the "8" at its shipped place and one moved by 15 cm along every axis -- on the CPU oracle the
    two 6-step 'htwa' loops from the same starts are then 8.6 apart in u (largest |u| 32) and 0.17 in x"""
    from safe_mpc_amd.tracking import tracking_curves
    par = params()
    c = tracking_curves(par, '8', offsets=np.asarray(par.offset_traj, float) + np.array([[0.0, 0.0, 0.0], [-0.15, 0.15, 0.15]]))
    c.setflags(write=False)
    return c
