"""Shared inputs of the safe-set data tests (test_safe_set_data_host.py, test_safe_set_data_gpu.py): the Z1-class backup OCP at
N = 8, the random and the designed rays, and the certificate checks recomposed from the CPU oracle.  Results that more than one
test needs are computed once per process and handed out read-only."""
import functools

import numpy as np

from conftest import constant_guess, sample_instances

N, BISECT, BUDGET, CHECK_EVERY = 8, 5, 30, 5
NQ = 6
RANDOM_BRACKETED = [0, 2, 12]          # of the random rays, on the CPU double and on the engine; the other 13 saturate


def ray_params():
    from safe_mpc_amd.parser import Parameters
    par = Parameters({}, 'z1')
    par.nq, par.n_dof_safe_set, par.net_size = NQ, NQ, [2 * NQ, 256, 1]
    return par


@functools.lru_cache(maxsize=None)
def backup_problem():
    from safe_mpc_amd.problem import OcpProblem
    par = ray_params()
    return par, OcpProblem(par, 'backup', 'zero', N=N)


def _s_hi(prob, d):
    from safe_mpc_amd.safe_set_data import velocity_box_along
    return velocity_box_along(prob, d)


@functools.lru_cache(maxsize=None)
def random_rays():
    """16 rays well inside the box: on the CPU double 0 dead, 3 bracketed (rays 0, 2, 12), 13 saturated"""
    par, prob = backup_problem()
    q = sample_instances(prob, 16, seed=1, margin=0.2)[:, :NQ].copy()
    d = np.random.default_rng(3).standard_normal((16, NQ))
    d /= np.linalg.norm(d, axis=1)[:, None]
    return _frozen(q, d, _s_hi(prob, d))


@functools.lru_cache(maxsize=None)
def designed_rays():
    """12 rays at one base configuration with joint j moved to x_max[j] - 0.01: rows 2 j and 2 j + 1 point into (+e_j) and away
    from (-e_j) that limit"""
    par, prob = backup_problem()
    base = sample_instances(prob, 12, seed=1)[0, :NQ]
    q, d = np.zeros((12, NQ)), np.zeros((12, NQ))
    for j in range(NQ):
        for k, sign in enumerate((1.0, -1.0)):
            q[2 * j + k] = base
            q[2 * j + k, j] = prob.x_max[j] - 0.01
            d[2 * j + k, j] = sign
    return _frozen(q, d, _s_hi(prob, d))


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _freeze_result(res):
    for v in res.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return res


def double_controller(batch):
    from fake_solver import make_double_controller
    return make_double_controller('backup', ray_params(), batch, N=N)


def engine_controller(batch):
    """the backup controller on the engine with the QP form pinned (a ray's SQP must not depend on the batch width)"""
    from safe_mpc_amd.controller import SafeBackupController
    ctrl = SafeBackupController(ray_params(), batch, N=N)
    ctrl.ocp_solver.set_qp_mode('throughput')
    return ctrl


@functools.lru_cache(maxsize=None)
def host_labels(which):
    """label_rays on the CPU oracle double, once per process"""
    from safe_mpc_amd.safe_set_data import label_rays
    q, d, s_hi = random_rays() if which == 'random' else designed_rays()
    return _freeze_result(label_rays(double_controller(len(q)), q, d, s_hi, bisect=BISECT, budget=BUDGET, check_every=CHECK_EVERY))


def certificate_report(q, d, res):
    """What a certificate has to meet, recomposed from Oracle.eval_nodes / Oracle.guess_correction (not through check_guess), for the
    rays that are not dead: a dict of [m] arrays of the values tested and the thresholds they are tested against."""
    from oracle.oracle import Oracle
    from safe_mpc_amd.safe_set_data import DEAD
    par, prob = backup_problem()
    o = Oracle(prob)
    live = res['kind'] != DEAD
    x, u = np.array(res['x_cert'][live]), np.array(res['u_cert'][live])
    m, nr = x.shape[0], int(prob.desc.n_rows)
    start = np.hstack([q[live], res['label'][live, None] * d[live]])
    _, _, p = constant_guess(prob, x[:, 0], alpha=par.alpha)
    ev = o.eval_nodes(x, u, p)
    rep = {'start': np.abs(x[:, 0] - start).max(1),
           'box': np.maximum(prob.x_min - x, x - prob.x_max).reshape(m, -1).max(1),
           'torque': np.maximum(prob.tau_min - ev['tau'][:, :N, :NQ], ev['tau'][:, :N, :NQ] - prob.tau_max).reshape(m, -1).max(1),
           'dynamics': np.linalg.norm((x - o.guess_correction(x, u)).reshape(m, -1), axis=1),
           'v_end': np.abs(x[:, N, NQ:]).max(1)}
    if nr:
        rv = ev['row_val'][:, :, :nr]
        rep['rows'] = np.maximum(prob.row_check[:, 0] - rv, rv - prob.row_check[:, 1]).reshape(m, -1).max(1)
    return rep, {'start': 1e-12, 'box': par.tol_x, 'torque': par.tol_tau, 'dynamics': par.tol_dyn * np.sqrt(N + 1), 'v_end': par.tol_x,
                 'rows': 0.0}


def assert_certificates(q, d, res):
    rep, thr = certificate_report(q, d, res)
    for k, v in rep.items():
        print(f'certificates: worst {k} {v.max():.3e} (threshold {thr[k]:.3e})')
    for k, v in rep.items():
        if k == 'dynamics':
            assert np.all(v < thr[k]), (k, v)
        else:
            assert np.all(v <= thr[k]), (k, v)


def assert_designed_order(res):
    """label(+e_j) <= label(-e_j) for every joint; smaller by more than two bisection cells for joints 0, 1, 2"""
    _, _, s_hi = designed_rays()
    lab = np.where(np.isnan(res['label']), -np.inf, res['label'])
    print('designed rays: labels (+, -) per joint', [(round(float(lab[2 * j]), 3), round(float(lab[2 * j + 1]), 3)) for j in range(NQ)])
    for j in range(NQ):
        assert lab[2 * j] <= lab[2 * j + 1], j
    for j in range(3):
        cell = s_hi[2 * j] / 2 ** BISECT
        assert lab[2 * j + 1] - lab[2 * j] > 2 * cell, (j, lab[2 * j], lab[2 * j + 1], cell)
