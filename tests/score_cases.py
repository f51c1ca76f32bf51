"""Logs with planted extremes for the tests of smpc_score_rollout (test_score_host.py checks the generator on the oracle side,
test_score_gpu.py runs the kernels on it).  Not a test module."""
import functools

import numpy as np

from conftest import halton, make_problem, make_problem_fr7, sample_instances

SEED = 3
B_GPU = 70                       # one full wavefront of instances plus a partial one
STEPS_GPU = (1, 45)              # 45: more than one segment of 32 steps and no multiple of it
PROBLEMS = ('htwa_nq5_N2', 'htwa_nq6_N20', 'fr7')


@functools.lru_cache(maxsize=None)
def case_problem(name):
    """(par, prob, net)"""
    if name == 'fr7':
        return make_problem_fr7()
    nq, N = {'htwa_nq5_N2': (5, 2), 'htwa_nq6_N20': (6, 20)}[name]
    return make_problem('htwa', N=N, nq=nq)


def colliding_configuration(prob, oracle):
    """a joint configuration inside the box whose collision rows fail their check bounds by a clear margin (the search of
    test_guess_until_gpu._colliding_configuration)"""
    nq = prob.nq
    lo, hi = prob.lbx[:nq] + 0.05, prob.ubx[:nq] - 0.05
    p1 = np.zeros((1, prob.N + 1, 5))
    for u in halton(400, nq, skip=3):
        q = lo + u * (hi - lo)
        x = np.tile(np.concatenate([q, np.zeros(nq)]), (1, prob.N + 1, 1))
        rv = oracle.eval_nodes(x, np.zeros((1, prob.N, nq)), p1)['row_val'][0, 0, :prob.desc.n_rows]
        if np.max(np.maximum(prob.row_check[:, 0] - rv, rv - prob.row_check[:, 1])) > 1e-3:
            return q
    raise AssertionError('no colliding configuration found')


def last_rows(B, T):
    """(last_x, last_u) [B] int64: complete logs, (j + 1, j) and (j, j) at an early, a middle and the last step, at the two sides of
    a 32-step segment boundary, (0, 0) and (0, -1) -- every case several times over the batch"""
    cases = [(T, T - 1), (0, 0), (0, -1)]
    for j in sorted({min(1, T - 1), T // 2, T - 1} | ({30, 31} if T > 32 else set())):
        cases += [(j + 1, j), (j, j)]
    cases = list(dict.fromkeys(cases))
    pick = [cases[b % len(cases)] for b in range(B)]
    return np.array([c[0] for c in pick], np.int64), np.array([c[1] for c in pick], np.int64)


def planted_logs(prob, oracle, B, T, seed=SEED):
    """Step-major logs x_log [T+1, B, nx], u_log [T, B, nu] with last_x / last_u from :func:`last_rows`: a slow random walk from
    collision-free starts with small velocities, in which every instance has, each at a valid step of its own where the log has
    three, one colliding configuration (d4), one joint beyond x_max (d5) and one velocity raised to 0.8 v_max (d6).  Every invalid
    row holds NaN or 1e300, alternating with every round through the cases of :func:`last_rows`."""
    nq, nx = prob.nq, prob.nx
    rng = np.random.default_rng(seed)
    x0 = sample_instances(prob, B, seed=seed)
    x = np.zeros((T + 1, B, nx))
    x[:, :, :nq] = x0[None, :, :nq] + np.cumsum(0.002 * rng.standard_normal((T + 1, B, nq)), axis=0)
    x[:, :, nq:] = 0.1 * rng.uniform(-1, 1, (T + 1, B, nq)) * prob.x_max[nq:]
    u = rng.uniform(-2, 2, (T, B, nq))
    lx, lu = last_rows(B, T)
    q_hit = colliding_configuration(prob, oracle) if prob.desc.n_rows else None
    for b in range(B):
        n = int(lx[b]) + 1
        jc, jb, js = (3 * b) % n, (3 * b + 1) % n, (3 * b + 2) % n
        if q_hit is not None:
            x[jc, b, :nq] = q_hit + 0.002 * rng.standard_normal(nq)
        x[jb, b, 1] = prob.x_max[1] + 0.3 + 0.3 * rng.uniform()
        x[js, b, nq:] = 0.8 * prob.x_max[nq:]
    n_cases = len(set(zip(lx.tolist(), lu.tolist())))
    pad = np.where((np.arange(B) // n_cases) % 2 == 0, np.nan, 1e300)          # (every case of last_rows meets both kinds)
    steps = np.arange(T + 1)[:, None]
    inv_x, inv_u = steps > lx[None, :], steps[:T] > lu[None, :]
    x[inv_x] = np.broadcast_to(pad[None, :, None], x.shape)[inv_x]
    u[inv_u] = np.broadcast_to(pad[None, :, None], u.shape)[inv_u]
    return x, u, lx, lu


def candidates(solver, prob, par, x_log, lx):
    """what the three extremes are taken over, on the solver's (the oracle's) side: the collision margins [B, T+1, n_rows], the
    state-box margin of every step [B, T+1] and g of every step [B, T+1]; invalid rows -inf / -inf / +inf"""
    from safe_mpc_amd import closed_loop as cl
    x = np.transpose(x_log, (1, 0, 2))
    B, T1 = x.shape[0], x.shape[1]
    valid = np.arange(T1)[None, :] <= lx[:, None]
    flat = np.where(valid[:, :, None], x, 0.0).reshape(-1, x.shape[2])
    _, rv, _ = cl._score_eval_chunks(solver, prob, flat, par.alpha, 4096, False)
    _, _, g = cl._score_eval_chunks(solver, prob, flat, par.alpha, 4096, True)
    nr = int(prob.desc.n_rows)
    rv = rv.reshape(B, T1, nr)
    rows = np.where(valid[:, :, None], np.maximum(prob.row_check[:, 0] - rv, rv - prob.row_check[:, 1]), -np.inf)
    box = np.where(valid, np.max(np.maximum(prob.x_min - x, x - prob.x_max), axis=2), -np.inf)
    return rows, box, np.where(valid, g.reshape(B, T1), np.inf)


@functools.lru_cache(maxsize=None)
def reference(name, T):
    """the logs of one (problem, n_steps) case and the statement's results on the CPU oracle, computed once and shared (read-only):
    dict(x, u, lx, lu, traj, ref = (out, outi) with the safe-set score and the constant ee_ref, ref_traj = (out, outi) without it
    and against a random trajectory shorter than the log)"""
    from fake_solver import OracleSolver
    from safe_mpc_amd import closed_loop as cl
    par, prob, net = case_problem(name)
    solver = OracleSolver(prob, net)
    x, u, lx, lu = planted_logs(prob, solver.o, B_GPU, T)
    traj = prob.ee_ref[:, None] + 0.2 * np.random.default_rng(SEED + T).standard_normal((3, max(1, (T + 1) // 2)))
    with np.errstate(invalid='ignore'):
        ref = cl.score_rollout_statement(solver, prob, par, x, u, lx, lu, want_safe=True)
        ref_traj = cl.score_rollout_statement(solver, prob, par, x, u, lx, lu, traj=traj)
    out = dict(x=x, u=u, lx=lx, lu=lu, traj=traj, ref=ref, ref_traj=ref_traj)
    for v in (x, u, lx, lu, traj, *ref, *ref_traj):
        v.setflags(write=False)
    return out
