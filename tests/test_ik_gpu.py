"""smpc_ik_batch (k_ik) and the tracking task on the GPU.  -m gpu only.

The kernel is held against its numpy statement safe_mpc_amd/ik.py::ik_batch_host and, independently of both, against the CPU oracle
and smpc_eval_nodes.  Inputs are ik_cases.py's: 32 reachable targets, 16 starts (Halton from point 11, start 0 the middle of
the box), for the 6-DoF arm with capsule rows, the 7-DoF arm with sphere and plane rows and a 6-DoF descriptor without rows; an
unreachable target (5, 5, 5) is instance 33.  S in {1, 16, 64}, B in {1, 33}, masks with holes.

Tolerances: 1e-9 (1 + |.|), the suite's FP64 tolerance, for one iteration and for every forward evaluation; 1e-7 (1 + |.|) for three
chained iterations (a hundredfold allowance for three chained nq x nq solves).  Full 40-iteration runs are not compared point-wise
with the statement: accept / reject branches make that ill-posed."""
import functools

import numpy as np
import pytest

from conftest import make_problem
from ik_cases import N_STARTS, N_TARGETS, case, oracle_margins, solved

pytestmark = pytest.mark.gpu

FAR = np.array([5.0, 5.0, 5.0])


@functools.lru_cache(maxsize=None)
def gcase(name):
    """(problem, oracle, targets [33, 3] with the unreachable one last, q_start [33, 16, nq]); 'norows': the 6-DoF arm without
    collision rows, at the 6-DoF case's targets and starts"""
    if name == 'norows':
        from oracle.oracle import Oracle
        _, prob, _ = make_problem('naive', N=10, collisions_pairs=[])
        assert len(prob.rows) == 0
        o = Oracle(prob)
        _, _, _, tgt, qs = case('z1')
    else:
        _, prob, o, tgt, qs = case(name)
    return prob, o, np.ascontiguousarray(np.vstack([tgt, FAR])), np.ascontiguousarray(np.concatenate([qs, qs[:1]]))


@functools.lru_cache(maxsize=None)
def solver(name):
    from safe_mpc_amd.solver import BatchedOcpSolver
    return BatchedOcpSolver(gcase(name)[0], None)


@functools.lru_cache(maxsize=None)
def device_default(name):
    """the kernel's answer at the default settings for the 33 instances, S = 16 (read-only, shared)"""
    prob, o, tgt, qs = gcase(name)
    return solver(name).ik(tgt, qs)


def _close(a, b, tol):
    return np.all(np.abs(a - b) <= tol * (1 + np.abs(b)))


def device_margins(name, q, target):
    """(|ee - target|_inf, worst row margin) of q [M, nq] through smpc_eval_nodes on the device"""
    from safe_mpc_amd.problem import INF
    prob = gcase(name)[0]
    M, N = q.shape[0], prob.N
    xg = np.zeros((M, N + 1, prob.nx))
    xg[:, :, :prob.nq] = q[:, None, :]
    ev = solver(name).eval_nodes(xg, np.zeros((M, N, prob.nu)), np.zeros((M, N + 1, 5)))
    ee_inf = np.abs(np.asarray(ev['ee'])[:, 0] - target).max(1)
    rv = np.asarray(ev['row_val'])[:, 0, :len(prob.rows)]
    lb = np.where(np.abs(prob.row_lb) < INF, prob.row_lb, -np.inf)
    ub = np.where(np.abs(prob.row_ub) < INF, prob.row_ub, np.inf)
    return ee_inf, (np.maximum(lb - rv, rv - ub).max(1) if len(prob.rows) else np.full(M, -np.inf))


# ---- step parity -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['z1', 'fr7', 'norows'])
@pytest.mark.parametrize('iters,tol', [(1, 1e-9), (3, 1e-7)])
def test_step_parity_with_the_statement(name, iters, tol):
    """every single start after 1 and after 3 iterations: the kernel with S = 1 per start (B = 512) against the statement's point of
    that start; starts whose accept test or row activation the statement decides by less than 1e-6 are skipped, at most 10 %"""
    from safe_mpc_amd.ik import ik_batch_host
    prob, o, tgt, qs = gcase(name)
    tgt, qs = tgt[:N_TARGETS], qs[:N_TARGETS]
    trace = {}
    ik_batch_host(prob, tgt, qs, trace=trace, max_iter=iters)
    q, info, resid = solver(name).ik(np.ascontiguousarray(np.repeat(tgt, N_STARTS, axis=0)),
                                     np.ascontiguousarray(qs.reshape(-1, 1, prob.nq)), max_iter=iters)
    ref = trace['q'].reshape(-1, prob.nq)
    skip = ((trace['accept_gap'] < 1e-6) | (trace['row_gap'] < 1e-6)).reshape(-1)
    err = np.abs(q - ref) / (1 + np.abs(ref))
    print(name, 'iterations', iters, 'skipped', int(skip.sum()), 'of', skip.size, 'worst error of the rest', err[~skip].max())
    assert skip.mean() <= 0.10
    assert np.all(err[~skip] <= tol)
    assert np.all(info[:, 0] == 0)
    assert np.array_equal(info[~skip, 1] > 0, trace['success'].reshape(-1)[~skip])


# ---- truthfulness and success at the default settings ------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['z1', 'fr7', 'norows'])
def test_outputs_are_truthful(name):
    """resid is what smpc_eval_nodes and the oracle see at q_out, info[:, 1] > 0 exactly when that re-evaluation meets the success
    predicate, q_out is inside the box"""
    prob, o, tgt, qs = gcase(name)
    q, info, resid = device_default(name)
    lo, hi = prob.x_min[:prob.nq], prob.x_max[:prob.nq]
    assert np.isfinite(q).all() and np.all((q >= lo) & (q <= hi))
    assert np.all((info[:, 0] >= 0) & (info[:, 0] < N_STARTS) & (info[:, 1] >= 0) & (info[:, 1] <= N_STARTS))
    for what, (e, m) in (('device', device_margins(name, q, tgt)), ('oracle', oracle_margins(prob, o, q, tgt))):
        fin = np.isfinite(m)
        print(name, what, 'ee', np.abs(resid[:, 0] - e).max(), 'margin', np.abs(resid[fin, 1] - m[fin]).max() if fin.any() else 0.0)
        assert _close(resid[:, 0], e, 1e-9)
        assert np.array_equal(np.isfinite(resid[:, 1]), fin) and _close(resid[fin, 1], m[fin], 1e-9)
        assert np.all(resid[~fin, 1] == -np.inf)
        assert np.array_equal(info[:, 1] > 0, (e <= 1e-6) & (m <= 0.0))


@pytest.mark.parametrize('name', ['z1', 'fr7', 'norows'])
def test_every_reachable_target_is_solved(name):
    """S = 16: all 32 reachable targets (the statement has at least 4 successful starts for each, test_ik_host.py); the unreachable
    one fails cleanly"""
    prob, o, tgt, qs = gcase(name)
    q, info, resid = device_default(name)
    print(name, 'successful starts per reachable target: min', int(info[:N_TARGETS, 1].min()))
    assert np.all(info[:N_TARGETS, 1] > 0)
    assert np.all(resid[:N_TARGETS, 0] <= 1e-6) and np.all(resid[:N_TARGETS, 1] <= 0.0)
    assert info[N_TARGETS, 1] == 0 and resid[N_TARGETS, 0] > 1.0 and np.isfinite(q[N_TARGETS]).all()
    if name != 'norows':        # (the winner is the successful start with the lowest index: the statement's, where it has the margin)
        _, info_h, _, trace = solved(name)
        same = info[:N_TARGETS, 0] == info_h[:, 0]
        print(name, 'same winner as the statement for', int(same.sum()), 'of', N_TARGETS)


# ---- determinism, isolation, mask --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['z1', 'fr7'])
def test_determinism_isolation_and_mask(name):
    """S = 64: two calls give the same bits; instance b of the B = 33 call equals the B = 1 call on it, bit for bit; masked-out
    instances keep what their rows held"""
    from safe_mpc_amd.closed_loop import halton
    prob, o, tgt, qs = gcase(name)
    sv = solver(name)
    lo, hi = prob.x_min[:prob.nq], prob.x_max[:prob.nq]
    B = tgt.shape[0]
    q64 = np.ascontiguousarray((lo + halton(B * 64, prob.nq, skip=3) * (hi - lo)).reshape(B, 64, prob.nq))
    a = sv.ik(tgt, q64)
    b = sv.ik(tgt, q64)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    for i in (0, 7, 31, 32):
        one = sv.ik(tgt[i:i + 1], q64[i:i + 1])
        for x, y in zip(a, one):
            assert np.array_equal(x[i:i + 1], y), i
    # the first 16 of the 64 starts alone: the lowest successful index cannot grow, and a start's fate does not depend on S
    c = sv.ik(tgt, np.ascontiguousarray(q64[:, :16]))
    hit = c[1][:, 1] > 0
    assert np.array_equal(c[1][hit, 0], a[1][hit, 0]) and np.array_equal(c[0][hit], a[0][hit])
    mask = (np.arange(B) % 3 != 1).astype(np.uint8)
    qo, io, ro = np.full((B, prob.nq), 7.0), np.full((B, 2), -5, np.int32), np.full((B, 2), 9.0)
    sv.ik(tgt, q64, mask=mask, q_out=qo, info=io, resid=ro)
    m = mask.astype(bool)
    assert np.array_equal(qo[m], a[0][m]) and np.array_equal(io[m], a[1][m]) and np.array_equal(ro[m], a[2][m])
    assert np.all(qo[~m] == 7.0) and np.all(io[~m] == -5) and np.all(ro[~m] == 9.0)


def test_device_pointers_only_enqueue_and_agree():
    import torch
    prob, o, tgt, qs = gcase('z1')
    sv = solver('z1')
    dev = torch.device('cuda', sv.device)
    qd, idd, rd = sv.ik(torch.as_tensor(tgt, device=dev), torch.as_tensor(qs, device=dev))
    sv.sync()
    q, info, resid = device_default('z1')
    assert np.array_equal(qd.cpu().numpy(), q) and np.array_equal(idd.cpu().numpy(), info) and np.array_equal(rd.cpu().numpy(), resid)


# ---- scenes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['z1', 'fr7'])
def test_rows_are_formed_in_the_instance_scene(name):
    from safe_mpc_amd._lib import EngineError
    from safe_mpc_amd.problem import INF, ROW_COORD
    from safe_mpc_amd.solver import BatchedOcpSolver
    prob, o, tgt, qs = gcase(name)
    sv = BatchedOcpSolver(prob, None)
    B = tgt.shape[0]
    base = device_default(name)
    geom = np.ascontiguousarray(np.repeat(prob.row_geometry()[None], B, axis=0))
    sv.set_instance_scene(geom)
    same = sv.ik(tgt, qs)
    for x, y in zip(base, same):            # every instance in the base geometry: the call without a scene, bit for bit
        assert np.array_equal(x, y)
    with pytest.raises(EngineError, match=r'engine error -1.*smpc_ik_batch.*33'):
        sv.ik(tgt[:1], qs[:1])
    # one obstacle moved onto the end-effector target of instance k: its rows are violated at the old answer
    k = 5
    r = next(i for i, (row, n) in enumerate(zip(prob.rows, prob.row_obstacle)) if n is not None and row.kind != ROW_COORD)
    geom[k] = prob.scene({prob.row_obstacle[r]: tgt[k] - np.array(prob.rows[r].C[:])})
    sv.set_instance_scene(geom)
    moved = sv.ik(tgt, qs)
    others = np.arange(B) != k
    for x, y in zip(base, moved):
        assert np.array_equal(x[others], y[others])
    assert not np.array_equal(moved[0][k], base[0][k])
    # resid[k] is the re-evaluation of q_out[k] in ITS scene (smpc_eval_nodes forms the rows there too)
    N = prob.N
    xg = np.zeros((B, N + 1, prob.nx))
    xg[:, :, :prob.nq] = moved[0][:, None, :]
    ev = sv.eval_nodes(xg, np.zeros((B, N, prob.nu)), np.zeros((B, N + 1, 5)))
    rv = np.asarray(ev['row_val'])[:, 0, :len(prob.rows)]
    lb = np.where(np.abs(prob.row_lb) < INF, prob.row_lb, -np.inf)
    ub = np.where(np.abs(prob.row_ub) < INF, prob.row_ub, np.inf)
    m = np.maximum(lb - rv, rv - ub).max(1)
    assert _close(moved[2][:, 1], m, 1e-9)
    assert np.array_equal(moved[1][:, 1] > 0, (moved[2][:, 0] <= 1e-6) & (m <= 0.0))
    sv.set_instance_scene(None)
    for x, y in zip(base, sv.ik(tgt, qs)):
        assert np.array_equal(x, y)


def test_argument_errors():
    from safe_mpc_amd._lib import EngineError
    prob, o, tgt, qs = gcase('z1')
    sv = solver('z1')
    with pytest.raises(EngineError, match=r'engine error -1.*S=65'):
        sv.ik(tgt[:1], np.zeros((1, 65, prob.nq)))
    with pytest.raises(EngineError, match=r'engine error -1.*max_iter=0'):
        sv.ik(tgt[:1], qs[:1], max_iter=0)
    assert sv.L.smpc_abi_version() == 5


# ---- the tracking task --------------------------------------------------------------------------------------------------------------
def tracking_params():
    from safe_mpc_amd.parser import Parameters
    par = Parameters({}, 'z1')
    par.nq, par.n_dof_safe_set, par.net_size, par.N, par.nlp_max_iter, par.back_hor = 6, 6, [12, 256, 1], 10, 200, 10
    par.n_steps_tracking = 20
    return par


@functools.lru_cache(maxsize=None)
def tracking_guess():
    """generate_guess(traj=...) for the "8": B = 8, N = 10, controller 'naive', SQP on the device (read-only, shared)"""
    from safe_mpc_amd import closed_loop as cl
    from safe_mpc_amd.tracking import tracking_trajectory
    par = tracking_params()
    traj = tracking_trajectory(par, '8')
    guess, good = cl.generate_guess(par, 'naive', 8, on_device=True, traj=traj)
    return par, traj, guess, good


def test_tracking_warm_starts():
    """every returned guess starts at rest with its end effector on the curve's first point and passes smpc_check_guess; the
    instances whose IK found nothing are listed and dropped"""
    from safe_mpc_amd import controller as C
    from safe_mpc_amd.problem import OcpProblem
    from oracle.oracle import Oracle
    par, traj, guess, good = tracking_guess()
    xg, ug = guess['xg'], guess['ug']
    print('accepted', int(good.sum()), 'of 8; IK failed for', list(guess['ik_failed']))
    assert good.shape == (8,) and xg.shape == (int(good.sum()), 11, 12) and not good[guess['ik_failed']].any()
    assert good.sum() >= 1
    prob = OcpProblem(par, 'naive', 'ext', N=10)
    e, m = oracle_margins(prob, Oracle(prob), xg[:, 0, :6], np.repeat(traj[:, :1].T, len(xg), axis=0))
    assert np.all(e <= 1e-6) and np.all(m <= 0.0)
    assert np.all(xg[:, 0, 6:] == 0.0)
    ctrl = C.get_controller('naive', par, len(xg))
    flags, worst = ctrl.ocp_solver.check_guess(xg, ug)
    assert np.all(flags == 0), (flags, worst)
    # n different arm configurations at the one point
    d = np.abs(xg[:, None, 0, :6] - xg[None, :, 0, :6]).max(2) + 10.0 * np.eye(len(xg))
    assert len(xg) < 2 or d.min() > 1e-2


def test_generate_guess_until_on_the_curve_and_ik_starts_in_scenes():
    """the refilling loop on the tracking stream: 4 accepted guesses, each at rest on the curve's first point, sample j being the
    j-th instance of ik_starts; ik_starts with every instance in the base geometry equals ik_starts without scenes"""
    from safe_mpc_amd import closed_loop as cl
    from safe_mpc_amd import controller as C
    from safe_mpc_amd.problem import OcpProblem
    from oracle.oracle import Oracle
    par, traj, guess, good = tracking_guess()
    g, info = cl.generate_guess_until(par, 'naive', 4, batch=4, check_every=50, traj=traj)
    assert g['xg'].shape == (4, 11, 12) and len(info['accepted']) == 4 and info['ik_failed'] == []
    prob = OcpProblem(par, 'naive', 'ext', N=10)
    e, m = oracle_margins(prob, Oracle(prob), g['xg'][:, 0, :6], np.repeat(traj[:, :1].T, 4, axis=0))
    assert np.all(e <= 1e-6) and np.all(m <= 0.0) and np.all(g['xg'][:, 0, 6:] == 0.0)
    sv = C.get_controller('naive', par, 4).ocp_solver
    x0, i0 = cl.ik_starts(sv, prob, traj[:, 0], 6)
    assert np.array_equal(g['xg'][:, 0], x0[np.array(info['accepted'])])      # (every IK succeeded: sample j is instance j)
    x1, i1 = cl.ik_starts(sv, prob, traj[:, 0], 6, scenes=np.repeat(prob.row_geometry()[None], 6, axis=0))
    assert np.array_equal(x0, x1) and np.array_equal(i0, i1)
    x2, _ = cl.ik_starts(sv, prob, traj[:, 0], 6)                              # the handle is left without a scene
    assert np.array_equal(x0, x2)


def test_tracking_closed_loop_is_scored_against_the_curve():
    """run_mpc(traj=...) as scripts/mpc.py --track 8 calls it, 20 steps from the tracking warm starts: x_log[0] is the IK start and
    the device score equals the statement evaluated with the CPU oracle on the returned logs (the tolerance of test_score_gpu.py)"""
    from fake_solver import OracleSolver
    from safe_mpc_amd import closed_loop as cl
    from safe_mpc_amd.problem import OcpProblem
    par, traj, guess, good = tracking_guess()
    xg, ug = guess['xg'], guess['ug']
    B, n_steps = len(xg), 20
    res = cl.run_mpc(par, 'naive', xg, ug, n_steps=n_steps, on_device=True, score=True, graphs=False, traj=traj)
    assert np.array_equal(res['x'][:, 0], xg[:, 0])
    bad_x, bad_u = np.isnan(res['x']).any(2), np.isnan(res['u']).any(2)
    lx = np.where(bad_x.any(1), np.argmax(bad_x, axis=1) - 1, n_steps).astype(np.int64)
    lu = np.where(bad_u.any(1), np.argmax(bad_u, axis=1) - 1, n_steps - 1).astype(np.int64)
    prob = OcpProblem(par, 'naive', 'ext', N=10)
    out, outi = cl.score_rollout_statement(OracleSolver(prob, None), prob, par, np.transpose(res['x'], (1, 0, 2)),
                                           np.transpose(res['u'], (1, 0, 2)), lx, lu, traj=traj)
    ref, s = cl._score_dict(out, outi), res['score']
    for k in ('cost', 'ee_err2', 'u2', 'ee_dist', 'coll_margin', 'box_margin'):
        print(k, np.abs(s[k] - ref[k]).max())
        assert _close(s[k], ref[k], 1e-9), k
    assert np.array_equal(s['box_step'], ref['box_step'])
    # the curve, not the constant ee_ref, is what was scored
    other, _ = cl.score_rollout_statement(OracleSolver(prob, None), prob, par, np.transpose(res['x'], (1, 0, 2)),
                                          np.transpose(res['u'], (1, 0, 2)), lx, lu)
    assert np.all(np.abs(other[:, 1] - out[:, 1]) > 1e-6)
