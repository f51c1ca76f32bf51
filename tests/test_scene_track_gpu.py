"""Obstacles that move along the horizon (smpc_set_instance_scene_track, smpc_set_scene_clock) on the GPU.  -m gpu only.

The principle: node k of the moving problem is node k of the static problem in the scene of column col(t + k).  The static problem
(smpc_set_instance_scene) is pinned to the oracle by test_scene_gpu.py, and neither interior-point kernel reads geometry, so what is
shown here is that every kernel that forms collision rows reads the right column -- BIT FOR BIT against calls in static scenes
wherever a result is node-wise, and against the Python statements on the CPU oracle (track_cases.TrackOracleSolver: one oracle per
scene, composed per node) at the tolerances of the tests that pin the same calls in a static scene: 1e-9 relative for the
linearisation (test_scene_gpu.py, eval_nodes), 1e-9 (1 + |.|) for FP64 margins, equality for verdicts and integer slots.

Fixtures: the four scenes of scene_cases.scene_family (SHIFTS); a track is a per-instance sequence of indices into them
(track_cases.track_indices).  Shapes: z1, N = 8, B = 5 (45 nodes: the stage builder's last wavefront has an empty group, the
interior point a half-filled wavefront) and B = 9 (81 nodes: the thread-per-node kernels cross a 64-thread block); fr7 with B = 3
for the NQ = 7 instantiations; T in {1, 3, N + 1, N + 4}; clock in {none, 0, 2, T + 5, -1}; controllers 'st' and 'receding'."""
import ctypes
import functools
import types

import numpy as np
import pytest

import scene_cases as sc
import track_cases as tc
from conftest import constant_guess, halton, make_problem, sample_instances
from fake_solver import OracleSolver

pytestmark = pytest.mark.gpu

N = 8
CASES = [('z1', 'st', 5), ('z1', 'receding', 9), ('fr7', 'constraint_everywhere', 3)]
CLOCKS = lambda T: (None, 0, 2, T + 5, -1)


def _rel(a, b):
    return np.abs(a - b).max() / (1e-12 + np.abs(b).max())


def _close(got, ref, tol):
    same_inf = np.isinf(ref) & (got == ref)
    with np.errstate(invalid='ignore'):
        return np.all(same_inf | (np.abs(got - ref) <= tol * (1.0 + np.abs(ref))))


def _solver(prob, net, mode=None):
    from safe_mpc_amd.solver import BatchedOcpSolver
    s = BatchedOcpSolver(prob, net)
    if mode is not None:
        s.set_qp_mode(mode)
    return s


def _cell(value=0):
    import torch
    return torch.full((1,), int(value), dtype=torch.int64, device='cuda:0')


def _set_clock(s, cell, c):
    """clock none, or the cell at c -- written and FINISHED before the next host-pointer call (the engine has a stream of its own)"""
    import torch
    if c is None:
        s.set_scene_clock(None)
        return 0
    cell.fill_(int(c))
    torch.cuda.synchronize()
    s.set_scene_clock(cell)
    return int(c)


@functools.lru_cache(maxsize=None)
def _case(system, controller, B):
    """(par, prob, net), moved problems, geometry [S, R, 8], and perturbed inputs as in test_eval_nodes_parity"""
    n_scenes = 4 if system == 'z1' else 3
    (par, prob, net), moved, geom = sc.scene_family(system, controller, N, n_scenes)
    x0 = sample_instances(prob, B, seed=1, vel_scale=0.5)
    xg, ug, p = constant_guess(prob, x0)
    rng = np.random.default_rng(0)
    xg[:, 1:] += 0.05 * rng.standard_normal(xg[:, 1:].shape)
    ug += rng.uniform(-5, 5, ug.shape)
    return (par, prob, net), moved, geom, n_scenes, (x0, xg, ug, p)


def _unequal_fields(a, b):
    return [f for f in a.dtype.names if not np.array_equal(a[f], b[f])]


# ---- 1. + 4. smpc_eval_nodes: node by node, every T, every clock ----------------------------------------------------------------------
@pytest.mark.parametrize('system,controller,B', CASES)
def test_eval_nodes_node_k_is_the_static_node_in_column_t_plus_k(system, controller, B):
    """every T and clock: all fields of node k of instance b bit-equal to the call in the static scene track[b, col(t + k)]; bit-equal
    to clock none on the track G'[b, j] = G[b, col(c + j)]; within 1e-9 relative of the per-scene oracles composed per node; and
    a clock cell rewritten between two device-pointer calls, with no other host call between them, is seen by the second"""
    import torch
    (par, prob, net), moved, geom, S, (x0, xg, ug, p) = _case(system, controller, B)
    nq, nr = prob.nq, len(prob.rows)
    s = _solver(prob, net)
    static = []
    for k in range(S):
        s.set_instance_scene(np.repeat(geom[k:k + 1], B, axis=0))
        static.append(s.eval_nodes(xg, ug, p))
    assert _rel(static[1]['row_val'][..., :nr], static[0]['row_val'][..., :nr]) > 1e-3       # the scenes are told apart
    oracle = tc.TrackOracleSolver(prob, net, [m[1] for m in moved], geom)
    ocell, cell = np.zeros(1, np.int64), _cell()
    oracle.set_scene_clock(ocell)
    seen_all = set()
    for T in (1, 3, N + 1, N + 4):
        idx = tc.track_indices(B, T, S)
        s.set_instance_scene_track(geom[idx])
        oracle.set_instance_scene_track(geom[idx])
        for c in CLOCKS(T):
            t = _set_clock(s, cell, c)
            a = s.eval_nodes(xg, ug, p)
            seen = tc.node_scenes(idx, t, N + 1)
            ref = tc.per_node(lambda k: static[k], seen)
            assert _unequal_fields(a, ref) == [], (T, c)
            seen_all.add(seen.tobytes())
            # the oracles of the same per-node scenes
            ocell[0] = t
            o = oracle.eval_nodes(xg, ug, p)
            for f, n in [('tau', nq), ('M', nq * nq), ('dtau_dq', nq * nq), ('dtau_dv', nq * nq), ('ee', 3), ('cost_grad_q', nq),
                         ('cost_hess_qq', nq * nq), ('row_val', nr), ('row_grad', nr * nq)]:
                assert _rel(a[f][..., :n], o[f][..., :n]) < 1e-9, (T, c, f)
            # the clock is a shift of the track
            if c is not None and T > 1:
                s.set_scene_clock(None)
                s.set_instance_scene_track(geom[tc.clocked(idx, c, N + 1)])
                assert _unequal_fields(s.eval_nodes(xg, ug, p), a) == [], (T, c)
                s.set_instance_scene_track(geom[idx])
    assert len(seen_all) >= 8                                    # (the cases do differ from one another)
    # the cell is read when the kernel runs: rewritten between two calls that only enqueue
    T = N + 4
    idx = tc.track_indices(B, T, S)
    dev = lambda v: torch.tensor(v, dtype=torch.float64, device='cuda:0')
    s.set_instance_scene_track(dev(geom[idx]))
    s.set_scene_clock(cell)
    dx, du, dp = dev(xg), dev(ug), dev(p)
    cell.fill_(0)
    a0 = s.eval_nodes(dx, du, dp)
    cell.fill_(3)
    a3 = s.eval_nodes(dx, du, dp)
    s.sync()
    for got, t in ((a0, 0), (a3, 3)):
        ref = tc.per_node(lambda k: static[k], tc.node_scenes(idx, t, N + 1))
        assert np.array_equal(got['row_val'].cpu().numpy(), ref['row_val']) and np.array_equal(got['row_grad'].cpu().numpy(), ref['row_grad'])
    assert not np.array_equal(a0['row_val'].cpu().numpy(), a3['row_val'].cpu().numpy())


# ---- 2. smpc_debug_stage_records: the QP the interior point is given -------------------------------------------------------------------
def _stage_records(s, x0, xg, ug, p, path):
    """the stage records [B, N + 1, stride] after either builder (path 1: k_stage_build, 0: k_node_linearise + k_qp_setup), no
    interior point; and the record's layout (the engine's test hook, as in test_gpu_parity.py)"""
    L = s.L
    L.smpc_debug_stage_records.argtypes = [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 4 + [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    lay = np.zeros(24, np.int32)
    B = x0.shape[0]
    arrs = [np.ascontiguousarray(a, np.float64) for a in (x0, xg, ug, p)]
    out = np.zeros(B * 64 * 2048)
    rc = L.smpc_debug_stage_records(s.h, B, *[a.ctypes.data for a in arrs], path, out.ctypes.data, lay.ctypes.data)
    assert rc == 0, L.smpc_last_error(s.h)
    stride, per = int(lay[0]), int(lay[14])
    assert per * B <= out.size and per >= (N + 1) * stride
    return out[:B * per].reshape(B, per)[:, :(N + 1) * stride].reshape(B, N + 1, stride), lay


def _blocks(lay, nq):
    stride, nIMG, oIMG, oSL, nF, oR0, oR1, oR2, oCZA, oCZN, oZ, oZN, NRT, nJ, per = [int(v) for v in lay[:15]]
    return {'jacobian': (oIMG, nJ), 'defect / scalars': (oIMG + nJ, nF - nJ), 'cost': (oIMG + nF, nIMG - nF),
            'scalars + partial sums + w': (oSL, 16), 'bounds': (oR0, 2 * NRT), 'slacks': (oR1, 2 * NRT), 'multipliers': (oR2, 2 * NRT),
            'c.z_aff': (oCZA, 32), 'c.z+': (oCZN, 32), 'z': (oZ, 3 * nq), 'z+': (oZN, 3 * nq)}


@pytest.mark.parametrize('system,controller,B', CASES)
def test_stage_records_of_stage_k_are_the_static_ones_in_column_t_plus_k(system, controller, B):
    """both builders, T = 3 (the clamp inside the horizon) and T = N + 4, clock none and 2: every block of stage k's record
    bit-equal to stage k's record of the static build in scene col(t + k).  With the interior point untouched this is the proof of
    the solve."""
    (par, prob, net), moved, geom, S, (x0, xg, ug, p) = _case(system, controller, B)
    s = _solver(prob, net)
    cell = _cell()
    for path in (1, 0):
        static = []
        for k in range(S):
            s.set_instance_scene(np.repeat(geom[k:k + 1], B, axis=0))
            static.append(_stage_records(s, x0, xg, ug, p, path))
        blocks = _blocks(static[0][1], prob.nq)
        o, n = blocks['jacobian']
        assert not np.array_equal(static[0][0][:, :, o:o + n], static[1][0][:, :, o:o + n])      # the scenes are told apart
        for T in (3, N + 4):
            idx = tc.track_indices(B, T, S)
            s.set_instance_scene_track(geom[idx])
            for c in (None, 2):
                t = _set_clock(s, cell, c)
                got, lay = _stage_records(s, x0, xg, ug, p, path)
                assert np.array_equal(lay, static[0][1])
                ref = tc.per_node(lambda k: static[k][0], tc.node_scenes(idx, t, N + 1))
                for name, (o, n) in blocks.items():
                    assert np.array_equal(got[:, :, o:o + n], ref[:, :, o:o + n]), (path, T, c, name)


# ---- 3. + 4. smpc_solve_batch ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('qp_mode', ['throughput', 'latency'])
@pytest.mark.parametrize('system,controller,B', CASES)
def test_solve_constant_tracks_equal_the_scene_and_the_clock_shifts_the_track(system, controller, B, qp_mode):
    """x, u, status, qp_iter bit-equal: a T = 1 track, and a track whose columns all hold one scene, against
    smpc_set_instance_scene with that scene, under any clock; and clock c on track G against clock none on G'[b, j] =
    G[b, col(c + j)], for c in {2, T + 5, -1}, T = 3 and N + 4"""
    (par, prob, net), moved, geom, S, (x0, xg, ug, p) = _case(system, controller, B)
    s = _solver(prob, net, qp_mode)
    cell = _cell()
    scene = geom[np.arange(B) % S]
    s.set_instance_scene(scene)
    want = s.solve(x0, xg, ug, p)
    shared = _solver(prob, net, qp_mode).solve(x0, xg, ug, p)
    assert not np.array_equal(want[1], shared[1])                  # (the scenes do enter the solve)
    for track in (scene[:, None], np.repeat(scene[:, None], 3, axis=1), np.repeat(scene[:, None], N + 4, axis=1)):
        s.set_instance_scene_track(np.ascontiguousarray(track))
        for c in CLOCKS(track.shape[1]):
            _set_clock(s, cell, c)
            got = s.solve(x0, xg, ug, p)
            assert all(np.array_equal(a, b) for a, b in zip(got, want)), (track.shape[1], c)
    moving = []
    for T in (3, N + 4):
        idx = tc.track_indices(B, T, S)
        for c in (2, T + 5, -1):
            s.set_instance_scene_track(geom[idx])
            _set_clock(s, cell, c)
            got = s.solve(x0, xg, ug, p)
            s.set_instance_scene_track(geom[tc.clocked(idx, c, N + 1)])
            _set_clock(s, cell, None)
            ref = s.solve(x0, xg, ug, p)
            assert all(np.array_equal(a, b) for a, b in zip(got, ref)), (T, c)
            moving.append(got[1])
    assert not np.array_equal(moving[3], moving[5])                 # (T = N + 4: clock 2 and clock -1 are other problems)
    # a scene set over a track replaces it, and clearing either clears both
    s.set_instance_scene_track(geom[tc.track_indices(B, 3, S)])
    s.set_instance_scene(scene)
    assert all(np.array_equal(a, b) for a, b in zip(s.solve(x0, xg, ug, p), want))
    s.set_instance_scene_track(geom[tc.track_indices(B, 3, S)])
    s.set_instance_scene(None)
    assert all(np.array_equal(a, b) for a, b in zip(s.solve(x0, xg, ug, p), shared))


# ---- 5. the forward-only entry points --------------------------------------------------------------------------------------------------
FWD_B = 9


@functools.lru_cache(maxsize=None)
def _forward_case():
    """z1 'st', B = 9: trajectories of which every third node is a state that collides in some of the four scenes and is free in
    the others (found on the oracle among 600 Halton states of the joint box), so that the column decides verdicts and margins;
    the other nodes sit near the instance's free start.  With them the track oracle -- CPU only"""
    (par, prob, net), moved, geom = sc.scene_family('z1', 'st', N, 4)
    nq, B = prob.nq, FWD_B
    q = (prob.lbx[:nq] + 0.05) + halton(600, nq, skip=1 + 7 * 5) * (prob.ubx[:nq] - prob.lbx[:nq] - 0.1)
    pool = np.hstack([q, np.zeros_like(q)])
    free = np.array([_rows_inside(m[1], pool, 0.0) for m in moved])           # [scene, state]
    some = pool[free.any(0) & ~free.all(0)]
    assert len(some) >= 12
    base = sample_instances(prob, B, seed=5, vel_scale=0.1)
    xg = np.repeat(base[:, None, :], N + 1, axis=1)
    far = (np.arange(B)[:, None] + np.arange(N + 1)[None, :]) % 3 == 1
    xg[far, :nq] = some[np.arange(far.sum()) % len(some), :nq]
    xg[:, :, :nq] += 0.02 * np.random.default_rng(7).standard_normal((B, N + 1, nq)) * ~far[:, :, None]
    _, ug, p = constant_guess(prob, base, flag=-1.0)              # (safe-set row off: the violation is FP64 end to end)
    oracle = tc.TrackOracleSolver(prob, net, [m[1] for m in moved], geom)
    return (par, prob, net), moved, geom, oracle, base, xg, ug, p


def _oracle_rows(oracle, geom, idx, t, xg, ug, p):
    cell = np.array([t], np.int64)
    oracle.set_instance_scene_track(geom[idx])
    oracle.set_scene_clock(cell)
    return np.asarray(oracle.eval_nodes(xg, ug, p)['row_val'])[..., :geom.shape[1]]


FWD_TRACKS = [(N + 4, 2), (3, -1), (3, None), (N + 1, N + 6)]


def test_check_trajectory_check_guess_and_merit_terms_read_node_k_in_column_t_plus_k():
    from safe_mpc_amd import closed_loop as cl
    (par, prob, net), moved, geom, oracle, base, xg, ug, p = _forward_case()
    B, nq = FWD_B, prob.nq
    lo, hi = prob.row_check[:, 0], prob.row_check[:, 1]
    s = _solver(prob, net)
    cell = _cell()
    verdicts = []
    for T, c in FWD_TRACKS:
        idx = tc.track_indices(B, T)
        t = 0 if c is None else c
        rv = _oracle_rows(oracle, geom, idx, t, xg, ug, p)                  # [B, N + 1, R], node k in column col(t + k)
        m = np.maximum(lo - rv, rv - hi)
        assert np.all(np.abs(m.max(2)) > 1e-7)                                # no node within rounding of a threshold
        s.set_instance_scene_track(geom[idx])
        _set_clock(s, cell, c)
        # check_trajectory, on the leading 4 nodes: free in the check bounds at every node, each in its column
        ok = s.check_trajectory(xg[:, :4], tol_x=1e30)
        ok_ref = (m[:, :4].max(2) <= 0.0).all(1)
        assert np.array_equal(ok.astype(bool), ok_ref), (T, c)
        verdicts.append(ok_ref)
        # check_guess: bit 1 and worst[1], node 0 alone and all nodes
        for coll_first in (1, 0):
            w_ref = m[:, :1 if coll_first else N + 1].reshape(B, -1).max(1)
            flags, worst = s.check_guess(xg, ug, collision_first_node=coll_first)
            assert np.array_equal((flags >> 1) & 1, (~(w_ref <= 0.0)).astype(np.int32)), (T, c, coll_first)
            assert _close(worst[:, 1], w_ref, 1e-9), (T, c, coll_first)
        # merit_terms: the l1 violation by the numpy statement on the track oracle
        ctrl = types.SimpleNamespace(problem=prob, ocp_solver=oracle, p=p, nq=nq, N=N, params=par)
        v_ref = cl.merit_terms(ctrl, base, xg, ug)[3]
        out = s.merit_terms(base, xg, ug, p)
        print('T', T, 'clock', c, 'free', int(ok_ref.sum()), 'of', B, 'merit viol error', np.abs(out[:, 1] - v_ref).max())
        assert _close(out[:, 1], v_ref, 1e-9), (T, c)
    # preconditions: verdicts of both kinds, and the column decides some of them
    assert any(0 < v.sum() < B for v in verdicts) and any(not np.array_equal(verdicts[0], v) for v in verdicts[1:])


def test_one_sqp_iteration_on_a_track_matches_the_host_loop_body():
    """one smpc_sqp_batch iteration at clock 2 on tracks of N + 4 columns against one pass of generate_guess' loop body -- the
    engine's solve and closed_loop.merit_terms on its eval_nodes, both reading the same track -- held as
    test_one_sqp_iteration_matches_the_host_loop_body holds it"""
    from safe_mpc_amd import controller as C
    from safe_mpc_amd.parser import Parameters
    from test_sqp_gpu import _host_iteration, _state_from
    par = Parameters({}, 'z1')
    par.nq, par.n_dof_safe_set, par.net_size, par.N, par.nlp_max_iter = 6, 6, [12, 256, 1], N, 200
    B = 9
    ctrl = C.get_controller('htwa', par, B)
    pr = ctrl.problem
    geom = np.array([pr.scene({n: sh for n in sc.Z1_OBSTACLES}) for sh in sc.SHIFTS])
    x0 = sample_instances(pr, B, seed=5, vel_scale=0.0)
    ctrl.setGuess(np.repeat(x0[:, None, :], N + 1, axis=1), np.zeros((B, N, ctrl.nu)))
    s = ctrl.ocp_solver
    idx = tc.track_indices(B, N + 4)
    s.set_instance_scene_track(geom[idx])
    cell = _cell()
    _set_clock(s, cell, 2)
    mu, done, status = np.full(B, 10.0), np.zeros(B, bool), np.zeros(B, np.int32)
    xg0, ug0 = ctrl.x_guess.copy(), ctrl.u_guess.copy()
    r = _host_iteration(ctrl, x0, mu, done, status)
    xd, ud, state = s.sqp(x0, xg0, ug0, ctrl.p, dict(max_iter=1), _state_from(s, B, mu, done, status))
    dec = r['margin'] > 1e-9
    print('undecidable', int((~dec).sum()), 'updated', int(r['updated'].sum()))
    assert (~dec).sum() <= 1 and r['updated'].sum() >= 1
    assert np.array_equal(state['updated'][dec].astype(bool), r['updated'][dec])
    assert np.array_equal(state['alpha'][dec], r['alpha'][dec])
    assert np.all(np.abs(state['mu'][dec] - r['mu'][dec]) <= 1e-9 * (1.0 + np.abs(r['mu'][dec])))
    assert np.array_equal(state['done'][dec].astype(bool), r['done'][dec]) and np.array_equal(state['status'][dec], r['status'][dec])
    ex = np.abs(xd - ctrl.x_guess).reshape(B, -1).max(1) / (1.0 + np.abs(ctrl.x_guess).reshape(B, -1).max(1))
    eu = np.abs(ud - ctrl.u_guess).reshape(B, -1).max(1) / (1.0 + np.abs(ctrl.u_guess).reshape(B, -1).max(1))
    assert np.all(ex[dec] <= 1e-9) and np.all(eu[dec] <= 1e-9)
    # and the track enters: the same iteration in every instance's column 0 is another one
    s.set_instance_scene(np.ascontiguousarray(geom[idx][:, 0]))
    xs, us, _ = s.sqp(x0, xg0, ug0, ctrl.p, dict(max_iter=1), _state_from(s, B, mu, done, status))
    assert not np.array_equal(us, ud)


def test_ik_runs_in_column_t():
    """smpc_ik_batch with a track at clock c: bit-equal to the call in the static scenes track[:, col(c)]"""
    (par, prob, net), moved, geom, S, (x0, xg, ug, p) = _case('z1', 'st', 9)
    B, nq, T = 9, prob.nq, 3
    s = _solver(prob, net)
    s.set_instance_scene(np.repeat(geom[:1], B, axis=0))
    tgt = np.ascontiguousarray(s.eval_nodes(xg, ug, p)['ee'][:, 0, :3])       # reachable targets: the end effector at the starts
    pr = prob
    qs = pr.x_min[:nq] + halton(B * 4, nq, skip=9).reshape(B, 4, nq) * (pr.x_max[:nq] - pr.x_min[:nq])
    idx = tc.track_indices(B, T)
    cell = _cell()
    results = {}
    for c in (None, 0, 1, 2, T + 5, -1):
        s.set_instance_scene_track(geom[idx])
        t = _set_clock(s, cell, c)
        got = s.ik(tgt, qs)
        s.set_instance_scene(geom[idx[:, tc.col(t, T)]])
        ref = s.ik(tgt, qs)
        assert all(np.array_equal(a, b) for a, b in zip(got, ref)), c
        results[c] = got
    assert not np.array_equal(results[0][2], results[2][2])                    # (the column enters the residuals)


def test_score_rollout_scores_state_j_in_column_j_whatever_the_clock():
    """n_steps = 12 > T = 4: d4 within 1e-9 (1 + |.|) of the statement on the track oracle (which evaluates state j in col(j)), the
    places as test_scene_gpu.py holds them; the clock, set to 7, is ignored"""
    from safe_mpc_amd import closed_loop as cl
    (par, prob, net), moved, geom, oracle, base, xg, ug, p = _forward_case()
    B, nq, nr, n_steps, T = FWD_B, prob.nq, len(prob.rows), 12, 4
    rng = np.random.default_rng(3)
    x_log = np.concatenate([np.transpose(xg, (1, 0, 2)), np.transpose(xg[:, :4], (1, 0, 2))])       # [13, B, nx]
    u_log = rng.standard_normal((n_steps, B, nq))
    last_x = np.array([12, 12, 7, 12, 3, 12, 12, 9, 12])
    last_u = np.minimum(last_x, n_steps - 1)
    idx = tc.track_indices(B, T)
    oracle.set_instance_scene_track(geom[idx])
    ocell = np.zeros(1, np.int64)
    oracle.set_scene_clock(ocell)
    ref, refi = cl.score_rollout_statement(oracle, prob, par, x_log, u_log, last_x=last_x, last_u=last_u, per_instance=True, scene_clock=ocell)
    s = _solver(prob, net)
    s.set_instance_scene_track(geom[idx])
    unclocked = s.score_rollout(x_log, u_log, last_x, last_u)
    cell = _cell()
    _set_clock(s, cell, 7)
    so, si = s.score_rollout(x_log, u_log, last_x, last_u)
    assert np.array_equal(so, unclocked[0]) and np.array_equal(si, unclocked[1])
    print('score d4 error', np.abs(so[:, 4] - ref[:, 4]).max())
    assert _close(so[:, :6], ref[:, :6], 1e-9) and np.array_equal(si[:, 2], refi[:, 2])
    # where it was taken: the engine's place holds the statement's maximum; where that stands alone, it is the statement's place
    lo, hi = prob.row_check[:, 0], prob.row_check[:, 1]
    singles = [OracleSolver(m[1], net) for m in moved]
    flat = np.transpose(x_log, (1, 0, 2)).reshape(-1, prob.nx)
    rows = np.array([cl._score_eval_chunks(o, prob, flat, par.alpha, 4096, False)[1].reshape(B, n_steps + 1, nr) for o in singles])
    cols = idx[:, tc.col(np.arange(n_steps + 1), T)]                             # [B, step]: the scene of state j
    rv = rows[cols, np.arange(B)[:, None], np.arange(n_steps + 1)[None, :]]
    m = np.where((np.arange(n_steps + 1)[None, :] <= last_x[:, None])[:, :, None], np.maximum(lo - rv, rv - hi), -np.inf)
    assert _close(m.reshape(B, -1).max(1), ref[:, 4], 1e-12)
    near = m >= (ref[:, 4] - 1e-9 * (1.0 + np.abs(ref[:, 4])))[:, None, None]
    decided = near.reshape(B, -1).sum(1) == 1
    assert near[np.arange(B), si[:, 0], si[:, 1]].all()
    assert np.array_equal(si[decided, :2], refi[decided, :2]) and decided.sum() >= B // 2
    assert (refi[:, 0] >= T).any()                                               # (a worst margin behind the track's last column)
    # the columns enter: every state in column 0 is another score
    s.set_instance_scene(np.ascontiguousarray(geom[idx[:, 0]]))
    assert not np.array_equal(s.score_rollout(x_log, u_log, last_x, last_u)[0][:, 4], so[:, 4])


# ---- 6. smpc_policy_step + smpc_loop_post: the closed loop ------------------------------------------------------------------------------
LOOP_B, LOOP_STEPS, FLIP_TO = 5, 3, 3


@functools.lru_cache(maxsize=None)
def _loop_case(controller):
    """Parameters per scene, the geometry, five starts at rest and their tracks (T = N + 4).  Instance 0 is the flip: a state that
    is free in scene 0 and collides in scene FLIP_TO, both by 5e-3 on the oracle's row values, in the track [0, 0, F, F, ..]: its
    state after step 1 is the first that is tested in scene F.  The others are free in every scene -- CPU only."""
    from safe_mpc_amd import controller as C
    from safe_mpc_amd.problem import scenes_from_problems
    pars = []
    for shift in sc.SHIFTS:
        par, _, _ = make_problem(controller, N=N)
        par.back_hor = 8
        sc.move_obstacles(par, shift, sc.Z1_OBSTACLES)
        pars.append(par)
    probs = [C.OcpProblem(pp, controller, 'ext', N=N) for pp in pars]
    geoms = scenes_from_problems(probs[0], probs)
    pr, nq = probs[0], probs[0].nq
    q = (pr.lbx[:nq] + 0.05) + halton(600, nq, skip=1 + 7 * 5) * (pr.ubx[:nq] - pr.lbx[:nq] - 0.1)
    rest = np.hstack([q, np.zeros_like(q)])
    clear = np.array([_clear_by(p_, rest, 5e-3) for p_ in probs])                     # [scene, state]
    hit = _hit_by(probs[FLIP_TO], rest, 5e-3)
    flip = np.where(clear[0] & hit)[0]
    free = np.where(clear.all(0))[0]
    assert len(flip) >= 1 and len(free) >= LOOP_B - 1
    x0 = np.vstack([rest[flip[0]], rest[free[:LOOP_B - 1]]])
    T = N + 4
    idx = tc.track_indices(LOOP_B, T)
    idx[0] = [0, 0] + [FLIP_TO] * (T - 2)
    return pars, probs, geoms, x0, idx


def _rows_inside(prob, x, by):
    """the oracle's verdict on the states x against the check bounds of the rows moved inwards by ``by`` (in the rows' own units;
    outwards if negative), the box aside"""
    from oracle.oracle import Oracle
    lo, hi = prob.row_check[:, 0], prob.row_check[:, 1]
    return Oracle(prob).check_trajectory(x[:, None, :], prob.x_min, prob.x_max, 1e30, lo + by, hi - by).astype(bool)


def _clear_by(prob, x, by):
    """free, and by at least ``by`` in every row"""
    return _rows_inside(prob, x, by)


def _hit_by(prob, x, by):
    """colliding, and by at least ``by`` in some row"""
    return ~_rows_inside(prob, x, -by)


@pytest.mark.parametrize('controller', ['st', 'receding'])
def test_device_loop_with_tracks_equals_the_host_loop_and_loop_post_reads_column_t_plus_1(controller):
    """three steps of run_mpc(on_device=True, scenes=track) against on_device=False on the same engine, compared as
    test_scene_gpu.py compares its two paths (x 1e-4, u 2e-3 (1 + |u|_inf), NaN patterns and outcome lists equal).  Instance 0's
    state after step 1 is free in column 1 and collides in column 2 (1e-3 either side, on the oracle's row values of the LOGGED
    state): it is marked collided at step 1 -- its log ends with x_2 -- and not one step later, on both paths."""
    from safe_mpc_amd import closed_loop as cl
    from safe_mpc_amd import controller as C
    pars, probs, geoms, x0, idx = _loop_case(controller)
    track = np.ascontiguousarray(geoms[idx])
    xg, ug = np.repeat(x0[:, None, :], N + 1, axis=1), np.zeros((LOOP_B, N, 6))

    def factories(on_device):
        def mk(name, batch):
            c = C.get_controller(name, pars[0], batch, device=0, device_state=on_device)
            c.ocp_solver.set_qp_mode('throughput')
            return c

        def mkb(batch):
            c = C.SafeBackupController(pars[0], batch, device=0, device_state=on_device)
            c.ocp_solver.set_qp_mode('throughput')
            return c
        return mk, mkb
    runs = []
    for on_device in (False, True):
        made = []
        mk, mkb = factories(on_device)

        def mk_log(name, batch, mk=mk, made=made):
            made.append(mk(name, batch))
            return made[-1]
        runs.append(cl.run_mpc(pars[0], controller, xg, ug, n_steps=LOOP_STEPS, on_device=on_device, groups=1, make_controller=mk_log,
                               make_backup=mkb, scenes=track))
        # the handle is left without a track and without a clock: a call of another batch size runs, in the shared scene
        sv = made[0].ocp_solver
        assert getattr(sv, '_scene_clock', None) is None
        assert np.asarray(sv.check_trajectory(x0[:2, None, :])).shape == (2,)
    host, dev = runs
    assert np.array_equal(dev['scenes'], track) and np.array_equal(host['scenes'], track)
    # the flip, on the host path's logged states and the oracle's row values
    x1, x2 = host['x'][0, 1], host['x'][0, 2]
    assert np.isfinite(x1).all() and np.isfinite(x2).all()
    assert _clear_by(probs[0], x1[None], 1e-3)[0] and _clear_by(probs[0], x2[None], 1e-3)[0] and _hit_by(probs[FLIP_TO], x2[None], 1e-3)[0]
    for res in (host, dev):
        assert np.isfinite(res['x'][0, :3]).all() and np.isnan(res['x'][0, 3]).all()       # collided at step 1, not one later
        assert 0 in res['collisions_idx']
    assert np.array_equal(np.isnan(dev['x']), np.isnan(host['x'])) and np.array_equal(np.isnan(dev['u']), np.isnan(host['u']))
    for key in ('conv_idx', 'collisions_idx', 'viable_idx', 'unconv_idx'):
        assert sorted(dev[key]) == sorted(host[key]), key
    tol_x, tol_u = 1e-4, 2e-3 * (1 + np.nanmax(np.abs(host['u'])))
    print(controller, 'closed loop: x error', np.nanmax(np.abs(dev['x'] - host['x'])), 'u error', np.nanmax(np.abs(dev['u'] - host['u'])))
    assert np.nanmax(np.abs(dev['x'] - host['x'])) < tol_x and np.nanmax(np.abs(dev['u'] - host['u'])) < tol_u
    assert np.nanmax(np.abs(host['u'])) > 0


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------
def test_misuse_is_refused_by_name_and_a_clear_restores_the_shared_path():
    import torch
    from safe_mpc_amd import _lib
    from safe_mpc_amd import closed_loop as cl
    from safe_mpc_amd import controller as C
    from safe_mpc_amd._lib import EngineError
    (par, prob, net), moved, geom, S, (x0, xg, ug, p) = _case('z1', 'st', 5)
    B, T, nq = 5, 3, prob.nq
    s = _solver(prob, net)
    tgt, qs = np.zeros((B, 3)) + 0.3, np.zeros((B, 2, nq))
    x_log, u_log = np.ascontiguousarray(np.transpose(xg[:, :4], (1, 0, 2))), np.zeros((3, B, nq))

    def calls(n=B):
        return [s.solve(x0[:n], xg[:n], ug[:n], p[:n]), s.eval_nodes(xg[:n], ug[:n], p[:n]), s.merit_terms(x0[:n], xg[:n], ug[:n], p[:n]),
                s.check_guess(xg[:n], ug[:n]), s.check_trajectory(xg[:n]), s.score_rollout(x_log[:, :n], u_log[:, :n]),
                s.ik(tgt[:n], qs[:n]), s.sqp(x0[:n], xg[:n], ug[:n], p[:n], dict(max_iter=1))[:2]]

    def flat(results):
        out = []
        for r in results:
            for a in (r if isinstance(r, (tuple, list)) else (r,)):
                out.extend([a[f] for f in a.dtype.names] if getattr(a, 'dtype', None) is not None and a.dtype.names else [np.asarray(a)])
        return out
    before = flat(calls())
    track = geom[tc.track_indices(B, T)]
    # T = 0
    L = _lib.lib()
    with pytest.raises(EngineError, match=r'engine error -1: smpc_set_instance_scene_track: T=0'):
        s._chk(L.smpc_set_instance_scene_track(s.h, B, 0, track.ctypes.data, 0))
    with pytest.raises(ValueError, match='at least one time column'):
        s.set_instance_scene_track(track[:, :0])
    with pytest.raises(ValueError, match='expected'):
        s.set_instance_scene_track(track[:, 0])
    with pytest.raises(ValueError, match='one-element int64'):
        s.set_scene_clock(torch.zeros(2, dtype=torch.int64, device='cuda:0'))
    with pytest.raises(ValueError, match='one-element int64'):
        s.set_scene_clock(np.zeros(1, np.int64))
    s.set_instance_scene_track(track)
    moved_results = flat(calls())
    assert not all(np.array_equal(a, b) for a, b in zip(moved_results, before))
    # another batch size: refused by every entry point of the table, both sizes named
    small = (x0[:4], xg[:4], ug[:4], p[:4])
    for call in (lambda: s.solve(*small), lambda: s.eval_nodes(*small[1:]), lambda: s.merit_terms(*small), lambda: s.sqp(*small),
                 lambda: s.check_guess(xg[:4], ug[:4]), lambda: s.check_trajectory(xg[:4]),
                 lambda: s.score_rollout(x_log[:, :4], u_log[:, :4]), lambda: s.ik(tgt[:4], qs[:4]),
                 lambda: _stage_records(s, *small, 1)):
        with pytest.raises((EngineError, AssertionError), match=r'batch size 4, .* 5 instances'):
            call()
    with pytest.raises(EngineError, match=r'engine error -4: smpc_rollout_batch'):
        s.rollout(x0, xg, ug, p, 2)
    # a NaN in a field that is read: refused with its place, the old track stays; in a field no row reads: accepted
    bad = track.copy()
    bad[3, 2, 1, 4] = np.nan
    with pytest.raises(EngineError, match=r'engine error -1: scene track of instance 3, column 2, row 1'):
        s.set_instance_scene_track(bad)
    assert all(np.array_equal(a, b) for a, b in zip(flat(calls()), moved_results))
    ok = track.copy()
    ok[:, :, :, 6:] = np.nan                                       # capsule rows read C and D only
    s.set_instance_scene_track(ok)
    assert all(np.array_equal(a, b) for a, b in zip(flat(calls()), moved_results))
    # growth while the stream is being captured: refused, the old track stays
    import warnings
    big = torch.tensor(np.repeat(track, 4, axis=1), dtype=torch.float64, device='cuda:0')
    with pytest.raises(EngineError, match='engine error -4: .* while the stream is being captured'), warnings.catch_warnings():
        warnings.filterwarnings('ignore', 'The CUDA Graph is empty')
        with torch.cuda.graph(torch.cuda.CUDAGraph()):
            s.set_instance_scene_track(big)
    torch.cuda.synchronize()
    assert all(np.array_equal(a, b) for a, b in zip(flat(calls()), moved_results))
    # cleared (through the scene's entry point): every call is the call without a scene, bit for bit, at any batch size
    s.set_scene_clock(_cell(2))
    s.set_instance_scene(None)
    assert all(np.array_equal(a, b) for a, b in zip(flat(calls()), before))
    s.set_scene_clock(None)
    calls(4)
    s.rollout(x0, xg, ug, p, 2)
    # the device loop's entry points: the parallel policy (ESTATE), and another batch size in smpc_policy_step / smpc_loop_post
    parp, probp, netp = make_problem('parallel', N=4)
    ctrl = C.get_controller('parallel', parp, 3, N=4, device_state=True)
    xp = torch.tensor(sample_instances(probp, 3, seed=2), dtype=torch.float64, device='cuda:0')
    ctrl.setGuess(xp[:, None, :].repeat(1, 5, 1), torch.zeros((3, 4, 6), dtype=torch.float64, device='cuda:0'))
    ctrl.ocp_solver.set_instance_scene_track(np.repeat(ctrl.problem.row_geometry()[None, None], 3, axis=0).repeat(2, axis=1))
    with pytest.raises(EngineError, match=r'engine error -4: smpc_policy_step: .*parallel'):
        ctrl.step_on_device(xp)
    ctrl.ocp_solver.set_instance_scene(None)
    par3, _, _ = make_problem('st', N=N)
    par3.back_hor = 8
    c3, b3 = C.get_controller('st', par3, 3, device_state=True), C.SafeBackupController(par3, 3, device_state=True)
    sv3 = c3.ocp_solver
    with torch.cuda.stream(torch.cuda.ExternalStream(sv3.L.smpc_stream(sv3.h), device=torch.device('cuda', sv3.device))):
        grp = cl._DeviceGroup(par3, xg[:3], ug[:3], 0.0, 0.0, c3, b3, 2, 0, False, use_graphs=False)
    c3.ocp_solver.set_instance_scene_track(track)
    with pytest.raises(EngineError, match=r'engine error -1: smpc_policy_step: batch size 3, .* 5 instances'):
        grp.part_a()
    with pytest.raises(EngineError, match=r'engine error -1: smpc_loop_post: batch size 3, .* 5 instances'):
        grp.part_b()
    c3.ocp_solver.set_instance_scene(None)
    c3.ocp_solver.sync()
