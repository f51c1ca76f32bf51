"""smpc_set_instance_curves on the GPU: a reference curve per instance through smpc_policy_step (k_policy_traj with a per-instance
stride), smpc_score_rollout (k_score_seg with the same), run_mpc and generate_guess.  -m gpu only.

Shapes are curve_cases.py's: N = 10, L = 23; B = 5 (55 threads of k_policy_traj: instances straddle inside one wavefront) and B = 13
(143 threads: instances straddle wavefronts and blocks, an odd batch for the two-instances-per-wavefront interior point); three
curves dealt round-robin; current_step different per instance with one at 0 and one at L + 3; a stepping mask with holes.  What a
curve feeds a solve is a copy, so it is compared to the bit: with the numpy statement, and with the shared-table launch of the same
curve."""
import ctypes

import numpy as np
import pytest

import curve_cases as cc
from conftest import sample_instances

pytestmark = pytest.mark.gpu

MODES = ['throughput', 'latency']


def _ctrl(name, B, mode='throughput', par=None, **kw):
    from safe_mpc_amd import controller as C
    c = C.get_controller(name, par or cc.params(), B, device_state=True, **kw)
    c.ocp_solver.set_qp_mode(mode)
    return c


def _starts(B):
    """B moving collision-free states and the constant guesses at them"""
    from safe_mpc_amd.problem import OcpProblem
    x0 = sample_instances(OcpProblem(cc.params(), 'naive', 'ext', N=cc.N), B, seed=3, vel_scale=0.3)
    return x0, np.repeat(x0[:, None, :], cc.N + 1, axis=1), np.zeros((B, cc.N, 6))


def _prepare(ctrl, xg, ug, cs):
    import torch
    ctrl.setGuess(xg, ug)
    ctrl.current_step = torch.tensor(cs, device='cuda')


def _state(ctrl, u, abort):
    ctrl.ocp_solver.sync()
    keys = ('p', 'x_temp', 'u_temp', 'last_status', 'qp_iter', 'current_step', 'fails', 'x_guess', 'u_guess')
    out = {k: getattr(ctrl, k).cpu().numpy().copy() for k in keys}
    out['u_out'], out['abort_out'] = u.cpu().numpy().copy(), abort.cpu().numpy().copy()
    return out


def _step(ctrl, x, stepping, u_other):
    import torch
    t = lambda a: torch.tensor(a, device='cuda')          # noqa: E731
    u, a = ctrl.step_on_device(t(x), t(stepping), t(u_other))
    return _state(ctrl, u, a)


# ---- arguments ---------------------------------------------------------------------------------------------------------------------
def test_misuse_is_refused_by_name():
    import torch
    from safe_mpc_amd._lib import EngineError
    B = 5
    ctrl = _ctrl('naive', B)
    sv, Lib = ctrl.ocp_solver, ctrl.ocp_solver.L
    x0, xg, ug = _starts(B)
    ctrl.setGuess(xg, ug)
    xd = torch.tensor(x0, device='cuda')
    x_log, u_log = np.repeat(x0[None], 3, axis=0), np.zeros((2, B, 6))
    curves = cc.dealt(B)
    err = lambda: Lib.smpc_last_error(sv.h).decode()      # noqa: E731
    # a score against curves that are not there is today's error
    with pytest.raises(EngineError, match='neither ee_ref nor traj'):
        sv.score_rollout(x_log, u_log, traj='instance')
    # another B: both sizes by name, on both entry points
    sv.set_instance_curves(cc.dealt(4))
    with pytest.raises(EngineError, match=r'engine error -1: smpc_policy_step: batch size 5, .* set for 4 instances'):
        ctrl.step_on_device(xd)
    with pytest.raises(EngineError, match=r'engine error -1: smpc_score_rollout: batch size 5, .* set for 4 instances'):
        sv.score_rollout(x_log, u_log, traj='instance')
    sv.score_rollout(x_log, u_log)                           # with a pointer given the call is today's, whatever the curves' size
    sv.score_rollout(x_log, u_log, traj=curves[0])
    # two sources for one input
    sv.set_instance_curves(curves)
    ctrl.setTrajectory(curves[0])                            # (the controller held no curves: the handle keeps the ones set above)
    with pytest.raises(EngineError, match=rf'engine error -1: smpc_policy_step: st->traj given \(traj_len {cc.L}\) while instance curves '
                                          rf'are set \({B} instances, {cc.L} columns\)'):
        ctrl.step_on_device(xd)
    # a NaN in a host table, L = 0, B = 0: refused, and the curves held stay
    bad = curves.copy()
    bad[3, 1, 7] = np.nan
    with pytest.raises(EngineError, match=rf'engine error -1: curve of instance 3 \(of B={B}\), axis 1, column 7 \(of L={cc.L}\) is not finite'):
        sv.set_instance_curves(bad)
    ptr = curves.ctypes.data
    assert Lib.smpc_set_instance_curves(sv.h, B, 0, ptr, 0) == -1 and f'B={B}, L=0' in err()
    assert Lib.smpc_set_instance_curves(sv.h, 0, cc.L, ptr, 0) == -1 and f'B=0, L={cc.L}' in err()
    assert Lib.smpc_set_instance_curves(sv.h, -2, ctypes.c_int64(-1), ptr, 0) == -1
    out, _ = sv.score_rollout(x_log, u_log, traj='instance')
    ref, _ = sv.score_rollout(x_log, u_log, traj=curves)     # (the ones held: not handed over again)
    assert np.array_equal(out, ref) and np.all(np.isfinite(out[:, :4]))
    # after NULL the shared path works again
    sv.set_instance_curves(None)
    ctrl.step_on_device(xd)
    sv.sync()
    assert np.array_equal(ctrl.p.cpu().numpy()[:, :, :3], cc.p_statement(np.repeat(curves[:1], B, axis=0), np.zeros(B, np.int64)))
    assert sv.L.smpc_abi_version() == 5


# ---- the same curve for everybody = the shared table -----------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', ['naive', 'stwa', 'receding', 'parallel'])
def test_one_curve_for_all_equals_the_shared_table(name, mode):
    """B = 5, every instance holding the same curve: one policy step is the step with that curve as st->traj, to the bit"""
    B = 5
    x0, xg, ug = _starts(B)
    cs, stp = cc.current_steps(B), cc.stepping(B)
    u_other = np.random.default_rng(1).normal(size=(B, 6))
    curve = cc.three_curves()[1]
    shared, own = _ctrl(name, B, mode), _ctrl(name, B, mode)
    shared.setTrajectory(curve)
    own.setTrajectory(np.repeat(curve[None], B, axis=0))
    assert own.traj.ndim == 3 and own.ocp_solver._holds_curves(own.traj)
    got = []
    for c in (shared, own):
        _prepare(c, xg, ug, cs)
        got.append(_step(c, x0, stp, u_other))
    for k in ('p', 'x_temp', 'u_temp', 'last_status', 'qp_iter', 'u_out', 'abort_out', 'current_step', 'fails'):
        assert np.array_equal(got[0][k], got[1][k]), k
    assert np.array_equal(got[1]['p'][stp][:, :, :3], cc.p_statement(np.repeat(curve[None], B, axis=0), cs)[stp])
    assert (got[1]['last_status'][stp] == 0).any()


# ---- a curve per instance -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', ['stwa', 'receding', 'parallel'])
def test_distinct_curves_feed_every_instance_its_own_columns(name, mode):
    """B = 13, three curves round-robin, two consecutive steps: p is the numpy statement to the bit and untouched where the instance
    did not step; the owners of curve c agree bit for bit with the same batch stepped under the shared traj = c"""
    B = 13
    x0, xg, ug = _starts(B)
    cs0, stp, own_of = cc.current_steps(B), cc.stepping(B), cc.owner(B)
    curves = cc.dealt(B)
    rng = np.random.default_rng(2)
    ctrls = [_ctrl(name, B, mode) for _ in range(4)]               # [0]: a curve per instance; [1 + c]: the shared curve c
    ctrls[0].setTrajectory(curves)
    for c in range(3):
        ctrls[1 + c].setTrajectory(cc.three_curves()[c])
    for c in ctrls:
        _prepare(c, xg, ug, cs0)
    x, cs = x0.copy(), cs0.copy()
    p_before = ctrls[0].p.cpu().numpy().copy()
    for t in range(2):
        u_other = rng.normal(size=(B, 6))
        got = [_step(c, x, stp, u_other) for c in ctrls]
        mine = got[0]
        want = cc.p_statement(curves, cs)
        assert np.array_equal(mine['p'][stp][:, :, :3], want[stp]), t
        assert np.array_equal(mine['p'][~stp], p_before[~stp]), t
        if name == 'stwa':
            assert np.array_equal(mine['p'][:, :, 3:], p_before[:, :, 3:]), t
        for c in range(3):
            m = (own_of == c) & stp
            assert m.sum() >= 2
            for k in ('p', 'x_temp', 'u_temp', 'last_status', 'u_out', 'abort_out', 'current_step'):
                assert np.array_equal(mine[k][m], got[1 + c][k][m]), (t, c, k)
            others = (own_of != c) & stp
            assert not np.array_equal(mine['p'][others], got[1 + c]['p'][others])
        assert (mine['last_status'][stp] == 0).any()
        # the step counters advance (not where the instance aborted or did not step): the second step reads the next columns
        assert np.array_equal(mine['current_step'], cs + (stp & ~mine['abort_out'].astype(bool)))
        cs, p_before = mine['current_step'], mine['p']
        x = x + cc.params().dt * np.hstack([x[:, 6:], mine['u_out']])
    assert (cs != cs0).any()


def test_curves_are_overwritten_in_place_and_cleared_by_the_controller():
    """setTrajectory with the same [B, 3, L] updates the controller's tensor and the handle's copy in place (a captured step keeps
    both addresses); the next step reads the new curves; back to [3, L] the handle holds none and the shared table is read"""
    import torch
    B = 5
    x0, xg, ug = _starts(B)
    cs = cc.current_steps(B)
    ctrl = _ctrl('naive', B)
    curves = cc.dealt(B)
    ctrl.setTrajectory(curves)
    held = ctrl.traj
    _prepare(ctrl, xg, ug, cs)
    xd = torch.tensor(x0, device='cuda')
    ctrl.step_on_device(xd)
    ctrl.ocp_solver.sync()
    assert np.array_equal(ctrl.p.cpu().numpy()[:, :, :3], cc.p_statement(curves, cs))
    moved = curves[::-1] + 0.01
    ctrl._traj_rebound = False
    ctrl.setTrajectory(moved)
    assert ctrl.traj is held and not ctrl._traj_rebound and ctrl.ocp_solver._holds_curves(held)
    ctrl.current_step = torch.tensor(cs, device='cuda')
    ctrl.step_on_device(xd)
    ctrl.ocp_solver.sync()
    assert np.array_equal(ctrl.p.cpu().numpy()[:, :, :3], cc.p_statement(moved, cs))
    ctrl.setTrajectory(curves[2])
    assert ctrl._traj_rebound and not ctrl.ocp_solver._holds_curves(held)
    ctrl.current_step = torch.tensor(cs, device='cuda')
    ctrl.step_on_device(xd)                                  # (would be refused as "two sources" had the handle kept the curves)
    ctrl.ocp_solver.sync()
    assert np.array_equal(ctrl.p.cpu().numpy()[:, :, :3], cc.p_statement(np.repeat(curves[2:3], B, axis=0), cs))


# ---- the score ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cols', [cc.L, 4])
def test_score_against_the_held_curves(cols):
    """6-step logs, B = 13: the owners of curve c are the call with the shared traj = c to the bit; the whole result is the numpy
    statement on the CPU oracle at test_score_gpu.py's 1e-9 (1 + |.|), integer slots equal.  cols = 4: curves shorter than the log"""
    from fake_solver import OracleSolver
    from safe_mpc_amd import closed_loop as cl
    from safe_mpc_amd.problem import OcpProblem
    from safe_mpc_amd.solver import BatchedOcpSolver
    B, T = 13, 6
    par = cc.params()
    prob = OcpProblem(par, 'naive', 'ext', N=cc.N)
    sv = BatchedOcpSolver(prob, None)
    rng = np.random.default_rng(2)
    x = np.stack([sample_instances(prob, B, seed=s, vel_scale=0.2) for s in range(T + 1)])
    u = rng.normal(size=(T, B, 6))
    lx = np.array([T, T, 3, T, 0, T, T, 5, T, T, 2, T, T], np.int64)
    lu = np.minimum(lx, T - 1)
    curves = np.ascontiguousarray(cc.dealt(B)[:, :, :cols])
    out, outi = sv.score_rollout(x, u, lx, lu, traj=curves)
    held, heldi = sv.score_rollout(x, u, lx, lu, traj='instance')
    assert np.array_equal(out, held) and np.array_equal(outi, heldi)
    for c in range(3):
        so, si = sv.score_rollout(x, u, lx, lu, traj=np.ascontiguousarray(cc.three_curves()[c][:, :cols]))
        m = cc.owner(B) == c
        assert np.array_equal(out[m], so[m]) and np.array_equal(outi[m], si[m]), c
        assert np.all(out[~m, 1] != so[~m, 1])
    ro, ri = cl.score_rollout_statement(OracleSolver(prob, None), prob, par, x, u, lx, lu, traj=curves)
    with np.errstate(invalid='ignore'):
        err = np.where(np.isinf(ro), (out != ro).astype(float), np.abs(out - ro) / (1.0 + np.abs(ro)))
    print('score with held curves, columns', cols, ': error', err.max(0))
    assert np.array_equal(outi, ri) and err[:, :6].max() <= 1e-9 and np.all(out[:, 6] == np.inf)
    # device pointers: the same bits
    import torch
    t = lambda a: torch.tensor(a, device='cuda')          # noqa: E731
    od, oid = sv.score_rollout(t(x), t(u), t(lx), t(lu), traj=t(curves))
    sv.sync()
    assert np.array_equal(od.cpu().numpy(), out) and np.array_equal(oid.cpu().numpy(), outi)


# ---- the closed loop ------------------------------------------------------------------------------------------------------------------
def test_device_closed_loop_on_two_curves_equals_the_per_curve_loops():
    """run_mpc on the fused device path, 'htwa', B = 4 on two curves interleaved, 6 steps, QP form pinned: against the two
    single-curve device loops, at the tolerances test_scene_gpu.py holds the two-scene loop to (1e-4 in x, 2e-3 (1 + max |u|) in u;
    outcome lists equal), the per-curve loops being first shown to be more than 100 x those apart.  Afterwards the handle holds no
    curves: a step with a shared traj on the same solver goes through."""
    import torch
    from safe_mpc_amd import closed_loop as cl
    from safe_mpc_amd import controller as C
    from safe_mpc_amd.problem import OcpProblem
    par, steps, B = cc.params(), 6, 4
    x0 = sample_instances(OcpProblem(par, 'htwa', 'ext', N=cc.N), 2, seed=5, vel_scale=0.1)[[0, 0, 1, 1]]     # each start on both curves
    xg, ug = np.repeat(x0[:, None, :], cc.N + 1, axis=1), np.zeros((B, cc.N, 6))
    own = np.array([0, 1, 0, 1])
    curves = np.ascontiguousarray(cc.loop_curves()[own])
    made = []

    def mk(name, batch):
        made.append(_ctrl(name, batch, 'throughput', par=par))
        return made[-1]

    def mkb(batch):
        c = C.SafeBackupController(par, batch, device=0, device_state=True)
        c.ocp_solver.set_qp_mode('throughput')
        return c
    kw = dict(n_steps=steps, on_device=True, groups=1, make_controller=mk, make_backup=mkb, score=True)
    parts = [cl.run_mpc(par, 'htwa', xg[own == c], ug[own == c], traj=cc.loop_curves()[c], **kw) for c in (0, 1)]
    tol_x, tol_u = 1e-4, 2e-3 * (1 + max(np.nanmax(np.abs(q['u'])) for q in parts))
    apart_x, apart_u = np.nanmax(np.abs(parts[0]['x'] - parts[1]['x'])), np.nanmax(np.abs(parts[0]['u'] - parts[1]['u']))
    print('closed loop: between the curves: x', apart_x, 'u', apart_u, '; tolerances', tol_x, tol_u)
    assert apart_x >= 100 * tol_x and apart_u >= 100 * tol_u
    res = cl.run_mpc(par, 'htwa', xg, ug, traj=curves, **kw)
    for c in (0, 1):
        m = own == c
        assert np.array_equal(np.isnan(res['x'][m]), np.isnan(parts[c]['x'])) and np.array_equal(np.isnan(res['u'][m]), np.isnan(parts[c]['u']))
        ex, eu = np.nanmax(np.abs(res['x'][m] - parts[c]['x'])), np.nanmax(np.abs(res['u'][m] - parts[c]['u']))
        print('closed loop: curve', c, 'x error', ex, 'u error', eu)
        assert ex < tol_x and eu < tol_u
        # each instance was scored against ITS curve (the other one is 15 cm away).  States within tol_x = 1e-4 move the end effector of
        # a 1 m arm with six joints by at most 6e-4: that for ee_dist, and 7 states x 2 |e| x 6e-4 < 1e-2 (|e| < 1) for ee_err2
        for key, tol in (('ee_dist', 6e-4), ('ee_err2', 1e-2)):
            got, ref = res['score'][key][m], parts[c]['score'][key]
            assert np.all(np.abs(got - ref) <= tol), (c, key, got, ref)
        assert np.all(res['score']['ee_dist'][m] < 1.0)
    for key in ('conv_idx', 'collisions_idx', 'viable_idx', 'unconv_idx'):
        assert sorted(res[key]) == sorted(int(np.where(own == c)[0][i]) for c, q in enumerate(parts) for i in q[key]), key
    # the run leaves the handle without curves
    sv = made[-1].ocp_solver
    again = C.get_controller('htwa', par, B, device_state=True, solver=sv, net=made[-1].net)
    again.setGuess(xg, ug)
    again.setTrajectory(cc.loop_curves()[0])
    again.step_on_device(torch.tensor(x0, device='cuda'))
    sv.sync()
    assert np.array_equal(again.p.cpu().numpy()[:, :, :3], cc.p_statement(np.repeat(cc.loop_curves()[:1], B, axis=0), np.zeros(B, np.int64)))


# ---- warm starts ------------------------------------------------------------------------------------------------------------------
def test_generate_guess_on_device_with_a_curve_per_instance():
    """generate_guess(on_device=True, traj=[4, 3, L]) on two curves interleaved: every start that did not fail sits on the first
    point of ITS curve within the IK's tol_ee = 1e-6 (through smpc_eval_nodes), and instance i is instance i of the single-curve run
    with its curve (same accepted set, 1e-4 (1 + |.|_inf) as test_scene_gpu.py holds the two-scene warm starts to)"""
    from safe_mpc_amd import closed_loop as cl
    from safe_mpc_amd import controller as C
    par, n = cc.params(), 4
    own = np.array([0, 1, 0, 1])
    two = cc.three_curves()[[0, 1]]
    curves = np.ascontiguousarray(two[own])

    def mk(name, batch):
        c = C.get_controller(name, par, batch)
        c.ocp_solver.set_qp_mode('throughput')
        return c
    got, mask = cl.generate_guess(par, 'naive', n, make_controller=mk, on_device=True, traj=curves)
    assert mask.shape == (n,) and not mask[got['ik_failed']].any() and mask.sum() >= 2
    assert np.array_equal(got['curves'], curves[mask])
    m = int(mask.sum())
    sv = mk('naive', m).ocp_solver
    p = np.zeros((m, cc.N + 1, 5))
    ee = np.asarray(sv.eval_nodes(got['xg'], got['ug'], p)['ee'])[:, 0, :]
    print('generate_guess: accepted', mask.tolist(), '|ee(x0) - curve start|', np.abs(ee - curves[mask][:, :, 0]).max(1))
    assert np.all(np.abs(ee - curves[mask][:, :, 0]).max(1) <= 1e-6) and np.all(got['xg'][:, 0, 6:] == 0.0)
    assert np.abs(two[0][:, 0] - two[1][:, 0]).max() > 1e-2
    single = [cl.generate_guess(par, 'naive', n, make_controller=mk, on_device=True, traj=two[c]) for c in (0, 1)]
    k = 0
    for i in range(n):
        g1, m1 = single[own[i]]
        assert m1[i] == mask[i] and (i in g1['ik_failed']) == (i in got['ik_failed']), i
        if not mask[i]:
            continue
        j = int(m1[:i].sum())
        assert np.array_equal(got['xg'][k, 0], g1['xg'][j, 0]), i           # the IK start: an instance's own Halton block, to the bit
        for a, b in ((got['xg'][k], g1['xg'][j]), (got['ug'][k], g1['ug'][j])):
            assert np.abs(a - b).max() <= 1e-4 * (1.0 + np.abs(b).max()), i
        k += 1
