"""A scene of its own for every instance (smpc_set_instance_scene) on the GPU.  -m gpu only.

Every statement is held against the CPU oracle called once per distinct scene, on the problem built from that scene's MOVED
PARAMETERS (scene_cases.py) -- the oracle knows nothing of scenes.  Tolerances are those of the tests that pin the same calls on the
shared scene: 1e-9 relative for the linearisation pieces (test_eval_nodes_parity), 1e-4 (1 + |u|_inf) for an RTI solve with the
network row (the 'st' row of test_rti_solve_parity), equality for verdicts and integer slots (test_callers_parity), 1e-9 (1 + |.|)
for FP64 margins (test_guess_until_gpu.py, test_score_gpu.py).

Scenes: base = make_problem('st', N = 30), the three gate capsules moved together by scene_cases.SHIFTS; states =
sample_instances(base, 24, seed = 5, vel_scale = 0.1)."""
import functools
import types

import numpy as np
import pytest

import scene_cases as sc
from conftest import constant_guess, make_problem, sample_instances
from fake_solver import OracleSolver

pytestmark = pytest.mark.gpu

N_ST = 30


def _rel(a, b):
    return np.abs(a - b).max() / (1e-12 + np.abs(b).max())


def _close(got, ref, tol):
    same_inf = np.isinf(ref) & (got == ref)
    with np.errstate(invalid='ignore'):
        return np.all(same_inf | (np.abs(got - ref) <= tol * (1.0 + np.abs(ref))))


def _oracle(prob, net):
    from oracle.oracle import Oracle
    return Oracle(prob, (net.weights, net.biases))


def _solver(prob, net, mode=None):
    from safe_mpc_amd.solver import BatchedOcpSolver
    s = BatchedOcpSolver(prob, net)
    if mode is not None:
        s.set_qp_mode(mode)
    return s


@functools.lru_cache(maxsize=None)
def _st():
    """the 'st' family: base, moved problems, geometry [4, 6, 8], one oracle per scene, the 24 states and which are free where"""
    base, moved, geom = sc.scene_family('z1', 'st', N_ST, 4)
    oracles = [_oracle(m[1], m[2]) for m in moved]
    x = sample_instances(base[1], 24, seed=5, vel_scale=0.1)
    pr, par = base[1], base[0]
    free = np.array([o.check_trajectory(x[:, None, :], pr.x_min, pr.x_max, par.tol_x, pr.row_check[:, 0], pr.row_check[:, 1])
                     for o in oracles]).astype(bool)                 # [scene, state]
    return base, moved, geom, oracles, x, free


# ---- a. linearisation ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('system,controller,n_scenes', [('z1', 'naive', 4), ('fr7', 'constraint_everywhere', 3)])
def test_eval_nodes_in_every_instances_own_scene(system, controller, n_scenes):
    """n_scenes x 3 instances, N = 12, inputs perturbed as in test_eval_nodes_parity: every FP64 field within 1e-9 relative of the
    oracle of the instance's scene (the network's row at that test's 2e-5 / 2e-4); the rows do differ between the scenes"""
    (par, prob, net), moved, geom = sc.scene_family(system, controller, 12, n_scenes)
    nq, nr = prob.nq, len(prob.rows)
    B = 3 * n_scenes
    idx = np.arange(B) % n_scenes                              # scenes interleaved over the batch
    x0 = sample_instances(prob, B, seed=1, vel_scale=0.5)
    xg, ug, p = constant_guess(prob, x0)
    rng = np.random.default_rng(0)
    xg[:, 1:] += 0.05 * rng.standard_normal(xg[:, 1:].shape)
    ug += rng.uniform(-5, 5, ug.shape)
    s = _solver(prob, net)
    s.set_instance_scene(geom[idx])
    a = s.eval_nodes(xg, ug, p)
    oracles = [_oracle(m[1], m[2]) for m in moved]
    b = sc.by_scene(lambda sn, m: oracles[sn].eval_nodes(xg[m], ug[m], p[m]), idx, B)
    for f, n in [('tau', nq), ('M', nq * nq), ('dtau_dq', nq * nq), ('dtau_dv', nq * nq), ('ee', 3), ('cost_grad_q', nq),
                 ('cost_hess_qq', nq * nq), ('row_val', nr), ('row_grad', nr * nq)]:
        err = _rel(a[f][..., :n], b[f][..., :n])
        print(system, f, err)
        assert err < 1e-9, f
    if controller != 'naive':
        assert _rel(a['nn_val'], b['nn_val']) < 2e-5
        assert _rel(a['nn_grad'][..., :2 * nq], b['nn_grad'][..., :2 * nq]) < 2e-4
    # precondition of the whole file: the scenes are told apart (the base oracle is off by far more than the tolerance)
    shared = oracles[0].eval_nodes(xg, ug, p)
    moved_rows = idx != 0
    assert _rel(shared['row_val'][moved_rows][..., :nr], b['row_val'][moved_rows][..., :nr]) > 1e-3
    # and the device-pointer path gives the bits of the host path
    import torch
    dev = lambda v: torch.tensor(v, dtype=torch.float64, device='cuda:0')
    s.set_instance_scene(dev(geom[idx]))
    d = s.eval_nodes(dev(xg), dev(ug), dev(p))
    s.sync()
    assert np.array_equal(d['row_val'].cpu().numpy(), a['row_val']) and np.array_equal(d['row_grad'].cpu().numpy(), a['row_grad'])


# ---- b. verdicts and margins ----------------------------------------------------------------------------------------------------------
def test_verdicts_and_margins_follow_the_scene():
    """all 24 states through all four scenes as one batch of 96: check_trajectory, check_guess (bit 1, worst[1]), merit_terms (viol)
    and score_rollout (d4, i0, i1 over a 3-step log) against the per-scene oracle statements"""
    from safe_mpc_amd import closed_loop as cl
    (par, prob, net), moved, geom, oracles, x, free = _st()
    # precondition: a state with different oracle verdicts in two scenes
    assert (free.any(0) & ~free.all(0)).any(), free.sum(1)
    S, n = 4, len(x)
    B = S * n
    idx = np.repeat(np.arange(S), n)
    xs = np.tile(x, (S, 1))
    s = _solver(prob, net)
    s.set_instance_scene(geom[idx])
    # check_trajectory: the verdict of the instance's scene
    ok = s.check_trajectory(xs[:, None, :])
    assert np.array_equal(ok, free.reshape(-1))
    # a short trajectory per instance: three small steps away from the state (so the nodes differ)
    rng = np.random.default_rng(7)
    nq, nr, N = prob.nq, len(prob.rows), prob.N
    xg, ug, p = constant_guess(prob, xs, flag=-1.0)            # (safe-set row off: viol is FP64 end to end)
    xg[:, 1:, :nq] += 0.02 * rng.standard_normal((B, N, nq)) * (np.arange(1, N + 1) <= 3)[None, :, None]
    ev = sc.by_scene(lambda sn, m: oracles[sn].eval_nodes(xg[m], ug[m], p[m]), idx, B)
    rv = ev['row_val'][..., :nr]
    lo, hi = prob.row_check[:, 0], prob.row_check[:, 1]
    for coll_first in (1, 0):
        w_ref = np.maximum(lo - rv, rv - hi)[:, :1 if coll_first else N + 1].reshape(B, -1).max(1)
        assert np.all(np.abs(w_ref) > 1e-7)                      # no verdict within rounding of its threshold
        flags, worst = s.check_guess(xg, ug, collision_first_node=coll_first)
        print('check_guess', coll_first, 'worst[1] error', np.abs(worst[:, 1] - w_ref).max(), 'colliding', int((w_ref > 0).sum()))
        assert np.array_equal((flags >> 1) & 1, (~(w_ref <= 0.0)).astype(np.int32))
        assert _close(worst[:, 1], w_ref, 1e-9)
        assert 0 < (w_ref > 0).sum() < B
    # merit_terms: the l1 violation, by the numpy statement on the scene's oracle
    def viol_of(sn, m):
        ctrl = types.SimpleNamespace(problem=moved[sn][1], ocp_solver=OracleSolver(moved[sn][1], net), p=p[m], nq=nq, N=N, params=par)
        return cl.merit_terms(ctrl, xs[m], xg[m], ug[m])[3]
    v_ref = sc.by_scene(viol_of, idx, B)
    out = s.merit_terms(xs, xg, ug, p)
    print('merit viol error', np.abs(out[:, 1] - v_ref).max())
    assert _close(out[:, 1], v_ref, 1e-9)
    v_base = viol_of(0, np.arange(B))
    assert np.abs(v_base - v_ref).max() > 1e-4                   # (the scenes are told apart)
    # score_rollout: worst collision margin of a 3-step log and where it was taken
    x_log = np.ascontiguousarray(np.transpose(xg[:, :4], (1, 0, 2)))
    u_log = np.zeros((3, B, nq))
    sref = sc.by_scene(lambda sn, m: cl.score_rollout_statement(OracleSolver(moved[sn][1], net), moved[sn][1], par, x_log[:, m],
                                                                u_log[:, m]), idx, B)
    so, si = s.score_rollout(x_log, u_log)
    print('score d4 error', np.abs(so[:, 4] - sref[0][:, 4]).max())
    assert _close(so[:, 4], sref[0][:, 4], 1e-9)
    # Where it was taken.  Capsules fixed2 and fixed3 share an end point: a robot capsule nearest to that corner is EXACTLY as far
    # from the one as from the other, and which of the two rows holds the maximum is then a matter of the last bit.  So: the
    # engine's place holds the maximum of the oracle's margins (to the 1e-9 of the value), and wherever the oracle's maximum
    # stands clear of every other entry by more than that, the place is the statement's.
    m = np.maximum(lo - rv[:, :4], rv[:, :4] - hi)                  # [B, step, row]
    near = m >= (sref[0][:, 4] - 1e-9 * (1.0 + np.abs(sref[0][:, 4])))[:, None, None]
    decided = near.reshape(B, -1).sum(1) == 1
    print('score slots: decided', int(decided.sum()), 'of', B, '; equal', int((si[:, :2] == sref[1][:, :2]).all(1).sum()))
    assert near[np.arange(B), si[:, 0], si[:, 1]].all()
    # (counted on the oracle: 35 of the 96 worst margins are such exact ties between the two rows, 61 stand alone)
    assert np.array_equal(si[decided, :2], sref[1][decided, :2]) and decided.sum() == 61


# ---- c. the solve -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _solve_reference():
    """8 states free in every scene x 4 scenes, three consecutive RTI steps of the per-scene oracles from constant_guess, each
    from the oracle's previous iterate: [(xg, ug, x_ref, u_ref, status_ref)] per step, the inputs, the scene of every instance"""
    (par, prob, net), moved, geom, oracles, x, free = _st()
    good = np.where(free.all(0))[0]
    assert len(good) == 23
    x8 = x[good[:8]]
    idx = np.tile(np.arange(4), 8)                             # instance i: state i // 4 in scene i % 4
    x0 = np.repeat(x8, 4, axis=0)
    xg, ug, p = constant_guess(prob, x0)
    steps = []
    for _ in range(3):
        xr, ur, sr, _ = sc.by_scene(lambda sn, m: oracles[sn].solve_batch(x0[m], xg[m], ug[m], p[m]), idx, 32)
        steps.append((xg, ug, xr, ur, sr))
        xg, ug = xr, ur
    return x0, p, idx, steps


@pytest.mark.parametrize('qp_mode', ['throughput', 'latency'])
@pytest.mark.parametrize('B', [32, 31])
def test_solve_in_every_instances_own_scene(qp_mode, B):
    """one batch of 8 states x 4 scenes (and 31 of them: an odd last wavefront), both forms of the interior point: statuses equal,
    |u - u_ref| < 1e-4 (1 + max |u_ref|) at each of three RTI steps"""
    (par, prob, net), moved, geom, oracles, x, free = _st()
    x0, p, idx, steps = _solve_reference()
    # preconditions: every oracle status is 0, and the scenes move some instance's controls by >= 100 x the tolerance
    assert all(np.all(st[4] == 0) for st in steps)
    # (the first step, from the constant guess, has no active row yet; the second and third do)
    apart = [np.abs(st[3].reshape(8, 4, -1) - st[3].reshape(8, 4, -1)[:, :1]).max() / (1e-4 * (1 + np.abs(st[3]).max())) for st in steps]
    assert max(apart) >= 100, apart
    s = _solver(prob, net, qp_mode)
    s.set_instance_scene(geom[idx[:B]])
    for k, (xg, ug, xr, ur, sr) in enumerate(steps):
        xa, ua, sa, ia = s.solve(x0[:B], xg[:B], ug[:B], p[:B])
        err = np.abs(ua - ur[:B]).max()
        print(qp_mode, B, 'step', k, 'status', sa.tolist(), 'u error', err, 'bound', 1e-4 * (1 + np.abs(ur[:B]).max()))
        assert np.array_equal(sa, sr[:B])
        assert err < 1e-4 * (1 + np.abs(ur[:B]).max())


@pytest.mark.parametrize('system,nq,drop_rows,B', [('z1', 5, 1, 5), ('z1', 6, 2, 3), ('fr7', 7, 0, 5)])
def test_solve_in_scenes_other_instantiations(system, nq, drop_rows, B):
    """the scene-aware stage builder's other instantiations -- a runtime row count (nq = 5, five rows), the four-row one (six less
    two; fr7's sphere, sphere, point and plane rows at nq = 7) -- at odd batch sizes, against the per-scene oracles"""
    n_scenes = 2
    if system == 'z1':
        fam = [sc.moved_problem('z1', 'st', 12, sh, nq=nq) for sh in sc.SHIFTS[:n_scenes]]
    else:
        fam = [sc.moved_problem('fr7', 'constraint_everywhere', 12, sh) for sh in sc.SHIFTS[:n_scenes]]
    for par, pr, net in fam:
        pr.desc.n_rows -= drop_rows                            # (the last capsule pairs go, as in test_kernel_instantiations_and_odd_batches)
    par, prob, net = fam[0]
    nr = prob.desc.n_rows
    geom = np.array([pr.row_geometry()[:nr] for _, pr, _ in fam])
    idx = np.arange(B) % n_scenes
    x0 = sample_instances(prob, B, seed=5, vel_scale=0.1)
    xg, ug, p = constant_guess(prob, x0)
    oracles = [_oracle(pr, nt) for _, pr, nt in fam]
    xr, ur, sr, _ = sc.by_scene(lambda sn, m: oracles[sn].solve_batch(x0[m], xg[m], ug[m], p[m]), idx, B)
    s = _solver(prob, net)
    from safe_mpc_amd import _lib
    g = np.ascontiguousarray(geom[idx])
    s._chk(_lib.lib().smpc_set_instance_scene(s.h, B, g.ctypes.data, 0))      # (the row count was changed behind the Python problem)
    xa, ua, sa, ia = s.solve(x0, xg, ug, p)
    ok = sr == 0
    print(system, nq, nr, 'status', sa.tolist(), sr.tolist(), 'u error', np.abs(ua[ok] - ur[ok]).max())
    assert np.array_equal(sa, sr) and ok.sum() >= B - 1
    assert np.abs(ua[ok] - ur[ok]).max() < 1e-4 * (1 + np.abs(ur[ok]).max())
    ev_a = s.eval_nodes(xg, ug, p)
    ev_b = sc.by_scene(lambda sn, m: oracles[sn].eval_nodes(xg[m], ug[m], p[m]), idx, B)
    assert _rel(ev_a['row_val'][..., :nr], ev_b['row_val'][..., :nr]) < 1e-9
    assert _rel(ev_a['row_grad'][..., :nr * prob.nq], ev_b['row_grad'][..., :nr * prob.nq]) < 1e-9


# ---- d. the shared path and isolation -------------------------------------------------------------------------------------------------
def test_base_scene_equals_the_shared_path_and_instances_are_isolated():
    """every instance in the BASE geometry against the same calls without a scene (eval_nodes 1e-9 relative, solve 1e-4
    (1 + |u|_inf); whether the bits are equal is printed); moving ONE instance's obstacles leaves every other instance's
    eval_nodes, solve and score bit-identical; clearing the scene restores the shared results bit for bit"""
    (par, prob, net), moved, geom, oracles, x, free = _st()
    x0, p, idx, steps = _solve_reference()
    B, nr, nq = 32, len(prob.rows), prob.nq
    xg, ug = steps[1][0], steps[1][1]
    x_log = np.ascontiguousarray(np.transpose(xg[:, :4], (1, 0, 2)))
    u_log = np.ascontiguousarray(np.transpose(ug[:, :3], (1, 0, 2)))
    for mode in ('throughput', 'latency'):
        s = _solver(prob, net, mode)

        def calls():
            ev = s.eval_nodes(xg, ug, p)
            return ev, s.solve(x0, xg, ug, p), s.score_rollout(x_log, u_log)
        ev0, sol0, sc0 = calls()
        s.set_instance_scene(np.repeat(geom[:1], B, axis=0))
        ev1, sol1, sc1 = calls()
        for f, n in [('ee', 3), ('cost_grad_q', nq), ('row_val', nr), ('row_grad', nr * nq), ('tau', nq), ('M', nq * nq)]:
            assert _rel(ev1[f][..., :n], ev0[f][..., :n]) < 1e-9, f
        assert np.array_equal(sol1[2], sol0[2])
        assert np.abs(sol1[1] - sol0[1]).max() < 1e-4 * (1 + np.abs(sol0[1]).max())
        assert _close(sc1[0][:, :6], sc0[0][:, :6], 1e-9) and np.array_equal(sc1[1], sc0[1])
        print(mode, 'base scene vs shared path, bits equal:', 'eval_nodes', all(np.array_equal(ev1[f], ev0[f]) for f in ev0.dtype.names),
              'solve', np.array_equal(sol1[0], sol0[0]) and np.array_equal(sol1[1], sol0[1]) and np.array_equal(sol1[3], sol0[3]),
              'score', np.array_equal(sc1[0], sc0[0]))
        # isolation: instance 9 alone moves to scene 3
        g = np.repeat(geom[:1], B, axis=0)
        g[9] = geom[3]
        s.set_instance_scene(g)
        ev2, sol2, sc2 = calls()
        others = np.arange(B) != 9
        for f in ev1.dtype.names:
            assert np.array_equal(ev2[f][others], ev1[f][others]), f
        for a2, a1 in zip(sol2, sol1):
            assert np.array_equal(a2[others], a1[others])
        assert np.array_equal(sc2[0][others], sc1[0][others]) and np.array_equal(sc2[1][others], sc1[1][others])
        assert not np.array_equal(ev2['row_val'][9], ev1['row_val'][9]) and not np.array_equal(sol2[1][9], sol1[1][9])
        # clearing the scene: the shared results, bit for bit
        s.set_instance_scene(None)
        ev3, sol3, sc3 = calls()
        assert all(np.array_equal(ev3[f], ev0[f]) for f in ev0.dtype.names)
        assert all(np.array_equal(a3, a0) for a3, a0 in zip(sol3, sol0))
        assert np.array_equal(sc3[0], sc0[0]) and np.array_equal(sc3[1], sc0[1])


# ---- e. misuse ------------------------------------------------------------------------------------------------------------------------
def test_misuse_is_refused_by_name():
    import warnings
    import torch
    from safe_mpc_amd import _lib
    from safe_mpc_amd import controller as C
    from safe_mpc_amd._lib import EngineError
    par, prob, net = make_problem('st', N=6)
    s = _solver(prob, net)
    B = 6
    x0 = sample_instances(prob, B, seed=2)
    xg, ug, p = constant_guess(prob, x0)
    g = np.repeat(prob.row_geometry()[None], B, axis=0)
    s.set_instance_scene(g)
    s.solve(x0, xg, ug, p)
    # another batch size: refused, both sizes named -- by every entry point that evaluates rows
    small = (x0[:4], xg[:4], ug[:4], p[:4])
    for call in (lambda: s.solve(*small), lambda: s.eval_nodes(*small[1:]), lambda: s.merit_terms(*small),
                 lambda: s.check_guess(xg[:4], ug[:4]), lambda: s.check_trajectory(xg[:4]),
                 lambda: s.score_rollout(np.zeros((3, 4, 12)), np.zeros((2, 4, 6))), lambda: s.sqp(*small)):
        with pytest.raises(EngineError, match=r'engine error -1: .*batch size 4, .* 6 instances'):
            call()
    # smpc_rollout_batch: refused while a scene is set, runs once it is cleared
    with pytest.raises(EngineError, match=r'engine error -4: smpc_rollout_batch'):
        s.rollout(x0, xg, ug, p, 2)
    # a NaN in a field that is read (host pointers): refused, the scene stays; in a field no row reads: accepted
    bad = g.copy()
    bad[3, 2, 4] = np.nan
    with pytest.raises(EngineError, match=r'engine error -1: scene of instance 3, row 2'):
        s.set_instance_scene(bad)
    ok = g.copy()
    ok[:, :, 6:] = np.nan                                       # capsule rows read C and D only
    before = s.solve(x0, xg, ug, p)
    s.set_instance_scene(ok)
    assert all(np.array_equal(a, b) for a, b in zip(s.solve(x0, xg, ug, p), before))
    with pytest.raises(EngineError, match=r'engine error -1: bad batch size'):
        s._chk(_lib.lib().smpc_set_instance_scene(s.h, 0, g.ctypes.data, 0))
    # a larger scene while the stream is being captured: refused (the copy would have to grow), the capture ends cleanly
    big = torch.tensor(np.repeat(prob.row_geometry()[None], 4 * B, axis=0), dtype=torch.float64, device='cuda:0')
    with pytest.raises(EngineError, match='engine error -4: .* while the stream is being captured'), warnings.catch_warnings():
        warnings.filterwarnings('ignore', 'The CUDA Graph is empty')
        with torch.cuda.graph(torch.cuda.CUDAGraph()):
            s.set_instance_scene(big)
    torch.cuda.synchronize()
    assert all(np.array_equal(a, b) for a, b in zip(s.solve(x0, xg, ug, p), before))     # the old scene is still there
    s.set_instance_scene(None)
    s.rollout(x0, xg, ug, p, 2)
    s.solve(*small)
    # a problem without rows has no scene
    prob.desc.n_rows = 0
    s0 = _solver(prob, net)
    with pytest.raises(EngineError, match=r'engine error -1: .*no collision rows'):
        s0._chk(_lib.lib().smpc_set_instance_scene(s0.h, B, g.ctypes.data, 0))
    # the parallel policy: its candidate slots are not instances
    parp, probp, netp = make_problem('parallel', N=4)
    ctrl = C.get_controller('parallel', parp, 3, N=4, device_state=True)
    xp = torch.tensor(sample_instances(probp, 3, seed=2), dtype=torch.float64, device='cuda:0')
    ctrl.setGuess(xp[:, None, :].repeat(1, 5, 1), torch.zeros((3, 4, 6), dtype=torch.float64, device='cuda:0'))
    ctrl.ocp_solver.set_instance_scene(np.repeat(ctrl.problem.row_geometry()[None], 3, axis=0))
    with pytest.raises(EngineError, match=r'engine error -4: smpc_policy_step: .*parallel'):
        ctrl.step_on_device(xp)
    ctrl.ocp_solver.set_instance_scene(None)
    ctrl.step_on_device(xp)
    ctrl.ocp_solver.sync()


# ---- f. the device closed loop ----------------------------------------------------------------------------------------------------
LOOP_N, LOOP_SHIFTS = 10, (sc.SHIFTS[0], sc.SHIFTS[3])


def _loop_problems():
    from safe_mpc_amd import controller as C
    pars = []
    for shift in LOOP_SHIFTS:
        par, _, _ = make_problem('htwa', N=LOOP_N)
        par.back_hor = 12
        sc.move_obstacles(par, shift, sc.Z1_OBSTACLES)
        pars.append(par)
    return pars, [C.OcpProblem(pp, 'htwa', 'ext', N=LOOP_N) for pp in pars]


def _margin_classes(probs, x):
    """[scene, state] on the oracle: 2 = clear of the OCP's row bounds, 1 = between them and the check bounds (inside the collision
    margin: no collision, but the QP of a solve from there is infeasible, its rows at node 0 being violated constants), 0 = colliding"""
    from oracle.oracle import Oracle
    out = []
    for pr in probs:
        o = Oracle(pr)
        in_ocp = o.check_trajectory(x[:, None, :], pr.x_min, pr.x_max, 0.0, pr.row_lb, pr.row_ub).astype(bool)
        in_chk = o.check_trajectory(x[:, None, :], pr.x_min, pr.x_max, 0.0, pr.row_check[:, 0], pr.row_check[:, 1]).astype(bool)
        out.append(np.where(in_ocp, 2, np.where(in_chk, 1, 0)))
    return np.array(out)


def _state_in_margin(probs, pool, cls, s_in, s_out):
    """a state at rest inside the collision margin of scene s_in and clear in scene s_out: bisection between a pool state that
    collides in s_in alone and one that is clear in both"""
    bad = pool[np.where((cls[s_in] == 0) & (cls[s_out] == 2))[0][0]]
    for good in pool[np.where((cls == 2).all(0))[0]]:
        lo, hi = bad.copy(), good.copy()
        for _ in range(60):
            mid = 0.5 * (lo + hi)
            c = _margin_classes(probs, mid[None])[:, 0]
            if c[s_in] == 1:
                if c[s_out] == 2:
                    return mid
                break
            lo, hi = (mid, hi) if c[s_in] == 0 else (lo, mid)
    raise AssertionError('no state inside the margin')


def _loop_states(probs):
    """three starts, each run in both scenes: a moving one near the gate whose loop the gate's place bends; one at rest inside the
    margin of scene A (clear in B); one at rest inside the margin of scene B (clear in A).  Inside the margin every solve fails,
    the instance stands still, and 'htwa' aborts at step N - 1."""
    from conftest import halton
    pr, nq = probs[0], probs[0].nq
    q = (pr.lbx[:nq] + 0.05) + halton(400, nq, skip=1 + 7 * 5) * (pr.ubx[:nq] - pr.lbx[:nq] - 0.1)
    rest = np.hstack([q, np.zeros_like(q)])
    moving = np.hstack([q, 0.1 * np.random.default_rng(5).uniform(-1, 1, q.shape) * pr.ubx[nq:]])
    cls = _margin_classes(probs, rest)
    x = np.vstack([moving[218], _state_in_margin(probs, rest, cls, 0, 1), _state_in_margin(probs, rest, cls, 1, 0)])
    assert np.array_equal(_margin_classes(probs, x), [[2, 1, 2], [2, 2, 1]])
    return x


def test_device_closed_loop_in_two_scenes_equals_the_per_scene_loops():
    """run_mpc on the fused device path, 'htwa', 2 scenes x 3 instances, 20 steps, QP form pinned: against the two per-scene runs of
    the shared-scene path on problems built from moved parameters (that path is pinned by the oracle in
    test_device_policy_loop_equals_scalar_oracle_loop, whose tolerances these are); outcome lists and abort events equal.

    The same three starts run in both scenes (_loop_states), and the per-scene runs are first shown to be far apart: the moving
    start's states and controls differ between the scenes by more than 100 x the tolerance, the start inside scene A's margin aborts
    in A and is lost there (its backup OCP is infeasible in A) while it runs on in B, and the other way round for the start inside
    B's margin.  So a policy step, a plant test or a backup solve that ran in the shared scene would change an outcome list."""
    from safe_mpc_amd import closed_loop as cl
    from safe_mpc_amd import controller as C
    from safe_mpc_amd.problem import scenes_from_problems
    N, steps = LOOP_N, 20
    pars, probs = _loop_problems()
    geoms = scenes_from_problems(probs[0], probs)
    x0 = np.tile(_loop_states(probs), (2, 1))                  # instances 0-2 in scene A, 3-5 the same starts in scene B
    xg, ug = np.repeat(x0[:, None, :], N + 1, axis=1), np.zeros((6, N, 6))
    scenes = np.repeat(geoms, 3, axis=0)

    def factories(par):
        def mk(name, batch):
            c = C.get_controller(name, par, batch, device=0, device_state=True)
            c.ocp_solver.set_qp_mode('throughput')
            return c

        def mkb(batch):
            c = C.SafeBackupController(par, batch, device=0, device_state=True)
            c.ocp_solver.set_qp_mode('throughput')
            return c
        return mk, mkb
    parts = []
    for sn, par in enumerate(pars):
        mk1, mkb1 = factories(par)
        parts.append(cl.run_mpc(par, 'htwa', xg[3 * sn:3 * sn + 3], ug[3 * sn:3 * sn + 3], n_steps=steps, on_device=True, groups=1,
                                make_controller=mk1, make_backup=mkb1))
    xo, uo = np.concatenate([q['x'] for q in parts]), np.concatenate([q['u'] for q in parts])
    tol_x, tol_u = 1e-4, 2e-3 * (1 + np.nanmax(np.abs(uo)))
    # preconditions, on the reference runs: the scenes are told apart, and each has its abort event
    apart_x, apart_u = np.abs(parts[0]['x'][0] - parts[1]['x'][0]).max(), np.abs(parts[0]['u'][0] - parts[1]['u'][0]).max()
    print('closed loop: the moving start between the scenes: x', apart_x, 'u', apart_u, '; tolerances', tol_x, tol_u)
    assert apart_x >= 100 * tol_x and apart_u >= 100 * tol_u
    assert [q['collisions_idx'] for q in parts] == [[1], [2]] and [len(q['x_viable']) for q in parts] == [1, 1]
    assert np.isnan(parts[0]['x'][1]).any() and np.isnan(parts[1]['x'][2]).any()
    assert not np.isnan(parts[0]['x'][2]).any() and not np.isnan(parts[1]['x'][1]).any()

    mk, mkb = factories(pars[0])
    res = cl.run_mpc(pars[0], 'htwa', xg, ug, n_steps=steps, on_device=True, groups=1, make_controller=mk, make_backup=mkb,
                     scenes=scenes)
    assert np.array_equal(res['scenes'], scenes)
    assert np.array_equal(np.isnan(res['x']), np.isnan(xo)) and np.array_equal(np.isnan(res['u']), np.isnan(uo))
    for key in ('conv_idx', 'collisions_idx', 'viable_idx', 'unconv_idx'):
        assert sorted(res[key]) == sorted(i + 3 * sn for sn, q in enumerate(parts) for i in q[key]), key
    assert res['collisions_idx'] == [1, 5]
    xv = np.concatenate([q['x_viable'] for q in parts])
    assert res['x_viable'].shape == xv.shape and np.abs(res['x_viable'] - xv).max() < 1e-5
    print('closed loop: x error', np.nanmax(np.abs(res['x'] - xo)), 'u error', np.nanmax(np.abs(res['u'] - uo)))
    assert np.nanmax(np.abs(res['x'] - xo)) < tol_x and np.nanmax(np.abs(res['u'] - uo)) < tol_u


# ---- g. warm starts -----------------------------------------------------------------------------------------------------------------
GUESS_SHIFTS = (sc.SHIFTS[0], (-0.4, -0.1, 0.2))


def test_generate_guess_on_device_in_two_scenes_equals_the_per_scene_runs():
    """generate_guess(on_device=True, scenes=...), N = 10, 2 scenes x 2 instances interleaved (A, B, A, B), against per-scene
    generate_guess on problems built from moved parameters, at the tolerance of test_generate_guess_engine_matches_oracle_double
    (1e-4 (1 + |.|_inf), same accepted set).

    Scene B has the gate where the second and the fourth Halton candidate collide with it, so the walk over the candidates is
    another than in either scene alone: instance 1 (scene B) skips the second candidate, which scene A would have taken.  Which
    start of its own scene's run an instance is follows from the oracle's verdicts on the candidates (the walk restated below).
    Preconditions, asserted first: a candidate is skipped that is free in the other scene; and a start that both per-scene runs
    hold gets warm starts in the two scenes that differ by more than 100 x the tolerance."""
    from oracle.oracle import Oracle
    from safe_mpc_amd import closed_loop as cl
    from safe_mpc_amd import controller as C
    from safe_mpc_amd.problem import scenes_from_problems
    N, n = 10, 4
    pars = []
    for shift in GUESS_SHIFTS:
        par, _, _ = make_problem('htwa', N=N)
        par.nlp_max_iter = 200
        sc.move_obstacles(par, shift, sc.Z1_OBSTACLES)
        pars.append(par)
    probs = [C.OcpProblem(pp, 'htwa', 'ext', N=N) for pp in pars]
    geoms = scenes_from_problems(probs[0], probs)
    scene_of = [0, 1, 0, 1]
    scenes = geoms[scene_of]
    # the walk, restated on the oracle: candidate by candidate, each tested in the scene of the instance it would start
    pr = probs[0]
    q = pr.x_min[:6] + cl.halton(4 * n + 16, 6) * (pr.x_max[:6] - pr.x_min[:6])
    cand = np.hstack([q, np.zeros_like(q)])
    fr = [Oracle(p_).check_trajectory(cand[:, None, :], p_.x_min, p_.x_max, 0.0, p_.row_check[:, 0], p_.row_check[:, 1]).astype(bool)
          for p_ in probs]
    taken, skipped, c = [], [], 0
    for sn in scene_of:
        while not fr[sn][c]:
            skipped.append((c, sn))
            c += 1
        taken.append(c)
        c += 1
    assert any(fr[1 - sn][c] for c, sn in skipped), (taken, skipped)              # skipped in its scene, free in the other
    rank = [int(fr[sn][:c].sum()) for sn, c in zip(scene_of, taken)]                # instance k = start rank[k] of its scene's own run
    n_own = [max(r for r, sn in zip(rank, scene_of) if sn == s_) + 1 for s_ in (0, 1)]

    def mk_for(par):
        def mk(name, batch):
            c = C.get_controller(name, par, batch)
            c.ocp_solver.set_qp_mode('throughput')
            return c
        return mk
    own = [cl.generate_guess(pars[s_], 'htwa', n_own[s_], make_controller=mk_for(pars[s_]), on_device=True) for s_ in (0, 1)]

    def start_of(s_, r):
        """(xg, ug) of start r of scene s_'s own run, None if it was not accepted"""
        g, m = own[s_]
        return (g['xg'][m[:r].sum()], g['ug'][m[:r].sum()]) if m[r] else None

    def rel(a, b):
        return np.abs(a - b).max() / (1.0 + np.abs(b).max())
    ref = [start_of(sn, r) for sn, r in zip(scene_of, rank)]
    apart = [0.0]
    for k, (sn, c) in enumerate(zip(scene_of, taken)):             # the same candidate as a start of the other scene's run
        r_other = int(fr[1 - sn][:c].sum())
        if fr[1 - sn][c] and r_other < n_own[1 - sn] and ref[k] is not None and start_of(1 - sn, r_other) is not None:
            other = start_of(1 - sn, r_other)
            apart.append(max(rel(ref[k][0], other[0]), rel(ref[k][1], other[1])))
    print('generate_guess: candidates taken', taken, 'skipped', skipped, 'ranks', rank, 'warm starts between the scenes', apart)
    assert max(apart) >= 100 * 1e-4

    got, mask = cl.generate_guess(pars[0], 'htwa', n, make_controller=mk_for(pars[0]), on_device=True, scenes=scenes)
    want_mask = np.array([r_ is not None for r_ in ref])
    assert np.array_equal(mask, want_mask), (mask, want_mask)
    assert mask.sum() >= 2
    ref_x, ref_u = np.array([r_[0] for r_ in ref if r_ is not None]), np.array([r_[1] for r_ in ref if r_ is not None])
    ex = np.abs(got['xg'] - ref_x).reshape(len(ref_x), -1).max(1) / (1.0 + np.abs(ref_x).reshape(len(ref_x), -1).max(1))
    eu = np.abs(got['ug'] - ref_u).reshape(len(ref_u), -1).max(1) / (1.0 + np.abs(ref_u).reshape(len(ref_u), -1).max(1))
    print('generate_guess: accepted', mask.tolist(), 'x error', ex, 'u error', eu)
    assert np.all(ex < 1e-4) and np.all(eu < 1e-4)
    assert np.array_equal(got['scenes'], scenes[mask])
