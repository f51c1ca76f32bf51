"""ParallelController (reference controller.py:567-644) on the CPU: the batched numpy class against a literal one-instance
transcription of the reference's step (tests/parallel_double.py), with scripted candidate failures and safe-set verdicts so that
every branch of the selection and the automaton is taken; its candidate flags; its place in get_controller; the header's policy
kind; and run_mpc end to end on the oracle double."""
import os
import subprocess

import numpy as np
import pytest

from conftest import sample_instances
import parallel_double as pd
from safe_mpc_amd import closed_loop as cl
from safe_mpc_amd import controller as C
from safe_mpc_amd.parser import Parameters

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _params(N=8, Nb=6):
    par = Parameters({}, 'z1')
    par.nq, par.n_dof_safe_set, par.net_size, par.N, par.back_hor = 6, 6, [12, 32, 1], N, Nb
    return par


# instance -> the switched nodes whose candidate fails at step j
def _fail_nodes(N):
    every = set(range(1, N + 1))

    def f(j, b):
        return {0: set(),                                   # succeeds at N
                1: {N},                                     # candidate N always fails: the choice comes from the others
                2: every,                                   # fails every step: r runs down to 1, then the abort
                3: set(range(3, N + 1)),                    # only candidates 1 and 2 can succeed
                4: every if j < N - 1 else set(),           # r reaches 1 at step N - 1, where no node is safe: result 1 -> abort
                5: {N, N - 1} if j % 2 else set()}.get(b, set())
    return f


def _no_safe_step(j, N):
    return j in (2, N - 1, N)          # steps on which no state is safe: ties at result r, the min(n, r) branch, result exactly 1


def test_batched_step_equals_scalar_reference_transcription():
    N, B, steps = 8, 6, 10
    par = _params(N)
    ctrl = pd.make_parallel_double(par, B)
    ctrl.checkSafeConstraints = pd.vec_safe
    rng = np.random.default_rng(4)
    x0 = sample_instances(ctrl.problem, B, seed=2, vel_scale=0.1)
    xg, ug = np.repeat(x0[:, None, :], N + 1, axis=1), rng.normal(scale=0.1, size=(B, N, 6))
    ctrl.setGuess(xg.copy(), ug.copy())
    ctrl.reset_controller()
    fail = _fail_nodes(N)
    ctrl.ocp_solver.fail_nodes = fail
    one = pd.CandidateFailSolver(ctrl.problem, ctrl.net)          # the scalar side solves one instance per call
    one.fail_nodes = fail
    check_state = lambda xt: bool(ctrl.checkStateConstraints(np.asarray(xt)[None])[0])
    insts = [pd.ScalarParallel(N, par, one, check_state, pd.safe_rule, xg[b], ug[b], ctrl.problem.ee_ref) for b in range(B)]
    x = x0.copy()
    seen = {'abort': 0, 'result_1': 0, 'low_n': 0, 'reject_shift': 0, 'tie': 0}
    try:
        for j in range(steps):
            pd.SAFE_MODE[0] = 'none' if _no_safe_step(j, N) else 'rule'
            for s in (ctrl.ocp_solver, one):
                s.x_cur, s.step_no = x.copy(), j
            um, am = ctrl.step(x)
            for b in range(B):
                r0 = insts[b].r
                uo, ao = insts[b].step(x[b])
                assert bool(am[b]) == ao, (j, b)
                assert int(ctrl.r[b]) == insts[b].r and int(ctrl.fails[b]) == insts[b].fails, (j, b)
                assert int(ctrl.current_step[b]) == insts[b].current_step, (j, b)
                assert np.abs(um[b] - uo).max() <= 1e-12 * (1 + np.abs(uo).max()), (j, b)
                assert np.abs(ctrl.x_guess[b] - insts[b].x_guess).max() <= 1e-12, (j, b)
                assert np.abs(ctrl.u_guess[b] - insts[b].u_guess).max() <= 1e-12 * (1 + np.abs(insts[b].u_guess).max()), (j, b)
                assert np.abs(ctrl.x_viable[b] - insts[b].x_viable).max() <= 1e-12, (j, b)
                assert int(ctrl.last_status[b]) == insts[b].last_status, (j, b)
                ns = insts[b].node_success
                seen['abort'] += int(ao)
                seen['result_1'] += int(ns == 1)
                seen['low_n'] += int(ns > 1 and insts[b].chosen is not None and insts[b].chosen < N)
                seen['reject_shift'] += int(ns <= 1 and r0 > 1)
                seen['tie'] += int(ns > 1 and pd.SAFE_MODE[0] == 'none' and r0 < N)
            x = x + par.dt * np.hstack([x[:, 6:], um]) + rng.normal(scale=1e-3, size=x.shape)
    finally:
        pd.SAFE_MODE[0] = 'rule'
    # every branch was taken: success at a low n, ties (largest n wins), result exactly 1, rejection with a shift, the abort
    assert all(v > 0 for v in seen.values()), seen


def test_abort_keeps_the_guess_and_the_step_count():
    """failure with r == 1: (u_guess[0], True), guess not shifted, current_step unchanged, x_viable = x_guess[1], r back to N"""
    N, B = 4, 2
    par = _params(N)
    ctrl = pd.make_parallel_double(par, B)
    ctrl.checkSafeConstraints = pd.vec_safe
    x0 = sample_instances(ctrl.problem, B, seed=5, vel_scale=0.05)
    ug = np.random.default_rng(1).normal(scale=0.1, size=(B, N, 6))
    ctrl.setGuess(np.repeat(x0[:, None, :], N + 1, axis=1), ug)
    ctrl.reset_controller()
    ctrl.ocp_solver.fail_nodes = lambda j, b: set(range(1, N + 1)) if b == 0 else set()
    ctrl.ocp_solver.x_cur = x0.copy()
    for j in range(N):
        ctrl.ocp_solver.step_no = j
        before = ctrl.getGuess()
        corrected = ctrl.ocp_solver.guess_correction(before[0].copy(), before[1])
        cs = int(ctrl.current_step[0])
        u, a = ctrl.step(x0)
        if j < N - 1:
            assert not a[0] and int(ctrl.r[0]) == N - 1 - j and int(ctrl.fails[0]) == j + 1
            assert int(ctrl.current_step[0]) == cs + 1
        else:
            assert a[0] and int(ctrl.r[0]) == N and int(ctrl.fails[0]) == N
            assert int(ctrl.current_step[0]) == cs
            assert np.array_equal(ctrl.x_guess[0], corrected[0]) and np.array_equal(ctrl.u_guess[0], before[1][0])
            assert np.array_equal(u[0], before[1][0, 0])
            assert np.array_equal(ctrl.x_viable[0], corrected[0, 1])
        assert not a[1] and int(ctrl.fails[1]) == 0


def test_candidate_flags():
    """constrain_n (:578-587): candidate n has p[n][4] = +1 and -1 at every other node of 1..N -- the terminal node included unless
    n = N (unlike Receding, whose terminal row is always on); node 0 keeps the instance's flag"""
    N = 6
    ctrl = pd.make_parallel_double(_params(N), 1)
    F = ctrl.candidate_flags()
    assert F.shape == (N, N + 1)
    for c, n in enumerate(range(N, 0, -1)):
        want = -np.ones(N + 1)
        want[n] = 1.0
        assert np.array_equal(F[c, 1:], want[1:]), n
        assert (F[c, N] > 0) == (n == N)
    # ... and what the solver receives: B * N candidates, the instance's own p left with its flags
    seen = []

    class Recording(pd.CandidateFailSolver):
        def solve(self, x0, xg, ug, p, out=None):
            seen.append(np.array(p))
            return super().solve(x0, xg, ug, p, out)
    ctrl = pd.make_parallel_double(_params(N), 2, solver_cls=Recording)
    x0 = sample_instances(ctrl.problem, 2, seed=1)
    ctrl.setGuess(np.repeat(x0[:, None, :], N + 1, axis=1), np.zeros((2, N, 6)))
    own = np.array(ctrl.p)
    ctrl.step(x0)
    P = seen[-1].reshape(2, N, N + 1, 5)
    assert np.array_equal(P[:, :, 1:, 4], np.broadcast_to(F[None, :, 1:], (2, N, N)))
    assert np.array_equal(P[:, :, 0, 4], np.broadcast_to(own[:, None, 0, 4], (2, N)))
    assert np.array_equal(ctrl.p[:, :, 4], own[:, :, 4])


def test_get_controller_finds_the_unregistered_class():
    par = _params(6)
    names = set(C.CONTROLLERS)
    assert 'parallel' not in names and C.UNREGISTERED_CONTROLLERS == {'parallel': C.ParallelController}
    assert issubclass(C.ParallelController, C.RecedingController)
    assert C.ParallelController.cont_name == 'parallel' and C.ParallelController.can_abort
    from safe_mpc_amd.problem import CONTROLLER_KINDS, NN_ALL
    assert CONTROLLER_KINDS['parallel'] == (NN_ALL, None, None, False)
    try:
        ctrl = C.get_controller('parallel', par, 2)
    except RuntimeError:           # (no GPU: the engine cannot be created -- the lookup itself is what is tested)
        ctrl = None
    if ctrl is not None:
        assert type(ctrl) is C.ParallelController
    with pytest.raises(ValueError):
        C.get_controller('nope', par, 2)
    prob = C.OcpProblem(par, 'parallel', 'ext', N=6)
    assert prob.desc.qp_stall_iters == 24 and prob.desc.nn_mode == NN_ALL
    assert prob.desc.nn_soft_e < 0 and prob.desc.nn_soft_run < 0          # both rows hard (:573-576)


def test_header_policy_kind_and_struct_sizes(tmp_path):
    from safe_mpc_amd import _lib
    import ctypes
    src = tmp_path / 'k.c'
    src.write_text('#include <stdio.h>\n#include "smpc.h"\n'
                   'int main(void) { printf("%d %zu %zu %zu %d\\n", SMPC_POLICY_PARALLEL, sizeof(smpc_policy_params), '
                   'sizeof(smpc_policy_state), sizeof(smpc_loop_state), SMPC_ABI_VERSION); return 0; }\n')
    exe = tmp_path / 'k'
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    v = [int(t) for t in subprocess.check_output([str(exe)]).split()]
    assert v[0] == C.ParallelController.policy_kind == 5
    assert v[1:4] == [ctypes.sizeof(_lib.PolicyParams), ctypes.sizeof(_lib.PolicyState), ctypes.sizeof(_lib.LoopState)]
    assert v[4] == 5


def test_run_mpc_parallel_on_the_oracle_double_reaches_the_backup_solve():
    """closed_loop.run_mpc(.., 'parallel') on the CPU double: instance 0 fails every candidate, so its receding index runs N, N-1,
    .., 1 and it aborts at step N - 1 into the backup OCP (scripts/mpc.py:161-190)"""
    from fake_solver import OracleSolver
    N, B, steps = 6, 4, 8
    par = _params(N, Nb=6)
    backups = []

    def make_controller(name, batch):
        assert name == 'parallel'
        ctrl = pd.make_parallel_double(par, batch)
        ctrl.ocp_solver.fail_nodes = lambda j, b: set(range(1, N + 1)) if b == 0 else set()
        step = ctrl.step

        def tracked(x):                     # (the scripted failures recognise instance 0 by its current state)
            ctrl.ocp_solver.x_cur = np.asarray(x, float).copy()
            return step(x)
        ctrl.step = tracked
        return ctrl

    def make_backup(batch):
        b = C.SafeBackupController.__new__(C.SafeBackupController)
        prob = C.OcpProblem(par, 'backup', 'zero', N=par.back_hor)
        net = C.SafeSetNet.from_params(par, prob.x_min, prob.x_max)
        C.AbstractController.__init__(b, par, batch, 'zero', par.back_hor, solver=OracleSolver(prob, net), net=net)
        orig = b.ocp_solver.solve

        def solve(x0, xg, ug, p, out=None):
            backups.append(np.array(x0))
            return orig(x0, xg, ug, p, out)
        b.ocp_solver.solve = solve
        return b

    x_start = sample_instances(C.OcpProblem(par, 'htwa', 'ext', N=N), B, seed=3, vel_scale=0.05)
    res = cl.run_mpc(par, 'parallel', np.repeat(x_start[:, None, :], N + 1, axis=1), np.zeros((B, N, 6)),
                     make_controller=make_controller, make_backup=make_backup, n_steps=steps)
    r = res['r_receding'][:, :, 0]
    assert r.shape == (B, steps)
    assert list(r[0, :N]) == list(range(N, 0, -1))          # instance 0: r = N, N-1, .., 1, then the abort
    assert res['x_viable'].shape[0] >= 1 and len(backups) >= 1
    assert np.all(r[1:, 0] == N)
