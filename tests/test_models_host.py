"""A controller model of its own for every instance, host side: the table's validation, run_mpc / generate_guess plumbing (set,
sliced per group, cleared; refusals before anything is built), the result file's name, and the property the feature is for -- a
controller that has its plant's model never asks for a torque that clips -- on the CPU oracle.  Runs without a GPU
(ModelOracleSolver, model_cases.py, is the solver)."""
import ctypes
import os
import types

import numpy as np
import pytest

import model_cases as mc
from conftest import make_problem, sample_instances
from fake_solver import OracleSolver
from safe_mpc_amd import closed_loop as cl
from safe_mpc_amd import controller as C


# ---- 1. the table -------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_entry_point_and_lib_declares_it():
    from safe_mpc_amd import _lib
    assert 'smpc_set_instance_models' in _lib.SYMBOLS
    assert os.path.exists(_lib.LIB_PATH), 'the engine is built before the tests run (__graft_entry__.build)'
    L = ctypes.CDLL(_lib.LIB_PATH)               # loads without a GPU
    assert hasattr(L, 'smpc_set_instance_models')
    assert L.smpc_abi_version() == 5


def test_perturbed_tables_move_the_inertials_only():
    """what smpc_set_instance_models checks with host pointers holds for the plant's tables: R0, p0, axis and the four limits are
    bit-equal to the descriptor's, the mass moves by up to 19.9 %"""
    (par, prob, net), tables, probs = mc.family()
    base = prob.joint_table()
    for f in mc.KINEMATICS_AND_LIMITS:
        assert np.array_equal(tables[f], np.broadcast_to(base[f], tables[f].shape)), f
    rel = np.abs(tables['mass'] / base['mass'] - 1.0).max()
    assert 0.19 < rel < 0.2
    for b in range(len(tables)):                 # problem_with_model: the descriptor carries the table's inertials and nothing else moved
        t = probs[b].joint_table()
        assert t.tobytes() == tables[b].tobytes()
    assert prob.joint_table().tobytes() == base.tobytes()


def test_table_validation_messages():
    from safe_mpc_amd.solver import BatchedOcpSolver
    (par, prob, net), tables, probs = mc.family()
    fake = types.SimpleNamespace(nq=6)           # (the shape checks come before the handle is touched)
    with pytest.raises(ValueError, match=r'set_instance_models: expected JOINT_DTYPE \[B, 6\], got float64 \(8, 6\)'):
        BatchedOcpSolver.set_instance_models(fake, np.zeros((8, 6)))
    with pytest.raises(ValueError, match=r'set_instance_models: expected JOINT_DTYPE \[B, 6\]'):
        BatchedOcpSolver.set_instance_models(fake, tables[:, :5])
    s = mc.ModelOracleSolver(prob, net)
    bad = tables.copy()
    bad['p0'][3, 2, 1] += 1e-12
    with pytest.raises(ValueError, match='p0 differs'):
        s.set_instance_models(bad)
    bad = tables.copy()
    bad['tau_max'][0, 0] *= 2
    with pytest.raises(ValueError, match='tau_max differs'):
        s.set_instance_models(bad)
    s.set_instance_models(tables)
    assert s.idx.tolist() == list(range(8))
    s.set_instance_models(tables[[2, 2, 5]])
    assert s.idx.tolist() == [2, 2, 5]


# ---- 2. run_mpc ---------------------------------------------------------------------------------------------------------------------
def _factories(par, N, calls, with_setter=True, made=None):
    """make_controller / make_backup of run_mpc around a ModelOracleSolver that writes down what it is given"""
    class Recording(mc.ModelOracleSolver):
        def set_instance_models(self, joints=None):
            calls.append((self.problem.controller, 'models', None if joints is None else np.array(joints)))
            super().set_instance_models(joints)

        def solve(self, x0, xg, ug, p, out=None):
            calls.append((self.problem.controller, 'solve', len(x0)))
            return super().solve(x0, xg, ug, p, out)

    def build(cls, name, cost, horizon, batch):
        ctrl = cls.__new__(cls)
        prob = C.OcpProblem(par, name, cost, N=horizon)
        net = C.SafeSetNet.from_params(par, prob.x_min, prob.x_max)
        prob.set_normalisation(net.mean, net.std)
        solver = Recording(prob, net) if with_setter else OracleSolver(prob, net)
        if made is not None:
            made.append(name)
        C.AbstractController.__init__(ctrl, par, batch, cost, horizon, solver=solver, net=net)
        return ctrl
    return (lambda name, batch: build(C.CONTROLLERS[name], C.CONTROLLERS[name].cont_name, 'ext', N, batch),
            lambda batch: build(C.SafeBackupController, 'backup', 'zero', par.back_hor, batch))


def _start(N, B):
    par, prob, net = make_problem('htwa', N=N)
    par.back_hor = 6
    x0 = sample_instances(prob, B, seed=5, vel_scale=0.1)
    return par, prob, np.repeat(x0[:, None, :], N + 1, axis=1), np.zeros((B, N, 6))


def test_run_mpc_sets_slices_and_clears_the_models():
    """two groups of 3: each group's controller gets its rows of the table before its first solve and is left without one when the
    run ends; models='plant' hands over the very tables the group draws for its plant (seeds = global instance indices); the backup
    solver gets exactly the rows of the aborting instances"""
    N, B = 4, 6
    par, prob, xg, ug = _start(N, B)
    table = mc.model_tables(par, 6, B)
    calls = []
    mk, mkb = _factories(par, N, calls)
    res = cl.run_mpc(par, 'htwa', xg, ug, make_controller=mk, make_backup=mkb, n_steps=3, groups=2, models=table)
    sets = [c for c in calls if c[0] == 'htwa' and c[1] == 'models']
    assert len(sets) == 4
    assert sets[0][2].tobytes() == table[:3].tobytes() and sets[1][2].tobytes() == table[3:].tobytes()
    assert sets[2][2] is None and sets[3][2] is None
    first_solve = [k for k, c in enumerate(calls) if c[1] == 'solve'][0]
    assert all(k > first_solve for k, c in enumerate(calls) if c[1] == 'models' and c[2] is None)
    assert [k for k, c in enumerate(calls) if c[1] == 'models' and c[2] is not None and c[0] == 'htwa'] == [0, 1]
    # the nominal run is another run: the models reach the solves
    calls0 = []
    mk0, mkb0 = _factories(par, N, calls0)
    res0 = cl.run_mpc(par, 'htwa', xg, ug, make_controller=mk0, make_backup=mkb0, n_steps=3, groups=2)
    assert not any(c[1] == 'models' for c in calls0)
    assert not np.array_equal(res['u'], res0['u'], equal_nan=True)
    # 'plant': the tables of the plant, by global seed
    calls.clear()
    cl.run_mpc(par, 'htwa', xg, ug, noise=20.0, make_controller=mk, make_backup=mkb, n_steps=2, groups=2, models='plant')
    sets = [c for c in calls if c[0] == 'htwa' and c[1] == 'models' and c[2] is not None]
    want = cl.perturbed_joint_tables(par, 6, 20.0, range(B))
    assert len(sets) == 2 and sets[0][2].tobytes() == want[:3].tobytes() and sets[1][2].tobytes() == want[3:].tobytes()
    # an abort event: N consecutive failed solves make instances 1 and 4 abort at step N - 1
    calls.clear()
    fail = np.array([0, 4, 0, 0, 4, 0], np.int32)

    def mk_scripted(name, batch):
        ctrl = mk(name, batch)
        ctrl.ocp_solver.scripted_status = [fail.copy() for _ in range(N)] + [np.zeros(B, np.int32)] * 4
        return ctrl
    res = cl.run_mpc(par, 'htwa', xg, ug, make_controller=mk_scripted, make_backup=mkb, n_steps=6, groups=1, models=table)
    back = [c for c in calls if c[0] == 'backup']
    assert [c[1] for c in back] == ['models', 'solve', 'models'], [c[:2] for c in back]
    assert back[0][2].tobytes() == table[[1, 4]].tobytes() and back[1][2] == 2 and back[2][2] is None
    assert res['x_viable'].shape[0] == 2


def test_refusals_come_before_anything_is_built():
    N, B = 4, 4
    par, prob, xg, ug = _start(N, B)
    table = mc.model_tables(par, 6, B)
    made, calls = [], []
    mk, mkb = _factories(par, N, calls, made=made)
    with pytest.raises(ValueError, match="models: the 'parallel' policy is not supported"):
        cl.run_mpc(par, 'parallel', xg, ug, make_controller=mk, make_backup=mkb, n_steps=2, models=table)
    with pytest.raises(ValueError, match="models='plant': .* noise > 0"):
        cl.run_mpc(par, 'htwa', xg, ug, make_controller=mk, make_backup=mkb, n_steps=2, models='plant')
    with pytest.raises(ValueError, match=r'models: expected a JOINT_DTYPE table \[4, nq\]'):
        cl.run_mpc(par, 'htwa', xg, ug, make_controller=mk, make_backup=mkb, n_steps=2, models=table[:3])
    with pytest.raises(ValueError, match=r"models: 'nominal'"):
        cl.run_mpc(par, 'htwa', xg, ug, make_controller=mk, make_backup=mkb, n_steps=2, models='nominal')
    with pytest.raises(ValueError, match='generate_guess_until: per-instance models are not supported'):
        cl.generate_guess_until(par, 'htwa', 2, make_controller=mk, models=table[:2])
    with pytest.raises(ValueError, match=r'models: expected a JOINT_DTYPE table \[2, nq\]'):
        cl.generate_guess(par, 'htwa', 2, make_controller=mk, models=table[:3])
    assert made == [] and calls == []
    # a solver without the setter: named, before the backup is built or anything runs
    mk0, mkb0 = _factories(par, N, calls, with_setter=False, made=made)
    with pytest.raises(ValueError, match='models: OracleSolver has no set_instance_models'):
        cl.run_mpc(par, 'htwa', xg, ug, make_controller=mk0, make_backup=mkb0, n_steps=2, models=table)
    assert made == ['htwa'] and calls == []
    with pytest.raises(ValueError, match='models: OracleSolver has no set_instance_models'):
        cl.generate_guess(par, 'htwa', 2, make_controller=mk0, models=table[:2])


def test_generate_guess_hands_every_instance_its_model():
    """generate_guess(models=table[n, nq]) on the host: the solver holds the table for the SQP and the check, the result carries the
    accepted instances' tables, the solver is left without one; another table gives other warm starts"""
    N, n = 4, 3
    par, _, _ = make_problem('htwa', N=N)
    par.nlp_max_iter = 3
    table = mc.model_tables(par, 6, n)
    calls = []
    mk, _ = _factories(par, N, calls)
    got, good = cl.generate_guess(par, 'htwa', n, make_controller=mk, models=table)
    sets = [c for c in calls if c[1] == 'models']
    assert sets[0][2].tobytes() == table.tobytes() and sets[-1][2] is None and len(sets) == 2
    assert got['models'].tobytes() == table[good].tobytes()
    calls.clear()
    plain, good0 = cl.generate_guess(par, 'htwa', n, make_controller=mk)
    assert 'models' not in plain and not any(c[1] == 'models' for c in calls)
    both = good & good0
    if both.any():
        assert not np.array_equal(got['ug'][both[good]], plain['ug'][both[good0]])


# ---- 3. the result file ---------------------------------------------------------------------------------------------------------------
def test_result_file_name_carries_the_controller_model():
    par, _, _ = make_problem('st', N=4)
    args = (par, 'z1', 'st', 30, True, 20.0, 0.0, 0.05, 0.01)
    plain = cl.result_file(*args)
    assert cl.result_file(*args, controller_model='nominal') == plain and plain.endswith('_0.05_0.01_mpc.pkl')
    assert cl.result_file(*args, controller_model='plant') == plain[:-len('_mpc.pkl')] + '_cmplant_mpc.pkl'
    with pytest.raises(ValueError, match='controller_model'):
        cl.result_file(*args, controller_model='other')


# ---- 4. what the feature is for -----------------------------------------------------------------------------------------------------
def test_a_controller_with_the_plants_model_never_asks_for_a_torque_that_clips():
    """make_problem('naive', N = 8), 8 instances at sample_instances(prob, 8, seed=1, vel_scale=0)[0], shared tau_max =
    max(1.10 |tau(x0, 0)|, 0.05), models = perturbed_joint_tables(par, 6, 20 %, range(8)), 6 steps of guessCorrection / solve / plant
    / provideControl on the oracle.  The plant applies qdd = M_b^-1 (clip(tau_b(x, u)) - h_b), which is u unless tau_b clips; at node 0
    the state is pinned and tau is affine in u_0, so a torque row formed with the plant's model admits no u_0 that clips.
    Recorded: nominal model, all 8 instances clip, worst |u_eff - u_0| per instance 0.14 .. 4.66; matched, 1.6e-12; 96 statuses 0.
    Asserted: nominal at least 6 of 8 above 1e-3; matched all within 1e-9 (1 + |u|_inf); all statuses 0."""
    (par, prob, net), tables, x0, probs = mc.clip_family()
    s = mc.ModelOracleSolver(prob, None)
    w0, u0, st0 = mc.clip_loop(s, x0, prob.N, 6, tables)
    s.set_instance_models(tables)
    w1, u1, st1 = mc.clip_loop(s, x0, prob.N, 6, tables)
    print('nominal', w0, 'matched', w1)
    assert (w0 > 1e-3).sum() >= 6
    assert np.all(w1 <= 1e-9 * (1 + u1))
    assert np.all(st0 == 0) and np.all(st1 == 0) and st0.size + st1.size == 96
