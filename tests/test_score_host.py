"""Scores of a closed-loop run without a GPU: closed_loop.score_rollout_statement on the CPU oracle double against sums written out
by hand, the planted-extremes logs the GPU tests run on, run_mpc(score=True), metrics_count_fails --scored and the C ABI."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import score_cases as sc
from conftest import ROOT, make_problem, sample_instances
from fake_solver import OracleSolver, make_double_controller
from test_metrics import _ee_by_oracle, _load_script, _two_instance_pickle


def _metrics_setup(tmp_path):
    from safe_mpc_amd.parser import Parameters, default_args
    from safe_mpc_amd.problem import OcpProblem
    params = Parameters({**default_args(), 'horizon': 30, 'alpha': 10.0}, 'z1', rti=True)
    params.N = 30
    params.DATA_DIR = os.path.join(str(tmp_path), '')
    prob = OcpProblem(params, 'naive', 'ext', N=2)
    return params, prob


def test_statement_equals_the_hand_computation(tmp_path):
    """d0..d3 of test_metrics' two-instance, three-step log against sums written out with Oracle.points, to 1e-12 relative: the
    complete instance's cost is closed_loop_costs', the truncated one counts its valid rows only."""
    import pickle
    from safe_mpc_amd import closed_loop as cl
    from safe_mpc_amd.solver import SCORE_INDEX_SLOTS, SCORE_SLOTS
    m = _load_script()
    params, prob = _metrics_setup(tmp_path)
    ee = _ee_by_oracle(prob)
    expect = _two_instance_pickle(tmp_path, params, prob, ee)
    res = pickle.load(open(cl.result_file(params, 'z1', 'st', params.N, True, 0.0, 0.0, 0.0, 0.0), 'rb'))
    x, u = res['x'], res['u']
    solver = OracleSolver(prob, None)
    x_log, u_log = np.transpose(x, (1, 0, 2)), np.transpose(u, (1, 0, 2))
    lx, lu = np.array([3, 1], np.int64), np.array([2, 0], np.int64)
    out, outi = cl.score_rollout_statement(solver, prob, params, x_log, u_log, lx, lu)
    assert out.shape == (2, len(SCORE_SLOTS)) and outi.shape == (2, len(SCORE_INDEX_SLOTS)) and outi.dtype == np.int32
    Q, R = params.Q_weight, params.R_weight
    for b in range(2):
        e2 = [np.sum((ee(x[b, j, :6]) - prob.ee_ref) ** 2) for j in range(lx[b] + 1)]
        u2 = [np.sum(u[b, j] ** 2) for j in range(lu[b] + 1)]
        hand = [Q * sum(e2) + R * sum(u2), sum(e2), sum(u2), np.sqrt(e2[-1])]
        assert np.all(np.abs(out[b, :4] - hand) <= 1e-12 * np.abs(hand)), (b, out[b, :4], hand)
    assert abs(out[0, 0] - expect) <= 1e-12 * abs(expect)
    costs = m.closed_loop_costs(params, prob, solver, x, u)
    assert abs(out[0, 0] - costs[0]) <= 1e-12 * abs(costs[0])
    assert out[1, 0] < costs[1]                        # the default path adds the EE terms of a zero state for the two padded rows
    # no safe-set score asked for; the box margin is the hand-computed one
    assert np.all(out[:, 6] == np.inf) and np.all(outi[:, 3] == -1)
    for b in range(2):
        mb = [np.max(np.maximum(prob.x_min - x[b, j], x[b, j] - prob.x_max)) for j in range(lx[b] + 1)]
        assert out[b, 5] == max(mb) and outi[b, 2] == int(np.argmax(mb))
    # rows past last_x / last_u affect nothing
    x2, u2_ = x_log.copy(), u_log.copy()
    x2[2:, 1], u2_[1:, 1] = 1e300, 1e300
    o2, i2 = cl.score_rollout_statement(solver, prob, params, x2, u2_, lx, lu)
    assert np.array_equal(o2, out) and np.array_equal(i2, outi)


def test_traj_clamps_at_its_last_column():
    """a 3 x 5 trajectory on a 7-step log: steps 4..7 are held against column 4"""
    from safe_mpc_amd import closed_loop as cl
    from oracle.oracle import Oracle
    par, prob, net = make_problem('naive', N=2)
    solver = OracleSolver(prob, None)
    o = Oracle(prob)
    rng = np.random.default_rng(1)
    x0 = sample_instances(prob, 2, seed=1)
    x_log = x0[None] + 0.01 * rng.standard_normal((8, 2, prob.nx))
    u_log = rng.standard_normal((7, 2, prob.nu))
    traj = prob.ee_ref[:, None] + 0.1 * rng.standard_normal((3, 5))
    out, _ = cl.score_rollout_statement(solver, prob, par, x_log, u_log, traj=traj)
    for b in range(2):
        e2 = [np.sum((o.points(x_log[j, b, :prob.nq])[prob.desc.ee_point] - traj[:, min(j, 4)]) ** 2) for j in range(8)]
        assert abs(out[b, 1] - sum(e2)) <= 1e-12 * sum(e2) and abs(out[b, 3] - np.sqrt(e2[7])) <= 1e-12 * np.sqrt(e2[7])
    other, _ = cl.score_rollout_statement(solver, prob, par, x_log, u_log, traj=traj[:, :4])
    assert np.all(np.abs(other[:, 1] - out[:, 1]) > 1e-9)


@pytest.mark.parametrize('name', sc.PROBLEMS)
@pytest.mark.parametrize('T', sc.STEPS_GPU)
def test_planted_extremes_are_well_separated(name, T):
    """the logs test_score_gpu.py runs on: for EVERY instance the top two candidates of d4 over (step, row) and of d5 over the steps
    differ by more than 1e-6 and those of d6 by more than 1e-3 on the oracle side, so the integer slots are decided; the
    extremes are the planted ones (a violated row, a joint beyond x_max, g below every unplanted step's)"""
    par, prob, net = sc.case_problem(name)
    solver = OracleSolver(prob, net)
    x_log, u_log, lx, lu = sc.planted_logs(prob, solver.o, sc.B_GPU, T)
    assert np.all(lx >= np.maximum(lu, 0)) and lx.max() == T and lx.min() == 0 and lu.min() == -1
    rows, box, g = sc.candidates(solver, prob, par, x_log, lx)
    B = sc.B_GPU
    for cand, gap in ((rows.reshape(B, -1), 1e-6), (box, 1e-6), (-g, 1e-3)):
        if cand.shape[1] < 2:
            continue
        top = np.sort(cand, axis=1)[:, -2:]
        assert np.all(np.isfinite(top[:, 1]))
        assert np.all(top[:, 1] - top[:, 0] > gap), (name, T, np.min(top[:, 1] - top[:, 0]))
    if prob.desc.n_rows:          # (a log of one or two states has its extremes planted at one step: the joint moved last decides)
        assert np.all(rows.reshape(B, -1).max(1)[lx >= 2] > 1e-3)
    assert np.all(box.max(1) > 0.29)


def test_run_mpc_score_on_the_oracle_double():
    """run_mpc(score=True) through the CPU double: 'score' carries every slot as a [B] array, ee_dist < tol_conv agrees with
    conv_idx for the instances with complete logs, and score=False returns exactly today's keys"""
    from safe_mpc_amd import closed_loop as cl
    from safe_mpc_amd.solver import SCORE_INDEX_SLOTS, SCORE_SLOTS
    par, prob, net = make_problem('st', N=8)
    par.back_hor = 8
    B, n_steps = 4, 6
    x0 = sample_instances(prob, B, seed=3)
    xg, ug = np.repeat(x0[:, None, :], 9, axis=1), np.zeros((B, 8, 6))
    mk = lambda name, batch: make_double_controller(name, par, batch, N=8)          # noqa: E731
    mkb = lambda batch: make_double_controller('backup', par, batch)                 # noqa: E731
    res = cl.run_mpc(par, 'st', xg, ug, make_controller=mk, make_backup=mkb, n_steps=n_steps, score=True)
    ref = cl.run_mpc(par, 'st', xg, ug, make_controller=mk, make_backup=mkb, n_steps=n_steps)
    assert set(ref) == {'x', 'u', 'r', 'r_receding', 'conv_idx', 'collisions_idx', 'unconv_idx', 'viable_idx', 'x_viable'}
    assert set(res) == set(ref) | {'score'}
    for k in ref:
        if isinstance(ref[k], np.ndarray):
            assert np.array_equal(ref[k], res[k], equal_nan=True), k
        else:
            assert ref[k] == res[k], k
    s = res['score']
    assert set(s) == set(SCORE_SLOTS) | set(SCORE_INDEX_SLOTS)
    assert all(s[k].shape == (B,) for k in s)
    complete = ~np.isnan(res['x'][:, -1]).any(1)
    assert complete.any()
    conv = np.isin(np.arange(B), res['conv_idx'])
    assert np.array_equal((s['ee_dist'] < par.tol_conv)[complete], conv[complete])
    # ... also with a tolerance that splits the instances (the run itself does not depend on tol_conv)
    par.tol_conv = float(np.median(s['ee_dist'][complete]))
    split = cl.run_mpc(par, 'st', xg, ug, make_controller=mk, make_backup=mkb, n_steps=n_steps, score=True)
    conv2 = np.isin(np.arange(B), split['conv_idx'])
    assert np.array_equal(split['score']['ee_dist'], s['ee_dist'])
    assert np.array_equal((s['ee_dist'] < par.tol_conv)[complete], conv2[complete]) and conv2.any() and not conv2.all()
    # the cost of a complete log is the metric's; the safe-set score is there ('st' has the row at node N)
    m = _load_script()
    costs = m.closed_loop_costs(par, prob, OracleSolver(prob, net), res['x'][complete], res['u'][complete])
    assert np.all(np.abs(s['cost'][complete] - costs) <= 1e-9 * (1 + np.abs(costs)))
    assert np.all(np.isfinite(s['safe_min'])) and np.all(s['safe_step'] >= 0)


def test_metrics_count_fails_scored(tmp_path):
    """--scored on the oracle double reproduces test_metrics' expected cost of the complete instance"""
    m = _load_script()
    params, prob = _metrics_setup(tmp_path)
    expect = _two_instance_pickle(tmp_path, params, prob, _ee_by_oracle(prob))
    scores = m.main(['-c', 'st', '--horizon', '30', '--alpha', '10', '--data_dir', str(tmp_path), '--scored'],
                    make_solver=lambda p: OracleSolver(p, None))
    s = scores['st']
    assert s['fails'] == 1 and s['completed_idx'] == [0] and s['costs'][1] == -100.0
    assert abs(s['costs'][0] - expect) < 1e-9 * abs(expect)
    # a truncated log counts its valid rows only
    import pickle
    from safe_mpc_amd import closed_loop as cl
    res = pickle.load(open(cl.result_file(params, 'z1', 'st', params.N, True, 0.0, 0.0, 0.0, 0.0), 'rb'))
    solver = OracleSolver(prob, None)
    both = m.closed_loop_costs_scored(params, prob, solver, res['x'], res['u'])
    ee = _ee_by_oracle(prob)
    hand = sum(params.Q_weight * np.sum((ee(res['x'][1, j, :6]) - prob.ee_ref) ** 2) for j in range(2)) + \
        params.R_weight * np.sum(res['u'][1, 0] ** 2)
    assert abs(both[0] - expect) < 1e-9 * abs(expect) and abs(both[1] - hand) < 1e-9 * abs(hand)


def test_header_declares_score_rollout_and_the_mirror_matches(tmp_path):
    from safe_mpc_amd import _lib
    from safe_mpc_amd.solver import SCORE_ND, SCORE_NI
    hdr = open(os.path.join(ROOT, 'include', 'smpc.h')).read()
    assert 'int smpc_score_rollout(' in hdr and 'smpc_score_rollout' in _lib.SYMBOLS
    src = tmp_path / 'sz.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "smpc.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %d %d %d\\n", sizeof(smpc_score_params), '
                   'offsetof(smpc_score_params, want_safe), offsetof(smpc_score_params, x_min), offsetof(smpc_score_params, traj), '
                   'offsetof(smpc_score_params, traj_len), SMPC_SCORE_ND, SMPC_SCORE_NI, SMPC_ABI_VERSION); return 0; }\n')
    exe = tmp_path / 'sz'
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    v = [int(t) for t in subprocess.check_output([str(exe)]).split()]
    P = _lib.ScoreParams
    assert v == [C.sizeof(P), P.want_safe.offset, P.x_min.offset, P.traj.offset, P.traj_len.offset, SCORE_ND, SCORE_NI, 5]
