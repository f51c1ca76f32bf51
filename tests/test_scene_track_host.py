"""Obstacle tracks (smpc_set_instance_scene_track, smpc_set_scene_clock) without a GPU: how tracks are made, what the closed loop
hands to its solvers and when, and the score statement's column rule -- on the CPU oracle (track_cases.TrackOracleSolver: one
oracle per scene, composed per node)."""
import ctypes
import importlib.util
import os
import pickle
import re

import numpy as np
import pytest

import scene_cases as sc
import track_cases as tc
from conftest import ROOT, make_problem, make_problem_fr7, sample_instances
from fake_solver import OracleSolver
from safe_mpc_amd import closed_loop as cl
from safe_mpc_amd import controller as C
from safe_mpc_amd.problem import (ROW_COORD, ROW_SEG_SEG, SCENE_ROW, extend_tracks, jittered_scenes, moving_scenes,
                                  scenes_from_problems)


# ---- 1. making tracks ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('system', ['z1', 'fr7'])
def test_scene_track_and_moving_scenes(system):
    par, prob, net = make_problem('st', N=8) if system == 'z1' else make_problem_fr7(N=8)
    R, dt = len(prob.rows), float(prob.desc.dt)
    names = sorted({n for n in prob.row_obstacle if n is not None})
    # scene_track: a scene per entry of moves; without a move, the descriptor's geometry
    d = np.array([0.01, -0.02, 0.03])
    tr = prob.scene_track([{}, {names[0]: d}, {n: 2 * d for n in names}])
    assert tr.shape == (3, R, SCENE_ROW)
    assert np.array_equal(tr[0], prob.row_geometry())
    assert np.array_equal(tr[1], prob.scene({names[0]: d})) and np.array_equal(tr[2], prob.scene({n: 2 * d for n in names}))
    with pytest.raises(ValueError, match='at least one time column'):
        prob.scene_track([])
    with pytest.raises(ValueError, match='unknown obstacle'):
        prob.scene_track([{}, {'no such thing': d}])
    # moving_scenes: shapes, column 0, constant velocity, reproducible by seed
    B, T, sv = 5, 7, 0.2
    m = moving_scenes(prob, B, T, sv, seed=3)
    assert m.shape == (B, T, R, SCENE_ROW)
    assert all(np.array_equal(m[b, 0], prob.row_geometry()) for b in range(B))
    step = m[:, 1] - m[:, 0]
    for j in range(T):
        assert np.allclose(m[:, j], m[:, 0] + j * step, rtol=0, atol=1e-14)
    assert np.array_equal(m, moving_scenes(prob, B, T, sv, seed=3)) and not np.array_equal(m, moving_scenes(prob, B, T, sv, seed=4))
    assert np.array_equal(m[:3], moving_scenes(prob, 3, T, sv, seed=3))             # instance b's draw does not depend on B
    assert np.array_equal(moving_scenes(prob, B, T, 0.0, seed=3), np.repeat(m[:, :1], T, axis=1))
    # velocities: one draw per (instance, obstacle), shared by its rows; of the size asked for; nothing else moves
    vel = step / dt                                                                    # [B, R, 8]
    for r, (row, name) in enumerate(zip(prob.rows, prob.row_obstacle)):
        if name is None:
            assert row.kind == ROW_SEG_SEG and not vel[:, r].any()
        elif row.kind == ROW_COORD:
            # a plane row moves only along its axis: the offset takes that component, C and D stay
            assert not vel[:, r, :6].any() and not vel[:, r, 7].any()
            mates = [k for k, n in enumerate(prob.row_obstacle) if n == name and prob.rows[k].kind != ROW_COORD]
            for k in mates:
                assert np.allclose(vel[:, r, 6], vel[:, k, row.axis], atol=1e-9)
        else:
            assert not vel[:, r, 6:].any()
            if row.kind == 0:
                assert np.allclose(vel[:, r, 0:3], vel[:, r, 3:6], atol=1e-9)       # a capsule translates: both end points alike
            else:
                assert not vel[:, r, 3:6].any()
    moving = [r for r, n in enumerate(prob.row_obstacle) if n is not None]
    big = moving_scenes(prob, 400, 2, sv, seed=1)
    v = ((big[:, 1] - big[:, 0]) / dt)[:, moving]
    comp = np.concatenate([v[:, k, 6:7] if prob.rows[r].kind == ROW_COORD else v[:, k, 0:3] for k, r in enumerate(moving)], axis=1)
    assert abs(comp.std() / sv - 1.0) < 0.1 and abs(comp.mean()) < 0.1 * sv
    # with a jitter the start column is jittered_scenes of the same seed, and the velocities are the same draws
    mj = moving_scenes(prob, B, T, sv, seed=3, sigma=0.05)
    assert np.array_equal(mj[:, 0], jittered_scenes(prob, B, 0.05, seed=3))
    assert np.allclose(mj[:, 1] - mj[:, 0], step, atol=1e-14)
    # extend_tracks: continued at the last step, or cut
    ext = extend_tracks(m[:, :3], T)
    assert ext.shape == m.shape and np.allclose(ext, m, atol=1e-13) and np.array_equal(ext[:, :3], m[:, :3])
    assert np.array_equal(extend_tracks(m, 2), m[:, :2])
    assert np.array_equal(extend_tracks(m[:, :1], 3), np.repeat(m[:, :1], 3, axis=1))


def test_check_scenes_takes_scenes_and_tracks():
    par, prob, net = make_problem('st', N=6)
    R = len(prob.rows)
    g3, g4 = np.zeros((4, R, 8), np.float32), np.zeros((4, 5, R, 8))
    a, b = cl._check_scenes(g3, 4, prob), cl._check_scenes(g4[:, ::1], 4, prob)
    assert a.shape == (4, R, 8) and a.dtype == np.float64 and a.flags.c_contiguous
    assert b.shape == (4, 5, R, 8) and b.flags.c_contiguous
    assert cl._check_scenes(np.zeros((4, 1, R, 8)), 4, prob).shape == (4, 1, R, 8)
    for bad, B in [(g3, 3), (g4, 5), (np.zeros((4, R, 7)), 4), (np.zeros((4, 5, R + 1, 8)), 4), (np.zeros((4, 0, R, 8)), 4),
                   (np.zeros((4, 2, 3, R, 8)), 4), (np.zeros((R, 8)), 4)]:
        with pytest.raises(ValueError, match='scenes: shape'):
            cl._check_scenes(bad, B, prob)
    prob.rows = []
    with pytest.raises(ValueError, match='no collision rows'):
        cl._check_scenes(np.zeros((4, 3, 0, 8)), 4, prob)


# ---- 2. the ABI -----------------------------------------------------------------------------------------------------------------
def test_library_exports_the_two_entry_points_and_the_header_states_the_rule():
    from safe_mpc_amd import _lib
    new = {'smpc_set_instance_scene_track', 'smpc_set_scene_clock'}
    assert new <= set(_lib.SYMBOLS)
    assert os.path.exists(_lib.LIB_PATH), 'the engine is built before the tests run (__graft_entry__.build)'
    L = ctypes.CDLL(_lib.LIB_PATH)               # loads without a GPU
    hdr = open(os.path.join(ROOT, 'include', 'smpc.h')).read()
    declared = set(re.findall(r'^(?:int|void|void\*|const char\*)\s+(smpc_[a-z_]+)\s*\(', hdr, re.M))
    assert new <= declared and declared == set(_lib.SYMBOLS)
    for name in new:
        assert hasattr(L, name), name
    L.smpc_abi_version.restype = ctypes.c_int
    assert L.smpc_abi_version() == 5             # nothing existing changed
    assert hdr.count('col(c) = clamp(c, 0, T - 1)') == 1


# ---- 3. the closed loop ---------------------------------------------------------------------------------------------------------------
LOOP_N = 6


def _pars(n_scenes):
    pars = []
    for shift in sc.SHIFTS[:n_scenes]:
        par, _, _ = make_problem('htwa', N=LOOP_N)
        par.back_hor = 8
        sc.move_obstacles(par, shift, sc.Z1_OBSTACLES)
        pars.append(par)
    return pars


def test_run_mpc_with_tracks_clocks_backup_and_clean_handles():
    """'htwa', 5 instances, 7 steps on the host path around TrackOracleSolver.  Every instance's track holds ONE scene in all its
    columns (the oracle solves in one scene), another for each neighbour.  The clock cell reads 0, 1, 2, .. at the solves and
    j + 1 at the plant's test of step j; scripted failures make instances 1 and 3 abort at step N - 1: the backup solver gets
    their tracks, in the order of the compact batch, and a clock cell that reads N - 1 at its solve; both solvers end without
    scene, track or clock; and the logs are bit for bit those of run_mpc(scenes=static)."""
    N, B, steps, T = LOOP_N, 5, 7, 4
    pars = _pars(2)
    base = C.OcpProblem(pars[0], 'htwa', 'ext', N=N)
    geoms = scenes_from_problems(base, [C.OcpProblem(p, 'htwa', 'ext', N=N) for p in pars])
    scene_of = np.array([0, 1, 0, 1, 1])
    static = geoms[scene_of]
    track = np.ascontiguousarray(np.repeat(static[:, None], T, axis=1))
    x0 = sample_instances(base, B, seed=5, vel_scale=0.1)
    xg, ug = np.repeat(x0[:, None, :], N + 1, axis=1), np.zeros((B, N, 6))
    fail = np.array([0, 4, 0, 4, 0], np.int32)

    def run(scenes):
        solvers = {}
        mk, mkb = tc.oracle_factories(pars[0], N, pars, geoms, log=solvers)

        def mk_scripted(name, batch):
            ctrl = mk(name, batch)
            ctrl.ocp_solver.scripted_status = [fail.copy() for _ in range(N)] + [np.zeros(B, np.int32)] * 8
            return ctrl
        return cl.run_mpc(pars[0], 'htwa', xg, ug, make_controller=mk_scripted, make_backup=mkb, n_steps=steps, scenes=scenes,
                          score=True), solvers
    res, sv = run(track)
    ref, sv_ref = run(static)
    main, back = sv['htwa'], sv['backup']
    assert res['scenes'].shape == (B, T, len(base.rows), 8) and np.array_equal(res['scenes'], track)
    # the controller's handle: the group's tracks once, before anything else; cleared at the end, the clock with it
    assert len(main.track_calls) == 1 and np.array_equal(main.track_calls[0], track)
    assert main.scene_calls[-1] is None and main.track is None and main.idx is None
    assert len(main.clock_calls) == 2 and main.clock_calls[-1] is None and main.clock is None
    cell = main.clock_calls[0]
    assert isinstance(cell, np.ndarray) and cell.dtype == np.int64 and cell.shape == (1,)
    # the clock at the solves of the loop: 0, 1, 2, ...; at the plant's outcome test of step j: j + 1
    loop_log = main.clock_log[:next(k for k, c in enumerate(main.clock_log) if c[0] == 'eval_nodes')]       # (the scores come after)
    assert [t for who, t in loop_log if who == 'solve'] == list(range(steps))
    plant = [t for k, (who, t) in enumerate(loop_log) if who == 'check_trajectory' and (k + 1 == len(loop_log) or loop_log[k + 1][0] == 'solve')]
    assert plant == list(range(1, steps + 1))
    # the abort event of step N - 1: rows 1 and 3, their tracks, the same clock
    assert len(back.track_calls) == 1 and np.array_equal(back.track_calls[0], track[[1, 3]])
    assert [c for c in back.clock_log if c[0] == 'solve'] == [('solve', N - 1)]
    assert back.clock is None and back.track is None and back.idx is None and back.scene_calls[-1] is None
    assert back.clock_calls[0] is not cell and back.clock_calls[-1] is None
    assert res['x_viable'].shape[0] == 2
    # all columns equal: the run in the static scenes, bit for bit
    for key in ('x', 'u'):
        assert np.array_equal(res[key], ref[key], equal_nan=True), key
    for key in ('conv_idx', 'collisions_idx', 'viable_idx', 'unconv_idx'):
        assert res[key] == ref[key], key
    for key, val in res['score'].items():
        assert np.array_equal(val, ref['score'][key], equal_nan=True), key
    assert not sv_ref['htwa'].track_calls and not sv_ref['htwa'].clock_log
    # a track is refused where a scene is: the parallel policy, another batch size, generate_guess_until
    mk, mkb = tc.oracle_factories(pars[0], N, pars, geoms)
    with pytest.raises(ValueError, match="'parallel' policy is not supported"):
        cl.run_mpc(pars[0], 'parallel', xg, ug, make_controller=mk, make_backup=mkb, n_steps=2, scenes=track)
    with pytest.raises(ValueError, match='scenes'):
        cl.run_mpc(pars[0], 'htwa', xg, ug, make_controller=mk, make_backup=mkb, n_steps=2, scenes=track[:4])
    with pytest.raises(ValueError, match='not supported'):
        cl.generate_guess_until(pars[0], 'htwa', 2, scenes=track[:2])

    # a solver that takes scenes but no tracks is refused by name, before the loop starts
    def mk_old(name, batch):
        return tc.oracle_factories(pars[0], N, pars, geoms, solver_cls=sc.SceneOracleSolver)[0](name, batch)
    with pytest.raises(ValueError, match='SceneOracleSolver has no set_instance_scene_track'):
        cl.run_mpc(pars[0], 'htwa', xg, ug, make_controller=mk_old, make_backup=mkb, n_steps=2, scenes=track)


# ---- 4. the score statement -----------------------------------------------------------------------------------------------------------
def test_score_statement_evaluates_state_j_in_column_j():
    """a 12-step log of 5 instances, tracks of T = 4 columns that differ from column to column: coll_margin, coll_step and coll_row
    against a loop over (instance, state) on the oracle of the scene in column min(j, T - 1); the statement's calls pack 9 states
    each (N = 8), so its second call runs at clock 9"""
    N, B, n_steps, T = 8, 5, 12, 4
    (par, prob, net), moved, geom = sc.scene_family('z1', 'st', N, 4)
    idx = tc.track_indices(B, T)
    track = np.ascontiguousarray(geom[idx])
    sv = tc.TrackOracleSolver(prob, net, [m[1] for m in moved], geom)
    sv.set_instance_scene_track(track)
    cell = np.zeros(1, np.int64)
    sv.set_scene_clock(cell)
    rng = np.random.default_rng(11)
    x0 = sample_instances(prob, B, seed=5, vel_scale=0.1)
    x_log = x0[None] + 0.03 * np.cumsum(rng.standard_normal((n_steps + 1, B, prob.nx)), axis=0) * (np.arange(prob.nx) < prob.nq)
    u_log = rng.standard_normal((n_steps, B, prob.nu))
    last_x = np.array([12, 12, 7, 12, 3])
    out, outi = cl.score_rollout_statement(sv, prob, par, x_log, u_log, last_x=last_x, last_u=np.minimum(last_x, 11),
                                           per_instance=True, scene_clock=cell)
    assert [t for who, t in sv.clock_log] == [0, N + 1]
    lo, hi = prob.row_check[:, 0], prob.row_check[:, 1]
    singles = [OracleSolver(m[1], net) for m in moved]
    nr = len(prob.rows)
    m = np.full((B, n_steps + 1, nr), -np.inf)
    for b in range(B):
        for j in range(int(last_x[b]) + 1):
            s = idx[b, min(j, T - 1)]
            xg = np.repeat(x_log[j, b][None, None, :], N + 1, axis=1)
            p = np.zeros((1, N + 1, 5))
            p[:, :, 3], p[:, :, 4] = par.alpha, 1.0
            rv = np.asarray(singles[s].eval_nodes(xg, np.zeros((1, N, prob.nu)), p)['row_val'])[0, 0, :nr]
            m[b, j] = np.maximum(lo - rv, rv - hi)
    at = m.reshape(B, -1).argmax(1)
    assert np.array_equal(out[:, 4], m.reshape(B, -1)[np.arange(B), at])
    assert np.array_equal(outi[:, 0], at // nr) and np.array_equal(outi[:, 1], at % nr)
    # the columns matter: every state in column 0 is another score
    sv.set_instance_scene(np.ascontiguousarray(track[:, 0]))
    out0, _ = cl.score_rollout_statement(sv, prob, par, x_log, u_log, last_x=last_x, last_u=np.minimum(last_x, 11), per_instance=True)
    assert (out0[:, 4] != out[:, 4]).any()
    assert np.array_equal(out0[:, [0, 1, 2, 3, 5]], out[:, [0, 1, 2, 3, 5]])           # (what no obstacle enters is the same)


# ---- 5. the entry scripts -----------------------------------------------------------------------------------------------------------
def _script(name):
    spec = importlib.util.spec_from_file_location('smpc_track_script_' + name, os.path.join(ROOT, 'scripts', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_entry_scripts_take_scene_velocity(monkeypatch, tmp_path):
    """--scene-velocity SIGMA on both scripts, with the engine calls replaced: guess_acados.py hands generate_guess tracks one
    horizon long and stores those of the accepted guesses as 'scenes' [n, T, R, 8]; mpc.py continues stored tracks over the run (or
    draws them) and its result carries them"""
    seen, saved = {}, {}
    monkeypatch.setattr(cl, 'save_pickle', lambda path, obj: saved.__setitem__(os.path.basename(str(path)), obj))

    def fake_guess(params, name, n, verbose=False, on_device=False, scenes=None, traj=None):
        seen['guess'] = scenes
        good = np.arange(n) % 3 != 1
        N = int(params.N)
        return {'xg': np.zeros((good.sum(), N + 1, 12)), 'ug': np.zeros((good.sum(), N, 6)), 'scenes': scenes[good]}, good
    monkeypatch.setattr(cl, 'generate_guess', fake_guess)
    argv = ['-c', 'naive', '--horizon', '10', '--scene-velocity', '0.3', '--scene-seed', '4', '--scene-jitter', '0.02']
    assert _script('guess_acados').main(argv) == 0
    tr = seen['guess']
    n, R = tr.shape[0], tr.shape[2]
    assert tr.shape == (n, 11, R, 8) and n >= 3
    prob = C.OcpProblem(make_problem('naive', N=10)[0], 'naive')
    assert np.array_equal(tr, moving_scenes(prob, n, 11, 0.3, seed=4, sigma=0.02))
    (gname, guess), = saved.items()
    assert guess['scenes'].shape == (guess['xg'].shape[0], 11, R, 8) and guess['scenes'].ndim == 4

    # mpc.py: loads that pickle, continues its tracks to n_steps + 1 + N columns at their velocity
    gfile = tmp_path / 'guess.pkl'
    pickle.dump(guess, open(gfile, 'wb'))
    monkeypatch.setattr(cl, 'guess_file', lambda *a, **k: str(gfile))
    monkeypatch.setattr(cl, 'result_file', lambda *a, **k: 'result.pkl')

    def fake_run(params, name, x_guess, u_guess, scenes=None, timing=None, **kw):
        seen['run'], seen['n_steps'] = scenes, int(params.n_steps)
        timing['ms_per_step'] = 0.0
        return {'conv_idx': [], 'collisions_idx': [], 'viable_idx': [], 'scenes': scenes}
    monkeypatch.setattr(cl, 'run_mpc', fake_run)
    saved.clear()
    assert _script('mpc').main(argv) == 0
    T = seen['n_steps'] + 1 + 10
    nb = guess['xg'].shape[0]
    assert seen['run'].shape == (nb, T, R, 8)
    assert np.array_equal(seen['run'][:, :11], guess['scenes'])
    assert np.allclose(seen['run'], moving_scenes(prob, n, T, 0.3, seed=4, sigma=0.02)[np.arange(n) % 3 != 1], atol=1e-12)
    assert saved['result.pkl']['scenes'].shape == (nb, T, R, 8)
    # without stored tracks it draws them for the loaded guesses
    pickle.dump({k: v for k, v in guess.items() if k != 'scenes'}, open(gfile, 'wb'))
    assert _script('mpc').main(argv) == 0
    assert np.array_equal(seen['run'], moving_scenes(prob, nb, T, 0.3, seed=4, sigma=0.02))
