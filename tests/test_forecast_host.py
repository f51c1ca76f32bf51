"""Obstacle forecasts (smpc_set_instance_world_track, smpc_forecast_scene) without a GPU: the numpy statement,
the track generator whose obstacles change course, what run_mpc(forecast=...) hands to its solvers and when -- on the CPU oracle
(track_cases.TrackOracleSolver) --, the ABI and the entry script's flags."""
import ctypes
import importlib.util
import os
import pickle
import re

import numpy as np
import pytest

import forecast_cases as fc
import scene_cases as sc
import track_cases as tc
from conftest import ROOT, make_problem, sample_instances
from safe_mpc_amd import closed_loop as cl
from safe_mpc_amd import controller as C
from safe_mpc_amd.problem import (FORECAST_MODES, ROW_COORD, forecast_statement, moving_scenes, scenes_from_problems,
                                  turning_scenes)


# ---- 1. the statement ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('system', ['z1', 'fr7'])
def test_statement_hold_cv_true(system):
    """all three modes over the clock family, T in {1, 2, N + 1, N + 4}: 'true' is the col(t + k) gather; 'hold' repeats column col(t);
    'cv' starts there and steps by W[col(t)] - W[col(t - 1)], which is nothing where the two columns coincide (t <= 0, t >= T, T = 1)"""
    N, B = 4, 3
    par, prob, net = fc.problem(system, N)
    for T in (1, 2, N + 1, N + 4):
        W = fc.world(prob, B, T)
        for t in fc.clocks(T):
            tt = 0 if t is None else min(max(t, -2 ** 62), 2 ** 62)
            c0, c1 = min(max(tt, 0), T - 1), min(max(tt - 1, 0), T - 1)
            hold, cv, true = (forecast_statement(W, t, N, m) for m in fc.MODES)
            assert hold.shape == cv.shape == true.shape == (B, N + 1, len(prob.rows), 8)
            assert np.array_equal(true, fc.gather_true(W, t, N)), (T, t)
            assert all(np.array_equal(hold[:, k], W[:, c0]) for k in range(N + 1)), (T, t)
            assert np.array_equal(cv[:, 0], W[:, c0])
            if c0 == c1:
                assert np.array_equal(cv, hold), (T, t)
            else:
                d = W[:, c0] - W[:, c1]
                assert (d != 0).all()
                f = W[:, c0]
                for k in range(1, N + 1):
                    f = f + d
                    assert np.array_equal(cv[:, k], f), (T, t, k)
                assert not np.array_equal(cv, hold)
            for m in fc.MODES:      # by number as by name
                assert np.array_equal(forecast_statement(W, t, N, FORECAST_MODES[m]), forecast_statement(W, t, N, m))
    with pytest.raises(ValueError, match='expected a world track'):
        forecast_statement(W[:, 0], 0, N, 'cv')
    with pytest.raises(KeyError):
        forecast_statement(W, 0, N, 'linear')
    with pytest.raises(ValueError, match='mode 7'):
        forecast_statement(W, 0, N, 7)


@pytest.mark.parametrize('N', [1, 8, 30])
def test_cv_on_a_constant_velocity_world_is_the_truth(N):
    """moving_scenes moves everything at constant velocity, so with 1 <= t and t + N <= T - 1 the CV forecast is the world up to
    rounding: |F - W[col(t + k)]| <= 1e-12 (1 + max|W|).  Derived, not measured: the one subtraction and each of at most 30 additions
    round by at most 2^-53 relative, about 1e-14 in all (and the track's own columns carry a rounding each); the bound leaves a
    factor 100."""
    par, prob, net = fc.problem('z1', 4)
    T = N + 6
    W = moving_scenes(prob, 4, T, 0.4, seed=3, sigma=0.02)
    for t in (1, 2, T - 1 - N):
        F = forecast_statement(W, t, N, 'cv')
        err = np.abs(F - fc.gather_true(W, t, N)).max()
        print(f'N = {N}, t = {t}: CV against the truth, max abs error {err:.3e}')
        assert err <= 1e-12 * (1 + np.abs(W).max()), (t, err)
    assert np.abs(forecast_statement(W, 2, N, 'hold') - fc.gather_true(W, 2, N)).max() > 1e-4        # (the world does move)


# ---- 2. obstacles that change course ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('system', ['z1', 'fr7'])
def test_turning_scenes(system):
    par, prob, net = fc.problem(system, 4)
    B, T, dt = 5, 12, float(prob.desc.dt)
    a = turning_scenes(prob, B, T, 0.3, 2.0, seed=4, sigma=0.01)
    assert a.shape == (B, T, len(prob.rows), 8)
    assert np.array_equal(a, turning_scenes(prob, B, T, 0.3, 2.0, seed=4, sigma=0.01))             # reproducible per seed
    assert not np.array_equal(a, turning_scenes(prob, B, T, 0.3, 2.0, seed=5, sigma=0.01))
    # without accelerations: the constant-velocity track of the same seed
    cv = moving_scenes(prob, B, T, 0.3, seed=4, sigma=0.01)
    assert np.abs(turning_scenes(prob, B, T, 0.3, 0.0, seed=4, sigma=0.01) - cv).max() <= 1e-12
    assert np.array_equal(a[:, 0], cv[:, 0]) and np.allclose(a[:, 1], cv[:, 1], atol=1e-12)        # column 0 and v_0 are its draws
    # the velocity does turn: the second differences are not zero, and they are N(0, sigma_a^2) dt^2 in size
    acc = np.diff(a, 2, axis=1) / dt ** 2
    moved = np.abs(np.diff(cv, axis=1)).max(axis=(0, 1)) > 0                                        # [row, slot]: what an obstacle moves
    assert moved.any() and (np.abs(acc[:, :, moved]) > 0).all() and (np.abs(acc[:, :, ~moved]) < 1e-6).all()
    assert 0.5 < acc[:, :, moved].std() / 2.0 < 1.5
    # one draw per (instance, obstacle), shared by the rows the obstacle appears in; a plane row takes its axis
    step = a[:, 1:] - a[:, :-1]
    names = {}
    for i, name in enumerate(prob.row_obstacle):
        if name is not None:
            names.setdefault(name, []).append(i)
    assert names
    for name, rows in names.items():
        ref = next((i for i in rows if prob.rows[i].kind != ROW_COORD), None)
        for i in rows:
            r = prob.rows[i]
            if r.kind == ROW_COORD:
                assert (np.abs(step[:, :, i, 6]) > 0).all() and np.abs(step[:, :, i, :6]).max() == 0
                if ref is not None:
                    assert np.allclose(step[:, :, i, 6], step[:, :, ref, r.axis], atol=1e-12)
            elif ref is not None:
                assert np.allclose(step[:, :, i, :3], step[:, :, ref, :3], atol=1e-12)
    for i, name in enumerate(prob.row_obstacle):
        if name is None:
            assert np.abs(step[:, :, i]).max() == 0
    with pytest.raises(ValueError, match='at least one time column'):
        turning_scenes(prob, B, 0, 0.3, 1.0)
    assert turning_scenes(prob, 2, 1, 0.3, 1.0).shape == (2, 1, len(prob.rows), 8)


# ---- 3. the ABI ---------------------------------------------------------------------------------------------------------------------
def test_the_symbols_are_declared_exported_and_prototyped():
    from safe_mpc_amd import _lib, solver
    hdr = open(os.path.join(ROOT, 'include', 'smpc.h')).read()
    declared = set(re.findall(r'^(?:int|void|const char\*|void\*) (smpc_\w+)\(', hdr, re.M))
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('smpc_set_instance_world_track', 'smpc_forecast_scene'):
        assert name in declared and name in _lib.SYMBOLS and hasattr(L, name), name
    assert declared == set(_lib.SYMBOLS)
    vp = ctypes.c_void_p
    assert _lib.lib().smpc_set_instance_world_track.argtypes == [vp, ctypes.c_int, ctypes.c_int64, vp, ctypes.c_int]
    assert _lib.lib().smpc_forecast_scene.argtypes == [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp]
    assert callable(solver.BatchedOcpSolver.set_instance_world_track) and callable(solver.BatchedOcpSolver.forecast_scene)
    assert solver.FORECAST_MODES == {'hold': 0, 'cv': 1, 'true': 2}
    for name, val in (('SMPC_FORECAST_HOLD', 0), ('SMPC_FORECAST_CV', 1), ('SMPC_FORECAST_TRUE', 2)):
        assert re.search(rf'\b{name} = {val}\b', hdr), name
    L.smpc_abi_version.restype = ctypes.c_int
    assert L.smpc_abi_version() == 5             # nothing existing changed


# ---- 4. the closed loop on the host path -----------------------------------------------------------------------------------------------
LOOP_N = 6


class Recorder(tc.TrackOracleSolver):
    """TrackOracleSolver that writes down, in order, what the loop hands it and at which clock it is asked.  The oracle behind it
    knows whole scenes only, so the worlds of these tests hold one scene per instance in all their columns; a CV forecast of such a
    world is W + 0.0, which turns a -0.0 into 0.0, so scenes are looked up by value (x + 0.0 on both sides)."""

    def __init__(self, *a):
        super().__init__(*a)
        self.keys = [(np.frombuffer(k, np.float64) + 0.0).tobytes() for k in self.keys]
        self.events = []

    def _now(self):
        return None if self.clock is None else int(np.asarray(self.clock).reshape(-1)[0])

    def set_instance_scene(self, geom=None):
        self.events.append(('scene', None if geom is None else np.array(geom)))
        super().set_instance_scene(None if geom is None else np.asarray(geom, float) + 0.0)

    def set_instance_scene_track(self, geom=None):
        self.events.append(('track', None if geom is None else np.array(geom)))
        super().set_instance_scene_track(None if geom is None else np.asarray(geom, float) + 0.0)

    def set_scene_clock(self, clock=None):
        self.events.append(('clock', clock))
        super().set_scene_clock(clock)

    def solve(self, *a, **kw):
        self.events.append(('solve', self._now()))
        return super().solve(*a, **kw)

    def check_trajectory(self, x, **kw):
        self.events.append(('check_trajectory', self._now(), np.asarray(x).shape[1]))
        return super().check_trajectory(x, **kw)

    def eval_nodes(self, *a):
        self.events.append(('eval_nodes', self._now()))
        return super().eval_nodes(*a)


def _loop_setup():
    pars = []
    for shift in sc.SHIFTS[:2]:
        par, _, _ = make_problem('htwa', N=LOOP_N)
        par.back_hor = 8
        sc.move_obstacles(par, shift, sc.Z1_OBSTACLES)
        pars.append(par)
    base = C.OcpProblem(pars[0], 'htwa', 'ext', N=LOOP_N)
    geoms = scenes_from_problems(base, [C.OcpProblem(p, 'htwa', 'ext', N=LOOP_N) for p in pars])
    return pars, base, geoms


def _same_events(a, b):
    if len(a) != len(b):
        return False
    for ea, eb in zip(a, b):
        if ea[0] != eb[0] or len(ea) != len(eb):
            return False
        for va, vb in zip(ea[1:], eb[1:]):
            if isinstance(va, np.ndarray) and isinstance(vb, np.ndarray) and va.dtype == np.int64 and va.shape == (1,):
                continue                                     # (a clock cell: each run makes its own)
            if isinstance(va, np.ndarray) or isinstance(vb, np.ndarray):
                if not (isinstance(va, np.ndarray) and isinstance(vb, np.ndarray) and np.array_equal(va, vb)):
                    return False
            elif va != vb:
                return False
    return True


@pytest.mark.parametrize('mode', ['hold', 'cv', 'true'])
def test_run_mpc_forecast_on_the_host_path_is_the_statement(mode):
    """'htwa', 5 instances, 7 steps around the recording double; the world holds one scene per instance in all T columns, scripted
    failures make instances 1 and 3 abort at step N - 1.  Every step, in this order: the forecast of the statement at time j as a
    track WITHOUT a clock, the solve, then the world with the clock at j + 1 and the plant's one-node test.  The backup solver gets
    the forecast of the aborting rows over ITS horizon at the event's time, without a clock.  The slot is re-set to the world before
    the scores, and both solvers end without scene, track and clock.  With every column alike the logs are those of the run
    without a forecast, bit for bit."""
    N, B, steps, T = LOOP_N, 5, 7, 4
    pars, base, geoms = _loop_setup()
    world = np.ascontiguousarray(np.repeat(geoms[np.array([0, 1, 0, 1, 1])][:, None], T, axis=1))
    x0 = sample_instances(base, B, seed=5, vel_scale=0.1)
    xg, ug = np.repeat(x0[:, None, :], N + 1, axis=1), np.zeros((B, N, 6))
    fail = np.array([0, 4, 0, 4, 0], np.int32)

    def run(**kw):
        solvers = {}
        mk, mkb = tc.oracle_factories(pars[0], N, pars, geoms, log=solvers, solver_cls=Recorder)

        def mk_scripted(name, batch):
            ctrl = mk(name, batch)
            ctrl.ocp_solver.scripted_status = [fail.copy() for _ in range(N)] + [np.zeros(B, np.int32)] * 8
            return ctrl
        return cl.run_mpc(pars[0], 'htwa', xg, ug, make_controller=mk_scripted, make_backup=mkb, n_steps=steps, scenes=world,
                          score=True, **kw), solvers
    res, sv = run(forecast=mode)
    ref, sv_ref = run()
    assert res['forecast'] == mode and 'forecast' not in ref
    main, back = sv['htwa'], sv['backup']
    ev = main.events
    first_score = next(k for k, e in enumerate(ev) if e[0] == 'eval_nodes')
    loop, rest = ev[:first_score], ev[first_score:]
    # the loop: per step  clock(None) - track(forecast) - [controller's tests] - solve - [tests] - track(world) - clock(cell) - plant test
    solves = [k for k, e in enumerate(loop) if e[0] == 'solve']
    assert len(solves) == steps
    cells = []
    for j, k in enumerate(solves):
        before = loop[(solves[j - 1] if j else -1) + 1:k]
        tracks = [e for e in before if e[0] == 'track']
        assert np.array_equal(tracks[-1][1], forecast_statement(world, j, N, mode)), j              # the forecast, made at time j
        assert tracks[-1][1].shape[1] == N + 1
        clocks = [e for e in before if e[0] == 'clock']
        assert clocks[-1][1] is None and loop[k][1] is None                                       # ... read from time 0
        kt, kc = [m for m, e in enumerate(before) if e[0] == 'track'][-1], [m for m, e in enumerate(before) if e[0] == 'clock'][-1]
        assert kc < kt                                                                            # no clock, then the forecast
        after = loop[k + 1:solves[j + 1] if j + 1 < steps else len(loop)]
        plant = [m for m, e in enumerate(after) if e[0] == 'check_trajectory' and e[2] == 1][-1]
        wt = [m for m, e in enumerate(after) if e[0] == 'track']
        wc = [m for m, e in enumerate(after) if e[0] == 'clock' and e[1] is not None]
        assert wt and wc and wt[0] < wc[0] < plant
        assert np.array_equal(after[wt[0]][1], world) and after[plant][1] == j + 1                # the plant meets the world at j + 1
        cells.append(after[wc[0]][1])
    assert all(c is cells[0] for c in cells)
    # before the scores: the world again, clocked by the loop's cell; at the end nothing is left
    rest = after[plant + 1:] + rest                                                               # (behind the last plant test)
    assert [e[0] for e in rest][:2] == ['track', 'clock'] and rest[2][0] == 'eval_nodes'
    assert np.array_equal(rest[0][1], world) and rest[1][1] is cells[0]
    assert main.track is None and main.idx is None and main.clock is None and main.scene_calls[-1] is None
    # the abort event of step N - 1: the forecast of rows 1 and 3 over the backup's horizon, no clock
    bt = [e for e in back.events if e[0] == 'track' and e[1] is not None]
    assert len(bt) == 1 and np.array_equal(bt[0][1], forecast_statement(world[[1, 3]], N - 1, pars[0].back_hor, mode))
    assert [e for e in back.events if e[0] == 'solve'] == [('solve', None)]
    assert back.track is None and back.idx is None and back.clock is None
    assert res['x_viable'].shape[0] == 2
    # all columns alike: the run without a forecast, bit for bit
    for key in ('x', 'u', 'scenes'):
        assert np.array_equal(res[key], ref[key], equal_nan=True), key
    for key in ('conv_idx', 'collisions_idx', 'viable_idx', 'unconv_idx'):
        assert res[key] == ref[key], key
    for key, val in res['score'].items():
        assert np.array_equal(val, ref['score'][key], equal_nan=True), key
    # forecast=None issues exactly the calls of a run without the argument
    ref2, sv2 = run(forecast=None)
    for name in ('htwa', 'backup'):
        assert _same_events(sv2[name].events, sv_ref[name].events), name
        assert not _same_events(sv[name].events, sv_ref[name].events), name


def test_run_mpc_forecast_value_errors():
    pars, base, geoms = _loop_setup()
    B, N = 2, LOOP_N
    x0 = sample_instances(base, B, seed=5, vel_scale=0.1)
    xg, ug = np.repeat(x0[:, None, :], N + 1, axis=1), np.zeros((B, N, 6))
    mk, mkb = tc.oracle_factories(pars[0], N, pars, geoms)
    kw = dict(make_controller=mk, make_backup=mkb, n_steps=2)
    with pytest.raises(ValueError, match='forecast: needs a scene track .* no scenes were given'):
        cl.run_mpc(pars[0], 'htwa', xg, ug, forecast='cv', **kw)
    with pytest.raises(ValueError, match='forecast: needs a scene track .* standing scenes'):
        cl.run_mpc(pars[0], 'htwa', xg, ug, scenes=geoms[[0, 1]], forecast='cv', **kw)
    with pytest.raises(ValueError, match="forecast: 'linear'"):
        cl.run_mpc(pars[0], 'htwa', xg, ug, scenes=np.repeat(geoms[[0, 1]][:, None], 3, axis=1), forecast='linear', **kw)
    assert cl.result_file(pars[0], 'z1', 'htwa', 6, True, 0.0, 0.0, 0, 0, forecast='cv').endswith('_fccv_mpc.pkl')
    assert cl.result_file(pars[0], 'z1', 'htwa', 6, True, 0.0, 0.0, 0, 0) == cl.result_file(pars[0], 'z1', 'htwa', 6, True, 0.0, 0.0, 0, 0,
                                                                                            forecast=None)


# ---- 5. the entry script --------------------------------------------------------------------------------------------------------------
def _script(name):
    spec = importlib.util.spec_from_file_location('smpc_forecast_script_' + name, os.path.join(ROOT, 'scripts', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_mpc_script_takes_scene_forecast_and_scene_accel(monkeypatch, tmp_path):
    seen, saved, names = {}, {}, []
    N, n = 10, 4
    guess = {'xg': np.zeros((n, N + 1, 12)), 'ug': np.zeros((n, N, 6))}
    gfile = tmp_path / 'guess.pkl'
    pickle.dump(guess, open(gfile, 'wb'))
    monkeypatch.setattr(cl, 'guess_file', lambda *a, **k: str(gfile))
    real_result_file = cl.result_file

    def result_file(*a, **k):
        names.append((real_result_file(*a, **k), dict(k)))
        return 'result.pkl'
    monkeypatch.setattr(cl, 'result_file', result_file)
    monkeypatch.setattr(cl, 'save_pickle', lambda path, obj: saved.__setitem__(os.path.basename(str(path)), obj))

    def fake_run(params, name, x_guess, u_guess, scenes=None, timing=None, **kw):
        seen['scenes'], seen['kw'], seen['n_steps'] = scenes, kw, int(params.n_steps)
        timing['ms_per_step'] = 0.0
        return {'conv_idx': [], 'collisions_idx': [], 'viable_idx': [], 'scenes': scenes}
    monkeypatch.setattr(cl, 'run_mpc', fake_run)
    base = ['-c', 'naive', '--horizon', str(N), '--scene-velocity', '0.3', '--scene-seed', '4']
    mpc = _script('mpc')
    assert mpc.main(base) == 0
    assert 'forecast' not in seen['kw'] and 'forecast' not in names[-1][1]              # without the flags: the calls and names of before
    plain_name = names[-1][0]
    prob = C.OcpProblem(make_problem('naive', N=N)[0], 'naive')
    T = seen['n_steps'] + 1 + N
    assert np.array_equal(seen['scenes'], moving_scenes(prob, n, T, 0.3, seed=4))
    assert mpc.main(base + ['--scene-forecast', 'cv', '--scene-accel', '1.5']) == 0
    assert seen['kw']['forecast'] == 'cv'
    assert np.array_equal(seen['scenes'], turning_scenes(prob, n, T, 0.3, 1.5, seed=4))
    assert names[-1][0] == plain_name.replace('_mpc.pkl', '_fccv_mpc.pkl')
    assert mpc.main(base + ['--scene-forecast', 'hold']) == 0
    assert seen['kw']['forecast'] == 'hold' and np.array_equal(seen['scenes'], moving_scenes(prob, n, T, 0.3, seed=4))
    with pytest.raises(SystemExit, match='expected hold, cv or true'):
        mpc.main(base + ['--scene-forecast', 'linear'])
    for flag, val in (('--scene-forecast', 'cv'), ('--scene-accel', '1.0')):
        with pytest.raises(SystemExit, match=f'{flag} needs --scene-velocity'):
            mpc.main(['-c', 'naive', '--horizon', str(N), flag, val])
