"""Row bounds per instance and node (smpc_set_instance_row_bounds) without a GPU: the numpy definition of
inflation, what run_mpc(row_margin=...) hands to its solvers and when -- around a recording double on the CPU oracle --, the ABI and
the entry script's flags."""
import ctypes
import importlib.util
import os
import pickle
import re

import numpy as np
import pytest

import row_bounds_cases as rb
import scene_cases as sc
import track_cases as tc
from conftest import ROOT, make_problem, sample_instances
from safe_mpc_amd import closed_loop as cl
from safe_mpc_amd import controller as C
from safe_mpc_amd.problem import INF, ROW_COORD, inflated_row_bounds, scenes_from_problems


def _ulps(a, b):
    """|a - b| in units of the last place of b"""
    return np.abs(a - b) / np.spacing(np.abs(b))


# ---- 1. the definition ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('system', ['z1', 'fr7'])
def test_inflated_row_bounds_shapes_rows_and_the_zero_rule(system):
    """the three margin shapes give the same table where they say the same; squared-distance rows get (sqrt(lb) + d)^2, plane rows
    lb + d and ub - d on the sides that are present, absent sides and rows without a world-fixed element keep the descriptor's
    doubles; d == 0.0 returns them bit for bit"""
    N, B = 4, 3
    par, prob, net = rb.problem(system, N)
    nr = len(prob.rows)
    d1 = rb.growing_margin(N)
    lo, hi = inflated_row_bounds(prob, B, d1)
    assert lo.shape == hi.shape == (B, N + 1, nr) and lo.dtype == hi.dtype == np.float64
    for other in (np.broadcast_to(d1, (B, N + 1)), np.broadcast_to(d1[None, :, None], (B, N + 1, nr))):
        lo2, hi2 = inflated_row_bounds(prob, B, other)
        assert np.array_equal(lo, lo2) and np.array_equal(hi, hi2)
    kinds = set()
    for i, (r, name) in enumerate(zip(prob.rows, prob.row_obstacle)):
        if name is None:
            assert np.all(lo[:, :, i] == r.lb) and np.all(hi[:, :, i] == r.ub)
            continue
        kinds.add(r.kind == ROW_COORD)
        if r.kind == ROW_COORD:
            assert abs(r.lb) < INF and abs(r.ub) < INF                      # (row_bounds_cases gives the floor a ceiling)
            assert np.array_equal(lo[:, :, i], np.broadcast_to(r.lb + d1, (B, N + 1)))
            assert np.array_equal(hi[:, :, i], np.broadcast_to(r.ub - d1, (B, N + 1)))
        else:
            assert np.array_equal(lo[:, :, i], np.broadcast_to((np.sqrt(r.lb) + d1) ** 2, (B, N + 1)))
            assert abs(r.ub) >= INF and np.all(hi[:, :, i] == r.ub)         # the absent side stays the descriptor's double
    assert kinds == ({False} if system == 'z1' else {False, True})
    assert np.all(lo[:, 1:] >= lo[:, :-1]) and np.all(lo[:, -1] > lo[:, 0])                              # more room further out
    # a margin per instance and per row: only what is named moves
    d3 = np.zeros((B, N + 1, nr))
    d3[1, 2, nr - 1] = 0.02
    lo3, hi3 = inflated_row_bounds(prob, B, d3)
    lo0, hi0 = rb.descriptor_table(prob, B)
    moved = (lo3 != lo0) | (hi3 != hi0)
    assert moved[1, 2, nr - 1] and moved.sum() == 1
    # d == 0: the descriptor's doubles, bit for bit
    z_lo, z_hi = inflated_row_bounds(prob, B, np.zeros(N + 1))
    assert z_lo.tobytes() == lo0.tobytes() and z_hi.tobytes() == hi0.tobytes()
    d2 = np.zeros((B, N + 1))
    d2[:, 1:] = 0.01
    lo2, hi2 = inflated_row_bounds(prob, B, d2)
    assert lo2[:, 0].tobytes() == lo0[:, 0].tobytes() and hi2[:, 0].tobytes() == hi0[:, 0].tobytes()
    assert np.all(lo2[:, 1:] > lo0[:, 1:])


def test_inflated_row_bounds_value_errors():
    N, B = 4, 2
    par, prob, net = rb.problem('fr7', N)
    nr = len(prob.rows)
    for bad in (np.zeros(N), np.zeros((B + 1, N + 1)), np.zeros((B, N + 1, nr + 1)), np.zeros((1, 1, 1, 1)), 0.01):
        with pytest.raises(ValueError, match='margin of shape'):
            inflated_row_bounds(prob, B, bad)
    for bad in (-1e-9, np.nan, np.inf):
        d = np.zeros(N + 1)
        d[2] = bad
        with pytest.raises(ValueError, match='finite and not negative'):
            inflated_row_bounds(prob, B, d)
    # a plane row whose sides would cross: the error names the row
    i = next(k for k, r in enumerate(prob.rows) if r.kind == ROW_COORD)
    r = prob.rows[i]
    d = np.zeros((B, N + 1))
    d[1, 3] = 0.5 * (r.ub - r.lb) + 1e-3
    with pytest.raises(ValueError, match=rf'row {i} \({re.escape(prob.row_names[i])}\).*instance 1, node 3.*cross'):
        inflated_row_bounds(prob, B, d)
    d[1, 3] = 0.25 * (r.ub - r.lb)
    inflated_row_bounds(prob, B, d)


@pytest.mark.parametrize('system', ['z1', 'fr7'])
@pytest.mark.parametrize('c', [0.003, rb.MARGIN, 0.05])
def test_uniform_margin_2c_reproduces_collision_margin_c(system, c):
    """Against the problem built with collision_margin = c: the squared-distance bounds within 4 ulp, the plane bounds within 1 ulp.
    Derived: the problem forms (R + 2c)^2 -- one addition, one square --, the inflation (sqrt(R^2) + 2c)^2 -- the square root of a
    square of a double, which gives back |R| up to 1/2 ulp, then the same addition and square, each rounding once and the square
    doubling what reached it: at most 2 (1/2 + 1/2) + 1/2 + what the reference itself rounded, under 4 ulp.  A plane bound is
    (b + r) + 2c against b + r + 2c, the same two additions: 1 ulp covers a different association."""
    N, B = 4, 2
    par0, prob0, _ = rb.problem(system, N)
    parc, probc, _ = rb.problem(system, N, margin=c)
    lo, hi = inflated_row_bounds(prob0, B, np.full(N + 1, 2.0 * c))
    worst_sq, worst_pl = 0.0, 0.0
    for i, (r, name) in enumerate(zip(prob0.rows, prob0.row_obstacle)):
        if name is None:
            continue
        if r.kind == ROW_COORD:
            worst_pl = max(worst_pl, _ulps(lo[:, :, i], probc.row_lb[i]).max(), _ulps(hi[:, :, i], probc.row_ub[i]).max())
        else:
            worst_sq = max(worst_sq, _ulps(lo[:, :, i], probc.row_lb[i]).max())
            assert np.all(hi[:, :, i] == probc.row_ub[i])
    print(f'{system}, c = {c}: worst squared-distance bound {worst_sq:.2f} ulp, worst plane bound {worst_pl:.2f} ulp')
    assert worst_sq <= 4.0 and worst_pl <= 1.0
    assert np.any(probc.row_lb != prob0.row_lb)                 # (the margin does move the rows)


# ---- 2. the ABI -----------------------------------------------------------------------------------------------------------------------
def test_the_symbol_is_declared_exported_and_prototyped():
    from safe_mpc_amd import _lib, solver
    hdr = open(os.path.join(ROOT, 'include', 'smpc.h')).read()
    declared = set(re.findall(r'^(?:int|void|const char\*|void\*) (smpc_\w+)\(', hdr, re.M))
    L = ctypes.CDLL(_lib.LIB_PATH)
    name = 'smpc_set_instance_row_bounds'
    assert name in declared and name in _lib.SYMBOLS and hasattr(L, name)
    vp = ctypes.c_void_p
    assert _lib.lib().smpc_set_instance_row_bounds.argtypes == [vp, ctypes.c_int, vp, vp, ctypes.c_int]
    assert callable(solver.BatchedOcpSolver.set_instance_row_bounds)
    L.smpc_abi_version.restype = ctypes.c_int
    assert L.smpc_abi_version() == 5             # nothing existing changed


# ---- 3. the closed loop on the host path ----------------------------------------------------------------------------------------------
LOOP_N = 6


class Recorder(tc.TrackOracleSolver):
    """TrackOracleSolver that writes down, in order, the tables and the solves it is handed.  The oracle behind it knows nothing of
    a table: what is tested here is what the loop sets, on which handle, and when."""

    def __init__(self, *a):
        super().__init__(*a)
        self.events = []
        self.row_bounds = None

    def set_instance_row_bounds(self, lo=None, hi=None):
        self.events.append(('row_bounds', None if lo is None else np.array(lo), None if hi is None else np.array(hi)))
        self.row_bounds = None if lo is None else (np.array(lo), np.array(hi))

    def set_instance_scene(self, geom=None):
        self.events.append(('scene', None if geom is None else np.array(geom)))
        super().set_instance_scene(geom)

    def solve(self, x0, *a, **kw):
        self.events.append(('solve', np.asarray(x0).shape[0], None if self.row_bounds is None else self.row_bounds[0].shape))
        return super().solve(x0, *a, **kw)

    def check_trajectory(self, x, **kw):
        self.events.append(('check_trajectory', np.asarray(x).shape[1]))
        return super().check_trajectory(x, **kw)


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
            if isinstance(va, np.ndarray) or isinstance(vb, np.ndarray):
                if not (isinstance(va, np.ndarray) and isinstance(vb, np.ndarray) and np.array_equal(va, vb)):
                    return False
            elif va != vb:
                return False
    return True


@pytest.mark.parametrize('with_scenes', [False, True])
def test_run_mpc_row_margin_on_the_host_path(with_scenes):
    """'htwa', 5 instances, 7 steps around the recording double; scripted failures make instances 1 and 3 abort at step N - 1.  The
    controller's handle gets inflated_row_bounds(problem, B, a + b k) ONCE, before its first solve, and every solve of the loop
    finds it set; the backup handle gets rows 1 and 3 of the table over ITS horizon right before its one compact solve; both end
    without a table.  With and without scenes.  row_margin=None makes the calls of a run without the argument, one for one."""
    N, B, steps = LOOP_N, 5, 7
    a, g = 0.004, 0.003
    pars, base, geoms = _loop_setup()
    scenes = geoms[np.array([0, 1, 0, 1, 1])] if with_scenes else None
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
        return cl.run_mpc(pars[0], 'htwa', xg, ug, make_controller=mk_scripted, make_backup=mkb, n_steps=steps, scenes=scenes,
                          **kw), solvers
    res, sv = run(row_margin=(a, g))
    ref, sv_ref = run()
    assert res['row_margin'] == (a, g) and 'row_margin' not in ref
    main, back = sv['htwa'], sv['backup']
    Nb = pars[0].back_hor
    # the controller's handle: one table, ahead of every solve; one clearing call, behind the last
    sets = [k for k, e in enumerate(main.events) if e[0] == 'row_bounds']
    solves = [k for k, e in enumerate(main.events) if e[0] == 'solve']
    assert len(sets) == 2 and len(solves) == steps and sets[0] < solves[0] and sets[1] > solves[-1]
    lo, hi = inflated_row_bounds(base, B, a + g * np.arange(N + 1))
    assert np.array_equal(main.events[sets[0]][1], lo) and np.array_equal(main.events[sets[0]][2], hi)
    assert main.events[sets[1]][1] is None and main.row_bounds is None
    assert all(main.events[k][1:] == (B, (B, N + 1, 6)) for k in solves)
    # the backup handle: the aborting rows over its own horizon, right before its one compact solve, then cleared
    bprob = C.OcpProblem(pars[0], 'backup', 'zero', N=Nb)
    blo, bhi = inflated_row_bounds(bprob, B, a + g * np.arange(Nb + 1))
    bev = [e for e in back.events if e[0] in ('row_bounds', 'solve')]
    assert [e[0] for e in bev] == ['row_bounds', 'solve', 'row_bounds']
    assert np.array_equal(bev[0][1], blo[[1, 3]]) and np.array_equal(bev[0][2], bhi[[1, 3]])
    assert bev[1][1:] == (2, (2, Nb + 1, 6)) and bev[2][1] is None and back.row_bounds is None
    assert res['x_viable'].shape[0] == 2
    # the double ignores the table: the logs are the reference run's
    for key in ('x', 'u'):
        assert np.array_equal(res[key], ref[key], equal_nan=True), key
    # row_margin=None: the calls of a run without the argument
    ref2, sv2 = run(row_margin=None)
    for name in ('htwa', 'backup'):
        assert _same_events(sv2[name].events, sv_ref[name].events), name
        assert not _same_events(sv[name].events, sv_ref[name].events), name
        assert not any(e[0] == 'row_bounds' for e in sv_ref[name].events)


def test_run_mpc_row_margin_value_errors():
    pars, base, geoms = _loop_setup()
    B, N = 2, LOOP_N
    x0 = sample_instances(base, B, seed=5, vel_scale=0.1)
    xg, ug = np.repeat(x0[:, None, :], N + 1, axis=1), np.zeros((B, N, 6))
    mk, mkb = tc.oracle_factories(pars[0], N, pars, geoms)
    kw = dict(make_controller=mk, make_backup=mkb, n_steps=2)
    with pytest.raises(ValueError, match="row_margin: the 'parallel' policy is not supported"):
        cl.run_mpc(pars[0], 'parallel', xg, ug, row_margin=(0.01, 0.0), **kw)
    with pytest.raises(ValueError, match=r'row_margin: expected \(a, b\)'):
        cl.run_mpc(pars[0], 'htwa', xg, ug, row_margin=(0.01, 0.0, 1.0), **kw)
    with pytest.raises(ValueError, match='TrackOracleSolver has no set_instance_row_bounds'):
        cl.run_mpc(pars[0], 'htwa', xg, ug, row_margin=(0.01, 0.0), **kw)
    with pytest.raises(ValueError, match='finite and not negative'):
        solvers = {}
        mk2, mkb2 = tc.oracle_factories(pars[0], N, pars, geoms, log=solvers, solver_cls=Recorder)
        cl.run_mpc(pars[0], 'htwa', xg, ug, row_margin=(0.0, -0.01), make_controller=mk2, make_backup=mkb2, n_steps=2)
    plain = cl.result_file(pars[0], 'z1', 'htwa', 6, True, 0.0, 0.0, 0, 0)
    assert cl.result_file(pars[0], 'z1', 'htwa', 6, True, 0.0, 0.0, 0, 0, row_margin=None) == plain
    assert cl.result_file(pars[0], 'z1', 'htwa', 6, True, 0.0, 0.0, 0, 0, row_margin=(0.01, 0.0)) == plain.replace('_mpc.pkl', '_rm0.01_mpc.pkl')
    assert cl.result_file(pars[0], 'z1', 'htwa', 6, True, 0.0, 0.0, 0, 0, row_margin=(0.01, 0.002)).endswith('_rm0.01_g0.002_mpc.pkl')


# ---- 4. the entry script --------------------------------------------------------------------------------------------------------------
def _script(name):
    spec = importlib.util.spec_from_file_location('smpc_row_bounds_script_' + name, os.path.join(ROOT, 'scripts', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_mpc_script_takes_row_margin(monkeypatch, tmp_path):
    seen, names = {}, []
    N, n = 10, 4
    gfile = tmp_path / 'guess.pkl'
    pickle.dump({'xg': np.zeros((n, N + 1, 12)), 'ug': np.zeros((n, N, 6))}, open(gfile, 'wb'))
    monkeypatch.setattr(cl, 'guess_file', lambda *a, **k: str(gfile))
    real_result_file = cl.result_file

    def result_file(*a, **k):
        names.append((real_result_file(*a, **k), dict(k)))
        return 'result.pkl'
    monkeypatch.setattr(cl, 'result_file', result_file)
    monkeypatch.setattr(cl, 'save_pickle', lambda path, obj: None)

    def fake_run(params, name, x_guess, u_guess, timing=None, **kw):
        seen['kw'] = kw
        timing['ms_per_step'] = 0.0
        return {'conv_idx': [], 'collisions_idx': [], 'viable_idx': []}
    monkeypatch.setattr(cl, 'run_mpc', fake_run)
    base = ['-c', 'naive', '--horizon', str(N)]
    mpc = _script('mpc')
    assert mpc.main(base) == 0
    assert 'row_margin' not in seen['kw'] and 'row_margin' not in names[-1][1]          # without the flag: the call and name of before
    plain = names[-1][0]
    assert mpc.main(base + ['--row-margin', '0.01']) == 0
    assert seen['kw']['row_margin'] == (0.01, 0.0) and names[-1][0] == plain.replace('_mpc.pkl', '_rm0.01_mpc.pkl')
    assert mpc.main(base + ['--row-margin', '0.01', '--row-margin-growth', '0.002']) == 0
    assert seen['kw']['row_margin'] == (0.01, 0.002) and names[-1][0] == plain.replace('_mpc.pkl', '_rm0.01_g0.002_mpc.pkl')
    with pytest.raises(SystemExit, match='--row-margin-growth needs --row-margin'):
        mpc.main(base + ['--row-margin-growth', '0.002'])
    with pytest.raises(SystemExit, match="'parallel' policy is not supported"):
        mpc.main(['-c', 'parallel', '--horizon', str(N), '--row-margin', '0.01'])
