"""Forecasts from noisy observations on the engine (smpc_set_instance_observed_track, smpc_forecast_scene_fit, k_scene_fit; DESIGN.md
section 9o).  The slots are read back through the engine's test hook smpc_debug_scene_slots (forecast_cases.read_slots).

1. the kernel equals problem.fit_forecast_statement bit for bit -- windows {1, 2, 3, 7, 32}, N in {1, 4}, T in {1, 2, N + 1, N + 4,
   40}, B in {1, 5, 23}, both robots, the clock family and the clocks that fill a window, host- and device-pointer tables, twice,
   every instance alone, with and without an observed track; and the fp32 context rows.  The worlds have full mantissas in all
   eight slots, so a product that is fused into its sum shows in the last bit: this is the proof of the rounding.
2. window 2 is smpc_forecast_scene(CV) on the device, bit for bit
3. who reads what: HOLD, CV and the fit read what was observed, TRUE and smpc_loop_post the world
4. the slot is a table like any other: after the fit, eval_nodes, the stage records of both builders and the solve in both QP forms
   are those after set_instance_scene_track(fit_forecast_statement(..)) with no clock
5. every refusal by name, and that it changed nothing; the state machine of section 9n with the fit in smpc_forecast_scene's place
6. a captured [forecast_scene_fit; solve] follows the rewritten clock cell; growth under capture is refused for each buffer
7. run_mpc(on_device=True, forecast='fit', observed=...) against the host loop"""
import warnings

import numpy as np
import pytest

import forecast_cases as fc
import forecast_fit_cases as ff
from conftest import constant_guess, make_problem, sample_instances
from safe_mpc_amd.problem import fit_forecast_statement, forecast_statement, observe_tracks, scene_context, turning_scenes
from test_forecast_gpu import CTX_MEAN, CTX_STD, SELECT, _calls, _dev, _same, _solver

pytestmark = pytest.mark.gpu


def _fit(s, window, select=None):
    s.forecast_scene_fit(window, select)
    return fc.read_slots(s)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


# ---- 1. the kernel equals the statement ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('system,N', [('z1', 4), ('z1', 1), ('fr7', 4), ('fr7', 1)])
def test_kernel_equals_statement_bit_for_bit(system, N):
    s, prob = _solver(system, N)
    nr = len(prob.rows)
    for T in (1, 2, N + 1, N + 4, 40):
        for B, on_device in ((5, False), (23, True)):
            W, O = fc.world(prob, B, T, seed=T), fc.world(prob, B, T, seed=T + 11)
            s.set_instance_world_track(_dev(W) if on_device else W)
            for observed in (False, True):
                # (the observed table through the OTHER kind of pointer than its world)
                s.set_instance_observed_track((O if on_device else _dev(O)) if observed else None)
                S = O if observed else W
                for c in ff.clocks(T):
                    keep = fc.set_clock(s, c)
                    for window in ff.WINDOWS:
                        want = fit_forecast_statement(S, c, N, window)
                        info, F, _ = _fit(s, window)
                        assert info['scene_B'] == B and info['scene_T'] == N + 1 and info['scene_fc'] == 1, (T, B, c, window, info)
                        assert F.shape == (B, N + 1, nr, 8)
                        assert np.array_equal(F, want), (T, B, observed, c, window, np.abs(F - want).max())
                        if observed == on_device:       # called twice: the same bits
                            assert np.array_equal(_bits(_fit(s, window)[1]), _bits(F)), (T, B, c, window)
                    del keep
    # every instance alone (B = 1: four lanes of a wavefront) equals its rows at B = 23, world and observed track alike
    T, B = 40, 23
    W, O = fc.world(prob, B, T, seed=T), fc.world(prob, B, T, seed=T + 11)
    keep = fc.set_clock(s, 35)
    for window in (3, 32):
        s.set_instance_world_track(W)
        s.set_instance_observed_track(O)
        F23 = _fit(s, window)[1]
        assert np.array_equal(F23, fit_forecast_statement(O, 35, N, window))
        for b in range(B):
            s.set_instance_world_track(W[b:b + 1])
            s.set_instance_observed_track(O[b:b + 1])
            info, F1, _ = _fit(s, window)
            assert info['scene_B'] == 1 and np.array_equal(_bits(F1), _bits(F23[b:b + 1])), (window, b)
    # a NaN in what was seen is carried, not trapped (device pointers are taken as they are)
    On = O.copy()
    On[2, 34, 1, 7] = np.nan
    s.set_instance_world_track(W)
    s.set_instance_observed_track(_dev(On))
    F = _fit(s, 7)[1]
    assert np.array_equal(F, fit_forecast_statement(On, 35, N, 7), equal_nan=True) and np.isnan(F).any()
    s.set_instance_world_track(None)
    s.set_scene_clock(None)


def test_context_rows_equal_the_statement_in_fp32():
    """n_ctx = 2, the pairs SELECT: ctx[b][k][i] = float32((F[b][k][row_i][slot_i] - mean_i) / std_i) from the same F"""
    N = 4
    s, prob = _solver('z1', N, ctx=True)
    for B, T, on_device in ((5, 40, False), (23, 2, True), (1, 1, False)):
        W, O = fc.world(prob, B, T, seed=3), fc.world(prob, B, T, seed=14)
        s.set_instance_world_track(_dev(W) if on_device else W)
        s.set_instance_observed_track(O if on_device else None)
        S = O if on_device else W
        for c in (None, 1, 33, -2 ** 63):
            keep = fc.set_clock(s, c)
            for window in ff.WINDOWS:
                F = fit_forecast_statement(S, c, N, window)
                want = ((scene_context(F, SELECT) - CTX_MEAN) / CTX_STD).astype(np.float32)
                info, got_F, got = _fit(s, window, SELECT)
                assert info['ctx_B'] == B and info['ctx_T'] == N + 1 and info['ctx_fc'] == 1, info
                assert np.array_equal(got_F, F) and got.shape == (B, N + 1, 2)
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (B, T, c, window)
            del keep
    s.set_instance_world_track(None)


# ---- 2. window 2 is CV on the device ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('system', ['z1', 'fr7'])
def test_window_2_is_the_cv_kernel_and_window_1_the_hold_kernel(system):
    N = 4
    s, prob = _solver(system, N)
    for T in (1, 2, N + 1, N + 4):
        W = fc.world(prob, 23, T, seed=T)
        s.set_instance_world_track(_dev(W))
        for c in fc.clocks(T):
            keep = fc.set_clock(s, c)
            for window, mode in ((2, 'cv'), (1, 'hold')):
                s.forecast_scene(mode)
                old = fc.read_slots(s)[1]
                assert np.array_equal(_bits(_fit(s, window)[1]), _bits(old)), (T, c, window)
            del keep
    s.set_instance_world_track(None)
    s.set_scene_clock(None)


# ---- 3. who reads what --------------------------------------------------------------------------------------------------------------------
def test_hold_cv_and_fit_read_what_was_observed_true_reads_the_world():
    N, B, T = 4, 5, 12
    s, prob = _solver('z1', N)
    W, O = fc.world(prob, B, T, seed=1), fc.world(prob, B, T, seed=2)
    s.set_instance_world_track(W)
    for observed in (None, O, None):
        s.set_instance_observed_track(observed)
        for c in (None, 3, T + 5):
            keep = fc.set_clock(s, c)
            for kind in ('hold', 'cv', 'true', 4):
                want = ff.seen_statement(W, observed, c, N, kind)
                s.forecast_scene(kind) if isinstance(kind, str) else s.forecast_scene_fit(kind)
                assert np.array_equal(fc.read_slots(s)[1], want), (observed is not None, c, kind)
                if observed is not None and kind != 'true' and c == 3:
                    assert not np.array_equal(want, ff.seen_statement(W, None, c, N, kind))
            del keep
    s.set_instance_world_track(None)
    s.set_scene_clock(None)


def _loop_arm(par, x0, world, observed, t, window=4):
    """one step of the device loop at clock t with forecasts fitted to ``observed``: (fails, u, collided, alive)"""
    import torch
    from safe_mpc_amd import closed_loop as cl
    from safe_mpc_amd import controller as C
    B, N = x0.shape[0], int(par.N)
    ctrl, backup = C.get_controller('htwa', par, B, device_state=True), C.SafeBackupController(par, B, device_state=True)
    sv = ctrl.ocp_solver
    xg, ug = np.repeat(x0[:, None, :], N + 1, axis=1), np.zeros((B, N, 6))
    with torch.cuda.stream(torch.cuda.ExternalStream(sv.L.smpc_stream(sv.h), device=torch.device('cuda', sv.device))):
        grp = cl._DeviceGroup(par, xg, ug, 0.0, 0.0, ctrl, backup, 6, 0, False, use_graphs=False, scenes=world, forecast='fit',
                              forecast_window=window, observed=observed)
        grp._jt.fill_(t)
        grp.part_a()
        fails, u = ctrl.fails.cpu().numpy().copy(), grp.u.cpu().numpy().copy()
        grp.part_b()
        sv.sync()
        out = fails, u, grp.collided.cpu().numpy().copy(), grp.alive.cpu().numpy().copy()
        grp.results()           # (leaves both handles without world, observed track, forecast and clock)
        info = fc.read_slots(sv)[0]
        assert info['scene_B'] == 0 and info['ctx_B'] == 0
    return out


def test_the_plant_meets_the_world_and_the_controller_what_it_observed():
    """Z1, 'htwa', three instances at rest, clock t = 2, a fit over 4 columns (3 have been shown).  Row 0's fixed capsule, collapsed to
    a point on the instance's end-effector point, is the obstacle "inside the robot"; elsewhere the obstacles drift slowly.
    (a) Far away in the observed track, inside the robot in the world: the controller's step is bit for bit the step of the run that
        observes the drifting world exactly -- the x_temp test of smpc_policy_step passes -- and smpc_loop_post reports the collision.
    (b) The other way round: the x_temp test fails, and the plant, which lives in the drifting world, is free."""
    from safe_mpc_amd.solver import BatchedOcpSolver
    N, B, T, t = 8, 3, 8, 2
    par, prob, net = make_problem('htwa', N=N)
    par.back_hor = 8
    x0 = sample_instances(prob, B, seed=5, vel_scale=0.0)
    xg, ug, p = constant_guess(prob, x0)
    s = BatchedOcpSolver(prob, net)
    ee = np.array(s.eval_nodes(xg, ug, p)['ee'])[:, 0, :3]
    s.close()
    calm = np.repeat(np.repeat(prob.row_geometry()[None, None], B, axis=0), T, axis=1)
    calm[..., 0] += 0.001 * np.arange(T)[None, :, None]           # every obstacle drifts along x
    hit = calm.copy()
    hit[:, :, 0, 0:3] = hit[:, :, 0, 3:6] = ee[:, None]
    calm, hit = np.ascontiguousarray(calm), np.ascontiguousarray(hit)
    f0, u0, coll0, alive0 = _loop_arm(par, x0, calm, None, t)
    assert (f0 == 0).all() and not coll0.any() and alive0.all()     # the premise: free in the drifting world
    # (a)
    f1, u1, coll1, alive1 = _loop_arm(par, x0, hit, calm, t)
    print('(a) fails', f0, f1, 'collided', coll0, coll1)
    assert np.array_equal(f0, f1) and np.array_equal(u0, u1)       # the controller has seen the calm table only
    assert coll1.all() and not alive1.any()                         # the plant meets the world
    # (b)
    f2, u2, coll2, alive2 = _loop_arm(par, x0, calm, hit, t)
    print('(b) fails', f2, 'collided', coll2)
    assert (f2 > 0).all()                                           # the controller plans in what it observed ...
    assert not coll2.any() and alive2.all()                         # ... and the plant lives in the world


# ---- 4. the slot is a table like any other -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('system,N,ctx', [('z1', 4, False), ('z1', 4, True), ('fr7', 4, False), ('z1', 1, False)])
def test_the_fit_in_the_slot_is_the_statement_set_as_a_track(system, N, ctx):
    B, T = 5, 12
    s, prob = _solver(system, N, ctx)
    select = SELECT if ctx else None
    x0 = sample_instances(prob, B, seed=1, vel_scale=0.5)
    xg, ug, p = constant_guess(prob, x0)
    rng = np.random.default_rng(0)
    xg[:, 1:] += 0.05 * rng.standard_normal(xg[:, 1:].shape)
    ug += rng.uniform(-5, 5, ug.shape)
    inputs = (x0, xg, ug, p)
    W, O = fc.world(prob, B, T), fc.world(prob, B, T, seed=5)
    refs = []
    for c, window, observed in ((None, 3, False), (5, 3, True), (T - 1, 7, True), (T + 5, 32, False), (2 ** 63 - 1, 2, True)):
        F = fit_forecast_statement(O if observed else W, c, N, window)
        # the statement as a track of the caller's, no clock
        s.set_instance_world_track(None)
        s.set_scene_clock(None)
        if ctx:
            s.set_instance_context_track(scene_context(F, SELECT))
        s.set_instance_scene_track(F)
        ref = _calls(s, N, inputs)
        refs.append(ref)
        # the engine's fit at clock c
        s.set_instance_world_track(_dev(W))
        s.set_instance_observed_track(O if observed else None)
        keep = fc.set_clock(s, c)
        s.forecast_scene_fit(window, select)
        assert _same(_calls(s, N, inputs), ref) == [], (c, window, observed)
        del keep
    assert all(_same(refs[0], r) for r in refs[1:])         # (the cases are different problems)
    s.set_instance_world_track(None)
    s.set_scene_clock(None)


# ---- 5. refusals and the state machine ----------------------------------------------------------------------------------------------------
def test_every_refusal_by_name_changes_nothing():
    from safe_mpc_amd._lib import EngineError
    N, B, T = 4, 5, 8
    s, prob = _solver('z1', N, ctx=True)
    plain, _ = _solver('z1', N)
    nr = len(prob.rows)
    W, O = fc.world(prob, B, T), fc.world(prob, B, T, seed=4)
    with pytest.raises(EngineError, match=r'engine error -4: smpc_forecast_scene_fit: no world is set'):
        s.forecast_scene_fit(4)
    s.set_instance_observed_track(O)                                # (an observed track alone is no world)
    with pytest.raises(EngineError, match=r'engine error -4: smpc_forecast_scene_fit: no world is set'):
        s.forecast_scene_fit(4, B=B)
    s.set_instance_world_track(W)

    def refused(match, call, code=-1):
        before = fc.read_slots(s)
        with pytest.raises(EngineError, match=rf'engine error {code}: {match}'):
            call()
        after = fc.read_slots(s)
        assert after[0] == before[0]
        for a, b in zip(after[1:], before[1:]):
            assert (a is None and b is None) or np.array_equal(a, b, equal_nan=True)

    def family():
        refused(r'smpc_forecast_scene_fit: batch size 4, .* 5 instances', lambda: s.forecast_scene_fit(4, B=4))
        for window in (0, 33, -1):
            refused(rf'smpc_forecast_scene_fit: window {window}\b', lambda: s.forecast_scene_fit(window))
        refused(r'smpc_forecast_scene_fit: n_sel=1, but the network has n_ctx=2', lambda: s.forecast_scene_fit(4, [(0, 0)]))
        for pair in ((nr, 0), (0, 8), (-1, 0)):
            refused(r'smpc_forecast_scene_fit: select\[1\] = .* outside 6 rows x 8 slots', lambda: s.forecast_scene_fit(4, [(0, 0), pair]))
        refused(r'smpc_forecast_scene_fit: n_sel=2 with select == NULL', lambda: s._chk(s.L.smpc_forecast_scene_fit(s.h, B, 4, 2, None)))
        refused(r'smpc_forecast_scene_fit: n_sel=-1', lambda: s._chk(s.L.smpc_forecast_scene_fit(s.h, B, 4, -1, None)))
        # an observed track of another shape than the world's, in either coordinate: every forecast call names both
        for shape, bad in (((4, T), O[:4]), ((B, T - 1), O[:, 1:])):
            s.set_instance_observed_track(np.ascontiguousarray(bad))
            msg = (rf'the instance observed track was set for {shape[0]} instances and {shape[1]} columns, but the instance world track '
                   rf'for {B} instances and {T} columns')
            refused('smpc_forecast_scene_fit: ' + msg, lambda: s.forecast_scene_fit(4))
            refused('smpc_forecast_scene: ' + msg, lambda: s.forecast_scene('cv'))
            s.set_instance_observed_track(O)
    family()                                                        # with empty slots: refused calls have set nothing ...
    assert fc.read_slots(s)[0]['scene_B'] == 0
    s.forecast_scene_fit(7, SELECT)
    assert fc.read_slots(s)[0] == dict(scene_B=B, scene_T=N + 1, scene_fc=1, ctx_B=B, ctx_T=N + 1, ctx_fc=1)
    family()                                                        # ... and with a forecast in them: it stays in force
    assert np.array_equal(fc.read_slots(s)[1], fit_forecast_statement(O, None, N, 7))
    plain.set_instance_world_track(W)
    with pytest.raises(EngineError, match=r'engine error -1: smpc_forecast_scene_fit: n_sel=2, but the network has no context columns'):
        plain.forecast_scene_fit(4, SELECT)
    with pytest.raises(EngineError, match=r'engine error -1: smpc_set_instance_observed_track: T=0'):
        s._chk(s.L.smpc_set_instance_observed_track(s.h, B, 0, O.ctypes.data, 0))
    bad = O.copy()
    bad[3, 2, 1, 4] = np.nan
    with pytest.raises(EngineError, match=r'engine error -1: scene track of instance 3, column 2, row 1'):
        s.set_instance_observed_track(bad)
    with pytest.raises(ValueError, match='set_instance_observed_track: expected'):
        s.set_instance_observed_track(O[:, 0])
    # the old entry point keeps its refusals (mode 3 is not the fit)
    refused(r'smpc_forecast_scene: mode 3', lambda: s.forecast_scene(3))
    refused(r'smpc_forecast_scene: mode -1', lambda: s.forecast_scene(-1))
    for sv in (s, plain):
        sv.set_instance_world_track(None)


def test_state_machine_with_the_fit_in_place_of_forecast_scene():
    from safe_mpc_amd._lib import EngineError
    N, B, T = 4, 5, 8
    s, prob = _solver('z1', N, ctx=True)
    x0 = sample_instances(prob, B, seed=1, vel_scale=0.5)
    xg, ug, p = constant_guess(prob, x0)
    W, O = fc.world(prob, B, T), fc.world(prob, B, T, seed=4)
    ev = lambda n=B: np.array(s.eval_nodes(xg[:n], ug[:n], p[:n])['row_val'])
    shared = ev()
    s.set_instance_world_track(W)
    s.set_instance_observed_track(O)
    assert np.array_equal(ev(), shared)                             # world and observed track alone change nothing the controller sees
    # forecast -> scene track -> clocked again
    keep = fc.set_clock(s, 3)
    s.forecast_scene_fit(4, SELECT)
    info, F, ctx = fc.read_slots(s)
    assert info == dict(scene_B=B, scene_T=N + 1, scene_fc=1, ctx_B=B, ctx_T=N + 1, ctx_fc=1)
    assert np.array_equal(F, fit_forecast_statement(O, 3, N, 4))
    fitted = ev()
    assert not np.array_equal(fitted, shared)
    s.set_instance_context_track(scene_context(W, SELECT))
    s.set_instance_scene_track(W)
    info = fc.read_slots(s)[0]
    assert info['scene_fc'] == 0 and info['scene_T'] == T and info['ctx_fc'] == 0 and info['ctx_T'] == T
    assert not np.array_equal(ev(), fitted)                         # (the clocked world, not the fit of what was observed)
    # a scene setter over a forecast drops the context the forecast wrote
    s.forecast_scene_fit(4, SELECT)
    s.set_instance_scene(np.ascontiguousarray(W[:, 0]))
    info = fc.read_slots(s)[0]
    assert info['scene_fc'] == 0 and info['ctx_B'] == 0
    # clearing the observed track alone: the next forecast reads the world; a forecast in the slot stays
    s.forecast_scene_fit(4, SELECT)
    s.set_instance_observed_track(None)
    assert np.array_equal(fc.read_slots(s)[1], fit_forecast_statement(O, 3, N, 4))
    s.forecast_scene_fit(4, SELECT)
    assert np.array_equal(fc.read_slots(s)[1], fit_forecast_statement(W, 3, N, 4))
    # clearing the world clears the forecast, the context it wrote -- and the observed track: a later world starts unobserved
    s.set_instance_observed_track(O)
    s.forecast_scene_fit(4, SELECT)
    s.set_instance_world_track(None)
    info = fc.read_slots(s)[0]
    assert info['scene_B'] == 0 and info['ctx_B'] == 0
    with pytest.raises(EngineError, match=r'engine error -4: smpc_forecast_scene_fit: no world is set'):
        s.forecast_scene_fit(4)
    s.set_instance_world_track(W)
    s.forecast_scene('cv')
    assert np.array_equal(fc.read_slots(s)[1], forecast_statement(W, 3, N, 'cv'))           # (the world: no observed track is left)
    s.forecast_scene_fit(4)
    assert np.array_equal(fc.read_slots(s)[1], fit_forecast_statement(W, 3, N, 4))
    s.set_instance_world_track(None)
    s.set_scene_clock(None)
    del keep
    assert np.array_equal(ev(), shared)
    # a scene of a setter's stays when the world goes
    s.set_instance_scene(np.ascontiguousarray(W[:, 0]))
    s.set_instance_world_track(W)
    s.set_instance_observed_track(O)
    s.set_instance_world_track(None)
    assert fc.read_slots(s)[0]['scene_B'] == B
    s.set_instance_scene(None)
    # smpc_set_horizon drops a fitted forecast and keeps world and observed track: the next one is laid out by the new horizon
    s.set_instance_world_track(W)
    s.set_instance_observed_track(O)
    s.forecast_scene_fit(4, SELECT)
    s.set_horizon(N)
    info = fc.read_slots(s)[0]
    assert info['scene_B'] == 0 and info['ctx_B'] == 0
    s.set_horizon(2)
    s.forecast_scene_fit(4)
    assert np.array_equal(fc.read_slots(s)[1], fit_forecast_statement(O, None, 2, 4))
    s.set_horizon(N)
    # another batch size while a fitted forecast is set: refused as for any scene; smpc_rollout_batch refuses the slot
    s.forecast_scene_fit(4)
    with pytest.raises(EngineError, match=r'batch size 4, .* 5 instances'):
        ev(n=4)
    with pytest.raises(EngineError, match=r'engine error -4: smpc_rollout_batch'):
        s.rollout(x0, xg, ug, p, 2)
    s.set_instance_world_track(None)


# ---- 6. capture ------------------------------------------------------------------------------------------------------------------------------
def test_growth_under_capture_is_refused_for_each_buffer_and_a_captured_fit_follows_the_clock():
    """capture as test_forecast_gpu.py does it: torch's capture stream, which the engine's stream joins for the call"""
    import torch
    from safe_mpc_amd._lib import EngineError
    N, B, T = 4, 5, 8
    s, prob = _solver('z1', N, ctx=True)
    x0 = sample_instances(prob, B, seed=1, vel_scale=0.5)
    xg, ug, p = constant_guess(prob, x0)
    dev_in = [_dev(a) for a in (x0, xg, ug, p)]
    W, O = fc.world(prob, B, T), fc.world(prob, B, T, seed=4)
    cell = fc.cell(1)
    torch.cuda.synchronize()
    s.set_scene_clock(cell)
    s.set_instance_world_track(_dev(W))

    def refused(what, call):
        with pytest.raises(EngineError, match=rf'engine error -4: .*{what} must grow .* while the stream is being captured'), \
                warnings.catch_warnings():
            warnings.filterwarnings('ignore', 'The CUDA Graph is empty')
            with torch.cuda.graph(torch.cuda.CUDAGraph()):
                call()
        torch.cuda.synchronize()
    # the scene buffer does not exist yet
    refused('smpc_forecast_scene_fit: the instance scene', lambda: s.forecast_scene_fit(4, SELECT))
    assert fc.read_slots(s)[0]['scene_B'] == 0
    # the scene buffer exists, the context buffer does not: the old forecast keeps serving
    s.forecast_scene_fit(4)
    before = fc.read_slots(s)
    refused('smpc_forecast_scene_fit: the instance context', lambda: s.forecast_scene_fit(7, SELECT))
    after = fc.read_slots(s)
    assert after[0] == before[0] and after[0]['ctx_B'] == 0 and np.array_equal(after[1], before[1])
    # the observed track: a first one, and a larger one over a smaller one, whose contents stay in force
    O_dev, small = _dev(O), _dev(O[:, :2])
    refused('the instance observed track', lambda: s.set_instance_observed_track(O_dev))
    s.forecast_scene_fit(4)
    assert np.array_equal(fc.read_slots(s)[1], fit_forecast_statement(W, 1, N, 4))          # (still unobserved)
    s.set_instance_world_track(_dev(W[:, :2]))
    s.set_instance_observed_track(small)
    refused('the instance observed track', lambda: s.set_instance_observed_track(O_dev))
    s.forecast_scene_fit(4)
    assert np.array_equal(fc.read_slots(s)[1], fit_forecast_statement(O[:, :2], 1, N, 4))
    s.set_instance_world_track(_dev(W))                             # (clears nothing: the observed track is re-set below)
    s.set_instance_observed_track(O_dev)
    # [forecast_scene_fit; solve] eager at clocks 1 and 5, then captured once at clock 1 and replayed after the cell was rewritten
    eager = {}
    for c in (1, 5):
        cell.fill_(c)
        s.forecast_scene_fit(4, SELECT)
        res = s.solve(*dev_in)
        s.sync()
        eager[c] = [a.cpu().numpy().copy() for a in res]
        assert np.array_equal(fc.read_slots(s)[1], fit_forecast_statement(O, c, N, 4))
    assert not np.array_equal(eager[1][1], eager[5][1])
    cell.fill_(1)
    out = tuple(torch.empty_like(a) for a in res)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        s.forecast_scene_fit(4, SELECT)
        s.solve(*dev_in, out=out)
    for c in (5, 1):
        cell.fill_(c)
        g.replay()
        torch.cuda.synchronize()
        assert all(np.array_equal(o.cpu().numpy(), w) for o, w in zip(out, eager[c])), c
        assert np.array_equal(fc.read_slots(s)[1], fit_forecast_statement(O, c, N, 4))
    s.set_instance_world_track(None)
    s.set_scene_clock(None)


# ---- 7. the closed loop ---------------------------------------------------------------------------------------------------------------------
def _loop_case(vel_scale=0.2, ghosts=(1, 3)):
    """'htwa', B = 5, N = 8, 12 steps on turning tracks seen through a sensor (sigma = 1e-3).  For the instances ``ghosts`` the sensor
    also shows a ghost: row 0's fixed capsule, collapsed to a point, on the instance's end-effector point at the start, in every
    column -- the x_temp test of their policy step fails step after step (the obstacle "inside the robot" of section 3) until the
    controller aborts, while their plant, which lives in the world, stays free."""
    from safe_mpc_amd.solver import BatchedOcpSolver
    N, B, steps = 8, 5, 12
    par, prob, net = make_problem('htwa', N=N)
    par.back_hor = 8
    x0 = sample_instances(prob, B, seed=9, vel_scale=vel_scale)
    xg, ug = np.repeat(x0[:, None, :], N + 1, axis=1), np.zeros((B, N, 6))
    world = turning_scenes(prob, B, steps + 1 + N, 0.3, 3.0, seed=2)
    observed = observe_tracks(prob, world, 1e-3, seed=1)
    s = BatchedOcpSolver(prob, net)
    ee = np.array(s.eval_nodes(xg, ug, constant_guess(prob, x0)[2])['ee'])[:, 0, :3]
    s.close()
    for b in ghosts:
        observed[b, :, 0, 0:3] = observed[b, :, 0, 3:6] = ee[b]
    return par, xg, ug, world, np.ascontiguousarray(observed), steps


def test_device_loop_with_a_fit_of_observations_equals_the_host_loop():
    """run_mpc(on_device=True, forecast='fit', forecast_window=4, observed=...) against on_device=False (the statement) on the case
    above: equal index lists and x within 1e-6 -- the shapes' kind and the tolerance of
    test_forecast_gpu.py::test_device_loop_with_a_forecast_equals_the_host_loop.  An abort event must occur (x_viable is not empty),
    so that the backup handle's path -- world rows, observed rows, a forecast over its own horizon -- has run."""
    from safe_mpc_amd import closed_loop as cl
    par, xg, ug, world, observed, steps = _loop_case()
    kw = dict(n_steps=steps, scenes=world, forecast='fit', forecast_window=4, observed=observed, score=True)
    dev = cl.run_mpc(par, 'htwa', xg, ug, on_device=True, groups=1, **kw)
    host = cl.run_mpc(par, 'htwa', xg, ug, on_device=False, **kw)
    assert dev['forecast'] == host['forecast'] == 'fit' and dev['forecast_window'] == host['forecast_window'] == 4
    assert dev['observed'] is True and host['observed'] is True
    print('abort events: x_viable', dev['x_viable'].shape, host['x_viable'].shape, 'viable_idx', dev['viable_idx'], 'collisions',
          dev['collisions_idx'], 'unconv', dev['unconv_idx'])
    assert dev['x_viable'].shape[0] > 0 and dev['x_viable'].shape == host['x_viable'].shape
    for k in ('conv_idx', 'collisions_idx', 'unconv_idx'):
        assert dev[k] == host[k], k
    assert sorted(dev['viable_idx']) == sorted(host['viable_idx'])
    assert np.array_equal(np.isnan(dev['x']), np.isnan(host['x']))
    err = np.nanmax(np.abs(dev['x'] - host['x']))
    print(f'forecast fit (window 4, observed): device loop against host loop, max |x| error {err:.3e}')
    assert err < 1e-6
    assert np.allclose(dev['score']['coll_margin'], host['score']['coll_margin'], atol=1e-6)        # both scored in the true world
    assert np.array_equal(dev['scenes'], world)
