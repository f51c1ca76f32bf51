"""Obstacle forecasts on the engine (smpc_set_instance_world_track, smpc_forecast_scene, k_scene_forecast).

How the slot is read back: through the engine's test hook smpc_debug_scene_slots (forecast_cases.read_slots), which copies the scene
and context slots to the host -- so test 1 compares the table itself, and tests 2 and 3 show that the solve-path kernels read it
from time 0.

1. the kernel equals problem.forecast_statement bit for bit: every mode and clock of the family, N in {1, 4}, T in {1, 2, N + 1,
   N + 4}, B in {1, 5, 23} (6, 30 and 138 records at six rows), both robots, host- and device-pointer worlds, twice, every instance
   alone; and the fp32 context rows of a net with two context inputs
2. 'true' at clock c is the clocked track at clock c: smpc_eval_nodes, the stage records of both builders, smpc_solve_batch in both
   QP forms, bit for bit
3. 'hold' at clock c is the standing scene of column col(c), the same calls
4. the plant meets the world: smpc_loop_post tests the plant's next state in column t + 1 of the WORLD, the x_temp test of
   smpc_policy_step in the forecast
5. run_mpc(on_device=True, forecast=m) against the host loop on turning tracks; 'true' against no forecast, bit for bit
6. the state machine and the refusals"""
import ctypes
import functools
import warnings

import numpy as np
import pytest

import forecast_cases as fc
from conftest import constant_guess, make_problem, sample_instances
from safe_mpc_amd.problem import forecast_statement, scene_context, turning_scenes

pytestmark = pytest.mark.gpu

SELECT = [(0, 0), (2, 6)]           # the two context numbers of the context net: row 0's C_x, row 2's offset slot
CTX_MEAN, CTX_STD = np.array([0.3, -0.1]), np.array([0.5, 2.0])


def _dev(a):
    import torch
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device='cuda:0')


@functools.lru_cache(maxsize=None)
def _context_net(N):
    """the Z1 problem with a seeded net of two context inputs that says where they come from (ctx_select)"""
    import context_cases as cc
    from safe_mpc_amd.safe_set import SafeSetNet
    par, prob, _ = fc.problem('z1', N)
    base = cc.context_net(prob, par, n_ctx=2)
    return SafeSetNet(base.model, base.mean, base.std, base.act, CTX_MEAN, CTX_STD, SELECT)


def _solver(system, N, ctx=False):
    from safe_mpc_amd.solver import BatchedOcpSolver
    par, prob, net = fc.problem(system, N, 'htwa' if system == 'z1' else 'constraint_everywhere')
    return BatchedOcpSolver(prob, _context_net(N) if ctx else net), prob


def _forecast(s, mode, select=None):
    s.forecast_scene(mode, select)
    info, scene, ctx = fc.read_slots(s)
    return info, scene, ctx


# ---- 1. the kernel equals the statement ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('system,N', [('z1', 4), ('z1', 1), ('fr7', 4), ('fr7', 1)])
def test_kernel_equals_statement_bit_for_bit(system, N):
    s, prob = _solver(system, N)
    nr = len(prob.rows)
    for T in (1, 2, N + 1, N + 4):
        for B, on_device in ((5, False), (23, True)):
            W = fc.world(prob, B, T, seed=T)
            s.set_instance_world_track(_dev(W) if on_device else W)
            for c in fc.clocks(T):
                keep = fc.set_clock(s, c)
                for mode in fc.MODES:
                    want = forecast_statement(W, c, N, mode)
                    info, F, _ = _forecast(s, mode)
                    assert info['scene_B'] == B and info['scene_T'] == N + 1 and info['scene_fc'] == 1, (T, B, c, mode, info)
                    assert F.shape == (B, N + 1, nr, 8)
                    assert np.array_equal(F, want, equal_nan=True), (T, B, c, mode, np.abs(F - want).max())
                    _, again, _ = _forecast(s, mode)
                    assert np.array_equal(again.view(np.uint64), F.view(np.uint64)), (T, B, c, mode)     # called twice: same bits
                del keep
    # every instance alone (B = 1, one record block under a wavefront) equals its rows at B = 23
    T, B = N + 4, 23
    W = fc.world(prob, B, T, seed=T)
    keep = fc.set_clock(s, 1)
    for mode in ('cv', 'true', 'hold'):
        s.set_instance_world_track(W)
        _, F23, _ = _forecast(s, mode)
        assert np.array_equal(F23, forecast_statement(W, 1, N, mode))
        for b in range(B):
            s.set_instance_world_track(W[b:b + 1])
            info, F1, _ = _forecast(s, mode)
            assert info['scene_B'] == 1 and np.array_equal(F1.view(np.uint64), F23[b:b + 1].view(np.uint64)), (mode, b)
    # a NaN in the world is carried, not trapped (device pointers are taken as they are)
    Wn = W.copy()
    Wn[2, 1, 1, 7] = np.nan
    s.set_instance_world_track(_dev(Wn))
    for mode in fc.MODES:
        _, F, _ = _forecast(s, mode)
        assert np.array_equal(F, forecast_statement(Wn, 1, N, mode), equal_nan=True) and np.isnan(F).any(), mode
    s.set_instance_world_track(None)
    s.set_scene_clock(None)


def test_context_rows_equal_the_statement_in_fp32():
    """n_ctx = 2, the pairs SELECT: ctx[b][k][i] = float32((F[b][k][row_i][slot_i] - mean_i) / std_i) from the same F, every mode,
    host- and device-pointer worlds, under and over a wavefront of rows"""
    N = 4
    s, prob = _solver('z1', N, ctx=True)
    for B, T, on_device in ((5, N + 4, False), (23, 2, True), (1, 1, False)):
        W = fc.world(prob, B, T, seed=3)
        s.set_instance_world_track(_dev(W) if on_device else W)
        for c in (None, 1, T + 5, -2 ** 63):
            keep = fc.set_clock(s, c)
            for mode in fc.MODES:
                F = forecast_statement(W, c, N, mode)
                want = ((scene_context(F, SELECT) - CTX_MEAN) / CTX_STD).astype(np.float32)
                info, got_F, got = _forecast(s, mode, SELECT)
                assert info['ctx_B'] == B and info['ctx_T'] == N + 1 and info['ctx_fc'] == 1, info
                assert np.array_equal(got_F, F) and got.shape == (B, N + 1, 2)
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (B, T, c, mode)
            del keep
    # without pairs the context slot is left alone: a setter's context stays what it was, clocked as it was
    raw = np.ascontiguousarray(scene_context(W, SELECT))
    s.set_instance_context_track(raw)
    info, _, before = fc.read_slots(s)
    assert info['ctx_fc'] == 0 and info['ctx_T'] == 1
    info, _, after = _forecast(s, 'cv')
    assert info['ctx_fc'] == 0 and info['scene_fc'] == 1 and np.array_equal(before, after)
    s.set_instance_world_track(None)


# ---- 2. + 3. a forecast in the slot is read from time 0 ---------------------------------------------------------------------------------
def _stage_records(s, N, x0, xg, ug, p, path):
    """the stage records [B, N + 1, stride] after either builder (test_scene_track_gpu.py's hook)"""
    L = s.L
    L.smpc_debug_stage_records.argtypes = [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 4 + [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    lay = np.zeros(24, np.int32)
    B = x0.shape[0]
    arrs = [np.ascontiguousarray(a, np.float64) for a in (x0, xg, ug, p)]
    out = np.zeros(B * 64 * 2048)
    rc = L.smpc_debug_stage_records(s.h, B, *[a.ctypes.data for a in arrs], path, out.ctypes.data, lay.ctypes.data)
    assert rc == 0, L.smpc_last_error(s.h)
    stride, per = int(lay[0]), int(lay[14])
    return out[:B * per].reshape(B, per)[:, :(N + 1) * stride].copy()


def _calls(s, N, inputs):
    """what tests 2 and 3 compare: eval_nodes (every field), the stage records of both builders, the solve in both QP forms"""
    x0, xg, ug, p = inputs
    ev = s.eval_nodes(xg, ug, p)
    out = [np.array(ev[f]) for f in ev.dtype.names]
    out += [_stage_records(s, N, x0, xg, ug, p, path) for path in (1, 0)]
    for qp in ('throughput', 'latency'):
        s.set_qp_mode(qp)
        out += [np.array(a) for a in s.solve(x0, xg, ug, p)]
    return out


def _same(a, b):
    return [k for k, (u, v) in enumerate(zip(a, b)) if not np.array_equal(u, v, equal_nan=True)]


@pytest.mark.parametrize('system,N,ctx', [('z1', 4, False), ('z1', 4, True), ('fr7', 4, False), ('z1', 1, False)])
def test_true_is_the_clocked_track_and_hold_a_standing_scene(system, N, ctx):
    B, T = 5, N + 4
    s, prob = _solver(system, N, ctx)
    select = SELECT if ctx else None
    x0 = sample_instances(prob, B, seed=1, vel_scale=0.5)
    xg, ug, p = constant_guess(prob, x0)
    rng = np.random.default_rng(0)
    xg[:, 1:] += 0.05 * rng.standard_normal(xg[:, 1:].shape)
    ug += rng.uniform(-5, 5, ug.shape)
    inputs = (x0, xg, ug, p)
    W = fc.world(prob, B, T)
    differ = 0
    for c in (None, 1, T - 2, T + 5, -1, 2 ** 63 - 1):
        # today's calls: the world as a clocked scene track, and the standing scene of column col(c) -- with their contexts
        s.set_instance_world_track(None)
        keep = fc.set_clock(s, c)
        if ctx:
            s.set_instance_context_track(scene_context(W, SELECT))
        s.set_instance_scene_track(W)
        ref_true = _calls(s, N, inputs)
        col = fc.gather_true(W, c, 0)[:, 0]
        if ctx:
            s.set_instance_context(scene_context(col, SELECT))
        s.set_instance_scene(col)
        ref_hold = _calls(s, N, inputs)
        differ += bool(_same(ref_true, ref_hold))
        # the forecasts of the same clock
        s.set_instance_world_track(_dev(W))
        s.forecast_scene('true', select)
        assert _same(_calls(s, N, inputs), ref_true) == [], ('true', c)
        s.forecast_scene('hold', select)
        assert _same(_calls(s, N, inputs), ref_hold) == [], ('hold', c)
        s.forecast_scene('cv', select)
        if c in (None, -1, T + 5, 2 ** 63 - 1):     # col(c) = col(c - 1): CV holds (F + 0.0: the same numbers)
            assert _same(_calls(s, N, inputs), ref_hold) == [], ('cv', c)
        del keep
    assert differ >= 3          # (the world does move: a track and its frozen column are other problems)
    s.set_instance_world_track(None)
    s.set_scene_clock(None)


# ---- 4. the plant meets the world --------------------------------------------------------------------------------------------------------
def _loop_arm(par, x0, world, mode, t):
    """one step of the device loop at clock t with the world ``world`` and forecasts of ``mode``: (fails, u, collided, alive)"""
    import torch
    from safe_mpc_amd import closed_loop as cl
    from safe_mpc_amd import controller as C
    B, N = x0.shape[0], int(par.N)
    ctrl, backup = C.get_controller('htwa', par, B, device_state=True), C.SafeBackupController(par, B, device_state=True)
    sv = ctrl.ocp_solver
    xg, ug = np.repeat(x0[:, None, :], N + 1, axis=1), np.zeros((B, N, 6))
    with torch.cuda.stream(torch.cuda.ExternalStream(sv.L.smpc_stream(sv.h), device=torch.device('cuda', sv.device))):
        grp = cl._DeviceGroup(par, xg, ug, 0.0, 0.0, ctrl, backup, 6, 0, False, use_graphs=False, scenes=world, forecast=mode)
        grp._jt.fill_(t)
        grp.part_a()
        fails, u = ctrl.fails.cpu().numpy().copy(), grp.u.cpu().numpy().copy()
        grp.part_b()
        sv.sync()
        out = fails, u, grp.collided.cpu().numpy().copy(), grp.alive.cpu().numpy().copy()
        grp.results()           # (leaves both handles without world, forecast and clock)
    return out


def test_the_plant_meets_the_world_and_the_controller_its_forecast():
    """Z1, 'htwa', three instances at rest, clock t = 2.  One row's obstacle -- row 0's fixed capsule, collapsed to a point and thus a
    sphere of the row's radius -- jumps onto the instance's end-effector point in ONE column of the world; everywhere else the
    obstacles drift slowly.
    (a) The jump is in column t + 1 only: the CV forecast from columns t - 1 and t keeps the obstacle away, so the controller's step
        is bit for bit the step in the world without the jump -- but smpc_loop_post's verdict is "collision".
    (b) The mirror: the jump is in column t only, and the forecast holds it over the horizon ('hold'): the x_temp test of
        smpc_policy_step fails (fails > 0, none without the jump), and the plant, tested in column t + 1, is free."""
    from safe_mpc_amd.solver import BatchedOcpSolver
    N, B, T, t = 8, 3, 8, 2
    par, prob, net = make_problem('htwa', N=N)
    par.back_hor = 8
    x0 = sample_instances(prob, B, seed=5, vel_scale=0.0)
    xg, ug, p = constant_guess(prob, x0)
    s = BatchedOcpSolver(prob, net)
    ee = np.array(s.eval_nodes(xg, ug, p)['ee'])[:, 0, :3]
    calm = np.repeat(np.repeat(prob.row_geometry()[None, None], B, axis=0), T, axis=1)
    calm[..., 0] += 0.001 * np.arange(T)[None, :, None]           # every obstacle drifts along x
    hit = calm[:, 0].copy()
    hit[:, 0, 0:3] = hit[:, 0, 3:6] = ee
    # the premise, on the engine's standing-scene path: the states are free in the drifting world and collide with the jumped obstacle
    s.set_instance_scene(np.ascontiguousarray(calm[:, t + 1]))
    assert np.asarray(s.check_trajectory(x0[:, None, :])).all()
    s.set_instance_scene(hit)
    assert not np.asarray(s.check_trajectory(x0[:, None, :])).any()
    s.close()

    def jump(col):
        W = calm.copy()
        W[:, col, 0] = hit[:, 0]
        return np.ascontiguousarray(W)
    # (a)
    f0, u0, coll0, alive0 = _loop_arm(par, x0, calm, 'cv', t)
    f1, u1, coll1, alive1 = _loop_arm(par, x0, jump(t + 1), 'cv', t)
    print('(a) fails', f0, f1, 'collided', coll0, coll1)
    assert np.array_equal(f0, f1) and np.array_equal(u0, u1)       # the controller has not seen column t + 1
    assert (f0 == 0).all() and not coll0.any() and alive0.all()
    assert coll1.all() and not alive1.any()                         # the plant has
    # (b)
    f2, u2, coll2, alive2 = _loop_arm(par, x0, jump(t), 'hold', t)
    f3, u3, coll3, alive3 = _loop_arm(par, x0, calm, 'hold', t)
    print('(b) fails', f2, f3, 'collided', coll2, coll3)
    assert (f2 > 0).all() and (f3 == 0).all()                       # the controller plans in its forecast ...
    assert not coll2.any() and alive2.all() and not coll3.any()     # ... and the plant lives in the world


# ---- 5. the closed loop ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _closed_loop_case():
    N, B, steps = 8, 8, 12
    par, prob, net = make_problem('htwa', N=N)
    par.back_hor = 8
    x0 = sample_instances(prob, B, seed=9, vel_scale=0.2)
    xg, ug = np.repeat(x0[:, None, :], N + 1, axis=1), np.zeros((B, N, 6))
    world = turning_scenes(prob, B, steps + 1 + N, 0.3, 3.0, seed=2)
    return par, xg, ug, world, steps


@pytest.mark.parametrize('mode', ['hold', 'cv'])
def test_device_loop_with_a_forecast_equals_the_host_loop(mode):
    """run_mpc(on_device=True, forecast=m) against on_device=False (the statement) on turning tracks, B = 8, N = 8, 12 steps: equal
    index lists and x within 1e-6, the bound test_parallel_gpu.py::test_closed_loop_on_device_equals_host_loop uses for the same
    comparison"""
    from safe_mpc_amd import closed_loop as cl
    par, xg, ug, world, steps = _closed_loop_case()
    dev = cl.run_mpc(par, 'htwa', xg, ug, n_steps=steps, on_device=True, groups=1, scenes=world, forecast=mode, score=True)
    host = cl.run_mpc(par, 'htwa', xg, ug, n_steps=steps, on_device=False, scenes=world, forecast=mode, score=True)
    assert dev['forecast'] == host['forecast'] == mode
    for k in ('conv_idx', 'collisions_idx', 'unconv_idx'):
        assert dev[k] == host[k], k
    assert sorted(dev['viable_idx']) == sorted(host['viable_idx'])
    assert np.array_equal(np.isnan(dev['x']), np.isnan(host['x']))
    err = np.nanmax(np.abs(dev['x'] - host['x']))
    print(f'forecast {mode}: device loop against host loop, max |x| error {err:.3e}')
    assert err < 1e-6
    assert np.allclose(dev['score']['coll_margin'], host['score']['coll_margin'], atol=1e-6)        # both scored in the true world


def test_device_loop_forecast_true_is_the_loop_without_a_forecast():
    from safe_mpc_amd import closed_loop as cl
    par, xg, ug, world, steps = _closed_loop_case()
    a = cl.run_mpc(par, 'htwa', xg, ug, n_steps=steps, on_device=True, groups=1, scenes=world, forecast='true', score=True)
    b = cl.run_mpc(par, 'htwa', xg, ug, n_steps=steps, on_device=True, groups=1, scenes=world, score=True)
    for k in ('x', 'u', 'x_viable', 'r_receding'):
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    for k in ('conv_idx', 'collisions_idx', 'unconv_idx', 'viable_idx'):
        assert a[k] == b[k], k
    for k, v in a['score'].items():
        assert np.array_equal(v, b['score'][k], equal_nan=True), k
    c = cl.run_mpc(par, 'htwa', xg, ug, n_steps=steps, on_device=True, groups=1, scenes=world, forecast='hold')
    assert not np.array_equal(a['u'], c['u'], equal_nan=True)         # (a frozen world is another controller)


# ---- 6. the state machine and the refusals -------------------------------------------------------------------------------------------
def test_state_machine_and_refusals():
    import torch
    from safe_mpc_amd import controller as C
    from safe_mpc_amd._lib import EngineError
    N, B, T = 4, 5, 8
    s, prob = _solver('z1', N, ctx=True)
    plain, _ = _solver('z1', N)
    nr = len(prob.rows)
    x0 = sample_instances(prob, B, seed=1, vel_scale=0.5)
    xg, ug, p = constant_guess(prob, x0)
    W = fc.world(prob, B, T)
    ev = lambda sv=s, n=B: np.array(sv.eval_nodes(xg[:n], ug[:n], p[:n])['row_val'])
    shared = ev()
    # every error of the contract, by name
    with pytest.raises(EngineError, match=r'engine error -4: smpc_forecast_scene: no world is set'):
        s.forecast_scene('cv')
    s.set_instance_world_track(W)
    assert np.array_equal(ev(), shared)                             # the world alone changes nothing the controller sees
    with pytest.raises(EngineError, match=r'engine error -1: smpc_forecast_scene: batch size 4, .* 5 instances'):
        s.forecast_scene('cv', B=4)
    with pytest.raises(EngineError, match=r'engine error -1: smpc_forecast_scene: mode 3'):
        s.forecast_scene(3)
    with pytest.raises(ValueError, match="mode 'linear'"):
        s.forecast_scene('linear')
    with pytest.raises(EngineError, match=r'engine error -1: smpc_forecast_scene: n_sel=1, but the network has n_ctx=2'):
        s.forecast_scene('cv', [(0, 0)])
    for pair in ((nr, 0), (0, 8), (-1, 0)):
        with pytest.raises(EngineError, match=r'engine error -1: smpc_forecast_scene: select\[1\] = .* outside 6 rows x 8 slots'):
            s.forecast_scene('cv', [(0, 0), pair])
    with pytest.raises(EngineError, match=r'engine error -1: smpc_forecast_scene: n_sel=2 with select == NULL'):
        s._chk(s.L.smpc_forecast_scene(s.h, B, 1, 2, None))
    plain.set_instance_world_track(W)
    with pytest.raises(EngineError, match=r'engine error -1: smpc_forecast_scene: n_sel=2, but the network has no context columns'):
        plain.forecast_scene('cv', SELECT)
    with pytest.raises(EngineError, match=r'engine error -1: smpc_set_instance_world_track: T=0'):
        s._chk(s.L.smpc_set_instance_world_track(s.h, B, 0, W.ctypes.data, 0))
    bad = W.copy()
    bad[3, 2, 1, 4] = np.nan
    with pytest.raises(EngineError, match=r'engine error -1: scene track of instance 3, column 2, row 1'):
        s.set_instance_world_track(bad)
    assert fc.read_slots(s)[0]['scene_B'] == 0                      # refused calls have set nothing
    # forecast -> scene track -> clocked again
    keep = fc.set_clock(s, 3)
    s.forecast_scene('true', SELECT)
    info, F, ctx = fc.read_slots(s)
    assert info == dict(scene_B=B, scene_T=N + 1, scene_fc=1, ctx_B=B, ctx_T=N + 1, ctx_fc=1)
    at3 = ev()
    s.set_instance_context_track(scene_context(W, SELECT))
    s.set_instance_scene_track(W)
    info = fc.read_slots(s)[0]
    assert info['scene_fc'] == 0 and info['scene_T'] == T and info['ctx_fc'] == 0 and info['ctx_T'] == T
    assert np.array_equal(ev(), at3)                                # the track at clock 3 = its 'true' forecast
    s.set_instance_scene_track(np.ascontiguousarray(W[:, 3:]))
    assert not np.array_equal(ev(), at3)                            # (clocked: now columns 6, 7, 7, ..)
    # a scene setter over a forecast drops the context the forecast wrote (a setter's own context stays)
    s.forecast_scene('cv', SELECT)
    s.set_instance_scene(np.ascontiguousarray(W[:, 0]))
    info = fc.read_slots(s)[0]
    assert info['scene_fc'] == 0 and info['ctx_B'] == 0
    # clearing the world clears the forecast, and the context it wrote; a scene of a setter's stays
    s.forecast_scene('cv', SELECT)
    s.set_instance_world_track(None)
    info = fc.read_slots(s)[0]
    assert info['scene_B'] == 0 and info['ctx_B'] == 0
    s.set_scene_clock(None)
    assert np.array_equal(ev(), shared)
    s.set_instance_scene(np.ascontiguousarray(W[:, 0]))
    s.set_instance_world_track(W)
    s.set_instance_world_track(None)
    assert fc.read_slots(s)[0]['scene_B'] == B
    s.set_instance_scene(None)
    # smpc_set_horizon drops a forecast (and keeps the world: the next forecast is laid out by the new horizon)
    s.set_instance_world_track(W)
    s.forecast_scene('hold', SELECT)
    s.set_horizon(N)
    info = fc.read_slots(s)[0]
    assert info['scene_B'] == 0 and info['ctx_B'] == 0
    s.set_horizon(2)
    s.forecast_scene('hold')
    assert fc.read_slots(s)[0]['scene_T'] == 3
    s.set_horizon(N)
    # another batch size while a forecast is set: refused as for any scene; smpc_rollout_batch refuses the slot
    s.forecast_scene('cv')
    with pytest.raises(EngineError, match=r'batch size 4, .* 5 instances'):
        ev(n=4)
    with pytest.raises(EngineError, match=r'engine error -4: smpc_rollout_batch'):
        s.rollout(x0, xg, ug, p, 2)
    s.set_instance_world_track(None)
    # the parallel policy refuses a forecast; smpc_loop_post guards the world's batch size
    parp, probp, netp = make_problem('parallel', N=4)
    ctrl = C.get_controller('parallel', parp, 3, N=4, device_state=True)
    xp = torch.tensor(sample_instances(probp, 3, seed=2), dtype=torch.float64, device='cuda:0')
    ctrl.setGuess(xp[:, None, :].repeat(1, 5, 1), torch.zeros((3, 4, 6), dtype=torch.float64, device='cuda:0'))
    ctrl.ocp_solver.set_instance_world_track(fc.world(ctrl.problem, 3, 4))
    ctrl.ocp_solver.forecast_scene('cv')
    with pytest.raises(EngineError, match=r'engine error -4: smpc_policy_step: .*parallel'):
        ctrl.step_on_device(xp)
    ctrl.ocp_solver.set_instance_world_track(None)
    from safe_mpc_amd import closed_loop as cl
    par3, prob3, _ = make_problem('st', N=8)
    par3.back_hor = 8
    c3, b3 = C.get_controller('st', par3, 3, device_state=True), C.SafeBackupController(par3, 3, device_state=True)
    sv3 = c3.ocp_solver
    x3 = sample_instances(prob3, 3, seed=1)
    with torch.cuda.stream(torch.cuda.ExternalStream(sv3.L.smpc_stream(sv3.h), device=torch.device('cuda', sv3.device))):
        grp = cl._DeviceGroup(par3, np.repeat(x3[:, None, :], 9, axis=1), np.zeros((3, 8, 6)), 0.0, 0.0, c3, b3, 2, 0, False, use_graphs=False)
        grp.part_a()
        sv3.set_instance_world_track(fc.world(prob3, 5, 4))
        with pytest.raises(EngineError, match=r'engine error -1: smpc_loop_post: batch size 3, .*world track was set for 5 instances'):
            grp.part_b()
        sv3.set_instance_world_track(None)
        sv3.sync()


def test_growth_under_capture_is_refused_and_a_captured_forecast_follows_the_clock():
    """capture as test_context_track_gpu.py does it: torch's capture stream, which the engine's stream joins for the call"""
    import torch
    from safe_mpc_amd._lib import EngineError
    N, B, T = 4, 5, 8
    s, prob = _solver('z1', N, ctx=True)
    x0 = sample_instances(prob, B, seed=1, vel_scale=0.5)
    xg, ug, p = constant_guess(prob, x0)
    dev_in = [_dev(a) for a in (x0, xg, ug, p)]
    W = fc.world(prob, B, T)
    cell = fc.cell(1)
    torch.cuda.synchronize()
    s.set_scene_clock(cell)
    s.set_instance_world_track(_dev(W))

    def refused():
        with pytest.raises(EngineError, match=r'engine error -4: smpc_forecast_scene: .* while the stream is being captured'), \
                warnings.catch_warnings():
            warnings.filterwarnings('ignore', 'The CUDA Graph is empty')
            with torch.cuda.graph(torch.cuda.CUDAGraph()):
                s.forecast_scene('cv', SELECT)
        torch.cuda.synchronize()
    # the slots do not exist yet: a first forecast inside a capture would have to grow them
    refused()
    assert fc.read_slots(s)[0]['scene_B'] == 0
    # a standing scene in the slot (smaller than a forecast): growth is refused and the old content keeps serving
    s.set_instance_context(scene_context(W[:, 0], SELECT))
    s.set_instance_scene(np.ascontiguousarray(W[:, 0]))
    before = [np.array(a) for a in s.solve(x0, xg, ug, p)]
    refused()
    info = fc.read_slots(s)[0]
    assert info['scene_fc'] == 0 and info['scene_T'] == 1 and info['ctx_fc'] == 0
    assert all(np.array_equal(a, b) for a, b in zip([np.array(a) for a in s.solve(x0, xg, ug, p)], before))
    # [forecast_scene; solve] eager at clocks 1 and 5, then captured once at clock 1 and replayed after the cell was rewritten
    eager = {}
    for c in (1, 5):
        cell.fill_(c)
        s.forecast_scene('cv', SELECT)
        res = s.solve(*dev_in)
        s.sync()
        eager[c] = [a.cpu().numpy().copy() for a in res]
        assert np.array_equal(fc.read_slots(s)[1], forecast_statement(W, c, N, 'cv'))
    assert not np.array_equal(eager[1][1], eager[5][1])
    cell.fill_(1)
    out = tuple(torch.empty_like(a) for a in res)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        s.forecast_scene('cv', SELECT)
        s.solve(*dev_in, out=out)
    for c in (5, 1):
        cell.fill_(c)
        g.replay()
        torch.cuda.synchronize()
        assert all(np.array_equal(o.cpu().numpy(), w) for o, w in zip(out, eager[c])), c
        assert np.array_equal(fc.read_slots(s)[1], forecast_statement(W, c, N, 'cv'))
    s.set_instance_world_track(None)
    s.set_scene_clock(None)
