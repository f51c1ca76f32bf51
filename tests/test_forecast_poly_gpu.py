"""Obstacle forecasts of degree 0 to 2 on the engine (smpc_forecast_scene_poly, k_scene_poly).  The slots are read
back through the engine's test hook smpc_debug_scene_slots (forecast_cases.read_slots).

1. the kernel equals problem.poly_forecast_statement bit for bit -- degrees 0 and 2, windows {1, 2, 3, 4, 7, 32}, N in {1, 4}, T in
   {1, 2, N + 1, N + 4, 40}, B in {1, 5, 23}, both robots, the clock family (clocks that leave m at 1, 2 and 3 and that fill 32), host-
   and device-pointer tables, twice, every instance alone, with and without an observed track, a NaN carried; and the fp32 context
   rows.  The worlds have full mantissas in all eight slots, so a product that is fused into its sum shows in the last bit: this is
   the proof of the rounding.
2. degree 1 is smpc_forecast_scene_fit on the device, degree 0 with window 1 the HOLD kernel, degree 2 with window 2 the CV kernel
3. the slot is a table like any other: after the call, eval_nodes, the stage records of both builders and the solve in both QP forms
   are those after set_instance_scene_track(poly_forecast_statement(..)) with no clock
4. every refusal by name, and that it changed nothing
5. a captured [forecast_scene_poly; solve] follows the rewritten clock cell; growth under capture is refused for each buffer
6. run_mpc(on_device=True, forecast='fit', forecast_degree=2, observed=...) against the host loop"""
import warnings

import numpy as np
import pytest

import forecast_cases as fc
import poly_forecast_cases as pf
from conftest import constant_guess, sample_instances
from safe_mpc_amd.problem import poly_forecast_statement, scene_context
from test_forecast_fit_gpu import _loop_case
from test_forecast_gpu import CTX_MEAN, CTX_STD, SELECT, _calls, _dev, _same, _solver

pytestmark = pytest.mark.gpu

NEW_DEGREES = (0, 2)            # what k_scene_poly itself computes (degree 1 launches k_scene_fit)


def _poly(s, window, degree, select=None):
    s.forecast_scene_poly(window, degree, select)
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
                for c in pf.clocks(T):
                    keep = fc.set_clock(s, c)
                    for degree in NEW_DEGREES:
                        for window in pf.WINDOWS:
                            want = poly_forecast_statement(S, c, N, window, degree)
                            info, F, _ = _poly(s, window, degree)
                            assert info['scene_B'] == B and info['scene_T'] == N + 1 and info['scene_fc'] == 1, (T, B, c, window, degree, info)
                            assert F.shape == (B, N + 1, nr, 8)
                            assert np.array_equal(_bits(F), _bits(want)), (T, B, observed, c, window, degree, np.abs(F - want).max())
                            if observed == on_device and window in (3, 32):      # called twice: the same bits
                                assert np.array_equal(_bits(_poly(s, window, degree)[1]), _bits(F)), (T, B, c, window, degree)
                    del keep
    # every instance alone (B = 1: four lanes of a wavefront) equals its rows at B = 23, world and observed track alike
    T, B = 40, 23
    W, O = fc.world(prob, B, T, seed=T), fc.world(prob, B, T, seed=T + 11)
    keep = fc.set_clock(s, 35)
    for window, degree in ((3, 2), (32, 2), (7, 0)):
        s.set_instance_world_track(W)
        s.set_instance_observed_track(O)
        F23 = _poly(s, window, degree)[1]
        assert np.array_equal(_bits(F23), _bits(poly_forecast_statement(O, 35, N, window, degree)))
        for b in range(B):
            s.set_instance_world_track(W[b:b + 1])
            s.set_instance_observed_track(O[b:b + 1])
            info, F1, _ = _poly(s, window, degree)
            assert info['scene_B'] == 1 and np.array_equal(_bits(F1), _bits(F23[b:b + 1])), (window, degree, b)
    # a NaN in what was seen is carried, not trapped (device pointers are taken as they are)
    On = O.copy()
    On[2, 34, 1, 7] = np.nan
    s.set_instance_world_track(W)
    s.set_instance_observed_track(_dev(On))
    for degree in NEW_DEGREES:
        F = _poly(s, 7, degree)[1]
        assert np.array_equal(F, poly_forecast_statement(On, 35, N, 7, degree), equal_nan=True) and np.isnan(F).any()
    # a world of -0.0 and zeros keeps its bits under degree 0 (F[k] = a is stored, not added)
    Z = W.copy()
    Z[..., 7] = 0.0
    Z[:, :, 0, :4] = -0.0
    s.set_instance_observed_track(_dev(Z))
    F = _poly(s, 7, 0)[1]
    assert np.array_equal(_bits(F), _bits(poly_forecast_statement(Z, 35, N, 7, 0)))
    assert np.array_equal(_bits(F[:, :, 0, :4]), _bits(np.full_like(F[:, :, 0, :4], -0.0)))
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
            for degree in NEW_DEGREES:
                for window in pf.WINDOWS:
                    F = poly_forecast_statement(S, c, N, window, degree)
                    want = ((scene_context(F, SELECT) - CTX_MEAN) / CTX_STD).astype(np.float32)
                    info, got_F, got = _poly(s, window, degree, SELECT)
                    assert info['ctx_B'] == B and info['ctx_T'] == N + 1 and info['ctx_fc'] == 1, info
                    assert np.array_equal(_bits(got_F), _bits(F)) and got.shape == (B, N + 1, 2)
                    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (B, T, c, window, degree)
            del keep
    s.set_instance_world_track(None)


# ---- 2. the older kernels -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('system', ['z1', 'fr7'])
def test_degree_1_is_the_fit_and_the_small_windows_are_hold_and_cv_on_the_device(system):
    N = 4
    s, prob = _solver(system, N)
    for T in (1, 2, N + 4, 40):
        W = fc.world(prob, 23, T, seed=T)
        s.set_instance_world_track(_dev(W))
        for c in pf.clocks(T):
            keep = fc.set_clock(s, c)
            for window in pf.WINDOWS:
                s.forecast_scene_fit(window)
                old = fc.read_slots(s)[1]
                assert np.array_equal(_bits(_poly(s, window, 1)[1]), _bits(old)), (T, c, window)
            for window, degree, mode in ((1, 0, 'hold'), (2, 2, 'cv'), (1, 2, 'hold')):
                s.forecast_scene(mode)
                old = fc.read_slots(s)[1]
                assert np.array_equal(_bits(_poly(s, window, degree)[1]), _bits(old)), (T, c, window, degree)
            del keep
    s.set_instance_world_track(None)
    s.set_scene_clock(None)


# ---- 3. the slot is a table like any other -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('system,N,ctx', [('z1', 4, False), ('z1', 4, True), ('fr7', 4, False), ('z1', 1, False)])
def test_the_forecast_in_the_slot_is_the_statement_set_as_a_track(system, N, ctx):
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
    for c, window, degree, observed in ((None, 3, 2, False), (5, 3, 2, True), (T - 1, 7, 2, True), (T + 5, 32, 0, False),
                                        (2 ** 63 - 1, 4, 2, True)):
        F = poly_forecast_statement(O if observed else W, c, N, window, degree)
        # the statement as a track of the caller's, no clock
        s.set_instance_world_track(None)
        s.set_scene_clock(None)
        if ctx:
            s.set_instance_context_track(scene_context(F, SELECT))
        s.set_instance_scene_track(F)
        ref = _calls(s, N, inputs)
        refs.append(ref)
        # the engine's forecast at clock c
        s.set_instance_world_track(_dev(W))
        s.set_instance_observed_track(O if observed else None)
        keep = fc.set_clock(s, c)
        s.forecast_scene_poly(window, degree, select)
        assert _same(_calls(s, N, inputs), ref) == [], (c, window, degree, observed)
        del keep
    assert all(_same(refs[0], r) for r in refs[1:])         # (the cases are different problems)
    s.set_instance_world_track(None)
    s.set_scene_clock(None)


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_by_name_changes_nothing():
    from safe_mpc_amd._lib import EngineError
    N, B, T = 4, 5, 8
    s, prob = _solver('z1', N, ctx=True)
    plain, _ = _solver('z1', N)
    nr = len(prob.rows)
    W, O = fc.world(prob, B, T), fc.world(prob, B, T, seed=4)
    with pytest.raises(EngineError, match=r'engine error -4: smpc_forecast_scene_poly: no world is set'):
        s.forecast_scene_poly(4, 2)
    s.set_instance_observed_track(O)                                # (an observed track alone is no world)
    with pytest.raises(EngineError, match=r'engine error -4: smpc_forecast_scene_poly: no world is set'):
        s.forecast_scene_poly(4, 2, B=B)
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
        refused(r'smpc_forecast_scene_poly: batch size 4, .* 5 instances', lambda: s.forecast_scene_poly(4, 2, B=4))
        for window in (0, 33, -1):
            refused(rf'smpc_forecast_scene_poly: window {window}\b', lambda: s.forecast_scene_poly(window, 2))
        for degree in (-1, 3):
            refused(rf'smpc_forecast_scene_poly: degree {degree}\b', lambda: s.forecast_scene_poly(4, degree))
        refused(r'smpc_forecast_scene_poly: n_sel=1, but the network has n_ctx=2', lambda: s.forecast_scene_poly(4, 2, [(0, 0)]))
        for pair in ((nr, 0), (0, 8), (-1, 0)):
            refused(r'smpc_forecast_scene_poly: select\[1\] = .* outside 6 rows x 8 slots', lambda: s.forecast_scene_poly(4, 0, [(0, 0), pair]))
        refused(r'smpc_forecast_scene_poly: n_sel=2 with select == NULL', lambda: s._chk(s.L.smpc_forecast_scene_poly(s.h, B, 4, 2, 2, None)))
        refused(r'smpc_forecast_scene_poly: n_sel=-1', lambda: s._chk(s.L.smpc_forecast_scene_poly(s.h, B, 4, 2, -1, None)))
        # an observed track of another shape than the world's
        s.set_instance_observed_track(np.ascontiguousarray(O[:4]))
        refused(rf'smpc_forecast_scene_poly: the instance observed track was set for 4 instances and {T} columns, but the instance world '
                rf'track for {B} instances and {T} columns', lambda: s.forecast_scene_poly(4, 2))
        s.set_instance_observed_track(O)
    family()                                                        # with empty slots: refused calls have set nothing ...
    assert fc.read_slots(s)[0]['scene_B'] == 0
    s.forecast_scene_poly(7, 2, SELECT)
    assert fc.read_slots(s)[0] == dict(scene_B=B, scene_T=N + 1, scene_fc=1, ctx_B=B, ctx_T=N + 1, ctx_fc=1)
    family()                                                        # ... and with a forecast in them: it stays in force
    assert np.array_equal(_bits(fc.read_slots(s)[1]), _bits(poly_forecast_statement(O, None, N, 7, 2)))
    plain.set_instance_world_track(W)
    with pytest.raises(EngineError, match=r'engine error -1: smpc_forecast_scene_poly: n_sel=2, but the network has no context columns'):
        plain.forecast_scene_poly(4, 2, SELECT)
    # the fit keeps its own name in its refusals
    refused(r'smpc_forecast_scene_fit: window 33\b', lambda: s.forecast_scene_fit(33))
    for sv in (s, plain):
        sv.set_instance_world_track(None)


# ---- 5. capture ------------------------------------------------------------------------------------------------------------------------------
def test_growth_under_capture_is_refused_for_each_buffer_and_a_captured_forecast_follows_the_clock():
    """capture as test_forecast_gpu.py does it: torch's capture stream, which the engine's stream joins for the call"""
    import torch
    from safe_mpc_amd._lib import EngineError
    N, B, T = 4, 5, 12
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
    refused('smpc_forecast_scene_poly: the instance scene', lambda: s.forecast_scene_poly(4, 2, SELECT))
    assert fc.read_slots(s)[0]['scene_B'] == 0
    # the scene buffer exists, the context buffer does not: the old forecast keeps serving
    s.forecast_scene_poly(4, 2)
    before = fc.read_slots(s)
    refused('smpc_forecast_scene_poly: the instance context', lambda: s.forecast_scene_poly(7, 0, SELECT))
    after = fc.read_slots(s)
    assert after[0] == before[0] and after[0]['ctx_B'] == 0 and np.array_equal(after[1], before[1])
    s.set_instance_observed_track(_dev(O))
    # [forecast_scene_poly; solve] eager at clocks 1 (two samples: a line) and 7 (a full window: a parabola), then captured once at
    # clock 1 and replayed after the cell was rewritten
    eager = {}
    for c in (1, 7):
        cell.fill_(c)
        s.forecast_scene_poly(4, 2, SELECT)
        res = s.solve(*dev_in)
        s.sync()
        eager[c] = [a.cpu().numpy().copy() for a in res]
        assert np.array_equal(_bits(fc.read_slots(s)[1]), _bits(poly_forecast_statement(O, c, N, 4, 2)))
    assert not np.array_equal(eager[1][1], eager[7][1])
    cell.fill_(1)
    out = tuple(torch.empty_like(a) for a in res)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        s.forecast_scene_poly(4, 2, SELECT)
        s.solve(*dev_in, out=out)
    for c in (7, 1):
        cell.fill_(c)
        g.replay()
        torch.cuda.synchronize()
        assert all(np.array_equal(o.cpu().numpy(), w) for o, w in zip(out, eager[c])), c
        assert np.array_equal(_bits(fc.read_slots(s)[1]), _bits(poly_forecast_statement(O, c, N, 4, 2)))
    s.set_instance_world_track(None)
    s.set_scene_clock(None)


# ---- 6. the closed loop ---------------------------------------------------------------------------------------------------------------------
def test_device_loop_with_a_parabola_through_observations_equals_the_host_loop():
    """run_mpc(on_device=True, forecast='fit', forecast_window=4, forecast_degree=2, observed=...) against on_device=False (the
    statement) on the case of test_forecast_fit_gpu.py: equal index lists and x within 1e-6, the comparison and the tolerance of its
    test_device_loop_with_a_fit_of_observations_equals_the_host_loop.  An abort event must occur (x_viable is not empty), so that the
    backup handle's path -- world rows, observed rows, the same estimator over its own horizon -- has run.  And a solver without
    forecast_scene_poly is refused by name before anything is enqueued."""
    from safe_mpc_amd import closed_loop as cl
    from safe_mpc_amd import controller as C
    par, xg, ug, world, observed, steps = _loop_case()
    kw = dict(n_steps=steps, scenes=world, forecast='fit', forecast_window=4, forecast_degree=2, observed=observed, score=True)
    dev = cl.run_mpc(par, 'htwa', xg, ug, on_device=True, groups=1, **kw)
    host = cl.run_mpc(par, 'htwa', xg, ug, on_device=False, **kw)
    assert dev['forecast'] == host['forecast'] == 'fit' and dev['forecast_window'] == host['forecast_window'] == 4
    assert dev['forecast_degree'] == host['forecast_degree'] == 2
    print('abort events: x_viable', dev['x_viable'].shape, host['x_viable'].shape, 'viable_idx', dev['viable_idx'], 'collisions',
          dev['collisions_idx'], 'unconv', dev['unconv_idx'])
    assert dev['x_viable'].shape[0] > 0 and dev['x_viable'].shape == host['x_viable'].shape
    for k in ('conv_idx', 'collisions_idx', 'unconv_idx'):
        assert dev[k] == host[k], k
    assert sorted(dev['viable_idx']) == sorted(host['viable_idx'])
    assert np.array_equal(np.isnan(dev['x']), np.isnan(host['x']))
    err = np.nanmax(np.abs(dev['x'] - host['x']))
    print(f'forecast fit (window 4, degree 2, observed): device loop against host loop, max |x| error {err:.3e}')
    assert err < 1e-6
    assert np.allclose(dev['score']['coll_margin'], host['score']['coll_margin'], atol=1e-6)        # both scored in the true world
    assert np.array_equal(dev['scenes'], world)

    # a solver that lacks the call: named, and nothing was handed to it
    calls = []

    class Hidden:
        """a solver proxy without forecast_scene_poly that writes down every other call"""

        def __init__(self, sv):
            object.__setattr__(self, '_sv', sv)

        def __getattr__(self, name):
            if name == 'forecast_scene_poly':
                raise AttributeError(name)
            attr = getattr(self._sv, name)
            if not (callable(attr) and name.startswith(('set_instance', 'forecast_scene', 'loop_', 'solve'))):
                return attr

            def noted(*a, **k):
                calls.append(name)
                return attr(*a, **k)
            return noted

    def mk(name, batch):
        ctrl = C.get_controller(name, par, batch, device_state=True)
        ctrl.ocp_solver = Hidden(ctrl.ocp_solver)
        return ctrl
    with pytest.raises(ValueError, match='forecast_degree: Hidden has no forecast_scene_poly'):
        cl.run_mpc(par, 'htwa', xg, ug, on_device=True, groups=1, make_controller=mk, **kw)
    assert calls == []
