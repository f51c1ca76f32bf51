"""Row margins from the fit's residuals on the engine (smpc_forecast_row_margin, k_fit_margin, smpc_get_instance_row_bounds; DESIGN.md
section 9r).  -m gpu only.  problem.fit_margin_statement is the definition and numpy the reference, never the kernel.

0. the device's f64 square root and division are correctly rounded on radicands with full mantissas: a plane row with lb = 0 hands
   d itself back (lo = 0 + d), so every bit of the two roots and the division shows.  It holds, so everything below is bit for bit.
1. the kernel equals inflated_row_bounds(fit_margin_statement) through get_instance_row_bounds: degrees 0, 1, 2, windows {1, 2, 3, 4, 7,
   32}, the clock family, both arms, N in {1, 4, 63}, B in {1, 5, 23}, T in {2, 40}, with and without an observed track, both kinds
   of pointer, twice, every instance alone, a NaN sample, z = 0, the cap reached
2. what reads the slot: stage records of both builders, the solve in both QP forms and one policy step equal those with
   set_instance_row_bounds(statement)
3. every refusal by name with the slot unchanged; the slot rule; set_horizon drops the table
4. growth under capture refused; a captured [forecast; margin; solve] follows the rewritten clock cell
5. the device loop against the host loop with an abort event; z = 0 and base (0, 0) against the loop without the argument"""
import warnings

import numpy as np
import pytest

import forecast_cases as fc
import margin_cases as mc
from conftest import make_problem_fr7
from safe_mpc_amd.problem import ROW_COORD, fit_margin_statement, inflated_row_bounds
from test_row_bounds_gpu import _dev, _same, _solver, _stage_records

pytestmark = pytest.mark.gpu

ARGS = dict(z=2.0, sigma_prior=1e-4, base=(0.003, 0.0005), d_max=0.04)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _want(prob, S, c, window, degree, **kw):
    d = fit_margin_statement(prob, S, c, window, degree, **kw)
    return inflated_row_bounds(prob, S.shape[0], d)


def _equal(got, want):
    return all(np.array_equal(_bits(np.asarray(g)), _bits(w)) for g, w in zip(got, want))


# ---- 0. square root and division ---------------------------------------------------------------------------------------------------------
def test_device_square_root_and_division_are_correctly_rounded():
    """Everything in k_fit_margin but two square roots and one division is add, multiply and select in the statement's order.  A plane
    row whose lower side is 0.0 and whose upper side is absent gets lo = 0.0 + d = d, bit for bit, so the table hands back d itself:
    (z sqrt(rss / nu)) sqrt(h_k) with z = 1, no base, no prior and the cap out of the way.  N = 63 (all 64 values of h_k), every
    window 2..32 and degree with nu >= 1 -- 29 values of nu as the divisor --, B = 23 instances of a world with full mantissas: 1 860
    radicands h_k and 2 001 pairs (rss, nu), each seen through up to 64 products.  numpy's sqrt and division are IEEE 754's, so
    equality of every d means the device's are correctly rounded on these; the figures are printed before the assertion."""
    N, B, T = 63, 23, 40
    par, prob, net = make_problem_fr7('constraint_everywhere', N=N)
    i = next(k for k, r in enumerate(prob.rows) if r.kind == ROW_COORD)
    prob.rows[i].lb = prob.desc.rows[i].lb = prob.row_lb[i] = 0.0
    assert abs(prob.rows[i].ub) >= 1e5
    s = _solver(prob, net)
    S = fc.world(prob, B, T, seed=5, amp=0.05)
    s.set_instance_world_track(_dev(S))
    keep = fc.set_clock(s, 35)
    n, wrong, worst = 0, 0, 0.0
    for m in range(2, 33):
        for p in mc.DEGREES:
            if m - min(p, m - 1) - 1 < 1:
                continue
            d = fit_margin_statement(prob, S, 35, m, p, 1.0, 0.0, (0.0, 0.0), 1e3)[:, :, i]
            s.forecast_row_margin(m, p, 1.0, 0.0, (0.0, 0.0), 1e3)
            lo, hi = s.get_instance_row_bounds()
            got = lo[:, :, i]
            assert (hi[:, :, i] == prob.row_ub[i]).all() and d.min() > 0.0
            n += d.size
            wrong += int((_bits(got) != _bits(d)).sum())
            worst = max(worst, float((np.abs(got - d) / np.spacing(d)).max()))
    print(f'd through the device\'s sqrt, sqrt and division against numpy: {wrong} of {n} values differ, worst {worst:.2f} ulp')
    assert wrong == 0
    del keep
    s.set_instance_world_track(None)
    s.set_scene_clock(None)


# ---- 1. the kernel equals the statement ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('system,N,B', [('z1', 4, 5), ('z1', 63, 23), ('z1', 1, 1), ('fr7', 4, 23), ('fr7', 1, 5), ('fr7', 63, 1)])
def test_kernel_equals_statement_bit_for_bit(system, N, B):
    """B = 1 is four lanes of a wavefront, B = 5 a partial one, B = 23 with six rows 552 lanes: records straddle blocks; N = 63 fills
    the LDS table with all 64 lanes.  Worlds with full mantissas in all eight slots (forecast_cases.world)."""
    par, prob, net = mc.problem(system, N)
    s = _solver(prob, net)
    nr = len(prob.rows)
    for T in (2, 40):
        W, O = fc.world(prob, B, T, seed=T), fc.world(prob, B, T, seed=T + 11)
        for observed in (False, True):
            on_device = observed == (T == 40)
            s.set_instance_world_track(_dev(W) if on_device else W)
            s.set_instance_observed_track((O if on_device else _dev(O)) if observed else None)
            S = O if observed else W
            for c in mc.clocks(T):
                keep = fc.set_clock(s, c)
                for degree in mc.DEGREES:
                    for window in mc.WINDOWS:
                        want = _want(prob, S, c, window, degree, **ARGS)
                        s.forecast_row_margin(window, degree, **ARGS)
                        got = s.get_instance_row_bounds(device=on_device)
                        if on_device:
                            got = [g.cpu().numpy() for g in got]
                        assert got[0].shape == got[1].shape == (B, N + 1, nr)
                        assert _equal(got, want), (T, observed, c, window, degree, np.abs(got[0] - want[0]).max())
                        if window in (3, 32) and degree == 2:             # called twice: the same bits
                            s.forecast_row_margin(window, degree, **ARGS)
                            assert _equal(s.get_instance_row_bounds(), want)
                del keep
    s.set_instance_world_track(None)
    s.set_scene_clock(None)


@pytest.mark.parametrize('system', ['z1', 'fr7'])
def test_every_instance_alone_a_nan_sample_z_zero_and_the_cap(system):
    N, B, T = 4, 23, 40
    par, prob, net = mc.problem(system, N)
    s = _solver(prob, net)
    W, O = fc.world(prob, B, T, seed=3), fc.world(prob, B, T, seed=14)
    keep = fc.set_clock(s, 35)
    for window, degree in ((3, 1), (32, 2), (7, 0)):
        s.set_instance_world_track(W)
        s.set_instance_observed_track(O)
        s.forecast_row_margin(window, degree, **ARGS)
        batch = s.get_instance_row_bounds()
        assert _equal(batch, _want(prob, O, 35, window, degree, **ARGS))
        for b in range(B):
            s.set_instance_world_track(W[b:b + 1])
            s.set_instance_observed_track(O[b:b + 1])
            s.forecast_row_margin(window, degree, **ARGS)
            assert _equal(s.get_instance_row_bounds(), [a[b:b + 1] for a in batch]), (window, degree, b)
    # a NaN sample gives the cap and never a NaN bound (device pointers are taken as they are)
    On = O.copy()
    slot = 6 if prob.rows[-1].kind == ROW_COORD else 1
    On[2, 33, len(prob.rows) - 1, slot] = np.nan
    On[4, 30, 0, 0] = np.nan
    s.set_instance_world_track(W)
    s.set_instance_observed_track(_dev(On))
    for degree in mc.DEGREES:
        s.forecast_row_margin(7, degree, **ARGS)
        got = s.get_instance_row_bounds()
        want = _want(prob, On, 35, 7, degree, **ARGS)
        assert _equal(got, want) and np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
        d = fit_margin_statement(prob, On, 35, 7, degree, **ARGS)
        assert (d[2, :, -1] == ARGS['d_max']).all() and (d[4, :, 0] == ARGS['d_max']).all()
    s.set_instance_observed_track(O)
    # z = 0 gives the base -- the table of run_mpc(row_margin=base) --, and with no base either the descriptor's own doubles
    s.forecast_row_margin(7, 2, 0.0, 1e-4, ARGS['base'], 0.04)
    assert _equal(s.get_instance_row_bounds(), inflated_row_bounds(prob, B, ARGS['base'][0] + ARGS['base'][1] * np.arange(N + 1)))
    s.forecast_row_margin(7, 2, 0.0, 0.0, (0.0, 0.0), 0.04)
    lo, hi = s.get_instance_row_bounds()
    assert _equal((lo, hi), (np.broadcast_to(prob.row_lb, lo.shape), np.broadcast_to(prob.row_ub, hi.shape)))
    # the cap reached by size
    kw = dict(z=50.0, sigma_prior=0.0, base=(0.0, 0.0), d_max=0.01)
    s.forecast_row_margin(7, 1, **kw)
    assert _equal(s.get_instance_row_bounds(), _want(prob, O, 35, 7, 1, **kw))
    assert (fit_margin_statement(prob, O, 35, 7, 1, **kw) == 0.01).any()
    del keep
    s.set_instance_world_track(None)
    s.set_scene_clock(None)


# ---- 2. what reads the slot ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('system,N,B', [('z1', 4, 5), ('fr7', 4, 23)])
def test_the_device_made_table_is_the_statement_set_as_a_table(system, N, B):
    import row_bounds_cases as rb
    par, prob, net = mc.problem(system, N)
    x0, xg, ug, p = rb.inputs(prob, B)
    T = 12
    W = fc.world(prob, B, T, seed=2, amp=0.002)
    kw = dict(z=2.0, sigma_prior=0.0, base=(0.001, 0.0), d_max=0.03)
    for mode in ('throughput', 'latency'):
        s = _solver(prob, net, mode)
        calls = lambda: [_stage_records(s, x0, xg, ug, p, 1)[0], _stage_records(s, x0, xg, ug, p, 0)[0]] + \
            [np.array(a) for a in s.solve(x0, xg, ug, p)]
        plain = calls()
        s.set_instance_row_bounds(*_want(prob, W, 9, 7, 2, **kw))
        ref = calls()
        assert not _same(ref[:2], plain[:2])                               # (the table is read)
        s.set_instance_row_bounds(None)
        s.set_instance_world_track(_dev(W))
        keep = fc.set_clock(s, 9)
        s.forecast_row_margin(7, 2, **kw)
        assert _same(calls(), ref)
        del keep
        s.set_instance_world_track(None)
        s.set_scene_clock(None)
        s.set_instance_row_bounds(None)
        assert _same(calls(), plain)


@pytest.mark.parametrize('name', ['stwa', 'receding'])
def test_policy_step_reads_the_device_made_table(name):
    import row_bounds_cases as rb
    import torch
    from safe_mpc_amd import controller as Cn
    N, B, T = 4, 5, 12
    par, prob, _ = rb.problem('z1', N, controller=name)
    x0, xg, ug, p = rb.inputs(prob, B)
    W = fc.world(prob, B, T, seed=2, amp=0.002)
    kw = dict(z=2.0, sigma_prior=0.0, base=(0.001, 0.0), d_max=0.03)

    def step(made_on_device):
        c = Cn.get_controller(name, par, B, N=N, device_state=True)
        sv = c.ocp_solver
        sv.set_qp_mode('throughput')
        c.setGuess(_dev(xg), _dev(ug))
        keep = None
        if made_on_device:
            sv.set_instance_world_track(_dev(W))
            keep = fc.set_clock(sv, 9)
            sv.forecast_row_margin(7, 2, **kw)
            sv.set_scene_clock(None)
        elif made_on_device is not None:
            sv.set_instance_row_bounds(*_want(sv.problem, W, 9, 7, 2, **kw))
        u, ab = c.step_on_device(_dev(x0))
        sv.sync()
        torch.cuda.synchronize()
        del keep
        return [t.cpu().numpy().copy() for t in (u, ab, c.x_guess, c.u_guess, c.x_temp, c.u_temp, c.last_status, c.fails)]
    ref = step(False)
    assert _same(step(True), ref)
    assert not _same(step(None)[4:6], ref[4:6])


# ---- 3. refusals and state --------------------------------------------------------------------------------------------------------------------
def test_every_refusal_by_name_leaves_the_slot_unchanged_and_the_slot_rule():
    import row_bounds_cases as rb
    from safe_mpc_amd._lib import EngineError
    N, B, T = 4, 5, 8
    par, prob, net = mc.problem('fr7', N)
    s = _solver(prob, net, 'throughput')
    W, O = fc.world(prob, B, T), fc.world(prob, B, T, seed=4)
    who = 'smpc_forecast_row_margin'
    with pytest.raises(EngineError, match=r'engine error -4: smpc_get_instance_row_bounds: no instance row-bounds table is set'):
        s.get_instance_row_bounds()
    with pytest.raises(EngineError, match=rf'engine error -4: {who}: no world is set'):
        s.forecast_row_margin(4, 2, 2.0)
    s.set_instance_observed_track(O)                                # (an observed track alone is no world)
    with pytest.raises(EngineError, match=rf'engine error -4: {who}: no world is set'):
        s.forecast_row_margin(4, 2, 2.0, B=B)
    s.set_instance_world_track(W)
    state = {'table': None}

    def refused(match, call, code=-1):
        with pytest.raises(EngineError, match=rf'engine error {code}: {match}'):
            call()
        if state['table'] is None:
            with pytest.raises(EngineError, match='no instance row-bounds table is set'):
                s.get_instance_row_bounds(B=B)
        else:
            assert _equal(s.get_instance_row_bounds(B=B), state['table'])
    i = next(k for k, r in enumerate(prob.rows) if r.kind == ROW_COORD)
    r = prob.rows[i]

    def family():
        refused(rf'{who}: batch size 4, .* 5 instances', lambda: s.forecast_row_margin(4, 2, 2.0, B=4))
        for window in (0, 33, -1):
            refused(rf'{who}: window {window}\b', lambda: s.forecast_row_margin(window, 2, 2.0))
        for degree in (-1, 3):
            refused(rf'{who}: degree {degree}\b', lambda: s.forecast_row_margin(4, degree, 2.0))
        for bad in (-1e-9, np.nan, np.inf):
            refused(rf'{who}: z=', lambda: s.forecast_row_margin(4, 2, bad))
            refused(rf'{who}: sigma_prior=', lambda: s.forecast_row_margin(4, 2, 2.0, sigma_prior=bad))
            refused(rf'{who}: base_a=', lambda: s.forecast_row_margin(4, 2, 2.0, base=(bad, 0.0)))
            refused(rf'{who}: base_b=', lambda: s.forecast_row_margin(4, 2, 2.0, base=(0.0, bad)))
            refused(rf'{who}: d_max=', lambda: s.forecast_row_margin(4, 2, 2.0, d_max=bad))
        refused(rf'{who}: row {i}: d_max=.*cross', lambda: s.forecast_row_margin(4, 2, 2.0, d_max=0.5 * (r.ub - r.lb) + 1e-3))
        s.set_instance_observed_track(np.ascontiguousarray(O[:4]))
        refused(rf'{who}: the instance observed track was set for 4 instances and {T} columns, but the instance world track for {B} '
                rf'instances and {T} columns', lambda: s.forecast_row_margin(4, 2, 2.0))
        s.set_instance_observed_track(O)
    family()                                                        # with an empty slot: refused calls have set nothing ...
    s.forecast_row_margin(4, 2, **ARGS)
    state['table'] = _want(prob, O, None, 4, 2, **ARGS)
    assert _equal(s.get_instance_row_bounds(), state['table'])
    family()                                                        # ... and with a table in it: it stays in force
    refused(r'smpc_get_instance_row_bounds: batch size 3, .* set for 5 instances', lambda: s.get_instance_row_bounds(B=3))
    refused(r'smpc_get_instance_row_bounds: lo and hi must both be given', lambda: s._chk(s.L.smpc_get_instance_row_bounds(s.h, B, None, None, 0)))
    # the slot rule: the guarded readers refuse another B while the device-made table is set, the slot's refusers refuse it
    x0, xg, ug, p = rb.inputs(prob, B)
    with pytest.raises(EngineError, match=r'engine error -1: smpc_solve_batch: batch size 3, .* set for 5 instances \(smpc_set_instance_row_bounds'):
        s.solve(x0[:3], xg[:3], ug[:3], p[:3])
    with pytest.raises(EngineError, match=r'engine error -4: smpc_rollout_batch: an instance row-bounds table is set'):
        s.rollout(x0, xg, ug, p, 2)
    with_table = [np.array(a) for a in s.solve(x0, xg, ug, p)]
    # the setter replaces the device-made table and the device-made table the setter's
    lo0, hi0 = rb.descriptor_table(prob, B)
    s.set_instance_row_bounds(lo0, hi0)
    assert _equal(s.get_instance_row_bounds(), (lo0, hi0))
    s.forecast_row_margin(4, 2, **ARGS)
    assert _equal(s.get_instance_row_bounds(), state['table'])
    # set_horizon drops the table
    s.set_horizon(N)
    with pytest.raises(EngineError, match='no instance row-bounds table is set'):
        s.get_instance_row_bounds(B=B)
    plain = [np.array(a) for a in s.solve(x0, xg, ug, p)]
    assert not _same(plain, with_table)
    s.solve(x0[:3], xg[:3], ug[:3], p[:3])
    s.set_instance_world_track(None)
    # no rows: refused as smpc_set_instance_row_bounds refuses
    from conftest import make_problem
    par0, prob0, net0 = make_problem('st', N=N)
    prob0.desc.n_rows = 0
    s0 = _solver(prob0, net0)
    try:
        with pytest.raises(EngineError, match=r'engine error -1: smpc_forecast_row_margin: the problem has no collision rows'):
            s0.forecast_row_margin(4, 2, 2.0, B=1)
    finally:
        prob0.desc.n_rows = len(prob0.rows)


# ---- 4. capture --------------------------------------------------------------------------------------------------------------------------------
def test_growth_under_capture_is_refused_and_a_captured_margin_follows_the_clock():
    """capture as test_forecast_poly_gpu.py does it: torch's capture stream, which the engine's stream joins for the call"""
    import row_bounds_cases as rb
    import torch
    from safe_mpc_amd._lib import EngineError
    N, B, T = 4, 5, 12
    par, prob, net = mc.problem('z1', N)
    s = _solver(prob, net, 'throughput')
    x0, xg, ug, p = rb.inputs(prob, B)
    dev_in = [_dev(a) for a in (x0, xg, ug, p)]
    W, O = fc.world(prob, B, T, amp=0.002), fc.world(prob, B, T, seed=4, amp=0.002)
    kw = dict(z=2.0, sigma_prior=0.0, base=(0.001, 0.0), d_max=0.03)
    cell = fc.cell(1)
    torch.cuda.synchronize()
    s.set_scene_clock(cell)
    s.set_instance_world_track(_dev(W))
    s.set_instance_observed_track(_dev(O))
    s.forecast_scene_poly(4, 2)                                     # (the scene buffer exists; the row-bounds buffer does not)
    with pytest.raises(EngineError, match=r'engine error -4: smpc_forecast_row_margin: the instance row-bounds table must grow .* while '
                                          r'the stream is being captured'), warnings.catch_warnings():
        warnings.filterwarnings('ignore', 'The CUDA Graph is empty')
        with torch.cuda.graph(torch.cuda.CUDAGraph()):
            s.forecast_row_margin(4, 2, **kw)
    torch.cuda.synchronize()
    with pytest.raises(EngineError, match='no instance row-bounds table is set'):
        s.get_instance_row_bounds(B=B)
    eager = {}
    for c in (1, 7):
        cell.fill_(c)
        s.forecast_scene_poly(4, 2)
        s.forecast_row_margin(4, 2, **kw)
        res = s.solve(*dev_in)
        s.sync()
        eager[c] = [a.cpu().numpy().copy() for a in res]
        assert _equal(s.get_instance_row_bounds(), _want(prob, O, c, 4, 2, **kw))
    assert not np.array_equal(eager[1][1], eager[7][1])
    cell.fill_(1)
    out = tuple(torch.empty_like(a) for a in res)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        s.forecast_scene_poly(4, 2)
        s.forecast_row_margin(4, 2, **kw)
        s.solve(*dev_in, out=out)
    for c in (7, 1):
        cell.fill_(c)
        g.replay()
        torch.cuda.synchronize()
        assert all(np.array_equal(o.cpu().numpy(), w) for o, w in zip(out, eager[c])), c
        assert _equal(s.get_instance_row_bounds(), _want(prob, O, c, 4, 2, **kw))
    s.set_instance_row_bounds(None)
    s.set_instance_world_track(None)
    s.set_scene_clock(None)


# ---- 5. the closed loop -------------------------------------------------------------------------------------------------------------------------
def test_device_loop_with_a_fitted_margin_equals_the_host_loop():
    """run_mpc(on_device=True, forecast='fit', row_margin_fit=...) against on_device=False (the statement and the setter per step) on
    the case of test_forecast_fit_gpu.py: equal index lists and x within 1e-6, that file's comparison and tolerance.  An abort event
    must occur, so that the backup handle's call has run; the run without the argument has other bits."""
    from safe_mpc_amd import closed_loop as cl
    from test_forecast_fit_gpu import _loop_case
    par, xg, ug, world, observed, steps = _loop_case()
    kw = dict(n_steps=steps, scenes=world, forecast='fit', forecast_window=4, observed=observed, row_margin=(0.002, 0.001))
    fit = (2.0, 1e-3, 0.04)
    dev = cl.run_mpc(par, 'htwa', xg, ug, on_device=True, groups=1, row_margin_fit=fit, **kw)
    host = cl.run_mpc(par, 'htwa', xg, ug, on_device=False, row_margin_fit=fit, **kw)
    assert dev['row_margin_fit'] == host['row_margin_fit'] == fit
    print('abort events: x_viable', dev['x_viable'].shape, host['x_viable'].shape, 'collisions', dev['collisions_idx'])
    assert dev['x_viable'].shape[0] > 0 and dev['x_viable'].shape == host['x_viable'].shape
    for k in ('conv_idx', 'collisions_idx', 'unconv_idx'):
        assert dev[k] == host[k], k
    assert sorted(dev['viable_idx']) == sorted(host['viable_idx'])
    assert np.array_equal(np.isnan(dev['x']), np.isnan(host['x']))
    err = np.nanmax(np.abs(dev['x'] - host['x']))
    print(f'fitted margin: device loop against host loop, max |x| error {err:.3e}')
    assert err < 1e-6
    plain = cl.run_mpc(par, 'htwa', xg, ug, on_device=True, groups=1, **kw)
    assert not np.array_equal(plain['u'], dev['u'], equal_nan=True)      # (the loop's solves did read the fitted table)


def test_device_loop_with_z_zero_and_no_base_is_the_loop_without_the_argument():
    from safe_mpc_amd import closed_loop as cl
    from test_forecast_fit_gpu import _loop_case
    par, xg, ug, world, observed, steps = _loop_case()
    kw = dict(n_steps=steps, on_device=True, groups=1, scenes=world, forecast='fit', forecast_window=4, observed=observed)
    a = cl.run_mpc(par, 'htwa', xg, ug, row_margin_fit=(0.0, 0.0, 0.04), **kw)
    b = cl.run_mpc(par, 'htwa', xg, ug, **kw)
    for k in ('x', 'u', 'x_viable', 'r_receding'):
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    for k in ('conv_idx', 'collisions_idx', 'unconv_idx', 'viable_idx'):
        assert a[k] == b[k], k
