"""Obstacle forecasts from a Kalman filter on the engine (smpc_forecast_scene_kalman, k_scene_kalman; smpc_kalman_row_margin,
k_kalman_margin).  -m gpu only.  problem.kalman_statement / kalman_margin_statement are the definition and numpy
the reference, never the kernel.

0. the ONE division and the square roots: after three advances on inputs with full mantissas the state read back from the state tensor
   (the gains went through the division) and d read through a plane row with lb = 0 equal numpy's bits.  They do, so everything below
   is bit for bit.
1. the kernel against the statement, the state carried on the device and on the host over 12 consecutive steps: B in {1, 5, 23}, N in
   {1, 4, 63}, T in {2, 40}, degrees 0..2, with and without an observed track, a NaN burst from step 0 and one mid-run, advance=False,
   every instance alone, twice from the same copied state, -0.0 at degree 0, the fp32 context rows; the margin through
   get_instance_row_bounds at every step, the cap, z = 0, a NaN in the state
2. rows of a subset imported into a second handle with another horizon
3. what reads the slots: F as a table in eval_nodes, stage records and the solve in both QP forms; the margin table against the setter
4. every refusal by name with the scene slot, the row-bounds slot and the state tensor unchanged
5. growth under capture; a graph of [forecast_scene_kalman; kalman_row_margin; solve] replayed three times equals three eager steps
6. the device loop against the host loop on turning_scenes with dropouts and an abort event"""
import warnings

import numpy as np
import pytest

import forecast_cases as fc
import kalman_cases as kc
from conftest import make_problem_fr7
from safe_mpc_amd.problem import (KALMAN_N, KALMAN_P, KALMAN_REC, KALMAN_S2, ROW_COORD, inflated_row_bounds, kalman_margin_statement,
                                  kalman_params, kalman_statement, scene_column, scene_context)
from test_forecast_gpu import CTX_MEAN, CTX_STD, SELECT, _calls, _dev, _same
from test_forecast_gpu import _solver as _ctx_solver
from test_row_bounds_gpu import _solver

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _equal(got, want):
    return all(np.array_equal(_bits(np.asarray(g)), _bits(w)) for g, w in zip(got, want))


def _host(t):
    return t.cpu().numpy().copy()


def _step(s, cell, c, par, state, select=None):
    """one advancing forecast at clock c: (F, ctx) as the slots hold them"""
    cell.fill_(c)
    s.forecast_scene_kalman(par, state, True, select)
    info, F, ctx = fc.read_slots(s)
    assert info['scene_B'] == state.shape[0] and info['scene_T'] == s.N + 1 and info['scene_fc'] == 1, info
    return F, ctx


def _table(prob, st, par, **kw):
    return inflated_row_bounds(prob, st.shape[0], kalman_margin_statement(prob, st, par, **kw))


def _clocked(s):
    import torch
    cell = fc.cell(0)
    torch.cuda.synchronize()
    s.set_scene_clock(cell)
    return cell


# ---- 0. the division and the square roots ---------------------------------------------------------------------------------------------------
def test_the_one_division_and_the_square_roots_are_correctly_rounded():
    """Everything in k_scene_kalman but ONE division, and everything in k_kalman_margin but two square roots per node, is add, multiply
    and select in the statement's order.  Three advances from the all-zero state on a world with full mantissas in all eight slots
    (forecast_cases.world), B = 23, the three degrees: the second and third divide, and every number of the state but n goes through
    the gains -- 23 x 4 x 31 doubles per degree read back from the state tensor.  Then a plane row whose lower side is 0.0 and whose
    upper side is absent gets lo = 0.0 + d = d, so the table hands back d itself: sqrt(s2) sqrt(Pi_k[0][0]) with z = 1, no base and the
    cap out of the way, N = 63 -- 64 radicands per record.  numpy's division and sqrt are IEEE 754's, so equality of every bit means the
    device's are correctly rounded on these; the figures are printed before the assertion."""
    N, B, T = 63, 23, 40
    par_, prob, net = make_problem_fr7('constraint_everywhere', N=N)
    i = next(k for k, r in enumerate(prob.rows) if r.kind == ROW_COORD)
    prob.rows[i].lb = prob.desc.rows[i].lb = prob.row_lb[i] = 0.0
    assert abs(prob.rows[i].ub) >= 1e5
    s = _solver(prob, net)
    S = fc.world(prob, B, T, seed=5, amp=0.05)
    s.set_instance_world_track(_dev(S))
    cell = _clocked(s)
    n, wrong, worst, nd, wrong_d, worst_d = 0, 0, 0.0, 0, 0, 0.0
    for p in kc.DEGREES:
        par = kalman_params(p, kc.PAR[p].q, kc.PAR[p].r, kc.PAR[p].v0, kc.PAR[p].a0, 0.25)
        state, st = s.new_kalman_state(B), np.zeros((B, len(prob.rows), KALMAN_REC))
        for c in (3, 4, 5):
            F, _ = _step(s, cell, c, par, state)
            st, want = kalman_statement(st, S[:, c], kc.kinds(prob), par, N)
            got = _host(state)
            n += got.size
            wrong += int((_bits(got) != _bits(st)).sum()) + int((_bits(F) != _bits(want)).sum())
            with np.errstate(all='ignore'):
                worst = max(worst, float(np.nanmax(np.where(st != 0, np.abs(got - st) / np.spacing(np.abs(st)), 0.0))))
            d = kalman_margin_statement(prob, st, par, 1.0, (0.0, 0.0), 1e3)[:, :, i]
            s.kalman_row_margin(par, state, 1.0, (0.0, 0.0), 1e3)
            lo, hi = s.get_instance_row_bounds()
            assert (hi[:, :, i] == prob.row_ub[i]).all() and d.min() > 0.0
            nd += d.size
            wrong_d += int((_bits(lo[:, :, i]) != _bits(d)).sum())
            worst_d = max(worst_d, float((np.abs(lo[:, :, i] - d) / np.spacing(d)).max()))
    print(f'state through the device\'s division against numpy: {wrong} of {n} values differ, worst {worst:.2f} ulp; '
          f'd through its square roots: {wrong_d} of {nd} differ, worst {worst_d:.2f} ulp')
    assert wrong == 0 and wrong_d == 0
    s.set_instance_world_track(None)
    s.set_instance_row_bounds(None)
    s.set_scene_clock(None)


# ---- 1. the kernel equals the statement ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('system,N,B', [('z1', 4, 5), ('z1', 63, 23), ('z1', 1, 1), ('fr7', 4, 23), ('fr7', 1, 5), ('fr7', 63, 1)])
def test_kernel_equals_statement_over_twelve_steps(system, N, B):
    """B = 1 is four lanes of a wavefront, B = 5 a partial one, B = 23 with six rows 552 lanes: records straddle blocks.  The first
    instance sees nothing in columns 0 and 1 (n stays 0: the record stays all zero and F is zero), the last loses columns 5..8; with
    T = 2 the clock runs past the track's end.  NaN tables go on by device pointer (host pointers are validated)."""
    par_, prob, net = kc.problem(system, N)
    s = _solver(prob, net)
    nr, kinds = len(prob.rows), kc.kinds(prob)
    cell = _clocked(s)
    for T in (2, 40):
        W = kc.bursts(prob, fc.world(prob, B, T, seed=T), [(0, 0, 2), (B - 1, 5, 9)])
        O = kc.bursts(prob, fc.world(prob, B, T, seed=T + 11), [(0, 0, 2), (B - 1, 5, 9)])
        W[..., 7] = -0.0                                                    # (a slot no row kind reads: -0.0 must stay one at degree 0)
        for observed in (False, True):
            s.set_instance_world_track(_dev(W))
            s.set_instance_observed_track(_dev(O) if observed else None)
            S = O if observed else W
            for p in kc.DEGREES:
                par = kc.PAR[p]
                state, st = s.new_kalman_state(B), np.zeros((B, nr, KALMAN_REC))
                for c in range(12):
                    F, _ = _step(s, cell, c, par, state)
                    if c == 6:
                        snap = state.clone()
                    st, want = kalman_statement(st, S[:, scene_column(c, T)], kinds, par, N)
                    assert F.shape == (B, N + 1, nr, 8)
                    assert np.array_equal(_bits(F), _bits(want)), (T, observed, p, c)
                    assert np.array_equal(_bits(_host(state)), _bits(st)), (T, observed, p, c)
                    if p == 0 and not observed and T == 40 and c in (0, 2):
                        # first seen (instance 0 at column 2, the others at column 0): pos = y = -0.0, stored N + 1 times.  (One
                        # update later it is 0.0 in the statement too: -0.0 + K 0.0.)
                        first = F[:1] if c == 2 else F[1:]
                        assert np.signbit(first[:, :, :, 7]).all() and (first[:, :, :, 7] == 0.0).all()
                    if c in (0, 1, 7, 11):
                        s.kalman_row_margin(par, state, **kc.MARGIN)
                        assert _equal(s.get_instance_row_bounds(), _table(prob, st, par, **kc.MARGIN)), (T, observed, p, c)
                # advance=False: the same forecast from the state as it is, the state untouched, whatever the clock says
                cell.fill_(3)
                s.forecast_scene_kalman(par, state, False)
                assert np.array_equal(_bits(fc.read_slots(s)[1]), _bits(want)) and np.array_equal(_bits(_host(state)), _bits(st))
                # twice from the same copied state: the same bits
                a, b = snap.clone(), snap.clone()
                Fa, _ = _step(s, cell, 7, par, a)
                Fb, _ = _step(s, cell, 7, par, b)
                assert np.array_equal(_bits(Fa), _bits(Fb)) and np.array_equal(_bits(_host(a)), _bits(_host(b)))
    s.set_instance_world_track(None)
    s.set_instance_row_bounds(None)
    s.set_scene_clock(None)


@pytest.mark.parametrize('system', ['z1', 'fr7'])
def test_every_instance_alone_the_cap_z_zero_and_a_nan_state(system):
    N, B, T = 4, 23, 40
    par_, prob, net = kc.problem(system, N)
    s = _solver(prob, net)
    kinds = kc.kinds(prob)
    cell = _clocked(s)
    O = kc.bursts(prob, fc.world(prob, B, T, seed=14), [(3, 4, 6)])
    W = fc.world(prob, B, T, seed=3)
    par = kc.PAR[2]
    runs = kc.run_statement(prob, O, par, N, range(8))
    s.set_instance_world_track(W)
    s.set_instance_observed_track(_dev(O))
    state = s.new_kalman_state(B)
    for c in range(8):
        F, _ = _step(s, cell, c, par, state)
    assert np.array_equal(_bits(F), _bits(runs[-1][1])) and np.array_equal(_bits(_host(state)), _bits(runs[-1][0]))
    for b in range(B):
        s.set_instance_world_track(W[b:b + 1])
        s.set_instance_observed_track(_dev(O[b:b + 1]))
        one = s.new_kalman_state(1)
        for c in range(8):
            F1, _ = _step(s, cell, c, par, one)
        assert np.array_equal(_bits(F1), _bits(F[b:b + 1])) and np.array_equal(_bits(_host(one)), _bits(_host(state)[b:b + 1])), b
        s.kalman_row_margin(par, one, **kc.MARGIN)
        assert _equal(s.get_instance_row_bounds(), [a[b:b + 1] for a in _table(prob, runs[-1][0], par, **kc.MARGIN)]), b
    st = runs[-1][0]
    # the cap reached by size; z = 0 gives the base -- run_mpc(row_margin=base)'s table --, and with no base the descriptor's doubles
    kw = dict(z=50.0, base=(0.0, 0.0), d_max=0.01)
    s.kalman_row_margin(par, state, **kw)
    assert _equal(s.get_instance_row_bounds(), _table(prob, st, par, **kw)) and (kalman_margin_statement(prob, st, par, **kw) == 0.01).any()
    s.kalman_row_margin(par, state, 0.0, kc.MARGIN['base'], 0.04)
    assert _equal(s.get_instance_row_bounds(), inflated_row_bounds(prob, B, kc.MARGIN['base'][0] + kc.MARGIN['base'][1] * np.arange(N + 1)))
    s.kalman_row_margin(par, state, 0.0, (0.0, 0.0), 0.04)
    lo, hi = s.get_instance_row_bounds()
    assert _equal((lo, hi), (np.broadcast_to(prob.row_lb, lo.shape), np.broadcast_to(prob.row_ub, hi.shape)))
    # a NaN in the state gives the cap and never a NaN bound
    bad = st.copy()
    bad[2, 0, KALMAN_P], bad[4, -1, KALMAN_S2] = np.nan, np.nan
    s.kalman_row_margin(par, _dev(bad), **kc.MARGIN)
    got = s.get_instance_row_bounds()
    assert _equal(got, _table(prob, bad, par, **kc.MARGIN)) and np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
    d = kalman_margin_statement(prob, bad, par, **kc.MARGIN)
    assert (d[2, :, 0] == kc.MARGIN['d_max']).all() and (d[4, :, -1] == kc.MARGIN['d_max']).all()
    s.set_instance_world_track(None)
    s.set_instance_row_bounds(None)
    s.set_scene_clock(None)


def test_context_rows_equal_the_statement_in_fp32():
    N = 4
    s, prob = _ctx_solver('z1', N, ctx=True)
    cell = _clocked(s)
    for B, T in ((5, 40), (23, 2), (1, 1)):
        W = fc.world(prob, B, T, seed=3)
        s.set_instance_world_track(_dev(W))
        for p in kc.DEGREES:
            state, st = s.new_kalman_state(B), np.zeros((B, len(prob.rows), KALMAN_REC))
            for c in range(4):
                got_F, got = _step(s, cell, c, kc.PAR[p], state, SELECT)
                st, F = kalman_statement(st, W[:, scene_column(c, T)], kc.kinds(prob), kc.PAR[p], N)
                want = ((scene_context(F, SELECT) - CTX_MEAN) / CTX_STD).astype(np.float32)
                info = fc.read_slots(s)[0]
                assert info['ctx_B'] == B and info['ctx_T'] == N + 1 and info['ctx_fc'] == 1, info
                assert np.array_equal(_bits(got_F), _bits(F)) and got.shape == (B, N + 1, 2)
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (B, T, p, c)
    s.set_instance_world_track(None)
    s.set_scene_clock(None)


# ---- 2. rows into a second handle ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('system', ['z1', 'fr7'])
def test_rows_of_a_subset_in_a_second_handle_with_another_horizon(system):
    """what the backup handle of an abort event does: no world on it, advance=False on the gathered rows, its own N"""
    import torch
    N, Nb, B, T = 4, 7, 23, 40
    par_, prob, net = kc.problem(system, N)
    parb, probb, netb = kc.problem(system, Nb)
    s, sb = _solver(prob, net), _solver(probb, netb)
    cell = _clocked(s)
    W = fc.world(prob, B, T, seed=8)
    s.set_instance_world_track(_dev(W))
    par = kc.PAR[1]
    state = s.new_kalman_state(B)
    for c in range(5):
        _step(s, cell, c, par, state)
    st = kc.run_statement(prob, W, par, N, range(5))[-1][0]
    rows = [17, 2, 9]
    part = state[torch.tensor(rows, device='cuda:0')]
    sb.forecast_scene_kalman(par, part, advance=False)
    sb.kalman_row_margin(par, part, **kc.MARGIN)
    info, F, _ = fc.read_slots(sb)
    _, want = kalman_statement(st[rows], None, kc.kinds(prob), par, Nb, advance=False)
    assert info['scene_B'] == 3 and info['scene_T'] == Nb + 1 and info['scene_fc'] == 1
    assert np.array_equal(_bits(F), _bits(want)) and _equal(sb.get_instance_row_bounds(), _table(probb, st[rows], par, **kc.MARGIN))
    assert np.array_equal(_bits(_host(part)), _bits(st[rows]))
    s.set_instance_world_track(None)
    s.set_scene_clock(None)


# ---- 3. what reads the slots ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('system,N,ctx', [('z1', 4, False), ('z1', 4, True), ('fr7', 4, False)])
def test_the_slots_are_read_as_the_statement_set_as_tables(system, N, ctx):
    from conftest import constant_guess, sample_instances
    B, T = 5, 12
    s, prob = _ctx_solver(system, N, ctx)
    select = SELECT if ctx else None
    x0 = sample_instances(prob, B, seed=1, vel_scale=0.5)
    xg, ug, p = constant_guess(prob, x0)
    rng = np.random.default_rng(0)
    xg[:, 1:] += 0.05 * rng.standard_normal(xg[:, 1:].shape)
    ug += rng.uniform(-5, 5, ug.shape)
    inputs = (x0, xg, ug, p)
    W = fc.world(prob, B, T, amp=0.002)
    par = kc.PAR[2]
    runs = kc.run_statement(prob, W, par, N, range(6))
    kw = dict(z=2.0, base=(0.001, 0.0), d_max=0.03)
    plain = _calls(s, N, inputs)
    refs = []
    for st, F in (runs[2], runs[5]):
        s.set_scene_clock(None)
        if ctx:
            s.set_instance_context_track(scene_context(F, SELECT))
        s.set_instance_scene_track(F)
        s.set_instance_row_bounds(*_table(prob, st, par, **kw))
        refs.append(_calls(s, N, inputs))
    assert _same(refs[0], refs[1]) and _same(refs[0], plain)                   # (the tables are read)
    s.set_instance_scene_track(None)
    s.set_instance_row_bounds(None)
    cell = _clocked(s)
    s.set_instance_world_track(_dev(W))
    state = s.new_kalman_state(B)
    for c in range(6):
        cell.fill_(c)
        s.forecast_scene_kalman(par, state, True, select)
        s.kalman_row_margin(par, state, **kw)
        if c in (2, 5):
            assert _same(_calls(s, N, inputs), refs[c // 3]) == [], c
    s.set_instance_world_track(None)
    s.set_instance_row_bounds(None)
    s.set_scene_clock(None)


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_by_name_leaves_the_slots_and_the_state_unchanged():
    import ctypes as C
    import row_bounds_cases as rb
    from safe_mpc_amd._lib import EngineError
    from safe_mpc_amd.problem import KalmanParams
    N, B, T = 4, 5, 8
    par_, prob, net = kc.problem('fr7', N)
    s = _solver(prob, net, 'throughput')
    W, O = fc.world(prob, B, T), fc.world(prob, B, T, seed=4)
    fk, km = 'smpc_forecast_scene_kalman', 'smpc_kalman_row_margin'
    par = kc.PAR[1]
    state = s.new_kalman_state(B)
    with pytest.raises(EngineError, match=rf'engine error -4: {fk}: no world is set'):
        s.forecast_scene_kalman(par, state)
    s.set_instance_observed_track(O)                                # (an observed track alone is no world)
    with pytest.raises(EngineError, match=rf'engine error -4: {fk}: no world is set'):
        s.forecast_scene_kalman(par, state)
    s.set_instance_world_track(W)
    keep = {'scene': None, 'table': None, 'state': _host(state)}

    def refused(match, call, code=-1):
        with pytest.raises(EngineError, match=rf'engine error {code}: {match}'):
            call()
        info, F, _ = fc.read_slots(s)
        if keep['scene'] is None:
            assert info['scene_B'] == 0
        else:
            assert info['scene_fc'] == 1 and np.array_equal(_bits(F), _bits(keep['scene']))
        if keep['table'] is None:
            with pytest.raises(EngineError, match='no instance row-bounds table is set'):
                s.get_instance_row_bounds(B=B)
        else:
            assert _equal(s.get_instance_row_bounds(B=B), keep['table'])
        assert np.array_equal(_bits(_host(state)), _bits(keep['state']))
    raw = lambda fn, *a: s._chk(fn(s.h, *a))
    rec = lambda **kw: KalmanParams(**{**dict(degree=1, reserved=0, q=0.003, r=0.01, v0=0.02, a0=0.005, beta=0.25), **kw})
    i = next(k for k, r in enumerate(prob.rows) if r.kind == ROW_COORD)
    r = prob.rows[i]

    def family():
        for who, call in ((fk, lambda rc: raw(s.L.smpc_forecast_scene_kalman, B, C.byref(rc), state.data_ptr(), 1, 0, None)),
                          (km, lambda rc: raw(s.L.smpc_kalman_row_margin, B, C.byref(rc), state.data_ptr(), 2.0, 0.0, 0.0, 0.04))):
            for degree in (-1, 3):
                refused(rf'{who}: degree {degree}\b', lambda: call(rec(degree=degree)))
            for bad in (0.0, -1e-9, np.nan, np.inf):
                refused(rf'{who}: r=', lambda: call(rec(r=bad)))
            for bad in (-1e-9, np.nan, np.inf):
                for name in ('q', 'v0', 'a0'):
                    refused(rf'{who}: {name}=', lambda: call(rec(**{name: bad})))
            for bad in (-1e-9, 1.0 + 1e-9, np.nan):
                refused(rf'{who}: beta=', lambda: call(rec(beta=bad)))
        refused(rf'{fk}: par == NULL', lambda: raw(s.L.smpc_forecast_scene_kalman, B, None, state.data_ptr(), 1, 0, None))
        refused(rf'{fk}: state == NULL', lambda: raw(s.L.smpc_forecast_scene_kalman, B, C.byref(rec()), None, 1, 0, None))
        refused(rf'{km}: par == NULL', lambda: raw(s.L.smpc_kalman_row_margin, B, None, state.data_ptr(), 2.0, 0.0, 0.0, 0.04))
        refused(rf'{km}: state == NULL', lambda: raw(s.L.smpc_kalman_row_margin, B, C.byref(rec()), None, 2.0, 0.0, 0.0, 0.04))
        refused(rf'{fk}: batch size 4, .* 5 instances', lambda: s.forecast_scene_kalman(par, state[:4].contiguous()))
        refused(rf'{fk}: bad batch size 0', lambda: raw(s.L.smpc_forecast_scene_kalman, 0, C.byref(rec()), state.data_ptr(), 0, 0, None))
        refused(rf'{km}: bad batch size 0', lambda: raw(s.L.smpc_kalman_row_margin, 0, C.byref(rec()), state.data_ptr(), 2.0, 0.0, 0.0, 0.04))
        refused(rf'{fk}: n_sel=2, but the network has no context columns', lambda: s.forecast_scene_kalman(par, state, True, [(0, 0), (1, 1)]))
        for bad in (-1e-9, np.nan, np.inf):
            refused(rf'{km}: z=', lambda: s.kalman_row_margin(par, state, bad))
            refused(rf'{km}: base_a=', lambda: s.kalman_row_margin(par, state, 2.0, base=(bad, 0.0)))
            refused(rf'{km}: base_b=', lambda: s.kalman_row_margin(par, state, 2.0, base=(0.0, bad)))
            refused(rf'{km}: d_max=', lambda: s.kalman_row_margin(par, state, 2.0, d_max=bad))
        refused(rf'{km}: row {i}: d_max=.*cross', lambda: s.kalman_row_margin(par, state, 2.0, d_max=0.5 * (r.ub - r.lb) + 1e-3))
        s.set_instance_observed_track(np.ascontiguousarray(O[:4]))
        refused(rf'{fk}: the instance observed track was set for 4 instances and {T} columns, but the instance world track for {B} '
                rf'instances and {T} columns', lambda: s.forecast_scene_kalman(par, state))
        s.set_instance_observed_track(O)
    family()                                                        # with empty slots: refused calls have set nothing ...
    s.forecast_scene_kalman(par, state)
    s.kalman_row_margin(par, state, **kc.MARGIN)
    st, F = kalman_statement(np.zeros((B, len(prob.rows), KALMAN_REC)), O[:, 0], kc.kinds(prob), par, N)
    keep.update(scene=F, table=_table(prob, st, par, **kc.MARGIN), state=st)
    assert np.array_equal(_bits(fc.read_slots(s)[1]), _bits(F)) and _equal(s.get_instance_row_bounds(), keep['table'])
    family()                                                        # ... and with a forecast and a table in them: they stay in force
    # the python layer names a state of the wrong kind before the engine sees it
    for bad in (state.float(), state[:, :, :31], state.cpu(), _host(state)):
        with pytest.raises(ValueError, match='forecast_scene_kalman: state'):
            s.forecast_scene_kalman(par, bad)
    # the slot rule: the parallel policy's refuser and rollout keep refusing both slots, whoever filled them
    x0, xg, ug, p = rb.inputs(prob, B)
    with pytest.raises(EngineError, match=r'engine error -4: smpc_rollout_batch: an instance '):
        s.rollout(x0, xg, ug, p, 2)
    s.set_instance_row_bounds(None)
    with pytest.raises(EngineError, match=r'engine error -4: smpc_rollout_batch: an instance '):
        s.rollout(x0, xg, ug, p, 2)
    # advance=False needs no world and takes any B; the margin needs none either
    s.set_instance_world_track(None)
    assert fc.read_slots(s)[0]['scene_B'] == 0                      # (the forecast went with its world)
    part = state[:3].contiguous()
    s.forecast_scene_kalman(par, part, advance=False)
    s.kalman_row_margin(par, part, **kc.MARGIN)
    assert np.array_equal(_bits(fc.read_slots(s)[1]), _bits(F[:3])) and _equal(s.get_instance_row_bounds(), [a[:3] for a in keep['table']])
    s.set_instance_scene_track(None)
    s.set_instance_row_bounds(None)
    # no rows: refused as the setters refuse
    from conftest import make_problem
    par0, prob0, net0 = make_problem('st', N=N)
    prob0.desc.n_rows = 0
    s0 = _solver(prob0, net0)
    try:
        import torch
        z = torch.zeros((1, max(len(prob0.rows), 1), KALMAN_REC), dtype=torch.float64, device='cuda:0')
        for who, call in ((km, lambda: raw0(s0.L.smpc_kalman_row_margin, 1, C.byref(rec()), z.data_ptr(), 2.0, 0.0, 0.0, 0.04)),
                          (fk, lambda: raw0(s0.L.smpc_forecast_scene_kalman, 1, C.byref(rec()), z.data_ptr(), 0, 0, None))):
            raw0 = lambda fn, *a: s0._chk(fn(s0.h, *a))
            with pytest.raises(EngineError, match=rf'engine error -1: {who}: the problem has no collision rows'):
                call()
    finally:
        prob0.desc.n_rows = len(prob0.rows)


# ---- 5. capture ----------------------------------------------------------------------------------------------------------------------------------------------
def test_growth_under_capture_is_refused_and_a_replayed_graph_is_three_eager_steps():
    """capture as test_forecast_margin_gpu.py does it: torch's capture stream, which the engine's stream joins for the call"""
    import row_bounds_cases as rb
    import torch
    from safe_mpc_amd._lib import EngineError
    N, B, T = 4, 5, 12
    s, prob = _ctx_solver('z1', N, ctx=True)
    s.set_qp_mode('throughput')
    x0, xg, ug, p = rb.inputs(prob, B)
    dev_in = [_dev(a) for a in (x0, xg, ug, p)]
    O = kc.bursts(prob, fc.world(prob, B, T, seed=4, amp=0.002), [(2, 6, 7)])
    kw = dict(z=2.0, base=(0.001, 0.0), d_max=0.03)
    par = kc.PAR[1]
    cell = _clocked(s)
    s.set_instance_world_track(_dev(fc.world(prob, B, T, amp=0.002)))
    s.set_instance_observed_track(_dev(O))
    state = s.new_kalman_state(B)

    def under_capture(call):
        with warnings.catch_warnings():
            warnings.filterwarnings('ignore', 'The CUDA Graph is empty')
            with torch.cuda.graph(torch.cuda.CUDAGraph()):
                call()
    # the scene buffer must grow; then the context buffer; then the row-bounds buffer -- each refused with nothing changed
    with pytest.raises(EngineError, match=r'engine error -4: smpc_forecast_scene_kalman: the instance scene.* must grow .* while the stream is being captured'):
        under_capture(lambda: s.forecast_scene_kalman(par, state))
    torch.cuda.synchronize()
    assert fc.read_slots(s)[0]['scene_B'] == 0 and not _host(state).any()
    s.forecast_scene_kalman(par, state, advance=False)              # (the scene buffer exists; the context buffer does not)
    with pytest.raises(EngineError, match=r'engine error -4: smpc_forecast_scene_kalman: the instance context.* must grow .* while the stream is being captured'):
        under_capture(lambda: s.forecast_scene_kalman(par, state, True, SELECT))
    torch.cuda.synchronize()
    assert fc.read_slots(s)[0]['ctx_B'] == 0 and not _host(state).any()
    with pytest.raises(EngineError, match=r'engine error -4: smpc_kalman_row_margin: the instance row-bounds table must grow .* while '
                                          r'the stream is being captured'):
        under_capture(lambda: s.kalman_row_margin(par, state, **kw))
    torch.cuda.synchronize()
    with pytest.raises(EngineError, match='no instance row-bounds table is set'):
        s.get_instance_row_bounds(B=B)
    # three eager steps at clocks 5, 6, 7 (column 6 is lost for instance 2) ...
    def warm():
        state.zero_()
        for c in range(5):
            cell.fill_(c)
            s.forecast_scene_kalman(par, state, True, SELECT)
    warm()
    eager = []
    for c in (5, 6, 7):
        cell.fill_(c)
        s.forecast_scene_kalman(par, state, True, SELECT)
        s.kalman_row_margin(par, state, **kw)
        res = s.solve(*dev_in)
        s.sync()
        eager.append([a.cpu().numpy().copy() for a in res] + [_host(state)] + list(s.get_instance_row_bounds()))
    st = kc.run_statement(prob, O, par, N, range(8))
    assert np.array_equal(_bits(eager[-1][-3]), _bits(st[-1][0])) and _equal(eager[-1][-2:], _table(prob, st[-1][0], par, **kw))
    assert not np.array_equal(eager[0][1], eager[2][1])
    # ... equal three replays of one captured [forecast_scene_kalman; kalman_row_margin; solve]: a replay is one more advance
    warm()
    out = tuple(torch.empty_like(a) for a in res)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    cell.fill_(5)
    with torch.cuda.graph(g):
        s.forecast_scene_kalman(par, state, True, SELECT)
        s.kalman_row_margin(par, state, **kw)
        s.solve(*dev_in, out=out)
    for k, c in enumerate((5, 6, 7)):
        cell.fill_(c)
        g.replay()
        torch.cuda.synchronize()
        got = [o.cpu().numpy() for o in out] + [_host(state)] + list(s.get_instance_row_bounds())
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(got, eager[k])), c
    s.set_instance_row_bounds(None)
    s.set_instance_world_track(None)
    s.set_scene_clock(None)


# ---- 6. the closed loop -------------------------------------------------------------------------------------------------------------------------------------
def test_device_loop_with_the_filter_equals_the_host_loop():
    """run_mpc(on_device=True, forecast='kalman', row_margin_kalman=...) against on_device=False (the statements and the setters per
    step) on the case of test_forecast_fit_gpu.py -- turning tracks seen through a sensor -- with dropouts on top: equal index lists and
    x within 1e-6, that file's comparison and tolerance.  An abort event must occur, so that the backup handle's calls have run; the
    run without the margin has other bits."""
    from safe_mpc_amd import closed_loop as cl
    from safe_mpc_amd.problem import occlude_tracks
    from test_forecast_fit_gpu import _loop_case
    from conftest import make_problem
    par, xg, ug, world, observed, steps = _loop_case()
    prob = make_problem('htwa', N=8)[1]
    occl = occlude_tracks(prob, observed, 0.15, 2.0, seed=3)
    occl[:, 0] = observed[:, 0]                                         # (every obstacle is seen once before it can be lost)
    assert np.isnan(occl[:, 1:steps]).any()
    kw = dict(n_steps=steps, scenes=world, forecast='kalman', forecast_degree=1, kalman=(0.002, 0.001, 0.003, 0.0, 0.1), observed=occl,
              row_margin=(0.002, 0.001))
    rmk = (2.0, 0.04)
    dev = cl.run_mpc(par, 'htwa', xg, ug, on_device=True, groups=1, row_margin_kalman=rmk, **kw)
    host = cl.run_mpc(par, 'htwa', xg, ug, on_device=False, row_margin_kalman=rmk, **kw)
    assert dev['row_margin_kalman'] == host['row_margin_kalman'] == rmk and dev['kalman'] == host['kalman'] == (0.002, 0.001, 0.003, 0.0, 0.1)
    print('abort events: x_viable', dev['x_viable'].shape, host['x_viable'].shape, 'collisions', dev['collisions_idx'])
    assert dev['x_viable'].shape[0] > 0 and dev['x_viable'].shape == host['x_viable'].shape
    for k in ('conv_idx', 'collisions_idx', 'unconv_idx'):
        assert dev[k] == host[k], k
    assert sorted(dev['viable_idx']) == sorted(host['viable_idx'])
    assert np.array_equal(np.isnan(dev['x']), np.isnan(host['x']))
    err = np.nanmax(np.abs(dev['x'] - host['x']))
    print(f'filter and margin: device loop against host loop, max |x| error {err:.3e}')
    assert err < 1e-6
    plain = cl.run_mpc(par, 'htwa', xg, ug, on_device=True, groups=1, **kw)
    assert not np.array_equal(plain['u'], dev['u'], equal_nan=True)      # (the loop's solves did read the filter's table)
