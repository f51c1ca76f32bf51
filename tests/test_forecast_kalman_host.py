"""Obstacle forecasts from a Kalman filter (smpc_forecast_scene_kalman, smpc_kalman_row_margin; problem.kalman_statement,
kalman_margin_statement, occlude_tracks) without a GPU:

1. the statement against a scalar restatement in Python floats, bit for bit; the recursion in exact rationals against the least-squares
   problem it solves; the float statement against the rational one within a running bound
2. occlusion: predict-only, growth over a burst, a NaN in a slot that does not move, a robot-robot row; the identities of the margin
3. the statistical claims: the normalised innovation and the forecast error against the predicted covariance; the innovation scale
4. the host loop around the recording double, occlude_tracks, the ValueErrors and SystemExits, suffixes, flags, symbols, ABI version"""
import ctypes
import os
import pickle
import re
from fractions import Fraction

import numpy as np
import pytest

import forecast_cases as fc
import kalman_cases as kc
import margin_cases as mc
import track_cases as tc
from conftest import ROOT, sample_instances
from safe_mpc_amd import closed_loop as cl
from safe_mpc_amd import controller as C
from safe_mpc_amd.problem import (FIT_MARGIN_CAP, KALMAN_N, KALMAN_P, KALMAN_REC, KALMAN_S2, ROW_COORD, ROW_SEG_SEG, inflated_row_bounds,
                                  kalman_margin_statement, kalman_params, kalman_predict_cov, kalman_statement, moving_slots,
                                  observe_tracks, occlude_tracks, scene_column)
from test_forecast_host import LOOP_N, _loop_setup, _same_events, _script


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ---- 1. restatement, exact values ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('system', ['z1', 'fr7'])
@pytest.mark.parametrize('T', [1, 2, 8, 40])
def test_statement_equals_the_scalar_restatement_bit_for_bit(system, T):
    """14 consecutive steps from the all-zero state, degrees 0..2, T in {1, 2, N + 4, 40} (the clock runs past the end of the shorter
    tracks), both arms -- all four moving-slot sets --, worlds with full mantissas in all eight slots, a NaN burst from step 0 (n stays
    0), one mid-run, and a NaN in slot 7, which no row kind reads as moving; with and without advance"""
    N, B = 4, 3
    par_, prob, net = kc.problem(system, N)
    S = kc.bursts(prob, fc.world(prob, B, T, seed=2), [(1, 0, 2), (2, 5, 9)])
    S[0, :, :, 7] = np.nan
    kinds = kc.kinds(prob)
    for p in kc.DEGREES:
        par = kc.PAR[p]
        st = np.zeros((B, len(prob.rows), KALMAN_REC))
        recs = [[[0.0] * KALMAN_REC for _ in prob.rows] for _ in range(B)]
        for c in range(14):
            y = S[:, scene_column(c, T)]
            st, F = kalman_statement(st, y, kinds, par, N)
            assert st.shape == (B, len(prob.rows), KALMAN_REC) and F.shape == (B, N + 1, len(prob.rows), 8) and F.dtype == np.float64
            same, F0 = kalman_statement(st, None, kinds, par, N, advance=False)
            assert np.array_equal(_bits(same), _bits(st)) and np.array_equal(_bits(F0), _bits(F))
            d = kalman_margin_statement(prob, st, par, **kc.MARGIN)
            for b in range(B):
                for i, r in enumerate(prob.rows):
                    recs[b][i] = kc.step_scalar(recs[b][i], y[b, i], r.kind, par)
                    assert np.array_equal(_bits(st[b, i]), _bits(np.array(recs[b][i]))), (p, c, b, i)
                    assert np.array_equal(_bits(F[b, :, i]), _bits(kc.forecast_scalar(recs[b][i], p, N))), (p, c, b, i)
                    assert np.array_equal(_bits(d[b, :, i]), _bits(kc.margin_scalar(recs[b][i], r.kind, par, N, **kc.MARGIN))), (p, c, b, i)
        n = st[:, :, KALMAN_N]
        # n counts the observed steps: instance 1 saw nothing in columns 0 and 1 -- with T <= 2 it never does --, instance 2 lost columns
        # 5..8 where there are any (with T = 8 the clock past the end keeps reading the lost column 7)
        cols = [scene_column(c, T) for c in range(14)]
        assert (n[0] == 14).all() and (n[1] == sum(c >= 2 for c in cols)).all() and (n[2] == sum(not 5 <= c < 9 for c in cols)).all()
        assert (n[1] == (0 if T <= 2 else 12)).all() and (n[2] == {1: 14, 2: 14, 8: 5, 40: 10}[T]).all()
        # the absent components were never written beyond zero
        assert not st[:, :, 8 * (p + 1):24].any()


def test_the_filter_is_the_least_squares_problem_in_exact_rationals():
    """q = 0: after n observed samples the state is the minimiser of sum_j (y_j - f(-j))^2 / r^2 + vel_init^2 / v0^2 + acc_init^2 / a0^2
    and P the inverse of that problem's normal matrix -- the recursion in Fractions against a rational solve, equal exactly, for
    n = 1..12 and p = 0..2; p = 0 is the running mean with P00 = r^2 / n"""
    rng = np.random.default_rng(0)
    ys = [Fraction(int(v), 64) for v in rng.integers(-50, 50, 12)]
    r, v0, a0 = Fraction(1, 8), Fraction(1, 4), Fraction(1, 16)
    where = {(0, 0): 0, (0, 1): 1, (0, 2): 2, (1, 1): 3, (1, 2): 4, (2, 2): 5}
    for p in kc.DEGREES:
        for n in range(1, 13):
            x, P = kc.rational_filter(ys[:n], p, 0, r, v0, a0)
            xl, inv = kc.rational_least_squares(ys[:n], p, r, v0, a0)
            assert x[:p + 1] == xl and x[p + 1:] == [0] * (2 - p), (p, n)
            for (i, j), k in where.items():
                assert P[k] == (inv[i][j] if j <= p else 0), (p, n, i, j)
            if p == 0:
                assert x[0] == sum(ys[:n]) / n and P[0] == r * r / n


def test_the_float_statement_against_the_rational_recursion_within_its_running_bound():
    """The statement in float64 against the same recursion in exact rationals (q > 0 now).  The bound is carried operation by
    operation (kalman_cases.Err: every rounded sum, product and the one division adds u times its result to the propagated errors of
    its operands, u = 2^-53, no first-order shortcut) through the statement's own operations in their order -- so it follows from the
    operation count and nothing else; it is loose where P - K P cancels (printed: the share of the bound that is used)."""
    rng = np.random.default_rng(1)
    ys = [float(v) / 64 for v in rng.integers(-50, 50, 12)]
    q, r, v0, a0 = 0.25, 0.125, 0.25, 0.0625
    worst = 0.0
    for p in kc.DEGREES:
        par = kalman_params(p, q, r, v0, a0, 0.0)
        st = np.zeros((1, 1, KALMAN_REC))
        for n in range(1, 13):
            y = np.full((1, 1, 8), ys[n - 1])
            st, _ = kalman_statement(st, y, [ROW_COORD], par, 1)
            xe, Pe = kc.rational_filter(ys[:n], p, q, r, v0, a0, num=kc.Err)
            got = [st[0, 0, 6], st[0, 0, 14], st[0, 0, 22]] + list(st[0, 0, KALMAN_P:KALMAN_P + 6])
            for g, e in zip(got, xe + Pe):
                err = abs(Fraction(float(g)) - e.val)
                assert err <= Fraction(e.err), (p, n, float(err), e.err)                # |float - exact| <= the running bound
                if e.err:
                    worst = max(worst, float(err) / e.err)
    print(f'float statement against exact rationals: at most {worst:.3g} of the running bound is used')


# ---- 2. occlusion and identities --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('system', ['z1', 'fr7'])
def test_occlusion_is_predict_only_and_the_margin_grows_over_a_burst(system):
    N, B, T = 4, 2, 40
    par_, prob, net = kc.problem(system, N)
    W = fc.world(prob, B, T, seed=3, amp=0.002)
    S = kc.bursts(prob, W, [(1, 12, 18)])
    kinds = kc.kinds(prob)
    for p in kc.DEGREES:
        par = kalman_params(kc.PAR[p].degree, kc.PAR[p].q, kc.PAR[p].r, kc.PAR[p].v0, kc.PAR[p].a0, 0.0)     # (beta = 0: s2 stays 1, so d follows P alone)
        runs = kc.run_statement(prob, S, par, N, range(24))
        free = kc.run_statement(prob, W, par, N, range(24))
        d = [kalman_margin_statement(prob, st, par, 2.0, (0.0, 0.0), 0.5) for st, _ in runs]
        for c in range(12, 18):
            before, (st, F) = runs[c - 1][0], runs[c]
            # an unobserved step equals predict-only: the state moved by the transition, P by kalman_predict_cov, s2 and n untouched
            Q = __import__('safe_mpc_amd.problem', fromlist=['kalman_noise']).kalman_noise(par)[0]
            Pm = kalman_predict_cov(p, tuple(before[1, :, KALMAN_P + i] for i in range(6)), Q)
            for i in range(6):
                assert np.array_equal(_bits(st[1, :, KALMAN_P + i]), _bits(Pm[i]))
            assert np.array_equal(st[1, :, KALMAN_S2], before[1, :, KALMAN_S2]) and np.array_equal(st[1, :, KALMAN_N], before[1, :, KALMAN_N])
            pos, vel, acc = before[1, :, 0:8], before[1, :, 8:16], before[1, :, 16:24]
            want = pos if p == 0 else (pos + vel if p == 1 else (pos + vel) + 0.5 * acc)
            assert np.array_equal(_bits(st[1, :, 0:8]), _bits(want))
            if p < 2:                                   # (pos- is last step's F[1]; at p = 2 that one sums in another order)
                assert np.array_equal(_bits(want), _bits(runs[c - 1][1][1, 1]))
            # P00 and d_k do not decrease over the burst (q > 0: they grow)
            assert (st[1, :, KALMAN_P] > before[1, :, KALMAN_P]).all() and (d[c][1] >= d[c - 1][1]).all() and (d[c][1, 0] > d[c - 1][1, 0]).all()
            # ... and the other instance is not touched by its neighbour's burst
            assert np.array_equal(_bits(st[0]), _bits(free[c][0][0]))
        # seen again: they shrink
        assert (runs[18][0][1, :, KALMAN_P] < runs[17][0][1, :, KALMAN_P]).all() and (d[18][1] <= d[17][1]).all() and (d[18][1, 0] < d[17][1, 0]).all()
        assert (runs[18][0][1, :, KALMAN_N] == runs[17][0][1, :, KALMAN_N] + 1).all()
        # along the horizon the margin grows too (the obstacle may turn), and it never is a NaN
        assert (d[20][:, 1:] >= d[20][:, :-1]).all() and np.isfinite(np.array(d)).all()


def test_a_nan_in_a_slot_that_does_not_move_a_robot_row_and_a_nan_state():
    N, B, T = 4, 2, 12
    par_, prob, net = kc.problem('fr7', N)
    robot = mc.with_robot_row(prob)
    kinds = kc.kinds(prob) + [ROW_SEG_SEG]
    W = np.concatenate([fc.world(prob, B, T, seed=1), np.full((B, T, 1, 8), np.nan)], axis=2)      # the robot row: NaN everywhere
    Wn = W.copy()
    for i, r in enumerate(prob.rows):
        for s_ in set(range(8)) - set(moving_slots(r.kind)):
            Wn[:, :, i, s_] = np.nan
    par = kc.PAR[1]
    st = stn = np.zeros((B, len(kinds), KALMAN_REC))
    for c in range(6):
        st, F = kalman_statement(st, W[:, c], kinds, par, N)
        stn, Fn = kalman_statement(stn, Wn[:, c], kinds, par, N)
    assert (stn[:, :, KALMAN_N] == 6).all() and (st[:, :, KALMAN_N] == 6).all()              # never unobserved, the robot row included
    assert np.array_equal(_bits(stn[:, :, KALMAN_P:]), _bits(st[:, :, KALMAN_P:]))            # same gains, same innovation scale
    for i, r in enumerate(prob.rows):
        m = list(moving_slots(r.kind))
        assert np.array_equal(_bits(Fn[:, :, i, m]), _bits(F[:, :, i, m]))
    d = kalman_margin_statement(robot, st, par, **kc.MARGIN)
    assert not d[:, :, -1].any() and (d[:, :, :-1] > 0).all()
    lo, hi = inflated_row_bounds(robot, B, d)
    assert (lo[:, :, -1] == robot.row_lb[-1]).all() and (hi[:, :, -1] == robot.row_ub[-1]).all()
    bad = st.copy()
    bad[0, 0, KALMAN_P], bad[1, 1, KALMAN_S2] = np.nan, np.nan
    dn = kalman_margin_statement(robot, bad, par, **kc.MARGIN)
    assert (dn[0, :, 0] == kc.MARGIN['d_max']).all() and (dn[1, :, 1] == kc.MARGIN['d_max']).all() and np.isfinite(dn).all()


@pytest.mark.parametrize('system', ['z1', 'fr7'])
def test_margin_identities(system):
    """z = 0 and base (0, 0) give the descriptor's bounds bit for bit; a margin with only a base equals row_margin's table"""
    N, B, T = 4, 3, 12
    par_, prob, net = kc.problem(system, N)
    st = kc.run_statement(prob, fc.world(prob, B, T), kc.PAR[2], N, range(8))[-1][0]
    d = kalman_margin_statement(prob, st, kc.PAR[2], 0.0, (0.0, 0.0), 0.04)
    assert not d.any()
    lo, hi = inflated_row_bounds(prob, B, d)
    assert lo.tobytes() == np.ascontiguousarray(np.broadcast_to(prob.row_lb, lo.shape)).tobytes()
    assert hi.tobytes() == np.ascontiguousarray(np.broadcast_to(prob.row_ub, hi.shape)).tobytes()
    base = (0.004, 0.003)
    d = kalman_margin_statement(prob, st, kc.PAR[2], 0.0, base, 0.04)
    want = inflated_row_bounds(prob, B, base[0] + base[1] * np.arange(N + 1))
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(inflated_row_bounds(prob, B, d), want))
    for bad, name in ((dict(z=-1.0), 'z='), (dict(z=1.0, base=(np.nan, 0.0)), 'base_a='), (dict(z=1.0, d_max=np.inf), 'd_max=')):
        with pytest.raises(ValueError, match=f'kalman_margin_statement: {name}'):
            kalman_margin_statement(prob, st, kc.PAR[2], **bad)
    for bad, name in (((3, 0.1, 0.1), 'degree 3'), ((1, -0.1, 0.1), 'q='), ((1, 0.1, 0.0), 'r='), ((1, 0.1, np.nan), 'r='),
                      ((1, 0.1, 0.1, -1.0), 'v0='), ((1, 0.1, 0.1, 0.1, np.inf), 'a0='), ((1, 0.1, 0.1, 0.1, 0.1, 1.5), 'beta=')):
        with pytest.raises(ValueError, match=f'kalman_params: {name}'):
            kalman_params(*bad)


# ---- 3. statistics --------------------------------------------------------------------------------------------------------------------------------
def _own_model_worlds(p, q, r, v0, a0, n, steps, rng, q_world=None):
    """n scalar worlds drawn from the filter's own model: the state at the first sample has vel ~ N(0, v0^2), acc ~ N(0, a0^2), then
    x' = Phi x + G w, w ~ N(0, q^2); y = pos + N(0, r^2).  (truth [steps, n], y [steps, n])"""
    G = np.array([[1.0, 0.0, 0.0], [0.5, 1.0, 0.0], [1.0 / 6.0, 0.5, 1.0]][p])
    x = np.zeros((n, 3))
    x[:, 0] = rng.normal(0.0, 1.0, n)
    if p >= 1:
        x[:, 1] = rng.normal(0.0, v0, n)
    if p == 2:
        x[:, 2] = rng.normal(0.0, a0, n)
    truth = np.empty((steps, n))
    for t in range(steps):
        truth[t] = x[:, 0]
        w = rng.normal(0.0, q if q_world is None else q_world, n)
        x = np.stack([x[:, 0] + x[:, 1] + 0.5 * x[:, 2], x[:, 1] + x[:, 2], x[:, 2]], axis=1) + w[:, None] * G[None]
    return truth, truth + rng.normal(0.0, r, (steps, n))


@pytest.mark.parametrize('p,ratio', [(1, 0.1), (2, 0.01)])
def test_innovations_and_forecast_errors_have_the_variance_the_filter_predicts(p, ratio):
    """20 007 scalar worlds drawn from the filter's own model (seed 0), a burn-in of 40 steps, then one more: THE CONDITIONS are
    (a) the mean of nu^2 / S -- chi-square with one degree of freedom under the model, variance 2 -- within 5 standard errors
        sqrt(2 / n) of 1, and
    (b) the mean squared forecast error at nodes k = 0, 4, 8 divided by Pi_k[0][0] within 5 sqrt(2 / n) of 1 (the error is normal
        with that variance: the truth k columns ahead holds the process noise of those columns, and no sensor noise)."""
    n, burn = 20007, 40
    r = 0.01
    q, v0, a0 = ratio * r, 0.02, 0.005
    par = kalman_params(p, q, r, v0, a0, 0.0)
    truth, y = _own_model_worlds(p, q, r, v0, a0, n, burn + 1 + 8, np.random.default_rng(0))
    st = np.zeros((n, 1, KALMAN_REC))
    Y = lambda t: np.repeat(y[t][:, None, None], 8, axis=2)
    for t in range(burn):
        st, F = kalman_statement(st, Y(t), [ROW_COORD], par, 8)
    assert (st[:, 0, KALMAN_N] == burn).all() and (st[:, 0, KALMAN_S2] == 1.0).all()
    from safe_mpc_amd.problem import kalman_noise
    Q, r2 = kalman_noise(par)[:2]
    Pi = tuple(st[:, 0, KALMAN_P + i] for i in range(6))
    se = np.sqrt(2.0 / n)
    # (a): the innovation of step `burn` against S = P-00 + r^2
    S = kalman_predict_cov(p, Pi, Q)[0] + r2
    nis = (y[burn] - F[:, 1, 0, 6]) ** 2 / S
    print(f'(p, q/r) = ({p}, {ratio}): mean nu^2/S = {nis.mean():.4f}, standard error {se:.4f}')
    assert abs(nis.mean() - 1.0) <= 5 * se
    # (b): the forecast made at time burn - 1 against the truth at burn - 1 + k
    for k in range(9):
        if k in (0, 4, 8):
            e2 = (F[:, k, 0, 6] - truth[burn - 1 + k]) ** 2 / Pi[0]
            print(f'  node {k}: mean squared error / Pi_k[0][0] = {e2.mean():.4f}')
            assert abs(e2.mean() - 1.0) <= 5 * se, k
        Pi = kalman_predict_cov(p, Pi, Q)


def test_the_innovation_scale_rises_on_a_world_that_turns_more_than_modelled():
    n, steps, r = 2000, 60, 0.01
    q, v0, a0 = 0.5 * r, 0.02, 0.005
    Y = lambda y, t: np.repeat(y[t][:, None, None], 8, axis=2)
    for beta, q_world, check in ((0.1, 3 * q, 'rises'), (0.0, q, 'floor')):
        par = kalman_params(1, q, r, v0, a0, beta)
        _, y = _own_model_worlds(1, q, r, v0, a0, n, steps, np.random.default_rng(3), q_world=q_world)
        st = np.zeros((n, 1, KALMAN_REC))
        for t in range(steps):
            st, _ = kalman_statement(st, Y(y, t), [ROW_COORD], par, 1)
        s2 = st[:, 0, KALMAN_S2]
        assert (s2 >= 1.0).all()
        if check == 'rises':       # three times the process noise: E nu^2 / S is well above 1, and the mean of s2 follows it
            print(f'innovation scale on a world with 3 q: mean {s2.mean():.2f}')
            assert s2.mean() > 1.5
        else:
            assert (s2 == 1.0).all()


# ---- 4. the interface -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('system', ['z1', 'fr7'])
def test_occlude_tracks(system):
    par_, prob, net = kc.problem(system, 4)
    B, T = 6, 50
    S = observe_tracks(prob, fc.world(prob, B, T), 0.001, seed=2)
    out = occlude_tracks(prob, S, 0.1, 4.0, seed=7)
    assert out.shape == S.shape and np.array_equal(_bits(occlude_tracks(prob, S, 0.0, 4.0)), _bits(S))
    nan = np.isnan(out)
    assert nan.any() and not nan.all(axis=1).any() and np.array_equal(_bits(out[~nan]), _bits(S[~nan]))
    names = sorted({n for n in prob.row_obstacle if n is not None})
    for i, (r, name) in enumerate(zip(prob.rows, prob.row_obstacle)):
        m = list(moving_slots(r.kind))
        rest = sorted(set(range(8)) - set(m))
        assert not nan[:, :, i, rest].any()
        assert (nan[:, :, i, m] == nan[:, :, i, m[:1]]).all()                       # a burst takes all of a row's moving slots
        for j, (r2, name2) in enumerate(zip(prob.rows, prob.row_obstacle)):          # ... in every row the obstacle appears in
            if name2 == name:
                assert np.array_equal(nan[:, :, i, m[0]], nan[:, :, j, moving_slots(r2.kind)[0]])
    assert len(names) >= 1
    # instance b's draws do not depend on B; reproducible per seed; another seed, other bursts
    assert np.array_equal(np.isnan(occlude_tracks(prob, S[:2], 0.1, 4.0, seed=7)), nan[:2])
    assert np.array_equal(_bits(occlude_tracks(prob, S, 0.1, 4.0, seed=7)), _bits(out))
    assert not np.array_equal(np.isnan(occlude_tracks(prob, S, 0.1, 4.0, seed=8)), nan)
    # the share of hidden columns is p L / (1 + p L) in the long run: 2/7 here, 6 x 50 x obstacles draws -- a loose sanity band
    share = nan[:, :, 0, moving_slots(prob.rows[0].kind)[0]].mean()
    assert 0.1 < share < 0.5, share
    for bad, msg in ((dict(p_start=-0.1, mean_len=4), 'p_start'), (dict(p_start=0.1, mean_len=0.5), 'mean_len')):
        with pytest.raises(ValueError, match=f'occlude_tracks: {msg}'):
            occlude_tracks(prob, S, **bad)
    with pytest.raises(ValueError, match='occlude_tracks: expected a track'):
        occlude_tracks(prob, S[:, :, :1], 0.1, 4)


def _host_case():
    N, B, steps, T = LOOP_N, 5, 7, 4
    pars, base, geoms = _loop_setup()
    world = np.ascontiguousarray(np.repeat(geoms[np.array([0, 1, 0, 1, 1])][:, None], T, axis=1))
    observed = np.ascontiguousarray(np.repeat(geoms[np.array([1, 0, 1, 0, 0])][:, None], T, axis=1))
    x0 = sample_instances(base, B, seed=5, vel_scale=0.1)
    xg, ug = np.repeat(x0[:, None, :], N + 1, axis=1), np.zeros((B, N, 6))
    fail = np.array([0, 4, 0, 4, 0], np.int32)

    def run(**kw):
        solvers = {}
        mk, mkb = tc.oracle_factories(pars[0], N, pars, geoms, log=solvers, solver_cls=kc.recorder_class())

        def mk_scripted(name, batch):
            ctrl = mk(name, batch)
            ctrl.ocp_solver.scripted_status = [fail.copy() for _ in range(N)] + [np.zeros(B, np.int32)] * 8
            return ctrl
        return cl.run_mpc(pars[0], 'htwa', xg, ug, make_controller=mk_scripted, make_backup=mkb, n_steps=steps, scenes=world,
                          score=True, **kw), solvers
    return run, pars, base, world, observed, N, steps, xg, ug


@pytest.mark.parametrize('degree', [None, 0, 2])
def test_run_mpc_kalman_on_the_host_path(degree):
    """'htwa', 5 instances, 7 steps around the recording double; scripted failures make instances 1 and 3 abort at step N - 1; the
    observed track (one scene per instance in all columns, ANOTHER one than the world's) loses instance 2 in column 2.  Per step ONE
    advance: the forecast of the statement carried from the all-zero state, as a track without a clock, then ONE table from the same
    state, then the solve; the backup handle gets the forecast and the table of the aborting rows' records with advance=False over its
    own horizon, and no world; the scene is re-set to the world before the scores; both handles end clean"""
    run, pars, base, world, observed, N, steps, xg, ug = _host_case()
    occl = kc.bursts(base, observed, [(2, 2, 3)])
    kal, rmk, rm = (0.0005, 0.002), (2.0, 0.04), (0.002, 0.001)
    p = 1 if degree is None else degree
    res, sv = run(forecast='kalman', forecast_degree=degree, kalman=kal, observed=occl, row_margin_kalman=rmk, row_margin=rm)
    par = kalman_params(p, *kal)
    assert res['forecast'] == 'kalman' and res['observed'] is True and res['forecast_degree'] == p
    assert res['kalman'] == (0.0005, 0.002, 0.002, 0.002, 0.0) and res['row_margin_kalman'] == rmk and res['row_margin'] == rm
    main, back = sv['htwa'], sv['backup']
    for sv_ in (main, back):    # the host path is the statement: no table and no engine forecast reaches a solver; the end clears both
        assert [(e[0], e[1]) for e in sv_.events if e[0] in ('world', 'observed')] == [('observed', None), ('world', None)]
        assert not [e for e in sv_.events if e[0].startswith('engine_kalman')]
    ev = main.events
    first_score = next(k for k, e in enumerate(ev) if e[0] == 'eval_nodes')
    loop = ev[:first_score]
    solves = [k for k, e in enumerate(loop) if e[0] == 'solve']
    assert len(solves) == steps
    st = np.zeros((5, len(base.rows), KALMAN_REC))
    kinds = kc.kinds(base)
    for j, k in enumerate(solves):
        st, F = kalman_statement(st, occl[:, scene_column(j, occl.shape[1])], kinds, par, N)
        before = [e for e in loop[(solves[j - 1] if j else -1) + 1:k] if e[0] in ('track', 'row_bounds')]
        assert [e[0] for e in before][-2:] == ['track', 'row_bounds'] and [e[0] for e in before].count('row_bounds') == 1, j
        assert np.array_equal(before[-2][1], F), j                                              # one advance per step, from what was seen
        lo, hi = inflated_row_bounds(base, 5, kalman_margin_statement(base, st, par, rmk[0], rm, rmk[1]))
        assert np.array_equal(before[-1][1], lo) and np.array_equal(before[-1][2], hi), j       # the margin behind the forecast
        assert loop[k][1] is None                                                               # read from time 0
        if j == N - 1:
            st_event = st.copy()
    assert (st[2, :, KALMAN_N] == steps - 1).all() and (st[[0, 1, 3, 4]][:, :, KALMAN_N] == steps).all()    # the lost column was skipped
    rest = ev[first_score - 2:first_score + 1]
    assert [e[0] for e in rest] == ['track', 'clock', 'eval_nodes'] and np.array_equal(rest[0][1], world)     # scored in the true world
    assert main.track is None and main.idx is None and main.clock is None and main.scene_calls[-1] is None
    Nb = pars[0].back_hor
    bprob = C.OcpProblem(pars[0], 'backup', 'zero', N=Nb)
    bev = [e for e in back.events if e[0] in ('row_bounds', 'solve') or (e[0] == 'track' and e[1] is not None)]
    assert [e[0] for e in bev] == ['track', 'row_bounds', 'solve', 'row_bounds']
    _, Fb = kalman_statement(st_event[[1, 3]], None, kinds, par, Nb, advance=False)
    assert np.array_equal(bev[0][1], Fb)
    blo, bhi = inflated_row_bounds(bprob, 2, kalman_margin_statement(bprob, st_event[[1, 3]], par, rmk[0], rm, rmk[1]))
    assert np.array_equal(bev[1][1], blo) and np.array_equal(bev[1][2], bhi) and bev[3][1] is None
    assert back.track is None and back.idx is None and back.clock is None
    assert res['x_viable'].shape[0] == 2


def test_run_mpc_without_the_new_arguments_makes_the_calls_of_before():
    run, pars, base, world, observed, N, steps, xg, ug = _host_case()
    for kw in (dict(), dict(forecast='fit', forecast_window=2, observed=observed)):
        ref, sv_ref = run(**kw)
        none, sv_none = run(kalman=None, row_margin_kalman=None, **kw)
        assert not {'kalman', 'row_margin_kalman'} & (set(ref) | set(none))
        for name in ('htwa', 'backup'):
            assert _same_events(sv_none[name].events, sv_ref[name].events), name
            assert not any(e[0] == 'row_bounds' for e in sv_ref[name].events)
    kal, sv_kal = run(forecast='kalman', kalman=(0.0005, 0.002), observed=observed)
    assert 'row_margin_kalman' not in kal and not any(e[0] == 'row_bounds' for e in sv_kal['htwa'].events)


def test_run_mpc_value_errors_and_result_file_names():
    run, pars, base, world, observed, N, steps, xg, ug = _host_case()
    kal = (0.0005, 0.002)
    with pytest.raises(ValueError, match=r"kalman: forecast='kalman' needs kalman=\(q, r"):
        run(forecast='kalman')
    for fcst in (None, 'cv', 'fit'):
        with pytest.raises(ValueError, match="kalman: forecast=.* has no filter: it goes with forecast='kalman'"):
            run(forecast=fcst, kalman=kal)
        with pytest.raises(ValueError, match="row_margin_kalman: forecast=.* it goes with forecast='kalman'"):
            run(forecast=fcst, row_margin_kalman=(2.0, 0.04))
    with pytest.raises(ValueError, match="row_margin_fit: forecast='kalman' .* it goes with forecast='fit'"):
        run(forecast='kalman', kalman=kal, row_margin_fit=(2.0, 0.0, 0.04))
    for bad in ((0.1,), (0.1, 0.1, 0.1, 0.1, 0.1, 0.1)):
        with pytest.raises(ValueError, match=r'kalman: expected \(q, r\[, v0, a0, beta\]\)'):
            run(forecast='kalman', kalman=bad)
    for bad, name in (((-0.1, 0.1), 'q='), ((0.1, 0.0), 'r='), ((0.1, 0.1, 0.1, 0.1, 2.0), 'beta=')):
        with pytest.raises(ValueError, match=f'kalman: {name}'):
            run(forecast='kalman', kalman=bad)
    with pytest.raises(ValueError, match='forecast_degree: 3'):
        run(forecast='kalman', kalman=kal, forecast_degree=3)
    for bad in ((2.0,), (2.0, 0.04, 1.0), (-1.0, 0.04), (2.0, np.inf)):
        with pytest.raises(ValueError, match=r'row_margin_kalman: expected \(z, d_max\)'):
            run(forecast='kalman', kalman=kal, row_margin_kalman=bad)
    with pytest.raises(ValueError, match="observed: a NaN .* only forecast='kalman' skips one"):
        run(forecast='fit', forecast_window=2, observed=kc.bursts(base, observed, [(2, 2, 3)]))
    mk, mkb = tc.oracle_factories(pars[0], N, pars, _loop_setup()[2])
    for arg in (dict(kalman=kal), dict(kalman=kal, row_margin_kalman=(2.0, 0.04))):
        with pytest.raises(ValueError, match="the 'parallel' policy is not supported"):
            cl.run_mpc(pars[0], 'parallel', xg, ug, forecast='kalman', scenes=world, make_controller=mk, make_backup=mkb, n_steps=2, **arg)
    with pytest.raises(ValueError, match='row_margin_kalman: TrackOracleSolver has no set_instance_row_bounds'):
        cl.run_mpc(pars[0], 'htwa', xg, ug, forecast='kalman', kalman=kal, row_margin_kalman=(2.0, 0.04), scenes=world, make_controller=mk,
                   make_backup=mkb, n_steps=2)
    # a device loop asks its solvers for the calls before anything runs
    fcst = cl._Forecast('kalman', None, 1, kal)
    with pytest.raises(ValueError, match='forecast: TrackOracleSolver has no forecast_scene'):
        fcst.require(mk('htwa', 2).ocp_solver, False, True)
    args = (pars[0], 'z1', 'htwa', 6, True, 0.0, 0.0, 0, 0)
    plain = cl.result_file(*args)
    assert cl.result_file(*args, kalman=None, row_margin_kalman=None, obs_dropout=None) == plain
    assert cl.result_file(*args, forecast='kalman', kalman=kal) == plain.replace('_mpc.pkl', '_fckalman_d1_q0.0005_r0.002_v0.002_a0.002_b0.0_mpc.pkl')
    assert cl.result_file(*args, forecast='kalman', forecast_degree=2, kalman=(0.1, 0.2, 0.3, 0.4, 0.5), obs_noise=0.005, obs_dropout=(0.1, 4),
                          row_margin=(0.01, 0.0), row_margin_kalman=(2, 0.05)).endswith(
        '_fckalman_d2_q0.1_r0.2_v0.3_a0.4_b0.5_on0.005_od0.1_l4.0_rm0.01_rmk2.0_c0.05_mpc.pkl')


def test_mpc_script_takes_the_kalman_flags(monkeypatch, tmp_path):
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
        return {'conv_idx': [], 'collisions_idx': [], 'viable_idx': [], 'scenes': kw.get('scenes')}
    monkeypatch.setattr(cl, 'run_mpc', fake_run)
    root = ['-c', 'naive', '--horizon', str(N), '--scene-velocity', '0.3']
    base = root + ['--scene-forecast', 'kalman', '--kalman-q', '0.001', '--kalman-r', '0.005']
    mpc = _script('mpc')
    assert mpc.main(base) == 0
    kw = seen['kw']
    assert kw['forecast'] == 'kalman' and kw['kalman'] == (0.001, 0.005, 0.005, 0.005, 0.0) and kw['forecast_degree'] == 1
    assert 'observed' not in kw and 'row_margin_kalman' not in kw and 'forecast_window' not in kw
    assert names[-1][0].endswith('_fckalman_d1_q0.001_r0.005_v0.005_a0.005_b0.0_mpc.pkl')
    assert mpc.main(base + ['--forecast-degree', '2', '--kalman-prior', '0.02', '0.003', '--kalman-beta', '0.1', '--scene-obs-noise', '0.005',
                            '--scene-obs-dropout', '0.05', '--scene-obs-dropout-len', '6', '--row-margin-z', '2', '--row-margin-cap', '0.03',
                            '--row-margin', '0.01']) == 0
    kw = seen['kw']
    assert kw['kalman'] == (0.001, 0.005, 0.02, 0.003, 0.1) and kw['forecast_degree'] == 2 and kw['row_margin_kalman'] == (2.0, 0.03)
    assert kw['row_margin'] == (0.01, 0.0) and 'row_margin_fit' not in kw
    assert kw['observed'].shape == kw['scenes'].shape and np.isnan(kw['observed']).any()
    assert names[-1][0].endswith('_fckalman_d2_q0.001_r0.005_v0.02_a0.003_b0.1_on0.005_od0.05_l6.0_rm0.01_rmk2.0_c0.03_mpc.pkl')
    assert mpc.main(base + ['--scene-obs-dropout', '0.05']) == 0                                 # dropouts without noise: of the world itself
    assert np.isnan(seen['kw']['observed']).any() and names[-1][0].endswith('_od0.05_l4.0_mpc.pkl')
    for extra, msg in ((root + ['--scene-forecast', 'kalman', '--kalman-r', '0.1'], '--scene-forecast kalman needs --kalman-q'),
                       (root + ['--scene-forecast', 'kalman', '--kalman-q', '0.1'], '--scene-forecast kalman needs --kalman-r'),
                       (root + ['--scene-forecast', 'cv', '--kalman-q', '0.1'], '--kalman-q needs --scene-forecast kalman'),
                       (root + ['--scene-forecast', 'fit', '--kalman-beta', '0.1'], '--kalman-beta needs --scene-forecast kalman'),
                       (root + ['--scene-forecast', 'fit', '--scene-obs-dropout', '0.1'], '--scene-obs-dropout needs --scene-forecast kalman'),
                       (base + ['--scene-obs-dropout-len', '4'], '--scene-obs-dropout-len needs --scene-obs-dropout'),
                       (base + ['--scene-obs-dropout', '1.5'], 'expected a probability'),
                       (base + ['--kalman-beta', '2'], 'beta=2.0'),
                       (base + ['--forecast-degree', '3'], '--forecast-degree 3: expected 0, 1 or 2'),
                       (base + ['--row-margin-z', '2', '--row-margin-prior', '0.1'], '--row-margin-prior goes with --scene-forecast fit'),
                       (base + ['--forecast-window', '4'], '--forecast-window needs --scene-forecast fit'),
                       (root + ['--scene-forecast', 'linear'], 'expected hold, cv or true, or fit, or kalman'),
                       (['-c', 'parallel'] + base[2:] + ['--row-margin-z', '2'], "--row-margin-z: the 'parallel' policy is not supported")):
        with pytest.raises(SystemExit, match=re.escape(msg)):
            mpc.main(extra)


def test_the_new_symbols_are_declared_exported_and_prototyped():
    from safe_mpc_amd import _lib, solver
    hdr = open(os.path.join(ROOT, 'include', 'smpc.h')).read()
    declared = set(re.findall(r'^(?:int|void|const char\*|void\*) (smpc_\w+)\(', hdr, re.M))
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('smpc_forecast_scene_kalman', 'smpc_kalman_row_margin'):
        assert name in declared and name in _lib.SYMBOLS and hasattr(L, name), name
    assert re.search(r'#define SMPC_KALMAN_REC 32\b', hdr) and KALMAN_REC == 32
    vp, i, dbl = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    from safe_mpc_amd.problem import KalmanParams
    assert _lib.lib().smpc_forecast_scene_kalman.argtypes == [vp, i, ctypes.POINTER(KalmanParams), vp, i, i, vp]
    assert _lib.lib().smpc_kalman_row_margin.argtypes == [vp, i, ctypes.POINTER(KalmanParams), vp, dbl, dbl, dbl, dbl]
    assert ctypes.sizeof(KalmanParams) == 48 and [f[0] for f in KalmanParams._fields_] == ['degree', 'reserved', 'q', 'r', 'v0', 'a0', 'beta']
    for m in ('forecast_scene_kalman', 'kalman_row_margin', 'new_kalman_state'):
        assert callable(getattr(solver.BatchedOcpSolver, m))
    L.smpc_abi_version.restype = ctypes.c_int
    assert L.smpc_abi_version() == 5             # nothing existing changed
    for flag in ('kalman-kernel', 'kalman-loop'):
        assert flag in open(os.path.join(ROOT, 'scripts', 'forecast_bench.py')).read()
    assert FIT_MARGIN_CAP == 0.05
