"""Obstacle forecasts of degree 0 to 2 (smpc_forecast_scene_poly) without a GPU: the weights against the exact
normal equations, the numpy statement against its scalar restatement and its ties to 'hold', 'cv' and the line fit, the lag claim on a
turning world and the noise claim on a straight one, what run_mpc(forecast='fit', forecast_degree=...) hands to its solvers -- on the
recording double of test_forecast_host.py --, the ABI and the entry script's flag."""
import ctypes
import os
import pickle
import re
from fractions import Fraction

import numpy as np
import pytest

import forecast_cases as fc
import poly_forecast_cases as pf
import track_cases as tc
from conftest import ROOT, sample_instances
from safe_mpc_amd import closed_loop as cl
from safe_mpc_amd.problem import (FIT_MAX, fit_forecast_statement, fit_weights, forecast_statement, moving_scenes, observe_tracks,
                                  poly_forecast_statement, poly_weights)
from test_forecast_fit_host import FitRecorder, _independent_draws
from test_forecast_host import LOOP_N, _loop_setup, _same_events, _script


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


# ---- 1. the weights ----------------------------------------------------------------------------------------------------------------------
def _exact_weights(m, p):
    """rows of (X'X)^-1 X' for X[j] = (1, -j, j^2)[:p + 1], j = 0..m-1, in exact rationals: [p + 1][m] -- the weights of a, b, c"""
    X = [[Fraction((-j) ** q) for q in range(p + 1)] for j in range(m)]
    n = p + 1
    A = [[sum(X[j][r] * X[j][c] for j in range(m)) for c in range(n)] + [Fraction(int(r == c)) for c in range(n)] for r in range(n)]
    for i in range(n):                      # Gauss-Jordan on [X'X | I]
        piv = next(r for r in range(i, n) if A[r][i] != 0)
        A[i], A[piv] = A[piv], A[i]
        A[i] = [v / A[i][i] for v in A[i]]
        for r in range(n):
            if r != i:
                A[r] = [vr - A[r][i] * vi for vr, vi in zip(A[r], A[i])]
    inv = [row[n:] for row in A]
    return [[sum(inv[r][q] * X[j][q] for q in range(n)) for j in range(m)] for r in range(n)]


def test_weights_are_the_normal_equations_in_one_rounded_division():
    """for m = 1..32 and degrees 0..2 every float64 weight is the correctly rounded exact least-squares weight (int / int in Python is
    correctly rounded): ua the weights of a, uv those of b + c, ue those of 2c; sum ua = 1 and sum uv = sum ue = 0 exactly in
    rationals and within m 2^-52 (times the largest weight) in floats; at m = 3 the weights are integers"""
    assert FIT_MAX == 32
    for m in range(1, FIT_MAX + 1):
        for degree in pf.DEGREES:
            p = min(degree, m - 1)
            got = poly_weights(m, degree)
            assert len(got) == (1, 2, 3)[p] and all(g.shape == (m,) and g.dtype == np.float64 for g in got), (m, degree)
            rows = _exact_weights(m, p)
            if p == 0:
                want = [rows[0]]
            elif p == 1:
                want = [rows[0], rows[1]]
                assert all(np.array_equal(g, f) for g, f in zip(got, fit_weights(m)))
            else:
                want = [rows[0], [b + c for b, c in zip(rows[1], rows[2])], [2 * c for c in rows[2]]]
                for j in range(m):
                    for (num, den), w in zip((pf.ua_int(m, j), pf.uv_int(m, j), pf.ue_int(m, j)), want):
                        assert Fraction(num, den) == w[j], (m, j)
                        assert abs(num) < 2 ** 31 and den <= 33390720
            for g, w, total in zip(got, want, (1, 0, 0)):
                assert sum(w) == total, (m, degree)
                for j in range(m):
                    assert g[j] == w[j].numerator / w[j].denominator, (m, degree, j)
                assert abs(g.sum() - total) <= m * 2.0 ** -52 * max(1.0, np.abs(g).max()), (m, degree)
    ua, uv, ue = poly_weights(3, 2)
    assert ua.tolist() == [1.0, 0.0, 0.0] and uv.tolist() == [2.0, -3.0, 1.0] and ue.tolist() == [1.0, -2.0, 1.0]
    assert poly_weights(1, 2)[0].tolist() == [1.0] and poly_weights(4, 0)[0].tolist() == [0.25] * 4
    for bad in (0, 33, -1):
        with pytest.raises(ValueError, match=f'm={bad}'):
            poly_weights(bad, 2)
    for bad in (-1, 3):
        with pytest.raises(ValueError, match=f'degree={bad}'):
            poly_weights(4, bad)


# ---- 2. the statement ---------------------------------------------------------------------------------------------------------------------
def test_statement_is_the_definition_and_its_errors():
    """against the scalar restatement with Python floats and integer formulas, bit for bit: the three degrees, every window and
    clock, full-mantissa worlds with T in {1, 2, N + 1, N + 4, 40}"""
    N = 4
    par, prob, net = fc.problem('z1', N)
    for T in (1, 2, N + 1, N + 4, 40):
        W = fc.world(prob, 2, T, seed=T)
        for degree in pf.DEGREES:
            for window in pf.WINDOWS:
                for t in pf.clocks(T):
                    F = poly_forecast_statement(W, t, N, window, degree)
                    assert F.shape == (2, N + 1, len(prob.rows), 8)
                    for (b, r, s) in ((0, 0, 0), (1, 3, 6), (1, 5, 7)):
                        assert np.array_equal(_bits(F[b, :, r, s]), _bits(pf.poly_scalar(W[b, :, r, s], window, degree, t, N))), \
                            (T, degree, window, t, b, r, s)
    W = fc.world(prob, 2, 40)
    # the parabola is not the line: on a full-mantissa world with a full window the three degrees differ
    F0, F1, F2 = (poly_forecast_statement(W, 35, N, 7, d) for d in pf.DEGREES)
    assert np.abs(F2 - F1).max() > 1e-4 and np.abs(F1 - F0).max() > 1e-4
    with pytest.raises(ValueError, match='poly_forecast_statement: expected a world track'):
        poly_forecast_statement(W[:, 0], 0, N, 4, 2)
    for bad in (0, 33):
        with pytest.raises(ValueError, match=f'poly_forecast_statement: window {bad}'):
            poly_forecast_statement(W, 0, N, bad, 2)
    for bad in (-1, 3):
        with pytest.raises(ValueError, match=f'poly_forecast_statement: degree {bad}'):
            poly_forecast_statement(W, 0, N, 4, bad)


@pytest.mark.parametrize('system', ['z1', 'fr7'])
def test_identities_bit_for_bit_at_every_clock(system):
    """degree 1 is the fit; degree 0 with window 1 is 'hold'; degree 2 is 'hold' where m = 1 and 'cv' where m = 2; a world of -0.0
    and zeros (slot 7 is zero everywhere) keeps its bits under degree 0"""
    for N in (1, 4):
        par, prob, net = fc.problem(system, N)
        for T in (1, 2, N + 4, 40):
            W = fc.world(prob, 3, T, seed=T)
            Z = W.copy()
            Z[..., 7] = 0.0
            Z[:, :, 0, :4] = -0.0
            for t in pf.clocks(T):
                tt = 0 if t is None else min(max(t, -2 ** 62), 2 ** 62)
                for window in pf.WINDOWS:
                    m = min(window, max(tt, 0) + 1)
                    assert np.array_equal(_bits(poly_forecast_statement(W, t, N, window, 1)), _bits(fit_forecast_statement(W, t, N, window)))
                    F2 = poly_forecast_statement(W, t, N, window, 2)
                    if m == 1:
                        assert np.array_equal(_bits(F2), _bits(forecast_statement(W, t, N, 'hold'))), (T, t, window)
                    if m == 2:
                        assert np.array_equal(_bits(F2), _bits(forecast_statement(W, t, N, 'cv'))), (T, t, window)
                    F0 = poly_forecast_statement(Z, t, N, window, 0)
                    assert np.array_equal(_bits(F0[..., 7]), _bits(np.zeros_like(F0[..., 7]))), (T, t, window)
                    assert np.array_equal(_bits(F0[:, :, 0, :4]), _bits(np.full_like(F0[:, :, 0, :4], -0.0))), (T, t, window)
                assert np.array_equal(_bits(poly_forecast_statement(W, t, N, 1, 0)), _bits(forecast_statement(W, t, N, 'hold'))), (T, t)


# ---- 3. the lag claim ------------------------------------------------------------------------------------------------------------------------
def test_a_parabola_follows_a_turning_obstacle_and_a_line_lags_by_the_formula():
    """A noise-free world whose slots are p0 + v c + (g / 2) c^2 in the column c, with dyadic p0, v and g / 2, so every sample is
    exact.  At t = 32 over N = 7 (T = 40: no clamped column), windows 3, 7 and 32:
    degree 2 is the truth at every node k, and degree 1 misses it by (g / 2) ((m - 1)(m - 2) / 6 + (m - 1) k + k^2) -- both held in
    exact rationals within a bound from the operation count.  An accumulation x = sum u_j y_j of m rounded weights, m rounded
    products and m - 1 rounded sums is off by at most (2m - 1 + 1) 2^-53 sum|u_j y_j| to first order: 2 m 2^-53 sum|u_j y_j|, the
    bound of test_forecast_fit_host.py.  Node k is a + k v + k (k - 1) / 2 e, so those three bounds enter with these factors.  The
    tail makes at most k additions into F and k (k - 1) / 2 into v that reach node k, k (k + 1) / 2 <= N (N + 1) / 2 roundings of at
    most 2^-53 M each, M the largest |F| or |v| on the way: |F| is at most the largest |truth| plus the largest lag, and every step
    -- the parabola's true steps, and the line's slope, which is a weighted mean of the window's steps -- at most the largest step
    between two columns of the world.  A factor 2 to spare on the tail, as on the accumulations."""
    N, T, t = 7, 40, 32
    rng = np.random.default_rng(3)
    p0 = rng.integers(-2048, 2048, (3, 8)) / 1024.0
    v = rng.integers(-64, 64, (3, 8)) / 1024.0
    h = rng.integers(-32, 32, (3, 8)) / 4096.0          # g / 2
    h[h == 0] = 1 / 4096.0
    c = np.arange(T)[:, None, None]
    S = np.ascontiguousarray((p0 + v * c + h * c * c)[None])           # [1, T, 3, 8]
    exact = lambda x: Fraction(float(x))
    for r in range(3):
        for s in range(8):
            for col in range(T):
                assert exact(S[0, col, r, s]) == exact(p0[r, s]) + exact(v[r, s]) * col + exact(h[r, s]) * col * col
    eps = 2.0 ** -53
    worst = {1: 0.0, 2: 0.0}
    for m in (3, 7, 32):
        y = S[0, t - np.arange(m)]                                      # ages 0..m-1: [m, 3, 8]
        F2, F1 = poly_forecast_statement(S, t, N, m, 2)[0], poly_forecast_statement(S, t, N, m, 1)[0]
        ua, uv, ue = poly_weights(m, 2)
        u, w = fit_weights(m)
        acc = lambda wt: 2 * m * eps * np.abs(wt[:, None, None] * y).sum(axis=0)
        ba, bv, be, bu, bw = acc(ua), acc(uv), acc(ue), acc(u), acc(w)
        truth = np.stack([S[0, t + k] for k in range(N + 1)])
        lag_max = np.abs(h) * ((m - 1) * (m - 2) / 6 + (m - 1) * N + N * N)
        M = np.maximum(np.abs(truth).max(axis=0) + lag_max, np.abs(np.diff(S[0, :t + N + 1], axis=0)).max(axis=0))
        for k in range(N + 1):
            tail = 2 * (k * (k + 1) / 2) * eps * M
            b2 = ba + k * bv + k * (k - 1) / 2 * be + tail
            b1 = bu + k * bw + tail
            for r in range(3):
                for s in range(8):
                    want = exact(truth[k, r, s])
                    e2 = abs(exact(F2[k, r, s]) - want)
                    lag = exact(h[r, s]) * (Fraction((m - 1) * (m - 2), 6) + (m - 1) * k + k * k)
                    e1 = abs(exact(F1[k, r, s]) - (want - lag))
                    assert e2 <= b2[r, s], (m, k, r, s, float(e2), b2[r, s])
                    assert e1 <= b1[r, s], (m, k, r, s, float(e1), b1[r, s])
                    worst[2], worst[1] = max(worst[2], float(e2) / b2[r, s]), max(worst[1], float(e1) / b1[r, s])
        # the claim in plain numbers: the line's lag at the last node grows with the window, the parabola has none
        assert np.abs(F2[N] - truth[N]).max() < 1e-9
        assert (np.abs(F1[N] - truth[N]) > 0.99 * np.abs(h) * ((m - 1) * (m - 2) / 6 + (m - 1) * N + N * N)).all()
    print(f'largest error / bound: degree 2 {worst[2]:.3f}, degree 1 against truth - lag {worst[1]:.3f}')


# ---- 4. the noise claim ----------------------------------------------------------------------------------------------------------------------
def test_forecast_error_under_observation_noise_is_what_the_weights_say():
    """A constant-velocity world (moving_scenes) observed with sigma = 1e-3, forecast at t = 35 over N = 8: degree 2 with windows 4, 16,
    32 and degree 0 with window 16, nodes 0, 4, 8.  The sample standard deviation over all (instance, obstacle, axis) draws is
    sigma node_sigma(m, p, k) within 5 % -- the margin and the reason of test_forecast_fit_host.py: n >= 20 000 independent draws, so
    the sample variance's own relative standard deviation is sqrt(2 / n) = 1 %, and 5 % is five of those.  Degree 2 is held against
    the TRUTH (a parabola through a straight track has no lag).  The window mean lags a moving obstacle by a deterministic
    v (m - 1) / 2 + v k that differs from draw to draw with v and is no noise: degree 0 is held against its own forecast of the
    noise-free world, which takes exactly that out (the statement is linear in what was seen)."""
    par, prob, net = fc.problem('z1', 4)
    draws = _independent_draws(prob)
    B = -(-20000 // len(draws))
    sigma, t, N = 1e-3, 35, 8
    W = moving_scenes(prob, B, t + N + 1, 0.3, seed=1, sigma=0.02)
    S = observe_tracks(prob, W, sigma, seed=7)
    truth = fc.gather_true(W, t, N)
    n = B * len(draws)
    assert n >= 20000
    for degree, window in ((2, 4), (2, 16), (2, 32), (0, 16)):
        F = poly_forecast_statement(S, t, N, window, degree)
        ref = truth if degree == 2 else poly_forecast_statement(W, t, N, window, degree)
        for k in (0, 4, 8):
            err = np.concatenate([F[:, k, r, s] - ref[:, k, r, s] for r, s in draws])
            assert err.size == n
            got, want = err.std(ddof=1), sigma * pf.node_sigma(window, degree, k)
            print(f'degree {degree}, window {window:2d}, node {k}: std of the forecast error {got:.4e}, sigma node_sigma = {want:.4e}, '
                  f'ratio {got / want:.4f} ({n} draws)')
            assert abs(got / want - 1.0) <= 0.05, (degree, window, k, got, want)
    # the arm's price and its gain in the weights' own terms: a parabola over 16 columns is noisier at the horizon's end than a line
    # over 16, and the mean is the quietest of all
    from forecast_fit_cases import node_sigma as line_sigma
    assert pf.node_sigma(16, 1, 8) == line_sigma(16, 8)
    assert pf.node_sigma(16, 2, 8) > pf.node_sigma(16, 1, 8) > pf.node_sigma(16, 0, 8) == pytest.approx(0.25)


# ---- 5. the ABI ----------------------------------------------------------------------------------------------------------------------------
def test_the_new_symbol_is_declared_exported_and_prototyped():
    from safe_mpc_amd import _lib, solver
    hdr = open(os.path.join(ROOT, 'include', 'smpc.h')).read()
    declared = set(re.findall(r'^(?:int|void|const char\*|void\*) (smpc_\w+)\(', hdr, re.M))
    L = ctypes.CDLL(_lib.LIB_PATH)
    assert 'smpc_forecast_scene_poly' in declared and 'smpc_forecast_scene_poly' in _lib.SYMBOLS and hasattr(L, 'smpc_forecast_scene_poly')
    assert declared == set(_lib.SYMBOLS)
    vp, ci = ctypes.c_void_p, ctypes.c_int
    assert _lib.lib().smpc_forecast_scene_poly.argtypes == [vp, ci, ci, ci, ci, vp]
    assert _lib.lib().smpc_forecast_scene_fit.argtypes == [vp, ci, ci, ci, vp]           # (the fit keeps its own)
    assert callable(solver.BatchedOcpSolver.forecast_scene_poly)
    assert re.search(r'^#define SMPC_FIT_MAX 32$', hdr, re.M)
    L.smpc_abi_version.restype = ctypes.c_int
    assert L.smpc_abi_version() == 5             # nothing existing changed


# ---- 6. the closed loop on the host path -------------------------------------------------------------------------------------------------
class PolyRecorder(FitRecorder):
    """FitRecorder that also writes down an engine forecast, which the host path must not make.  The oracle behind it knows whole
    scenes only, and a parabola through three equal columns is that scene within rounding only (uv = (2, -3, 1), and 3 y is rounded):
    the track is written down as it was handed over, and each of its columns is then served as the scene within 1e-12 of it."""

    def set_instance_scene_track(self, geom=None):
        if geom is None:
            return super().set_instance_scene_track(None)
        self.events.append(('track', np.array(geom)))
        known = [np.frombuffer(k, np.float64) for k in self.keys]
        g = np.array(geom, float)
        for blk in g.reshape(-1, known[0].size):
            near = [k for k in known if np.abs(blk - k).max() < 1e-12]
            assert len(near) == 1
            blk[:] = near[0]
        tc.TrackOracleSolver.set_instance_scene_track(self, g)

    def forecast_scene_poly(self, *a, **k):
        self.events.append(('poly', a))

    def forecast_scene_fit(self, *a, **k):
        self.events.append(('fit', a))


def _host_case():
    """test_forecast_fit_host._host_case with a window of 3: one scene per instance in all columns and ANOTHER one observed.  The
    oracle behind the double knows whole scenes only; constant columns are forecast exactly by the one sample at t = 0 and the line
    through two at t = 1, and within rounding by the parabola through three (a = y, but v = (2 y - 3 y) + y with 3 y rounded), which
    PolyRecorder serves as the scene it is next to"""
    N, B, steps, T = LOOP_N, 5, 7, 4
    pars, base, geoms = _loop_setup()
    world = np.ascontiguousarray(np.repeat(geoms[np.array([0, 1, 0, 1, 1])][:, None], T, axis=1))
    observed = np.ascontiguousarray(np.repeat(geoms[np.array([1, 0, 1, 0, 0])][:, None], T, axis=1))
    x0 = sample_instances(base, B, seed=5, vel_scale=0.1)
    xg, ug = np.repeat(x0[:, None, :], N + 1, axis=1), np.zeros((B, N, 6))
    fail = np.array([0, 4, 0, 4, 0], np.int32)

    def run(**kw):
        solvers = {}
        mk, mkb = tc.oracle_factories(pars[0], N, pars, geoms, log=solvers, solver_cls=PolyRecorder)

        def mk_scripted(name, batch):
            ctrl = mk(name, batch)
            ctrl.ocp_solver.scripted_status = [fail.copy() for _ in range(N)] + [np.zeros(B, np.int32)] * 8
            return ctrl
        return cl.run_mpc(pars[0], 'htwa', xg, ug, make_controller=mk_scripted, make_backup=mkb, n_steps=steps, scenes=world,
                          score=True, **kw), solvers
    return run, pars, world, observed, N, steps


def test_run_mpc_on_the_host_path_forecasts_a_parabola_from_what_was_observed():
    """'htwa', 5 instances, 7 steps around the recording double, scripted failures make instances 1 and 3 abort at step N - 1.  Every
    step the track handed over before the solve is poly_forecast_statement at time j FROM THE OBSERVED TRACK with no clock; the backup
    solver gets the same estimator on the aborting instances' observed rows over its own horizon; no engine forecast is called."""
    run, pars, world, observed, N, steps = _host_case()
    want = lambda S, t, n: poly_forecast_statement(S, t, n, 3, 2)
    res, sv = run(observed=observed, forecast='fit', forecast_window=3, forecast_degree=2)
    assert res['forecast'] == 'fit' and res['observed'] is True and res['forecast_window'] == 3 and res['forecast_degree'] == 2
    main, back = sv['htwa'], sv['backup']
    for sv_ in (main, back):
        assert not [e for e in sv_.events if e[0] in ('poly', 'fit')]
        assert [(e[0], e[1]) for e in sv_.events if e[0] in ('world', 'observed')] == [('observed', None), ('world', None)]
    ev = main.events
    loop = ev[:next(k for k, e in enumerate(ev) if e[0] == 'eval_nodes')]
    solves = [k for k, e in enumerate(loop) if e[0] == 'solve']
    assert len(solves) == steps
    for j, k in enumerate(solves):
        before = loop[(solves[j - 1] if j else -1) + 1:k]
        tracks = [e for e in before if e[0] == 'track']
        assert np.array_equal(_bits(tracks[-1][1]), _bits(want(observed, j, N))), j            # formed at time j from what was seen
        assert not np.array_equal(tracks[-1][1], want(world, j, N))
        assert [e for e in before if e[0] == 'clock'][-1][1] is None and loop[k][1] is None     # ... read from time 0
    bt = [e for e in back.events if e[0] == 'track' and e[1] is not None]
    assert len(bt) == 1 and np.array_equal(_bits(bt[0][1]), _bits(want(observed[[1, 3]], N - 1, pars[0].back_hor)))
    assert main.track is None and main.clock is None and back.track is None and back.clock is None
    assert res['x_viable'].shape[0] == 2
    assert np.array_equal(res['scenes'], world)


def test_degree_1_makes_the_calls_of_a_run_without_the_argument():
    run, pars, world, observed, N, steps = _host_case()
    plain, sv_plain = run(observed=observed, forecast='fit', forecast_window=3)
    one, sv_one = run(observed=observed, forecast='fit', forecast_window=3, forecast_degree=1)
    for name in ('htwa', 'backup'):
        assert _same_events(sv_plain[name].events, sv_one[name].events), name
    assert set(plain) == set(one) and 'forecast_degree' not in one
    for key in ('x', 'u'):
        assert np.array_equal(plain[key], one[key], equal_nan=True), key
    # degree 0 with window 1 is 'hold': the same numbers in the same order, and the result says which estimator it was
    hold, sv_hold = run(observed=observed, forecast='hold')
    mean, sv_mean = run(observed=observed, forecast='fit', forecast_window=1, forecast_degree=0)
    for name in ('htwa', 'backup'):
        assert _same_events(sv_hold[name].events, sv_mean[name].events), name
    assert mean['forecast_degree'] == 0 and mean['forecast_window'] == 1 and 'forecast_degree' not in hold


def test_run_mpc_value_errors_and_result_file_names():
    pars, base, geoms = _loop_setup()
    B, N = 2, LOOP_N
    x0 = sample_instances(base, B, seed=5, vel_scale=0.1)
    xg, ug = np.repeat(x0[:, None, :], N + 1, axis=1), np.zeros((B, N, 6))
    mk, mkb = tc.oracle_factories(pars[0], N, pars, geoms)
    track = np.repeat(geoms[[0, 1]][:, None], 3, axis=1)
    kw = dict(make_controller=mk, make_backup=mkb, n_steps=2, scenes=track)
    for fcst in (None, 'hold', 'cv', 'true'):
        for degree in (0, 1, 2):
            with pytest.raises(ValueError, match=r"forecast_degree: forecast=.* has no degree: it goes with forecast='fit'"):
                cl.run_mpc(pars[0], 'htwa', xg, ug, forecast=fcst, forecast_degree=degree, **kw)
    for bad in (-1, 3, 2.0, '2'):
        with pytest.raises(ValueError, match='forecast_degree: .* a polynomial fit has degree 0, 1 or 2'):
            cl.run_mpc(pars[0], 'htwa', xg, ug, forecast='fit', forecast_degree=bad, **kw)
    name = lambda **k: cl.result_file(pars[0], 'z1', 'htwa', 6, True, 0.0, 0.0, 0, 0, **k)
    assert name(forecast='fit', forecast_window=16, forecast_degree=2).endswith('_fcfit_w16_d2_mpc.pkl')
    assert name(forecast='fit', forecast_window=4, forecast_degree=0, obs_noise=0.001).endswith('_fcfit_w4_d0_on0.001_mpc.pkl')
    assert name(forecast='fit', forecast_window=16, forecast_degree=1) == name(forecast='fit', forecast_window=16)
    assert name(forecast='fit', forecast_window=16).endswith('_fcfit_w16_mpc.pkl')
    assert name(forecast='cv').endswith('_fccv_mpc.pkl') and name() == name(forecast=None)


# ---- 7. the entry script --------------------------------------------------------------------------------------------------------------------
def test_mpc_script_takes_forecast_degree(monkeypatch, tmp_path):
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

    def fake_run(params, name, x_guess, u_guess, scenes=None, timing=None, **kw):
        seen['scenes'], seen['kw'] = scenes, kw
        timing['ms_per_step'] = 0.0
        return {'conv_idx': [], 'collisions_idx': [], 'viable_idx': [], 'scenes': scenes}
    monkeypatch.setattr(cl, 'run_mpc', fake_run)
    base = ['-c', 'naive', '--horizon', str(N), '--scene-velocity', '0.3', '--scene-accel', '3.0', '--scene-seed', '4']
    mpc = _script('mpc')
    assert mpc.main(base + ['--scene-forecast', 'fit', '--forecast-window', '16']) == 0
    assert 'forecast_degree' not in seen['kw'] and set(names[-1][1]) == {'controller_model', 'forecast', 'forecast_window'}
    fit_name = names[-1][0]
    assert fit_name.endswith('_fcfit_w16_mpc.pkl')
    assert mpc.main(base + ['--scene-forecast', 'fit', '--forecast-window', '16', '--forecast-degree', '1']) == 0
    assert 'forecast_degree' not in seen['kw'] and names[-1][0] == fit_name                 # the call and the name of before
    assert mpc.main(base + ['--scene-forecast', 'fit', '--forecast-window', '16', '--forecast-degree', '2', '--scene-obs-noise', '0.002']) == 0
    assert seen['kw']['forecast'] == 'fit' and seen['kw']['forecast_window'] == 16 and seen['kw']['forecast_degree'] == 2
    assert seen['kw']['observed'].shape == seen['scenes'].shape
    assert names[-1][0] == fit_name.replace('_fcfit_w16_mpc.pkl', '_fcfit_w16_d2_on0.002_mpc.pkl')
    assert mpc.main(base + ['--scene-forecast', 'fit', '--forecast-degree', '0']) == 0
    assert seen['kw']['forecast_window'] == 8 and seen['kw']['forecast_degree'] == 0
    assert names[-1][0] == fit_name.replace('_fcfit_w16_mpc.pkl', '_fcfit_w8_d0_mpc.pkl')
    for extra, msg in ((['--scene-forecast', 'cv', '--forecast-degree', '2'], '--forecast-degree needs --scene-forecast fit'),
                       (['--forecast-degree', '2'], '--forecast-degree needs --scene-forecast fit'),
                       (['--scene-forecast', 'fit', '--forecast-degree', '3'], '--forecast-degree 3: expected 0, 1 or 2'),
                       (['--scene-forecast', 'fit', '--forecast-degree', '-1'], '--forecast-degree -1: expected 0, 1 or 2')):
        with pytest.raises(SystemExit, match=msg):
            mpc.main(base + extra)
