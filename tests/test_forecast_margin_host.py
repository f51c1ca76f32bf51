"""Row margins from the fit's residuals (smpc_forecast_row_margin, problem.fit_margin_statement) without a GPU:

1. the growth h_k against exact rationals, and the statement against a scalar restatement in Python floats, bit for bit
2. the identities: a world the fit reproduces, nu == 0, z = 0, a NaN sample, a robot-robot row, the base alone
3. the statistical claims: the residual variance is unbiased and the interval covers as Student's t says
4. the host loop around the recording double, the ValueErrors, names, suffixes, flags, the two symbols and the ABI version"""
import ctypes
import os
import pickle
import re
from fractions import Fraction

import numpy as np
import pytest

import forecast_cases as fc
import margin_cases as mc
import track_cases as tc
from conftest import ROOT, sample_instances
from safe_mpc_amd import closed_loop as cl
from safe_mpc_amd import controller as C
from safe_mpc_amd.problem import (FIT_MARGIN_CAP, FIT_MAX, INF, ROW_COORD, fit_margin_statement, inflated_row_bounds, margin_growth,
                                  moving_slots, poly_forecast_statement, poly_weights)
from test_forecast_fit_host import FitRecorder
from test_forecast_host import LOOP_N, _loop_setup, _same_events, _script


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ---- 1. exact values and restatement -----------------------------------------------------------------------------------------------------
def test_growth_against_exact_rationals():
    """h_k = sum_j c_kj^2 with the weights as exact rationals.  The bound, from the operation count with u = 2^-53: a weight is one
    rounded division (u), k w_j and (k (k - 1) / 2) ue_j one rounded product each (u), the two sums of c_kj one rounding each (2 u) --
    so |c - c_exact| <= 4 u A_j to first order, A_j = |ua_j| + k |uv_j| + (k (k - 1) / 2) |ue_j| >= |c_exact|; the square doubles that
    and rounds once (8 u + u) A_j^2, and the m - 1 additions of the sum add at most (m - 1) u of the partial sums, each <= sum A_j^2:
    |h - h_exact| <= (m + 8) u sum_j A_j^2, asserted with a factor 1.01 for the second-order terms."""
    u = 2.0 ** -53
    worst = 0.0
    for m in range(1, FIT_MAX + 1):
        for degree in mc.DEGREES:
            p = min(degree, m - 1)
            h = margin_growth(m, degree, 63)
            assert h.shape == (64,) and h.dtype == np.float64
            for k in (0, 1, 4, 30, 63):
                exact, A2 = Fraction(0), Fraction(0)
                for j in range(m):
                    w = [Fraction(n, d) for n, d in mc.weights_int(m, p, j)] + [Fraction(0)] * 2
                    kk = Fraction(k * (k - 1) // 2)
                    exact += (w[0] + k * w[1] + kk * w[2]) ** 2
                    A2 += (abs(w[0]) + k * abs(w[1]) + kk * abs(w[2])) ** 2
                err, bound = abs(Fraction(float(h[k])) - exact), 1.01 * (m + 8) * u * float(A2)
                worst = max(worst, float(err) / bound)
                assert err <= bound, (m, degree, k, float(err), bound)
    print(f'h_k against exact rationals: worst error {worst:.3f} of its bound')
    assert np.array_equal(margin_growth(8, 2, 4), margin_growth(8, 2, 63)[:5])                  # node k does not depend on N
    assert np.array_equal(margin_growth(2, 2, 9), margin_growth(2, 1, 9)) and np.array_equal(margin_growth(1, 2, 9), np.ones(10))


@pytest.mark.parametrize('system', ['z1', 'fr7'])
def test_statement_equals_the_scalar_restatement_bit_for_bit(system):
    """the clock family of the polynomial tests (t < 0 and t past T included), windows {1, 2, 3, 4, 7, 32}, the three degrees, both
    arms: fixed-capsule rows on the one, capsule-sphere, sphere-sphere and plane rows on the other, so all four moving-slot sets"""
    N, B, T = 4, 3, 40
    par, prob, net = mc.problem(system, N)
    S = fc.world(prob, B, T, seed=2)
    z, prior, base, cap = 2.0, 1e-4, (0.003, 0.0005), 0.04
    sets = set()
    for c in mc.clocks(T):
        for window in mc.WINDOWS:
            for degree in mc.DEGREES:
                d = fit_margin_statement(prob, S, c, window, degree, z, prior, base, cap)
                assert d.shape == (B, N + 1, len(prob.rows)) and d.dtype == np.float64
                lo, hi = inflated_row_bounds(prob, B, d)
                for b in range(B):
                    for i, r in enumerate(prob.rows):
                        sets.add((r.kind, moving_slots(r.kind)))
                        want = mc.margin_scalar(S[b, :, i], r.kind, N, c, window, degree, z, prior, base, cap)
                        assert np.array_equal(_bits(d[b, :, i]), _bits(want)), (c, window, degree, b, i, d[b, :, i], want)
                        for k in range(N + 1):
                            assert (lo[b, k, i], hi[b, k, i]) == mc.bounds_scalar(r, want[k]), (c, window, degree, b, k, i)
    assert sorted(sets) == ([(0, (0, 1, 2, 3, 4, 5))] if system == 'z1' else [(2, (0, 1, 2)), (3, (0, 1, 2)), (4, (6,))])
    # the margins do depend on what was seen, on the row and on the node (the cap out of the way; above, some entries reach it)
    d = fit_margin_statement(prob, S, 20, 7, 1, z, prior, base, 0.5)
    assert (d[0] != d[1]).any() and (d[:, 1:] > d[:, :-1]).all() and d.max() < 0.5


# ---- 2. identities ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('system', ['z1', 'fr7'])
def test_a_world_the_fit_reproduces_leaves_the_base(system):
    """A world that is a polynomial of degree <= p is fitted without residual.  EXACTLY so where the fit's arithmetic is exact: the
    window mean over m = 2, 4, 8, 16, 32 columns of a constant dyadic world (weights 1 / m dyadic) -- there d == base bit for bit, and
    with base (0, 0) the bounds are the descriptor's doubles bit for bit.  Every other (m, p) has weights like 5 / 6 that are rounded, so
    a dyadic polynomial world leaves residuals of rounding size: |res| <= 2 (m + 4) u Y sum_j (|ua_j| + (m - 1) |uv_j| + (m (m - 1) / 2)
    |ue_j|), u = 2^-53, Y = max |y| (m rounded products and sums per accumulator, three accumulators recombined at ages up to
    m - 1), hence d - base <= z sqrt(m / nu) max|res| g_k: below 1e-9 m here, asserted from the bound and not from the result."""
    N, B, T = 4, 3, 40
    par, prob, net = mc.problem(system, N)
    lo0 = np.broadcast_to(prob.row_lb, (B, N + 1, len(prob.rows)))
    hi0 = np.broadcast_to(prob.row_ub, (B, N + 1, len(prob.rows)))
    S0 = mc.dyadic_world(prob, B, T, 0)
    for m in (2, 4, 8, 16, 32):
        d = fit_margin_statement(prob, S0, 35, m, 0, 3.0, 0.0, (0.0, 0.0), 0.05)
        assert not d.any()
        lo, hi = inflated_row_bounds(prob, B, d)
        assert lo.tobytes() == np.ascontiguousarray(lo0).tobytes() and hi.tobytes() == np.ascontiguousarray(hi0).tobytes()
        base = (0.004, 0.003)
        d = fit_margin_statement(prob, S0, 35, m, 0, 3.0, 0.0, base, 0.05)
        assert np.array_equal(d, np.broadcast_to((base[0] + base[1] * np.arange(N + 1.0))[None, :, None], d.shape))
    u = 2.0 ** -53
    for p in mc.DEGREES:
        S = mc.dyadic_world(prob, B, T, p)
        for m in (3, 4, 7, 32):
            if m - p - 1 < 1:
                continue
            us = list(poly_weights(m, p)) + [np.zeros(m)] * 2
            A = (np.abs(us[0]) + (m - 1) * np.abs(us[1]) + (m * (m - 1) / 2) * np.abs(us[2])).sum()
            res = 2 * (m + 4) * u * np.abs(S).max() * A
            g = np.sqrt(margin_growth(m, p, N))
            bound = 3.0 * np.sqrt(m / (m - p - 1)) * res * g
            d = fit_margin_statement(prob, S, 35, m, p, 3.0, 0.0, (0.0, 0.0), 0.05)
            assert (d <= bound[None, :, None]).all() and bound.max() < 1e-9, (p, m, d.max(), bound.max())


def test_nu_zero_gives_the_prior_z_zero_the_base_a_nan_the_cap_and_a_robot_row_keeps_its_bounds():
    N, B, T = 4, 3, 40
    par, prob, net = mc.problem('fr7', N)
    nr = len(prob.rows)
    S = fc.world(prob, B, T, seed=1)
    z, prior, base, cap = 2.0, 0.002, (0.001, 0.0005), 0.05
    ramp = base[0] + base[1] * np.arange(N + 1.0)
    # nu == 0: window <= p + 1 at any clock, and early clocks under any window
    for c, window, degree in ((20, 1, 0), (20, 2, 1), (20, 3, 2), (20, 1, 2), (0, 7, 2), (1, 7, 1), (2, 32, 2), (-5, 4, 0), (None, 4, 1)):
        t = 0 if c is None else c
        m = min(window, max(t, 0) + 1)
        p = min(degree, m - 1)
        assert m - p - 1 == 0
        d = fit_margin_statement(prob, S, c, window, degree, z, prior, base, cap)
        want = ramp + (z * np.sqrt(prior * prior)) * np.sqrt(margin_growth(m, p, N))
        want = np.where(want <= cap, want, cap)                                  # (a parabola through three columns reaches the cap)
        assert np.array_equal(d, np.broadcast_to(want[None, :, None], d.shape)), (c, window, degree)
    assert not fit_margin_statement(prob, S, 20, 3, 2, z, 0.0, (0.0, 0.0), cap).any()           # no prior, no base: no margin
    # z = 0: the base, whatever was seen
    d = fit_margin_statement(prob, S, 20, 7, 2, 0.0, prior, base, cap)
    assert np.array_equal(d, np.broadcast_to(ramp[None, :, None], d.shape))
    # a NaN sample in a moving slot of the window: the cap at every node of that (instance, row), nothing else moves
    ref = fit_margin_statement(prob, S, 20, 7, 2, z, prior, base, cap)
    i = next(k for k, r in enumerate(prob.rows) if r.kind == ROW_COORD)
    for row, slot in ((0, 1), (i, 6)):
        Sn = S.copy()
        Sn[1, 17, row, slot] = np.nan
        d = fit_margin_statement(prob, Sn, 20, 7, 2, z, prior, base, cap)
        assert (d[1, :, row] == cap).all() and np.isfinite(d).all()
        d[1, :, row] = ref[1, :, row]
        assert np.array_equal(d, ref)
        inflated_row_bounds(prob, B, fit_margin_statement(prob, Sn, 20, 7, 2, z, prior, base, cap))      # finite: a table can be formed
    for row, slot, col in ((0, 5, 17), (i, 0, 17), (0, 1, 13)):                  # a slot the kind does not read; a column outside the window
        Sn = S.copy()
        Sn[1, col, row, slot] = np.nan
        assert np.array_equal(fit_margin_statement(prob, Sn, 20, 7, 2, z, prior, base, cap), ref)
    # the cap is reached by size as well
    d = fit_margin_statement(prob, S, 20, 7, 2, 50.0, prior, base, 0.01)
    assert (d == 0.01).any() and d.max() == 0.01
    # a robot-robot row: d = 0 at every node, base included, and its bounds are the descriptor's
    prob2 = mc.with_robot_row(prob)
    S2 = np.concatenate([S, S[:, :, :1]], axis=2)
    d = fit_margin_statement(prob2, S2, 20, 7, 2, z, prior, base, cap)
    assert not d[:, :, nr].any() and np.array_equal(d[:, :, :nr], ref)
    lo, hi = inflated_row_bounds(prob2, B, d)
    assert (lo[:, :, nr] == prob2.rows[nr].lb).all() and (hi[:, :, nr] == prob2.rows[nr].ub).all()


@pytest.mark.parametrize('system', ['z1', 'fr7'])
def test_the_base_alone_is_the_table_of_row_margin(system):
    """z = 0 and no prior: inflated_row_bounds of the statement is the table run_mpc(row_margin=(a, b)) sets, bit for bit"""
    N, B = 4, 3
    par, prob, net = mc.problem(system, N)
    a, b = 0.004, 0.003
    S = fc.world(prob, B, 12)
    got = inflated_row_bounds(prob, B, fit_margin_statement(prob, S, 9, 7, 2, 0.0, 0.0, (a, b), 0.05))
    want = inflated_row_bounds(prob, B, a + b * np.arange(N + 1))
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()


def test_statement_value_errors():
    N, B = 4, 2
    par, prob, net = mc.problem('fr7', N)
    S = fc.world(prob, B, 12)
    ok = dict(window=4, degree=2, z=2.0, sigma_prior=0.0, base=(0.0, 0.0), d_max=0.05)
    for key, bad, match in [('window', 0, 'window 0'), ('window', FIT_MAX + 1, f'window {FIT_MAX + 1}'), ('degree', -1, 'degree -1'),
                            ('degree', 3, 'degree 3')]:
        with pytest.raises(ValueError, match=f'fit_margin_statement: {match}'):
            fit_margin_statement(prob, S, 3, **{**ok, key: bad})
    for key in ('z', 'sigma_prior', 'd_max'):
        for bad in (-1e-9, np.nan, np.inf):
            with pytest.raises(ValueError, match=f'fit_margin_statement: {key}='):
                fit_margin_statement(prob, S, 3, **{**ok, key: bad})
    for idx, name in ((0, 'base_a'), (1, 'base_b')):
        for bad in (-1e-9, np.nan, np.inf):
            base = [0.0, 0.0]
            base[idx] = bad
            with pytest.raises(ValueError, match=f'fit_margin_statement: {name}='):
                fit_margin_statement(prob, S, 3, **{**ok, 'base': tuple(base)})
    i = next(k for k, r in enumerate(prob.rows) if r.kind == ROW_COORD)
    r = prob.rows[i]
    assert abs(r.lb) < INF and abs(r.ub) < INF
    with pytest.raises(ValueError, match=rf'fit_margin_statement: row {i} \({re.escape(prob.row_names[i])}\).*cross'):
        fit_margin_statement(prob, S, 3, **{**ok, 'd_max': 0.5 * (r.ub - r.lb) + 1e-3})
    fit_margin_statement(prob, S, 3, **{**ok, 'd_max': 0.25 * (r.ub - r.lb)})
    with pytest.raises(ValueError, match='fit_margin_statement: expected a track'):
        fit_margin_statement(prob, S[:, :, :2], 3, **ok)
    assert FIT_MARGIN_CAP == 0.05


# ---- 3. the statistical claims ----------------------------------------------------------------------------------------------------------------
def _student_two_sided(nu, x=2.0):
    """P(|T_nu| <= x) by integrating the density with numpy (composite Simpson on 20 001 points: the integrand is smooth, the error
    far below 1e-9)"""
    from math import gamma, pi, sqrt
    t = np.linspace(-x, x, 20001)
    f = gamma((nu + 1) / 2) / (sqrt(nu * pi) * gamma(nu / 2)) * (1 + t * t / nu) ** (-(nu + 1) / 2)
    w = np.ones_like(t)
    w[1:-1:2], w[2:-1:2] = 4.0, 2.0
    return float((w * f).sum() * (t[1] - t[0]) / 3.0)


@pytest.mark.parametrize('m,p', [(16, 2), (8, 1)])
def test_the_interval_is_the_textbook_prediction_interval(m, p):
    """A plane row, so one moving slot: the offset follows a polynomial of degree p -- constant acceleration for p = 2, and constant
    velocity for the line, whose interval holds only for a world the model can follow -- seen through N(0, sigma^2), sigma = 1e-3,
    20 007 draws.  (1) the mean of s2 / sigma^2 is 1 within 5 standard errors, 5 sqrt(2 / (nu n)) (s2 nu / sigma^2 is chi-square with
    nu degrees of freedom).  (2) with z = 2 and no prior the share of draws with |forecast_k - truth_k| <= d_k at k = 0, 4, 30 is
    P(|T_nu| <= 2) of Student's t within 5 binomial standard errors: the forecast's error is N(0, sigma^2 h_k) and independent of s."""
    assert _student_two_sided(13) == pytest.approx(0.9332, abs(2e-4)) and _student_two_sided(6) == pytest.approx(0.9076, abs(2e-4))
    n, sigma, N, z = 20007, 1e-3, 30, 2.0
    par, prob, net = mc.problem('fr7', N)
    i = next(k for k, r in enumerate(prob.rows) if r.kind == ROW_COORD)
    nu, t = m - p - 1, m - 1
    tau = np.arange(m + N, dtype=float)
    truth = 0.3 + 0.004 * tau + (0.0002 * tau * tau if p == 2 else 0.0)            # [m + N]: columns 0..t seen, t + k forecast
    rng = np.random.default_rng(11)
    S = np.zeros((n, m, len(prob.rows), 8))
    S[:, :, i, 6] = truth[None, :m] + rng.normal(0.0, sigma, (n, m))
    d = fit_margin_statement(prob, S, t, m, p, z, 0.0, (0.0, 0.0), 0.5)[:, :, i]   # (the cap out of the way)
    g = np.sqrt(margin_growth(m, p, N))
    s2 = (d[:, 0] / (z * g[0])) ** 2
    mean, se = s2.mean() / sigma ** 2 - 1.0, np.sqrt(2.0 / (nu * n))
    print(f'(m, p) = ({m}, {p}): mean s2 / sigma^2 - 1 = {mean:+.4f}, standard error {se:.4f}')
    assert abs(mean) <= 5 * se
    F = poly_forecast_statement(S, t, N, m, p)[:, :, i, 6]
    want = _student_two_sided(nu)
    se = np.sqrt(want * (1 - want) / n)
    for k in (0, 4, 30):
        share = float((np.abs(F[:, k] - truth[t + k]) <= d[:, k]).mean())
        print(f'(m, p) = ({m}, {p}), k = {k}: coverage {share:.4f} against {want:.4f}, standard error {se:.4f}')
        assert abs(share - want) <= 5 * se, (k, share, want)


# ---- 4. the interface ----------------------------------------------------------------------------------------------------------------------------
class MarginRecorder(FitRecorder):
    """the recording double of the forecast tests that also writes down the row-bounds tables it is handed"""

    def set_instance_row_bounds(self, lo=None, hi=None):
        self.events.append(('row_bounds', None if lo is None else np.array(lo), None if hi is None else np.array(hi)))


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
        mk, mkb = tc.oracle_factories(pars[0], N, pars, geoms, log=solvers, solver_cls=MarginRecorder)

        def mk_scripted(name, batch):
            ctrl = mk(name, batch)
            ctrl.ocp_solver.scripted_status = [fail.copy() for _ in range(N)] + [np.zeros(B, np.int32)] * 8
            return ctrl
        return cl.run_mpc(pars[0], 'htwa', xg, ug, make_controller=mk_scripted, make_backup=mkb, n_steps=steps, scenes=world, **kw), solvers
    return run, pars, base, world, observed, N, steps, xg, ug


def test_run_mpc_row_margin_fit_on_the_host_path():
    """'htwa', 5 instances, 7 steps around the recording double, scripted failures make instances 1 and 3 abort at step N - 1.  Per
    step, behind the forecast and ahead of the solve: ONE table, inflated_row_bounds of the statement at time j from what was
    observed, with row_margin as its base; the backup handle gets the aborting rows' table over its own horizon at the event, behind
    its forecast and ahead of its one solve; both end with one clearing call.  None makes the calls of a run without the argument."""
    run, pars, base, world, observed, N, steps, xg, ug = _host_case()
    fit = (2.0, 0.003, 0.04)
    kw = dict(forecast='fit', forecast_window=2, forecast_degree=None, observed=observed)
    for rm in (None, (0.002, 0.001)):
        res, sv = run(row_margin_fit=fit, row_margin=rm, **kw)
        assert res['row_margin_fit'] == fit and res.get('row_margin') == rm
        main, back = sv['htwa'], sv['backup']
        ev = main.events
        solves = [k for k, e in enumerate(ev) if e[0] == 'solve']
        sets = [k for k, e in enumerate(ev) if e[0] == 'row_bounds']
        assert len(solves) == steps and len(sets) == steps + 1
        for j, k in enumerate(solves):
            before = ev[(solves[j - 1] if j else -1) + 1:k]
            kinds = [e[0] for e in before if e[0] in ('track', 'row_bounds')]
            assert kinds[-2:] == ['track', 'row_bounds'] and kinds.count('row_bounds') == 1, (j, kinds)
            d = fit_margin_statement(base, observed, j, 2, 1, *fit[:2], (0.0, 0.0) if rm is None else rm, fit[2])
            lo, hi = inflated_row_bounds(base, 5, d)
            got = [e for e in before if e[0] == 'row_bounds'][0]
            assert np.array_equal(got[1], lo) and np.array_equal(got[2], hi), j
            assert (lo > base.row_lb).any()                                                      # (the prior does make room)
        assert sets[-1] > solves[-1] and ev[sets[-1]][1] is None
        Nb = pars[0].back_hor
        bprob = C.OcpProblem(pars[0], 'backup', 'zero', N=Nb)
        bev = [e for e in back.events if e[0] in ('row_bounds', 'solve') or (e[0] == 'track' and e[1] is not None)]
        assert [e[0] for e in bev] == ['track', 'row_bounds', 'solve', 'row_bounds']
        d = fit_margin_statement(bprob, observed[[1, 3]], N - 1, 2, 1, *fit[:2], (0.0, 0.0) if rm is None else rm, fit[2])
        blo, bhi = inflated_row_bounds(bprob, 2, d)
        assert np.array_equal(bev[1][1], blo) and np.array_equal(bev[1][2], bhi) and bev[3][1] is None
        assert res['x_viable'].shape[0] == 2
    ref, sv_ref = run(**kw)
    none, sv_none = run(row_margin_fit=None, **kw)
    assert 'row_margin_fit' not in ref and 'row_margin_fit' not in none
    for name in ('htwa', 'backup'):
        assert _same_events(sv_none[name].events, sv_ref[name].events), name
        assert not any(e[0] == 'row_bounds' for e in sv_ref[name].events)
        assert not _same_events(sv[name].events, sv_ref[name].events), name


def test_run_mpc_value_errors_and_result_file_names():
    run, pars, base, world, observed, N, steps, xg, ug = _host_case()
    fit = (2.0, 0.0, 0.04)
    for fcst in (None, 'cv', 'hold', 'true'):
        with pytest.raises(ValueError, match="row_margin_fit: forecast=.* it goes with forecast='fit'"):
            run(row_margin_fit=fit, forecast=fcst)
    for bad in ((2.0, 0.0), (2.0, 0.0, 0.04, 1.0), (-1.0, 0.0, 0.04), (2.0, np.nan, 0.04), (2.0, 0.0, np.inf)):
        with pytest.raises(ValueError, match=r'row_margin_fit: expected \(z, sigma_prior, d_max\)'):
            run(row_margin_fit=bad, forecast='fit', forecast_window=4)
    mk, mkb = tc.oracle_factories(pars[0], N, pars, _loop_setup()[2])
    with pytest.raises(ValueError, match="the 'parallel' policy is not supported"):         # (its scenes are refused first)
        cl.run_mpc(pars[0], 'parallel', xg, ug, row_margin_fit=fit, forecast='fit', scenes=world, make_controller=mk, make_backup=mkb,
                   n_steps=2)
    with pytest.raises(ValueError, match='row_margin_fit: TrackOracleSolver has no set_instance_row_bounds'):
        cl.run_mpc(pars[0], 'htwa', xg, ug, row_margin_fit=fit, forecast='fit', scenes=world, make_controller=mk, make_backup=mkb,
                   n_steps=2)
    args = (pars[0], 'z1', 'htwa', 6, True, 0.0, 0.0, 0, 0)
    plain = cl.result_file(*args, forecast='fit', forecast_window=4)
    assert cl.result_file(*args, forecast='fit', forecast_window=4, row_margin_fit=None) == plain
    assert cl.result_file(*args, forecast='fit', forecast_window=4, row_margin_fit=(2, 0.001, 0.05)) == \
        plain.replace('_mpc.pkl', '_rmf2.0_p0.001_c0.05_mpc.pkl')
    assert cl.result_file(*args, forecast='fit', forecast_window=4, row_margin=(0.01, 0.002), row_margin_fit=(2, 0.001, 0.05)).endswith(
        '_rm0.01_g0.002_rmf2.0_p0.001_c0.05_mpc.pkl')


def test_mpc_script_takes_row_margin_z(monkeypatch, tmp_path):
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
    base = ['-c', 'naive', '--horizon', str(N), '--scene-velocity', '0.3', '--scene-forecast', 'fit', '--forecast-window', '6']
    mpc = _script('mpc')
    assert mpc.main(base) == 0
    assert 'row_margin_fit' not in seen['kw'] and 'row_margin_fit' not in names[-1][1]  # without the flag: the call and name of before
    plain = names[-1][0]
    assert mpc.main(base + ['--row-margin-z', '2']) == 0
    assert seen['kw']['row_margin_fit'] == (2.0, 0.0, FIT_MARGIN_CAP) and 'row_margin' not in seen['kw']
    assert names[-1][0] == plain.replace('_mpc.pkl', f'_rmf2.0_p0.0_c{FIT_MARGIN_CAP}_mpc.pkl')
    assert mpc.main(base + ['--row-margin-z', '3', '--row-margin-prior', '0.002', '--row-margin-cap', '0.03', '--row-margin', '0.01']) == 0
    assert seen['kw']['row_margin_fit'] == (3.0, 0.002, 0.03) and seen['kw']['row_margin'] == (0.01, 0.0)
    assert names[-1][0] == plain.replace('_mpc.pkl', '_rm0.01_rmf3.0_p0.002_c0.03_mpc.pkl')
    for flag in ('--row-margin-prior', '--row-margin-cap'):
        with pytest.raises(SystemExit, match=f'{flag} needs --row-margin-z'):
            mpc.main(base + [flag, '0.01'])
    with pytest.raises(SystemExit, match='--row-margin-z needs --scene-forecast fit'):
        mpc.main(['-c', 'naive', '--horizon', str(N), '--scene-velocity', '0.3', '--scene-forecast', 'cv', '--row-margin-z', '2'])
    with pytest.raises(SystemExit, match="--row-margin-z: the 'parallel' policy is not supported"):
        mpc.main(['-c', 'parallel'] + base[2:] + ['--row-margin-z', '2'])
    with pytest.raises(SystemExit, match='not negative'):
        mpc.main(base + ['--row-margin-z', '-1'])


def test_the_new_symbols_are_declared_exported_and_prototyped():
    from safe_mpc_amd import _lib, solver
    hdr = open(os.path.join(ROOT, 'include', 'smpc.h')).read()
    declared = set(re.findall(r'^(?:int|void|const char\*|void\*) (smpc_\w+)\(', hdr, re.M))
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('smpc_forecast_row_margin', 'smpc_get_instance_row_bounds'):
        assert name in declared and name in _lib.SYMBOLS and hasattr(L, name), name
    vp, i, dbl = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    assert _lib.lib().smpc_forecast_row_margin.argtypes == [vp, i, i, i, dbl, dbl, dbl, dbl, dbl]
    assert _lib.lib().smpc_get_instance_row_bounds.argtypes == [vp, i, vp, vp, i]
    assert callable(solver.BatchedOcpSolver.forecast_row_margin) and callable(solver.BatchedOcpSolver.get_instance_row_bounds)
    L.smpc_abi_version.restype = ctypes.c_int
    assert L.smpc_abi_version() == 5             # nothing existing changed
    for flag in ('interval-kernel', 'interval-loop'):
        assert flag in open(os.path.join(ROOT, 'scripts', 'forecast_bench.py')).read()
