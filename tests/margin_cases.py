"""Shared pieces of the fitted-margin tests (test_forecast_margin_host.py, test_forecast_margin_gpu.py), on top of
forecast_cases, poly_forecast_cases and row_bounds_cases: the two arms, the definition once more for one (instance, row) with Python
floats and integer formulas, worlds that are exact polynomials, and a problem stand-in with a robot-robot row.  Not a test module.

The principle: ``problem.fit_margin_statement`` is the definition, ``k_fit_margin`` repeats it operation for operation -- every
product rounded before its sum -- so the worlds of forecast_cases (full mantissas in all eight slots) show a contraction, or another
order of the sums, in the last bit."""
import math
import types

import numpy as np

import poly_forecast_cases as pf
import row_bounds_cases as rb
from safe_mpc_amd.problem import INF, ROW_COORD, ROW_SEG_SEG, moving_slots

DEGREES = pf.DEGREES
WINDOWS = pf.WINDOWS
clocks = pf.clocks


def problem(system, N):
    """(par, prob, net) of row_bounds_cases: the Z1-class arm (six fixed-capsule rows) or the 7-DoF arm (two capsule-sphere rows, a
    sphere-sphere row and a plane row with both sides present) -- together the four non-empty moving-slot sets"""
    return rb.problem(system, N)


def weights_int(m, p, j):
    """the weights of age j as (numerator, denominator) pairs of integers, one pair per accumulator of the effective degree p"""
    if p == 0:
        return ((1, m),)
    if p == 1:
        return ((4 * m - 2 - 6 * j, m * (m + 1)), (6 * (m - 1) - 12 * j, m * (m * m - 1)) if m > 1 else (0, 1))
    return pf.ua_int(m, j), pf.uv_int(m, j), pf.ue_int(m, j)


def _w(m, p, j):
    if p == 0:
        return (1.0 / float(m),)
    return tuple(float(n) / float(d) for n, d in weights_int(m, p, j))


def margin_scalar(y, kind, N, t, window, degree, z, sigma_prior=0.0, base=(0.0, 0.0), d_max=0.05):
    """the definition once more for ONE record series y[0..T-1][0..7] of a row of ``kind``, with Python floats: [N + 1] margins"""
    T = len(y)
    t = 0 if t is None else min(max(int(t), -2 ** 62), 2 ** 62)
    m = min(window, max(t, 0) + 1)
    p = min(degree, m - 1)
    nu = m - p - 1
    col = lambda c: min(max(c, 0), T - 1)
    slots = moving_slots(kind)
    if not slots:
        return np.zeros(N + 1)
    var_prior = float(sigma_prior) * float(sigma_prior)
    s2 = var_prior
    if nu >= 1:
        rss = 0.0
        for s in slots:
            acc = None
            for j in range(m):
                yj = float(y[col(t - j)][s])
                w = _w(m, p, j)
                acc = [u * yj for u in w] if j == 0 else [x + u * yj for x, u in zip(acc, w)]
            q = None
            for j in range(m):
                yj = float(y[col(t - j)][s])
                if p == 0:
                    f = acc[0]
                elif p == 1:
                    f = acc[0] - float(j) * acc[1]
                else:
                    f = (acc[0] - float(j) * acc[1]) + float(j * (j + 1) // 2) * acc[2]
                res = yj - f
                q = res * res if j == 0 else q + res * res
            rss = q if (q > rss or q != q) else rss
        v = rss / float(nu)
        s2 = v if (v > var_prior or v != v) else var_prior
    s = math.sqrt(s2) if s2 == s2 else float('nan')
    out = []
    for k in range(N + 1):
        h = None
        for j in range(m):
            w = _w(m, p, j)
            if p == 0:
                c = w[0]
            elif p == 1:
                c = w[0] + float(k) * w[1]
            else:
                c = (w[0] + float(k) * w[1]) + float(k * (k - 1) // 2) * w[2]
            h = c * c if j == 0 else h + c * c
        d = (float(base[0]) + float(base[1]) * float(k)) + (float(z) * s) * math.sqrt(h)
        out.append(d if d <= d_max else float(d_max))
    return np.array(out)


def bounds_scalar(row, d):
    """inflated_row_bounds once more for one row and one margin"""
    lo, hi = row.lb, row.ub
    if d != 0.0:
        if row.kind == ROW_COORD:
            lo = row.lb + d if abs(row.lb) < INF else lo
            hi = row.ub - d if abs(row.ub) < INF else hi
        elif row.kind != ROW_SEG_SEG and abs(row.lb) < INF:
            lo = (math.sqrt(row.lb) + d) * (math.sqrt(row.lb) + d)
    return lo, hi


def dyadic_world(prob, B, T, degree):
    """[B, T, n_rows, 8]: every slot an exact polynomial of ``degree`` in the column index with small dyadic coefficients around a
    dyadic base, so that every sum and product of a fit over it is exact in float64 and the fit reproduces it: residual 0"""
    b, j, r, s = np.meshgrid(np.arange(B), np.arange(T), np.arange(len(prob.rows)), np.arange(8), indexing='ij')
    W = 0.25 + (b + 2 * r + s) / 64.0
    if degree >= 1:
        W = W + j * ((1 + b + s) / 256.0)
    if degree >= 2:
        W = W - j * j * ((1 + r) / 1024.0)
    return np.ascontiguousarray(W)


def with_robot_row(prob):
    """a stand-in for ``prob`` as the statement and inflated_row_bounds read it, with one robot-robot row (SEG_SEG, no world-fixed
    element) appended"""
    r = types.SimpleNamespace(kind=ROW_SEG_SEG, lb=0.05 ** 2, ub=1e6)
    return types.SimpleNamespace(N=prob.N, rows=list(prob.rows) + [r], row_names=list(prob.row_names) + ['forearm-ee'],
                                 row_obstacle=list(prob.row_obstacle) + [None], row_lb=np.append(prob.row_lb, r.lb),
                                 row_ub=np.append(prob.row_ub, r.ub))
