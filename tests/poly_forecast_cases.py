"""Shared pieces of the polynomial forecast tests (test_forecast_poly_host.py, test_forecast_poly_gpu.py), on top
of forecast_cases and forecast_fit_cases: the degrees, the windows, the clock family, the definition once more for one series with
Python floats and integer formulas, and the noise gain of a node.  Not a test module.

The principle: ``problem.poly_forecast_statement`` is the definition, ``k_scene_poly`` repeats it bit for bit -- every product rounded
before its sum -- so the worlds of forecast_cases (full mantissas in all eight slots) show a contraction in the last bit."""
import numpy as np

import forecast_fit_cases as ff
from safe_mpc_amd.problem import poly_weights

DEGREES = (0, 1, 2)
WINDOWS = (1, 2, 3, 4, 7, 32)

clocks = ff.clocks              # forecast_cases.clocks and the clocks that leave m at 7 and 32 (and, at 1 and T - 2, at 2 and 3)


def ua_int(m, j):
    return 3 * (3 * m * m - 3 * m + 2) - 18 * (2 * m - 1) * j + 30 * j * j, m * (m + 1) * (m + 2)


def uv_int(m, j):
    return (36 * m ** 3 - 96 * m * m + 36 * m + 24) + (-192 * m * m + 180 * m + 48) * j + 180 * m * j * j, m * (m * m - 1) * (m * m - 4)


def ue_int(m, j):
    return 60 * ((m - 1) * (m - 2) - 6 * (m - 1) * j + 6 * j * j), m * (m * m - 1) * (m * m - 4)


def poly_scalar(y, window, degree, t, N):
    """the definition once more for ONE series y[0..T-1], with Python floats and integer formulas: [N + 1] forecasts"""
    T = len(y)
    t = 0 if t is None else min(max(int(t), -2 ** 62), 2 ** 62)
    m = min(window, max(t, 0) + 1)
    p = min(degree, m - 1)
    col = lambda c: min(max(c, 0), T - 1)
    if p == 1:
        return ff.fit_scalar(y, m, t, N)
    a = v = e = None
    for j in range(m):
        yj = float(y[col(t - j)])
        if p == 0:
            u = 1.0 / float(m)
            a = u * yj if j == 0 else a + u * yj
            continue
        (na, da), (nv, dv), (ne, de) = ua_int(m, j), uv_int(m, j), ue_int(m, j)
        wa, wv, we = float(na) / float(da), float(nv) / float(dv), float(ne) / float(de)
        a, v, e = (wa * yj, wv * yj, we * yj) if j == 0 else (a + wa * yj, v + wv * yj, e + we * yj)
    out = [a]
    for _ in range(N):
        if p == 0:
            out.append(a)
        else:
            out.append(out[-1] + v)
            v = v + e
    return np.array(out)


def node_sigma(m, p, k):
    """the standard deviation of node k's forecast error per unit of independent observation noise, for m samples and the effective
    degree p: sqrt(sum_j (ua_j + k uv_j + k (k - 1) / 2 ue_j)^2), with the weights a degree does not have taken as zero"""
    us = poly_weights(m, p)
    g = us[0].copy()
    if len(us) > 1:
        g = g + k * us[1]
    if len(us) > 2:
        g = g + k * (k - 1) / 2 * us[2]
    return float(np.sqrt((g ** 2).sum()))
