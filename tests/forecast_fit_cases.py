"""Shared pieces of the line-fit forecast tests (test_forecast_fit_host.py, test_forecast_fit_gpu.py), on top of
forecast_cases: the windows, the clock family with clocks that fill a 32-sample window, the statement of what every forecast call
reads ("what was seen"), and the fit's own restatement with Python floats.  Not a test module.

The principle: ``problem.fit_forecast_statement`` is the definition, ``k_scene_fit`` repeats it bit for bit -- every product rounded
before its sum, which a fused multiply-add would not do, so the worlds of forecast_cases (full mantissas in all eight slots) show a
contraction in the last bit."""
import numpy as np

import forecast_cases as fc
from safe_mpc_amd.problem import fit_forecast_statement, fit_weights, forecast_statement

WINDOWS = (1, 2, 3, 7, 32)


def clocks(T):
    """forecast_cases.clocks and the clocks at which windows of 7 and 32 samples are full or nearly so (where the track has them)"""
    return fc.clocks(T) + [t for t in (6, 31, 39) if t < T + 8]


def seen_statement(world, observed, t, N, kind):
    """what a forecast call of ``kind`` ('hold', 'cv', 'true', or an int: the fit's window) gives with this world and this observed
    track (None: none set): 'true' reads the world, everything else what was seen"""
    S = world if observed is None else observed
    if isinstance(kind, str):
        return forecast_statement(world if kind == 'true' else S, t, N, kind)
    return fit_forecast_statement(S, t, N, kind)


def fit_scalar(y, window, t, N):
    """the definition once more for ONE series y[0..T-1], with Python floats and integer formulas: [N + 1] forecasts"""
    T = len(y)
    t = 0 if t is None else min(max(int(t), -2 ** 62), 2 ** 62)
    m = min(window, max(t, 0) + 1)
    col = lambda c: min(max(c, 0), T - 1)
    a = d = None
    for j in range(m):
        u = float(4 * m - 2 - 6 * j) / float(m * (m + 1))
        w = 0.0 if m == 1 else float(6 * (m - 1) - 12 * j) / float(m * (m * m - 1))
        yj = float(y[col(t - j)])
        a, d = (u * yj, w * yj) if j == 0 else (a + u * yj, d + w * yj)
    out = [a]
    for _ in range(N):
        out.append(out[-1] + d)
    return np.array(out)


def node_sigma(m, k):
    """the standard deviation of node k's forecast error per unit of independent observation noise: sqrt(sum_j (u_j + k w_j)^2)"""
    u, w = fit_weights(m)
    return float(np.sqrt(((u + k * w) ** 2).sum()))
