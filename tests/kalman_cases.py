"""Shared pieces of the obstacle-filter tests (test_forecast_kalman_host.py, test_forecast_kalman_gpu.py), on top
of forecast_cases and margin_cases: the definition once more for ONE record with Python floats, the recursion and its least-squares
meaning in exact rationals, worlds with NaN bursts, and a recording double.  Not a test module.

The principle: ``problem.kalman_statement`` / ``kalman_margin_statement`` are the definition, ``k_scene_kalman`` / ``k_kalman_margin``
repeat them operation for operation -- every product rounded before its sum, one division per record and step -- so worlds with full
mantissas (forecast_cases.world) show a contraction, another order of the sums or a second division in the last bit."""
import math
from fractions import Fraction

import numpy as np

import margin_cases as mc
from safe_mpc_amd.problem import KALMAN_REC, kalman_params, moving_slots

problem = mc.problem
DEGREES = (0, 1, 2)
PAR = {0: kalman_params(0, 0.004, 0.01, 0.02, 0.005, 0.25), 1: kalman_params(1, 0.003, 0.01, 0.02, 0.005, 0.25),
       2: kalman_params(2, 0.0007, 0.01, 0.02, 0.005, 0.25)}
MARGIN = dict(z=2.0, base=(0.003, 0.0005), d_max=0.04)


def noise_scalar(par):
    p, q = par.degree, float(par.q)
    G = [[1.0], [0.5, 1.0], [1.0 / 6.0, 0.5, 1.0]][p]
    gq = [q * g for g in G] + [0.0] * (2 - p)
    return [gq[0] * gq[0], gq[0] * gq[1], gq[0] * gq[2], gq[1] * gq[1], gq[1] * gq[2], gq[2] * gq[2]]


def predict_cov_scalar(p, P, Q, half=0.5):
    """Phi P Phi' + Q on six numbers of any field (floats, Fractions): rows of Phi P, times Phi', plus Q"""
    P00, P01, P02, P11, P12, P22 = P
    if p == 0:
        return [P00 + Q[0], P01, P02, P11, P12, P22]
    if p == 1:
        a00, a01 = P00 + P01, P01 + P11
        return [(a00 + a01) + Q[0], a01 + Q[1], P02, P11 + Q[3], P12, P22]
    a00 = (P00 + P01) + half * P02
    a01 = (P01 + P11) + half * P12
    a02 = (P02 + P12) + half * P22
    a11, a12 = P11 + P12, P12 + P22
    return [((a00 + a01) + half * a02) + Q[0], (a01 + a02) + Q[1], a02 + Q[2], (a11 + a12) + Q[3], a12 + Q[4], P22 + Q[5]]


def step_scalar(rec, y, kind, par, advance=True):
    """the definition once more for ONE record ``rec`` (a list of KALMAN_REC Python floats) and one sample y[0..7]: the record after"""
    rec = [float(v) for v in rec]
    if not advance:
        return rec
    p = par.degree
    pos, vel, acc, P, s2, n = rec[0:8], rec[8:16], rec[16:24], rec[24:30], rec[30], rec[31]
    slots = moving_slots(kind)
    obs = not any(float(y[s]) != float(y[s]) for s in slots)
    r2 = float(par.r) * float(par.r)
    if not n >= 1.0:
        if not obs:
            return rec
        P0 = [r2, 0.0, 0.0, float(par.v0) * float(par.v0) if p >= 1 else 0.0, 0.0, float(par.a0) * float(par.a0) if p == 2 else 0.0]
        return [float(v) for v in y] + [0.0] * 16 + P0 + [1.0, 1.0]
    Q = noise_scalar(par)
    for s in range(8):
        if p == 1:
            pos[s] = pos[s] + vel[s]
        if p == 2:
            pos[s] = (pos[s] + vel[s]) + 0.5 * acc[s]
            vel[s] = vel[s] + acc[s]
    P = predict_cov_scalar(p, P, Q)
    if obs:
        inv = 1.0 / (P[0] + r2)
        K = [P[0] * inv, P[1] * inv, P[2] * inv]
        nis = 0.0
        for s in range(8):
            nu = float(y[s]) - pos[s]
            pos[s] = pos[s] + K[0] * nu
            if p >= 1:
                vel[s] = vel[s] + K[1] * nu
            if p == 2:
                acc[s] = acc[s] + K[2] * nu
            if s in slots:
                x = (nu * nu) * inv
                nis = x if (x > nis or x != x) else nis
        M = list(P)
        P[0] = M[0] - K[0] * M[0]
        if p >= 1:
            P[1] = M[1] - K[0] * M[1]
            P[3] = M[3] - K[1] * M[1]
        if p == 2:
            P[2] = M[2] - K[0] * M[2]
            P[4] = M[4] - K[1] * M[2]
            P[5] = M[5] - K[2] * M[2]
        s2 = s2 + float(par.beta) * (nis - s2)
        s2 = 1.0 if s2 < 1.0 else s2
        n = n + 1.0
    return pos + vel + acc + P + [s2, n]


def forecast_scalar(rec, p, N):
    """[N + 1][8] from one record, by repeated addition"""
    pos, vel, acc = list(rec[0:8]), list(rec[8:16]), list(rec[16:24])
    out = [list(pos)]
    v = [vel[s] + 0.5 * acc[s] for s in range(8)] if p == 2 else vel
    for k in range(1, N + 1):
        if p >= 1:
            pos = [pos[s] + v[s] for s in range(8)]
        if p == 2:
            v = [v[s] + acc[s] for s in range(8)]
        out.append(list(pos))
    return np.array(out)


def margin_scalar(rec, kind, par, N, z, base=(0.0, 0.0), d_max=0.05):
    """[N + 1] margins of one record"""
    if not moving_slots(kind):
        return np.zeros(N + 1)
    Pi, Q = [float(v) for v in rec[24:30]], noise_scalar(par)
    s2 = float(rec[30])
    zs = float(z) * (math.sqrt(s2) if s2 >= 0.0 else float('nan'))
    out = []
    for k in range(N + 1):
        g = math.sqrt(Pi[0]) if Pi[0] >= 0.0 else float('nan')
        d = (float(base[0]) + float(base[1]) * float(k)) + zs * g
        out.append(d if d <= d_max else float(d_max))
        Pi = predict_cov_scalar(par.degree, Pi, Q)
    return np.array(out)


# ---- exact rationals ------------------------------------------------------------------------------------------------------------------------
class Err:
    """A float computation followed in exact rationals: ``val`` is what exact arithmetic gives on the exact inputs, ``err`` a bound on
    |computed float - val|, carried operation by operation.  With u = 2^-53 one rounded operation returns fl(x) with
    |fl(x) - x| <= u |x|, x the exact result on the COMPUTED operands, |x| <= |val| + (propagated error): so
        a + b:  e = (ea + eb)(1 + u) + u |a + b|
        a b:    e = (|a| eb + |b| ea + ea eb)(1 + u) + u |a b|
        1 / a:  e = ea / (|a| (|a| - ea)) (1 + u) + u / |a|           (ea < |a| asserted)
    -- no first-order shortcut, so the bound is rigorous for the operations counted.  The bound itself is kept as a float, each of its
    own operations blown up by UP = 1 + 2^-40 (far more than the float operations lose), which keeps the rationals small."""
    U = 2.0 ** -53
    UP = 1.0 + 2.0 ** -40

    def __init__(self, val, err=0.0):
        self.val, self.err = Fraction(val), float(err)
        self.mag = abs(float(self.val)) * Err.UP

    @staticmethod
    def of(x):
        return x if isinstance(x, Err) else Err(x)

    def __add__(self, o):
        o = Err.of(o)
        out = Err(self.val + o.val)
        out.err = ((self.err + o.err) * (1 + Err.U) + Err.U * out.mag) * Err.UP
        return out
    __radd__ = __add__

    def __sub__(self, o):
        o = Err.of(o)
        return self + Err(-o.val, o.err)

    def __mul__(self, o):
        o = Err.of(o)
        out = Err(self.val * o.val)
        out.err = ((self.mag * o.err + o.mag * self.err + self.err * o.err) * (1 + Err.U) + Err.U * out.mag) * Err.UP
        return out
    __rmul__ = __mul__

    def inverse(self):
        low = abs(float(self.val)) / Err.UP          # (a lower bound on |val| for the denominators)
        assert self.err < low
        out = Err(1 / self.val)
        out.err = (self.err / (low * (low - self.err)) * (1 + Err.U) + Err.U * out.mag) * Err.UP
        return out


def rational_filter(ys, p, q, r, v0, a0, num=Fraction):
    """the recursion for one scalar series ys (newest last), every sample observed: (x [3], P [6]) after all of them -- in exact
    Fractions, or with ``num=Err`` in the statement's own operations with a running bound on what float64 makes of them (the inputs
    must then be floats' exact values)"""
    F = Fraction
    one, half = num(1), num(F(1, 2))
    inverse = (lambda v: v.inverse()) if num is Err else (lambda v: 1 / v)
    q, r, v0, a0 = num(F(q)), num(F(r)), num(F(v0)), num(F(a0))
    sixth = Err(F(1, 6), float(abs(F(1.0 / 6.0) - F(1, 6))) * Err.UP) if num is Err else F(1, 6)
    G = [[one], [half, one], [sixth, half, one]][p]
    gq = [q * g for g in G] + [num(0)] * (2 - p)
    Q = [gq[i] * gq[j] for i, j in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))]
    r2 = r * r
    x = [num(F(ys[0])), num(0), num(0)]
    P = [r2, num(0), num(0), v0 * v0 if p >= 1 else num(0), num(0), a0 * a0 if p == 2 else num(0)]
    for y in ys[1:]:
        if p == 1:
            x = [x[0] + x[1], x[1], x[2]]
        if p == 2:
            x = [(x[0] + x[1]) + half * x[2], x[1] + x[2], x[2]]
        P = predict_cov_scalar(p, P, Q, half=half)
        inv = inverse(P[0] + r2)
        K = [P[0] * inv, P[1] * inv, P[2] * inv]
        nu = num(F(y)) - x[0]
        x = [x[i] + K[i] * nu if i <= p else x[i] for i in range(3)]
        M = list(P)
        P = [M[0] - K[0] * M[0], M[1] - K[0] * M[1], M[2] - K[0] * M[2], M[3] - K[1] * M[1], M[4] - K[1] * M[2], M[5] - K[2] * M[2]]
        P = [P[i] if on else M[i] for i, on in enumerate((True, p >= 1, p == 2, p >= 1, p == 2, p == 2))]
    return x, P


def rational_least_squares(ys, p, r, v0, a0):
    """The minimiser of  sum_j (y_j - f(-j))^2 / r^2 + vel_init^2 / v0^2 + acc_init^2 / a0^2  over the state NOW (pos, vel, acc), and
    the inverse of that problem's normal matrix, by a rational solve.  ys newest last; the sample of age j is ys[-1 - j];
    f(tau) = pos + vel tau + acc tau^2 / 2, and the state at the first sample (age n - 1) is what the prior is about:
    vel_init = vel - (n - 1) acc, acc_init = acc."""
    F = Fraction
    n, d = len(ys), p + 1
    r, v0, a0 = F(r), F(v0), F(a0)
    rows, rhs, wts = [], [], []
    for j in range(n):
        tau = F(-j)
        rows.append([F(1), tau, tau * tau / 2][:d])
        rhs.append(F(ys[-1 - j]))
        wts.append(1 / (r * r))
    if p >= 1:
        rows.append([F(0), F(1), F(-(n - 1))][:d])
        rhs.append(F(0))
        wts.append(1 / (v0 * v0))
    if p == 2:
        rows.append([F(0), F(0), F(1)])
        rhs.append(F(0))
        wts.append(1 / (a0 * a0))
    A = [[sum(w * row[i] * row[j] for row, w in zip(rows, wts)) for j in range(d)] for i in range(d)]
    bvec = [sum(w * row[i] * y for row, w, y in zip(rows, wts, rhs)) for i in range(d)]
    inv = _rational_inverse(A)
    x = [sum(inv[i][j] * bvec[j] for j in range(d)) for i in range(d)]
    return x, inv


def _rational_inverse(A):
    d = len(A)
    M = [list(row) + [Fraction(int(i == j)) for j in range(d)] for i, row in enumerate(A)]
    for c in range(d):
        piv = next(i for i in range(c, d) if M[i][c] != 0)
        M[c], M[piv] = M[piv], M[c]
        M[c] = [v / M[c][c] for v in M[c]]
        for i in range(d):
            if i != c and M[i][c] != 0:
                M[i] = [a - M[i][c] * b for a, b in zip(M[i], M[c])]
    return [row[d:] for row in M]


# ---- worlds ------------------------------------------------------------------------------------------------------------------------------------
def bursts(prob, S, spans):
    """``S`` with NaN in the moving slots of every row over the columns of ``spans`` = [(instance, first, last + 1), ...]; and a NaN in
    a slot NO row kind of the problem reads as moving (slot 7), in every column of instance 0 -- it must not unobserve a record"""
    out = np.array(S, float)
    for b, lo, hi in spans:
        for i, r in enumerate(prob.rows):
            for s in moving_slots(r.kind):
                out[b, lo:hi, i, s] = np.nan
    return out


def kinds(prob):
    return [int(r.kind) for r in prob.rows]


def run_statement(prob, S, par, N, clocks, state=None):
    """the statement carried over ``clocks`` (a list of scene-clock values): [(state, F) after each]"""
    from safe_mpc_amd.problem import kalman_statement, scene_column
    st = np.zeros((S.shape[0], len(prob.rows), KALMAN_REC)) if state is None else np.array(state, float)
    out = []
    for c in clocks:
        st, F = kalman_statement(st, S[:, scene_column(c, S.shape[1])], kinds(prob), par, N)
        out.append((st, F))
    return out


# ---- the recording double ------------------------------------------------------------------------------------------------------------------
def recorder_class():
    """fake_solver's oracle double (through the recorders of the forecast tests, which subclass it) that also writes down the
    row-bounds tables it is handed and every world, observed track or engine forecast -- none of which the host path may hand it"""
    from test_forecast_fit_host import FitRecorder

    class KalmanRecorder(FitRecorder):
        def set_instance_row_bounds(self, lo=None, hi=None):
            self.events.append(('row_bounds', None if lo is None else np.array(lo), None if hi is None else np.array(hi)))

        def forecast_scene_kalman(self, *a, **kw):
            self.events.append(('engine_kalman',))

        def kalman_row_margin(self, *a, **kw):
            self.events.append(('engine_kalman_margin',))
    return KalmanRecorder
