"""Multi-start inverse kinematics with collision rows: the numpy statement of ``smpc_ik_batch`` (include/smpc.h).

The problem per instance b is the one ``InverseKinematicsOCP`` states (ocp.py:321-326 of the reference): a joint configuration q
inside the box whose end-effector point sits at ``target[b]`` and whose collision rows are within their bounds; the caller
appends the zero velocity.  The reference hands it to IPOPT, one instance at a time.  Here S starts per instance run a projected
Levenberg-Marquardt iteration side by side -- ``ik_batch_host`` is the same algorithm as the kernel ``k_ik`` (csrc/kernels_ik.hpp),
FP64, vectorised over (b, s), and the statement the kernel is tested against.  It is also what :func:`ik` runs for a solver
without a device entry point.

Per start, with r(q) the stacked residual
  * ee(q) - target                                                                                    (3 entries)
  * w (lb' - v_r(q)) for every row below its PUSHED lower bound lb' = lb + push |lb|  (= lb (1 + push) for the squared
    distances, whose lb > 0), w (v_r(q) - ub') for every row above ub' = ub - push |ub|, w = 1 / max(sqrt|bound|, 1e-3);
    a bound with |.| >= SMPC_INF is absent
and F = |r|^2:
  q <- clip(q_start)  (a non-finite start component becomes the middle of its interval);  lam <- damping
  repeat max_iter times:  dq = -(J^T J + lam I)^-1 J^T r  (Cholesky);  q' = clip(q + dq)
                          F(q') < F(q):  q <- q', lam <- max(lam * damping_accept, damping_min)
                          otherwise:     lam <- min(lam * damping_reject, damping_max)
A start SUCCEEDS when at its final point |ee - target|_inf <= tol_ee and every row is within its UNPUSHED bounds.  The winner is
the successful start with the lowest index; without one, the start with the least final F (ties: lowest index).
"""
from __future__ import annotations

import numpy as np

from .problem import INF, ROW_COORD, ROW_POINT_POINT, ROW_SEG_FIXEDSEG, ROW_SEG_POINT, ROW_SEG_SEG

IK_DEFAULTS = dict(max_iter=40, tol_ee=1e-6, push=1e-2, damping=1e-2, damping_accept=0.3, damping_reject=4.0, damping_min=1e-9,
                   damping_max=1e6)
MAX_STARTS = 64


def ik_params(problem, **over):
    """The parameters of an IK call: IK_DEFAULTS, the model's joint box (ocp.py:321) and the OCP's row bounds (ocp.py:325-326),
    each overridable by name (q_lo, q_hi [nq]; row_lb, row_ub [n_rows])."""
    unknown = set(over) - set(IK_DEFAULTS) - {'q_lo', 'q_hi', 'row_lb', 'row_ub'}
    if unknown:
        raise TypeError(f'ik: unknown argument(s) {sorted(unknown)}')
    nq = problem.nq
    par = {**IK_DEFAULTS, 'q_lo': problem.x_min[:nq], 'q_hi': problem.x_max[:nq], 'row_lb': problem.row_lb, 'row_ub': problem.row_ub}
    par.update(over)
    for k, n in (('q_lo', nq), ('q_hi', nq), ('row_lb', len(problem.rows)), ('row_ub', len(problem.rows))):
        par[k] = np.ascontiguousarray(par[k], np.float64).reshape(-1)
        if par[k].shape != (n,):
            raise ValueError(f'ik: {k} has shape {par[k].shape}, expected ({n},)')
    par['max_iter'] = int(par['max_iter'])
    return par


# ---- value + nq tangents, vectorised over the leading axis (the DQ<NQ> of csrc/device_model.hpp) -----------------------------
class _Dual:
    __slots__ = ('v', 'd')

    def __init__(self, v, d):
        self.v, self.d = v, d

    def __add__(self, o):
        return _Dual(self.v + o.v, self.d + o.d)

    def __sub__(self, o):
        return _Dual(self.v - o.v, self.d - o.d)

    def __mul__(self, o):
        return _Dual(self.v * o.v, self.d * o.v[:, None] + self.v[:, None] * o.d)

    def __truediv__(self, o):
        v = self.v / o.v
        return _Dual(v, (self.d - v[:, None] * o.d) / o.v[:, None])


def _const(a, like):
    return _Dual(np.broadcast_to(np.asarray(a, float), like.v.shape).copy(), np.zeros_like(like.d))


def _pick(cond, a, b):
    return _Dual(np.where(cond, a.v, b.v), np.where(cond[:, None], a.d, b.d))


def _clamp01(t):
    """min(., 1) then max(., 0) with CasADi's tie rule, as clamp01 of device_model.hpp"""
    m = _pick(t.v <= 1.0, t, _const(1.0, t))
    return _pick(m.v >= 0.0, m, _const(0.0, t))


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _vsub(a, b):
    return [a[0] - b[0], a[1] - b[1], a[2] - b[2]]


def _segment_dist2(A, B, Cc, Dd):
    """utils.py:94-113 as segment_dist2 of device_model.hpp writes it"""
    ab, cd, ac = _vsub(B, A), _vsub(Dd, Cc), _vsub(Cc, A)
    R, S1, D1, S2, D2 = _dot(ab, cd), _dot(ab, ac), _dot(ab, ab), _dot(cd, ac), _dot(cd, cd)
    t = (S1 * D2 - S2 * R) / (D1 * D2 - (R * R + _const(1e-5, R)))
    t = _clamp01(t)
    u = _clamp01((t * R - S2) / D2)
    t = _clamp01((u * R + S1) / D1)
    w = [ab[i] * t - cd[i] * u - ac[i] for i in range(3)]
    return _dot(w, w)


def _ball_segment_dist2(A, B, len2, P):
    """utils.py:115-118: max(., 0) then min(., 1)"""
    t = _dot(_vsub(P, A), _vsub(B, A)) / _const(len2, P[0])
    m = _pick(t.v >= 0.0, t, _const(0.0, t))
    t = _pick(m.v <= 1.0, m, _const(1.0, t))
    w = [P[i] - (A[i] + (B[i] - A[i]) * t) for i in range(3)]
    return _dot(w, w)


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def _fk(chain, q):
    """World rotation, origin and axis of every actuated link frame for q [M, nq] (fk_world of device_model.hpp)"""
    M = q.shape[0]
    R = np.broadcast_to(np.eye(3), (M, 3, 3)).copy()
    p = np.zeros((M, 3))
    Rw, pw, zw = [], [], []
    for i, j in enumerate(chain.joints):
        p = p + np.einsum('mij,j->mi', R, j.p0)
        a = j.axis
        K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
        s, c = np.sin(q[:, i])[:, None, None], np.cos(q[:, i])[:, None, None]
        Q = c * np.eye(3) + (1.0 - c) * np.outer(a, a) + s * K
        R = np.einsum('mij,mjk->mik', R @ j.R0, Q)
        Rw.append(R)
        pw.append(p)
        zw.append(np.einsum('mij,j->mi', R, a))
    return Rw, pw, zw


def _point(problem, idx, fk, M, nq):
    """A robot point's world position with its Jacobian columns z_j x (P - p_j), j <= link, as three _Dual"""
    link, local = problem._points[idx]
    Rw, pw, zw = fk
    d = np.zeros((M, 3, nq))
    if link < 0:
        w = np.broadcast_to(np.asarray(local, float), (M, 3)).copy()
    else:
        w = pw[link] + np.einsum('mij,j->mi', Rw[link], np.asarray(local, float))
        for j in range(link + 1):
            d[:, :, j] = _cross(zw[j], w - pw[j])
    return [_Dual(w[:, c], d[:, c, :]) for c in range(3)]


def ik_eval(problem, q, target, par, geom=None):
    """The stacked residual's pieces at q [M, nq] for targets [M, 3] (``geom`` [M, n_rows, 8]: each point's own scene): a dict of
    F = |r|^2, g = J^T r [M, nq], A = J^T J [M, nq, nq], ee [M, 3] and its Jacobian ee_jac [M, 3, nq], ee_inf = |ee - target|_inf,
    rows [M, n_rows] and their gradients row_jac [M, n_rows, nq], margin = worst max(lb - v, v - ub) over the present bounds (-inf
    without one) and gap = least distance of a row value to a pushed bound."""
    q = np.asarray(q, float)
    M, nq = q.shape
    fk = _fk(problem.chain, q)
    pt = lambda i: _point(problem, i, fk, M, nq)
    ee = pt(int(problem.desc.ee_point))
    like = ee[0]
    e = np.stack([ee[c].v - target[:, c] for c in range(3)], axis=1)
    Je = np.stack([ee[c].d for c in range(3)], axis=1)                     # [M, 3, nq]
    F = (e * e).sum(1)
    g = np.einsum('mci,mc->mi', Je, e)
    A = np.einsum('mci,mcj->mij', Je, Je)
    rows = np.zeros((M, len(problem.rows)))
    row_jac = np.zeros((M, len(problem.rows), nq))
    margin = np.full(M, -np.inf)
    gap = np.full(M, np.inf)
    push = float(par['push'])
    for r, row in enumerate(problem.rows):
        if geom is None:
            Cc, Dd, off = np.array(row.C[:]), np.array(row.D[:]), float(row.offset)
            cC = [_const(Cc[c], like) for c in range(3)]
            cD = [_const(Dd[c], like) for c in range(3)]
            off = np.full(M, off)
        else:
            cC = [_Dual(geom[:, r, c].copy(), np.zeros_like(like.d)) for c in range(3)]
            cD = [_Dual(geom[:, r, 3 + c].copy(), np.zeros_like(like.d)) for c in range(3)]
            off = geom[:, r, 6]
        if row.kind == ROW_SEG_FIXEDSEG:
            v = _segment_dist2(pt(row.pa), pt(row.pb), cC, cD)
        elif row.kind == ROW_SEG_SEG:
            v = _segment_dist2(pt(row.pa), pt(row.pb), pt(row.pc), pt(row.pd))
        elif row.kind == ROW_SEG_POINT:
            v = _ball_segment_dist2(pt(row.pa), pt(row.pb), float(row.len2), cC)
        elif row.kind == ROW_POINT_POINT:
            w = _vsub(pt(row.pa), cC)
            v = _dot(w, w)
        elif row.kind == ROW_COORD:
            P = pt(row.pa)[int(row.axis)]
            v = _Dual(P.v - off, P.d)
        else:
            raise ValueError(f'row kind {row.kind}')
        rows[:, r], row_jac[:, r] = v.v, v.d
        for bound, sign in ((float(par['row_lb'][r]), -1.0), (float(par['row_ub'][r]), 1.0)):
            if not abs(bound) < INF:
                continue
            # sign = -1: lower bound (violated below it), +1: upper bound
            m = sign * (v.v - bound)
            margin = np.where((m > margin) | np.isnan(m), m, margin)      # (a max that keeps a NaN: it has to fail)
            bp = bound - sign * push * abs(bound)
            w = 1.0 / max(np.sqrt(abs(bound)), 1e-3)
            res = w * sign * (v.v - bp)
            on = res > 0.0
            gap = np.minimum(gap, np.abs(v.v - bp))
            res = np.where(on, res, 0.0)
            jr = np.where(on[:, None], (w * sign) * v.d, 0.0)
            F = F + res * res
            g = g + jr * res[:, None]
            A = A + jr[:, :, None] * jr[:, None, :]
    return {'F': F, 'g': g, 'A': A, 'ee': np.stack([ee[c].v for c in range(3)], axis=1), 'ee_inf': np.abs(e).max(1), 'rows': rows,
            'margin': margin, 'gap': gap, 'ee_jac': Je, 'row_jac': row_jac}


def _chol_solve(A, g, lam):
    """dq = -(A + lam I)^-1 g through a Cholesky factor, pivots floored at 1e-30 like the kernel's"""
    M, n = g.shape
    Mx = A + lam[:, None, None] * np.eye(n)
    L = np.zeros_like(Mx)
    for j in range(n):
        d = Mx[:, j, j] - (L[:, j, :j] ** 2).sum(1)
        d = np.where(d > 1e-30, d, 1e-30)
        L[:, j, j] = np.sqrt(d)
        for i in range(j + 1, n):
            L[:, i, j] = (Mx[:, i, j] - (L[:, i, :j] * L[:, j, :j]).sum(1)) / L[:, j, j]
    y = np.zeros_like(g)
    for i in range(n):
        y[:, i] = (-g[:, i] - (L[:, i, :i] * y[:, :i]).sum(1)) / L[:, i, i]
    x = np.zeros_like(g)
    for i in range(n - 1, -1, -1):
        x[:, i] = (y[:, i] - (L[:, i + 1:, i] * x[:, i + 1:]).sum(1)) / L[:, i, i]
    return x


def ik_batch_host(problem, target, q_start, mask=None, q_out=None, info=None, resid=None, scenes=None, trace=None, **over):
    """``smpc_ik_batch`` in numpy.  target [B, 3], q_start [B, S, nq], 1 <= S <= 64; ``mask`` [B]: instances with 0 keep their rows
    of the outputs; ``scenes`` [B, n_rows, 8]: rows formed in the instance's scene.  Returns ``(q_out [B, nq], info [B, 2] int32 =
    (winning start, number of successful starts), resid [B, 2] = (|ee - target|_inf, worst row margin))``.  ``trace`` (a dict)
    receives every start's outcome -- 'q' [B, S, nq], 'F', 'success' [B, S] -- and how closely its branches were decided:
    'accept_gap' = least |F(q') - F(q)| / max(F(q'), F(q)) over the iterations, 'row_gap' = least distance of a row value to a
    pushed bound over every evaluation."""
    par = ik_params(problem, **over)
    target = np.asarray(target, float)
    q_start = np.asarray(q_start, float)
    B, S, nq = q_start.shape
    if not 1 <= S <= MAX_STARTS:
        raise ValueError(f'ik: S={S} outside 1..{MAX_STARTS}')
    if par['max_iter'] < 1:
        raise ValueError('ik: max_iter must be >= 1')
    if target.shape != (B, 3) or nq != problem.nq:
        raise ValueError('ik: target [B, 3] and q_start [B, S, nq] expected')
    lo, hi = par['q_lo'], par['q_hi']
    M = B * S
    tg = np.repeat(target, S, axis=0)
    geom = None if scenes is None else np.repeat(np.asarray(scenes, float), S, axis=0)
    q = q_start.reshape(M, nq)
    q = np.where(np.isfinite(q), np.clip(q, lo, hi), 0.5 * (lo + hi))
    lam = np.full(M, float(par['damping']))
    acc_gap, row_gap = np.full(M, np.inf), np.full(M, np.inf)
    cur = ik_eval(problem, q, tg, par, geom)
    row_gap = np.minimum(row_gap, cur['gap'])
    for _ in range(par['max_iter']):
        with np.errstate(all='ignore'):
            dq = _chol_solve(cur['A'], cur['g'], lam)
            qn = np.clip(q + dq, lo, hi)
            new = ik_eval(problem, np.where(np.isfinite(qn), qn, q), tg, par, geom)
        Fn = np.where(np.isfinite(qn).all(1), new['F'], np.nan)
        acc = Fn < cur['F']
        with np.errstate(all='ignore'):
            acc_gap = np.fmin(acc_gap, np.abs(Fn - cur['F']) / np.maximum(np.maximum(Fn, cur['F']), 1e-300))
        row_gap = np.minimum(row_gap, new['gap'])
        q = np.where(acc[:, None], qn, q)
        for k in ('F', 'g', 'A', 'ee_inf', 'margin'):
            a = acc.reshape((M,) + (1,) * (cur[k].ndim - 1))
            cur[k] = np.where(a, new[k], cur[k])
        lam = np.where(acc, np.maximum(lam * par['damping_accept'], par['damping_min']),
                       np.minimum(lam * par['damping_reject'], par['damping_max']))
    succ = (cur['ee_inf'] <= par['tol_ee']) & (cur['margin'] <= 0.0)
    qs, Fs, succ = q.reshape(B, S, nq), cur['F'].reshape(B, S), succ.reshape(B, S)
    n_ok = succ.sum(1)
    win = np.where(n_ok > 0, np.argmax(succ, axis=1), np.argmin(np.where(np.isnan(Fs), np.inf, Fs), axis=1))
    rows = np.arange(B)
    o_q = qs[rows, win]
    o_info = np.stack([win, n_ok], axis=1).astype(np.int32)
    o_res = np.stack([cur['ee_inf'].reshape(B, S)[rows, win], cur['margin'].reshape(B, S)[rows, win]], axis=1)
    if trace is not None:
        trace.update(q=qs, F=Fs, success=succ, accept_gap=acc_gap.reshape(B, S), row_gap=row_gap.reshape(B, S))
    keep = np.ones(B, bool) if mask is None else np.asarray(mask).astype(bool)
    q_out = np.zeros((B, nq)) if q_out is None else q_out
    info = np.zeros((B, 2), np.int32) if info is None else info
    resid = np.zeros((B, 2)) if resid is None else resid
    q_out[keep], info[keep], resid[keep] = o_q[keep], o_info[keep], o_res[keep]
    return q_out, info, resid


def ik(solver, problem, target, q_start, mask=None, scenes=None, **over):
    """The batched IK through ``solver.ik`` (the device kernel) where the solver has one, through :func:`ik_batch_host` otherwise.
    With ``scenes`` the solver's instance scene is set for the call and cleared behind it."""
    if hasattr(solver, 'ik'):
        if scenes is None:
            return solver.ik(target, q_start, mask=mask, **over)
        solver.set_instance_scene(scenes)
        try:
            return solver.ik(target, q_start, mask=mask, **over)
        finally:
            solver.set_instance_scene(None)
    return ik_batch_host(problem, target, q_start, mask=mask, scenes=scenes, **over)
