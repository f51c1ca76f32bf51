"""Every way out of the interior point's loop, and the isolation of instances that share a wavefront or a workgroup, on the
engine against the CPU oracle (inputs: tests/qp_exit_cases.py; the oracle's side of each fact: test_qp_exits_oracle.py).  -m gpu only.
Every test runs in both forms of the solve (k_qp_ipm, k_qp_ipm_wg), forced.

The kernels apply a step lazily (the next factorisation sweep, or the epilogue if none follows); the oracle applies it at once.  The
exits and what is asserted on each:

  converged / cap not reached ...... test_a_cap_out_of_reach_means_converged
  iteration cap (1, 2, 3) .......... test_cap_parity: status, qp_iter EQUAL, controls and states within 1e-9 (1 + |u|inf) where the
                                     path is FP64 end to end ('naive', 'zerovel'; the oracle itself moves by 1.7e-10 under a 1e-11
                                     perturbation) and 1e-4 (1 + |u|inf) with a network row.  Cap 1 returns only a pending step.
  breakdown at iteration 0 ......... test_stall_and_breakdown_parity, test_breakdown_of_every_instance: iterate equal to 1e-9
  failure at iteration 6 / 2 ....... test_stall_and_breakdown_parity ('late'): qp_iter equal, iterate to 1e-6
  stall exit ....................... test_stall_and_breakdown_parity: qp_iter equal (24), iterate to 1e-4 (oracle moves by 1.4e-6)
  min-step exit .................... test_min_step_exit: status, 0 < qp_iter < 200, finite.  Nothing more: under a 1e-11 perturbation
                                     the ORACLE's own iteration count on these instances moves by up to 17 and its iterate by O(1)
                                     (a crawl of 30-70 blocked steps on an infeasible QP), so no parity exists to assert.
  non-finite complementarity ....... test_non_finite_inputs (last in the file): the step is dropped, the output is the guess

Isolation (test_instances_do_not_touch_each_other) is the engine against itself, to the bit, every instance included.

GAPS SEEN ON THE MI355X (printed by the tests, run with -s), next to what they are held to:
  cap parity, u relative to 1 + |u|inf .... naive 2e-15 / 2e-15 / 3e-14 at caps 1 / 2 / 3, zerovel 7e-14 / 6e-13 / 9e-12 (1e-9);
                                           st 2e-10, constraint_everywhere 2e-10, fr7 1.2e-9, nq5 9e-11 at cap 1, less at 2, 3 (1e-4)
  breakdown at iteration 0 ............... 0 (1e-9)
  late failures (iterations 6, 2) ........ 8e-7, 3e-7 from the oracle (1e-6); 5e-18 from the engine's own capped run (1e-12)
  stall exit ............................. qp_iter 24 = 24, iterate 2e-6 (1e-4)
  clean / slow instances ................. 2e-7 (1e-4) / qp_iter equal (within 2), iterate 4e-3 (not asserted: the oracle moves by 3e-3)
  min-step exit .......................... qp_iter 31-78 against the oracle's 32-76, iterates O(1) apart (nothing asserted, see above)
"""
import numpy as np
import pytest

import qp_exit_cases as Q

pytestmark = pytest.mark.gpu

_QP_MODE = [None]


def _solver(prob, net):
    from safe_mpc_amd.solver import BatchedOcpSolver
    s = BatchedOcpSolver(prob, net)
    if _QP_MODE[0] is not None:
        s.set_qp_mode(_QP_MODE[0])
    return s


@pytest.fixture(params=['throughput', 'latency'])
def qp_mode(request):
    """both forms of the interior-point solve, forced (the pattern of test_gpu_parity.py)"""
    _QP_MODE[0] = request.param
    yield request.param
    _QP_MODE[0] = None


def _dx(a, b):
    """largest absolute difference per instance"""
    return np.abs(a - b).reshape(len(a), -1).max(1)


# ---- a. the iteration cap ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cap', [1, 2, 3])
@pytest.mark.parametrize('case', Q.CAP_CASES)
def test_cap_parity(case, cap, qp_mode):
    par, prob, net, x0, xg, ug, p, _, classes = Q.capped(case, cap)
    assert np.all(classes == 'capped')
    s, o = _solver(prob, net), Q._oracle(prob, net)
    xa, ua, sa, ia = s.solve(x0, xg, ug, p)
    xb, ub, sb, ib = o.solve_batch(x0, xg, ug, p)
    tol = 1e-9 if case in Q.FP64_CASES else 1e-4
    gu, gx = Q.rel_u(ua, ub), _dx(xa, xb) / (1.0 + np.abs(ub).reshape(len(ub), -1).max(1))
    print(f'cap parity {case} cap {cap} {qp_mode}: u {gu.max():.2e} x {gx.max():.2e} (tolerance {tol:.0e}), qp_iter {np.unique(ia).tolist()}')
    assert np.array_equal(sa, sb) and np.all(sa == 0)
    assert np.array_equal(ia, ib) and np.all(ia == cap)
    assert np.all(gu < tol) and np.all(gx < tol)               # every instance
    assert np.array_equal(xa[:, 0], x0)


# ---- b. a cap that is not reached; the cap belongs to the handle ---------------------------------------------------------------------
def test_a_cap_out_of_reach_means_converged(qp_mode):
    par, prob, net = Q.cap_problem('st', 200)
    _, prob3, _ = Q.cap_problem('st', 3)
    _, prob_d, _ = Q.cap_problem('st')
    x0 = Q.sample_instances(prob, Q.B_CAP, seed=2, vel_scale=0.1)
    xg, ug, p = Q.constant_guess(prob, x0)
    s3 = _solver(prob3, net)                                     # the capped handle first: a cap read once per process would stick
    x3, u3, st3, it3 = s3.solve(x0, xg, ug, p)
    s, sd = _solver(prob, net), _solver(prob_d, net)
    xa, ua, sa, ia = s.solve(x0, xg, ug, p)
    xd, ud, sd_, id_ = sd.solve(x0, xg, ug, p)
    xb, ub, sb, ib = Q._oracle(prob_d, net).solve_batch(x0, xg, ug, p)
    assert np.all(it3 == 3) and np.all(st3 == 0)
    assert np.all(sa == 0) and np.all((ia >= 4) & (ia <= Q.CLEAN_MAX_ITER)) and np.array_equal(ia, ib)
    assert np.array_equal(xa, xd) and np.array_equal(ua, ud) and np.array_equal(ia, id_)
    assert np.all(Q.rel_u(ua, ub) < 1e-4)
    # three iterations are not the converged answer for any instance (how far off is the instance's business: 4e-7 to 2e-2 here),
    # and they are the oracle's three iterations
    x3o, u3o, _, _ = Q._oracle(prob3, net).solve_batch(x0, xg, ug, p)
    assert all(not np.array_equal(u3[b], ua[b]) and not np.array_equal(u3o[b], ub[b]) for b in range(len(x0)))
    assert np.all(Q.rel_u(u3, u3o) < 1e-4) and Q.rel_u(u3, ua).max() > 100 * Q.rel_u(u3, u3o).max()
    x3b, u3b, _, it3b = s3.solve(x0, xg, ug, p)                 # ... and the capped handle still is capped
    assert np.array_equal(u3b, u3) and np.array_equal(x3b, x3) and np.all(it3b == 3)


# ---- c. stall exit and breakdown ---------------------------------------------------------------------------------------------------------
def _mixed_engine(stall, **over):
    par, prob, net, x0, xg, ug, p, bounds, classes = Q.mixed_batch(stall, **over)
    s, o = _solver(prob, net), Q._oracle(prob, net)
    s.set_instance_bounds(*bounds)
    o.set_instance_bounds(*bounds)
    return prob, net, s, o, x0, xg, ug, p, bounds, classes


def _check_mixed_common(classes, eng, orc, x0, qp_mode, tag):
    xa, ua, sa, ia = eng
    xb, ub, sb, ib = orc
    ia, ib = ia.astype(int), ib.astype(int)
    gu, gx = Q.rel_u(ua, ub), _dx(xa, xb)
    for c in np.unique(classes):
        m = classes == c
        print(f'{tag} {qp_mode} {c}: n {int(m.sum())} qp_iter engine {ia[m].tolist()} oracle {ib[m].tolist()} iterate gap u {gu[m].max():.2e} x {gx[m].max():.2e}')
    assert np.array_equal(sa, sb), (sa, sb)
    assert np.array_equal(xa[:, 0], x0)
    for c in ('clean', 'breakdown0'):
        assert np.array_equal(ia[classes == c], ib[classes == c]), c
    assert np.abs(ia - ib)[classes == 'slow'].max() <= 2
    assert np.all(gu[classes == 'clean'] < 1e-4)
    # breakdown at iteration 0: nothing was solved, the iterate is the guess plus the initial point -- and nothing is pending
    bd = classes == 'breakdown0'
    assert np.all(gu[bd] < 1e-9) and np.all(gx[bd] < 1e-9)
    return ia, ib, gu, gx


def _check_late(stall, net, eng, orc, x0, xg, ug, p, bounds, classes, qp_mode):
    """The solve fails in iteration k >= 1, in the sweep that has just applied step k - 1: the epilogue must not apply that step
    again, nor lose it.  Against the oracle: status, qp_iter equal, controls and states within 1e-6 (1 + |u|inf) (these instances carry
    the fp32 network row and a cost gradient of 3e4: measured 8e-7 in u, 2e-6 absolute in x, |u|inf = 60).  And, much sharper, against
    the engine itself: the oracle's failing run returns the bits of its run with qp_max_iter = k (test_qp_exits_oracle.py), so the
    engine's must return its own qp_max_iter = k iterate -- there the epilogue applies step k - 1, here the sweep did -- to a few
    roundings of one update: 1e-12 (1 + |u|inf), nine orders below the step itself."""
    xa, ua, sa, ia = eng
    xb, ub, sb, ib = orc
    late = np.where(classes == 'late')[0]
    assert len(late) == len(Q.LATE)
    for b, (_, _, _, k) in zip(late, Q.LATE):
        scale = 1.0 + np.abs(ub[b]).max()
        gu, gx = np.abs(ua[b] - ub[b]).max() / scale, np.abs(xa[b] - xb[b]).max() / scale
        _, prob_c, _ = Q.mixed_problem(stall)
        prob_c.desc.qp_max_iter = k
        sc = _solver(prob_c, net)
        sc.set_instance_bounds(np.ascontiguousarray(bounds[0][b:b + 1]), np.ascontiguousarray(bounds[1][b:b + 1]))
        xc, uc, stc, itc = sc.solve(x0[b:b + 1], xg[b:b + 1], ug[b:b + 1], p[b:b + 1])
        su, sx = np.abs(ua[b] - uc[0]).max() / scale, np.abs(xa[b] - xc[0]).max() / scale
        print(f'late instance {b} {qp_mode}: status {sa[b]} qp_iter {ia[b]} (oracle {ib[b]}), against the oracle u {gu:.2e} x {gx:.2e}, '
              f'against the engine capped at {k} u {su:.2e} x {sx:.2e}, |u|inf {scale - 1:.1f}')
        assert sa[b] == 4 and sb[b] == 4 and ia[b] == ib[b] == k
        assert stc[0] == 0 and itc[0] == k
        assert gu < 1e-6 and gx < 1e-6
        assert su < 1e-12 and sx < 1e-12


def test_stall_and_breakdown_parity(qp_mode):
    prob, net, s, o, x0, xg, ug, p, bounds, classes = _mixed_engine(24)
    eng, orc = s.solve(x0, xg, ug, p), o.solve_batch(x0, xg, ug, p)
    ia, ib, gu, gx = _check_mixed_common(classes, eng, orc, x0, qp_mode, 'mixed batch, stall 24')
    st = classes == 'stall'
    assert st.sum() >= 6 and np.array_equal(ia[st], ib[st]) and np.all(ia[st] == 24)
    assert np.all(gu[st] < 1e-4) and np.all(gx[st] < 1e-4)
    _check_late(24, net, eng, orc, x0, xg, ug, p, bounds, classes, qp_mode)
    assert np.isfinite(eng[0]).all() and np.isfinite(eng[1]).all()


def test_breakdown_of_every_instance(qp_mode):
    """lm_stage = -1: the stage Hessian is indefinite for every instance, every first factorisation fails"""
    par, prob, net = Q.mixed_problem(24)
    prob.desc.lm_stage = -1.0
    x0, xg, ug, p, bounds = Q.mixed_inputs(prob)
    s, o = _solver(prob, net), Q._oracle(prob, net)
    xa, ua, sa, ia = s.solve(x0, xg, ug, p)
    xb, ub, sb, ib = o.solve_batch(x0, xg, ug, p)
    assert np.all(sb == 4) and np.all(ib == 0)
    assert np.array_equal(sa, sb) and np.array_equal(ia, ib)
    print(f'breakdown of every instance {qp_mode}: iterate gap u {Q.rel_u(ua, ub).max():.2e} x {_dx(xa, xb).max():.2e}')
    assert np.all(Q.rel_u(ua, ub) < 1e-9) and np.all(_dx(xa, xb) < 1e-9)


# ---- d. min-step exit --------------------------------------------------------------------------------------------------------------------
def test_min_step_exit(qp_mode):
    """qp_stall_iters = 0: the unreachable tubes crawl until the step length falls below the minimum.  Status, 0 < qp_iter < 200,
    finite outputs and x_out[0] = x0 only -- the module docstring says why no parity is asserted on this class; the other classes
    of the batch are held to what test_stall_and_breakdown_parity holds them to."""
    prob, net, s, o, x0, xg, ug, p, bounds, classes = _mixed_engine(0)
    eng, orc = s.solve(x0, xg, ug, p), o.solve_batch(x0, xg, ug, p)
    ia, ib, gu, gx = _check_mixed_common(classes, eng, orc, x0, qp_mode, 'mixed batch, stall 0')
    ms = classes == 'minstep'
    assert ms.sum() >= 6
    assert np.all(eng[2][ms] == 4) and np.all((ia[ms] > 0) & (ia[ms] < 200))
    assert np.isfinite(eng[0]).all() and np.isfinite(eng[1]).all()
    _check_late(0, net, eng, orc, x0, xg, ug, p, bounds, classes, qp_mode)


# ---- e. isolation ------------------------------------------------------------------------------------------------------------------------
def _same(got, ref, idx, what):
    """every output row of ``got`` equals row idx[i] of ``ref``, bit for bit"""
    for a, b, name in zip(got, ref, ('x', 'u', 'status', 'qp_iter')):
        a, b = np.asarray(a), np.asarray(b)[idx]
        bad = [int(i) for i in range(len(a)) if not np.array_equal(a[i], b[i], equal_nan=True)]
        assert not bad, f'{what}: {name} differs for instances {[int(idx[i]) for i in bad]}'


def _solve_subset(prob, net, x0, xg, ug, p, bounds, idx, s=None):
    s = s or _solver(prob, net)
    s.set_instance_bounds(np.ascontiguousarray(bounds[0][idx]), np.ascontiguousarray(bounds[1][idx]))
    return s, s.solve(x0[idx], xg[idx], ug[idx], p[idx])


@pytest.mark.parametrize('stall', [24, 0])
def test_instances_do_not_touch_each_other(stall, qp_mode):
    """The mixed batch (iteration counts 4-6, 24 or 30-100, 0, 11-27 and 6 / 2 side by side), form fixed, against its own first solve
    on a fresh handle, where k_qp_ipm pairs instances 2 i and 2 i + 1 on a wavefront.  x, u, status and qp_iter of EVERY instance
    are the same bits (i) in a second call on the same handle, paired through order[] sorted by the first call's counts; (ii) in a
    random permutation of the batch; (iii) in a batch without its last instance (a lone half-wave), in the first 31, and alone
    (B = 1, two instances of each class); (iv) with a different twin: every clean instance next to a breakdown-at-0 instance, then
    next to an unreachable-tube instance (stall or min-step exit)."""
    par, prob, net, x0, xg, ug, p, bounds, classes = Q.mixed_batch(stall)
    B = len(x0)
    all_ = np.arange(B)
    s, ref = _solve_subset(prob, net, x0, xg, ug, p, bounds, all_)
    ref = tuple(np.array(a) for a in ref)
    print(f'isolation stall {stall} {qp_mode}: qp_iter {ref[3].tolist()}')
    assert len(np.unique(ref[3])) >= 5
    # (i)
    for rep in range(2):
        _same(s.solve(x0, xg, ug, p), ref, all_, f'call {rep + 2} on one handle')
    # (ii)
    perm = np.random.default_rng(17).permutation(B)
    assert not np.array_equal(perm, all_)
    sp, got = _solve_subset(prob, net, x0, xg, ug, p, bounds, perm)
    _same(got, ref, perm, 'permuted batch')
    _same(sp.solve(x0[perm], xg[perm], ug[perm], p[perm]), ref, perm, 'permuted batch, second call')
    # (iii)
    for n in (B - 1, 31):
        _, got = _solve_subset(prob, net, x0, xg, ug, p, bounds, all_[:n])
        _same(got, ref, all_[:n], f'first {n} instances')
    s1 = None
    for c in np.unique(classes):
        for b in np.where(classes == c)[0][:2]:
            s1, got = _solve_subset(prob, net, x0, xg, ug, p, bounds, all_[b:b + 1], s1)
            _same(got, ref, all_[b:b + 1], f'instance {b} ({c}) alone')
    # (iv)
    clean = np.where(classes == 'clean')[0]
    tube = np.where(np.isin(classes, ['stall', 'minstep']))[0]
    for twins, name in ((np.where(classes == 'breakdown0')[0], 'breakdown-at-0'), (tube, 'unreachable-tube')):
        assert len(twins) >= len(clean)
        front = np.stack([clean, twins[:len(clean)]], axis=1).reshape(-1)          # c0 t0 c1 t1 ...
        order = np.concatenate([front, np.setdiff1d(all_, front)])
        assert sorted(order.tolist()) == all_.tolist()
        _, got = _solve_subset(prob, net, x0, xg, ug, p, bounds, order)           # a fresh handle: paired by position
        _same(got, ref, order, f'clean instances next to {name} twins')


# ---- f. non-finite inputs: LAST in the file, one such solve per form -----------------------------------------------------------------
def test_non_finite_inputs(qp_mode):
    """One NaN / Inf / 1e308 entry in x0, the guess or the parameters of every other instance.  Per instance: the oracle's status (4),
    qp_iter 0 where the oracle says 0, the same entries of the output finite, equal outputs where finite; the eight clean instances
    in between carry the bits of the same handle's run on the batch without the corrupted entries (solved first)."""
    par, prob, net, x0, xg, ug, p, _, classes = Q.nonfinite_batch()
    o = Q._oracle(prob, net)
    xb, ub, sb, ib = o.solve_batch(x0, xg, ug, p)
    assert not np.any(sb == 1)
    s = _solver(prob, net)
    odd = np.arange(len(x0)) % 2 == 1
    x0c, xgc, ugc, pc = (np.array(a) for a in (x0, xg, ug, p))
    for a in (x0c, xgc, ugc, pc):
        a[odd] = a[np.where(odd)[0] - 1]                          # a clean batch: every odd instance a copy of its left neighbour
    ref = tuple(np.array(a) for a in s.solve(x0c, xgc, ugc, pc))
    assert np.all(ref[2] == 0)
    xa, ua, sa, ia = s.solve(x0, xg, ug, p)                       # the one solve with non-finite inputs
    for b in np.where(odd)[0]:
        fx, fu = np.isfinite(xa[b]), np.isfinite(ua[b])
        print(f'non-finite {qp_mode} {Q.NONFINITE[b // 2][0]}: status {sa[b]} / {sb[b]} qp_iter {ia[b]} / {ib[b]} non-finite outputs {int((~fx).sum() + (~fu).sum())} / '
              f'{int((~np.isfinite(xb[b])).sum() + (~np.isfinite(ub[b])).sum())}')
    assert np.array_equal(sa, sb)
    assert np.array_equal(ia[ib == 0], ib[ib == 0])
    for b in range(len(x0)):
        fx, fu = np.isfinite(xb[b]), np.isfinite(ub[b])
        assert np.array_equal(np.isfinite(xa[b]), fx) and np.array_equal(np.isfinite(ua[b]), fu), (b, Q.NONFINITE[b // 2][0])
        if not odd[b]:
            assert Q.rel_u(ua[b:b + 1], ub[b:b + 1])[0] < 1e-4 and _dx(xa[b:b + 1], xb[b:b + 1])[0] < 1e-4, b
            continue
        with np.errstate(over='ignore'):                        # entry by entry (one guess holds 1e308); nothing was solved
            assert np.all(np.abs(xa[b][fx] - xb[b][fx]) <= 1e-9 * (1.0 + np.abs(xb[b][fx]))), b
            assert np.all(np.abs(ua[b][fu] - ub[b][fu]) <= 1e-9 * (1.0 + np.abs(ub[b][fu]))), b
    for a, r in zip((xa, ua, sa, ia), ref):
        assert np.array_equal(a[~odd], r[~odd])
