"""What the CPU oracle does on the exits of the interior point other than "converged" (tests/qp_exit_cases.py builds the inputs).
test_qp_exits_gpu.py compares the engine with the oracle on these inputs; the facts it relies on are pinned here, so that a change
of the oracle fails on the CPU and says what moved.

Measured with oracle/ as committed (1e-11 relative perturbation of x0 and of the guess built from it):
  capped iterate, qp_max_iter in {1, 2, 3} ... controls move by at most 4.6e-10 (1 + |u|inf) ('fr7' at cap 1; 'naive' 1.7e-10, 'zerovel'
                                               3e-11), states by at most 1.3e-10; held below 1e-9
  stall exit (qp_stall_iters = 24) ........... status 4 at exactly 24 iterations, iterate moves by 1.4e-6 (held below 1e-5)
  min-step exit (qp_stall_iters = 0) ......... status 4 after 32-76 iterations; the count moves by up to 17 and the iterate by O(1)
  breakdown at iteration 0 ................... status stable, iterate moves by the perturbation itself
  the two 'late' instances ................... status 4 at iterations 6 and 2 under 1e-11 and 1e-9, iterate moves by 1.5e-10
"""
import numpy as np
import pytest

import qp_exit_cases as Q

CAPS = (1, 2, 3)


@pytest.mark.parametrize('case', Q.CAP_CASES)
def test_cap_ends_the_loop_and_the_capped_iterate_is_well_conditioned(case):
    """per cap: every instance status 0 with qp_iter == cap; the iterate moves by less than 1e-9 (1 + |u|inf) under a 1e-11 relative
    perturbation; caps k and k + 1 return different iterates (the cap is what ended the loop)"""
    prev = None
    for cap in CAPS:
        par, prob, net, x0, xg, ug, p, _, classes = Q.capped(case, cap)
        assert np.all(classes == 'capped'), (case, cap, classes)
        du, dx = Q.oracle_cap_sensitivity(case, cap)
        print(case, cap, 'sensitivity u', du.max(), 'x', dx.max())
        assert du.max() < 1e-9 and dx.max() < 1e-9
        xo, uo, st, it = Q._oracle(prob, net).solve_batch(x0, xg, ug, p)
        assert np.all(st == 0) and np.all(it == cap)
        assert np.allclose(xo[:, 0], x0, atol=1e-12)
        if prev is not None:
            gap = Q.rel_u(uo, prev)
            assert gap.min() > 1e-6, (case, cap, gap.min())            # every instance, not only some
        prev = uo


@pytest.mark.parametrize('case', Q.CAP_CASES)
def test_a_cap_that_is_not_reached_changes_nothing(case):
    """qp_max_iter = 200, and a cap equal to the iteration count of the slowest instance, give the converged solve bit for bit"""
    par, prob, net = Q.cap_problem(case)
    assert prob.desc.qp_max_iter == 200
    x0 = Q.sample_instances(prob, Q.B_CAP, seed=2, vel_scale=0.1)
    xg, ug, p = Q.constant_guess(prob, x0)
    ref = Q._oracle(prob, net).solve_batch(x0, xg, ug, p)
    assert np.all(ref[2] == 0) and 4 <= ref[3].min() and ref[3].max() <= Q.CLEAN_MAX_ITER
    for cap in (200, int(ref[3].max())):
        _, prob_c, _ = Q.cap_problem(case, cap)
        got = Q._oracle(prob_c, net).solve_batch(x0, xg, ug, p)
        for a, b in zip(got, ref):
            assert np.array_equal(a, b), (case, cap)


@pytest.mark.parametrize('stall', [24, 0])
def test_mixed_batch_classes(stall):
    """b % 4 = 0 / 1 / 2 / 3 of the first 32: at least 6 of 8 are clean / stall (min-step with the option off) / breakdown at
    iteration 0 / slow; iteration counts as the GPU tests assume them"""
    par, prob, net, x0, xg, ug, p, bounds, classes = Q.mixed_batch(stall)
    o = Q._oracle(prob, net)
    o.set_instance_bounds(*bounds)
    xo, uo, st, it = o.solve_batch(x0, xg, ug, p)
    B = Q.B_MIXED
    slot = np.arange(len(x0)) % 4
    first = np.arange(len(x0)) < B
    want = {0: 'clean', 1: 'stall' if stall else 'minstep', 2: 'breakdown0', 3: 'slow'}
    for r, name in want.items():
        n = int((classes[first & (slot == r)] == name).sum())
        print(stall, name, n, it[first & (slot == r)].tolist())
        assert n >= 6, (name, classes[first & (slot == r)])
    assert not np.any(classes == 'other')
    assert np.all(st[classes == 'clean'] == 0) and np.all(st[classes == 'slow'] == 0) and np.all(st[np.isin(classes, ['stall', 'minstep', 'breakdown0', 'late'])] == 4)
    assert np.all((it[classes == 'clean'] >= 4) & (it[classes == 'clean'] <= 6))
    assert np.all(it[classes == 'breakdown0'] == 0)
    assert np.all((it[classes == 'slow'] > Q.CLEAN_MAX_ITER) & (it[classes == 'slow'] < 40))
    if stall:
        assert np.all(it[classes == 'stall'] == 24)
    else:
        mi = it[classes == 'minstep']
        assert np.all((mi > 24) & (mi < 200))
        assert np.isfinite(xo).all() and np.isfinite(uo).all()
    assert np.allclose(xo[:, 0], x0, atol=1e-12)
    # a solve that breaks down at iteration 0 returns the guess plus the initial point: here x0 == x_guess[0], so the guess itself
    bd = classes == 'breakdown0'
    assert np.array_equal(xo[bd], xg[bd]) and np.array_equal(uo[bd], ug[bd])


def test_mixed_batch_sensitivity_of_the_oracle():
    """statuses and iteration counts of every class but min-step are stable under the 1e-11 perturbation; the stall-class iterate
    moves by less than 1e-5, the clean one by less than 1e-5 (the fp32 network row); the min-step class is NOT stable, which is why
    the GPU test asserts no parity on it"""
    for stall in (24, 0):
        par, prob, net, x0, xg, ug, p, bounds, classes = Q.mixed_batch(stall)
        o = Q._oracle(prob, net)
        o.set_instance_bounds(*bounds)
        xa, ua, sa, ia = o.solve_batch(x0, xg, ug, p)
        x1, g1 = Q.perturbed(x0, xg)
        xb, ub, sb, ib = o.solve_batch(x1, g1, ug, p)
        assert np.array_equal(sa, sb)
        steady = classes != 'minstep'
        assert np.array_equal(ia[steady], ib[steady])
        du = Q.rel_u(ub, ua)
        dx = np.abs(xb - xa).reshape(len(xa), -1).max(1)
        for c in np.unique(classes):
            print(stall, c, 'u', du[classes == c].max(), 'x', dx[classes == c].max(), 'it', np.abs(ib - ia)[classes == c].max())
        for c in ('clean', 'stall'):
            if (classes == c).any():
                assert du[classes == c].max() < 1e-5 and dx[classes == c].max() < 1e-5
        for c in ('breakdown0', 'late'):
            assert du[classes == c].max() < 1e-9 and dx[classes == c].max() < 1e-9


def test_late_failures_apply_nothing_in_the_failing_iteration():
    """the instances LATE of the mixed batch fail (status 4) in iteration k = 6 / 2 >= 1 whatever the stall option; their iterate
    is, bit for bit, what qp_max_iter = k returns (the failing iteration applies no step: an engine that applies its pending step
    lazily must have applied step k - 1 exactly once) and differs from what qp_max_iter = k - 1 returns"""
    for stall in (24, 0):
        par, prob, net, x0, xg, ug, p, bounds, classes = Q.mixed_batch(stall)
        o = Q._oracle(prob, net)
        o.set_instance_bounds(*bounds)
        xo, uo, st, it = o.solve_batch(x0, xg, ug, p)
        for j, (_, _, _, k) in enumerate(Q.LATE):
            b = Q.B_MIXED + j
            assert classes[b] == 'late' and st[b] == 4 and it[b] == k
            for cap, same in ((k, True), (k - 1, False)):
                _, prob_c, _ = Q.mixed_problem(stall)
                prob_c.desc.qp_max_iter = cap
                oc = Q._oracle(prob_c, net)
                oc.set_instance_bounds(*bounds)
                xc, uc, sc, ic = oc.solve_batch(x0, xg, ug, p)
                assert sc[b] == 0 and ic[b] == cap
                assert (np.array_equal(xc[b], xo[b]) and np.array_equal(uc[b], uo[b])) == same
    x1, g1 = Q.perturbed(x0, xg, 1e-9)
    sb, ib = o.solve_batch(x1, g1, ug, p)[2:]
    late = classes == 'late'
    assert np.array_equal(sb[late], st[late]) and np.array_equal(ib[late], it[late])


def test_indefinite_stage_hessian_breaks_down_at_iteration_0():
    """lm_stage = -1: every factorisation fails at once -- status 4, no iteration, the guess comes back"""
    par, prob, net = Q.mixed_problem(24)
    prob.desc.lm_stage = -1.0
    x0, xg, ug, p, bounds = Q.mixed_inputs(prob)
    xo, uo, st, it = Q._oracle(prob, net).solve_batch(x0, xg, ug, p)
    assert np.all(st == 4) and np.all(it == 0)
    assert np.array_equal(xo, xg) and np.array_equal(uo, ug)


def test_non_finite_inputs():
    """one NaN, Inf or 1e308 in x0, the guess or the parameters of an instance: status 4 at iteration 0, never SMPC_STATUS_NAN
    (DESIGN.md section 5 says why); the output is not finite where the input was not and nowhere else -- x0 = +Inf passes the first
    factorisation and takes a step of no numbers, which is dropped when the complementarity after it is no number either; the
    clean instances in between give the bits of a batch without the corrupted entries"""
    par, prob, net, x0, xg, ug, p, _, classes = Q.nonfinite_batch()
    o = Q._oracle(prob, net)
    xo, uo, st, it = o.solve_batch(x0, xg, ug, p)
    odd = np.arange(Q.B_NONFINITE) % 2 == 1
    assert np.all(st[odd] == 4) and np.all(it[odd] == 0) and np.all(classes[odd] == 'breakdown0')
    assert np.all(st[~odd] == 0) and np.all(classes[~odd] == 'clean')
    clean = [np.where(np.isfinite(a) & (np.abs(a) < 1e300), a, 0.0) for a in (x0, xg, ug, p)]
    clean[3][13, 12, 3] = p[12, 12, 3]
    ref = o.solve_batch(*clean)
    for a, b in zip((xo, uo, st, it), ref):
        assert np.array_equal(a[~odd], b[~odd])
    fin = lambda b: np.isfinite(xo[b]).all() and np.isfinite(uo[b]).all()
    bad_x = {b: np.argwhere(~np.isfinite(xo[b])).tolist() for b in range(Q.B_NONFINITE)}
    bad_u = {b: np.argwhere(~np.isfinite(uo[b])).tolist() for b in range(Q.B_NONFINITE)}
    assert bad_x[1] == [[0, 3]] and not bad_u[1]
    assert bad_x[5] == [[5, 2]] and bad_x[7] == [[12, 7]] and bad_u[9] == [[4, 1]] and not bad_x[9]
    assert fin(11) and fin(13) and fin(15)
    assert bad_x[3] == [[0, 8]] and not bad_u[3]
    for b in (1, 3, 5, 7, 9, 11, 13, 15):                 # nothing solved: what is finite is the guess
        m = np.isfinite(xo[b])
        assert np.array_equal(xo[b][m], xg[b][m])
        m = np.isfinite(uo[b])
        assert np.array_equal(uo[b][m], ug[b][m])
