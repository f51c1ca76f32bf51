"""Inputs that drive the interior point to each of its exits (helpers, no tests), shared by test_qp_exits_oracle.py (CPU) and
test_qp_exits_gpu.py.  Every builder returns ``(par, prob, net, x0, xg, ug, p, bounds, classes)``: ``bounds`` is None or the
``(lo, hi)`` of set_instance_bounds, ``classes`` labels every instance by what the ORACLE does with it (a numpy array of strings,
computed from oracle runs here, never from the engine):

  capped ....... status 0 with qp_iter equal to a qp_max_iter below the 4-6 iterations convergence takes
  clean ........ status 0 within CLEAN_MAX_ITER iterations
  slow ......... status 0 after more than CLEAN_MAX_ITER iterations (ill-conditioned but solvable)
  breakdown0 ... status 4 at iteration 0: the first factorisation fails (or the input is not finite), nothing is solved
  stall ........ status 4 through the stall exit: qp_stall_iters > 0 ends the solve earlier than it ends with qp_stall_iters = 0
  minstep ...... status 4 with qp_stall_iters = 0 after at least one iteration: the step length falls below the minimum
  late ......... status 4 after at least one iteration, at the SAME count with and without the stall option: the solve fails in
                 iteration k >= 1 (the factorisation breaks down, or the step length is not a number or below the minimum)
                 before the stall count is reached.  The two instances LATE of the mixed batch are of this kind: found by a scan
                 of the oracle over 1200 instances with reference magnitudes between 50 and 1e3, they fail in iteration 6 and 2
                 right after steps of 2e-3, and their iterate equals, bit for bit, what qp_max_iter = 6 / 2 returns -- the failing
                 iteration applies nothing (test_qp_exits_oracle.py pins both facts)
  other ........ anything else (a status the ABI has and none of the above)
"""
import numpy as np

from conftest import constant_guess, make_problem, make_problem_fr7, sample_instances

CLEAN_MAX_ITER = 8
CAP_CASES = ['naive', 'st', 'zerovel', 'constraint_everywhere', 'fr7', 'nq5']
FP64_CASES = ('naive', 'zerovel')            # no network row: FP64 end to end
B_CAP, B_MIXED, B_NONFINITE, N_MIXED = 32, 32, 16, 12
# the mixed batch's instances B_MIXED, B_MIXED + 1: (index into sample_instances(prob, 400, seed=9), reference components, value, iteration)
LATE = [(180, slice(0, 3), 234.79696676838591, 6), (388, slice(0, 1), 370.4538917557722, 2)]


def _oracle(prob, net):
    from oracle.oracle import Oracle
    return Oracle(prob, (net.weights, net.biases))


def cap_problem(case, cap=None):
    """the problem of a cap case; qp_max_iter is set in the descriptor BEFORE any handle is made from it"""
    if case == 'naive':
        par, prob, net = make_problem('naive', 'ext', N=30)
    elif case == 'st':
        par, prob, net = make_problem('st', 'ext', N=30)
    elif case == 'zerovel':
        par, prob, net = make_problem('zerovel', 'nls', N=20)
    elif case == 'constraint_everywhere':
        par, prob, net = make_problem('constraint_everywhere', 'ext', N=10)
    elif case == 'fr7':
        par, prob, net = make_problem_fr7(N=16)
    elif case == 'nq5':
        par, prob, net = make_problem('st', 'ext', N=12, nq=5)
    else:
        raise KeyError(case)
    if cap is not None:
        prob.desc.qp_max_iter = int(cap)
    return par, prob, net


def capped(case, cap):
    par, prob, net = cap_problem(case, cap)
    x0 = sample_instances(prob, B_CAP, seed=2, vel_scale=0.1)
    xg, ug, p = constant_guess(prob, x0)
    _, _, st, it = _oracle(prob, net).solve_batch(x0, xg, ug, p)
    classes = np.where((st == 0) & (it == cap), 'capped', np.where((st == 0) & (it < cap), 'clean', 'other'))
    return par, prob, net, x0, xg, ug, p, None, classes


def unreachable_tube(prob, x0, N, node=3, shift=0.4):
    """RealReceding's box at one node, centred where the arm cannot be after `node` steps (the tube of test_oracle_qp.py)"""
    from test_oracle_qp import _unreachable_tube
    return _unreachable_tube(prob, x0, N, node=node, shift=shift)


def classify(st, it, st_other, it_other, stall):
    """classes of one oracle run (st, it) with qp_stall_iters = ``stall``, given the run with the other stall setting"""
    out = np.full(len(st), 'other', dtype='<U12')
    for b in range(len(st)):
        if st[b] == 0:
            out[b] = 'clean' if it[b] <= CLEAN_MAX_ITER else 'slow'
        elif st[b] == 4 and it[b] == 0:
            out[b] = 'breakdown0'
        elif st[b] == 4:
            it_on, it_off = (it[b], it_other[b]) if stall > 0 else (it_other[b], it[b])
            if st_other[b] == 4 and it_on < it_off:
                out[b] = 'stall' if stall > 0 else 'minstep'
            elif st_other[b] == 4 and it_on == it_off:
                out[b] = 'late'
    return out


def mixed_problem(stall, **over):
    return make_problem('real_receding', N=N_MIXED, qp_stall_iters=stall, **over)


def mixed_inputs(prob, B=B_MIXED):
    """b % 4: 0 clean, 1 unreachable tube, 2 end-effector reference at 1e3 (the exact Hessian of the 'ext' cost goes indefinite),
    3 reference at 50 (ill-conditioned, mostly solvable); then the instances of LATE"""
    N = prob.N
    x0 = np.concatenate([sample_instances(prob, B, seed=4), sample_instances(prob, 400, seed=9)[[l[0] for l in LATE]]])
    xg, ug, p = constant_guess(prob, x0)
    lo, hi = unreachable_tube(prob, x0, N)
    free = (np.arange(len(x0)) % 4 != 1) | (np.arange(len(x0)) >= B)
    lo[free], hi[free] = prob.x_min, prob.x_max
    lo[free, N], hi[free, N] = prob.lbx_e, prob.ubx_e
    p[:B][np.arange(B) % 4 == 2, :, 0:3] = 1e3
    p[:B][np.arange(B) % 4 == 3, :, 0:3] = 50.0
    for j, (_, comp, val, _) in enumerate(LATE):
        p[B + j, :, comp] = val
    return x0, xg, ug, p, (lo, hi)


def mixed_classes(x0, xg, ug, p, bounds, net, stall, **over):
    runs = {}
    for s in sorted({int(stall), 0, 24}):
        _, prob_s, _ = mixed_problem(s, **over)
        o = _oracle(prob_s, net)
        o.set_instance_bounds(*bounds)
        runs[s] = o.solve_batch(x0, xg, ug, p)[2:]
    other = 0 if stall > 0 else 24
    return classify(runs[int(stall)][0], runs[int(stall)][1], runs[other][0], runs[other][1], stall)


def mixed_batch(stall, **over):
    """real_receding, N = 12, B = 32 + 2: iteration counts 4-6, 24 (or 32-100 with stall = 0), 0 and 11-27 in neighbouring slots, then
    the two instances of LATE"""
    par, prob, net = mixed_problem(stall, **over)
    x0, xg, ug, p, bounds = mixed_inputs(prob)
    classes = mixed_classes(x0, xg, ug, p, bounds, net, stall, **over)
    return par, prob, net, x0, xg, ug, p, bounds, classes


# (name, array, index, value): one entry of one input of instance 2 j + 1 is made non-finite (or huge); even instances stay clean
NONFINITE = [('x0 nan', 'x0', (3,), np.nan), ('x0 +inf', 'x0', (8,), np.inf),
             ('xg running nan', 'xg', (5, 2), np.nan), ('xg terminal -inf', 'xg', (12, 7), -np.inf),
             ('ug nan', 'ug', (4, 1), np.nan), ('p[...,0] nan', 'p', (6, 0), np.nan),
             ('p[...,3] +inf', 'p', (12, 3), np.inf), ('ug 1e308', 'ug', (0, 0), 1e308)]


def nonfinite_batch():
    """'st', N = 12, B = 16: odd instances carry one non-finite (or 1e308) input entry each (NONFINITE), even ones are clean"""
    par, prob, net = make_problem('st', 'ext', N=12)
    x0 = sample_instances(prob, B_NONFINITE, seed=2, vel_scale=0.1)
    xg, ug, p = constant_guess(prob, x0)
    arrs = {'x0': x0, 'xg': xg, 'ug': ug, 'p': p}
    for j, (_, name, idx, val) in enumerate(NONFINITE):
        arrs[name][(2 * j + 1,) + idx] = val
    with np.errstate(all='ignore'):
        _, _, st, it = _oracle(prob, net).solve_batch(x0, xg, ug, p)
    classes = classify(st, it, st, it, 0)
    return par, prob, net, x0, xg, ug, p, None, classes


def perturbed(x0, xg, eps=1e-11, seed=7):
    """x0 and the guess built from it moved by eps relative (the known disagreement of the stage records, see
    test_stage_builder_equals_thread_per_node_kernels)"""
    d = eps * x0 * np.random.default_rng(seed).choice([-1.0, 1.0], x0.shape)
    return x0 + d, xg + d[:, None, :]


def rel_u(a, b):
    """|a - b|inf / (1 + |b|inf) per instance"""
    B = len(a)
    return np.abs(a - b).reshape(B, -1).max(1) / (1.0 + np.abs(b).reshape(B, -1).max(1))


def oracle_cap_sensitivity(case, cap, eps=1e-11):
    """how far the ORACLE's capped iterate moves, per instance, under ``perturbed``: (controls relative to 1 + |u|inf, states absolute)"""
    par, prob, net, x0, xg, ug, p, _, _ = capped(case, cap)
    o = _oracle(prob, net)
    xa, ua, sa, ia = o.solve_batch(x0, xg, ug, p)
    x1, g1 = perturbed(x0, xg, eps)
    xb, ub, sb, ib = o.solve_batch(x1, g1, ug, p)
    assert np.array_equal(sa, sb) and np.array_equal(ia, ib)
    return rel_u(ub, ua), np.abs(xb - xa).reshape(len(xa), -1).max(1)
