"""The callers on either side of the solve (kernels_callers.hpp) at the shapes test_callers_parity (nq = 6, B = 16, N = 10) does
not reach, against the CPU oracle:

  plant_step ......... nq in {5, 6, 7}: 9, 8, 7 instances per block of 64 lanes, one lane idle for nq = 5 and 7;
                       B in {1, PER - 1, PER, PER + 1, 2 PER + 3}; nominal, per-instance joints, torque noise; host and device path
  provide_control .... N in {1, 2, 3} (N = 1 is a branch of its own), nq in {5, 7}, odd B, mixed accept: exact, it only copies
  guess_correction ... same shapes: 1e-13 scaled by the state's magnitude
  check_trajectory ... a component exactly at x_max + tol_x / x_min - tol_x passes, the next double beyond fails, on the first and
                       the last component, node and instance; the last node of the last instance as the only bad one; n_nodes = 1
  accumulate_stats ... B in {1, 63, 64, 65, 4097}, sums past 2^32, negative and NULL qp_iter, several calls into one counter, B = 0

Every test prints a line `LOOPKERNELS callers ...` (profiles/loop_kernel_tests.txt)."""
import numpy as np
import pytest

from conftest import make_problem, make_problem_fr7, sample_instances
from loop_cases import Dev

pytestmark = pytest.mark.gpu

_MADE = {}


def _made(nq, N):
    """(par, prob, engine, oracle), one per shape for the whole module"""
    from oracle.oracle import Oracle
    from safe_mpc_amd.solver import BatchedOcpSolver
    if (nq, N) not in _MADE:
        par, prob, net = make_problem_fr7('naive', 'ext', N=N) if nq == 7 else make_problem('naive', 'ext', N=N, nq=nq)
        _MADE[nq, N] = (par, prob, BatchedOcpSolver(prob, None), Oracle(prob))
    return _MADE[nq, N]


@pytest.mark.parametrize('nq', [5, 6, 7])
def test_plant_step_partial_blocks_and_idle_lanes(nq):
    """Which instances saturate a torque is part of the inputs: instance b commands accelerations of 500 to 1000 rad/s^2 if
    b + B is odd, of 0.5 to 1 rad/s^2 otherwise -- asserted on the oracle's side (nominal and noise: from its inverse dynamics;
    per-instance joints: an unclipped step returns the commanded acceleration)."""
    import torch
    par, prob, s, o = _made(nq, 1)
    PER = 64 // (nq + 2)
    rng = np.random.default_rng(40 + nq)
    worst = dict(x=0.0, u=0.0, res=0.0)
    n_clip = n_all = 0
    for B in (1, PER - 1, PER, PER + 1, 2 * PER + 3):
        x = np.concatenate([rng.uniform(prob.lbx[:nq], prob.ubx[:nq], (B, nq)), rng.uniform(-1, 1, (B, nq))], 1)
        hard = (np.arange(B) + B) % 2 == 1
        u = rng.choice([-1.0, 1.0], (B, nq)) * rng.uniform(0.5, 1, (B, nq)) * np.where(hard, 1000.0, 1.0)[:, None]
        jt = np.tile(prob.joint_table(), (B, 1))
        jt['mass'] *= 1 + 0.1 * rng.uniform(-1, 1, jt['mass'].shape)
        jt['com'] *= 1 + 0.1 * rng.uniform(-1, 1, jt['com'].shape)
        noise = rng.normal(0, 0.5, (B, nq))
        for mode, joints, tn in (('nominal', None, None), ('joints', jt, None), ('noise', None, noise)):
            xo, eo = o.plant_step(x, u, joints, tn)
            if joints is None:
                tau = np.array([o.rnea(x[b, :nq], x[b, nq:], u[b]) for b in range(B)]) + (0.0 if tn is None else tn)
                clipped = (np.abs(tau) > prob.tau_max).any(1)
            else:
                clipped = np.abs(eo - u).max(1) > 1e-6
            assert np.array_equal(clipped, hard), (nq, B, mode)
            n_clip, n_all = n_clip + int(clipped.sum()), n_all + B
            # host path
            xa, ea = s.plant_step(x, u, joints, tn)
            # device path, u_eff requested, outputs between sentinels
            dev = Dev(dict(x=x, u=u, xn=np.full((B, 2 * nq), 7.5), ue=np.full((B, nq), 7.5),
                           jn=None if joints is None else np.ascontiguousarray(joints).view(np.float64).reshape(B, nq, -1), tn=tn))
            s.plant_step(dev.t['x'], dev.t['u'], dev.t['jn'], dev.t['tn'], out=(dev.t['xn'], dev.t['ue']))
            h = dev.host()
            assert np.array_equal(h['xn'], xa) and np.array_equal(h['ue'], ea) and np.array_equal(h['x'], x) and np.array_equal(h['u'], u)
            assert np.allclose(xa, xo, rtol=0, atol=1e-10) and np.allclose(ea, eo, rtol=0, atol=1e-7), (nq, B, mode)
            worst['x'], worst['u'] = max(worst['x'], np.abs(xa - xo).max()), max(worst['u'], np.abs(ea - eo).max())
            if joints is None:
                # the acceleration the step applied, pushed back through the torque row, gives the clipped command
                tau_of = lambda a: s.eval_nodes(np.stack([x, x], 1), a[:, None, :], np.zeros((B, 2, 5)))['tau'][:, 0, :nq]
                tau_cmd = np.clip(tau_of(u) + (0.0 if tn is None else tn), -prob.tau_max, prob.tau_max)
                res = np.abs(tau_of(ea) - tau_cmd).max() / (1.0 + np.abs(tau_cmd).max())
                assert res < 1e-9, (nq, B, mode, res)
                worst['res'] = max(worst['res'], res)
            dt = par.dt
            assert np.allclose(xa[:, :nq], x[:, :nq] + dt * x[:, nq:] + 0.5 * dt * dt * ea, rtol=0, atol=1e-13)
            assert np.allclose(xa[:, nq:], x[:, nq:] + dt * ea, rtol=0, atol=1e-13)
    print(f'LOOPKERNELS callers plant_step nq {nq} ({PER} per block): B 1 {PER - 1} {PER} {PER + 1} {2 * PER + 3} x nominal joints noise, '
          f'{n_clip} of {n_all} instances clip, x error {worst["x"]:.1e} (1e-10), u_eff error {worst["u"]:.1e} (1e-7), torque residual '
          f'{worst["res"]:.1e} (1e-9), device path = host path bit for bit')


@pytest.mark.parametrize('nq', [5, 7])
@pytest.mark.parametrize('N', [1, 2, 3])
def test_provide_control_and_guess_correction_short_horizons(nq, N):
    par, prob, s, o = _made(nq, N)
    B = 13
    rng = np.random.default_rng(10 * nq + N)
    xg = rng.uniform(-2, 2, (B, N + 1, 2 * nq))
    ug = rng.uniform(-30, 30, (B, N, nq))
    xt, ut = rng.uniform(-2, 2, xg.shape), rng.uniform(-30, 30, ug.shape)
    accept = (rng.random(B) < 0.5).astype(np.int32)
    assert 0 < accept.sum() < B
    for got, want, name in zip(s.provide_control(accept, xt, ut, xg, ug), o.provide_control(accept, xt, ut, xg, ug), ('x_guess', 'u_guess', 'u_apply')):
        assert np.array_equal(got, want), (nq, N, name)
    # what provideControl does, said once more without the oracle: the accepted iterate or the old guess, shifted by one node
    xs, us = np.where(accept[:, None, None] != 0, xt, xg), np.where(accept[:, None, None] != 0, ut, ug)
    gx, gu, ua = s.provide_control(accept, xt, ut, xg, ug)
    assert np.array_equal(ua, us[:, 0]) and np.array_equal(gx[:, :N], xs[:, 1:]) and np.array_equal(gx[:, N], xs[:, N])
    assert np.array_equal(gu[:, :N - 1], us[:, 1:]) and np.array_equal(gu[:, N - 1], us[:, N - 1])
    a, b = s.guess_correction(xg, ug), o.guess_correction(xg, ug)
    tol = 1e-13 * max(1.0, np.abs(b).max())
    assert np.array_equal(a[:, 0], xg[:, 0]) and np.abs(a - b).max() <= tol, (nq, N, np.abs(a - b).max())
    print(f'LOOPKERNELS callers provide_control / guess_correction nq {nq} N {N} B {B}: {int(accept.sum())} accepted, copies exact, '
          f'roll-out error {np.abs(a - b).max():.1e} (bound {tol:.1e})')


def test_check_trajectory_at_the_edge_of_the_box():
    par, prob, s, o = _made(6, 2)
    nq, B, n = 6, 5, 4
    nx = 2 * nq
    base = np.repeat(sample_instances(prob, B, seed=9, margin=0.3)[:, None, :], n, axis=1)
    chk = lambda m, x: m.check_trajectory(x, prob.x_min, prob.x_max, par.tol_x, prob.row_check[:, 0], prob.row_check[:, 1])
    both = lambda x: (np.asarray(chk(s, x), bool), np.asarray(chk(o, x), bool))
    assert both(base)[0].all() and both(base)[1].all()
    n_cases = 0
    for i in (0, nx - 1):
        for k in (0, n - 1):
            for b in (0, B - 1):
                for edge, beyond in ((prob.x_max[i] + par.tol_x, np.inf), (prob.x_min[i] - par.tol_x, -np.inf)):
                    for value, passes in ((edge, True), (np.nextafter(edge, beyond), False)):
                        x = base.copy()
                        x[b, k, i] = value
                        want = np.ones(B, bool)
                        want[b] = passes
                        got, ref = both(x)
                        assert np.array_equal(ref, want), ('oracle', i, k, b, value)
                        assert np.array_equal(got, want), (i, k, b, value)
                        n_cases += 1
    x = base.copy()
    x[B - 1, n - 1, 3] = prob.x_max[3] + 1.0                # the only bad node: the last node of the last instance
    got, ref = both(x)
    assert np.array_equal(ref, np.arange(B) < B - 1) and np.array_equal(got, ref)
    x1 = base[:, :1].copy()                                 # n_nodes = 1
    x1[2, 0, nq + 1] = prob.x_min[nq + 1] - 1.0
    got, ref = both(x1)
    assert np.array_equal(ref, np.arange(B) != 2) and np.array_equal(got, ref)
    dx = Dev(dict(x=x))                                     # ... and the device path on the last-node case
    assert np.array_equal(s.check_trajectory(dx.t['x']).cpu().numpy().astype(bool), np.arange(B) < B - 1)
    print(f'LOOPKERNELS callers check_trajectory: {n_cases} edge cases (at the bound: ok, next double: not), last node of the last '
          f'instance, n_nodes = 1: engine = oracle = expected')


@pytest.mark.parametrize('B', [1, 63, 64, 65, 4097])
def test_accumulate_stats_counts_exactly(B):
    par, prob, s, o = _made(6, 2)
    rng = np.random.default_rng(B)
    start = np.array([5, 7, 11], np.int64)
    dev = Dev(dict(acc=start))
    want = [int(v) for v in start]
    calls = []
    for c in range(4):
        status = rng.choice(np.array([0, 0, 4, 2, -1], np.int32), B)
        qp = rng.integers(1_600_000_000, 2**31 - 1, B, endpoint=True).astype(np.int32)
        if B > 1:
            qp[rng.random(B) < 0.2] = rng.integers(-2**31, 0)          # counted as 0
        qp[0] = 2**31 - 1
        calls.append((status, qp))
    for c, (status, qp) in enumerate(calls):
        d = Dev(dict(status=status, qp=qp))
        s.accumulate_stats(d.t['status'], d.t['qp'] if c != 1 else None, dev.t['acc'])          # (the second call: qp_iter NULL)
        h = d.host()
        assert np.array_equal(h['status'], status) and np.array_equal(h['qp'], qp)
        want[0] += 0 if c == 1 else sum(max(int(v), 0) for v in qp)
        want[1] += int(np.count_nonzero(status))
        want[2] += B
    got = dev.host()['acc']
    assert [int(v) for v in got] == want, (B, got, want)
    assert want[0] - 5 > 2**32
    # B = 0: nothing is enqueued, the counters stay
    d = Dev(dict(status=calls[0][0], qp=calls[0][1]))
    assert s.L.smpc_accumulate_stats(s.h, 0, d.t['status'].data_ptr(), d.t['qp'].data_ptr(), dev.t['acc'].data_ptr()) == 0
    s.sync()
    assert [int(v) for v in dev.host()['acc']] == want
    print(f'LOOPKERNELS callers accumulate_stats B {B}: four calls (one without qp_iter) into one counter, iterations {want[0] - 5} '
          f'(> 2^32), failed {want[1] - 7}, solves {want[2] - 11}: exact; B = 0 leaves them')
