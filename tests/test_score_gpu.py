"""smpc_score_rollout (k_score_seg / k_score_safe / k_score_combine) on the GPU.  -m gpu only.

The kernels are held against closed_loop.score_rollout_statement evaluated with the CPU oracle (Oracle.eval_nodes for ee / row_val,
its network value for g) on logs with planted extremes (score_cases.py; test_score_host.py checks that they are well separated, so
the integer slots are decided).  Tolerances are the suite's two: 1e-9 (1 + |.|) for what is FP64 end to end, 2e-5 (1 + |.|) for what
passes through the fp32 network.  B = 70 (a full wavefront of instances and a partial one), n_steps 1 and 45 (segments of 32)."""
import functools

import numpy as np
import pytest

import score_cases as sc
from conftest import make_problem, sample_instances

pytestmark = pytest.mark.gpu

F64 = slice(0, 6)        # d0..d5
CASES = [(n, T) for n in sc.PROBLEMS for T in sc.STEPS_GPU]


@functools.lru_cache(maxsize=None)
def _solver(name):
    from safe_mpc_amd.solver import BatchedOcpSolver
    par, prob, net = sc.case_problem(name)
    return BatchedOcpSolver(prob, net)


def _close(got, ref, tol):
    same_inf = np.isinf(ref) & (got == ref)
    with np.errstate(invalid='ignore'):
        return np.all(same_inf | (np.abs(got - ref) <= tol * (1.0 + np.abs(ref))))


def _err(got, ref):
    with np.errstate(invalid='ignore'):
        return np.nanmax(np.where(np.isinf(ref), 0.0, np.abs(got - ref) / (1.0 + np.abs(ref))), axis=0)


@pytest.mark.parametrize('name,T', CASES)
def test_score_matches_the_oracle_statement(name, T):
    """out within 1e-9 (1 + |.|) (d0..d5) and 2e-5 (1 + |.|) (d6), outi equal for all 70 instances; with the constant ee_ref and
    with a trajectory shorter than the log; with the safe-set score and without (d6 = +inf, i3 = -1, the rest the same bits)"""
    c, s = sc.reference(name, T), _solver(name)
    out, outi = s.score_rollout(c['x'], c['u'], c['lx'], c['lu'], want_safe=True)
    ro, ri = c['ref']
    print(name, T, 'error', _err(out, ro), 'index mismatches', int((outi != ri).sum()))
    assert np.array_equal(outi, ri)
    assert _close(out[:, F64], ro[:, F64], 1e-9) and _close(out[:, 6], ro[:, 6], 2e-5)
    off, offi = s.score_rollout(c['x'], c['u'], c['lx'], c['lu'])
    assert np.all(off[:, 6] == np.inf) and np.all(offi[:, 3] == -1)
    assert np.array_equal(off[:, F64], out[:, F64]) and np.array_equal(offi[:, :3], outi[:, :3])
    to, ti = s.score_rollout(c['x'], c['u'], c['lx'], c['lu'], traj=c['traj'])
    ro, ri = c['ref_traj']
    print(name, T, 'traj error', _err(to, ro))
    assert np.array_equal(ti, ri) and _close(to[:, F64], ro[:, F64], 1e-9) and np.all(to[:, 6] == np.inf)
    assert np.all(to[:, 1] != out[:, 1]) and np.array_equal(to[:, [2, 4, 5]], out[:, [2, 4, 5]])
    ts, tsi = s.score_rollout(c['x'], c['u'], c['lx'], c['lu'], traj=c['traj'], want_safe=True)
    assert np.array_equal(ts[:, 6], out[:, 6]) and np.array_equal(tsi[:, 3], outi[:, 3]) and np.array_equal(ts[:, F64], to[:, F64])
    # last_x = last_u = None: the logs are complete
    xf, uf = np.where(np.abs(c['x']) < 1e100, c['x'], 0.1), np.where(np.abs(c['u']) < 1e100, c['u'], 0.1)
    B = sc.B_GPU
    full, fulli = s.score_rollout(xf, uf, np.full(B, T, np.int64), np.full(B, T - 1, np.int64), want_safe=True)
    none, nonei = s.score_rollout(xf, uf, want_safe=True)
    assert np.array_equal(none, full) and np.array_equal(nonei, fulli) and np.all(np.isfinite(none))


@pytest.mark.parametrize('name,T', CASES)
def test_score_is_deterministic_and_isolated(name, T):
    """a second call gives the same bits; instances 64..69 scored alone give the bits they had inside the batch of 70 (d0..d5,
    i0..i2)"""
    c, s = sc.reference(name, T), _solver(name)
    out, outi = s.score_rollout(c['x'], c['u'], c['lx'], c['lu'], want_safe=True)
    o2, i2 = s.score_rollout(c['x'], c['u'], c['lx'], c['lu'], want_safe=True)
    assert np.array_equal(o2, out, equal_nan=True) and np.array_equal(i2, outi)
    t = slice(64, 70)
    o6, i6 = s.score_rollout(np.ascontiguousarray(c['x'][:, t]), np.ascontiguousarray(c['u'][:, t]), c['lx'][t], c['lu'][t], want_safe=True)
    assert np.array_equal(o6[:, F64], out[t, F64]) and np.array_equal(i6[:, :3], outi[t, :3])
    assert _close(o6[:, 6], out[t, 6], 2e-5) and np.array_equal(i6[:, 3], outi[t, 3])


@pytest.mark.parametrize('name', sc.PROBLEMS)
def test_score_mask_and_device_pointers(name):
    """masked-out rows keep a sentinel; torch tensors give the bits of the numpy path, read after sync()"""
    import torch
    c, s = sc.reference(name, 45), _solver(name)
    B = sc.B_GPU
    out, outi = s.score_rollout(c['x'], c['u'], c['lx'], c['lu'], want_safe=True)
    mask = (np.arange(B) % 3 != 1).astype(np.uint8)
    om, im = np.full((B, 7), -7.5), np.full((B, 4), -7, np.int32)
    s.score_rollout(c['x'], c['u'], c['lx'], c['lu'], want_safe=True, mask=mask, out=om, outi=im)
    assert np.all(om[mask == 0] == -7.5) and np.all(im[mask == 0] == -7)
    assert np.array_equal(om[mask != 0], out[mask != 0]) and np.array_equal(im[mask != 0], outi[mask != 0])
    dev = torch.device('cuda', s.device)
    t = lambda a: torch.tensor(a, device=dev)          # noqa: E731
    od, idv = s.score_rollout(t(c['x']), t(c['u']), t(c['lx']), t(c['lu']), want_safe=True, mask=t(mask),
                              out=torch.full((B, 7), -7.5, dtype=torch.float64, device=dev),
                              outi=torch.full((B, 4), -7, dtype=torch.int32, device=dev))
    s.sync()
    assert np.array_equal(od.cpu().numpy(), om) and np.array_equal(idv.cpu().numpy(), im)
    od, idv = s.score_rollout(t(c['x']), t(c['u']), t(c['lx']), t(c['lu']), traj=t(c['traj']))
    s.sync()
    oh, ih = s.score_rollout(c['x'], c['u'], c['lx'], c['lu'], traj=c['traj'])
    assert np.array_equal(od.cpu().numpy(), oh) and np.array_equal(idv.cpu().numpy(), ih)


@pytest.mark.parametrize('name', sc.PROBLEMS)
def test_score_nan_rule(name):
    """a NaN in one valid u row: NaN u2 and cost of that instance only; a NaN in the last valid x row: NaN ee_err2, ee_dist, both
    margins (placed at that step) and safe_min; every other instance keeps its bits"""
    T = 45
    c, s = sc.reference(name, T), _solver(name)
    out, outi = s.score_rollout(c['x'], c['u'], c['lx'], c['lu'], want_safe=True)
    complete = np.where((c['lx'] == T) & (c['lu'] == T - 1))[0]
    bu, bx = int(complete[0]), int(complete[1])
    x, u = c['x'].copy(), c['u'].copy()
    u[5, bu, 2] = np.nan
    x[T, bx, 0] = np.nan
    on, oin = s.score_rollout(x, u, c['lx'], c['lu'], want_safe=True)
    others = np.setdiff1d(np.arange(sc.B_GPU), [bu, bx])
    assert np.array_equal(on[others], out[others]) and np.array_equal(oin[others], outi[others])
    assert np.isnan(on[bu, 0]) and np.isnan(on[bu, 2]) and np.array_equal(on[bu, [1, 3, 4, 5, 6]], out[bu, [1, 3, 4, 5, 6]])
    assert np.array_equal(oin[bu], outi[bu])
    assert np.all(np.isnan(on[bx, [0, 1, 3, 5, 6]])) and on[bx, 2] == out[bx, 2]
    assert oin[bx, 2] == T and oin[bx, 3] == T
    if sc.case_problem(name)[1].desc.n_rows:
        assert np.isnan(on[bx, 4]) and oin[bx, 0] == T and oin[bx, 1] == 0


def test_score_safe_set_over_several_network_passes():
    """A log of more than 2^18 flat rows (B = 70, n_steps = 3800: 266 070 rows, the pass boundary at row 262 144 falls inside step
    3744, between instances 63 and 64), so the network runs in two passes and k_score_safe carries its minimum across them.  d6 / i3
    against (a) the minimum over single-pass calls on the two halves of the same log, (b) the planted step of every instance --
    before, at both sides of and after the boundary, also in logs that end before it -- and (c) the oracle's g of the chosen
    state, all within 2e-5 (1 + |.|); the places equal."""
    from fake_solver import OracleSolver
    from safe_mpc_amd import closed_loop as cl
    par, prob, net = sc.case_problem('htwa_nq6_N20')
    s = _solver('htwa_nq6_N20')
    B, T, nq = sc.B_GPU, 3800, prob.nq
    assert (T + 1) * B > 2 ** 18 and 2 ** 18 // B == 3744 and 2 ** 18 % B == 64
    rng = np.random.default_rng(11)
    x = np.zeros((T + 1, B, prob.nx))
    x[:, :, :nq] = sample_instances(prob, B, seed=4)[None, :, :nq] + 0.01 * rng.standard_normal((T + 1, B, nq))
    x[:, :, nq:] = 0.1 * rng.uniform(-1, 1, (T + 1, B, nq)) * prob.x_max[nq:]
    u = rng.uniform(-1, 1, (T, B, nq))
    lx = np.full(B, T, np.int64)
    lx[5::7] = 100 + np.arange(len(lx[5::7]))                          # logs that end long before the second pass
    lx[6::7] = 3744                                                    # ... and at the boundary step
    lu = np.minimum(lx, T - 1)
    spots = np.array([3, 3743, 3744, 3744, 3745, 3799, 1900])          # (3744: pass 0 for b < 64, pass 1 for b >= 64)
    at = np.minimum(spots[np.arange(B) % 7], lx)
    at[62:66] = 3744
    lx[62:66], lu[62:66] = T, T - 1
    x[at, np.arange(B), nq:] = 0.8 * prob.x_max[nq:]
    out, outi = s.score_rollout(x, u, lx, lu, want_safe=True)
    assert np.array_equal(outi[:, 3], at), (outi[:, 3], at)
    # (a) the two halves, each one pass
    cut = 2000
    lo_o, lo_i = s.score_rollout(x[:cut], u[:cut - 1], np.minimum(lx, cut - 1), np.minimum(lu, cut - 2), want_safe=True)
    hi_o, hi_i = s.score_rollout(np.ascontiguousarray(x[cut:]), np.ascontiguousarray(u[cut:]), np.maximum(lx - cut, 0),
                                 np.maximum(lu - cut, -1), want_safe=True)
    reaches = lx >= cut
    halves = np.where(reaches & (hi_o[:, 6] < lo_o[:, 6]), hi_o[:, 6], lo_o[:, 6])
    halves_at = np.where(reaches & (hi_o[:, 6] < lo_o[:, 6]), hi_i[:, 3] + cut, lo_i[:, 3])
    print('several passes: against the halves', _err(out[:, 6], halves))
    assert _close(out[:, 6], halves, 2e-5) and np.array_equal(outi[:, 3], halves_at)
    # (c) the oracle's g of the chosen states, and of a sample of other valid states (none below the minimum)
    o = OracleSolver(prob, net)
    _, _, g = cl._score_eval_chunks(o, prob, x[outi[:, 3], np.arange(B)], par.alpha, 4096, True)
    print('several passes: against the oracle', _err(out[:, 6], g))
    assert _close(out[:, 6], g, 2e-5)
    js = rng.integers(0, lx + 1)
    _, _, gs = cl._score_eval_chunks(o, prob, x[js, np.arange(B)], par.alpha, 4096, True)
    assert np.all(gs >= out[:, 6] - 2e-5 * (1 + np.abs(gs)))
    # the f64 slots of the long log are those of the statement's order: a second call gives the same bits
    o2, i2 = s.score_rollout(x, u, lx, lu, want_safe=True)
    assert np.array_equal(o2, out) and np.array_equal(i2, outi)


def test_metrics_script_takes_its_costs_from_the_engine():
    """closed_loop_costs_scored with BatchedOcpSolver (the smpc_score_rollout branch) against closed_loop_costs on complete logs"""
    from test_metrics import _load_script
    from safe_mpc_amd.solver import BatchedOcpSolver
    m = _load_script()
    par, prob, net = make_problem('naive', N=2)
    solver = BatchedOcpSolver(prob, None)
    rng = np.random.default_rng(2)
    x = sample_instances(prob, 5, seed=2)[:, None, :] + 0.01 * rng.standard_normal((5, 8, prob.nx))
    u = rng.uniform(-2, 2, (5, 7, prob.nu))
    a, b = m.closed_loop_costs_scored(par, prob, solver, x, u), m.closed_loop_costs(par, prob, solver, x, u)
    assert _close(a, b, 1e-9)
    x[1, 3:], u[1, 2:] = np.nan, np.nan                    # a truncated log: its valid rows only
    t = m.closed_loop_costs_scored(par, prob, solver, x, u)
    assert t[1] < a[1] and np.array_equal(t[[0, 2, 3, 4]], a[[0, 2, 3, 4]])


def test_score_errors():
    from safe_mpc_amd._lib import EngineError
    from safe_mpc_amd.solver import BatchedOcpSolver
    par, prob, net = sc.case_problem('htwa_nq6_N20')
    x, u = np.zeros((4, 2, prob.nx)), np.zeros((3, 2, prob.nu))
    with pytest.raises(EngineError, match=r'engine error -4.*smpc_set_mlp'):
        BatchedOcpSolver(prob, None).score_rollout(x, u, want_safe=True)
    with pytest.raises(EngineError, match=r'engine error -1.*n_steps'):
        _solver('htwa_nq6_N20').score_rollout(x[:1], u[:0])


def test_run_mpc_scores_its_device_logs():
    """run_mpc(on_device=True, score=True, graphs=False), 64 instances, 12 steps, 'st': 'score' equals the statement evaluated on
    the returned host logs with the CPU oracle, and everything else in the dict equals the score=False run bit for bit"""
    from fake_solver import OracleSolver
    from safe_mpc_amd import closed_loop as cl
    par, prob, net = make_problem('st', 'ext', N=10)
    par.back_hor = 10
    B, n_steps = 64, 12
    x0 = sample_instances(prob, B, seed=1)
    xg, ug = np.repeat(x0[:, None, :], 11, axis=1), np.zeros((B, 10, 6))
    res = cl.run_mpc(par, 'st', xg, ug, n_steps=n_steps, on_device=True, score=True, graphs=False)
    ref = cl.run_mpc(par, 'st', xg, ug, n_steps=n_steps, on_device=True, graphs=False)
    assert set(res) == set(ref) | {'score'}
    for k in ref:
        if isinstance(ref[k], np.ndarray):
            assert np.array_equal(ref[k], res[k], equal_nan=True), k
        else:
            assert ref[k] == res[k], k
    bad_x, bad_u = np.isnan(res['x']).any(2), np.isnan(res['u']).any(2)
    lx = np.where(bad_x.any(1), np.argmax(bad_x, axis=1) - 1, n_steps).astype(np.int64)
    lu = np.where(bad_u.any(1), np.argmax(bad_u, axis=1) - 1, n_steps - 1).astype(np.int64)
    out, outi = cl.score_rollout_statement(OracleSolver(prob, net), prob, par, np.transpose(res['x'], (1, 0, 2)),
                                           np.transpose(res['u'], (1, 0, 2)), lx, lu, want_safe=True)
    ref_s = cl._score_dict(out, outi)
    s = res['score']
    assert set(s) == set(ref_s) and all(s[k].shape == (B,) for k in s)
    for k in ('cost', 'ee_err2', 'u2', 'ee_dist', 'coll_margin', 'box_margin'):
        print(k, _err(s[k], ref_s[k]))
        assert _close(s[k], ref_s[k], 1e-9), k
    print('safe_min', _err(s['safe_min'], ref_s['safe_min']))
    assert _close(s['safe_min'], ref_s['safe_min'], 2e-5)
    # the places: the box margin is exact arithmetic on the logged states, so its step is the statement's; for the other two the
    # oracle's value at the place the kernel chose is its extreme within the same tolerances (closed-loop data is not planted)
    assert np.array_equal(s['box_step'], ref_s['box_step'])
    rows, _, g = sc.candidates(OracleSolver(prob, net), prob, par, np.transpose(res['x'], (1, 0, 2)), lx)
    b = np.arange(B)
    assert _close(rows[b, s['coll_step'], s['coll_row']], ref_s['coll_margin'], 1e-9)
    assert _close(g[b, s['safe_step']], ref_s['safe_min'], 2e-5)
