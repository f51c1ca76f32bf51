"""smpc_ray_update (k_ray_update) and the device path of safe_set_data.label_rays on the GPU.  -m gpu only.

The kernel is held bit for bit against safe_set_data.ray_update_statement on a fabricated state with one ray on every branch of the
rule; the labelling loop against the statement-driven loop on the same engine; its labels and certificates against the checks
recomposed from the CPU oracle (ray_cases.py)."""
import functools

import numpy as np
import pytest
import torch  # noqa: F401  (before the engine's library is loaded: PyTorch-ROCm must find the HIP runtime it ships with)

import ray_cases as rc
from conftest import make_problem, make_problem_fr7

pytestmark = pytest.mark.gpu

BISECT_K, BUDGET_K, TOL_TERM, MU0 = 4, 20, 5e-3, 10.0
BRANCHES = ['pending', 'feasible trial 0', 'feasible trial 1', 'feasible middle', 'feasible last', 'budget at trial 0',
            'done status 4 at trial 1', 'done with flags at a middle trial', 'terminal velocity at the last trial', 'node 0 off x0',
            'NaN in the trajectory', 'finished, sentinels', 'pending: terminal velocity, not ended']
OPEN_AFTER = [0, 1, 3, 6, 7, 9, 10, 12]


def _fabricated(nq, N):
    """13 rays, one per branch of the rule: (rays, sqp, flags, x0, x_guess, u_guess) as numpy arrays.  Everything a branch does not
    decide holds random or sentinel values, so a write that should not happen shows."""
    from safe_mpc_amd._lib import SqpState
    from safe_mpc_amd.safe_set_data import BRACKETED, new_ray_state
    B, nx = 13, 2 * nq
    rng = np.random.default_rng(11)
    q = rng.uniform(-1, 1, (B, nq))
    d = rng.standard_normal((B, nq))
    d /= np.linalg.norm(d, axis=1)[:, None]
    rays = new_ray_state(q, d, rng.uniform(2, 4, B), N)
    rays['x_cert'][...] = rng.standard_normal(rays['x_cert'].shape)
    rays['u_cert'][...] = rng.standard_normal(rays['u_cert'].shape)
    rays['iters_total'][:] = rng.integers(0, 50, B)
    last = BISECT_K + 1
    trial = np.array([2, 0, 1, 3, last, 0, 1, 2, last, 3, 2, 4, 3])
    rays['trial'][:] = trial
    rays['lo'][:] = np.where(trial >= 2, 0.25 * rays['hi'], 0.0)
    rays['s'][:] = np.where(trial == 0, 0.0, np.where(trial == 1, rays['hi'], 0.5 * (rays['lo'] + rays['hi'])))
    x0 = np.hstack([q, rays['s'][:, None] * d])
    xg = 0.3 * rng.standard_normal((B, N + 1, nx))
    xg[:, 0] = x0
    xg[:, N, nq:] = rng.uniform(-1, 1, (B, nq)) * TOL_TERM          # at rest within the tolerance
    ug = rng.standard_normal((B, N, nq))
    sqp = {k: np.zeros(B, dt) for k, dt in SqpState.FIELDS}
    sqp['mu'][:] = rng.uniform(10, 1000, B)
    for k in ('alpha', 'merit_before', 'merit', 'violation'):
        sqp[k][:] = rng.uniform(0, 1, B)
    sqp['updated'][:] = 1
    sqp['iters'][:] = 5
    sqp['qp_iter_total'][:] = rng.integers(20, 90, B)
    flags = np.zeros(B, np.int32)
    flags[0] = 8                                                    # pending: not feasible, not ended
    sqp['iters'][5], flags[5] = BUDGET_K, 2                         # ended by the budget
    sqp['done'][6], sqp['status'][6], flags[6] = 1, 4, 0            # the QP failed
    sqp['done'][7], flags[7] = 1, 4                                 # converged to an iterate that fails the torque test
    sqp['iters'][8] = BUDGET_K
    xg[8, N, nq + 1] = 100.0 * TOL_TERM                             # not at rest
    sqp['iters'][9] = BUDGET_K
    xg[9, 0, 2] += 1e-9                                             # does not start where it should
    xg[10, N // 2, 1] = np.nan
    rays['open'][11], rays['kind'][11], sqp['done'][11] = 0, BRACKETED, 1
    rays['lo'][11], rays['hi'][11], rays['s'][11] = -7.5, -7.25, -7.0
    xg[11], ug[11], x0[11] = -7.5, -7.5, -7.5
    xg[12, N, nq] = -100.0 * TOL_TERM
    return rays, sqp, flags, x0, np.ascontiguousarray(xg), ug


def _copy(case):
    rays, sqp, flags, x0, xg, ug = case
    return ({k: v.copy() for k, v in rays.items()}, {k: v.copy() for k, v in sqp.items()}, flags.copy(), x0.copy(), xg.copy(), ug.copy())


def _outputs(case, n_open):
    rays, sqp, flags, x0, xg, ug = case
    out = {f'rays.{k}': np.asarray(v) for k, v in rays.items()}
    out.update({f'sqp.{k}': np.asarray(v) for k, v in sqp.items()})
    out.update(x0=x0, x_guess=xg, u_guess=ug, n_open=np.asarray([int(n_open)], np.int32))
    return out


def _same_bits(got, ref, rows=None):
    for k in ref:
        if k == 'n_open' and rows is not None:
            continue
        a, b = (got[k], ref[k]) if rows is None or k == 'n_open' else (got[k], ref[k][rows])
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k


def _run_statement(case):
    from safe_mpc_amd.safe_set_data import ray_update_statement
    c = _copy(case)
    n = ray_update_statement(*c, bisect=BISECT_K, budget=BUDGET_K, tol_term=TOL_TERM, mu0=MU0)
    return _outputs(c, n)


def _run_kernel(s, case, on_device=False):
    c = _copy(case)
    rays, sqp, flags, x0, xg, ug = c
    kw = dict(bisect=BISECT_K, budget=BUDGET_K, tol_term=TOL_TERM, mu0=MU0)
    if not on_device:
        n = s.ray_update(rays, sqp, flags, x0, xg, ug, **kw)
        return _outputs(c, n[0])
    import torch
    dev = torch.device('cuda', s.device)
    t = lambda a: torch.as_tensor(a, device=dev)
    rays, sqp = {k: t(v) for k, v in rays.items()}, {k: t(v) for k, v in sqp.items()}
    flags, x0, xg, ug = t(flags), t(x0), t(xg), t(ug)
    n = s.ray_update(rays, sqp, flags, x0, xg, ug, torch.full((1,), -3, dtype=torch.int32, device=dev), **kw)
    s.sync()
    h = lambda a: a.cpu().numpy()
    return _outputs(({k: h(v) for k, v in rays.items()}, {k: h(v) for k, v in sqp.items()}, h(flags), h(x0), h(xg), h(ug)), h(n)[0])


def _kernel_problem(case):
    if case == 'nq6_N8':
        return rc.backup_problem()[1]
    if case == 'nq5_N2':
        return make_problem('naive', N=2, nq=5)[1]
    return make_problem_fr7(N=63)[1]


@pytest.mark.parametrize('case', ['nq6_N8', 'nq5_N2', 'fr7_N63'])
def test_ray_update_equals_the_statement(case):
    """every output array bit for bit, on 13 rays that take every branch; the statement itself does what the branch names say"""
    from safe_mpc_amd import safe_set_data as sd
    from safe_mpc_amd.solver import BatchedOcpSolver
    prob = _kernel_problem(case)
    s = BatchedOcpSolver(prob, None)
    nq, N = prob.nq, prob.N
    fab = _fabricated(nq, N)
    ref = _run_statement(fab)
    # the statement: kinds, brackets and the untouched rays are what the branches say
    before = _outputs(_copy(fab), 12)
    kind, is_open, trial = ref['rays.kind'], ref['rays.open'], ref['rays.trial']
    assert np.where(is_open != 0)[0].tolist() == OPEN_AFTER and ref['n_open'][0] == len(OPEN_AFTER)
    assert kind.tolist() == [0, 0, sd.SATURATED, 0, sd.BRACKETED, sd.DEAD, 0, 0, sd.BRACKETED, 0, 0, sd.BRACKETED, 0]
    for b in (0, 11, 12):                                            # pending and finished rays: nothing moves
        for k in ref:
            if k != 'n_open':
                assert ref[k][b].tobytes() == before[k][b].tobytes(), (BRANCHES[b], k)
    for b in (1, 2, 3, 4):                                           # feasible: certificate kept, lo = s
        assert np.array_equal(ref['rays.x_cert'][b], fab[4][b]) and np.array_equal(ref['rays.u_cert'][b], fab[5][b])
        assert ref['rays.lo'][b] == fab[0]['s'][b] and ref['rays.hi'][b] == fab[0]['hi'][b]
    for b in (5, 6, 7, 8, 9, 10):                                    # infeasible: certificate as it was, hi = s
        assert np.array_equal(ref['rays.x_cert'][b], fab[0]['x_cert'][b])
        assert ref['rays.hi'][b] == fab[0]['s'][b] and ref['rays.lo'][b] == fab[0]['lo'][b]
    for b in (1, 3, 6, 7, 9, 10):                                    # the next trial: constant guess at the new s, fresh SQP state
        s_new = fab[0]['hi'][b] if fab[0]['trial'][b] == 0 else 0.5 * (ref['rays.lo'][b] + ref['rays.hi'][b])
        start = np.concatenate([fab[0]['q'][b], s_new * fab[0]['d'][b]])
        assert ref['rays.s'][b] == s_new and np.array_equal(ref['x0'][b], start)
        assert np.array_equal(ref['x_guess'][b], np.tile(start, (N + 1, 1))) and not ref['u_guess'][b].any()
        assert ref['sqp.mu'][b] == MU0 and all(ref[f'sqp.{k}'][b] == 0 for k in ('done', 'status', 'iters', 'qp_iter_total', 'updated'))
        assert trial[b] == fab[0]['trial'][b] + 1 and ref['rays.iters_total'][b] == fab[0]['iters_total'][b] + fab[1]['iters'][b]
    for b in (2, 4, 5, 8):                                           # finished now
        assert is_open[b] == 0 and ref['sqp.done'][b] == 1
    # the kernel, host pointers: the statement's bits, twice
    got = _run_kernel(s, fab)
    _same_bits(got, ref)
    _same_bits(_run_kernel(s, fab), got)
    # torch device pointers
    _same_bits(_run_kernel(s, fab, on_device=True), ref)
    # every ray alone (B = 1) gives the bits it gets among the 13
    for b in range(13):
        one = tuple({k: v[b:b + 1].copy() for k, v in part.items()} if isinstance(part, dict) else part[b:b + 1].copy() for part in fab)
        g1 = _run_kernel(s, one)
        _same_bits(g1, ref, rows=slice(b, b + 1))
        assert g1['n_open'][0] == int(b in OPEN_AFTER), BRANCHES[b]


def test_ray_update_refuses_bad_arguments():
    from safe_mpc_amd._lib import EngineError
    from safe_mpc_amd.solver import BatchedOcpSolver
    prob = rc.backup_problem()[1]
    s = BatchedOcpSolver(prob, None)
    rays, sqp, flags, x0, xg, ug = _fabricated(prob.nq, prob.N)
    with pytest.raises(EngineError, match='bisect'):
        s.ray_update(rays, sqp, flags, x0, xg, ug, bisect=-1, budget=5)
    with pytest.raises(EngineError, match='budget'):
        s.ray_update(rays, sqp, flags, x0, xg, ug, bisect=2, budget=0)
    with pytest.raises(ValueError, match='ray state lo'):
        s.ray_update(dict(rays, lo=rays['lo'].astype(np.float32)), sqp, flags, x0, xg, ug)


def test_new_ray_state_and_sample_rays_through_the_solver():
    """BatchedOcpSolver.new_ray_state is the module's state, as numpy and on a tensor's device; sample_rays filters through the
    solver's check_trajectory to the configurations its numpy filter keeps"""
    from safe_mpc_amd import safe_set_data as sd
    from safe_mpc_amd.solver import BatchedOcpSolver
    prob = rc.backup_problem()[1]
    s = BatchedOcpSolver(prob, None)
    q, d, s_hi = rc.random_rays()
    ref = sd.new_ray_state(q, d, s_hi, prob.N)
    like = torch.zeros(1, device=torch.device('cuda', s.device))
    for st in (s.new_ray_state(q, d, s_hi), {k: v.cpu().numpy() for k, v in s.new_ray_state(q, d, s_hi, like=like).items()}):
        assert all(st[k].dtype == ref[k].dtype and np.array_equal(st[k], ref[k]) for k in ref)
    a, b = sd.sample_rays(prob, 40, seed=2, solver=s), sd.sample_rays(prob, 40, seed=2)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


# ---- 2. the labelling loop on the device ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _device_labels(which, batch, bookkeeping):
    from safe_mpc_amd.safe_set_data import label_rays
    q, d, s_hi = rc.random_rays() if which == 'random' else rc.designed_rays()
    ctrl = rc.engine_controller(batch)
    return rc._freeze_result(label_rays(ctrl, q, d, s_hi, bisect=rc.BISECT, budget=rc.BUDGET, check_every=rc.CHECK_EVERY, batch=batch,
                                        bookkeeping=bookkeeping))


def test_device_loop_equals_the_statement_driven_loop():
    """on the random rays: labels, kinds, trials, iterations and certificates bit for bit those of the loop that calls the same sqp
    and check_guess and decides on the host; the same with batch = 16 and batch = 5"""
    from safe_mpc_amd import safe_set_data as sd
    dev16, dev5 = _device_labels('random', 16, 'device'), _device_labels('random', 5, 'device')
    ref = _device_labels('random', 16, 'statement')
    print('device: kinds', dev16['kind'].tolist(), 'trials', dev16['trials'].tolist(), 'iters', dev16['iters'].tolist(), 'rounds',
          dev16['rounds'], 'labels', np.round(dev16['label'], 3).tolist())
    assert np.where(dev16['kind'] == sd.BRACKETED)[0].tolist() == rc.RANDOM_BRACKETED and (dev16['kind'] == sd.SATURATED).sum() == 13
    for k in ('label', 'kind', 'lo', 'hi', 'trials', 'iters', 'x_cert', 'u_cert'):
        assert np.array_equal(dev16[k], ref[k], equal_nan=True), k
        assert np.array_equal(dev5[k], dev16[k], equal_nan=True), k


# ---- 3. the device's certificates and labels against the oracle ----------------------------------------------------------------------
def test_device_certificates_pass_the_oracle_checks():
    q, d, _ = rc.random_rays()
    rc.assert_certificates(q, d, _device_labels('random', 16, 'device'))


def test_device_labels_of_the_designed_rays():
    res = _device_labels('designed', 12, 'device')
    print('kinds', res['kind'].tolist(), 'trials', res['trials'].tolist())
    rc.assert_designed_order(res)


# ---- 4. end to end: labels -> fit -> checkpoint -> a controller that uses it ------------------------------------------------------------
def test_end_to_end_checkpoint_in_a_controller(tmp_path):
    """fit hidden = 32 for 50 epochs on the 28 labelled rays, save, build an htwa controller whose network_path names the file: nn_val
    of eval_nodes equals the torch forward of the reference's formula (safe_set.py:82-94) within 2e-5 (1 + |.|), and one RTI solve
    returns finite iterates"""
    import torch
    from conftest import constant_guess, sample_instances
    from safe_mpc_amd import safe_set_data as sd
    from safe_mpc_amd.controller import get_controller
    rnd, des = _device_labels('random', 16, 'device'), _device_labels('designed', 12, 'device')
    (q1, d1, _), (q2, d2, _) = rc.random_rays(), rc.designed_rays()
    data = {'q': np.vstack([q1, q2]), 'd': np.vstack([d1, d2]), 'label': np.concatenate([rnd['label'], des['label']]),
            'kind': np.concatenate([rnd['kind'], des['kind']])}
    par = rc.ray_params()
    par.net_size = [2 * rc.NQ, 32, 1]
    net, mean, std, info = sd.fit_safe_set(data, par, epochs=50, seed=0, hidden=32)
    path = str(tmp_path / 'safe_set.pt')
    sd.save_checkpoint(path, net, mean, std)
    par.net_path, par.use_net, par.N = path, True, 10
    ctrl = get_controller('htwa', par, 8)
    prob, N, nq = ctrl.problem, ctrl.N, ctrl.nq
    assert np.array_equal(ctrl.net.mean, mean) and np.array_equal(ctrl.net.std, std)
    x0 = sample_instances(prob, 8, seed=4, vel_scale=0.3)
    xg, ug, p = constant_guess(prob, x0, alpha=par.alpha)
    g = np.asarray(ctrl.ocp_solver.eval_nodes(xg, ug, p)['nn_val'])[:, N]
    v = x0[:, nq:].copy()
    v[:, 0] += par.eps
    vn = np.linalg.norm(v, axis=1)
    inp = torch.as_tensor(np.hstack([(x0[:, :nq] - mean) / std, v / vn[:, None]]), dtype=torch.float32)
    with torch.no_grad():
        ref = net(inp).reshape(-1).numpy().astype(float) * (100.0 - par.alpha) / 100.0 - vn
    print('nn_val', g, 'torch', ref)
    assert np.all(np.abs(g - ref) <= 2e-5 * (1.0 + np.abs(ref)))
    ctrl.setGuess(xg, ug)
    ctrl.solve(x0)
    assert np.all(np.isfinite(ctrl.x_temp)) and np.all(np.isfinite(ctrl.u_temp))
