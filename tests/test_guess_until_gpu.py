"""smpc_check_guess (k_check_guess) and closed_loop.generate_guess_until on the GPU.  -m gpu only.

The kernel is held against a statement composed from the CPU oracle (Oracle.eval_nodes for tau / row_val / nn_val,
Oracle.guess_correction for the roll-out) and numpy, and against the shipped four-call checkGuess; the loop against one plain batch
advanced round by round.  Tolerances are the suite's two: 1e-9 (1 + |.|) for what is FP64 end to end, 2e-5 (1 + |.|) for what
passes through the fp32 network."""
import numpy as np
import pytest

from conftest import constant_guess, halton, make_problem, make_problem_fr7, sample_instances

pytestmark = pytest.mark.gpu

NEG_INF = -np.inf


# ---- 1. the kernel against the oracle-composed statement --------------------------------------------------------------------------
CASES = ['htwa_nq5_N2', 'htwa_nq6_N20', 'htwa_nq6_N63', 'fr7', 'naive']


def _case_problem(case):
    """(par, prob, net, safe_node)"""
    if case == 'fr7':
        par, prob, net = make_problem_fr7()
        return par, prob, net, prob.N // 2          # the row is on every node: test one in the middle
    if case == 'naive':
        par, prob, net = make_problem('naive', N=20)
        return par, prob, net, None
    nq, N = {'htwa_nq5_N2': (5, 2), 'htwa_nq6_N20': (6, 20), 'htwa_nq6_N63': (6, 63)}[case]
    par, prob, net = make_problem('htwa', N=N, nq=nq)
    return par, prob, net, N


def _colliding_configuration(prob, oracle):
    """a joint configuration inside the box whose collision rows fail their check bounds by a clear margin"""
    nq = prob.nq
    lo, hi = prob.lbx[:nq] + 0.05, prob.ubx[:nq] - 0.05
    p1 = np.zeros((1, prob.N + 1, 5))
    for u in halton(400, nq, skip=3):
        q = lo + u * (hi - lo)
        x = np.tile(np.concatenate([q, np.zeros(nq)]), (1, prob.N + 1, 1))
        rv = oracle.eval_nodes(x, np.zeros((1, prob.N, nq)), p1)['row_val'][0, 0, :prob.desc.n_rows]
        if np.max(np.maximum(prob.row_check[:, 0] - rv, rv - prob.row_check[:, 1])) > 1e-3:
            return q
    raise AssertionError('no colliding configuration found')


def _case_trajectories(par, prob, oracle, safe_node):
    """B = 7 trajectories: a consistent roll-out of small random controls from collision-free starts, of which six are perturbed in
    one predicate each by at least 100 x its tolerance.  Where the perturbation can be made before the roll-out it is (the
    trajectory then stays dynamically consistent), otherwise a node is overwritten (which also breaks the dynamics)."""
    B, N, nq = 7, prob.N, prob.nq
    rng = np.random.default_rng(5)
    x0 = sample_instances(prob, B, seed=2)
    u = 0.05 * rng.standard_normal((B, N, nq))
    k_late = max(1, N // 2)
    x0[1, 1] = prob.x_max[1] + 0.6                                       # box: a joint beyond x_max (tol_x = 5e-3)
    if prob.desc.n_rows:
        q_hit = _colliding_configuration(prob, oracle)
        x0[2, :nq] = q_hit                                               # rows: node 0 inside an obstacle
    u[4, N - 1, 1] = 1000.0                  # torque: one control scaled up (the last one: only node N moves, out of its box as well)
    x = oracle.guess_correction(np.repeat(x0[:, None, :], N + 1, axis=1), u)
    if prob.desc.n_rows:
        x[3, k_late, :nq] = q_hit                                        # rows: a LATER node inside an obstacle (the quirk's case)
    x[5, k_late, 0] += 1e-3                                              # dynamics: one node shifted (tol_dyn sqrt(N + 1) <= 8e-6)
    if safe_node is not None:
        x[6, safe_node, nq:] = 0.8 * prob.x_max[nq:]                     # safe set: the velocity at the tested node raised
    return x, u


def _statement(par, prob, oracle, x, u, safe_node, coll_first):
    """worst [B, 5], flags [B] and the distance of every instance's values from their thresholds, from the oracle and numpy"""
    B, N, nq, nr = x.shape[0], prob.N, prob.nq, prob.desc.n_rows
    _, _, p = constant_guess(prob, x[:, 0], alpha=par.alpha)
    ev = oracle.eval_nodes(x, u, p)
    w = np.full((B, 5), NEG_INF)
    w[:, 0] = np.maximum(prob.x_min - x, x - prob.x_max).reshape(B, -1).max(1)
    if nr:
        rv = ev['row_val'][:, :1 if coll_first else N + 1, :nr]
        w[:, 1] = np.maximum(prob.row_check[:, 0] - rv, rv - prob.row_check[:, 1]).reshape(B, -1).max(1)
    tau = ev['tau'][:, :N, :nq]
    w[:, 2] = np.maximum(prob.tau_min - tau, tau - prob.tau_max).reshape(B, -1).max(1)
    w[:, 3] = np.linalg.norm((x - oracle.guess_correction(x, u)).reshape(B, -1), axis=1)
    thr = np.array([par.tol_x, 0.0, par.tol_tau, par.tol_dyn * np.sqrt(N + 1), par.tol_safe_set])
    flags = (~(w[:, 0] <= thr[0])) * 1 + (~(w[:, 1] <= thr[1])) * 2 + (~(w[:, 2] <= thr[2])) * 4 + (~(w[:, 3] < thr[3])) * 8
    if safe_node is not None:
        g = ev['nn_val'][:, safe_node]
        w[:, 4] = -g
        flags = flags + (~((g >= -thr[4]) & (g <= 1e6 + thr[4]))) * 16
    dist = np.abs(w - thr)
    dist[~np.isfinite(w)] = np.inf
    return w, flags.astype(np.int32), dist


def _close(got, ref, tol):
    same_inf = np.isinf(ref) & (got == ref)
    with np.errstate(invalid='ignore'):
        return np.all(same_inf | (np.abs(got - ref) <= tol * (1.0 + np.abs(ref))))


@pytest.mark.parametrize('case', CASES)
def test_check_guess_matches_the_oracle_statement(case):
    """flags equal for every instance, worst[:, 0:4] within 1e-9 (1 + |.|), worst[:, 4] within 2e-5 (1 + |.|), with
    collision_first_node 1 and 0; every bit the case has is set somewhere and clear somewhere; no instance within 1e-7 of a threshold
    (1e-3 for the safe set) on the oracle side.  Then: masked-out rows keep a sentinel, two calls give the same bits, torch device
    pointers give the bits of numpy, a NaN in u sets bits 2 and 3."""
    import torch
    from oracle.oracle import Oracle
    from safe_mpc_amd.solver import BatchedOcpSolver
    par, prob, net, safe_node = _case_problem(case)
    oracle = Oracle(prob, (net.weights, net.biases))
    s = BatchedOcpSolver(prob, net)
    x, u = _case_trajectories(par, prob, oracle, safe_node)
    B = x.shape[0]
    have = [0, 2, 3] + ([1] if prob.desc.n_rows else []) + ([4] if safe_node is not None else [])
    seen_set, seen_clear = np.zeros(5, bool), np.zeros(5, bool)
    results = {}
    for coll_first in (1, 0):
        w_ref, f_ref, dist = _statement(par, prob, oracle, x, u, safe_node, coll_first)
        assert np.all(dist[:, :4] > 1e-7) and np.all(dist[:, 4] > 1e-3), dist.min(0)
        flags, worst = s.check_guess(x, u, safe_node=safe_node, collision_first_node=coll_first)
        print(case, 'first node only' if coll_first else 'every node', 'flags', flags.tolist(), 'oracle', f_ref.tolist())
        with np.errstate(invalid='ignore'):
            print('  worst error', np.nanmax(np.where(np.isinf(w_ref), 0.0, np.abs(worst - w_ref) / (1.0 + np.abs(w_ref))), axis=0))
        assert np.array_equal(flags, f_ref)
        assert _close(worst[:, :4], w_ref[:, :4], 1e-9)
        assert _close(worst[:, 4], w_ref[:, 4], 2e-5)
        for i in have:
            seen_set[i] |= bool(((f_ref >> i) & 1).any())
            seen_clear[i] |= bool((((f_ref >> i) & 1) == 0).any())
        results[coll_first] = (flags, worst)
    assert seen_set[have].all() and seen_clear[have].all(), (seen_set, seen_clear)
    if safe_node is None:
        assert np.all(results[1][1][:, 4] == NEG_INF) and not (results[1][0] & 16).any()
    if prob.desc.n_rows:            # the quirk: the instance whose LATER node collides passes the first-node test only
        assert (results[1][0][3] & 2) == 0 and (results[0][0][3] & 2) == 2
    flags, worst = results[1]
    # the same bits twice; masked-out rows keep what was there
    f2, w2 = s.check_guess(x, u, safe_node=safe_node, collision_first_node=1)
    assert np.array_equal(f2, flags) and np.array_equal(w2, worst)
    mask = np.array([1, 0, 1, 1, 0, 1, 0], np.uint8)
    fm, wm = np.full(B, -7, np.int32), np.full((B, 5), -7.5)
    s.check_guess(x, u, safe_node=safe_node, collision_first_node=1, mask=mask, flags=fm, worst=wm)
    assert np.all(fm[mask == 0] == -7) and np.all(wm[mask == 0] == -7.5)
    assert np.array_equal(fm[mask != 0], flags[mask != 0]) and np.array_equal(wm[mask != 0], worst[mask != 0])
    # device pointers
    dev = torch.device('cuda', s.device)
    fd, wd = s.check_guess(torch.tensor(x, device=dev), torch.tensor(u, device=dev), safe_node=safe_node, collision_first_node=1,
                           mask=torch.tensor(mask, device=dev), flags=torch.full((B,), -7, dtype=torch.int32, device=dev),
                           worst=torch.full((B, 5), -7.5, dtype=torch.float64, device=dev))
    s.sync()
    assert np.array_equal(fd.cpu().numpy(), fm) and np.array_equal(wd.cpu().numpy(), wm)
    # a NaN in u fails the torque and the dynamics test
    un = u.copy()
    un[0, 0, 0] = np.nan
    fn, wn = s.check_guess(x, un, safe_node=safe_node, collision_first_node=1)
    assert (fn[0] & 12) == 12 and np.isnan(wn[0, 2]) and np.isnan(wn[0, 3])
    assert np.array_equal(fn[1:], flags[1:]) and np.array_equal(wn[1:], worst[1:])


def test_check_guess_refuses_bad_safe_nodes():
    from safe_mpc_amd._lib import EngineError
    from safe_mpc_amd.solver import BatchedOcpSolver
    par, prob, net = make_problem('htwa', N=4)
    x, u = np.zeros((2, 5, prob.nx)), np.zeros((2, 4, prob.nu))
    with pytest.raises(EngineError, match='safe_node'):
        BatchedOcpSolver(prob, net).check_guess(x, u, safe_node=5)
    with pytest.raises(EngineError, match='smpc_set_mlp'):
        BatchedOcpSolver(prob, None).check_guess(x, u, safe_node=4)


# ---- 2. the kernel against the shipped checkGuess -----------------------------------------------------------------------------------
def _guess_par():
    from safe_mpc_amd.parser import Parameters
    par = Parameters({}, 'z1')
    par.nq, par.n_dof_safe_set, par.net_size, par.N, par.nlp_max_iter = 6, 6, [12, 256, 1], 20, 200
    return par


def _pinned(par):
    """make_controller with the QP form pinned, so that a result does not depend on the batch size a controller was made for"""
    from safe_mpc_amd import controller as C

    def make(name, batch):
        ctrl = C.get_controller(name, par, batch)
        ctrl.ocp_solver.set_qp_mode('throughput')
        return ctrl
    return make


def _free_starts(ctrl, n):
    """the first n samples of generate_guess' stream: Halton starts at rest that pass the collision filter"""
    from safe_mpc_amd.closed_loop import halton as cl_halton
    pr, nq = ctrl.problem, ctrl.problem.nq
    q = pr.x_min[:nq] + cl_halton(4 * n + 16, nq) * (pr.x_max[:nq] - pr.x_min[:nq])
    x_all = np.hstack([q, np.zeros_like(q)])
    free = np.asarray(ctrl.ocp_solver.check_trajectory(x_all[:, None, :], tol_x=0.0))
    x0 = x_all[free][:n]
    assert len(x0) == n
    return x0


def test_check_guess_agrees_with_checkGuess():
    """On the 48-start problem of test_sqp_gpu (htwa, N = 20), after 50 and after 200 device iterations: flags == 0 equals
    ctrl.checkGuess() except for undecidable instances -- one of whose worst values is within 1e-9 (1 + |threshold|) of its threshold
    (2e-5 for the safe set); at most 2 of 48.  Both verdicts occur at 50 iterations."""
    par = _guess_par()
    ctrl = _pinned(par)('htwa', 48)
    s, N = ctrl.ocp_solver, ctrl.N
    x0 = _free_starts(ctrl, 48)
    xg, ug = np.repeat(x0[:, None, :], N + 1, axis=1), np.zeros((48, N, ctrl.nu))
    ctrl.p[:, :, 3] = par.alpha
    thr = np.array([par.tol_x, 0.0, par.tol_tau, par.tol_dyn * np.sqrt(N + 1), par.tol_safe_set])
    band = np.array([1e-9, 1e-9, 1e-9, 1e-9, 2e-5]) * (1.0 + np.abs(thr))
    state = None
    for upto, more in ((50, 50), (200, 150)):
        xg, ug, state = s.sqp(x0, xg, ug, ctrl.p, dict(max_iter=more), state)
        ctrl.x_temp, ctrl.u_temp = xg.copy(), ug.copy()
        ref = np.asarray(ctrl.checkGuess()).astype(bool)
        flags, worst = ctrl.guess_report()
        undecidable = (np.abs(worst - thr) <= band).any(1)
        print('after', upto, 'iterations: accepted', int(ref.sum()), 'kernel', int((flags == 0).sum()), 'undecidable',
              int(undecidable.sum()), 'closest', np.abs(worst - thr).min(0))
        assert undecidable.sum() <= 2
        assert np.array_equal((flags == 0)[~undecidable], ref[~undecidable])
        if upto == 50:
            assert ref.any() and not ref.all()


# ---- 3. the loop equals the per-sample statement ------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def first_statement():
    """One batch of the first 64 free samples advanced by solver.sqp(max_iter=50) four times, check_guess after each call: each
    sample's fate under accept='first' (the first round with status == 0 and flags == 0), and its iterate at that round."""
    par = _guess_par()
    ctrl = _pinned(par)('htwa', 64)
    s, N = ctrl.ocp_solver, ctrl.N
    x0 = _free_starts(ctrl, 64)
    xg, ug = np.repeat(x0[:, None, :], N + 1, axis=1), np.zeros((64, N, ctrl.nu))
    ctrl.p[:, :, 3] = par.alpha
    state = None
    fate = np.zeros(64, int)                 # 0 open, 1 accepted, -1 failed
    at = {}
    for rnd in range(4):
        xg, ug, state = s.sqp(x0, xg, ug, ctrl.p, dict(max_iter=50), state)
        flags, _ = s.check_guess(xg, ug, safe_node=N)
        ok = (state['status'] == 0) & (flags == 0)
        ended = (state['done'] != 0) | (rnd == 3)
        for j in np.where(fate == 0)[0]:
            if ok[j]:
                fate[j], at[j] = 1, (xg[j].copy(), ug[j].copy())
            elif ended[j]:
                fate[j] = -1
    return par, fate, at


@pytest.mark.parametrize('batch', [8, 24, 64])
def test_generate_guess_until_equals_the_statement(first_statement, batch):
    """accept='first', nlp_max_iter = 200, check_every = 50, n = 24: the statement's first 24 accepted samples, bit for bit, for
    every batch; info lists the same failed samples."""
    from safe_mpc_amd import closed_loop as cl
    par, fate, at = first_statement
    n = 24
    accepted = np.where(fate == 1)[0]
    assert len(accepted) >= n, f'the statement accepts {len(accepted)} of 64 samples'
    want = accepted[:n]
    g, info = cl.generate_guess_until(par, 'htwa', n, batch=batch, check_every=50, accept='first', make_controller=_pinned(par))
    print('batch', batch, 'issued', info['issued'], 'rounds', info['rounds'], 'instance-iterations', info['instance_iterations'],
          'failed', info['failed'])
    assert info['accepted'] == want.tolist() and not info['exhausted']
    assert info['issued'] == want[-1] + 1
    assert info['failed'] == [j for j in range(want[-1] + 1) if fate[j] == -1]
    assert g['xg'].shape == (n, par.N + 1, 12) and g['ug'].shape == (n, par.N, 6)
    assert np.array_equal(g['xg'], np.stack([at[j][0] for j in want]))
    assert np.array_equal(g['ug'], np.stack([at[j][1] for j in want]))
    assert info['instance_iterations'] == sum(info['iters'].values())


# ---- 4. 'final' equals today's path, 5. max_samples ------------------------------------------------------------------------------
def test_generate_guess_until_final_equals_generate_guess():
    """accept='final' with check_every = nlp_max_iter = 200 and n = the accepted count of generate_guess(on_device=True) on 48
    starts: identical guesses, bit for bit; a fresh controller's checkGuess accepts all of them."""
    from safe_mpc_amd import closed_loop as cl
    par = _guess_par()
    mk = _pinned(par)
    g0, good = cl.generate_guess(par, 'htwa', 48, make_controller=mk, on_device=True)
    n = int(good.sum())
    assert n >= 24
    g1, info = cl.generate_guess_until(par, 'htwa', n, check_every=200, accept='final', make_controller=mk)
    print('accepted', n, 'issued', info['issued'], 'rounds', info['rounds'])
    assert info['accepted'] == np.where(good)[0].tolist() and info['failed'] == np.where(~good)[0][:len(info['failed'])].tolist()
    assert np.array_equal(g1['xg'], g0['xg']) and np.array_equal(g1['ug'], g0['ug'])
    ctrl = mk('htwa', n)
    ctrl.x_temp, ctrl.u_temp = g1['xg'].copy(), g1['ug'].copy()
    assert np.all(ctrl.checkGuess())


def test_generate_guess_until_max_samples():
    from safe_mpc_amd import closed_loop as cl
    par = _guess_par()
    g, info = cl.generate_guess_until(par, 'htwa', 24, batch=8, check_every=50, accept='first', max_samples=10,
                                      make_controller=_pinned(par))
    assert info['issued'] == 10 and info['exhausted'] and len(info['accepted']) + len(info['failed']) == 10
    assert len(info['accepted']) < 24 and g['xg'].shape[0] == len(info['accepted']) == g['ug'].shape[0]
