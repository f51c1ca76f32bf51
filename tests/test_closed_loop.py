"""scripts/mpc.py / guess_acados.py semantics through the CPU test double."""
import numpy as np

from conftest import make_problem
from fake_solver import OracleSolver
from safe_mpc_amd import closed_loop as cl
from safe_mpc_amd import controller as C


def _factories(par, N, hidden=256):
    def make_controller(name, batch):
        cls = C.CONTROLLERS[name]
        ctrl = cls.__new__(cls)
        prob = C.OcpProblem(par, cls.cont_name, 'ext', N=N)
        net = C.SafeSetNet.from_params(par, prob.x_min, prob.x_max)
        prob.set_normalisation(net.mean, net.std)
        C.AbstractController.__init__(ctrl, par, batch, 'ext', N, solver=OracleSolver(prob, net), net=net)
        return ctrl

    def make_backup(batch):
        ctrl = C.SafeBackupController.__new__(C.SafeBackupController)
        prob = C.OcpProblem(par, 'backup', 'zero', N=par.back_hor)
        net = C.SafeSetNet.from_params(par, prob.x_min, prob.x_max)
        C.AbstractController.__init__(ctrl, par, batch, 'zero', par.back_hor, solver=OracleSolver(prob, net), net=net)
        return ctrl
    return make_controller, make_backup


def test_generate_guess_then_run_mpc():
    par, prob, net = make_problem('naive', N=8)
    par.back_hor, par.nlp_max_iter, par.n_steps = 10, 120, 12
    par.levenberg_marquardt = 1e-3           # the default 0.5 makes full-step SQP crawl (config.yaml:21 comment)
    mk, mkb = _factories(par, 8)
    guess, good = cl.generate_guess(par, 'naive', 6, make_controller=mk, sqp_tol=1e-5)
    assert guess['xg'].shape[1:] == (9, 12) and guess['ug'].shape[1:] == (8, 6)
    n = guess['xg'].shape[0]
    assert n >= 1
    res = cl.run_mpc(par, 'naive', guess['xg'], guess['ug'], make_controller=mk, make_backup=mkb, n_steps=12)
    assert res['x'].shape == (n, 13, 12) and res['u'].shape == (n, 12, 6)
    idx = set(res['conv_idx']) | set(res['collisions_idx']) | set(res['unconv_idx']) | set(res['viable_idx'])
    assert idx == set(range(n))                                  # the taxonomy partitions the instances
    for i in res['collisions_idx']:
        assert np.isnan(res['x'][i, -1]).any()                   # broken runs are NaN-padded (mpc.py:114)
    for i in set(range(n)) - set(res['collisions_idx']):
        assert np.all(np.isfinite(res['x'][i]))


def test_model_noise_tables_and_file_names():
    par, prob, net = make_problem('st', N=8)
    jt = cl.perturbed_joint_tables(par, 6, 10.0, [0, 1, 1])
    base = prob.joint_table()
    assert jt.shape == (3, 6)
    assert np.array_equal(jt[1]['mass'], jt[2]['mass'])           # same seed, same plant
    rel = np.abs(jt[0]['mass'] / base['mass'] - 1)
    assert np.all(rel <= 0.10 + 1e-12) and rel.max() > 1e-3
    assert np.array_equal(jt[0]['axis'], base['axis']) and np.array_equal(jt[0]['p0'], base['p0'])
    zero = cl.perturbed_joint_tables(par, 6, 0.0, [5])
    assert np.allclose(zero[0]['mass'], base['mass']) and np.allclose(zero[0]['inertia'], base['inertia'])
    # the batched generator (BASELINE config 2's 65 536 plants) against the per-seed statement: the draws to the bit (mass and centre
    # of mass are sums and quotients of drawn values only), the lumped inertias to rounding (BLAS matmuls there, written-out sums here)
    for quirks in (True, False):
        par.reference_quirks = quirks
        seeds = np.arange(64) * 1021 + 3
        a, b = cl.perturbed_joint_tables(par, 6, 10.0, seeds), cl.perturbed_joint_tables_batched(par, 6, 10.0, seeds)
        for fld in a.dtype.names:
            if fld == 'inertia':
                assert np.abs(a[fld] - b[fld]).max() <= 1e-15 * np.abs(a[fld]).max()
            else:
                assert np.array_equal(a[fld], b[fld]), fld
    par.reference_quirks = True
    assert np.array_equal(cl.perturbed_joint_tables_batched(par, 6, 10.0, [7])[0]['mass'], cl.perturbed_joint_tables_batched(par, 6, 10.0, np.arange(16))[7]['mass'])
    f = cl.guess_file(par, 'z1', 'st', 30, True)
    assert f.endswith('z1_st_30hor_10sm_use_netTrue__q_collision_margins_0.0_0.0_guess.pkl')
    g = cl.result_file(par, 'z1', 'st', 30, True, 5.0, 1.0, 0.0, 0.0)
    assert g.endswith('z1_st_use_netTrue_30hor_10sm_noise_5.0_control_noise1.0_q_collision_margins_0.0_0.0_mpc.pkl')


def test_masked_step_leaves_inactive_rows_untouched():
    par, prob, net = make_problem('htwa', N=6)
    mk, _ = _factories(par, 6)
    c = mk('htwa', 3)
    x0 = np.tile(np.concatenate([0.5 * (prob.lbx[:6] + prob.ubx[:6]), np.zeros(6)]), (3, 1))
    c.setGuess(np.repeat(x0[:, None, :], 7, 1), np.zeros((3, 6, 6)))
    before = (c.x_guess.copy(), c.fails.copy(), c.current_step.copy())
    u, ab = cl._masked_step(c, x0, np.array([True, False, True]))
    assert np.array_equal(c.x_guess[1], before[0][1]) and c.current_step.tolist() == [1, 0, 1]
    assert not ab[1]


def _merit_sqp_checks(mk, par, cont, n):
    hist = []
    guess, good = cl.generate_guess(par, cont, n, make_controller=mk, sqp_tol=1e-6, history=hist)
    assert good.sum() >= 1 and len(hist) >= 2
    # the l1 merit never increases along the accepted steps (Armijo, parser.py:139 MERIT_BACKTRACKING): compared at equal mu
    for h in hist:
        up = h['updated'] & (h['alpha'] > 0.05)
        assert np.all(h['merit'][up] <= h['merit_before'][up] + 1e-9 * (1 + np.abs(h['merit_before'][up])))
    assert max(h['alpha'].max() for h in hist) == 1.0                 # full steps are taken when they are good ...
    viol_end = hist[-1]['violation']
    assert np.all(viol_end[good] < 1e-5)                              # ... and the accepted guesses are feasible
    return guess, good, hist


def test_generate_guess_merit_backtracking_on_oracle_double():
    """guess_acados.py:98-158 with parser.py:139 MERIT_BACKTRACKING: merit decrease, feasibility of accepted guesses, and a
    start far from feasibility (default LM 0.5, aggressive reference) where the step length actually has to be cut."""
    par, prob, net = make_problem('naive', N=8)
    par.nlp_max_iter = 150
    par.levenberg_marquardt = 1e-3
    mk, _ = _factories(par, 8)
    guess, good, hist = _merit_sqp_checks(mk, par, 'naive', 6)
    # guesses pass the reference's acceptance test (checkGuess: state, torque, dynamics) by construction of `good`
    assert guess['xg'].shape[0] == good.sum()
    # NLS cost + terminal zero velocity (the OCP guess_acados.py builds for naive / zerovel warm starts)
    par2, prob2, net2 = make_problem('zerovel', 'nls', N=8)
    par2.nlp_max_iter, par2.levenberg_marquardt = 150, 1e-3

    def mk2(name, batch):
        cls = C.CONTROLLERS[name]
        ctrl = cls.__new__(cls)
        prob = C.OcpProblem(par2, cls.cont_name, 'nls', N=8)
        net = C.SafeSetNet.from_params(par2, prob.x_min, prob.x_max)
        prob.set_normalisation(net.mean, net.std)
        C.AbstractController.__init__(ctrl, par2, batch, 'nls', 8, solver=OracleSolver(prob, net), net=net)
        return ctrl
    _merit_sqp_checks(mk2, par2, 'zerovel', 4)


def test_real_receding_closed_loop_same_outcomes_with_and_without_stall_exit():
    """the stall exit (qp_stall_iters = 24, RealReceding's default) must only shorten solves that fail anyway.  The
    same closed loop with the exit off and on: identical statuses at every step (so identical accept / reject / abort
    decisions, hence trajectories), the failed solves of the 'on' run are the failed solves of the 'off' run, and none of
    the 'on' run's failures is an iterate that met the exit test (those report success)."""
    from conftest import sample_instances
    N, B, steps = 30, 48, 16
    logs = {}
    for stall in (0, 24):
        par, prob, net = make_problem('real_receding', N=N, qp_stall_iters=stall)
        par.back_hor = 30
        assert prob.desc.qp_stall_iters == stall
        log = []

        class Logging(OracleSolver):
            def solve(self, x0, xg, ug, p, out=None):
                r = super().solve(x0, xg, ug, p, out)
                log.append((np.asarray(r[2]).copy(), np.asarray(r[3]).copy(), np.asarray(r[1][:, 0]).copy()))
                return r

        def mk(name, batch, par=par):
            cls = C.CONTROLLERS[name]
            ctrl = cls.__new__(cls)
            pr = C.OcpProblem(par, cls.cont_name, 'ext', N=N)
            nt = C.SafeSetNet.from_params(par, pr.x_min, pr.x_max)
            pr.set_normalisation(nt.mean, nt.std)
            C.AbstractController.__init__(ctrl, par, batch, 'ext', N, solver=Logging(pr, nt), net=nt)
            return ctrl
        _, mkb = _factories(par, N)
        x0 = sample_instances(prob, B, seed=0)
        res = cl.run_mpc(par, 'real_receding', np.repeat(x0[:, None, :], N + 1, axis=1), np.zeros((B, N, 6)), make_controller=mk,
                         make_backup=mkb, n_steps=steps)
        logs[stall] = (log, res)
    (l0, r0), (l1, r1) = logs[0], logs[24]
    assert len(l0) == len(l1)
    n_fail = 0
    for (s0, i0, u0), (s1, i1, u1) in zip(l0, l1):
        assert np.array_equal(s0, s1)                     # same verdict for every solve
        ok = s0 == 0
        assert np.array_equal(i0[ok], i1[ok]) and np.array_equal(u0[ok], u1[ok])      # successful solves: bit-identical
        assert np.all(i1[~ok] <= i0[~ok])                 # failing ones only get shorter
        n_fail += int((~ok).sum())
    assert n_fail > 0, 'the fixture is meant to contain infeasible tubes'
    for key in ('conv_idx', 'collisions_idx', 'viable_idx', 'unconv_idx'):
        assert r0[key] == r1[key]
    assert np.array_equal(np.nan_to_num(r0['x']), np.nan_to_num(r1['x']))


def test_run_mpc_collects_solver_times_like_the_reference():
    """scripts/mpc.py:239,300-303: one row of the seven acados timers per step, and their 99 % quantiles"""
    par, prob, net = make_problem('st', N=8)
    par.back_hor = 10
    mk, mkb = _factories(par, 8)
    from conftest import sample_instances
    x0 = sample_instances(prob, 4, seed=1)
    res = cl.run_mpc(par, 'st', np.repeat(x0[:, None, :], 9, axis=1), np.zeros((4, 8, 6)), make_controller=mk, make_backup=mkb,
                     n_steps=6, collect_times=True)
    ts = res['time_stats']
    assert res['time_fields'] == ['time_lin', 'time_sim', 'time_qp', 'time_qp_solver_call', 'time_glob', 'time_reg', 'time_tot']
    assert ts.shape == (6, 7) and res['time_lost'] == 0
    assert np.all(ts[:, 6] > 0) and np.all(ts[:, 6] >= ts[:, 2]) and np.all(ts[:, 2] >= ts[:, 3])
    assert np.allclose(res['time_q99'], np.quantile(ts, 0.99, axis=0))
    ref = cl.run_mpc(par, 'st', np.repeat(x0[:, None, :], 9, axis=1), np.zeros((4, 8, 6)), make_controller=mk, make_backup=mkb, n_steps=6)
    assert 'time_stats' not in ref and np.array_equal(ref['x'], res['x'])      # collecting times changes nothing else


def test_event_ring_reader_never_loses_or_duplicates_a_solve():
    """closed_loop._DeviceGroup._read_times against a simulated 64-deep event ring (smpc_get_timing_history): solves finish a varying
    number of steps after they were enqueued; the reader takes entries at least 32 solves old, waits (sync) rather than letting the
    ring lap an unread entry, and drains the rest at the end -- every solve's row exactly once, in order."""
    class Ring:
        """solve j becomes readable once `done` > j; back = number of solves since"""
        def __init__(self):
            self.enq, self.done, self.syncs = 0, 0, 0

        def timing_history(self, back):
            j = self.enq - 1 - back
            if back >= 64 or j < 0 or j >= self.done:
                return None
            return {'time_lin': 1e-3 * j, 'time_nn': 0.0, 'time_qp_setup': 0.0, 'time_qp_ipm': 2e-3, 'time_tot': 1.0 + j}

        def sync(self):
            self.syncs += 1
            self.done = self.enq

    for lag in (0, 5, 40, 100):                      # how far the GPU trails the host's enqueueing
        ring = Ring()
        g = cl._DeviceGroup.__new__(cl._DeviceGroup)
        g._ctrl = type('C', (), {'ocp_solver': ring})()
        g._time_rows, g._time_next, g._time_lost = [], 0, 0
        n = 150
        for j in range(n):
            ring.enq = j + 1
            ring.done = max(ring.done, j + 1 - lag)
            g._read_times(j)
        g._read_times(n - 1, final=True)
        rows = np.array(g._time_rows)
        assert g._time_lost == 0 and rows.shape == (n, 7), (lag, g._time_lost, rows.shape)
        assert np.array_equal(rows[:, 6], 1.0 + np.arange(n))          # every solve once, in order
        if lag <= 5:
            assert ring.syncs == 1                                      # only the final drain waits
