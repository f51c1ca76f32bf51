"""Parity of the HIP engine (through the C ABI) with the CPU oracle on identical seeded inputs.  -m gpu only.

Tolerances (FP64 paths are compared tightly; rows that pass through the fp32 network inherit its rounding):
  linearisation pieces ...... 1e-9 relative to the field's scale
  fp32 MLP value / gradient . 2e-5 relative
  RTI solution without NN ... 1e-6 * (1 + |u|_inf)  (two IPMs converging to one QP solution from rounding-different paths)
  RTI solution with NN ...... 1e-4 * (1 + |u|_inf)
  terminal q_dot = 0 ........ 2e-5 * (1 + |u|_inf)  (zerovel pins the velocity with lb == ub: the two barrier terms of
                              a zero-width box make the last Newton systems ill-conditioned)
  backup OCP ................ 5e-4 * (1 + |u|_inf)  (zero cost: the only curvature is the 1e-4 regularisation, so the
                              minimiser is resolved to about sqrt(tol_ipm / 1e-4) only -- a feasibility problem)
"""
import numpy as np
import pytest

from conftest import constant_guess, make_problem, sample_instances

pytestmark = pytest.mark.gpu


_QP_MODE = [None]      # None: the engine's own choice by batch size; 'throughput' / 'latency': forced (fixture qp_mode)


def _solver(prob, net):
    from safe_mpc_amd.solver import BatchedOcpSolver
    s = BatchedOcpSolver(prob, net)
    if _QP_MODE[0] is not None:
        s.set_qp_mode(_QP_MODE[0])
    return s


@pytest.fixture(params=['throughput', 'latency'])
def qp_mode(request):
    """Both forms of the interior-point solve (smpc_set_qp_mode): k_qp_ipm, a wavefront per two instances, and k_qp_ipm_wg, a
    workgroup per instance.  Tests that take this fixture run once with each; the others run with the engine's own choice."""
    _QP_MODE[0] = request.param
    yield request.param
    _QP_MODE[0] = None


def _oracle(prob, net):
    from oracle.oracle import Oracle
    return Oracle(prob, (net.weights, net.biases))


def _rel(a, b):
    return np.abs(a - b).max() / (1e-12 + np.abs(b).max())


@pytest.mark.parametrize('controller,cost', [('naive', 'ext'), ('constraint_everywhere', 'nls')])
def test_eval_nodes_parity(controller, cost):
    par, prob, net = make_problem(controller, cost, N=12)
    s, o = _solver(prob, net), _oracle(prob, net)
    x0 = sample_instances(prob, 24, seed=1, vel_scale=0.5)
    xg, ug, p = constant_guess(prob, x0)
    rng = np.random.default_rng(0)
    xg[:, 1:] += 0.05 * rng.standard_normal(xg[:, 1:].shape)
    ug += rng.uniform(-5, 5, ug.shape)
    a, b = s.eval_nodes(xg, ug, p), o.eval_nodes(xg, ug, p)
    nq = 6
    for f, n in [('tau', nq), ('M', 36), ('dtau_dq', 36), ('dtau_dv', 36), ('ee', 3), ('cost_grad_q', nq),
                 ('cost_hess_qq', 36), ('row_val', 6), ('row_grad', 36)]:
        assert _rel(a[f][..., :n], b[f][..., :n]) < 1e-9, f
    if controller != 'naive':
        assert _rel(a['nn_val'], b['nn_val']) < 2e-5
        assert _rel(a['nn_grad'][..., :12], b['nn_grad'][..., :12]) < 2e-4
        assert np.all(a['nn_val'][:, 0] == 0)        # node 0 never carries the row


@pytest.mark.parametrize('controller,cost,N,tol', [('naive', 'ext', 30, 1e-6), ('zerovel', 'nls', 20, 2e-5),
                                                   ('st', 'ext', 30, 1e-4), ('htwa', 'ext', 15, 1e-4),
                                                   ('constraint_everywhere', 'ext', 10, 1e-4),
                                                   ('receding', 'ext', 12, 1e-4), ('backup', 'ext', 25, 5e-4)])
def test_rti_solve_parity(controller, cost, N, tol, qp_mode):
    par, prob, net = make_problem(controller, cost, N=N)
    s, o = _solver(prob, net), _oracle(prob, net)
    B = 32
    x0 = sample_instances(prob, B, seed=2, vel_scale=0.1)
    xg, ug, p = constant_guess(prob, x0)
    if controller == 'receding':
        p[:, 1:N, 4] = -1.0
        p[np.arange(B), 1 + np.arange(B) % (N - 1), 4] = 1.0      # one switched-on running node per instance
    xa, ua, sa, ia = s.solve(x0, xg, ug, p)
    xb, ub, sb, ib = o.solve_batch(x0, xg, ug, p)
    assert np.array_equal(sa, sb)
    ok = sb == 0
    assert ok.sum() >= B - 2
    assert np.abs(ia[ok] - ib[ok]).max() <= 2
    scale = 1 + np.abs(ub[ok]).max()
    assert np.abs(ua[ok] - ub[ok]).max() < tol * scale
    assert np.abs(xa[ok] - xb[ok]).max() < max(tol, 1e-6)
    # second step from the shifted solution with a perturbed measured state (x0 != x_guess[0])
    xg2, ug2, _ = o.provide_control(np.ones(B, np.int32), xb, ub, xg, ug)
    xg2 = o.guess_correction(xg2, ug2)
    x1 = xg2[:, 0] + 1e-3 * np.random.default_rng(1).standard_normal((B, 12))
    xa, ua, sa, ia = s.solve(x1, xg2, ug2, p)
    xb, ub, sb, ib = o.solve_batch(x1, xg2, ug2, p)
    assert np.array_equal(sa, sb)
    ok = sb == 0
    assert np.abs(ua[ok] - ub[ok]).max() < tol * (1 + np.abs(ub[ok]).max())


def test_callers_parity():
    par, prob, net = make_problem('st', N=10)
    s, o = _solver(prob, net), _oracle(prob, net)
    B = 16
    rng = np.random.default_rng(3)
    x0 = sample_instances(prob, B, seed=3, vel_scale=0.3)
    xg, ug, p = constant_guess(prob, x0)
    ug += rng.uniform(-3, 3, ug.shape)
    assert np.allclose(s.guess_correction(xg, ug), o.guess_correction(xg, ug), atol=1e-13)
    xt, ut = xg + 0.1, ug - 0.2
    acc = (np.arange(B) % 2).astype(np.int32)
    a, b = s.provide_control(acc, xt, ut, xg, ug), o.provide_control(acc, xt, ut, xg, ug)
    for u, v in zip(a, b):
        assert np.array_equal(u, v)
    # feasibility predicates on a trajectory that leaves the box for some instances
    traj = o.guess_correction(xg, ug)
    traj[::4, 5, 2] += 10.0                                  # out of the joint box
    q_hit = None                                             # a configuration the collision rows reject
    for q in rng.uniform(prob.lbx[:6], prob.ubx[:6], (4000, 6)):
        xq = np.concatenate([q, np.zeros(6)])[None, None]
        if not o.check_trajectory(xq, prob.x_min, prob.x_max, par.tol_x, prob.row_check[:, 0], prob.row_check[:, 1])[0]:
            q_hit = q
            break
    assert q_hit is not None
    traj[1, 7, :6] = q_hit
    ok_a, nn_a = s.check_trajectory(traj, want_nn=True)
    ok_b, nn_b = o.check_trajectory(traj, prob.x_min, prob.x_max, par.tol_x, prob.row_check[:, 0], prob.row_check[:, 1],
                                    par.alpha, par.tol_safe_set, want_nn=True)
    assert np.array_equal(ok_a, ok_b) and 0 < ok_b.sum() < B
    assert (nn_a != nn_b).mean() < 0.01
    # plant step, nominal and with perturbed inertias + torque noise
    u = rng.uniform(-10, 10, (B, 6))
    xa, ea = s.plant_step(x0, u)
    xb, eb = o.plant_step(x0, u)
    assert np.allclose(xa, xb, atol=1e-10) and np.allclose(ea, eb, atol=1e-8)
    jt = np.tile(prob.joint_table(), (B, 1))
    jt['mass'] *= 1 + 0.1 * rng.uniform(-1, 1, jt['mass'].shape)
    jt['com'] *= 1 + 0.1 * rng.uniform(-1, 1, jt['com'].shape)
    tn = rng.normal(0, 0.5, (B, 6))
    xa, ea = s.plant_step(x0, u * 5, jt, tn)
    xb, eb = o.plant_step(x0, u * 5, jt, tn)
    assert np.allclose(xa, xb, atol=1e-10) and np.allclose(ea, eb, atol=1e-7)


def test_full_size_properties():
    """BASELINE config 1 size (B=4096, N=30, 'st'): properties that need no oracle run."""
    par, prob, net = make_problem('st', N=30)
    s = _solver(prob, net)
    B = 4096
    x0 = sample_instances(prob, B, seed=4)
    xg, ug, p = constant_guess(prob, x0)
    x, u, st, it = s.solve(x0, xg, ug, p)
    assert (st == 0).mean() > 0.99
    ok = st == 0
    assert np.allclose(x[:, 0], x0, atol=1e-12)
    dt = par.dt
    assert np.allclose(x[ok, 1:, :6], x[ok, :-1, :6] + dt * x[ok, :-1, 6:] + 0.5 * dt * dt * u[ok], atol=1e-9)
    assert np.allclose(x[ok, 1:, 6:], x[ok, :-1, 6:] + dt * u[ok], atol=1e-9)
    assert np.all(x[ok, 1:] >= prob.lbx - 1e-6) and np.all(x[ok, 1:] <= prob.ubx + 1e-6)
    # determinism and batch-independence.  The engine picks the FORM of the QP solve by batch size (smpc_set_qp_mode: k_qp_ipm for
    # 4096 instances, k_qp_ipm_wg for 100), and the two agree to rounding, not to the bit: with the form fixed a sub-batch gives
    # bit-identical results in either form; with the engine's own choice it stays inside the kernels' mutual tolerance
    # (test_qp_kernels_agree)
    x2, u2, st2, it2 = s.solve(x0[:100], xg[:100], ug[:100], p[:100])
    assert np.array_equal(st2, st[:100]) and np.abs(it2.astype(int) - it[:100].astype(int)).max() <= 1
    same = it2 == it[:100]
    assert np.abs(u2[same] - u[:100][same]).max() < 1e-7 * (1 + np.abs(u).max())
    s.set_qp_mode('throughput')
    x3, u3, st3, it3 = s.solve(x0[:100], xg[:100], ug[:100], p[:100])
    assert np.array_equal(x3, x[:100]) and np.array_equal(u3, u[:100]) and np.array_equal(it3, it[:100])
    s.set_qp_mode('latency')
    x4, u4, st4, it4 = s.solve(x0[:300], xg[:300], ug[:300], p[:300])          # (300: the 4-half-wave workgroups; 100: the 8-half-wave ones)
    assert np.array_equal(x2, x4[:100]) and np.array_equal(u2, u4[:100]) and np.array_equal(it2, it4[:100])
    s.set_qp_mode('auto')
    # spot parity against the oracle on a slice
    from oracle.oracle import Oracle
    o = Oracle(prob, (net.weights, net.biases))
    xb, ub, sb, ib = o.solve_batch(x0[:64], xg[:64], ug[:64], p[:64])
    assert np.array_equal(sb, st[:64])
    assert np.abs(ub - u[:64]).max() < 1e-4 * (1 + np.abs(ub).max())


def test_device_pointer_path_matches_host_path():
    import torch
    par, prob, net = make_problem('st', N=30)
    s = _solver(prob, net)
    B = 256
    x0 = sample_instances(prob, B, seed=5)
    xg, ug, p = constant_guess(prob, x0)
    xh, uh, sh, ih = s.solve(x0, xg, ug, p)
    dev = torch.device('cuda:0')
    t = lambda a: torch.tensor(a, dtype=torch.float64, device=dev)
    xd, ud, sd, idd = s.solve(t(x0), t(xg), t(ug), t(p))
    s.sync()
    assert np.array_equal(xd.cpu().numpy(), xh) and np.array_equal(ud.cpu().numpy(), uh)
    assert np.array_equal(sd.cpu().numpy(), sh)


def test_buffer_growth_inside_a_graph_capture_is_a_state_error():
    """A handle's buffers grow in eager calls only.  The engine's stream joins a capture through BatchedOcpSolver._ordered, as in
    closed_loop._DeviceGroup._run_half: a captured solve of a warmed-up batch size replays what the eager solve computed, and a captured
    solve that would have to grow a buffer fails with SMPC_ESTATE instead of synchronising the capturing stream -- the capture still
    ends cleanly, and the next eager call grows the buffers."""
    import warnings
    import torch
    from safe_mpc_amd._lib import EngineError
    par, prob, net = make_problem('st', N=20)
    s, o = _solver(prob, net), _oracle(prob, net)
    B = 128
    x0 = sample_instances(prob, B, seed=7, vel_scale=0.1)
    xg, ug, p = constant_guess(prob, x0)
    big = [torch.tensor(a, dtype=torch.float64, device='cuda:0') for a in (x0, xg, ug, p)]
    small = [a[:B // 2] for a in big]
    eager = s.solve(*small)                      # (grows every buffer of B / 2 instances)
    out = tuple(torch.empty_like(a) for a in eager)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        s.solve(*small, out=out)
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip(out, eager):
        assert torch.equal(a, b)
    with pytest.raises(EngineError, match='engine error -4: .* while the stream is being captured'), warnings.catch_warnings():
        warnings.filterwarnings('ignore', 'The CUDA Graph is empty')       # (the refused solve captured nothing)
        with torch.cuda.graph(torch.cuda.CUDAGraph()):
            s.solve(*big)
    torch.cuda.synchronize()
    xa, ua, sa, ia = (a.cpu().numpy() for a in s.solve(*big))
    xb, ub, sb, ib = o.solve_batch(x0, xg, ug, p)
    assert np.array_equal(sa, sb)
    ok = sb == 0
    assert ok.sum() >= B - 2
    assert np.abs(ia[ok] - ib[ok]).max() <= 2
    assert np.abs(ua[ok] - ub[ok]).max() < 1e-4 * (1 + np.abs(ub[ok]).max())
    assert np.abs(xa[ok] - xb[ok]).max() < 1e-4


def test_policy_layer_and_scripts_on_engine(tmp_path):
    """The batched controllers + run_mpc on the real engine agree with the same code on the CPU test double."""
    from fake_solver import OracleSolver
    from safe_mpc_amd import closed_loop as cl
    from safe_mpc_amd import controller as C
    from safe_mpc_amd.parser import Parameters
    par = Parameters({}, 'z1')
    par.nq, par.n_dof_safe_set, par.net_size, par.N, par.back_hor = 6, 6, [12, 256, 1], 10, 12
    prob0 = C.OcpProblem(par, 'htwa', 'ext', N=10)
    x0 = sample_instances(prob0, 12, seed=9)
    xg = np.repeat(x0[:, None, :], 11, axis=1)
    ug = np.zeros((12, 10, 6))

    def cpu_ctrl(name, batch):
        cls = C.CONTROLLERS[name]
        c = cls.__new__(cls)
        prob = C.OcpProblem(par, cls.cont_name, 'ext', N=10)
        net = C.SafeSetNet.from_params(par, prob.x_min, prob.x_max)
        prob.set_normalisation(net.mean, net.std)
        C.AbstractController.__init__(c, par, batch, 'ext', 10, solver=OracleSolver(prob, net), net=net)
        return c

    def cpu_backup(batch):
        c = C.SafeBackupController.__new__(C.SafeBackupController)
        prob = C.OcpProblem(par, 'backup', 'zero', N=12)
        C.AbstractController.__init__(c, par, batch, 'zero', 12, solver=OracleSolver(prob, None), net=None)
        return c

    for name in ('htwa', 'receding'):
        gpu = cl.run_mpc(par, name, xg, ug, n_steps=15)
        cpu = cl.run_mpc(par, name, xg, ug, n_steps=15, make_controller=cpu_ctrl, make_backup=cpu_backup)
        assert gpu['collisions_idx'] == cpu['collisions_idx'] and gpu['viable_idx'] == cpu['viable_idx']
        both = ~np.isnan(cpu['x']).any(axis=(1, 2))
        assert both.sum() >= 8
        assert np.nanmax(np.abs(gpu['x'][both] - cpu['x'][both])) < 1e-4


def test_instance_bounds_parity(qp_mode):
    """smpc_set_instance_bounds: per-instance state tubes (RealReceding) agree with the oracle and clear again."""
    par, prob, net = make_problem('real_receding', N=10)
    s, o = _solver(prob, net), _oracle(prob, net)
    B = 16
    x0 = sample_instances(prob, B, seed=12, vel_scale=0.1)
    xg, ug, p = constant_guess(prob, x0)
    xa0, ua0, sa0, _ = s.solve(x0, xg, ug, p)
    lo = np.broadcast_to(prob.x_min, (B, 11, 12)).copy(); hi = np.broadcast_to(prob.x_max, (B, 11, 12)).copy()
    r = 2 + np.arange(B) % 7
    lo[np.arange(B), r] = xa0[np.arange(B), r] - 1e-3
    hi[np.arange(B), r] = xa0[np.arange(B), r] + 1e-3
    s.set_instance_bounds(lo, hi); o.set_instance_bounds(lo, hi)
    xa, ua, sa, ia = s.solve(x0, xg, ug, p)
    xb, ub, sb, ib = o.solve_batch(x0, xg, ug, p)
    assert np.array_equal(sa, sb)
    ok = sb == 0
    assert ok.sum() >= B - 2 and np.abs(ua[ok] - ub[ok]).max() < 1e-4 * (1 + np.abs(ub[ok]).max())
    assert np.all(np.abs(xa[ok, r[ok]] - xa0[ok, r[ok]]) <= 1e-3 + 1e-6)
    s.set_instance_bounds(None, None)
    xa1, ua1, _, _ = s.solve(x0, xg, ug, p)
    assert np.array_equal(ua1, ua0)


def test_stall_exit_parity_on_infeasible_tubes(qp_mode):
    """qp_stall_iters -- engine and oracle give up on the same infeasible RealReceding QPs at the same
    iteration (QP failure, iterate still returned), and the option leaves feasible solves alone."""
    from test_oracle_qp import _unreachable_tube
    N = 12
    par, prob, net = make_problem('real_receding', N=N)
    s, o = _solver(prob, net), _oracle(prob, net)
    x0 = sample_instances(prob, 24, seed=4)
    xg, ug, p = constant_guess(prob, x0)
    lo, hi = _unreachable_tube(prob, x0, N)
    lo[::2], hi[::2] = prob.x_min, prob.x_max                     # every other instance keeps the model bounds: feasible
    lo[::2, N], hi[::2, N] = prob.lbx_e, prob.ubx_e
    s.set_instance_bounds(lo, hi); o.set_instance_bounds(lo, hi)
    xa, ua, sa, ia = s.solve(x0, xg, ug, p)
    xb, ub, sb, ib = o.solve_batch(x0, xg, ug, p)
    assert np.array_equal(sa, sb) and np.all(sb[1::2] == 4) and np.all(sb[::2] == 0)
    assert np.abs(ia.astype(int) - ib.astype(int)).max() <= 2 and ia[1::2].max() <= 32
    ok = sb == 0
    assert np.abs(ua[ok] - ub[ok]).max() < 1e-4 * (1 + np.abs(ub[ok]).max())
    s.set_instance_bounds(None, None)


@pytest.mark.parametrize('nq,B,drop_rows', [(6, 1, 0), (6, 33, 0), (5, 17, 0), (6, 9, 2), (6, 12, 6), (6, 11, -6), (7, 6, -4)])
def test_kernel_instantiations_and_odd_batches(nq, B, drop_rows, qp_mode):
    """k_qp_ipm pairs two instances per wavefront: odd batches leave a lone half-wave; nq = 5 (the reference's default
    n_dofs, config.yaml:10) and a row count other than the specialised 6 take other template instantiations.  The extremes:
    no collision rows at all, SMPC_MAX_ROWS = 12 of them, and (nq = 7, 10 rows) the stage that fills all 32 row lanes."""
    par, prob, net = make_problem('st', 'ext', N=12, nq=nq)
    x0 = sample_instances(prob, B, seed=5, vel_scale=0.1)
    if drop_rows > 0:
        prob.desc.n_rows -= drop_rows          # the last capsule pairs go: the runtime-row-count kernel
    elif drop_rows < 0:
        # more rows: the same capsule pairs again with a laxer lower bound (distinct rows, mostly inactive)
        n0 = prob.desc.n_rows
        for r in range(-drop_rows):
            src = prob.desc.rows[r % n0]
            dst = prob.desc.rows[n0 + r]
            for f, _ in type(src)._fields_:
                setattr(dst, f, getattr(src, f))
            dst.lb = 0.6 * src.lb
        prob.desc.n_rows = n0 - drop_rows
        assert 3 * nq + prob.desc.n_rows + 1 <= 32
    s, o = _solver(prob, net), _oracle(prob, net)
    xg, ug, p = constant_guess(prob, x0)
    xa, ua, sa, ia = s.solve(x0, xg, ug, p)
    xb, ub, sb, ib = o.solve_batch(x0, xg, ug, p)
    assert np.array_equal(sa, sb)
    ok = sb == 0
    assert ok.sum() >= B - 1
    assert np.abs(ia[ok] - ib[ok]).max() <= 2
    assert np.abs(ua[ok] - ub[ok]).max() < 1e-4 * (1 + np.abs(ub[ok]).max())
    assert np.abs(xa[ok] - xb[ok]).max() < 1e-4


def _stage_records(s, x0, xg, ug, p, path):
    """the QP workspace after the stage records are built (no interior point), by either builder: test hook of the engine"""
    import ctypes as C
    L = s.L
    L.smpc_debug_stage_records.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 4 + [C.c_int, C.c_void_p, C.c_void_p]
    lay = np.zeros(24, np.int32)
    B = x0.shape[0]
    # (first call with a one-element buffer only to learn the size)
    arrs = [np.ascontiguousarray(a, np.float64) for a in (x0, xg, ug, p)]
    from safe_mpc_amd.problem import OcpProblem  # noqa: F401
    probe = np.zeros(1)
    per = None
    for _ in range(2):
        out = probe if per is None else np.zeros((B, per))
        if per is None:
            # learn the layout from a B = 1 call into a generous buffer
            out = np.zeros(64 * 2048)
            rc = L.smpc_debug_stage_records(s.h, 1, *[a[:1].ctypes.data for a in arrs], path, out.ctypes.data, lay.ctypes.data)
            assert rc == 0, L.smpc_last_error(s.h)
            per = int(lay[14])
            assert per <= out.size
            continue
        rc = L.smpc_debug_stage_records(s.h, B, *[a.ctypes.data for a in arrs], path, out.ctypes.data, lay.ctypes.data)
        assert rc == 0, L.smpc_last_error(s.h)
    return out, lay


@pytest.mark.parametrize('case', ['st', 'constraint_everywhere', 'zerovel_nls', 'receding_flags', 'real_receding_tubes', 'fr7', 'nq5',
                                  'rows12', 'rows0', 'backup_zero_cost'])
def test_stage_builder_equals_thread_per_node_kernels(case):
    """Round 4: the lane-cooperative stage builder (kernel_build.hpp: k_stage_build, linearisation + QP set-up in one pass, 8
    lanes per node) against the thread-per-node kernels of rounds 1-3 (k_node_linearise -> k_qp_setup), block by block of the
    stage record: Jacobian image, cost blocks, defect, bounds, initial slacks / multipliers, start vectors, the stage's partial
    sums.  Same formulas, different distribution and summation order: 1e-11 relative to each block's scale.  (The thread-per-node
    path is itself pinned to the oracle at 1e-9 by test_eval_nodes_parity; the solves below it run through the builder.)"""
    from conftest import make_problem_fr7
    N = 12
    kw = {}
    if case == 'fr7':
        par, prob, net = make_problem_fr7(N=16)
        N = 16
    elif case == 'zerovel_nls':
        par, prob, net = make_problem('zerovel', 'nls', N=N)
    elif case == 'backup_zero_cost':
        par, prob, net = make_problem('backup', 'zero', N=N)
    elif case == 'nq5':
        par, prob, net = make_problem('st', 'ext', N=N, nq=5)
    elif case in ('rows12', 'rows0'):
        par, prob, net = make_problem('st', 'ext', N=N)
        x0_pre = sample_instances(prob, 11, seed=3, vel_scale=0.3)       # (sampled against the unmodified geometry)
        if case == 'rows0':
            prob.desc.n_rows = 0
        else:
            n0 = prob.desc.n_rows
            for r in range(6):
                src, dst = prob.desc.rows[r % n0], prob.desc.rows[n0 + r]
                for f, _ in type(src)._fields_:
                    setattr(dst, f, getattr(src, f))
                dst.lb = 0.6 * src.lb
            prob.desc.n_rows = 12
    else:
        name = {'receding_flags': 'receding', 'real_receding_tubes': 'real_receding'}.get(case, case)
        par, prob, net = make_problem(name, 'ext', N=N)
    B = 11
    s = _solver(prob, net)
    x0 = x0_pre if case in ('rows12', 'rows0') else sample_instances(prob, B, seed=3, vel_scale=0.3)
    xg, ug, p = constant_guess(prob, x0)
    rng = np.random.default_rng(2)
    ug += rng.uniform(-3, 3, ug.shape)
    xg = s.guess_correction(xg, ug)
    xg[:, 1:] += 0.01 * rng.standard_normal(xg[:, 1:].shape)          # a dynamics defect
    x0 = x0 + 0.003 * rng.standard_normal(x0.shape)                   # dx_0 != 0
    if case == 'receding_flags':
        p[:, :, 4] = np.where(rng.uniform(size=p.shape[:2]) < 0.5, 1.0, -1.0)
        s.set_slack_weights(np.concatenate([[0.0], rng.choice([0.0, 1e2, 1e4], N)]))
    if case == 'real_receding_tubes':
        lo = np.broadcast_to(prob.x_min, (B, N + 1, prob.nx)).copy()
        hi = np.broadcast_to(prob.x_max, (B, N + 1, prob.nx)).copy()
        lo[:, N], hi[:, N] = prob.lbx_e, prob.ubx_e
        for b in range(B):
            r = 1 + b % (N - 1)
            lo[b, r], hi[b, r] = xg[b, r + 1] - 1e-3, xg[b, r + 1] + 1e-3
        s.set_instance_bounds(lo, hi)
    new, lay = _stage_records(s, x0, xg, ug, p, 1)
    old, lay2 = _stage_records(s, x0, xg, ug, p, 0)
    assert np.array_equal(lay, lay2)
    stride, nIMG, oIMG, oSL, nF, oR0, oR1, oR2, oCZA, oCZN, oZ, oZN, NRT, nJ, per = [int(v) for v in lay[:15]]
    new, old = new.reshape(B, N + 1, stride), old.reshape(B, N + 1, stride)
    blocks = {'jacobian': (oIMG, nJ), 'defect / scalars': (oIMG + nJ, nF - nJ), 'cost': (oIMG + nF, nIMG - nF),
              'scalars + partial sums + w': (oSL, 16), 'bounds': (oR0, 2 * NRT), 'slacks': (oR1, 2 * NRT), 'multipliers': (oR2, 2 * NRT),
              'c.z_aff': (oCZA, 32), 'c.z+': (oCZN, 32), 'z': (oZ, 3 * prob.nq), 'z+': (oZN, 3 * prob.nq)}
    for name, (o, n) in blocks.items():
        a, b = new[:, :, o:o + n], old[:, :, o:o + n]
        big = np.abs(b) >= 1e299                                 # the "absent" sentinel
        assert np.array_equal(np.abs(a) >= 1e299, big), name
        a, b = np.where(big, 0.0, a), np.where(big, 0.0, b)
        scale = np.abs(b).max() + 1e-300
        assert np.abs(a - b).max() <= 1e-11 * scale + 1e-13, (case, name, np.abs(a - b).max(), scale)
    assert np.abs(old[:, :, oIMG:oIMG + nJ]).max() > 0


@pytest.mark.parametrize('case', ['st', 'constraint_everywhere', 'zerovel_nls', 'fr7'])
def test_stage_builder_records_equal_oracle_qp(case):
    """The stage records the builder writes (the QP the interior point then solves) against the oracle's stage QP
    (Oracle.build_qp: link-frame Newton-Euler with dual numbers, dense stage matrices -- nothing shared), entry by entry:
    constraint Jacobian (torque rows' M | dtau/dq | dtau/dqd, collision rows, the network's row), cost Hessian and gradient,
    dynamics defect, bounds.  1e-9 of each block's scale (the tolerance of test_eval_nodes_parity, which covers the
    thread-per-node kernels behind smpc_eval_nodes); the network's row 2e-4 (fp32 MFMA against the oracle's fp64 restatement)."""
    from conftest import make_problem_fr7
    N = 10
    if case == 'fr7':
        par, prob, net = make_problem_fr7(N=N)
    elif case == 'zerovel_nls':
        par, prob, net = make_problem('zerovel', 'nls', N=N)
    else:
        par, prob, net = make_problem(case, 'ext', N=N)
    nq, nx, nu = prob.nq, prob.nx, prob.nu
    B = 5
    s, o = _solver(prob, net), _oracle(prob, net)
    x0 = sample_instances(prob, B, seed=4, vel_scale=0.3)
    xg, ug, p = constant_guess(prob, x0, ee_ref=prob.ee_ref)
    rng = np.random.default_rng(3)
    ug += rng.uniform(-3, 3, ug.shape)
    xg = s.guess_correction(xg, ug)
    xg[:, 1:] += 0.01 * rng.standard_normal(xg[:, 1:].shape)
    x0 = x0 + 0.003 * rng.standard_normal(x0.shape)
    ws, lay = _stage_records(s, x0, xg, ug, p, 1)
    stride, nIMG, oIMG, oSL, nF, oR0, oR1, oR2, oCZA, oCZN, oZ, oZN, NRT, nJ, per = [int(v) for v in lay[:15]]
    ws = ws.reshape(B, N + 1, stride)
    MR = prob.desc.n_rows
    NQP, MRP, NZ = nq + nq % 2, MR + MR % 2, 3 * nq
    iTT, iGT, iGN, iB, iSC, iHQQ, iGZ = [int(v) for v in lay[16:23]]        # (record v12: the hook reports the image's own offsets)
    assert (iTT, iGT, iGN) == (0, NZ * NQP, NZ * NQP + nq * MRP) and iGN + nx == nJ and int(lay[15]) == 12
    assert sorted([iB, iSC, iHQQ, iGZ])[0] == nJ and max(iB + nx, iSC + 4, iHQQ + nq * nq, iGZ + NZ) <= nIMG

    def close(a, b, tol, what):
        scale = np.abs(b).max() + 1e-300
        assert np.abs(a - b).max() <= tol * scale + 1e-12, (case, what, np.abs(a - b).max(), scale)
    for b in range(B):
        qp = o.build_qp(x0[b], xg[b], ug[b], p[b])
        for k in range(N + 1):
            img = ws[b, k, oIMG:oIMG + nIMG]
            last = k == N
            off = 0 if last else nu                        # the oracle's stage variable is [u; x], [x] at the end
            Cm, H, g = qp['C'][k], qp['H'][k], qp['g'][k]
            TT = img[iTT:iTT + NZ * NQP].reshape(NZ, NQP)[:, :nq]                      # Tt[c][r]
            GT = img[iGT:iGT + nq * MRP].reshape(nq, MRP)[:, :MR] if MR else np.zeros((nq, 0))
            GN = img[iGN:iGN + nx]
            if not last:
                close(TT.T, Cm[nx:nx + nq, :NZ], 1e-9, 'torque rows')
            else:
                assert np.all(TT == 0.0)
            close(GT.T, Cm[nx + nq:nx + nq + MR, off:off + nq], 1e-9, 'collision rows')
            close(GN, Cm[nx + nq + MR, off:off + nx], 2e-4, 'network row')
            close(img[iHQQ:iHQQ + nq * nq].reshape(nq, nq), H[off:off + nq, off:off + nq], 1e-9, 'cost Hessian')
            gz = img[iGZ:iGZ + NZ]
            if not last:
                close(gz[:nu], g[:nu], 1e-12, 'cost gradient u')
            close(gz[nu:nu + nq], g[off:off + nq], 1e-9, 'cost gradient q')
            assert np.all(gz[nu + nq:] == 0.0)
            close(img[iB:iB + nx], qp['b'][k][:nx], 1e-9, 'defect')
            if not last:
                assert abs(img[iSC] - H[0, 0]) <= 1e-12 * abs(H[0, 0])              # Huu diagonal
            r0 = ws[b, k, oR0:oR0 + 2 * NRT].reshape(NRT, 2)
            nr = int(qp['nr'][k])
            assert nr == NRT
            lo = np.where(qp['has_lo'][k][:nr], qp['lo'][k][:nr], -1e300)
            hi = np.where(qp['has_hi'][k][:nr], qp['hi'][k][:nr], 1e300)
            absent = np.abs(r0) >= 1e299
            assert np.array_equal(absent[:, 0], lo <= -1e299) and np.array_equal(absent[:, 1], hi >= 1e299), (case, b, k)
            rows_fp64 = np.arange(nr) != nx + nq + MR               # (the network's row: its value is an fp32 product)
            close(np.where(absent[:, 0], 0.0, r0[:, 0])[rows_fp64], np.where(absent[:, 0], 0.0, lo)[rows_fp64], 1e-9, 'lower bounds')
            close(np.where(absent[:, 1], 0.0, r0[:, 1])[rows_fp64], np.where(absent[:, 1], 0.0, hi)[rows_fp64], 1e-9, 'upper bounds')
            if not absent[nx + nq + MR, 0]:
                assert abs(r0[nx + nq + MR, 0] - lo[nx + nq + MR]) < 2e-4 * (1 + abs(lo[nx + nq + MR]))


@pytest.mark.parametrize('case', ['st', 'constraint_everywhere', 'receding', 'zerovel_nls', 'fr7', 'nq5_rows4'])
def test_qp_kernels_agree(case):
    """k_qp_ipm_wg (a workgroup per instance: stage-parallel row work, recursions through LDS; round 6) against k_qp_ipm (a wavefront
    per two instances) on the SAME handle-built stage records: same algorithm and per-row arithmetic, a few sums in another order.
    Over a ten-step closed loop driven by the throughput kernel's result: statuses equal at every solve, iteration counts equal but
    for the odd instance whose exit test is decided by rounding (<= 1 apart), every control within 5e-6 (1 + |u|) where the counts
    are equal -- the tolerance of two IPMs walking the same path from rounding-different starts (the first, cold solve agrees to
    1e-8; from the second step on the QPs have flat directions, DESIGN.md section 5, and rounding-level differences of the Newton
    systems show up at 1e-7); a different count means one more IPM step, i.e. the solution tolerance."""
    from conftest import make_problem_fr7
    nq = 6
    if case == 'fr7':
        par, prob, net = make_problem_fr7(N=40)
        nq = 7
    elif case == 'zerovel_nls':
        par, prob, net = make_problem('zerovel', 'nls', N=20)
    elif case == 'nq5_rows4':
        par, prob, net = make_problem('st', 'ext', N=12, nq=5)
        prob.desc.n_rows -= 2
        nq = 5
    else:
        par, prob, net = make_problem(case, 'ext', N=30)
    N = prob.N
    a, b = _solver(prob, net), _solver(prob, net)
    a.set_qp_mode('throughput'); b.set_qp_mode('latency')
    B = 96 if case != 'fr7' else 40
    x = sample_instances(prob, B, seed=21, vel_scale=0.1)
    xg, ug, p = constant_guess(prob, x)
    if case == 'receding':
        p[:, 1:N, 4] = -1.0
        p[np.arange(B), 1 + np.arange(B) % (N - 1), 4] = 1.0
    # (zerovel pins the terminal velocity with lb == ub: the two barrier terms of a zero-width box make the last Newton systems
    #  ill-conditioned -- the tolerance of this case against the oracle, test_rti_solve_parity, is 2e-5 for the same reason)
    tol0, tol1 = (5e-5, 5e-5) if case == 'zerovel_nls' else (1e-7, 5e-6)
    worst, differ = 0.0, 0
    for step in range(10):
        xa, ua, sa, ia = a.solve(x, xg, ug, p)
        xb, ub, sb, ib = b.solve(x, xg, ug, p)
        assert np.array_equal(sa, sb), step
        d = np.abs(ia.astype(int) - ib.astype(int))
        assert d.max() <= 1, (step, ia, ib)
        differ += int((d > 0).sum())
        same = (d == 0) & (sa == 0)
        if same.any():
            err = np.abs(ua[same] - ub[same]).max() / (1 + np.abs(ua[same]).max())
            worst = max(worst, err)
            assert err < (tol0 if step == 0 else tol1), (step, err)
            assert np.abs(xa[same] - xb[same]).max() < tol1
        xg, ug, uapp = a.provide_control((sa == 0).astype(np.int32), xa, ua, xg, ug)
        x, _ = a.plant_step(x, uapp)
        xg = a.guess_correction(xg, ug)
    assert differ <= max(2, B // 10), differ
    print(f'[qp kernels, {case}] worst control gap {worst:.1e}, {differ} solves with iteration counts one apart')


def test_qp_mode_argument_is_checked():
    """smpc_set_qp_mode: anything but AUTO / THROUGHPUT / LATENCY is API misuse (an error code and a message, no change of mode); the
    three valid modes give the same statuses and the same controls to the kernels' mutual tolerance."""
    par, prob, net = make_problem('st', 'ext', N=8)
    s = _solver(prob, net)
    assert s.L.smpc_set_qp_mode(s.h, 7) != 0 and b'qp mode' in s.L.smpc_last_error(s.h)
    assert s.L.smpc_set_qp_mode(s.h, -2) != 0
    x0 = sample_instances(prob, 6, seed=3)
    xg, ug, p = constant_guess(prob, x0)
    ref = s.solve(x0, xg, ug, p)
    for mode in ('throughput', 'latency', 'auto'):
        s.set_qp_mode(mode)
        out = s.solve(x0, xg, ug, p)
        assert np.array_equal(out[2], ref[2]) and np.abs(out[1] - ref[1]).max() < 1e-7 * (1 + np.abs(ref[1]).max())


@pytest.mark.parametrize('N', [1, 2, 3, 63])
def test_horizon_extremes(N, qp_mode):
    """Shortest horizons (the unrolled / look-ahead loops of the QP kernel degenerate) and SMPC_MAX_N."""
    par, prob, net = make_problem('st', 'ext', N=N)
    s, o = _solver(prob, net), _oracle(prob, net)
    B = 10
    x0 = sample_instances(prob, B, seed=7, vel_scale=0.1)
    xg, ug, p = constant_guess(prob, x0)
    xa, ua, sa, ia = s.solve(x0, xg, ug, p)
    xb, ub, sb, ib = o.solve_batch(x0, xg, ug, p)
    assert np.array_equal(sa, sb)
    ok = sb == 0
    assert ok.sum() >= B - 1
    assert np.abs(ia[ok] - ib[ok]).max() <= 2
    assert np.abs(ua[ok] - ub[ok]).max() < 1e-4 * (1 + np.abs(ub[ok]).max())
    assert np.abs(xa[ok] - xb[ok]).max() < 1e-4


def test_empty_batch_is_a_no_op():
    par, prob, net = make_problem('naive', N=5)
    s = _solver(prob, net)
    x, u, st, it = s.solve(np.zeros((0, 12)), np.zeros((0, 6, 12)), np.zeros((0, 5, 6)), np.zeros((0, 6, 5)))
    assert x.shape == (0, 6, 12) and u.shape == (0, 5, 6) and st.shape == (0,) and it.shape == (0,)


@pytest.mark.parametrize('controller', ['st', 'constraint_everywhere'])
def test_closed_loop_tracks_oracle(controller, qp_mode):
    """Eight closed-loop RTI steps (guessCorrection -> solve -> provideControl -> plant) on the engine and on the oracle from the
    same start: same statuses every step, states within 1e-5 at the end (the fp32 network is the only non-FP64 piece)."""
    par, prob, net = make_problem(controller, 'ext', N=20)
    s, o = _solver(prob, net), _oracle(prob, net)
    B = 48
    x0 = sample_instances(prob, B, seed=11, vel_scale=0.1)
    xg, ug, p = constant_guess(prob, x0)
    xa, xga, uga = x0.copy(), xg.copy(), ug.copy()
    xb, xgb, ugb = x0.copy(), xg.copy(), ug.copy()
    for step in range(8):
        ra, rb = s.solve(xa, xga, uga, p), o.solve_batch(xb, xgb, ugb, p)
        assert np.array_equal(ra[2], rb[2]), step
        acc = (rb[2] == 0).astype(np.int32)
        xga, uga, ua = s.provide_control(acc, ra[0], ra[1], xga, uga)
        xgb, ugb, ub = o.provide_control(acc, rb[0], rb[1], xgb, ugb)
        xa, _ = s.plant_step(xa, ua)
        xb, _ = o.plant_step(xb, ub)
        xga, xgb = s.guess_correction(xga, uga), o.guess_correction(xgb, ugb)
    assert np.abs(xa - xb).max() < 1e-5
    assert np.abs(xga - xgb).max() < 1e-4


def test_rollout_equals_step_by_step():
    """smpc_rollout_batch is the same launch sequence as the step-by-step calls: bitwise equal trajectories, host and
    device pointer paths, with per-step torque noise."""
    import torch
    par, prob, net = make_problem('st', 'ext', N=15)
    s = _solver(prob, net)
    B, n = 33, 6
    x0 = sample_instances(prob, B, seed=13, vel_scale=0.1)
    xg, ug, p = constant_guess(prob, x0)
    noise = 0.05 * np.random.default_rng(3).standard_normal((n, B, 6))
    # step by step (host path)
    x, xg1, ug1, fails = x0.copy(), xg.copy(), ug.copy(), np.zeros(B, np.int64)
    X, U, S = [x0.copy()], [], []
    for t in range(n):
        xg1 = s.guess_correction(xg1, ug1)
        xo, uo, st, it = s.solve(x, xg1, ug1, p)
        fails = np.where(st == 0, 0, fails + 1)
        xg1, ug1, ua = s.provide_control((fails == 0).astype(np.int32), xo, uo, xg1, ug1)
        x, _ = s.plant_step(x, ua, tau_noise=noise[t])
        X.append(x.copy()); U.append(ua.copy()); S.append(st.copy())
    X, U, S = np.array(X), np.array(U), np.array(S)
    # one call, host pointers
    xt, ut, st_, it_, xg2, ug2 = s.rollout(x0, xg, ug, p, n, tau_noise=noise)
    assert np.array_equal(st_, S) and np.array_equal(xt, X) and np.array_equal(ut, U)
    assert np.array_equal(xg2, xg1) and np.array_equal(ug2, ug1)
    assert (it_ > 0).all()
    # one call, device pointers
    dev = torch.device('cuda:0')
    t = lambda a: torch.tensor(a, dtype=torch.float64, device=dev)
    xgd, ugd = t(xg), t(ug)
    xtd, utd, std, itd, _, _ = s.rollout(t(x0), xgd, ugd, t(p), n, tau_noise=t(noise))
    s.sync()
    assert np.array_equal(xtd.cpu().numpy(), X) and np.array_equal(utd.cpu().numpy(), U) and np.array_equal(std.cpu().numpy(), S)
    assert np.array_equal(xgd.cpu().numpy(), xg1)


def test_eval_nodes_device_path_matches_host_path():
    import torch
    par, prob, net = make_problem('st', 'ext', N=8)
    s = _solver(prob, net)
    B = 9
    x0 = sample_instances(prob, B, seed=4, vel_scale=0.2)
    xg, ug, p = constant_guess(prob, x0)
    ug += 1.0
    a = s.eval_nodes(xg, ug, p)
    dev = torch.device('cuda:0')
    t = lambda v: torch.tensor(v, dtype=torch.float64, device=dev)
    b = s.eval_nodes(t(xg), t(ug), t(p))
    s.sync()
    for f in ('tau', 'M', 'dtau_dq', 'dtau_dv', 'ee', 'cost_grad_q', 'cost_hess_qq', 'row_val', 'row_grad', 'nn_val', 'nn_grad'):
        assert np.array_equal(np.asarray(a[f]), b[f].cpu().numpy()), f


def test_mlp_layer_by_layer_gemm_kernels_in_child_processes():
    """From 8 192 network rows on the default is the one-wave fused kernel (k_mlp_wave, round 5); the layer-by-layer GEMM chain of
    rounds 1-4 stays selectable (SMPC_MLP_LARGE=chain: one-wave blocks of k_gemm_f32) for A/B runs and for networks that are not
    256 wide with three hidden layers.  The knob is read once per process, so the chain is exercised in a child process running the
    large-row tests of this file."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, SMPC_MLP_LARGE='chain')
    r = subprocess.run([sys.executable, '-m', 'pytest', os.path.join(root, 'tests', 'test_gpu_parity.py'), '-m', 'gpu', '-q', '-x', '-k',
                        'test_mlp_large_row_counts or test_mlp_activations_fused_and_large_paths'], env=env, cwd=root, capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert '7 passed' in r.stdout, r.stdout[-500:]


@pytest.mark.parametrize('switched', [False, True])
def test_mlp_large_row_counts(switched):
    """The safe-set row on every node of 520 instances x 16 stages = 8 320 MLP rows: the large-row path (default: k_mlp_wave, one-wave
    blocks of 16 rows; the GEMM chain in the child processes above).  `switched`: the per-node switch p[4] random, so the rows are a
    compacted list (mode 3) whose length is not a multiple of a block's 16 rows, and the switched-off nodes' slots must stay zero."""
    par, prob, net = make_problem('constraint_everywhere', 'ext', N=16)
    s, o = _solver(prob, net), _oracle(prob, net)
    B = 520
    x0 = sample_instances(prob, B, seed=6, vel_scale=0.3)
    xg, ug, p = constant_guess(prob, x0)
    rng = np.random.default_rng(0)
    xg[:, 1:] += 0.05 * rng.standard_normal(xg[:, 1:].shape)
    if switched:
        p[:, :, 4] = np.where(rng.uniform(size=p.shape[:2]) < 0.55, 1.0, -1.0)
        if int((p[:, 1:, 4] > 0).sum()) % 16 == 0:
            p[np.unravel_index(np.argmax(p[:, 1:, 4] > 0), p[:, 1:, 4].shape)[0], 1 + np.unravel_index(np.argmax(p[:, 1:, 4] > 0), p[:, 1:, 4].shape)[1], 4] = -1.0
        assert int((p[:, 1:, 4] > 0).sum()) % 16 != 0
    a, b = s.eval_nodes(xg, ug, p), o.eval_nodes(xg, ug, p)
    assert _rel(a['nn_val'], b['nn_val']) < 2e-5
    assert _rel(a['nn_grad'][..., :12], b['nn_grad'][..., :12]) < 2e-4
    if switched:
        off = p[:, :, 4] <= 0
        assert np.all(a['nn_val'][off] == 0.0) and np.all(a['nn_grad'][off] == 0.0) and np.abs(a['nn_val'][~off][:, None]).max() > 0
    # ... and through the solve (the stage builder reads the compact per-node buffer the kernel writes)
    xa, ua, sa, ia = s.solve(x0[:64], xg[:64], ug[:64], p[:64])       # (64 x 16 rows: the small-row kernel -- same numbers expected)
    xb, ub, sb, ib = o.solve_batch(x0[:64], xg[:64], ug[:64], p[:64])
    assert np.array_equal(sa, sb)


@pytest.mark.parametrize('act', ['gelu', 'relu', 'elu', 'tanh', 'silu'])
def test_mlp_activations_fused_and_large_paths(act):
    """VERDICT r2 item 7 / missing #3: every activation of parser.py:95-102 on the engine, through the fused small-batch
    kernel (terminal row: one launch for the whole network pass) and through the large-row path (row on every node, 8 192 rows:
    k_mlp_wave by default, the GEMM chains in test_mlp_layer_by_layer_gemm_kernels_in_child_processes), against the oracle's fp32 loops."""
    for controller, B, N in (('st', 96, 12), ('constraint_everywhere', 512, 16)):
        par, prob, net = make_problem(controller, 'ext', N=N, act=act)
        from oracle.oracle import Oracle
        s, o = _solver(prob, net), Oracle(prob, (net.weights, net.biases, net.act))
        x0 = sample_instances(prob, B, seed=6, vel_scale=0.3)
        xg, ug, p = constant_guess(prob, x0)
        xg[:, 1:] += 0.05 * np.random.default_rng(0).standard_normal(xg[:, 1:].shape)
        a, b = s.eval_nodes(xg, ug, p), o.eval_nodes(xg, ug, p)
        assert np.abs(b['nn_val']).max() > 0
        assert _rel(a['nn_val'], b['nn_val']) < 2e-5, (act, controller)
        assert _rel(a['nn_grad'][..., :12], b['nn_grad'][..., :12]) < 2e-4, (act, controller)


def test_mlp_fused_kernel_partial_blocks():
    """the fused network pass with a row count that is not a multiple of its 16-row blocks; the other nodes' slots stay untouched"""
    par, prob, net = make_problem('st', 'ext', N=10)
    x0 = sample_instances(prob, 77, seed=8, vel_scale=0.3)
    xg, ug, p = constant_guess(prob, x0)
    a = _solver(prob, net).eval_nodes(xg, ug, p)
    b = _oracle(prob, net).eval_nodes(xg, ug, p)
    assert _rel(a['nn_val'][:, -1], b['nn_val'][:, -1]) < 2e-5
    assert _rel(a['nn_grad'][:, -1, :12], b['nn_grad'][:, -1, :12]) < 2e-4
    assert np.all(a['nn_val'][:, :-1] == 0.0)                     # terminal row only: the other nodes' slots are untouched


def test_eval_nodes_device_path_large_batch_stream_order():
    """torch zero-fills the output on ITS stream while the engine writes it on its own non-blocking stream; the
    solver orders the two (solver._ordered).  Large enough that an unordered fill would land after the engine's records."""
    import torch
    par, prob, net = make_problem('st', 'ext', N=30)
    s = _solver(prob, net)
    B = 4096
    x0 = sample_instances(prob, 64, seed=4, vel_scale=0.2)[np.arange(B) % 64]
    xg, ug, p = constant_guess(prob, x0)
    ug += 1.0
    a = s.eval_nodes(xg, ug, p)
    dev = torch.device('cuda:0')
    for rep in range(3):
        # inputs produced by torch kernels right before the call, temporaries dropped right after it
        b = s.eval_nodes(torch.tensor(xg, device=dev) * 1.0, torch.tensor(ug, device=dev) + 0.0, torch.tensor(p, device=dev).clone())
        junk = torch.full((B, 31, 324), 7.0, dtype=torch.float64, device=dev)      # reuses freed blocks if unordered
        tau = b['tau'].cpu().numpy()
        assert np.array_equal(np.asarray(a['tau']), tau), rep
        assert np.array_equal(np.asarray(a['row_grad']), b['row_grad'].cpu().numpy())
        del junk


def test_rows_at_node0_status_parity(qp_mode):
    """controller.py:77-79: a start inside the collision band reports QP failure, engine and oracle alike."""
    par, prob, net = make_problem('naive', 'ext', N=8)
    s, o = _solver(prob, net), _oracle(prob, net)
    rng = np.random.default_rng(0)
    qs = rng.uniform(prob.lbx[:6], prob.ubx[:6], (600, 6))
    x0 = np.hstack([qs, np.zeros((600, 6))])
    free = o.check_trajectory(x0[:, None, :], prob.x_min, prob.x_max, 0.0, prob.row_lb, prob.row_ub)
    x0 = np.vstack([x0[~free][:12], x0[free][:12]])
    assert len(x0) == 24
    xg, ug, p = constant_guess(prob, x0)
    sa, sb = s.solve(x0, xg, ug, p)[2], o.solve_batch(x0, xg, ug, p)[2]
    assert np.array_equal(sa, sb) and np.all(sb[:12] == 4) and (sb[12:] == 0).sum() >= 10


def test_timing_before_any_solve_is_a_state_error():
    from safe_mpc_amd._lib import EngineError
    par, prob, net = make_problem('naive', N=5)
    s = _solver(prob, net)
    s.enable_timing(True)
    with pytest.raises(EngineError):
        s.timing()
    x0 = sample_instances(prob, 4, seed=0)
    s.solve(x0, *constant_guess(prob, x0))
    assert s.timing()['time_tot'] > 0


@pytest.mark.parametrize('name', ['htwa', 'receding', 'real_receding'])
def test_device_resident_policy_layer_equals_host_automaton(name):
    """the policy automata (controller.py:375-388, 448-498, 524-565) and the driver's abort / backup / PD
    loop (mpc.py:130-190) with all state in HBM (run_mpc(on_device=True)) against the same code on numpy arrays through the
    engine's host path: same outcome lists, same abort events, same receding indices, trajectories to rounding."""
    from safe_mpc_amd import closed_loop as cl
    from safe_mpc_amd import controller as C
    from safe_mpc_amd.parser import Parameters
    par = Parameters({}, 'z1')
    par.nq, par.n_dof_safe_set, par.net_size, par.N, par.back_hor = 6, 6, [12, 256, 1], 10, 12
    prob0 = C.OcpProblem(par, 'htwa', 'ext', N=10)
    B = 40
    x0 = sample_instances(prob0, B, seed=9, vel_scale=0.3)       # moving starts: some instances will have to abort
    xg = np.repeat(x0[:, None, :], 11, axis=1)
    ug = np.zeros((B, 10, 6))
    host = cl.run_mpc(par, name, xg, ug, n_steps=30, control_noise=1.0)
    # two pipelined groups on their own engine handles / streams: instances are independent, the split changes nothing
    dev = cl.run_mpc(par, name, xg, ug, n_steps=30, control_noise=1.0, on_device=True, groups=2 if name != 'htwa' else 1)
    for k in ('conv_idx', 'collisions_idx', 'unconv_idx', 'viable_idx'):
        assert host[k] == dev[k], k
    assert host['x_viable'].shape == dev['x_viable'].shape
    assert np.array_equal(host['r_receding'], dev['r_receding'])
    assert np.array_equal(np.isnan(host['x']), np.isnan(dev['x']))
    assert np.nanmax(np.abs(host['x'] - dev['x'])) < 1e-9 and np.nanmax(np.abs(host['u'] - dev['u'])) < 1e-7
    if host['x_viable'].size:
        assert np.abs(host['x_viable'] - dev['x_viable']).max() < 1e-9


def test_row_list_counter_is_handed_back_at_zero_by_every_chain():
    """Round 5: a policy step has no memset launches any more.  The length of the compacted row lists (the network pass of a
    formulation with the per-node switch, the receding policies' safe-set test) lives in one device counter that every chain of
    kernels using it hands back at zero -- k_stage_build after the network pass, k_policy_post after the safe-set test, a memset
    on the paths that have neither (smpc_eval_nodes).  Interleave all of them on ONE handle and hold every result against a
    fresh handle's / the oracle's: a counter left behind by one chain would inflate the next chain's list."""
    import torch
    from safe_mpc_amd import controller as C
    from safe_mpc_amd.parser import Parameters
    par = Parameters({}, 'z1')
    par.nq, par.n_dof_safe_set, par.net_size, par.N = 6, 6, [12, 256, 1], 8
    N, B = 8, 24
    dev = C.get_controller('receding', par, B, device_state=True)      # row switched per node: the network pass runs on a compacted list
    ref = C.get_controller('receding', par, B, device_state=True)      # the same policy steps on a handle that sees nothing else
    sv = dev.ocp_solver
    x0 = sample_instances(dev.problem, B, seed=3, vel_scale=0.3)
    xg, ug = np.repeat(x0[:, None, :], N + 1, axis=1), np.zeros((B, N, 6))
    dev.setGuess(xg, ug); ref.setGuess(xg, ug)
    rng = np.random.default_rng(1)
    p = np.zeros((B, N + 1, 5)); p[:, :, :3] = dev.problem.ee_ref; p[:, :, 3] = par.alpha
    p[:, :, 4] = np.where(rng.uniform(size=(B, N + 1)) < 0.5, 1.0, -1.0)
    fresh = lambda: C.get_controller('receding', par, B, device_state=True).ocp_solver
    ev_want = fresh().eval_nodes(xg, ug, p)
    sol_want = fresh().solve(x0, xg, ug, p)
    x = x0.copy()
    for t in range(6):
        xd = torch.tensor(x, device='cuda')
        ua, aa = dev.step_on_device(xd)
        ub, ab = ref.step_on_device(xd)
        sv.sync(); ref.ocp_solver.sync()
        assert np.array_equal(ua.cpu().numpy(), ub.cpu().numpy()) and np.array_equal(aa.cpu().numpy(), ab.cpu().numpy()), t
        assert np.array_equal(dev.r.cpu().numpy(), ref.r.cpu().numpy()), t
        # ... with the other entry points of the same handle in between, each against a fresh handle
        ev = sv.eval_nodes(xg, ug, p)
        assert np.array_equal(np.asarray(ev['nn_val']), np.asarray(ev_want['nn_val'])), t
        assert np.array_equal(np.asarray(ev['nn_grad']), np.asarray(ev_want['nn_grad'])), t
        xs, us, ss, its = sv.solve(x0, xg, ug, p)
        assert np.array_equal(ss, sol_want[2]) and np.array_equal(us, sol_want[1]), t
        x = x + par.dt * np.hstack([x[:, 6:], ua.cpu().numpy()])


@pytest.mark.parametrize('name,B', [('naive', 24), ('zerovel', 24), ('st', 24), ('stwa', 24), ('htwa', 24), ('receding', 24),
                                    ('real_receding', 24), ('constraint_everywhere', 24), ('receding', 1), ('htwa', 7)])
def test_policy_step_kernels_equal_numpy_automaton(name, B):
    """smpc_policy_step (kernels_policy.hpp) against <Controller>.step on numpy arrays (the readable statement of
    controller.py:274-284, 375-388, 448-498, 524-565, 651-661), step by step with a stepping mask: same controls, abort flags,
    counters, receding indices, viable states and shifted guesses for the instances that step; the others untouched."""
    import torch
    from safe_mpc_amd import closed_loop as cl
    from safe_mpc_amd import controller as C
    from safe_mpc_amd.parser import Parameters
    par = Parameters({}, 'z1')
    par.nq, par.n_dof_safe_set, par.net_size, par.N = 6, 6, [12, 256, 1], 8
    N = 8
    host = C.get_controller(name, par, B)
    dev = C.get_controller(name, par, B, device_state=True)
    x0 = sample_instances(host.problem, B, seed=3, vel_scale=0.4)      # moving starts: failures and aborts do happen
    xg, ug = np.repeat(x0[:, None, :], N + 1, axis=1), np.zeros((B, N, 6))
    host.setGuess(xg, ug)
    dev.setGuess(xg, ug)
    rng = np.random.default_rng(0)
    x = x0.copy()
    n_abort = n_fail = 0
    for t in range(2 * N + 4):
        stepping = rng.random(B) > 0.2 if t % 3 else np.ones(B, bool)
        u_other = rng.normal(size=(B, 6))
        before = {k: np.array(getattr(host, k)) for k in cl._STATE if hasattr(host, k)}
        uh, ah = cl._masked_step(host, x, stepping)
        uh = np.where(stepping[:, None], uh, u_other)
        xd = torch.tensor(x, device='cuda')
        ud, ad = dev.step_on_device(xd, torch.tensor(stepping, device='cuda'), torch.tensor(u_other, device='cuda'))
        dev.ocp_solver.sync()
        assert np.array_equal(ad.cpu().numpy(), ah), t
        assert bool(dev._any_abort.item()) == bool(ah.any())
        assert np.abs(ud.cpu().numpy() - uh).max() < 1e-9, t
        for k in before:
            got, want = getattr(dev, k).cpu().numpy(), np.array(getattr(host, k))
            if got.dtype.kind == 'f':
                assert np.abs(got - want).max() < 1e-9, (t, k)
            else:
                assert np.array_equal(got, want), (t, k)
            assert np.array_equal(want[~stepping], before[k][~stepping]), (t, k)     # masked-out instances did not move
        n_abort += int(ah.sum())
        n_fail += int((np.array(host.fails) > 0).sum())
        # a crude plant keeps the states moving: apply the control on the double integrator, with a kick now and then; the
        # first six instances are pushed outside the velocity limits for good after a few steps (their state test fails at
        # node 0, step after step: the reject and abort branches)
        x = x + par.dt * np.hstack([x[:, 6:], uh])
        if t % 5 == 4:
            x[:, 6:] += rng.normal(scale=0.5, size=(B, 6))
        if t >= 2:
            x[:max(B // 4, 1), 6] = 1.5 * host.problem.x_max[6]
    if name in ('stwa', 'htwa', 'receding', 'real_receding', 'constraint_everywhere'):
        assert n_fail > 0                                                            # the reject branches were exercised
    if name in ('stwa', 'htwa', 'receding', 'real_receding'):
        assert n_abort > 0


@pytest.mark.parametrize('name', ['st', 'constraint_everywhere', 'htwa', 'receding', 'real_receding'])
def test_policy_step_kernels_equal_scalar_oracle(name):
    """smpc_policy_step (kernels_policy.hpp) against oracle/policy_oracle.py -- the scalar, one-instance
    restatement of controller.py:274-284, 369-388, 448-498, 524-565, 651-661 that shares no code with the product -- step by
    step on kicked states, the oracle's numerics being the engine's own host path (one instance per call)."""
    import torch
    from oracle import policy_oracle as po
    from policy_numerics import SolverNumerics
    from safe_mpc_amd import controller as C
    from safe_mpc_amd.parser import Parameters
    from safe_mpc_amd.solver import BatchedOcpSolver
    par = Parameters({}, 'z1')
    par.nq, par.n_dof_safe_set, par.net_size, par.N = 6, 6, [12, 256, 1], 8
    N, B = 8, 12
    dev = C.get_controller(name, par, B, device_state=True)
    x0 = sample_instances(dev.problem, B, seed=3, vel_scale=0.4)
    xg, ug = np.repeat(x0[:, None, :], N + 1, axis=1), np.zeros((B, N, 6))
    dev.setGuess(xg, ug)
    host_solver = BatchedOcpSolver(dev.problem, dev.net)
    insts, nums = [], []
    for b in range(B):
        inst = po.PolicyInstance(name, N, dev.nx, dev.nu, abort_flag=bool(par.abort_flag))
        inst.set_guess(xg[b], ug[b])
        inst.reset()
        insts.append(inst)
        nums.append(SolverNumerics(host_solver, dev.problem, par))
    rng = np.random.default_rng(0)
    x = x0.copy()
    n_abort = n_fail = 0
    for t in range(2 * N + 4):
        ud, ad = dev.step_on_device(torch.tensor(x, device='cuda'))
        dev.ocp_solver.sync()
        ud, ad = ud.cpu().numpy(), ad.cpu().numpy()
        for b in range(B):
            uo, ao = po.step(insts[b], nums[b], x[b])
            assert bool(ad[b]) == ao, (t, b)
            # (the oracle integrates its guess in numpy, the engine in a kernel: rounding-level differences in the QP's data, which
            #  the kicked, partly infeasible problems of this test amplify to ~1e-5 in single controls of size 1 next to others
            #  of size 1e2..1e3 -- the automaton's integers below are compared exactly)
            tol_u = 1e-4 * (1 + np.abs(uo).max())     # (= the RTI parity tolerance with the fp32 network in the loop)
            assert np.abs(ud[b] - uo).max() < tol_u, (t, b)
            assert int(dev.fails[b]) == insts[b].fails and int(dev.current_step[b]) == insts[b].current_step, (t, b)
            assert np.abs(dev.x_guess[b].cpu().numpy() - np.array(insts[b].x_guess)).max() < 1e-4, (t, b)
            ug_o = np.array(insts[b].u_guess)
            assert np.abs(dev.u_guess[b].cpu().numpy() - ug_o).max() < 1e-4 * (1 + np.abs(ug_o).max()), (t, b)
            if hasattr(dev, 'r'):
                assert int(dev.r[b]) == insts[b].r, (t, b)
            if dev.can_abort:
                assert np.abs(dev.x_viable[b].cpu().numpy() - insts[b].x_viable).max() < 1e-4, (t, b)
            n_abort += int(ao)
            n_fail += int(insts[b].fails > 0)
        x = x + par.dt * np.hstack([x[:, 6:], ud])
        if t % 5 == 4:
            x[:, 6:] += rng.normal(scale=0.5, size=(B, 6))
        if t >= 2:
            x[:max(B // 4, 1), 6] = 1.5 * dev.problem.x_max[6]       # pushed outside the velocity limits: reject / abort branches
    if name != 'st':
        assert n_fail > 0
    if dev.can_abort:
        assert n_abort > 0


@pytest.mark.parametrize('name', ['st', 'htwa', 'receding'])
def test_policy_step_reference_trajectory_advances_with_the_step(name):
    """smpc_policy_state.traj -- p[b][i][0:3] = traj[:, current_step[b] + i] before every solve
    (controller.py:153-156, cost_definition.py:30-31) -- on the device against the scalar oracle carrying the same moving
    trajectory; an instance that aborts does not advance its step and sees the same columns again."""
    import torch
    from oracle import policy_oracle as po
    from policy_numerics import SolverNumerics
    from safe_mpc_amd import controller as C
    from safe_mpc_amd.parser import Parameters
    from safe_mpc_amd.solver import BatchedOcpSolver
    par = Parameters({}, 'z1')
    par.nq, par.n_dof_safe_set, par.net_size, par.N = 6, 6, [12, 256, 1], 8
    N, B, steps = 8, 10, 20
    dev = C.get_controller(name, par, B, device_state=True)
    x0 = sample_instances(dev.problem, B, seed=3, vel_scale=0.3)
    xg, ug = np.repeat(x0[:, None, :], N + 1, axis=1), np.zeros((B, N, 6))
    dev.setGuess(xg, ug)
    t_ = np.arange(steps + 1 + N) * 0.15
    traj = np.asarray(dev.problem.ee_ref, float)[:, None] + 0.05 * np.vstack([np.cos(t_) - 1.0, np.sin(t_), 0.5 * np.sin(2 * t_)])
    dev.setTrajectory(traj)
    host_solver = BatchedOcpSolver(dev.problem, dev.net)
    insts, nums = [], []
    for b in range(B):
        inst = po.PolicyInstance(name, N, dev.nx, dev.nu, abort_flag=bool(par.abort_flag))
        inst.set_guess(xg[b], ug[b])
        inst.reset()
        inst.traj = traj
        insts.append(inst)
        nums.append(SolverNumerics(host_solver, dev.problem, par))
    x = x0.copy()
    n_abort = 0
    for t in range(steps):
        cs = [inst.current_step for inst in insts]
        ud, ad = dev.step_on_device(torch.tensor(x, device='cuda'))
        dev.ocp_solver.sync()
        ud, ad, pd = ud.cpu().numpy(), ad.cpu().numpy(), dev.p.cpu().numpy()
        for b in range(B):
            assert np.array_equal(pd[b, :, :3], traj[:, cs[b]:cs[b] + N + 1].T), (t, b)      # the columns of THIS solve
            uo, ao = po.step(insts[b], nums[b], x[b])
            assert bool(ad[b]) == ao, (t, b)
            assert np.abs(ud[b] - uo).max() < 1e-4 * (1 + np.abs(uo).max()), (t, b)
            assert int(dev.current_step[b]) == insts[b].current_step, (t, b)
            n_abort += int(ao)
        x = x + par.dt * np.hstack([x[:, 6:], ud])
        if t >= 2:
            x[:max(B // 4, 1), 6] = 1.5 * dev.problem.x_max[6]       # outside the velocity limits: reject / abort branches
    if dev.can_abort:
        assert n_abort > 0
    # traj = NULL leaves p[:, :, 0:3] alone (the constant ee_ref of the in-scope costs)
    dev.setTrajectory(None)
    before = dev.p.clone()
    dev.step_on_device(torch.tensor(x, device='cuda'))
    dev.ocp_solver.sync()
    assert torch.equal(dev.p[:, :, :3], before[:, :, :3])


@pytest.mark.parametrize('name', ['htwa', 'receding'])
def test_device_policy_loop_equals_scalar_oracle_loop(name):
    """... and the whole closed loop with all state in HBM (run_mpc(on_device=True): smpc_loop_pre / smpc_policy_step /
    smpc_loop_classify_aborts / smpc_loop_apply_backup / smpc_loop_post) against oracle/policy_oracle.py::run_closed_loop
    (scripts/mpc.py:118-287 restated per instance): same abort events, receding indices, NaN patterns of the logs and
    outcome lists; trajectories to the tolerance the zero-cost backup OCP allows."""
    from oracle import policy_oracle as po
    from policy_numerics import SolverNumerics
    from safe_mpc_amd import closed_loop as cl
    from safe_mpc_amd import controller as C
    from safe_mpc_amd.parser import Parameters
    from safe_mpc_amd.solver import BatchedOcpSolver
    par = Parameters({}, 'z1')
    par.nq, par.n_dof_safe_set, par.net_size, par.N, par.back_hor = 6, 6, [12, 256, 1], 10, 12
    prob0 = C.OcpProblem(par, 'htwa', 'ext', N=10)
    B, n_steps, cn = 40, 30, 1.0
    x0 = sample_instances(prob0, B, seed=9, vel_scale=0.3)       # moving starts: some instances will have to abort
    xg, ug = np.repeat(x0[:, None, :], 11, axis=1), np.zeros((B, 10, 6))
    dev = cl.run_mpc(par, name, xg, ug, n_steps=n_steps, control_noise=cn, on_device=True, groups=1)
    ctrl = C.get_controller(name, par, 1)
    backup = C.SafeBackupController(par, 1)
    outs = []
    for b in range(B):
        tau_noise = np.random.default_rng(b).normal(np.zeros(6), ctrl.problem.tau_max * cn / 100, 6)     # mpc.py:126, env_model.py:196
        num = SolverNumerics(ctrl.ocp_solver, ctrl.problem, par, backup.ocp_solver, backup.problem, tau_noise=tau_noise)
        inst = po.PolicyInstance(name, par.N, ctrl.nx, ctrl.nu, abort_flag=bool(par.abort_flag))
        outs.append(po.run_closed_loop(inst, num, xg[b], ug[b], n_steps, backup.N, ctrl.nq, on_step=num.on_step))
    xo, uo = np.array([r['x'] for r in outs]), np.array([r['u'] for r in outs])
    assert np.array_equal(np.isnan(dev['x']), np.isnan(xo)) and np.array_equal(np.isnan(dev['u']), np.isnan(uo))
    conv, coll, viable, unconv = po.outcome_lists(outs)
    assert (dev['conv_idx'], dev['collisions_idx'], sorted(dev['viable_idx']), dev['unconv_idx']) == (conv, coll, sorted(viable), unconv)
    ev = [(b, j, xv) for b, r in enumerate(outs) for (j, xv) in r['events']]
    assert dev['x_viable'].shape[0] == len(ev)
    if name == 'receding':
        assert len(ev) > 0                       # (htwa needs N - 1 failures in a row: rare with a real solver; scripted on the CPU)
    if ev:
        assert np.abs(dev['x_viable'] - np.array([e[2] for e in ev])).max() < 1e-5
    if name == 'receding':
        assert np.array_equal(dev['r_receding'][:, :, 0], np.array([r['r'] for r in outs]))
    assert np.nanmax(np.abs(dev['x'] - xo)) < 1e-4 and np.nanmax(np.abs(dev['u'] - uo)) < 2e-3 * (1 + np.nanmax(np.abs(uo)))


def test_device_policy_loop_at_bench_size_invariants():
    """The receding policy with all state in HBM at the bench's batch size (4096 instances, N = 30, two pipelined groups, graph
    replay, asynchronous backup solves): size-independent properties of the result the reference's script would pickle."""
    import bench
    from safe_mpc_amd import closed_loop as cl
    from safe_mpc_amd.solver import BatchedOcpSolver
    par, prob, net = bench.build_problem()
    par.back_hor = 30
    B, N, steps = 4096, prob.N, 24
    s = BatchedOcpSolver(prob, net)
    x0 = bench.initial_states(s, prob, B, 0)
    xg, ug = np.repeat(x0[:, None, :], N + 1, axis=1), np.zeros((B, N, prob.nu))
    res = cl.run_mpc(par, 'receding', xg, ug, n_steps=steps, on_device=True)
    x, u, r = res['x'], res['u'], res['r_receding'][:, :, 0]
    assert x.shape == (B, steps + 1, prob.nx) and u.shape == (B, steps, prob.nu)
    # the four outcome lists partition the instances (mpc.py:273-286)
    lists = [res[k] for k in ('conv_idx', 'collisions_idx', 'viable_idx', 'unconv_idx')]
    assert sorted(i for l in lists for i in l) == list(range(B))
    # logs: an instance's rows are valid up to the step it was lost at and NaN afterwards, inputs one row shorter
    xnan, unan = np.isnan(x).any(2), np.isnan(u).any(2)
    assert not xnan[:, 0].any()
    assert (np.diff(xnan.astype(int), axis=1) >= 0).all() and (np.diff(unan.astype(int), axis=1) >= 0).all()
    lost = xnan.any(1) | unan.any(1)
    assert set(np.where(lost)[0]) <= set(res['collisions_idx'])
    # receding index: -1 exactly where the instance did not step its controller, otherwise inside the horizon
    assert ((r == -1) | ((r >= 1) & (r <= N))).all() and (r[:, 0] == N).all()
    # every abort event recorded a viable state: one row each, inside the model bounds
    assert len(res['x_viable']) >= len(res['viable_idx'])
    if len(res['x_viable']):
        assert (res['x_viable'] >= prob.x_min - 1e-6).all() and (res['x_viable'] <= prob.x_max + 1e-6).all()
    # applied controls of live, stepping instances respect the torque bounds of the OCP to solver tolerance (naive check on u:
    # finite and bounded by the largest PD / backup control seen in the reference's loop)
    assert np.isfinite(u[~unan]).all()


def test_policy_entry_points_reject_misuse():
    """API misuse of the policy entry points comes back as a negative code with text, never as a launch on bad pointers."""
    import ctypes as C
    import torch
    from safe_mpc_amd import _lib
    from safe_mpc_amd import controller as Cn
    from safe_mpc_amd.parser import Parameters
    par = Parameters({}, 'z1')
    par.nq, par.n_dof_safe_set, par.net_size, par.N = 6, 6, [12, 256, 1], 6
    ctrl = Cn.get_controller('receding', par, 4, device_state=True)
    sv, L = ctrl.ocp_solver, ctrl.ocp_solver.L
    x = torch.zeros((4, 12), dtype=torch.float64, device='cuda')
    ptr = lambda t: t.data_ptr()
    pp = sv._policy_params(ctrl.policy_kind, True)
    full = [ptr(ctrl.x_guess), ptr(ctrl.u_guess), ptr(ctrl.x_temp), ptr(ctrl.u_temp), ptr(ctrl.p), ptr(ctrl.x_viable), ptr(ctrl.fails),
            ptr(ctrl.current_step), ptr(ctrl.r), ptr(ctrl.last_status), ptr(ctrl.qp_iter)]
    call = lambda pp_, st_, step=None, uo=None: L.smpc_policy_step(sv.h, 4, C.byref(pp_), C.byref(st_), ptr(x), step, uo, ptr(ctrl._u_out),
                                                                   ptr(ctrl._abort_out), ptr(ctrl._any_abort))
    no_r = list(full); no_r[8] = None
    assert call(pp, _lib.PolicyState(*no_r)) < 0 and b'without r' in L.smpc_last_error(sv.h)
    no_guess = list(full); no_guess[0] = None
    assert call(pp, _lib.PolicyState(*no_guess)) < 0 and b'incomplete' in L.smpc_last_error(sv.h)
    bad = sv._policy_params(17, True)
    assert call(bad, _lib.PolicyState(*full)) < 0 and b'unknown policy' in L.smpc_last_error(sv.h)
    mask = torch.ones(4, dtype=torch.bool, device='cuda')
    assert call(pp, _lib.PolicyState(*full), step=ptr(mask), uo=None) < 0 and b'u_other' in L.smpc_last_error(sv.h)
    rr = sv._policy_params(4, True)                          # RealReceding without its stage bounds
    assert call(rr, _lib.PolicyState(*full)) < 0 and b'stage_lo' in L.smpc_last_error(sv.h)
    assert L.smpc_loop_pre(sv.h, 4, 5, None, None, None, None, None) < 0
    assert call(pp, _lib.PolicyState(*full)) == 0            # and the well-formed call still goes through
    sv.sync()


@pytest.mark.parametrize('controller', ['st', 'constraint_everywhere'])
def test_engine_against_independent_dense_qp_solver_at_full_horizon(controller, qp_mode):
    """The engine's RTI step at the bench's size (Z1, N = 30) against tests/qp_ref.py -- a condensed dense QP solved by a plain
    log-barrier Newton method with numpy.linalg: no Riccati recursion, no Mehrotra corrector, different variables.  The QP data
    come from the oracle's linearisation (which the engine matches to 1e-14, test_eval_nodes_parity); what is pinned here is
    the QP solution itself, independently of the oracle's interior-point method."""
    from qp_ref import condense, solve_condensed
    par, prob, net = make_problem(controller, 'ext', N=30)
    s, o = _solver(prob, net), _oracle(prob, net)
    x0 = sample_instances(prob, 4, seed=5, vel_scale=0.2)
    xg, ug, p = constant_guess(prob, x0)
    rng = np.random.default_rng(1)
    ug += rng.uniform(-2, 2, ug.shape)
    xg[:, 1:] += 0.01 * rng.standard_normal(xg[:, 1:].shape)
    xa, ua, sa, ia = s.solve(x0 + 0.002, xg, ug, p)
    assert (sa == 0).sum() >= 3
    for b in range(4):
        if sa[b] != 0:
            continue
        cq = condense(o.build_qp(x0[b] + 0.002, xg[b], ug[b], p[b]), 30, 6, par.dt)
        v, _, _, nit = solve_condensed(cq)
        assert nit < 150
        du = (ua[b] - ug[b]).reshape(-1)
        assert np.abs(du - v).max() < 2e-6 * (1.0 + np.abs(v).max()), (controller, b, np.abs(du - v).max())
        assert np.allclose(xa[b, 30] - xg[b, 30], cq['Phi'][30] @ v + cq['c'][30], atol=1e-6)


@pytest.mark.parametrize('case', ['st', 'constraint_everywhere', 'receding', 'fr7'])
def test_late_closed_loop_qps_against_independent_dense_solver(case, qp_mode):
    """the solver-independent cross-check on QPs taken from the RUNNING closed loop of the engine
    itself, not only on cold starts -- Z1 'st' and 'constraint_everywhere' (steps 40, 100), 'receding' with its switched running
    row (the row on at ONE running node that recedes with the step, controller.py:452-469), and BASELINE config 4's 7-DoF / N = 40
    problem (steps 20, 40).  Late QPs are soft: the stage Hessian's smallest eigenvalues are LM x dt = 2.5e-3, so an exit at mean
    complementarity 1e-8 (HPIPM's level, config.yaml:15-18) bounds the OBJECTIVE gap (duality gap <= m x 1e-8) but leaves single
    controls free by up to ~1e-2 along the flat directions -- for this IPM, for the oracle's, and for any other (measured on the
    oracle: tests/experiments/late_qp_crosscheck.py).  Pinned by tests/late_qp.py::run_case for every
    instance of the batch (the slowest by iteration count included):
      (a) engine == oracle on the same late QP at the RTI tolerance (same algorithm, rounding-different paths);
      (b) the engine's step is feasible for the dense QP and its objective is within the duality-gap bound of the dense optimum;
      (c) the measured gap in the controls at the default exit stays below 5e-2 (the softness, stated);
      (d) with the exit tightened to 1e-12 the engine's step converges to the dense solver's optimum: 2e-3 (1 + |v*|).
    (c) and (d) follow the bound the flat directions allow: an objective gap <= m x tol over a Hessian whose smallest eigenvalue is
    LM x dt = 2.5e-3 leaves |dz| <= sqrt(2 m tol / 2.5e-3): ~0.1 at tol = 1e-8 (m ~ 1300 complementarity pairs), ~1e-3 at 1e-12;
    measured over the loops of rounds 3-5: 1e-2 and 2e-6 .. 8e-4 -- which instance shows the largest gap changes with rounding-level
    changes of the linearisation (the builder of round 4 moved it from 1.8e-4 to 8.1e-4)."""
    from late_qp import CASES, run_case
    checked, worst, rows = run_case(case, _solver, _oracle)
    assert checked >= CASES[case][3] * 2 - 8              # (almost) every instance at each of the two steps
    print(f'late QPs [{case}]: {checked} checked; control gap to the dense optimum at the default exit {worst["gap_default"]:.2e}, '
          f'at qp_tol 1e-12 {worst["gap_tight"]:.2e}; relative objective gap {worst["obj"]:.2e}; per step (step, mean it, max it, '
          f'gap default, gap tight, objective): {[tuple(float(f"{v:.3g}") for v in r) for r in rows]}')


def test_engine_against_independent_dense_qp_solver_c4(qp_mode):
    """The same for BASELINE config 4 (7-DoF, N = 40, safe-set row on every node)."""
    from conftest import make_problem_fr7
    from qp_ref import condense, solve_condensed
    par, prob, net = make_problem_fr7(N=40)
    s, o = _solver(prob, net), _oracle(prob, net)
    x0 = sample_instances(prob, 3, seed=2, vel_scale=0.1)
    xg, ug, p = constant_guess(prob, x0, ee_ref=prob.ee_ref)
    rng = np.random.default_rng(0)
    ug += rng.uniform(-1, 1, ug.shape)
    xg[:, 1:] += 0.005 * rng.standard_normal(xg[:, 1:].shape)
    xa, ua, sa, ia = s.solve(x0 + 0.001, xg, ug, p)
    assert (sa == 0).all()
    for b in range(3):
        cq = condense(o.build_qp(x0[b] + 0.001, xg[b], ug[b], p[b]), 40, 7, par.dt)
        v, _, _, nit = solve_condensed(cq)
        du = (ua[b] - ug[b]).reshape(-1)
        # (fp32 network in the engine, fp64 restatement in the oracle's QP data: the row differs by ~1e-7 relative)
        assert np.abs(du - v).max() < 1e-4 * (1.0 + np.abs(v).max()), (b, np.abs(du - v).max())


@pytest.mark.parametrize('nq', [6, 7])
def test_engine_jacobians_by_central_differences_of_its_own_values(nq):
    """Independent of the oracle: every Jacobian the engine's linearisation kernels produce (closed-form RNEA derivatives,
    tangents through the clamped segment-distance expressions, the network's input gradient, the cost gradient) against
    central differences of the engine's OWN values at perturbed states / controls."""
    if nq == 6:
        par, prob, net = make_problem('constraint_everywhere', 'ext', N=4)
    else:
        from conftest import make_problem_fr7
        par, prob, net = make_problem_fr7(N=4)
    s = _solver(prob, net)
    B, N, nx = 6, 4, 2 * nq
    x0 = sample_instances(prob, B, seed=4, vel_scale=0.4)
    xg, ug, p = constant_guess(prob, x0) if nq == 6 else constant_guess(prob, x0, ee_ref=prob.ee_ref)
    rng = np.random.default_rng(2)
    xg = xg + 0.05 * rng.standard_normal(xg.shape)
    ug = ug + rng.uniform(-3, 3, ug.shape)
    base = s.eval_nodes(xg, ug, p)
    nr = prob.desc.n_rows
    h = 1e-6

    def shifted(arr, idx, sign, step=None):
        a = arr.copy()
        a[..., idx] += sign * (h if step is None else step)
        return a
    # d tau / dq, d tau / dqd, rows, network, cost: central differences in every state coordinate
    d_tau = np.zeros((B, N + 1, nq, nx)); d_row = np.zeros((B, N + 1, nr, nx)); d_nn = np.zeros((B, N + 1, nx)); d_cost = np.zeros((B, N + 1, nq))
    d_grad = np.zeros((B, N + 1, nq, nq))
    for i in range(nx):
        ep, em = s.eval_nodes(shifted(xg, i, +1), ug, p), s.eval_nodes(shifted(xg, i, -1), ug, p)
        d_tau[..., i] = (ep['tau'][..., :nq] - em['tau'][..., :nq]) / (2 * h)
        d_row[..., i] = (ep['row_val'][..., :nr] - em['row_val'][..., :nr]) / (2 * h)
        # (the network runs in fp32: its value resolves a difference only over a much wider step)
        hn = 4e-3
        d_nn[..., i] = (s.eval_nodes(shifted(xg, i, +1, hn), ug, p)['nn_val'] - s.eval_nodes(shifted(xg, i, -1, hn), ug, p)['nn_val']) / (2 * hn)
        if i < nq:
            # cost value is not exported; its gradient is Q d|ee - ref|^2 / dq = 2 Q J^T (ee - ref): differentiate ee instead
            de = (ep['ee'] - em['ee']) / (2 * h)                                     # [B, N+1, 3] = column i of J
            d_cost[..., i] = 2.0 * prob.desc.Q * (de * (base['ee'] - p[:, :, :3])).sum(-1)
            d_grad[..., i] = (ep['cost_grad_q'][..., :nq] - em['cost_grad_q'][..., :nq]) / (2 * h)
    M_fd = np.zeros((B, N + 1, nq, nq))
    for i in range(nq):
        ep, em = s.eval_nodes(xg, shifted(ug, i, +1), p), s.eval_nodes(xg, shifted(ug, i, -1), p)
        M_fd[..., i] = (ep['tau'][..., :nq] - em['tau'][..., :nq]) / (2 * h)
    run = slice(0, N)                                                                # the torque row lives on nodes 0 .. N-1
    J = lambda f: base[f][:, run, :nq * nq].reshape(B, N, nq, nq)
    scale = 1.0 + np.abs(base['tau'][:, run, :nq]).max()
    assert np.abs(J('dtau_dq') - d_tau[:, run, :, :nq]).max() < 2e-5 * scale
    assert np.abs(J('dtau_dv') - d_tau[:, run, :, nq:]).max() < 2e-5 * scale
    assert np.abs(J('M') - M_fd[:, run]).max() < 2e-5 * scale
    rg = base['row_grad'][..., :nr * nq].reshape(B, N + 1, nr, nq)
    assert np.abs(rg - d_row[..., :nq]).max() < 1e-5 * (1.0 + np.abs(rg).max()) and np.abs(d_row[..., nq:]).max() < 1e-8
    assert np.abs(base['cost_grad_q'][..., :nq] - d_cost).max() < 1e-5 * (1.0 + np.abs(d_cost).max())
    if prob.desc.hessian == 1:                                                       # SMPC_HESS_EXACT: the true second derivative
        Hq = base['cost_hess_qq'][..., :nq * nq].reshape(B, N + 1, nq, nq)
        assert np.abs(Hq - d_grad).max() < 1e-5 * (1.0 + np.abs(Hq).max())
    ng = base['nn_grad'][:, 1:, :]                                                   # (fp32 network: differences of fp32 values)
    g_fd = d_nn[:, 1:]
    assert np.abs(np.concatenate([ng[..., :nq], ng[..., nq:2 * nq]], -1) - g_fd).max() < 2e-2 * (1.0 + np.abs(g_fd).max())


def test_engine_inverse_dynamics_known_answer_double_pendulum():
    """First principles, no oracle: a planar 2R arm (both axes y, point masses at the link tips) embedded as the first two joints
    of a 5-joint chain whose other links are massless.  The engine's torque row, mass matrix and Jacobians against the textbook
    M(q) qdd + C(q, qd) + g(q) and its derivatives."""
    G = 9.80665
    par, prob, net = make_problem('naive', 'ext', N=3, nq=5)
    m1, m2, l1, l2 = 0.9, 0.6, 0.5, 0.4
    for i in range(5):
        J = prob.desc.joints[i]
        J.R0[:] = np.eye(3).reshape(-1).tolist()
        J.p0[:] = [0.0, 0.0, 0.0]
        J.axis[:] = [0.0, 1.0, 0.0]
        J.mass = 0.0
        J.com[:] = [0.0, 0.0, 0.0]
        J.inertia[:] = [0.0] * 6
        J.tau_max = 1e3
    for i, (m, l, p0) in enumerate([(m1, l1, [0, 0, 0]), (m2, l2, [l1, 0, 0])]):
        J = prob.desc.joints[i]
        J.p0[:] = [float(v) for v in p0]
        J.mass = m
        J.com[:] = [l, 0.0, 0.0]
    prob.desc.gravity[:] = [0.0, 0.0, -G]
    s = _solver(prob, None)
    rng = np.random.default_rng(3)
    B, N = 8, 3
    xg = rng.uniform(-2, 2, (B, N + 1, 10))
    ug = rng.uniform(-3, 3, (B, N, 5))
    p = np.zeros((B, N + 1, 5)); p[:, :, 4] = 1.0
    ev = s.eval_nodes(xg, ug, p)

    def textbook(q, qd, qdd):
        c2, s2 = np.cos(q[1]), np.sin(q[1])
        M = np.array([[m1 * l1 ** 2 + m2 * (l1 ** 2 + l2 ** 2 + 2 * l1 * l2 * c2), m2 * (l2 ** 2 + l1 * l2 * c2)],
                      [m2 * (l2 ** 2 + l1 * l2 * c2), m2 * l2 ** 2]])
        h = m2 * l1 * l2 * s2
        Cv = np.array([-h * (2 * qd[0] * qd[1] + qd[1] ** 2), h * qd[0] ** 2])
        g = -G * np.array([(m1 + m2) * l1 * np.cos(q[0]) + m2 * l2 * np.cos(q[0] + q[1]), m2 * l2 * np.cos(q[0] + q[1])])
        return M, Cv, g, M @ qdd + Cv + g
    for b in range(B):
        for k in range(N):
            q, qd, qdd = xg[b, k, :2], xg[b, k, 5:7], ug[b, k, :2]
            M, Cv, g, tau = textbook(q, qd, qdd)
            assert np.allclose(ev['tau'][b, k, :2], tau, atol=1e-11) and np.allclose(ev['tau'][b, k, 2:5], 0.0, atol=1e-12)
            Me = ev['M'][b, k, :25].reshape(5, 5)
            assert np.allclose(Me[:2, :2], M, atol=1e-11) and np.allclose(Me[2:], 0.0, atol=1e-12)
            # d tau / d qd of the textbook Coriolis terms
            h = m2 * l1 * l2 * np.sin(q[1])
            dv = np.array([[-2 * h * qd[1], -2 * h * (qd[0] + qd[1])], [2 * h * qd[0], 0.0]])
            assert np.allclose(ev['dtau_dv'][b, k, :25].reshape(5, 5)[:2, :2], dv, atol=1e-11)
            # d tau / dq by differencing the textbook expression
            dq = np.zeros((2, 2))
            for j in range(2):
                e = np.zeros(2); e[j] = 1e-6
                dq[:, j] = (textbook(q + e, qd, qdd)[3] - textbook(q - e, qd, qdd)[3]) / 2e-6
            assert np.allclose(ev['dtau_dq'][b, k, :25].reshape(5, 5)[:2, :2], dq, atol=1e-7)


def test_engine_safe_set_row_against_torch_autograd():
    """Oracle-free pin of the MFMA network kernels and the chain rule back to the state: the engine's safe-set row value and
    gradient at every node against safe_set.py:82-94 restated in torch (float64 copy of the network, autograd)."""
    import torch
    par, prob, net = make_problem('constraint_everywhere', 'ext', N=5)
    s = _solver(prob, net)
    rng = np.random.default_rng(7)
    B, N = 12, 5
    xg = np.concatenate([rng.uniform(prob.lbx[:6], prob.ubx[:6], (B, N + 1, 6)), rng.uniform(-1, 1, (B, N + 1, 6))], -1)
    ug = np.zeros((B, N, 6))
    p = np.zeros((B, N + 1, 5)); p[:, :, :3], p[:, :, 3], p[:, :, 4] = prob.ee_ref, par.alpha, 1.0
    ev = s.eval_nodes(xg, ug, p)
    net64 = net.model.double()
    try:
        mean, std = torch.tensor(net.mean), torch.tensor(net.std)
        worst_v = worst_g = 0.0
        for b in range(B):
            for k in range(1, N + 1):
                xt = torch.tensor(xg[b, k], dtype=torch.float64, requires_grad=True)
                xc = xt + torch.nn.functional.one_hot(torch.tensor(6), 12).double() * par.eps
                vn = torch.linalg.norm(xc[6:])
                g = net64(torch.cat([(xc[:6] - mean) / std, xc[6:] / vn]))[0] * (100 - par.alpha) / 100 - vn
                g.backward()
                worst_v = max(worst_v, abs(ev['nn_val'][b, k] - g.item()) / (1.0 + abs(g.item())))
                worst_g = max(worst_g, np.abs(ev['nn_grad'][b, k, :12] - xt.grad.numpy()).max() / (1.0 + np.abs(xt.grad.numpy()).max()))
        assert worst_v < 2e-5 and worst_g < 5e-4, (worst_v, worst_g)
    finally:
        net.model.float()


def test_engine_collision_rows_against_brute_force_geometry():
    """Oracle-free: the engine's collision-row values against the geometry done by hand -- forward kinematics as a product of
    the URDF's transforms in numpy, then the squared distance between the two capsule axes by brute force over a fine grid
    (the reference's expression, utils.py:94-113, is that distance up to its 1e-5 regulariser, never below it)."""
    from safe_mpc_amd.urdf import _axis_angle
    par, prob, net = make_problem('naive', 'ext', N=2)
    s = _solver(prob, None)
    rng = np.random.default_rng(5)
    B, N = 10, 2
    q = rng.uniform(prob.lbx[:6], prob.ubx[:6], (B, 6))
    xg = np.tile(np.concatenate([q, np.zeros((B, 6))], 1)[:, None, :], (1, N + 1, 1))
    ev = s.eval_nodes(xg, np.zeros((B, N, 6)), np.zeros((B, N + 1, 5)))

    def world_point(qb, pt):
        R, pw = np.eye(3), np.zeros(3)
        for i, j in enumerate(prob.chain.joints[:pt.link + 1]):
            pw = pw + R @ j.p0
            R = R @ j.R0 @ _axis_angle(j.axis, qb[i])
        return pw + R @ np.array(pt.local)
    t = np.linspace(0, 1, 300)
    checked = 0
    for b in range(B):
        for r in range(prob.desc.n_rows):
            row = prob.desc.rows[r]
            if row.kind not in (0, 1):                       # SEG_FIXEDSEG / SEG_SEG: the capsule pairs of config.yaml:205-216
                continue
            A, Bp = world_point(q[b], prob.desc.points[row.pa]), world_point(q[b], prob.desc.points[row.pb])
            if row.kind == 0:
                Cc, Dd = np.array(row.C), np.array(row.D)
            else:
                Cc, Dd = world_point(q[b], prob.desc.points[row.pc]), world_point(q[b], prob.desc.points[row.pd])
            P = A[None] + t[:, None] * (Bp - A)[None]
            Qp = Cc[None] + t[:, None] * (Dd - Cc)[None]
            bf = np.min(np.sum((P[:, None, :] - Qp[None, :, :]) ** 2, axis=-1))
            assert bf - 1e-4 <= ev['row_val'][b, 1, r] <= bf + 5e-3, (b, r, bf, ev['row_val'][b, 1, r])
            checked += 1
    assert checked >= 30


def test_engine_plant_step_is_consistent_with_its_inverse_dynamics():
    """AdamModel.integrate (env_model.py:192-206) restated through the engine's own pieces: the acceleration the plant step
    applies, pushed back through the torque row, must give the clipped commanded torque; then the double integrator."""
    par, prob, net = make_problem('naive', 'ext', N=1)
    s = _solver(prob, None)
    rng = np.random.default_rng(11)
    B = 32
    x = np.concatenate([rng.uniform(prob.lbx[:6], prob.ubx[:6], (B, 6)), rng.uniform(-1, 1, (B, 6))], 1)
    u = rng.uniform(-1, 1, (B, 6)) * np.where(rng.random((B, 1)) < 0.5, 4.0, 600.0)       # half of them saturate the torques
    noise = rng.normal(scale=0.3, size=(B, 6))
    xn, acc = s.plant_step(x, u, None, noise)
    tau_of = lambda a: s.eval_nodes(np.stack([x, x], 1), a[:, None, :], np.zeros((B, 2, 5)))['tau'][:, 0, :6]
    tau_cmd = np.clip(tau_of(u) + noise, -prob.tau_max, prob.tau_max)
    assert (np.abs(tau_of(u) + noise) > prob.tau_max).any()                                 # the clip was exercised
    assert np.abs(tau_of(acc) - tau_cmd).max() < 1e-9 * (1.0 + np.abs(tau_cmd).max())
    dt = par.dt
    assert np.allclose(xn[:, :6], x[:, :6] + dt * x[:, 6:] + 0.5 * dt * dt * acc, atol=1e-13)
    assert np.allclose(xn[:, 6:], x[:, 6:] + dt * acc, atol=1e-13)


def test_generate_guess_merit_backtracking_on_engine():
    """guess generation = SQP with merit backtracking (parser.py:115-117,139; guess_acados.py:98-158) on the
    engine: accepted guesses satisfy checkGuess, the l1 merit never increases along accepted steps, and the hard-terminal
    safe-set OCP ('htwa', what every safe-set controller's warm start is generated with) ends feasible."""
    from safe_mpc_amd import closed_loop as cl
    from safe_mpc_amd import controller as C
    from safe_mpc_amd.parser import Parameters
    par = Parameters({}, 'z1')
    par.nq, par.n_dof_safe_set, par.net_size, par.N, par.nlp_max_iter = 6, 6, [12, 256, 1], 20, 200
    hist = []
    guess, good = cl.generate_guess(par, 'htwa', 48, history=hist)
    assert good.sum() >= 24 and guess['xg'].shape == (good.sum(), 21, 12)
    for h in hist:
        up = h['updated'] & (h['alpha'] > 0.05)
        assert np.all(h['merit'][up] <= h['merit_before'][up] + 1e-9 * (1 + np.abs(h['merit_before'][up])))
    assert np.all(hist[-1]['violation'][good] < 1e-5)
    # the accepted guesses pass the reference's acceptance test when re-checked from scratch
    ctrl = C.get_controller('htwa', par, int(good.sum()))
    ctrl.x_temp, ctrl.u_temp = guess['xg'].copy(), guess['ug'].copy()
    assert np.all(ctrl.checkGuess())


def test_generate_guess_engine_matches_oracle_double():
    """guess generation (guess_acados.py:98-158: SQP with merit backtracking to
    convergence, then checkGuess) run twice from the same 48 Halton starts -- once on the HIP engine, once on the CPU oracle
    behind the same policy-layer code.  Same accepted set; warm starts equal within 1e-4 (1 + |.|inf) -- or, where the fp32
    network's rounding tipped an Armijo test and the two SQP paths parted, the same final merit within 1e-6 relative (the
    two then sit at the same local solution of the OCP) and checkGuess on both."""
    from fake_solver import make_double_controller
    from safe_mpc_amd import closed_loop as cl
    from safe_mpc_amd.parser import Parameters
    par = Parameters({}, 'z1')
    par.nq, par.n_dof_safe_set, par.net_size, par.N, par.nlp_max_iter = 6, 6, [12, 256, 1], 20, 200
    he, hd = [], []
    ge, good_e = cl.generate_guess(par, 'htwa', 48, history=he)
    gd, good_d = cl.generate_guess(par, 'htwa', 48, make_controller=lambda n, b: make_double_controller(n, par, b), history=hd)
    assert np.array_equal(good_e, good_d), (np.where(good_e)[0], np.where(good_d)[0])
    assert good_e.sum() >= 24
    xe, ue, xd, ud = ge['xg'], ge['ug'], gd['xg'], gd['ug']
    ex = np.abs(xe - xd).reshape(len(xe), -1).max(1) / (1.0 + np.abs(xd).reshape(len(xd), -1).max(1))
    eu = np.abs(ue - ud).reshape(len(ue), -1).max(1) / (1.0 + np.abs(ud).reshape(len(ud), -1).max(1))
    close = (ex < 1e-4) & (eu < 1e-4)
    me, md = he[-1]['merit'][good_e], hd[-1]['merit'][good_d]
    same_merit = np.abs(me - md) <= 1e-6 * (1.0 + np.abs(md))
    assert np.all(close | same_merit), (ex.max(), eu.max(), np.abs(me - md).max())
    assert close.mean() >= 0.9, close.mean()                     # parting ways is the exception
    assert np.all(he[-1]['violation'][good_e] < 1e-5) and np.all(hd[-1]['violation'][good_d] < 1e-5)


def test_rollout_sub_batch_workers_change_nothing(monkeypatch):
    """smpc_rollout_batch splits a large batch into sub-batches on their own streams (worker handles borrowing the network
    weights): instances are independent, so the trajectories are the same bits whatever the split -- host and device pointers,
    per-instance plants and per-step torque noise included."""
    import torch
    from safe_mpc_amd import closed_loop as cl
    par, prob, net = make_problem('st', 'ext', N=12)
    s = _solver(prob, net)
    B, n = 50, 5
    x0 = sample_instances(prob, B, seed=21, vel_scale=0.1)
    xg, ug, p = constant_guess(prob, x0)
    noise = 0.05 * np.random.default_rng(4).standard_normal((n, B, 6))
    jt = cl.perturbed_joint_tables(par, 6, 5.0, np.arange(B))
    monkeypatch.setenv('SMPC_ROLLOUT_STREAMS', '1')
    ref = s.rollout(x0, xg, ug, p, n, joints_noisy=jt, tau_noise=noise)
    for streams in ('3', '7'):
        monkeypatch.setenv('SMPC_ROLLOUT_STREAMS', streams)
        got = s.rollout(x0, xg, ug, p, n, joints_noisy=jt, tau_noise=noise)
        for a, b in zip(ref, got):
            assert np.array_equal(a, b), streams
    dev = torch.device('cuda:0')
    t = lambda a: torch.tensor(a, dtype=torch.float64, device=dev)
    xgd, ugd = t(xg), t(ug)
    jtd = torch.tensor(np.ascontiguousarray(jt).view(np.float64).reshape(B, 6, -1), device=dev)
    got = s.rollout(t(x0), xgd, ugd, t(p), n, joints_noisy=jtd, tau_noise=t(noise))
    s.sync()
    for a, b in zip(ref[:3], got[:3]):
        assert np.array_equal(a, b.cpu().numpy())
    assert np.array_equal(ref[4], xgd.cpu().numpy())


def test_entry_scripts_end_to_end(tmp_path, monkeypatch):
    """The reference's two live entry points, same flags and file names: scripts/guess_acados.py writes the
    warm-start pickle {'xg','ug'} that scripts/mpc.py loads (mpc.py:79-84); mpc.py runs the closed loop with all state on the
    device and writes the result pickle (mpc.py:307-315); its exit code is the number of failed instances (mpc.py:317)."""
    import importlib.util
    import os
    import pickle
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    monkeypatch.setenv('SMPC_DATA_DIR', str(tmp_path))
    monkeypatch.setenv('SMPC_TEST_NUM', '12')
    monkeypatch.setenv('SMPC_N_STEPS', '25')

    def load(name):
        spec = importlib.util.spec_from_file_location(name, os.path.join(root, 'scripts', name + '.py'))
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
        return m
    argv = ['-c', 'htwa', '--horizon', '12', '--alpha', '10']
    assert load('guess_acados').main(argv) == 0
    gfile = [f for f in os.listdir(tmp_path) if f.endswith('_guess.pkl')]
    assert gfile == ['z1_htwa_12hor_10sm_use_netTrue__q_collision_margins_0.0_0.0_guess.pkl']
    g = pickle.load(open(os.path.join(tmp_path, gfile[0]), 'rb'))
    n = g['xg'].shape[0]
    assert 1 <= n <= 12 and g['xg'].shape[1:] == (13, g['xg'].shape[2]) and g['ug'].shape[:2] == (n, 12)
    rc = load('mpc').main(argv)
    rfile = [f for f in os.listdir(tmp_path) if f.endswith('_mpc.pkl')]
    assert rfile == ['z1_htwa_use_netTrue_12hor_10sm_noise_0.0_control_noise0.0_q_collision_margins_0.0_0.0_mpc.pkl']
    res = pickle.load(open(os.path.join(tmp_path, rfile[0]), 'rb'))
    assert set(res) >= {'x', 'u', 'r', 'conv_idx', 'collisions_idx', 'unconv_idx', 'viable_idx', 'x_viable'}
    assert res['x'].shape == (n, 26, g['xg'].shape[2]) and res['u'].shape[:2] == (n, 25)
    assert rc == len(res['collisions_idx'])
    parts = set(res['conv_idx']) | set(res['collisions_idx']) | set(res['unconv_idx']) | set(res['viable_idx'])
    assert parts == set(range(n))


@pytest.mark.parametrize('on_device', [True, False])
def test_run_mpc_reports_the_reference_solver_time_statistics(on_device, capsys):
    """scripts/mpc.py:239 appends controller.getTime() at every step and :300-303 prints the 99 % quantile of
    the seven acados timers.  run_mpc(collect_times=True) on the engine: one row per step and group -- on the device the rows
    come out of the engine's 64-deep event ring, read at least 32 solves late (70 steps: the ring is lapped once) -- with
    time_tot >= time_qp >= time_qp_solver_call > 0, time_lin > 0, and nothing else changed by collecting them."""
    from safe_mpc_amd import closed_loop as cl
    from safe_mpc_amd.parser import Parameters
    par = Parameters({}, 'z1')
    par.nq, par.n_dof_safe_set, par.net_size, par.N, par.back_hor = 6, 6, [12, 256, 1], 10, 10
    probe = make_problem('st', 'ext', N=10)[1]
    B, n_steps = 40, 70
    x0 = sample_instances(probe, B, seed=1)
    xg, ug = np.repeat(x0[:, None, :], 11, axis=1), np.zeros((B, 10, 6))
    res = cl.run_mpc(par, 'st', xg, ug, n_steps=n_steps, on_device=on_device, collect_times=True, groups=2 if on_device else 1)
    ts = res['time_stats']
    groups = 2 if on_device else 1
    assert res['time_fields'] == ['time_lin', 'time_sim', 'time_qp', 'time_qp_solver_call', 'time_glob', 'time_reg', 'time_tot']
    assert ts.shape == (groups * n_steps, 7) and res['time_lost'] == 0
    lin, sim, qp, call, glob, reg, tot = ts.T
    assert np.all(tot > 0) and np.all(lin > 0) and np.all(call > 0)
    assert np.all(tot >= qp - 1e-9) and np.all(qp >= call - 1e-9)
    assert np.all(sim == 0) and np.all(glob == 0) and np.all(reg == 0)
    assert np.all(tot < 0.5)                                          # seconds, like acados' get_stats
    assert np.allclose(res['time_q99'], np.quantile(ts, 0.99, axis=0))
    # the same run without the statistics: on the device that is the hipGraph path (graphs=True is run_mpc's default and
    # collect_times switches it off) -- the captured step halves replayed for 67 of the 70 steps must give the eager run's states bit for bit
    ref = cl.run_mpc(par, 'st', xg, ug, n_steps=n_steps, on_device=on_device, groups=groups, graphs=True)
    assert 'time_stats' not in ref and np.array_equal(np.nan_to_num(ref['x']), np.nan_to_num(res['x']))
