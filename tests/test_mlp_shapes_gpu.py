"""The safe-set network's kernels at the shapes the ABI takes and the suite never ran: n_dof_safe_set < nq on the one-kernel passes
(k_mlp_fused, k_mlp_wave) and on the layer-by-layer chain, every hidden width and depth smpc_set_mlp accepts through the chain,
networks swapped on a live handle, and smpc_set_mlp's refusals.  -m gpu only.

The reference is the float64 numpy statement of mlp_shape_cases.py; errors are in its spread norm and held to
max(16 E_o, floor), E_o the CPU oracle's fp32 error on the same rows (test_mlp_shapes_host.py), floors 2e-5 (value) and 2e-4
(gradient).  Every comparison prints a line `MLPSHAPE ...` with E_o, the engine's error and the bound (profiles/mlp_shape_tests.txt)."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (before the engine's library is loaded: PyTorch-ROCm must find the HIP runtime it ships with)

import mlp_shape_cases as mc
from conftest import constant_guess, sample_instances

pytestmark = pytest.mark.gpu
SMPC_EINVAL = -1


def _engine(prob, net, qp_mode=None):
    from safe_mpc_amd.solver import BatchedOcpSolver
    s = BatchedOcpSolver(prob, None)
    s.set_mlp(net, **({'ctx_default': np.array(mc.CTX)} if net.n_ctx else {}))
    if qp_mode:
        s.set_qp_mode(qp_mode)
    return s


def _held_to_the_reference(s, case, which=0, ctx=None):
    """eval_nodes of inputs(which) against the float64 statement: value and the 2 nd live gradient entries within the case's bound,
    the 2 (nq - nd) entries of the unseen joints, the tail behind 2 nq and every switched-off node exactly zero"""
    nq, nd = case.nq, case.nd
    x0, xg, ug, p = case.inputs(which)
    on = case.live(p)
    e_o, e_og, bv, bg, norms = mc.yardstick(case, which, ctx)
    g, dg, y = case.reference(which, case.net.folded(np.array(ctx)) if ctx is not None else None)
    a = s.eval_nodes(xg, ug, p)
    val, grad = np.array(a['nn_val']), np.array(a['nn_grad'])
    ev, eg = mc.errors(case, val[on], grad[on], g, dg, norms)
    print(f'MLPSHAPE {case.name} call {which}: rows {int(on.sum())} E_o {e_o:.2e} engine {ev:.2e} bound {bv:.2e} | '
          f'grad E_o {e_og:.2e} engine {eg:.2e} bound {bg:.2e}')
    assert on.sum() > 16 and (~on).sum() > 0
    assert np.all(val[~on] == 0.0) and np.all(grad[~on] == 0.0)
    dead = np.setdiff1d(np.arange(grad.shape[-1]), np.r_[0:nd, nq:nq + nd])
    assert dead.size == grad.shape[-1] - 2 * nd and np.all(grad[on][:, dead] == 0.0)
    assert np.all(val[on] != 0.0)
    assert ev < bv, (case.name, which, ev, bv)
    assert eg < bg, (case.name, which, eg, bg)
    return val, grad


def _twice(case, ctx=None):
    """two calls on one handle with different states (and switches): the second must not see a tail of the first"""
    s = _engine(case.prob, case.net)
    _held_to_the_reference(s, case, 0, ctx)
    _held_to_the_reference(s, case, 1, ctx)


# ---- 1. nn_dof < nq on the three kernel families ------------------------------------------------------------------------------------
@pytest.mark.parametrize('controller,B,N,switched', mc.SMALL_SHAPES, ids=['st', 'everywhere'])
@pytest.mark.parametrize('nq,nd', mc.ND_PAIRS)
@pytest.mark.parametrize('family', ['fused', 'chain'])
def test_unseen_joints_small_row_counts(family, nq, nd, controller, B, N, switched):
    """k_mlp_fused (256 wide, three hidden layers) and the GEMM chain (128 wide, in this process: no knob): the terminal row of
    17 instances -- a full 16-row block and a block of one row -- and the row on every node of 9 x 7 with half the switches off"""
    _twice(mc.nd_case(family, nq, nd, controller, B, N, switched))


@pytest.mark.parametrize('switched', [False, True])
def test_unseen_joints_large_row_count(switched):
    """k_mlp_wave at nd = 5 < nq = 6: 520 x 16 = 8 320 candidate rows, all live or about half of them"""
    _twice(mc.wave_case(switched))


# ---- 2. through the solve ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('qp_mode', ['throughput', 'latency'])
@pytest.mark.parametrize('H', [256, 128])
@pytest.mark.parametrize('controller', ['st', 'constraint_everywhere'])
def test_solve_with_unseen_joints(controller, H, qp_mode):
    """nd = 5 < nq = 6 through solve against Oracle.solve_batch at the tolerance of test_rti_solve_parity for these controllers
    (1e-4): the stage builder reads the compact nn[node][1 + nx] record, the unseen joints' zeros included.  H = 128: k_nn_chain
    writes that record."""
    case = mc.Case(controller, 6, 5, H, 4, 16, 8, seed=31)
    x0 = sample_instances(case.prob, 16, seed=2, vel_scale=0.1)         # (the inputs of test_rti_solve_parity)
    xg, ug, p = constant_guess(case.prob, x0)
    # alpha per instance puts the start state ON the set's boundary (g = 0), so that the row binds: with the default alpha the set
    # is far away, the row inactive, and the solution independent of the network to 1e-15
    g0, _, y = mc.row64(case.net, x0, 6, case.par.eps, 0.0)
    p[:, :, 3] = (100.0 * (1.0 - (y - g0) / y))[:, None]
    s, o = _engine(case.prob, case.net, qp_mode), mc.oracle_of(case)
    xb, ub, sb, ib = o.solve_batch(x0, xg, ug, p)
    p_off = p.copy()
    p_off[:, :, 4] = -1.0
    moved = np.abs(ub - o.solve_batch(x0, xg, ug, p_off)[1]).reshape(16, -1).max(axis=1)
    assert (moved > 0.1).sum() >= 6, moved            # (the row decides the solution of at least six instances)
    xa, ua, sa, ia = s.solve(x0, xg, ug, p)
    assert np.array_equal(sa, sb), (sa, sb)
    ok = sb == 0
    assert ok.sum() >= 14
    eu, ex = np.abs(ua[ok] - ub[ok]).max(), np.abs(xa[ok] - xb[ok]).max()
    print(f'MLPSHAPE solve {case.name} {qp_mode}: u error {eu:.2e} (|u| {np.abs(ub[ok]).max():.1f}) x error {ex:.2e}')
    assert eu < 1e-4 * (1 + np.abs(ub[ok]).max())
    assert ex < 1e-4


# ---- 3. the forward-only consumers at nd < nq -------------------------------------------------------------------------------------------
def _verdicts(got, g, thr, bound, what):
    """got == (g >= thr) wherever the reference is more than the bound away from the threshold; at most 2 % of rows sit closer"""
    far = np.abs(g - thr) > bound
    assert (~far).sum() <= 0.02 * g.size, (what, int((~far).sum()), g.size)
    assert np.array_equal(np.asarray(got, bool)[far], (g >= thr)[far]), what
    assert (g >= thr).any() and (g < thr).any(), what


def _threshold(g):
    gs = np.sort(np.ravel(g))
    return 0.5 * (gs[gs.size // 2 - 1] + gs[gs.size // 2])


@pytest.mark.parametrize('nq,nd', mc.ND_PAIRS)
@pytest.mark.parametrize('H', [256, 128])
def test_forward_only_consumers_with_unseen_joints(nq, nd, H):
    """k_check_nn over a plain list (check_trajectory), k_check_guess, k_score_safe on a step-major log (B = 5, 7 steps) and
    k_merit's safe-set violation, each against the float64 g of the same states.  H = 256: the one-kernel forward pass; H = 128:
    the chain's."""
    par, prob = mc.shape_problem('constraint_everywhere', nq, nd, 4)
    N, nx = 4, 2 * nq
    net = mc.make_net(prob, H, 4, seed=41)
    s = _engine(prob, net)

    # check_trajectory: 7 instances x 3 nodes, a plain list of 21 rows; the threshold between the two middle values of g
    x = np.ascontiguousarray(sample_instances(prob, 21, seed=5, vel_scale=0.3).reshape(7, 3, nx))
    g, bound = mc.rows_reference(prob, net, x, par.alpha)
    g = g.reshape(7, 3)
    thr = _threshold(g)
    ok, nn_ok = s.check_trajectory(x, want_nn=True, tol_safe=-thr)
    print(f'MLPSHAPE check_trajectory nq{nq} nd{nd} H{H}: bound on g {bound:.2e}, nearest row {np.abs(g - thr).min():.2e}')
    _verdicts(nn_ok, g, thr, bound, 'check_trajectory')

    # check_guess: the safe-set test at node N of 7 guesses; worst[:, 4] is -g itself
    x0 = sample_instances(prob, 7, seed=6, vel_scale=0.3)
    xg, ug, p = constant_guess(prob, x0)
    xg[:, 1:] += 0.05 * np.random.default_rng(6).standard_normal(xg[:, 1:].shape)
    g, bound = mc.rows_reference(prob, net, xg[:, N], par.alpha)
    thr = _threshold(g)
    flags, worst = s.check_guess(xg, ug, safe_node=N, tol_safe=-thr)
    print(f'MLPSHAPE check_guess nq{nq} nd{nd} H{H}: -g error {np.abs(np.asarray(worst)[:, 4] + g).max():.2e} bound {bound:.2e}')
    assert np.abs(np.asarray(worst)[:, 4] + g).max() < bound
    _verdicts((np.asarray(flags) >> 4 & 1) == 0, g, thr, bound, 'check_guess')

    # score_rollout: the least g over the 8 states of 5 instances, step-major rows m = j B + b
    x_log = np.ascontiguousarray(sample_instances(prob, 40, seed=7, vel_scale=0.3).reshape(8, 5, nx))
    u_log = np.zeros((7, 5, nq))
    g, bound = mc.rows_reference(prob, net, x_log, par.alpha)
    g = g.reshape(8, 5)
    out, outi = s.score_rollout(x_log, u_log, want_safe=True)
    out, outi = np.asarray(out), np.asarray(outi)
    print(f'MLPSHAPE score_rollout nq{nq} nd{nd} H{H}: safe_min error {np.abs(out[:, 6] - g.min(axis=0)).max():.2e} bound {bound:.2e}')
    assert np.abs(out[:, 6] - g.min(axis=0)).max() < bound
    gs = np.sort(g, axis=0)
    clear = gs[1] - gs[0] > 2 * bound
    assert clear.sum() >= 4 and np.array_equal(outi[clear, 3], g.argmin(axis=0)[clear])
    assert len(set(g.argmin(axis=0).tolist())) > 1          # (the least value is not at one step for every instance)

    # merit_terms: the l1 violation with the rows on minus the same with the rows off = sum over the live nodes of max(-g, 0);
    # alpha shrinks the set until about half the nodes are outside: (100 - alpha) / 100 = the median of |v| / y
    xg, ug, p = mc.case_inputs(prob, 5, 8, switched=True)[1:]
    on = p[:, :, 4] > 0
    on[:, 0] = False
    g0, _, y = mc.row64(net, xg[on], nq, par.eps, 0.0)
    p[:, :, 3] = 100.0 * (1.0 - np.median((y - g0) / y))
    g, bound = mc.rows_reference(prob, net, xg[on], p[on][:, 3])
    want = np.zeros(p.shape[:2])
    want[on] = np.maximum(-g, 0.0)
    assert (g < -10 * bound).sum() >= 3 and (g > 10 * bound).sum() >= 3
    p_off = p.copy()
    p_off[:, :, 4] = 0.0
    got = np.asarray(s.merit_terms(xg[:, 0], xg, ug, p))[:, 1] - np.asarray(s.merit_terms(xg[:, 0], xg, ug, p_off))[:, 1]
    err = np.abs(got - want.sum(axis=1))
    print(f'MLPSHAPE merit_terms nq{nq} nd{nd} H{H}: safe violation error {err.max():.2e} bound per node {bound:.2e}')
    assert np.all(err < on.sum(axis=1) * bound + 1e-10)


def test_receding_policy_step_with_unseen_joints():
    """k_check_nn over the LISTED rows (mode 3: the receding policy tests the nodes whose switch is on) at nd = 5 < nq = 6: the
    device automaton (smpc_policy_step) against the numpy automaton, whose safe-set test is check_trajectory's plain list -- held
    to the float64 statement above.  Same controls, abort flags and receding indices, step by step on kicked states."""
    from safe_mpc_amd import closed_loop as cl
    from safe_mpc_amd import controller as C
    from safe_mpc_amd.parser import Parameters
    par = Parameters({}, 'z1')
    par.nq, par.n_dof_safe_set, par.net_size, par.N = 6, 5, [10, 256, 1], 8
    N, B = 8, 24
    host = C.get_controller('receding', par, B)
    dev = C.get_controller('receding', par, B, device_state=True)
    assert host.problem.desc.nn_dof == 5 and host.net.dims[0] == 10
    x0 = sample_instances(host.problem, B, seed=3, vel_scale=0.4)
    xg, ug = np.repeat(x0[:, None, :], N + 1, axis=1), np.zeros((B, N, 6))
    host.setGuess(xg, ug)
    dev.setGuess(xg, ug)
    rng = np.random.default_rng(0)
    x = x0.copy()
    r_seen = set()
    for t in range(N + 4):
        stepping = rng.random(B) > 0.2 if t % 3 else np.ones(B, bool)
        u_other = rng.normal(size=(B, 6))
        uh, ah = cl._masked_step(host, x, stepping)
        uh = np.where(stepping[:, None], uh, u_other)
        ud, ad = dev.step_on_device(torch.tensor(x, device='cuda'), torch.tensor(stepping, device='cuda'), torch.tensor(u_other, device='cuda'))
        dev.ocp_solver.sync()
        assert np.array_equal(ad.cpu().numpy(), ah), t
        assert np.abs(ud.cpu().numpy() - uh).max() < 1e-9, t
        assert np.array_equal(dev.r.cpu().numpy(), np.array(host.r)), t
        r_seen.update(np.array(host.r).tolist())
        x = x + par.dt * np.hstack([x[:, 6:], uh])
        if t % 5 == 4:
            x[:, 6:] += rng.normal(scale=0.5, size=(B, 6))
    assert len(r_seen) > 2          # (the safe-set test moved the receding index: its verdicts differed between nodes and steps)


# ---- 4. width and depth through the chain -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('controller,B,N,switched', mc.CHAIN_SHAPES, ids=['st', 'everywhere'])
@pytest.mark.parametrize('H,L', mc.WIDTH_DEPTH)
def test_width_and_depth(H, L, controller, B, N, switched):
    """k_nn_features, k_gemm_f32 on an H / 64 grid with K = H, k_nn_output and k_nn_chain for L - 1 hidden layers of width H:
    mode 1 with 33 rows, mode 3 with 135 candidates of which about half are live.  256 wide with two or four hidden layers must
    take this path as well."""
    _twice(mc.chain_case(H, L, controller, B, N, switched))


@pytest.mark.parametrize('act', [a for a in mc.ACTS if a != 'gelu'])
def test_activations_through_the_chain(act):
    _twice(mc.chain_case(128, 3, *mc.CHAIN_SHAPES[0], act=act))


@pytest.mark.parametrize('controller,B,N,switched', mc.CHAIN_SHAPES, ids=['st', 'everywhere'])
def test_context_that_fills_the_padded_input(controller, B, N, switched):
    """nd = 5 < nq = 6 with n_ctx = 6: state features and context fill all MLP_KPAD = 16 columns of layer 0's input.  Against the
    folded net."""
    case = mc.context_case(controller, B, N, switched)
    assert case.net.dims[0] == 16
    _twice(case, mc.CTX)
    # a context per instance, every one the default's numbers: the same bits as the default row alone
    s = _engine(case.prob, case.net)
    x0, xg, ug, p = case.inputs(0)
    alone = s.eval_nodes(xg, ug, p)
    s.set_instance_context(np.repeat(np.array(mc.CTX)[None], B, axis=0))
    each = s.eval_nodes(xg, ug, p)
    assert np.array_equal(np.array(alone['nn_val']), np.array(each['nn_val']))
    assert np.array_equal(np.array(alone['nn_grad']), np.array(each['nn_grad']))


# ---- 5. networks swapped on a live handle -----------------------------------------------------------------------------------------------
SWAPS = [(256, 4), (128, 4), (512, 4), (64, 2), (256, 4)]      # three hidden layers of 256, 128, 512; one of 64; 256 again


@pytest.mark.parametrize('controller,B,N,switched', mc.CHAIN_SHAPES, ids=['st', 'everywhere'])
def test_networks_swapped_on_a_live_handle(controller, B, N, switched):
    """smpc_set_mlp on a handle that has run another network re-carves the weight block and re-reserves every activation buffer:
    after each swap eval_nodes gives the bits of a fresh handle that was only ever given that network (same kernel, same
    arithmetic), which in turn is held to the float64 statement"""
    cases = [mc.chain_case(H, L, controller, B, N, switched) for H, L in SWAPS]
    x0, xg, ug, p = cases[0].inputs(0)
    live = _engine(cases[0].prob, cases[0].net)
    for i, case in enumerate(cases):
        if i:
            live.set_mlp(case.net)
        fresh = _engine(case.prob, case.net)
        val, grad = _held_to_the_reference(fresh, case)
        a = live.eval_nodes(xg, ug, p)
        assert np.array_equal(np.array(a['nn_val']), val), (i, case.name)
        assert np.array_equal(np.array(a['nn_grad']), grad), (i, case.name)
        fresh.close()


# ---- 6. what smpc_set_mlp refuses ----------------------------------------------------------------------------------------------------------
def _set_mlp_raw(s, dims):
    n = len(dims) - 1
    rng = np.random.default_rng(0)
    Ws = [rng.uniform(-0.1, 0.1, (dims[l + 1], dims[l])).astype(np.float32) for l in range(n)]
    bs = [np.zeros(dims[l + 1], np.float32) for l in range(n)]
    d = np.array(dims, np.int32)
    Wp = (C.c_void_p * n)(*[w.ctypes.data for w in Ws])
    bp = (C.c_void_p * n)(*[b.ctypes.data for b in bs])
    rc = s.L.smpc_set_mlp(s.h, n, d.ctypes.data_as(C.POINTER(C.c_int32)), Wp, bp, 0)
    return rc, s.L.smpc_last_error(s.h).decode()


@pytest.mark.parametrize('dims,message', [
    ([12, 1], 'nlayers=1 outside 2..6'),
    ([12] + [64] * 6 + [1], 'nlayers=7 outside 2..6'),
    ([10, 128, 1], 'input width 10 != 2*n_dof_safe_set'),
    ([12, 96, 96, 1], 'hidden width must be a multiple of 64 and output 1'),
    ([12, 128, 64, 1], 'hidden layers must share one width'),
    ([12, 128, 128, 2], 'hidden width must be a multiple of 64 and output 1'),
], ids=['one-layer', 'seven-layers', 'input-width', 'H96', 'mixed-widths', 'two-outputs'])
def test_set_mlp_refusals_leave_the_network_in_force(dims, message):
    """SMPC_EINVAL with the engine's message, and the network set before still evaluates to the same bits: the checks sit before
    any state is touched"""
    case = mc.chain_case(128, 3, *mc.CHAIN_SHAPES[1])
    x0, xg, ug, p = case.inputs(0)
    s = _engine(case.prob, case.net)
    before = s.eval_nodes(xg, ug, p)
    assert np.abs(np.array(before['nn_val'])).max() > 0
    rc, msg = _set_mlp_raw(s, dims)
    assert rc == SMPC_EINVAL and message in msg, (rc, msg)
    after = s.eval_nodes(xg, ug, p)
    assert np.array_equal(np.array(before['nn_val']), np.array(after['nn_val']))
    assert np.array_equal(np.array(before['nn_grad']), np.array(after['nn_grad']))
    # ... and the same dims made acceptable are accepted
    rc, msg = _set_mlp_raw(s, [12, 128, 128, 1])
    assert rc == 0, msg
