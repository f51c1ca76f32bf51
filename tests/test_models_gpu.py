"""A controller model of its own for every instance (smpc_set_instance_models) on the GPU.  -m gpu only.

Every statement is held against the CPU oracle called once per distinct model, on the problem whose DESCRIPTOR carries that
model's inertials (model_cases.problem_with_model) -- the oracle knows nothing of instance models.  Tolerances are those of the
tests that pin the same calls on the shared model: 1e-9 relative for the linearisation pieces (test_eval_nodes_parity), 1e-4
(1 + |u|_inf) with equal statuses for an RTI solve (test_rti_solve_parity), 1e-9 (1 + |.|) for merit terms and check-guess margins
(test_sqp_gpu.py, test_guess_until_gpu.py), 1e-11 of each block's scale for the stage records of the two builders
(test_stage_builder_equals_thread_per_node_kernels), equality for verdicts and integer outputs.

Models: perturbed_joint_tables(par, nq, 20 %, seeds 0..7), the plant tables of run_mpc(noise=20); Z1 (nq = 6), N = 8 unless said
otherwise."""
import ctypes as C
import types

import numpy as np
import pytest

import model_cases as mc
import scene_cases as sc
from conftest import constant_guess, make_problem, sample_instances
from fake_solver import OracleSolver

pytestmark = pytest.mark.gpu


def _rel(a, b):
    return np.abs(a - b).max() / (1e-12 + np.abs(b).max())


def _close(got, ref, tol):
    same_inf = np.isinf(ref) & (got == ref)
    with np.errstate(invalid='ignore'):
        return np.all(same_inf | (np.abs(got - ref) <= tol * (1.0 + np.abs(ref))))


def _solver(prob, net, mode=None):
    from safe_mpc_amd.solver import BatchedOcpSolver
    s = BatchedOcpSolver(prob, net)
    if mode is not None:
        s.set_qp_mode(mode)
    return s


def _dev(v):
    import torch
    return torch.tensor(v, dtype=torch.float64, device='cuda:0')


def _dev_table(t):
    """[B, nq] JOINT_DTYPE as the float64 tensor [B, nq, 29] the device paths take"""
    return _dev(np.ascontiguousarray(t).view(np.float64).reshape(t.shape[0], t.shape[1], -1))


def _perturbed_inputs(prob, B, seed=1):
    """the inputs of test_eval_nodes_parity"""
    x0 = sample_instances(prob, B, seed=seed, vel_scale=0.5)
    xg, ug, p = constant_guess(prob, x0)
    rng = np.random.default_rng(0)
    xg[:, 1:] += 0.05 * rng.standard_normal(xg[:, 1:].shape)
    ug += rng.uniform(-5, 5, ug.shape)
    return x0, xg, ug, p


# ---- 1. linearisation -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('system,controller,N,B', [('z1', 'naive', 8, 8), ('fr7', 'constraint_everywhere', 6, 4)])
def test_eval_nodes_with_every_instances_own_model(system, controller, N, B):
    """B tables, inputs perturbed as in test_eval_nodes_parity: tau, M, dtau_dq and dtau_dv of instance b within 1e-9 relative of the
    oracle on problem_with_model(b); every kinematic field (ee, cost pieces, rows) bit-equal to the call without models; tau with
    and without models more than 1e-3 apart (the models are told apart); the device-pointer table gives the bits of the host one"""
    from oracle.oracle import Oracle
    (par, prob, net), tables, probs = mc.family(system, controller, N, B)
    nq, nr = prob.nq, len(prob.rows)
    x0, xg, ug, p = _perturbed_inputs(prob, B)
    s = _solver(prob, net)
    shared = s.eval_nodes(xg, ug, p)
    s.set_instance_models(tables)
    a = s.eval_nodes(xg, ug, p)
    dyn = [('tau', nq), ('M', nq * nq), ('dtau_dq', nq * nq), ('dtau_dv', nq * nq)]
    for b in range(B):
        ref = Oracle(probs[b]).eval_nodes(xg[b:b + 1], ug[b:b + 1], p[b:b + 1])
        for f, n in dyn:
            err = _rel(a[f][b:b + 1, ..., :n], ref[f][..., :n])
            print(system, b, f, err)
            assert err < 1e-9, (b, f)
    for f in a.dtype.names:
        if f not in [d[0] for d in dyn]:
            assert np.array_equal(a[f], shared[f], equal_nan=True), f
    assert all(_rel(a['tau'][b, :N, :nq], shared['tau'][b, :N, :nq]) > 1e-3 for b in range(B))
    s.set_instance_models(_dev_table(tables))
    d = s.eval_nodes(_dev(xg), _dev(ug), _dev(p))
    s.sync()
    for f, _ in dyn:
        assert np.array_equal(d[f].cpu().numpy(), a[f]), f


# ---- 2. the two builders --------------------------------------------------------------------------------------------------------------
def _stage_records(s, x0, xg, ug, p, path):
    """the QP workspace after the stage records are built, by either builder (smpc_debug_stage_records), and its layout"""
    L = s.L
    L.smpc_debug_stage_records.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 4 + [C.c_int, C.c_void_p, C.c_void_p]
    lay = np.zeros(24, np.int32)
    B = x0.shape[0]
    arrs = [np.ascontiguousarray(a, np.float64) for a in (x0, xg, ug, p)]
    out = np.zeros(B * 64 * 2048)
    rc = L.smpc_debug_stage_records(s.h, B, *[a.ctypes.data for a in arrs], path, out.ctypes.data, lay.ctypes.data)
    assert rc == 0, L.smpc_last_error(s.h)
    per = int(lay[14])
    assert B * per <= out.size
    return out[:B * per].reshape(B, per), lay


@pytest.mark.parametrize('with_scene', [False, True])
def test_stage_builder_equals_thread_per_node_kernels_with_models(with_scene):
    """k_stage_build<., ., SCENE, true> against k_node_linearise<., SCENE, true> -> k_qp_setup, block by block of the stage record, 1e-11
    of each block's scale (test_stage_builder_equals_thread_per_node_kernels); with a scene set as well (B = 4, scene_cases.SHIFTS)
    the instantiation with both flags runs.  The records differ from those without models."""
    N = 8
    if with_scene:
        (par, prob, net), moved, geom = sc.scene_family('z1', 'st', N, 4)
        B = 4
    else:
        par, prob, net = make_problem('naive', N=N)
        B = 8
    tables = mc.model_tables(par, prob.nq, B)
    s = _solver(prob, net)
    x0 = sample_instances(prob, B, seed=3, vel_scale=0.3)
    xg, ug, p = constant_guess(prob, x0)
    rng = np.random.default_rng(2)
    ug += rng.uniform(-3, 3, ug.shape)
    xg = s.guess_correction(xg, ug)
    xg[:, 1:] += 0.01 * rng.standard_normal(xg[:, 1:].shape)
    x0 = x0 + 0.003 * rng.standard_normal(x0.shape)
    plain, _ = _stage_records(s, x0, xg, ug, p, 1)
    if with_scene:
        s.set_instance_scene(geom[np.arange(B) % 4])
    s.set_instance_models(tables)
    new, lay = _stage_records(s, x0, xg, ug, p, 1)
    old, lay2 = _stage_records(s, x0, xg, ug, p, 0)
    assert np.array_equal(lay, lay2)
    stride, nIMG, oIMG, oSL, nF, oR0, oR1, oR2, oCZA, oCZN, oZ, oZN, NRT, nJ, per = [int(v) for v in lay[:15]]
    new, old, plain = (a.reshape(B, -1)[:, :(N + 1) * stride].reshape(B, N + 1, stride) for a in (new, old, plain))
    blocks = {'jacobian': (oIMG, nJ), 'defect / scalars': (oIMG + nJ, nF - nJ), 'cost': (oIMG + nF, nIMG - nF),
              'scalars + partial sums + w': (oSL, 16), 'bounds': (oR0, 2 * NRT), 'slacks': (oR1, 2 * NRT), 'multipliers': (oR2, 2 * NRT),
              'c.z_aff': (oCZA, 32), 'c.z+': (oCZN, 32), 'z': (oZ, 3 * prob.nq), 'z+': (oZN, 3 * prob.nq)}
    for name, (o, n) in blocks.items():
        a, b = new[:, :, o:o + n], old[:, :, o:o + n]
        big = np.abs(b) >= 1e299
        assert np.array_equal(np.abs(a) >= 1e299, big), name
        a, b = np.where(big, 0.0, a), np.where(big, 0.0, b)
        scale = np.abs(b).max() + 1e-300
        print(with_scene, name, np.abs(a - b).max(), scale)
        assert np.abs(a - b).max() <= 1e-11 * scale + 1e-13, (name, np.abs(a - b).max(), scale)
    jac, jac0 = new[:, :, oIMG:oIMG + nJ], plain[:, :, oIMG:oIMG + nJ]
    assert np.abs(jac - jac0).max() > 1e-3 * np.abs(jac0).max()


# ---- 3. the solve ---------------------------------------------------------------------------------------------------------------------
def _rti_reference(steps=3):
    """the tightened-torque problem of the clip property, 8 instances at one state, three consecutive RTI steps of the per-model
    oracles and of the nominal oracle from constant_guess, each from its own previous iterate"""
    (par, prob, net), tables, x0, probs = mc.clip_family()
    out = {}
    for key in ('models', 'nominal'):
        o = mc.ModelOracleSolver(prob, net)
        if key == 'models':
            o.set_instance_models(tables)
        xg, ug, p = constant_guess(prob, x0)
        seq = []
        for _ in range(steps):
            xr, ur, sr, _ = o.solve(x0, xg, ug, p)
            seq.append((xg, ug, xr, ur, sr))
            xg, ug = xr, ur
        out[key] = seq
    return prob, net, tables, x0, p, out


@pytest.mark.parametrize('qp_mode', ['throughput', 'latency'])
def test_rti_solve_with_every_instances_own_model(qp_mode):
    """B = 8, three RTI steps on the tightened-torque problem (the torque rows are active: the model decides the control), both
    forms of the interior point: statuses equal, |u - u_ref| < 1e-4 (1 + max |u_ref|) at each step against ModelOracleSolver.
    Precondition on the CPU: with and without models the oracle's controls are more than 100 x the tolerance apart in at least
    half of the instances."""
    prob, net, tables, x0, p, ref = _rti_reference()
    assert all(np.all(st[4] == 0) for st in ref['models'])
    tol = 1e-4 * (1 + max(np.abs(st[3]).max() for st in ref['models']))
    apart = np.max([np.abs(a[3] - b[3]).reshape(8, -1).max(1) for a, b in zip(ref['models'], ref['nominal'])], axis=0)
    print('apart / tol', apart / tol)
    assert (apart > 100 * tol).sum() >= 4
    s = _solver(prob, net, qp_mode)
    s.set_instance_models(tables)
    for k, (xg, ug, xr, ur, sr) in enumerate(ref['models']):
        xa, ua, sa, ia = s.solve(x0, xg, ug, p)
        err = np.abs(ua - ur).max()
        print(qp_mode, 'step', k, 'status', sa.tolist(), 'u error', err, 'bound', 1e-4 * (1 + np.abs(ur).max()))
        assert np.array_equal(sa, sr)
        assert err < 1e-4 * (1 + np.abs(ur).max())


# ---- 4. what the feature is for ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('device_state', [False, True])
def test_a_controller_with_the_plants_model_never_asks_for_a_torque_that_clips(device_state):
    """The clip property through the engine: NaiveController.step (smpc_policy_step kind 0 on device state; guessCorrection / solve /
    provideControl with host pointers on host state) plus plant_step with the SAME tables, 6 steps, 8 instances at one state,
    tau_max = max(1.10 |tau(x0, 0)|, 0.05).  With the nominal controller model at least 6 of 8 instances clip by more than 1e-3
    (the oracle: all 8, worst |u_eff - u_0| 0.14 .. 4.66); with the instance's own model every |u_eff - u_0| is within 1e-9
    (1 + |u|_inf) (the oracle: 1.6e-12); all statuses 0."""
    from safe_mpc_amd import controller as Cn
    from safe_mpc_amd.solver import BatchedOcpSolver
    (par, prob, net), tables, x0, probs = mc.clip_family()
    B, N, steps = len(x0), prob.N, 6
    worst = {}
    for key in ('nominal', 'matched'):
        ctrl = Cn.NaiveController.__new__(Cn.NaiveController)
        Cn.AbstractController.__init__(ctrl, par, B, 'ext', N, solver=BatchedOcpSolver(prob, net), net=net, device_state=device_state)
        sv = ctrl.ocp_solver
        plant = _dev_table(tables) if device_state else tables
        if key == 'matched':
            sv.set_instance_models(plant)
        xp = ctrl.xp
        ctrl.setGuess(xp.asarray(np.repeat(x0[:, None, :], N + 1, axis=1), xp.f64), xp.zeros((B, N, prob.nu)))
        x = xp.asarray(x0, xp.f64)
        w, um, status = np.zeros(B), 0.0, []
        for _ in range(steps):
            u, _ = ctrl.step(x)
            u = xp.copy(u)
            x, ue = sv.plant_step(x, u, plant)
            w = np.maximum(w, np.abs(xp.host(ue) - xp.host(u)).max(1))
            um = max(um, np.abs(xp.host(u)).max())
            status.append(xp.host(ctrl.last_status).copy())
        sv.sync()
        print(key, 'device state' if device_state else 'host state', 'worst |u_eff - u_0|', w, '|u|_inf', um)
        assert np.all(np.array(status) == 0)
        worst[key] = (w, um)
    assert (worst['nominal'][0] > 1e-3).sum() >= 6
    assert np.all(worst['matched'][0] <= 1e-9 * (1 + worst['matched'][1]))


# ---- 5. merit, check_guess, SQP -----------------------------------------------------------------------------------------------------
def _host_ctrl(par, prob, solver, B, p=None):
    """a NaiveController on host state around ``solver`` whose problem is ``prob`` (the tightened one)"""
    from safe_mpc_amd import controller as Cn
    ctrl = Cn.NaiveController.__new__(Cn.NaiveController)
    Cn.AbstractController.__init__(ctrl, par, B, 'ext', prob.N, solver=solver, net=None)
    ctrl.problem = ctrl.model = prob
    ctrl._tau_min, ctrl._tau_max = prob.tau_min, prob.tau_max
    return ctrl


def test_merit_check_guess_and_sqp_follow_the_models():
    """merit_terms (f, viol), check_guess (flags equal; worst[2], the torque margin, is the only entry that moves with the models)
    and sqp (2 iterations: status, updated and iters equal, alpha equal, iterate within 1e-4 (1 + |.|_inf), the tolerance of an RTI
    solve) on the tightened-torque problem, each against the numpy statement over ModelOracleSolver"""
    from safe_mpc_amd import closed_loop as cl
    (par, prob, net), tables, x0, probs = mc.clip_family()
    B, N, nq = len(x0), prob.N, prob.nq
    o = mc.ModelOracleSolver(prob, net)
    o.set_instance_models(tables)
    s = _solver(prob, net)
    xg, ug, p = constant_guess(prob, x0)
    rng = np.random.default_rng(4)
    ug += rng.uniform(-3, 3, ug.shape)
    xg = s.guess_correction(xg, ug)
    xg[:, 1:] += 0.01 * rng.standard_normal(xg[:, 1:].shape)
    shared_m = s.merit_terms(x0, xg, ug, p)
    shared_f, shared_w = s.check_guess(xg, ug)
    s.set_instance_models(tables)
    # merit terms
    host = types.SimpleNamespace(problem=prob, ocp_solver=o, p=p, N=N, nq=nq, params=par)
    f_ref, _, _, v_ref = cl.merit_terms(host, x0, xg, ug)
    out = s.merit_terms(x0, xg, ug, p)
    print('merit f error', np.abs(out[:, 0] - f_ref).max(), 'viol error', np.abs(out[:, 1] - v_ref).max())
    assert _close(out[:, 0], f_ref, 1e-9) and _close(out[:, 1], v_ref, 1e-9)
    assert np.abs(out[:, 1] - shared_m[:, 1]).max() > 1e-4            # (the models are told apart)
    # check_guess: the torque margin by the statement, max over nodes 0..N-1 of max(tau_min - tau, tau - tau_max)
    tau = np.asarray(o.eval_nodes(xg, ug, p)['tau'])[:, :N, :nq]
    w_ref = np.maximum(prob.tau_min - tau, tau - prob.tau_max).reshape(B, -1).max(1)
    assert np.all(np.abs(w_ref - par.tol_tau) > 1e-7)              # no verdict within rounding of its threshold
    flags, worst = s.check_guess(xg, ug)
    print('check_guess worst[2] error', np.abs(worst[:, 2] - w_ref).max())
    assert _close(worst[:, 2], w_ref, 1e-9)
    others = [0, 1, 3, 4]
    assert np.array_equal(worst[:, others], shared_w[:, others])
    assert np.abs(worst[:, 2] - shared_w[:, 2]).max() > 1e-4
    assert np.array_equal(flags & ~4, shared_f & ~4)
    assert np.array_equal((flags >> 2) & 1, (~(w_ref <= par.tol_tau)).astype(np.int32))
    # two SQP iterations from the constant guess
    xg0, ug0, _ = constant_guess(prob, x0)
    ctrl = _host_ctrl(par, prob, o, B)
    ctrl.setGuess(xg0.copy(), ug0.copy())
    state_h = cl.sqp_host_advance(ctrl, x0, cl.new_host_sqp_state(B), 2)
    xd, ud, state = s.sqp(x0, xg0, ug0, ctrl.p, dict(max_iter=2))
    for k in ('status', 'iters'):
        assert np.array_equal(np.asarray(state[k]), state_h[k]), k
    assert np.array_equal(np.asarray(state['done']).astype(bool), state_h['done'].astype(bool))
    ex = np.abs(xd - ctrl.x_guess).max() / (1 + np.abs(ctrl.x_guess).max())
    eu = np.abs(ud - ctrl.u_guess).max() / (1 + np.abs(ctrl.u_guess).max())
    print('sqp iterate error', ex, eu, 'status', state_h['status'])
    assert ex < 1e-4 and eu < 1e-4


# ---- 6. the shared path ---------------------------------------------------------------------------------------------------------------
def test_base_model_equals_the_shared_path_bit_for_bit():
    """every instance gets prob.joint_table(): eval_nodes, solve and check_guess are BIT-EQUAL to the same calls without models, in
    both forms of the interior point, at B = 32 and N = 30 ('st': the network row and six collision rows ride along)"""
    par, prob, net = make_problem('st', N=30)
    B = 32
    x0 = sample_instances(prob, B, seed=5, vel_scale=0.1)
    xg, ug, p = constant_guess(prob, x0)
    rng = np.random.default_rng(6)
    ug += rng.uniform(-2, 2, ug.shape)
    tables = np.repeat(prob.joint_table()[None], B, axis=0)
    for mode in ('throughput', 'latency'):
        s = _solver(prob, net, mode)
        xg1 = s.guess_correction(xg, ug)

        def calls():
            return s.eval_nodes(xg1, ug, p), s.solve(x0, xg1, ug, p), s.check_guess(xg1, ug)
        ev0, sol0, cg0 = calls()
        s.set_instance_models(tables)
        ev1, sol1, cg1 = calls()
        for f in ev0.dtype.names:
            assert np.array_equal(ev1[f], ev0[f], equal_nan=True), (mode, f)
        for a1, a0 in zip(sol1 + cg1, sol0 + cg0):
            assert np.array_equal(a1, a0, equal_nan=True), mode
        s.set_instance_models(_dev_table(tables))
        ev2, sol2, cg2 = calls()
        for a2, a0 in zip(sol2 + cg2, sol0 + cg0):
            assert np.array_equal(a2, a0, equal_nan=True), mode


# ---- 7. the slot rule -----------------------------------------------------------------------------------------------------------------
def test_the_model_table_follows_the_slot_rule():
    """After tests/test_instance_slots_gpu.py: another B is refused by every guarded entry point with both sizes and the setter named,
    and runs once cleared; the parallel policy and rollout are engine error -4; a refused set (non-finite mass; a moved p0 with host
    pointers) leaves the previous table in force; an overwrite in place under a captured solve takes effect at the next replay;
    growth while capturing is refused and the old table stays; a new horizon keeps the table."""
    import warnings
    import torch
    from safe_mpc_amd import controller as Cn
    from safe_mpc_amd._lib import EngineError
    N, B_SET, B_CALL = 4, 5, 3
    par, prob, net = make_problem('st', N=N)
    tables = mc.model_tables(par, prob.nq, B_SET)
    s = _solver(prob, net)
    x0 = sample_instances(prob, B_SET, seed=3, vel_scale=0.3)
    xg, ug, p = constant_guess(prob, x0)
    ug += np.random.default_rng(1).uniform(-3, 3, ug.shape)
    small = (x0[:B_CALL], xg[:B_CALL], ug[:B_CALL], p[:B_CALL])
    ctrl = Cn.get_controller('st', par, B_CALL, device_state=True)
    ctrl.setGuess(_dev(xg[:B_CALL]), _dev(ug[:B_CALL]))
    x_dev = _dev(x0[:B_CALL])
    calls = {'smpc_solve_batch': (s, lambda: s.solve(*small)), 'smpc_eval_nodes': (s, lambda: s.eval_nodes(*small[1:])),
             'smpc_merit_terms': (s, lambda: s.merit_terms(*small)), 'smpc_sqp_batch': (s, lambda: s.sqp(*small, dict(max_iter=1))),
             'smpc_check_guess': (s, lambda: s.check_guess(small[1], small[2])),
             'smpc_debug_stage_records': (s, lambda: _stage_records(s, *small, 1)),
             'smpc_policy_step': (ctrl.ocp_solver, lambda: ctrl.step_on_device(x_dev))}
    for entry, (sv, call) in calls.items():
        sv.set_instance_models(tables)
        pat = rf'{entry}: batch size {B_CALL}, .* set for {B_SET} instances \(smpc_set_instance_models'
        if entry == 'smpc_debug_stage_records':
            with pytest.raises(AssertionError, match=pat):
                call()
        else:
            with pytest.raises(EngineError, match='engine error -1: ' + pat):
                call()
        sv.set_instance_models(None)
        call()
        sv.sync()
    # what does not read the table runs with any B while it is set
    s.set_instance_models(tables)
    s.check_trajectory(small[1])
    s.plant_step(small[0], small[2][:, 0], tables[:B_CALL])
    with pytest.raises(EngineError, match=r'engine error -4: smpc_rollout_batch: an instance model table is set'):
        s.rollout(x0, xg, ug, p, 2)
    # a refused set leaves the previous table in force
    want = [np.array(a) for a in s.solve(x0, xg, ug, p)] + [np.array(s.eval_nodes(xg, ug, p)['tau'])]
    same = lambda: all(np.array_equal(a, b) for a, b in zip([np.array(a) for a in s.solve(x0, xg, ug, p)] +
                                                             [np.array(s.eval_nodes(xg, ug, p)['tau'])], want))
    bad = tables.copy()
    bad['mass'][2, 1] = np.nan
    with pytest.raises(EngineError, match=r'engine error -1: smpc_set_instance_models: instance 2 \(of B=5\), joint 1: mass'):
        s.set_instance_models(bad)
    bad = tables.copy()
    bad['mass'][0, 0] = -1.0
    with pytest.raises(EngineError, match=r'instance 0 \(of B=5\), joint 0: mass is negative'):
        s.set_instance_models(bad)
    bad = tables.copy()
    bad['p0'][4, 3, 0] += 1e-9
    with pytest.raises(EngineError, match=r'instance 4 \(of B=5\), joint 3: p0 differs'):
        s.set_instance_models(bad)
    bad = tables.copy()
    bad['inertia'][1, 5, 4] = np.inf
    with pytest.raises(EngineError, match=r'instance 1 \(of B=5\), joint 5: inertia is not finite'):
        s.set_instance_models(bad)
    with pytest.raises(EngineError, match=r'engine error -1: bad batch size'):
        s._chk(s.L.smpc_set_instance_models(s.h, 0, tables.ctypes.data, 0))
    assert same()
    # with device pointers the seven fields are not read: a moved p0 there changes nothing
    moved = tables.copy()
    moved['p0'] += 0.1
    moved['tau_max'] *= 0.5
    s.set_instance_models(_dev_table(moved))
    assert same()
    # a new horizon keeps the table
    s.set_horizon(N)
    assert same()
    # an overwrite in place under a captured solve takes effect at the next replay; growth while capturing is refused
    other = mc.model_tables(par, prob.nq, 2 * B_SET)[B_SET:]
    dev_in = [_dev(a) for a in (x0, xg, ug, p)]
    eager = s.solve(*dev_in)
    out = tuple(torch.empty_like(a) for a in eager)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        s.solve(*dev_in, out=out)
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out[1].cpu().numpy(), want[1])
    s.set_instance_models(other)
    g.replay()
    torch.cuda.synchronize()
    replayed = out[1].cpu().numpy().copy()
    assert not np.array_equal(replayed, want[1])
    assert np.array_equal(replayed, np.array(s.solve(x0, xg, ug, p)[1]))
    big = _dev_table(mc.model_tables(par, prob.nq, 4 * B_SET))
    with pytest.raises(EngineError, match='engine error -4: .* while the stream is being captured'), warnings.catch_warnings():
        warnings.filterwarnings('ignore', 'The CUDA Graph is empty')
        with torch.cuda.graph(torch.cuda.CUDAGraph()):
            s.set_instance_models(big)
    torch.cuda.synchronize()
    assert np.array_equal(np.array(s.solve(x0, xg, ug, p)[1]), replayed)
    s.set_instance_models(None)
    s.rollout(x0, xg, ug, p, 2)
    # the parallel policy: its candidate slots are not instances
    parp, probp, netp = make_problem('parallel', N=4)
    cp = Cn.get_controller('parallel', parp, 3, N=4, device_state=True)
    xp_ = _dev(sample_instances(probp, 3, seed=2))
    cp.setGuess(xp_[:, None, :].repeat(1, 5, 1), torch.zeros((3, 4, 6), dtype=torch.float64, device='cuda:0'))
    cp.ocp_solver.set_instance_models(mc.model_tables(parp, 6, 3))
    with pytest.raises(EngineError, match=r'engine error -4: smpc_policy_step: .*parallel'):
        cp.step_on_device(xp_)
    cp.ocp_solver.set_instance_models(None)
    cp.step_on_device(xp_)
    cp.ocp_solver.sync()


# ---- 8. the closed loop ---------------------------------------------------------------------------------------------------------------
def test_device_closed_loop_with_the_plants_models_equals_the_host_loop_over_the_oracle(monkeypatch):
    """run_mpc(on_device=True, models='plant', noise=20) against run_mpc(on_device=False, models='plant', noise=20) over
    ModelOracleSolver: 'st', B = 8, N = 8, 6 steps, QP form pinned; tol_x 1e-4, tol_u 2e-3 (1 + max |u|), equal outcome lists
    (test_device_closed_loop_in_two_scenes_equals_the_per_scene_loops).  With the URDF's torque limits no torque row is active in
    these six steps, so the matched and the nominal run of the oracle agree to 8e-8 in u (printed): what tells a loop that dropped
    the models from one that kept them is tests 3 and 4 above, and here the hand-over itself -- the controller's handle is given
    ONE table before its first step, a [8, 6, 29] device tensor whose bits are the plant tables of seeds 0..7, and is left without
    one when the run ends."""
    from safe_mpc_amd import closed_loop as cl
    from safe_mpc_amd import controller as Cn
    N, B, steps = 8, 8, 6
    par, prob, net = make_problem('st', N=N)
    par.back_hor = 8
    x0 = sample_instances(prob, B, seed=5, vel_scale=0.1)
    xg, ug = np.repeat(x0[:, None, :], N + 1, axis=1), np.zeros((B, N, 6))
    mk, mkb = mc.oracle_factories(par, N)
    ref = cl.run_mpc(par, 'st', xg, ug, noise=20.0, make_controller=mk, make_backup=mkb, n_steps=steps, models='plant')
    nominal = cl.run_mpc(par, 'st', xg, ug, noise=20.0, make_controller=mk, make_backup=mkb, n_steps=steps)
    tol_x, tol_u = 1e-4, 2e-3 * (1 + np.nanmax(np.abs(ref['u'])))
    print('closed loop: matched against nominal on the oracle: u', np.nanmax(np.abs(ref['u'] - nominal['u'])), '; tolerance', tol_u)
    from safe_mpc_amd.solver import BatchedOcpSolver
    given, real = [], BatchedOcpSolver.set_instance_models

    def recording(self, joints=None):
        given.append((self.problem.controller, None if joints is None else joints.cpu().numpy().copy()))
        return real(self, joints)
    monkeypatch.setattr(BatchedOcpSolver, 'set_instance_models', recording)

    def mkd(name, batch):
        c = Cn.get_controller(name, par, batch, device=0, device_state=True)
        c.ocp_solver.set_qp_mode('throughput')
        return c

    def mkbd(batch):
        c = Cn.SafeBackupController(par, batch, device=0, device_state=True)
        c.ocp_solver.set_qp_mode('throughput')
        return c
    res = cl.run_mpc(par, 'st', xg, ug, noise=20.0, n_steps=steps, on_device=True, groups=1, make_controller=mkd, make_backup=mkbd,
                     models='plant')
    main = [g for g in given if g[0] == 'st']
    want = mc.model_tables(par, 6, B).view(np.float64).reshape(B, 6, -1)
    assert len(main) == 2 and np.array_equal(main[0][1], want) and main[1][1] is None
    assert all(g[1] is None for g in given if g[0] != 'st')              # (no abort event: the backup handle is only cleared)
    assert np.array_equal(np.isnan(res['x']), np.isnan(ref['x'])) and np.array_equal(np.isnan(res['u']), np.isnan(ref['u']))
    for key in ('conv_idx', 'collisions_idx', 'viable_idx', 'unconv_idx'):
        assert sorted(res[key]) == sorted(ref[key]), key
    print('closed loop: x error', np.nanmax(np.abs(res['x'] - ref['x'])), 'u error', np.nanmax(np.abs(res['u'] - ref['u'])))
    assert np.nanmax(np.abs(res['x'] - ref['x'])) < tol_x and np.nanmax(np.abs(res['u'] - ref['u'])) < tol_u


# ---- 9. an overwrite in place under a captured loop step --------------------------------------------------------------------------------
def test_an_overwrite_in_place_reaches_the_next_replay_of_a_captured_group_step():
    """_DeviceGroup on the tightened-torque problem (the model decides the control), 'naive', B = 8: the first half of a step
    (smpc_loop_pre + smpc_policy_step) runs eagerly three times and is captured as a hipGraph at the fourth (_run_half); then the
    table is overwritten in place (same B) and the graph replayed.  The replayed step's controls are bit for bit those of the same
    sequence run eagerly, and differ from the fifth step of a run that kept the first table."""
    import torch
    from safe_mpc_amd import closed_loop as cl
    from safe_mpc_amd import controller as Cn
    from safe_mpc_amd.solver import BatchedOcpSolver
    (par, prob, net), tables, x0, probs = mc.clip_family()
    B, N = len(x0), prob.N
    first, second = _dev_table(tables), _dev_table(tables[::-1].copy())
    xg, ug = np.repeat(x0[:, None, :], N + 1, axis=1), np.zeros((B, N, prob.nu))

    def fifth_step(graphs, swap):
        ctrl = Cn.NaiveController.__new__(Cn.NaiveController)
        Cn.AbstractController.__init__(ctrl, par, B, 'ext', N, solver=BatchedOcpSolver(prob, net), net=net, device_state=True)
        sv = ctrl.ocp_solver
        sv.set_qp_mode('throughput')
        backup = Cn.SafeBackupController(par, B, device_state=True)
        with torch.cuda.stream(torch.cuda.ExternalStream(sv.L.smpc_stream(sv.h), device=torch.device('cuda', sv.device))):
            grp = cl._DeviceGroup(par, xg, ug, 0.0, 0.0, ctrl, backup, 8, 0, False, use_graphs=graphs)
            sv.set_instance_models(first)
            for j in range(4):
                grp._run_half('a', grp.part_a, j)
            assert ('a' in grp._graphs) == graphs
            if swap:
                sv.set_instance_models(second)
            grp._run_half('a', grp.part_a, 4)
            u = grp.u.clone()
        sv.sync()
        torch.cuda.synchronize()
        sv.set_instance_models(None)
        return u.cpu().numpy()
    replayed, eager, kept = fifth_step(True, True), fifth_step(False, True), fifth_step(False, False)
    assert np.array_equal(replayed, eager)
    assert np.abs(replayed - kept).max() > 1e-3
