"""A safe-set network with a per-instance context on the GPU.  -m gpu only.

The engine with instance contexts is held against the CPU oracle on ``net.folded(c)``, a plain network per context, composed in
instance order (context_cases.py); the oracle has no notion of a context.  Z1, N = 4.  The three code paths of the network pass
(k_mlp_fused, k_mlp_wave, k_nn_features + the GEMM chain) are chosen by knobs that are read once per process, so the parity and
bit-equality tests run again in two child processes."""
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch  # noqa: F401  (before the engine's library is loaded: PyTorch-ROCm must find the HIP runtime it ships with)

import context_cases as cc
from conftest import constant_guess, make_problem, sample_instances

pytestmark = pytest.mark.gpu
N = 4


def _rel(a, b):
    return np.abs(a - b).max() / (1e-12 + np.abs(b).max())


def _inputs(controller, B, seed=3):
    par, prob, net = cc.context_problem(controller, N)
    x0 = sample_instances(prob, B, seed=seed, vel_scale=0.3)
    xg, ug, p = constant_guess(prob, x0)
    xg[:, 1:] += 0.05 * np.random.default_rng(seed).standard_normal(xg[:, 1:].shape)
    if controller == 'receding':
        # the row on at two nodes per instance (one running node and the end node): the mode-3 list is shorter than its capacity
        p[:, 1:N, 4] = -1.0
        p[np.arange(B), 1 + np.arange(B) % (N - 1), 4] = 1.0
    return x0, xg, ug, p


# ---- 1. the engine against the folded oracles -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('controller,B', [('st', 5), ('st', 17), ('receding', 5)])
def test_engine_against_the_folded_oracle(controller, B):
    """eval_nodes with instance contexts b % 3: the terminal row at B = 5 (one block of 16 rows, 5 live) and B = 17 (instance 16 is
    row 0 of a second block), the row on two nodes per instance through the unordered mode-3 list.  Tolerances of
    test_gpu_parity.py for the network row.  A wrong row-to-instance rule fails: the oracle with the contexts rotated by one
    instance is shown to be 100 tolerances away first."""
    x0, xg, ug, p = _inputs(controller, B)
    ctx, idx = cc.instance_contexts(B)
    ref = cc.oracle_by_context(controller, 'eval_nodes', idx, [xg, ug, p])
    rot = cc.oracle_by_context(controller, 'eval_nodes', (idx + 1) % 3, [xg, ug, p])
    on = p[:, :, 4] > 0
    on[:, 0] = False
    if controller == 'st':
        on[:, :N] = False
    assert on.sum() == (B if controller == 'st' else 2 * B)
    assert np.all(ref['nn_val'][~on] == 0.0) and np.all(np.abs(ref['nn_val'][on]) > 0)
    apart = _rel(rot['nn_val'], ref['nn_val'])
    print('contexts rotated by one instance: nn_val apart by', apart)
    assert apart > 100 * 2e-5
    s = cc.engine(controller, N)
    s.set_instance_context(ctx)
    a = s.eval_nodes(xg, ug, p)
    print('nn_val error', _rel(a['nn_val'], ref['nn_val']), 'nn_grad error', _rel(a['nn_grad'][..., :12], ref['nn_grad'][..., :12]))
    assert _rel(a['nn_val'], ref['nn_val']) < 2e-5
    assert _rel(a['nn_grad'][..., :12], ref['nn_grad'][..., :12]) < 2e-4
    assert np.all(a['nn_val'][~on] == 0.0) and np.all(a['nn_grad'][~on] == 0.0)
    # without an instance context every row takes the default context
    s.set_instance_context(None)
    d = s.eval_nodes(xg, ug, p)
    dref = cc.folded_solvers(controller, N)[3].eval_nodes(xg, ug, p)
    assert _rel(d['nn_val'], dref['nn_val']) < 2e-5 and _rel(d['nn_grad'][..., :12], dref['nn_grad'][..., :12]) < 2e-4


@pytest.mark.parametrize('controller', ['st', 'receding'])
def test_solve_against_the_folded_oracle(controller):
    """the same through solve (the stage builder reads the row the pass wrote), at the solve tolerance of test_gpu_parity.py with a
    network: 1e-4 (1 + |u|)"""
    B = 5
    x0, xg, ug, p = _inputs(controller, B, seed=2)
    ctx, idx = cc.instance_contexts(B)
    xb, ub, sb, ib = cc.oracle_by_context(controller, 'solve', idx, [x0, xg, ug, p])
    s = cc.engine(controller, N)
    s.set_instance_context(ctx)
    xa, ua, sa, ia = s.solve(x0, xg, ug, p)
    assert np.array_equal(sa, sb)
    ok = sb == 0
    assert ok.sum() >= B - 1
    print('solve: u error', np.abs(ua[ok] - ub[ok]).max(), 'x error', np.abs(xa[ok] - xb[ok]).max())
    assert np.abs(ua[ok] - ub[ok]).max() < 1e-4 * (1 + np.abs(ub[ok]).max())
    assert np.abs(xa[ok] - xb[ok]).max() < 1e-4


# ---- 2. bit equality ----------------------------------------------------------------------------------------------------------------
def _bits(s, x0, xg, ug, p):
    ev = s.eval_nodes(xg, ug, p)
    return [np.array(ev['nn_val']), np.array(ev['nn_grad'])] + [np.array(a) for a in s.solve(x0, xg, ug, p)]


def _same(a, b):
    return all(np.array_equal(u, v) for u, v in zip(a, b))


@pytest.mark.parametrize('controller', ['st', 'receding'])
def test_bit_equality_of_the_paths_without_a_context(controller):
    from safe_mpc_amd import _lib
    from safe_mpc_amd.solver import BatchedOcpSolver
    B = 17
    par, prob, net = cc.context_problem(controller, N)
    x0, xg, ug, p = _inputs(controller, B)
    plain = net.folded(net.ctx_mean)           # the state columns and b0: an all-zero normalised context folds to nothing
    assert np.array_equal(plain.biases[0], net.biases[0])
    s0 = BatchedOcpSolver(prob, plain)
    want = _bits(s0, x0, xg, ug, p)
    # context columns with an all-zero normalised context = no context columns at all
    s = BatchedOcpSolver(prob, None)
    s.set_mlp(net, ctx_default=net.ctx_mean)
    assert _same(_bits(s, x0, xg, ug, p), want)
    s.set_instance_context(np.repeat(net.ctx_mean[None], B, axis=0))
    assert _same(_bits(s, x0, xg, ug, p), want)
    # an instance context equal to the default for every instance = the default alone; host and device pointers alike
    s.set_mlp(net, ctx_default=cc.DEFAULT)
    alone = _bits(s, x0, xg, ug, p)
    assert not np.array_equal(alone[0], want[0])
    s.set_instance_context(np.repeat(cc.DEFAULT[None], B, axis=0))
    assert _same(_bits(s, x0, xg, ug, p), alone)
    ctx, _ = cc.instance_contexts(B)
    s.set_instance_context(ctx)
    host = _bits(s, x0, xg, ug, p)
    assert not np.array_equal(host[0], alone[0])
    s.set_instance_context(torch.tensor(ctx, dtype=torch.float64, device='cuda:0'))
    assert _same(_bits(s, x0, xg, ug, p), host)
    # no context: the handle that never saw smpc_set_mlp_context, then with context columns set and cleared (both ways)
    s0.set_mlp(net, ctx_default=cc.DEFAULT)
    assert _same(_bits(s0, x0, xg, ug, p), alone)
    s0._chk(_lib.lib().smpc_set_mlp_context(s0.h, 0, None, None, None, None, 0))
    assert _same(_bits(s0, x0, xg, ug, p), want)
    s0.set_mlp(net, ctx_default=cc.DEFAULT)
    s0.set_mlp(plain)
    assert _same(_bits(s0, x0, xg, ug, p), want)


# ---- 3. the three code paths of the network pass ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('knob', ['SMPC_MLP_FUSED_MAX', 'SMPC_MLP_UNFUSED'])
def test_network_paths_in_child_processes(knob):
    """SMPC_MLP_FUSED_MAX=1: every pass is k_mlp_wave; SMPC_MLP_UNFUSED=1: k_nn_features and the layer-by-layer GEMMs.  Both knobs are
    read once per process, so the parity and bit-equality tests above run again in a child process each."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, **{knob: '1'})
    r = subprocess.run([sys.executable, '-m', 'pytest', os.path.join(root, 'tests', 'test_safe_set_context_gpu.py'), '-m', 'gpu', '-q', '-x',
                        '-k', 'test_engine_against_the_folded_oracle or test_solve_against_the_folded_oracle or test_bit_equality'],
                       env=env, cwd=root, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert '7 passed' in r.stdout, r.stdout[-500:]


# ---- 4. the forward-only consumers ------------------------------------------------------------------------------------------------------
def _g_values(fnet, par, x):
    """g = nn(s) (100 - alpha) / 100 - |v| of the folded net on states x [..., nx], torch fp32 forward (safe_set.py:82-94)"""
    nq = 6
    q, v = x[..., :nq].reshape(-1, nq), x[..., nq:].reshape(-1, nq).copy()
    v[:, 0] += par.eps
    vn = np.linalg.norm(v, axis=1)
    y, _ = fnet.torch_value_and_grad(np.hstack([(q - fnet.mean) / fnet.std, v / vn[:, None]]))
    return (y.astype(float) * (100.0 - par.alpha) / 100.0 - vn).reshape(x.shape[:-1])


def _shared_states(prob, n, seed):
    """n states, the same for every instance: outputs then differ between instances by their context only"""
    return sample_instances(prob, n, seed=seed, vel_scale=0.3)


def test_verdicts_of_the_forward_only_consumers_follow_the_context():
    """every instance the same states, the contexts b % 3; tol_safe = minus the midpoint of two instances' oracle values, so the
    verdicts provably differ between them -- asserted of the oracle's verdicts before the engine's are looked at.
    check_trajectory(want_nn) with 3 nodes (a node count that is not N + 1), check_guess(safe_node = N), score_rollout(want_safe) at
    B = 3 with n_steps = 4 (the step-major log: row j B + b belongs to instance b)."""
    par, prob, net = cc.context_problem('st', N)
    folded = [net.folded(c) for c in cc.CONTEXTS]
    s = cc.engine('st', N)

    # check_trajectory: B = 6 instances x 3 nodes
    B = 6
    ctx, idx = cc.instance_contexts(B)
    xs = _shared_states(prob, 3, seed=5)
    x = np.ascontiguousarray(np.repeat(xs[None], B, axis=0))
    g = np.stack([_g_values(folded[c], par, xs) for c in idx])                  # [B, 3]
    mid = 0.5 * (g[0, 1] + g[1, 1])
    want = g >= mid
    print('check_trajectory: oracle g', g[:3].tolist(), 'threshold', mid)
    assert want[0, 1] != want[1, 1] and np.abs(g - mid).min() > 1e-3
    s.set_instance_context(ctx)
    ok, nn_ok = s.check_trajectory(x, want_nn=True, tol_safe=-mid)
    assert np.array_equal(nn_ok, want)

    # check_guess: the safe-set test at node N of a constant guess
    xg, ug, p = constant_guess(prob, np.repeat(xs[:1], B, axis=0))
    gN = np.array([_g_values(folded[c], par, xs[0]) for c in idx])
    mid = 0.5 * (gN[1] + gN[2])
    want = gN >= mid
    assert want[1] != want[2] and np.abs(gN - mid).min() > 1e-3      # (margins 20 times the fp32 pass's 2e-5 (1 + |g|))
    flags, worst = s.check_guess(xg, ug, safe_node=N, tol_safe=-mid)
    assert np.array_equal((flags & 16) == 0, want)
    assert np.all(np.abs(-worst[:, 4] - gN) < 2e-5 * (1 + np.abs(gN)))
    s.set_instance_context(None)

    # score_rollout: B = 3, n_steps = 4
    B, n_steps = 3, 4
    ctx, idx = cc.instance_contexts(B)
    xs = _shared_states(prob, n_steps + 1, seed=6)
    x_log = np.ascontiguousarray(np.repeat(xs[:, None, :], B, axis=1))          # [n_steps + 1, B, nx]
    u_log = np.zeros((n_steps, B, 6))
    g = np.stack([_g_values(folded[c], par, xs) for c in idx])                  # [B, n_steps + 1]
    print('score_rollout: oracle least g per instance', g.min(1).tolist(), 'at', g.argmin(1).tolist())
    assert np.abs(g.min(1)[:, None] - g.min(1)[None, :])[~np.eye(B, dtype=bool)].min() > 1e-3
    s.set_instance_context(ctx)
    so, si = s.score_rollout(x_log, u_log, want_safe=True)
    assert np.all(np.abs(so[:, 6] - g.min(1)) < 2e-5 * (1 + np.abs(g.min(1))))
    assert np.array_equal(si[:, 3], g.argmin(1))
    # merit_terms runs the network on the mode-3 list of the [B][N+1] arrays: with every instance's context it is the sum of the
    # per-context calls
    x0 = np.repeat(xs[:1], B, axis=0)
    xg, ug, p = constant_guess(prob, x0)
    both = np.array(s.merit_terms(x0, xg, ug, p))
    for b in range(B):
        s.set_instance_context(np.repeat(cc.CONTEXTS[idx[b]][None], B, axis=0))
        assert np.array_equal(np.array(s.merit_terms(x0, xg, ug, p))[b], both[b])


# ---- 5. guards ------------------------------------------------------------------------------------------------------------------------
def test_misuse_is_refused_by_name(monkeypatch):
    from safe_mpc_amd import _lib
    from safe_mpc_amd import controller as C
    from safe_mpc_amd._lib import EngineError
    from safe_mpc_amd.solver import BatchedOcpSolver
    par, prob, net = cc.context_problem('st', N)
    B = 6
    x0, xg, ug, p = _inputs('st', B)
    ctx, _ = cc.instance_contexts(B)
    s = cc.engine('st', N)
    s.set_instance_context(ctx)
    # another batch size: refused, both sizes named -- by every entry point that runs the network
    small = (x0[:4], xg[:4], ug[:4], p[:4])
    for call in (lambda: s.solve(*small), lambda: s.eval_nodes(*small[1:]), lambda: s.merit_terms(*small),
                 lambda: s.check_guess(xg[:4], ug[:4], safe_node=N), lambda: s.check_trajectory(xg[:4], want_nn=True),
                 lambda: s.score_rollout(np.zeros((3, 4, 12)), np.zeros((2, 4, 6)), want_safe=True), lambda: s.sqp(*small)):
        with pytest.raises(EngineError, match=r'engine error -1: .*batch size 4, .*context was set for 6 instances'):
            call()
    # smpc_rollout_batch: refused while an instance context is set; with the default context alone it runs, and its worker handles
    # read the same default row (two sub-batches give the bits of one)
    with pytest.raises(EngineError, match=r'engine error -4: smpc_rollout_batch: an instance context'):
        s.rollout(x0, xg, ug, p, 2)
    s.set_instance_context(None)
    one = s.rollout(x0, xg, ug, p, 2)
    monkeypatch.setenv('SMPC_ROLLOUT_STREAMS', '2')
    two = s.rollout(x0, xg, ug, p, 2)
    monkeypatch.delenv('SMPC_ROLLOUT_STREAMS')
    assert all(np.array_equal(a, b) for a, b in zip(one, two))
    sp = BatchedOcpSolver(prob, net.folded(cc.DEFAULT))
    ref = sp.rollout(x0, xg, ug, p, 2)
    assert np.array_equal(one[2], ref[2]) and np.abs(one[1] - ref[1]).max() < 1e-4 * (1 + np.abs(ref[1]).max())
    # a non-finite context (host pointers) is refused and the old one stays
    s.set_instance_context(ctx)
    before = s.eval_nodes(xg, ug, p)['nn_val'].copy()
    bad = ctx.copy()
    bad[4, 2] = np.inf
    with pytest.raises(EngineError, match=r'engine error -1: context of instance 4 \(of B=6\), number 2'):
        s.set_instance_context(bad)
    assert np.array_equal(s.eval_nodes(xg, ug, p)['nn_val'], before)
    # a larger context while the stream is being captured: refused (the copy would have to grow), the capture ends cleanly
    big = torch.zeros((64 * B, cc.N_CTX), dtype=torch.float64, device='cuda:0')
    with pytest.raises(EngineError, match='engine error -4: .* while the stream is being captured'), warnings.catch_warnings():
        warnings.filterwarnings('ignore', 'The CUDA Graph is empty')
        with torch.cuda.graph(torch.cuda.CUDAGraph()):
            s.set_instance_context(big)
    torch.cuda.synchronize()
    assert np.array_equal(s.eval_nodes(xg, ug, p)['nn_val'], before)
    # smpc_set_mlp drops the context columns, and with them the instance context
    s.set_mlp(net.folded(cc.DEFAULT))
    with pytest.raises(EngineError, match=r'engine error -1: .*no context columns'):
        s._chk(_lib.lib().smpc_set_instance_context(s.h, B, ctx.ctypes.data, 0))
    s.eval_nodes(*small[1:])
    # too many context numbers: refused with the limit; bad normalisation; no network
    L = _lib.lib()
    wide = cc.context_net(prob, par, n_ctx=5)
    with pytest.raises(EngineError, match=r'engine error -1: .*n_ctx=5 outside 0\.\.4'):
        s.set_mlp(wide)
    Wc = np.ascontiguousarray(net.weights[0][:, 12:])
    m, sd_, d = np.zeros(4), np.ones(4), np.zeros(4)
    call = lambda Wc, m, sd_, d: s._chk(L.smpc_set_mlp_context(s.h, 4, Wc.ctypes.data, m.ctypes.data, sd_.ctypes.data, d.ctypes.data, 0))
    with pytest.raises(EngineError, match=r'engine error -1: .*ctx_std\[1\] = 0: must be > 0'):
        call(Wc, m, np.array([1.0, 0.0, 1.0, 1.0]), d)
    with pytest.raises(EngineError, match=r'engine error -1: .*context number 3 is not finite'):
        call(Wc, m, sd_, np.array([0.0, 0.0, 0.0, np.nan]))
    Wbad = Wc.copy()
    Wbad[7, 1] = np.nan
    with pytest.raises(EngineError, match=r'engine error -1: .*Wc\[7\]\[1\] is not finite'):
        call(Wbad, m, sd_, d)
    call(Wc, m, sd_, d)
    s0 = BatchedOcpSolver(prob, None)
    with pytest.raises(EngineError, match=r'engine error -4: .*smpc_set_mlp was not called'):
        s0._chk(L.smpc_set_mlp_context(s0.h, 4, Wc.ctypes.data, m.ctypes.data, sd_.ctypes.data, d.ctypes.data, 0))
    # the parallel policy: its candidate slots are not instances; with the default context alone it runs
    parp, probp, _ = make_problem('parallel', N=4)
    parp.net_size = [12 + cc.N_CTX, 256, 1]
    ctrl = C.get_controller('parallel', parp, 3, N=4, device_state=True)
    assert ctrl.net.n_ctx == cc.N_CTX
    xp = torch.tensor(sample_instances(probp, 3, seed=2), dtype=torch.float64, device='cuda:0')
    ctrl.setGuess(xp[:, None, :].repeat(1, 5, 1), torch.zeros((3, 4, 6), dtype=torch.float64, device='cuda:0'))
    ctrl.ocp_solver.set_instance_context(cc.CONTEXTS)
    with pytest.raises(EngineError, match=r'engine error -4: smpc_policy_step: an instance context .*parallel'):
        ctrl.step_on_device(xp)
    ctrl.ocp_solver.set_instance_context(None)
    ctrl.step_on_device(xp)
    ctrl.ocp_solver.sync()


# ---- 6. the pipeline: rays labelled in scenes of their own, a net fitted with the context, a closed loop that uses it -------------------
def _scene_pars(make, second):
    import scene_cases as sc
    pars = []
    for shift in (sc.SHIFTS[0], second):
        par = make()
        sc.move_obstacles(par, shift, sc.Z1_OBSTACLES)
        pars.append(par)
    return pars


def test_pipeline_label_fit_checkpoint_closed_loop(tmp_path):
    """label_rays on 8 rays with two scenes alternating (QP form pinned): per ray exactly the result of the same rays labelled with
    scene 0 for all (even rays) and scene 1 for all (odd rays), and every certificate passes check_guess in its own scene.  Then
    fit_safe_set(context=...) for two epochs -> save_checkpoint -> get_controller with that network_path -> run_mpc(scenes=...), two
    steps on the device path, against the host path on oracle doubles that hold the FOLDED net of every scene, at the tolerances of
    test_scene_gpu.py for that comparison (x 1e-4, u 2e-3 (1 + |u|))."""
    import ray_cases as rc
    import scene_cases as sc
    from fake_solver import OracleSolver
    from oracle.oracle import Oracle
    from safe_mpc_amd import closed_loop as cl
    from safe_mpc_amd import controller as C
    from safe_mpc_amd import safe_set_data as sd
    from safe_mpc_amd.problem import scene_context, scenes_from_problems
    from safe_mpc_amd.safe_set import SafeSetNet
    # scene 1 of the labelling: the gate moved onto the configurations of rays 5 and 6, which are DEAD there and BRACKETED / SATURATED
    # in scene 0 -- one odd and one even ray, so a ray labelled in its neighbour's scene changes its kind either way
    bprobs = [C.OcpProblem(p, 'backup', 'zero', N=rc.N) for p in _scene_pars(rc.ray_params, (-0.4, -0.1, 0.2))]
    geoms = scenes_from_problems(bprobs[0], bprobs)
    n = 8
    q, d, s_hi = (a[:n] for a in rc.random_rays())
    scenes = np.ascontiguousarray(geoms[np.arange(n) % 2])

    def label(sc_):
        return sd.label_rays(rc.engine_controller(n), q, d, s_hi, bisect=rc.BISECT, budget=rc.BUDGET, check_every=rc.CHECK_EVERY, batch=n,
                             scenes=sc_)
    mixed, all0, all1 = label(scenes), label(np.repeat(geoms[:1], n, axis=0)), label(np.repeat(geoms[1:], n, axis=0))
    print('kinds: mixed', mixed['kind'].tolist(), 'scene 0', all0['kind'].tolist(), 'scene 1', all1['kind'].tolist())
    print('labels: scene 0', np.round(all0['label'], 4).tolist(), 'scene 1', np.round(all1['label'], 4).tolist())
    even = np.arange(n) % 2 == 0
    differ = all0['kind'] != all1['kind']
    assert (differ & even).any() and (differ & ~even).any(), differ
    for k in ('label', 'kind', 'lo', 'hi', 'trials', 'iters', 'x_cert', 'u_cert'):
        want = np.where(even.reshape((n,) + (1,) * (all0[k].ndim - 1)), all0[k], all1[k])
        assert np.array_equal(mixed[k], want, equal_nan=True), k
    sv = rc.engine_controller(n).ocp_solver
    sv.set_instance_scene(scenes)
    flags, _ = sv.check_guess(mixed['x_cert'], mixed['u_cert'], safe_node=None, collision_first_node=0)
    alive = mixed['kind'] != sd.DEAD
    assert alive.sum() >= 2 and np.all(flags[alive] == 0), flags

    # the fit with the context, the checkpoint, the controller
    Nn, steps, B = 6, 2, 4
    pars = _scene_pars(rc.ray_params, sc.SHIFTS[3])
    hprobs = [C.OcpProblem(p, 'htwa', 'ext', N=Nn) for p in pars]
    hgeoms = scenes_from_problems(hprobs[0], hprobs)
    r = [i for i, name in enumerate(hprobs[0].row_obstacle) if name in sc.Z1_OBSTACLES][0]
    select = [(r, 1), (r, 4)]                                 # the y of the first gate capsule's two end points: what the shift moves
    ctxs = scene_context(hgeoms, select)
    assert np.abs(ctxs[0] - ctxs[1]).min() > 0.1
    fit_par = rc.ray_params()
    fit_par.net_size = [2 * rc.NQ + 2, 32, 1]
    data = {'q': q, 'd': d, 'label': mixed['label'], 'kind': mixed['kind']}
    net, mean, std, info = sd.fit_safe_set(data, fit_par, epochs=2, seed=0, context=scene_context(hgeoms[np.arange(n) % 2], select))
    path = str(tmp_path / 'safe_set_ctx.pt')
    sd.save_checkpoint(path, net, mean, std, info['ctx_mean'], info['ctx_std'], select)
    for p in pars:
        p.net_path, p.use_net, p.N, p.back_hor, p.net_size = path, True, Nn, 8, [2 * rc.NQ, 32, 1]
    cnet = SafeSetNet.from_params(pars[0])
    assert cnet.n_ctx == 2 and cnet.ctx_select == select
    folded = [cnet.folded(c) for c in ctxs]
    assert np.abs(folded[0].biases[0] - folded[1].biases[0]).max() > 1e-3           # the scenes' nets are told apart
    pool = sample_instances(hprobs[0], 24, seed=4, vel_scale=0.1)
    o1 = Oracle(hprobs[1])
    free = o1.check_trajectory(pool[:, None, :], hprobs[1].x_min, hprobs[1].x_max, 0.0, hprobs[1].row_lb, hprobs[1].row_ub).astype(bool)
    x0 = pool[free][:B]
    assert len(x0) == B
    xg, ug = np.repeat(x0[:, None, :], Nn + 1, axis=1), np.zeros((B, Nn, 6))
    scenes4 = np.ascontiguousarray(hgeoms[np.arange(B) % 2])

    def mk(name, batch):
        c = C.get_controller(name, pars[0], batch, device=0, device_state=True)
        c.ocp_solver.set_qp_mode('throughput')
        return c

    def mkb(batch):
        c = C.SafeBackupController(pars[0], batch, device=0, device_state=True)
        c.ocp_solver.set_qp_mode('throughput')
        return c
    res = cl.run_mpc(pars[0], 'htwa', xg, ug, n_steps=steps, on_device=True, groups=1, make_controller=mk, make_backup=mkb, scenes=scenes4)

    def build(cls, name, cost, horizon, batch):
        ctrl = cls.__new__(cls)
        prob = C.OcpProblem(pars[0], name, cost, N=horizon)
        prob.set_normalisation(cnet.mean, cnet.std)
        subs = []
        for sp in pars:
            pr = C.OcpProblem(sp, name, cost, N=horizon)
            pr.set_normalisation(cnet.mean, cnet.std)
            subs.append(pr)
        shared = cnet.folded(prob.context_default(select))
        solver = sc.SceneOracleSolver(prob, shared, subs, hgeoms)
        solver.subs = [OracleSolver(pr, f) for pr, f in zip(subs, folded)]       # every scene's oracle holds the net folded for it
        C.AbstractController.__init__(ctrl, pars[0], batch, cost, horizon, solver=solver, net=shared)
        return ctrl
    ref = cl.run_mpc(pars[0], 'htwa', xg, ug, n_steps=steps, scenes=scenes4,
                     make_controller=lambda name, batch: build(C.CONTROLLERS[name], C.CONTROLLERS[name].cont_name, 'ext', Nn, batch),
                     make_backup=lambda batch: build(C.SafeBackupController, 'backup', 'zero', pars[0].back_hor, batch))
    tol_x, tol_u = 1e-4, 2e-3 * (1 + np.nanmax(np.abs(ref['u'])))
    print('closed loop: x error', np.nanmax(np.abs(res['x'] - ref['x'])), 'u error', np.nanmax(np.abs(res['u'] - ref['u'])), 'tolerances', tol_x, tol_u)
    assert np.array_equal(np.isnan(res['x']), np.isnan(ref['x'])) and np.array_equal(np.isnan(res['u']), np.isnan(ref['u']))
    assert np.nanmax(np.abs(res['x'] - ref['x'])) < tol_x and np.nanmax(np.abs(res['u'] - ref['u'])) < tol_u
    for key in ('conv_idx', 'collisions_idx', 'viable_idx', 'unconv_idx'):
        assert sorted(res[key]) == sorted(ref[key]), key
