"""A safe-set context that follows a scene track on the GPU.  -m gpu only.

The engine with a context track is held against the CPU oracle on ``net.folded(ctx[b, col(t + k)])``, a plain network per context,
recomposed NODE BY NODE (context_track_cases.py); the oracle has no notion of a context or of a track.  Z1, N = 4, T = 3, the context
of (instance b, column c) being CONTEXTS[(b + c) % 3]; clocks none, -3, -2, 0 and 7.  The three code paths of the network pass
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
import context_track_cases as ctc
import track_cases as tc
from conftest import constant_guess, make_problem, sample_instances

pytestmark = pytest.mark.gpu
N, T = ctc.N, ctc.T
TOL_VAL, TOL_GRAD = 2e-5, 2e-4          # the project's own for the network row (test_safe_set_context_gpu.py), relative as _rel


def _rel(a, b):
    return np.abs(a - b).max() / (1e-12 + np.abs(b).max())


def _inputs(controller, B, seed=3):
    """as _inputs of test_safe_set_context_gpu.py"""
    par, prob, net = cc.context_problem(controller, N)
    x0 = sample_instances(prob, B, seed=seed, vel_scale=0.3)
    xg, ug, p = constant_guess(prob, x0)
    xg[:, 1:] += 0.05 * np.random.default_rng(seed).standard_normal(xg[:, 1:].shape)
    if controller == 'receding':
        # the row on at two nodes per instance (one running node and the end node): the mode-3 list is shorter than its capacity
        p[:, 1:N, 4] = -1.0
        p[np.arange(B), 1 + np.arange(B) % (N - 1), 4] = 1.0
    return x0, xg, ug, p


def _live(controller, p):
    on = p[:, :, 4] > 0
    on[:, 0] = False
    if controller == 'st':
        on[:, :N] = False
    return on


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a), device='cuda:0')


# ---- 1. eval_nodes against the folded oracles, node by node ---------------------------------------------------------------------------
@pytest.mark.parametrize('controller,B', [('st', 5), ('st', 17), ('receding', 5)])
def test_eval_nodes_against_the_folded_oracle_by_column(controller, B):
    """every clock of the family, and -7: the network row of node k of instance b against the oracle on net.folded(ctx[b, col(t + k)]) --
    one oracle call per distinct context, taking the nodes that see it.  The terminal row at B = 5 and B = 17 (instance 16 is row 0
    of a second block), the row on two nodes per instance through the unordered mode-3 list.  A wrong column rule fails: on oracle
    values alone, the recomposition with every column shifted by one (down and up) is shown to be more than 100 tolerances away on
    the live nodes whose column the shift changes -- among them the terminal node at t = -3 (column 1, both ways) and at t = -2
    (column 2, the last: downwards).  Rows that are off read exactly 0."""
    x0, xg, ug, p = _inputs(controller, B)
    ctx, idx = ctc.track_contexts(B)
    subs = cc.folded_solvers(controller, N)
    full = [subs[c].eval_nodes(xg, ug, p) for c in range(len(cc.CONTEXTS))]           # one oracle call per context, shared by all clocks
    on = _live(controller, p)
    assert on.sum() == (B if controller == 'st' else 2 * B)
    s = cc.engine(controller, N)
    s.set_instance_context_track(ctx)
    shown = set()
    for t in ctc.CLOCKS + [-7]:                             # (-7: the terminal node on the clamped FIRST column)
        seen = ctc.node_contexts(idx, t, N + 1)
        ref = tc.per_node(lambda c: full[c], seen)
        assert np.all(ref['nn_val'][~on] == 0.0) and np.all(np.abs(ref['nn_val'][on]) > 0)
        for d in (-1, 1):
            moved = ctc.node_contexts(idx, (0 if t is None else t) + d, N + 1)
            m = on & (moved != seen)                       # (the live nodes that are unclamped in this direction)
            if m.any():
                apart = np.abs(tc.per_node(lambda c: full[c], moved)['nn_val'][m] - ref['nn_val'][m]).max() / np.abs(ref['nn_val']).max()
                print('clock', t, 'columns shifted by', d, ': nn_val apart by', apart)
                assert apart > 100 * TOL_VAL
                if m[:, N].all():
                    shown.add((t, d))
        cell = ctc.set_clock(s, t)
        a = s.eval_nodes(xg, ug, p)
        ev, eg = _rel(a['nn_val'], ref['nn_val']), _rel(a['nn_grad'][..., :12], ref['nn_grad'][..., :12])
        print('clock', t, 'nn_val error', ev, 'nn_grad error', eg)
        assert ev < TOL_VAL and eg < TOL_GRAD
        assert np.all(a['nn_val'][~on] == 0.0) and np.all(a['nn_grad'][~on] == 0.0)
        del cell
    assert {(-3, -1), (-3, 1), (-2, -1)} <= shown, shown
    s.set_scene_clock(None)


# ---- 3. solve ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('controller', ['st', 'receding'])
def test_solve_against_the_folded_oracle_by_column(controller):
    """solve at clock -3 (the stage builder reads the row the pass wrote) against per-context oracle solves, 1e-4 (1 + |u|) as in
    test_safe_set_context_gpu.py, statuses equal.  'st': the one live node, N, sits in column col(-3 + 4) = 1.  'receding': the oracle
    solves with ONE network per instance, so p switches the row on at two running nodes of 1 .. 3 and off at the end node: at clock
    -3 they all read column 0 (k - 3 <= 0), and an instance's live nodes share its context idx[b, 0].
    (On these inputs the safe-set row is far from active: the oracle's u under the neighbouring context differs by 3e-10, so this
    test holds the path from the pass to the stage builder and the statuses, and the eval_nodes test above holds the column rule.)"""
    B, t = 5, -3
    x0, xg, ug, p = _inputs(controller, B, seed=2)
    ctx, idx = ctc.track_contexts(B)
    if controller == 'receding':
        p[:, 1:, 4] = -1.0
        p[np.arange(B), 1 + np.arange(B) % (N - 1), 4] = 1.0
        p[np.arange(B), 1 + (np.arange(B) + 1) % (N - 1), 4] = 1.0
    seen = ctc.node_contexts(idx, t, N + 1)
    on = _live(controller, p)
    per_inst = np.array([np.unique(seen[b][on[b]]) for b in range(B)])
    assert per_inst.shape == (B, 1)                         # an instance's live nodes share a column
    want = per_inst[:, 0]
    assert np.array_equal(want, idx[:, 1] if controller == 'st' else idx[:, 0]) and len(np.unique(want)) == 3
    xb, ub, sb, ib = cc.oracle_by_context(controller, 'solve', want, [x0, xg, ug, p])
    s = cc.engine(controller, N)
    s.set_instance_context_track(ctx)
    cell = ctc.set_clock(s, t)
    xa, ua, sa, ia = s.solve(x0, xg, ug, p)
    assert np.array_equal(sa, sb)
    ok = sb == 0
    assert ok.sum() >= B - 1
    print('solve: u error', np.abs(ua[ok] - ub[ok]).max(), 'x error', np.abs(xa[ok] - xb[ok]).max())
    assert np.abs(ua[ok] - ub[ok]).max() < 1e-4 * (1 + np.abs(ub[ok]).max())
    assert np.abs(xa[ok] - xb[ok]).max() < 1e-4
    s.set_scene_clock(None)
    del cell


# ---- 4. bit equality ----------------------------------------------------------------------------------------------------------------
def _bits(s, x0, xg, ug, p):
    ev = s.eval_nodes(xg, ug, p)
    return [np.array(ev['nn_val']), np.array(ev['nn_grad'])] + [np.array(a) for a in s.solve(x0, xg, ug, p)]


def _same(a, b):
    return all(np.array_equal(u, v) for u, v in zip(a, b))


@pytest.mark.parametrize('controller', ['st', 'receding'])
def test_bit_equality_of_constant_tracks_and_of_a_track_of_one_column(controller):
    """a track whose columns are all equal gives the bits of set_instance_context with that column, at every clock, for eval_nodes
    and solve, host and device pointers alike; set_instance_context(ctx) is the track [B, 1, n], whose clock is not read; and a
    track that does vary is told apart from all of these"""
    B = 17
    x0, xg, ug, p = _inputs(controller, B)
    ctx, _ = cc.instance_contexts(B)
    s = cc.engine(controller, N)
    s.set_instance_context(ctx)
    want = _bits(s, x0, xg, ug, p)
    const = np.ascontiguousarray(np.repeat(ctx[:, None], T, axis=1))
    for t in ctc.CLOCKS:
        cell = ctc.set_clock(s, t)
        s.set_instance_context_track(const if t != 0 else _dev(const))
        assert _same(_bits(s, x0, xg, ug, p), want), t
        # the track of one column, at a clock it does not read; and the 2-D setter under the same clock
        s.set_instance_context_track(np.ascontiguousarray(ctx[:, None]))
        assert _same(_bits(s, x0, xg, ug, p), want), t
        s.set_instance_context(ctx)
        assert _same(_bits(s, x0, xg, ug, p), want), t
        del cell
    moving, _ = ctc.track_contexts(B)
    s.set_instance_context_track(moving)
    assert not np.array_equal(_bits(s, x0, xg, ug, p)[0], want[0])
    s.set_scene_clock(None)


# ---- 2. the three code paths of the network pass ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('knob', ['SMPC_MLP_FUSED_MAX', 'SMPC_MLP_UNFUSED'])
def test_network_paths_in_child_processes(knob):
    """SMPC_MLP_FUSED_MAX=1: every pass is k_mlp_wave; SMPC_MLP_UNFUSED=1: k_nn_features and the layer-by-layer GEMMs.  Both knobs are
    read once per process, so the parity and bit-equality tests above run again in a child process each."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, **{knob: '1'})
    r = subprocess.run([sys.executable, '-m', 'pytest', os.path.join(root, 'tests', 'test_context_track_gpu.py'), '-m', 'gpu', '-q', '-x',
                        '-k', 'test_eval_nodes_against or test_solve_against or test_bit_equality'],
                       env=env, cwd=root, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert '7 passed' in r.stdout, r.stdout[-500:]


# ---- 5. the clock is read on the device ---------------------------------------------------------------------------------------------------
def test_a_captured_solve_follows_the_clock_cell_and_an_overwrite_in_place():
    B = 5
    x0, xg, ug, p = _inputs('st', B, seed=2)
    ctx, idx = ctc.track_contexts(B)
    other = np.ascontiguousarray(ctx[:, ::-1])              # the same (B, T), other contents
    s = cc.engine('st', N)
    s.set_instance_context_track(ctx)

    def eager(t, table):
        e = cc.engine('st', N)
        e.set_instance_context_track(table)
        c = ctc.set_clock(e, t)
        r = [np.array(a) for a in e.solve(x0, xg, ug, p)]
        del c
        return r
    at = {t: eager(t, ctx) for t in (-3, -2)}
    assert not np.array_equal(at[-3][1], at[-2][1])         # the terminal node in column 1, then in column 2
    cell = ctc.cell(-3)
    s.set_scene_clock(cell)
    dev_in = [_dev(a) for a in (x0, xg, ug, p)]
    out = tuple(torch.empty_like(a) for a in s.solve(*dev_in))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        s.solve(*dev_in, out=out)
    g.replay()
    torch.cuda.synchronize()
    assert all(np.array_equal(o.cpu().numpy(), w) for o, w in zip(out, at[-3]))
    cell.fill_(-2)                                          # the cell rewritten, nothing else: the replay follows it
    g.replay()
    torch.cuda.synchronize()
    assert all(np.array_equal(o.cpu().numpy(), w) for o, w in zip(out, at[-2]))
    s.set_instance_context_track(other)                     # overwritten in place: the captured step keeps seeing the buffer
    g.replay()
    torch.cuda.synchronize()
    want = eager(-2, other)
    assert not np.array_equal(want[1], at[-2][1])
    assert all(np.array_equal(o.cpu().numpy(), w) for o, w in zip(out, want))
    s.set_scene_clock(None)


# ---- 6. + 7. the forward-only consumers -----------------------------------------------------------------------------------------------
def _g_values(fnet, par, x):
    """g = nn(s) (100 - alpha) / 100 - |v| of the folded net on states x [..., nx], torch fp32 forward (safe_set.py:82-94)"""
    nq = 6
    q, v = x[..., :nq].reshape(-1, nq), x[..., nq:].reshape(-1, nq).copy()
    v[:, 0] += par.eps
    vn = np.linalg.norm(v, axis=1)
    y, _ = fnet.torch_value_and_grad(np.hstack([(q - fnet.mean) / fnet.std, v / vn[:, None]]))
    return (y.astype(float) * (100.0 - par.alpha) / 100.0 - vn).reshape(x.shape[:-1])


def _g_table(par, net, xs):
    """[context, state]: the oracle value of every context of the family on every state of xs"""
    return np.stack([_g_values(net.folded(c), par, xs) for c in cc.CONTEXTS])


def test_verdicts_of_check_trajectory_and_check_guess_follow_the_column():
    """every instance the same states; tol_safe = minus the midpoint of two COLUMNS' oracle values at one node, so the verdict
    provably depends on the column -- the verdicts with every column shifted by one are shown to differ before the engine's are
    looked at.  check_trajectory(want_nn) with n_nodes = 3 (not N + 1), check_guess(safe_node) at node N and at node 2."""
    par, prob, net = cc.context_problem('st', N)
    B, n_nodes = 3, 3
    ctx, idx = ctc.track_contexts(B)
    xs = sample_instances(prob, n_nodes, seed=5, vel_scale=0.3)
    G = _g_table(par, net, xs)                                                  # [context, node]
    x = np.ascontiguousarray(np.repeat(xs[None], B, axis=0))
    mid = 0.5 * (G[idx[0, 0], 1] + G[idx[0, 1], 1])                             # instance 0, node 1: column 0 against column 1
    print('check_trajectory: oracle g [context, node]', G.tolist(), 'threshold', mid)
    assert np.abs(G - mid).min() > 1e-3                                         # (margins 20 times the fp32 pass's 2e-5 (1 + |g|))
    s = cc.engine('st', N)
    s.set_instance_context_track(ctx)
    told_apart = 0
    for t in ctc.CLOCKS:
        seen = ctc.node_contexts(idx, t, n_nodes)
        want = G[seen, np.arange(n_nodes)[None, :]] >= mid
        shifted = ctc.node_contexts(idx, (0 if t is None else t) - 1, n_nodes)
        told_apart += not np.array_equal(G[shifted, np.arange(n_nodes)[None, :]] >= mid, want)
        cell = ctc.set_clock(s, t)
        ok, nn_ok = s.check_trajectory(x, want_nn=True, tol_safe=-mid)
        assert np.array_equal(nn_ok, want), t
        del cell
    assert told_apart >= 2
    # check_guess: the safe-set test at node N and at node 2 of a constant guess
    xg, ug, p = constant_guess(prob, np.repeat(xs[:1], B, axis=0))
    g0 = G[:, 0]
    mid = 0.5 * (g0[0] + g0[1])
    if abs(g0[2] - mid) < 1e-3:
        mid = 0.5 * (g0[1] + g0[2])
    assert np.abs(g0 - mid).min() > 1e-3
    told_apart = 0
    for t in ctc.CLOCKS:
        cell = ctc.set_clock(s, t)
        for node in (N, 2):
            c = idx[np.arange(B), tc.col((0 if t is None else t) + node, T)]
            want = g0[c] >= mid
            told_apart += not np.array_equal(g0[idx[np.arange(B), tc.col((0 if t is None else t) + node - 1, T)]] >= mid, want)
            flags, worst = s.check_guess(xg, ug, safe_node=node, tol_safe=-mid)
            assert np.array_equal((flags & 16) == 0, want), (t, node)
            assert np.all(np.abs(-worst[:, 4] - g0[c]) < 2e-5 * (1 + np.abs(g0[c]))), (t, node)
        del cell
    assert told_apart >= 2
    s.set_scene_clock(None)


def test_score_rollout_scores_state_j_in_column_j_whatever_the_clock():
    """B = 3, n_steps = 4, every instance the same states: the least safe-set value and its step follow col(j) -- the step-major
    log, row j B + b is state j of instance b -- whatever the clock cell holds"""
    par, prob, net = cc.context_problem('st', N)
    B, n_steps = 3, 4
    ctx, idx = ctc.track_contexts(B)
    xs = sample_instances(prob, n_steps + 1, seed=6, vel_scale=0.3)
    G = _g_table(par, net, xs)                                                  # [context, state]
    seen = ctc.log_contexts(idx, n_steps + 1)                                   # [state, B]
    g = G[seen, np.arange(n_steps + 1)[:, None]].T                              # [B, state]
    still = G[idx[:, 0]]                                                        # what a context that stands in column 0 would give
    print('score_rollout: oracle least g per instance', g.min(1).tolist(), 'at', g.argmin(1).tolist(), '; standing', still.min(1).tolist())
    assert np.abs(g.min(1) - still.min(1)).max() > 1e-3
    srt = np.sort(g, axis=1)
    assert (srt[:, 1] - srt[:, 0]).min() > 1e-3                                 # the step of the least value is decided
    x_log = np.ascontiguousarray(np.repeat(xs[:, None, :], B, axis=1))          # [n_steps + 1, B, nx]
    u_log = np.zeros((n_steps, B, 6))
    s = cc.engine('st', N)
    s.set_instance_context_track(ctx)
    for t in (None, 7, -3):
        cell = ctc.set_clock(s, t)
        so, si = s.score_rollout(x_log, u_log, want_safe=True)
        assert np.all(np.abs(so[:, 6] - g.min(1)) < 2e-5 * (1 + np.abs(g.min(1)))), t
        assert np.array_equal(si[:, 3], g.argmin(1)), t
        del cell
    # every state the same as well: all instances then report the same least value, that of the context with the least g, and the
    # STEP at which each reports it is one whose column shows that context in its own track (columns 2, 3, 4 of the log all read
    # column 2 and tie)
    Gs = G[:, 2]
    cmin = int(np.argmin(Gs))
    assert np.sort(Gs)[1] - Gs[cmin] > 1e-3
    x_same = np.ascontiguousarray(np.broadcast_to(xs[2], (n_steps + 1, B, 12)))
    so, si = s.score_rollout(x_same, u_log, want_safe=True)
    assert np.all(np.abs(so[:, 6] - Gs[cmin]) < 2e-5 * (1 + abs(Gs[cmin])))
    assert np.array_equal(seen[si[:, 3], np.arange(B)], np.full(B, cmin)), si[:, 3]
    assert len(set(si[:, 3].tolist())) > 1
    s.set_scene_clock(None)


# ---- 8. score_rollout across the boundary of two network passes -------------------------------------------------------------------------
@pytest.mark.parametrize('b_star,j_star', [(5, 255), (600, 254)])
def test_score_rollout_keeps_instance_and_state_across_the_pass_boundary(b_star, j_star):
    """B = 1031, n_steps = 255: 263 936 rows, of which the second network pass starts at flat row 262 144 = state 254 of instance 270.
    Every state is the same x*, every context the same c0 but ctx[b*, j*] = c1, behind the boundary.  Instance b* reports its least
    value at step j*, equal to the folded oracle's g(x*; c1); every other instance reports g(x*; c0).  Two CPU evaluations."""
    par, prob, net = cc.context_problem('st', N)
    B, n_steps = 1031, 255
    assert j_star * B + b_star >= (1 << 18) and ctc.rows_of_step_major_log([1 << 18], B, n_steps + 1)[0][0] == 270
    xs = sample_instances(prob, 1, seed=6, vel_scale=0.3)
    G = _g_table(par, net, xs)[:, 0]
    c1, c0 = int(np.argmin(G)), int(np.argmax(G))
    tol = 2e-5 * (1 + np.abs(G).max())
    print('oracle g(x*; c)', G.tolist(), 'c0', c0, 'c1', c1)
    assert G[c0] - G[c1] > 100 * tol
    ctx = np.ascontiguousarray(np.broadcast_to(cc.CONTEXTS[c0], (B, n_steps + 1, cc.N_CTX)))
    ctx[b_star, j_star] = cc.CONTEXTS[c1]
    x_log = np.ascontiguousarray(np.broadcast_to(xs[0], (n_steps + 1, B, 12)))
    u_log = np.zeros((n_steps, B, 6))
    s = cc.engine('st', N)
    s.set_instance_context_track(ctx)
    so, si = s.score_rollout(x_log, u_log, want_safe=True)
    others = np.arange(B) != b_star
    assert abs(so[b_star, 6] - G[c1]) < tol and si[b_star, 3] == j_star
    assert np.all(np.abs(so[others, 6] - G[c0]) < tol)


# ---- 9. guards ------------------------------------------------------------------------------------------------------------------------
def test_misuse_is_refused_by_name():
    from safe_mpc_amd import _lib
    from safe_mpc_amd import controller as C
    from safe_mpc_amd._lib import EngineError
    par, prob, net = cc.context_problem('st', N)
    L = _lib.lib()
    B = 6
    x0, xg, ug, p = _inputs('st', B)
    ctx, _ = ctc.track_contexts(B)
    s = cc.engine('st', N)
    s.set_instance_context_track(ctx)
    # another batch size: refused, both sizes named -- by every entry point that runs the network
    small = (x0[:4], xg[:4], ug[:4], p[:4])
    runs = (lambda: s.solve(*small), lambda: s.eval_nodes(*small[1:]), lambda: s.merit_terms(*small),
            lambda: s.check_guess(xg[:4], ug[:4], safe_node=N), lambda: s.check_trajectory(xg[:4], want_nn=True),
            lambda: s.score_rollout(np.zeros((3, 4, 12)), np.zeros((2, 4, 6)), want_safe=True), lambda: s.sqp(*small))
    for call in runs:
        with pytest.raises(EngineError, match=r'engine error -1: .*batch size 4, .*context was set for 6 instances'):
            call()
    with pytest.raises(EngineError, match=r'engine error -4: smpc_rollout_batch: an instance context'):
        s.rollout(x0, xg, ug, p, 2)
    # a non-finite number (host pointers): refused with instance, column and number, and the old table stays
    before = s.eval_nodes(xg, ug, p)['nn_val'].copy()
    bad = ctx.copy()
    bad[4, 1, 2] = np.inf
    with pytest.raises(EngineError, match=r'engine error -1: context track of instance 4 \(of B=6\), column 1 \(of T=3\), number 2'):
        s.set_instance_context_track(bad)
    assert np.array_equal(s.eval_nodes(xg, ug, p)['nn_val'], before)
    # T = 0, and shapes
    with pytest.raises(EngineError, match=r'engine error -1: smpc_set_instance_context_track: T=0'):
        s._chk(L.smpc_set_instance_context_track(s.h, B, 0, ctx.ctypes.data, 0))
    with pytest.raises(EngineError, match=r'engine error -1: bad batch size'):
        s._chk(L.smpc_set_instance_context_track(s.h, 0, T, ctx.ctypes.data, 0))
    with pytest.raises(ValueError, match='at least one time column'):
        s.set_instance_context_track(ctx[:, :0])
    with pytest.raises(ValueError, match='expected'):
        s.set_instance_context_track(ctx[:, 0])
    with pytest.raises(ValueError, match='expected'):
        s.set_instance_context_track(ctx[:, :, :3])
    assert np.array_equal(s.eval_nodes(xg, ug, p)['nn_val'], before)
    # growth while the stream is being captured: refused, the capture ends cleanly, the old table stays
    big = torch.zeros((B, 64 * T, cc.N_CTX), dtype=torch.float64, device='cuda:0')
    with pytest.raises(EngineError, match='engine error -4: .* while the stream is being captured'), warnings.catch_warnings():
        warnings.filterwarnings('ignore', 'The CUDA Graph is empty')
        with torch.cuda.graph(torch.cuda.CUDAGraph()):
            s.set_instance_context_track(big)
    torch.cuda.synchronize()
    assert np.array_equal(s.eval_nodes(xg, ug, p)['nn_val'], before)
    # after a clear -- through either setter -- a call of another size runs
    s.set_instance_context(None)
    for call in runs:
        call()
    s.set_instance_context_track(ctx)
    s.set_instance_context_track(None)
    s.eval_nodes(*small[1:])
    # smpc_set_mlp_context drops the slot, and so does smpc_set_mlp
    s.set_instance_context_track(ctx)
    Wc = np.ascontiguousarray(net.weights[0][:, 12:])
    m, sd_, d = np.zeros(4), np.ones(4), np.zeros(4)
    s._chk(L.smpc_set_mlp_context(s.h, 4, Wc.ctypes.data, m.ctypes.data, sd_.ctypes.data, d.ctypes.data, 0))
    s.eval_nodes(*small[1:])
    s.set_instance_context_track(ctx)
    s.set_mlp(net.folded(cc.DEFAULT))
    with pytest.raises(EngineError, match=r'engine error -1: .*no context columns'):
        s._chk(L.smpc_set_instance_context_track(s.h, B, T, ctx.ctypes.data, 0))
    s.eval_nodes(*small[1:])
    # the parallel policy: its candidate slots are not instances; with the default context alone it runs
    parp, probp, _ = make_problem('parallel', N=4)
    parp.net_size = [12 + cc.N_CTX, 256, 1]
    ctrl = C.get_controller('parallel', parp, 3, N=4, device_state=True)
    assert ctrl.net.n_ctx == cc.N_CTX
    xp = torch.tensor(sample_instances(probp, 3, seed=2), dtype=torch.float64, device='cuda:0')
    ctrl.setGuess(xp[:, None, :].repeat(1, 5, 1), torch.zeros((3, 4, 6), dtype=torch.float64, device='cuda:0'))
    ctrl.ocp_solver.set_instance_context_track(ctc.track_contexts(3)[0])
    with pytest.raises(EngineError, match=r'engine error -4: smpc_policy_step: an instance context .*parallel'):
        ctrl.step_on_device(xp)
    ctrl.ocp_solver.set_instance_context(None)
    ctrl.step_on_device(xp)
    ctrl.ocp_solver.sync()


# ---- 10. the closed loop ------------------------------------------------------------------------------------------------------------
def test_closed_loop_on_moving_scenes_with_a_context_network(tmp_path, monkeypatch):
    """a checkpoint with ctx_select written from a synthetic context net (no fit); run_mpc(on_device=True, scenes=moving_scenes(..))
    against on_device=False on the same engine: 'htwa', one group, 3 steps, N = 6, T = N + 2 so that later steps clamp.  Compared as
    test_scene_track_gpu.py compares its two paths (x 1e-4, u 2e-3 (1 + |u|_inf), NaN patterns and outcome lists equal).  Every
    controller handle gets the context of every (instance, column) of its track, and both handles are left without track, context
    and clock."""
    import ray_cases as rc
    import scene_cases as sc
    from oracle.oracle import Oracle
    from safe_mpc_amd import closed_loop as cl
    from safe_mpc_amd import controller as C
    from safe_mpc_amd import safe_set_data as sd
    from safe_mpc_amd.problem import moving_scenes, scene_context
    from safe_mpc_amd.safe_set import SafeSetNet
    from safe_mpc_amd.solver import BatchedOcpSolver
    Nn, steps, B = 6, 3, 4
    Tn = Nn + 2
    par = rc.ray_params()
    hprob = C.OcpProblem(par, 'htwa', 'ext', N=Nn)
    r = [i for i, name in enumerate(hprob.row_obstacle) if name in sc.Z1_OBSTACLES][0]
    select = [(r, 1), (r, 4)]                                  # the y of the first gate capsule's two end points
    track = moving_scenes(hprob, B, Tn, 4.0)
    ctxs = scene_context(track, select)                        # [B, Tn, 2]
    base = scene_context(hprob.row_geometry()[None], select)[0]
    spread = np.abs(ctxs - base).max()
    assert ctxs.shape == (B, Tn, 2) and spread > 1e-2 and np.abs(ctxs[:, 1] - ctxs[:, 0]).min() > 0
    syn = SafeSetNet.synthetic([2 * rc.NQ + 2, 256, 1], rc.NQ, hprob.x_min, hprob.x_max, 0, par.act)
    path = str(tmp_path / 'safe_set_ctx.pt')
    sd.save_checkpoint(path, syn.model, syn.mean, syn.std, base, np.full(2, spread / 2), select)     # (normalised contexts of order 1)
    par.net_path, par.use_net, par.N, par.back_hor, par.net_size = path, True, Nn, 8, [2 * rc.NQ, 256, 1]
    cnet = SafeSetNet.from_params(par)
    assert cnet.n_ctx == 2 and cnet.ctx_select == select
    assert np.abs(cnet.folded(ctxs[0, 0]).biases[0] - cnet.folded(ctxs[0, Tn - 1]).biases[0]).max() > 1e-3     # the columns' nets are told apart
    pool = sample_instances(hprob, 24, seed=4, vel_scale=0.1)
    free = Oracle(hprob).check_trajectory(pool[:, None, :], hprob.x_min, hprob.x_max, 0.0, hprob.row_lb, hprob.row_ub).astype(bool)
    x0 = pool[free][:B]
    assert len(x0) == B
    xg, ug = np.repeat(x0[:, None, :], Nn + 1, axis=1), np.zeros((B, Nn, 6))
    seen = []
    real = BatchedOcpSolver.set_instance_context_track

    def spy(self, ctx=None):
        seen.append(None if ctx is None else ctx.cpu().numpy() if hasattr(ctx, 'cpu') else np.array(ctx))
        return real(self, ctx)
    monkeypatch.setattr(BatchedOcpSolver, 'set_instance_context_track', spy)
    runs = []
    for on_device in (False, True):
        made = []

        def mk(name, batch, on_device=on_device, made=made):
            c = C.get_controller(name, par, batch, device=0, device_state=on_device)
            c.ocp_solver.set_qp_mode('throughput')
            made.append(c)
            return c

        def mkb(batch, on_device=on_device, made=made):
            c = C.SafeBackupController(par, batch, device=0, device_state=on_device)
            c.ocp_solver.set_qp_mode('throughput')
            made.append(c)
            return c
        del seen[:]
        runs.append(cl.run_mpc(par, 'htwa', xg, ug, n_steps=steps, on_device=on_device, groups=1, make_controller=mk, make_backup=mkb,
                               scenes=track))
        assert len(seen) >= 1 and seen[0].shape == (B, Tn, 2) and np.array_equal(seen[0], ctxs)
        # both handles are left without track, context and clock: calls of another batch size run
        assert len(made) == 2
        for c in made:
            sv = c.ocp_solver
            assert getattr(sv, '_scene_clock', None) is None
            xs3 = np.repeat(x0[:3, None, :], sv.N + 1, axis=1)
            res = sv.check_trajectory(xs3, want_nn=True) if sv.net is not None else sv.check_trajectory(xs3)
            assert np.asarray(res[0] if isinstance(res, tuple) else res).shape == (3,)
    host, dev = runs
    tol_x, tol_u = 1e-4, 2e-3 * (1 + np.nanmax(np.abs(host['u'])))
    print('closed loop: x error', np.nanmax(np.abs(dev['x'] - host['x'])), 'u error', np.nanmax(np.abs(dev['u'] - host['u'])), 'tolerances',
          tol_x, tol_u)
    assert np.array_equal(np.isnan(dev['x']), np.isnan(host['x'])) and np.array_equal(np.isnan(dev['u']), np.isnan(host['u']))
    assert np.nanmax(np.abs(dev['x'] - host['x'])) < tol_x and np.nanmax(np.abs(dev['u'] - host['u'])) < tol_u
    for key in ('conv_idx', 'collisions_idx', 'viable_idx', 'unconv_idx'):
        assert sorted(dev[key]) == sorted(host[key]), key
    assert np.nanmax(np.abs(host['u'])) > 0
