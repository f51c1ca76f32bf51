"""The per-instance inputs of a handle as ONE protocol: scene, scene track, curves, context, and the
per-instance bounds beside them.  -m gpu only.

Z1 (six collision rows) with a seeded context network (context_cases.py) at N = 4; batch sizes 3 and 5, odd so that k_qp_ipm's last
wavefront is half filled.  What is pinned: which entry point guards which slot, what a slot holds after growth, an overwrite in place
and a refused set, what a new horizon drops, and that the workers of smpc_rollout_batch read their parent's network."""
import numpy as np
import pytest
import torch

import context_cases as cc
import scene_cases as sc
import track_cases as tc
from conftest import constant_guess, make_problem, sample_instances

pytestmark = pytest.mark.gpu
N = 4
B_SET, B_CALL = 5, 3
L_CURVE = 7
SLOTS = ['scene', 'track', 'curves', 'context']

ENTRY = {'solve': 'smpc_solve_batch', 'eval_nodes': 'smpc_eval_nodes', 'check_trajectory': 'smpc_check_trajectory',
         'merit_terms': 'smpc_merit_terms', 'sqp': 'smpc_sqp_batch', 'check_guess': 'smpc_check_guess', 'score_rollout': 'smpc_score_rollout',
         'policy_step': 'smpc_policy_step', 'loop_post': 'smpc_loop_post', 'ik': 'smpc_ik_batch'}
ROWS_AND_NETWORK = ['solve', 'eval_nodes', 'check_trajectory', 'merit_terms', 'sqp', 'check_guess', 'score_rollout', 'policy_step']
# who guards what: the guard call sites of engine.hip, by slot (a track is the scene's slot)
GUARDED_BY = {'scene': ROWS_AND_NETWORK + ['loop_post', 'ik'], 'track': ROWS_AND_NETWORK + ['loop_post', 'ik'],
              'curves': ['policy_step', 'score_rollout'], 'context': ROWS_AND_NETWORK}
SETTER = {'scene': 'smpc_set_instance_scene', 'track': 'smpc_set_instance_scene', 'curves': 'smpc_set_instance_curves',
          'context': 'smpc_set_instance_context'}


def _inputs(B=B_SET):
    par, prob, net = cc.context_problem('st', N)
    x0 = sample_instances(prob, B, seed=3, vel_scale=0.3)
    xg, ug, p = constant_guess(prob, x0)
    xg[:, 1:] += 0.05 * np.random.default_rng(3).standard_normal(xg[:, 1:].shape)
    return x0, xg, ug, p


def _geom():
    return sc.scene_family('z1', 'st', N, 4)[2]          # [4, n_rows, 8]: four distinct scenes of the same rows


def _curves(B, turn=0):
    """[B, 3, L_CURVE]: a short line per instance around the problem's reference point, every instance and every ``turn`` another"""
    par, prob, net = cc.context_problem('st', N)
    b, j = np.arange(B)[:, None, None], np.arange(L_CURVE)[None, None, :]
    return np.ascontiguousarray(prob.ee_ref[None, :, None] + 0.01 * (b + 3 * turn + 1) * np.array([1.0, -1.0, 0.5])[None, :, None] + 0.002 * j)


def _data(slot, B, turn=0):
    """what instance b of a batch of B is given, ``turn`` = another assignment"""
    if slot == 'scene':
        return np.ascontiguousarray(_geom()[(np.arange(B) + turn) % 4])
    if slot == 'track':
        return np.ascontiguousarray(_geom()[(tc.track_indices(B, 2) + turn) % 4])
    if slot == 'curves':
        return _curves(B, turn)
    return np.ascontiguousarray(cc.CONTEXTS[(np.arange(B) + turn) % 3])


def _set(s, slot, data):
    {'scene': s.set_instance_scene, 'track': s.set_instance_scene_track, 'curves': s.set_instance_curves,
     'context': s.set_instance_context}[slot](data)


BAD_ENTRY = {'scene': (1, 2, 4), 'track': (1, 1, 2, 4), 'curves': (1, 1, 2), 'context': (1, 2)}     # (capsule rows read entries 0..5)


# ---- 1. who guards what ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def rig():
    """a controller, a backup controller and a device loop group for B_CALL instances whose handle has collision rows and a context
    network; the numpy inputs of the other entry points"""
    from safe_mpc_amd import closed_loop as cl
    from safe_mpc_amd import controller as C
    par, _, _ = make_problem('st', N=N)
    par.net_size = [12 + cc.N_CTX, 256, 1]
    par.back_hor = 8
    ctrl, backup = C.get_controller('st', par, B_CALL, device_state=True), C.SafeBackupController(par, B_CALL, device_state=True)
    sv = ctrl.ocp_solver
    assert ctrl.net.n_ctx == cc.N_CTX and len(sv.problem.rows) > 0
    x0, xg, ug, p = (a[:B_CALL] for a in _inputs())
    with torch.cuda.stream(torch.cuda.ExternalStream(sv.L.smpc_stream(sv.h), device=torch.device('cuda', sv.device))):
        grp = cl._DeviceGroup(par, xg, ug, 0.0, 0.0, ctrl, backup, 4, 0, False, use_graphs=False)
    nq = sv.nq
    x_log, u_log = np.ascontiguousarray(np.transpose(xg[:, :3], (1, 0, 2))), np.zeros((2, B_CALL, nq))
    tgt, qs = np.zeros((B_CALL, 3)) + 0.3, np.zeros((B_CALL, 2, nq))
    calls = {'solve': lambda: sv.solve(x0, xg, ug, p), 'eval_nodes': lambda: sv.eval_nodes(xg, ug, p),
             'check_trajectory': lambda: sv.check_trajectory(xg, want_nn=True), 'merit_terms': lambda: sv.merit_terms(x0, xg, ug, p),
             'sqp': lambda: sv.sqp(x0, xg, ug, p, dict(max_iter=1)), 'check_guess': lambda: sv.check_guess(xg, ug, safe_node=N),
             'score_rollout': lambda: sv.score_rollout(x_log, u_log, want_safe=True), 'policy_step': grp.part_a, 'loop_post': grp.part_b,
             'ik': lambda: sv.ik(tgt, qs),
             'score_rollout_instance': lambda: sv.score_rollout(x_log, u_log, traj='instance')}
    return sv, calls


@pytest.mark.parametrize('slot', SLOTS)
def test_guard_matrix(rig, slot):
    """The slot set for 5 instances, every entry point that reads it called with 3: refused with its own name, both sizes and the
    setter, before anything is launched; once the slot is cleared the same call runs.  score_rollout(traj='instance') has nothing to
    score against once the curves are cleared (that refusal is then the one of a handle without curves): it runs with curves of its
    own size."""
    from safe_mpc_amd._lib import EngineError
    sv, calls = rig
    _set(sv, slot, _data(slot, B_SET))
    names = GUARDED_BY[slot]
    for name in names:
        call = calls['score_rollout_instance' if slot == 'curves' and name == 'score_rollout' else name]
        with pytest.raises(EngineError, match=rf'engine error -1: {ENTRY[name]}: batch size {B_CALL}, .* set for {B_SET} instances '
                                              rf'\({SETTER[slot]}'):
            call()
    _set(sv, slot, None)
    for name in names:
        if slot == 'curves' and name == 'score_rollout':
            with pytest.raises(EngineError, match='neither ee_ref nor traj'):
                calls['score_rollout_instance']()
            sv.set_instance_curves(_data('curves', B_CALL))
            calls['score_rollout_instance']()
            sv.set_instance_curves(None)
        else:
            calls[name]()
    sv.sync()


# ---- 2. what a slot holds -------------------------------------------------------------------------------------------------------------
def _bits(s, slot, x0, xg, ug, p):
    """the reading entry points of the slot, as a flat list of arrays"""
    if slot == 'curves':
        x_log, u_log = np.ascontiguousarray(np.transpose(xg[:, :3], (1, 0, 2))), np.zeros((2, len(x0), s.nq))
        return [np.array(a) for a in s.score_rollout(x_log, u_log, traj='instance')]
    ev = s.eval_nodes(xg, ug, p)
    return [np.array(ev[f]) for f in ev.dtype.names] + [np.array(a) for a in s.solve(x0, xg, ug, p)]


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(u, v, equal_nan=True) for u, v in zip(a, b))


@pytest.mark.parametrize('slot', SLOTS)
def test_slot_lifecycle(slot):
    from safe_mpc_amd._lib import EngineError
    par, prob, net = cc.context_problem('st', N)
    x0, xg, ug, p = (a[:B_CALL] for a in _inputs())
    last = _data(slot, B_CALL, turn=1)
    fresh = cc.engine('st', N)
    _set(fresh, slot, last)
    want = _bits(fresh, slot, x0, xg, ug, p)
    # set for 3, for 5 (the buffer grows), for 3 again (overwritten in place): what counts is the last set
    s = cc.engine('st', N)
    _set(s, slot, _data(slot, B_CALL))
    first = _bits(s, slot, x0, xg, ug, p)
    assert not _same(first, want)                 # (the two assignments are told apart by what is read)
    _set(s, slot, _data(slot, B_SET))
    _set(s, slot, last)
    assert _same(_bits(s, slot, x0, xg, ug, p), want)
    # a set that fails validation leaves the content in force
    bad = _data(slot, B_CALL)
    bad[BAD_ENTRY[slot]] = np.nan
    with pytest.raises(EngineError, match='engine error -1: .*is not finite'):
        _set(s, slot, bad)
    assert _same(_bits(s, slot, x0, xg, ug, p), want)
    # a new horizon drops the per-instance bounds and nothing else
    lo, hi = np.tile(prob.lbx, (B_CALL, N + 1, 1)), np.tile(prob.ubx, (B_CALL, N + 1, 1))
    lo[:, 1:, prob.nq:] *= 0.02
    hi[:, 1:, prob.nq:] *= 0.02
    plain = [np.array(a) for a in s.solve(x0, xg, ug, p)]
    assert _same(plain, [np.array(a) for a in fresh.solve(x0, xg, ug, p)])
    s.set_instance_bounds(lo, hi)
    tight = [np.array(a) for a in s.solve(x0, xg, ug, p)]
    assert not np.array_equal(tight[1], plain[1])
    s.set_horizon(N)
    assert _same([np.array(a) for a in s.solve(x0, xg, ug, p)], plain)
    assert _same(_bits(s, slot, x0, xg, ug, p), want)


# ---- 3. the workers of smpc_rollout_batch read their parent's network -------------------------------------------------------------------
def test_workers_read_the_parents_network(monkeypatch):
    """Two workers exist; then the activation and the context columns with their default row change through the C entry points,
    which leave the workers alive (the Python set_mlp goes through smpc_set_mlp, which destroys them).  The next rollout over two
    sub-batches must give the bits of one sub-batch and of a fresh handle configured the same way."""
    from safe_mpc_amd.safe_set import SafeSetNet
    par, prob, net = cc.context_problem('st', N)
    x0, xg, ug, p = _inputs()
    n_steps = 3
    other = cc.context_net(prob, par, seed=1)
    Wc = np.ascontiguousarray(other.weights[0][:, 12:], np.float32)
    mean, std, default = np.zeros(cc.N_CTX), np.ones(cc.N_CTX), np.ascontiguousarray(cc.CONTEXTS[0])
    act = SafeSetNet.ACT_CODES['tanh' if par.act != 'tanh' else 'relu']

    def reconfigure(s):
        s._chk(s.L.smpc_set_mlp_activation(s.h, act))
        s._chk(s.L.smpc_set_mlp_context(s.h, cc.N_CTX, Wc.ctypes.data, mean.ctypes.data, std.ctypes.data, default.ctypes.data, 0))

    def roll(s):
        return [np.array(a) for a in s.rollout(x0, xg, ug, p, n_steps)[:4]]

    s = cc.engine('st', N, qp_mode='throughput')      # (pinned: the form of the solve must not follow the sub-batch size)
    monkeypatch.setenv('SMPC_ROLLOUT_STREAMS', '2')
    before = roll(s)
    reconfigure(s)
    two = roll(s)
    assert not np.array_equal(two[1], before[1])      # (the new settings are told apart by the trajectories)
    monkeypatch.setenv('SMPC_ROLLOUT_STREAMS', '1')
    one = roll(s)
    fresh = cc.engine('st', N, qp_mode='throughput')
    reconfigure(fresh)
    assert _same(two, one)
    assert _same(two, roll(fresh))
