"""A safe-set context that follows a scene track: the host side -- scene_context on a track, closed_loop's
_set_scene on recording stubs, the exported symbol, and the numpy statement of "row -> (instance, node-time index) -> column" that
the GPU tests pick their folded oracles by.  No GPU."""
import numpy as np
import pytest

import context_cases as cc
import context_track_cases as ctc
import track_cases as tc
from conftest import make_problem


def test_scene_context_of_a_track_is_the_stack_of_its_columns():
    from safe_mpc_amd.problem import jittered_scenes, scene_context
    par, prob, _ = make_problem('st', N=4)
    B, T = 5, 3
    cols = [jittered_scenes(prob, B, 0.05, seed=s) for s in range(T)]
    track = np.ascontiguousarray(np.stack(cols, axis=1))              # [B, T, n_rows, 8]
    sel = [(0, 1), (2, 6), (1, 3)]
    c = scene_context(track, sel)
    assert c.shape == (B, T, 3) and c.flags['C_CONTIGUOUS']
    assert np.array_equal(c, np.stack([scene_context(g, sel) for g in cols], axis=1))
    assert not np.array_equal(c[:, 0], c[:, 1])
    assert scene_context(track, []).shape == (B, T, 0)
    # a 3-D input behaves as before; anything else still raises
    assert np.array_equal(scene_context(cols[0], sel), np.stack([cols[0][:, 0, 1], cols[0][:, 2, 6], cols[0][:, 1, 3]], axis=1))
    with pytest.raises(ValueError, match='expected'):
        scene_context(cols[0][0], sel)
    with pytest.raises(ValueError, match='expected'):
        scene_context(track[None], sel)
    with pytest.raises(ValueError, match='expected'):
        scene_context(track[..., :7], sel)
    with pytest.raises(ValueError, match='outside'):
        scene_context(track, [(len(prob.rows), 0)])


class _Recorder:
    """a solver stub that records what _set_scene hands over, in order"""

    def __init__(self, net):
        self.net, self.log = net, []

    def set_instance_scene(self, geom=None):
        self.log.append(('scene', None if geom is None else np.array(geom)))

    def set_instance_scene_track(self, geom=None):
        self.log.append(('scene_track', None if geom is None else np.array(geom)))

    def set_instance_context(self, ctx=None):
        self.log.append(('context', None if ctx is None else np.array(ctx)))


class _TrackRecorder(_Recorder):
    def set_instance_context_track(self, ctx=None):
        self.log.append(('context_track', None if ctx is None else np.array(ctx)))


def _select_net():
    from safe_mpc_amd.safe_set import SafeSetNet
    par, prob, plain = make_problem('st', N=4)
    base = cc.context_net(prob, par, n_ctx=2)
    sel = [(0, 0), (1, 2)]
    return prob, SafeSetNet(base.model, base.mean, base.std, base.act, np.zeros(2), np.ones(2), sel), sel


def test_set_scene_brings_the_context_track_beside_the_scene_track():
    from safe_mpc_amd import closed_loop as cl
    from safe_mpc_amd.problem import jittered_scenes, scene_context
    prob, net, sel = _select_net()
    B, T = 3, 3
    cols = [jittered_scenes(prob, B, 0.05, seed=s) for s in range(T)]
    track = np.ascontiguousarray(np.stack(cols, axis=1))
    sv = _TrackRecorder(net)
    cl._set_scene(sv, track)
    assert [k for k, _ in sv.log] == ['context_track', 'scene_track']
    assert sv.log[0][1].shape == (B, T, 2)
    assert np.array_equal(sv.log[0][1], np.stack([scene_context(g, sel) for g in cols], axis=1))
    assert np.array_equal(sv.log[1][1], track)
    # a track of one column is a scene: the 2-D call, as before
    sv = _TrackRecorder(net)
    cl._set_scene(sv, track[:, :1])
    assert [k for k, _ in sv.log] == ['context', 'scene_track']
    assert sv.log[0][1].shape == (B, 2) and np.array_equal(sv.log[0][1], scene_context(cols[0], sel))
    # a scene: as before
    sv = _TrackRecorder(net)
    cl._set_scene(sv, cols[1])
    assert [k for k, _ in sv.log] == ['context', 'scene'] and np.array_equal(sv.log[0][1], scene_context(cols[1], sel))
    # None clears: the context's clear is the track's clear (one slot), so no new call is needed
    sv = _TrackRecorder(net)
    cl._set_scene(sv, None)
    assert sv.log == [('context', None), ('scene', None)]
    sv = _TrackRecorder(net)
    cl._clear_scene(sv)
    assert sv.log == [('scene', None), ('context', None)]


def test_a_solver_that_cannot_take_a_context_track_is_refused_before_anything_is_set():
    from safe_mpc_amd import closed_loop as cl
    from safe_mpc_amd.problem import jittered_scenes
    prob, net, sel = _select_net()
    geom = jittered_scenes(prob, 3, 0.05, seed=1)
    sv = _Recorder(net)
    with pytest.raises(ValueError) as e:
        cl._set_scene(sv, np.repeat(geom[:, None], 2, axis=1))
    assert str(e.value) == ('scenes: a track of T = 2 time columns with a safe-set network that has a context: the context is a '
                            'constant of the instance, one that moves along a track is not supported')
    assert sv.log == []
    cl._set_scene(sv, geom[:, None])                      # one column: still served
    assert [k for k, _ in sv.log] == ['context', 'scene_track']


def test_the_symbol_is_declared_exported_and_prototyped():
    import ctypes
    import os
    import re
    from safe_mpc_amd import _lib
    from safe_mpc_amd.solver import BatchedOcpSolver
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, 'include', 'smpc.h')).read()
    declared = set(re.findall(r'^(?:int|void|const char\*|void\*) (smpc_\w+)\(', hdr, re.M))
    name = 'smpc_set_instance_context_track'
    assert name in declared and name in _lib.SYMBOLS and hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    assert _lib.lib().smpc_set_instance_context_track.argtypes == [ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p,
                                                                   ctypes.c_int]
    assert callable(BatchedOcpSolver.set_instance_context_track)


def test_the_statement_of_rows_instances_and_columns():
    """the three row layouts of the network pass, on the case family (T = 3, N = 4) and its clocks"""
    N, T = ctc.N, ctc.T
    B = 5
    idx = ctc.track_indices(B)
    assert idx.shape == (B, T) and np.all(idx[1:] != idx[:-1]) and np.all(idx[:, 1:] != idx[:, :-1])     # neighbours differ both ways
    # instance-major node arrays: node b (N + 1) + k is node k of instance b
    b, k, c = ctc.rows_of_node_arrays(np.arange(B * (N + 1)), N + 1, -3, T)
    assert np.array_equal(b, np.repeat(np.arange(B), N + 1)) and np.array_equal(k, np.tile(np.arange(N + 1), B))
    assert c.reshape(B, N + 1)[0].tolist() == [0, 0, 0, 0, 1]
    # where the terminal node falls at every clock of the family (and at -7, the clamped first column)
    term = {t: int(ctc.rows_of_node_arrays([N], N + 1, t, T)[2][0]) for t in ctc.CLOCKS + [-7]}
    assert term == {None: 2, -3: 1, -2: 2, 0: 2, 7: 2, -7: 0}
    assert ctc.rows_of_node_arrays([N], N + 1, -2, T)[2][0] != ctc.rows_of_node_arrays([N - 1], N + 1, -2, T)[2][0]
    # a node count that is not N + 1 (smpc_check_trajectory)
    b, k, c = ctc.rows_of_node_arrays(np.arange(9), 3, 1, T)
    assert b.tolist() == [0, 0, 0, 1, 1, 1, 2, 2, 2] and k.tolist() == [0, 1, 2] * 3 and c.tolist() == [1, 2, 2] * 3
    # the mode-3 list in any order: the node is idx[m], never m
    order = np.array([13, 4, 22, 9, 1])
    b, k, c = ctc.rows_of_node_list(order, N + 1, -2, T)
    assert b.tolist() == [2, 0, 4, 1, 0] and k.tolist() == [3, 4, 2, 4, 1] and c.tolist() == [1, 2, 0, 2, 0]
    # the step-major log: flat row j B + b, the clock plays no part; the second pass of a long log starts mid-state
    b, j, c = ctc.rows_of_step_major_log(np.arange(4 * 3), 3, T)
    assert b.tolist() == [0, 1, 2] * 4 and j.tolist() == [0] * 3 + [1] * 3 + [2] * 3 + [3] * 3 and c.tolist() == [0] * 3 + [1] * 3 + [2] * 6
    b, j, c = ctc.rows_of_step_major_log([1 << 18], 1031, 256)
    assert (int(b[0]), int(j[0]), int(c[0])) == (270, 254, 254)
    # the composed tables agree with track_cases' rule for scenes
    for t in ctc.CLOCKS:
        assert np.array_equal(ctc.node_contexts(idx, t, N + 1), tc.node_scenes(idx, 0 if t is None else t, N + 1))
    assert np.array_equal(ctc.log_contexts(idx, 5), idx[:, tc.col(np.arange(5), T)].T)
