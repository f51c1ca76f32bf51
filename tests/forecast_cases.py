"""Shared pieces of the obstacle-forecast tests (test_forecast_host.py, test_forecast_gpu.py): small WORLD
tracks on the Z1-class problem (6 rows) and the fr7 problem (4 rows, sphere + plane, so the ``offset`` slot moves), the clock family,
and the read-back of the engine's scene and context slots.  Not a test module.

The principle every GPU test rests on: ``problem.forecast_statement`` is the definition, the kernel repeats it bit for bit, and a
forecast in the scene slot is read from time 0 -- so 'true' at clock c is the clocked track at clock c, and 'hold' the standing scene
of column col(c)."""
import ctypes
import functools

import numpy as np

from conftest import make_problem, make_problem_fr7

MODES = ('hold', 'cv', 'true')


def clocks(T):
    """the clock family: none, the track's ends and beyond, and the ends of int64 (the kernels hold the cell to +-2^62)"""
    return [None, 0, 1, T - 2, T - 1, T + 5, -1, 2 ** 63 - 1, -2 ** 63]


@functools.lru_cache(maxsize=None)
def problem(system, N, controller='htwa'):
    """(par, prob, net) of the Z1-class problem as the scene tests build it, or of fr7"""
    return make_problem(controller, N=N) if system == 'z1' else make_problem_fr7(N=N)


def world(prob, B, T, seed=0, amp=0.02):
    """[B, T, n_rows, 8]: the problem's own geometry moved by a smooth, generic function of (instance, column, row, slot) in ALL
    eight slots -- what no row kind reads is forecast as well.  Adjacent columns and adjacent instances differ in every slot (checked
    here), and the numbers have full mantissas, so that the order of the additions shows in the last bit."""
    b, j, r, s = np.meshgrid(np.arange(B), np.arange(T), np.arange(len(prob.rows)), np.arange(8), indexing='ij')
    W = prob.row_geometry()[None, None] + amp * np.sin(1.7 * b + 0.9 * j + 0.37 * r + 0.11 * s + 0.5 + seed) + 0.003 * j * (1 + 0.1 * s) / 0.7
    assert T < 2 or (W[:, 1:] != W[:, :-1]).all()
    assert B < 2 or (W[1:] != W[:-1]).all()
    return np.ascontiguousarray(W)


def gather_true(W, t, N):
    """F[b][k] = W[b][col(t + k)], restated with numpy's clip (t: a Python int, held to +-2^62 like the clock)"""
    t = 0 if t is None else min(max(int(t), -2 ** 62), 2 ** 62)
    cols = [min(max(t + k, 0), W.shape[1] - 1) for k in range(N + 1)]
    return W[:, cols]


def cell(value=0):
    """a scene clock cell on the device; any int64 bit pattern"""
    import torch
    return torch.tensor([int(value)], dtype=torch.int64, device='cuda:0')


def set_clock(solver, c):
    """clock none, or a new cell holding c -- written and FINISHED before the next call (the engine has a stream of its own).
    Returns the cell: keep it alive while it is set."""
    import torch
    if c is None:
        solver.set_scene_clock(None)
        return None
    k = cell(c)
    torch.cuda.synchronize()
    solver.set_scene_clock(k)
    return k


def read_slots(solver):
    """(info, scene, ctx) through the engine's test hook smpc_debug_scene_slots: info = dict(scene_B, scene_T, scene_fc, ctx_B, ctx_T,
    ctx_fc); scene [B, T, n_rows, 8] float64 and ctx [B, T, n_ctx] float32 as the slots hold them (None where a slot is empty)"""
    L = solver.L
    L.smpc_debug_scene_slots.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    info = np.zeros(6, np.int64)
    rc = L.smpc_debug_scene_slots(solver.h, None, 0, None, 0, info.ctypes.data)
    assert rc == 0, L.smpc_last_error(solver.h)
    nr, nc = len(solver.problem.rows), int(getattr(solver.net, 'n_ctx', 0) or 0) if getattr(solver, 'net', None) is not None else 0
    scene = np.zeros((int(info[0]), int(info[1]), nr, 8))
    ctx = np.zeros((int(info[3]), int(info[4]), nc), np.float32)
    rc = L.smpc_debug_scene_slots(solver.h, scene.ctypes.data, scene.size, ctx.ctypes.data, ctx.size, info.ctypes.data)
    assert rc == 0, L.smpc_last_error(solver.h)
    keys = ('scene_B', 'scene_T', 'scene_fc', 'ctx_B', 'ctx_T', 'ctx_fc')
    return dict(zip(keys, (int(v) for v in info))), (scene if scene.size else None), (ctx if ctx.size else None)
