"""Shared pieces of the context-track tests (test_context_track_host.py, test_context_track_gpu.py): the case family -- Z1 through
context_cases.context_problem, N = 4, T = 3, the context of (instance b, column c) being CONTEXTS[(b + c) % 3], so that neighbours
differ along both axes --, the numpy statement of "row -> (instance, node-time index) -> column" for the three row layouts of the
network pass, and the CPU doubles: one OracleSolver per context on ``net.folded(c)`` (context_cases.folded_solvers), recomposed NODE
BY NODE as track_cases.per_node does for scenes.  The oracle has no notion of a context, let alone of a track.  Not a test module.

The clocks: none, then cells holding -3, -2, 0 and 7.  With T = 3 and N = 4 the terminal node falls on the clamped last column at
t = 0 and t = 7, on unclamped column 1 at t = -3 and on column 2, the last, at t = -2, where an off-by-one downwards still shows;
t = -7 puts it on the clamped first column."""
import numpy as np

import context_cases as cc
import track_cases as tc

N, T = 4, 3
CLOCKS = [None, -3, -2, 0, 7]


def track_indices(B, T=T):
    """idx [B, T]: the context of (instance b, column c) is CONTEXTS[(b + c) % 3]"""
    return (np.arange(B)[:, None] + np.arange(T)[None, :]) % len(cc.CONTEXTS)


def track_contexts(B, T=T):
    """(ctx [B, T, N_CTX] raw numbers, idx [B, T])"""
    idx = track_indices(B, T)
    return np.ascontiguousarray(cc.CONTEXTS[idx]), idx


# ---- row -> (instance, node-time index) -> column: the statement --------------------------------------------------------------------
def rows_of_node_arrays(nodes, per, t, T):
    """instance-major node arrays with ``per`` nodes per instance ([B][N+1]: per = N + 1; smpc_check_trajectory: per = n_nodes):
    the row of flat node ``nodes`` belongs to instance b = node // per, is node k = node - b per of it, and reads column
    col(t + k), t = the clock (0 without one).  Returns (b, k, column)."""
    nodes = np.asarray(nodes, np.int64)
    b = nodes // per
    k = nodes - b * per
    return b, k, tc.col((0 if t is None else int(t)) + k, T)


def rows_of_node_list(idx_list, per, t, T):
    """the compacted list of live nodes (mode 3): row m is node idx_list[m], never m -- the list's order is whatever the atomics
    gave"""
    return rows_of_node_arrays(np.asarray(idx_list), per, t, T)


def rows_of_step_major_log(flat, B, T):
    """the step-major log of smpc_score_rollout: flat row ``flat`` is state j = flat // B of instance b = flat % B and reads column
    col(j); the clock is not read.  Returns (b, j, column)."""
    flat = np.asarray(flat, np.int64)
    b, j = flat % B, flat // B
    return b, j, tc.col(j, T)


def node_contexts(idx, t, n_nodes):
    """[B, n_nodes]: which context of the family node k of instance b sees at clock t, by the statement above"""
    B, Tn = idx.shape
    b, k, c = rows_of_node_arrays(np.arange(B * n_nodes), n_nodes, t, Tn)
    return idx[b, c].reshape(B, n_nodes)


def log_contexts(idx, n_states):
    """[n_states, B]: which context state j of instance b sees in a step-major log"""
    B, Tn = idx.shape
    b, j, c = rows_of_step_major_log(np.arange(n_states * B), B, Tn)
    return idx[b, c].reshape(n_states, B)


# ---- the CPU doubles ---------------------------------------------------------------------------------------------------------------
def eval_nodes_by_column(controller, seen, xg, ug, p, N=N):
    """eval_nodes of the folded oracles recomposed node by node: one oracle call per distinct context of ``seen [B, N + 1]``, taking
    the nodes that see it"""
    subs = cc.folded_solvers(controller, N)
    return tc.per_node(lambda c: subs[c].eval_nodes(xg, ug, p), seen)


def cell(value):
    """a scene clock cell on the device holding ``value``"""
    import torch
    return torch.full((1,), int(value), dtype=torch.int64, device='cuda:0')


def set_clock(solver, t):
    """the clock of the case family onto the solver: None = no cell; returns the cell (keep it alive).  The cell is written and
    FINISHED before the next host-pointer call (the engine has a stream of its own)."""
    import torch
    c = None if t is None else cell(t)
    torch.cuda.synchronize()
    solver.set_scene_clock(c)
    return c
