"""Shared pieces of the safe-set-context tests (test_safe_set_context_host.py, test_safe_set_context_gpu.py): a seeded network with
context inputs, a family of three distinct contexts assigned b % 3 so that neighbours differ, and the CPU doubles -- one OracleSolver
per context on ``net.folded(c)``, a plain network, composed in instance order as scene_cases.by_scene does.  The oracle itself has no
notion of a context.  Not a test module."""
import functools

import numpy as np

from conftest import make_problem
from fake_solver import OracleSolver
from scene_cases import by_scene

N_CTX = 4
# three contexts, raw numbers (the synthetic net normalises with mean 0, std 1); DEFAULT is none of them
CONTEXTS = np.array([[1.5, -1.0, 0.5, 2.0], [-2.0, 1.25, 0.0, -2.5], [0.5, 2.5, -1.5, 1.0]])
DEFAULT = np.array([0.25, -0.5, 1.0, 0.0])


def context_net(prob, par, n_ctx=N_CTX, seed=0, hidden=256):
    from safe_mpc_amd.safe_set import SafeSetNet
    return SafeSetNet.synthetic([2 * prob.nq + n_ctx, hidden, 1], prob.nq, prob.x_min, prob.x_max, seed, par.act)


@functools.lru_cache(maxsize=None)
def context_problem(controller, N=4, n_ctx=N_CTX):
    """(par, prob, net): Z1 with a seeded net of ``n_ctx`` context inputs (the state normalisation is the plain net's)"""
    par, prob, _ = make_problem(controller, 'ext', N=N)
    net = context_net(prob, par, n_ctx)
    prob.set_normalisation(net.mean, net.std)
    return par, prob, net


def instance_contexts(B):
    """(ctx [B, N_CTX], idx [B]): instance b has context b % 3"""
    idx = np.arange(B) % len(CONTEXTS)
    return np.ascontiguousarray(CONTEXTS[idx]), idx


@functools.lru_cache(maxsize=None)
def folded_solvers(controller, N=4):
    """the OracleSolver of every context of the family on the folded net, and the default context's last"""
    par, prob, net = context_problem(controller, N)
    return [OracleSolver(prob, net.folded(c)) for c in list(CONTEXTS) + [DEFAULT]]


def oracle_by_context(controller, name, idx, batched, N=4, **kw):
    """``name`` of the per-context oracle doubles on the members' rows of ``batched``, put back in instance order"""
    subs = folded_solvers(controller, N)
    return by_scene(lambda c, m: getattr(subs[c], name)(*[np.ascontiguousarray(a[m]) for a in batched], **kw), idx, len(idx))


def engine(controller, N=4, default=DEFAULT, qp_mode=None):
    from safe_mpc_amd.solver import BatchedOcpSolver
    par, prob, net = context_problem(controller, N)
    s = BatchedOcpSolver(prob, None)
    s.set_mlp(net, ctx_default=default)
    if qp_mode:
        s.set_qp_mode(qp_mode)
    return s
