"""Cases shared by test_row_bounds_host.py and test_row_bounds_gpu.py: the two arms the row-bounds tests run on, margins along
the horizon, and perturbed inputs whose collision rows are not all inactive."""
import functools

import numpy as np

from conftest import constant_guess, make_problem, make_problem_fr7, sample_instances

CEILING = 1.4          # metres: the upper bound the 7-DoF arm's floor plane gets in these cases
MARGIN = 0.01          # metres: the collision_margin c of the margin-equivalence tests (rows inflate by 2 c)


@functools.lru_cache(maxsize=None)
def problem(system, N, margin=0.0, controller=None):
    """(par, prob, net): the Z1-class arm (nq = 6, six capsule rows) or the 7-DoF arm (sphere, point and plane rows) at horizon N,
    built with ``collision_margin = margin``.  The 7-DoF arm's floor is one-sided as shipped (bounds [0, 1e6]); here it gets a
    ceiling at CEILING metres, so that its plane rows are two-sided.  Unless a controller is named, the Z1's formulation is 'st' (the safe-set
    row soft on the end node) and the 7-DoF arm's 'constraint_everywhere' (hard on every node)."""
    if system == 'z1':
        return make_problem(controller or 'st', N=N, collision_margin=margin)
    from safe_mpc_amd.problem import OcpProblem
    from safe_mpc_amd.safe_set import SafeSetNet
    par, _, _ = make_problem_fr7(controller or 'constraint_everywhere', N=N)
    par.collision_margin = margin
    for obs in par.obstacles:               # (the collision pairs hold the same dicts)
        if obs['type'] == 'plane':
            obs['bounds'] = np.array([float(obs['bounds'][0]), CEILING])
    prob = OcpProblem(par, controller or 'constraint_everywhere', 'ext', N=N)
    net = SafeSetNet.from_params(par, prob.x_min, prob.x_max)
    prob.set_normalisation(net.mean, net.std)
    return par, prob, net


def inputs(prob, B, seed=3):
    """x0, xg, ug, p of B instances: collision-free starts, a perturbed guess (the nodes differ, the defects are not zero) and a
    start state a little off the guess's node 0 (dx_0 is not zero)"""
    x0 = sample_instances(prob, B, seed=seed, vel_scale=0.3)
    xg, ug, p = constant_guess(prob, x0)
    rng = np.random.default_rng(seed)
    ug += rng.uniform(-3, 3, ug.shape)
    xg[:, 1:] += 0.01 * rng.standard_normal(xg[:, 1:].shape)
    x0 = x0 + 0.003 * rng.standard_normal(x0.shape)
    return x0, xg, ug, p


def descriptor_table(prob, B):
    """the table that says what the descriptor says: every entry the row's own row_lb / row_ub"""
    nr = len(prob.rows)
    lo = np.ascontiguousarray(np.broadcast_to(prob.row_lb, (B, prob.N + 1, nr)))
    hi = np.ascontiguousarray(np.broadcast_to(prob.row_ub, (B, prob.N + 1, nr)))
    return lo, hi


def growing_margin(N, a=0.004, b=0.003):
    """d_k = a + b k metres"""
    return a + b * np.arange(N + 1)
