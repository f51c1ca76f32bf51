"""The engine's four host-cached parameter blocks (check bounds, guess check bounds, inverse kinematics bounds, score bounds): the
small host arrays of smpc_check_trajectory, smpc_check_guess, smpc_ik_batch and smpc_score_rollout, uploaded only when they change.
-m gpu only.

The shape smoke() uses (make_problem('st', N=10), 8 sampled instances), device tensors throughout, so that nothing but a block can
synchronise; the bound overrides go through the wrappers' keyword arguments.  Every comparison is bit-equality between two runs of the
same kernels on the same inputs, so no tolerance enters."""
import functools
import warnings

import numpy as np
import pytest

from conftest import constant_guess, make_problem, sample_instances

pytestmark = pytest.mark.gpu

ENTRIES = ('check_trajectory', 'check_guess', 'ik', 'score_rollout')
B, S, N_STEPS = 8, 4, 4
REFUSED = 'engine error -4: .* while the stream is being captured'


@functools.lru_cache(maxsize=None)
def setup():
    """(problem, net, device inputs, tightened bounds).  The tightened bound lies below instance 3's first joint: x_max[0] for the three
    state tests, q_hi[0] -- below the first joint of EVERY configuration that produced a target -- for the inverse kinematics."""
    import torch
    from safe_mpc_amd.ik import ik_eval, ik_params
    par, prob, net = make_problem('st', 'ext', N=10)
    nq = prob.nq
    x0 = sample_instances(prob, B, seed=0)
    xg, ug, p = constant_guess(prob, x0)
    q = x0[:, :nq]
    target = ik_eval(prob, q, np.zeros((B, 3)), ik_params(prob))['ee']
    # starts: the middle of the box, then three other sampled configurations per instance
    q_start = sample_instances(prob, B * S, seed=1)[:, :nq].reshape(B, S, nq).copy()
    q_start[:, 0] = 0.5 * (prob.x_min[:nq] + prob.x_max[:nq])
    x_log = np.repeat(x0[None], N_STEPS + 1, axis=0)
    u_log = np.zeros((N_STEPS, B, prob.nu))
    t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device='cuda:0')
    dev = dict(xg=t(xg), ug=t(ug), target=t(target), q_start=t(q_start), x_log=t(x_log), u_log=t(u_log))
    x_max = prob.x_max.copy()
    x_max[0] = q[3, 0] - 0.05
    q_hi = prob.x_max[:nq].copy()
    q_hi[0] = q[:, 0].min() - 0.05
    assert prob.x_min[0] < x_max[0] and prob.x_min[0] < q_hi[0]
    ee = np.asarray(prob.ee_ref, float) + 0.1           # (not the problem's own: the wrapper passes that one when none is given)
    return prob, net, dev, dict(x_max=x_max, q_hi=q_hi, ee_ref=ee)


def call(s, entry, tight=False, **kw):
    """one call of the entry point with the problem's own bounds, or with the tightened one; a tuple of device tensors"""
    prob, net, d, tb = setup()
    if entry == 'check_trajectory':
        return (s.check_trajectory(d['xg'], x_max=tb['x_max'] if tight else None),)
    if entry == 'check_guess':
        return s.check_guess(d['xg'], d['ug'], **({'x_max': tb['x_max']} if tight else {}))
    if entry == 'ik':
        return s.ik(d['target'], d['q_start'], **({'q_hi': tb['q_hi']} if tight else {}))
    return s.score_rollout(d['x_log'], d['u_log'], **{'ee_ref': tb['ee_ref'], **({'x_max': tb['x_max']} if tight else {}), **kw})


def new_solver():
    from safe_mpc_amd.solver import BatchedOcpSolver
    prob, net = setup()[:2]
    return BatchedOcpSolver(prob, net, device=0)


@functools.lru_cache(maxsize=None)
def solver():
    return new_solver()


@functools.lru_cache(maxsize=None)
def fresh_tight(entry):
    """the tightened call as the first call of a freshly created solver (read-only, shared)"""
    import torch
    s = new_solver()
    out = tuple(a.clone() for a in call(s, entry, tight=True))
    torch.cuda.synchronize()
    s.close()
    return out


def same(a, b):
    import torch
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def keep(out):
    import torch
    out = tuple(a.clone() for a in out)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('entry', ENTRIES)
def test_a_change_takes_effect_and_a_change_back_does_too(entry):
    s = solver()
    a = keep(call(s, entry))
    tight = keep(call(s, entry, tight=True))
    assert not same(tight, a)
    assert same(tight, fresh_tight(entry))
    assert same(keep(call(s, entry)), a)


@pytest.mark.parametrize('entry', ENTRIES)
def test_an_unchanged_block_is_accepted_inside_a_capture(entry):
    """The engine's stream joins the capture through BatchedOcpSolver._ordered, as in
    test_gpu_parity.py::test_buffer_growth_inside_a_graph_capture_is_a_state_error."""
    import torch
    s = solver()
    eager = keep(call(s, entry))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = call(s, entry)
    g.replay()
    torch.cuda.synchronize()
    assert same(out, eager)


def test_the_score_block_carries_ee_ref_across_a_call_with_traj():
    """A call with traj does not read ee_ref and keeps the last one in the block: the capture of a call with that ee_ref again is no
    change."""
    import torch
    s = solver()
    eager = keep(call(s, 'score_rollout'))
    traj = torch.tensor(np.linspace(0.2, 0.5, 3 * 6).reshape(3, 6), dtype=torch.float64, device='cuda:0')
    with_traj = keep(call(s, 'score_rollout', ee_ref=None, traj=traj))
    assert not same(with_traj, eager)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = call(s, 'score_rollout')
    g.replay()
    torch.cuda.synchronize()
    assert same(out, eager)


@pytest.mark.parametrize('entry', ENTRIES)
def test_a_changed_block_inside_a_capture_is_refused_and_the_capture_survives(entry):
    """SMPC_ESTATE instead of synchronising the capturing stream; the refused call enqueued nothing, the capture ends cleanly and the
    next eager call uploads the block."""
    import torch
    from safe_mpc_amd._lib import EngineError
    s = solver()
    keep(call(s, entry))
    with pytest.raises(EngineError, match=REFUSED), warnings.catch_warnings():
        warnings.filterwarnings('ignore', 'The CUDA Graph is empty')       # (the refused call captured nothing)
        with torch.cuda.graph(torch.cuda.CUDAGraph()):
            call(s, entry, tight=True)
    torch.cuda.synchronize()
    assert same(keep(call(s, entry, tight=True)), fresh_tight(entry))
