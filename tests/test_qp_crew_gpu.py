"""k_qp_ipm's crew (smpc_set_qp_crew; DESIGN.md section 4, point 4c): a launch of G wavefronts works through all pairs of instances, taking them
from a ticket.  Scheduling only -- every output byte must equal the full crew's (G = one wavefront per pair), which
tests/test_qp_pass_tables_gpu.py pins to the recorded bits.  -m gpu only.

6-DoF with six rows (the flagship's instantiation), N = 4 and N = 30, B = 1, 2, 37 (odd) and 130, G in {1, 2, 3, (B + 1) / 2}:
  * two solves of the same inputs per crew on a fresh handle: the first has no order (pairs in instance order), the second is ordered by
    the first one's iteration counts;
  * a policy step whose mask switches off a whole pair, one half of a pair and the last instance;
  * ticket hygiene with G = 2: three solves in a row, then the same solve captured once and replayed twice as a graph on the handle's
    stream -- the iteration histogram of every solve totals B (every instance solved exactly once) and the results are the eager bits.
"""
import ctypes as C

import numpy as np
import pytest

from conftest import constant_guess, make_problem, sample_instances

pytestmark = pytest.mark.gpu

HORIZONS = (4, 30)
BATCHES = (1, 2, 37, 130)
_cache = {}


def _inputs(N):
    """(prob, net, x0 [130]) of a horizon -- sampled once, moving starts (iteration counts that differ from instance to instance)"""
    if N not in _cache:
        par, prob, net = make_problem('st', 'ext', N=N)
        _cache[N] = (par, prob, net, sample_instances(prob, max(BATCHES), seed=11, vel_scale=0.4))
    return _cache[N]


def _crews(B):
    return [1, 2, 3, (B + 1) // 2]


def _solver(prob, net, waves):
    from safe_mpc_amd.solver import BatchedOcpSolver
    s = BatchedOcpSolver(prob, net)
    s.set_qp_mode('throughput')
    s.set_qp_crew(waves=waves)
    return s


def _dispatch(s):
    """(histogram [256], pair ticket) the last solve left on the handle"""
    out = np.zeros(520, np.int32)
    s.L.smpc_debug_qp_dispatch.argtypes = [C.c_void_p, C.c_void_p]
    assert s.L.smpc_debug_qp_dispatch(s.h, out.ctypes.data) == 0
    return out[:256], int(out[513])


def _same(a, b, what):
    for n, u, v in zip(('x', 'u', 'status', 'qp_iter'), a, b):
        u, v = np.asarray(u), np.asarray(v)
        assert u.dtype == v.dtype and u.shape == v.shape and u.tobytes() == v.tobytes(), f'{what}: {n} differs from the full crew'


@pytest.fixture(scope='module')
def full_crew():
    """the two solves of every (N, B) with a wavefront per pair: computed once, never modified"""
    ref = {}
    for N in HORIZONS:
        par, prob, net, x0 = _inputs(N)
        for B in BATCHES:
            s = _solver(prob, net, (B + 1) // 2)
            xg, ug, p = constant_guess(prob, x0[:B])
            ref[N, B] = [tuple(np.array(a) for a in s.solve(x0[:B], xg, ug, p)) for _ in range(2)]
            hist, ticket = _dispatch(s)
            assert np.array_equal(hist, np.bincount(ref[N, B][1][3], minlength=256)) and ticket == 0       # a full crew never draws a ticket
    return ref


@pytest.mark.parametrize('B', BATCHES)
@pytest.mark.parametrize('N', HORIZONS)
def test_every_crew_gives_the_full_crews_bytes(N, B, full_crew):
    par, prob, net, x0 = _inputs(N)
    xg, ug, p = constant_guess(prob, x0[:B])
    ref = full_crew[N, B]
    _same(ref[0], ref[1], f'N {N} B {B}: the ordered solve against the unordered one')       # (same inputs: the order changes nothing)
    print(f'N {N} B {B}: qp_iter min {ref[0][3].min()} max {ref[0][3].max()} status {np.unique(ref[0][2]).tolist()}')
    for G in _crews(B):
        s = _solver(prob, net, G)
        for k in range(2):      # k = 0: no order yet; k = 1: ordered by the first solve's iterations
            out = s.solve(x0[:B], xg, ug, p)
            _same(out, ref[k], f'N {N} B {B} G {G} solve {k}')
            hist, ticket = _dispatch(s)
            assert hist.sum() == B and np.array_equal(hist, np.bincount(out[3], minlength=256)), (N, B, G, k)
            g = min(G, (B + 1) // 2)
            # every wavefront of a partial crew draws until the tickets run out: pairs - G served, G draws that came back empty
            assert ticket == (0 if g == (B + 1) // 2 else (B + 1) // 2), (N, B, G, k, ticket)


def _policy_step(N, B, waves, mask, order_first):
    """one masked policy step on a fresh controller (after an unmasked one when `order_first`): everything the step leaves behind"""
    import torch
    from safe_mpc_amd import controller as Cn
    par, prob, net, x0 = _inputs(N)
    ctrl = Cn.get_controller('st', par, B, device_state=True)
    sv = ctrl.ocp_solver
    sv.set_qp_mode('throughput')
    sv.set_qp_crew(waves=waves)
    ctrl.setGuess(np.repeat(x0[:B, None, :], N + 1, axis=1), np.zeros((B, N, 6)))
    xd = torch.tensor(x0[:B], device='cuda')
    u_other = torch.tensor(np.random.default_rng(2).normal(size=(B, 6)), device='cuda')
    if order_first:
        ctrl.step_on_device(xd)
    u, ab = ctrl.step_on_device(xd, torch.tensor(mask, device='cuda'), u_other)
    sv.sync()
    hist, _ = _dispatch(sv)
    keep = {k: getattr(ctrl, k).cpu().numpy().copy() for k in ('x_guess', 'u_guess', 'last_status', 'qp_iter', 'fails', 'current_step')}
    keep['u'], keep['abort'] = u.cpu().numpy().copy(), ab.cpu().numpy().copy()
    live = np.asarray(mask)
    keep['x_temp'], keep['u_temp'] = ctrl.x_temp.cpu().numpy()[live], ctrl.u_temp.cpu().numpy()[live]
    return keep, hist


@pytest.mark.parametrize('order_first', [False, True])
@pytest.mark.parametrize('N', HORIZONS)
def test_masked_instances_sit_their_pair_out(N, order_first):
    B = 37
    mask = np.ones(B, bool)
    mask[[4, 5]] = False        # a whole pair (in instance order)
    mask[10] = False            # one half of a pair
    mask[B - 1] = False         # the last instance: the lone half of the odd batch's last pair
    ref, hist_ref = _policy_step(N, B, (B + 1) // 2, mask, order_first)
    assert hist_ref.sum() == B and hist_ref[0] >= 4         # the masked ones are counted with zero iterations
    for G in (1, 2, 3):
        got, hist = _policy_step(N, B, G, mask, order_first)
        assert np.array_equal(hist, hist_ref), (N, G)
        for k in ref:
            assert got[k].dtype == ref[k].dtype and got[k].tobytes() == ref[k].tobytes(), f'N {N} G {G} order {order_first}: {k}'


def test_ticket_hygiene_over_solves_and_graph_replays(full_crew):
    import torch
    N, B = 30, 37
    par, prob, net, x0 = _inputs(N)
    xg, ug, p = constant_guess(prob, x0[:B])
    ref = full_crew[N, B][1]
    s = _solver(prob, net, 2)
    dev = torch.device('cuda', 0)
    t = lambda a: torch.tensor(a, dtype=torch.float64, device=dev)
    xd, xgd, ugd, pd = t(x0[:B]), t(xg), t(ug), t(p)
    out = (torch.empty((B, N + 1, prob.nx), dtype=torch.float64, device=dev), torch.empty((B, N, prob.nu), dtype=torch.float64, device=dev),
           torch.empty((B,), dtype=torch.int32, device=dev), torch.empty((B,), dtype=torch.int32, device=dev))
    stream = torch.cuda.ExternalStream(s.L.smpc_stream(s.h), device=dev)
    torch.cuda.synchronize()

    def check(what):
        hist, ticket = _dispatch(s)
        got = tuple(a.cpu().numpy() for a in out)
        assert hist.sum() == B and np.array_equal(hist, np.bincount(got[3], minlength=256)), (what, hist.sum())
        assert ticket == (B + 1) // 2, (what, ticket)
        _same(got, ref, what)
        for a in out:
            a.zero_()
        torch.cuda.synchronize()

    with torch.cuda.stream(stream):
        for k in range(3):
            s.solve(xd, xgd, ugd, pd, out=out)
            check(f'eager solve {k}')
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream, capture_error_mode='relaxed'):
            s.solve(xd, xgd, ugd, pd, out=out)
        for k in range(2):
            g.replay()
            check(f'graph replay {k}')
        s.solve(xd, xgd, ugd, pd, out=out)
        check('eager solve after the replays')
