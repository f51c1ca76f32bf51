"""The streams of engine handles (engine.hip: create_handle_stream): three busy handles beside an idle one run side by side, running
side by side changes no bit, and SMPC_STREAM_PRIORITY=default -- the plain stream of earlier builds -- gives the same bits.  -m gpu only.

The process is set up as a bench process is: a torch tensor on the device first (the null stream exists), one handle that serves
``check_trajectory`` and then idles (the bench's probe handle), three handles that each solve the same 256 instances of controller
'st' at N = 30 from device-resident inputs, each under its own stream as the bench's sub-batches are (``torch.cuda.stream`` of the
handle's ExternalStream: no ordering against torch's current stream).  The throughput form is forced: 256 instances are 128
one-wavefront blocks of k_qp_ipm, three launches 384 blocks on 256 CUs -- lone wavefronts (scripts/qp_launch_time.py), where company
on the chip costs a few percent at most.  (The form the engine would pick by itself at 256 instances, a 4-wave workgroup per
instance with 72 KB of LDS, fills the chip with two launches: a third could not run beside them whatever the queues do.)

The bound of the first test is a model, not a measurement: t3 / t1 is 1.0-1.15 when the three launches share the chip, 2 when two of
the handles share a hardware queue and take turns, 3 when all do; 1.5 is the midpoint of the first two.  Measured with four queues per
priority level (profiles/stream_queues_trace.txt): 1.20 on this build (1.25 under SMPC_STREAM_PRIORITY=low), 2.11 on the build before
create_handle_stream and under SMPC_STREAM_PRIORITY=default, where the test fails as it should.
"""
import gc
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from conftest import constant_guess, make_problem, sample_instances

pytestmark = pytest.mark.gpu

B = 256
NAMES = ('x', 'u', 'status', 'qp_iter')


class _Rig:
    pass


@pytest.fixture(scope='module')
def rig():
    import torch
    from safe_mpc_amd.solver import BatchedOcpSolver
    dev = torch.device('cuda', 0)
    gc.collect()      # (a handle an earlier test dropped without closing still holds its stream, and with it a share of a queue)
    first = torch.zeros(16, dtype=torch.float64, device=dev)      # the null stream, before any engine stream
    par, prob, net = make_problem('st')
    x0 = sample_instances(prob, B, seed=3)
    xg, ug, p = constant_guess(prob, x0)
    r = _Rig()
    r.torch, r.first = torch, first
    r.idle = BatchedOcpSolver(prob, net)
    assert r.idle.check_trajectory(x0[:, None, :], tol_x=0.0, row_lb=prob.row_lb, row_ub=prob.row_ub).all()
    r.solvers = [BatchedOcpSolver(prob, net) for _ in range(3)]
    t = lambda a: torch.tensor(a, dtype=torch.float64, device=dev)
    r.inputs = (t(x0), t(xg), t(ug), t(p))
    N, nx, nu = prob.N, prob.nx, prob.nu
    r.streams, r.outs = [], []
    for sv in r.solvers:
        sv.set_qp_mode('throughput')
        r.streams.append(torch.cuda.ExternalStream(sv.L.smpc_stream(sv.h), device=dev))
        r.outs.append((torch.empty((B, N + 1, nx), dtype=torch.float64, device=dev), torch.empty((B, N, nu), dtype=torch.float64, device=dev),
                       torch.empty((B,), dtype=torch.int32, device=dev), torch.empty((B,), dtype=torch.int32, device=dev)))
    torch.cuda.synchronize()      # (the engine's streams are non-blocking: the inputs above were written on the null stream)
    for _ in range(2):
        for i in range(3):
            _enqueue(r, i)
        _sync_all(r)
    yield r
    for sv in r.solvers + [r.idle]:
        sv.close()


def _enqueue(r, i):
    with r.torch.cuda.stream(r.streams[i]):
        r.solvers[i].solve(*r.inputs, out=r.outs[i])


def _sync_all(r):
    for sv in r.solvers:
        sv.sync()


def _host_copy(r, i):
    return tuple(a.cpu().numpy().copy() for a in r.outs[i])


def test_three_handles_beside_an_idle_one_run_side_by_side(rig):
    r = rig
    t1s, t3s = [], []
    for _ in range(5):
        _sync_all(r)
        t0 = time.perf_counter()
        _enqueue(r, 0)
        r.solvers[0].sync()
        t1s.append(time.perf_counter() - t0)
    for _ in range(5):
        _sync_all(r)
        t0 = time.perf_counter()
        for i in range(3):
            _enqueue(r, i)
        _sync_all(r)
        t3s.append(time.perf_counter() - t0)
    t1, t3 = float(np.median(t1s)), float(np.median(t3s))
    print(f'stream queues: t1 {1e3 * t1:.3f} ms (one handle), t3 {1e3 * t3:.3f} ms (three enqueued back to back), t3 / t1 = {t3 / t1:.3f} '
          f'(side by side 1.0-1.15, two on one queue 2, all on one 3; bound 1.5); SMPC_HIP_LIB={os.environ.get("SMPC_HIP_LIB", "")} '
          f'SMPC_STREAM_PRIORITY={os.environ.get("SMPC_STREAM_PRIORITY", "")}')
    assert t3 < 1.5 * t1


def test_side_by_side_changes_no_bit(rig):
    r = rig
    _sync_all(r)
    for i in range(3):
        _enqueue(r, i)
    _sync_all(r)
    together = [_host_copy(r, i) for i in range(3)]
    for o in r.outs:
        for a in o:
            a.zero_()
    r.torch.cuda.synchronize()
    for i in range(3):
        _enqueue(r, i)
        r.solvers[i].sync()
        alone = _host_copy(r, i)
        assert (alone[3] > 0).all(), 'the solves did not run'      # (every instance takes at least one interior-point iteration)
        for n, a, b in zip(NAMES, together[i], alone):
            assert np.array_equal(a, b), f'handle {i}: {n} differs between the concurrent and the sequential solve'


def _small_solve():
    """handle creation and a B = 8 solve (host arrays): the outputs"""
    from safe_mpc_amd.solver import BatchedOcpSolver
    par, prob, net = make_problem('st', 'ext', N=10)
    x0 = sample_instances(prob, 8, seed=0)
    sv = BatchedOcpSolver(prob, net)
    out = tuple(np.array(a) for a in sv.solve(x0, *constant_guess(prob, x0)))
    sv.close()
    return out


def test_switch_default_gives_the_same_bits(tmp_path):
    """SMPC_STREAM_PRIORITY is read once per process: `default` runs in a fresh child (started here, never an exec of this process)."""
    here = _small_solve()
    assert (here[3] > 0).all()
    f = str(tmp_path / 'default_route.npz')
    env = dict(os.environ, SMPC_STREAM_PRIORITY='default')
    res = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', f], env=env, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    with np.load(f) as z:
        for n, a in zip(NAMES, here):
            assert a.dtype == z[n].dtype and np.array_equal(a, z[n]), f'{n} differs under SMPC_STREAM_PRIORITY=default'


if __name__ == '__main__':
    if sys.argv[1:2] != ['--child'] or len(sys.argv) != 3:
        sys.exit('usage: python tests/test_stream_queues_gpu.py --child <file.npz>   (the child of test_switch_default_gives_the_same_bits)')
    np.savez(sys.argv[2], **dict(zip(NAMES, _small_solve())))
