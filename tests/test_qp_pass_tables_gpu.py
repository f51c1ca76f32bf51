"""k_qp_ipm's factorisation sweep on the shapes that reach every branch of its lane-parallel passes (the u-u triangle, the u-x
block, the x-x triangle of the P update, the end stage's own x-x loop), throughput form forced.  -m gpu only.

Two closed-loop steps per case (solve, provide_control, plant_step, guess_correction: all on the engine), each solve held

  * to the CPU oracle on the same inputs, with the tolerances of test_gpu_parity.py::test_kernel_instantiations_and_odd_batches
    (status equal, qp_iter within 2, u within 1e-4 (1 + |u|inf), x within 1e-4), and
  * to the bits the engine returned before the passes' index handling was touched: tests/golden/qp_pass_tables_parent.npz holds
    x_out, u_out, status, qp_iter of every case and step as recorded then (``python tests/test_qp_pass_tables_gpu.py --dump`` on
    that build).  The passes may change where an address or a predicate comes from, never an operand or the order of a sum: any bit
    that differs is a failure.

Cases (name: nq, rows, N, B):
  nq5 .......... 5, 6 rows (odd nq: padded rows, the unpaired D-scaling), N = 12, B = 3
  nq6 .......... 6, 6 rows, N = 30, B = 8 (the flagship's instantiation and horizon)
  nq7 .......... 7, 4 rows, N = 16, B = 3
  rows3 ........ 6, 3 rows (runtime row count), N = 12, B = 1 (one half-wave, no twin)
  rows0 ........ 6, no collision rows, N = 12, B = 3 (odd batch)
  n2 / n3 ...... 6, 6 rows, N = 2 (the end stage and stage 0 only: no P update at all) and N = 3, B = 3 / B = 1
"""
import os
import sys

import numpy as np
import pytest

from conftest import constant_guess, make_problem, make_problem_fr7, sample_instances

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'qp_pass_tables_parent.npz')
CASES = ['nq5', 'nq6', 'nq7', 'rows3', 'rows0', 'n2', 'n3']
STEPS = 2
NAMES = ('x', 'u', 'status', 'qp_iter')


def _case(name):
    """(prob, net, x0) of a case; rows are dropped from the descriptor after the states were sampled against the full geometry"""
    nq, N, B, rows = {'nq5': (5, 12, 3, None), 'nq6': (6, 30, 8, None), 'nq7': (7, 16, 3, None), 'rows3': (6, 12, 1, 3),
                      'rows0': (6, 12, 3, 0), 'n2': (6, 2, 3, None), 'n3': (6, 3, 1, None)}[name]
    par, prob, net = make_problem_fr7(N=N) if nq == 7 else make_problem('st', 'ext', N=N, nq=nq)
    x0 = sample_instances(prob, B, seed=5, vel_scale=0.1)
    if rows is not None:
        assert rows < prob.desc.n_rows
        prob.desc.n_rows = rows
    return prob, net, x0


def _run(name, with_oracle):
    """the engine's two closed-loop steps of a case: [(x, u, status, qp_iter)] per step, and the oracle's solve of each step's inputs"""
    from safe_mpc_amd.solver import BatchedOcpSolver
    prob, net, x = _case(name)
    s = BatchedOcpSolver(prob, net)
    s.set_qp_mode('throughput')
    orc = None
    if with_oracle:
        from oracle.oracle import Oracle
        orc = Oracle(prob, (net.weights, net.biases))
    xg, ug, p = constant_guess(prob, x)
    eng, ref = [], []
    for _ in range(STEPS):
        out = tuple(np.array(a) for a in s.solve(x, xg, ug, p))
        eng.append(out)
        if orc is not None:
            ref.append(orc.solve_batch(x, xg, ug, p))
        xg, ug, ua = s.provide_control((out[2] == 0).astype(np.int32), out[0], out[1], xg, ug)
        x, _ = s.plant_step(x, ua)
        xg = s.guess_correction(xg, ug)
    return eng, ref


@pytest.fixture(scope='module')
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize('name', CASES)
def test_pass_shapes_against_oracle_and_recorded_bits(name, golden):
    eng, ref = _run(name, True)
    for k, ((xa, ua, sa, ia), (xb, ub, sb, ib)) in enumerate(zip(eng, ref)):
        ok = sb == 0
        scale = 1 + np.abs(ub[ok]).max()
        print(f'{name} step {k}: status {sa.tolist()} qp_iter {ia.tolist()} / oracle {ib.tolist()}, u {np.abs(ua[ok] - ub[ok]).max() / scale:.2e} '
              f'(1e-4) x {np.abs(xa[ok] - xb[ok]).max():.2e} (1e-4)')
        assert np.array_equal(sa, sb)
        assert ok.sum() >= len(sb) - 1
        assert np.abs(ia[ok].astype(int) - ib[ok].astype(int)).max() <= 2
        assert np.abs(ua[ok] - ub[ok]).max() < 1e-4 * scale
        assert np.abs(xa[ok] - xb[ok]).max() < 1e-4
    for k, out in enumerate(eng):
        for n, a in zip(NAMES, out):
            g = golden[f'{name}/{k}/{n}']
            assert a.dtype == g.dtype and a.shape == g.shape, (name, k, n)
            assert a.tobytes() == g.tobytes(), f'{name} step {k}: {n} is not the recorded bits'


if __name__ == '__main__':
    if sys.argv[1:2] != ['--dump'] or len(sys.argv) > 3:
        sys.exit('usage: python tests/test_qp_pass_tables_gpu.py --dump [file]   (records the loaded engine build\'s results as the golden file)')
    GOLDEN = sys.argv[2] if len(sys.argv) == 3 else GOLDEN
    rec = {}
    for name in CASES:
        for k, out in enumerate(_run(name, False)[0]):
            for n, a in zip(NAMES, out):
                rec[f'{name}/{k}/{n}'] = a
            print(name, k, 'status', out[2].tolist(), 'qp_iter', out[3].tolist())
    np.savez_compressed(GOLDEN, **rec)
    print('wrote', GOLDEN, os.path.getsize(GOLDEN), 'bytes')
