#!/usr/bin/env python3
"""The GPU timings of profiles/ik.txt, all in one process on one GPU: smpc_ik_batch at the default settings
(40 iterations) with device pointers, by HIP events on the handle's stream (3 warm-up calls, mean of 10 back-to-back calls),

* B = 4096, S = 64 on the 6-DoF arm with its six capsule rows,
* B = 4096, S = 16 on the 7-DoF arm with its sphere and plane rows,

next to the wall time of the numpy statement (ik.ik_batch_host) on the first 256 instances of the same inputs, and how many
instances each side solves.  Targets: ee(q*) of Halton q* in the joint box (reachable, not necessarily collision-free there);
starts: Halton points in the box.

    python scripts/ik_bench.py [output file]
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch                                                # noqa: E402
from safe_mpc_amd.closed_loop import halton                 # noqa: E402
from safe_mpc_amd.ik import ik_batch_host, ik_eval, ik_params  # noqa: E402
from safe_mpc_amd.parser import Parameters                  # noqa: E402
from safe_mpc_amd.problem import OcpProblem                 # noqa: E402
from safe_mpc_amd.solver import BatchedOcpSolver            # noqa: E402

OUT = open(sys.argv[1], 'a') if len(sys.argv) > 1 else open(os.devnull, 'w')


def say(*a):
    line = ' '.join(str(x) for x in a)
    print(line, flush=True)
    OUT.write(line + '\n')
    OUT.flush()


def problem(name):
    if name == 'z1':
        par = Parameters({}, 'z1')
        par.nq, par.n_dof_safe_set, par.net_size = 6, 6, [12, 256, 1]
    else:
        par = Parameters({}, 'fr7', filename=os.path.join(ROOT, 'config_fr7.yaml'))
    return OcpProblem(par, 'naive', 'ext', N=10)


B, HOST_B = 4096, 256
dev = torch.device('cuda', 0)
say('# python scripts/ik_bench.py -- smpc_ik_batch, 40 iterations, device pointers; one MI355X, one session')
say('robot | rows | B | S | ms per call | instances solved | statement on the first 256 instances: s | the same scaled to B (x16) | solved of 256')
for name, S in (('z1', 64), ('fr7', 16)):
    prob = problem(name)
    nq = prob.nq
    lo, hi = prob.x_min[:nq], prob.x_max[:nq]
    q_star = lo + halton(B, nq, skip=5) * (hi - lo)
    tgt = np.ascontiguousarray(ik_eval(prob, q_star, np.zeros((B, 3)), ik_params(prob))['ee'])
    qs = np.ascontiguousarray((lo + halton(B * S, nq, skip=100003) * (hi - lo)).reshape(B, S, nq))
    sv = BatchedOcpSolver(prob, None)
    t_d, q_d = torch.as_tensor(tgt, device=dev), torch.as_tensor(qs, device=dev)
    out = (torch.zeros((B, nq), dtype=torch.float64, device=dev), torch.zeros((B, 2), dtype=torch.int32, device=dev),
           torch.zeros((B, 2), dtype=torch.float64, device=dev))
    call = lambda: sv.ik(t_d, q_d, q_out=out[0], info=out[1], resid=out[2])
    for _ in range(3):
        call()
    sv.sync()
    reps = 10
    with torch.cuda.stream(sv._ext_stream):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            call()
        e1.record()
    e1.synchronize()
    ms = e0.elapsed_time(e1) / reps
    solved = int((out[1][:, 1] > 0).sum().item())
    t0 = time.perf_counter()
    _, info_h, _ = ik_batch_host(prob, tgt[:HOST_B], qs[:HOST_B])
    th = time.perf_counter() - t0
    agree = int(((out[1][:HOST_B, 1] > 0).cpu().numpy() == (info_h[:, 1] > 0)).sum())
    say(f'{name} | {len(prob.rows)} | {B} | {S} | {ms:.3f} | {solved} | {th:.2f} | {th * B / HOST_B:.1f} | {int((info_h[:, 1] > 0).sum())} '
        f'(the two sides agree on {agree} of {HOST_B})')
