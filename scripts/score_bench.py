#!/usr/bin/env python3
"""The measurements of profiles/score_rollout.txt, all in one process on one GPU:

* smpc_score_rollout on Z1 with its six collision rows, n_steps = 300, at B = 4096 and B = 65 536, with and without the safe-set
  score, by HIP events on the handle's stream (warm-up, then the mean of 20 back-to-back calls); next to each time the bytes the call
  must read (144 B per step and instance: the logged state and control; with the safe-set score the network pass and k_score_safe
  read the state again) and the share of the HBM peak that this corresponds to;
* the wall time of the existing closed_loop_costs path (scripts/metrics_count_fails.py: one linearisation record per node through
  smpc_eval_nodes) at the largest B of the list below whose records fit in host memory.

    python scripts/score_bench.py [output file]
"""
import importlib.util, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import bench
from safe_mpc_amd.problem import NODE_EVAL_DTYPE
from safe_mpc_amd.solver import BatchedOcpSolver

OUT = open(sys.argv[1], 'w') if len(sys.argv) > 1 else open(os.devnull, 'w')
def say(*a):
    line = ' '.join(str(x) for x in a)
    print(line, flush=True)
    OUT.write(line + '\n'); OUT.flush()

HBM_PEAK = 8.0e12            # B/s, the MI355X's specification
T = 300
par, prob, net = bench.build_problem(controller='htwa')
nq, nx = prob.nq, prob.nx
s = BatchedOcpSolver(prob, net)
dev = torch.device('cuda', 0)
say(f'# python scripts/score_bench.py -- smpc_score_rollout on Z1 ({prob.desc.n_rows} collision rows), n_steps = {T}; one MI355X, one session')

def logs(B, seed=0):
    """a slow random walk inside the joint box with small velocities, generated on the device"""
    g = torch.Generator(device=dev); g.manual_seed(seed)
    lo, hi = torch.tensor(prob.x_min[:nq], device=dev), torch.tensor(prob.x_max[:nq], device=dev)
    q0 = lo + torch.rand((1, B, nq), generator=g, device=dev, dtype=torch.float64) * (hi - lo)
    x = torch.empty((T + 1, B, nx), dtype=torch.float64, device=dev)
    x[:, :, :nq] = q0 + torch.cumsum(0.002 * torch.randn((T + 1, B, nq), generator=g, device=dev, dtype=torch.float64), 0)
    x[:, :, nq:] = 0.1 * (2 * torch.rand((T + 1, B, nq), generator=g, device=dev, dtype=torch.float64) - 1) * torch.tensor(prob.x_max[nq:], device=dev)
    u = 4 * torch.rand((T, B, nq), generator=g, device=dev, dtype=torch.float64) - 2
    return x, u

def timed(fn, reps=20):
    with torch.cuda.stream(s._ext_stream):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps

say('## smpc_score_rollout, device pointers (HIP events, 3 warm-up calls, mean of 20 back-to-back calls)')
say('# the calls rotate over logs that together exceed the 256 MB Infinity Cache (4 logs of 177 MB at B = 4096; one log of 2.84 GB at')
say('# 65 536 does by itself), so that a call finds none of its log on the die and the last column is a share of HBM bandwidth')
say('B | safe-set score | ms | bytes the call must read | that over the time | share of the 8 TB/s HBM peak')
for B in (4096, 65536):
    sets = [logs(B, seed) for seed in range(4 if B == 4096 else 1)]
    x, u = sets[0]
    out = torch.zeros((B, 7), dtype=torch.float64, device=dev); outi = torch.zeros((B, 4), dtype=torch.int32, device=dev)
    for safe in (False, True):
        turn = [0]
        def call():
            xs, us = sets[turn[0] % len(sets)]
            turn[0] += 1
            s.score_rollout(xs, us, want_safe=safe, out=out, outi=outi)
        for _ in range(max(3, len(sets))):
            call()
        s.sync()
        turn[0] = 1                 # (the timed calls end on log 0, whose scores are compared below)
        ms = timed(call)
        # the log once (96 B of state for T + 1 steps, 48 B of control for T); with the safe-set score the network's feature pass
        # reads the state again (96 B) and k_score_safe the velocities and the network's output (48 + 4 B)
        need = B * ((T + 1) * 8 * nx + T * 8 * nq) + (B * (T + 1) * (8 * nx + 8 * nq + 4) if safe else 0)
        say(f'{B} | {"yes" if safe else "no"} | {ms:.3f} | {need / 1e6:.1f} MB | {need / (ms * 1e-3) / 1e12:.3f} TB/s | {100 * need / (ms * 1e-3) / HBM_PEAK:.1f} %')
    if B == 4096:
        keep = (x.cpu().numpy(), u.cpu().numpy(), out.cpu().numpy().copy())
    del x, u, out, outi, sets
    torch.cuda.empty_cache()

say('## the existing path: closed_loop_costs of scripts/metrics_count_fails.py (one smpc_node_eval record per node, N + 1 = 3 nodes per state)')
spec = importlib.util.spec_from_file_location('metrics_count_fails', os.path.join(ROOT, 'scripts', 'metrics_count_fails.py'))
m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
_, prob2, _ = bench.build_problem(N=2, controller='naive')
s2 = BatchedOcpSolver(prob2, None)
per_state = 3 * (NODE_EVAL_DTYPE.itemsize + 8 * nx + 8 * nq + 8 * 5)
avail = os.sysconf('SC_PHYS_PAGES') * os.sysconf('SC_PAGE_SIZE')
say(f'records and inputs per logged state: {per_state} B; host memory {avail / 1e9:.0f} GB')
xh, uh, cost_dev = keep
fits = [n for n in (4096, 1024, 256) if 2.5 * n * (T + 1) * per_state < avail]    # (the records, numpy temporaries)
if not fits:
    say(f'closed_loop_costs: not run, the records of 256 instances ({256 * (T + 1) * per_state / 1e9:.1f} GB) do not fit')
    OUT.close()
    sys.exit(0)
n = fits[0]
xs, us = np.ascontiguousarray(np.transpose(xh[:, :n], (1, 0, 2))), np.ascontiguousarray(np.transpose(uh[:, :n], (1, 0, 2)))
t0 = time.perf_counter()
costs = m.closed_loop_costs(par, prob2, s2, xs, us)
w = time.perf_counter() - t0
say(f'closed_loop_costs at B = {n} (the largest of 4096, 1024, 256 whose {n * (T + 1) * per_state / 1e9:.1f} GB of records fit): {w:.2f} s wall')
say(f'largest relative difference of its costs from smpc_score_rollout\'s d0: {np.max(np.abs(costs - cost_dev[:n, 0]) / np.abs(costs)):.2e}')
say(f'B = 65536: {65536 * (T + 1) * per_state / 1e9:.0f} GB of records -- not run')
OUT.close()
