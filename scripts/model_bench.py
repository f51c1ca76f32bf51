#!/usr/bin/env python3
"""What a controller model per instance costs (smpc_set_instance_models; profiles/instance_models.txt): the stage builder's time of
one solve (smpc_get_timing ms[0], HIP events on the handle's stream) and the whole solve, at the bench's workload (Z1, 'st', N = 30,
B = 4096 unless SMPC_B), with the shared model and with a model per instance -- the SAME inputs and the SAME robot (every instance
gets the descriptor's own inertials, so both runs solve the same QPs), alternating the two, SMPC_ROUNDS (default 5) rounds of
SMPC_REPS (default 10) timed solves each after a warm-up.

    python scripts/model_bench.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench                                                   # noqa: E402
from safe_mpc_amd.solver import BatchedOcpSolver               # noqa: E402


def main():
    import torch
    par, prob, net = bench.build_problem()
    B, N = int(os.environ.get('SMPC_B', '4096')), prob.N
    rounds, reps = int(os.environ.get('SMPC_ROUNDS', '5')), int(os.environ.get('SMPC_REPS', '10'))
    s = BatchedOcpSolver(prob, net)
    x0 = bench.initial_states(s, prob, B, 0)
    xg = np.repeat(x0[:, None, :], N + 1, axis=1)
    p = np.zeros((B, N + 1, 5))
    p[:, :, :3], p[:, :, 3], p[:, :, 4] = prob.ee_ref, par.alpha, 1.0
    dev = lambda a: torch.tensor(a, dtype=torch.float64, device=f'cuda:{s.device}')
    x0_d, xg_d, ug_d, p_d = dev(x0), dev(xg), dev(np.zeros((B, N, prob.nu))), dev(p)
    table = dev(np.repeat(prob.joint_table()[None], B, axis=0).view(np.float64).reshape(B, prob.nq, -1))
    out = s.solve(x0_d, xg_d, ug_d, p_d)
    shared = [a.clone() for a in out]
    s.enable_timing(2)
    res = {False: [], True: []}
    for r in range(rounds + 1):                                 # (round 0 warms both paths up)
        for own in (False, True):
            s.set_instance_models(table if own else None)
            lin, tot = [], []
            for _ in range(reps):
                s.solve(x0_d, xg_d, ug_d, p_d, out=out)
                s.sync()
                t = s.timing_history(0)
                lin.append(1e3 * t['time_lin'])
                tot.append(1e3 * t['time_tot'])
            if r:
                res[own].append((np.mean(lin), np.min(lin), np.mean(tot)))
                print(f'round {r} {"model per instance" if own else "shared model      "}: builder mean {np.mean(lin):.4f} ms, min {np.min(lin):.4f} ms; '
                      f'solve mean {np.mean(tot):.3f} ms', flush=True)
            elif own:
                print('same QPs: the solve with the descriptor\'s inertials per instance equals the shared one bit for bit:',
                      all(torch.equal(a, b) for a, b in zip(out, shared)), flush=True)
    for own in (False, True):
        a = np.array(res[own])
        print(f'{"model per instance" if own else "shared model      "}: builder {a[:, 0].mean():.4f} ms (rounds {a[:, 0].min():.4f} .. {a[:, 0].max():.4f}), '
              f'solve {a[:, 2].mean():.3f} ms (rounds {a[:, 2].min():.3f} .. {a[:, 2].max():.3f}); B = {B}, N = {N}, nq = {prob.nq}, '
              f'table = {table.numel() * 8 / 1e6:.2f} MB')


if __name__ == '__main__':
    main()
