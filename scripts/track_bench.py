#!/usr/bin/env python3
"""What a scene track costs (smpc_set_instance_scene_track; profiles/scene_tracks.txt): the stage builder's time of one solve
(smpc_get_timing ms[0], HIP events on the handle's stream) and the whole solve, at the bench's workload (Z1, 'st', N = 30,
B = 4096 unless SMPC_B), in the modes of SMPC_MODES (default shared,scene,track): the shared scene, a scene per instance, and a
track of SMPC_T (default 131) columns per instance read at clock SMPC_CLOCK (default 50, so that node k reads column 50 + k).
The SAME inputs and the SAME world throughout -- every instance gets the base geometry in every column, so all modes solve the
same QPs -- alternating the modes, SMPC_ROUNDS (default 5) rounds of SMPC_REPS (default 10) timed solves each after a warm-up.
With SMPC_HIP_LIB naming the parent commit's library, SMPC_MODES=shared,scene gives the parent's figures.

    python scripts/track_bench.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench                                                   # noqa: E402
from safe_mpc_amd.solver import BatchedOcpSolver               # noqa: E402

NAMES = {'shared': 'shared scene      ', 'scene': 'scene per instance', 'track': 'track per instance'}


def main():
    import torch
    par, prob, net = bench.build_problem()
    B, N = int(os.environ.get('SMPC_B', '4096')), prob.N
    rounds, reps = int(os.environ.get('SMPC_ROUNDS', '5')), int(os.environ.get('SMPC_REPS', '10'))
    T, clock = int(os.environ.get('SMPC_T', '131')), int(os.environ.get('SMPC_CLOCK', '50'))
    modes = os.environ.get('SMPC_MODES', 'shared,scene,track').split(',')
    s = BatchedOcpSolver(prob, net)
    x0 = bench.initial_states(s, prob, B, 0)
    xg = np.repeat(x0[:, None, :], N + 1, axis=1)
    p = np.zeros((B, N + 1, 5))
    p[:, :, :3], p[:, :, 3], p[:, :, 4] = prob.ee_ref, par.alpha, 1.0
    device = torch.device('cuda', s.device)
    dev = lambda a: torch.tensor(a, dtype=torch.float64, device=device)
    x0_d, xg_d, ug_d, p_d = dev(x0), dev(xg), dev(np.zeros((B, N, prob.nu))), dev(p)
    geom = dev(np.repeat(prob.row_geometry()[None], B, axis=0))
    track = geom[:, None].expand(B, T, *geom.shape[1:]).contiguous() if 'track' in modes else None
    cell = torch.full((1,), clock, dtype=torch.int64, device=device)
    out = s.solve(x0_d, xg_d, ug_d, p_d)
    s.enable_timing(2)
    res = {m: [] for m in modes}
    for r in range(rounds + 1):                                 # (round 0 warms every path up)
        for m in modes:
            if m == 'track':
                s.set_instance_scene_track(track)
                s.set_scene_clock(cell)
            else:
                s.set_instance_scene(geom if m == 'scene' else None)
            lin, tot = [], []
            for _ in range(reps):
                s.solve(x0_d, xg_d, ug_d, p_d, out=out)
                s.sync()
                t = s.timing_history(0)
                lin.append(1e3 * t['time_lin'])
                tot.append(1e3 * t['time_tot'])
            if r:
                res[m].append((np.mean(lin), np.min(lin), np.mean(tot)))
                print(f'round {r} {NAMES[m]}: builder mean {np.mean(lin):.4f} ms, min {np.min(lin):.4f} ms; solve mean {np.mean(tot):.3f} ms', flush=True)
    for m in modes:
        a = np.array(res[m])
        size = {'shared': 0, 'scene': geom.numel(), 'track': 0 if track is None else track.numel()}[m] * 8 / 1e6
        print(f'{NAMES[m]}: builder {a[:, 0].mean():.4f} ms (rounds {a[:, 0].min():.4f} .. {a[:, 0].max():.4f}), '
              f'solve {a[:, 2].mean():.3f} ms (rounds {a[:, 2].min():.3f} .. {a[:, 2].max():.3f}); B = {B}, N = {N}, {len(prob.rows)} rows, '
              f'geometry = {size:.2f} MB' + (f', T = {T}, clock {clock}' if m == 'track' else ''))


if __name__ == '__main__':
    main()
