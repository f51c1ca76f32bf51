#!/usr/bin/env python3
"""ms per closed-loop step of the full policy layer with all state in HBM (run_mpc(on_device=True)): the controller's
accept / reject / abort automaton, the driver's backup-OCP + PD abort handling, plant and outcome tests -- at the bench's
workload size (B = 4096, Z1, N = 30), next to the plain-policy number bench.py reports.

    python scripts/policy_bench.py [controller ...]      (default: st htwa receding)
SMPC_WARM=1: start from generate_guess warm starts (full SQP with merit backtracking on the hard-terminal OCP, as the reference's
guess_acados.py writes them for every safe-set controller, utils.py:46-58, and scripts/mpc.py:79-84 loads them) instead of the
constant guess -- what the reference times; the share of infeasible QPs is then the policy's, not the cold start's.
SMPC_WARM_DEVICE=1: generate them with the engine's device-resident SQP (generate_guess(on_device=True), smpc_sqp_batch) instead of
the host loop; SMPC_WARM_UNTIL=1: generate them until SMPC_B are accepted (generate_guess_until; SMPC_WARM_ACCEPT = final | first,
SMPC_WARM_EVERY = iterations per round, SMPC_WARM_BATCH = device slots), so the loop runs on as many instances as were asked for;
SMPC_WARM_STATS=1 runs the generation a second time with a history, to report SQP iterations and trial passes (with SMPC_WARM_UNTIL=1
it prints the loop's own iteration counts instead).
SMPC_SCENE_JITTER=SIGMA: every instance runs in a scene of its own (run_mpc(scenes=problem.jittered_scenes(prob, B, SIGMA)); 0 = the
base geometry for every instance, i.e. the same world through the scene-aware kernels: the cost of a scene, profiles/instance_scenes.txt).
SMPC_SCENE_VELOCITY=SIGMA: every instance runs in a scene TRACK of its own, steps + 1 + N columns (run_mpc(scenes=problem.moving_scenes(prob,
B, T, SIGMA, sigma=SMPC_SCENE_JITTER or 0)); 0 = the base geometry in every column, the same world through the track: the cost of a track,
profiles/scene_tracks.txt)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench                                                   # noqa: E402
from safe_mpc_amd import closed_loop as cl                     # noqa: E402
from safe_mpc_amd.solver import BatchedOcpSolver               # noqa: E402


def main():
    names = sys.argv[1:] or ['st', 'htwa', 'receding']
    par, prob, net = bench.build_problem()
    par.back_hor = 30
    B, N, steps = int(os.environ.get('SMPC_B', '4096')), prob.N, int(os.environ.get('SMPC_STEPS', '60'))
    s = BatchedOcpSolver(prob, net)
    x0 = bench.initial_states(s, prob, B, 0)
    xg = np.repeat(x0[:, None, :], N + 1, axis=1)
    ug = np.zeros((B, N, prob.nu))
    warm = os.environ.get('SMPC_WARM', '0') == '1'
    if warm:
        import copy
        pg = copy.copy(par)
        pg.nlp_max_iter = int(os.environ.get('SMPC_SQP_ITERS', '60'))
        on_dev = os.environ.get('SMPC_WARM_DEVICE', '0') == '1'
        t0 = time.perf_counter()
        until = os.environ.get('SMPC_WARM_UNTIL', '0') == '1'
        if until:
            guess, info = cl.generate_guess_until(pg, 'htwa', B, batch=int(os.environ['SMPC_WARM_BATCH']) if 'SMPC_WARM_BATCH' in os.environ else None,
                                                  check_every=int(os.environ.get('SMPC_WARM_EVERY', '50')),
                                                  accept=os.environ.get('SMPC_WARM_ACCEPT', 'final'))
            xg, ug = guess['xg'], guess['ug']
            B = len(xg)
            print(f'warm starts (device SQP until accepted): {B} of {info["issued"]} samples accepted in {info["rounds"]} rounds, '
                  f'{info["instance_iterations"]} instance-iterations, budget {pg.nlp_max_iter} ({time.perf_counter() - t0:.2f} s); '
                  f'running {B} instances', flush=True)
            if os.environ.get('SMPC_WARM_STATS', '0') == '1':          # (no second run here: the loop keeps its own counts)
                it = np.array(list(info['iters'].values()))
                print(f'  SQP iterations per sample min / median / max {it.min()} / {int(np.median(it))} / {it.max()}, '
                      f'{len(info["failed"])} samples failed, {info["instance_iterations"] / max(info["rounds"], 1):.0f} instance-iterations per round',
                      flush=True)
        else:
            guess, good = cl.generate_guess(pg, 'htwa', B, on_device=on_dev)
            xg, ug = guess['xg'], guess['ug']
            B = len(xg)
            print(f'warm starts ({"device" if on_dev else "host"} SQP): {good.sum()} of {len(good)} Halton starts accepted by checkGuess after '
                  f'<= {pg.nlp_max_iter} SQP iterations ({time.perf_counter() - t0:.2f} s); running {B} instances', flush=True)
        if not until and os.environ.get('SMPC_WARM_STATS', '0') == '1':
            hist = []
            t0 = time.perf_counter()
            cl.generate_guess(pg, 'htwa', len(good), on_device=on_dev, history=hist)
            dt = time.perf_counter() - t0
            # trial passes of an iteration: the position of the smallest accepted step length on the ladder 1, 0.7, .., 0.05
            passes = [1 + int(np.ceil(np.log(h['alpha'][h['updated']].min()) / np.log(0.7) - 1e-9)) if h['updated'].any() else 1 for h in hist]
            print(f'  with a history: {len(hist)} SQP iterations in {dt:.2f} s = {1e3 * dt / len(hist):.2f} ms per iteration, '
                  f'mean trial passes per iteration {np.mean(np.minimum(passes, 10)):.2f}, '
                  f'instances updated per iteration {np.mean([h["updated"].sum() for h in hist]):.0f}', flush=True)
    scenes = None
    if 'SMPC_SCENE_JITTER' in os.environ:
        from safe_mpc_amd.problem import jittered_scenes
        scenes = jittered_scenes(prob, B, float(os.environ['SMPC_SCENE_JITTER']), int(os.environ.get('SMPC_SCENE_SEED', '0')))
    if 'SMPC_SCENE_VELOCITY' in os.environ:
        from safe_mpc_amd.problem import moving_scenes
        scenes = moving_scenes(prob, B, steps + 1 + N, float(os.environ['SMPC_SCENE_VELOCITY']), int(os.environ.get('SMPC_SCENE_SEED', '0')),
                               sigma=float(os.environ.get('SMPC_SCENE_JITTER', '0')))
    for name in names:
        for dev in (True, False):
            if not dev and os.environ.get('SMPC_HOST', '0') != '1':
                continue
            tm = {}
            t0 = time.perf_counter()
            res = cl.run_mpc(par, name, xg, ug, n_steps=steps, on_device=dev, timing=tm,
                             groups=int(os.environ['SMPC_GROUPS']) if 'SMPC_GROUPS' in os.environ else None,
                             graphs=os.environ.get('SMPC_GRAPHS', '1') != '0', scenes=scenes)
            print(f"{name:12s} {'device' if dev else 'host  '} state{' (warm starts)' if warm else ''}{'' if scenes is None else (' (a scene per instance)' if scenes.ndim == 3 else f' (a track of {scenes.shape[1]} scenes per instance)')}: {tm['ms_per_step']:.3f} ms/step over {tm['steps']} steps "
                  f"(B={B}, N={N}, groups {tm.get('groups')}; total {time.perf_counter() - t0:.1f} s incl. set-up) | collisions {len(res['collisions_idx'])} "
                  f"viable {len(res['viable_idx'])} converged {len(res['conv_idx'])} unconverged {len(res['unconv_idx'])} abort events {len(res['x_viable'])}", flush=True)


if __name__ == '__main__':
    main()
