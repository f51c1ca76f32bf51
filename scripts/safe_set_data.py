#!/usr/bin/env python3
"""Training data of the learned safe set for the robot and scene of config.yaml, and optionally the fitted network:

    python scripts/safe_set_data.py --rays n [--bisect K] [--budget I] [--check-every C] [--batch B] [--seed S]
                                    [--horizon N] [--fit EPOCHS] [--hidden H] [--out PATH]
                                    [--scene-jitter SIGMA --scene-seed S] [--context row:slot,row:slot,...]

Rays (q, d) are sampled in the joint box (collision-free Halton configurations, seeded directions) and labelled on the device by
bisection on the speed along d, every trial one run of the backup OCP (safe_mpc_amd/safe_set_data.py).  Writes
PATH.npz (q, d, s_hi, label, kind, trials; default PATH: <DATA_DIR><system>_safe_set) and, with --fit, PATH.pt: a checkpoint in the
reference's format that ``network_path:`` of config.yaml can name.  --horizon defaults to back_hor.

--scene-jitter gives every ray a scene of its own (problem.jittered_scenes: every obstacle moved by N(0, SIGMA^2) per axis) and labels
it there; --context names the numbers of a scene's 8-double records that the network is fitted on as extra inputs (DESIGN.md section
9j; at most 16 - 2 nq of them), written into the checkpoint with their normalisation and read back from it by
``SafeSetNet.from_params``.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from safe_mpc_amd import safe_set_data as sd                    # noqa: E402
from safe_mpc_amd.controller import SafeBackupController        # noqa: E402
from safe_mpc_amd.parser import Parameters                      # noqa: E402
from safe_mpc_amd.problem import jittered_scenes, scene_context # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--rays', type=int, required=True)
    ap.add_argument('--bisect', type=int, default=8)
    ap.add_argument('--budget', type=int, default=30)
    ap.add_argument('--check-every', type=int, default=5)
    ap.add_argument('--batch', type=int, default=None)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--system', default='z1')
    ap.add_argument('--horizon', type=int, default=None)
    ap.add_argument('--fit', type=int, default=0, metavar='EPOCHS')
    ap.add_argument('--hidden', type=int, default=None)
    ap.add_argument('--out', default=None)
    ap.add_argument('--scene-jitter', type=float, default=0.0, metavar='SIGMA')
    ap.add_argument('--scene-seed', type=int, default=0)
    ap.add_argument('--context', default=None, metavar='ROW:SLOT,...')
    a = ap.parse_args(argv)
    select = [tuple(int(v) for v in pair.split(':')) for pair in a.context.split(',')] if a.context else None
    if select and not a.scene_jitter > 0.0:
        ap.error('--context needs --scene-jitter: in one shared scene the context is a constant')
    params = Parameters({}, a.system, rti=False)
    B = min(a.batch or a.rays, a.rays)
    ctrl = SafeBackupController(params, B, N=a.horizon)
    ctrl.ocp_solver.set_qp_mode('throughput')                   # a ray's label must not depend on the width of its chunk
    q, d, s_hi = sd.sample_rays(ctrl.problem, a.rays, a.seed, solver=ctrl.ocp_solver)
    scenes = jittered_scenes(ctrl.problem, a.rays, a.scene_jitter, a.scene_seed) if a.scene_jitter > 0.0 else None
    ctx = scene_context(scenes, select) if select else None
    t0 = time.time()
    res = sd.label_rays(ctrl, q, d, s_hi, bisect=a.bisect, budget=a.budget, check_every=a.check_every, batch=B, scenes=scenes)
    dt = time.time() - t0
    kinds = {sd.KIND_NAMES[k]: int((res['kind'] == k).sum()) for k in (sd.DEAD, sd.BRACKETED, sd.SATURATED)}
    print(f'{a.rays} rays labelled in {dt:.1f} s ({a.rays / dt:.1f} rays/s), {res["rounds"]} rounds, {int(res["iters"].sum())} '
          f'instance-iterations: {kinds}')
    out = a.out or os.path.join(params.DATA_DIR, f'{a.system}_safe_set')
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    sd.save_dataset(out + '.npz', q, d, s_hi, res, ctx=ctx)
    print(out + '.npz')
    if a.fit > 0:
        data = {'q': q, 'd': d, 'label': res['label'], 'kind': res['kind']}
        if select:
            params.net_size = [2 * ctrl.nq + len(select)] + [int(v) for v in params.net_size[1:]]
        net, mean, std, info = sd.fit_safe_set(data, params, a.fit, a.seed, hidden=a.hidden, context=ctx)
        sd.save_checkpoint(out + '.pt', net, mean, std, info.get('ctx_mean'), info.get('ctx_std'), select)
        print(f'fit on {info["rays"]} rays ({info["dropped"]} dead dropped), network_size {info["net_size"]}, training RMSE '
              f'{info["train_rmse"]:.4f} rad/s')
        print(out + '.pt')
    return 0


if __name__ == '__main__':
    sys.exit(main())
