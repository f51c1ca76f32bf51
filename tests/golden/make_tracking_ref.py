#!/usr/bin/env python3
"""Generator of tests/golden/tracking_ref.npz: the two curve generators of the reference, run on a small parameter object.

Run once by hand where a checkout of the reference is at hand; never imported by a test:

    python tests/golden/make_tracking_ref.py /path/to/reference

Nothing of the reference's text is kept here.  At run time the script parses ``src/safe_mpc/cost_definition.py`` and
``src/safe_mpc/utils.py`` with ``ast``, picks the function definitions it needs BY NAME, drops the function-local
``from .utils import ...`` (which cannot resolve outside the package) and executes them with only ``np`` and ``sym`` in scope.
The file it writes holds data only: the inputs and the ``[3, 71]`` outputs for both curves and both ``vel_const`` settings.
It also evaluates safe_mpc_amd/tracking.py on the same inputs and prints the largest absolute difference.
"""
import ast
import os
import sys
import types

import numpy as np
import sympy as sym

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

WANTED = {'cost_definition.py': ('generate_8shape_trajectory', 'generate_moving_circle_trajectory'),
          'utils.py': ('rot_mat_x', 'rot_mat_y', 'rot_mat_z')}


def load_functions(ref_root):
    scope = {'np': np, 'sym': sym}
    for fname, names in WANTED.items():
        path = os.path.join(ref_root, 'src', 'safe_mpc', fname)
        tree = ast.parse(open(path).read(), path)
        picked = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
        if sorted(n.name for n in picked) != sorted(names):
            raise SystemExit(f'{path}: expected the functions {names}')
        for fn in picked:
            fn.body = [st for st in fn.body if not (isinstance(st, ast.ImportFrom) and st.level > 0)]
        exec(compile(ast.Module(body=picked, type_ignores=[]), path, 'exec'), scope)
    return scope


def small_params(vel_const):
    """the shipped curve keys (config.yaml) on a run of 60 steps with a horizon of 10"""
    import yaml
    cfg = yaml.safe_load(open(os.path.join(ROOT, 'config.yaml')))
    p = types.SimpleNamespace(n_steps_tracking=60, n_steps=60, N=10, dt=float(cfg['dt']), vel_const=bool(vel_const))
    for k in ('dim_shape_8', 'vel_max_traj', 'acc_time', 'circle_rad', 'circle_traj_vel', 'circle_center_vel'):
        setattr(p, k, float(cfg[k]))
    for k in ('offset_traj', 'theta_rot_traj', 'circle_offset_traj'):
        setattr(p, k, np.array(cfg[k], float))
    return p


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    ref = load_functions(sys.argv[1])
    from safe_mpc_amd.tracking import lemniscate_trajectory, moving_circle_trajectory
    out, worst = {}, 0.0
    for vc in (True, False):
        p = small_params(vc)
        tag = 'const' if vc else 'ramp'
        for name, theirs, ours in (('eight', ref['generate_8shape_trajectory'], lemniscate_trajectory),
                                   ('circle', ref['generate_moving_circle_trajectory'], moving_circle_trajectory)):
            a = np.asarray(theirs(p), float)
            d = float(np.abs(a - ours(p)).max())
            print(f'{name:7s} vel_const={vc!s:5s} shape {a.shape}  max |reference - tracking.py| = {d:.3e}')
            worst = max(worst, d)
            out[f'{name}_{tag}'] = a
    p = small_params(True)
    for k, v in vars(p).items():
        if k != 'vel_const':
            out[f'in_{k}'] = np.asarray(v)
    np.savez(os.path.join(HERE, 'tracking_ref.npz'), **out)
    print(f'largest absolute difference: {worst:.3e}')


if __name__ == '__main__':
    main()
