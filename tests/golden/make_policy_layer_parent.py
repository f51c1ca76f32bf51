#!/usr/bin/env python3
"""Recipe of tests/golden/policy_layer_parent.npz: results of ``run_mpc`` recorded at the commit BEFORE the policy layer was
split into its host and device paths, which tests/test_policy_layer_host.py and tests/test_policy_layer_gpu.py hold the
split code against, bit for bit.  Run at that commit (every name used here exists there):

    python tests/golden/make_policy_layer_parent.py                  the host cases (CPU double, scripted statuses)
    python tests/golden/make_policy_layer_parent.py --device         the device cases (needs the GPU); keeps the host ones

``--out FILE`` writes somewhere else than next to this script; what the file next to this script already holds is kept.

The cases are defined here once; the two tests import :func:`run_host` / :func:`run_device` / :func:`pack` from this file.

* host (``h_<kind>_*``): ``run_mpc`` through the scripted mirror of tests/test_policy_oracle.py (``_run_mirror`` with
  ``_status_matrix``, its ``_params()``: N = 5, Nb = 4; B = 6, 44 steps) for htwa, receding and real_receding.
* device (``d_<name>_*``): ``run_mpc(on_device=True, groups=1)``; receding and real_receding on the fixture of
  test_gpu_parity.py::test_device_policy_loop_equals_scalar_oracle_loop (Z1, nq = 6, net [12, 256, 1], N = 10, back_hor = 12,
  B = 40, 30 steps, control_noise = 1.0, starts sample_instances(prob, 40, seed=9, vel_scale=0.3)), parallel on the fixture of
  test_parallel_gpu.py::test_closed_loop_on_device_equals_host_loop.  Every case is recorded twice, each time in a process
  of its own, with graph replay and with eager launches; the file is written only if all four recordings of a case are
  equal to the bit.

Every recorded host case, and the device case 'receding', must contain at least one abort event (asserted).  The fixtures of the
other two device cases are fixed by the tests they come from; their event counts are printed (none in either: the host cases
cover their abort branches).
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for _p in (ROOT, os.path.join(ROOT, 'tests')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

GOLDEN = os.path.join(HERE, 'policy_layer_parent.npz')
ARRAYS = ('x', 'u', 'r_receding', 'x_viable')
LISTS = ('conv_idx', 'collisions_idx', 'viable_idx', 'unconv_idx')
HOST_CASES = ('htwa', 'receding', 'real_receding')
DEVICE_CASES = ('receding', 'real_receding', 'parallel')


def pack(prefix, res):
    """the compared part of a run_mpc result as arrays ``<prefix>_<key>`` (lists as int64, in the order run_mpc returns them)"""
    out = {f'{prefix}_{k}': np.ascontiguousarray(res[k]) for k in ARRAYS}
    out.update({f'{prefix}_{k}': np.asarray(res[k], np.int64).reshape(-1) for k in LISTS})
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def run_host(kind):
    """the set-up of test_policy_oracle.py::test_numpy_mirror_equals_scalar_oracle_closed_loop for ``kind``"""
    import test_policy_oracle as tpo
    from conftest import sample_instances
    from fake_solver import make_double_controller
    N, Nb, B, n_steps = 5, 4, 6, 44
    par = tpo._params(N, Nb, True)
    probe = make_double_controller(kind, par, 1)
    x0 = sample_instances(probe.problem, B, seed=5, vel_scale=0.05)
    xg, ug = np.repeat(x0[:, None, :], N + 1, axis=1), np.zeros((B, N, 6))
    matrix = tpo._status_matrix(kind, n_steps, B, N)
    x3 = float(x0[3, 0])
    backup_rule = lambda xv, x3=x3: (4 if abs(xv[0] - x3) < 0.3 else None)      # instance 3: its backup OCP fails
    res, _ = tpo._run_mirror(par, kind, xg, ug, n_steps, matrix, backup_rule, kind in ('receding', 'real_receding'))
    return res


def run_device(name, graphs=True):
    from conftest import sample_instances
    from safe_mpc_amd import closed_loop as cl
    from safe_mpc_amd import controller as C
    from safe_mpc_amd.parser import Parameters
    par = Parameters({}, 'z1')
    if name == 'parallel':
        N, Nb, B, n_steps, seed, vel = 8, 10, 16, 16, 9, 0.35
    else:
        N, Nb, B, n_steps, seed, vel = 10, 12, 40, 30, 9, 0.3
    par.nq, par.n_dof_safe_set, par.net_size, par.N, par.back_hor = 6, 6, [12, 256, 1], N, Nb
    x0 = sample_instances(C.OcpProblem(par, 'htwa', 'ext', N=N), B, seed=seed, vel_scale=vel)
    xg, ug = np.repeat(x0[:, None, :], N + 1, axis=1), np.zeros((B, N, 6))
    return cl.run_mpc(par, name, xg, ug, n_steps=n_steps, control_noise=1.0, on_device=True, groups=1, graphs=graphs)


def _record_device_child(name, out):
    rec = {}
    for graphs in (True, False):
        rec.update(pack(f'd_{name}' if graphs else f'eager_{name}', run_device(name, graphs)))
    np.savez(out, **rec)


def _record_device():
    rec = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name in DEVICE_CASES:
            runs = []
            for k in range(2):
                f = os.path.join(tmp, f'{name}_{k}.npz')
                # a process of its own per recording; one that fails ends the recipe (nothing more is started on the GPU)
                subprocess.run([sys.executable, os.path.abspath(__file__), '--device-child', name, f], check=True, timeout=300)
                with np.load(f) as z:
                    runs.append({key: z[key] for key in z.files})
            first = {key: v for key, v in runs[0].items() if key.startswith('d_')}
            n_events = len(first[f'd_{name}_x_viable'])
            print(f'{name}: {n_events} abort events, {len(first[f"d_{name}_collisions_idx"])} collisions', flush=True)
            differ = [key for key in runs[0] if not same_bits(runs[0][key], runs[1][key])]
            differ += [key for key in first if not same_bits(first[key], runs[0]['eager_' + key[2:]])]
            if differ:
                raise SystemExit(f'{name}: the recordings differ in {sorted(set(differ))}: the parent is not reproducible to the bit, '
                                 'nothing written')
            assert n_events >= 1 or name != 'receding', f'{name}: no abort event in the recorded case'
            rec.update(first)
    return rec


def main():
    argv = sys.argv[1:]
    if argv[:1] == ['--device-child']:
        return _record_device_child(argv[1], argv[2])
    out = argv[argv.index('--out') + 1] if '--out' in argv else GOLDEN
    rec = {}
    if os.path.exists(GOLDEN):
        with np.load(GOLDEN) as z:
            rec = {key: z[key] for key in z.files}
    if '--device' in argv:
        rec.update(_record_device())
    else:
        for kind in HOST_CASES:
            a, b = pack(f'h_{kind}', run_host(kind)), pack(f'h_{kind}', run_host(kind))
            assert all(same_bits(a[key], b[key]) for key in a), f'{kind}: two host runs differ'
            assert len(a[f'h_{kind}_x_viable']) >= 1, f'{kind}: no abort event in the recorded case'
            print(f'{kind}: {len(a[f"h_{kind}_x_viable"])} abort events, {len(a[f"h_{kind}_collisions_idx"])} collisions')
            rec.update(a)
    np.savez_compressed(out, **rec)
    print(f'{out}: {len(rec)} arrays, {os.path.getsize(out)} bytes')


if __name__ == '__main__':
    main()
