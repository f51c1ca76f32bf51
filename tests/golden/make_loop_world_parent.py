#!/usr/bin/env python3
"""Recipe of tests/golden/loop_world_parent.npz: what ``run_mpc`` computes and what it hands to its two solver handles when scenes,
forecast, observed track and row margin come TOGETHER, recorded at the commit before the closed loop got one owner for what a run
sets on its handles.  tests/test_loop_world_host.py and tests/test_loop_world_gpu.py hold the code of today against it, bit for bit.
The pattern is that of make_policy_layer_parent.py.  Run at that commit (every name used here exists there):

    python tests/golden/make_loop_world_parent.py                        the host cases (recording double on the CPU oracle)
    python tests/golden/make_loop_world_parent.py --device [--margin a b]   the device case (needs the GPU); keeps the host ones

``--out FILE`` writes somewhere else than next to this script; what the file next to this script already holds is kept.

The cases are defined here once; the two tests import :func:`run_host` / :func:`run_device` and the packers from this file.

* host (``h_<case>_*``): the set-up of test_forecast_host.py (``_loop_setup``, 'htwa', B = 5, 7 steps, scripted failures that make
  instances 1 and 3 abort at step N - 1; the world holds one scene per instance in all its columns and the observed track another)
  around its recording double.  ``all``: ``scenes=world, forecast='fit', forecast_window=3, forecast_degree=2, observed=...,
  row_margin=(a, b), score=True``; ``scenes``: nothing but ``scenes=world``.  The double is test_forecast_poly_host.PolyRecorder --
  test_forecast_host.Recorder with the calls a host loop must not make written down and a parabola through three equal columns
  served as the scene it is within rounding of, which degree 2 needs -- with ``set_instance_row_bounds`` written down as
  test_row_bounds_host.py does.  Recorded per case: the result (:func:`pack`) and, for the controller's and the backup's handle,
  the event list (:func:`pack_events`): names, clocks and counts as text, a clock cell by its presence, arrays by their bytes.
* device (``d_*``): ``run_mpc(on_device=True, groups=1)`` on test_forecast_fit_gpu.py::_loop_case ('htwa', B = 5, N = 8, 12 steps,
  back_hor 8) with ``forecast='fit', forecast_window=4, observed=..., score=True`` and a row margin, which the file keeps as
  ``d_row_margin``.  Recorded twice, each time in a process of its own, with graph replay and with eager launches; the file is
  written only if all four recordings are equal to the bit.

Every recorded case must contain an abort event (asserted: ``x_viable`` is not empty), so that the backup handle's path has run.
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

GOLDEN = os.path.join(HERE, 'loop_world_parent.npz')
ARRAYS = ('x', 'u', 'r_receding', 'x_viable', 'scenes')
LISTS = ('conv_idx', 'collisions_idx', 'viable_idx', 'unconv_idx')
HOST_CASES = ('all', 'scenes')
HANDLES = ('htwa', 'backup')
HOST_MARGIN = (0.004, 0.003)            # (test_row_bounds_host.py's)
DEVICE_MARGIN = (0.004, 0.003)          # the first margin tried on the GPU; the file says which one was recorded


def pack(prefix, res):
    """the compared part of a run_mpc result as arrays ``<prefix>_<key>`` (lists as int64, in the order run_mpc returns them; the
    scores of a scored run; the keys a forecast and a row margin add, as text)"""
    out = {f'{prefix}_{k}': np.ascontiguousarray(res[k]) for k in ARRAYS}
    out.update({f'{prefix}_{k}': np.asarray(res[k], np.int64).reshape(-1) for k in LISTS})
    out.update({f'{prefix}_score_{k}': np.ascontiguousarray(v) for k, v in res.get('score', {}).items()})
    said = {k: res[k] for k in ('forecast', 'observed', 'forecast_window', 'forecast_degree', 'row_margin') if k in res}
    out[f'{prefix}_keys'] = np.array([f'{k}={v!r}' for k, v in sorted(said.items())], dtype=np.str_)
    return out


def pack_events(prefix, events):
    """the event list of a recording double as ``<prefix>_events`` (one line of text per event: its name, then every value -- an
    array as its dtype and shape, a clock cell as 'cell', anything else by repr) and ``<prefix>_bytes`` (the arrays' bytes, in order)"""
    lines, blob = [], []
    for e in events:
        words = [e[0]]
        for v in e[1:]:
            if isinstance(v, np.ndarray) and v.dtype == np.int64 and v.shape == (1,):
                words.append('cell')                         # (each run makes its own: compared by presence, as _same_events does)
            elif isinstance(v, np.ndarray):
                words.append(f'{v.dtype}{list(v.shape)}')
                blob.append(np.ascontiguousarray(v).tobytes())
            else:
                words.append(repr(v))
        lines.append(' '.join(words))
    return {f'{prefix}_events': np.array(lines, dtype=np.str_), f'{prefix}_bytes': np.frombuffer(b''.join(blob), np.uint8)}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype.kind == 'U' and b.dtype.kind == 'U':
        return a.shape == b.shape and a.tolist() == b.tolist()
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def run_host(case):
    """``(result, {handle: events})`` of the host case ``case``"""
    import track_cases as tc
    from conftest import sample_instances
    from safe_mpc_amd import closed_loop as cl
    from test_forecast_host import LOOP_N, _loop_setup
    from test_forecast_poly_host import PolyRecorder

    class WorldRecorder(PolyRecorder):
        def set_instance_row_bounds(self, lo=None, hi=None):
            self.events.append(('row_bounds', None if lo is None else np.array(lo), None if hi is None else np.array(hi)))

    N, B, steps, T = LOOP_N, 5, 7, 4
    pars, base, geoms = _loop_setup()
    world = np.ascontiguousarray(np.repeat(geoms[np.array([0, 1, 0, 1, 1])][:, None], T, axis=1))
    observed = np.ascontiguousarray(np.repeat(geoms[np.array([1, 0, 1, 0, 0])][:, None], T, axis=1))
    x0 = sample_instances(base, B, seed=5, vel_scale=0.1)
    xg, ug = np.repeat(x0[:, None, :], N + 1, axis=1), np.zeros((B, N, 6))
    fail = np.array([0, 4, 0, 4, 0], np.int32)
    solvers = {}
    mk, mkb = tc.oracle_factories(pars[0], N, pars, geoms, log=solvers, solver_cls=WorldRecorder)

    def mk_scripted(name, batch):
        ctrl = mk(name, batch)
        ctrl.ocp_solver.scripted_status = [fail.copy() for _ in range(N)] + [np.zeros(B, np.int32)] * 8
        return ctrl
    kw = {'all': dict(forecast='fit', forecast_window=3, forecast_degree=2, observed=observed, row_margin=HOST_MARGIN, score=True),
          'scenes': {}}[case]
    res = cl.run_mpc(pars[0], 'htwa', xg, ug, make_controller=mk_scripted, make_backup=mkb, n_steps=steps, scenes=world, **kw)
    return res, {name: solvers[name].events for name in HANDLES}


def pack_host(case):
    res, events = run_host(case)
    out = pack(f'h_{case}', res)
    for name in HANDLES:
        out.update(pack_events(f'h_{case}_{name}', events[name]))
    return out


def run_device(graphs, margin):
    from safe_mpc_amd import closed_loop as cl
    from test_forecast_fit_gpu import _loop_case
    par, xg, ug, world, observed, steps = _loop_case()
    return cl.run_mpc(par, 'htwa', xg, ug, on_device=True, groups=1, graphs=graphs, n_steps=steps, scenes=world, forecast='fit',
                      forecast_window=4, observed=observed, score=True, row_margin=tuple(float(v) for v in margin))


def _record_device_child(out, margin):
    rec = {}
    for graphs in (True, False):
        rec.update(pack('d' if graphs else 'eager', run_device(graphs, margin)))
    np.savez(out, **rec)


def _record_device(margin):
    runs = []
    with tempfile.TemporaryDirectory() as tmp:
        for k in range(2):
            f = os.path.join(tmp, f'{k}.npz')
            # a process of its own per recording; one that fails ends the recipe (nothing more is started on the GPU)
            subprocess.run([sys.executable, os.path.abspath(__file__), '--device-child', f, str(margin[0]), str(margin[1])],
                           check=True, timeout=300)
            with np.load(f) as z:
                runs.append({key: z[key] for key in z.files})
    first = {key: v for key, v in runs[0].items() if key.startswith('d_')}
    print(f'device, row_margin {margin}: {len(first["d_x_viable"])} abort events, {len(first["d_collisions_idx"])} collisions', flush=True)
    differ = [key for key in runs[0] if not same_bits(runs[0][key], runs[1][key])]
    differ += [key for key in first if not same_bits(first[key], runs[0]['eager_' + key[2:]])]
    if differ:
        raise SystemExit(f'the recordings differ in {sorted(set(differ))}: the parent is not reproducible to the bit, nothing written')
    assert len(first['d_x_viable']) >= 1, 'no abort event in the recorded case: try another --margin'
    first['d_row_margin'] = np.array(margin, np.float64)
    return first


def main():
    argv = sys.argv[1:]
    if argv[:1] == ['--device-child']:
        return _record_device_child(argv[1], (float(argv[2]), float(argv[3])))
    out = argv[argv.index('--out') + 1] if '--out' in argv else GOLDEN
    rec = {}
    if os.path.exists(GOLDEN):
        with np.load(GOLDEN) as z:
            rec = {key: z[key] for key in z.files}
    if '--device' in argv:
        k = argv.index('--margin') if '--margin' in argv else None
        rec.update(_record_device(DEVICE_MARGIN if k is None else (float(argv[k + 1]), float(argv[k + 2]))))
    else:
        for case in HOST_CASES:
            a, b = pack_host(case), pack_host(case)
            assert all(same_bits(a[key], b[key]) for key in a), f'{case}: two host runs differ'
            assert len(a[f'h_{case}_x_viable']) >= 1, f'{case}: no abort event in the recorded case'
            print(f'{case}: {len(a[f"h_{case}_x_viable"])} abort events, {len(a[f"h_{case}_collisions_idx"])} collisions, '
                  + ', '.join(f'{len(a[f"h_{case}_{name}_events"])} events on {name}' for name in HANDLES))
            rec.update(a)
    np.savez_compressed(out, **rec)
    print(f'{out}: {len(rec)} arrays, {os.path.getsize(out)} bytes')


if __name__ == '__main__':
    main()
