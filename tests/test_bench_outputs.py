"""bench.py's plain run and --dump-outputs: a run without --full prints the headline only, and --dump-outputs writes what the
last timed step computed, from inputs that are the same for the same arguments (two builds can be compared file by file).
bench.py runs as a child process: it starts its own GPU context, and importing it sets a HIP environment default."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = {'roofline', 'cpu_baseline', 'survey_window', 'latency_b1_ms', 'strong_proxy'}


def test_dump_outputs_writes_a_fixed_sample_under_its_cap(tmp_path):
    """Above the cap the same seeded sample of instances is written every time, rows kept with their instance, all of it
    under the cap; below it every row is written."""
    code = f"""
import sys
import numpy as np
sys.path.insert(0, {ROOT!r})
import bench
B = 1000
ids = np.arange(B)
big = np.arange(B * 50, dtype=np.float64).reshape(B, 50)
named = {{'a': (ids, big), 'b': (ids[600:], np.arange(400, dtype=np.int32) + 600)}}
bench.dump_outputs(sys.argv[1] + '/whole', named, B)
bench.dump_outputs(sys.argv[1] + '/s1', named, B, cap=100000)
bench.dump_outputs(sys.argv[1] + '/s2', named, B, cap=100000)
"""
    subprocess.run([sys.executable, '-c', code, str(tmp_path)], check=True, cwd=str(tmp_path))
    whole = {f: np.load(tmp_path / 'whole' / f) for f in os.listdir(tmp_path / 'whole')}
    assert set(whole) == {'a.npy', 'b.npy'} and whole['a.npy'].shape == (1000, 50) and whole['b.npy'].dtype == np.float64
    s1 = {f: np.load(tmp_path / 's1' / f) for f in os.listdir(tmp_path / 's1')}
    s2 = {f: np.load(tmp_path / 's2' / f) for f in os.listdir(tmp_path / 's2')}
    assert set(s1) == {'a.npy', 'b.npy', 'instance_index.npy'}
    keep = s1['instance_index.npy'].astype(np.int64)
    assert 0 < len(keep) < 1000 and np.all(np.diff(keep) > 0)
    assert sum(a.nbytes for a in s1.values()) <= 100000
    np.testing.assert_array_equal(s1['a.npy'], whole['a.npy'][keep])
    np.testing.assert_array_equal(s1['b.npy'], keep[keep >= 600])
    for f in s1:
        np.testing.assert_array_equal(s1[f], s2[f])


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_its_last_step(tmp_path):
    runs = []
    for k in range(2):
        out = tmp_path / f'run{k}'
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--batch', '96', '--streams', '2',
                            '--steps', '4', '--warmup', '2', '--dump-outputs', str(out)],
                           capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [l for l in r.stdout.splitlines() if l.strip()]
        assert len(lines) == 1, r.stdout[-2000:]
        d = json.loads(lines[0])
        assert d['steps'] == 4 and d['warmup'] == 2 and d['ms_per_step'] > 0 and d['value'] > 0
        assert d['unit'] == 'instance-steps/s' and d['higher_is_better'] is True and d['dtype'] == 'f64'
        assert d['config']['batch_per_gpu'] == 96 and d['config']['streams_per_gpu'] == 2 and d['config']['failed_instance_steps'] == 0
        assert not FULL_ONLY & set(d), FULL_ONLY & set(d)
        files = {f[:-4]: np.load(out / f) for f in os.listdir(out)}
        shapes = {'u': (96, 6), 'x': (96, 12), 'status': (96,), 'ipm_iterations': (96,), 'x_guess': (96, 31, 12), 'u_guess': (96, 30, 6)}
        assert {k_: a.shape for k_, a in files.items()} == shapes
        assert all(a.dtype == np.float64 and np.isfinite(a).all() for a in files.values())
        assert (files['status'] == 0).all() and (files['ipm_iterations'] > 0).all()
        runs.append(files)
    # the same arguments: the same inputs, so the same outputs
    for k_ in runs[0]:
        np.testing.assert_allclose(runs[1][k_], runs[0][k_], rtol=1e-9, atol=1e-12, err_msg=k_)
