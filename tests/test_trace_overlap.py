"""scripts/trace_overlap.py on hand-made traces (no GPU), and the engine's refusal of an unknown SMPC_STREAM_PRIORITY (no GPU either:
smpc_create checks the switch before it looks for a device)."""
import importlib.util
import os
import subprocess
import sys

from conftest import ROOT

spec = importlib.util.spec_from_file_location('trace_overlap', os.path.join(ROOT, 'scripts', 'trace_overlap.py'))
trace_overlap = importlib.util.module_from_spec(spec)
spec.loader.exec_module(trace_overlap)

QP = 'void smpc::k_qp_ipm<6, 6, false>(smpc::QpArgs)'


def _row(disp, queue, start, end, name=QP, stream=None):
    r = {'Kernel_Name': name, 'Dispatch_Id': str(disp), 'Queue_Id': str(queue), 'Start_Timestamp': str(start), 'End_Timestamp': str(end)}
    if stream is not None:
        r['Stream_Id'] = str(stream)
    return r


def _trace(starts, queues, steps=4, length=1000, period=None, streams=None):
    """`steps` steps of three sub-batches; sub-batch i starts `starts[i]` into the step's period and runs `length`"""
    period = period or max(starts) + length
    rows, d = [], 0
    for k in range(steps):
        for i in range(3):
            d += 1
            rows.append(_row(d, queues[i], k * period + starts[i], k * period + starts[i] + length, stream=None if streams is None else streams[i]))
            d += 1
            rows.append(_row(d, queues[i], k * period + starts[i] + length, k * period + starts[i] + length + 10, name='void smpc::k_plant_step<6>(int)'))
    return rows


def test_two_sub_batches_on_one_queue_take_turns():
    out = trace_overlap.report(_trace([0, 0, 1000], [1, 2, 2]), warmup=1, steps=2)
    print(out)
    assert '3 sub-batches told apart by dispatch order; launches 1..2' in out
    assert 'distinct queues: 2 of 3' in out
    assert 'sub-batches 0 and 1: 100.0 %' in out
    assert 'sub-batches 1 and 2:   0.0 %   (same queue)' in out
    assert 'sub-batches 0 and 2:   0.0 %' in out
    # per period of 2000: two in flight for 1000, one for 1000
    assert '  0:   0.0 %' in out and '  1:  50.0 %' in out and '  2:  50.0 %' in out and '  3:   0.0 %' in out


def test_three_queues_side_by_side_by_stream_id():
    # the stream ids tell the sub-batches apart even when the dispatch ids do not come round robin
    rows = _trace([0, 100, 200], [5, 6, 7], streams=[11, 12, 13])
    rows[0]['Dispatch_Id'], rows[2]['Dispatch_Id'] = rows[2]['Dispatch_Id'], rows[0]['Dispatch_Id']
    rows.append(_row(1000, 9, 0, 5000, stream=99))       # a fourth stream's one launch of the same kernel (a probe) is no sub-batch
    out = trace_overlap.report(rows, warmup=0, steps=4)
    print(out)
    assert 'told apart by Stream_Id' in out
    assert 'distinct queues: 3 of 3' in out
    # (sub-batch 0 is now the stream that starts 100 into the period, 1 the one that starts it, 2 the one 200 in)
    assert 'sub-batches 0 and 1:  90.0 %' in out and 'sub-batches 0 and 2:  90.0 %' in out and 'sub-batches 1 and 2:  80.0 %' in out
    # a period of 1200: 0-100 one, 100-200 two, 200-1000 three, 1000-1100 two, 1100-1200 one
    assert '  3:  66.7 %' in out and '  2:  16.7 %' in out and '  1:  16.7 %' in out


def test_too_short_a_trace_says_so():
    assert 'no timed step' in trace_overlap.report(_trace([0, 0, 0], [1, 2, 3], steps=2), warmup=10, steps=100)


def test_unknown_stream_priority_is_refused():
    code = ('import ctypes, sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n'
            'from conftest import make_problem\n'
            'from safe_mpc_amd import _lib\n'
            'L = _lib.lib(); h = ctypes.c_void_p()\n'
            'rc = L.smpc_create(ctypes.byref(make_problem("st")[1].desc), 0, ctypes.byref(h))\n'
            'print(rc, L.smpc_last_error(None).decode())\n' % (ROOT, os.path.join(ROOT, 'tests')))
    res = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, SMPC_STREAM_PRIORITY='urgent'), capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    rc, msg = res.stdout.strip().split(' ', 1)
    assert int(rc) != 0
    assert 'SMPC_STREAM_PRIORITY=urgent' in msg and 'default, high or low' in msg
