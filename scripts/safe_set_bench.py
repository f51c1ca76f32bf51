#!/usr/bin/env python3
"""The measurement of profiles/safe_set_data.txt: rays labelled per second at B rays in flight on the backup
OCP at N = back_hor, bisect = 8, budget 30, a look every 5 iterations -- with the bookkeeping on the device (smpc_ray_update and a
4-byte read per round) against the statement-driven loop on the same engine (host decisions by ray_update_statement; the engine's
host-pointer path carries the arrays), alternating the two in one session, wall clock around a synchronise.  Also the time inside
smpc_ray_update (events on the engine's stream) and inside ray_update_statement (host clock), and the share of rays per kind.

    python scripts/safe_set_bench.py [output file] [--rays 4096] [--reps 2]

SMPC_CONTEXT=1 measures something else with the same tools (profiles/safe_set_context.txt): what the feature
stage of the network pass costs with a four-number instance context against a network without context columns.  The forward-only
pass of smpc_check_trajectory(nn_ok) over --rays instances x 1 node (4096 rows: k_mlp_fused) and x 30 nodes (122 880 rows:
k_mlp_wave), the two networks alternating on one handle, wall clock around a synchronise over 50 calls each; k_check_nodes and
k_check_nn run in both and are part of both figures.
SMPC_CONTEXT_TRACK=T beside it (profiles/context_tracks.txt): the instance context is a track of T time
columns (smpc_set_instance_context_track) read through a scene clock cell that holds 3, so every row looks its column up.
"""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from safe_mpc_amd import safe_set_data as sd
from safe_mpc_amd.controller import SafeBackupController
from safe_mpc_amd.parser import Parameters
from safe_mpc_amd.solver import BatchedOcpSolver

args = sys.argv[1:]
def opt(flag, default):
    if flag in args:
        i = args.index(flag)
        v = int(args[i + 1])
        del args[i:i + 2]
        return v
    return default
B, REPS = opt('--rays', 4096), opt('--reps', 2)
OUT = open(args[0], 'w') if args else open(os.devnull, 'w')
def say(*a):
    line = ' '.join(str(x) for x in a)
    print(line, flush=True)
    OUT.write(line + '\n'); OUT.flush()

par = Parameters({}, 'z1', rti=False)
par.nq, par.n_dof_safe_set, par.net_size = 6, 6, [12, 256, 1]

def context_bench():
    from safe_mpc_amd.problem import OcpProblem
    from safe_mpc_amd.safe_set import SafeSetNet
    prob = OcpProblem(par, 'st', 'ext', N=30)
    net = SafeSetNet.synthetic([16, 256, 1], 6, prob.x_min, prob.x_max, 0, par.act)
    prob.set_normalisation(net.mean, net.std)
    plain = net.folded(np.zeros(4))
    sv = BatchedOcpSolver(prob, None)
    dev = torch.device('cuda', sv.device)
    rng = np.random.default_rng(0)
    ctx = torch.as_tensor(rng.standard_normal((B, 4)), device=dev)
    T = int(os.environ.get('SMPC_CONTEXT_TRACK', '1'))
    if T > 1:
        ctx = torch.as_tensor(rng.standard_normal((B, T, 4)), device=dev)
        cell = torch.full((1,), 3, dtype=torch.int64, device=dev)
        sv.set_scene_clock(cell)
    set_ctx = sv.set_instance_context_track if T > 1 else sv.set_instance_context
    CALLS = 50
    say(f'# SMPC_CONTEXT=1 python scripts/safe_set_bench.py -- the forward-only network pass of smpc_check_trajectory(nn_ok), {B} instances, a '
        f'four-number instance context against a network without context columns; one MI355X, one session, {CALLS} calls per figure')
    if T > 1:
        say(f'# SMPC_CONTEXT_TRACK={T}: the context is a track of {T} time columns, the scene clock cell holds 3')
    for n_nodes in (1, 30):
        x = torch.as_tensor(prob.x_min + rng.uniform(size=(B, n_nodes, 12)) * (prob.x_max - prob.x_min), device=dev)
        times = {'none': [], 'context': []}
        for rep in range(REPS + 1):                 # (the first round warms both up and is not reported)
            for mode in ('none', 'context'):
                sv.set_mlp(plain if mode == 'none' else net)
                if mode == 'context':
                    set_ctx(ctx)
                sv.check_trajectory(x, want_nn=True)
                sv.sync(); torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(CALLS):
                    sv.check_trajectory(x, want_nn=True)
                sv.sync(); torch.cuda.synchronize()
                if rep:
                    times[mode].append((time.perf_counter() - t0) / CALLS * 1e6)
        for mode in ('none', 'context'):
            say(f'{B * n_nodes:7d} rows ({"k_mlp_fused" if B * n_nodes < 8192 else "k_mlp_wave"}), {mode:7s}: '
                f'{min(times[mode]):8.1f} us per call best of {REPS}; all {[round(t, 1) for t in times[mode]]}')
    OUT.close()

if os.environ.get('SMPC_CONTEXT') == '1':
    context_bench()
    sys.exit(0)

BISECT, BUDGET, EVERY = 8, 30, 5
ctrl = SafeBackupController(par, B)
sv = ctrl.ocp_solver
sv.set_qp_mode('throughput')
N = ctrl.N
say(f'# python scripts/safe_set_bench.py -- safe-set ray labelling; Z1-class arm, backup OCP, N = back_hor = {N}, {B} rays in flight, bisect = {BISECT}, '
    f'budget {BUDGET}, a look every {EVERY} SQP iterations; one MI355X, one session')
q, d, s_hi = sd.sample_rays(ctrl.problem, B, 0, solver=sv)

_upd, _stmt = BatchedOcpSolver.ray_update, sd.ray_update_statement
spent = {'events': [], 'host': 0.0}
def upd_timed(self, *a, **k):
    # (events on the engine's stream, recorded from outside it: the call keeps ordering its stream against torch's current one.  The
    #  engine's stream is ordered behind torch's BEFORE the start event, so the interval holds the call's own work only)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    self._ext_stream.wait_stream(torch.cuda.current_stream(self.device))
    e0.record(self._ext_stream)
    r = _upd(self, *a, **k)
    e1.record(self._ext_stream)
    spent['events'].append((e0, e1))
    return r
def stmt_timed(*a, **k):
    t1 = time.perf_counter()
    r = _stmt(*a, **k)
    spent['host'] += time.perf_counter() - t1
    return r
BatchedOcpSolver.ray_update, sd.ray_update_statement = upd_timed, stmt_timed

def run(mode):
    spent['events'], spent['host'] = [], 0.0
    sv.sync(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = sd.label_rays(ctrl, q, d, s_hi, bisect=BISECT, budget=BUDGET, check_every=EVERY, bookkeeping=mode)
    sv.sync(); torch.cuda.synchronize()
    w = time.perf_counter() - t0
    book = sum(a.elapsed_time(b) for a, b in spent['events']) * 1e-3 if mode == 'device' else spent['host']
    return res, w, book

results = {}
for rep in range(REPS):
    for mode in ('device', 'statement'):
        res, w, book = run(mode)
        results.setdefault(mode, []).append((w, book, res))
        say(f'run {rep} {mode:9s}: {w:7.2f} s wall, {B / w:8.1f} rays/s, {res["rounds"]} rounds, {int(res["iters"].sum())} instance-iterations, '
            f'bookkeeping {book * 1e3:9.2f} ms in all ({book * 1e3 / res["rounds"]:.3f} ms per round)')
a, b = results['device'][-1][2], results['statement'][-1][2]
same = all(np.array_equal(a[k], b[k], equal_nan=True) for k in ('label', 'kind', 'trials', 'iters', 'x_cert', 'u_cert'))
say(f'device and statement-driven results identical bit for bit: {same}')
for mode in ('device', 'statement'):
    ws = [w for w, _, _ in results[mode]]
    say(f'{mode:9s}: best of {REPS}: {B / min(ws):.1f} rays/s; all runs {[round(B / w, 1) for w in ws]}')
kind = a['kind']
say('share of rays per kind: ' + ', '.join(f'{sd.KIND_NAMES[k]} {100.0 * (kind == k).mean():.1f} %' for k in (sd.DEAD, sd.BRACKETED, sd.SATURATED)))
lab = a['label'][kind != sd.DEAD]
say(f'labels of the rays that are not dead: min {lab.min():.3f}, median {np.median(lab):.3f}, max {lab.max():.3f} rad/s; trials per ray mean {a["trials"].mean():.2f}')
OUT.close()
