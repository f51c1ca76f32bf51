#!/usr/bin/env python3
"""The measurements of profiles/guess_until.txt, all in one process on one GPU:

* smpc_check_guess, k_check_guess alone and one smpc_merit_terms pass at B = 4096, N = 30, by HIP events on the handle's stream, and
  the four-call checkGuess on device tensors by wall clock;
* warm-start generation on the bench workload (Z1, N = 30, 4096 Halton starts, htwa, nlp_max_iter 1000): generate_guess(on_device=True)
  and generate_guess_until under 'final' (K = 50) and 'first' (K = 20), each also with batch = 1024 -- wall time, of which the time
  inside solver.sqp / solver.check_guess, instance-iterations, samples issued and accepted, rounds;
* 100 steps of the htwa controller from the guesses: solves with status != 0, and run_mpc's outcome line.

    python scripts/guess_until_bench.py [output file]
"""
import copy, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import bench
from safe_mpc_amd import closed_loop as cl
from safe_mpc_amd.controller import get_controller
from safe_mpc_amd.solver import BatchedOcpSolver

OUT = open(sys.argv[1], 'w') if len(sys.argv) > 1 else open(os.devnull, 'w')
def say(*a):
    line = ' '.join(str(x) for x in a)
    print(line, flush=True)
    OUT.write(line + '\n'); OUT.flush()

par, prob, net = bench.build_problem()
par.back_hor = 30
B = 4096
N = prob.N
say(f'# python scripts/guess_until_bench.py -- warm-start generation until n are accepted; Z1, htwa, N = {N}, {B} Halton starts; one MI355X, one session')

# ---- kernel alone ----
ctrl = get_controller('htwa', par, B)
s = ctrl.ocp_solver
pr, nq = ctrl.problem, ctrl.problem.nq
q = pr.x_min[:nq] + cl.halton(4 * B + 16, nq) * (pr.x_max[:nq] - pr.x_min[:nq])
x_all = np.hstack([q, np.zeros_like(q)])
free = np.asarray(s.check_trajectory(x_all[:, None, :], tol_x=0.0))
x0 = x_all[free][:B]
dev = torch.device('cuda', 0)
t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)
ctrl.p[:, :, 3] = par.alpha
x0d, xd, ud, pd = t(x0), t(np.repeat(x0[:, None, :], N + 1, axis=1)), t(np.zeros((B, N, nq))), t(ctrl.p)
s.sqp(x0d, xd, ud, pd, dict(max_iter=20))
s.sync()
fl = torch.zeros((B,), dtype=torch.int32, device=dev); wo = torch.zeros((B, 5), dtype=torch.float64, device=dev)
mo = torch.zeros((B, 3), dtype=torch.float64, device=dev)
s.check_guess(xd, ud, safe_node=N, flags=fl, worst=wo); s.check_guess(xd, ud, flags=fl, worst=wo); s.merit_terms(x0d, xd, ud, pd, out=mo); s.sync()
def timed(fn, reps=20):
    with torch.cuda.stream(s._ext_stream):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps
say('## kernel alone, B = 4096, N = 30, after 20 SQP iterations from the constant guess (HIP events, mean of 20 back-to-back calls)')
say(f'smpc_check_guess, safe_node = N (list + forward network pass on 4096 rows + k_check_guess + counter reset): {timed(lambda: s.check_guess(xd, ud, safe_node=N, flags=fl, worst=wo)):.3f} ms')
say(f'smpc_check_guess, safe_node none (k_check_guess alone): {timed(lambda: s.check_guess(xd, ud, flags=fl, worst=wo)):.3f} ms')
say(f'smpc_check_guess, safe_node = N, collision rows on every node: {timed(lambda: s.check_guess(xd, ud, safe_node=N, collision_first_node=0, flags=fl, worst=wo)):.3f} ms')
say(f'one launch_merit pass (smpc_merit_terms at the iterate, no step): {timed(lambda: s.merit_terms(x0d, xd, ud, pd, out=mo)):.3f} ms')
cd_ = get_controller('htwa', par, B, device_state=True, solver=s, net=ctrl.net)
cd_.x_temp, cd_.u_temp = xd, ud
cd_.checkGuess(); s.sync()
t0 = time.perf_counter()
for _ in range(5):
    ok = cd_.checkGuess()
s.sync(); torch.cuda.synchronize()
say(f'four-call checkGuess on device tensors (wall, mean of 5, synchronised at the end): {1e3 * (time.perf_counter() - t0) / 5:.2f} ms; accepts {int(ok.sum())}, flags == 0 for {int((fl == 0).sum())}')
del cd_, ctrl, s, xd, ud
torch.cuda.empty_cache()

# ---- generation ----
iters_seen = {}
_orig, _orig_check = BatchedOcpSolver.sqp, BatchedOcpSolver.check_guess
def _spy(self, *a, **k):
    r = _orig(self, *a, **k)
    iters_seen['state'] = r[2]
    return r
BatchedOcpSolver.sqp = _spy

def closed_loop_fails(xg, ug, steps=100):
    """solves with status != 0 over `steps` plain steps of the htwa controller on the device (nominal plant, no backup controller)"""
    n = len(xg)
    c = get_controller('htwa', par, n, device_state=True)
    c.setGuess(xg, ug)
    x = t(xg[:, 0])
    bad = torch.zeros((), dtype=torch.int64, device=dev)
    for _ in range(steps):
        u, _ab = c.step(x)
        bad += (c.last_status != 0).sum()
        x, _ = c.ocp_solver.plant_step(x, u.contiguous())
    c.ocp_solver.sync()
    return int(bad.item()), n * steps

say('## generation on the bench workload')
pg = copy.copy(par); pg.nlp_max_iter = 1000
t0 = time.perf_counter()
ga, good = cl.generate_guess(pg, 'htwa', B, on_device=True)
wa = time.perf_counter() - t0
st = iters_seen['state']
say(f'(a) generate_guess(on_device=True), nlp_max_iter 1000: {wa:.2f} s, {int(st["iters"].sum().item())} instance-iterations, 4096 samples, {int(good.sum())} accepted')
BatchedOcpSolver.sqp = _orig
runs = {}
for tag, kw in (('(b) until, final, K = 50', dict(accept='final', check_every=50)),
                ('(c) until, first, K = 20', dict(accept='first', check_every=20)),
                ('(d) until, final, K = 50, batch = 1024', dict(accept='final', check_every=50, batch=1024)),
                ('(e) until, first, K = 20, batch = 1024', dict(accept='first', check_every=20, batch=1024))):
    spent = {'sqp': 0.0, 'check': 0.0}
    def _clocked(name, fn):
        def run(self, *a, **k):
            t1 = time.perf_counter()
            r = fn(self, *a, **k)
            self.sync()
            spent[name] += time.perf_counter() - t1
            return r
        return run
    BatchedOcpSolver.sqp, BatchedOcpSolver.check_guess = _clocked('sqp', _orig), _clocked('check', _orig_check)
    t0 = time.perf_counter()
    g, info = cl.generate_guess_until(pg, 'htwa', B, **kw)
    w = time.perf_counter() - t0
    BatchedOcpSolver.sqp, BatchedOcpSolver.check_guess = _orig, _orig_check
    runs[tag] = g
    it = np.array(list(info['iters'].values()))
    say(f'{tag}: {w:.2f} s (of which {spent["sqp"]:.2f} s in solver.sqp and {spent["check"]:.3f} s in solver.check_guess, each waited for), {info["instance_iterations"]} instance-iterations, {info["issued"]} samples issued, {len(info["accepted"])} accepted, '
        f'{len(info["failed"])} failed, {info["rounds"]} rounds; iterations per sample min / median / max {it.min()} / {int(np.median(it))} / {it.max()}')
say('## htwa closed loop from the guesses: solves with status != 0 over 100 steps (nominal plant, controller steps only)')
for tag, g in (('(a)', ga), ('(b)', runs['(b) until, final, K = 50']), ('(c)', runs['(c) until, first, K = 20'])):
    bad, tot = closed_loop_fails(g['xg'], g['ug'])
    say(f'{tag}: {bad} failed instance-steps of {tot}')
say('## scripts/policy_bench.py run_mpc(htwa, 100 steps, device state) from the guesses')
for tag, g in (('(a)', ga), ('(c)', runs['(c) until, first, K = 20'])):
    tm = {}
    res = cl.run_mpc(par, 'htwa', g['xg'], g['ug'], n_steps=100, on_device=True, timing=tm)
    say(f"{tag}: {tm['ms_per_step']:.3f} ms/step, B = {len(g['xg'])} | collisions {len(res['collisions_idx'])} viable {len(res['viable_idx'])} "
        f"converged {len(res['conv_idx'])} unconverged {len(res['unconv_idx'])} abort events {len(res['x_viable'])}")
OUT.close()
