"""Replay of k_qp_ipm's crew (point 4c) on recorded iteration counts: no GPU.

A launch over P pairs of instances runs G = ceil(f P) wavefronts.  The pairs are laid out longest-expected-first -- by the PREVIOUS
step's iteration counts, as the engine's k_order_by_iters does -- wavefront w starts on pair w, and a wavefront that has finished its
pair takes the next one from the ticket.  That is list scheduling of the pairs on G machines.  A pair lasts as long as the longer of its
two instances; the unit of time is one IPM iteration (set-up and write-back of a pair are a fraction of one, --overhead adds them).

Input: tests/golden/qp_crew_iters_c1.npz -- `iters` [steps, B] uint8, the IPM iterations of every instance in every step of the bench's
own closed loop (C1, 4096 instances, 10 warm-up + 100 timed steps), and `pieces` [S, 2], the sub-batches' instance ranges (a launch
each).  Recorded once with `python scripts/qp_crew_replay.py --record FILE` on an MI355X (results do not depend on the crew).

Output per f: the launch makespan relative to f = 1 (mean / 95th percentile / maximum over steps and sub-batches; at f = 1 the makespan
is the slowest pair), the paper bound (sum of the pair maxima) / (P x launch maximum) of the fixture, and the residency profile -- the
wavefronts of a launch still resident after t iterations, averaged over the launches.

usage: python scripts/qp_crew_replay.py [--fractions 1 0.9 0.8 ...] [--overhead 0.0] [--file FIXTURE]
       python scripts/qp_crew_replay.py --record FILE [--steps 110]
"""
import argparse
import heapq
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'qp_crew_iters_c1.npz')


def crew_size(f, pairs):
    """G = ceil(f pairs), as engine.hip's qp_crew_waves"""
    return int(min(max(int(np.ceil(f * pairs)), 1), max(pairs, 1)))


def pair_durations(prev, cur):
    """durations of a launch's pairs in ticket order: instances sorted by decreasing `prev` (stable inside a bin: the engine's order
    there is arbitrary), two per pair, a pair as long as the longer of its two `cur`"""
    order = np.argsort(-np.asarray(prev, dtype=np.int64), kind='stable')
    d = np.asarray(cur, dtype=np.float64)[order]
    if len(d) % 2:
        d = np.append(d, 0.0)           # (odd batch: the last pair's second half sits it out)
    return d.reshape(-1, 2).max(axis=1)


def list_schedule(durations, G, overhead=0.0):
    """pairs in ticket order on G wavefronts: (makespan, the time every wavefront retires at, every pair's start time)"""
    P = len(durations)
    G = min(G, P)
    ends = [(0.0, w) for w in range(G)]         # (a heap of (free-at, wavefront): wavefront w starts on pair w)
    heapq.heapify(ends)
    starts = np.zeros(P)
    for p in range(P):
        t, w = heapq.heappop(ends)
        starts[p] = t
        heapq.heappush(ends, (t + durations[p] + overhead, w))
    retire = np.array(sorted(t for t, _ in ends))
    return (float(retire[-1]) if P else 0.0), retire, starts


def residency(retire, t_max):
    """wavefronts still resident at t = 0, 1, .. t_max"""
    return np.array([(retire > t).sum() for t in range(t_max + 1)])


def replay(iters, pieces, fractions, overhead=0.0):
    """per f: dict(ratio [launches] makespan / makespan at f = 1, resid [t] mean resident wavefronts, peak, G)"""
    out = {}
    steps = iters.shape[0]
    t_max = int(iters.max()) * 2 + 2
    for f in fractions:
        ratios, resid, n = [], np.zeros(t_max + 1), 0
        for lo, hi in pieces:
            G = crew_size(f, (hi - lo + 1) // 2)
            for k in range(1, steps):
                d = pair_durations(iters[k - 1, lo:hi], iters[k, lo:hi])
                full, _, _ = list_schedule(d, len(d), overhead)
                ms, retire, _ = list_schedule(d, G, overhead)
                ratios.append(ms / full if full > 0 else 1.0)
                resid += residency(retire, t_max)
                n += 1
        out[f] = {'ratio': np.array(ratios), 'resid': resid / max(n, 1), 'G': [crew_size(f, (hi - lo + 1) // 2) for lo, hi in pieces]}
    return out


def paper_bound(iters, pieces):
    """(sum of pair maxima) / (pairs x launch maximum), mean over launches: below this f the launch lengthens by construction"""
    v = []
    for lo, hi in pieces:
        for k in range(1, iters.shape[0]):
            d = pair_durations(iters[k - 1, lo:hi], iters[k, lo:hi])
            if d.max() > 0:
                v.append(d.sum() / (len(d) * d.max()))
    return float(np.mean(v))


def record(path, steps):
    """the bench's own loop (bench.py: build_problem, initial_states, three sub-batches, <controller>.step_on_device + plant_step), one
    sub-batch after the other, with the iteration counts of every step copied out"""
    sys.path.insert(0, ROOT)
    import torch
    import bench
    from safe_mpc_amd.controller import get_controller
    from safe_mpc_amd.sharding import shard_range
    from safe_mpc_amd.solver import BatchedOcpSolver
    par, prob, net = bench.build_problem()
    dev = torch.device('cuda', 0)
    B, S, N, nu = bench.B_PER_GPU, 3, prob.N, prob.nu
    t = lambda a: torch.tensor(a, dtype=torch.float64, device=dev)
    x0 = bench.initial_states(BatchedOcpSolver(prob, net, device=0), prob, B, 0)
    p = np.zeros((B, N + 1, 5))
    p[:, :, :3], p[:, :, 3], p[:, :, 4] = prob.ee_ref, par.alpha, 1.0
    pieces = [shard_range(B, S, i) for i in range(S)]
    iters = np.zeros((steps, B), np.uint8)
    for lo, hi in pieces:
        sv = BatchedOcpSolver(prob, net, device=0)
        sv.set_qp_mode('throughput')
        with torch.cuda.stream(torch.cuda.ExternalStream(sv.L.smpc_stream(sv.h), device=dev)):
            ctrl = get_controller(bench.CONTROLLER, par, hi - lo, cost='ext', N=N, solver=sv, net=net, device=0, device_state=True)
            ctrl.setGuess(t(np.repeat(x0[lo:hi, None, :], N + 1, axis=1)), t(np.zeros((hi - lo, N, nu))))
            ctrl.p.copy_(t(p[lo:hi]))
            x, xn = t(x0[lo:hi]), t(x0[lo:hi])
            u, ue = torch.empty((hi - lo, nu), dtype=torch.float64, device=dev), torch.empty((hi - lo, nu), dtype=torch.float64, device=dev)
            for k in range(steps):
                ctrl.step_on_device(x, u_out=u)
                sv.plant_step(x, u, None, None, out=(xn, ue))
                x, xn = xn, x
                sv.sync()
                iters[k, lo:hi] = np.minimum(ctrl.qp_iter.cpu().numpy(), 255)
    np.savez_compressed(path, iters=iters, pieces=np.array(pieces, np.int32))
    print('wrote', path, os.path.getsize(path), 'bytes; mean iterations over the last', steps - 10, 'steps', iters[10:].mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--file', default=FIXTURE)
    ap.add_argument('--fractions', type=float, nargs='+', default=[1.0, 0.9, 0.8, 0.75, 0.7, 0.65, 0.6, 0.5])
    ap.add_argument('--overhead', type=float, default=0.0, help='set-up and write-back of a pair, in iterations')
    ap.add_argument('--record', metavar='FILE', default=None)
    ap.add_argument('--steps', type=int, default=110)
    a = ap.parse_args()
    if a.record:
        return record(a.record, a.steps)
    with np.load(a.file) as z:
        iters, pieces = z['iters'], [tuple(int(v) for v in r) for r in z['pieces']]
    print(f'{a.file}: {iters.shape[0]} steps x {iters.shape[1]} instances, launches {pieces}')
    print(f'mean iterations {iters[1:].mean():.2f}, mean launch maximum {np.mean([iters[k, lo:hi].max() for lo, hi in pieces for k in range(1, len(iters))]):.2f}, '
          f'paper bound on f {paper_bound(iters, pieces):.3f}')
    res = replay(iters, pieces, a.fractions, a.overhead)
    print('    f      G   makespan / (f = 1): mean    p95     max   launches longer   resident wavefronts after t iterations: 0, 2, 4, .. 16')
    for f in a.fractions:
        r = res[f]
        print('%5.2f  %5d  %26.4f %6.4f %7.4f %16.1f%%   %s' % (f, r['G'][0], r['ratio'].mean(), np.percentile(r['ratio'], 95), r['ratio'].max(),
                                                           100.0 * (r['ratio'] > 1.0 + 1e-12).mean(), ' '.join('%4.0f' % v for v in r['resid'][0:17:2])))


if __name__ == '__main__':
    main()
