"""Do the sub-batches' QP launches of bench.py run side by side?  Reads the per-dispatch rows of a rocprofv3 --kernel-trace CSV
(scripts/prof_bench.sh keeps it as kernel_trace.csv) and prints, for the timed steps of the loop,

  * the hardware queue (Queue_Id) each sub-batch's k_qp_ipm<6,6,false> launches ran on,
  * for every pair of sub-batches, the time during which both had a QP launch running, as a share of the QP launch time of the one
    that ran less (100 % = the shorter one never ran alone, 0 % = the two took turns),
  * the share of the wall time with 0, 1, 2, .. QP launches in flight, and the step time that wall time amounts to.

A sub-batch is a stream: where the trace carries a Stream_Id that tells the launches apart it is used (the --subs streams with the
most launches of the kernel); otherwise the launches are dealt out in dispatch order, which is the order bench.py's host loop
enqueues them in (sub-batch 0, 1, 2, 0, ..).  Of each sub-batch's
launches the first --warmup are skipped and the next --steps kept (bench.py's defaults; what follows them in a --full run -- the
event-ring continuation, the survey window -- is left out as well).  Two streams on one hardware queue run in order: they show
up here as one Queue_Id and no overlap.  Needs no GPU.

usage: trace_overlap.py <kernel_trace.csv> [--kernel 'k_qp_ipm<6,6,false>'] [--subs 3] [--warmup 10] [--steps 100]"""
import argparse
import collections
import csv
import itertools


def short_name(full):
    return full.split('(')[0].replace('void ', '').replace(' ', '')


def qp_launches(rows, kernel):
    """[(dispatch id, queue id, stream id or None, start, end)] of the kernel's launches, in dispatch order"""
    out = []
    for r in rows:
        if kernel not in short_name(r['Kernel_Name']):
            continue
        sid = r.get('Stream_Id')
        out.append((int(r.get('Dispatch_Id') or 0), int(r['Queue_Id']), int(sid) if sid not in (None, '') else None,
                    int(r['Start_Timestamp']), int(r['End_Timestamp'])))
    out.sort(key=lambda l: (l[0], l[3]))
    return out


def split_sub_batches(launches, n_subs):
    """-> (how the sub-batches were told apart, [launches of sub-batch 0, 1, ..])"""
    by_stream = collections.OrderedDict()
    for l in launches:
        by_stream.setdefault(l[2], []).append(l)
    if None not in by_stream and len(by_stream) >= n_subs:
        # (a stream with fewer launches than the sub-batches' -- a probe handle running the same kernel -- is left out)
        busiest = sorted(by_stream, key=lambda k: -len(by_stream[k]))[:n_subs]
        return 'Stream_Id', [v for k, v in by_stream.items() if k in busiest]
    return 'dispatch order', [launches[i::n_subs] for i in range(n_subs)]


def in_flight_profile(intervals):
    """{number of intervals open: time} between the first start and the last end"""
    ev = sorted([(s, 1) for s, _ in intervals] + [(e, -1) for _, e in intervals])
    acc, n, t_prev = collections.Counter(), 0, ev[0][0]
    for t, d in ev:
        acc[n] += t - t_prev
        n, t_prev = n + d, t
    return acc


def overlap(a, b):
    """time during which an interval of a and an interval of b are both open (each list disjoint in itself: one stream)"""
    tot, j = 0, 0
    a, b = sorted(a), sorted(b)
    for s, e in a:
        while j < len(b) and b[j][1] <= s:
            j += 1
        k = j
        while k < len(b) and b[k][0] < e:
            tot += max(0, min(e, b[k][1]) - max(s, b[k][0]))
            k += 1
    return tot


def report(rows, kernel='k_qp_ipm<6,6,false>', n_subs=3, warmup=10, steps=100):
    launches = qp_launches(rows, kernel.replace(' ', ''))
    if len(launches) < n_subs:
        return f'{len(launches)} launches of {kernel} in the trace: nothing to compare'
    how, subs = split_sub_batches(launches, n_subs)
    timed = [s[warmup:warmup + steps] for s in subs]
    if any(len(t) == 0 for t in timed):
        return f'fewer than {warmup} + 1 launches per sub-batch ({[len(s) for s in subs]}): no timed step in the trace'
    iv = [[(l[3], l[4]) for l in t] for t in timed]
    busy = [sum(e - s for s, e in v) for v in iv]
    out = [f'{kernel}: {len(launches)} launches, {n_subs} sub-batches told apart by {how}; launches {warmup}..{warmup + len(timed[0]) - 1} '
           f'of each (the timed steps)']
    for i, t in enumerate(timed):
        q = collections.Counter(l[1] for l in t)
        sid = sorted({l[2] for l in t if l[2] is not None})
        out.append(f'  sub-batch {i}: queue ' + ', '.join(f'{k} ({n} launches)' for k, n in sorted(q.items())) +
                   (f'; stream {", ".join(map(str, sid))}' if sid else '') +
                   f'; {len(t)} launches, {busy[i] / len(t) / 1e3:.1f} us each')
    queues = [collections.Counter(l[1] for l in t).most_common(1)[0][0] for t in timed]
    out.append(f'  distinct queues: {len(set(queues))} of {n_subs}')
    out.append('both running, as a share of the QP launch time of the one that ran less:')
    for i, j in itertools.combinations(range(n_subs), 2):
        out.append(f'  sub-batches {i} and {j}: {100.0 * overlap(iv[i], iv[j]) / max(min(busy[i], busy[j]), 1):5.1f} %'
                   + ('   (same queue)' if queues[i] == queues[j] else ''))
    prof = in_flight_profile([x for v in iv for x in v])
    wall = sum(prof.values())
    out.append(f'QP launches in flight, share of the {wall / 1e6:.2f} ms between the first start and the last end '
               f'({wall / 1e6 / max(len(t) for t in timed):.3f} ms per step):')
    for n in range(n_subs + 1):
        out.append(f'  {n}: {100.0 * prof.get(n, 0) / wall:5.1f} %')
    return '\n'.join(out)


if __name__ == '__main__':
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('trace')
    ap.add_argument('--kernel', default='k_qp_ipm<6,6,false>')
    ap.add_argument('--subs', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--steps', type=int, default=100)
    a = ap.parse_args()
    with open(a.trace, newline='') as f:
        print(report(list(csv.DictReader(f)), a.kernel, a.subs, a.warmup, a.steps))
