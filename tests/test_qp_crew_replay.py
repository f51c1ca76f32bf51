"""scripts/qp_crew_replay.py, the replay of k_qp_ipm's crew on recorded iteration counts: its list scheduler against a brute-force
simulation that shares nothing with it, and its f = 1 makespan against the recorded fixture's per-step maxima.  No GPU."""
import importlib.util
import itertools
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location('qp_crew_replay', os.path.join(ROOT, 'scripts', 'qp_crew_replay.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


T = _tool()


def _brute(durations, G):
    """the crew, tick by tick: wavefront w starts on pair w; whenever a wavefront has no work left it takes the next ticket (any number
    of zero-length pairs in one tick); integer durations.  Returns (makespan, sorted retire times, start time of every pair)."""
    P = len(durations)
    G = min(G, P)
    left = [0] * G              # ticks of work the wavefront still has
    retire = [None] * G
    starts = [None] * P
    nxt, t = 0, 0
    while any(r is None for r in retire):
        for w in range(G):
            while retire[w] is None and left[w] == 0:
                if nxt < P:
                    starts[nxt] = t
                    left[w] = durations[nxt]
                    nxt += 1
                else:
                    retire[w] = t
        for w in range(G):
            if left[w] > 0:
                left[w] -= 1
        t += 1
    return max(retire), sorted(retire), starts


def test_list_scheduler_equals_brute_force_up_to_8_pairs_and_3_wavefronts():
    rng = np.random.default_rng(0)
    cases = [list(c) for P in range(1, 5) for c in itertools.product([0, 1, 3], repeat=P)]          # every small array, zeros included
    cases += [list(rng.integers(0, 14, P)) for P in range(5, 9) for _ in range(60)]                 # ... and random ones up to 8 pairs
    cases += [sorted(rng.integers(1, 20, 8), reverse=True) for _ in range(20)]                      # longest-first, as the engine aims at
    n = 0
    for d in cases:
        for G in (1, 2, 3):
            ms, retire, starts = T.list_schedule(np.array(d, float), G)
            ms_b, retire_b, starts_b = _brute([int(v) for v in d], G)
            assert ms == ms_b, (d, G)
            assert retire.tolist() == [float(v) for v in retire_b], (d, G)
            assert starts.tolist() == [float(v) for v in starts_b], (d, G)
            # what list scheduling guarantees (Graham): no shorter than the longest pair or the mean load, within one pair of the latter
            g = min(G, len(d))
            assert ms >= max(max(d), sum(d) / g) - 1e-12 and ms <= sum(d) / g + max(d) * (1 - 1 / g) + 1e-12, (d, G)
            n += 1
    assert n > 1000


def test_crew_size_is_the_engines():
    # G = ceil(f pairs), at least one wavefront, at most one per pair
    assert [T.crew_size(f, 683) for f in (1.0, 0.75, 0.5, 1e-9)] == [683, 513, 342, 1]
    assert T.crew_size(1.0, 1) == 1 and T.crew_size(0.3, 1) == 1


def test_pairs_follow_the_previous_steps_order():
    prev, cur = np.array([3, 9, 5, 7, 1]), np.array([4, 8, 6, 20, 2])
    # order by decreasing prev: instances 1, 3, 2, 0, 4 -> pairs (1, 3), (2, 0), (4, -)
    assert T.pair_durations(prev, cur).tolist() == [20.0, 6.0, 2.0]


@pytest.fixture(scope='module')
def fixture():
    with np.load(T.FIXTURE) as z:
        return z['iters'], [tuple(int(v) for v in r) for r in z['pieces']]


def test_fixture_is_the_benchs_loop(fixture):
    iters, pieces = fixture
    assert iters.dtype == np.uint8 and iters.shape == (110, 4096)
    assert pieces == [(0, 1366), (1366, 2731), (2731, 4096)]
    assert os.path.getsize(T.FIXTURE) < (1 << 20)
    assert iters.min() >= 1 and iters[10:].mean() > 5.0        # (every instance steps in the bench's loop; ~7.7 iterations on average)


def test_full_crew_makespan_is_the_per_step_maximum(fixture):
    iters, pieces = fixture
    for lo, hi in pieces:
        for k in range(1, iters.shape[0], 7):
            d = T.pair_durations(iters[k - 1, lo:hi], iters[k, lo:hi])
            ms, retire, starts = T.list_schedule(d, T.crew_size(1.0, len(d)))
            assert ms == float(iters[k, lo:hi].max())
            assert not starts.any() and len(retire) == len(d)
    res = T.replay(iters[:12], pieces, [1.0, 0.5])
    assert np.all(res[1.0]['ratio'] == 1.0)
    assert np.all(res[0.5]['ratio'] >= 1.0) and res[0.5]['resid'][0] == pytest.approx(np.mean(res[0.5]['G']))
