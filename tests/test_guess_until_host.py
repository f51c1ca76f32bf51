"""smpc_check_guess and generate_guess_until as far as they can be held without a GPU: the entry point is declared and exported,
the ctypes mirror of smpc_guess_check matches the header, the slot bookkeeping (closed_loop.GuessSlots) yields the first n accepted
samples in sampling order whatever the batch, and generate_guess_until refuses a solver that has no device SQP."""
import ctypes as C
import os
import re
import subprocess

import pytest

from conftest import ROOT


def test_check_guess_declared_and_exported():
    from safe_mpc_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    hdr = open(os.path.join(ROOT, 'include', 'smpc.h')).read()
    declared = set(re.findall(r'^int\s+(smpc_[a-z_]+)\s*\(', hdr, re.M))
    L = C.CDLL(_lib.LIB_PATH)
    assert 'smpc_check_guess' in declared and 'smpc_check_guess' in _lib.SYMBOLS and hasattr(L, 'smpc_check_guess')
    assert re.search(r'#define SMPC_ABI_VERSION 5\b', hdr)


def test_guess_check_struct_matches_the_header(tmp_path):
    """sizeof / offsetof of smpc_guess_check compiled from the header with gcc against the ctypes mirror"""
    from safe_mpc_amd import _lib
    G = _lib.GuessCheck
    gf = [n for n, _ in G._fields_]
    fmt = ' '.join(['%zu'] * (1 + len(gf)))
    args = ', '.join(['sizeof(smpc_guess_check)'] + [f'offsetof(smpc_guess_check, {n})' for n in gf])
    src = tmp_path / 'sz.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "smpc.h"\n'
                   f'int main(void) {{ printf("{fmt}\\n", {args}); return 0; }}\n')
    exe = tmp_path / 'sz'
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    v = [int(t) for t in subprocess.check_output([str(exe)]).split()]
    assert v == [C.sizeof(G)] + [getattr(G, n).offset for n in gf]
    assert gf == ['tol_x', 'tol_tau', 'tol_dyn', 'tol_safe', 'alpha', 'collision_first_node', 'safe_node', 'x_min', 'x_max', 'tau_min',
                  'tau_max', 'row_lb_chk', 'row_ub_chk']


# ---- the bookkeeping on scripted fates ---------------------------------------------------------------------------------------------
def _play(fates, n, batch, max_samples=None):
    """fates[j] = (rounds until sample j is resolved, accepted?).  Runs GuessSlots the way generate_guess_until does -- issue, one
    round for every live slot, resolve -- and returns (book, most in flight seen, samples issued at each issue call)."""
    from safe_mpc_amd.closed_loop import GuessSlots
    book = GuessSlots(n, batch, max_samples)
    age, most, issues = {}, 0, []
    while True:
        new = book.issue()
        issues.append([j for _, j in new])
        for _, j in new:
            assert j not in age
            age[j] = 0
        assert len(book.accepted) + book.in_flight <= n                 # never more in flight than n - accepted
        assert book.in_flight <= book.batch
        most = max(most, book.in_flight)
        live = book.live()
        if not live:
            break
        for slot, j in live:
            age[j] += 1
            rounds, ok = fates[j]
            if age[j] >= rounds:
                assert book.resolve(slot, ok) == j
    return book, most, issues


def _first_n_accepted(fates, n):
    return [j for j, (_, ok) in enumerate(fates) if ok][:n]


FATES = [(1 + (7 * j) % 4, j % 3 != 1) for j in range(64)]          # every third sample fails, 1..4 rounds each


@pytest.mark.parametrize('batch', [1, 3, 10, None])
def test_slots_give_the_first_n_accepted_in_sampling_order(batch):
    n = 10
    book, most, _ = _play(FATES, n, batch)
    want = _first_n_accepted(FATES, n)
    assert book.result_order() == want
    assert book.finished() and not book.exhausted and book.in_flight == 0
    # the issued samples are a prefix of the stream, all resolved
    assert sorted(book.accepted + book.failed) == list(range(book.issued))
    assert book.issued == want[-1] + 1
    assert sorted(book.failed) == [j for j in range(book.issued) if not FATES[j][1]]
    assert most == min(batch or n, n)


def test_slots_result_does_not_depend_on_the_batch():
    runs = [_play(FATES, 17, b)[0] for b in (1, 3, 17)]
    assert runs[0].result_order() == runs[1].result_order() == runs[2].result_order()
    assert sorted(runs[0].failed) == sorted(runs[1].failed) == sorted(runs[2].failed)
    assert runs[0].issued == runs[1].issued == runs[2].issued


def test_a_late_failure_issues_exactly_one_more_sample():
    """n = 4 in 4 slots; samples 0..2 are accepted after one round, sample 3 fails after three: one more sample, and only then"""
    fates = [(1, True), (1, True), (1, True), (3, False), (1, True), (1, True)]
    book, _, issues = _play(fates, 4, 4)
    assert issues == [[0, 1, 2, 3], [], [], [4], []]
    assert book.result_order() == [0, 1, 2, 4] and book.failed == [3] and book.issued == 5


def test_max_samples_stops_the_stream():
    book, _, _ = _play(FATES, 10, 3, max_samples=8)
    assert book.issued == 8 and book.finished() and book.exhausted
    assert book.result_order() == [j for j in range(8) if FATES[j][1]] and len(book.accepted) < 10
    # enough samples: not exhausted
    book, _, _ = _play(FATES, 4, 3, max_samples=40)
    assert not book.exhausted and len(book.accepted) == 4


def test_resolving_a_free_slot_is_an_error():
    from safe_mpc_amd.closed_loop import GuessSlots
    book = GuessSlots(2, 2)
    book.issue()
    book.resolve(0, True)
    with pytest.raises(ValueError):
        book.resolve(0, True)


def test_slots_fill_in_time_linear_in_the_batch():
    """issue() does a constant amount of work per slot: 65536 slots fill at once (a count of the live slots per slot filled made
    this quadratic), the lowest free slot first"""
    from safe_mpc_amd.closed_loop import GuessSlots
    book = GuessSlots(65536)
    new = book.issue()
    assert new == [(k, k) for k in range(65536)] and book.in_flight == 65536 and book.issue() == []
    book.resolve(7, False)
    book.resolve(3, True)
    assert book.in_flight == 65534 and book.issue() == [(3, 65536)] and book.in_flight == 65535     # (one accepted: one fewer needed)
    assert book.live()[3] == (3, 65536) and len(book.live()) == 65535


def test_a_filter_that_rejects_everything_raises():
    """the sample stream stops drawing when the collision filter lets nothing through; max_samples would not stop it"""
    import types
    import numpy as np
    from safe_mpc_amd.closed_loop import _FreeStarts
    calls = []

    def none_free(x, tol_x):
        calls.append(len(x))
        return np.zeros(len(x), bool)
    pr = types.SimpleNamespace(nq=6, nx=12, x_min=-np.ones(12), x_max=np.ones(12))
    with pytest.raises(RuntimeError, match='collision filter rejected'):
        _FreeStarts(types.SimpleNamespace(check_trajectory=none_free), pr, chunk=32, max_barren=5).take(0)
    assert calls == [32] * 5
    # and one that lets some through is the same stream whatever the chunking
    some = types.SimpleNamespace(check_trajectory=lambda x, tol_x: x[:, 0, 0] > 0.0)
    a, b = _FreeStarts(some, pr, chunk=7), _FreeStarts(some, pr, chunk=64)
    assert all(np.array_equal(a.take(j), b.take(j)) for j in (0, 5, 40))


# ---- a solver without a device SQP ---------------------------------------------------------------------------------------------------
def test_generate_guess_until_needs_a_device_sqp():
    """the oracle-backed controller has no device SQP: the same clear ValueError as generate_guess(on_device=True)"""
    from fake_solver import make_double_controller
    from safe_mpc_amd import closed_loop as cl
    from safe_mpc_amd.parser import Parameters
    par = Parameters({}, 'z1')
    par.nq, par.n_dof_safe_set, par.net_size, par.N, par.nlp_max_iter = 6, 6, [12, 256, 1], 20, 200
    mk = lambda n, b: make_double_controller(n, par, b)
    with pytest.raises(ValueError, match='device SQP') as until:
        cl.generate_guess_until(par, 'htwa', 8, make_controller=mk)
    with pytest.raises(ValueError, match='device SQP') as plain:
        cl.generate_guess(par, 'htwa', 8, make_controller=mk, on_device=True)
    assert str(until.value) == str(plain.value)
