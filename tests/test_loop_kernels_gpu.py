"""The closed-loop driver's kernels (k_loop_pre, k_loop_classify_aborts, k_loop_apply_backup, k_loop_post; kernels_policy.hpp)
against their numpy statements (tests/loop_cases.py, pinned to the scalar oracle by tests/test_loop_kernels_host.py), through
BatchedOcpSolver.loop_pre / .loop_classify_aborts / .loop_apply_backup / .loop_post with a stand-in for the group object.

1. one call of each entry point on scripted state tables in which every instance belongs to a named branch class, for
   nq in {5, 6, 7}, Nb in {1, 2, 5}, B in {1, 63, 64, 65, 130} (one thread per instance, blocks of 64);
2. the scripted scenario of loop_cases.Scenario in closed_loop._DeviceGroup's call order, every call held against the statement
   applied to the device's own previous state, the discrete outcome against the scalar oracle's.

Everything is compared bit for bit except (a) the PD controls: the compiler may contract kp dq + kd dv into an fma, so
4 eps (|u_abort| + kp |dq| + kd |dv|) per component; (b) what the plant step computes: test_callers_parity's 1e-10 on the state.
Every array lies between 256 bytes of sentinel on both sides, which must come back untouched; arrays an entry point is not
documented to write must come back bit for bit.  Every test prints a line `LOOPKERNELS ...` (profiles/loop_kernel_tests.txt)."""
import numpy as np
import pytest

import loop_cases as lc
from loop_cases import Dev
from conftest import make_problem, make_problem_fr7

pytestmark = pytest.mark.gpu

X_ATOL = 1e-10                   # the plant step against the oracle's, as in test_callers_parity


class Group:
    """what BatchedOcpSolver._loop_state reads of a closed_loop._DeviceGroup"""

    def __init__(self, t, B, Nb):
        self._B, self._Nb = B, Nb
        for k in lc.STATE_KEYS:
            setattr(self, {'step': '_jt', 'resumed': '_resumed'}.get(k, k), t.get(k))


_SOLVERS = {}


def _solver(nq):
    from oracle.oracle import Oracle
    from safe_mpc_amd.solver import BatchedOcpSolver
    if nq not in _SOLVERS:
        par, prob, net = make_problem_fr7('naive', 'ext', N=2) if nq == 7 else make_problem('naive', 'ext', N=2, nq=nq)
        _SOLVERS[nq] = (par, prob, BatchedOcpSolver(prob, None), Oracle(prob))
    return _SOLVERS[nq]


def _call(sv, entry, d, B, Nb, quirks=True):
    """upload d, run one entry point, download"""
    dev = Dev(d)
    t, g = dev.t, Group(dev.t, B, Nb)
    if entry == 'pre':
        sv.loop_pre(g, t['r'], t['pending'], t['u_other'], t['stepping'])
    elif entry == 'classify':
        sv.problem.params.reference_quirks = bool(quirks)
        sv.loop_classify_aborts(g, t['abort'], t['any_event'])
    elif entry == 'backup':
        sv.loop_apply_backup(g, t['rows'], t['status_c'], t['x_c'], t['u_c'], t['viable'], t['u'], t['pending'])
    else:
        sv.loop_post(g, t['u'])
    return dev.host()


def _post_bounds(d, ok_next):
    """what of loop_post's outputs the plant step computed: row step + 1 of x_log, x_cur of the live instances that stay"""
    j = int(d['step'][0])
    xl = np.zeros(d['x_log'].shape)
    xl[j + 1] = X_ATOL
    return {'x_log': xl, 'x_cur': X_ATOL * (d['alive'].astype(bool) & ok_next)[:, None] * np.ones(d['x_cur'].shape)}


@pytest.mark.parametrize('nq', [5, 6, 7])
def test_one_call_on_the_state_tables(nq):
    par, prob, sv, oracle = _solver(nq)
    worst, n_calls, seen = 0.0, 0, set()

    def pd_ratio(got, want, key):
        nz = want['u_bound'] > 0
        return float((np.abs(got[key] - want[key])[nz] / want['u_bound'][nz]).max()) if nz.any() else 0.0

    for Nb in (1, 2, 5):
        for B in (1, 63, 64, 65, 130):
            for offset in (range(len(lc.CLASSES)) if B == 1 else (0,)):
                d, cls = lc.state_table(prob, Nb, B, seed=nq, offset=offset)
                seen |= set(cls)
                if B >= 63:
                    lc.check_table(d, cls, Nb)
                tag = f'nq {nq} Nb {Nb} B {B} offset {offset}'
                # ---- smpc_loop_pre, and each of its optional arguments as NULL --------------------------------------------------
                for null in ({}, {'r': None}, {'r_log': None}, {'pending': None}, {'resumed': None}):
                    s = lc.pick(d, lc.PRE_KEYS, **null)
                    want, got = lc.loop_pre(s, Nb), _call(sv, 'pre', s, B, Nb)
                    assert not lc.differences(got, want, {'u_other': want['u_bound']}), (tag, null, lc.differences(got, want, {'u_other': want['u_bound']}))
                    worst, n_calls = max(worst, pd_ratio(got, want, 'u_other')), n_calls + 1
                # ---- smpc_loop_classify_aborts: abort x resumed x quirks, resumed NULL, nothing left / nothing raised ---------------
                s = lc.pick(d, lc.CLASSIFY_KEYS)
                for quirks in (1, 0):
                    for var in (s, dict(s, resumed=None), dict(s, abort=np.zeros(B, np.uint8)), dict(s, abort=s['resumed'].copy())):
                        want, got = lc.classify_aborts(var, quirks), _call(sv, 'classify', var, B, Nb, quirks)
                        assert not lc.differences(got, want), (tag, quirks, lc.differences(got, want))
                        n_calls += 1
                assert lc.classify_aborts(dict(s, abort=np.zeros(B, np.uint8)), 1)['any_event'][0] == 0 and s['any_event'][0] == 1
                # ---- smpc_loop_apply_backup, and n_c = 0 -------------------------------------------------------------------------
                s = lc.pick(d, lc.BACKUP_KEYS)
                want, got = lc.apply_backup(s, Nb), _call(sv, 'backup', s, B, Nb)
                assert not lc.differences(got, want, {'u': want['u_bound']}), (tag, lc.differences(got, want, {'u': want['u_bound']}))
                worst = max(worst, pd_ratio(got, want, 'u'))
                none = dict(s, rows=s['rows'][:0], status_c=s['status_c'][:0], x_c=s['x_c'][:0], u_c=s['u_c'][:0])
                assert not lc.differences(_call(sv, 'backup', none, B, Nb), none), tag
                # ---- smpc_loop_post ---------------------------------------------------------------------------------------------
                s = lc.pick(d, lc.POST_KEYS)
                x_next, ok_next = lc.oracle_next(oracle, prob, par, s['x_cur'], s['u'])
                if B >= 63:
                    live = s['alive'].astype(bool)
                    assert (live & ok_next).any() and (live & ~ok_next).any() and (~live).any()      # (on the oracle's side)
                want, got = lc.loop_post(s, x_next, ok_next), _call(sv, 'post', s, B, Nb)
                bad = lc.differences(got, want, _post_bounds(s, ok_next))
                assert not bad, (tag, bad)
                n_calls += 3
    assert seen == set(lc.CLASSES)
    assert worst <= 1.0
    print(f'LOOPKERNELS tables nq {nq}: {n_calls} calls, Nb 1 2 5 x B 1 63 64 65 130, {len(seen)} classes, PD controls at most '
          f'{worst:.2f} of 4 eps (|u_abort| + kp |dq| + kd |dv|), everything else bit for bit, sentinels intact')


@pytest.mark.parametrize('quirks', [True, False])
def test_scripted_scenario_in_device_call_order(quirks):
    """loop_pre, the scripted step, classify, the previous step's events, loop_post -- per step, on state that stays on the device
    at fixed addresses; the last step's events after the loop.

    The discrete outcome can only be required to equal the scalar oracle's if no tested quantity of the oracle's run is near its
    threshold: the 5e-3 velocity test, the box +- tol_x and the collision rows' check bounds stay >= 1e-6 away (a condition on the
    script, asserted on the oracle's run), and the device's trajectory must stay within a tenth of the smallest such margin."""
    par, prob, sv, oracle = _solver(6)
    sc = lc.Scenario(prob, par, oracle)
    ref, margin = sc.reference(quirks)
    assert margin >= 1e-6, margin
    B, Nb, n = sc.B, sc.Nb, sc.n_steps
    dev = Dev(sc.initial_state())
    t, g = dev.t, Group(dev.t, B, Nb)
    sv.problem.params.reference_quirks = bool(quirks)
    n_events, events, inflight, worst, n_calls = np.zeros(B, int), [], None, 0.0, 0

    def held(s0, want, bounds, what):
        nonlocal n_calls
        got = dev.host()
        bad = lc.differences(got, {k: v for k, v in want.items() if k in got}, bounds)
        assert not bad, (what, int(s0['step'][0]), bad)
        n_calls += 1
        return got

    def apply(ev, s0):
        nonlocal worst
        evd = Dev(ev)
        sv.loop_apply_backup(g, evd.t['rows'], evd.t['status_c'], evd.t['x_c'], evd.t['u_c'], t['viable'], t['u'], t['pending'])
        want = lc.apply_backup(dict(s0, **ev), Nb)
        got = held(s0, want, {'u': want['u_bound']}, 'apply_backup')
        assert not lc.differences(evd.host(), ev)
        return got

    s = dev.host()
    for j in range(n):
        dev.write('r', sc.r_table[j])
        s = dict(s, r=sc.r_table[j])
        sv.loop_pre(g, t['r'], t['pending'], t['u_other'], t['stepping'])
        want = lc.loop_pre(s, Nb)
        nz = want['u_bound'] > 0
        s = held(s, want, {'u_other': want['u_bound']}, 'loop_pre')
        if nz.any():
            worst = max(worst, float((np.abs(s['u_other'] - want['u_other'])[nz] / want['u_bound'][nz]).max()))
        u, abort = sc.scripted_step(s)
        dev.write('u', u)
        dev.write('abort', abort)
        s = dict(s, u=u, abort=abort)
        sv.loop_classify_aborts(g, t['abort'], t['any_event'])
        s = held(s, lc.classify_aborts(s, quirks), None, 'classify_aborts')
        if inflight is not None:
            s = apply(inflight, s)
            inflight = None
        if s['any_event'][0]:
            inflight = sc.events_of(s, n_events)
            events += [(j, int(b)) for b in inflight['rows']]
            dev.write('pending', s['abort'])
            s = dict(s, pending=s['abort'].copy())
        x_next, ok_next = lc.oracle_next(oracle, prob, par, s['x_cur'], s['u'])
        sv.loop_post(g, t['u'])
        s = held(s, lc.loop_post(s, x_next, ok_next), _post_bounds(s, ok_next), 'loop_post')
    if inflight is not None:
        s = apply(inflight, s)
    # ---- the discrete outcome is the scalar oracle's ------------------------------------------------------------------------
    x, u = lc.blanked_logs(s)
    xo, uo = np.array([r['x'] for r in ref]), np.array([r['u'] for r in ref])
    last = lambda a: np.array([np.where(~np.isnan(v).any(1))[0].max() for v in a])
    assert np.array_equal(np.isnan(x), np.isnan(xo)) and np.array_equal(np.isnan(u), np.isnan(uo))
    assert np.array_equal(s['last_x'], np.where(s['collided'], last(xo), n)) and np.array_equal(s['last_u'], np.where(s['collided'], last(uo), n - 1))
    assert s['collided'].astype(bool).tolist() == [r['collided'] for r in ref] and np.array_equal(s['alive'], 1 - s['collided'])
    assert s['viable'].tolist() == [r['n_viable'] for r in ref]
    assert np.array_equal(s['r_log'].T, np.array([r['r'] for r in ref])) and (s['r_log'] >= 0).any() and (s['r_log'] < 0).any()
    assert sorted(events) == sorted((e[0], b) for b, r in enumerate(ref) for e in r['events'])
    gap = float(np.nanmax(np.abs(x - xo)))
    print(f'LOOPKERNELS scenario quirks {int(quirks)}: {n_calls} calls held against their statements, {len(events)} events, '
          f'{int(s["collided"].sum())} lost, device - oracle trajectory {gap:.2e}, smallest margin of the oracle run {margin:.2e}, '
          f'PD controls at most {worst:.2f} of their bound')
    assert gap < 0.1 * margin
