"""The numpy statements of the closed-loop driver's four entry points (tests/loop_cases.py) against the scalar oracle
(oracle/policy_oracle.py::run_closed_loop): the statements, chained in the device loop's call order over a scripted scenario with
a table-driven controller and scripted backup outcomes, must give per instance what the oracle's loop gives with the same script --
the same NaN pattern of the logs, the same values, events, failures and abort counts.  tests/test_loop_kernels_gpu.py then holds
the kernels against these statements.  CPU only."""
import numpy as np
import pytest

import loop_cases as lc
from conftest import make_problem


@pytest.fixture(scope='module')
def scenario():
    from oracle.oracle import Oracle
    par, prob, net = make_problem('naive', 'ext', N=2)
    return lc.Scenario(prob, par, Oracle(prob))


@pytest.mark.parametrize('quirks', [True, False])
def test_chained_statements_equal_scalar_oracle_loop(scenario, quirks):
    sc = scenario
    ref, margin = sc.reference(quirks)
    d, events = sc.chain(quirks)
    n, Nb = sc.n_steps, sc.Nb
    # ---- the script does what it was written for (asserted on the oracle's run) -----------------------------------------------
    assert not ref[0]['events'] and not ref[0]['collided'] and not np.isnan(ref[0]['x']).any()          # never aborts
    r1 = ref[1]
    assert [e[0] for e in r1['events']] == [2] and r1['rest_tests'] and r1['rest_tests'][0] == 3 + Nb    # abort -> follow -> hold
    assert len(r1['rest_tests']) > 1 and r1['resumes'] == [r1['rest_tests'][-1]] and r1['resumes'][0] < n - 2 and not r1['collided']
    assert ref[2]['collided'] and [e[0] for e in ref[2]['events']] == [3] and ref[2]['n_viable'] == 0    # a failing backup OCP
    assert ref[3]['aborts_on_resume']                                                                    # abort on the resume step
    assert (len(ref[3]['events']) == 1) if quirks else (len(ref[3]['events']) > 1)
    assert ref[4]['collided'] and not ref[4]['events'] and np.isnan(ref[4]['x'][sc.LEAVES + 2]).all() \
        and not np.isnan(ref[4]['x'][sc.LEAVES + 1]).any()                                               # out of the box
    assert [e[0] for e in ref[5]['events']] == [1, 17] and ref[5]['n_viable'] == 2                       # two events
    assert [e[0] for e in ref[6]['events']] == [n - 1] and ref[6]['n_viable'] == 1 and not ref[6]['collided']   # on the last step
    assert [e[0] for e in ref[7]['events']] == [n - 1] and ref[7]['collided'] and np.isnan(ref[7]['x'][n]).all()
    assert [e[0] for e in ref[8]['events']] == [sc.LEAVES] and ref[8]['n_viable'] == 1 and ref[8]['collided']   # event, then lost
    assert len(ref[9]['rest_tests']) >= Nb + 4 and not ref[9]['resumes']                                 # holds past Nb + 3
    assert margin >= 1e-6, margin
    # ---- the chained statements give the same run -----------------------------------------------------------------------------
    x, u = lc.blanked_logs(d)
    xo, uo = np.array([r['x'] for r in ref]), np.array([r['u'] for r in ref])
    assert np.array_equal(np.isnan(x), np.isnan(xo)), np.where(np.isnan(x).any(2) != np.isnan(xo).any(2))
    assert np.array_equal(np.isnan(u), np.isnan(uo)), np.where(np.isnan(u).any(2) != np.isnan(uo).any(2))
    # (same double arithmetic in the same order on both sides, the same plant: nothing but the batch size of the oracle's calls differs)
    assert np.nanmax(np.abs(x - xo)) < 1e-12 and np.nanmax(np.abs(u - uo)) < 1e-10 * (1 + np.nanmax(np.abs(uo)))
    assert np.array_equal(d['r_log'].T, np.array([r['r'] for r in ref]))
    assert sorted(events) == sorted((e[0], b) for b, r in enumerate(ref) for e in r['events'])
    assert d['collided'].astype(bool).tolist() == [r['collided'] for r in ref]
    assert d['viable'].tolist() == [r['n_viable'] for r in ref]
    assert (1 - d['alive']).tolist() == d['collided'].tolist()
    print(f'LOOPKERNELS host scenario quirks {int(quirks)}: {len(events)} events, margin {margin:.2e}, statement - oracle x '
          f'{np.nanmax(np.abs(x - xo)):.1e} u {np.nanmax(np.abs(u - uo)):.1e}')


def test_state_table_classes_give_their_branches():
    """the tables are what their class names say: the statement of loop_pre takes the branch the class was built for"""
    for nq in (5, 6):
        par, prob, net = make_problem('naive', 'ext', N=2, nq=nq)
        for Nb in (1, 2, 5):
            d, cls = lc.state_table(prob, Nb, 130, seed=nq)
            lc.check_table(d, cls, Nb)
