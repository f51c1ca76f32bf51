"""Everything a run can set on its two solver handles at once -- scene track, forecast of degree 2 from an observed track, row margin,
scores -- on the host path, against tests/golden/loop_world_parent.npz: the results and the calls both handles received at the
commit before the closed loop got one owner for them (tests/golden/make_loop_world_parent.py is the recipe and defines the cases).
The tests of each feature alone pin its calls; this one pins their order when they come together."""
import importlib.util
import os

import numpy as np
import pytest

_spec = importlib.util.spec_from_file_location('make_loop_world_parent', os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden',
                                                                                     'make_loop_world_parent.py'))
recipe = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(recipe)


@pytest.fixture(scope='module')
def golden():
    with np.load(recipe.GOLDEN) as z:
        return {key: z[key] for key in z.files}


@pytest.mark.parametrize('case', recipe.HOST_CASES)
def test_host_loop_equals_the_parent_in_results_and_calls(golden, case):
    got = recipe.pack_host(case)
    want = {key: v for key, v in golden.items() if key.startswith(f'h_{case}_')}
    assert set(got) == set(want) and len(got[f'h_{case}_x_viable']) >= 1
    for name in recipe.HANDLES:        # the first call that differs says more than "not equal"
        a, b = got[f'h_{case}_{name}_events'].tolist(), want[f'h_{case}_{name}_events'].tolist()
        first = next((k for k, (ea, eb) in enumerate(zip(a, b)) if ea != eb), min(len(a), len(b)))
        assert a == b, f'{name}: {len(a)} calls against {len(b)}, call {first}: {a[first:first + 1]} against {b[first:first + 1]}'
    for key in sorted(want):
        assert recipe.same_bits(got[key], want[key]), key
    if case == 'all':
        assert got['h_all_keys'].tolist() == ["forecast='fit'", 'forecast_degree=2', 'forecast_window=3', 'observed=True',
                                              f'row_margin={recipe.HOST_MARGIN!r}']
        assert any(e.startswith('row_bounds float64') for e in got['h_all_backup_events'].tolist())       # the backup handle's path ran
    else:
        assert got['h_scenes_keys'].size == 0
