"""The device loop with a fit of observations, a row margin and scores together, with graph replay and with eager launches, against
tests/golden/loop_world_parent.npz: what the commit before the closed loop got one owner for what a run sets on its handles
computed, bit for bit (tests/golden/make_loop_world_parent.py is the recipe and defines the case)."""
import importlib.util
import os

import numpy as np
import pytest

_spec = importlib.util.spec_from_file_location('make_loop_world_parent', os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden',
                                                                                     'make_loop_world_parent.py'))
recipe = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(recipe)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('graphs', [True, False], ids=['graphs', 'eager'])
def test_device_loop_equals_the_parent_bit_for_bit(graphs):
    with np.load(recipe.GOLDEN) as z:
        want = {key: z[key] for key in z.files if key.startswith('d_')}
    margin = tuple(want.pop('d_row_margin').tolist())
    res = recipe.run_device(graphs, margin)
    assert res['row_margin'] == margin and res['forecast'] == 'fit' and res['forecast_window'] == 4 and res['observed'] is True
    got = recipe.pack('d', res)
    assert set(got) == set(want) and len(got['d_x_viable']) >= 1
    for key in sorted(want):
        assert recipe.same_bits(got[key], want[key]), key
