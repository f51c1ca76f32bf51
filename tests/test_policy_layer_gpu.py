"""The policy layer's device path after its split from the host path (closed_loop._DeviceGroup): ``run_mpc(on_device=True,
groups=1)`` returns, to the bit, what the commit before the split returned on an MI355X (tests/golden/policy_layer_parent.npz,
recorded there twice in separate processes by tests/golden/make_policy_layer_parent.py --device, which also defines the cases) --
with graph replay, where each half of a step is now captured once instead of a second time after the first abort event, and
with eager launches.  -m gpu only."""
import pytest

from test_policy_layer_host import assert_recorded_bits, load_recipe

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('graphs', [True, False], ids=['graphs', 'eager'])
@pytest.mark.parametrize('name', ['receding', 'real_receding', 'parallel'])
def test_device_loop_returns_the_bits_recorded_before_the_split(name, graphs):
    recipe = load_recipe()
    res = recipe.run_device(name, graphs=graphs)
    if name == 'receding':
        assert len(res['x_viable']) >= 1                               # abort events occur in this fixture
    assert_recorded_bits(recipe, f'd_{name}', res)
