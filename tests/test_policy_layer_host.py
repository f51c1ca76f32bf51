"""The policy layer's host path after its split from the device path (safe_mpc_amd/controller.py ``_step_host``,
closed_loop._HostGroup): ``run_mpc`` through the scripted mirror of tests/test_policy_oracle.py returns, to the bit, what the
commit before the split returned (tests/golden/policy_layer_parent.npz, recorded there by tests/golden/make_policy_layer_parent.py,
which also defines the cases), and the misuse the split refuses."""
import importlib.util
import os

import numpy as np
import pytest

from fake_solver import OracleSolver, make_double_controller
from safe_mpc_amd import closed_loop as cl
from safe_mpc_amd import controller as C

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def load_recipe():
    spec = importlib.util.spec_from_file_location('make_policy_layer_parent', os.path.join(GOLDEN_DIR, 'make_policy_layer_parent.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def assert_recorded_bits(recipe, prefix, res):
    """x, u, r_receding, x_viable and the four outcome lists of ``res`` against the recording, bit for bit"""
    with np.load(recipe.GOLDEN) as gold:
        for key, got in recipe.pack(prefix, res).items():
            want = gold[key]
            assert got.shape == want.shape and got.dtype == want.dtype, (key, got.shape, want.shape, got.dtype, want.dtype)
            assert got.tobytes() == want.tobytes(), (key, int((got != want).sum()))


@pytest.mark.parametrize('kind', ['htwa', 'receding', 'real_receding'])
def test_host_loop_returns_the_bits_recorded_before_the_split(kind):
    recipe = load_recipe()
    res = recipe.run_host(kind)
    assert len(res['x_viable']) >= 1                                   # the abort branches ran
    assert_recorded_bits(recipe, f'h_{kind}', res)


def test_run_mpc_on_device_refuses_a_host_state_controller():
    import test_policy_oracle as tpo
    par = tpo._params()
    mk = lambda name, batch: make_double_controller(name, par, batch)       # device_state=False
    mkb = lambda batch: make_double_controller('backup', par, batch)
    xg, ug = np.zeros((2, par.N + 1, 12)), np.zeros((2, par.N, 6))
    with pytest.raises(ValueError, match='device_state'):
        cl.run_mpc(par, 'htwa', xg, ug, n_steps=2, make_controller=mk, make_backup=mkb, on_device=True)


def test_device_state_refuses_a_solver_without_the_policy_kernels():
    import test_policy_oracle as tpo
    par = tpo._params()
    probe = make_double_controller('htwa', par, 1)
    solver = OracleSolver(probe.problem, probe.net)
    with pytest.raises(ValueError, match='OracleSolver'):
        C.get_controller('htwa', par, 2, solver=solver, net=probe.net, device_state=True)
