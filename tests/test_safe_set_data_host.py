"""safe_mpc_amd/safe_set_data.py without a GPU: the labelling rule on a scripted solver, label_rays on the CPU oracle double (designed
rays, certificates), the fit and the checkpoint, and the exported symbol."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ray_cases as rc
from conftest import ROOT


# ---- 1. the statement on a scripted solver ------------------------------------------------------------------------------------------
class _ScriptedSolver:
    """An 'SQP' whose trial at speed s is feasible iff s <= s_star[ray], from the look ``looks[ray]`` on; an infeasible trial either
    never ends (the budget ends it) or, for the rays in ``quits``, reports done with status 4 at its second look."""

    def __init__(self, q, s_star, looks, quits, nq, N):
        self.q, self.s_star, self.looks, self.quits, self.nq, self.N = q, s_star, looks, quits, nq, N
        self.calls = 0

    def _ray(self, x0):
        return np.array([int(np.where((self.q == row[:self.nq]).all(1))[0][0]) for row in x0])

    def sqp(self, x0, xg, ug, p, opts, state):
        self.calls += 1
        xg, ug = xg.copy(), ug.copy()
        ray = self._ray(x0)
        s = np.linalg.norm(x0[:, self.nq:], axis=1)
        live = state['done'] == 0
        state['iters'][live] += opts['max_iter']
        looks = state['iters'] // opts['max_iter']
        ok = live & (s <= self.s_star[ray] * (1 + 1e-15)) & (looks >= self.looks[ray])
        xg[ok, -1, self.nq:] = 0.0                               # a feasible iterate ends at rest
        self.bad = live & ~ok
        quit_ = self.bad & self.quits[ray] & (looks >= 2) & ~(s <= self.s_star[ray] * (1 + 1e-15))
        state['status'][live] = 0
        state['status'][quit_] = 4
        state['done'][quit_] = 1
        return xg, ug, state

    def check_guess(self, x, u, safe_node=None, collision_first_node=None, mask=None):
        return np.where(self.bad, 8, 0).astype(np.int32), None


class _ScriptedCtrl:
    """the handful of attributes label_rays reads of a controller"""

    class _Np:
        on_device = False

    def __init__(self, solver, nq, N, tol_x=5e-3):
        from types import SimpleNamespace
        self.ocp_solver, self.nq, self.nu, self.N, self.B, self.xp = solver, nq, nq, N, 0, self._Np()
        self.params = SimpleNamespace(tol_x=tol_x, alpha=10.0)
        self._alloc()

    def _alloc(self):
        self.p = np.zeros((self.B, self.N + 1, 5))

    def reset_controller(self):
        pass


def _scripted_case():
    nq, N, n = 3, 2, 11
    rng = np.random.default_rng(0)
    q = rng.uniform(-1, 1, (n, nq))
    d = rng.standard_normal((n, nq))
    d /= np.linalg.norm(d, axis=1)[:, None]
    s_hi = rng.uniform(1.0, 3.0, n)
    s_star = s_hi * np.array([-0.5, -0.1, 1.5, 1.0001, 0.03, 0.37, 0.5, 0.81, 0.999, 0.64, 0.25])
    looks = np.array([1, 1, 1, 3, 1, 3, 1, 2, 1, 1, 3])
    quits = np.array([0, 1, 0, 0, 0, 0, 1, 0, 1, 0, 1], bool)
    return nq, N, q, d, s_hi, s_star, looks, quits


def _scripted_labels(batch, bisect=6, budget=12, every=5):
    from safe_mpc_amd import safe_set_data as sd
    nq, N, q, d, s_hi, s_star, looks, quits = _scripted_case()
    sv = _ScriptedSolver(q, s_star, looks, quits, nq, N)
    return sd.label_rays(_ScriptedCtrl(sv, nq, N), q, d, s_hi, bisect=bisect, budget=budget, check_every=every, batch=batch,
                         bookkeeping='statement')


@pytest.mark.parametrize('batch', [None, 5, 1])
def test_statement_on_a_scripted_solver(batch):
    """labels in [s_star - s_hi / 2^bisect, s_star], kinds and trial counts as specified, the same for every batch; an outcome that
    needs three looks is resolved at the third (15 iterations at check_every = 5); a trial that never becomes feasible ends at the
    budget rounded up (12 -> 15)"""
    from safe_mpc_amd import safe_set_data as sd
    nq, N, q, d, s_hi, s_star, looks, quits = _scripted_case()
    bisect, budget, every = 6, 12, 5
    res = _scripted_labels(batch, bisect, budget, every)
    dead, sat = s_star < 0, s_star >= s_hi
    mid = ~dead & ~sat
    assert np.array_equal(res['kind'], np.where(dead, sd.DEAD, np.where(sat, sd.SATURATED, sd.BRACKETED)))
    assert np.array_equal(res['trials'], np.where(dead, 1, np.where(sat, 2, bisect + 2)))
    assert np.all(np.isnan(res['label'][dead])) and np.array_equal(res['label'][sat], s_hi[sat])
    cell = s_hi / 2 ** bisect
    assert np.all(res['label'][mid] <= s_star[mid]) and np.all(res['label'][mid] >= s_star[mid] - cell[mid])
    assert np.all(res['hi'][mid] - res['lo'][mid] <= cell[mid] * (1 + 1e-12)) and np.array_equal(res['lo'][mid], res['label'][mid])
    # iterations: a feasible trial costs looks * every, an infeasible one the budget rounded up (15) or, where the solver quits, 2 looks
    for b in range(len(q)):
        s_tried = [0.0, s_hi[b]]
        lo, hi = 0.0, s_hi[b]
        want = 0
        for t in range(int(res['trials'][b])):
            s = s_tried[t] if t < 2 else 0.5 * (lo + hi)
            if s <= s_star[b]:
                want, lo = want + looks[b] * every, s
            else:
                want, hi = want + (2 * every if quits[b] else 15), s
        assert res['iters'][b] == want, (b, res['iters'][b], want)
    # a certificate starts at (q, label d) and ends at rest
    live = ~dead
    assert np.array_equal(res['x_cert'][live, 0], np.hstack([q[live], res['label'][live, None] * d[live]]))
    assert np.all(res['x_cert'][live, -1, nq:] == 0.0)
    if batch is not None:
        ref = _scripted_labels(None, bisect, budget, every)
        for k in ('label', 'kind', 'lo', 'hi', 'trials', 'iters', 'x_cert', 'u_cert'):
            assert np.array_equal(res[k], ref[k], equal_nan=True), k


def test_sample_rays():
    """collision-free Halton configurations in the box, unit directions, s_hi d on the velocity box; n_dof_safe_set < nq refused"""
    from oracle.oracle import Oracle
    from safe_mpc_amd import safe_set_data as sd
    from safe_mpc_amd.closed_loop import halton
    par, prob = rc.backup_problem()
    q, d, s_hi = sd.sample_rays(prob, 40, seed=2)
    nq = prob.nq
    assert q.shape == d.shape == (40, nq) and s_hi.shape == (40,)
    x = np.hstack([q, np.zeros_like(q)])
    assert np.all(Oracle(prob).check_trajectory(x[:, None, :], prob.x_min, prob.x_max, 0.0, prob.row_check[:, 0], prob.row_check[:, 1]))
    # the stream is the free points of the Halton sequence in order
    pts = prob.x_min[:nq] + halton(200, nq) * (prob.x_max[:nq] - prob.x_min[:nq])
    idx = [int(np.where(np.all(np.isclose(pts, row, rtol=0, atol=1e-15), axis=1))[0][0]) for row in q]
    assert idx == sorted(idx) and len(set(idx)) == 40
    assert np.allclose(np.linalg.norm(d, axis=1), 1.0, rtol=0, atol=1e-14)
    v = s_hi[:, None] * d
    worst = np.maximum(prob.x_min[nq:] - v, v - prob.x_max[nq:]).max(1)
    assert np.all(worst <= 1e-12) and np.all(worst >= -1e-12)
    q2, d2, _ = sd.sample_rays(prob, 40, seed=3)
    assert np.array_equal(q2, q) and not np.array_equal(d2, d)
    par3 = rc.ray_params()
    par3.n_dof_safe_set = 3
    from safe_mpc_amd.problem import OcpProblem
    with pytest.raises(ValueError, match='n_dof_safe_set'):
        sd.sample_rays(OcpProblem(par3, 'backup', 'zero', N=rc.N), 4, seed=0)


# ---- 2. / 3. label_rays on the oracle double -----------------------------------------------------------------------------------------
def test_designed_rays_on_the_oracle_double():
    """a ray pointing into a joint limit 0.01 rad away is labelled no faster than the ray pointing away from it, and clearly slower
    for the three proximal joints"""
    res = rc.host_labels('designed')
    print('kinds', res['kind'].tolist(), 'trials', res['trials'].tolist(), 'iters', res['iters'].tolist())
    rc.assert_designed_order(res)
    q, d, s_hi = rc.designed_rays()
    rc.assert_certificates(q, d, res)


def test_certificates_on_the_oracle_double():
    """every non-dead random ray comes with a trajectory that passes the checks recomposed from the oracle"""
    from safe_mpc_amd import safe_set_data as sd
    q, d, s_hi = rc.random_rays()
    res = rc.host_labels('random')
    kinds = [int((res['kind'] == k).sum()) for k in (sd.DEAD, sd.BRACKETED, sd.SATURATED)]
    print('random rays: dead, bracketed, saturated', kinds, 'labels', np.round(res['label'], 3).tolist())
    assert kinds == [0, 3, 13] and np.where(res['kind'] == sd.BRACKETED)[0].tolist() == rc.RANDOM_BRACKETED
    assert np.array_equal(res['label'][res['kind'] == sd.SATURATED], s_hi[res['kind'] == sd.SATURATED])
    rc.assert_certificates(q, d, res)


# ---- 4. the fit and the checkpoint ----------------------------------------------------------------------------------------------------
def _smooth_label(q, d):
    return 2.0 + 0.8 * np.sin(q[:, 0]) * d[:, 0] + 0.5 * np.cos(q[:, 1] + d[:, 1]) - 0.4 * d[:, 2] ** 2 + 0.3 * q[:, 3] * d[:, 4]


def _fit_data(n, seed):
    rng = np.random.default_rng(seed)
    q = rng.uniform(-2.0, 2.0, (n, rc.NQ))
    d = rng.standard_normal((n, rc.NQ))
    d /= np.linalg.norm(d, axis=1)[:, None]
    return {'q': q, 'd': d, 'label': _smooth_label(q, d), 'kind': np.full(n, 3, np.int32)}


def test_fit_and_checkpoint(tmp_path):
    import torch
    import yaml
    from safe_mpc_amd import safe_set_data as sd
    from safe_mpc_amd.parser import Parameters
    from safe_mpc_amd.safe_set import SafeSetNet
    par = rc.ray_params()
    train, held = _fit_data(2048, 0), _fit_data(512, 1)
    train['kind'][:7] = sd.DEAD                                  # dropped: their labels must not be read
    train['label'][:7] = np.nan
    net, mean, std, info = sd.fit_safe_set(train, par, epochs=40, seed=5, hidden=64)
    assert info['rays'] == 2041 and info['dropped'] == 7 and info['net_size'] == [12, 64, 1]
    assert np.allclose(mean, train['q'][7:].mean(0)) and np.allclose(std, train['q'][7:].std(0))
    rmse = np.sqrt(np.mean((sd.predict(net, mean, std, held['q'], held['d']) - held['label']) ** 2))
    base = np.sqrt(np.mean((train['label'][7:].mean() - held['label']) ** 2))
    print(f'held-out RMSE {rmse:.4f}, of predicting the training mean {base:.4f}, ratio {rmse / base:.3f}')
    assert rmse < base
    net2, _, _, _ = sd.fit_safe_set(train, par, epochs=40, seed=5, hidden=64)
    for a, b in zip(net.state_dict().values(), net2.state_dict().values()):
        assert torch.equal(a, b)
    # the checkpoint, through a config file whose network_path names it
    cfg = yaml.safe_load(open(os.path.join(ROOT, 'config.yaml')))
    for name, m, s in (('vec', mean, std), ('scalar', torch.tensor(0.25), torch.tensor(1.5))):
        path = str(tmp_path / f'{name}.pt')
        if name == 'vec':
            sd.save_checkpoint(path, net, m, s)
        else:
            torch.save({'model': net.state_dict(), 'mean': m, 'std': s}, path)
        cfg.update(network_path=path, network_size=[12, 64, 1], n_dofs=6, n_dof_safe_set=6, use_net=True)
        cfg_path = tmp_path / f'{name}.yaml'
        cfg_path.write_text(yaml.safe_dump(cfg))
        loaded = SafeSetNet.from_params(Parameters({}, 'z1', filename=str(cfg_path)))
        lin = [l for l in net.linear_stack if isinstance(l, torch.nn.Linear)]
        for l, w, b in zip(lin, loaded.weights, loaded.biases):
            assert np.array_equal(l.weight.detach().numpy(), w) and np.array_equal(l.bias.detach().numpy(), b)
        if name == 'vec':
            assert np.array_equal(loaded.mean, mean) and np.array_equal(loaded.std, std)
        else:
            assert np.array_equal(loaded.mean, np.full(6, 0.25)) and np.array_equal(loaded.std, np.full(6, 1.5))


def test_padded_hidden_units_change_nothing():
    """a hidden width the engine does not take (32) is padded with zero units to 256: value and input gradient of the padded net,
    through the CPU oracle's network, equal those of the net as given; a width it takes is handed on untouched"""
    import torch
    from safe_mpc_amd.safe_set import NeuralNetwork, SafeSetNet, activation
    from safe_mpc_amd.solver import pad_hidden_units
    for act in ('gelu', 'relu', 'elu', 'tanh', 'silu'):
        torch.manual_seed(3)
        net = SafeSetNet(NeuralNetwork(12, 32, 1, activation(act)), np.zeros(6), np.ones(6), act)
        Wp, bp = pad_hidden_units(net.weights, net.biases)
        assert [w.shape for w in Wp] == [(256, 12), (256, 256), (256, 256), (1, 256)]
        big = NeuralNetwork(12, 256, 1, activation(act))
        lin = [m for m in big.linear_stack if isinstance(m, torch.nn.Linear)]
        with torch.no_grad():
            for m, w, b in zip(lin, Wp, bp):
                m.weight.copy_(torch.as_tensor(w))
                m.bias.copy_(torch.as_tensor(b))
        s = np.random.default_rng(0).standard_normal((9, 12)).astype(np.float32)
        y0, g0 = net.torch_value_and_grad(s)
        y1, g1 = SafeSetNet(big, np.zeros(6), np.ones(6), act).torch_value_and_grad(s)
        assert np.allclose(y1, y0, rtol=0, atol=1e-6) and np.allclose(g1, g0, rtol=0, atol=1e-6), act
    W64 = [np.zeros((64, 12), np.float32), np.zeros((64, 64), np.float32), np.zeros((1, 64), np.float32)]
    assert pad_hidden_units(W64, [None] * 3)[0] is W64


# ---- 5. the exported symbol ----------------------------------------------------------------------------------------------------------
def test_library_exports_smpc_ray_update():
    from safe_mpc_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    hdr = open(os.path.join(ROOT, 'include', 'smpc.h')).read()
    declared = set(re.findall(r'^(?:int|void|void\*|const char\*)\s+(smpc_[a-z_]+)\s*\(', hdr, re.M))
    assert 'smpc_ray_update' in declared and 'smpc_ray_update' in _lib.SYMBOLS
    assert hasattr(C.CDLL(_lib.LIB_PATH), 'smpc_ray_update')
    assert C.sizeof(_lib.RayOpts) == 24 and C.sizeof(_lib.RayState) == 11 * 8
