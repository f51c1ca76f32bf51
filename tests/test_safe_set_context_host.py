"""A safe-set network with a per-instance context: the host side -- SafeSetNet.folded against a torch
forward pass on the stacked input, the checkpoint keys, the fit's extra inputs, label_rays(scenes=...) on a recording fake solver,
scene_context / context_default and the refusals.  No GPU."""
import types

import numpy as np
import pytest
import torch

import context_cases as cc
from conftest import make_problem


def _stacked_value_and_grad(net, s_state, ctx):
    """fp32 torch forward / autograd of the net with context on [s_state | (ctx - mean) / std]: (y [n], dy/ds_state [n, 2 nq])"""
    cn = (np.asarray(ctx, float) - net.ctx_mean) / net.ctx_std
    s = np.hstack([s_state, np.broadcast_to(cn, (len(s_state), net.n_ctx))])
    y, g = net.torch_value_and_grad(s)
    return y, g[:, :s_state.shape[1]]


@pytest.mark.parametrize('act', ['gelu', 'tanh'])
def test_folded_equals_the_stacked_forward_pass(act):
    from safe_mpc_amd.safe_set import SafeSetNet
    par, prob, _ = make_problem('st', N=4, act=act)
    net = cc.context_net(prob, par, n_ctx=3, seed=5, hidden=64)
    net = SafeSetNet(net.model, net.mean, net.std, act, ctx_mean=[0.2, -0.1, 0.4], ctx_std=[0.5, 2.0, 1.5], ctx_select=[(0, 0), (0, 1), (2, 6)])
    assert net.n_ctx == 3 and net.dims[0] == 15 and net.ctx_select == [(0, 0), (0, 1), (2, 6)]
    s = np.random.default_rng(0).standard_normal((40, 12))
    for ctx in ([0.3, -0.2, 0.1], [-1.0, 2.0, 0.7]):
        f = net.folded(ctx)
        assert f.n_ctx == 0 and f.dims == [12, 64, 64, 64, 1] and f.act == act
        assert np.array_equal(f.weights[0], net.weights[0][:, :12]) and all(np.array_equal(a, b) for a, b in zip(f.weights[1:], net.weights[1:]))
        b0 = net.biases[0].astype(np.float64) + net.weights[0][:, 12:].astype(np.float64) @ ((np.array(ctx) - net.ctx_mean) / net.ctx_std)
        assert np.array_equal(f.biases[0], b0.astype(np.float32))
        y, g = _stacked_value_and_grad(net, s, ctx)
        yf, gf = f.torch_value_and_grad(s)
        # fp32 rounding: the fold moves H products per unit from the fp32 sum into the bias (eps = 6e-8, values O(1))
        assert np.abs(y - yf).max() < 2e-5 * (1 + np.abs(y).max()) and np.abs(g - gf).max() < 2e-5 * (1 + np.abs(g).max())
    assert np.abs(net.folded([0.3, -0.2, 0.1]).torch_value_and_grad(s)[0] - net.folded([-1.0, 2.0, 0.7]).torch_value_and_grad(s)[0]).max() > 1e-3
    with pytest.raises(ValueError, match='context numbers'):
        net.folded([1.0])


def test_synthetic_net_with_context_inputs_and_plain_net_unchanged():
    par, prob, plain = make_problem('st', N=4)
    assert plain.n_ctx == 0 and plain.ctx_select == [] and plain.ctx_mean.size == 0
    net = cc.context_net(prob, par)
    assert net.n_ctx == cc.N_CTX and np.array_equal(net.ctx_mean, np.zeros(4)) and np.array_equal(net.ctx_std, np.ones(4))
    assert np.array_equal(net.mean, plain.mean) and np.array_equal(net.std, plain.std)
    again = cc.context_net(prob, par)
    assert all(np.array_equal(a, b) for a, b in zip(net.weights, again.weights))
    # a plain net folds to itself
    f = plain.folded([])
    assert all(np.array_equal(a, b) for a, b in zip(f.weights + f.biases, plain.weights + plain.biases))


def _fit_data(n=24, seed=3):
    from safe_mpc_amd import safe_set_data as sd
    rng = np.random.default_rng(seed)
    q, d = rng.uniform(-1, 1, (n, 6)), rng.standard_normal((n, 6))
    d /= np.linalg.norm(d, axis=1)[:, None]
    kind = np.where(np.arange(n) % 7 == 0, sd.DEAD, sd.BRACKETED)
    label = np.where(kind == sd.DEAD, np.nan, rng.uniform(0.5, 2.0, n))
    return {'q': q, 'd': d, 'label': label, 'kind': kind}, rng.uniform(-0.3, 0.3, (n, 2))


def test_checkpoint_round_trip(tmp_path):
    from safe_mpc_amd import safe_set_data as sd
    from safe_mpc_amd.parser import Parameters
    from safe_mpc_amd.safe_set import SafeSetNet
    data, ctx = _fit_data()
    par = Parameters({}, 'z1')
    par.net_size = [14, 32, 1]
    net, mean, std, info = sd.fit_safe_set(data, par, epochs=2, seed=1, context=ctx)
    keep = data['kind'] != sd.DEAD
    assert np.array_equal(info['ctx_mean'], ctx[keep].mean(0)) and np.array_equal(info['ctx_std'], ctx[keep].std(0))
    sel = [(0, 1), (1, 4)]
    path = str(tmp_path / 'ctx.pt')
    sd.save_checkpoint(path, net, mean, std, info['ctx_mean'], info['ctx_std'], sel)
    load = Parameters({}, 'z1')           # (the parser sets net_size[0] = 2 nq: the context inputs come from the checkpoint)
    load.net_size, load.net_path = [12, 32, 1], path
    got = SafeSetNet.from_params(load)
    assert got.n_ctx == 2 and got.ctx_select == sel and got.dims == [14, 32, 32, 32, 1]
    assert np.array_equal(got.ctx_mean, info['ctx_mean']) and np.array_equal(got.ctx_std, info['ctx_std'])
    assert np.array_equal(got.mean, mean) and np.array_equal(got.std, std)
    want = [p.detach().numpy() for p in net.parameters()]
    assert all(np.array_equal(a, b) for a, b in zip(got.weights, want[0::2])) and all(np.array_equal(a, b) for a, b in zip(got.biases, want[1::2]))
    # predict with the normalised context is the net's forward pass; the dataset keeps the raw context
    cn = (ctx - info['ctx_mean']) / info['ctx_std']
    y = sd.predict(net, mean, std, data['q'], data['d'], ctx=cn)
    y2, _ = got.torch_value_and_grad(np.hstack([(data['q'] - mean) / std, data['d'], cn]))
    assert np.array_equal(y.astype(np.float32), y2)
    sd.save_dataset(str(tmp_path / 'rays.npz'), data['q'], data['d'], np.ones(len(ctx)), dict(data, trials=np.zeros(len(ctx), np.int32)), ctx=ctx)
    assert np.array_equal(np.load(str(tmp_path / 'rays.npz'))['ctx'], ctx)
    with pytest.raises(ValueError, match='go together'):
        sd.save_checkpoint(path, net, mean, std, info['ctx_mean'])
    # a checkpoint without the new keys loads as before
    par.net_size = [12, 32, 1]
    plain, m2, s2, _ = sd.fit_safe_set(data, par, epochs=1, seed=1)
    sd.save_checkpoint(path, plain, m2, s2)
    assert sorted(torch.load(path, map_location='cpu')) == ['mean', 'model', 'std']
    got = SafeSetNet.from_params(load)
    assert got.n_ctx == 0 and got.ctx_select == [] and got.dims == [12, 32, 32, 32, 1]
    assert np.array_equal(got.weights[0], plain.linear_stack[0].weight.detach().numpy())


def test_fit_without_context_is_the_parent_procedure_bit_for_bit():
    """the weights of fit_safe_set(seed) without ``context`` against the procedure as it stood before the keyword existed, restated
    here: same seed, same draws, same mini-batches"""
    from safe_mpc_amd import safe_set_data as sd
    from safe_mpc_amd.parser import Parameters
    from safe_mpc_amd.safe_set import NeuralNetwork, activation
    data, ctx = _fit_data()
    par = Parameters({}, 'z1')
    par.net_size = [12, 32, 1]
    seed, epochs, bs = 4, 3, 8
    net, mean, std, info = sd.fit_safe_set(data, par, epochs, seed, batch_size=bs)
    keep = data['kind'] != sd.DEAD
    q, d, y = data['q'][keep], data['d'][keep], data['label'][keep]
    m, s = q.mean(0), q.std(0)
    s = np.where(s > 0.0, s, 1.0)
    torch.manual_seed(seed)
    ref = NeuralNetwork(12, 32, 1, activation(par.act)).float()
    with torch.no_grad():
        ref.linear_stack[-1].bias.fill_(float(y.mean()))
    X = torch.as_tensor(np.hstack([(q - m) / s, d]), dtype=torch.float32)
    Y = torch.as_tensor(y, dtype=torch.float32)
    opt = torch.optim.Adam(ref.parameters(), lr=3e-3)
    gen = torch.Generator().manual_seed(seed)
    for _ in range(epochs):
        order = torch.randperm(len(X), generator=gen)
        for lo in range(0, len(X), bs):
            idx = order[lo:lo + bs]
            opt.zero_grad()
            loss = torch.mean((ref(X[idx]).reshape(-1) - Y[idx]) ** 2)
            loss.backward()
            opt.step()
    assert np.array_equal(mean, m) and np.array_equal(std, s) and 'ctx_mean' not in info
    for a, b in zip(net.parameters(), ref.parameters()):
        assert torch.equal(a, b)
    # with a context: other inputs, and the input width is checked
    with pytest.raises(ValueError, match='14 inputs'):
        sd.fit_safe_set(data, par, 1, seed, context=ctx)
    with pytest.raises(ValueError, match='context'):
        sd.fit_safe_set(data, par, 1, seed, context=ctx[:5])


class _RecordingSolver:
    def __init__(self):
        self.calls = []

    def set_instance_scene(self, geom=None):
        self.calls.append(None if geom is None else np.array(geom))


def _stub_controller(solver, nq=6, N=3):
    c = types.SimpleNamespace(nq=nq, N=N, nu=nq, B=0, ocp_solver=solver, xp=types.SimpleNamespace(on_device=False))
    c._alloc = lambda: None
    c.reset_controller = lambda: None
    return c


def test_label_rays_sets_each_chunks_padded_scenes_and_clears_them(monkeypatch):
    from safe_mpc_amd import safe_set_data as sd
    n, B = 5, 2
    rng = np.random.default_rng(0)
    q, d, s_hi = rng.standard_normal((n, 6)), rng.standard_normal((n, 6)), np.ones(n)
    scenes = rng.standard_normal((n, 3, 8))
    seen = []

    def chunk(ctrl, rays, n_live, *a):
        seen.append((len(ctrl.ocp_solver.calls), n_live))
        assert ctrl.ocp_solver.calls[-1] is not None              # the scene is on while the chunk runs
        rays['open'][:] = 0
        rays['kind'][:] = sd.DEAD
        return 1
    monkeypatch.setattr(sd, '_label_chunk_statement', chunk)
    sv = _RecordingSolver()
    res = sd.label_rays(_stub_controller(sv), q, d, s_hi, batch=B, bookkeeping='statement', scenes=scenes)
    assert res['rounds'] == 3 and seen == [(1, 2), (3, 2), (5, 1)]
    sets, clears = sv.calls[0::2], sv.calls[1::2]
    assert all(c is None for c in clears) and len(sv.calls) == 6
    assert np.array_equal(sets[0], scenes[0:2]) and np.array_equal(sets[1], scenes[2:4])
    assert np.array_equal(sets[2], np.stack([scenes[4], scenes[4]]))           # the last chunk: padded like q, with its first ray
    # a round that raises: the scene is cleared all the same
    sv = _RecordingSolver()

    def boom(*a):
        raise RuntimeError('round failed')
    monkeypatch.setattr(sd, '_label_chunk_statement', boom)
    with pytest.raises(RuntimeError, match='round failed'):
        sd.label_rays(_stub_controller(sv), q, d, s_hi, batch=B, bookkeeping='statement', scenes=scenes)
    assert len(sv.calls) == 2 and sv.calls[0] is not None and sv.calls[1] is None
    # without scenes the solver's scene is not touched
    sv = _RecordingSolver()
    monkeypatch.setattr(sd, '_label_chunk_statement', lambda ctrl, rays, *a: rays['open'].fill(0) or 1)
    sd.label_rays(_stub_controller(sv), q, d, s_hi, batch=B, bookkeeping='statement')
    assert sv.calls == []
    # refusals
    with pytest.raises(ValueError, match='has no set_instance_scene'):
        sd.label_rays(_stub_controller(object()), q, d, s_hi, bookkeeping='statement', scenes=scenes)
    with pytest.raises(ValueError, match='scenes'):
        sd.label_rays(_stub_controller(_RecordingSolver()), q, d, s_hi, bookkeeping='statement', scenes=scenes[:3])


def test_scene_context_and_context_default_pick_the_named_fields():
    from safe_mpc_amd.problem import jittered_scenes, scene_context
    par, prob, _ = make_problem('st', N=4)
    geom = jittered_scenes(prob, 5, 0.05, seed=2)
    sel = [(0, 1), (2, 6), (1, 3)]
    c = scene_context(geom, sel)
    assert c.shape == (5, 3) and c.flags['C_CONTIGUOUS']
    assert np.array_equal(c, np.stack([geom[:, 0, 1], geom[:, 2, 6], geom[:, 1, 3]], axis=1))
    g0 = prob.row_geometry()
    assert np.array_equal(prob.context_default(sel), [g0[0, 1], g0[2, 6], g0[1, 3]])
    assert scene_context(geom, []).shape == (5, 0)
    with pytest.raises(ValueError, match='outside'):
        scene_context(geom, [(len(prob.rows), 0)])
    with pytest.raises(ValueError, match='outside'):
        scene_context(geom, [(0, 8)])
    with pytest.raises(ValueError, match='expected'):
        scene_context(geom[0], sel)


class _ContextSolver(_RecordingSolver):
    def __init__(self, net):
        super().__init__()
        self.net, self.ctx = net, []

    def set_instance_scene_track(self, geom=None):
        self.calls.append(geom)

    def set_instance_context(self, ctx=None):
        self.ctx.append(None if ctx is None else np.array(ctx))


def test_scenes_carry_the_context_onto_the_solver_and_a_track_is_refused():
    from safe_mpc_amd import closed_loop as cl
    from safe_mpc_amd.problem import jittered_scenes, scene_context
    from safe_mpc_amd.safe_set import SafeSetNet
    par, prob, plain = make_problem('st', N=4)
    base = cc.context_net(prob, par, n_ctx=2)
    sel = [(0, 0), (1, 2)]
    net = SafeSetNet(base.model, base.mean, base.std, base.act, np.zeros(2), np.ones(2), sel)
    geom = jittered_scenes(prob, 3, 0.05, seed=1)
    sv = _ContextSolver(net)
    cl._set_scene(sv, geom)
    assert np.array_equal(sv.calls[-1], geom) and np.array_equal(sv.ctx[-1], scene_context(geom, sel))
    cl._set_scene(sv, geom[:, None])                       # a track of one column is a scene
    assert np.array_equal(sv.ctx[-1], scene_context(geom, sel))
    cl._set_scene(sv, None)
    assert sv.calls[-1] is None and sv.ctx[-1] is None
    cl._clear_scene(sv)
    assert sv.ctx[-1] is None and len(sv.ctx) == 4
    n_calls = len(sv.calls)
    with pytest.raises(ValueError, match='moves along a track'):
        cl._set_scene(sv, np.repeat(geom[:, None], 2, axis=1))
    assert len(sv.calls) == n_calls                        # refused before anything was set
    # a net with a context that does not say where it comes from; a plain net sets no context
    with pytest.raises(ValueError, match='ctx_select'):
        cl._set_scene(_ContextSolver(base), geom)
    sv = _ContextSolver(plain)
    cl._set_scene(sv, geom)
    assert sv.ctx == [] and len(sv.calls) == 1


def test_new_entry_points_are_declared_and_exported():
    import ctypes
    import os
    import re
    from safe_mpc_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, 'include', 'smpc.h')).read()
    declared = set(re.findall(r'^(?:int|void|const char\*|void\*) (smpc_\w+)\(', hdr, re.M))
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('smpc_set_mlp_context', 'smpc_set_instance_context'):
        assert name in declared and name in _lib.SYMBOLS and hasattr(L, name), name
