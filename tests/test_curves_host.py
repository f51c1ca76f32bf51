"""A reference curve of its own for every instance, without a GPU: the batched generators of tracking.py against the reference's
golden and the scalar generators, the host controller's gather, the score's statement, run_mpc on the host path through the CPU
oracle, and the entry scripts' options.  Shapes and patterns are curve_cases.py's."""
import copy
import os
import types

import numpy as np
import pytest

import curve_cases as cc
from conftest import ROOT, sample_instances
from fake_solver import make_double_controller


# ---- the generators ----------------------------------------------------------------------------------------------------------------
def _golden_params(g, vel_const):
    p = types.SimpleNamespace(vel_const=vel_const)
    for k in g.files:
        if k.startswith('in_'):
            v = g[k]
            setattr(p, k[3:], v if v.ndim else v.item())
    return p


@pytest.mark.parametrize('curve,name', [('8', 'eight'), ('circle', 'circle')])
@pytest.mark.parametrize('tag', ['const', 'ramp'])
def test_tracking_curves_equal_the_reference_generators(curve, name, tag):
    """without overrides, B = 2: both instances are the golden the reference's own generators wrote, at the 1e-10 test_ik_host.py
    holds tracking.py to"""
    from safe_mpc_amd.tracking import tracking_curves
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'tracking_ref.npz'))
    p = _golden_params(g, tag == 'const')
    ours = tracking_curves(p, curve, B=2)
    ref = g[f'{name}_{tag}']
    assert ours.shape == (2,) + ref.shape
    print(curve, tag, 'max abs difference', np.abs(ours - ref[None]).max())
    assert np.abs(ours - ref[None]).max() <= 1e-10
    assert p.n_steps == int(p.n_steps_tracking) and p.track_traj is True


@pytest.mark.parametrize('curve', ['8', 'circle'])
@pytest.mark.parametrize('vel_const', [True, False])
def test_overrides_equal_the_scalar_generator_on_changed_keys(curve, vel_const):
    """instance b = tracking_trajectory on a copy of the parameters with b's keys, 1e-10; the circle's instances include one that
    turns round inside the table and a ramp that ends inside it"""
    from safe_mpc_amd.tracking import tracking_curves, tracking_trajectory
    par = cc.params(vel_const=vel_const, acc_time=0.5, n_steps_tracking=40)
    B = 4
    rng = np.random.default_rng(1)
    eight = curve == '8'
    off = np.asarray(par.offset_traj if eight else par.circle_offset_traj, float) + rng.normal(0, 0.05, (B, 3))
    size = float(par.dim_shape_8 if eight else par.circle_rad) * np.array([1.0, 1.3, 0.7, 1.1])
    vmax = np.array([0.3, 0.5, 0.1, 0.9])
    rot = np.asarray(par.theta_rot_traj, float) + rng.normal(0, 0.3, (B, 3))
    if not eight:
        off[1, 1] = -0.49             # this one passes y = -0.5 and turns
    got = tracking_curves(par, curve, offsets=off, sizes=size, v_max=vmax, rotations=rot if eight else None)
    assert got.shape == (B, 3, 40 + 1 + cc.N)
    for b in range(B):
        pb = copy.deepcopy(par)
        if eight:
            pb.offset_traj, pb.dim_shape_8, pb.vel_max_traj, pb.theta_rot_traj = off[b], size[b], vmax[b], rot[b]
        else:
            pb.circle_offset_traj, pb.circle_rad, pb.circle_traj_vel = off[b], size[b], vmax[b]
        ref = tracking_trajectory(pb, curve)
        print(curve, vel_const, b, np.abs(got[b] - ref).max())
        assert np.abs(got[b] - ref).max() <= 1e-10
    assert np.abs(got[0] - got[1]).max() > 1e-2
    if not eight:
        assert (got[1, 1] < -0.5).any() and not (got[0, 1] < -0.5).any()         # (instance 1 turns round, instance 0 does not)
    with pytest.raises(ValueError):
        tracking_curves(par, curve, offsets=off, sizes=size[:3])
    if not eight:
        with pytest.raises(ValueError, match='8'):
            tracking_curves(par, curve, rotations=rot)


@pytest.mark.parametrize('curve', ['8', 'circle'])
def test_jittered_curves(curve):
    from safe_mpc_amd.tracking import jittered_curves, tracking_curves, tracking_trajectory
    par = cc.params()
    a = jittered_curves(par, curve, 5, 0.02, seed=4, scale_sigma=0.1)
    assert a.shape == (5, 3, cc.L) and np.array_equal(a, jittered_curves(par, curve, 5, 0.02, seed=4, scale_sigma=0.1))
    assert not np.array_equal(a, jittered_curves(par, curve, 5, 0.02, seed=5, scale_sigma=0.1))
    assert not np.array_equal(a[0], a[1])
    plain = tracking_trajectory(cc.params(), curve)
    assert np.array_equal(jittered_curves(par, curve, 3, 0.0), np.repeat(plain[None], 3, axis=0))
    # the offsets do not depend on whether the size is jittered: the first column's centre of the unscaled run is where the draws
    # put it, and the draws are those of the documented order (three for the offset, one for the size, instance by instance)
    rng = np.random.default_rng(4)
    draws = rng.normal(0.0, 1.0, (5, 4))
    eight = curve == '8'
    base = np.asarray(par.offset_traj if eight else par.circle_offset_traj, float)
    size = float(par.dim_shape_8 if eight else par.circle_rad)
    want = tracking_curves(par, curve, offsets=base + 0.02 * draws[:, :3], sizes=size * np.exp(0.1 * draws[:, 3]))
    assert np.array_equal(a, want)
    unscaled = jittered_curves(par, curve, 5, 0.02, seed=4)
    assert np.array_equal(unscaled, tracking_curves(par, curve, offsets=base + 0.02 * draws[:, :3], sizes=np.full(5, size)))


# ---- the controller ------------------------------------------------------------------------------------------------------------------
def test_apply_traj_gathers_every_instances_own_columns():
    B = 13
    par = cc.params()
    ctrl = make_double_controller('naive', par, B)
    curves, cs, stp = cc.dealt(B), cc.current_steps(B), cc.stepping(B)
    ctrl.setTrajectory(curves)
    assert ctrl.traj.shape == (B, 3, cc.L)
    ctrl.current_step = cs.copy()
    ctrl.p[:, :, 3:] = np.random.default_rng(0).normal(size=(B, cc.N + 1, 2))
    before = ctrl.p.copy()
    ctrl._apply_traj()
    want = cc.p_statement(curves, cs)
    assert np.array_equal(ctrl.p[:, :, :3], want) and np.array_equal(ctrl.p[:, :, 3:], before[:, :, 3:])
    assert np.array_equal(ctrl.p[1, :, :3], curves[1][:, :cc.N + 1].T)                       # current_step 0
    assert np.array_equal(ctrl.p[B - 1, :, :3], np.repeat(curves[B - 1][:, -1:].T, cc.N + 1, axis=0))   # past the end: last column
    for b in range(B):
        for i in range(cc.N + 1):
            assert np.array_equal(ctrl.p[b, i, :3], curves[b, :, min(cs[b] + i, cc.L - 1)])
    # rows: the others keep their p
    ctrl.p[...] = before
    ctrl._apply_traj(rows=stp)
    assert np.array_equal(ctrl.p[stp][:, :, :3], want[stp]) and np.array_equal(ctrl.p[~stp], before[~stp])
    assert np.array_equal(ctrl.p[:, :, 3:], before[:, :, 3:])
    # in place for the same shape (a captured step keeps its pointer), rebound for another
    held = ctrl.traj
    ctrl._traj_rebound = False
    ctrl.setTrajectory(curves + 0.01)
    assert ctrl.traj is held and not ctrl._traj_rebound and np.array_equal(ctrl.traj, curves + 0.01)
    ctrl.setTrajectory(curves[0])
    assert ctrl.traj.shape == (3, cc.L) and ctrl._traj_rebound
    ctrl.current_step = cs.copy()
    ctrl._apply_traj()
    assert np.array_equal(ctrl.p[:, :, :3], cc.p_statement(np.repeat(curves[:1], B, axis=0), cs))
    ctrl.setTrajectory(None)
    assert ctrl.traj is None and np.all(ctrl.p[:, :, :3] == ctrl.problem.ee_ref)


def test_set_trajectory_refuses_other_shapes():
    B = 5
    ctrl = make_double_controller('naive', cc.params(), B)
    curves = cc.dealt(B)
    with pytest.raises(ValueError, match=r'\[5, 3, n_columns\]'):
        ctrl.setTrajectory(curves[:4])
    with pytest.raises(ValueError):
        ctrl.setTrajectory(curves[:, :2])
    with pytest.raises(ValueError):
        ctrl.setTrajectory(curves[None])
    with pytest.warns(RuntimeWarning, match='columns'):
        ctrl.setTrajectory(curves[:, :, :cc.N])          # shorter than n_steps + 1 + N: held at the last column, and said so
    assert ctrl.traj.shape == (B, 3, cc.N)


# ---- the score ---------------------------------------------------------------------------------------------------------------------
def test_score_statement_with_a_curve_per_instance():
    from safe_mpc_amd import closed_loop as cl
    B, T = 13, 6
    par = cc.params()
    ctrl = make_double_controller('naive', par, B)
    prob, sv = ctrl.problem, ctrl.ocp_solver
    rng = np.random.default_rng(2)
    x = np.stack([sample_instances(prob, B, seed=s, vel_scale=0.2) for s in range(T + 1)])
    u = rng.normal(size=(T, B, 6))
    lx = np.array([T, T, 3, T, 0, T, T, 5, T, T, 2, T, T], np.int64)
    lu = np.minimum(lx, T - 1)
    curves = cc.dealt(B)[:, :, :4]                       # shorter than the log: column min(j, L - 1)
    out, outi = cl.score_rollout_statement(sv, prob, par, x, u, lx, lu, traj=curves)
    for b in range(B):
        ob, oib = cl.score_rollout_statement(sv, prob, par, x, u, lx, lu, traj=curves[b])
        assert np.array_equal(out[b], ob[b]) and np.array_equal(outi[b], oib[b]), b
    one, _ = cl.score_rollout_statement(sv, prob, par, x, u, lx, lu, traj=curves[0])
    assert np.all(one[cc.owner(B) != 0, 1] != out[cc.owner(B) != 0, 1])
    with pytest.raises(ValueError, match='traj'):
        cl.score_rollout_statement(sv, prob, par, x, u, lx, lu, traj=curves[:12])


# ---- the closed loop and the warm starts ---------------------------------------------------------------------------------------------
def test_run_mpc_on_two_curves_equals_the_per_curve_runs():
    """2 curves x 2 instances interleaved, 'naive', 6 steps on the host path through the CPU oracle: instance for instance the two
    single-curve runs (same oracle, so to the bit), scores included; in two groups too"""
    from safe_mpc_amd import closed_loop as cl
    steps, B = 6, 4
    par = cc.params()
    mk = lambda name, batch: make_double_controller(name, par, batch)        # noqa: E731
    mkb = lambda batch: make_double_controller('backup', par, batch)        # noqa: E731
    prob = mk('naive', 1).problem
    x0 = sample_instances(prob, B, seed=5, vel_scale=0.1)
    xg, ug = np.repeat(x0[:, None, :], cc.N + 1, axis=1), np.zeros((B, cc.N, 6))
    own = np.array([0, 1, 0, 1])
    curves = np.ascontiguousarray(cc.three_curves()[own])
    res = cl.run_mpc(par, 'naive', xg, ug, make_controller=mk, make_backup=mkb, n_steps=steps, score=True, traj=curves)
    parts = [cl.run_mpc(par, 'naive', xg[own == c], ug[own == c], make_controller=mk, make_backup=mkb, n_steps=steps, score=True,
                        traj=cc.three_curves()[c]) for c in (0, 1)]
    for c in (0, 1):
        for key in ('x', 'u'):
            assert np.array_equal(res[key][own == c], parts[c][key], equal_nan=True), (c, key)
        for key, val in res['score'].items():
            assert np.array_equal(val[own == c], parts[c]['score'][key]), (c, key)
    assert not np.array_equal(parts[0]['u'], parts[1]['u'])
    # ... and the curve matters: instance 1 on curve 0 is another run
    assert not np.array_equal(res['u'][1], cl.run_mpc(par, 'naive', xg[1:2], ug[1:2], make_controller=mk, make_backup=mkb, n_steps=steps,
                                                      traj=cc.three_curves()[0])['u'][0])
    two = cl.run_mpc(par, 'naive', xg, ug, make_controller=mk, make_backup=mkb, n_steps=steps, score=True, traj=curves, groups=2)
    assert np.array_equal(two['x'], res['x'], equal_nan=True) and np.array_equal(two['score']['cost'], res['score']['cost'])
    with pytest.raises(ValueError, match='traj'):
        cl.run_mpc(par, 'naive', xg, ug, make_controller=mk, make_backup=mkb, n_steps=2, traj=curves[:3])


def test_generate_guess_until_refuses_curves():
    from safe_mpc_amd import closed_loop as cl
    with pytest.raises(ValueError, match='per-instance curves are not supported'):
        cl.generate_guess_until(cc.params(), 'naive', 2, traj=cc.dealt(2))


def test_generate_guess_hands_every_instance_its_curve():
    """the host path with a solver double: x0 of instance i comes from ik_starts at traj[i, :, 0] and the controller holds traj[i];
    an instance whose IK fails is dropped with its curve"""
    from safe_mpc_amd import closed_loop as cl
    par = cc.params(nlp_max_iter=1)
    n = 4
    curves = cc.dealt(n)
    made, seen = [], {}

    def mk(name, batch):
        made.append(make_double_controller(name, par, batch))
        return made[-1]
    real = cl.ik_starts

    def fake_ik(solver, problem, target, n_, scenes=None, **kw):
        seen['target'] = np.array(target)
        x0 = np.zeros((n_, problem.nx))
        x0[:, 0] = 0.1 * np.arange(n_)
        return x0, np.array([[0, 1], [0, 0], [0, 2], [0, 1]], np.int32)
    cl.ik_starts = fake_ik
    try:
        guess, mask = cl.generate_guess(par, 'naive', n, make_controller=mk, traj=curves)
    finally:
        cl.ik_starts = real
    assert np.array_equal(seen['target'], curves[:, :, 0])
    assert guess['ik_failed'].tolist() == [1] and not mask[1] and mask.shape == (n,)
    ctrl = made[-1]
    assert ctrl.B == 3 and np.array_equal(ctrl.traj, curves[[0, 2, 3]])
    assert np.array_equal(ctrl.p[:, :, :3], np.transpose(curves[[0, 2, 3]][:, :, :cc.N + 1], (0, 2, 1)))
    assert np.array_equal(guess['curves'], curves[[0, 2, 3]][mask[[0, 2, 3]]])


# ---- the entry scripts -----------------------------------------------------------------------------------------------------------------
def test_track_jitter_options():
    import importlib.util
    from safe_mpc_amd import closed_loop as cl
    from safe_mpc_amd.tracking import jittered_curves
    par = cc.params()
    for argv in (['--track-jitter', '0.01'], ['--track-scale-jitter', '0.1'], ['--track-seed', '2', '-c', 'naive']):
        with pytest.raises(ValueError, match='only for a tracking run'):
            cl.tracking_from_cli(cc.params(), argv, n=3)
    with pytest.raises(ValueError, match='needs --track-jitter'):
        cl.tracking_from_cli(cc.params(), ['--track', '8', '--track-seed', '2'], n=3)
    with pytest.raises(ValueError, match='needs a value'):
        cl.tracking_from_cli(cc.params(), ['--track', '8', '--track-jitter'], n=3)
    got = cl.tracking_from_cli(par, ['--track', 'circle', '--track-jitter', '0.01', '--track-scale-jitter', '0.1', '--track-seed', '2'], n=3)
    assert par.track_traj and np.array_equal(got, jittered_curves(cc.params(), 'circle', 3, 0.01, seed=2, scale_sigma=0.1))
    cfg = cc.params(track_traj=True)
    assert np.array_equal(cl.tracking_from_cli(cfg, ['--track-jitter', '0.02'], n=2), jittered_curves(cc.params(), '8', 2, 0.02))
    assert cl.tracking_from_cli(cc.params(), ['--track', '8'], n=3).shape == (3, cc.L)          # no jitter: the one curve, as before
    # the scripts refuse the option without a tracking run, before they load or build anything
    for script in ('mpc.py', 'guess_acados.py'):
        spec = importlib.util.spec_from_file_location('smpc_script_' + script[:-3], os.path.join(ROOT, 'scripts', script))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        with pytest.raises(ValueError, match='only for a tracking run'):
            mod.main(['-c', 'naive', '--track-jitter', '0.01'])


def test_library_exports_the_entry_point():
    import ctypes
    from safe_mpc_amd import _lib
    assert 'smpc_set_instance_curves' in _lib.SYMBOLS
    assert os.path.exists(_lib.LIB_PATH), 'the engine is built before the tests run (__graft_entry__.build)'
    L = ctypes.CDLL(_lib.LIB_PATH)               # loads without a GPU
    assert hasattr(L, 'smpc_set_instance_curves') and L.smpc_abi_version() == 5
