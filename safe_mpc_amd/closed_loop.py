"""Batched versions of the reference's two live entry points, as library functions:

* :func:`generate_guess`  -- scripts/guess_acados.py:72-158,235-244 (warm starts by SQP to convergence)
* :func:`generate_guess_until` -- the same with the reference's ``while succ < num_ics``: on the device, until n are accepted
* :func:`run_mpc`         -- scripts/mpc.py:102-317 (closed loop with safe abort, failure taxonomy, result dict)

Every instance of the reference's outer loop (mpc.py:102) is one row of the arrays handled here; the inner loop over MPC
steps stays a Python loop, each iteration being a handful of batched engine calls.  ``scripts/mpc.py`` and
``scripts/guess_acados.py`` are thin CLI wrappers that keep the reference's flags, file names and pickle formats.
"""
from __future__ import annotations

import copy
import heapq
import os
import pickle
from collections import namedtuple

import numpy as np

from .controller import SafeBackupController, get_controller
from .problem import JOINT_DTYPE
from .urdf import Inertial, Origin, RobotDescription, SerialChain


# ---- file names --------------------------------------------------------------------------------------
def guess_file(params, model_name, cont_name, horizon, use_net):
    track = 'traj_track' if params.track_traj else ''
    return (f'{params.DATA_DIR}{model_name}_{cont_name}_{horizon}hor_{int(params.alpha)}sm_use_net{use_net}_{track}'
            f'_q_collision_margins_{params.q_margin}_{params.collision_margin}_guess.pkl')


def result_file(params, model_name, cont_name, horizon, use_net, noise, control_noise, jm, cm, controller_model='nominal', forecast=None,
                forecast_window=None, obs_noise=0.0, forecast_degree=1, row_margin=None, row_margin_fit=None, kalman=None,
                row_margin_kalman=None, obs_dropout=None):
    """``controller_model='plant'`` (scripts/mpc.py --controller-model plant, run_mpc(models='plant')): the suffix ``_cmplant``
    before ``_mpc.pkl``; ``forecast`` (scripts/mpc.py --scene-forecast, run_mpc(forecast=...)): the suffix ``_fc<mode>`` behind
    it, ``_fcfit_w<m>`` for a fit over ``forecast_window = m`` columns, ``_d<p>`` behind that for ``forecast_degree = p`` other than 1
    (a polynomial fit, --forecast-degree); ``obs_noise = s > 0`` (--scene-obs-noise): ``_on<s>`` behind
    that; ``row_margin = (a, b)`` (--row-margin, run_mpc(row_margin=...)): ``_rm<a>`` behind that, and ``_g<b>`` for b other than 0;
    ``row_margin_fit = (z, sigma_prior, d_max)`` (--row-margin-z, run_mpc(row_margin_fit=...)): ``_rmf<z>_p<sigma_prior>_c<d_max>`` behind that;
    ``forecast='kalman'`` with ``kalman = (q, r[, v0, a0, beta])`` (--scene-forecast kalman): ``_fckalman_d<p>_q<q>_r<r>_v<v0>_a<a0>_b<beta>``
    in the forecast's place, ``obs_dropout = (p, len)`` (--scene-obs-dropout): ``_od<p>_l<len>`` behind ``_on``, and
    ``row_margin_kalman = (z, d_max)`` (--row-margin-z with the filter): ``_rmk<z>_c<d_max>`` at the end;
    the defaults give the reference's name"""
    if controller_model not in ('nominal', 'plant'):
        raise ValueError(f"controller_model: {controller_model!r}: expected 'nominal' or 'plant'")
    track = 'traj_track' if params.track_traj else ''
    return (f'{params.DATA_DIR}{model_name}_{cont_name}_use_net{use_net}_{horizon}hor_{int(params.alpha)}sm_{track}'
            f'noise_{noise}_control_noise{control_noise}_q_collision_margins_{jm}_{cm}'
            f"{'_cmplant' if controller_model == 'plant' else ''}"
            f"{'' if forecast is None else _Forecast(forecast, forecast_window, forecast_degree, kalman).file_suffix()}"
            f"{f'_on{obs_noise}' if obs_noise > 0 else ''}"
            f"{'' if obs_dropout is None else '_od{}_l{}'.format(*(float(v) for v in obs_dropout))}"
            f"{'' if row_margin is None else f'_rm{float(row_margin[0])}' + (f'_g{float(row_margin[1])}' if float(row_margin[1]) != 0.0 else '')}"
            f"{'' if row_margin_fit is None else '_rmf{}_p{}_c{}'.format(*(float(v) for v in row_margin_fit))}"
            f"{'' if row_margin_kalman is None else '_rmk{}_c{}'.format(*(float(v) for v in row_margin_kalman))}"
            "_mpc.pkl")


def tracking_from_cli(params, argv, n=None):
    """The curve of a tracking run as the entry scripts select it: ``--track 8|circle`` on the command line, or ``track_traj: true``
    in config.yaml (the "8").  Returns ``tracking.tracking_trajectory(params, curve)`` -- which also makes the run
    n_steps_tracking long and sets ``params.track_traj`` -- or None for the reach task.

    ``--track-jitter SIGMA [--track-scale-jitter S] [--track-seed S]``: a curve of its own for each of the ``n`` instances,
    ``tracking.jittered_curves(params, curve, n, SIGMA, seed, S)`` ``[n, 3, L]``.  Only with a tracking run (ValueError
    otherwise); without ``n`` the options are checked and the plain curve is returned."""
    from .tracking import jittered_curves, tracking_trajectory
    argv = list(argv)

    def opt(flag, default, cast):
        if flag not in argv:
            return default
        if argv.index(flag) + 1 >= len(argv):
            raise ValueError(f'{flag} needs a value')
        return cast(argv[argv.index(flag) + 1])
    curve = None
    if '--track' in argv:
        if argv.index('--track') + 1 >= len(argv):
            raise ValueError('--track needs a curve: 8 or circle')
        curve = argv[argv.index('--track') + 1]
    elif getattr(params, 'track_traj', False):
        curve = '8'
    jitter = [f for f in ('--track-jitter', '--track-scale-jitter', '--track-seed') if f in argv]
    if jitter and curve is None:
        raise ValueError(f"{jitter[0]} is valid only for a tracking run: give --track 8|circle (or track_traj: true in config.yaml)")
    if jitter and '--track-jitter' not in argv:
        raise ValueError(f'{jitter[0]} needs --track-jitter SIGMA')
    if jitter and n is not None:
        return jittered_curves(params, curve, int(n), opt('--track-jitter', 0.0, float), opt('--track-seed', 0, int),
                               opt('--track-scale-jitter', 0.0, float))
    return None if curve is None else tracking_trajectory(params, curve)


def halton(n, dim, skip=1):
    """Unscrambled Halton points (guess_acados.py:79 uses scipy's qmc.Halton(d, scramble=False))."""
    primes = [2, 3, 5, 7, 11, 13, 17, 19, 23, 29]
    idx = np.arange(skip, skip + n)
    out = np.zeros((n, dim))
    for d in range(dim):
        b, f, k, r = primes[d], 1.0, idx.copy(), np.zeros(n)
        while k.max() > 0:
            f /= b
            r += f * (k % b)
            k //= b
        out[:, d] = r
    return out


# ---- model noise (utils.py:126-171, generate_urdf_noise.py:20-36, env_model.py:321-328) ----------------------------------
def perturbed_joint_tables(params, nq, noise_pct, seeds):
    """Per-instance plant models: every URDF link's mass, inertia entries and COM coordinates are multiplied by
    1 + U(-noise, noise)% (utils.py:138-166) BEFORE lumping -- in memory, instead of one URDF file per instance."""
    base = params.robot_descr
    out = np.zeros((len(seeds), nq), JOINT_DTYPE)
    # The reference draws uniform(-n, n) for EVERY field, also where the field and hence n is zero (ixy = 0 ...): the draw returns 0
    # but advances the generator, so a replay of its seeded perturbations needs the same.  Default (reference_quirks); without it
    # zero-magnitude fields consume nothing (rounds 1-4).
    always_draw = bool(getattr(params, 'reference_quirks', True))
    for row, seed in enumerate(seeds):
        rng = np.random.default_rng(int(seed))
        draw = lambda n_: rng.uniform(-n_, n_) if (n_ > 0 or (always_draw and noise_pct > 0)) else 0.0
        links = []
        for l in base.links:
            l2 = copy.copy(l)
            if l.inertial is not None:
                m = l.inertial.mass
                m = m + draw(abs(m) * noise_pct / 100)
                I = l.inertial.inertia.copy()
                for (a, b) in [(0, 0), (1, 1), (2, 2), (0, 1), (1, 2), (0, 2)]:       # ixx iyy izz ixy iyz ixz (utils.py:128)
                    v = I[a, b] + draw(abs(I[a, b]) * noise_pct / 100)
                    I[a, b] = I[b, a] = v
                xyz = l.inertial.origin.xyz.copy()
                for k in range(3):
                    xyz[k] += draw(abs(xyz[k] * noise_pct / 100))
                l2.inertial = Inertial(Origin(xyz, l.inertial.origin.rpy), m, I)
            links.append(l2)
        chain = SerialChain(RobotDescription(links, base.joints, base.name), nq)
        for i, j in enumerate(chain.joints):
            o = out[row, i]
            o['R0'], o['p0'], o['axis'] = j.R0.reshape(-1), j.p0, j.axis
            o['mass'], o['com'] = j.mass, j.com
            I = j.inertia
            o['inertia'] = [I[0, 0], I[0, 1], I[0, 2], I[1, 1], I[1, 2], I[2, 2]]
            o['q_min'], o['q_max'], o['v_max'], o['tau_max'] = j.q_min, j.q_max, j.v_max, j.tau_max
    return out


def _mv3(R, v):
    """R [3, 3] (or [..., 3, 3]) times v [..., 3] with the sums written out: elementwise numpy only, so that a row of a batch gets the
    same bits whatever the batch's size (a BLAS matmul may pick another kernel, and another summation order, per shape)."""
    return R[..., :, 0] * v[..., None, 0] + R[..., :, 1] * v[..., None, 1] + R[..., :, 2] * v[..., None, 2]


def _mm3(A, B):
    """A [..., 3, 3] times B [..., 3, 3], sums written out (see _mv3)."""
    return (A[..., :, 0, None] * B[..., None, 0, :] + A[..., :, 1, None] * B[..., None, 1, :]) + A[..., :, 2, None] * B[..., None, 2, :]


def perturbed_joint_tables_batched(params, nq, noise_pct, seeds):
    """The per-instance plant models of :func:`perturbed_joint_tables` for MANY seeds at once (BASELINE config 2: 65 536 instances,
    seed = instance id): the same draws in the same order -- one ``default_rng(seed)`` per instance, ten draws per URDF
    link in the reference's order (mass, ixx iyy izz ixy iyz ixz, x y z; utils.py:128, 138-166), bit for bit those of the per-seed
    function -- and the lumping into joint tables as elementwise array arithmetic over the batch.  The per-seed function stays the
    statement the tests hold this one against (draws equal to the bit, tables to 1e-13 of their scale: SerialChain lumps with
    BLAS-backed matmuls, this one with written-out sums)."""
    base = params.robot_descr
    seeds = np.asarray(seeds, np.int64).reshape(-1)
    B = len(seeds)
    always_draw = bool(getattr(params, 'reference_quirks', True))
    chain0 = SerialChain(base, nq)                      # structure: carriers of every link, joint frames, limits (not perturbed)
    # nominal value of every field that is drawn for, in the reference's order
    fields = []                                         # (link index, kind, a, b)
    for li, l in enumerate(base.links):
        if l.inertial is None:
            continue
        fields.append((li, 'm', 0, 0))
        fields += [(li, 'I', a, b) for (a, b) in [(0, 0), (1, 1), (2, 2), (0, 1), (1, 2), (0, 2)]]
        fields += [(li, 'c', k, 0) for k in range(3)]

    def nominal(f):
        l = base.links[f[0]].inertial
        return l.mass if f[1] == 'm' else (l.inertia[f[2], f[3]] if f[1] == 'I' else l.origin.xyz[f[2]])
    nom = np.array([nominal(f) for f in fields])
    # (the magnitudes exactly as the per-seed function forms them: abs(v) * noise / 100 for mass and inertia, abs(v * noise / 100) for
    #  the centre of mass)
    mag = np.array([abs(v * noise_pct / 100) if f[1] == 'c' else abs(v) * noise_pct / 100 for f, v in zip(fields, nom)])
    drawn = (mag > 0) | (always_draw and noise_pct > 0)
    nd = int(drawn.sum())
    U = np.zeros((B, len(fields)))
    if nd:
        R = np.empty((B, nd))
        for r_, sd in enumerate(seeds):                 # one generator per instance, as the reference reseeds per model
            R[r_] = np.random.default_rng(int(sd)).random(nd)
        lo, hi = -mag[drawn], mag[drawn]
        U[:, drawn] = lo + (hi - lo) * R                # Generator.uniform(low, high) = low + (high - low) * next_double
    val = nom[None, :] + U                              # [B, fields]
    # lump: every link's inertial into the actuated link that carries it
    m = np.zeros((B, nq))
    mc = np.zeros((B, nq, 3))
    parts = [[] for _ in range(nq)]
    col = 0
    for li, l in enumerate(base.links):
        if l.inertial is None:
            continue
        mass, ent, xyz = val[:, col], val[:, col + 1:col + 7], val[:, col + 7:col + 10]
        col += 10
        if l.name not in chain0._carrier:
            continue
        idx, Rc, pc = chain0._carrier[l.name]
        if idx < 0:
            continue
        I = np.empty((B, 3, 3))
        for e_, (a, b) in enumerate([(0, 0), (1, 1), (2, 2), (0, 1), (1, 2), (0, 2)]):
            I[:, a, b] = ent[:, e_]
            I[:, b, a] = ent[:, e_]
        c = pc + _mv3(Rc, xyz)
        Ro = Rc @ l.inertial.origin.R                   # (constants of the model)
        Ic = _mm3(_mm3(np.broadcast_to(Ro, (B, 3, 3)), I), np.broadcast_to(Ro.T, (B, 3, 3)))
        m[:, idx] += mass
        mc[:, idx] += mass[:, None] * c
        parts[idx].append((mass, c, Ic))
    out = np.zeros((B, nq), JOINT_DTYPE)
    eye = np.eye(3)
    for i, j in enumerate(chain0.joints):
        if np.any(m[:, i] <= 0):
            raise ValueError(f'link moved by {j.name} has no mass')
        com = mc[:, i] / m[:, i, None]
        I = np.zeros((B, 3, 3))
        for (mi, ci, Ici) in parts[i]:
            d = ci - com
            dd = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
            I += Ici + mi[:, None, None] * (dd[:, None, None] * eye - d[:, :, None] * d[:, None, :])
        o = out[:, i]
        o['R0'], o['p0'], o['axis'] = j.R0.reshape(-1), j.p0, j.axis
        o['mass'], o['com'] = m[:, i], com
        o['inertia'] = np.stack([I[:, 0, 0], I[:, 0, 1], I[:, 0, 2], I[:, 1, 1], I[:, 1, 2], I[:, 2, 2]], axis=1)
        o['q_min'], o['q_max'], o['v_max'], o['tau_max'] = j.q_min, j.q_max, j.v_max, j.tau_max
    return out


# ---- warm-start generation ----------------------------------------------------------------------------------------------------
def merit_terms(ctrl, x0, x, u):
    """Pieces of the l1 merit function of the OCP at the iterate (x, u), per instance, from one batched linearisation
    (``smpc_eval_nodes``): cost f, its gradient (dq, du parts) and the l1 norm of every constraint's violation -- initial
    state, dynamics defects, state box, torque rows, collision rows, safe-set row (where the formulation has it)."""
    pr, d = ctrl.problem, ctrl.problem.desc
    nq, N, dt = ctrl.nq, ctrl.N, ctrl.params.dt
    x, u = np.asarray(x, float), np.asarray(u, float)
    ev = ctrl.ocp_solver.eval_nodes(x, u, ctrl.p)
    ee = np.asarray(ev['ee'])
    cs = np.full(N + 1, d.cost_scale_stage)
    cs[N] = d.cost_scale_term
    if d.cost_kind != 0:
        err = np.sum((ee - ctrl.p[:, :, :3]) ** 2, axis=2)                           # [B, N+1]
        f = (cs * d.Q * err).sum(1) + (cs[:N] * d.R * np.sum(u ** 2, axis=2)).sum(1)
        gq = cs[None, :, None] * np.asarray(ev['cost_grad_q'])[:, :, :nq]
        gu = cs[None, :N, None] * 2.0 * d.R * u
    else:
        f, gq, gu = np.zeros(len(x)), np.zeros((len(x), N + 1, nq)), np.zeros_like(u)
    pos = lambda a: np.maximum(a, 0.0)
    viol = np.abs(x[:, 0] - x0).sum(1)
    xn = np.empty_like(x[:, 1:])
    xn[:, :, :nq] = x[:, :-1, :nq] + dt * x[:, :-1, nq:] + 0.5 * dt * dt * u
    xn[:, :, nq:] = x[:, :-1, nq:] + dt * u
    viol += np.abs(x[:, 1:] - xn).sum(axis=(1, 2))
    lo = np.tile(pr.lbx, (N + 1, 1)); hi = np.tile(pr.ubx, (N + 1, 1))
    lo[N], hi[N] = pr.lbx_e, pr.ubx_e
    viol += (pos(lo[1:] - x[:, 1:]) + pos(x[:, 1:] - hi[1:])).sum(axis=(1, 2))
    tau = np.asarray(ev['tau'])[:, :N, :nq]
    viol += pos(np.abs(tau) - pr.tau_max).sum(axis=(1, 2))
    if d.n_rows:
        rv = np.asarray(ev['row_val'])[:, 1:, :d.n_rows]
        lb = np.where(np.abs(pr.row_lb) < 1e5, pr.row_lb, -np.inf)
        ub = np.where(np.abs(pr.row_ub) < 1e5, pr.row_ub, np.inf)
        viol += (pos(lb - rv) + pos(rv - ub)).sum(axis=(1, 2))
    if d.nn_mode != 0:
        g = np.asarray(ev['nn_val'])
        on = ctrl.p[:, :, 4] > 0
        on[:, 0] = False
        if d.nn_mode == 1:
            on[:, :N] = False
        viol += (pos(-g) * on).sum(1)
    return f, gq, gu, viol


def _sqp_on_device(ctrl, x0, max_iter, history, verbose, opts):
    """The SQP loop of :func:`generate_guess` through the engine (smpc_sqp_batch) on device tensors: one call for all iterations,
    or one call per iteration when ``history`` is wanted.  Leaves the iterate in ctrl.x_guess / u_guess (numpy); returns status."""
    import torch
    sv = ctrl.ocp_solver
    ctrl.p[:, :, 3] = ctrl.params.alpha                     # what ctrl.solve does before every solve
    ctrl._apply_traj()
    dev = torch.device('cuda', sv.device)
    to = lambda a: torch.as_tensor(np.ascontiguousarray(np.asarray(a), np.float64), device=dev)
    x0_d, xg, ug, p_d = to(x0), to(ctrl.x_guess), to(ctrl.u_guess), to(ctrl.p)
    B = x0_d.shape[0]
    state = sv.new_sqp_state(B, x0_d)
    if history is None:
        sv.sqp(x0_d, xg, ug, p_d, dict(max_iter=max_iter, **opts), state)
    else:
        for it in range(max_iter):
            was_done = state['done'].cpu().numpy().astype(bool)
            sv.sqp(x0_d, xg, ug, p_d, dict(max_iter=1, **opts), state)
            h = {k: state[k].cpu().numpy() for k in ('merit', 'merit_before', 'alpha', 'mu', 'violation', 'updated', 'done')}
            # (an instance that was done before this iteration took no part in it: its entries are those of its last iteration,
            #  reported the way the host loop reports an instance it does not move)
            upd = h['updated'].astype(bool) & ~was_done
            history.append({'merit': h['merit'], 'merit_before': np.where(was_done, h['merit'], h['merit_before']),
                            'alpha': np.where(upd, h['alpha'], 0.0), 'mu': h['mu'], 'violation': h['violation'], 'updated': upd})
            if verbose:
                print(f'SQP iteration {it}: {int(h["done"].sum())}/{B} done')
            if h['done'].all():
                break
    sv.sync()
    ctrl.x_guess, ctrl.u_guess = xg.cpu().numpy(), ug.cpu().numpy()
    return state['status'].cpu().numpy()


def _require(solver, feature, method):
    """the capability check of every per-instance feature: ValueError, naming the feature, unless ``solver`` has ``method``"""
    if not hasattr(solver, method):
        raise ValueError(f'{feature}: {type(solver).__name__} has no {method}')


def _check_scenes(scenes, B, problem):
    """``scenes`` as a contiguous float64 array: [B, n_rows, SCENE_ROW] (problem.row_geometry's layout per instance), or a track
    [B, T, n_rows, SCENE_ROW] with T >= 1 time columns (problem.moving_scenes); ValueError otherwise"""
    from .problem import SCENE_ROW
    g = np.ascontiguousarray(scenes, np.float64)
    want = (int(B), len(problem.rows), SCENE_ROW)
    if g.ndim == 4:
        if (g.shape[0],) + g.shape[2:] != want or g.shape[1] < 1:
            raise ValueError(f'scenes: shape {g.shape}, expected {want[:1] + ("T >= 1",) + want[1:]} (a track: one [n_rows, '
                             f'{SCENE_ROW}] geometry per instance and time column)')
    elif g.shape != want:
        raise ValueError(f'scenes: shape {g.shape}, expected {want} (one [n_rows, {SCENE_ROW}] geometry per instance) or '
                         f'{want[:1] + ("T",) + want[1:]} (a track)')
    if not len(problem.rows):
        raise ValueError('scenes: the problem has no collision rows')
    return g


def _context_select(solver):
    """the ``(row, slot)`` pairs of the solver's safe-set net if that net has a context, else None"""
    net = getattr(solver, 'net', None)
    if not getattr(net, 'n_ctx', 0) or not hasattr(solver, 'set_instance_context'):
        return None
    if not net.ctx_select:
        raise ValueError(f'scenes: the safe-set network has {net.n_ctx} context inputs but no ctx_select that says which numbers of '
                         f'a scene they are')
    return net.ctx_select


def _set_scene(solver, geom):
    """the scenes [B, n_rows, 8], or the scene track [B, T, n_rows, 8], of a batch onto the solver (None clears either).  Where the
    solver's safe-set net has a context, the instances' contexts go on and off with the scenes: a track of T > 1 columns brings a
    context track of the same T (solver.set_instance_context_track), so that the network row of node k is asked
    about the scene its collision rows see."""
    _require(solver, 'scenes', 'set_instance_scene')
    select = _context_select(solver)
    if select is not None:
        from .problem import scene_context
        if geom is not None and geom.ndim == 4 and geom.shape[1] > 1:
            if not hasattr(solver, 'set_instance_context_track'):
                raise ValueError(f'scenes: a track of T = {geom.shape[1]} time columns with a safe-set network that has a context: the '
                                 f'context is a constant of the instance, one that moves along a track is not supported')
            solver.set_instance_context_track(scene_context(geom, select))
        else:
            solver.set_instance_context(None if geom is None else scene_context(geom.reshape((geom.shape[0],) + geom.shape[-2:]), select))
    if geom is not None and geom.ndim == 4:
        _require(solver, 'scenes', 'set_instance_scene_track')
        solver.set_instance_scene_track(geom)
    else:
        solver.set_instance_scene(geom)


def _clear_scene(solver):
    """the handle keeps no scene (or track, or clock) behind a run: ``make_controller`` / ``make_backup`` may hand out a solver
    that is used again, with another batch size (refused while a scene of the old size is set) or with the same one (which would
    run in the old scenes)"""
    if hasattr(solver, 'set_instance_scene'):
        solver.set_instance_scene(None)
    if hasattr(solver, 'set_instance_context'):
        solver.set_instance_context(None)
    if hasattr(solver, 'set_scene_clock'):
        solver.set_scene_clock(None)


def _set_models(solver, table):
    """the controller models [B, nq] of a batch onto the solver (None clears them)"""
    _require(solver, 'models', 'set_instance_models')
    solver.set_instance_models(table)


def _new_scene_clock(solver):
    """a one-element int64 cell for ``solver.set_scene_clock`` on a host loop: in HBM for an engine handle (the kernels read it
    there), a numpy array for a CPU double"""
    if hasattr(solver, 'L'):
        import torch
        return torch.zeros((1,), dtype=torch.int64, device=torch.device('cuda', solver.device))
    return np.zeros(1, np.int64)


def _write_scene_clock(cell, t):
    """cell <- t, finished before the next engine call is enqueued (the engine runs on a stream of its own; a host loop waits
    for every call anyway)"""
    if cell is None:
        return
    cell[0] = int(t)
    if not isinstance(cell, np.ndarray):
        import torch
        torch.cuda.current_stream(cell.device).synchronize()


def _free_starts_per_scene(solver, scenes, cand):
    """The start states of :func:`generate_guess` with a scene per instance: the Halton candidates ``cand`` are walked in sampling
    order, each one tested IN THE SCENE OF THE INSTANCE IT WOULD START (the next unfilled one) and skipped if it collides there --
    with one scene for everybody, the free candidates in order, as without scenes.  The walk pairs all remaining candidates with
    the remaining instances at once, keeps the pairs up to the first collision and re-pairs behind it: one engine call per
    rejected candidate.  Returns (x0 [n, nx], filled [n] bool): filled is False where the candidates ran out."""
    n = scenes.shape[0]
    x0, filled = np.zeros((n, cand.shape[1])), np.zeros(n, bool)
    c = k = 0
    if hasattr(solver, 'set_scene_clock'):
        solver.set_scene_clock(None)                # (a track: its column 0, where the instance starts)
    while k < n and c < len(cand):
        m = min(n - k, len(cand) - c)
        _set_scene(solver, scenes[k:k + m])
        free = np.asarray(solver.check_trajectory(cand[c:c + m, None, :], tol_x=0.0)).astype(bool)      # guess_acados.py:109
        ok = m if free.all() else int(np.argmin(free))          # pairs before the first collision stand
        x0[k:k + ok], filled[k:k + ok] = cand[c:c + ok], True
        c, k = c + ok + (ok < m), k + ok
    _set_scene(solver, None)
    return x0, filled


def ik_starts(solver, problem, target, n, starts_per=16, seed=0, scenes=None, first=0, **over):
    """n start states at rest whose end effector sits at ``target`` ([3], or [n, 3]) -- the x0 of a tracking run, which the
    reference takes from InverseKinematicsOCP (guess_acados.py:179-183) -- by the batched multi-start IK (``solver.ik``,
    smpc_ik_batch; ik.ik_batch_host for a solver without one).  Instance i draws its OWN block of ``starts_per`` Halton points in the
    joint box (points ``seed + (first + i) * starts_per`` onwards of :func:`halton`), so n instances get n different arm
    configurations at the same end-effector point.  ``scenes`` [n, n_rows, 8]: instance i is solved in its scene (of a track
    [n, T, n_rows, 8]: in its column 0, where the run starts).
    Returns ``(x0 [n, nx], info [n, 2])``: info[i] = (winning start, number of successful starts); ``info[i, 1] == 0`` means NO
    solution was found for instance i, and x0[i] is then only the closest point reached."""
    from .ik import ik, ik_params
    n, starts_per, nq = int(n), int(starts_per), problem.nq
    par = ik_params(problem, **over)
    lo, hi = par['q_lo'], par['q_hi']
    if n <= 0:
        return np.zeros((0, problem.nx)), np.zeros((0, 2), np.int32)
    tg = np.ascontiguousarray(np.broadcast_to(np.asarray(target, float).reshape(-1, 3), (n, 3)))
    q_start = lo + halton(n * starts_per, nq, skip=1 + int(seed) + int(first) * starts_per).reshape(n, starts_per, nq) * (hi - lo)
    if scenes is not None:
        scenes = _check_scenes(scenes, n, problem)
        if scenes.ndim == 4:
            scenes = np.ascontiguousarray(scenes[:, 0])
    q, info, _ = ik(solver, problem, tg, q_start, scenes=scenes, **over)
    return np.hstack([np.asarray(q, float), np.zeros((n, nq))]), np.asarray(info)


class _IkStarts:
    """The sample stream of a tracking run in chunks: sample j = the j-th instance of :func:`ik_starts` at ``target`` whose IK
    succeeded (``failed`` lists the instance numbers that did not).  ``take(j)`` as _FreeStarts'."""

    def __init__(self, solver, problem, target, chunk=64, max_barren=16):
        self.sv, self.pr, self.target, self.chunk, self.max_barren = solver, problem, target, int(chunk), int(max_barren)
        self.drawn, self.failed = 0, []
        self.x = np.zeros((0, problem.nx))

    def take(self, j):
        barren = 0
        while j >= len(self.x):
            x0, info = ik_starts(self.sv, self.pr, self.target, self.chunk, first=self.drawn)
            ok = info[:, 1] > 0
            self.failed += [int(self.drawn + i) for i in np.where(~ok)[0]]
            self.drawn += self.chunk
            barren = 0 if ok.any() else barren + 1
            if barren >= self.max_barren:
                raise RuntimeError(f'the inverse kinematics found no start state at {np.asarray(self.target).tolist()} in '
                                   f'{barren * self.chunk} instances in a row')
            self.x = np.vstack([self.x, x0[ok]])
        return self.x[j]


def new_host_sqp_state(B, mu0=10.0):
    """The per-instance state of :func:`sqp_host_advance` at its start values: the fields of ``smpc_sqp_state`` (_lib.SqpState) as
    numpy arrays, what ``BatchedOcpSolver.new_sqp_state`` returns for the host."""
    from ._lib import SqpState
    st = {k: np.zeros(B, dt) for k, dt in SqpState.FIELDS}
    st['mu'][:] = float(mu0)
    return st


def sqp_host_advance(ctrl, x0, state, max_iter, sqp_tol=1e-6, armijo=1e-4, alpha_reduction=0.7, alpha_min=0.05, history=None,
                     verbose=False):
    """Up to ``max_iter`` iterations of the numpy SQP of :func:`generate_guess` (its docstring states the iteration) on
    ctrl.x_guess / ctrl.u_guess, resuming from ``state`` (:func:`new_host_sqp_state`, updated in place): the round of an SQP that is
    looked at between rounds, as ``solver.sqp(max_iter=...)`` is on the device.  k calls of one iteration equal one call of k.  An
    instance with ``state['done']`` set takes no part; the call returns once every instance is done."""
    nq = ctrl.problem.nq
    B = len(x0)
    done = state['done'].astype(bool)
    status, mu = state['status'], state['mu']
    for it in range(int(max_iter)):
        st = ctrl.solve(x0)
        dx, du = ctrl.x_temp - ctrl.x_guess, ctrl.u_temp - ctrl.u_guess
        step = np.maximum(np.abs(dx).reshape(B, -1).max(1), np.abs(du).reshape(B, -1).max(1))
        f0, gq, gu, c0 = merit_terms(ctrl, x0, ctrl.x_guess, ctrl.u_guess)
        gd = (gq * dx[:, :, :nq]).sum(axis=(1, 2)) + (gu * du).sum(axis=(1, 2))
        # penalty large enough for  D = grad f . d - mu |c|_1 < 0  wherever the iterate is infeasible
        need = np.where(c0 > 1e-12, 2.0 * np.maximum(gd, 0.0) / np.maximum(c0, 1e-12), 0.0)
        mu[:] = np.minimum(np.maximum(mu, need), 1e8)
        m0 = f0 + mu * c0
        D = gd - mu * c0
        alpha = np.ones(B)
        settled = done | (st != 0)
        while True:
            xt = ctrl.x_guess + alpha[:, None, None] * dx
            ut = ctrl.u_guess + alpha[:, None, None] * du
            ft, _, _, ct = merit_terms(ctrl, x0, xt, ut)
            ok = (ft + mu * ct <= m0 + armijo * alpha * np.minimum(D, 0.0) + 1e-12 * (1.0 + np.abs(m0)))
            settled = settled | ok | (alpha <= alpha_min)
            if settled.all():
                break
            alpha = np.where(settled, alpha, np.maximum(alpha * alpha_reduction, alpha_min))
        upd = ~done & (st == 0)
        ctrl.x_guess = np.where(upd[:, None, None], xt, ctrl.x_guess)
        ctrl.u_guess = np.where(upd[:, None, None], ut, ctrl.u_guess)
        status[:] = np.where(~done, st, status)
        state['iters'] += (~done).astype(np.int32)
        state['qp_iter_total'] += np.where(~done, np.asarray(ctrl.qp_iter), 0).astype(np.int32)
        if history is not None:
            history.append({'merit': np.where(upd, ft + mu * ct, m0), 'merit_before': m0.copy(), 'alpha': np.where(upd, alpha, 0.0),
                            'mu': mu.copy(), 'violation': np.where(upd, ct, c0), 'updated': upd.copy()})
        done |= (alpha * step < sqp_tol) | (st != 0)
        state['done'][:] = done
        if verbose:
            print(f'SQP iteration {it}: {done.sum()}/{B} done, max step {step[upd].max() if upd.any() else 0:.2e}, '
                  f'min alpha {alpha[upd].min() if upd.any() else 1:.2f}')
        if done.all():
            break
    return state


def generate_guess(params, cont_name, n, make_controller=None, sqp_tol=1e-6, verbose=False, armijo=1e-4, alpha_reduction=0.7,
                   alpha_min=0.05, history=None, on_device=False, scenes=None, traj=None, models=None):
    """guess_acados.py:98-158: Halton q0 in the joint box, collision filter, constant guess, SQP to convergence, checkGuess.

    SQP with merit backtracking (the reference runs acados with nlp_solver_type SQP, globalization MERIT_BACKTRACKING,
    parser.py:115-117,139): every iteration solves the engine's stage QP at the current iterate (one RTI solve from it),
    then backtracks the step length per instance on the l1 merit  f + mu |c|_1  until the Armijo condition
    merit(alpha) <= merit(0) + armijo * alpha * (grad f . d - mu |c(0)|_1)  holds (factor ``alpha_reduction``, floor
    ``alpha_min`` at which the step is taken regardless -- acados' defaults 0.7 / 0.05 [EXT-UNVERIFIED]; the reference parses
    alpha_reduction / alpha_min from config.yaml but never hands them to acados, parser.py:119-120).  The penalty mu grows
    so that the QP step is a descent direction of the merit.  All instances advance together; one batched linearisation per
    trial step length.  Returns (dict(xg [m,N+1,nx], ug [m,N,nu]) of the accepted instances in sampling order, good mask);
    ``history`` (a list) receives the per-iteration merit values [B] for inspection.

    ``on_device=True``: the same sampling, filter and checkGuess, with the SQP iterations run by the engine on device-resident
    arrays (``solver.sqp``, smpc_sqp_batch) instead of the numpy loop below, which stays the statement the engine's iteration is
    tested against.  With ``history`` the engine advances one iteration per call and the same keys are appended.

    ``scenes`` ([n, n_rows, 8], ``OcpProblem.scene`` / ``jittered_scenes``): instance i is sampled, solved and tested in ITS scene
    (solver.set_instance_scene): the Halton candidates are walked in order and each is tested against the scene of the instance it
    would start, so a candidate that collides there is skipped (:func:`_free_starts_per_scene`).  The result gains ``'scenes'``, the
    geometry of the accepted instances, and the returned mask has one entry per requested instance (False too where the
    candidates ran out).  A track [n, T, n_rows, 8] with a safe-set network that has a context (``ctx_select``): the network row
    of node k is given the context of the column its collision rows read (solver.set_instance_context_track).

    ``traj`` ([3, L], tracking.tracking_trajectory): the tracking branch, guess_acados.py:167-226.  The controller follows the curve
    (setTrajectory: p[:, i, :3] = traj[:, i]) and every start state comes from :func:`ik_starts` at ``traj[:, 0]`` -- instance i in
    its scene where ``scenes`` is given -- instead of the Halton filter; the guess is constant at it, as the reference builds it,
    and the SQP and checkGuess are the same.  An instance whose IK found no solution is dropped, never replaced: its entry of the
    returned mask (one per requested instance) is False and the result's ``'ik_failed'`` lists it.
    ``traj`` [n, 3, L] (tracking.tracking_curves / jittered_curves): a curve of its own for every instance -- instance i starts from
    an IK solution at ``traj[i, :, 0]`` and follows ``traj[i]`` (p[i, k, :3] = traj[i, :, k]); the result gains ``'curves'``, the
    curves of the accepted instances.

    ``models`` (``JOINT_DTYPE`` [n, nq], ``perturbed_joint_tables``): a warm start for the robot it will run on -- instance i is
    solved and tested with the link inertials of ``models[i]`` (solver.set_instance_models; the start states do not depend on them).
    The result gains ``'models'``, the tables of the accepted instances; the solver is left without a table."""
    make_controller = make_controller or (lambda name, batch: get_controller(name, params, batch))
    if models is not None:
        models = np.ascontiguousarray(models)
        if models.dtype != JOINT_DTYPE or models.ndim != 2 or models.shape[0] != n:
            raise ValueError(f'models: expected a JOINT_DTYPE table [{n}, nq], got {models.dtype} {models.shape}')
    ctrl = make_controller(cont_name, n)
    if models is not None:
        _require(ctrl.ocp_solver, 'models', 'set_instance_models')
    curves = traj is not None and np.ndim(traj) == 3
    if traj is not None:
        traj = np.ascontiguousarray(traj, np.float64)
        if curves and (traj.shape[0] != n or traj.shape[1] != 3):
            raise ValueError(f'traj: expected [3, L] or [{n}, 3, L], got {traj.shape}')
        ctrl.setTrajectory(traj)
    if on_device and not hasattr(ctrl.ocp_solver, 'sqp'):
        raise ValueError(f'generate_guess(on_device=True) needs a solver with a device SQP (BatchedOcpSolver.sqp); '
                         f'{type(ctrl.ocp_solver).__name__} has none')
    pr = ctrl.problem
    nq = pr.nq

    q = pr.x_min[:nq] + halton(4 * n + 16, nq) * (pr.x_max[:nq] - pr.x_min[:nq])        # guess_acados.py:100
    x_all = np.hstack([q, np.zeros_like(q)])
    ik_failed = None
    if traj is not None:
        if scenes is not None:
            scenes = _check_scenes(scenes, n, pr)
        x0, ik_info = ik_starts(ctrl.ocp_solver, pr, traj[:, :, 0] if curves else traj[:, 0], n, scenes=scenes)   # guess_acados.py:179-183
        filled = ik_info[:, 1] > 0
        ik_failed = np.where(~filled)[0]
        if verbose and len(ik_failed):
            print(f'inverse kinematics: no start state for {len(ik_failed)} of {n} instances: {ik_failed.tolist()}')
        x0 = x0[filled]
        scenes = scenes[filled] if scenes is not None else None
        traj = traj[filled] if curves else traj
    elif scenes is not None:
        scenes = _check_scenes(scenes, n, pr)
        x0, filled = _free_starts_per_scene(ctrl.ocp_solver, scenes, x_all)
        x0, scenes = x0[filled], scenes[filled]
    else:
        filled = None
        free = np.asarray(ctrl.ocp_solver.check_trajectory(x_all[:, None, :], tol_x=0.0))      # guess_acados.py:109
        x0 = x_all[free][:n]
    if len(x0) < n:
        ctrl = make_controller(cont_name, len(x0))
        if traj is not None:
            ctrl.setTrajectory(traj)
    B = len(x0)
    if models is not None:
        models = models[filled] if filled is not None else models[:B]      # (instance k of B is the k-th start that was found)
        if B:
            _set_models(ctrl.ocp_solver, models)
    if scenes is not None and B:
        _set_scene(ctrl.ocp_solver, scenes)
        if hasattr(ctrl.ocp_solver, 'set_scene_clock'):
            ctrl.ocp_solver.set_scene_clock(None)       # (a track: the guess is made at time 0, node k in column min(k, T - 1))

    def result(good):
        out = {'xg': ctrl.x_guess[good], 'ug': ctrl.u_guess[good]}
        if models is not None:
            out['models'] = models[good]
            _set_models(ctrl.ocp_solver, None)
        if ik_failed is not None:
            out['ik_failed'] = ik_failed
        if filled is None:
            return out, good
        if scenes is not None:
            out['scenes'] = scenes[good]
        if curves:
            out['curves'] = traj[good]
        mask = np.zeros(n, bool)
        mask[np.where(filled)[0][good]] = True
        return out, mask

    ctrl.setGuess(np.repeat(x0[:, None, :], ctrl.N + 1, axis=1), np.zeros((B, ctrl.N, ctrl.nu)))
    if on_device:
        status = _sqp_on_device(ctrl, x0, int(params.nlp_max_iter), history, verbose,
                                dict(tol=sqp_tol, armijo=armijo, alpha_reduction=alpha_reduction, alpha_min=alpha_min))
        ctrl.x_temp, ctrl.u_temp = ctrl.x_guess.copy(), ctrl.u_guess.copy()
        good = ((status == 0) | (status == 2)) & ctrl.checkGuess()
        return result(good)
    state = new_host_sqp_state(B)
    sqp_host_advance(ctrl, x0, state, int(params.nlp_max_iter), sqp_tol=sqp_tol, armijo=armijo, alpha_reduction=alpha_reduction,
                     alpha_min=alpha_min, history=history, verbose=verbose)
    status = state['status']
    ctrl.x_temp, ctrl.u_temp = ctrl.x_guess.copy(), ctrl.u_guess.copy()
    good = ((status == 0) | (status == 2)) & ctrl.checkGuess()              # guess_acados.py:115 accepts status 0 or 2
    return result(good)


class GuessSlots:
    """Bookkeeping of :func:`generate_guess_until`: which sample of the stream sits in which of ``batch`` slots, who was accepted,
    who failed.  No arrays, no engine: samples are numbers 0, 1, 2, .. in sampling order.

    :meth:`issue` hands out the next samples to free slots, but only while ``accepted + in_flight < n`` -- so never more are in
    flight than could still be needed.  :meth:`resolve` records a slot's fate and frees it.  When nothing is in flight and nothing
    can be issued, the issued samples are a prefix of the stream, all resolved, with exactly ``n`` accepted (fewer only when
    ``max_samples`` ran out): the first ``n`` accepted in sampling order, whatever ``batch`` was."""

    def __init__(self, n, batch=None, max_samples=None):
        self.n = int(n)
        self.batch = max(1, min(int(batch) if batch else self.n, self.n)) if self.n > 0 else 0
        self.max_samples = None if max_samples is None else int(max_samples)
        self.slot_sample = [None] * self.batch      # sample in each slot, None = free
        self._free = list(range(self.batch))        # free slots as a min-heap: the lowest free slot is filled first
        self.in_flight = 0                          # slots that hold a sample (kept as a count: issue() asks for it per slot)
        self.issued = 0                             # samples handed out so far = index of the next one
        self.accepted, self.failed = [], []         # sample indices, in the order they were resolved

    @property
    def exhausted(self):
        """max_samples ran out before n samples were accepted"""
        return (self.max_samples is not None and self.issued >= self.max_samples and self.in_flight == 0
                and len(self.accepted) < self.n)

    def live(self):
        """[(slot, sample)] of the slots in flight, by slot"""
        return [(k, s) for k, s in enumerate(self.slot_sample) if s is not None]

    def issue(self):
        """fill free slots with the next samples while accepted + in_flight < n; returns [(slot, sample)] issued now"""
        out = []
        while self._free and len(self.accepted) + self.in_flight < self.n:
            if self.max_samples is not None and self.issued >= self.max_samples:
                break
            k = heapq.heappop(self._free)
            self.slot_sample[k] = self.issued
            self.in_flight += 1
            out.append((k, self.issued))
            self.issued += 1
        return out

    def resolve(self, slot, accepted):
        s = self.slot_sample[slot]
        if s is None:
            raise ValueError(f'slot {slot} is free')
        (self.accepted if accepted else self.failed).append(s)
        self.slot_sample[slot] = None
        heapq.heappush(self._free, slot)
        self.in_flight -= 1
        return s

    def finished(self):
        return self.in_flight == 0 and (len(self.accepted) >= self.n or
                                        (self.max_samples is not None and self.issued >= self.max_samples))

    def result_order(self):
        """accepted samples in sampling order: the order of the returned guesses"""
        return sorted(self.accepted)


class _FreeStarts:
    """The sample stream of generate_guess in chunks: Halton q0 in the joint box at rest (guess_acados.py:100), collision filter
    (:109).  ``take(j)`` = the j-th free start, whatever the chunking.  A filter that lets nothing through (check bounds that no
    configuration meets, a fully obstructed box) would draw for ever: after ``max_barren`` chunks in a row without one free start
    ``take`` raises."""

    def __init__(self, solver, problem, chunk=256, max_barren=64):
        self.sv, self.pr, self.chunk, self.max_barren = solver, problem, int(chunk), int(max_barren)
        self.drawn = 0
        self.x = np.zeros((0, problem.nx))

    def take(self, j):
        pr, nq = self.pr, self.pr.nq
        barren = 0
        while j >= len(self.x):
            q = pr.x_min[:nq] + halton(self.chunk, nq, skip=1 + self.drawn) * (pr.x_max[:nq] - pr.x_min[:nq])
            self.drawn += self.chunk
            x_all = np.hstack([q, np.zeros_like(q)])
            free = np.asarray(self.sv.check_trajectory(x_all[:, None, :], tol_x=0.0)).astype(bool)
            barren = 0 if free.any() else barren + 1
            if barren >= self.max_barren:
                raise RuntimeError(f'the collision filter rejected {barren * self.chunk} Halton starts in a row ({self.drawn} drawn, '
                                   f'{len(self.x)} free so far): no collision-free start to sample')
            self.x = np.vstack([self.x, x_all[free]])
        return self.x[j]


def generate_guess_until(params, cont_name, n, batch=None, check_every=50, accept='final', max_samples=None, make_controller=None,
                         sqp_tol=1e-6, verbose=False, armijo=1e-4, alpha_reduction=0.7, alpha_min=0.05, scenes=None, traj=None,
                         models=None):
    """guess_acados.py:98-158 with its ``while succ < num_ics``: sample, solve and test warm starts until ``n`` are ACCEPTED, on
    the device.  Returns ``(guess, info)``: ``guess['xg'] [n, N+1, nx]``, ``guess['ug'] [n, N, nu]`` in sampling order.

    The sample stream is :func:`generate_guess`'s (sample j = its j-th collision-free Halton start, constant guess, mu = mu0).
    ``B = min(batch or n, n)`` slots live on the device.  A round is ``solver.sqp(max_iter=check_every)`` on all slots followed by
    one ``solver.check_guess`` (smpc_check_guess) on the live ones; the host then reads flags, status, done and iters -- a few
    bytes per slot -- and decides each live sample's fate:

    * ``accept='final'`` (the reference's rule, what generate_guess applies): once the sample is done or has used its budget, it
      is accepted if ``status in (0, 2)`` and ``flags == 0`` and fails otherwise.
    * ``accept='first'``: accepted at the first round where ``status == 0`` and ``flags == 0``; it fails when it is done
      otherwise or has used its budget.

    The budget is ``params.nlp_max_iter`` ROUNDED UP to a multiple of ``check_every``: samples are only looked at between rounds.
    Resolved slots get ``done = 1`` in the SQP state, so they cost nothing until they are refilled, which happens only between
    rounds and only while ``accepted + in_flight < n`` (:class:`GuessSlots`).  The result is therefore the first ``n`` accepted
    samples of the stream in sampling order, whatever ``batch`` is.  WHICH samples those are, and their bits, do not depend on
    ``batch`` only if a sample's SQP does not: the engine picks the form of the QP solve and the network kernel by the width of the
    launch (smpc_set_qp_mode 'auto'), the forms agree to rounding, and over hundreds of iterations rounding can move an iteration
    count.  Pin the form through ``make_controller`` (``ctrl.ocp_solver.set_qp_mode('throughput')``) where bit-identical results
    across batch sizes are wanted; the tests do.  With ``max_samples`` the stream stops after that many
    samples and ``info['exhausted']`` says whether that cut the result short.

    ``traj`` ([3, L]): the tracking branch (guess_acados.py:167-226, see :func:`generate_guess`): the controller follows the curve
    and sample j is the j-th instance of :func:`ik_starts` at ``traj[:, 0]`` whose IK succeeded; the instances without a solution are
    listed in ``info['ik_failed']`` and are not part of the stream.

    ``info``: 'accepted' / 'failed' (sample indices, sampling order), 'iters' (SQP iterations of every issued sample),
    'status', 'flags' (at the sample's resolution), 'issued', 'rounds', 'instance_iterations', 'exhausted'."""
    if scenes is not None:
        raise ValueError('generate_guess_until: per-instance scenes are not supported (a refilled slot would need the scene of its '
                         'new sample); use generate_guess(scenes=...)')
    if traj is not None and np.ndim(traj) == 3:
        raise ValueError('generate_guess_until: per-instance curves are not supported (a refilled slot would need a curve for its '
                         'new sample); use generate_guess(traj=[n, 3, L])')
    if models is not None:
        raise ValueError('generate_guess_until: per-instance models are not supported (a refilled slot would be a new sample in an old '
                         'robot); use generate_guess(models=[n, nq])')
    if accept not in ('final', 'first'):
        raise ValueError("accept must be 'final' or 'first'")
    check_every = int(check_every)
    if check_every < 1:
        raise ValueError('check_every must be >= 1')
    make_controller = make_controller or (lambda name, batch: get_controller(name, params, batch))
    book = GuessSlots(n, batch, max_samples)
    B = max(book.batch, 1)
    ctrl = make_controller(cont_name, B)
    sv = ctrl.ocp_solver
    if not hasattr(sv, 'sqp') or not hasattr(sv, 'check_guess'):
        raise ValueError(f'generate_guess(on_device=True) needs a solver with a device SQP (BatchedOcpSolver.sqp); '
                         f'{type(sv).__name__} has none')
    N, nx, nu = ctrl.N, ctrl.nx, ctrl.nu
    info = {'accepted': [], 'failed': [], 'iters': {}, 'status': {}, 'flags': {}, 'issued': 0, 'rounds': 0, 'instance_iterations': 0,
            'exhausted': False}
    if n <= 0:
        return {'xg': np.zeros((0, N + 1, nx)), 'ug': np.zeros((0, N, nu))}, info
    import torch
    dev = torch.device('cuda', sv.device)
    if traj is not None:
        traj = np.ascontiguousarray(traj, np.float64)
        ctrl.setTrajectory(traj)
    ctrl.p[:, :, 3] = ctrl.params.alpha                     # what ctrl.solve does before every solve
    ctrl._apply_traj()
    to = lambda a: torch.as_tensor(np.ascontiguousarray(np.asarray(a), np.float64), device=dev)
    p_d = to(ctrl.p)
    x0_d = torch.zeros((B, nx), dtype=torch.float64, device=dev)
    xg = torch.zeros((B, N + 1, nx), dtype=torch.float64, device=dev)
    ug = torch.zeros((B, N, nu), dtype=torch.float64, device=dev)
    opts = dict(tol=sqp_tol, armijo=armijo, alpha_reduction=alpha_reduction, alpha_min=alpha_min)
    from ._lib import SqpOpts, SqpState
    mu0 = SqpOpts().mu0                                     # generate_guess' start value of the penalty
    state = sv.new_sqp_state(B, x0_d, mu0)
    state['done'].fill_(1)                                  # a free slot is a finished instance: every kernel skips it
    flags_d = torch.zeros((B,), dtype=torch.int32, device=dev)
    worst_d = torch.zeros((B, 5), dtype=torch.float64, device=dev)
    mask_d = torch.zeros((B,), dtype=torch.uint8, device=dev)
    safe_node = N if getattr(ctrl, 'guess_safe_node', False) else None
    budget = -(-int(params.nlp_max_iter) // check_every) * check_every
    stream = _FreeStarts(sv, ctrl.problem) if traj is None else _IkStarts(sv, ctrl.problem, traj[:, 0])
    got_x, got_u = {}, {}
    while True:
        new = book.issue()
        if new:
            slots = torch.as_tensor([k for k, _ in new], dtype=torch.long, device=dev)
            xs = to(np.stack([stream.take(j) for _, j in new]))
            x0_d[slots] = xs
            xg[slots] = xs[:, None, :].expand(-1, N + 1, -1)
            ug[slots] = 0.0
            for key, _ in SqpState.FIELDS:                      # a fresh sample: the state new_sqp_state would give it
                state[key][slots] = mu0 if key == 'mu' else 0
        live = book.live()
        if not live:
            break
        sv.sqp(x0_d, xg, ug, p_d, dict(max_iter=check_every, **opts), state)
        mask_d.zero_()
        live_slots = torch.as_tensor([k for k, _ in live], dtype=torch.long, device=dev)
        mask_d[live_slots] = 1
        sv.check_guess(xg, ug, safe_node=safe_node, mask=mask_d, flags=flags_d, worst=worst_d)
        small = torch.stack([flags_d, state['status'], state['done'].to(torch.int32), state['iters']]).cpu().numpy()
        fl, st, dn, it = small
        info['rounds'] += 1
        take, resolved = [], []
        for k, j in live:
            ended = bool(dn[k]) or it[k] >= budget
            if accept == 'final':
                ok = ended and st[k] in (0, 2) and fl[k] == 0
            else:
                ok = st[k] == 0 and fl[k] == 0
            if not (ok or ended):
                continue
            book.resolve(k, ok)
            resolved.append(k)
            info['iters'][j], info['status'][j], info['flags'][j] = int(it[k]), int(st[k]), int(fl[k])
            if ok:
                take.append((k, j))
        if resolved:
            state['done'][torch.as_tensor(resolved, dtype=torch.long, device=dev)] = 1
        if take:
            ts = torch.as_tensor([k for k, _ in take], dtype=torch.long, device=dev)
            hx, hu = xg[ts].cpu().numpy(), ug[ts].cpu().numpy()
            for i, (_, j) in enumerate(take):
                got_x[j], got_u[j] = hx[i], hu[i]
        if verbose:
            print(f'round {info["rounds"]}: {len(book.accepted)}/{n} accepted, {len(book.failed)} failed, {book.in_flight} in flight, '
                  f'{book.issued} issued')
    sv.sync()
    order = book.result_order()
    info.update(accepted=order, failed=sorted(book.failed), issued=book.issued, exhausted=book.exhausted,
                instance_iterations=int(sum(info['iters'].values())))
    if traj is not None:
        info['ik_failed'] = list(stream.failed)
    xg_out = np.stack([got_x[j] for j in order]) if order else np.zeros((0, N + 1, nx))
    ug_out = np.stack([got_u[j] for j in order]) if order else np.zeros((0, N, nu))
    return {'xg': xg_out, 'ug': ug_out}, info


# ---- closed loop -----------------------------------------------------------------------------------------------------------------
_STATE = ('x_guess', 'u_guess', 'fails', 'current_step', 'x_viable', 'r')


# ---- scores of a closed-loop run ------------------------------------------------------------------------------------------
def _score_eval_chunks(solver, problem, states, alpha, chunk, safe):
    """ee [M, 3] and row_val [M, n_rows] of M states (``safe`` false), or g [M] (``safe`` true), through ``solver.eval_nodes``, at
    most ``chunk`` states per call.  The states are packed into the nodes of evaluated trajectories: all N + 1 nodes for ee /
    row_val, the nodes that carry the safe-set row for g (1..N with the row on every node, node N alone otherwise)."""
    N, nx, nr = solver.N, problem.nx, int(problem.desc.n_rows)
    M = states.shape[0]
    ee, rows, g = np.zeros((M, 3)), np.zeros((M, nr)), np.zeros(M)
    nodes = slice(0, N + 1) if not safe else (slice(1, N + 1) if int(problem.desc.nn_mode) == 2 else slice(N, N + 1))
    per = nodes.stop - nodes.start
    for lo in range(0, M, chunk):
        s = states[lo:lo + chunk]
        m = s.shape[0]
        packed = np.zeros((-(-m // per) * per, nx))
        packed[:m] = s
        xg = np.zeros((packed.shape[0] // per, N + 1, nx))
        xg[:, nodes] = packed.reshape(-1, per, nx)
        p = np.zeros((xg.shape[0], N + 1, 5))
        p[:, :, 3], p[:, :, 4] = alpha, 1.0
        ev = solver.eval_nodes(xg, np.zeros((xg.shape[0], N, problem.nu)), p)
        if safe:
            g[lo:lo + m] = np.asarray(ev['nn_val'])[:, nodes].reshape(-1)[:m]
        else:
            ee[lo:lo + m] = np.asarray(ev['ee']).reshape(-1, 3)[:m]
            rows[lo:lo + m] = np.asarray(ev['row_val']).reshape(-1, np.asarray(ev['row_val']).shape[-1])[:m, :nr]
    return ee, rows, g


def _score_eval_instances(solver, problem, x, alpha, safe, scene_clock=None):
    """:func:`_score_eval_chunks` for a solver that holds a scene per instance: every call evaluates all B instances, instance b's
    own states packed into the nodes of ITS trajectory (so its rows are formed in its scene).  x [B, M, nx] -> the same three
    arrays for the B * M states, instance-major.  ``scene_clock``: the cell of ``solver.set_scene_clock`` when the solver holds a
    scene TRACK -- a call that packs the states j0, j0 + 1, .. into the nodes n0, n0 + 1, .. runs at time j0 - n0, so that state
    j is formed in column clip(j, 0, T - 1): the log starts at time 0."""
    N, nx, nr = solver.N, problem.nx, int(problem.desc.n_rows)
    B, M = x.shape[0], x.shape[1]
    ee, rows, g = np.zeros((B, M, 3)), np.zeros((B, M, nr)), np.zeros((B, M))
    nodes = slice(0, N + 1) if not safe else (slice(1, N + 1) if int(problem.desc.nn_mode) == 2 else slice(N, N + 1))
    per = nodes.stop - nodes.start
    p = np.zeros((B, N + 1, 5))
    p[:, :, 3], p[:, :, 4] = alpha, 1.0
    for lo in range(0, M, per):
        m = min(per, M - lo)
        xg = np.zeros((B, N + 1, nx))
        xg[:, nodes.start:nodes.start + m] = x[:, lo:lo + m]
        _write_scene_clock(scene_clock, lo - nodes.start)
        ev = solver.eval_nodes(xg, np.zeros((B, N, problem.nu)), p)
        sl = slice(nodes.start, nodes.start + m)
        if safe:
            g[:, lo:lo + m] = np.asarray(ev['nn_val'])[:, sl]
        else:
            ee[:, lo:lo + m] = np.asarray(ev['ee'])[:, sl]
            rows[:, lo:lo + m] = np.asarray(ev['row_val'])[:, sl, :nr]
    return ee.reshape(-1, 3), rows.reshape(-1, nr), g.reshape(-1)


def score_rollout_statement(solver, problem, params, x_log, u_log, last_x=None, last_u=None, ee_ref=None, traj=None, want_safe=False,
                            chunk=4096, per_instance=False, scene_clock=None, **bounds):
    """The readable numpy statement of ``BatchedOcpSolver.score_rollout`` (smpc_score_rollout, include/smpc.h), and the host path of
    ``run_mpc(score=True)``.  STEP-major logs ``x_log [T+1, B, nx]``, ``u_log [T, B, nu]``; ``last_x`` / ``last_u`` [B]: last valid
    row of each, None = complete; rows past them affect nothing.  Returns ``(out [B, 7], outi [B, 4] int32)`` with the columns
    ``solver.SCORE_SLOTS`` / ``SCORE_INDEX_SLOTS``:

    * cost = Q ee_err2 + R u2 (metrics_count_fails.py:19-28 for a complete log), ee_err2 = sum_{j <= last_x} |ee(x_j) - ref_j|^2,
      u2 = sum_{j <= last_u} |u_j|^2, ee_dist = |ee(x_last_x) - ref_last_x| (what mpc.py:273 compares with tol_conv);
      ref_j = ``ee_ref`` (default: the problem's) or column min(j, L - 1) of ``traj [3, L]`` -- of ``traj[b]`` for instance b
      with ``traj [B, 3, L]``
    * coll_margin = max over j <= last_x and rows of max(row_lb - v, v - row_ub) (env_model.py:236-243), -inf without rows;
      box_margin = max over j <= last_x and components of max(x_min - x, x - x_max) (env_model.py:170-172);
      safe_min = min over j <= last_x of g(x_j, alpha) (safe_set.py:61-68), +inf unless ``want_safe``
    * coll_step, coll_row, box_step, safe_step: where they were taken, earliest step then lowest row among equals; -1 where there is
      nothing.  A NaN in a valid row makes the values it enters NaN (placed at the first one).

    Uses only ``solver.eval_nodes`` (``ee``, ``row_val``; ``nn_val`` for g), ``chunk`` states per call -- or, with ``per_instance``
    (the solver holds a scene per instance, set_instance_scene), all B instances per call with every instance's states in its own
    trajectory.  With a scene TRACK on the solver (set_instance_scene_track) pass ``scene_clock``, the cell handed to
    ``solver.set_scene_clock``: state j of the log is then evaluated in column clip(j, 0, T - 1) of its instance's track, as
    smpc_score_rollout does (the statement writes the cell before every call and leaves it at its last value)."""
    x = np.transpose(np.asarray(x_log, float), (1, 0, 2))          # [B, T+1, nx]
    u = np.transpose(np.asarray(u_log, float), (1, 0, 2))          # [B, T, nu]
    B, T = u.shape[0], u.shape[1]
    unknown = set(bounds) - {'x_min', 'x_max', 'row_lb', 'row_ub', 'alpha', 'tol_safe'}
    if unknown:
        raise TypeError(f'score_rollout_statement: unknown argument(s) {sorted(unknown)}')
    if T < 1:
        raise ValueError('a log has at least one step')
    nr = int(problem.desc.n_rows)
    x_min, x_max = np.asarray(bounds.get('x_min', problem.x_min), float), np.asarray(bounds.get('x_max', problem.x_max), float)
    row_lb = np.asarray(bounds.get('row_lb', problem.row_check[:, 0]), float)
    row_ub = np.asarray(bounds.get('row_ub', problem.row_check[:, 1]), float)
    alpha = float(bounds.get('alpha', params.alpha))
    lx = np.full(B, T, np.int64) if last_x is None else np.clip(np.asarray(last_x, np.int64), 0, T)
    lu = np.full(B, T - 1, np.int64) if last_u is None else np.clip(np.asarray(last_u, np.int64), -1, T - 1)
    steps = np.arange(T + 1)
    vx, vu = steps[None, :] <= lx[:, None], steps[None, :T] <= lu[:, None]           # valid rows
    if traj is not None:
        traj = np.asarray(traj, float)
        if traj.ndim == 3:
            if traj.shape[0] != B or traj.shape[1] != 3:
                raise ValueError(f'traj: expected [3, L] or [{B}, 3, L], got {traj.shape}')
            ref = np.transpose(traj[:, :, np.minimum(steps, traj.shape[2] - 1)], (0, 2, 1))      # [B, T+1, 3]
        else:
            ref = traj[:, np.minimum(steps, traj.shape[1] - 1)].T[None, :, :]         # [1, T+1, 3]
    else:
        ref = np.asarray(problem.ee_ref if ee_ref is None else ee_ref, float)[None, None, :]
    flat = np.where(vx[:, :, None], x, 0.0).reshape(-1, x.shape[2])                  # invalid rows: any finite state, masked below
    if per_instance:
        ee, rv, _ = _score_eval_instances(solver, problem, flat.reshape(B, T + 1, -1), alpha, False, scene_clock)
    else:
        ee, rv, _ = _score_eval_chunks(solver, problem, flat, alpha, chunk, False)
    e2 = np.sum((ee.reshape(B, T + 1, 3) - ref) ** 2, axis=2)
    out, outi = np.zeros((B, 7)), np.full((B, 4), -1, np.int32)
    out[:, 1] = np.where(vx, e2, 0.0).sum(1)
    out[:, 2] = np.sum(np.where(vu[:, :, None], u, 0.0) ** 2, axis=2).sum(1)
    out[:, 0] = params.Q_weight * out[:, 1] + params.R_weight * out[:, 2]
    out[:, 3] = np.sqrt(e2[np.arange(B), lx])
    out[:, 4] = -np.inf
    if nr:
        rv = rv.reshape(B, T + 1, nr)
        m = np.where(vx[:, :, None], np.maximum(row_lb - rv, rv - row_ub), -np.inf).reshape(B, -1)
        at = np.argmax(m, axis=1)                       # first occurrence in (step, row) order; a NaN counts as the maximum
        out[:, 4], outi[:, 0], outi[:, 1] = m[np.arange(B), at], at // nr, at % nr
    mb = np.where(vx, np.max(np.maximum(x_min - x, x - x_max), axis=2), -np.inf)
    at = np.argmax(mb, axis=1)
    out[:, 5], outi[:, 2] = mb[np.arange(B), at], at
    out[:, 6] = np.inf
    if want_safe:
        if int(problem.desc.nn_mode) == 0:
            raise ValueError('want_safe needs a formulation with a safe-set row (eval_nodes reports g on the nodes that carry it)')
        if per_instance:
            _, _, g = _score_eval_instances(solver, problem, flat.reshape(B, T + 1, -1), alpha, True, scene_clock)
        else:
            _, _, g = _score_eval_chunks(solver, problem, flat, alpha, chunk, True)
        g = np.where(vx, g.reshape(B, T + 1), np.inf)
        at = np.argmin(g, axis=1)
        out[:, 6], outi[:, 3] = g[np.arange(B), at], at
    return out, outi


def _score_dict(out, outi):
    from .solver import SCORE_INDEX_SLOTS, SCORE_SLOTS
    return {**{k: np.array(out[:, i]) for i, k in enumerate(SCORE_SLOTS)},
            **{k: np.array(outi[:, i]) for i, k in enumerate(SCORE_INDEX_SLOTS)}}


def _masked_step(ctrl, x, active):
    """controller.step on all rows, then roll back the rows that must not have stepped (host state: numpy)."""
    snap = {k: np.copy(getattr(ctrl, k)) for k in _STATE if hasattr(ctrl, k)}
    u, abort = ctrl.step(x)
    for k, v in snap.items():
        cur = getattr(ctrl, k)
        m = active.reshape((-1,) + (1,) * (cur.ndim - 1))
        setattr(ctrl, k, np.where(m, cur, v))
    return u, abort & active


class _Forecast:
    """What the controller forecasts the world with (run_mpc(forecast=, forecast_window=, forecast_degree=); DESIGN.md sections 9n-9p):
    'hold', 'cv', 'true', or 'fit' -- a least-squares polynomial of ``degree`` through the last ``window`` columns seen -- and the one
    place that tells the kinds apart, on the host path and the device path.  Degree 1 keeps the line fit's own statement and entry point."""

    def __init__(self, kind, window=None, degree=None, kalman=None):
        self.kind, self._fit, self.is_kalman = kind, kind == 'fit', kind == 'kalman'
        self.window, self.degree = int(window) if self._fit else None, 1 if degree is None else int(degree)
        self._poly = self._fit and self.degree != 1
        self.kalman = self.par = None       # (q, r, v0, a0, beta) as the result reports it, and the model as the entry points take it
        if self.is_kalman:
            from .problem import kalman_params
            self.par = kalman_params(self.degree, *kalman, who='kalman')
            self.kalman = tuple(float(getattr(self.par, k)) for k in ('q', 'r', 'v0', 'a0', 'beta'))

    @classmethod
    def checked(cls, kind, window, degree, scenes, kalman=None):
        """run_mpc's forecast arguments against its (checked) ``scenes``: the spec, None without a forecast, or ValueError"""
        if kalman is not None and kind != 'kalman':
            raise ValueError(f"kalman: forecast={kind!r} has no filter: it goes with forecast='kalman'")
        if kind is not None:
            from .problem import FIT_MAX, FORECAST_MODES
            if kind not in ('fit', 'kalman') and kind not in FORECAST_MODES:
                raise ValueError(f"forecast: {kind!r}: expected None, 'fit' or one of {sorted(FORECAST_MODES)}, or 'kalman'")
            if kind == 'kalman':
                if kalman is None:
                    raise ValueError("kalman: forecast='kalman' needs kalman=(q, r[, v0, a0, beta])")
                kalman = tuple(np.asarray(kalman, float).reshape(-1))
                if not 2 <= len(kalman) <= 5:
                    raise ValueError(f'kalman: expected (q, r[, v0, a0, beta]), got {kalman}')
            if kind == 'fit' and not (isinstance(window, (int, np.integer)) and 1 <= window <= FIT_MAX):
                raise ValueError(f'forecast_window: {window!r}: a fit takes 1 to {FIT_MAX} columns')
            if scenes is None or scenes.ndim != 4:
                raise ValueError('forecast: needs a scene track (scenes [B, T, n_rows, 8]) to forecast from; '
                                 + ('no scenes were given' if scenes is None else 'standing scenes have nothing to predict'))
        if degree is not None:
            if kind not in ('fit', 'kalman'):
                raise ValueError(f"forecast_degree: forecast={kind!r} has no degree: it goes with forecast='fit' or 'kalman'")
            if not (isinstance(degree, (int, np.integer)) and 0 <= degree <= 2):
                raise ValueError(f'forecast_degree: {degree!r}: a polynomial fit has degree 0, 1 or 2')
        return None if kind is None else cls(kind, window, degree, kalman)     # (a bad kalman tuple: kalman_params' ValueError)

    def statement(self, world, observed, rows, t, N, state=None, advance=True):
        """the host path: the N + 1 scenes forecast at time t for the instances ``rows``, by the statement of the engine's entry point.
        'hold', 'cv', 'fit' (of any degree) and 'kalman' are formed from what was seen, the observed track where the run has one; 'true'
        from the world.  'kalman': ``state`` is the filter state of the instances ``rows`` -- advanced IN PLACE by the column seen at
        time t with ``advance``, only read without"""
        from .problem import fit_forecast_statement, forecast_statement, poly_forecast_statement
        seen = world if observed is None or self.kind == 'true' else observed
        if self.is_kalman:
            from .problem import kalman_statement, scene_column
            y = seen[rows][:, scene_column(t, seen.shape[1])] if advance else None
            new, F = kalman_statement(state, y, self._kinds, self.par, N, advance)
            if advance:
                state[...] = new
            return F
        if not self._fit:
            return forecast_statement(seen[rows], t, N, self.kind)
        if not self._poly:
            return fit_forecast_statement(seen[rows], t, N, self.window)
        return poly_forecast_statement(seen[rows], t, N, self.window, self.degree)

    def enqueue(self, sv, select, state=None, advance=True):
        """the device path: one forecast from ``sv``'s world (and observed track) at its clock cell, into its scene slot.  'kalman':
        one step of the filter on the device tensor ``state`` first (``advance``), or the forecast from it as it is"""
        if self.is_kalman:
            sv.forecast_scene_kalman(self.par, state, advance, select)
        elif self._poly:
            sv.forecast_scene_poly(self.window, self.degree, select)
        elif self._fit:
            sv.forecast_scene_fit(self.window, select)
        else:
            sv.forecast_scene(self.kind, select)

    def margin_statement(self, prob, state, z, base, cap):
        """the host path of a margin from the filter's covariance: d [B, N + 1, n_rows] for the records ``state``"""
        from .problem import kalman_margin_statement
        return kalman_margin_statement(prob, state, self.par, z, base, cap)

    def enqueue_margin(self, sv, state, z, base, cap):
        sv.kalman_row_margin(self.par, state, z, base, cap)

    def bind(self, problem):
        """the row kinds of the run's problem, which the filter's statement takes"""
        self._kinds = [int(r.kind) for r in problem.rows]

    def require(self, sv, observed, margin=False):
        """ValueError unless ``sv`` has the entry points :meth:`enqueue` calls (and takes an observed track, for a run with one)"""
        for need, feature, method in ((True, 'forecast', 'forecast_scene'), (self._fit, 'forecast', 'forecast_scene_fit'),
                                      (self.is_kalman, 'forecast', 'forecast_scene_kalman'),
                                      (self.is_kalman and margin, 'row_margin_kalman', 'kalman_row_margin'),
                                      (self._poly, 'forecast_degree', 'forecast_scene_poly'), (observed, 'observed', 'set_instance_observed_track')):
            if need:
                _require(sv, feature, method)

    def result_keys(self, observed):
        return {'forecast': self.kind, 'observed': bool(observed), **({'forecast_window': self.window} if self._fit else {}),
                **({'forecast_degree': self.degree} if self._poly else {}),
                **({'forecast_degree': self.degree, 'kalman': self.kalman} if self.is_kalman else {})}

    def file_suffix(self):
        if self.is_kalman:
            return '_fckalman_d{}_q{}_r{}_v{}_a{}_b{}'.format(self.degree, *self.kalman)
        return f"_fc{self.kind}{f'_w{self.window}' if self._fit else ''}{f'_d{self.degree}' if self._poly else ''}"


class _RunWorld(namedtuple('_RunWorld', 'scenes models forecast observed row_margin row_margin_fit row_margin_kalman', defaults=(None,) * 7)):
    """run_mpc's ``scenes``, ``models``, ``forecast*`` (a :class:`_Forecast`), ``observed``, ``row_margin`` and ``row_margin_fit``, checked
    (:func:`_check_world`): of the whole run, or of one group's instances (:meth:`rows`)"""

    def rows(self, lo, hi):
        cut = lambda a: a if a is None or isinstance(a, str) else a[lo:hi]
        return self._replace(scenes=cut(self.scenes), models=cut(self.models), observed=cut(self.observed))


def _check_world(B, cont_name, noise, scenes, row_margin, forecast, forecast_window, forecast_degree, observed, models,
                 row_margin_fit=None, kalman=None, row_margin_kalman=None):
    """run_mpc's arguments about the world of its B instances, before anything is built: the :class:`_RunWorld`, or ValueError"""
    for name, given, thing in (('models', models, 'model table'), ('scenes', scenes, 'scene'), ('row_margin', row_margin, 'row-bounds table'),
                               ('row_margin_fit', row_margin_fit, 'row-bounds table'), ('kalman', kalman, 'scene'),
                               ('row_margin_kalman', row_margin_kalman, 'row-bounds table')):
        if cont_name == 'parallel' and given is not None:
            raise ValueError(f"{name}: the 'parallel' policy is not supported (its solver works on candidate slots, not instances, and "
                             f"the engine refuses a {thing} there)")
    if isinstance(models, str):
        if models != 'plant':
            raise ValueError(f"models: {models!r}: expected None, 'plant' or a joint table [{B}, nq]")
        if not noise > 0:
            raise ValueError("models='plant': the plant has a model of its own per instance only with noise > 0")
    elif models is not None:
        models = np.ascontiguousarray(models)
        if models.dtype != JOINT_DTYPE or models.ndim != 2 or models.shape[0] != B:
            raise ValueError(f'models: expected a JOINT_DTYPE table [{B}, nq], got {models.dtype} {models.shape}')
    if scenes is not None:
        scenes = np.ascontiguousarray(scenes, np.float64)
        if scenes.ndim not in (3, 4) or scenes.shape[0] != B:
            raise ValueError(f'scenes: expected [{B}, n_rows, 8] or a track [{B}, T, n_rows, 8], got {scenes.shape}')
    if row_margin is not None:
        row_margin = tuple(float(v) for v in np.asarray(row_margin, float).reshape(-1))
        if len(row_margin) != 2 or not all(np.isfinite(row_margin)):
            raise ValueError(f'row_margin: expected (a, b), the margin a + b k metres at node k, got {row_margin}')
    fc = _Forecast.checked(forecast, forecast_window, forecast_degree, scenes, kalman)
    if row_margin_kalman is not None:
        if forecast != 'kalman':
            raise ValueError(f"row_margin_kalman: forecast={forecast!r} has no covariance to form a margin from: it goes with "
                             f"forecast='kalman'")
        row_margin_kalman = tuple(float(v) for v in np.asarray(row_margin_kalman, float).reshape(-1))
        if len(row_margin_kalman) != 2 or not all(np.isfinite(v) and v >= 0.0 for v in row_margin_kalman):
            raise ValueError(f'row_margin_kalman: expected (z, d_max), finite and not negative, got {row_margin_kalman}')
    if row_margin_fit is not None:
        if forecast != 'fit':
            raise ValueError(f"row_margin_fit: forecast={forecast!r} leaves no residuals to form a margin from: it goes with forecast='fit'")
        row_margin_fit = tuple(float(v) for v in np.asarray(row_margin_fit, float).reshape(-1))
        if len(row_margin_fit) != 3 or not all(np.isfinite(v) and v >= 0.0 for v in row_margin_fit):
            raise ValueError(f'row_margin_fit: expected (z, sigma_prior, d_max), finite and not negative, got {row_margin_fit}')
    if observed is not None:
        if fc is None or fc.kind == 'true':
            raise ValueError(f"observed: forecast={forecast!r} does not read an observed track: it goes with 'hold', 'cv', 'fit' or 'kalman'")
        observed = np.ascontiguousarray(observed, np.float64)
        if observed.shape != scenes.shape:
            raise ValueError(f'observed: expected the world\'s shape {scenes.shape}, got {observed.shape}')
        if not fc.is_kalman and np.isnan(observed).any():
            raise ValueError(f"observed: a NaN (a sample that is missing): only forecast='kalman' skips one, forecast={forecast!r} would carry it "
                             f"into the scenes")
    return _RunWorld(scenes, models, fc, observed, row_margin, row_margin_fit, row_margin_kalman)


def _joint_tensor(xp, table, B, nq):        # [B, nq] smpc_joint records as a float64 device tensor [B, nq, 29]
    return xp.asarray(np.ascontiguousarray(table).view(np.float64).reshape(B, nq, -1), xp.f64)


class _World:
    """Everything ONE group of a run sets on its two solver handles beyond the OCP itself (``run``: the group's :class:`_RunWorld`;
    run_mpc's docstring says what each argument means).  The controller's handle holds the group's scenes or track -- with a forecast
    the track is the WORLD, which only the plant meets, and the scene slot holds what the controller forecasts at the head of every
    step --, its row-bounds table and its models for the whole run; the backup's handle gets the aborting instances' rows of each, over
    its own horizon, before each of its compact solves.  The loop's step counter is the scene clock of both handles."""

    def __init__(self, run, ctrl, backup, B):
        self._run, self._ctrl, self._backup, self._B, self._xp = run, ctrl, backup, B, ctrl.xp
        self._sv, self._bsv, self.forecast, self.track = ctrl.ocp_solver, backup.ocp_solver, run.forecast, False
        self.scenes = self.observed = self.row_bounds = self.models = self.clock = self.backup_clock = self._select = self._backup_select = None
        self.margin_fit = None      # (z, sigma_prior, base, d_max) of a margin formed from the fit's residuals at the head of every step
        self.margin_kalman = None   # (z, base, d_max) of a margin formed from the filter's covariance there
        self.kalman_state = None    # the filter state [B, n_rows, KALMAN_REC]: numpy on the host path, ONE device tensor on the device path
        self._backup_state = None   # its rows of the last abort event, as the backup handle's calls read them

    def attach(self):
        """what the run's arguments alone say: the scenes (without a forecast) and the row bounds onto the controller's handle"""
        run, xp, ctrl, backup, B = self._run, self._xp, self._ctrl, self._backup, self._B
        if run.scenes is not None:
            self.scenes = xp.asarray(_check_scenes(run.scenes, B, ctrl.problem), xp.f64)
            if run.observed is not None:
                self.observed = xp.asarray(_check_scenes(run.observed, B, ctrl.problem), xp.f64)
            self.track = self.scenes.ndim == 4
            if self.forecast is None:
                _set_scene(self._sv, self.scenes)
            if self.track:
                for sv in (self._sv, self._bsv):
                    _require(sv, 'scenes', 'set_scene_clock')
        if self.forecast is not None and self.forecast.is_kalman:
            from .problem import KALMAN_REC
            self.forecast.bind(ctrl.problem)
            self.kalman_state = xp.zeros((B, len(ctrl.problem.rows), KALMAN_REC))
        if run.row_margin_kalman is not None:
            # the margin follows the filter, step by step; row_margin is its base, as for row_margin_fit
            z, cap = run.row_margin_kalman
            self.margin_kalman = (z, (0.0, 0.0) if run.row_margin is None else tuple(float(v) for v in run.row_margin), cap)
            for sv in (self._sv, self._bsv):
                _require(sv, 'row_margin_kalman', 'kalman_row_margin' if xp.on_device else 'set_instance_row_bounds')
        elif run.row_margin_fit is not None:
            # the margin follows the fit, step by step; row_margin is its base, not a table of its own
            z, prior, cap = run.row_margin_fit
            self.margin_fit = (z, prior, (0.0, 0.0) if run.row_margin is None else tuple(float(v) for v in run.row_margin), cap)
            for sv in (self._sv, self._bsv):
                _require(sv, 'row_margin_fit', 'forecast_row_margin' if xp.on_device else 'set_instance_row_bounds')
        elif run.row_margin is not None:
            from .problem import inflated_row_bounds
            for sv in (self._sv, self._bsv):
                _require(sv, 'row_margin', 'set_instance_row_bounds')
            a, g = (float(v) for v in run.row_margin)
            table = lambda c: tuple(xp.asarray(v, xp.f64) for v in inflated_row_bounds(c.problem, B, a + g * np.arange(c.N + 1)))
            self._sv.set_instance_row_bounds(*table(ctrl))
            self.row_bounds = table(backup)

    def attach_loop(self, counter, plant):
        """what needs the loop's own state: the clock cells of a track and the controller models.  ``counter``: the step counter of a
        device loop, which IS the controller handle's scene clock (smpc_loop_post reads column j + 1, then advances it); its backup
        handle solves on its own stream while the loop goes on, so that clock is a cell of its own, which receives the counter's value
        at the abort event.  None on the host: one cell per handle, written before the calls of a step.  ``plant``: the tables the plant
        steps with, which models='plant' hands to the controller -- on the device the very tensor.  A device loop with a forecast
        sets the world (and what was observed of it) once: the engine's forecast at the head of every step reads it."""
        xp, sv, bsv, dev, table = self._xp, self._sv, self._bsv, self._xp.on_device, self._run.models
        if table is not None:
            for s in (sv, bsv):
                _require(s, 'models', 'set_instance_models')
            self.models = plant if isinstance(table, str) else _joint_tensor(xp, table, self._B, self._ctrl.nq) if dev else table
            if dev:                             # (the two loops hand the models over on either side of the clocks)
                _set_models(sv, self.models)
        if self.track:
            self.clock, self.backup_clock = (counter, xp.step_index(0)) if dev else (_new_scene_clock(sv), _new_scene_clock(bsv))
            sv.set_scene_clock(self.clock)
            bsv.set_scene_clock(self.backup_clock)
        if table is not None and not dev:
            _set_models(sv, self.models)
        if dev and self.forecast is not None:
            for s in (sv, bsv):
                self.forecast.require(s, self.observed is not None and not (s is bsv and self.forecast.is_kalman), self.margin_kalman is not None)
            self._select, self._backup_select = _context_select(sv), _context_select(bsv)
            sv.set_instance_world_track(self.scenes)
            if self.observed is not None:       # (what HOLD, CV and the fit then read instead of the world)
                sv.set_instance_observed_track(self.observed)

    def _forecast_into(self, sv, select, rows, t, N):
        """one forecast into ``sv``'s scene slot: on the device from its world (and observed track) at its clock cell; on the host the
        statement at time ``t`` for the instances ``rows`` (with their context rows, _set_scene) and no clock -- node k reads column k.
        A filter advances on the controller's handle and is only read on the backup's, from the rows of the event"""
        advance = sv is self._sv
        state = self.kalman_state if advance else self._backup_state
        if self._xp.on_device:
            return self.forecast.enqueue(sv, select, state, advance) if self.forecast.is_kalman else self.forecast.enqueue(sv, select)
        sv.set_scene_clock(None)
        if self.forecast.is_kalman:
            return _set_scene(sv, self.forecast.statement(self.scenes, self.observed, rows, t, N, state, advance))
        _set_scene(sv, self.forecast.statement(self.scenes, self.observed, rows, t, N))

    def _kalman_margin_into(self, sv, prob):
        """the row-bounds table of ``sv`` from the covariance of the filter it has just forecast with: on the device one enqueued call;
        on the host the statement over ``prob``'s horizon, then the setter"""
        z, base, cap = self.margin_kalman
        state = self.kalman_state if sv is self._sv else self._backup_state
        if self._xp.on_device:
            return self.forecast.enqueue_margin(sv, state, z, base, cap)
        from .problem import inflated_row_bounds
        d = self.forecast.margin_statement(prob, state, z, base, cap)
        sv.set_instance_row_bounds(*inflated_row_bounds(prob, d.shape[0], d))

    def pick_backup_rows(self, rows):
        """the filter's records of the aborting instances ``rows`` as they are now -- gathered where the state is written (a device
        loop: on the loop's stream, before the event that the backup's stream waits for, because the next step's advance overwrites
        the state in place); kept until the next event, when the previous one's solve has been waited for"""
        if self.kalman_state is not None:
            self._backup_state = self.kalman_state[rows]

    def _margin_into(self, sv, prob, rows, t):
        """the row-bounds table of ``sv`` from the residuals of the fit it has just forecast with: on the device one enqueued call at
        its clock cell; on the host the statement at time ``t`` for the instances ``rows`` over ``prob``'s horizon, then the setter"""
        z, prior, base, cap = self.margin_fit
        fc = self.forecast
        if self._xp.on_device:
            return sv.forecast_row_margin(fc.window, fc.degree, z, prior, base, cap)
        from .problem import fit_margin_statement, inflated_row_bounds
        seen = self.scenes if self.observed is None else self.observed
        d = fit_margin_statement(prob, seen[rows], t, fc.window, fc.degree, z, prior, base, cap)
        sv.set_instance_row_bounds(*inflated_row_bounds(prob, d.shape[0], d))

    def head_of_step(self, t=None):
        """what the controller plans in at the step that begins (``t``: the step, on the host): the scenes forecast at time t, read from
        node 0 on; without a forecast node k of the step's solve and tests is formed at time t + k, by the clock"""
        if self.forecast is not None:
            self._forecast_into(self._sv, self._select, slice(None), t, self._ctrl.N)
            if self.margin_fit is not None:
                self._margin_into(self._sv, self._ctrl.problem, slice(None), t)
            if self.margin_kalman is not None:
                self._kalman_margin_into(self._sv, self._ctrl.problem)
        elif not self._xp.on_device:
            _write_scene_clock(self.clock, t)

    def dress_backup(self, rows, t=None):
        """the backup OCP of an abort event is solved in the scenes of the aborting instances ``rows`` (in the compact batch's order) --
        with a forecast, in what the controller knows of their world at the event --, with their row bounds and with their models"""
        sv = self._bsv
        if self.scenes is not None and self.forecast is None:
            _set_scene(sv, self.scenes[rows])
        elif self.scenes is not None:
            if self.forecast.is_kalman:         # (forecast from the event's records: no table is read, so no world goes on)
                if not self._xp.on_device:
                    self.pick_backup_rows(rows)
            elif self._xp.on_device:            # (the forecast reads them at the handle's own clock cell)
                sv.set_instance_world_track(self.scenes[rows])
                if self.observed is not None:
                    sv.set_instance_observed_track(self.observed[rows])
            self._forecast_into(sv, self._backup_select, rows, t, self._backup.N)
            if self.margin_fit is not None:
                self._margin_into(sv, self._backup.problem, rows, t)
            if self.margin_kalman is not None:
                self._kalman_margin_into(sv, self._backup.problem)
        if self.row_bounds is not None:
            sv.set_instance_row_bounds(self.row_bounds[0][rows], self.row_bounds[1][rows])
        if self.models is not None:
            _set_models(sv, self.models[rows])

    def to_true_world(self):
        """the plant lives, and the run is scored, in the TRUE world: with a forecast the track replaces the last forecast in the scene
        slot of the controller's handle (with its context track where the net has one), read by the loop's clock again"""
        if self.forecast is not None:
            _set_scene(self._sv, self.scenes)
            self._sv.set_scene_clock(self.clock)

    def detach(self):
        """both handles keep nothing behind the run, every call of which has been enqueued by now: no scene, context or clock, no world
        nor what was observed of it, no row-bounds or model table, no curves (the controller hands those over again should it step)"""
        sv, bsv = self._sv, self._bsv
        if self.scenes is not None:
            _clear_scene(sv)
            _clear_scene(bsv)
            if self.forecast is not None:
                for s in (sv, bsv):
                    if self.observed is not None and hasattr(s, 'set_instance_observed_track'):
                        s.set_instance_observed_track(None)
                    if hasattr(s, 'set_instance_world_track'):
                        s.set_instance_world_track(None)
        if self.row_bounds is not None or self.margin_fit is not None or self.margin_kalman is not None:
            sv.set_instance_row_bounds(None)
            bsv.set_instance_row_bounds(None)
        if self.models is not None:
            _set_models(sv, None)
            _set_models(bsv, None)
        traj = getattr(self._ctrl, 'traj', None)
        if traj is not None and traj.ndim == 3 and hasattr(sv, 'set_instance_curves'):
            sv.set_instance_curves(None)


class _Group:
    """The closed loop of ONE group of instances (global indices first .. first + B): the driver's safe-abort automaton around
    the controller's ``step``.  A step has two halves, ``part_a`` (PD abort tracking, controller step) and ``part_b`` (plant,
    outcome tests, logs), with the step's single host decision between them (``did any instance raise abort?``,
    ``handle_aborts``).  This base holds what the two loops share -- arguments, noise tables, logs and flags (numpy arrays or
    device tensors, by the controller's backend), the generator around the loop and the results; :class:`_HostGroup` is the
    numpy statement of the loop, :class:`_DeviceGroup` the same loop as engine calls."""

    def __init__(self, params, x_guess, u_guess, noise, control_noise, ctrl, backup, n_steps, first, callback, collect_times=False,
                 scenes=None, models=None, forecast=None, forecast_window=None, observed=None, forecast_degree=1, row_margin=None,
                 world=None):
        self._params, self._ctrl, self._backup, self._n_steps, self._first, self._callback = params, ctrl, backup, n_steps, first, callback
        B = x_guess.shape[0]
        xp = ctrl.xp
        self._xp, self._B = xp, B
        if world is None:           # (run_mpc hands over the group's _RunWorld; a caller of this class the single arguments)
            world = _RunWorld(scenes, models, None if forecast is None else _Forecast(forecast, forecast_window, forecast_degree), observed,
                              row_margin)
        self._world = _World(world, ctrl, backup, B)
        self._world.attach()
        # stats.append(controller.getTime()) of scripts/mpc.py:239: one row of the seven time_fields per step of this group's
        # controller (host: read when step() returns; device: _DeviceGroup._read_times)
        self._collect_times = bool(collect_times) and hasattr(ctrl.ocp_solver, 'timing_history')
        self._time_rows, self._time_lost = [], 0
        if self._collect_times:
            ctrl.ocp_solver.enable_timing(2)
        pr, nq, nx, nu = ctrl.problem, ctrl.nq, ctrl.nx, ctrl.nu
        self._Nb = backup.N
        seeds = np.arange(first, first + B)
        self._joints_noisy = perturbed_joint_tables(params, nq, noise, seeds) if noise > 0 else None          # mpc.py:106-107
        # model.reset_seed(i) is called at EVERY step (mpc.py:126): each instance sees the same torque-noise draw each step
        self._tau_noise = None
        if control_noise > 0:
            self._tau_noise = np.stack([np.random.default_rng(int(i)).normal(np.zeros(nu), pr.tau_max * control_noise / 100, nu)
                                        for i in seeds])
        # step-major logs (one contiguous [B, .] slab per step); transposed to the reference's [B, step, .] at the end
        nan = float('nan')
        self.x_log = xp.full((n_steps + 1, B, nx), nan)
        self.u_log = xp.full((n_steps, B, nu), nan)
        self.r_log = xp.full((n_steps, B), -1, xp.i64)
        self.x_cur = xp.asarray(x_guess[:, 0], xp.f64)
        self.x_log[0] = self.x_cur
        ctrl.setGuess(x_guess, u_guess)                                                  # mpc.py:119-120
        ctrl.reset_controller()
        self.alive = xp.full((B,), True, xp.bool_)
        self.sa = xp.full((B,), False, xp.bool_)
        self.ja = xp.zeros((B,), xp.i64)
        self.x_abort = xp.zeros((B, self._Nb + 1, nx))
        self.u_abort = xp.zeros((B, self._Nb, nu))
        self.collided = xp.full((B,), False, xp.bool_)
        self.viable = xp.zeros((B,), xp.u8)            # successful abort events so far (mpc.py:189 appends once per event)
        self._quirks = bool(getattr(params, 'reference_quirks', True))
        self.u = xp.zeros((B, nu))
        # last valid row of the state / input logs of every instance (mpc.py:114 pre-fills with NaN, :240-264 and :186-190 break)
        self.last_x, self.last_u = xp.full((B,), n_steps, xp.i64), xp.full((B,), n_steps - 1, xp.i64)
        self._abort_events = []

    def _progress(self, j):
        xp = self._xp
        if self._callback and j % 50 == 0:
            print(f'step {j} (instances {self._first}..{self._first + self._B - 1}): alive {int(xp.host(self.alive).sum())}/{self._B}, '
                  f'in abort {int(xp.host(self.sa & self.alive).sum())}, failures {int(xp.host(self.collided).sum())}')

    def run(self):
        """generator: yields once per step, after the first half has run / is enqueued (run_mpc serves the other groups meanwhile)"""
        try:
            yield from self._run()
        finally:
            # whatever path ran (device loop, host state on the HIP engine, an exception in between): the handle stops recording
            # events when the run is over
            sv = self._ctrl.ocp_solver
            if self._collect_times and hasattr(sv, 'enable_timing'):
                try:
                    sv.enable_timing(0)
                except Exception:
                    pass

    def results(self, score=False):
        xp, ctrl, params, B, n_steps = self._xp, self._ctrl, self._params, self._B, self._n_steps
        solver, pr = ctrl.ocp_solver, ctrl.problem
        scored, world = None, self._world
        world.to_true_world()
        if score:
            # the run's scores: on the device from the logs where they are (one enqueue on the group's stream, ahead of the wait
            # below), on the host by the statement; the safe-set score where the formulation has a safe-set row
            want_safe = int(pr.desc.nn_mode) != 0 and getattr(ctrl, 'net', None) is not None
            traj = getattr(ctrl, 'traj', None)
            if xp.on_device:
                scored = solver.score_rollout(self.x_log, self.u_log, self.last_x, self.last_u, traj=traj, want_safe=want_safe)
            else:
                scored = score_rollout_statement(solver, pr, params, self.x_log, self.u_log, self.last_x, self.last_u,
                                                 traj=None if traj is None else xp.host(traj), want_safe=want_safe,
                                                 per_instance=world.scenes is not None,
                                                 scene_clock=world.clock if world.track else None)
        if xp.on_device:
            solver.sync()
        # convergence at the last step (mpc.py:273): the reference tests x_sim[-1], NaN for instances that broke
        x_sim = np.ascontiguousarray(np.transpose(xp.host(self.x_log), (1, 0, 2)))
        u_sim = np.ascontiguousarray(np.transpose(xp.host(self.u_log), (1, 0, 2)))
        steps = np.arange(n_steps + 1)[None, :]
        x_sim[steps > xp.host(self.last_x)[:, None]] = np.nan
        u_sim[steps[:, :n_steps] > xp.host(self.last_u)[:, None]] = np.nan
        x_last = np.nan_to_num(x_sim[:, -1])
        ev = solver.eval_nodes(xp.repeat_nodes(xp.asarray(x_last, xp.f64), ctrl.N + 1), xp.zeros((B, ctrl.N, ctrl.nu)), ctrl.p)
        ee = xp.host(ev['ee'])[:, 0, :]
        conv = ~np.isnan(x_sim[:, -1]).any(1) & (np.linalg.norm(ee - pr.ee_ref, axis=1) < params.tol_conv)
        if not self._quirks:
            conv &= xp.host(self.alive)        # (the reference tests x_sim[-1] even of an instance it has just recorded as failed)
        extra = {'score': _score_dict(xp.host(scored[0]), xp.host(scored[1]))} if score else {}
        if world.scenes is not None:
            extra['scenes'] = xp.host(world.scenes)
        world.detach()
        return dict(**extra, x=x_sim, u=u_sim, r_receding=np.transpose(xp.host(self.r_log), (1, 0))[:, :, None], conv=conv,
                    time_rows=np.array(self._time_rows, float).reshape(-1, len(TIME_FIELDS)), time_lost=self._time_lost,
                    collided=xp.host(self.collided), viable=xp.host(self.viable).astype(np.int64),
                    abort_events=[(e[0], e[1], xp.host(e[2])) for e in self._abort_events])


class _HostGroup(_Group):
    """The loop on host state, in numpy: the readable statement of scripts/mpc.py:118-287 for B instances at once, what
    ``run_mpc(on_device=False)`` runs (CPU double, or the engine's host path) and what the GPU tests hold :class:`_DeviceGroup`
    against."""

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        B = self._B
        self.resumed = np.zeros(B, bool)          # left the backup trajectory at this step (mpc.py:137-141)
        self.new_abort = np.zeros(B, bool)
        self._zeros_u = np.zeros((B, self._ctrl.nu))
        self._jt = 0                              # the step counter
        self._ever_aborted = False
        self._world.attach_loop(None, self._joints_noisy)

    # ---- first half: everything up to the controller's verdict ---------------------------------------------------------------
    def part_a(self):
        ctrl, B, Nb = self._ctrl, self._B, self._Nb
        nq = ctrl.nq
        kp, kd = 1.0, 1e2                                                               # mpc.py:97
        x_cur = self.x_cur
        if self._ever_aborted:
            # --- instances following their safe-abort trajectory (mpc.py:130-146)
            in_abort = self.sa & self.alive
            follow = in_abort & (self.ja < Nb)
            idx = np.minimum(self.ja, Nb - 1)
            xa = self.x_abort[np.arange(B), idx]
            ua = self.u_abort[np.arange(B), idx]
            u_f = ua - (kp * (x_cur[:, :nq] - xa[:, :nq]) + kd * (x_cur[:, nq:] - xa[:, nq:]))
            u = np.where(follow[:, None], u_f, self._zeros_u)
            hold = in_abort & (self.ja >= Nb)
            resume = hold & np.all(x_cur[:, nq:] < 5e-3, axis=1)                      # mpc.py:138
            still = hold & ~resume
            xe = self.x_abort[:, -1]
            u_h = -(kp * (x_cur[:, :nq] - xe[:, :nq]) + 3e2 * (x_cur[:, nq:] - xe[:, nq:]))
            u = np.where(still[:, None], u_h, u)
            self.sa = self.sa & ~resume
            self.ja = self.ja + in_abort.astype(np.int64)
            self.resumed = resume
        else:
            u = self._zeros_u
        # --- instances under MPC (mpc.py:151)
        stepping = self.alive & ~self.sa
        if hasattr(ctrl, 'r'):
            self.r_log[self._jt] = np.where(stepping, ctrl.r, -1)
        self._world.head_of_step(self._jt)
        # (until the first abort event every live instance steps: no snapshot / roll-back needed; dead instances are never
        #  read again, so they may step along)
        if self._ever_aborted:
            u_m, ab = _masked_step(ctrl, x_cur, stepping)
        else:
            u_m, ab = ctrl.step(x_cur)
        self.u = np.where(stepping[:, None], u_m, u)
        self.new_abort = ab & stepping
        if self._ever_aborted and self._quirks:
            # An abort raised on the very step an instance resumed MPC sits inside the reference's `if sa_flag:` branch
            # (mpc.py:137-141): no viable state is recorded and no backup OCP solved -- the instance is in safe abort again
            # with its OLD backup trajectory, its abort clock keeps running, and it re-tests its velocity at the next step.
            again = self.new_abort & self.resumed
            self.sa = self.sa | again
            self.new_abort = self.new_abort & ~again

    # ---- the step's decision: abort events (mpc.py:161-190) ----------------------------------------------------------------------
    def handle_aborts(self):
        ctrl, backup, B, Nb = self._ctrl, self._backup, self._B, self._Nb
        if not ctrl.can_abort or not self.new_abort.any():
            return
        self._ever_aborted = True
        # the backup OCP is solved for the aborting instances only (a compact batch), from their viable states
        rows = np.where(self.new_abort)[0]
        j, n_c = self._jt, len(rows)
        xv_c = ctrl.getLastViableState()[rows]
        xg_c = np.repeat(xv_c[:, None, :], Nb + 1, axis=1)
        self._world.dress_backup(rows, j)
        _write_scene_clock(self._world.backup_clock, j)
        xo_c, uo_c, st_c, _ = backup.ocp_solver.solve(np.ascontiguousarray(xv_c), xg_c, np.zeros((n_c, Nb, ctrl.nu)), backup.p[:n_c])
        self._abort_events.append((rows + self._first, np.full(n_c, j), xv_c))
        ok_c = np.asarray(st_c) == 0
        failed, okb = np.zeros(B, bool), np.zeros(B, bool)
        failed[rows] = ~ok_c
        okb[rows] = ok_c
        xa_new, ua_new = np.copy(self.x_abort), np.copy(self.u_abort)
        xa_new[rows] = np.asarray(xo_c)
        ua_new[rows] = np.asarray(uo_c)
        self.collided = self.collided | failed
        self.alive = self.alive & ~failed
        self.last_x, self.last_u = np.where(failed, j, self.last_x), np.where(failed, j, self.last_u)   # mpc.py:186-190
        self.x_abort = np.where(okb[:, None, None], xa_new, self.x_abort)
        self.u_abort = np.where(okb[:, None, None], ua_new, self.u_abort)
        self.ja = self.ja * (~okb).astype(np.int64)
        self.sa = self.sa | okb
        self.viable = np.minimum(self.viable.astype(np.int64) + okb.astype(np.int64), 255).astype(np.uint8)   # saturating, like k_loop_apply_backup

    # ---- second half: plant, outcome tests, logs ----------------------------------------------------------------------------------
    def part_b(self):
        solver, j = self._ctrl.ocp_solver, self._jt
        # plant (mpc.py:240, env_model.py:192-206).  Logs are written unmasked; rows of an instance after its failure are
        # blanked at the end from the step it died at (mpc.py:114 pre-fills them with NaN)
        self.u_log[j] = self.u
        x_next, _ = solver.plant_step(self.x_cur, self.u, self._joints_noisy, self._tau_noise)
        # outcome tests on the new state (mpc.py:246-264): one node per instance, so the engine's box + collision test
        # (model bounds widened by tol_x, rows against the check bounds) is exactly checkStateConstraints; the new state is
        # the state of time j + 1, which is where a scene track is read -- with a forecast the WORLD's track, not the controller's
        self._world.to_true_world()
        _write_scene_clock(self._world.clock, j + 1)
        okn = np.asarray(solver.check_trajectory(x_next[:, None, :]))
        self.x_log[j + 1] = x_next
        bad = self.alive & ~okn
        self.last_x, self.last_u = np.where(bad, j + 1, self.last_x), np.where(bad, j, self.last_u)   # the failing state stays logged
        self.collided = self.collided | bad
        self.alive = self.alive & ~bad
        self.x_cur = np.where(self.alive[:, None], x_next, self.x_cur)
        self._jt += 1

    def _run(self):
        for j in range(self._n_steps):
            self.part_a()
            if self._collect_times:
                self._time_rows.append(self._ctrl.getTime())       # the solve has finished when step() returns
            yield j
            self.handle_aborts()
            self.part_b()
            self._progress(j)
            if not self.alive.any():
                break


class _DeviceGroup(_Group):
    """The loop with all state in HBM: both halves of a step are engine kernels (smpc_loop_pre / smpc_policy_step /
    smpc_loop_classify_aborts, then smpc_loop_post) on state tensors that keep their addresses for the whole run -- nothing here
    rebinds one -- so after a few eager steps each half is captured once as a hipGraph and replayed: one graph launch instead of
    ~50 kernel launches per half.  :class:`_HostGroup` is the readable statement of the same automaton."""

    def __init__(self, *args, use_graphs=True, **kw):
        super().__init__(*args, **kw)
        import torch
        xp, ctrl, B, nu = self._xp, self._ctrl, self._B, self._ctrl.nu
        if self._joints_noisy is not None:
            self._joints_noisy = _joint_tensor(xp, self._joints_noisy, B, ctrl.nq)
        if self._tau_noise is not None:
            self._tau_noise = xp.asarray(self._tau_noise, xp.f64)
        self._jt = xp.step_index(0)               # the step counter, a device tensor: smpc_loop_post advances it, graphs replay it
        self._world.attach_loop(self._jt, self._joints_noisy)
        self._use_graphs = bool(use_graphs)
        self._graphs = {}                         # half -> captured graph
        self._u_other = xp.zeros((B, nu))
        self._stepping = xp.full((B,), True, xp.bool_)
        self.new_abort = ctrl._abort_out          # (the controller's own output buffer: no copy per step)
        # abort events: the backup OCPs of a step's events are solved on the backup solver's own stream WHILE the next
        # step's solve runs; until their outcome is applied (smpc_loop_apply_backup) the instances are only kept from stepping
        self._pending = xp.full((B,), False, xp.bool_)
        self._resumed = xp.full((B,), False, xp.bool_)      # written by smpc_loop_pre
        self._any_event = xp.zeros((1,), xp.i32)            # written by smpc_loop_classify_aborts
        self._inflight = None
        bs = self._backup.ocp_solver
        self._side = torch.cuda.ExternalStream(bs.L.smpc_stream(bs.h), device=torch.device('cuda', bs.device))
        # the engine keeps HIP events of its last 64 solves (smpc_get_timing_history); they are read at least 32 solves late --
        # finished by then, so nothing waits inside the loop
        self._time_next = 0

    def part_a(self):
        ctrl, sv = self._ctrl, self._ctrl.ocp_solver
        self._world.head_of_step()
        sv.loop_pre(self, getattr(ctrl, 'r', None), self._pending, self._u_other, self._stepping)
        ctrl.step_on_device(self.x_cur, self._stepping, self._u_other, u_out=self.u)
        if ctrl.can_abort:
            sv.loop_classify_aborts(self, self.new_abort, self._any_event)

    def _apply_inflight(self):
        if self._inflight is None:
            return
        import torch
        rows_b, xv_c, xo_c, uo_c, st_c, ev = self._inflight
        torch.cuda.current_stream().wait_event(ev)
        self._ctrl.ocp_solver.loop_apply_backup(self, rows_b, st_c, xo_c, uo_c, self.viable, self.u, self._pending)
        self._inflight = None

    def handle_aborts(self, j):
        """Same events and outcomes as :meth:`_HostGroup.handle_aborts`; what differs is WHEN the backup OCP's result is
        consumed: the solve is enqueued on the backup solver's stream and its outcome applied one step later, after the next
        controller step has been enqueued -- in between the instance only must not step (``_pending``), which is all the
        reference's loop needs of it (it either follows the backup trajectory from the next step on or is lost at this one)."""
        import torch
        xp, ctrl, backup, Nb = self._xp, self._ctrl, self._backup, self._Nb
        if not ctrl.can_abort:
            return
        self._apply_inflight()                               # the previous step's events (their first tracking control goes into u)
        if not bool(self._any_event.item()):                 # (the step's one host synchronisation)
            return
        rows = np.where(xp.host(self.new_abort))[0]
        rows_b = xp.asarray(rows, xp.i64)
        xv_c = ctrl.x_viable[rows_b]
        n_c = len(rows)
        self._abort_events.append((rows + self._first, np.full(n_c, j), xv_c))      # (xv_c goes to the host in results())
        self._pending.copy_(self.new_abort)
        if self._world.backup_clock is not None:
            self._world.backup_clock.copy_(self._jt)         # (the previous event's solve has finished: _apply_inflight above)
        self._world.pick_backup_rows(rows_b)                 # (a filter's records of the event: before ev0, like xv_c)
        main = torch.cuda.current_stream()
        ev0 = torch.cuda.Event()
        ev0.record(main)
        with torch.cuda.stream(self._side):
            self._side.wait_event(ev0)
            xg_c = xp.repeat_nodes(xv_c, Nb + 1)
            self._world.dress_backup(rows_b)
            xo_c, uo_c, st_c, _ = backup.ocp_solver.solve(xv_c, xg_c, xp.zeros((n_c, Nb, ctrl.nu)), backup.p[:n_c])
            ev = torch.cuda.Event()
            ev.record(self._side)
        # (These tensors cross streams.  Their lifetimes are ordered by the events, not by the caching allocator: they are released
        #  in _apply_inflight, after the main stream has been told to wait for `ev`, and the side stream's next work waits for an
        #  event recorded on the main stream after that.  torch's record_stream is not usable here -- on this ROCm build it
        #  faults on an ExternalStream.)
        self._inflight = (rows_b, xv_c, xo_c, uo_c, st_c, ev)

    def part_b(self):
        self._ctrl.ocp_solver.loop_post(self, self.u, self._joints_noisy, self._tau_noise)

    def _run_half(self, half, fn, j):
        """eager for the first steps (workspaces get allocated), then captured once and replayed"""
        if getattr(self._ctrl, '_traj_rebound', False):      # setTrajectory bound a new device tensor: captured steps hold the old one
            self._graphs.clear()
            self._ctrl._traj_rebound = False
        g = self._graphs.get(half)
        if g is None and self._use_graphs and j >= 3:
            import torch
            try:
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=torch.cuda.current_stream(), capture_error_mode='relaxed'):
                    fn()                  # (capturing records the launches without executing them)
                self._graphs[half] = g
            except Exception as e:        # report once, stay eager
                print(f'[run_mpc] hipGraph capture of step half {half} failed ({type(e).__name__}: {e}); eager launches')
                self._use_graphs, g = False, None
        if g is not None:
            g.replay()
        else:
            fn()

    def _read_times(self, j, final=False):
        """rows of the solves up to step j whose events have finished (never the 32 most recent unless ``final``)"""
        sv = self._ctrl.ocp_solver
        if final:
            sv.sync()                              # end of the run: everything has finished, drain the ring
        while self._time_next <= j:
            back = j - self._time_next
            if back >= 64:                         # the ring has lapped it (the host ran more than 64 solves ahead of this read)
                self._time_lost += 1
                self._time_next += 1
                continue
            if not final and back < 32:
                break
            if not final and back >= 56:
                sv.sync()                          # about to be lapped: wait rather than lose the row
            tm = sv.timing_history(back)
            if tm is None:
                if final:
                    self._time_lost += 1
                    self._time_next += 1
                    continue
                break
            self._time_rows.append(time_row(tm))
            self._time_next += 1

    def _run(self):
        for j in range(self._n_steps):
            self._run_half('a', self.part_a, j)
            if self._collect_times:
                self._read_times(j)
            yield j
            self.handle_aborts(j)
            self._run_half('b', self.part_b, j)
            self._progress(j)
        self._apply_inflight()                # (events of the last step)
        if self._collect_times:
            self._read_times(self._n_steps - 1, final=True)


TIME_FIELDS = ('time_lin', 'time_sim', 'time_qp', 'time_qp_solver_call', 'time_glob', 'time_reg', 'time_tot')   # controller.py:123-124


def time_row(t):
    """the engine's per-kernel times of one solve (seconds) as the reference's seven acados fields (controller.py:192-193):
    time_lin = linearisation + network pass (acados evaluates the l4casadi row inside its linearisation), time_qp = stage-QP
    set-up + interior point, time_qp_solver_call = the interior point alone; nothing of the kind of time_sim / time_glob /
    time_reg runs here (closed-form dynamics, FIXED_STEP, LM folded into the set-up)"""
    qp_setup, qp_ipm = t.get('time_qp_setup', 0.0), t.get('time_qp_ipm', 0.0)
    qp = t['time_qp'] if 'time_qp' in t else qp_setup + qp_ipm
    return [t.get('time_lin', 0.0) + t.get('time_nn', 0.0), 0.0, qp, qp_ipm, 0.0, 0.0, t.get('time_tot', 0.0)]


def _check_state_kind(ctrl, backup, on_device):
    """run_mpc's two loops take the state where they expect it: ValueError, before anything is enqueued, otherwise"""
    for c in (ctrl, backup):
        if bool(c.xp.on_device) != bool(on_device):
            raise ValueError(f'run_mpc(on_device={bool(on_device)}): {type(c).__name__} was built with device_state={bool(c.xp.on_device)}; '
                             'make_controller / make_backup must hand back controllers with device_state=on_device')
    if on_device and not hasattr(ctrl.ocp_solver, 'loop_pre'):
        raise ValueError(f'run_mpc(on_device=True) needs a solver with the engine\'s loop kernels (BatchedOcpSolver.loop_pre); '
                         f'{type(ctrl.ocp_solver).__name__} has none')


def run_mpc(params, cont_name, x_guess, u_guess, noise=0.0, control_noise=0.0, make_controller=None, make_backup=None,
            n_steps=None, callback=False, on_device=False, device=0, timing=None, groups=None, graphs=True, collect_times=False,
            score=False, scenes=None, traj=None, models=None, forecast=None, forecast_window=8, observed=None,
            forecast_degree=None, row_margin=None, row_margin_fit=None, kalman=None, row_margin_kalman=None):
    """scripts/mpc.py:102-317 for all instances at once.  Returns the result dict the reference pickles (mpc.py:307-315).

    ``on_device=True``: the whole loop state -- the policy automaton of the controller, the safe-abort automaton of the driver
    (flags, abort clocks, backup trajectories, PD tracking), trajectories and outcome masks -- lives in HBM as torch tensors
    and every engine call takes the device-pointer path.  The only host synchronisation inside a step is one scalar per
    group for the policies that can abort: "did any instance raise abort in this step?" (the backup OCP is solved only then,
    as in the reference, mpc.py:161-190, and only for the aborting instances).  The instances are split into ``groups``
    independent sub-batches (default 2 on the device), each with its own engine handle and HIP stream, advanced in turn:
    while the host waits for one group's flag the others' kernels keep the GPU busy, and the long tail of one group's QP
    launch overlaps the bulk of another's.  With ``graphs`` each half of a step (before / after that flag) is captured as a
    hipGraph after a few eager steps and replayed.  ``timing``: optional dict that receives wall-clock ms per step.
    ``collect_times``: append the controller's solver times at every step like ``stats.append(controller.getTime())`` of
    scripts/mpc.py:239; the result then carries ``'time_stats'`` (one row of ``TIME_FIELDS`` per step and group, seconds) and
    ``'time_q99'`` (the 99 % quantiles mpc.py:300-303 prints).  A captured graph cannot record into the engine's event ring,
    so this runs the steps as eager launches.
    ``score``: the result gains ``'score'``, a dict of [B] arrays keyed by ``solver.SCORE_SLOTS`` / ``SCORE_INDEX_SLOTS`` -- closed-loop
    cost, EE distance of the last state, worst collision / state-box margins, least safe-set value and where each was taken
    (:func:`score_rollout_statement`).  On the device every group scores its logs where they are (smpc_score_rollout); nothing else
    in the result changes.
    ``scenes`` ([B, n_rows, 8], ``OcpProblem.scene`` / ``jittered_scenes``): a scene of its own for every instance -- where the fixed
    obstacles of its collision rows sit (solver.set_instance_scene; bounds, radii and kinds stay the problem's).  The controller's
    solves and tests, the plant's outcome test, the scores and the backup OCP of an abort event all run in the instance's scene;
    the result gains ``'scenes'``, and the controller's and the backup solver's handles are left without a scene when the run ends.
    Not with the parallel policy (ValueError): its solver works on B x N candidate slots, which are not instances.
    ``scenes`` [B, T, n_rows, 8] (``OcpProblem.scene_track`` / ``moving_scenes``): obstacles that MOVE, a scene per instance and
    time column (solver.set_instance_scene_track).  The loop's step counter j is the scene clock of both handles: node k of
    step j's solve and tests is formed in column min(j + k, T - 1), the plant's new state is tested in column min(j + 1, T - 1),
    state j of the log is scored there, and the backup OCP of an abort event at step j is solved at clock j in the aborting
    instances' tracks.  Both handles are left without a track and without a clock when the run ends.  A safe-set network with a
    context (``ctx_select``) follows the track: both handles get the context of every (instance, column)
    (solver.set_instance_context_track), the network row of node k reads the column its collision rows read, and the handles are
    left without it.  The meaning is quasi-static: a network trained on standing scenes, asked at node k
    about the scene as it will stand at time j + k.
    ``forecast`` ('hold', 'cv', 'true'; needs a track): the track is the WORLD, which only the plant meets, and the controller plans
    against a forecast of it (``problem.forecast_statement``): at the head of step j the scene slot gets the
    horizon's N + 1 scenes as forecast from the world's columns up to j -- 'hold' the frozen world, 'cv' constant velocity from
    the last two columns, 'true' the world itself (the clairvoyant controller that ``forecast=None`` is) -- and, for a net with a
    context, their context rows; the plant's new state is tested in column j + 1 of the world.  On the device that is one
    smpc_forecast_scene per step inside the captured half and smpc_loop_post reading the world; on the host the statement.  The
    backup OCP of an abort event gets the aborting instances' world rows and one forecast over its own horizon at the event's
    clock.  The run is scored in the true world, both handles end without world, forecast, context and clock, and the result
    gains ``'forecast'``.  None: the calls of a run without the argument, one for one.
    ``forecast='fit'`` with ``forecast_window`` (1..``problem.FIT_MAX``, default 8): the forecast is a
    least-squares line through the last ``forecast_window`` columns seen (``problem.fit_forecast_statement``; window 1 is 'hold',
    window 2 'cv') -- on the device one smpc_forecast_scene_fit per step where 'hold' and 'cv' enqueue smpc_forecast_scene.
    ``forecast_degree`` (0, 1 or 2, only with ``forecast='fit'``; None: 1): the fit is a least-squares
    polynomial of that degree (``problem.poly_forecast_statement``) -- 0 the window mean, 2 a constant-acceleration model.  Degree 1
    makes exactly the calls of a run without the argument; degrees 0 and 2 apply the statement on the host path and enqueue one
    smpc_forecast_scene_poly per step on the device, the backup handle of an abort event included.  ValueError with any other
    ``forecast`` or outside 0..2.  The result gains ``'forecast_degree'`` only when the degree is not 1.
    ``observed`` ([B, T, n_rows, 8], the world's shape; ``problem.observe_tracks`` draws one): what the controller observes of the
    world.  'hold', 'cv' and 'fit' are then formed from it instead of the world (smpc_set_instance_observed_track on the device,
    the statement on it on the host), the plant still meets the world, and the backup handle of an abort event gets the aborting
    instances' observed rows with their world rows.  ValueError with ``forecast`` None or 'true', which do not read it.  The
    result gains ``'forecast_window'`` (with 'fit') and ``'observed'`` (bool, with any forecast); both handles end without an
    observed track.  Without ``observed``, None, 'hold', 'cv' and 'true' make the calls of before, one for one.
    ``traj`` ([3, L], tracking.tracking_trajectory): every group's controller follows this curve (``setTrajectory``), the tracking
    task of the reference's Tracking8* / TrackingMovingCircle* costs.  ``traj`` [B, 3, L] (tracking.tracking_curves /
    jittered_curves): a curve of its own for every instance -- every group's controller gets its slice (on the device its handle
    holds the curves, solver.set_instance_curves), the score uses each instance's own curve, the backup OCP has zero cost and needs
    none, and the handles are left without curves when the run ends.
    ``models``: the link inertials the CONTROLLER forms its dynamics with, per instance (solver.set_instance_models; kinematics and
    limits stay the problem's).  ``'plant'``: every group's controller gets the very tables the loop draws for its plant
    (``perturbed_joint_tables`` with the instances' seeds; on the device the same tensor) -- the matched-model arm of the model-noise
    study, which needs ``noise > 0`` --; a ``JOINT_DTYPE`` table [B, nq]: each group gets its rows.  The backup OCP of an abort
    event is solved with the aborting instances' models, and both handles are left without a table when the run ends.  Not with the
    parallel policy (ValueError), and the plant keeps stepping with its own tables whatever the controller is given.
    ``row_margin`` ``(a, b)``: obstacle inflation along the horizon -- node k of every solve leaves
    ``d_k = a + b k`` metres of extra room around the world-fixed obstacles (``problem.inflated_row_bounds``,
    solver.set_instance_row_bounds), set once per group on the controller's handle before the loop, and on the backup handle, over its
    own horizon, for the aborting instances of an abort event.  The outcome tests and the scores keep the physical check bounds.  With
    or without ``scenes`` and ``forecast``; both handles are left without a table when the run ends and the result gains
    ``'row_margin'``.  Not with the parallel policy (ValueError).  None: the calls of a run without the argument, one for one.
    ``row_margin_fit`` ``(z, sigma_prior, d_max)``, only with ``forecast='fit'`` (ValueError otherwise): the
    margin is formed at the head of every step from the residuals of the fit the step forecasts with -- node k leaves
    ``d_k = a + b k + z s g_k`` metres, at most ``d_max``, per instance and row (``problem.fit_margin_statement``): s the residual
    standard deviation of the window, at least ``sigma_prior``, g_k the growth of the forecast's error along the horizon, and
    ``(a, b)`` the ``row_margin`` of the same call, (0, 0) without one -- which then is this margin's base and no table of its own.
    On the device one smpc_forecast_row_margin behind the forecast inside the captured half of every step, and on the backup handle
    behind its forecast at an abort event, over its own horizon; on the host the statement and solver.set_instance_row_bounds per
    step.  Both handles end without a table and the result gains ``'row_margin_fit'``.  Not with the parallel policy (ValueError).
    None: the calls of a run without the argument, one for one.
    ``forecast='kalman'`` with ``kalman = (q, r[, v0, a0, beta])``: the controller forecasts with a Kalman filter
    per (instance, row) -- ``forecast_degree`` 0, 1 (the default here) or 2 its model, q the process noise, r the sensor noise in
    metres (``problem.kalman_params``, ``problem.kalman_statement``); ``forecast_window`` is not read.  One advancing forecast at the
    head of every step, inside the captured half on the device; ``observed`` may hold NaN here, samples that are missing
    (``problem.occlude_tracks``): the filter skips its update and its covariance grows.  The backup handle of an abort event forecasts
    from the aborting instances' records as they are, over its own horizon, and is given no world.  The state is the run's: numpy on
    the host path, one device tensor of a fixed address on the device path.
    ``row_margin_kalman`` ``(z, d_max)``, only with ``forecast='kalman'``: the margin formed behind every such forecast from the
    filter's predicted covariance (``problem.kalman_margin_statement``), ``row_margin`` its base as for ``row_margin_fit``.  The result
    gains ``'kalman'`` (all five numbers), ``'forecast_degree'`` and ``'row_margin_kalman'``.  ValueError before anything is built:
    the parallel policy, ``forecast='kalman'`` without ``kalman`` or either argument without it, ``row_margin_fit`` with it, a solver
    without the calls."""
    import time
    B = x_guess.shape[0]
    world = _check_world(B, cont_name, noise, scenes, row_margin, forecast, forecast_window, forecast_degree, observed, models,
                         row_margin_fit, kalman, row_margin_kalman)
    curves = traj is not None and np.ndim(traj) == 3
    if curves:
        traj = np.ascontiguousarray(traj, np.float64)
        if traj.shape[0] != B or traj.shape[1] != 3:
            raise ValueError(f'traj: expected [3, L] or [{B}, 3, L], got {traj.shape}')
    n_steps = int(n_steps if n_steps is not None else params.n_steps)
    if on_device:
        make_controller = make_controller or (lambda name, batch: get_controller(name, params, batch, device=device, device_state=True))
        make_backup = make_backup or (lambda batch: SafeBackupController(params, batch, device=device, device_state=True))
    else:
        make_controller = make_controller or (lambda name, batch: get_controller(name, params, batch))
        make_backup = make_backup or (lambda batch: SafeBackupController(params, batch))
    if collect_times:
        graphs = False
    if groups is None:
        groups = max(1, min(2, B // 512)) if on_device else 1      # measured at B = 4096 (MI355X, r2): 1: 5.1, 2: 4.55, 3: 5.8 ms/step
    from .sharding import shard_range
    spans = [shard_range(B, groups, g) for g in range(groups)]
    gens, grps, streams = [], [], []
    for lo, hi in spans:
        ctrl = make_controller(cont_name, hi - lo)
        if world.models is not None:
            _require(ctrl.ocp_solver, 'models', 'set_instance_models')
        backup = make_backup(hi - lo)
        _check_state_kind(ctrl, backup, on_device)
        if traj is not None:
            ctrl.setTrajectory(traj[lo:hi] if curves else traj)
        args = (params, x_guess[lo:hi], u_guess[lo:hi], noise, control_noise, ctrl, backup, n_steps, lo, callback, collect_times)
        if on_device:
            import torch
            sv = ctrl.ocp_solver
            streams.append(torch.cuda.ExternalStream(sv.L.smpc_stream(sv.h), device=torch.device('cuda', sv.device)))
            with torch.cuda.stream(streams[-1]):
                grp = _DeviceGroup(*args, use_graphs=graphs, world=world.rows(lo, hi))
        else:
            streams.append(None)
            grp = _HostGroup(*args, world=world.rows(lo, hi))
        grps.append(grp)
        gens.append(grp.run())

    def advance(g):
        """runs group g up to its next yield (end of the enqueue phase of a step); False once the group is finished"""
        try:
            if streams[g] is not None:
                import torch
                with torch.cuda.stream(streams[g]):      # torch ops and engine calls of a group share the handle's stream
                    next(gens[g])
            else:
                next(gens[g])
            return True
        except StopIteration:
            return False

    live = [True] * groups
    t_loop, j_loop, j = time.perf_counter(), 0, 0
    warm = min(4, n_steps // 2)
    while any(live):
        for g in range(groups):
            if live[g]:
                live[g] = advance(g)
        j += 1
        if timing is not None and j == warm + 1:          # the first steps allocate workspaces: time the rest
            if on_device:
                import torch
                torch.cuda.synchronize()
            t_loop, j_loop = time.perf_counter(), j
    if timing is not None:
        if on_device:
            import torch
            torch.cuda.synchronize()
        done = max(n_steps + 1 - j_loop, 1)
        timing['ms_per_step'] = 1e3 * (time.perf_counter() - t_loop) / done
        timing['steps'], timing['groups'] = done, groups

    # merge the groups (global instance indices)
    outs = []
    for g, grp in enumerate(grps):
        if streams[g] is not None:
            import torch
            with torch.cuda.stream(streams[g]):
                outs.append(grp.results(score))
        else:
            outs.append(grp.results(score))
    x_sim = np.concatenate([o['x'] for o in outs], axis=0)
    conv = np.concatenate([o['conv'] for o in outs])
    collided = np.concatenate([o['collided'] for o in outs])
    viable = np.concatenate([o['viable'] for o in outs])
    conv_idx = np.where(conv)[0].tolist()
    coll_idx = np.where(collided)[0].tolist()
    cs, ks = set(conv_idx), set(coll_idx)
    if getattr(params, 'reference_quirks', True):
        # mpc.py:189 appends an instance to viable_idx at EVERY abort event and :277-278 removes it ONCE when it converges: one that
        # went through two events and converged is in both lists; a failure recorded at the last step does not stop the
        # convergence test of :273 either (results(): conv is taken from x_sim[-1] alone)
        viable_idx = [int(i) for i in np.where(viable - conv.astype(np.int64) > 0)[0] if i not in ks]
    else:
        viable_idx = [int(i) for i in np.where(viable)[0] if i not in cs and i not in ks]
    unconv_idx = sorted(set(range(B)) - cs - ks - set(viable_idx))
    # x_viable: one row per abort event, in the order the reference's loops produce them (instance-major, then time: mpc.py:102,125)
    ev = [e for o in outs for e in o['abort_events']]
    if ev:
        inst, step, xv = np.concatenate([e[0] for e in ev]), np.concatenate([e[1] for e in ev]), np.concatenate([e[2] for e in ev])
        x_viable = xv[np.lexsort((step, inst))]
    else:
        x_viable = np.zeros((0, x_sim.shape[2]))
    # 'r': the reference allocates r_index as NaN and never writes it (mpc.py:116, 281) -- kept NaN for format parity; the
    # receding index actually used at every step is returned next to it as 'r_receding' (-1 where the policy has none)
    extra = {}
    if collect_times:
        ts = np.concatenate([o['time_rows'] for o in outs], axis=0)
        extra = {'time_stats': ts, 'time_fields': list(TIME_FIELDS), 'time_lost': int(sum(o['time_lost'] for o in outs)),
                 'time_q99': np.quantile(ts, 0.99, axis=0) if len(ts) else np.zeros(len(TIME_FIELDS))}
    if score:
        extra['score'] = {k: np.concatenate([o['score'][k] for o in outs]) for k in outs[0]['score']}
    if scenes is not None:
        extra['scenes'] = np.concatenate([o['scenes'] for o in outs], axis=0)
    if world.forecast is not None:
        extra.update(world.forecast.result_keys(observed is not None))
    if world.row_margin is not None:
        extra['row_margin'] = world.row_margin
    if world.row_margin_fit is not None:
        extra['row_margin_fit'] = world.row_margin_fit
    if world.row_margin_kalman is not None:
        extra['row_margin_kalman'] = world.row_margin_kalman
    return {**extra, 'x': x_sim, 'u': np.concatenate([o['u'] for o in outs], axis=0),
            'r': np.full((B, n_steps, 1), np.nan), 'r_receding': np.concatenate([o['r_receding'] for o in outs], axis=0),
            'conv_idx': conv_idx, 'collisions_idx': coll_idx, 'unconv_idx': unconv_idx, 'viable_idx': viable_idx,
            'x_viable': x_viable}


def save_pickle(path, obj):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, 'wb') as f:
        pickle.dump(obj, f)
