"""Training data of the learned safe set, and its fit.

What the reference's ``NetSafeSet`` learns (safe_set.py:71-104: ``nn(q_norm, d) (100 - alpha) / 100 - |qd| >= 0``) is, for a joint
configuration ``q`` and a unit direction ``d``, the largest speed ``s`` such that ``(q, s d)`` can still be brought to rest without
leaving the state box, the torque limits or the collision-free space.  This module makes that function for the robot and scene at
hand: rays ``(q, d)`` are labelled by bisection on ``s``, every trial one solve of the backup OCP (zero cost, terminal zero
velocity) from ``x0 = (q, s d)``, and every label comes with the trajectory that proves it.

* :func:`sample_rays`           -- collision-free Halton configurations, seeded directions, the velocity box along them
* :func:`ray_update_statement`  -- the rule for one look at every ray, numpy; ``smpc_ray_update`` (k_ray_update) is held against it
* :func:`label_rays`            -- the labelling loop: on the device (``solver.sqp`` / ``check_guess`` / ``ray_update`` and a 4-byte
  read per round) or driven by the statement, with any solver
* :func:`fit_safe_set`, :func:`save_checkpoint`, :func:`save_dataset` -- the network and the reference's checkpoint format

DESIGN.md section 9g has the contract and the measurements behind the acceptance rule.
"""
from __future__ import annotations

import numpy as np

from ._lib import RAY_BRACKETED, RAY_DEAD, RAY_OPEN, RAY_SATURATED, RayState, SqpOpts, SqpState

OPEN, DEAD, SATURATED, BRACKETED = RAY_OPEN, RAY_DEAD, RAY_SATURATED, RAY_BRACKETED
KIND_NAMES = {OPEN: 'open', DEAD: 'dead', SATURATED: 'saturated', BRACKETED: 'bracketed'}


# ---- rays ----------------------------------------------------------------------------------------------------------------------------
def velocity_box_along(problem, d):
    """s_hi [n]: the largest s with s d inside the velocity box (the last nq entries of problem.x_min / x_max)"""
    nq = problem.nq
    d = np.asarray(d, float)
    lo, hi = problem.x_min[nq:], problem.x_max[nq:]
    with np.errstate(divide='ignore', invalid='ignore'):
        lim = np.where(d > 0.0, hi / d, np.where(d < 0.0, lo / d, np.inf))
    return lim.min(axis=1)


def sample_rays(problem, n, seed, solver=None):
    """``n`` rays for ``problem``: ``(q [n, nq], d [n, nq], s_hi [n])``.

    q: the Halton points of the joint box that pass the collision filter at rest, in sampling order -- the
    stream ``closed_loop._FreeStarts`` draws.  The filter is ``solver.check_trajectory(.., tol_x=0)`` where a solver is given,
    as there; without one, the numpy row values of ``ik.ik_eval`` against the same check bounds.  d: ``default_rng(seed)`` standard
    normal draws, normalised.  s_hi: :func:`velocity_box_along`.  The network's inputs are (q, d) of ALL joints: ``n_dof_safe_set <
    nq`` is not supported and raises ValueError."""
    from .closed_loop import halton
    nq = problem.nq
    if int(problem.params.n_dof_safe_set) != nq:
        raise ValueError(f'sample_rays: n_dof_safe_set = {problem.params.n_dof_safe_set} != nq = {nq} is not supported')
    n = int(n)
    q = np.zeros((0, nq))
    drawn, barren = 0, 0
    while len(q) < n:
        chunk = max(64, 2 * (n - len(q)))
        c = problem.x_min[:nq] + halton(chunk, nq, skip=1 + drawn) * (problem.x_max[:nq] - problem.x_min[:nq])
        drawn += chunk
        if solver is not None:
            x = np.hstack([c, np.zeros_like(c)])
            free = np.asarray(solver.check_trajectory(x[:, None, :], tol_x=0.0)).astype(bool)
        elif len(problem.rows):
            from .ik import ik_eval, ik_params
            rv = ik_eval(problem, c, np.zeros((chunk, 3)), ik_params(problem))['rows']
            free = np.all((rv >= problem.row_check[:, 0]) & (rv <= problem.row_check[:, 1]), axis=1)
        else:
            free = np.ones(chunk, bool)
        barren = 0 if free.any() else barren + 1
        if barren >= 64:
            raise RuntimeError(f'the collision filter rejected {barren * chunk} Halton configurations in a row')
        q = np.vstack([q, c[free]])
    q = np.ascontiguousarray(q[:n])
    d = np.random.default_rng(int(seed)).standard_normal((n, nq))
    d = d / np.sqrt((d * d).sum(1))[:, None]
    return q, d, velocity_box_along(problem, d)


# ---- the rule for one look ------------------------------------------------------------------------------------------------------------
def new_ray_state(q, d, s_hi, N):
    """numpy ``smpc_ray_state`` of the rays (q, d) before trial 0 (what ``BatchedOcpSolver.new_ray_state`` builds)"""
    q, d = np.ascontiguousarray(q, np.float64), np.ascontiguousarray(d, np.float64)
    B, nq = q.shape
    shapes = {'q': (B, nq), 'd': (B, nq), 'x_cert': (B, N + 1, 2 * nq), 'u_cert': (B, N, nq)}
    st = {k: np.zeros(shapes.get(k, (B,)), dt) for k, dt in RayState.FIELDS}
    st['q'][...], st['d'][...], st['hi'][...] = q, d, np.asarray(s_hi, np.float64)
    st['open'][:] = 1
    return st


def ray_update_statement(rays, sqp, flags, x0, x_guess, u_guess, bisect, budget, tol_term, mu0=10.0):
    """The rule of ``smpc_ray_update`` (include/smpc.h) on numpy arrays, in place; returns the number of rays still open.

    For every ray with ``open != 0``, after a round of SQP iterations and a ``check_guess`` (flags): the trial in flight is
    *feasible* if status == 0, flags == 0, max |v_N| <= tol_term, node 0 of the iterate equals x0 to 1e-12 and the iterate holds no
    NaN; *infeasible* if it is not feasible and the instance is done, has used ``budget`` iterations or holds a NaN; *pending*
    otherwise (left untouched).  Feasible: the iterate becomes the ray's certificate, lo = s.  Infeasible: hi = s.  Then the ray ends
    (trial 0 infeasible: DEAD; trial 1 feasible: SATURATED; trial bisect + 1: BRACKETED; open = 0, done = 1) or its next trial starts
    from the constant guess at s = hi (after trial 0) or (lo + hi) / 2, with a fresh SQP state."""
    B, nq = rays['q'].shape
    X = x_guess.reshape(B, -1)
    U = u_guess.reshape(B, -1)
    e0 = x_guess[:, 0] - x0
    nan_any = np.isnan(X).any(1) | np.isnan(U).any(1) | np.isnan(e0).any(1)
    with np.errstate(invalid='ignore'):
        vmax = np.abs(np.nan_to_num(x_guess[:, -1, nq:], nan=0.0)).max(1)
        off = np.abs(np.nan_to_num(e0, nan=0.0)).max(1)
        is_open = rays['open'] != 0
        feasible = is_open & (sqp['status'] == 0) & (flags == 0) & (vmax <= tol_term) & (off <= 1e-12) & ~nan_any
        ended = (sqp['done'] != 0) | (sqp['iters'] >= int(budget)) | nan_any
    infeasible = is_open & ~feasible & ended
    resolved = feasible | infeasible
    t = rays['trial'].copy()
    rays['x_cert'][feasible] = x_guess[feasible]
    rays['u_cert'][feasible] = u_guess[feasible]
    rays['lo'][feasible] = rays['s'][feasible]
    rays['hi'][infeasible] = rays['s'][infeasible]
    rays['trial'][resolved] += 1
    rays['iters_total'][resolved] += sqp['iters'][resolved]
    dead = infeasible & (t == 0)
    saturated = feasible & (t == 1)
    bracketed = resolved & ~dead & ~saturated & (t >= int(bisect) + 1)
    for mask, kind in ((dead, DEAD), (saturated, SATURATED), (bracketed, BRACKETED)):
        rays['kind'][mask] = kind
    finished = dead | saturated | bracketed
    rays['open'][finished] = 0
    sqp['done'][finished] = 1
    nxt = resolved & ~finished
    s_new = np.where(t == 0, rays['hi'], 0.5 * (rays['lo'] + rays['hi']))
    start = np.hstack([rays['q'], s_new[:, None] * rays['d']])
    rays['s'][nxt] = s_new[nxt]
    x0[nxt] = start[nxt]
    x_guess[nxt] = start[nxt][:, None, :]
    u_guess[nxt] = 0.0
    for key, _ in SqpState.FIELDS:
        sqp[key][nxt] = mu0 if key == 'mu' else 0
    return int((rays['open'] != 0).sum())


def check_guess_host(ctrl, x, u):
    """flags [B] of ``smpc_check_guess`` (bits 0 state box, 1 collision rows on EVERY node, 2 torque, 3 dynamics; no safe node)
    composed from ``solver.eval_nodes`` and ``solver.guess_correction``: for a solver without ``check_guess``"""
    pr, par, sv = ctrl.problem, ctrl.params, ctrl.ocp_solver
    B, N, nq, nr = x.shape[0], ctrl.N, ctrl.nq, int(pr.desc.n_rows)
    ev = sv.eval_nodes(x, u, ctrl.p)
    with np.errstate(invalid='ignore'):
        w0 = np.maximum(pr.x_min - x, x - pr.x_max).reshape(B, -1).max(1)
        flags = (~(w0 <= par.tol_x)) * 1
        if nr:
            rv = np.asarray(ev['row_val'])[:, :, :nr]
            w1 = np.maximum(pr.row_check[:, 0] - rv, rv - pr.row_check[:, 1]).reshape(B, -1).max(1)
            flags = flags + (~(w1 <= 0.0)) * 2
        tau = np.asarray(ev['tau'])[:, :N, :nq]
        w2 = np.maximum(pr.tau_min - tau, tau - pr.tau_max).reshape(B, -1).max(1)
        w3 = np.linalg.norm((x - np.asarray(sv.guess_correction(x.copy(), u))).reshape(B, -1), axis=1)
        flags = flags + (~(w2 <= par.tol_tau)) * 4 + (~(w3 < par.tol_dyn * np.sqrt(N + 1))) * 8
    return flags.astype(np.int32)


# ---- the labelling loop ----------------------------------------------------------------------------------------------------------------
def _resize(ctrl, B):
    """the controller at the chunk's batch size.  The controller classes have no public way to change B, so this re-allocates
    through ``_alloc`` / ``reset_controller`` as ``resetHorizon`` does: the guesses, x_viable, fails and current_step start over and
    ``p`` is rebuilt from the problem (ee_ref, alpha, flag 1; a trajectory set with setTrajectory stays attached).  None of that
    state means anything to a backup controller that is only solved from constant guesses."""
    if ctrl.xp.on_device:
        raise ValueError('label_rays: a controller with numpy state is expected (device_state=False)')
    if ctrl.B != B:
        ctrl.B = int(B)
        ctrl._alloc()
        ctrl.reset_controller()


def _label_chunk_statement(ctrl, rays, n_live, bisect, budget, check_every, opts, mu0):
    """one chunk driven by :func:`ray_update_statement`: the SQP rounds through ``solver.sqp`` on numpy arrays where the solver has
    one (the engine, host-pointer path), through closed_loop.sqp_host_advance otherwise"""
    from .closed_loop import new_host_sqp_state, sqp_host_advance
    sv, N = ctrl.ocp_solver, ctrl.N
    B = rays['q'].shape[0]
    x0 = np.hstack([rays['q'], rays['s'][:, None] * rays['d']])
    xg = np.ascontiguousarray(np.repeat(x0[:, None, :], N + 1, axis=1))
    ug = np.zeros((B, N, ctrl.nu))
    state = new_host_sqp_state(B, mu0)
    state['done'][n_live:] = 1
    flags = np.zeros(B, np.int32)
    engine = hasattr(sv, 'sqp') and hasattr(sv, 'check_guess')
    rounds = 0
    while int((rays['open'] != 0).sum()):
        if engine:
            xg, ug, _ = sv.sqp(x0, xg, ug, ctrl.p, dict(max_iter=check_every, mu0=mu0, **opts), state)
            f, _ = sv.check_guess(xg, ug, safe_node=None, collision_first_node=0, mask=rays['open'])
            flags = np.where(rays['open'] != 0, f, flags).astype(np.int32)
        else:
            ctrl.setGuess(xg, ug)
            sqp_host_advance(ctrl, x0, state, check_every, sqp_tol=opts['tol'], armijo=opts['armijo'],
                             alpha_reduction=opts['alpha_reduction'], alpha_min=opts['alpha_min'])
            xg, ug = np.ascontiguousarray(ctrl.x_guess), np.ascontiguousarray(ctrl.u_guess)
            flags = np.where(rays['open'] != 0, check_guess_host(ctrl, xg, ug), flags).astype(np.int32)
        ray_update_statement(rays, state, flags, x0, xg, ug, bisect, budget, ctrl.params.tol_x, mu0)
        rounds += 1
    return rounds


def _label_chunk_device(ctrl, rays_np, n_live, bisect, budget, check_every, opts, mu0):
    """one chunk with the bookkeeping on the device: a round is sqp, check_guess, ray_update and a 4-byte read"""
    import torch
    sv, N = ctrl.ocp_solver, ctrl.N
    dev = torch.device('cuda', sv.device)
    to = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)
    B = rays_np['q'].shape[0]
    p_d = to(ctrl.p)
    rays = {k: to(v) for k, v in rays_np.items()}
    x0_np = np.hstack([rays_np['q'], rays_np['s'][:, None] * rays_np['d']])
    x0 = to(x0_np)
    xg = to(np.repeat(x0_np[:, None, :], N + 1, axis=1))
    ug = torch.zeros((B, N, ctrl.nu), dtype=torch.float64, device=dev)
    state = sv.new_sqp_state(B, x0, mu0)
    state['done'][n_live:] = 1
    flags = torch.zeros((B,), dtype=torch.int32, device=dev)
    worst = torch.zeros((B, 5), dtype=torch.float64, device=dev)
    n_open = torch.zeros((1,), dtype=torch.int32, device=dev)
    sqp_opts = dict(max_iter=check_every, mu0=mu0, **opts)
    rounds, left = 0, n_live
    while left:
        sv.sqp(x0, xg, ug, p_d, sqp_opts, state)
        sv.check_guess(xg, ug, safe_node=None, collision_first_node=0, mask=rays['open'], flags=flags, worst=worst)
        sv.ray_update(rays, state, flags, x0, xg, ug, n_open, bisect=bisect, budget=budget, tol_term=ctrl.params.tol_x, mu0=mu0)
        left = int(n_open.item())
        rounds += 1
    sv.sync()
    for k in rays_np:
        rays_np[k][...] = rays[k].cpu().numpy()
    return rounds


def label_rays(ctrl, q, d, s_hi, bisect=8, budget=30, check_every=5, batch=None, bookkeeping='auto', sqp_tol=1e-6, armijo=1e-4,
               alpha_reduction=0.7, alpha_min=0.05, scenes=None):
    """Labels of the rays ``(q, d)`` [n, nq] by bisection on the speed, on a backup controller (``get_controller`` has none: a
    ``controller.SafeBackupController``).

    Per ray the trials run in a fixed order: trial 0 at s = 0, trial 1 at s = ``s_hi``, trials 2 .. ``bisect`` + 1 at the middle of
    the bracket.  A trial starts from the constant guess at ``x0 = (q, s d)`` with a fresh SQP state and is looked at after every
    ``check_every`` SQP iterations (:func:`ray_update_statement` has the rule): it is feasible at the FIRST look where the iterate
    passes -- a feasible iterate is a complete certificate, and the zero-cost backup OCP does not settle -- and infeasible once the
    instance is done or has used ``budget`` iterations (rounded up to a multiple of ``check_every``).  Trial 0 infeasible: DEAD, label
    NaN.  Trial 1 feasible: SATURATED, label ``s_hi``.  Otherwise BRACKETED after the last bisection step, label ``lo``; the last
    feasible trial's iterate is the certificate.

    ``batch`` splits the rays into chunks (the last one padded with finished slots); a ray's result does not depend on it provided its
    SQP does not -- pin the engine's QP form (``ctrl.ocp_solver.set_qp_mode('throughput')``) as closed_loop.generate_guess_until
    documents.  The controller is resized to the chunk.  ``bookkeeping``: 'device' (``solver.ray_update``), 'statement' (host
    decisions by :func:`ray_update_statement`, any solver) or 'auto' (the device where the solver has ``ray_update``).

    ``scenes`` [n, n_rows, 8]: a scene of its own for every ray (problem.jittered_scenes).  Per chunk, the
    chunk's scenes, padded like ``q``, are set on the controller's solver (``set_instance_scene``; ValueError for a solver without
    one) and cleared behind the loop, also when a round raises.  A ray whose ``q`` collides in its own scene comes out DEAD.

    Returns a dict: ``label`` [n], ``kind`` [n] (DEAD / SATURATED / BRACKETED), ``lo``, ``hi``, ``trials`` (trials run), ``iters`` (SQP
    iterations of all trials), ``x_cert`` [n, N+1, nx], ``u_cert`` [n, N, nu], ``rounds`` (of all chunks)."""
    if bookkeeping not in ('auto', 'device', 'statement'):
        raise ValueError("bookkeeping must be 'auto', 'device' or 'statement'")
    bisect, budget, check_every = int(bisect), int(budget), int(check_every)
    if bisect < 0 or budget < 1 or check_every < 1:
        raise ValueError('label_rays: bisect >= 0, budget >= 1 and check_every >= 1 expected')
    q, d, s_hi = np.atleast_2d(np.asarray(q, float)), np.atleast_2d(np.asarray(d, float)), np.asarray(s_hi, float).reshape(-1)
    n, nq = q.shape
    if nq != ctrl.nq or d.shape != q.shape or s_hi.shape != (n,):
        raise ValueError(f'label_rays: q, d [n, {ctrl.nq}] and s_hi [n] expected')
    if scenes is not None:
        scenes = np.ascontiguousarray(scenes, np.float64)
        if not hasattr(ctrl.ocp_solver, 'set_instance_scene'):
            raise ValueError(f'label_rays(scenes=...): {type(ctrl.ocp_solver).__name__} has no set_instance_scene')
        if scenes.ndim != 3 or scenes.shape[0] != n:
            raise ValueError(f'label_rays: scenes [n = {n}, n_rows, 8] expected, got {scenes.shape}')
    on_device = hasattr(ctrl.ocp_solver, 'ray_update') if bookkeeping == 'auto' else bookkeeping == 'device'
    if on_device and not hasattr(ctrl.ocp_solver, 'ray_update'):
        raise ValueError(f"label_rays(bookkeeping='device') needs a solver with ray_update; {type(ctrl.ocp_solver).__name__} has none")
    N = ctrl.N
    budget = -(-budget // check_every) * check_every
    opts = dict(tol=sqp_tol, armijo=armijo, alpha_reduction=alpha_reduction, alpha_min=alpha_min)
    mu0 = SqpOpts().mu0
    out = {'label': np.full(n, np.nan), 'kind': np.zeros(n, np.int32), 'lo': np.zeros(n), 'hi': np.zeros(n), 'trials': np.zeros(n, np.int32),
           'iters': np.zeros(n, np.int32), 'x_cert': np.zeros((n, N + 1, 2 * nq)), 'u_cert': np.zeros((n, N, nq)), 'rounds': 0}
    if n == 0:
        return out
    B = max(1, min(int(batch) if batch else n, n))
    _resize(ctrl, B)
    for lo in range(0, n, B):
        m = min(B, n - lo)
        pad = lambda a: np.concatenate([a[lo:lo + m], np.repeat(a[lo:lo + 1], B - m, axis=0)])
        rays = new_ray_state(pad(q), pad(d), pad(s_hi), N)
        rays['open'][m:] = 0                                        # padding slots: finished rays, skipped by every kernel
        run = _label_chunk_device if on_device else _label_chunk_statement
        if scenes is None:
            out['rounds'] += run(ctrl, rays, m, bisect, budget, check_every, opts, mu0)
        else:
            try:
                ctrl.ocp_solver.set_instance_scene(pad(scenes))
                out['rounds'] += run(ctrl, rays, m, bisect, budget, check_every, opts, mu0)
            finally:
                ctrl.ocp_solver.set_instance_scene(None)
        sl = slice(lo, lo + m)
        out['kind'][sl], out['lo'][sl], out['hi'][sl] = rays['kind'][:m], rays['lo'][:m], rays['hi'][:m]
        out['trials'][sl], out['iters'][sl] = rays['trial'][:m], rays['iters_total'][:m]
        out['x_cert'][sl], out['u_cert'][sl] = rays['x_cert'][:m], rays['u_cert'][:m]
    out['label'] = np.where(out['kind'] == DEAD, np.nan, out['lo'])
    return out


# ---- the fit and the checkpoint -----------------------------------------------------------------------------------------------------
def fit_safe_set(data, params, epochs, seed, hidden=None, device='cpu', lr=3e-3, batch_size=256, context=None):
    """Fits the reference's network (``NeuralNetwork(*params.net_size, activation(params.act))``; ``hidden`` overrides the width) to
    labelled rays: ``data`` with ``q``, ``d``, ``label`` and ``kind`` (DEAD rays are dropped).  Inputs ``((q - mean) / std, d)`` with
    mean / std per joint from the sampled q, target the label, MSE, Adam, mini-batches in a seeded order; the output bias starts at
    the mean label.  The ``eps`` the reference adds to the first velocity before normalising it (safe_set.py:83) is not modelled.
    ``context`` [n, n_ctx]: numbers of every ray's scene (problem.scene_context) as extra inputs behind (q, d), normalised by their
    own mean / std over the kept rays (``info['ctx_mean']``, ``info['ctx_std']``); ``net_size[0]`` must then be ``2 nq + n_ctx``
    (DESIGN.md section 9j).
    Returns ``(net, mean, std, info)``; the same seed gives the same weights."""
    import torch
    from .safe_set import NeuralNetwork, activation
    keep = np.asarray(data['kind']) != DEAD
    q, d = np.asarray(data['q'], float)[keep], np.asarray(data['d'], float)[keep]
    y = np.asarray(data['label'], float)[keep]
    if len(q) == 0 or not np.all(np.isfinite(y)):
        raise ValueError('fit_safe_set: no labelled ray, or a non-finite label on a ray that is not DEAD')
    mean, std = q.mean(0), q.std(0)
    std = np.where(std > 0.0, std, 1.0)
    size = [int(v) for v in params.net_size]
    if hidden is not None:
        size[1] = int(hidden)
    cols = [None, d]
    extra = {}
    if context is not None:
        ctx = np.asarray(context, float)
        if ctx.ndim != 2 or ctx.shape[0] != len(keep):
            raise ValueError(f'fit_safe_set: context [n = {len(keep)}, n_ctx] expected, got {ctx.shape}')
        ctx = ctx[keep]
        ctx_mean, ctx_std = ctx.mean(0), ctx.std(0)
        ctx_std = np.where(ctx_std > 0.0, ctx_std, 1.0)
        cols.append((ctx - ctx_mean) / ctx_std)
        extra = {'ctx_mean': ctx_mean, 'ctx_std': ctx_std}
    n_in = 2 * q.shape[1] + (0 if context is None else ctx.shape[1])
    if size[0] != n_in or size[2] != 1:
        raise ValueError(f'fit_safe_set: net_size {size} does not take (q, d) of {q.shape[1]} joints'
                         + ('' if context is None else f' and {ctx.shape[1]} context numbers ({n_in} inputs)') + ' to one output')
    torch.manual_seed(int(seed))
    net = NeuralNetwork(*size, activation(params.act)).float()
    with torch.no_grad():
        net.linear_stack[-1].bias.fill_(float(y.mean()))
    dev = torch.device(device)
    net = net.to(dev)
    cols[0] = (q - mean) / std
    X = torch.as_tensor(np.hstack(cols), dtype=torch.float32, device=dev)
    Y = torch.as_tensor(y, dtype=torch.float32, device=dev)
    opt = torch.optim.Adam(net.parameters(), lr=lr)
    gen = torch.Generator().manual_seed(int(seed))
    loss = torch.zeros(())
    for _ in range(int(epochs)):
        order = torch.randperm(len(X), generator=gen).to(dev)
        for lo in range(0, len(X), int(batch_size)):
            idx = order[lo:lo + int(batch_size)]
            opt.zero_grad()
            loss = torch.mean((net(X[idx]).reshape(-1) - Y[idx]) ** 2)
            loss.backward()
            opt.step()
    net = net.cpu().eval()
    with torch.no_grad():
        rmse = float(torch.sqrt(torch.mean((net(X.cpu()).reshape(-1) - Y.cpu()) ** 2)))
    return net, mean, std, {'rays': int(keep.sum()), 'dropped': int((~keep).sum()), 'train_rmse': rmse, 'net_size': size, **extra}


def predict(net, mean, std, q, d, ctx=None):
    """the fitted network's labels for rays (q, d), numpy; ``ctx`` [n, n_ctx]: the NORMALISED context of a net fitted with one"""
    import torch
    cols = [(np.asarray(q, float) - mean) / std, np.asarray(d, float)] + ([] if ctx is None else [np.asarray(ctx, float)])
    X = torch.as_tensor(np.hstack(cols), dtype=torch.float32)
    with torch.no_grad():
        return net(X).reshape(-1).numpy().astype(float)


def save_checkpoint(path, net, mean, std, ctx_mean=None, ctx_std=None, ctx_select=None):
    """``{'model': state_dict, 'mean', 'std'}``: the reference's checkpoint (safe_set.py:76-85), what ``network_path:`` names and
    ``SafeSetNet.from_params`` reads.  A net fitted with a context also carries ``ctx_mean``, ``ctx_std`` and ``ctx_select`` (the
    ``(row, slot)`` pairs of problem.scene_context); without them the file is the reference's, key for key."""
    import torch
    ck = {'model': {k: v.detach().cpu() for k, v in net.state_dict().items()},
          'mean': torch.as_tensor(np.asarray(mean, np.float64)), 'std': torch.as_tensor(np.asarray(std, np.float64))}
    if ctx_mean is not None:
        if ctx_std is None or ctx_select is None:
            raise ValueError('save_checkpoint: ctx_mean, ctx_std and ctx_select go together')
        ck['ctx_mean'] = torch.as_tensor(np.asarray(ctx_mean, np.float64))
        ck['ctx_std'] = torch.as_tensor(np.asarray(ctx_std, np.float64))
        ck['ctx_select'] = torch.as_tensor(np.asarray(ctx_select, np.int64).reshape(-1, 2))
    torch.save(ck, path)


def save_dataset(path, q, d, s_hi, labels, ctx=None):
    """the dataset as .npz: q, d, s_hi, label, kind, trials (and ctx [n, n_ctx], the raw context of every ray, where given)"""
    extra = {} if ctx is None else {'ctx': np.asarray(ctx, float)}
    np.savez(path, q=q, d=d, s_hi=s_hi, label=labels['label'], kind=labels['kind'], trials=labels['trials'], **extra)
