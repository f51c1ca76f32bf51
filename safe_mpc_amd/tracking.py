"""The reference curves of the trajectory-tracking task: ``cost.traj`` of the reference's Tracking8* and TrackingMovingCircle*
costs (cost_definition.py:102-288), ``[3, n_steps_tracking + 1 + N]`` end-effector points that ``AbstractController.setTrajectory``
takes -- column ``current_step + i`` is the reference of node i (controller.py:153-156).

* :func:`lemniscate_trajectory`    -- generate_8shape_trajectory (cost_definition.py:170-199)
* :func:`moving_circle_trajectory` -- generate_moving_circle_trajectory (cost_definition.py:264-288)
* :func:`tracking_trajectory`      -- the entry: picks the curve and sets ``params.n_steps`` like the reference's cost classes
* :func:`tracking_curves`          -- the batched form: ``[B, 3, L]``, a displaced / resized / re-timed curve per instance
* :func:`jittered_curves`          -- ``tracking_curves`` with seeded normal draws on the offset and log-normal ones on the size

Both curves advance their parameter theta by ``velocity * dt`` divided by the curve's speed per unit theta, one column at a time;
with ``vel_const: false`` the velocity ramps from 0 by ``v_max / (n_steps_tracking * acc_time)`` per column while it is <= v_max.
"""
from __future__ import annotations

import numpy as np

CURVES = ('8', 'circle')

# every key of config.yaml's tracking section: (name, conversion, shipped value)
TRACKING_KEYS = (('n_steps_tracking', int, 5000), ('dim_shape_8', float, 0.27), ('offset_traj', 'vec', [0.65, 0.08, 0.1]),
                 ('theta_rot_traj', 'vec', [0.0, 0.0, 1.570]), ('vel_max_traj', float, 0.3), ('vel_const', bool, True),
                 ('acc_time', float, 0.2), ('circle_rad', float, 0.13), ('circle_traj_vel', float, 0.0),
                 ('circle_center_vel', float, 0.35), ('circle_offset_traj', 'vec', [0.78, 0.4, 0.06]))


def read_tracking_keys(params, cfg):
    """Parameters' part for the tracking section of config.yaml (cost_definition.py:105-114, 205-214); a key the file does not
    carry takes the shipped value"""
    for name, conv, default in TRACKING_KEYS:
        v = cfg.get(name, default)
        setattr(params, name, np.array(v, float) if conv == 'vec' else conv(v))


def _columns(params):
    return int(params.n_steps_tracking) + 1 + int(params.N)


def _ramp(params, v_max):
    """(start velocity, increment per column): constant v_max, or from 0 by v_max / (n_steps_tracking * acc_time) -- the reference
    divides by params.n_steps, which its cost classes have set to n_steps_tracking before (cost_definition.py:107, 185)"""
    if params.vel_const:
        return float(v_max), 0.0
    return 0.0, float(v_max) / (int(params.n_steps_tracking) * float(params.acc_time))


def _rot_xyz(th):
    cx, cy, cz = np.cos(th)
    sx, sy, sz = np.sin(th)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rx @ Ry @ Rz


def lemniscate_trajectory(params):
    """The "8": x = a cos t / (1 + sin^2 t), y = x sin t in the plane z = 0, rotated by Rx Ry Rz(theta_rot_traj) and then moved by
    offset_traj.  With s = sin t the derivative is dx/dt = -a s (3 - s^2) / (1 + s^2)^2, dy/dt = a (1 - 3 s^2) / (1 + s^2)^2."""
    a, dt = float(params.dim_shape_8), float(params.dt)
    vel, acc = _ramp(params, params.vel_max_traj)
    n = _columns(params)
    flat = np.zeros((3, n))
    theta = 0.0
    for i in range(n):
        s, c = np.sin(theta), np.cos(theta)
        den = 1.0 + s * s
        flat[0, i] = a * c / den
        flat[1, i] = a * c * s / den
        dx = -a * s * (3.0 - s * s) / (den * den)
        dy = a * (1.0 - 3.0 * s * s) / (den * den)
        theta = theta + vel / np.sqrt(dx * dx + dy * dy) * dt
        if not params.vel_const and vel <= params.vel_max_traj:
            vel += acc
    return _rot_xyz(np.asarray(params.theta_rot_traj, float)) @ flat + np.asarray(params.offset_traj, float).reshape(3, 1)


def moving_circle_trajectory(params):
    """A circle of radius circle_rad about a centre that slides along y by circle_center_vel * dt per column, turning round once
    the point's y has passed -0.5 or +0.5; circle_offset_traj is added, no rotation.  theta advances by
    velocity * dt / sqrt(circle_rad) (the reference's expression: the radius enters under the root)."""
    rad, dt = float(params.circle_rad), float(params.dt)
    vel, acc = _ramp(params, params.circle_traj_vel)
    off = np.asarray(params.circle_offset_traj, float)
    n = _columns(params)
    traj = np.zeros((3, n))
    theta, slide, sign = 0.0, 0.0, 1
    for i in range(n):
        slide = slide - sign * float(params.circle_center_vel) * dt
        traj[:, i] = np.array([-rad * np.cos(theta), rad * np.sin(theta) + slide, 0.0]) + off
        theta = theta + vel / np.sqrt(rad * (np.sin(theta) ** 2 + np.cos(theta) ** 2)) * dt
        if sign > 0 and traj[1, i] < -0.5:
            sign = -1
        if sign < 0 and traj[1, i] > 0.5:
            sign = 1
        if not params.vel_const and vel <= params.circle_traj_vel:
            vel += acc
    return traj


def tracking_trajectory(params, curve='8'):
    """The reference trajectory of a tracking run, ``[3, n_steps_tracking + 1 + N]``.  Like the reference's tracking costs
    (cost_definition.py:107, 117, 207, 216) it makes the run n_steps_tracking long (``params.n_steps``) and marks it as a
    tracking run (``params.track_traj``, which the file names carry)."""
    curve = str(curve)
    if curve not in CURVES:
        raise ValueError(f"curve must be one of {CURVES}, got {curve!r}")
    params.n_steps = int(params.n_steps_tracking)
    params.track_traj = True
    return lemniscate_trajectory(params) if curve == '8' else moving_circle_trajectory(params)


def _per_instance(name, value, default, B, tail):
    """``value`` ([B, *tail], or None = the key's value for everybody) as a float array [B, *tail]"""
    if value is None:
        return np.broadcast_to(np.asarray(default, float), (B,) + tail).copy()
    a = np.asarray(value, float)
    if a.shape != (B,) + tail:
        raise ValueError(f'{name}: shape {a.shape}, expected {(B,) + tail}')
    return a


def tracking_curves(params, curve='8', offsets=None, sizes=None, v_max=None, rotations=None, B=None):
    """The batched form of :func:`tracking_trajectory`: ``[B, 3, n_steps_tracking + 1 + N]``, instance b's curve being what
    ``tracking_trajectory`` gives on a copy of ``params`` with b's entries for the keys

    * ``offsets [B, 3]``   -> offset_traj / circle_offset_traj          * ``sizes [B]`` -> dim_shape_8 / circle_rad
    * ``v_max [B]``        -> vel_max_traj / circle_traj_vel            * ``rotations [B, 3]`` -> theta_rot_traj (the "8" only)

    An argument left None keeps the key's value for every instance; B is the arrays' first dimension (``B=`` where none is given,
    default 1).  Same arithmetic as the two generators above -- the ramp ``while vel <= v_max``, the circle's turn once y has passed
    -0.5 / +0.5 -- as array operations over the instances inside the column loop (L iterations).  Sets ``params.n_steps`` and
    ``params.track_traj`` like :func:`tracking_trajectory`."""
    curve = str(curve)
    if curve not in CURVES:
        raise ValueError(f"curve must be one of {CURVES}, got {curve!r}")
    given = [np.asarray(a).shape[0] for a in (offsets, sizes, v_max, rotations) if a is not None]
    if B is None:
        B = given[0] if given else 1
    B = int(B)
    if B < 1 or any(g != B for g in given):
        raise ValueError(f'tracking_curves: the per-instance arrays have {given} entries for B = {B}')
    if curve != '8' and rotations is not None:
        raise ValueError("rotations apply to the '8' only")
    eight = curve == '8'
    off = _per_instance('offsets', offsets, params.offset_traj if eight else params.circle_offset_traj, B, (3,))
    size = _per_instance('sizes', sizes, params.dim_shape_8 if eight else params.circle_rad, B, ())
    vmax = _per_instance('v_max', v_max, params.vel_max_traj if eight else params.circle_traj_vel, B, ())
    params.n_steps = int(params.n_steps_tracking)
    params.track_traj = True
    dt, n = float(params.dt), _columns(params)
    ramp = not params.vel_const
    vel = np.zeros(B) if ramp else vmax.copy()
    acc = vmax / (int(params.n_steps_tracking) * float(params.acc_time)) if ramp else np.zeros(B)
    theta = np.zeros(B)
    out = np.zeros((B, 3, n))
    if eight:
        a = size
        for i in range(n):
            s, c = np.sin(theta), np.cos(theta)
            den = 1.0 + s * s
            out[:, 0, i] = a * c / den
            out[:, 1, i] = a * c * s / den
            dx = -a * s * (3.0 - s * s) / (den * den)
            dy = a * (1.0 - 3.0 * s * s) / (den * den)
            theta = theta + vel / np.sqrt(dx * dx + dy * dy) * dt
            if ramp:
                vel = np.where(vel <= vmax, vel + acc, vel)
        rot = _per_instance('rotations', rotations, params.theta_rot_traj, B, (3,))
        R = np.stack([_rot_xyz(th) for th in rot])
        return np.matmul(R, out) + off[:, :, None]
    cvel = float(params.circle_center_vel)
    slide, sign = np.zeros(B), np.ones(B)
    for i in range(n):
        slide = slide - sign * cvel * dt
        out[:, 0, i] = -size * np.cos(theta) + off[:, 0]
        out[:, 1, i] = size * np.sin(theta) + slide + off[:, 1]
        out[:, 2, i] = 0.0 + off[:, 2]
        theta = theta + vel / np.sqrt(size * (np.sin(theta) ** 2 + np.cos(theta) ** 2)) * dt
        y = out[:, 1, i]
        sign = np.where((sign > 0) & (y < -0.5), -1.0, sign)
        sign = np.where((sign < 0) & (y > 0.5), 1.0, sign)
        if ramp:
            vel = np.where(vel <= vmax, vel + acc, vel)
    return out


def jittered_curves(params, curve, B, sigma, seed=0, scale_sigma=0.0):
    """B curves for a Monte-Carlo study of the tracking task: instance b's offset is the key's plus three N(0, sigma^2) draws and its
    size the key's times exp of one N(0, scale_sigma^2) draw, from ``np.random.default_rng(seed)`` taken instance by instance in that
    order.  The fourth draw is always taken, so the offsets do not depend on whether the size is jittered.  ``[B, 3, L]``
    (:func:`tracking_curves`)."""
    eight = str(curve) == '8'
    rng = np.random.default_rng(seed)
    base = np.asarray(params.offset_traj if eight else params.circle_offset_traj, float)
    size = float(params.dim_shape_8 if eight else params.circle_rad)
    offsets, sizes = np.zeros((int(B), 3)), np.zeros(int(B))
    for b in range(int(B)):
        offsets[b] = base + rng.normal(0.0, 1.0, 3) * float(sigma)
        sizes[b] = size * np.exp(rng.normal(0.0, 1.0) * float(scale_sigma))
    return tracking_curves(params, curve, offsets=offsets, sizes=sizes)
