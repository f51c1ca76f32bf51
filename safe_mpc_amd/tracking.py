"""The reference curves of the trajectory-tracking task: ``cost.traj`` of the reference's Tracking8* and TrackingMovingCircle*
costs (cost_definition.py:102-288), ``[3, n_steps_tracking + 1 + N]`` end-effector points that ``AbstractController.setTrajectory``
takes -- column ``current_step + i`` is the reference of node i (controller.py:153-156).

* :func:`lemniscate_trajectory`    -- generate_8shape_trajectory (cost_definition.py:170-199)
* :func:`moving_circle_trajectory` -- generate_moving_circle_trajectory (cost_definition.py:264-288)
* :func:`tracking_trajectory`      -- the entry: picks the curve and sets ``params.n_steps`` like the reference's cost classes

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
