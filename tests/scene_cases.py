"""Shared pieces of the per-instance-scene tests (test_scene_host.py, test_scene_gpu.py): the scenes the tests use, problems built
from MOVED PARAMETERS (what the oracle understands: one descriptor per scene), and SceneOracleSolver, the CPU double of a solver that
holds a scene per instance.  Not a test module."""
import functools

import numpy as np

from conftest import make_problem, make_problem_fr7
from fake_solver import OracleSolver

# the three gate capsules of config.yaml (fixed1..3) move together by one of these; the fr7 sphere by the first three
SHIFTS = [(0.0, 0.0, 0.0), (0.0, 0.06, 0.0), (-0.05, 0.0, 0.05), (0.0, 0.15, 0.0)]
Z1_OBSTACLES = ('fixed1', 'fixed2', 'fixed3')
FR7_OBSTACLES = ('ball',)


def move_obstacles(par, shift, names):
    """translate the named world-fixed capsules / spheres of a Parameters object in place (the collision pairs hold the same dicts)"""
    d = np.asarray(shift, float)
    for cap in par.obst_capsules:
        if cap['name'] in names:
            cap['end_points'] = np.asarray(cap['end_points'], float) + d
            cap['end_points_fk'] = cap['end_points']
    for obs in par.obstacles:
        if obs['name'] in names and obs['type'] == 'sphere-obs':
            obs['position'] = np.asarray(obs['position'], float) + d


def moved_problem(system, controller, N, shift, cost='ext', **over):
    """(par, prob, net) of a problem whose obstacles were moved BEFORE the rows were built"""
    from safe_mpc_amd.problem import OcpProblem
    if system == 'z1':
        par, _, net = make_problem(controller, cost, N=N, **over)
        names = Z1_OBSTACLES
    else:
        par, _, net = make_problem_fr7(controller, cost, N=N)
        names = FR7_OBSTACLES
    move_obstacles(par, shift, names)
    prob = OcpProblem(par, controller, cost, N=N)
    prob.set_normalisation(net.mean, net.std)
    return par, prob, net


@functools.lru_cache(maxsize=None)
def scene_family(system, controller, N, n_scenes, cost='ext'):
    """base (par, prob, net), the moved-parameter problems of the first n_scenes SHIFTS and their geometry [n_scenes, n_rows, 8]"""
    from safe_mpc_amd.problem import scenes_from_problems
    base = moved_problem(system, controller, N, SHIFTS[0], cost)
    moved = [moved_problem(system, controller, N, s, cost) for s in SHIFTS[:n_scenes]]
    geom = scenes_from_problems(base[1], [m[1] for m in moved])
    return base, moved, geom


class SceneOracleSolver(OracleSolver):
    """OracleSolver with ``set_instance_scene``: one OracleSolver per distinct scene (each on the problem built from that scene's
    moved parameters), and every batched call split by scene, sent to the scene's solver and put back in instance order.  Without a
    scene it is the OracleSolver of the base problem."""

    def __init__(self, problem, net, scene_problems, scene_geoms):
        super().__init__(problem, net)
        self.subs = [OracleSolver(pr, net) for pr in scene_problems]
        self.keys = [np.ascontiguousarray(g, np.float64).tobytes() for g in scene_geoms]
        self.idx = None
        self.scene_calls = []

    def set_instance_scene(self, geom=None):
        self.scene_calls.append(None if geom is None else np.array(geom, float))
        if geom is None:
            self.idx = None
            return
        geom = np.ascontiguousarray(geom, np.float64)
        self.idx = np.array([self.keys.index(g.tobytes()) for g in geom])      # (ValueError: a scene no oracle was built for)

    def set_horizon(self, N):
        super().set_horizon(N)
        for s in self.subs:
            s.set_horizon(N)

    def _split(self, name, batched, rest=(), kw=None):
        """call ``name`` of every scene's solver on its members' rows of the ``batched`` arrays; results (array or tuple of arrays
        with the batch in front) are put back in instance order"""
        kw = kw or {}
        B = len(batched[0])
        if self.idx is None:
            return getattr(OracleSolver, name)(self, *batched, *rest, **kw)
        assert len(self.idx) == B, f'{name}: batch {B}, scene set for {len(self.idx)} instances'
        out = None
        for s in np.unique(self.idx):
            m = np.where(self.idx == s)[0]
            r = getattr(self.subs[s], name)(*[np.ascontiguousarray(a[m]) for a in batched], *rest, **kw)
            tup = r if isinstance(r, tuple) else (r,)
            if out is None:
                out = [np.zeros((B,) + np.asarray(t).shape[1:], np.asarray(t).dtype) for t in tup]
            for o, t in zip(out, tup):
                o[m] = np.asarray(t)
        return tuple(out) if isinstance(r, tuple) else out[0]

    def solve(self, x0, xg, ug, p, out=None):
        x, u, st, it = self._split('solve', [np.asarray(x0), np.asarray(xg), np.asarray(ug), np.asarray(p)])
        if self.idx is not None and self.scripted_status:
            st = np.asarray(self.scripted_status.pop(0), np.int32)
        return x, u, st, it

    def eval_nodes(self, xg, ug, p):
        return self._split('eval_nodes', [np.asarray(xg), np.asarray(ug), np.asarray(p)])

    def check_trajectory(self, x, x_min=None, x_max=None, tol_x=None, row_lb=None, row_ub=None, alpha=None, tol_safe=None,
                         want_nn=False):
        return self._split('check_trajectory', [np.asarray(x)], kw=dict(x_min=x_min, x_max=x_max, tol_x=tol_x, row_lb=row_lb,
                                                                         row_ub=row_ub, alpha=alpha, tol_safe=tol_safe, want_nn=want_nn))


def by_scene(fn, idx, B):
    """fn(scene, members) -> array (or tuple) with the members in front, assembled over the scenes in instance order"""
    out = None
    for s in np.unique(idx):
        m = np.where(idx == s)[0]
        r = fn(int(s), m)
        tup = r if isinstance(r, tuple) else (r,)
        if out is None:
            out = [np.zeros((B,) + np.asarray(t).shape[1:], np.asarray(t).dtype) for t in tup]
        for o, t in zip(out, tup):
            o[m] = np.asarray(t)
    return tuple(out) if isinstance(r, tuple) else out[0]
