"""Shared pieces of the scene-track tests (test_scene_track_host.py, test_scene_track_gpu.py): tracks built from the four scenes of
scene_cases.scene_family as per-instance sequences of scene indices, the column rule restated, and TrackOracleSolver, the CPU double
of a solver that holds a scene track and a scene clock.  Not a test module.

The principle every test rests on: node k of the moving problem is node k of the static problem in the scene of column
col(t + k).  The static problem is pinned to the oracle by test_scene_gpu.py and scene_cases.SceneOracleSolver."""
import numpy as np

import scene_cases as sc
from fake_solver import OracleSolver

PATTERN = np.array([0, 1, 2, 3, 3, 2, 1, 0])      # neighbouring columns differ (but for the two turning points)


def col(c, T):
    """THE column rule of include/smpc.h, restated"""
    return np.clip(np.asarray(c, np.int64), 0, int(T) - 1)


def track_indices(B, T, n_scenes=4):
    """idx [B, T]: instance b's scene in column j -- every instance another rotation of PATTERN (by 3 b: neighbouring instances
    differ in every column); with fewer scenes the indices fold back"""
    j = np.arange(T)[None, :] + 3 * np.arange(B)[:, None]
    idx = PATTERN[j % len(PATTERN)]
    return np.where(idx < n_scenes, idx, 2 * (n_scenes - 1) - idx) if n_scenes < 4 else idx


def clocked(idx, c, n_nodes):
    """the track that, without a clock, is what ``idx`` is at clock c: idx'[b, j] = idx[b, col(c + j)], for j up to the last node
    that reads it (with only T columns and c < 0, idx' would end before idx's last columns and the clamp would repeat an earlier
    one for the nodes behind it)"""
    T = idx.shape[1]
    return idx[:, col(c + np.arange(max(T, n_nodes)), T)]


def node_scenes(idx, t, n_nodes, off=0):
    """[B, n_nodes]: the scene index of node k of every instance at clock t"""
    return idx[:, col(t + off + np.arange(n_nodes), idx.shape[1])]


def per_node(fn, scene_of_node):
    """Compose a node-wise result from static calls: ``fn(scene) -> array [B, n_nodes, ...]`` evaluated once per distinct scene, node
    (b, k) taken from the call in scene ``scene_of_node[b, k]``.  Structured arrays are composed field by field."""
    out = None
    for s in np.unique(scene_of_node):
        r = np.asarray(fn(int(s)))
        if out is None:
            out = np.zeros_like(r)
        m = scene_of_node == s
        if r.dtype.names:
            for f in r.dtype.names:
                out[f][m] = r[f][m]
        else:
            out[m] = r[m]
    return out


class TrackOracleSolver(sc.SceneOracleSolver):
    """SceneOracleSolver with ``set_instance_scene_track`` and ``set_scene_clock``: the per-scene oracle solvers composed PER NODE.
    ``eval_nodes`` and ``check_trajectory`` are node-wise statements, so node k of instance b comes from the solver of the scene in
    column col(t + k) of b's track.  A ``solve`` couples the nodes: the oracle solves in ONE scene, so it is served only where all
    the columns an instance's horizon sees are the same scene (NotImplementedError otherwise).  The clock is a one-element array
    read when a call is made; ``clock_log`` records (call, value) for every solve and check."""

    def __init__(self, problem, net, scene_problems, scene_geoms):
        super().__init__(problem, net, scene_problems, scene_geoms)
        self.track = None              # [B, T] scene indices
        self.clock = None
        self.track_calls, self.clock_calls, self.clock_log = [], [], []

    def set_instance_scene(self, geom=None):
        super().set_instance_scene(geom)
        self.track = None

    def set_instance_scene_track(self, geom=None):
        self.track_calls.append(None if geom is None else np.array(geom, float))
        self.idx = None
        if geom is None:
            self.track = None
            return
        geom = np.ascontiguousarray(geom, np.float64)
        assert geom.ndim == 4 and geom.shape[1] >= 1
        self.track = np.array([[self.keys.index(g.tobytes()) for g in inst] for inst in geom])

    def set_scene_clock(self, clock=None):
        self.clock_calls.append(clock)
        self.clock = clock

    def _t(self, who):
        t = 0 if self.clock is None else int(np.asarray(self.clock).reshape(-1)[0])
        self.clock_log.append((who, t))
        return t

    def _static(self, idx_b, name, *a, **kw):
        """``name`` of SceneOracleSolver with instance b in scene idx_b[b]"""
        keep = self.idx
        self.idx = np.asarray(idx_b)
        try:
            return getattr(sc.SceneOracleSolver, name)(self, *a, **kw)
        finally:
            self.idx = keep

    def solve(self, x0, xg, ug, p, out=None):
        if self.track is None:
            return super().solve(x0, xg, ug, p, out)
        seen = node_scenes(self.track, self._t('solve'), self.N + 1)
        if not (seen == seen[:, :1]).all():
            raise NotImplementedError('TrackOracleSolver.solve: the oracle solves in one scene per instance')
        return self._static(seen[:, 0], 'solve', x0, xg, ug, p, out)

    def eval_nodes(self, xg, ug, p):
        if self.track is None:
            return super().eval_nodes(xg, ug, p)
        B, n = np.asarray(xg).shape[:2]
        seen = node_scenes(self.track, self._t('eval_nodes'), n)
        return per_node(lambda s: self._static(np.full(B, s), 'eval_nodes', xg, ug, p), seen)

    def check_trajectory(self, x, **kw):
        if self.track is None:
            return super().check_trajectory(x, **kw)
        x = np.asarray(x)
        B, n = x.shape[:2]
        seen = node_scenes(self.track, self._t('check_trajectory'), n)
        want_nn = kw.get('want_nn', False)
        # node by node (a trajectory's verdict is the AND over its nodes; the safe-set verdict is per node already)
        ok, nn = np.ones(B, bool), None
        for k in range(n):
            r = self._static(seen[:, k], 'check_trajectory', x[:, k:k + 1], **kw)
            if want_nn:
                ok &= np.asarray(r[0]).astype(bool)
                nn = np.asarray(r[1]) if nn is None else np.concatenate([nn, np.asarray(r[1])], axis=1)
            else:
                ok &= np.asarray(r).astype(bool)
        return (ok, nn) if want_nn else ok


def oracle_factories(par, N, scene_pars, geoms, log=None, solver_cls=TrackOracleSolver):
    """make_controller / make_backup of run_mpc around ``solver_cls`` (one oracle per scene, built from moved parameters); ``log``
    receives the solvers by controller name"""
    from safe_mpc_amd import controller as C

    def build(cls, name, cost, horizon, batch):
        ctrl = cls.__new__(cls)
        prob = C.OcpProblem(par, name, cost, N=horizon)
        net = C.SafeSetNet.from_params(par, prob.x_min, prob.x_max)
        prob.set_normalisation(net.mean, net.std)
        subs = []
        for sp in scene_pars:
            pr = C.OcpProblem(sp, name, cost, N=horizon)
            pr.set_normalisation(net.mean, net.std)
            subs.append(pr)
        solver = solver_cls(prob, net, subs, geoms)
        if log is not None:
            log[name] = solver
        C.AbstractController.__init__(ctrl, par, batch, cost, horizon, solver=solver, net=net)
        return ctrl
    return (lambda name, batch: build(C.CONTROLLERS[name], C.CONTROLLERS[name].cont_name, 'ext', N, batch),
            lambda batch: build(C.SafeBackupController, 'backup', 'zero', par.back_hor, batch))
