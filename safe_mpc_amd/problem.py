"""ctypes mirror of include/smpc.h and the builder that turns ``Parameters`` + URDF into a ``smpc_problem_desc``.

This is the host-side restatement of the OCP *formulation* layer of the reference (L2 in SURVEY section 1):
``AdamModel.__init__`` / ``generate_NLconstraints_list`` (env_model.py:19-165, 246-319) and
``AbstractController.__init__`` + the ``additionalSetting`` of each policy (controller.py:13-125, 295-306, 332-357,
411-442, 514-515, 663-689, 692-712).  Instead of CasADi expressions it emits plain data: a joint table, robot-attached
points, collision rows with their bounds, and scalar options.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .urdf import SerialChain

ABI_VERSION = 5
MAX_NQ, MAX_NX, MAX_POINTS, MAX_ROWS, MAX_LAYERS, MAX_N, NP = 7, 14, 12, 12, 6, 63, 5
SCENE_ROW = 8         # SMPC_SCENE_ROW: doubles per (instance, row) of a scene -- C[3], D[3], offset, 0
INF = 1.0e5

ROW_SEG_FIXEDSEG, ROW_SEG_SEG, ROW_SEG_POINT, ROW_POINT_POINT, ROW_COORD = 0, 1, 2, 3, 4
COST_ZERO, COST_REACH = 0, 1
HESS_GAUSS_NEWTON, HESS_EXACT = 0, 1
NN_NONE, NN_TERMINAL, NN_ALL = 0, 1, 2

STATUS_NAMES = {0: 'SUCCESS', 1: 'NAN', 2: 'MAXITER', 3: 'MINSTEP', 4: 'QP_FAILURE'}


class Joint(C.Structure):
    _fields_ = [('R0', C.c_double * 9), ('p0', C.c_double * 3), ('axis', C.c_double * 3), ('mass', C.c_double),
                ('com', C.c_double * 3), ('inertia', C.c_double * 6), ('q_min', C.c_double), ('q_max', C.c_double),
                ('v_max', C.c_double), ('tau_max', C.c_double)]


class Point(C.Structure):
    _fields_ = [('link', C.c_int32), ('reserved', C.c_int32), ('local', C.c_double * 3)]


class Row(C.Structure):
    _fields_ = [('kind', C.c_int32), ('pa', C.c_int32), ('pb', C.c_int32), ('pc', C.c_int32), ('pd', C.c_int32),
                ('axis', C.c_int32), ('C', C.c_double * 3), ('D', C.c_double * 3), ('len2', C.c_double),
                ('offset', C.c_double), ('lb', C.c_double), ('ub', C.c_double)]


class ProblemDesc(C.Structure):
    _fields_ = [('abi_version', C.c_int32), ('nq', C.c_int32), ('N', C.c_int32), ('n_points', C.c_int32),
                ('n_rows', C.c_int32), ('ee_point', C.c_int32), ('cost_kind', C.c_int32), ('hessian', C.c_int32),
                ('nn_mode', C.c_int32), ('nn_dof', C.c_int32), ('qp_max_iter', C.c_int32), ('rows_at_node0', C.c_int32),
                ('qp_stall_iters', C.c_int32), ('reserved_i0', C.c_int32),
                ('dt', C.c_double), ('Q', C.c_double), ('R', C.c_double), ('cost_scale_stage', C.c_double),
                ('cost_scale_term', C.c_double), ('lm_stage', C.c_double), ('lm_term', C.c_double),
                ('nn_eps', C.c_double), ('nn_soft_e', C.c_double), ('nn_soft_run', C.c_double),
                ('qp_tol', C.c_double), ('qp_tol_res', C.c_double), ('qp_mu0', C.c_double), ('gravity', C.c_double * 3),
                ('nn_mean', C.c_double * MAX_NQ), ('nn_std', C.c_double * MAX_NQ),
                ('x_lo', C.c_double * MAX_NX), ('x_hi', C.c_double * MAX_NX),
                ('x_lo_e', C.c_double * MAX_NX), ('x_hi_e', C.c_double * MAX_NX),
                ('joints', Joint * MAX_NQ), ('points', Point * MAX_POINTS), ('rows', Row * MAX_ROWS)]


class NodeEval(C.Structure):
    _fields_ = [('tau', C.c_double * MAX_NQ), ('M', C.c_double * (MAX_NQ * MAX_NQ)),
                ('dtau_dq', C.c_double * (MAX_NQ * MAX_NQ)), ('dtau_dv', C.c_double * (MAX_NQ * MAX_NQ)),
                ('ee', C.c_double * 3), ('cost_grad_q', C.c_double * MAX_NQ),
                ('cost_hess_qq', C.c_double * (MAX_NQ * MAX_NQ)), ('row_val', C.c_double * MAX_ROWS),
                ('row_grad', C.c_double * (MAX_ROWS * MAX_NQ)), ('nn_val', C.c_double),
                ('nn_grad', C.c_double * MAX_NX)]


NODE_EVAL_DTYPE = np.dtype([('tau', 'f8', MAX_NQ), ('M', 'f8', MAX_NQ * MAX_NQ), ('dtau_dq', 'f8', MAX_NQ * MAX_NQ),
                            ('dtau_dv', 'f8', MAX_NQ * MAX_NQ), ('ee', 'f8', 3), ('cost_grad_q', 'f8', MAX_NQ),
                            ('cost_hess_qq', 'f8', MAX_NQ * MAX_NQ), ('row_val', 'f8', MAX_ROWS),
                            ('row_grad', 'f8', MAX_ROWS * MAX_NQ), ('nn_val', 'f8'), ('nn_grad', 'f8', MAX_NX)])
assert NODE_EVAL_DTYPE.itemsize == C.sizeof(NodeEval)

JOINT_DTYPE = np.dtype([('R0', 'f8', 9), ('p0', 'f8', 3), ('axis', 'f8', 3), ('mass', 'f8'), ('com', 'f8', 3),
                        ('inertia', 'f8', 6), ('q_min', 'f8'), ('q_max', 'f8'), ('v_max', 'f8'), ('tau_max', 'f8')])
assert JOINT_DTYPE.itemsize == C.sizeof(Joint)


def _rot(axis, th):
    c, s = np.cos(th), np.sin(th)
    if axis == 0:
        return np.array([[1, 0, 0], [0, c, -s], [0, s, c]])
    if axis == 1:
        return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])


# controller name -> how the safe-set row enters
CONTROLLER_KINDS = {
    #                  nn_mode      soft_e     soft_run  term_zero_vel  cost      lm
    'naive':           (NN_NONE,     None,      None,     False),
    'zerovel':         (NN_NONE,     None,      None,     True),
    'st':              (NN_TERMINAL, 'ws_r',    None,     False),
    'stwa':            (NN_TERMINAL, 'ws_r',    None,     False),
    'htwa':            (NN_TERMINAL, None,      None,     False),
    'receding':        (NN_ALL,      'ws_t',    None,     False),
    'real_receding':   (NN_TERMINAL, None,      None,     False),
    'constraint_everywhere': (NN_ALL, None,     None,     False),
    'parallel':        (NN_ALL,      None,      None,     False),     # both rows hard (controller.py:573-576)
    'backup':          (NN_NONE,     None,      None,     True),
}


class OcpProblem:
    """Everything the engine needs about one OCP family; ``desc`` is the C struct handed to ``smpc_create``."""

    def __init__(self, params, controller='naive', cost='ext', N=None, chain=None, rows_at_node0=None):
        if controller not in CONTROLLER_KINDS:
            raise ValueError(f'Controller {controller} not available')
        self.params = params
        self.controller = controller
        nq = params.nq
        if nq > MAX_NQ:
            raise ValueError(f'nq={nq} exceeds SMPC_MAX_NQ={MAX_NQ}')
        self.chain = chain or SerialChain(params.robot_descr, nq)
        self.nq, self.nx, self.nu = nq, 2 * nq, nq
        self.N = int(N if N is not None else (params.back_hor if controller == 'backup' else params.N))
        if not (1 <= self.N <= MAX_N):
            raise ValueError(f'horizon {self.N} outside 1..{MAX_N}')
        nn_mode, soft_e, soft_run, zero_vel = CONTROLLER_KINDS[controller]
        if nn_mode != NN_NONE and not params.use_net:
            raise NotImplementedError('AnalyticSafeSet (use_net: false) is out of scope of this engine')

        d = ProblemDesc()
        d.abi_version, d.nq, d.N = ABI_VERSION, nq, self.N
        d.dt = params.dt
        d.gravity[:] = [0.0, 0.0, -9.80665]

        # joints, limits (env_model.py:107-121)
        jl = np.array([[j.q_min, j.q_max, j.v_max, j.tau_max] for j in self.chain.joints])
        for i, j in enumerate(self.chain.joints):
            J = d.joints[i]
            J.R0[:] = j.R0.reshape(-1)
            J.p0[:] = j.p0
            J.axis[:] = j.axis
            J.mass = j.mass
            J.com[:] = j.com
            I = j.inertia
            J.inertia[:] = [I[0, 0], I[0, 1], I[0, 2], I[1, 1], I[1, 2], I[2, 2]]
            J.q_min, J.q_max, J.v_max, J.tau_max = jl[i]
        self.tau_min, self.tau_max = -jl[:, 3].copy(), jl[:, 3].copy()
        x_min_nom = np.hstack([jl[:, 0], -jl[:, 2]])
        x_max_nom = np.hstack([jl[:, 1], jl[:, 2]])
        self.bounds_diff = np.abs(x_max_nom - x_min_nom)
        mg = params.q_margin / 100.0
        # model bounds are widened by the margin, the OCP shrinks them back (env_model.py:118-121, controller.py:49-55)
        self.x_min = x_min_nom - self.bounds_diff * mg
        self.x_max = x_max_nom + self.bounds_diff * mg
        lo = self.x_min + mg * self.bounds_diff
        hi = self.x_max - mg * self.bounds_diff
        lo_e, hi_e = lo.copy(), hi.copy()
        if controller == 'zerovel':                           # controller.py:300-306
            lo_e[nq:], hi_e[nq:] = 0.0, 0.0
        if controller == 'backup':                            # controller.py:701-707 (model bounds, zero velocity)
            lo_e = np.hstack([self.x_min[:nq], np.zeros(nq)])
            hi_e = np.hstack([self.x_max[:nq], np.zeros(nq)])
        d.x_lo[:2 * nq], d.x_hi[:2 * nq] = lo, hi
        d.x_lo_e[:2 * nq], d.x_hi_e[:2 * nq] = lo_e, hi_e
        self.lbx, self.ubx, self.lbx_e, self.ubx_e = lo, hi, lo_e, hi_e

        # robot-attached points
        self._points = []
        fr_idx, fr_R, fr_p = self.chain.frame(params.frame_name)
        d.ee_point = self._add_point(fr_idx, fr_p + fr_R @ params.ee_pos)      # env_model.py:92-95
        self.ee_ref = np.array(params.ee_ref, float)

        # collision rows (env_model.py:263-316)
        self.rows = []
        self.row_names = []
        self.row_obstacle = []         # name of the row's world-fixed element (what a scene moves); None for robot-robot rows
        self.row_check = []            # (lo, hi) used by checkCollision (env_model.py:236-243)
        m2 = 2.0 * params.collision_margin
        tol = params.tol_obs
        for i, pair in enumerate(params.collisions_pairs):
            e0, e1 = pair['elements']
            r = Row()
            if pair['type'] == 'capsule-capsule':
                a, b = self._capsule_points(e0)
                r.pa, r.pb = a, b
                if e1['type'] == 'fixed_capsule':
                    r.kind = ROW_SEG_FIXEDSEG
                    r.C[:], r.D[:] = e1['end_points'][0], e1['end_points'][1]
                else:
                    r.kind = ROW_SEG_SEG
                    r.pc, r.pd = self._capsule_points(e1)
                r.lb, r.ub = (e0['radius'] + e1['radius'] + m2) ** 2, 1e6
                self._push_row(r, f"{e0['name']}-{e1['name']}", (e0['radius'] + e1['radius']) ** 2 - tol, 1e6 + tol,
                               e1['name'] if r.kind == ROW_SEG_FIXEDSEG else None)
            elif pair['type'] == 'capsule-sphere':
                r.kind = ROW_SEG_POINT
                r.pa, r.pb = self._capsule_points(e0)
                r.C[:] = e1['position']
                r.len2 = e0['length'] ** 2
                r.lb, r.ub = (e1['radius'] + e0['radius'] + m2) ** 2, 1e6
                self._push_row(r, f"{e0['name']}-{e1['name']}", (e1['radius'] + e0['radius']) ** 2 - tol, 1e6 + tol, e1['name'])
            elif pair['type'] == 'capsule-plane':
                for pt in self._capsule_points(e0):
                    r = Row()
                    r.kind, r.pa, r.axis, r.offset = ROW_COORD, pt, int(e1['perpendicular_axis']), 0.0
                    r.lb = e1['bounds'][0] + e0['radius'] + m2
                    r.ub = e1['bounds'][1] - e0['radius'] - m2
                    self._push_row(r, f"{e0['name']}-{e1['name']}", e1['bounds'][0] + e0['radius'] - tol,
                                   e1['bounds'][1] - e0['radius'] + tol, e1['name'])
            elif pair['type'] == 'sphere-sphere':
                r.kind, r.pa = ROW_POINT_POINT, d.ee_point      # the reference uses t_glob here (env_model.py:300)
                r.C[:] = e1['position']
                r.lb, r.ub = (e0['radius'] + e1['radius'] + m2) ** 2, 1e6
                self._push_row(r, f"{e0['name']}-{e1['name']}", (e0['radius'] + e1['radius']) ** 2 - tol, 1e6 + tol, e1['name'])
            elif pair['type'] == 'sphere-plane':
                li, lR, lp = self.chain.frame(e0['link_name'])
                r.kind = ROW_COORD
                r.pa = self._add_point(li, lp + lR @ np.array(e0['spatial_offset'], float))
                r.axis = int(e1['perpendicular_axis'])
                r.offset = float(e1['bounds'][int(e1['real_bound'])])           # utils.py:123-124
                r.lb = e1['bounds'][0] + e0['radius'] + m2
                r.ub = e1['bounds'][1] - e0['radius'] - m2
                self._push_row(r, f"{e0['name']}-{e1['name']}", e1['bounds'][0] + e0['radius'] - tol,
                               e1['bounds'][1] - e0['radius'] + tol, e1['name'])
            else:
                raise ValueError(f"unsupported collision pair type {pair['type']}")
        if len(self.rows) > MAX_ROWS:
            raise ValueError(f'{len(self.rows)} collision rows exceed SMPC_MAX_ROWS={MAX_ROWS}')
        if len(self._points) > MAX_POINTS:
            raise ValueError(f'{len(self._points)} robot points exceed SMPC_MAX_POINTS={MAX_POINTS}')
        d.n_rows, d.n_points = len(self.rows), len(self._points)
        for i, r in enumerate(self.rows):
            d.rows[i] = r
        for i, (li, loc) in enumerate(self._points):
            d.points[i].link = li
            d.points[i].local[:] = loc
        self.row_lb = np.array([r.lb for r in self.rows])
        self.row_ub = np.array([r.ub for r in self.rows])
        self.row_check = np.array(self.row_check).reshape(-1, 2)

        # cost (cost_definition.py:34-100)
        cost = 'zero' if controller == 'backup' else cost
        self.cost = cost
        d.cost_kind = COST_ZERO if cost == 'zero' else COST_REACH
        d.hessian = HESS_EXACT if cost == 'ext' else HESS_GAUSS_NEWTON
        d.Q, d.R = params.Q_weight, params.R_weight
        # acados: stage costs x dt, terminal x 1 [EXT-UNVERIFIED]; NONLINEAR_LS is 1/2 |y|^2_W (cost_definition.py:61-81:
        # W = diag(Q, R) -> gradient Q J^T delta, R u; Gauss-Newton Hessian Q J^T J, R I), EXTERNAL is the expression itself
        # (cost_definition.py:91-96: Q |delta|^2 + R |u|^2 -> 2Q ..., 2R ...).  The engine differentiates Q|delta|^2 + R|u|^2.
        half = 0.5 if cost == 'nls' else 1.0
        d.cost_scale_stage, d.cost_scale_term = half * params.dt, half
        # controller.py:711 sets LM = 0 for the backup OCP, whose cost is zero as well: the QP Hessian vanishes and the
        # reference relies on HPIPM's internal primal regularisation [EXT-UNVERIFIED].  The engine states it: a 1e-4
        # diagonal makes the QP strictly convex (minimum-norm feasible correction of the guess) and well enough
        # conditioned that its solution is resolved at the IPM's 1e-8 exit tolerance.
        lm = 1e-4 / params.dt if controller == 'backup' else params.levenberg_marquardt
        d.lm_stage, d.lm_term = lm * params.dt, (1e-4 if controller == 'backup' else lm)

        # safe set (safe_set.py:72-104)
        d.nn_mode, d.nn_dof, d.nn_eps = nn_mode, params.n_dof_safe_set, params.eps
        d.nn_soft_e = getattr(params, soft_e) if soft_e else -1.0
        d.nn_soft_run = getattr(params, soft_run) if soft_run else -1.0
        for i in range(MAX_NQ):
            d.nn_mean[i], d.nn_std[i] = 0.0, 1.0

        # collision rows at node 0: kept by the reference unless the run is noisy (controller.py:68-79)
        d.rows_at_node0 = int(not float(getattr(params, 'noise', 0.0) or 0.0) > 0.0) if rows_at_node0 is None \
            else int(bool(rows_at_node0))
        d.qp_max_iter = params.qp_max_iter
        d.qp_tol, d.qp_mu0 = float(getattr(params, 'qp_tol', 1e-8)), 1.0
        # stall exit of the IPM (include/smpc.h): on for RealReceding, whose tubes make ~1 % of its QPs infeasible
        # the stall exit (include/smpc.h) is on where infeasible QPs are part of normal operation: RealReceding's tubes, and the backup
        # OCP (terminal zero velocity from the viable state of an aborting instance: in RealReceding's loop 27 of 29 such solves
        # are infeasible and used to run 34 iterations on average, 52 at worst, until the step length underflowed; feasible ones take 5)
        # ... and ParallelController's low-n candidates, whose hard row at a single early node is often infeasible: without the exit each
        # would run 40-90 iterations until its step underflows.  A QP given up on yields candidate result 0 -- which can drop a slow but
        # feasible candidate that acados would have solved, the trade RealReceding already makes
        d.qp_stall_iters = int(getattr(params, 'qp_stall_iters', 24 if controller in ('real_receding', 'parallel', 'backup') else 0))
        d.qp_tol_res = float(getattr(params, 'qp_tol_res', 0.0))     # 0: same as qp_tol
        self.desc = d

    # -- helpers ----------------------------------------------------------------------------------------------------
    def set_normalisation(self, mean, std):
        n = self.params.n_dof_safe_set
        self.desc.nn_mean[:n] = np.asarray(mean, float).reshape(-1)[:n]
        self.desc.nn_std[:n] = np.asarray(std, float).reshape(-1)[:n]

    def _add_point(self, link, local):
        local = np.asarray(local, float)
        for i, (li, loc) in enumerate(self._points):
            if li == link and np.array_equal(loc, local):
                return i
        self._points.append((int(link), local))
        return len(self._points) - 1

    def _capsule_points(self, cap):
        """Two end points of a moving capsule in the frame of the actuated link that carries it
        (env_model.py:131-150: FK_link . Trans(spatial_offset) . Rx Ry Rz . e_i)."""
        cache = self.__dict__.setdefault('_cap_pts', {})
        if cap['name'] not in cache:
            li, lR, lp = self.chain.frame(cap['link_name'])
            R = np.eye(3)
            if cap.get('rotation_offset') is not None:
                th = cap['rotation_offset']
                R = _rot(0, th[0]) @ _rot(1, th[1]) @ _rot(2, th[2])
            off = np.zeros(3) if cap.get('spatial_offset') is None else np.array(cap['spatial_offset'], float)
            pts = []
            for e in cap['end_points']:
                pts.append(self._add_point(li, lp + lR @ (off + R @ np.asarray(e[:3], float))))
            cache[cap['name']] = tuple(pts)
        return cache[cap['name']]

    def _push_row(self, r, name, chk_lo, chk_hi, obstacle=None):
        self.rows.append(r)
        self.row_names.append(name)
        self.row_obstacle.append(obstacle)
        self.row_check.append((chk_lo, chk_hi))

    # -- per-instance scenes (smpc_set_instance_scene) ---------------------------------------------------------------------------
    def row_geometry(self):
        """[n_rows, SCENE_ROW]: where every row's world-fixed element sits -- C[3], D[3], offset, 0 -- as the descriptor has it.
        The record of one (instance, row) of a scene; a row reads C and D (fixed capsule), C (sphere centre, fixed point) or
        offset (plane) by its kind and nothing of a robot-robot row."""
        g = np.zeros((len(self.rows), SCENE_ROW))
        for i, r in enumerate(self.rows):
            g[i, 0:3], g[i, 3:6], g[i, 6] = r.C[:], r.D[:], r.offset
        return g

    def scene(self, moves):
        """The geometry [n_rows, SCENE_ROW] of this problem with some obstacles translated: ``moves = {obstacle name: (dx, dy, dz)}``,
        names as in ``row_obstacle``.  Capsules and spheres translate; a plane's ``offset`` takes the component of the move along
        its perpendicular axis.  Bounds, radii and kinds are not part of a scene: they stay the descriptor's."""
        known = {n for n in self.row_obstacle if n is not None}
        unknown = sorted(set(moves) - known)
        if unknown:
            raise ValueError(f'scene: unknown obstacle name(s) {unknown}; this problem has {sorted(known)}')
        g = self.row_geometry()
        for i, (r, name) in enumerate(zip(self.rows, self.row_obstacle)):
            if name not in moves:
                continue
            d = np.asarray(moves[name], float).reshape(3)
            if r.kind == ROW_COORD:
                g[i, 6] = g[i, 6] + d[r.axis]
            else:
                g[i, 0:3] = g[i, 0:3] + d
                if r.kind == ROW_SEG_FIXEDSEG:
                    g[i, 3:6] = g[i, 3:6] + d
        return g

    def scene_track(self, moves):
        """[T, n_rows, SCENE_ROW]: a scene per time column (smpc_set_instance_scene_track) -- ``moves[j]`` is the ``moves`` of
        :meth:`scene` for column j, so ``scene_track([{}])`` is ``row_geometry()`` with a leading axis."""
        moves = list(moves)
        if not moves:
            raise ValueError('scene_track: a track has at least one time column')
        return np.stack([self.scene(m) for m in moves])

    def context_default(self, select):
        """[n_ctx]: the context of the shared scene -- :func:`scene_context` of ``row_geometry()``"""
        return scene_context(self.row_geometry()[None], select)[0]

    # per-instance perturbed joint tables for the plant (utils.py:126-171 semantics on the lumped inertias is NOT what
    # the reference does -- it perturbs each URDF link before lumping; see noise.py)
    def joint_table(self):
        out = np.zeros(self.nq, JOINT_DTYPE)
        for i in range(self.nq):
            J = self.desc.joints[i]
            for f in ('R0', 'p0', 'axis', 'com', 'inertia'):
                out[i][f] = np.array(getattr(J, f))
            for f in ('mass', 'q_min', 'q_max', 'v_max', 'tau_max'):
                out[i][f] = getattr(J, f)
        return out


def scene_context(geom, select):
    """[B, n_ctx] from scenes ``geom [B, n_rows, SCENE_ROW]`` (a numpy array, or a ROCm tensor that gives a tensor): the numbers a safe-set network with a context is given about its
    instance's scene -- entry ``slot`` of row ``row``'s record for every ``(row, slot)`` of ``select``, in
    that order (``SafeSetNet.ctx_select``).  A track ``[B, T, n_rows, SCENE_ROW]`` gives ``[B, T, n_ctx]``, the context of every
    (instance, time column) (smpc_set_instance_context_track)."""
    on_device = type(geom).__module__.startswith('torch')      # (a ROCm tensor stays one: the device loop holds its scenes there)
    if not on_device:
        geom = np.asarray(geom, float)
    if geom.ndim == 4 and geom.shape[3] == SCENE_ROW:
        B, T = int(geom.shape[0]), int(geom.shape[1])
        flat = scene_context(geom.reshape((B * T,) + tuple(geom.shape[2:])), select)
        return flat.reshape((B, T, flat.shape[1]))
    if geom.ndim != 3 or geom.shape[2] != SCENE_ROW:
        raise ValueError(f'scene_context: expected [B, n_rows, {SCENE_ROW}], got {tuple(geom.shape)}')
    sel = [(int(r), int(c)) for r, c in select]
    for r, c in sel:
        if not (0 <= r < geom.shape[1] and 0 <= c < SCENE_ROW):
            raise ValueError(f'scene_context: (row {r}, slot {c}) outside a scene of {geom.shape[1]} rows x {SCENE_ROW} slots')
    if on_device:
        import torch
        return torch.stack([geom[:, r, c] for r, c in sel], dim=1).contiguous() if sel else geom.new_zeros((geom.shape[0], 0))
    return np.ascontiguousarray(np.stack([geom[:, r, c] for r, c in sel], axis=1)) if sel else np.zeros((geom.shape[0], 0))


def _row_signature(prob):
    """everything of the collision rows that a scene does NOT carry: what two problems must share to be scenes of one descriptor"""
    return ([(r.kind, r.pa, r.pb, r.pc, r.pd, r.axis, r.len2, r.lb, r.ub) for r in prob.rows],
            [(int(li), tuple(np.asarray(loc, float))) for li, loc in prob._points], np.asarray(prob.row_check, float).tolist())


def scenes_from_problems(base, problems):
    """[len(problems), n_rows, SCENE_ROW]: the geometry of problems built from moved parameters, as scenes of ``base``.  Every
    problem must agree with ``base`` in what a scene does not carry -- row kinds, robot points, len2, lb / ub and the check bounds
    -- so that each scene is a descriptor the oracle understands (``problems[i]`` itself); ValueError otherwise."""
    ref = _row_signature(base)
    out = []
    for i, pr in enumerate(problems):
        sig = _row_signature(pr)
        for what, a, b in zip(('rows (kind, points, len2, lb, ub)', 'robot points', 'check bounds'), ref, sig):
            if a != b:
                raise ValueError(f'scenes_from_problems: problem {i} differs from the base in its {what}: only the obstacles\' '
                                 f'positions may differ between scenes')
        out.append(pr.row_geometry())
    return np.array(out).reshape(len(out), len(base.rows), SCENE_ROW)


def jittered_scenes(prob, B, sigma, seed=0):
    """[B, n_rows, SCENE_ROW]: B random scenes of ``prob`` -- every obstacle translated by its own N(0, sigma^2) draw per axis,
    one draw per (scene, obstacle) shared by all the rows that obstacle appears in."""
    rng = np.random.default_rng(seed)
    names = sorted({n for n in prob.row_obstacle if n is not None})
    out = np.empty((B, len(prob.rows), SCENE_ROW))
    for b in range(B):
        d = rng.normal(0.0, float(sigma), (len(names), 3))
        out[b] = prob.scene({n: d[i] for i, n in enumerate(names)})
    return out


def moving_scenes(prob, B, T, sigma_v, seed=0, sigma=0.0):
    """[B, T, n_rows, SCENE_ROW]: B constant-velocity scene tracks of ``prob`` over T time columns, one column per time step ``prob.desc.dt``.
    Every world-fixed obstacle of instance b moves by ``v * dt`` per column, ``v ~ N(0, sigma_v^2)`` per axis, one draw per
    (instance, obstacle) shared by all the rows that obstacle appears in (plane rows take the component along their axis, as
    :meth:`OcpProblem.scene` does).  Column 0 is ``jittered_scenes(prob, B, sigma, seed)``: the problem's own geometry with the
    default ``sigma = 0``."""
    B, T = int(B), int(T)
    if T < 1:
        raise ValueError('moving_scenes: a track has at least one time column')
    names = sorted({n for n in prob.row_obstacle if n is not None})
    rng0, rngv = np.random.default_rng(seed), np.random.default_rng([int(seed), 1])
    # the draws in the order of jittered_scenes: instance by instance, one [obstacle, axis] block each
    d0 = np.stack([rng0.normal(0.0, float(sigma), (len(names), 3)) for _ in range(B)]).reshape(B, len(names), 3)
    v = np.stack([rngv.normal(0.0, float(sigma_v), (len(names), 3)) for _ in range(B)]).reshape(B, len(names), 3)
    move = d0[:, None] + v[:, None] * (float(prob.desc.dt) * np.arange(T))[None, :, None, None]      # [B, T, obstacle, axis]
    return _moved_tracks(prob, names, move)


def _moved_tracks(prob, names, move):
    """[B, T, n_rows, SCENE_ROW] from ``move [B, T, obstacle, axis]``, the translation of every obstacle of ``names`` in every
    (instance, column): OcpProblem.scene, for all of them at once"""
    B, T = move.shape[:2]
    out = np.broadcast_to(prob.row_geometry(), (B, T, len(prob.rows), SCENE_ROW)).copy()
    for i, (r, name) in enumerate(zip(prob.rows, prob.row_obstacle)):
        if name is None:
            continue
        d = move[:, :, names.index(name)]
        if r.kind == ROW_COORD:
            out[:, :, i, 6] += d[:, :, r.axis]
        else:
            out[:, :, i, 0:3] += d
            if r.kind == ROW_SEG_FIXEDSEG:
                out[:, :, i, 3:6] += d
    return out


def turning_scenes(prob, B, T, sigma_v, sigma_a, seed=0, sigma=0.0):
    """[B, T, n_rows, SCENE_ROW]: :func:`moving_scenes` with obstacles that change course -- the velocity random-walks,
    ``p_{j+1} = p_j + v_j dt``, ``v_{j+1} = v_j + a_j dt``, ``a_j ~ N(0, sigma_a^2)`` per obstacle and axis, one draw per (instance,
    obstacle, column) shared by all the rows the obstacle appears in (plane rows take their axis).  Column 0 and ``v_0`` are the
    draws of ``moving_scenes(prob, B, T, sigma_v, seed, sigma)``, so ``sigma_a = 0`` is that constant-velocity track (up to the
    rounding of a running sum), and the tracks are reproducible per seed.  What a constant-velocity forecast gets wrong on these
    tracks is the obstacle's turning."""
    B, T = int(B), int(T)
    if T < 1:
        raise ValueError('turning_scenes: a track has at least one time column')
    names = sorted({n for n in prob.row_obstacle if n is not None})
    rng0, rngv, rnga = np.random.default_rng(seed), np.random.default_rng([int(seed), 1]), np.random.default_rng([int(seed), 2])
    n, dt = len(names), float(prob.desc.dt)
    d0 = np.stack([rng0.normal(0.0, float(sigma), (n, 3)) for _ in range(B)]).reshape(B, n, 3)
    v0 = np.stack([rngv.normal(0.0, float(sigma_v), (n, 3)) for _ in range(B)]).reshape(B, n, 3)
    a = np.stack([rnga.normal(0.0, float(sigma_a), (T - 1, n, 3)) for _ in range(B)]).reshape(B, T - 1, n, 3)
    vel = v0[:, None] + dt * np.concatenate([np.zeros((B, 1, n, 3)), np.cumsum(a, axis=1)], axis=1)             # v_j, j = 0..T-1
    move = d0[:, None] + dt * np.concatenate([np.zeros((B, 1, n, 3)), np.cumsum(vel[:, :-1], axis=1)], axis=1)  # p_j - p_0's base
    return _moved_tracks(prob, names, move)


FORECAST_MODES = {'hold': 0, 'cv': 1, 'true': 2}      # SMPC_FORECAST_* of include/smpc.h


def scene_column(c, T):
    """THE column rule of a scene track (include/smpc.h): the scene at time c is column clamp(c, 0, T - 1)"""
    return min(max(int(c), 0), int(T) - 1)


def forecast_statement(world, t, N, mode):
    """[B, N + 1, n_rows, SCENE_ROW]: the horizon's scenes as a controller forecasts them at time ``t`` from what the world track
    ``world [B, T, n_rows, SCENE_ROW]`` has shown up to then -- the numpy statement of smpc_forecast_scene and its readable definition
    (DESIGN.md section 9n).  ``t``: the scene clock (None: 0; held to +-2^62 as the kernels hold it).  With ``col`` the column rule
    with the world's T:

    ``'hold'``  every node sees the world as it stands now, column col(t): the frozen world.
    ``'cv'``    constant velocity: d = W[col(t)] - W[col(t - 1)], F[0] = W[col(t)], F[k] = F[k-1] + d -- repeated addition in this
                order for all eight slots of a record, which the kernel repeats bit for bit; d = 0 where col(t) = col(t - 1).
    ``'true'``  F[k] = W[col(t + k)]: the clairvoyant controller of run_mpc(scenes=track) without a forecast."""
    W = np.asarray(world, float)
    if W.ndim != 4 or W.shape[3] != SCENE_ROW:
        raise ValueError(f'forecast_statement: expected a world track [B, T, n_rows, {SCENE_ROW}], got {W.shape}')
    mode = FORECAST_MODES[mode] if isinstance(mode, str) else int(mode)
    if mode not in FORECAST_MODES.values():
        raise ValueError(f'forecast_statement: mode {mode}: expected one of {sorted(FORECAST_MODES)}')
    T, N = W.shape[1], int(N)
    t = 0 if t is None else min(max(int(t), -2 ** 62), 2 ** 62)
    F = np.empty((W.shape[0], N + 1) + W.shape[2:])
    if mode == FORECAST_MODES['true']:
        for k in range(N + 1):
            F[:, k] = W[:, scene_column(t + k, T)]
        return F
    F[:, 0] = W[:, scene_column(t, T)]
    d = W[:, scene_column(t, T)] - W[:, scene_column(t - 1, T)] if mode == FORECAST_MODES['cv'] else None
    for k in range(1, N + 1):
        F[:, k] = F[:, k - 1] + d if d is not None else F[:, 0]
    return F


FIT_MAX = 32                                           # SMPC_FIT_MAX of include/smpc.h: the longest window of a line fit


def fit_weights(m):
    """(u, w), two float64 arrays of length m: the weights of a least-squares line through m equally spaced samples y_j of ages
    j = 0..m-1 (j = 0 the newest).  ``sum u_j y_j`` is the line's value now and ``sum w_j y_j`` its step per column:
    ``u_j = (4m - 2 - 6j) / (m (m + 1))``, ``w_j = (6(m - 1) - 12j) / (m (m^2 - 1))`` (m = 1: w_0 = 0).  Numerators and denominators
    are small integers, so each weight is one correctly rounded division -- the bits of the engine's table (FIT_WEIGHTS,
    kernels_forecast.hpp)."""
    m = int(m)
    if not 1 <= m <= FIT_MAX:
        raise ValueError(f'fit_weights: m={m}: expected 1..{FIT_MAX}')
    j = np.arange(m)
    u = (4 * m - 2 - 6 * j).astype(float) / float(m * (m + 1))
    w = np.zeros(1) if m == 1 else (6 * (m - 1) - 12 * j).astype(float) / float(m * (m * m - 1))
    return u, w


def fit_forecast_statement(seen, t, N, window):
    """[B, N + 1, n_rows, SCENE_ROW]: the horizon's scenes forecast at time ``t`` by a least-squares line through the last ``window``
    columns of ``seen [B, T, n_rows, SCENE_ROW]``, what the controller has seen of the world (the observed track, or the world) --
    the numpy statement of smpc_forecast_scene_fit and its readable definition.  ``t``: the scene clock
    (None: 0; held to +-2^62).  With ``col`` the column rule with T, ``m = min(window, max(t, 0) + 1)`` (nothing was seen before
    time 0), ``y_j = S[col(t - j)]`` and ``(u, w) = fit_weights(m)``, for all eight slots of a record:

    ``a = u_0 y_0; a = a + u_j y_j`` (j = 1..m-1, in this order, every product rounded before its sum), ``d`` likewise with ``w``;
    ``F[0] = a, F[k] = F[k-1] + d`` -- repeated addition, as 'cv'.  The kernel repeats it bit for bit.  ``window = 1`` is 'hold',
    ``window = 2`` is 'cv' (u = (1, 0), w = (1, -1))."""
    S = np.asarray(seen, float)
    if S.ndim != 4 or S.shape[3] != SCENE_ROW:
        raise ValueError(f'fit_forecast_statement: expected a world track [B, T, n_rows, {SCENE_ROW}], got {S.shape}')
    window = int(window)
    if not 1 <= window <= FIT_MAX:
        raise ValueError(f'fit_forecast_statement: window {window}: expected 1..{FIT_MAX}')
    T, N = S.shape[1], int(N)
    t = 0 if t is None else min(max(int(t), -2 ** 62), 2 ** 62)
    m = min(window, max(t, 0) + 1)
    u, w = fit_weights(m)
    y = S[:, scene_column(t, T)]
    a, d = u[0] * y, w[0] * y
    for j in range(1, m):
        y = S[:, scene_column(t - j, T)]
        a = a + u[j] * y
        d = d + w[j] * y
    F = np.empty((S.shape[0], N + 1) + S.shape[2:])
    F[:, 0] = a
    for k in range(1, N + 1):
        F[:, k] = F[:, k - 1] + d
    return F


def poly_weights(m, degree):
    """The weights of a least-squares polynomial of degree ``p = min(degree, m - 1)`` through m equally spaced samples y_j of ages
    j = 0..m-1 (j = 0 the newest; the model is y(tau) = a + b tau + c tau^2 at tau = -j), a tuple of float64 arrays of length m:

    ``p = 0``  ``(u,)`` with ``u_j = 1.0 / float(m)``: the window mean.
    ``p = 1``  ``fit_weights(m)``: the line's value now and its step per column.
    ``p = 2``  ``(ua, uv, ue)``: ``sum ua_j y_j`` is a, the value now; ``sum uv_j y_j`` is v = b + c, the first step F[1] - F[0];
               ``sum ue_j y_j`` is e = 2c, the step of the step:
               ``ua_j = (3(3m^2 - 3m + 2) - 18(2m - 1) j + 30 j^2) / (m (m + 1)(m + 2))``
               ``uv_j = ((36m^3 - 96m^2 + 36m + 24) + (-192m^2 + 180m + 48) j + 180 m j^2) / (m (m^2 - 1)(m^2 - 4))``
               ``ue_j = (60 ((m - 1)(m - 2) - 6(m - 1) j + 6 j^2)) / (m (m^2 - 1)(m^2 - 4))``
               At m = 3 they are integers, ua = (1, 0, 0), uv = (2, -3, 1), ue = (1, -2, 1): the parabola through three columns.

    Numerators and denominators are integers (below 2^31 and up to 33 390 720 at m = 32), so each weight is one correctly rounded
    division -- the bits of the engine's table (POLY_WEIGHTS, kernels_forecast.hpp)."""
    m, degree = int(m), int(degree)
    if not 1 <= m <= FIT_MAX:
        raise ValueError(f'poly_weights: m={m}: expected 1..{FIT_MAX}')
    if not 0 <= degree <= 2:
        raise ValueError(f'poly_weights: degree={degree}: expected 0, 1 or 2')
    p = min(degree, m - 1)
    if p == 0:
        return (np.full(m, 1.0 / float(m)),)
    if p == 1:
        return fit_weights(m)
    j = np.arange(m, dtype=np.int64)
    da, dv = m * (m + 1) * (m + 2), m * (m * m - 1) * (m * m - 4)
    ua = (3 * (3 * m * m - 3 * m + 2) - 18 * (2 * m - 1) * j + 30 * j * j).astype(float) / float(da)
    uv = ((36 * m ** 3 - 96 * m * m + 36 * m + 24) + (-192 * m * m + 180 * m + 48) * j + 180 * m * j * j).astype(float) / float(dv)
    ue = (60 * ((m - 1) * (m - 2) - 6 * (m - 1) * j + 6 * j * j)).astype(float) / float(dv)
    return ua, uv, ue


def poly_forecast_statement(seen, t, N, window, degree):
    """[B, N + 1, n_rows, SCENE_ROW]: the horizon's scenes forecast at time ``t`` by a least-squares polynomial of degree 0, 1 or 2
    through the last ``window`` columns of ``seen [B, T, n_rows, SCENE_ROW]``, what the controller has seen of the world -- the numpy
    statement of smpc_forecast_scene_poly and its readable definition.  ``t``, ``col``,
    ``m = min(window, max(t, 0) + 1)`` and ``y_j = S[col(t - j)]`` as in :func:`fit_forecast_statement`; the effective degree is
    ``p = min(degree, m - 1)`` -- nothing was seen before time 0, so one sample gives a constant and two give a line.  With
    ``poly_weights(m, p)``, for all eight slots of a record:

    ``p = 0``  ``a = u_0 y_0; a = a + u_j y_j`` (j = 1..m-1, every product rounded before its sum); ``F[k] = a`` for every k --
               stored, not added, so a -0.0 stays one.  The window mean; with m = 1 it is 'hold' bit for bit.
    ``p = 1``  ``fit_forecast_statement(seen, t, N, m)``: today's line, bit for bit.
    ``p = 2``  ``a``, ``v``, ``e`` each as ``x = u_0 y_0; x = x + u_j y_j`` in increasing j, every product rounded before its sum;
               ``F[0] = a``, then for k = 1..N: ``F[k] = F[k-1] + v; v = v + e``, in that order -- repeated addition, as 'cv' and the
               fit: a constant-acceleration model.  The kernel repeats it bit for bit."""
    S = np.asarray(seen, float)
    if S.ndim != 4 or S.shape[3] != SCENE_ROW:
        raise ValueError(f'poly_forecast_statement: expected a world track [B, T, n_rows, {SCENE_ROW}], got {S.shape}')
    window, degree = int(window), int(degree)
    if not 1 <= window <= FIT_MAX:
        raise ValueError(f'poly_forecast_statement: window {window}: expected 1..{FIT_MAX}')
    if not 0 <= degree <= 2:
        raise ValueError(f'poly_forecast_statement: degree {degree}: expected 0, 1 or 2')
    T, N = S.shape[1], int(N)
    t = 0 if t is None else min(max(int(t), -2 ** 62), 2 ** 62)
    m = min(window, max(t, 0) + 1)
    p = min(degree, m - 1)
    if p == 1:
        return fit_forecast_statement(S, t, N, m)
    us = poly_weights(m, p)
    y = S[:, scene_column(t, T)]
    acc = [u[0] * y for u in us]
    for j in range(1, m):
        y = S[:, scene_column(t - j, T)]
        acc = [x + u[j] * y for x, u in zip(acc, us)]
    F = np.empty((S.shape[0], N + 1) + S.shape[2:])
    F[:, 0] = acc[0]
    if p == 0:
        for k in range(1, N + 1):
            F[:, k] = acc[0]
        return F
    v, e = acc[1], acc[2]
    for k in range(1, N + 1):
        F[:, k] = F[:, k - 1] + v
        v = v + e
    return F


def observe_tracks(prob, world, sigma, seed=0):
    """[B, T, n_rows, SCENE_ROW]: ``world`` as a sensor with independent noise shows it -- every obstacle's position in every
    (instance, column) off by its own N(0, sigma^2) draw per axis, one draw per (instance, obstacle, column) shared by all the rows
    the obstacle appears in (plane rows take their axis in slot 6, capsule rows move both end points, as ``_moved_tracks`` does).
    The draws come instance by instance, so instance b's do not depend on B; reproducible per seed; ``sigma = 0`` returns the
    world's bits.  What run_mpc(observed=...) and smpc_set_instance_observed_track take."""
    W = np.asarray(world, float)
    if W.ndim != 4 or W.shape[2:] != (len(prob.rows), SCENE_ROW):
        raise ValueError(f'observe_tracks: expected a world track [B, T, {len(prob.rows)}, {SCENE_ROW}], got {W.shape}')
    if float(sigma) < 0:
        raise ValueError(f'observe_tracks: sigma={sigma}: a standard deviation is not negative')
    out = W.copy()
    if float(sigma) == 0.0:
        return out
    B, T = W.shape[:2]
    names = sorted({n for n in prob.row_obstacle if n is not None})
    rng = np.random.default_rng([int(seed), 3])
    e = np.stack([rng.normal(0.0, float(sigma), (T, len(names), 3)) for _ in range(B)]).reshape(B, T, len(names), 3)
    for i, (r, name) in enumerate(zip(prob.rows, prob.row_obstacle)):
        if name is None:
            continue
        d = e[:, :, names.index(name)]
        if r.kind == ROW_COORD:
            out[:, :, i, 6] += d[:, :, r.axis]
        else:
            out[:, :, i, 0:3] += d
            if r.kind == ROW_SEG_FIXEDSEG:
                out[:, :, i, 3:6] += d
    return out


def extend_tracks(tracks, T):
    """Scene tracks [B, T0, n_rows, SCENE_ROW] continued to T columns at constant velocity -- the step between their last two
    columns (none for T0 = 1) -- or cut to T columns: what turns the tracks stored with warm starts (one horizon long) into the
    tracks of a closed-loop run."""
    tracks = np.asarray(tracks, float)
    T0, T = tracks.shape[1], int(T)
    if T <= T0:
        return np.ascontiguousarray(tracks[:, :max(T, 1)])
    step = tracks[:, -1] - tracks[:, -2] if T0 > 1 else np.zeros_like(tracks[:, -1])
    more = tracks[:, -1:, :, :] + step[:, None] * np.arange(1, T - T0 + 1)[None, :, None, None]
    return np.concatenate([tracks, more], axis=1)


def inflated_row_bounds(prob, B, margin):
    """``(lo, hi)``, each ``[B, N+1, n_rows]``: the collision rows' bounds with ``margin`` metres of extra room around every
    world-fixed element, per instance, node and row -- what smpc_set_instance_row_bounds takes.  ``margin`` is
    ``[N+1]`` (a profile along the horizon for every instance and row), ``[B, N+1]`` or ``[B, N+1, n_rows]``, finite and >= 0.
    Rows without a world-fixed element (``row_obstacle`` None: robot against robot) keep their bounds.  A squared-distance row
    (fixed capsule, sphere, fixed point) gets ``lb' = (sqrt(lb) + d)^2``; a plane row ``lb' = lb + d`` and ``ub' = ub - d``; a side
    that is absent (``|v| >= INF``) stays absent.  Where ``d == 0.0`` the descriptor's own doubles come back, bit for bit.  With
    ``d = 2 c`` this is what ``collision_margin = c`` does to a problem built without one."""
    N, nr, B = int(prob.N), len(prob.rows), int(B)
    m = np.asarray(margin, float)
    shapes = {1: (N + 1,), 2: (B, N + 1), 3: (B, N + 1, nr)}
    if B < 1 or m.ndim not in shapes or m.shape != shapes[m.ndim]:
        raise ValueError(f'inflated_row_bounds: margin of shape {m.shape}: expected [{N + 1}], [{B}, {N + 1}] or [{B}, {N + 1}, {nr}]')
    if not np.all(np.isfinite(m)) or np.any(m < 0.0):
        raise ValueError('inflated_row_bounds: a margin is finite and not negative')
    d = np.broadcast_to(m if m.ndim == 3 else (m[:, :, None] if m.ndim == 2 else m[None, :, None]), (B, N + 1, nr))
    lo = np.broadcast_to(np.asarray(prob.row_lb, float), (B, N + 1, nr)).copy()
    hi = np.broadcast_to(np.asarray(prob.row_ub, float), (B, N + 1, nr)).copy()
    for i, (r, name) in enumerate(zip(prob.rows, prob.row_obstacle)):
        di = d[:, :, i]
        on = di != 0.0
        if name is None or not on.any():
            continue
        if r.kind == ROW_COORD:
            if abs(r.lb) < INF:
                lo[:, :, i] = np.where(on, r.lb + di, r.lb)
            if abs(r.ub) < INF:
                hi[:, :, i] = np.where(on, r.ub - di, r.ub)
            if abs(r.lb) < INF and abs(r.ub) < INF and np.any(lo[:, :, i] > hi[:, :, i]):
                b, k = np.argwhere(lo[:, :, i] > hi[:, :, i])[0]
                raise ValueError(f'inflated_row_bounds: row {i} ({prob.row_names[i]}): a margin of {di[b, k]:g} m at instance {b}, '
                                 f'node {k} makes its sides cross ({lo[b, k, i]:g} > {hi[b, k, i]:g})')
        elif abs(r.lb) < INF:
            lo[:, :, i] = np.where(on, (np.sqrt(r.lb) + di) ** 2, r.lb)
    return lo, hi


FIT_MARGIN_CAP = 0.05                                  # the default d_max of a fitted margin, metres

# the slots of a scene record that move with the row's world-fixed element, by row kind: the ones smpc_set_instance_scene_track
# validates (set_scene_table, engine.hip).  A robot-robot row has none.
_MOVING_SLOTS = {ROW_SEG_FIXEDSEG: (0, 1, 2, 3, 4, 5), ROW_SEG_POINT: (0, 1, 2), ROW_POINT_POINT: (0, 1, 2), ROW_COORD: (6,),
                 ROW_SEG_SEG: ()}


def moving_slots(kind):
    """The slots of a scene record that a row of ``kind`` reads of its world-fixed element: 0..5 for a fixed capsule, 0..2 for a
    fixed point, 6 for a plane, none for a robot-robot row."""
    return _MOVING_SLOTS[int(kind)]


def margin_growth(m, degree, N):
    """``h [N + 1]``: the sum of the squared weights with which a least-squares polynomial of degree ``p = min(degree, m - 1)``
    through m samples forms its forecast k columns ahead, ``h_k = sum_j c_kj^2`` -- the variance of the forecast at node k in units
    of the variance of one sample; ``g_k = sqrt(h_k)`` is the growth of a fitted margin along the horizon.
    With ``poly_weights(m, p)``: ``c_kj = 1 / m`` (p = 0), ``u_j + k w_j`` (p = 1), ``(ua_j + k uv_j) + (k (k - 1) / 2) ue_j``
    (p = 2); every product rounded before its sum, the sum in increasing j starting from the j = 0 term.  k_fit_margin repeats it
    operation for operation."""
    m, N = int(m), int(N)
    p = min(int(degree), m - 1)
    us = poly_weights(m, p)
    k = np.arange(N + 1, dtype=float)
    kk = np.arange(N + 1, dtype=float) * (np.arange(N + 1, dtype=float) - 1.0) / 2.0      # k (k - 1) / 2: small integers, exact
    h = None
    for j in range(m):
        if p == 0:
            c = np.full(N + 1, us[0][j])
        elif p == 1:
            c = us[0][j] + k * us[1][j]
        else:
            c = (us[0][j] + k * us[1][j]) + kk * us[2][j]
        h = c * c if h is None else h + c * c
    return h


def _check_fit_margin(who, prob, window, degree, z, sigma_prior, base, d_max):
    window, degree = int(window), int(degree)
    if not 1 <= window <= FIT_MAX:
        raise ValueError(f'{who}: window {window}: expected 1..{FIT_MAX}')
    if not 0 <= degree <= 2:
        raise ValueError(f'{who}: degree {degree}: expected 0, 1 or 2')
    base = tuple(float(v) for v in np.asarray(base, float).reshape(-1))
    if len(base) != 2:
        raise ValueError(f'{who}: base {base}: expected (a, b), the margin a + b k metres at node k')
    vals = {'z': float(z), 'sigma_prior': float(sigma_prior), 'base_a': base[0], 'base_b': base[1], 'd_max': float(d_max)}
    for name, v in vals.items():
        if not (np.isfinite(v) and v >= 0.0):
            raise ValueError(f'{who}: {name}={v}: expected a finite number that is not negative')
    for i, r in enumerate(prob.rows):
        if r.kind == ROW_COORD and abs(r.lb) < INF and abs(r.ub) < INF and r.lb + vals['d_max'] > r.ub - vals['d_max']:
            raise ValueError(f'{who}: row {i} ({prob.row_names[i]}): d_max={vals["d_max"]:g} makes its sides cross '
                             f'({r.lb + vals["d_max"]:g} > {r.ub - vals["d_max"]:g})')
    return window, degree, vals['z'], vals['sigma_prior'], base, vals['d_max']


def fit_margin_statement(prob, seen, t, window, degree, z, sigma_prior=0.0, base=(0.0, 0.0), d_max=FIT_MARGIN_CAP):
    """``d [B, N + 1, n_rows]``, metres: the margin a controller leaves around the world-fixed element of every collision row at
    every node, formed from the residuals of the fit it forecasts with -- the prediction interval of a least-squares polynomial, the
    numpy statement of smpc_forecast_row_margin and its readable definition.  ``inflated_row_bounds(prob, B,
    d)`` turns it into the table the entry point writes.

    ``seen``, ``t``, ``col``, ``m = min(window, max(t, 0) + 1)``, ``p = min(degree, m - 1)`` and ``y_j = S[col(t - j)]`` as in
    :func:`poly_forecast_statement`, and ``a``, ``v``, ``e`` are that statement's numbers for every slot (p = 0: a; p = 1: a and the
    step, here v; p = 2: a, v, e), formed by the same operations in the same order.

    The residual variance.  ``nu = m - p - 1``.  With ``nu >= 1``, per slot in increasing j: ``f_j = a`` (p = 0), ``a - j v``
    (p = 1), ``(a - j v) + T_j e`` with ``T_j = j (j + 1) / 2`` (p = 2) -- the fitted polynomial at age j --, ``res = y_j - f_j``,
    ``q = res res`` at j = 0 and ``q = q + res res`` afterwards, every product rounded before its sum.  ``rss`` is the largest q
    over the row's moving slots (:func:`moving_slots`), taken so that a NaN wins; ``s2 = rss / float(nu)``, raised to
    ``var_prior = sigma_prior^2`` where it is below it (a NaN stays).  ``nu == 0``: nothing can be estimated, ``s2 = var_prior``.
    ``s = sqrt(s2)``.

    The growth.  ``g_k = sqrt(h_k)``, ``h = margin_growth(m, p, N)``: without a "+ 1" under the root, because the true obstacle
    carries no noise -- what is bounded is the forecast's error against the truth.

    The margin.  ``d_k = (base_a + base_b k) + (z s) g_k``, every product rounded; ``d_k = d_k if d_k <= d_max else d_max``, so a
    NaN anywhere in a moving slot of the window gives the cap, never a NaN bound.  A row without a world-fixed element (``row_obstacle``
    None, kind SEG_SEG) has d = 0 at every node.

    The margin is per axis: the largest residual sum over the moving slots stands for the element's whole displacement, and the
    distance to an obstacle that errs along three axes can exceed it by up to sqrt(3).  Taking the maximum, not the mean, over the
    slots errs on the wide side of a per-axis interval.

    ValueError: window outside 1..FIT_MAX, degree outside 0..2, a negative or non-finite z, sigma_prior, base or d_max, or a d_max
    that makes a plane row's two sides cross (the message names the row)."""
    S = np.asarray(seen, float)
    nr = len(prob.rows)
    if S.ndim != 4 or S.shape[2:] != (nr, SCENE_ROW):
        raise ValueError(f'fit_margin_statement: expected a track [B, T, {nr}, {SCENE_ROW}], got {S.shape}')
    window, degree, z, sigma_prior, (base_a, base_b), d_max = _check_fit_margin('fit_margin_statement', prob, window, degree, z,
                                                                                 sigma_prior, base, d_max)
    B, T, N = S.shape[0], S.shape[1], int(prob.N)
    t = 0 if t is None else min(max(int(t), -2 ** 62), 2 ** 62)
    m = min(window, max(t, 0) + 1)
    p = min(degree, m - 1)
    nu = m - p - 1
    var_prior = sigma_prior * sigma_prior
    s2 = np.full((B, nr), var_prior)
    if nu >= 1:
        us = poly_weights(m, p)
        y = S[:, scene_column(t, T)]
        acc = [u[0] * y for u in us]
        for j in range(1, m):
            y = S[:, scene_column(t - j, T)]
            acc = [x + u[j] * y for x, u in zip(acc, us)]
        q = None
        for j in range(m):
            y = S[:, scene_column(t - j, T)]
            if p == 0:
                f = acc[0]
            elif p == 1:
                f = acc[0] - float(j) * acc[1]
            else:
                f = (acc[0] - float(j) * acc[1]) + float(j * (j + 1) // 2) * acc[2]
            res = y - f
            q = res * res if q is None else q + res * res
        for i, r in enumerate(prob.rows):
            slots = moving_slots(r.kind)
            if not slots:
                continue
            rss = np.zeros(B)
            for s_ in slots:
                rss = np.maximum(rss, q[:, i, s_])              # (a NaN wins)
            v = rss / float(nu)
            s2[:, i] = np.where((v > var_prior) | (v != v), v, var_prior)
    s = np.sqrt(s2)
    g = np.sqrt(margin_growth(m, p, N))
    k = np.arange(N + 1, dtype=float)
    with np.errstate(invalid='ignore'):
        d = (base_a + base_b * k)[None, :, None] + (z * s)[:, None, :] * g[None, :, None]
        d = np.where(d <= d_max, d, d_max)
    for i, r in enumerate(prob.rows):
        if not moving_slots(r.kind):
            d[:, :, i] = 0.0
    return d


KALMAN_REC = 32                                        # SMPC_KALMAN_REC of include/smpc.h: doubles per (instance, row) filter record
# the record's layout: pos[8] | vel[8] | acc[8] | P00 P01 P02 P11 P12 P22 | s2 | n
KALMAN_POS, KALMAN_VEL, KALMAN_ACC, KALMAN_P, KALMAN_S2, KALMAN_N = 0, 8, 16, 24, 30, 31


class KalmanParams(C.Structure):
    """smpc_kalman_params (include/smpc.h): the model of one filter, shared by every record of a call"""
    _fields_ = [('degree', C.c_int32), ('reserved', C.c_int32), ('q', C.c_double), ('r', C.c_double), ('v0', C.c_double),
                ('a0', C.c_double), ('beta', C.c_double)]


def kalman_params(degree, q, r, v0=None, a0=None, beta=0.0, who='kalman_params'):
    """A checked :class:`KalmanParams`: ``degree`` 0..2 (constant, constant velocity, constant acceleration), ``q >= 0`` the process
    noise, ``r > 0`` the sensor noise in metres, ``v0``, ``a0 >= 0`` the prior standard deviations of velocity and acceleration per
    column (default: ``r`` each -- before anything moves, a step is as uncertain as one sample), ``beta`` in [0, 1] the rate at which
    the innovation scale s2 follows the normalised innovation.  ValueError names the argument."""
    if isinstance(degree, KalmanParams):      # (a record is checked again: its fields are the caller's to write)
        par = degree
        degree, q, r, v0, a0, beta = par.degree, par.q, par.r, par.v0, par.a0, par.beta
    elif isinstance(degree, (tuple, list)):
        return kalman_params(*degree, who=who)
    degree = int(degree)
    if not 0 <= degree <= 2:
        raise ValueError(f'{who}: degree {degree}: expected 0, 1 or 2')
    q, r, beta = float(q), float(r), float(beta)
    if not (np.isfinite(r) and r > 0.0):
        raise ValueError(f'{who}: r={r}: expected a finite number above zero')
    v0, a0 = (r if v is None else float(v) for v in (v0, a0))
    for name, v in (('q', q), ('v0', v0), ('a0', a0)):
        if not (np.isfinite(v) and v >= 0.0):
            raise ValueError(f'{who}: {name}={v}: expected a finite number that is not negative')
    if not 0.0 <= beta <= 1.0:
        raise ValueError(f'{who}: beta={beta}: expected a number in [0, 1]')
    return KalmanParams(degree, 0, q, r, v0, a0, beta)


def kalman_noise(par):
    """``(Q, r2, v02, a02)`` as the engine forms them on the host: ``Q = q^2 G G'`` with G = (1), (1/2, 1) or (1/6, 1/2, 1) as the six
    numbers Q00 Q01 Q02 Q11 Q12 Q22 -- ``gq_i = q G_i`` rounded, ``Q_ij = gq_i gq_j`` rounded, zero where a component is absent --
    and the three squares."""
    p, q = int(par.degree), float(par.q)
    G = ((1.0,), (0.5, 1.0), (1.0 / 6.0, 0.5, 1.0))[p]
    gq = [q * g for g in G] + [0.0] * (2 - p)
    Q = (gq[0] * gq[0], gq[0] * gq[1], gq[0] * gq[2], gq[1] * gq[1], gq[1] * gq[2], gq[2] * gq[2])
    return Q, float(par.r) * float(par.r), float(par.v0) * float(par.v0), float(par.a0) * float(par.a0)


def kalman_predict_cov(p, P, Q):
    """``Phi P Phi' + Q`` for the six numbers ``P = (P00, P01, P02, P11, P12, P22)`` (floats or arrays) of a filter of degree p, with
    Phi = ((1, 1, 1/2), (0, 1, 1), (0, 0, 1)) cut to p + 1 components, in THE order of operations (k_scene_kalman and k_kalman_margin
    repeat it): first the rows of ``A = Phi P``, then ``A Phi'``, then ``+ Q``; entries of absent components pass through."""
    P00, P01, P02, P11, P12, P22 = P
    if p == 0:
        return (P00 + Q[0], P01, P02, P11, P12, P22)
    if p == 1:
        A00 = P00 + P01
        A01 = P01 + P11
        return ((A00 + A01) + Q[0], A01 + Q[1], P02, P11 + Q[3], P12, P22)
    A00 = (P00 + P01) + 0.5 * P02
    A01 = (P01 + P11) + 0.5 * P12
    A02 = (P02 + P12) + 0.5 * P22
    A11 = P11 + P12
    A12 = P12 + P22
    return (((A00 + A01) + 0.5 * A02) + Q[0], (A01 + A02) + Q[1], A02 + Q[2], (A11 + A12) + Q[3], A12 + Q[4], P22 + Q[5])


def new_kalman_state(B, n_rows):
    """``[B, n_rows, KALMAN_REC]`` zeros: every record "nothing seen" """
    return np.zeros((int(B), int(n_rows), KALMAN_REC))


def kalman_statement(state, y, kinds, par, N, advance=True):
    """``(state', F)``: one step of the obstacle filter and its forecast -- the numpy statement of smpc_forecast_scene_kalman and its
    readable definition.  ``state [B, n_rows, KALMAN_REC]``: per (instance, row) record
    ``pos[8] | vel[8] | acc[8] | P00 P01 P02 P11 P12 P22 | s2 | n`` (all zero: nothing seen); ``y [B, n_rows, SCENE_ROW]``: the column
    of what was seen at the scene clock, ``S[:, col(t)]`` (not read with ``advance=False``; may be None then); ``kinds [n_rows]``: the
    row kinds; ``par``: :func:`kalman_params`; ``F [B, N + 1, n_rows, SCENE_ROW]``.  Time is in columns.  All eight slots of a record
    are filtered with the record's gains; only components 0..p of the state are used, the others are written as zero when a record
    is first seen and otherwise neither read nor written.

    A record is OBSERVED when none of its row kind's moving slots (:func:`moving_slots`) holds a NaN in y; a robot-robot row always is.

    Advance, n < 1 (nothing seen).  Observed: ``pos = y``, ``vel = acc = 0``, ``P = diag(r^2, v0^2, a0^2)`` (an absent component: 0),
    ``s2 = 1``, ``n = 1``.  Unobserved: the record stays.

    Advance, n >= 1.  Predict: ``pos- = (pos + vel) + 0.5 acc``, ``vel- = vel + acc`` (without the absent terms),
    ``P- = kalman_predict_cov(p, P, Q)``.  Observed: ``S = P-00 + r^2``, ``inv = 1.0 / S`` -- the ONE division --, ``K_i = P-0i inv``;
    per slot ``nu = y - pos-``, ``x_i = x-_i + K_i nu``; ``P_ij = P-ij - K_i P-0j`` for i <= j; ``nis`` the largest ``(nu nu) inv``
    over the moving slots from 0.0, a NaN winning; ``s2 = s2 + beta (nis - s2)``, then 1.0 where it is below 1.0; ``n = n + 1``.
    Unobserved: ``x = x-``, ``P = P-``; s2 and n stay.  Every product is rounded before its sum.

    Forecast, from the state after the advance.  p = 0: ``F[k] = pos`` for every k, stored.  p = 1: ``F[0] = pos``,
    ``F[k] = F[k-1] + vel``.  p = 2: ``v = vel + 0.5 acc``, ``F[0] = pos``, then ``F[k] = F[k-1] + v; v = v + acc``, in that order."""
    st = np.array(state, float)
    if st.ndim != 3 or st.shape[2] != KALMAN_REC:
        raise ValueError(f'kalman_statement: expected a state [B, n_rows, {KALMAN_REC}], got {st.shape}')
    par = kalman_params(par, 0, 1, who='kalman_statement')
    p, beta, N = int(par.degree), float(par.beta), int(N)
    kinds = [int(k) for k in kinds]
    B, nr = st.shape[:2]
    if len(kinds) != nr:
        raise ValueError(f'kalman_statement: {len(kinds)} row kinds for {nr} rows')
    Q, r2, v02, a02 = kalman_noise(par)
    pos, vel, acc = st[:, :, 0:8].copy(), st[:, :, 8:16].copy(), st[:, :, 16:24].copy()
    if advance:
        y = np.asarray(y, float)
        if y.shape != (B, nr, SCENE_ROW):
            raise ValueError(f'kalman_statement: expected y [{B}, {nr}, {SCENE_ROW}], got {y.shape}')
        P = tuple(st[:, :, KALMAN_P + i].copy() for i in range(6))
        s2, n = st[:, :, KALMAN_S2].copy(), st[:, :, KALMAN_N].copy()
        obs = np.ones((B, nr), bool)
        for i, kind in enumerate(kinds):
            for s_ in moving_slots(kind):
                obs[:, i] &= ~np.isnan(y[:, i, s_])
        seen = n >= 1.0
        with np.errstate(all='ignore'):
            # predict
            pos_m = pos if p == 0 else (pos + vel if p == 1 else (pos + vel) + 0.5 * acc)
            vel_m = vel + acc if p == 2 else vel
            Pm = kalman_predict_cov(p, P, Q)
            # update
            inv = 1.0 / (Pm[0] + r2)
            K = (Pm[0] * inv, Pm[1] * inv, Pm[2] * inv)
            nu = y - pos_m
            pos_u = pos_m + K[0][:, :, None] * nu
            vel_u = vel_m + K[1][:, :, None] * nu if p >= 1 else vel
            acc_u = acc + K[2][:, :, None] * nu if p == 2 else acc
            Pu = [Pm[0] - K[0] * Pm[0], Pm[1] - K[0] * Pm[1], Pm[2] - K[0] * Pm[2], Pm[3] - K[1] * Pm[1], Pm[4] - K[1] * Pm[2],
                  Pm[5] - K[2] * Pm[2]]
            used = (True, p >= 1, p == 2, p >= 1, p == 2, p == 2)
            Pu = [u if on else m for u, m, on in zip(Pu, Pm, used)]
            nis = np.zeros((B, nr))
            for i, kind in enumerate(kinds):
                for s_ in moving_slots(kind):
                    nis[:, i] = np.maximum(nis[:, i], (nu[:, i, s_] * nu[:, i, s_]) * inv[:, i])       # (a NaN wins)
            s2_u = s2 + beta * (nis - s2)
            s2_u = np.where(s2_u < 1.0, 1.0, s2_u)
        first, upd, pred = ~seen & obs, seen & obs, seen & ~obs
        P0 = (r2, 0.0, 0.0, v02 if p >= 1 else 0.0, 0.0, a02 if p == 2 else 0.0)

        def pick(old, init, predicted, updated):
            sel = [x[:, :, None] if np.ndim(old) == 3 else x for x in (first, pred, upd)]
            return np.where(sel[0], init, np.where(sel[1], predicted, np.where(sel[2], updated, old)))
        pos, vel, acc = pick(pos, y, pos_m, pos_u), pick(vel, 0.0, vel_m, vel_u), pick(acc, 0.0, acc, acc_u)
        P = tuple(pick(P[i], P0[i], Pm[i], Pu[i]) for i in range(6))
        s2, n = pick(s2, 1.0, s2, s2_u), pick(n, 1.0, n, n + 1.0)
        st[:, :, 0:8], st[:, :, 8:16], st[:, :, 16:24] = pos, vel, acc
        for i in range(6):
            st[:, :, KALMAN_P + i] = P[i]
        st[:, :, KALMAN_S2], st[:, :, KALMAN_N] = s2, n
    F = np.empty((B, N + 1, nr, SCENE_ROW))
    F[:, 0] = pos
    with np.errstate(all='ignore'):
        v = vel + 0.5 * acc if p == 2 else vel
        for k in range(1, N + 1):
            if p == 0:
                F[:, k] = pos
                continue
            F[:, k] = F[:, k - 1] + v
            if p == 2:
                v = v + acc
    return st, F


def kalman_margin_statement(prob, state, par, z, base=(0.0, 0.0), d_max=FIT_MARGIN_CAP):
    """``d [B, N + 1, n_rows]``, metres: the margin around the world-fixed element of every collision row at every node from the
    filter's own covariance -- the numpy statement of smpc_kalman_row_margin and its readable definition.
    ``inflated_row_bounds(prob, B, d)`` turns it into the table the entry point writes.  It reads P and s2 of ``state [B, n_rows,
    KALMAN_REC]`` and nothing else:

    ``Pi_0 = P``, ``Pi_k = kalman_predict_cov(p, Pi_{k-1}, Q)``, ``g_k = sqrt(Pi_k[0][0])`` -- the predicted covariance grows along the
    horizon because the obstacle may turn (Q), not only because the state is uncertain; no ``+ r^2``, the true obstacle carries no
    noise (as in 9r).  ``d_k = (base_a + base_b k) + (z sqrt(s2)) g_k``, every product rounded; ``d_k = d_k if d_k <= d_max else
    d_max``, so a NaN gives the cap.  A row without a moving slot (SEG_SEG) has d = 0.  A record that has seen nothing (all zero)
    has P = 0 and s2 = 0: only the base and what Q adds along the horizon.

    ValueError as :func:`fit_margin_statement`'s for z, base and d_max, and :func:`kalman_params`' for ``par``."""
    st = np.asarray(state, float)
    nr = len(prob.rows)
    if st.ndim != 3 or st.shape[1:] != (nr, KALMAN_REC):
        raise ValueError(f'kalman_margin_statement: expected a state [B, {nr}, {KALMAN_REC}], got {st.shape}')
    par = kalman_params(par, 0, 1, who='kalman_margin_statement')
    _, _, z, _, (base_a, base_b), d_max = _check_fit_margin('kalman_margin_statement', prob, 1, 0, z, 0.0, base, d_max)
    p, N, B = int(par.degree), int(prob.N), st.shape[0]
    Q = kalman_noise(par)[0]
    Pi = tuple(st[:, :, KALMAN_P + i] for i in range(6))
    d = np.empty((B, N + 1, nr))
    with np.errstate(invalid='ignore'):
        zs = z * np.sqrt(st[:, :, KALMAN_S2])
        for k in range(N + 1):
            dk = (base_a + base_b * float(k)) + zs * np.sqrt(Pi[0])
            d[:, k] = np.where(dk <= d_max, dk, d_max)
            Pi = kalman_predict_cov(p, Pi, Q)
    for i, r in enumerate(prob.rows):
        if not moving_slots(r.kind):
            d[:, :, i] = 0.0
    return d


def occlude_tracks(prob, observed, p_start, mean_len, seed=0):
    """``observed [B, T, n_rows, SCENE_ROW]`` with NaN bursts where a sensor loses sight of an obstacle: per (instance, obstacle),
    walking the columns, a visible obstacle starts a burst with probability ``p_start`` and an occluded one comes back with
    probability ``1 / mean_len`` (burst lengths are geometric with that mean; ``mean_len >= 1``).  A burst sets NaN in the moving
    slots (:func:`moving_slots`) of every row the obstacle appears in, and nowhere else.  The draws come instance by instance, one
    ``[T, obstacle]`` block of uniforms each, so instance b's do not depend on B; reproducible per seed; ``p_start = 0`` returns the
    input's bits.  What run_mpc(observed=..., forecast='kalman') studies dropouts with."""
    S = np.asarray(observed, float)
    if S.ndim != 4 or S.shape[2:] != (len(prob.rows), SCENE_ROW):
        raise ValueError(f'occlude_tracks: expected a track [B, T, {len(prob.rows)}, {SCENE_ROW}], got {S.shape}')
    p_start, mean_len = float(p_start), float(mean_len)
    if not 0.0 <= p_start <= 1.0:
        raise ValueError(f'occlude_tracks: p_start={p_start}: expected a probability')
    if not (np.isfinite(mean_len) and mean_len >= 1.0):
        raise ValueError(f'occlude_tracks: mean_len={mean_len}: expected a finite number >= 1')
    out = S.copy()
    if p_start == 0.0:
        return out
    B, T = S.shape[:2]
    names = sorted({n for n in prob.row_obstacle if n is not None})
    rng = np.random.default_rng([int(seed), 4])
    u = np.stack([rng.random((T, len(names))) for _ in range(B)]).reshape(B, T, len(names))
    hidden = np.zeros((B, T, len(names)), bool)
    now = np.zeros((B, len(names)), bool)
    for j in range(T):
        now = np.where(now, u[:, j] >= 1.0 / mean_len, u[:, j] < p_start)
        hidden[:, j] = now
    for i, (r, name) in enumerate(zip(prob.rows, prob.row_obstacle)):
        if name is None:
            continue
        h = hidden[:, :, names.index(name)]
        for s_ in moving_slots(r.kind):
            out[:, :, i, s_] = np.where(h, np.nan, out[:, :, i, s_])
    return out
