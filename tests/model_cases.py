"""Shared pieces of the per-instance-model tests (test_models_host.py, test_models_gpu.py): the perturbed joint tables the tests
use, problems whose DESCRIPTOR carries one instance's inertials (what the oracle understands: one descriptor per model), the same
with a shared tightened torque limit, and ModelOracleSolver, the CPU double of a solver that holds a model per instance.  Not a
test module."""
import copy
import functools

import numpy as np

from conftest import make_problem, make_problem_fr7, sample_instances
from fake_solver import OracleSolver

N_MODELS, NOISE = 8, 20.0
INERTIALS = ('mass', 'com', 'inertia')
KINEMATICS_AND_LIMITS = ('R0', 'p0', 'axis', 'q_min', 'q_max', 'v_max', 'tau_max')


def model_tables(par, nq, n=N_MODELS, noise=NOISE):
    """[n, nq] JOINT_DTYPE: perturbed_joint_tables(par, nq, 20 %, seeds 0 .. n - 1), the plant tables of run_mpc(noise=20)"""
    from safe_mpc_amd.closed_loop import perturbed_joint_tables
    return perturbed_joint_tables(par, nq, noise, range(n))


def problem_with_model(prob, table_b, tau_max=None):
    """a copy of ``prob`` whose descriptor carries the inertials of ``table_b [nq]`` (and the torque limits ``tau_max [nq]`` in the
    descriptor and in the problem's check arrays, when given); everything else is shared with ``prob``"""
    new = copy.copy(prob)
    new.desc = type(prob.desc).from_buffer_copy(prob.desc)
    for i in range(prob.nq):
        J = new.desc.joints[i]
        J.mass = float(table_b['mass'][i])
        for k in range(3):
            J.com[k] = float(table_b['com'][i][k])
        for k in range(6):
            J.inertia[k] = float(table_b['inertia'][i][k])
        if tau_max is not None:
            J.tau_max = float(tau_max[i])
    if tau_max is not None:
        new.tau_max, new.tau_min = np.array(tau_max, float), -np.array(tau_max, float)
    return new


def tightened(prob, tables, x0):
    """The clip-property problem: (problem, tables, tau_max) with the shared limit tau_max = max(1.10 |tau(x0, 0)|, 0.05) of the
    NOMINAL model at the state x0 [nx] written into the descriptor, the problem's check arrays and every plant table"""
    from oracle.oracle import Oracle
    nq = prob.nq
    tau0 = Oracle(prob).rnea(x0[:nq], x0[nq:], np.zeros(nq))
    tau_max = np.maximum(1.10 * np.abs(tau0), 0.05)
    tables = tables.copy()
    tables['tau_max'] = tau_max[None, :]
    return problem_with_model(prob, prob.joint_table(), tau_max), tables, tau_max


@functools.lru_cache(maxsize=None)
def family(system='z1', controller='naive', N=8, n=N_MODELS):
    """(par, prob, net), the n tables and the n problems with a model each"""
    par, prob, net = make_problem(controller, N=N) if system == 'z1' else make_problem_fr7(controller, N=N)
    tables = model_tables(par, prob.nq, n)
    return (par, prob, net), tables, [problem_with_model(prob, t) for t in tables]


@functools.lru_cache(maxsize=None)
def clip_family(N=8, n=N_MODELS):
    """the issue's clip-property set-up: make_problem('naive', N), all n instances at sample_instances(prob, 8, seed=1,
    vel_scale=0)[0], shared tightened limits: (par, prob_tight, net), tables (tightened tau_max), x0 [n, nx], per-model problems"""
    par, prob, net = make_problem('naive', N=N)
    x1 = sample_instances(prob, 8, seed=1, vel_scale=0.0)[0]
    tight, tables, tau_max = tightened(prob, model_tables(par, prob.nq, n), x1)
    return (par, tight, net), tables, np.repeat(x1[None], n, axis=0), [problem_with_model(tight, t, tau_max) for t in tables]


class ModelOracleSolver(OracleSolver):
    """OracleSolver with ``set_instance_models``: one OracleSolver per distinct table (each on the problem whose descriptor carries
    that table's inertials), and every batched call split by model, sent to the model's solver and put back in instance order.
    Without models it is the OracleSolver of the base problem.  The plant keeps its own ``joints_noisy`` argument."""

    def __init__(self, problem, net=None, device=0):
        super().__init__(problem, net)
        self.net_ = net
        self.subs, self.keys = [], []
        self.idx = None
        self.model_calls = []

    @staticmethod
    def _key(t):
        return b''.join(np.ascontiguousarray(t[f]).tobytes() for f in INERTIALS)

    def set_instance_models(self, joints=None):
        self.model_calls.append(None if joints is None else np.array(joints))
        if joints is None:
            self.idx = None
            return
        base = self.problem.joint_table()
        for f in KINEMATICS_AND_LIMITS:
            if not np.array_equal(joints[f], np.broadcast_to(base[f], joints[f].shape)):
                raise ValueError(f'set_instance_models: {f} differs from the descriptor\'s')
        idx = []
        for t in joints:
            k = self._key(t)
            if k not in self.keys:
                sub = OracleSolver(problem_with_model(self.problem, t), self.net_)
                sub.set_horizon(self.N)
                self.keys.append(k)
                self.subs.append(sub)
            idx.append(self.keys.index(k))
        self.idx = np.array(idx)

    def set_horizon(self, N):
        super().set_horizon(N)
        for s in self.subs:
            s.set_horizon(N)

    def _split(self, name, batched):
        B = len(batched[0])
        if self.idx is None:
            return getattr(OracleSolver, name)(self, *batched)
        assert len(self.idx) == B, f'{name}: batch {B}, models set for {len(self.idx)} instances'
        out, r = None, None
        for s in np.unique(self.idx):
            m = np.where(self.idx == s)[0]
            r = getattr(self.subs[s], name)(*[np.ascontiguousarray(a[m]) for a in batched])
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


def clip_loop(solver, x0, N, steps, plant_tables):
    """``steps`` of guessCorrection / solve / plant / provideControl from the state x0 [B, nx] held as the guess: returns the worst
    |u_eff - u_0| and the worst |u_0| per instance, and the statuses [steps, B].  ``solver``: anything with solve,
    guess_correction, provide_control and plant_step (an OracleSolver, a ModelOracleSolver, a BatchedOcpSolver)."""
    from conftest import constant_guess
    xg, ug, p = constant_guess(solver.problem, x0)
    x = x0.copy()
    B = len(x0)
    worst, umax, status = np.zeros(B), np.zeros(B), []
    for _ in range(steps):
        xg[:, 0] = x
        xg = np.asarray(solver.guess_correction(xg, ug))
        xs, us, st, _ = solver.solve(x, xg, ug, p)
        xs, us, st = np.asarray(xs), np.asarray(us), np.asarray(st)
        xn, ue = solver.plant_step(x, us[:, 0], plant_tables)
        worst = np.maximum(worst, np.abs(np.asarray(ue) - us[:, 0]).max(1))
        umax = np.maximum(umax, np.abs(us[:, 0]).max(1))
        status.append(st.copy())
        xg, ug, _ = solver.provide_control(np.ones(B, np.int32), xs, us, xg, ug)
        xg, ug = np.asarray(xg), np.asarray(ug)
        x = np.asarray(xn)
    return worst, umax, np.array(status)


def oracle_factories(par, N, solver_cls=None):
    """make_controller / make_backup of run_mpc around ``solver_cls(prob, net)`` (default ModelOracleSolver): the policy layer on
    host state over the CPU oracle"""
    from safe_mpc_amd import controller as C
    solver_cls = solver_cls or ModelOracleSolver

    def build(cls, name, cost, horizon, batch):
        ctrl = cls.__new__(cls)
        prob = C.OcpProblem(par, name, cost, N=horizon)
        net = C.SafeSetNet.from_params(par, prob.x_min, prob.x_max)
        prob.set_normalisation(net.mean, net.std)
        C.AbstractController.__init__(ctrl, par, batch, cost, horizon, solver=solver_cls(prob, net), net=net)
        return ctrl
    return (lambda name, batch: build(C.CONTROLLERS[name], C.CONTROLLERS[name].cont_name, 'ext', N, batch),
            lambda batch: build(C.SafeBackupController, 'backup', 'zero', par.back_hor, batch))
