"""Test helpers for ParallelController (controller.py:567-644 of the reference): a CPU double of the class on the oracle, a solver
wrapper that makes chosen candidates fail, a scalar safe-set rule, and a literal one-instance transcription of the reference's
``step`` to compare the batched class with.  Lives under tests/: the product never imports it."""
import numpy as np

from fake_solver import OracleSolver


def switched_node(p_row):
    """the node n whose row a candidate switches on (constrain_n: p[n][4] = +1, every other node of 1..N at -1), or None"""
    on = np.flatnonzero(np.asarray(p_row)[1:, 4] > 0) + 1
    return int(on[0]) if len(on) == 1 else None


class CandidateFailSolver(OracleSolver):
    """The oracle with scripted failures: instance b's candidate fails (status 4) whenever its switched node is in
    ``fail_nodes(step, b)``.  Instances are recognised by their x0 among the rows of ``x_cur`` (set before every step), so the batched
    class (B * N rows per solve) and the scalar transcription (one row per solve) see the same failures."""

    def __init__(self, problem, net=None):
        super().__init__(problem, net)
        self.x_cur, self.step_no, self.fail_nodes = None, 0, None

    def solve(self, x0, xg, ug, p, out=None):
        x, u, st, it = super().solve(x0, xg, ug, p, out)
        st = np.array(st, np.int32)
        if self.fail_nodes is not None and self.x_cur is not None:
            x0, p = np.asarray(x0), np.asarray(p)
            for i in range(len(st)):
                hit = np.flatnonzero(np.all(self.x_cur == x0[i], axis=1))
                n = switched_node(p[i])
                if len(hit) and n is not None and n in self.fail_nodes(self.step_no, int(hit[0])):
                    st[i] = 4
        return x, u, st, it


SAFE_MODE = ['rule']     # 'rule': safe_rule below; 'none': no state is safe (a step on which only the min(n, r) branch can succeed)


def safe_rule(x):
    """a scripted safe-set verdict, a pure function of the node's state, so that both statements see the same answers"""
    if SAFE_MODE[0] == 'none':
        return False
    return bool(np.sin(37.0 * x[0] + 11.0 * x[1]) > -0.2)


def vec_safe(x):
    x = np.asarray(x, float)
    flat = x.reshape(-1, x.shape[-1])
    return np.array([safe_rule(v) for v in flat]).reshape(x.shape[:-1])


def make_parallel_double(params, batch, N=None, solver_cls=CandidateFailSolver):
    """ParallelController around the CPU oracle (make_double_controller of fake_solver.py for the unregistered class)"""
    from safe_mpc_amd import controller as C
    from safe_mpc_amd.safe_set import SafeSetNet
    cls = C.ParallelController
    N = int(N if N is not None else params.N)
    prob = C.OcpProblem(params, cls.cont_name, 'ext', N=N)
    net = SafeSetNet.from_params(params, prob.x_min, prob.x_max)
    prob.set_normalisation(net.mean, net.std)
    ctrl = cls.__new__(cls)
    C.AbstractController.__init__(ctrl, params, batch, 'ext', N, solver=solver_cls(prob, net), net=net)
    return ctrl


class ScalarParallel:
    """ParallelController of the reference for ONE instance, transcribed line by line (controller.py:567-612 and 614-644, with solve
    :136-167 and provideControl :169-184).  ``solver`` solves one instance per call (BatchedOcpSolver interface, B = 1);
    ``check_state(x_traj)`` / ``check_safe(x_node)`` are checkStateConstraints / checkSafeConstraints of one instance."""

    def __init__(self, N, params, solver, check_state, check_safe, x_guess, u_guess, ee_ref):
        self.N, self.params, self.solver = N, params, solver
        self.check_state, self.check_safe_node = check_state, check_safe
        self.x_guess, self.u_guess = np.array(x_guess, float), np.array(u_guess, float)
        self.x_temp, self.u_temp = np.copy(self.x_guess), np.copy(self.u_guess)
        self.x_viable = np.copy(self.x_guess[-1])          # STWAController.setGuess (controller.py:390-393)
        self.fails, self.current_step, self.r = 0, 0, N
        self.last_status, self.qp_iter = 4, 0
        # the solver's per-node parameters: they persist between solves, as acados' do
        self.p_solver = np.zeros((N + 1, 5))
        self.p_solver[:, :3] = ee_ref
        self.p_solver[:, 3] = params.alpha
        self.p_solver[:, 4] = 1.0
        self.constraints = np.linspace(1, self.N, self.N).round().astype(int).tolist()

    def guessCorrection(self):
        self.x_guess = np.asarray(self.solver.guess_correction(self.x_guess[None].copy(), self.u_guess[None]))[0]

    def constrain_n(self, n_constr):
        self.p_solver[n_constr, 4] = 1.0
        for i in range(1, self.N + 1):
            if i != n_constr:
                self.p_solver[i, 4] = -1.0

    def solve(self, x0):
        self.p_solver[:, 3] = self.params.alpha
        x, u, st, it = self.solver.solve(np.asarray(x0, float)[None], self.x_guess[None], self.u_guess[None], self.p_solver[None].copy())
        self.x_temp, self.u_temp = np.array(x[0]), np.array(u[0])
        self.last_status, self.qp_iter = int(st[0]), int(it[0])
        return self.last_status

    def check_safe_n(self):
        r = 0
        for i in range(self.r, self.N + 1):
            if self.check_safe_node(self.x_temp[i]):
                r = i
        return r

    def sing_step(self, x, n_constr):
        success = False
        constr_ver = 0
        self.constrain_n(n_constr)
        status = self.solve(x)
        checked_r = self.check_safe_n()
        if status == 0:
            constr_ver = checked_r if checked_r >= self.r else min(n_constr, self.r)
            if (constr_ver - self.r >= 0) and self.check_state(self.x_temp):
                success = True
        return constr_ver if success else 0

    def provideControl(self):
        if self.fails > 0:
            u = self.u_guess[0]
            self.x_guess = np.roll(self.x_guess, -1, axis=0)
            self.u_guess = np.roll(self.u_guess, -1, axis=0)
        else:
            u = self.u_temp[0]
            self.x_guess = np.roll(self.x_temp, -1, axis=0)
            self.u_guess = np.roll(self.u_temp, -1, axis=0)
        self.x_guess[-1] = np.copy(self.x_guess[-2])
        self.u_guess[-1] = np.copy(self.u_guess[-2])
        return u, False

    def step(self, x):
        self.guessCorrection()
        node_success = 0
        self.chosen = None
        for i in reversed(self.constraints):
            result = self.sing_step(x, i)
            if result > node_success:
                node_success = result
                self.chosen = i
                tmp_x = np.copy(self.x_temp)
                tmp_u = np.copy(self.u_temp)
                if result == self.N:
                    break
        self.node_success = node_success
        if node_success > 1:
            self.r = node_success
            self.x_temp = tmp_x
            self.u_temp = tmp_u
            self.fails = 0
        else:
            self.fails += 1
            if self.r == 1:
                self.x_viable = np.copy(self.x_guess[1])
                self.r = self.N
                return np.copy(self.u_guess[0]), True
        self.r -= 1
        self.current_step += 1
        return self.provideControl()
