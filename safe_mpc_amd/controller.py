"""Batched mirrors of the reference's controller classes (src/safe_mpc/controller.py:251-712).

Same class names, same method names (``initialize``, ``step``, ``setGuess``/``getGuess``, ``resetHorizon``,
``reset_controller``, ``getTime``, ``getLastViableState``, ``checkGuess``, ``solve``, ``provideControl``,
``guessCorrection``), same accept / reject / abort automata -- but every piece of per-instance state is an array over
the B instances that the reference walks one at a time (scripts/mpc.py:102).  ``step(x)`` takes ``x[B, nx]`` and returns
``(u[B, nu], abort[B])``.  The numerics all go through ``self.ocp_solver`` (a :class:`BatchedOcpSolver`, i.e. the HIP
engine); this file is pure bookkeeping, so it can be unit-tested with a scripted fake solver.

Two paths, each stated once.  The host path is the numpy statement of each class (``_step_host``, ``provideControl``,
``_set_flags`` / ``_post_solve``), written to be read next to the reference.  A ``device_state=True`` controller never runs it:
its ``step`` is ``step_on_device``, the same automaton as engine kernels (smpc_policy_step), which the GPU tests hold against the
statement.  There is no third path: ``device_state=True`` with a solver that lacks those kernels is refused in the constructor.

Instances whose ``step`` returns ``abort=True`` keep their guess unshifted and their step counter unchanged, exactly
like the early ``return self.u_guess[0], True`` of the reference (controller.py:384-385, 483-487).
"""
from __future__ import annotations

import numpy as np

from ._xp import InPlaceState, NumpyOps, TorchOps
from .problem import OcpProblem
from .safe_set import SafeSetNet


class AbstractController(InPlaceState):
    """``device_state=True`` keeps every per-instance array of the policy (guesses, counters, receding indices, viable states,
    per-node parameters) as ROCm torch tensors and drives the engine through its device-pointer path: ``step`` then enqueues
    kernels only -- no array crosses PCIe and nothing synchronises with the host.  The default (numpy) is the host path."""
    cont_name = 'naive'
    can_abort = False            # policies whose step() may return abort=True (the driver then needs one flag per step)
    policy_kind = 0              # SMPC_POLICY_* of include/smpc.h: which automaton smpc_policy_step runs for this class
    guess_safe_node = False      # checkGuess includes checkSafeConstraints on the last node (STWA and below)

    def __init__(self, params, batch, cost='ext', N=None, solver=None, net=None, device=0, device_state=False):
        self.params = params
        self.B = int(batch)
        self.problem = OcpProblem(params, self.cont_name, cost, N=N)
        self.model = self.problem                      # x_min/x_max/tau_max/ee_ref live here (AdamModel's role)
        self.N = self.problem.N
        self.nx, self.nu, self.nq = self.problem.nx, self.problem.nu, self.problem.nq
        if net is None and params.use_net:
            net = SafeSetNet.from_params(params, self.problem.x_min, self.problem.x_max)
        self.net = net
        if net is not None:
            self.problem.set_normalisation(net.mean, net.std)
        if solver is None:
            from .solver import BatchedOcpSolver
            solver = BatchedOcpSolver(self.problem, net, device=device)
        if device_state and not hasattr(solver, 'policy_step'):
            raise ValueError(f'device_state=True needs a solver with the engine\'s policy kernels (BatchedOcpSolver.policy_step): '
                             f'{type(solver).__name__} has none; the numpy statement runs on host state only')
        self.ocp_solver = solver
        self.xp = TorchOps(device) if device_state else NumpyOps()     # set-up, predicates and results; never a step (_xp.py)
        self.time_fields = ['time_lin', 'time_sim', 'time_qp', 'time_qp_solver_call', 'time_glob', 'time_reg', 'time_tot']
        xp = self.xp
        self._x_min, self._x_max = xp.asarray(self.problem.x_min, xp.f64), xp.asarray(self.problem.x_max, xp.f64)
        self._tau_min, self._tau_max = xp.asarray(self.problem.tau_min, xp.f64), xp.asarray(self.problem.tau_max, xp.f64)
        self._lbx_e, self._ubx_e = xp.asarray(self.problem.lbx_e, xp.f64), xp.asarray(self.problem.ubx_e, xp.f64)
        self._alloc()
        self.reset_controller()
        self._inplace = bool(device_state)       # device mode: state arrays keep their addresses (see _xp.InPlaceState)

    # -- state --------------------------------------------------------------------------------------------------------
    def _alloc(self):
        B, N, xp = self.B, self.N, self.xp
        self.x_guess = xp.zeros((B, N + 1, self.nx))
        self.u_guess = xp.zeros((B, N, self.nu))
        self.x_temp, self.u_temp = xp.copy(self.x_guess), xp.copy(self.u_guess)
        # per-node parameters p = [ee_ref(3), alpha, flag] (controller.py:27-37, 153-156)
        self.p = xp.zeros((B, N + 1, 5))
        self.p[:, :, :3] = xp.asarray(self.problem.ee_ref, xp.f64)
        self.p[:, :, 3] = self.params.alpha
        self.p[:, :, 4] = 1.0
        self.traj = getattr(self, 'traj', None)                    # reference trajectory (setTrajectory); None = constant ee_ref
        self.last_status = xp.full((B,), 4, xp.i32)                # controller.py:125
        self.qp_iter = xp.zeros((B,), xp.i32)
        self.x_viable = xp.zeros((B, self.nx))
        if xp.on_device:       # outputs of the fused device step (smpc_policy_step): fixed addresses, so a step can be graph-captured
            self._u_out = xp.zeros((B, self.nu))
            self._abort_out = xp.full((B,), False, xp.bool_)
            self._any_abort = xp.zeros((1,), xp.i32)

    def reset_controller(self):
        self.fails = self.xp.zeros((self.B,), self.xp.i64)
        self.current_step = self.xp.zeros((self.B,), self.xp.i64)

    def setReference(self, ee_ref):
        self.problem.ee_ref = np.asarray(ee_ref, float)
        self.p[:, :, :3] = self.xp.asarray(self.problem.ee_ref, self.xp.f64)

    def setTrajectory(self, traj):
        """``cost.traj`` of the reference (cost_definition.py:30-31, 89): ``[3, n_steps + 1 + N]`` reference points, of which
        ``solve`` hands node i the column ``current_step + i`` (controller.py:153-156).  ``None`` (the default) = the constant
        ``ee_ref`` of the ReachTarget / Zero costs, for which the indexing changes nothing.

        ``[B, 3, n_columns]`` (tracking.tracking_curves / jittered_curves): a curve of its own for every instance, instance b
        reading ``traj[b]`` the same way.  On a device-backed controller the engine's handle then holds the curves
        (``solver.set_instance_curves``) and the policy step is called without a shared table; going back to ``[3, n_columns]``
        or ``None`` clears them."""
        had_curves = self.traj is not None and self.traj.ndim == 3
        to_engine = self.xp.on_device and hasattr(self.ocp_solver, 'set_instance_curves')
        if traj is None:
            self.traj = None
            self.p[:, :, :3] = self.xp.asarray(self.problem.ee_ref, self.xp.f64)
            if had_curves and to_engine:
                self.ocp_solver.set_instance_curves(None)
            return
        traj = np.ascontiguousarray(traj, float)
        if traj.ndim == 3:
            if traj.shape[0] != self.B or traj.shape[1] != 3 or traj.shape[2] < 1:
                raise ValueError(f'traj must be [3, n_columns] or [{self.B}, 3, n_columns] (one curve per instance of the batch), '
                                 f'got {traj.shape}')
        elif traj.ndim != 2 or traj.shape[0] != 3 or traj.shape[1] < 1:
            raise ValueError('traj must be [3, n_columns]')
        # the reference indexes cost.traj[:, current_step + i] for i <= N over a run of n_steps steps and would raise on a shorter
        # array; here the column index is clamped (the device kernel must not read past the end), so say so instead of silently
        # holding the last point
        need = int(getattr(self.params, 'n_steps', 0)) + 1 + self.N
        if traj.shape[-1] < need:
            import warnings
            warnings.warn(f'setTrajectory: {traj.shape[-1]} columns < n_steps + 1 + N = {need}: the reference would fail with an '
                          'IndexError past the end; this engine holds the last column', RuntimeWarning, stacklevel=2)
        new = self.xp.asarray(traj, self.xp.f64)
        if self.traj is not None and tuple(self.traj.shape) == tuple(new.shape):
            self.traj[...] = new       # in place: a captured step (hipGraph) keeps the device pointer and length it was captured with
        else:
            self.traj = new
            self._traj_rebound = True  # (closed_loop._DeviceGroup drops its captured graphs when it sees this)
        if to_engine and (new.ndim == 3 or had_curves):
            # the handle's copy follows: same (B, L) overwrites the handle's buffer in place, which a captured step keeps reading
            self.ocp_solver.set_instance_curves(self.traj if new.ndim == 3 else None)

    def _apply_traj(self, rows=None):
        """p[b, i, 0:3] = traj[:, current_step[b] + i] (controller.py:153-156)"""
        if self.traj is None:
            return
        xp = self.xp
        col = xp.clip_max(self.current_step[:, None] + xp.arange(self.N + 1)[None, :], self.traj.shape[-1] - 1)    # [B, N+1]
        if self.traj.ndim == 3:                                    # a curve per instance: traj[b, :, col[b, i]]
            ref = xp.swap_last(self.traj[xp.arange(self.B)[None, :, None], xp.arange(3)[:, None, None], col[None]])
        else:
            ref = xp.swap_last(self.traj[:, col])                  # [3, B, N+1] -> [B, N+1, 3]
        if rows is None:
            self.p[:, :, :3] = ref
        else:
            self.p[:, :, :3] = xp.where(rows[:, None, None], ref, self.p[:, :, :3])

    def setGuess(self, x_guess, u_guess):
        self.x_guess = self.xp.asarray(x_guess, self.xp.f64)
        self.u_guess = self.xp.asarray(u_guess, self.xp.f64)

    def getGuess(self):
        return self.xp.copy(self.x_guess), self.xp.copy(self.u_guess)

    def getLastViableState(self):
        return self.xp.copy(self.x_viable)

    def getTime(self):
        """controller.py:192-193: the seven acados timers of the last solve, in seconds (zeros when timing is off)"""
        from .closed_loop import time_row
        try:
            t = self.ocp_solver.timing_history(0) if hasattr(self.ocp_solver, 'timing_history') else self.ocp_solver.timing()
        except Exception:
            t = None
        return np.array(time_row(t)) if t else np.zeros(len(self.time_fields))

    def resetHorizon(self, N):
        """controller.py:205-214: new horizon without re-creating the solver."""
        self.N = int(N)
        self.params.N = self.N
        self.problem.N = self.N
        self.ocp_solver.set_horizon(self.N)
        self._alloc()

    # -- the solve and its neighbours -----------------------------------------------------------------------------------
    def solve(self, x0):
        """controller.py:136-167 for all instances: returns status[B]; x_temp / u_temp hold the iterate regardless."""
        self.p[:, :, 3] = self.params.alpha
        self._apply_traj()
        if not self.xp.on_device:
            x0 = np.asarray(x0, float)
        if self.xp.on_device:     # the engine writes straight into the controller's persistent buffers
            self.ocp_solver.solve(x0, self.x_guess, self.u_guess, self.p, out=(self.x_temp, self.u_temp, self.last_status, self.qp_iter))
            return self.last_status
        x, u, st, it = self.ocp_solver.solve(x0, self.x_guess, self.u_guess, self.p)
        self.x_temp, self.u_temp = np.asarray(x), np.asarray(u)
        self.last_status = np.asarray(st).copy()
        self.qp_iter = np.asarray(it).copy()
        return self.last_status

    def guessCorrection(self):
        self.x_guess = self.ocp_solver.guess_correction(self.x_guess, self.u_guess)

    def provideControl(self, active=None):
        """controller.py:169-184.  ``active`` masks out instances that returned early (abort)."""
        accept = (self.fails == 0).astype(np.int32)
        xg, ug, u = self.ocp_solver.provide_control(accept, self.x_temp, self.u_temp, self.x_guess, self.u_guess)
        if active is None:
            self.x_guess, self.u_guess = xg, ug
        else:
            u = np.where(active[:, None], u, self.u_guess[:, 0])
            self.x_guess = np.where(active[:, None, None], xg, self.x_guess)
            self.u_guess = np.where(active[:, None, None], ug, self.u_guess)
        return u, np.zeros((self.B,), np.bool_)

    # -- feasibility predicates (env_model.py:170-243, safe_set.py:61-68) ------------------------------------------------
    def _as_state(self, x):
        if not self.xp.on_device:
            x = np.asarray(x, float)
        return x[:, None, :] if x.ndim == 2 else x

    def checkStateConstraints(self, x):
        """env_model.py:170-173.  Reference quirk kept by default (``params.reference_quirks``):
        ``checkCollision`` returns inside its loop after the FIRST row (env_model.py:238-243), so a trajectory is
        collision-checked at its first node only, while the box test covers every node."""
        xp = self.xp
        x = self._as_state(x)
        tol = self.params.tol_x
        in_box = xp.all_tail((x >= self._x_min - tol) & (x <= self._x_max + tol))
        xc = x[:, :1] if getattr(self.params, 'reference_quirks', True) else x
        if xp.on_device:
            xc = xc.contiguous()
            free = self.ocp_solver.check_trajectory(xc, tol_x=1e30) != 0
        else:
            free = np.asarray(self.ocp_solver.check_trajectory(np.ascontiguousarray(xc), tol_x=1e30))
        return in_box & free

    def checkSafeConstraints(self, x):
        """x[B, n_nodes, nx] (or [B, nx]) -> bool per (instance, node)."""
        squeeze = x.ndim == 2
        x = self._as_state(x)
        if self.xp.on_device:
            _, nn = self.ocp_solver.check_trajectory(x.contiguous(), want_nn=True)
            nn = nn != 0
        else:
            _, nn = self.ocp_solver.check_trajectory(x, want_nn=True)
            nn = np.asarray(nn)
        return nn[:, 0] if squeeze else nn

    def checkTorqueConstraints(self, x, u):
        ev = self.ocp_solver.eval_nodes(x, u, self.p)
        tau = ev['tau'][:, :self.N, :self.nq]
        tol = self.params.tol_tau
        return self.xp.all_tail((tau >= self._tau_min - tol) & (tau <= self._tau_max + tol))

    def checkDynamicsConstraints(self, x, u):
        """env_model.py:226-234 with the controller's own model (no torque saturation inside the rollout)."""
        sim = self.ocp_solver.guess_correction(self.xp.copy(x), u)       # (the device path integrates in place)
        n = u.shape[1]
        return self.xp.norm_tail(x - sim) < self.params.tol_dyn * np.sqrt(n + 1)

    def checkGuess(self):
        return (self.checkStateConstraints(self.x_temp) & self.checkTorqueConstraints(self.x_temp, self.u_temp) &
                self.checkDynamicsConstraints(self.x_temp, self.u_temp))

    def guess_report(self, mask=None, flags=None, worst=None):
        """``checkGuess`` on x_temp / u_temp as ONE engine call (smpc_check_guess): ``(flags [B], worst [B, 5])``, where
        ``flags == 0`` is checkGuess' verdict and the bits say which predicate failed (BatchedOcpSolver.check_guess)."""
        return self.ocp_solver.check_guess(self.x_temp, self.u_temp, safe_node=self.N if self.guess_safe_node else None,
                                           mask=mask, flags=flags, worst=worst)

    def initialize(self, x0, u0=None):
        """controller.py:260-272: trivial guess, one solve, keep it where it checks out.  Returns 1/0 per instance."""
        xp = self.xp
        x0 = xp.asarray(x0, xp.f64)
        self.x_guess = xp.repeat_nodes(x0, self.N + 1)
        self.u_guess = xp.zeros((self.B, self.N, self.nu)) if u0 is None else xp.repeat_nodes(xp.asarray(u0, xp.f64), self.N)
        status = self.solve(x0)
        good = (status == 0) & self.checkGuess()
        self.x_guess = xp.where(good[:, None, None], self.x_temp, self.x_guess)
        self.u_guess = xp.where(good[:, None, None], self.u_temp, self.u_guess)
        return xp.cast(good, xp.i64)

    def step(self, x):
        """x[B, nx] -> (u[B, nu], abort[B]): the engine kernels for a device-state controller, the class's numpy statement otherwise"""
        if self.xp.on_device:
            return self.step_on_device(x)
        return self._step_host(x)

    def _step_host(self, x):
        raise NotImplementedError

    def step_on_device(self, x, stepping=None, u_other=None, u_out=None):
        """``step`` with the state in HBM: the class's automaton as engine kernels (smpc_policy_step, kernels_policy.hpp) -- the
        numpy ``_step_host`` of each class is the readable statement of the same thing, and the GPU tests run the two side by side.
        ``stepping`` masks out instances that must not step (they are left untouched and get ``u_other``)."""
        return self.ocp_solver.policy_step(self, x, stepping, u_other, u_out)


class NaiveController(AbstractController):
    cont_name = 'naive'

    def _step_host(self, x):
        """controller.py:274-284"""
        self.guessCorrection()
        status = self.solve(x)
        self.fails = (self.fails + 1) * (status != 0).astype(np.int64)      # 0 on success, fails + 1 otherwise
        self.current_step = self.current_step + 1
        return self.provideControl()


class TerminalZeroVelocity(NaiveController):
    cont_name = 'zerovel'


class STController(NaiveController):
    cont_name = 'st'


class STWAController(STController):
    cont_name = 'stwa'
    can_abort = True
    policy_kind = 2
    guess_safe_node = True

    def setGuess(self, x_guess, u_guess):
        super().setGuess(x_guess, u_guess)
        self.x_viable = self.xp.copy(self.x_guess[:, -1])

    def checkGuess(self):
        return super().checkGuess() & self.checkSafeConstraints(self.x_temp[:, -1])

    def _step_host(self, x):
        """controller.py:375-388"""
        self.guessCorrection()
        status = self.solve(x)
        ok = (status == 0) & self.checkStateConstraints(self.x_temp)
        first_fail = ~ok & (self.fails == 0)
        self.x_viable = np.where(first_fail[:, None], self.x_guess[:, -2], self.x_viable)
        abort = ~ok & (self.fails == self.N - 1)
        u_abort = np.copy(self.u_guess[:, 0])
        # ok: 0 ; abort: unchanged ; otherwise fails + 1
        self.fails = np.where(abort, self.fails, self.fails + 1) * (~ok).astype(np.int64)
        active = ~abort
        self.current_step = self.current_step + active.astype(np.int64)
        u, _ = self.provideControl(active)
        return np.where(abort[:, None], u_abort, u), abort


class HTWAController(STWAController):
    cont_name = 'htwa'


class RecedingController(STWAController):
    cont_name = 'receding'
    policy_kind = 3

    def reset_controller(self):
        super().reset_controller()
        self.r = self.xp.full((self.B,), self.N, self.xp.i64)
        self.abort_flag = bool(self.params.abort_flag)

    def resetHorizon(self, N):
        super().resetHorizon(N)
        self.r = self.xp.full((self.B,), self.N, self.xp.i64)

    def _set_flags(self):
        """controller.py:452-469: running nodes off except node r; terminal node always on."""
        k = np.arange(self.N + 1)[None, :]
        r = self.r[:, None]
        on = (k == self.N) | ((k == r) & (r < self.N)) | (k == 0)   # node 0 keeps the default flag (never carries the row anyway)
        self.p[:, :, 4] = on.astype(np.float64) * 2.0 - 1.0

    def _post_solve(self, x, status, u_abort):
        if self.abort_flag:
            self.r = self.r - 1
            abort = self.r == 0
        else:
            self.r = self.r - (self.r > 0).astype(np.int64)
            abort = np.zeros((self.B,), np.bool_)
        self.x_viable = np.where(abort[:, None], self.x_guess[:, 1], self.x_viable)
        self.r = self.r + abort.astype(np.int64) * self.N            # r = 0 -> N for the aborting instances
        ok = (status == 0) & self.checkStateConstraints(self.x_temp) & ~abort
        # r <- largest i-1, i in r+2..N, whose node passes the safe-set test (controller.py:491-494)
        safe = self.checkSafeConstraints(self.x_temp)                      # [B, N+1]
        i = np.arange(self.N + 1)[None, :]
        cand = safe & (i >= (self.r[:, None] + 2))
        best = np.where(cand.any(1), self.N - np.argmax(cand[:, ::-1], axis=1), -1)      # largest such i, -1 if none
        self.r = np.where(ok & (best >= 0), best - 1, self.r)
        # abort: unchanged ; ok: 0 ; otherwise fails + 1
        self.fails = np.where(abort, self.fails, (self.fails + 1) * (~ok).astype(np.int64))
        active = ~abort
        self.current_step = self.current_step + active.astype(np.int64)
        u, _ = self.provideControl(active)
        return np.where(abort[:, None], u_abort, u), abort

    def _step_host(self, x):
        """controller.py:448-498"""
        self.guessCorrection()
        self._set_flags()
        u_abort = np.copy(self.u_guess[:, 0])
        status = self.solve(x)
        return self._post_solve(x, status, u_abort)


class RealReceding(RecedingController):
    """controller.py:504-565: hard terminal safe set; instead of a running safe-set row, node r of each instance is boxed to
    the previously planned state x_guess[r+1] +- 1e-3 (per-instance stage bounds in the engine).  No guessCorrection."""
    cont_name = 'real_receding'
    policy_kind = 4
    TUBE = 1e-3

    def _alloc(self):
        super()._alloc()
        if self.xp.on_device:      # the bounds away from node r (:534-536): model bounds, the terminal node its own
            xp = self.xp
            self._stage_lo = xp.asarray(np.vstack([np.tile(self.problem.x_min, (self.N, 1)), self.problem.lbx_e[None, :]]), xp.f64)
            self._stage_hi = xp.asarray(np.vstack([np.tile(self.problem.x_max, (self.N, 1)), self.problem.ubx_e[None, :]]), xp.f64)

    def _step_host(self, x):
        """controller.py:524-565"""
        N = self.N
        # other nodes: the model bounds (:534-536); the terminal node keeps lbx_e / ubx_e
        k = np.arange(N + 1)[None, :, None]
        last = k == N
        lo = np.where(last, self._lbx_e[None, None, :], self._x_min[None, None, :])
        hi = np.where(last, self._ubx_e[None, None, :], self._x_max[None, None, :])
        sel = self.r < N
        centre = self.x_guess[np.arange(self.B), np.minimum(self.r, N - 1) + 1][:, None, :]     # x_guess[b, r_b + 1]
        at_r = (k == self.r[:, None, None]) & sel[:, None, None]
        lo = np.where(at_r, centre - self.TUBE, lo + 0.0 * centre)      # (+ 0 * centre: broadcast to [B, N+1, nx])
        hi = np.where(at_r, centre + self.TUBE, hi + 0.0 * centre)
        self.ocp_solver.set_instance_bounds(lo, hi)
        u_abort = np.copy(self.u_guess[:, 0])
        status = self.solve(x)
        return self._post_solve(x, status, u_abort)


class ParallelController(RecedingController):
    """controller.py:567-644: every step solves N candidate OCPs from the same corrected guess -- candidate n (n = N .. 1) with the
    hard safe-set row switched on at node n alone (constrain_n, :578-587: all other nodes of 1..N off, the terminal node included
    unless n = N) -- and keeps the one whose trajectory reaches the furthest safe node (sing_step / check_safe_n, :589-612).  The
    reference solves them one after another; here they are one batch of B * N instances (numpy path) or, on the device, candidate
    N for every instance followed by the other N - 1 for the instances it did not settle (smpc_policy_step, kernels_policy.hpp).
    acados is assumed to keep no state between the candidate solves (exact_hess_constr = 0, :110; reset() in solve, :141)
    [EXT-UNVERIFIED].  The reference's get_controller table (utils.py:64-75) does not list this class: get_controller finds it in
    UNREGISTERED_CONTROLLERS."""
    cont_name = 'parallel'
    policy_kind = 5
    can_abort = True

    def candidate_flags(self):
        """[N, N+1] p[4] of candidate n = N, N-1, .., 1 (row c is candidate N - c); node 0 keeps the instance's own flag"""
        N = self.N
        k, n = np.arange(N + 1)[None, :], np.arange(N, 0, -1)[:, None]
        return np.where(k == n, 1.0, -1.0)

    def _step_host(self, x):
        """controller.py:614-640 with every candidate evaluated: the choice is the one the reference's loop (order N .. 1, break at
        the first result N) makes; status / qp_iter (and x_temp / u_temp on failure) are those of the last candidate it solves"""
        B, N, nx, nu = self.B, self.N, self.nx, self.nu
        self.guessCorrection()
        xg, ug = np.asarray(self.x_guess), np.asarray(self.u_guess)
        u_abort, xg1 = ug[:, 0].copy(), xg[:, 1].copy()          # (taken after guessCorrection, :615-616, 636)
        # what solve() writes into the instance's own parameters (controller.py:153-156); the flags stay the instance's
        self.p[:, :, 3] = self.params.alpha
        self._apply_traj()
        # the B * N candidates, instance-major: candidate c of instance b is row b * N + c, c = N - n
        P = np.repeat(np.asarray(self.p)[:, None], N, axis=1)                      # [B, N, N+1, 5]
        P[:, :, 1:, 4] = self.candidate_flags()[None, :, 1:]
        rep = lambda a: np.ascontiguousarray(np.repeat(a[:, None], N, axis=1).reshape((B * N,) + a.shape[1:]))
        xs, us, st, it = self.ocp_solver.solve(rep(np.asarray(x, float)), rep(xg), rep(ug), P.reshape(B * N, N + 1, 5))
        xs, us = np.asarray(xs).reshape(B, N, N + 1, nx), np.asarray(us).reshape(B, N, N, nu)
        st, it = np.asarray(st).reshape(B, N), np.asarray(it).reshape(B, N)
        state_ok = np.asarray(self.checkStateConstraints(xs.reshape(B * N, N + 1, nx))).reshape(B, N)
        safe = np.asarray(self.checkSafeConstraints(xs.reshape(B * N, N + 1, nx))).reshape(B, N, N + 1)
        # sing_step / check_safe_n (:589-612) with r at the start of the step
        r = np.asarray(self.r)[:, None]                                               # [B, 1]
        i = np.arange(N + 1)
        in_range = safe & (i[None, None, :] >= r[:, :, None])
        checked = np.where(in_range.any(axis=2), N - np.argmax(in_range[:, :, ::-1], axis=2), 0)    # last safe node of r..N, else 0
        ns = np.arange(N, 0, -1)[None, :]
        constr_ver = np.where(checked >= r, checked, np.minimum(ns, r))
        result = np.where((st == 0) & (constr_ver >= r) & state_ok, constr_ver, 0)   # [B, N], candidates in the order N .. 1
        self.candidate_results = result            # (kept for diagnostics: result[:, 0] == N is what the device schedule settles first)
        # selection (:614-624): the largest result, ties to the first candidate in that order (the largest n)
        best = result.max(axis=1)
        chosen = np.argmax(result, axis=1)
        last = np.where(best == N, chosen, N - 1)        # the loop broke at the chosen candidate, or ran down to candidate 1
        success = best > 1
        pick = np.where(success, chosen, last)
        rows = np.arange(B)
        self.x_temp, self.u_temp = xs[rows, pick].copy(), us[rows, pick].copy()
        self.last_status = st[rows, last].astype(np.int32)
        self.qp_iter = it[rows, last].astype(np.int32)
        # automaton (:625-640); the abort returns before r -= 1, the step count and provideControl
        r = r[:, 0]
        abort = ~success & (r == 1)
        self.x_viable = np.where(abort[:, None], xg1, self.x_viable)
        self.fails = np.where(success, 0, self.fails + 1).astype(np.int64)
        self.r = np.where(success, best - 1, np.where(abort, N, r - 1)).astype(np.int64)
        active = ~abort
        self.current_step = self.current_step + active.astype(np.int64)
        u, _ = self.provideControl(active)
        return np.where(abort[:, None], u_abort, u), abort


class ControllerSafeSetEverywhere(STController):
    cont_name = 'constraint_everywhere'
    policy_kind = 1

    def _step_host(self, x):
        """controller.py:651-661"""
        self.guessCorrection()
        status = self.solve(x)
        ok = (status == 0) & self.checkStateConstraints(self.x_temp)
        self.fails = (self.fails + 1) * (~ok).astype(np.int64)
        self.current_step = self.current_step + 1
        return self.provideControl()


class SafeBackupController(AbstractController):
    """controller.py:692-712: zero cost, terminal zero velocity, horizon back_hor; only ``solve`` is used (mpc.py:177)."""
    cont_name = 'backup'

    def __init__(self, params, batch, N=None, **kw):
        super().__init__(params, batch, cost='zero', N=N if N is not None else params.back_hor, **kw)


CONTROLLERS = {'naive': NaiveController, 'zerovel': TerminalZeroVelocity, 'st': STController, 'stwa': STWAController,
               'htwa': HTWAController, 'receding': RecedingController, 'real_receding': RealReceding,
               'constraint_everywhere': ControllerSafeSetEverywhere}


# complete in the reference's controller.py but missing from its get_controller table (utils.py:64-75); scripts/run_all_mpc.sh:12 runs it
UNREGISTERED_CONTROLLERS = {'parallel': ParallelController}


def get_controller(cont_name, params, batch, **kw):
    """utils.py:64-75, and the classes of UNREGISTERED_CONTROLLERS"""
    cls = CONTROLLERS.get(cont_name, UNREGISTERED_CONTROLLERS.get(cont_name))
    if cls is None:
        raise ValueError(f'Controller {cont_name} not available')
    return cls(params, batch, **kw)
