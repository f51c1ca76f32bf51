"""``BatchedOcpSolver``: Python face of the HIP engine (include/smpc.h) -- what ``self.ocp_solver`` is in the reference
(an ``acados_template.AcadosOcpSolver``, controller.py:247), but for B instances per call.

Inputs may be numpy arrays (host path: copied in and out by the engine, synchronous) or ROCm torch tensors
(device path: the engine only gets ``data_ptr()``s and enqueues on its own stream; call :meth:`sync`).
PyTorch is used for device memory only.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import sys

import numpy as np

from . import _lib
from .problem import FIT_MARGIN_CAP, FORECAST_MODES, KALMAN_REC, JOINT_DTYPE, NODE_EVAL_DTYPE, SCENE_ROW, OcpProblem     # noqa: F401 (FORECAST_MODES: re-exported)


# columns of BatchedOcpSolver.score_rollout's two results (SMPC_SCORE_ND doubles, SMPC_SCORE_NI int32 of include/smpc.h)
SCORE_SLOTS = ('cost', 'ee_err2', 'u2', 'ee_dist', 'coll_margin', 'box_margin', 'safe_min')
SCORE_INDEX_SLOTS = ('coll_step', 'coll_row', 'box_step', 'safe_step')
SCORE_ND, SCORE_NI = len(SCORE_SLOTS), len(SCORE_INDEX_SLOTS)


def _is_torch(a):
    return type(a).__module__.startswith('torch')


def pad_hidden_units(Ws, bs, to=256):
    """Weights [out, in] and biases of an MLP whose hidden width the engine's network kernels do not take (not a multiple of 64: a
    small fitted net, safe_set_data.fit_safe_set) with zero units added up to a multiple of ``to``, the width the one-kernel pass is
    built for; any other net as given.  A unit with zero weights and bias outputs act(0) = 0 for every activation on offer and feeds
    zero weights, so the value and the input gradient are those of the net as given."""
    n, H = len(Ws), Ws[0].shape[0]
    if n < 2 or H % 64 == 0 or any(w.shape[0] != H for w in Ws[:-1]):
        return Ws, bs
    Hp = -(-H // to) * to
    Wo, bo = [], []
    for l in range(n):
        rows, cols = (Hp if l < n - 1 else Ws[l].shape[0]), (Hp if l > 0 else Ws[l].shape[1])
        W = np.zeros((rows, cols), np.float32)
        W[:Ws[l].shape[0], :Ws[l].shape[1]] = Ws[l]
        b = np.zeros(rows, np.float32)
        b[:bs[l].shape[0]] = bs[l]
        Wo.append(W)
        bo.append(b)
    return Wo, bo


class BatchedOcpSolver:
    def __init__(self, problem: OcpProblem, net=None, device=0):
        self.problem = problem
        self.L = _lib.lib()
        self.device = int(device)
        h = C.c_void_p()
        rc = self.L.smpc_create(C.byref(problem.desc), self.device, C.byref(h))
        if rc != 0:
            raise _lib.EngineError(f'smpc_create failed ({rc}): {self.L.smpc_last_error(None).decode()}')
        self.h = h
        self.nq, self.nx, self.nu = problem.nq, problem.nx, problem.nu
        self.N = problem.N
        self.net = None
        if net is not None:
            self.set_mlp(net)

    # -- lifetime ------------------------------------------------------------------------------------------------------
    def close(self):
        if getattr(self, 'h', None):
            self.L.smpc_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise _lib.EngineError(f'engine error {rc}: {self.L.smpc_last_error(self.h).decode()}')

    @contextlib.contextmanager
    def _ordered(self, dev):
        """Stream contract of the device path ("Streams"): the engine enqueues on its OWN non-blocking
        stream, torch on its current stream.  On entry the engine's stream waits for everything already enqueued on
        torch's current stream (inputs produced / buffers zero-filled by torch kernels); on exit torch's current stream
        waits for the engine's work, so later torch ops -- and the caching allocator's reuse of temporaries freed after
        the call -- are ordered behind it.  No host synchronisation.  A caller that already runs under
        ``torch.cuda.stream(ExternalStream(smpc_stream))`` (bench.py) pays nothing."""
        if not dev:
            yield
            return
        import torch
        if getattr(self, '_ext_stream', None) is None:
            self._ext_stream = torch.cuda.ExternalStream(self.L.smpc_stream(self.h), device=torch.device('cuda', self.device))
        cur = torch.cuda.current_stream(self.device)
        same = cur.cuda_stream == self._ext_stream.cuda_stream
        if not same:
            self._ext_stream.wait_stream(cur)
        try:
            yield
        finally:
            if not same:
                cur.wait_stream(self._ext_stream)

    def set_mlp(self, net, ctx_default=None):
        """net: SafeSetNet (weights as numpy fp32) -- or anything with .weights/.biases lists of [out, in] / [out].

        A net with a context (``net.n_ctx > 0``): the state columns of ``weights[0]`` go through smpc_set_mlp,
        the last ``n_ctx`` columns through smpc_set_mlp_context with the net's ``ctx_mean`` / ``ctx_std``.  ``ctx_default [n_ctx]`` is
        the context of every row while no instance context is set (:meth:`set_instance_context`): unless given, the shared scene's
        (``problem.context_default(net.ctx_select)``), or ``ctx_mean`` for a net that does not say where its context comes from.

        The engine's network kernels take hidden widths that are multiples of 64 (smpc_set_mlp refuses any other).  A net of another
        width -- a small one from safe_set_data.fit_safe_set -- is handed over with ZERO UNITS ADDED up to the next multiple of 256
        (:func:`pad_hidden_units`): same value and gradient, but the network pass then costs what a 256-wide net costs, up to 64
        times the arithmetic of a 32-wide one.  ``self.net`` keeps the net as given; fit with a width the engine takes where the
        pass's cost matters."""
        Ws = [np.ascontiguousarray(w, np.float32) for w in net.weights]
        bs = [np.ascontiguousarray(b, np.float32) for b in net.biases]
        n = len(Ws)
        n_ctx = int(getattr(net, 'n_ctx', 0))
        Wc = np.ascontiguousarray(Ws[0][:, Ws[0].shape[1] - n_ctx:]) if n_ctx else None
        if n_ctx:
            Ws[0] = np.ascontiguousarray(Ws[0][:, :Ws[0].shape[1] - n_ctx])
        Ws, bs = pad_hidden_units(Ws, bs)
        dims = np.array([Ws[0].shape[1]] + [w.shape[0] for w in Ws], np.int32)
        Wp = (C.c_void_p * n)(*[w.ctypes.data for w in Ws])
        bp = (C.c_void_p * n)(*[b.ctypes.data for b in bs])
        self._chk(self.L.smpc_set_mlp(self.h, n, dims.ctypes.data_as(C.POINTER(C.c_int32)), Wp, bp, 0))
        act = getattr(net, 'act', 'gelu')
        from .safe_set import SafeSetNet
        self._chk(self.L.smpc_set_mlp_activation(self.h, SafeSetNet.ACT_CODES[act]))      # SMPC_ACT_* (parser.py:95-102)
        if n_ctx:
            Wcp = np.zeros((Ws[0].shape[0], n_ctx), np.float32)       # (zero rows for the zero units pad_hidden_units added)
            Wcp[:Wc.shape[0]] = Wc
            if ctx_default is None:
                sel = getattr(net, 'ctx_select', None)
                ctx_default = self.problem.context_default(sel) if sel else net.ctx_mean
            cm, cs, cd = (np.ascontiguousarray(a, np.float64).reshape(-1) for a in (net.ctx_mean, net.ctx_std, ctx_default))
            if cm.shape != (n_ctx,) or cs.shape != (n_ctx,) or cd.shape != (n_ctx,):
                raise ValueError(f'set_mlp: ctx_mean, ctx_std and ctx_default must have {n_ctx} entries')
            self._chk(self.L.smpc_set_mlp_context(self.h, n_ctx, Wcp.ctypes.data, cm.ctypes.data, cs.ctypes.data, cd.ctypes.data, 0))
        self.net = net

    def set_instance_context(self, ctx=None):
        """The context of every instance for a net that has one (smpc_set_instance_context): ``ctx [B, n_ctx]`` float64, the raw
        numbers (``problem.scene_context(geom, net.ctx_select)``), a numpy array or a contiguous ROCm tensor; the engine keeps a
        normalised fp32 copy.  None clears it: every row then takes the default context again.  While set, every call that runs the
        network must come with the same B; the parallel policy and :meth:`rollout` refuse it.  The engine does not derive it from
        :meth:`set_instance_scene`: set and clear the two together."""
        n_ctx = int(getattr(self.net, 'n_ctx', 0)) if self.net is not None else 0
        if ctx is not None and (ctx.ndim != 2 or (n_ctx and ctx.shape[1] != n_ctx)):
            raise ValueError(f'set_instance_context: expected [B, {n_ctx}], got {tuple(ctx.shape)}')
        self._set_instance(self.L.smpc_set_instance_context, 'set_instance_context', [ctx], None if ctx is None else ctx.shape[1:])

    def set_instance_context_track(self, ctx=None):
        """A context that follows a scene track (smpc_set_instance_context_track): ``ctx [B, T, n_ctx]`` float64,
        the raw numbers of every (instance, time column) -- ``problem.scene_context(track, net.ctx_select)`` -- a numpy array or a
        contiguous ROCm tensor; the engine keeps a normalised fp32 copy (4 B x n_ctx x T x B).  The network row of node k reads
        column ``clip(t + k, 0, T - 1)``, t = the scene clock (:meth:`set_scene_clock`; 0 without one), state j of a score_rollout
        log column ``clip(j, 0, T - 1)``: the scene track's rule with this table's own T.  A context and a context track are one
        slot: setting one replaces the other, and None (here or in :meth:`set_instance_context`) clears both."""
        n_ctx = int(getattr(self.net, 'n_ctx', 0)) if self.net is not None else 0
        T = 1
        if ctx is not None:
            if ctx.ndim != 3 or (n_ctx and ctx.shape[2] != n_ctx):
                raise ValueError(f'set_instance_context_track: expected [B, T, {n_ctx}], got {tuple(ctx.shape)}')
            T = int(ctx.shape[1])
            if T < 1:
                raise ValueError('set_instance_context_track: a track has at least one time column')
        self._set_instance(self.L.smpc_set_instance_context_track, 'set_instance_context_track', [ctx],
                           None if ctx is None else ctx.shape[1:], T)

    QP_MODES = {'auto': -1, 'throughput': 0, 'latency': 1}

    def set_qp_mode(self, mode):
        """Which form of the QP solve this handle launches (smpc_set_qp_mode): 'auto' (by batch size), 'throughput' (k_qp_ipm, a
        wavefront per two instances) or 'latency' (k_qp_ipm_wg, a workgroup per instance).  Same result to rounding."""
        self._chk(self.L.smpc_set_qp_mode(self.h, self.QP_MODES[mode] if isinstance(mode, str) else int(mode)))

    def set_qp_crew(self, fraction=1.0, waves=0):
        """Wavefronts of a k_qp_ipm launch (smpc_set_qp_crew): ``fraction`` of its pairs of instances, or exactly ``waves`` of them.
        The crew takes the pairs longest-first from a ticket; results do not depend on it."""
        self._chk(self.L.smpc_set_qp_crew(self.h, float(fraction), int(waves)))

    def set_horizon(self, N):
        self._chk(self.L.smpc_set_horizon(self.h, int(N)))
        self.N = int(N)
        self._rowb_B = 0            # (the engine drops the row-bounds table with the horizon)

    def set_stage_bounds(self, lo=None, hi=None):
        if lo is None:
            self._chk(self.L.smpc_set_stage_bounds(self.h, None, None))
            return
        lo = np.ascontiguousarray(lo, np.float64)
        hi = np.ascontiguousarray(hi, np.float64)
        assert lo.shape == (self.N + 1, self.nx) and hi.shape == lo.shape
        self._chk(self.L.smpc_set_stage_bounds(self.h, lo.ctypes.data, hi.ctypes.data))

    def set_slack_weights(self, zl=None):
        """cost_set(k, 'zl', v) for every node at once (controller.py:455-468): zl[N+1], None restores the formulation's."""
        if zl is None:
            self._chk(self.L.smpc_set_slack_weights(self.h, None))
            return
        zl = np.ascontiguousarray(zl, np.float64)
        assert zl.shape == (self.N + 1,)
        self._chk(self.L.smpc_set_slack_weights(self.h, zl.ctypes.data))

    def set_instance_bounds(self, lo=None, hi=None):
        """Per-instance stage bounds [B, N+1, nx] (RealReceding's state tube, controller.py:530-536); None clears."""
        self._set_instance(self.L.smpc_set_instance_bounds, 'set_instance_bounds', [None, None] if lo is None else [lo, hi],
                           (self.N + 1, self.nx))

    def set_instance_row_bounds(self, lo=None, hi=None):
        """The collision rows' bounds per instance and node (smpc_set_instance_row_bounds): ``lo``, ``hi``
        ``[B, N+1, n_rows]`` -- ``problem.inflated_row_bounds`` forms them from a margin in metres -- as numpy arrays or contiguous
        ROCm float64 tensors; the engine keeps a copy.  Entry (b, k, r) replaces ``row_lb[r]`` / ``row_ub[r]`` at node k of instance b
        in the QP's rows and the merit's violation (solve, sqp, merit_terms, policy_step's solve); a value with |v| >= 1e5 is an
        absent side.  The tests against check bounds (check_trajectory, check_guess, score_rollout, loop_post) do not read it.  None
        clears it, and so does :meth:`set_horizon`.  While set, the calls that read it must come with the same B; the parallel policy
        and :meth:`rollout` refuse it."""
        self._set_instance(self.L.smpc_set_instance_row_bounds, 'set_instance_row_bounds', [None, None] if lo is None else [lo, hi],
                           (self.N + 1, int(self.problem.desc.n_rows)))
        self._rowb_B = 0 if lo is None else int(lo.shape[0])

    def get_instance_row_bounds(self, device=False, B=None):
        """``(lo, hi)``, each ``[B, N+1, n_rows]``: the row-bounds table as the slot holds it (smpc_get_instance_row_bounds), whoever
        filled it -- :meth:`set_instance_row_bounds` or :meth:`forecast_row_margin`.  numpy arrays (the call waits for the copy), or
        ROCm tensors with ``device=True`` (stream-ordered).  ``B``: the table's batch size, the one this solver set it with unless
        given.  The engine refuses while no table is set."""
        B = int(getattr(self, '_rowb_B', 0) if B is None else B)
        shape = (max(B, 1), self.N + 1, int(self.problem.desc.n_rows))
        if device:
            import torch
            lo, hi = (torch.empty(shape, dtype=torch.float64, device=torch.device('cuda', self.device)) for _ in range(2))
            with self._ordered(True):
                self._chk(self.L.smpc_get_instance_row_bounds(self.h, max(B, 1), lo.data_ptr(), hi.data_ptr(), 1))
            return lo, hi
        lo, hi = np.empty(shape), np.empty(shape)
        with self._ordered('torch' in sys.modules):
            self._chk(self.L.smpc_get_instance_row_bounds(self.h, max(B, 1), lo.ctypes.data, hi.ctypes.data, 0))
        return lo, hi

    def set_instance_scene(self, geom=None):
        """A scene of its own for every instance (smpc_set_instance_scene): ``geom [B, n_rows, 8]`` -- per (instance, row) the
        world-fixed element's C[3], D[3], offset, 0, as ``OcpProblem.row_geometry`` / ``scene`` / ``jittered_scenes`` lay it out --
        as a numpy array or a contiguous ROCm float64 tensor; the engine keeps a copy.  None clears it.  While set, every call that
        evaluates collision rows uses it and must come with the same B; the parallel policy and :meth:`rollout` refuse it."""
        self._set_instance(self.L.smpc_set_instance_scene, 'set_instance_scene', [geom], (len(self.problem.rows), SCENE_ROW))

    def _set_track(self, fn, name, geom):
        """what the three track setters share: ``geom`` is None (clears the slot) or ``[B, T >= 1, n_rows, 8]``"""
        T = 1
        if geom is not None:
            if geom.ndim != 4:
                raise ValueError(f'{name}: expected [B, T, n_rows, {SCENE_ROW}], got {tuple(geom.shape)}')
            T = int(geom.shape[1])
            if T < 1:
                raise ValueError(f'{name}: a track has at least one time column')
        self._set_instance(fn, name, [geom], (T, len(self.problem.rows), SCENE_ROW), T)

    def set_instance_scene_track(self, geom=None):
        """Obstacles that move along the horizon (smpc_set_instance_scene_track): ``geom [B, T, n_rows, 8]``, one scene of
        :meth:`set_instance_scene`'s layout per (instance, time column) -- ``OcpProblem.scene_track`` / ``moving_scenes`` -- as a
        numpy array or a contiguous ROCm float64 tensor; the engine keeps a copy (64 B x n_rows x T x B).  Node k of a call is
        formed in column ``clip(t + k, 0, T - 1)``, t = the scene clock (:meth:`set_scene_clock`; 0 without one); the table of
        include/smpc.h says it for every entry point.  A track and a scene are one slot: setting one replaces the other, and None
        (here or in ``set_instance_scene``) clears both."""
        self._set_track(self.L.smpc_set_instance_scene_track, 'set_instance_scene_track', geom)

    def set_instance_world_track(self, geom=None):
        """The WORLD of every instance (smpc_set_instance_world_track): ``geom [B, T, n_rows, 8]``, a scene
        track's layout, as a numpy array or a contiguous ROCm float64 tensor; the engine keeps a copy.  Only :meth:`forecast_scene`
        and the plant's outcome test of :meth:`loop_post` read it -- the controller plans in the scene slot, which a forecast
        fills.  None clears it, and with it a forecast in the scene slot and a context that the forecast wrote."""
        self._set_track(self.L.smpc_set_instance_world_track, 'set_instance_world_track', geom)
        self._world_B = 0 if geom is None else int(geom.shape[0])

    def _forecast(self, fn, select, B, *ints):
        """what the three forecast entry points share, for ``fn(h, B, *ints, n_sel, select)``.  Ordered like a device-path call wherever
        torch is in play: the clock cell is the caller's to write on torch's stream, and a capture on torch's stream must see the launch"""
        sel = np.ascontiguousarray([] if select is None else select, np.int32).reshape(-1, 2)
        B = int(getattr(self, '_world_B', 0) if B is None else B)
        with self._ordered('torch' in sys.modules):
            self._chk(fn(self.h, B, *ints, len(sel), sel.ctypes.data if len(sel) else None))

    def forecast_scene(self, mode, select=None, B=None):
        """The horizon's N + 1 scenes as forecast from the world at the scene clock, into the scene slot (smpc_forecast_scene;
        ``problem.forecast_statement`` is its definition): ``mode`` 'hold', 'cv' or 'true' (``FORECAST_MODES``).  Enqueue-only.
        ``select``: the ``(row, slot)`` pairs of a safe-set net with a context (``SafeSetNet.ctx_select``) -- the context rows of
        the N + 1 forecast scenes are then written as well; None or empty leaves the context slot alone.  While the slot holds a
        forecast it is read from time 0: node k in column min(k, N).  ``B``: the batch size handed to the engine, the world's unless
        given (the engine refuses any other).  While an observed track is set (:meth:`set_instance_observed_track`) 'hold' and 'cv'
        are formed from it instead of the world; 'true' always reads the world."""
        if isinstance(mode, str):
            if mode not in FORECAST_MODES:
                raise ValueError(f'forecast_scene: mode {mode!r}: expected one of {sorted(FORECAST_MODES)}')
            mode = FORECAST_MODES[mode]
        self._forecast(self.L.smpc_forecast_scene, select, B, int(mode))

    def set_instance_observed_track(self, geom=None):
        """What the controller OBSERVES of the world (smpc_set_instance_observed_track): ``geom [B, T, n_rows,
        8]``, the world's shape, as a numpy array or a contiguous ROCm float64 tensor (``problem.observe_tracks`` draws one); the
        engine keeps a copy.  While it is set, :meth:`forecast_scene` ('hold', 'cv') and :meth:`forecast_scene_fit` read it instead
        of the world; 'true' and the plant's outcome test of :meth:`loop_post` keep reading the world.  None clears it, and so does
        clearing the world."""
        self._set_track(self.L.smpc_set_instance_observed_track, 'set_instance_observed_track', geom)

    def forecast_scene_fit(self, window, select=None, B=None):
        """The horizon's N + 1 scenes forecast by a least-squares line through the last ``window`` (1..``problem.FIT_MAX``) columns of
        what was seen -- the observed track, or the world without one -- at the scene clock, into the scene slot
        (smpc_forecast_scene_fit; ``problem.fit_forecast_statement`` is its definition).  Enqueue-only; ``select`` and ``B`` as for
        :meth:`forecast_scene`, and the slot is read from time 0 in the same way.  Window 1 is 'hold', window 2 is 'cv'."""
        self._forecast(self.L.smpc_forecast_scene_fit, select, B, int(window))

    def forecast_scene_poly(self, window, degree, select=None, B=None):
        """The horizon's N + 1 scenes forecast by a least-squares polynomial of degree 0, 1 or 2 through the last ``window``
        (1..``problem.FIT_MAX``) columns of what was seen, at the scene clock, into the scene slot (smpc_forecast_scene_poly;
        ``problem.poly_forecast_statement`` is its definition).  Enqueue-only; ``select`` and ``B`` as for :meth:`forecast_scene`.
        Degree 1 is :meth:`forecast_scene_fit`, degree 0 the window mean, degree 2 a constant-acceleration model."""
        self._forecast(self.L.smpc_forecast_scene_poly, select, B, int(window), int(degree))

    def forecast_row_margin(self, window, degree, z, sigma_prior=0.0, base=(0.0, 0.0), d_max=FIT_MARGIN_CAP, B=None):
        """The row-bounds table formed on the device from the residuals of the fit (smpc_forecast_row_margin;
        ``problem.fit_margin_statement`` is its definition): node k of every instance and row leaves
        ``d_k = base[0] + base[1] k + z s g_k`` metres of room, at most ``d_max`` -- s the residual standard deviation of a polynomial
        of ``degree`` through the last ``window`` columns seen (at least ``sigma_prior``), g_k the growth of its forecast's error along
        the horizon.  Enqueue-only, read at the scene clock like :meth:`forecast_scene_poly`, which it is meant to follow with the
        same window and degree; it fills the slot of :meth:`set_instance_row_bounds`.  ``B`` as for :meth:`forecast_scene`."""
        a, b = (float(v) for v in base)
        B = int(getattr(self, '_world_B', 0) if B is None else B)
        with self._ordered('torch' in sys.modules):
            self._chk(self.L.smpc_forecast_row_margin(self.h, B, int(window), int(degree), float(z), float(sigma_prior), a, b, float(d_max)))
        self._rowb_B = B

    def new_kalman_state(self, B):
        """``[B, n_rows, KALMAN_REC]`` zeros on this solver's device: the filter state of :meth:`forecast_scene_kalman`, every record
        "nothing seen".  The caller owns it; the engine keeps no filter state."""
        import torch
        return torch.zeros((int(B), len(self.problem.rows), KALMAN_REC), dtype=torch.float64, device=torch.device('cuda', self.device))

    def _kalman_args(self, name, par, state, B):
        from .problem import kalman_params
        import torch
        par = kalman_params(par, 0, 1, who=name)
        nr = len(self.problem.rows)
        if not _is_torch(state) or state.dtype != torch.float64 or not state.is_cuda or not state.is_contiguous():
            raise ValueError(f'{name}: state: expected a contiguous float64 tensor on the device (new_kalman_state)')
        if state.device.index != self.device:
            raise ValueError(f'{name}: state is on device {state.device.index}, the solver on {self.device}')
        if state.ndim != 3 or tuple(state.shape[1:]) != (nr, KALMAN_REC) or (B is not None and int(B) != state.shape[0]):
            raise ValueError(f'{name}: state of shape {tuple(state.shape)}: expected [{"B" if B is None else int(B)}, {nr}, {KALMAN_REC}]')
        return par, int(state.shape[0])

    def forecast_scene_kalman(self, par, state, advance=True, select=None, B=None):
        """One step of the obstacle filter and its forecast over the horizon, into the scene slot (smpc_forecast_scene_kalman;
        ``problem.kalman_statement`` is its definition).  ``par``: ``problem.kalman_params(degree, q, r, ...)``;
        ``state``: the ROCm tensor of :meth:`new_kalman_state`, updated in place.  ``advance=True`` reads what was seen (the observed
        track while one is set, else the world) at the scene clock and needs the world; a NaN in a moving slot leaves the record
        unobserved: predict only.  ``advance=False`` forecasts from the state as it is: no table is read, no world is needed and any B
        goes -- what a second solver with another horizon calls on rows of the first one's state.  Enqueue-only; ``select`` as for
        :meth:`forecast_scene`; ``B``: the state's unless given."""
        if not hasattr(self.L, 'smpc_forecast_scene_kalman'):
            raise _lib.EngineError('forecast_scene_kalman: this build of the engine has no smpc_forecast_scene_kalman')
        par, B = self._kalman_args('forecast_scene_kalman', par, state, B)
        sel = np.ascontiguousarray([] if select is None else select, np.int32).reshape(-1, 2)
        with self._ordered(True):
            self._chk(self.L.smpc_forecast_scene_kalman(self.h, B, C.byref(par), state.data_ptr(), 1 if advance else 0, len(sel),
                                                        sel.ctypes.data if len(sel) else None))

    def kalman_row_margin(self, par, state, z, base=(0.0, 0.0), d_max=FIT_MARGIN_CAP, B=None):
        """The row-bounds table formed on the device from the filter's covariance (smpc_kalman_row_margin;
        ``problem.kalman_margin_statement`` is its definition): node k leaves ``d_k = base[0] + base[1] k + z sqrt(s2) g_k`` metres,
        at most ``d_max`` -- g_k the predicted standard deviation of the position k columns ahead, s2 the innovation scale.  Reads
        ``state`` alone; enqueue-only; fills the slot of :meth:`set_instance_row_bounds`.  Meant to follow
        :meth:`forecast_scene_kalman` with the same ``par`` and ``state``."""
        if not hasattr(self.L, 'smpc_kalman_row_margin'):
            raise _lib.EngineError('kalman_row_margin: this build of the engine has no smpc_kalman_row_margin')
        par, B = self._kalman_args('kalman_row_margin', par, state, B)
        a, b = (float(v) for v in base)
        with self._ordered(True):
            self._chk(self.L.smpc_kalman_row_margin(self.h, B, C.byref(par), state.data_ptr(), float(z), a, b, float(d_max)))
        self._rowb_B = B

    def set_scene_clock(self, clock=None):
        """The time of node 0 for a scene track (smpc_set_scene_clock): a ONE-element int64 ROCm tensor that the engine reads on
        the device whenever a kernel runs -- write to it between calls (stream-ordered, no synchronisation), or hand over the
        step counter of a device loop.  The solver keeps a reference, so the cell lives as long as it is set.  None: time 0."""
        if clock is None:
            self._chk(self.L.smpc_set_scene_clock(self.h, None))
            self._scene_clock = None
            return
        import torch
        if not _is_torch(clock) or clock.dtype != torch.int64 or clock.numel() != 1 or not clock.is_cuda:
            raise ValueError('set_scene_clock: expected a one-element int64 tensor on the device')
        if clock.device.index != self.device:
            raise ValueError(f'set_scene_clock: the cell is on device {clock.device.index}, the solver on {self.device}')
        self._chk(self.L.smpc_set_scene_clock(self.h, clock.data_ptr()))
        self._scene_clock = clock

    def set_instance_curves(self, curves=None):
        """A reference curve of its own for every instance of the tracking task (smpc_set_instance_curves): ``curves [B, 3, L]``
        (tracking.tracking_curves / jittered_curves), a numpy array or a contiguous ROCm float64 tensor; the engine keeps a copy
        (24 B x L x B).  None clears them.  While set, :meth:`policy_step` feeds instance b the columns of ``curves[b]`` (and
        refuses a shared table), ``score_rollout(traj='instance')`` scores against them, and both must come with the same B."""
        if curves is not None and (curves.ndim != 3 or curves.shape[1] != 3):
            raise ValueError(f'set_instance_curves: expected [B, 3, L], got {tuple(curves.shape)}')
        L = 0 if curves is None else int(curves.shape[2])
        self._set_instance(self.L.smpc_set_instance_curves, 'set_instance_curves', [curves], (3, L), L)
        # what the handle holds: the tensor it was copied from (its owner says when it changes), or a copy of the host array
        self._curves_src = curves if _is_torch(curves) else None
        self._curves_host = None if curves is None or _is_torch(curves) else np.array(curves, np.float64)

    def set_instance_models(self, joints=None):
        """A controller model of its own for every instance (smpc_set_instance_models): ``joints [B, nq]`` of ``JOINT_DTYPE``
        (``closed_loop.perturbed_joint_tables``, the records ``plant_step`` takes as ``joints_noisy``), or the same records as a
        contiguous ROCm float64 tensor ``[B, nq, 29]``; the engine keeps a copy (232 B x nq x B).  Only mass, com and inertia are
        per instance: a numpy table that moves a kinematic field or a limit is refused, a tensor's are not read.  None clears it.
        While set, every call that forms the controller's dynamics (solve, eval_nodes, merit_terms, sqp, check_guess, policy_step)
        uses instance b's inertials and must come with the same B; the parallel policy and :meth:`rollout` refuse it."""
        words = JOINT_DTYPE.itemsize // 8
        if joints is not None and not _is_torch(joints):
            joints = np.ascontiguousarray(joints)
            if joints.dtype != JOINT_DTYPE or joints.ndim != 2 or joints.shape[1] != self.nq:
                raise ValueError(f'set_instance_models: expected JOINT_DTYPE [B, {self.nq}], got {joints.dtype} {tuple(joints.shape)}')
            joints = joints.view(np.float64).reshape(joints.shape[0], self.nq, words)
        elif joints is not None and (joints.ndim != 3 or tuple(joints.shape[1:]) != (self.nq, words)):
            raise ValueError(f'set_instance_models: expected [B, {self.nq}, {words}], got {tuple(joints.shape)}')
        self._set_instance(self.L.smpc_set_instance_models, 'set_instance_models', [joints], (self.nq, words))

    def _holds_curves(self, curves):
        if _is_torch(curves):
            return getattr(self, '_curves_src', None) is curves
        held = getattr(self, '_curves_host', None)
        return held is not None and held.shape == tuple(curves.shape) and np.array_equal(held, curves)

    def sync(self):
        self._chk(self.L.smpc_sync(self.h))

    def enable_timing(self, on=True):
        """True / 1: HIP events + the load-balance probe inside k_qp_ipm; 2: events only; False / 0: off"""
        self._chk(self.L.smpc_enable_timing(self.h, int(on)))

    def timing(self):
        ms = (C.c_float * 4)()
        self._chk(self.L.smpc_get_timing(self.h, ms))
        q = (C.c_float * 2)()
        self._chk(self.L.smpc_get_qp_timing(self.h, q))
        w = (C.c_double * 3)()
        self._chk(self.L.smpc_get_qp_wave_stats(self.h, w))
        return {'time_lin': ms[0] * 1e-3, 'time_nn': ms[1] * 1e-3, 'time_qp': ms[2] * 1e-3, 'time_tot': ms[3] * 1e-3,
                'time_qp_setup': q[0] * 1e-3, 'time_qp_ipm': q[1] * 1e-3,
                'qp_wave_busy_mean': w[0] * 1e-6, 'qp_wave_span': w[1] * 1e-6}

    def timing_history(self, back=0):
        """per-kernel times of the solve ``back`` solves before the last one (the engine keeps 64), or None if it has not
        finished / does not exist; never waits"""
        ms = (C.c_float * 6)()
        self._chk(self.L.smpc_get_timing_history(self.h, int(back), ms))
        if ms[5] == 0.0:
            return None
        return {'time_lin': ms[0] * 1e-3, 'time_nn': ms[1] * 1e-3, 'time_qp_setup': ms[2] * 1e-3, 'time_qp_ipm': ms[3] * 1e-3,
                'time_tot': ms[4] * 1e-3}

    def accumulate_stats(self, status, qp_iter, acc):
        """acc (3 x int64 on the device) += [sum of IPM iterations, failed solves, solves] -- no host round trip"""
        with self._ordered(1):
            self._chk(self.L.smpc_accumulate_stats(self.h, int(status.shape[0]), status.data_ptr(), qp_iter.data_ptr() if qp_iter is not None else None,
                                                   acc.data_ptr()))

    # -- argument plumbing -----------------------------------------------------------------------------------------------
    def _prep(self, arrs, shapes, dtypes=None):
        """returns (pointers, on_device, keepalive)"""
        dev = _is_torch(arrs[0])
        ptrs, keep = [], []
        for i, (a, shp) in enumerate(zip(arrs, shapes)):
            if a is None:
                ptrs.append(None)
                continue
            if _is_torch(a) != dev:
                raise TypeError('mix of torch and numpy arguments')
            if dev:
                if not a.is_cuda or not a.is_contiguous():
                    raise ValueError('device path needs contiguous ROCm tensors')
                if a.device.index != self.device:
                    raise ValueError(f'tensor on device {a.device.index}, solver on {self.device}')
                if tuple(a.shape) != tuple(shp):
                    raise ValueError(f'argument {i}: shape {tuple(a.shape)} != {tuple(shp)}')
                ptrs.append(a.data_ptr())
                keep.append(a)
            else:
                dt = np.float64 if dtypes is None else dtypes[i]
                b = np.ascontiguousarray(a, dt)
                if tuple(b.shape) != tuple(shp):
                    raise ValueError(f'argument {i}: shape {tuple(b.shape)} != {tuple(shp)}')
                ptrs.append(b.ctypes.data)
                keep.append(b)
        return ptrs, int(dev), keep

    def _set_instance(self, fn, name, arrs, tail, *ints):
        """The steps every per-instance input shares, for ``fn(h, B, *ints, *arrays, on_device)``: None clears the
        slot; a tensor must be float64; every array is ``[B, *tail]``, B read off the first; the engine's stream is ordered against
        torch's around the call."""
        if arrs[0] is None:
            self._chk(fn(self.h, 0, *ints, *[None] * len(arrs), 0))
            return
        if _is_torch(arrs[0]):
            import torch
            if any(_is_torch(a) and a.dtype != torch.float64 for a in arrs):
                raise ValueError(f'{name}: a tensor argument must be float64')
        B = int(arrs[0].shape[0])
        ptrs, dev, keep = self._prep(arrs, [(B, *tail)] * len(arrs))
        with self._ordered(dev):
            self._chk(fn(self.h, B, *ints, *ptrs, dev))

    def _state_pointers(self, what, d, fields, shapes, B, dev):
        """pointers of the per-instance arrays ``d[k]`` of a ctypes struct of arrays (``fields``: (name, dtype); ``shapes``: the
        names that are not [B]), each checked for kind, shape, dtype and contiguity"""
        out = []
        for k, dt in fields:
            a, shp = d[k], tuple(shapes.get(k, (B,)))
            if _is_torch(a) != bool(dev):
                raise TypeError('mix of torch and numpy arguments')
            if dev:
                if not a.is_cuda or not a.is_contiguous() or tuple(a.shape) != shp or a.element_size() != np.dtype(dt).itemsize:
                    raise ValueError(f'{what} {k}: expected a contiguous {list(shp)} device tensor of {dt}')
                out.append(a.data_ptr())
            else:
                if a.dtype != np.dtype(dt) or a.shape != shp or not a.flags.c_contiguous:
                    raise ValueError(f'{what} {k}: expected a contiguous {list(shp)} array of {dt}')
                out.append(a.ctypes.data)
        return out

    # -- the hot path ------------------------------------------------------------------------------------------------------
    def solve(self, x0, x_guess, u_guess, p, out=None):
        """One SQP-RTI solve per instance (controller.py:136-167).  Returns (x, u, status, qp_iter)."""
        B = x0.shape[0]
        N, nx, nu = self.N, self.nx, self.nu
        if B == 0:      # an empty batch is a loop over no instances (scripts/mpc.py:102), not an error
            if _is_torch(x0):
                import torch
                kw = dict(device=x0.device)
                return (torch.empty((0, N + 1, nx), dtype=torch.float64, **kw), torch.empty((0, N, nu), dtype=torch.float64, **kw),
                        torch.empty((0,), dtype=torch.int32, **kw), torch.empty((0,), dtype=torch.int32, **kw))
            return np.empty((0, N + 1, nx)), np.empty((0, N, nu)), np.empty(0, np.int32), np.empty(0, np.int32)
        shapes = [(B, nx), (B, N + 1, nx), (B, N, nu), (B, N + 1, 5)]
        ptrs, dev, keep = self._prep([x0, x_guess, u_guess, p], shapes)
        if dev:
            import torch
            if out is None:
                kw = dict(device=x0.device)
                out = (torch.empty((B, N + 1, nx), dtype=torch.float64, **kw),
                       torch.empty((B, N, nu), dtype=torch.float64, **kw),
                       torch.empty((B,), dtype=torch.int32, **kw), torch.empty((B,), dtype=torch.int32, **kw))
            op = [o.data_ptr() for o in out]
        else:
            if out is None:
                out = (np.empty((B, N + 1, nx)), np.empty((B, N, nu)), np.empty(B, np.int32), np.empty(B, np.int32))
            op = [o.ctypes.data for o in out]
        with self._ordered(dev):
            self._chk(self.L.smpc_solve_batch(self.h, B, *ptrs, *op, dev))
        return out

    def eval_nodes(self, x_guess, u_guess, p):
        B = x_guess.shape[0]
        N, nx, nu = self.N, self.nx, self.nu
        ptrs, dev, keep = self._prep([x_guess, u_guess, p], [(B, N + 1, nx), (B, N, nu), (B, N + 1, 5)])
        if dev:
            # device path: a dict of float64 views into one [B, N+1, sizeof(smpc_node_eval)/8] tensor, same field names
            import torch
            nd = NODE_EVAL_DTYPE.itemsize // 8
            raw = torch.zeros((B, N + 1, nd), dtype=torch.float64, device=x_guess.device)
            with self._ordered(1):
                self._chk(self.L.smpc_eval_nodes(self.h, B, *ptrs, raw.data_ptr(), 1))
            out = {}
            for name in NODE_EVAL_DTYPE.names:
                dt, off = NODE_EVAL_DTYPE.fields[name][:2]
                n = dt.itemsize // 8
                out[name] = raw[..., off // 8: off // 8 + n] if dt.shape else raw[..., off // 8]
            return out
        out = np.zeros((B, N + 1), NODE_EVAL_DTYPE)
        self._chk(self.L.smpc_eval_nodes(self.h, B, *ptrs, out.ctypes.data, 0))
        return out

    # -- SQP with merit backtracking (a11) ---------------------------------------------------------------------------------
    def merit_terms(self, x0, x, u, p, dx=None, du=None, alpha=None, mask=None, out=None):
        """[B, 3] = (f, viol, gd) of the l1 merit function at (x + alpha dx, u + alpha du), forward-only on the device
        (smpc_merit_terms; the numpy statement is closed_loop.merit_terms).  gd = grad f . (dx, du) where alpha is 0 / None.
        ``mask`` (uint8 [B]): instances with 0 are skipped and keep their row of ``out``."""
        B = x.shape[0]
        N, nx, nu = self.N, self.nx, self.nu
        arrs = [x0, x, u, p, dx, du, alpha, mask]
        shapes = [(B, nx), (B, N + 1, nx), (B, N, nu), (B, N + 1, 5), (B, N + 1, nx), (B, N, nu), (B,), (B,)]
        ptrs, dev, keep = self._prep(arrs, shapes, [np.float64] * 7 + [np.uint8])
        if dev:
            import torch
            if mask is not None and mask.dtype not in (torch.uint8, torch.bool):
                raise ValueError('mask must be uint8 or bool')
            if out is None:
                out = torch.zeros((B, 3), dtype=torch.float64, device=x.device)
            op = out.data_ptr()
        else:
            out = np.zeros((B, 3)) if out is None else out
            assert out.dtype == np.float64 and out.shape == (B, 3) and out.flags.c_contiguous
            op = out.ctypes.data
        with self._ordered(dev):
            self._chk(self.L.smpc_merit_terms(self.h, B, *ptrs, op, dev))
        return out

    def new_sqp_state(self, B, like=None, mu0=10.0):
        """the per-instance in/out arrays of :meth:`sqp` (smpc_sqp_state) at their start values, numpy or on ``like``'s device"""
        if like is not None and _is_torch(like):
            import torch
            tdt = {'f8': torch.float64, 'u1': torch.uint8, 'i4': torch.int32}
            st = {k: torch.zeros((B,), dtype=tdt[dt], device=like.device) for k, dt in _lib.SqpState.FIELDS}
            st['mu'].fill_(float(mu0))
        else:
            st = {k: np.zeros(B, dt) for k, dt in _lib.SqpState.FIELDS}
            st['mu'][:] = float(mu0)
        return st

    def sqp(self, x0, x_guess, u_guess, p, opts=None, state=None):
        """SQP with l1-merit backtracking for B instances on the device (smpc_sqp_batch): up to ``opts.max_iter`` iterations from
        (x_guess, u_guess), resuming from ``state`` (a dict from :meth:`new_sqp_state`, updated in place) when given.  ``opts``: an
        _lib.SqpOpts, a dict of its fields, or None for generate_guess' defaults with max_iter = 1.  Torch tensors are updated in
        place; numpy arrays are copied.  Returns (x_guess, u_guess, state)."""
        B = x0.shape[0]
        N, nx, nu = self.N, self.nx, self.nu
        if opts is None or isinstance(opts, dict):
            opts = _lib.SqpOpts(**(opts or {}))
        dev = _is_torch(x0)
        if not dev:
            x_guess = np.array(x_guess, np.float64, order='C', copy=True)
            u_guess = np.array(u_guess, np.float64, order='C', copy=True)
        if state is None:
            state = self.new_sqp_state(B, x0, opts.mu0)
        ptrs, dev, keep = self._prep([x0, x_guess, u_guess, p], [(B, nx), (B, N + 1, nx), (B, N, nu), (B, N + 1, 5)])
        if not dev:
            ptrs[1], ptrs[2] = x_guess.ctypes.data, u_guess.ctypes.data
        cst = _lib.SqpState(*self._state_pointers('SQP state', state, _lib.SqpState.FIELDS, {}, B, dev))
        with self._ordered(dev):
            self._chk(self.L.smpc_sqp_batch(self.h, B, C.byref(opts), ptrs[0], ptrs[1], ptrs[2], ptrs[3], C.byref(cst), dev))
        return x_guess, u_guess, state

    def check_guess(self, x, u, safe_node=None, collision_first_node=None, mask=None, flags=None, worst=None, **tol):
        """The acceptance test of a warm start per instance, forward-only on the device (smpc_check_guess; the statement is
        AbstractController.checkGuess).  Returns ``(flags [B] int32, worst [B, 5])``: bit i of ``flags`` is set when predicate i
        fails -- 0 state box, 1 collision rows, 2 torque, 3 dynamics, 4 safe set at node ``safe_node`` (None: not tested) -- and
        ``worst[:, i]`` is the value the predicate tests (include/smpc.h).  ``mask`` (uint8 [B]): instances with 0 are skipped and
        keep their rows of ``flags`` / ``worst``.  ``collision_first_node`` defaults to ``params.reference_quirks``; ``tol`` may
        override tol_x, tol_tau, tol_dyn, tol_safe, alpha, x_min, x_max, tau_min, tau_max, row_lb, row_ub (defaults from the
        problem and its params, as in :meth:`check_trajectory`)."""
        pr, par = self.problem, self.problem.params
        unknown = set(tol) - {'tol_x', 'tol_tau', 'tol_dyn', 'tol_safe', 'alpha', 'x_min', 'x_max', 'tau_min', 'tau_max', 'row_lb', 'row_ub'}
        if unknown:
            raise TypeError(f'check_guess: unknown argument(s) {sorted(unknown)}')
        if collision_first_node is None:
            collision_first_node = bool(getattr(par, 'reference_quirks', True))
        small = [np.ascontiguousarray(tol.get(k, d), np.float64)
                 for k, d in (('x_min', pr.x_min), ('x_max', pr.x_max), ('tau_min', pr.tau_min), ('tau_max', pr.tau_max),
                              ('row_lb', pr.row_check[:, 0]), ('row_ub', pr.row_check[:, 1]))]
        for a, n in zip(small, (self.nx, self.nx, self.nq, self.nq, len(pr.row_check), len(pr.row_check))):
            if a.shape != (n,):
                raise ValueError(f'check_guess: a bound has shape {a.shape}, expected ({n},)')
        gc = _lib.GuessCheck(float(tol.get('tol_x', par.tol_x)), float(tol.get('tol_tau', par.tol_tau)),
                             float(tol.get('tol_dyn', par.tol_dyn)), float(tol.get('tol_safe', par.tol_safe_set)),
                             float(tol.get('alpha', par.alpha)), int(bool(collision_first_node)),
                             -1 if safe_node is None else int(safe_node), *[a.ctypes.data for a in small])
        B = x.shape[0]
        N, nx, nu = self.N, self.nx, self.nu
        ptrs, dev, keep = self._prep([x, u, mask, flags, worst], [(B, N + 1, nx), (B, N, nu), (B,), (B,), (B, 5)],
                                     [np.float64, np.float64, np.uint8, np.int32, np.float64])
        if dev:
            import torch
            if mask is not None and mask.dtype not in (torch.uint8, torch.bool):
                raise ValueError('mask must be uint8 or bool')
            if flags is None:
                flags = torch.zeros((B,), dtype=torch.int32, device=x.device)
            if worst is None:
                worst = torch.zeros((B, 5), dtype=torch.float64, device=x.device)
            if flags.dtype != torch.int32 or worst.dtype != torch.float64:
                raise ValueError('flags must be int32 and worst float64')
            fp, wp = flags.data_ptr(), worst.data_ptr()
        else:
            flags = np.zeros(B, np.int32) if flags is None else flags
            worst = np.zeros((B, 5)) if worst is None else worst
            assert flags.dtype == np.int32 and flags.shape == (B,) and flags.flags.c_contiguous
            assert worst.dtype == np.float64 and worst.shape == (B, 5) and worst.flags.c_contiguous
            fp, wp = flags.ctypes.data, worst.ctypes.data
        with self._ordered(dev):
            self._chk(self.L.smpc_check_guess(self.h, B, ptrs[0], ptrs[1], C.byref(gc), ptrs[2], fp, wp, dev))
        return flags, worst

    # -- safe-set training data: the bookkeeping of ray labelling ---------------------------------------------------------
    def _ray_shapes(self, B):
        N, nx, nu, nq = self.N, self.nx, self.nu, self.nq
        return {'q': (B, nq), 'd': (B, nq), 'x_cert': (B, N + 1, nx), 'u_cert': (B, N, nu)}

    def new_ray_state(self, q, d, s_hi, like=None):
        """The per-ray in/out arrays of :meth:`ray_update` (smpc_ray_state) for the rays ``(q, d)`` [B, nq] whose velocity box ends
        at ``s_hi`` [B], before trial 0: bracket [0, s_hi], s = 0, every ray open.  numpy, or tensors on ``like``'s device."""
        from .safe_set_data import new_ray_state
        st = new_ray_state(q, d, s_hi, self.N)
        if like is not None and _is_torch(like):
            import torch
            st = {k: torch.as_tensor(v, device=like.device) for k, v in st.items()}
        return st

    def ray_update(self, rays, state, flags, x0, x_guess, u_guess, n_open=None, bisect=8, budget=30, tol_term=None, mu0=10.0):
        """One look at every open ray after a round of :meth:`sqp` and :meth:`check_guess` (smpc_ray_update; the numpy statement is
        safe_set_data.ray_update_statement): resolves the trials that are feasible or have ended, keeps certificates, moves
        brackets, ends rays or starts their next trial -- all in place on ``rays`` (:meth:`new_ray_state`), ``state``
        (:meth:`new_sqp_state`), ``x0``, ``x_guess``, ``u_guess``.  Returns ``n_open``: a one-element int32 array / tensor holding
        the number of rays still open (on the device path nothing is read back: the caller does)."""
        B = x0.shape[0]
        N, nx, nu = self.N, self.nx, self.nu
        ptrs, dev, keep = self._prep([x0, x_guess, u_guess, flags], [(B, nx), (B, N + 1, nx), (B, N, nu), (B,)],
                                     [np.float64, np.float64, np.float64, np.int32])
        if dev:
            import torch
            if flags.dtype != torch.int32:
                raise ValueError('flags must be int32')
            if n_open is None:
                n_open = torch.zeros((1,), dtype=torch.int32, device=x0.device)
            if n_open.dtype != torch.int32 or not n_open.is_cuda:
                raise ValueError('n_open must be an int32 device tensor')
            open_ptr = n_open.data_ptr()
        else:
            for a, dt in ((x0, np.float64), (x_guess, np.float64), (u_guess, np.float64), (flags, np.int32)):
                if not isinstance(a, np.ndarray) or a.dtype != dt or not a.flags.c_contiguous:
                    raise ValueError('ray_update works in place: contiguous float64 x0 / x_guess / u_guess and int32 flags expected')
            n_open = np.zeros(1, np.int32) if n_open is None else n_open
            if not isinstance(n_open, np.ndarray) or n_open.dtype != np.int32 or n_open.shape != (1,):
                raise ValueError('n_open must be a one-element int32 array')
            open_ptr = n_open.ctypes.data

        rs = _lib.RayState(*self._state_pointers('ray state', rays, _lib.RayState.FIELDS, self._ray_shapes(B), B, dev))
        cst = _lib.SqpState(*self._state_pointers('SQP state', state, _lib.SqpState.FIELDS, {}, B, dev))
        ro = _lib.RayOpts(int(bisect), int(budget), float(self.problem.params.tol_x if tol_term is None else tol_term), float(mu0))
        with self._ordered(dev):
            self._chk(self.L.smpc_ray_update(self.h, B, C.byref(ro), C.byref(rs), C.byref(cst), ptrs[3], ptrs[0], ptrs[1], ptrs[2],
                                             open_ptr, dev))
        return n_open

    # -- start states at a chosen end-effector position ---------------------------------------------------------------------
    def ik(self, target, q_start, mask=None, q_out=None, info=None, resid=None, **over):
        """Batched multi-start inverse kinematics with collision rows on the device (smpc_ik_batch; the numpy statement is
        ik.ik_batch_host): per instance a q in the joint box with ee(q) = ``target[b]`` and every collision row within its bounds,
        from the ``S`` starts ``q_start[b]`` (``target [B, 3]``, ``q_start [B, S, nq]``, 1 <= S <= 64).  Returns ``(q_out [B, nq],
        info [B, 2] int32 = (winning start, number of successful starts; 0 = no solution), resid [B, 2] = (|ee - target|_inf, worst
        row margin) at q_out)``.  ``mask`` (uint8 [B]): instances with 0 are skipped and keep their rows of the outputs.  While a
        scene is set (:meth:`set_instance_scene`) the rows are formed in each instance's scene.  ``over`` may override
        ik.IK_DEFAULTS (max_iter, tol_ee, push, damping, ...) and q_lo, q_hi, row_lb, row_ub (defaults: the model's joint box and
        the OCP's row bounds)."""
        from .ik import ik_params
        par = ik_params(self.problem, **over)
        if q_start.ndim != 3:
            raise ValueError('ik: q_start [B, S, nq] expected')
        B, S = int(q_start.shape[0]), int(q_start.shape[1])
        ptrs, dev, keep = self._prep([target, q_start, mask, q_out, info, resid], [(B, 3), (B, S, self.nq), (B,), (B, self.nq), (B, 2), (B, 2)],
                                     [np.float64, np.float64, np.uint8, np.float64, np.int32, np.float64])
        if dev:
            import torch
            if target.dtype != torch.float64 or q_start.dtype != torch.float64:
                raise ValueError('target and q_start must be float64')
            if mask is not None and mask.dtype not in (torch.uint8, torch.bool):
                raise ValueError('mask must be uint8 or bool')
            kw = dict(device=target.device)
            q_out = torch.zeros((B, self.nq), dtype=torch.float64, **kw) if q_out is None else q_out
            info = torch.zeros((B, 2), dtype=torch.int32, **kw) if info is None else info
            resid = torch.zeros((B, 2), dtype=torch.float64, **kw) if resid is None else resid
            if q_out.dtype != torch.float64 or info.dtype != torch.int32 or resid.dtype != torch.float64:
                raise ValueError('q_out and resid must be float64 and info int32')
            op = [q_out.data_ptr(), info.data_ptr(), resid.data_ptr()]
        else:
            q_out = np.zeros((B, self.nq)) if q_out is None else q_out
            info = np.zeros((B, 2), np.int32) if info is None else info
            resid = np.zeros((B, 2)) if resid is None else resid
            assert q_out.dtype == np.float64 and q_out.shape == (B, self.nq) and q_out.flags.c_contiguous
            assert info.dtype == np.int32 and info.shape == (B, 2) and info.flags.c_contiguous
            assert resid.dtype == np.float64 and resid.shape == (B, 2) and resid.flags.c_contiguous
            op = [q_out.ctypes.data, info.ctypes.data, resid.ctypes.data]
        small = [par[k] for k in ('q_lo', 'q_hi', 'row_lb', 'row_ub')]
        ip = _lib.IkParams(par['max_iter'], 0, float(par['tol_ee']), float(par['push']), float(par['damping']),
                           float(par['damping_accept']), float(par['damping_reject']), float(par['damping_min']),
                           float(par['damping_max']), *[a.ctypes.data for a in small])
        with self._ordered(dev):
            self._chk(self.L.smpc_ik_batch(self.h, B, S, ptrs[0], ptrs[1], C.byref(ip), ptrs[2], *op, dev))
        return q_out, info, resid

    # -- scoring a closed-loop run --------------------------------------------------------------------------------------
    def score_rollout(self, x_log, u_log, last_x=None, last_u=None, ee_ref=None, traj=None, want_safe=False, mask=None, out=None,
                      outi=None, **bounds):
        """Scores of a closed-loop run from its STEP-major logs ``x_log [n_steps+1, B, nx]``, ``u_log [n_steps, B, nu]``, forward-only
        on the device (smpc_score_rollout; the numpy statement is closed_loop.score_rollout_statement).  Returns
        ``(out [B, 7], outi [B, 4] int32)`` with the columns ``SCORE_SLOTS`` / ``SCORE_INDEX_SLOTS``: closed-loop cost
        (metrics_count_fails.py:19-28), its two sums, the EE distance of the last state (mpc.py:273), the worst collision and
        state-box margins and the least safe-set value with the step (and row) each was taken at.  ``last_x`` / ``last_u`` (int64
        [B]): last valid row of each log, None = complete; rows past them affect nothing.  The reference point is ``traj [3, L]``
        (column min(j, L - 1) at step j) or the constant ``ee_ref`` (default: the problem's).  ``traj [B, 3, L]``: instance b is
        scored against ``traj[b]`` -- the curves are handed to the handle first unless they are the ones it holds
        (:meth:`set_instance_curves`) -- and ``traj='instance'`` scores against the curves already held.  ``want_safe`` needs a network.
        ``mask`` (uint8 [B]): instances with 0 are skipped and keep their rows of ``out`` / ``outi``.  ``bounds`` may override
        x_min, x_max, row_lb, row_ub, alpha, tol_safe (defaults from the problem and its params, as in :meth:`check_guess`)."""
        pr, par = self.problem, self.problem.params
        unknown = set(bounds) - {'x_min', 'x_max', 'row_lb', 'row_ub', 'alpha', 'tol_safe'}
        if unknown:
            raise TypeError(f'score_rollout: unknown argument(s) {sorted(unknown)}')
        small = [np.ascontiguousarray(bounds.get(k, d), np.float64)
                 for k, d in (('x_min', pr.x_min), ('x_max', pr.x_max), ('row_lb', pr.row_check[:, 0]), ('row_ub', pr.row_check[:, 1]))]
        small.append(np.ascontiguousarray(pr.ee_ref if ee_ref is None else ee_ref, np.float64))
        for a, n in zip(small, (self.nx, self.nx, len(pr.row_check), len(pr.row_check), 3)):
            if a.shape != (n,):
                raise ValueError(f'score_rollout: a bound has shape {a.shape}, expected ({n},)')
        if x_log.ndim != 3 or u_log.ndim != 3:
            raise ValueError('score_rollout: x_log [n_steps+1, B, nx] and u_log [n_steps, B, nu] expected')
        n_steps, B = int(u_log.shape[0]), int(x_log.shape[1])
        own = isinstance(traj, str) or (traj is not None and traj.ndim == 3)       # against the handle's curves: neither pointer is passed
        if isinstance(traj, str):
            if traj != 'instance':
                raise ValueError(f"score_rollout: traj must be an array or 'instance', got {traj!r}")
        elif own:
            if traj.shape[0] != B:
                raise ValueError(f'score_rollout: {traj.shape[0]} curves for logs of {B} instances')
            if not self._holds_curves(traj):
                self.set_instance_curves(traj)
        if own:
            traj = None
        L = int(traj.shape[1]) if traj is not None else 0
        ptrs, dev, keep = self._prep([x_log, u_log, last_x, last_u, traj, mask, out, outi],
                                     [(n_steps + 1, B, self.nx), (n_steps, B, self.nu), (B,), (B,), (3, L), (B,), (B, SCORE_ND), (B, SCORE_NI)],
                                     [np.float64, np.float64, np.int64, np.int64, np.float64, np.uint8, np.float64, np.int32])
        if dev:
            import torch
            if mask is not None and mask.dtype not in (torch.uint8, torch.bool):
                raise ValueError('mask must be uint8 or bool')
            for a in (last_x, last_u):
                if a is not None and a.dtype != torch.int64:
                    raise ValueError('last_x / last_u must be int64')
            if traj is not None and traj.dtype != torch.float64:
                raise ValueError('traj must be float64')
            if out is None:
                out = torch.zeros((B, SCORE_ND), dtype=torch.float64, device=x_log.device)
            if outi is None:
                outi = torch.zeros((B, SCORE_NI), dtype=torch.int32, device=x_log.device)
            if out.dtype != torch.float64 or outi.dtype != torch.int32:
                raise ValueError('out must be float64 and outi int32')
            op, ip = out.data_ptr(), outi.data_ptr()
        else:
            out = np.zeros((B, SCORE_ND)) if out is None else out
            outi = np.zeros((B, SCORE_NI), np.int32) if outi is None else outi
            assert out.dtype == np.float64 and out.shape == (B, SCORE_ND) and out.flags.c_contiguous
            assert outi.dtype == np.int32 and outi.shape == (B, SCORE_NI) and outi.flags.c_contiguous
            op, ip = out.ctypes.data, outi.ctypes.data
        sp = _lib.ScoreParams(float(bounds.get('alpha', par.alpha)), float(bounds.get('tol_safe', par.tol_safe_set)), int(bool(want_safe)), 0,
                              *[a.ctypes.data for a in small], ptrs[4], L)
        if own:
            sp.ee_ref = None
        with self._ordered(dev):
            self._chk(self.L.smpc_score_rollout(self.h, B, n_steps, ptrs[0], ptrs[1], ptrs[2], ptrs[3], C.byref(sp), ptrs[5], op, ip, dev))
        return out, outi

    # -- callers around the solve (a13, a15, a16) ------------------------------------------------------------------------
    def guess_correction(self, x_guess, u_guess):
        """In place on torch tensors; returns a corrected copy for numpy."""
        B = x_guess.shape[0]
        if not _is_torch(x_guess):
            x_guess = np.array(x_guess, np.float64, order='C', copy=True)
        ptrs, dev, keep = self._prep([x_guess, u_guess], [(B, self.N + 1, self.nx), (B, self.N, self.nu)])
        with self._ordered(dev):
            self._chk(self.L.smpc_guess_correction(self.h, B, *ptrs, dev))
        return x_guess

    def provide_control(self, accept, x_temp, u_temp, x_guess, u_guess):
        B = x_temp.shape[0]
        N, nx, nu = self.N, self.nx, self.nu
        if not _is_torch(x_guess):
            x_guess = np.array(x_guess, np.float64, order='C', copy=True)
            u_guess = np.array(u_guess, np.float64, order='C', copy=True)
            u_apply = np.empty((B, nu))
            accept = np.ascontiguousarray(accept, np.int32)
        else:
            import torch
            u_apply = torch.empty((B, nu), dtype=torch.float64, device=x_guess.device)
        ptrs, dev, keep = self._prep([accept, x_temp, u_temp, x_guess, u_guess, u_apply],
                                     [(B,), (B, N + 1, nx), (B, N, nu), (B, N + 1, nx), (B, N, nu), (B, nu)],
                                     [np.int32] + [np.float64] * 5)
        if not dev:
            # _prep may have re-wrapped the arrays; make sure outputs are the ones we return
            ptrs[3], ptrs[4], ptrs[5] = x_guess.ctypes.data, u_guess.ctypes.data, u_apply.ctypes.data
        with self._ordered(dev):
            self._chk(self.L.smpc_provide_control(self.h, B, *ptrs, dev))
        return x_guess, u_guess, u_apply

    def check_trajectory(self, x, x_min=None, x_max=None, tol_x=None, row_lb=None, row_ub=None, alpha=None,
                         tol_safe=None, want_nn=False):
        """checkStateConstraints (env_model.py:170-173) per instance; optionally the safe-set test per node."""
        pr, par = self.problem, self.problem.params
        x_min = pr.x_min if x_min is None else x_min
        x_max = pr.x_max if x_max is None else x_max
        tol_x = par.tol_x if tol_x is None else tol_x
        row_lb = pr.row_check[:, 0] if row_lb is None else row_lb
        row_ub = pr.row_check[:, 1] if row_ub is None else row_ub
        alpha = par.alpha if alpha is None else alpha
        tol_safe = par.tol_safe_set if tol_safe is None else tol_safe
        B, n_nodes = x.shape[0], x.shape[1]
        small = [np.ascontiguousarray(a, np.float64) for a in (x_min, x_max, row_lb, row_ub)]
        if _is_torch(x):
            import torch
            ok = torch.empty((B,), dtype=torch.int32, device=x.device)
            nn = torch.empty((B, n_nodes), dtype=torch.int32, device=x.device) if want_nn else None
            with self._ordered(1):
                self._chk(self.L.smpc_check_trajectory(self.h, B, n_nodes, x.data_ptr(), small[0].ctypes.data,
                                                       small[1].ctypes.data, tol_x, small[2].ctypes.data,
                                                       small[3].ctypes.data, alpha, tol_safe, ok.data_ptr(),
                                                       nn.data_ptr() if want_nn else None, 1))
            return (ok, nn) if want_nn else ok
        xx = np.ascontiguousarray(x, np.float64)
        ok = np.empty(B, np.int32)
        nn = np.empty((B, n_nodes), np.int32) if want_nn else None
        self._chk(self.L.smpc_check_trajectory(self.h, B, n_nodes, xx.ctypes.data, small[0].ctypes.data,
                                               small[1].ctypes.data, tol_x, small[2].ctypes.data, small[3].ctypes.data,
                                               alpha, tol_safe, ok.ctypes.data, nn.ctypes.data if want_nn else None, 0))
        return (ok.astype(bool), nn.astype(bool)) if want_nn else ok.astype(bool)

    def rollout(self, x0, x_guess, u_guess, p, n_steps, joints_noisy=None, tau_noise=None):
        """n_steps of the plain RTI policy + plant without a host round trip per step (smpc_rollout_batch).
        x_guess / u_guess are updated in place (torch) or returned updated (numpy).  Returns step-major
        (x_traj[n+1, B, nx], u_traj[n, B, nu], status[n, B], qp_iter[n, B], x_guess, u_guess)."""
        B, n = x0.shape[0], int(n_steps)
        N, nx, nu = self.N, self.nx, self.nu
        if _is_torch(x0):
            import torch
            kw = dict(device=x0.device)
            xt = torch.empty((n + 1, B, nx), dtype=torch.float64, **kw)
            ut = torch.empty((n, B, nu), dtype=torch.float64, **kw)
            st = torch.empty((n, B), dtype=torch.int32, **kw)
            it = torch.empty((n, B), dtype=torch.int32, **kw)
            jn = joints_noisy.data_ptr() if joints_noisy is not None else None
            tn = tau_noise.data_ptr() if tau_noise is not None else None
            for a, shp in ((x0, (B, nx)), (x_guess, (B, N + 1, nx)), (u_guess, (B, N, nu)), (p, (B, N + 1, 5))):
                if tuple(a.shape) != shp or a.dtype != torch.float64 or not a.is_contiguous():
                    raise ValueError(f'rollout: expected a contiguous float64 tensor of shape {shp}')
            with self._ordered(1):
                self._chk(self.L.smpc_rollout_batch(self.h, B, n, x0.data_ptr(), x_guess.data_ptr(), u_guess.data_ptr(), p.data_ptr(),
                                                    jn, tn, xt.data_ptr(), ut.data_ptr(), st.data_ptr(), it.data_ptr(), 1))
            return xt, ut, st, it, x_guess, u_guess
        x0 = np.ascontiguousarray(x0, np.float64)
        xg = np.array(x_guess, np.float64, order='C', copy=True)
        ug = np.array(u_guess, np.float64, order='C', copy=True)
        pp = np.ascontiguousarray(p, np.float64)
        assert x0.shape == (B, nx) and xg.shape == (B, N + 1, nx) and ug.shape == (B, N, nu) and pp.shape == (B, N + 1, 5)
        xt, ut = np.empty((n + 1, B, nx)), np.empty((n, B, nu))
        st, it = np.empty((n, B), np.int32), np.empty((n, B), np.int32)
        jn = tn = None
        if joints_noisy is not None:
            joints_noisy = np.ascontiguousarray(joints_noisy, JOINT_DTYPE)
            assert joints_noisy.shape == (B, self.nq)
            jn = joints_noisy.ctypes.data
        if tau_noise is not None:
            tau_noise = np.ascontiguousarray(tau_noise, np.float64)
            assert tau_noise.shape == (n, B, nu)
            tn = tau_noise.ctypes.data
        self._chk(self.L.smpc_rollout_batch(self.h, B, n, x0.ctypes.data, xg.ctypes.data, ug.ctypes.data, pp.ctypes.data, jn, tn,
                                            xt.ctypes.data, ut.ctypes.data, st.ctypes.data, it.ctypes.data, 0))
        return xt, ut, st, it, xg, ug

    # -- the policy layer with all state in HBM (smpc_policy_step / smpc_loop_pre / smpc_loop_post) -------------------------------
    def _policy_params(self, kind=0, abort_flag=0, tube=0.0, stage_lo=None, stage_hi=None):
        """smpc_policy_params from the problem's parameters; the small host arrays it points to are kept alive here"""
        pr, par = self.problem, self.problem.params
        small = [np.ascontiguousarray(a, np.float64) for a in (pr.x_min, pr.x_max, pr.row_check[:, 0], pr.row_check[:, 1])]
        pp = _lib.PolicyParams(int(kind), int(bool(abort_flag)), int(bool(getattr(par, 'reference_quirks', True))), 0,
                               float(par.tol_x), float(par.alpha), float(par.tol_safe_set), float(tube),
                               small[0].ctypes.data, small[1].ctypes.data, small[2].ctypes.data, small[3].ctypes.data,
                               stage_lo.data_ptr() if stage_lo is not None else None,
                               stage_hi.data_ptr() if stage_hi is not None else None)
        pp._keep = small
        return pp

    def policy_step(self, ctrl, x, stepping=None, u_other=None, u_out=None):
        """<Controller>.step(x) of ``ctrl`` (device state) as engine kernels.  Returns (u, abort) -- persistent tensors of the
        controller -- and leaves "did any instance abort" in ``ctrl._any_abort`` (one int32 on the device)."""
        ptr = lambda t: t.data_ptr() if t is not None else None
        pp = self._policy_params(ctrl.policy_kind, getattr(ctrl, 'abort_flag', False), getattr(ctrl, 'TUBE', 0.0),
                                 getattr(ctrl, '_stage_lo', None), getattr(ctrl, '_stage_hi', None))
        traj = getattr(ctrl, 'traj', None)
        if traj is not None and traj.ndim == 3:     # a curve per instance: the handle holds them and the step passes no shared table
            if not self._holds_curves(traj):        # (cleared, or another controller's, since setTrajectory handed them over)
                self.set_instance_curves(traj)
            traj = None
        st = _lib.PolicyState(ptr(ctrl.x_guess), ptr(ctrl.u_guess), ptr(ctrl.x_temp), ptr(ctrl.u_temp), ptr(ctrl.p), ptr(ctrl.x_viable),
                              ptr(ctrl.fails), ptr(ctrl.current_step), ptr(getattr(ctrl, 'r', None)), ptr(ctrl.last_status),
                              ptr(ctrl.qp_iter), ptr(traj), int(traj.shape[1]) if traj is not None else 0)
        u_out = ctrl._u_out if u_out is None else u_out
        with self._ordered(1):
            self._chk(self.L.smpc_policy_step(self.h, ctrl.B, C.byref(pp), C.byref(st), x.data_ptr(), ptr(stepping), ptr(u_other),
                                              u_out.data_ptr(), ctrl._abort_out.data_ptr(), ctrl._any_abort.data_ptr()))
        return u_out, ctrl._abort_out

    def _loop_state(self, g):
        ptr = lambda t: t.data_ptr() if t is not None else None
        return _lib.LoopState(ptr(g.x_cur), ptr(g.alive), ptr(g.sa), ptr(g.collided), ptr(g.ja), ptr(g.last_x), ptr(g.last_u),
                              ptr(g.x_abort), ptr(g.u_abort), ptr(g._jt), ptr(g.x_log), ptr(g.u_log), ptr(g.r_log),
                              ptr(getattr(g, '_resumed', None)))

    def loop_pre(self, g, r, pending, u_other, stepping):
        """scripts/mpc.py:130-151 for the group ``g`` (closed_loop._DeviceGroup)"""
        ls = self._loop_state(g)
        with self._ordered(1):
            self._chk(self.L.smpc_loop_pre(self.h, g._B, g._Nb, C.byref(ls), r.data_ptr() if r is not None else None,
                                           pending.data_ptr() if pending is not None else None, u_other.data_ptr(), stepping.data_ptr()))

    def loop_classify_aborts(self, g, abort, any_event):
        """scripts/mpc.py:137-141 vs 161-190: which of this step's aborts open an abort event (smpc_loop_classify_aborts)"""
        ls = self._loop_state(g)
        quirks = int(bool(getattr(self.problem.params, 'reference_quirks', True)))
        with self._ordered(1):
            self._chk(self.L.smpc_loop_classify_aborts(self.h, g._B, C.byref(ls), quirks, abort.data_ptr(), any_event.data_ptr()))

    def loop_apply_backup(self, g, rows, status_c, x_c, u_c, viable, u, pending):
        """scripts/mpc.py:161-190 (second half) for the previous step's abort events, see smpc_loop_apply_backup"""
        ls = self._loop_state(g)
        with self._ordered(1):
            self._chk(self.L.smpc_loop_apply_backup(self.h, g._B, g._Nb, C.byref(ls), int(rows.shape[0]), rows.data_ptr(), status_c.data_ptr(),
                                                    x_c.data_ptr(), u_c.data_ptr(), viable.data_ptr(), u.data_ptr(), pending.data_ptr()))

    def loop_post(self, g, u, joints_noisy=None, tau_noise=None):
        """scripts/mpc.py:240-264: plant, outcome tests, logs, j += 1"""
        ls, pp = self._loop_state(g), self._policy_params()
        with self._ordered(1):
            self._chk(self.L.smpc_loop_post(self.h, g._B, C.byref(pp), C.byref(ls), u.data_ptr(),
                                            joints_noisy.data_ptr() if joints_noisy is not None else None,
                                            tau_noise.data_ptr() if tau_noise is not None else None))

    def plant_step(self, x, u, joints_noisy=None, tau_noise=None, out=None):
        """AdamModel.integrate (env_model.py:192-206) for B instances.  ``out`` (device path): (x_next, u_eff) tensors to fill."""
        B = x.shape[0]
        if _is_torch(x):
            import torch
            xn, ue = out if out is not None else (torch.empty_like(x), torch.empty_like(u))
            jn = joints_noisy.data_ptr() if joints_noisy is not None else None
            tn = tau_noise.data_ptr() if tau_noise is not None else None
            with self._ordered(1):
                self._chk(self.L.smpc_plant_step(self.h, B, x.data_ptr(), u.data_ptr(), jn, tn, xn.data_ptr(),
                                                 ue.data_ptr(), 1))
            return xn, ue
        xx, uu = np.ascontiguousarray(x, np.float64), np.ascontiguousarray(u, np.float64)
        xn, ue = np.empty_like(xx), np.empty_like(uu)
        jn = tn = None
        if joints_noisy is not None:
            joints_noisy = np.ascontiguousarray(joints_noisy, JOINT_DTYPE)
            assert joints_noisy.shape == (B, self.nq)
            jn = joints_noisy.ctypes.data
        if tau_noise is not None:
            tau_noise = np.ascontiguousarray(tau_noise, np.float64)
            tn = tau_noise.ctypes.data
        self._chk(self.L.smpc_plant_step(self.h, B, xx.ctypes.data, uu.ctypes.data, jn, tn, xn.ctypes.data,
                                         ue.ctypes.data, 0))
        return xn, ue
