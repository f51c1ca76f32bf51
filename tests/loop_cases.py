"""Test infrastructure for the closed-loop driver kernels (k_loop_pre, k_loop_classify_aborts, k_loop_apply_backup, k_loop_post;
kernels_policy.hpp, reached through smpc_loop_*): one plain numpy statement per entry point, scripted state tables in which every
instance belongs to a named branch class, and a scripted closed-loop scenario with a table-driven controller.

The statements are written from the text of include/smpc.h and the lines of the reference's scripts/mpc.py that it cites
(:130-151 before the controller's step, :137-141 vs :161-190 for the aborts, :161-190 for the backup outcome, :240-264 after
the plant step).  They loop over instances one at a time, share nothing with closed_loop._HostGroup or the kernels, and each
takes a dict of arrays and returns a new dict: every array the entry point does not write comes back unchanged, so comparing
whole dicts also checks what must NOT have been touched.

Only tests import this file.  tests/test_loop_kernels_host.py pins the statements to oracle/policy_oracle.py::run_closed_loop;
tests/test_loop_kernels_gpu.py holds the kernels against the statements.
"""
import numpy as np

from oracle import policy_oracle as po

KP, KD, KD_HOLD = 1.0, 1e2, 3e2          # scripts/mpc.py:97 and the hold law's own gain, :144
V_REST = 5e-3                             # scripts/mpc.py:138
EPS = float(np.finfo(np.float64).eps)

U8, I64, I32 = np.uint8, np.int64, np.int32


def _copy(d):
    return {k: (None if v is None else np.array(v, copy=True)) for k, v in d.items()}


def _pd(u_ff, x, x_ref, nq, kd):
    """u_ff - (kp dq + kd dv) in plain double arithmetic, and the bound on what an fma contraction of kp dq + kd dv may change:
    4 eps (|u_ff| + kp |dq| + kd |dv|) per component"""
    dq, dv = x[:nq] - x_ref[:nq], x[nq:] - x_ref[nq:]
    u = u_ff - (KP * dq + kd * dv)
    return u, 4.0 * EPS * (np.abs(u_ff) + KP * np.abs(dq) + kd * np.abs(dv))


# =========================================================================================================================
# the four statements
# =========================================================================================================================
def loop_pre(d, Nb):
    """smpc_loop_pre (scripts/mpc.py:130-151 before the controller's step).  Reads x_cur, alive, sa, ja, x_abort, u_abort, step,
    r (or None), pending (or None); writes sa, ja, u_other, stepping, resumed (unless None), row `step` of r_log (unless None).
    Adds 'u_bound' [B][nq], the rounding allowance of u_other (zero where the control is an exact 0)."""
    o = _copy(d)
    B, nx = d['x_cur'].shape
    nq = nx // 2
    j = int(d['step'][0])
    o['u_bound'] = np.zeros((B, nq))
    for b in range(B):
        x = d['x_cur'][b]
        alive, sa, ja = bool(d['alive'][b]), bool(d['sa'][b]), int(d['ja'][b])
        u, bound, resume = np.zeros(nq), np.zeros(nq), False
        if alive and sa:                                                      # :130
            if ja < Nb:                                                       # :132-134  follow the backup trajectory
                u, bound = _pd(d['u_abort'][b, ja], x, d['x_abort'][b, ja], nq, KD)
            elif np.all(x[nq:] < V_REST):                                     # :138  at rest (signed, as there): back to MPC
                resume, sa = True, False
            else:                                                             # :144  hold the last node
                u, bound = _pd(np.zeros(nq), x, d['x_abort'][b, Nb], nq, KD_HOLD)
            ja += 1                                                           # :146
        pending = d.get('pending') is not None and bool(d['pending'][b])
        stepping = alive and not sa and not pending
        o['sa'][b], o['ja'][b], o['u_other'][b], o['u_bound'][b], o['stepping'][b] = sa, ja, u, bound, stepping
        if d.get('resumed') is not None:
            o['resumed'][b] = resume and stepping
        if d.get('r_log') is not None:
            o['r_log'][j, b] = d['r'][b] if (stepping and d.get('r') is not None) else -1
    return o


def classify_aborts(d, quirks):
    """smpc_loop_classify_aborts (scripts/mpc.py:137-141 vs :161-190).  Reads abort, resumed (or None), sa; writes abort, sa,
    any_event (always: 1 if an event remains, else 0)."""
    o = _copy(d)
    any_event = 0
    for b in range(len(d['abort'])):
        if not d['abort'][b]:
            continue
        if quirks and d.get('resumed') is not None and d['resumed'][b]:
            o['sa'][b], o['abort'][b] = 1, 0                                  # inside `if sa_flag:`: no event, in abort again
        else:
            any_event = 1
    o['any_event'][0] = any_event
    return o


def apply_backup(d, Nb):
    """smpc_loop_apply_backup (scripts/mpc.py:161-190, second half) for the events rows / status_c / x_c / u_c of the PREVIOUS
    step (step - 1).  Writes, of the event rows only: pending, and either collided / alive / last_x / last_u (failed) or x_abort /
    u_abort / sa / viable / ja / u (solved).  Adds 'u_bound' like loop_pre."""
    o = _copy(d)
    B, nx = d['x_cur'].shape
    nq = nx // 2
    j = int(d['step'][0]) - 1
    o['u_bound'] = np.zeros((B, nq))
    for c, b in enumerate(d['rows']):
        o['pending'][b] = 0
        if d['status_c'][c] != 0:                                             # :180-187  lost at the step of the event
            o['collided'][b], o['alive'][b], o['last_x'][b], o['last_u'][b] = 1, 0, j, j
            continue
        o['x_abort'][b], o['u_abort'][b] = d['x_c'][c], d['u_c'][c]           # :190
        o['sa'][b], o['ja'][b] = 1, 1                                         # :188 and this step's tracking of node 0, :132-134,146
        o['viable'][b] = min(int(d['viable'][b]) + 1, 255)                    # :189, as a saturating count
        o['u'][b], o['u_bound'][b] = _pd(d['u_c'][c, 0], d['x_cur'][b], d['x_c'][c, 0], nq, KD)
    return o


def loop_post(d, x_next, ok_next):
    """smpc_loop_post (scripts/mpc.py:240-264) given the plant's next states and their verdicts (from the CPU oracle).  Writes row
    `step` of u_log and row `step + 1` of x_log for every instance (what is valid is told by last_x / last_u), the outcome flags
    of the live instances whose new state fails, x_cur of the live ones whose new state passes, and step += 1."""
    o = _copy(d)
    j = int(d['step'][0])
    o['u_log'][j], o['x_log'][j + 1] = d['u'], x_next
    for b in range(d['x_cur'].shape[0]):
        if not d['alive'][b]:
            continue
        if ok_next[b]:
            o['x_cur'][b] = x_next[b]
        else:                                                                 # :246-264  the failing state stays logged
            o['last_x'][b], o['last_u'][b], o['collided'][b], o['alive'][b] = j + 1, j, 1, 0
    o['step'][0] = j + 1
    return o


def oracle_next(oracle, prob, par, x_cur, u, joints_noisy=None, tau_noise=None):
    """(x_next, ok_next) of smpc_loop_post's plant step and state test, from the CPU oracle"""
    x_next, _ = oracle.plant_step(x_cur, u, joints_noisy, tau_noise)
    ok = oracle.check_trajectory(x_next[:, None, :], prob.x_min, prob.x_max, par.tol_x, prob.row_check[:, 0], prob.row_check[:, 1])
    return x_next, np.asarray(ok, bool)


# =========================================================================================================================
# scripted state tables: every instance belongs to a named branch class
# =========================================================================================================================
CLASSES = ('live', 'dead', 'follow_0', 'follow_Nb-2', 'follow_Nb-1', 'hold_Nb', 'hold_Nb+3', 'rest_all_below', 'rest_one_above',
           'rest_one_exact', 'rest_one_nextafter', 'rest_minus_3', 'pending', 'sa_on_dead', 'rest_and_pending')


def expected_of_class(cls):
    """(stepping, resumed, kind of u_other) the statement must give for a class: a check of the table itself"""
    return {'live': (1, 0, 'zero'), 'dead': (0, 0, 'zero'), 'follow_0': (0, 0, 'follow'), 'follow_Nb-2': (0, 0, 'follow'),
            'follow_Nb-1': (0, 0, 'follow'), 'hold_Nb': (0, 0, 'hold'), 'hold_Nb+3': (0, 0, 'hold'), 'rest_all_below': (1, 1, 'zero'),
            'rest_one_above': (0, 0, 'hold'), 'rest_one_exact': (0, 0, 'hold'), 'rest_one_nextafter': (1, 1, 'zero'),
            'rest_minus_3': (1, 1, 'zero'), 'pending': (0, 0, 'zero'), 'sa_on_dead': (0, 0, 'zero'),
            'rest_and_pending': (0, 0, 'zero')}[cls]


def state_table(prob, Nb, B, seed=0, offset=0, n_steps=5, step=2):
    """One state of the loop for B instances, instance b of class CLASSES[(b + offset) % len(CLASSES)], with everything the four
    entry points take.  Backup tables, logs and outputs are filled with distinct random values, so that a wrong node, row or
    instance index shows and so does a write where none belongs."""
    rng = np.random.default_rng(1000 * seed + 17 * Nb + B)
    nq = prob.nq
    nx = 2 * nq
    cls = [CLASSES[(b + offset) % len(CLASSES)] for b in range(B)]
    q = rng.uniform(prob.lbx[:nq] + 0.05, prob.ubx[:nq] - 0.05, (B, nq))
    out_of_box = rng.random(B) < 0.15                                         # (loop_post: some next states leave the joint box)
    q[out_of_box, rng.integers(0, nq, int(out_of_box.sum()))] += 7.0
    v = rng.uniform(-0.5, 0.5, (B, nq))
    alive, sa, ja, pending = np.ones(B, U8), np.zeros(B, U8), rng.integers(0, 4, B).astype(I64), np.zeros(B, U8)
    small = lambda: rng.uniform(-4e-3, 4e-3, nq)
    for b, c in enumerate(cls):
        i = int(rng.integers(0, nq))
        if c == 'dead':
            alive[b] = 0
        elif c.startswith('follow'):
            sa[b], ja[b] = 1, {'follow_0': 0, 'follow_Nb-2': max(Nb - 2, 0), 'follow_Nb-1': Nb - 1}[c]
        elif c.startswith('hold'):
            sa[b], ja[b] = 1, Nb + (3 if c.endswith('+3') else 0)
            v[b, i] = abs(v[b, i]) + 0.01                                     # (well above 5e-3)
        elif c.startswith('rest'):
            sa[b], ja[b], v[b] = 1, Nb + int(rng.integers(0, 3)), small()
            if c == 'rest_one_above':
                v[b, i] = 6e-3
            elif c == 'rest_one_exact':
                v[b, i] = V_REST
            elif c == 'rest_one_nextafter':
                v[b, i] = np.nextafter(V_REST, 0.0)
            elif c == 'rest_minus_3':
                v[b, i] = -3.0
            elif c == 'rest_and_pending':
                pending[b] = 1
        elif c == 'pending':
            pending[b] = 1
        elif c == 'sa_on_dead':
            alive[b], sa[b], ja[b] = 0, 1, 1
    x_cur = np.hstack([q, v])
    x_abort = x_cur[:, None, :] + rng.uniform(-0.2, 0.2, (B, Nb + 1, nx))
    u_abort = rng.uniform(-3, 3, (B, Nb, nq))
    d = dict(x_cur=x_cur, alive=alive, sa=sa, collided=(1 - alive).astype(U8), ja=ja,
             last_x=np.where(alive, n_steps, rng.integers(0, step + 1, B)).astype(I64),
             last_u=np.where(alive, n_steps - 1, rng.integers(0, step + 1, B)).astype(I64),
             x_abort=x_abort, u_abort=u_abort, step=np.array([step], I64),
             x_log=rng.uniform(-1, 1, (n_steps + 1, B, nx)), u_log=rng.uniform(-1, 1, (n_steps, B, nq)),
             r_log=rng.integers(-50, -40, (n_steps, B)).astype(I64), resumed=rng.integers(0, 2, B).astype(U8),
             # smpc_loop_pre
             r=rng.integers(0, 30, B).astype(I64), pending=pending, u_other=rng.uniform(-9, 9, (B, nq)),
             stepping=rng.integers(0, 2, B).astype(U8),
             # smpc_loop_post
             u=rng.uniform(-3, 3, (B, nq)))
    # smpc_loop_apply_backup: events on about half of the instances, in no order, solved and failed, on live and on lost instances
    n_c = max(1, B // 2)
    rows = rng.permutation(B)[:n_c].astype(I64)
    if n_c > 2 and np.all(np.diff(rows) > 0):
        rows = rows[::-1].copy()
    viable = rng.integers(0, 256, B).astype(U8)
    viable[rows[0::3]], viable[rows[1::3]], viable[rows[2::3]] = 0, 254, 255
    d.update(rows=rows, status_c=np.where(rng.random(n_c) < 0.4, 4, 0).astype(I32), x_c=rng.uniform(-1, 1, (n_c, Nb + 1, nx)),
             u_c=rng.uniform(-3, 3, (n_c, Nb, nq)), viable=viable)
    if n_c >= 6:                                                             # every preload meets a solved event
        d['status_c'][:6] = [0, 0, 0, 4, 4, 4]
    # smpc_loop_classify_aborts
    d.update(abort=rng.integers(0, 2, B).astype(U8), any_event=np.array([1], I32))
    return d, cls


def check_table(d, cls, Nb):
    """a table of at least 63 instances is what its class names say: loop_pre's statement takes the branch each class was built
    for, and the events are solved and failed, unsorted, on live and on lost instances, with every preload of the count"""
    assert set(cls) == set(CLASSES)
    o = loop_pre(pick(d, PRE_KEYS), Nb)
    j = int(d['step'][0])
    for b, c in enumerate(cls):
        stp, res, kind = expected_of_class(c)
        assert (int(o['stepping'][b]), int(o['resumed'][b])) == (stp, res), (Nb, b, c)
        assert np.all(o['u_other'][b] == 0) == (kind == 'zero'), (Nb, b, c)
        assert int(o['ja'][b]) == int(d['ja'][b]) + (kind != 'zero' or res or c == 'rest_and_pending'), (Nb, b, c)
        assert int(o['r_log'][j, b]) == (int(d['r'][b]) if stp else -1)
    rows, st = d['rows'], d['status_c']
    assert np.any(np.diff(rows) < 0) and len(set(rows.tolist())) == len(rows)
    for v in (0, 254, 255):
        assert np.any((d['viable'][rows] == v) & (st == 0))
    assert np.any(d['alive'][rows] == 0) and np.any(st != 0) and np.any(st == 0)
    o = apply_backup(pick(d, BACKUP_KEYS), Nb)
    assert set(o['viable'][rows[st == 0]].tolist()) >= {1, 255} and not np.any(o['pending'][rows])
    assert d['abort'].any() and d['resumed'].any() and (d['abort'] & d['resumed']).any() and (d['abort'] & (1 - d['resumed'])).any()


PRE_KEYS = ('x_cur', 'alive', 'sa', 'ja', 'x_abort', 'u_abort', 'step', 'r_log', 'resumed', 'r', 'pending', 'u_other', 'stepping')
CLASSIFY_KEYS = ('sa', 'resumed', 'abort', 'any_event')
BACKUP_KEYS = ('x_cur', 'alive', 'sa', 'collided', 'ja', 'last_x', 'last_u', 'x_abort', 'u_abort', 'step', 'rows', 'status_c', 'x_c',
               'u_c', 'viable', 'u', 'pending')
POST_KEYS = ('x_cur', 'alive', 'collided', 'last_x', 'last_u', 'step', 'x_log', 'u_log', 'u')
STATE_KEYS = ('x_cur', 'alive', 'sa', 'collided', 'ja', 'last_x', 'last_u', 'x_abort', 'u_abort', 'step', 'x_log', 'u_log', 'r_log',
              'resumed')


def pick(d, keys, **null):
    """the sub-dict an entry point sees; ``name=None`` passes that argument as NULL"""
    s = {k: d[k] for k in keys}
    s.update(null)
    return s


def differences(got, want, bounds=None):
    """names of the arrays of ``want`` that ``got`` does not reproduce bit for bit.  ``bounds`` {name: array or scalar}: those
    arrays within the bound instead -- and bit for bit wherever the bound is zero"""
    bad = []
    for k, w in want.items():
        if k == 'u_bound' or w is None:
            continue
        g = np.asarray(got[k])
        if g.shape != w.shape or g.dtype != w.dtype:
            bad.append(f'{k}: {g.dtype}{g.shape} for {w.dtype}{w.shape}')
        elif bounds is not None and k in bounds:
            bound = np.broadcast_to(np.asarray(bounds[k], float), w.shape)
            exact = bound == 0
            if not (np.all(np.abs(g - w)[~exact] <= bound[~exact]) and g[exact].tobytes() == w[exact].tobytes()):
                bad.append(k)
        elif g.tobytes() != w.tobytes():
            bad.append(k)
    return bad


PAD, SENTINEL = 256, 0xA5
DEVICE = 'cuda'          # ('cpu' lets the GPU tests' own plumbing be tried without a device, with the statements as the engine)


class Dev:
    """arrays on the device (the GPU tests' plumbing), each in a buffer of its own between PAD bytes of sentinel"""

    def __init__(self, arrays):
        import torch
        self.torch, self.buf, self.t, self.meta = torch, {}, {}, {}
        for k, a in arrays.items():
            self.put(k, a)

    def put(self, k, a):
        torch = self.torch
        if a is None:
            self.buf.pop(k, None)
            self.t[k] = None
            return
        a = np.ascontiguousarray(a)
        n = a.nbytes
        buf = torch.full((2 * PAD + n,), SENTINEL, dtype=torch.uint8, device=DEVICE)
        if n:
            buf[PAD:PAD + n] = torch.from_numpy(a.reshape(-1).view(np.uint8).copy()).to(DEVICE)
        self.buf[k], self.meta[k] = buf, (a.dtype, a.shape)
        dtype = getattr(torch, a.dtype.name)
        self.t[k] = buf[PAD:PAD + n].view(dtype).view(a.shape) if n else torch.empty(a.shape, dtype=dtype, device=DEVICE)

    def write(self, k, a):
        """new contents at the same address"""
        assert (a.dtype, a.shape) == self.meta[k]
        self.t[k].copy_(self.torch.from_numpy(np.ascontiguousarray(a)).to(DEVICE))

    def host(self):
        """{name: numpy array}; the sentinels must be intact"""
        if DEVICE == 'cuda':
            self.torch.cuda.synchronize()
        out = {}
        for k, t in self.t.items():
            if t is None:
                out[k] = None
                continue
            raw = self.buf[k].cpu().numpy()
            n = raw.size - 2 * PAD
            assert np.all(raw[:PAD] == SENTINEL) and np.all(raw[PAD + n:] == SENTINEL), f'{k}: wrote outside its array'
            dtype, shape = self.meta[k]
            out[k] = raw[PAD:PAD + n].copy().view(dtype).reshape(shape)
        return out


# =========================================================================================================================
# the scripted scenario: a table-driven controller, scripted aborts and scripted backup outcomes
# =========================================================================================================================
class Scenario:
    """nq = 6, Nb = 3, 24 steps, 10 instances.  The controller is a table: u[j][b] = table[j][b], abort[j][b] = script[j][b]; the
    backup OCP of instance b's k-th event returns ``backup(b, k, x_viable)``; its receding index at step j is r_table[j][b].

      0  never aborts
      1  abort at step 2 -> follows (3 nodes) -> holds -> at rest -> resumes MPC to the end
      2  abort at step 3, the backup OCP fails: lost at step 3
      3  abort at step 2, and again on every later step it steps its controller: aborts on each step it resumes
      4  driven out of the velocity box by its table
      5  two events: abort at step 1, resumes, abort at step 17
      6  abort at the last step, backup solved
      7  abort at the last step, backup fails
      8  like 4, and aborts at the very step whose next state leaves the box (backup solved: an event on a lost instance)
      9  abort at step 4 into a backup trajectory whose last node moves: holds to the end, never at rest
    """
    nq, Nb, n_steps, B = 6, 3, 24, 10
    LEAVES = 6                                       # the step of instance 4 and 8 whose next state is out of the box (asserted)

    def __init__(self, prob, par, oracle):
        from conftest import sample_instances
        self.prob, self.par, self.oracle = prob, par, oracle
        nq, n, B = self.nq, self.n_steps, self.B
        rng = np.random.default_rng(2024)
        self.x0 = sample_instances(prob, B, seed=3, vel_scale=0.0, margin=0.3)
        self.x0[:, nq:] = rng.uniform(-0.02, 0.02, (B, nq))
        self.table = rng.uniform(-0.5, 0.5, (n, B, nq))
        self.script = np.zeros((n, B), bool)
        self.script[2, 1] = self.script[3, 2] = self.script[4, 9] = True
        self.script[2:, 3] = True
        self.script[1, 5] = self.script[17, 5] = True
        self.script[n - 1, 6] = self.script[n - 1, 7] = True
        for b in (4, 8):                             # velocity of joint 2 near its bound, and a steady push (1 rad/s^2 for dt = 5e-3)
            self.x0[b, nq + 2] = prob.x_max[nq + 2] + par.tol_x - (self.LEAVES + 0.5) * par.dt * 1.0
            self.table[:, b, :] = 0.0
            self.table[:, b, 2] = 1.0
        self.script[self.LEAVES, 8] = True
        self.r_table = rng.integers(0, 30, (n, B)).astype(I64)      # the receding index the controller shows at each step

    def backup(self, b, k, xv):
        """(status, x_abort [Nb+1][nx], u_abort [Nb][nq]) of instance b's k-th abort event: slow trajectories near the viable
        state, distinct in every node, last node at rest (instance 9: moving, so that the hold law never comes to rest)"""
        rng = np.random.default_rng(100 * b + k + 1)
        nq, Nb = self.nq, self.Nb
        xa = np.repeat(np.asarray(xv, float)[None], Nb + 1, 0)
        xa[:, :nq] += rng.uniform(-0.01, 0.01, (Nb + 1, nq))
        xa[:, nq:] = rng.uniform(-0.01, 0.01, (Nb + 1, nq))
        xa[Nb - 1, nq] = 0.03                        # (still moving when the trajectory ends: at least one step of the hold law)
        xa[Nb, nq:] = 0.02 if b == 9 else 0.0
        ua = rng.uniform(-0.3, 0.3, (Nb, nq))
        return (4 if b in (2, 7) else 0), xa, ua

    # ---- the scalar oracle's run -------------------------------------------------------------------------------------------------
    def reference(self, quirks):
        """run_closed_loop per instance with the table as the controller; returns (results, margin): margin is the smallest
        distance of any tested quantity from its threshold -- the 5e-3 velocity test, the box +- tol_x, the rows' check bounds"""
        out, margins = [], []
        for b in range(self.B):
            num = _ScriptNumerics(self, b)
            inst = num.inst = po.PolicyInstance('receding', 1, 2 * self.nq, self.nq)
            xg = np.repeat(self.x0[b][None], 2, 0)
            r = po.run_closed_loop(inst, num, xg, np.zeros((1, self.nq)), self.n_steps, self.Nb, self.nq, on_step=num.on_step,
                                   step_fn=num.step, reference_quirks=quirks)
            r['aborts_on_resume'] = [j for j in r['resumes'] if self.script[j, b]]
            rest = [float(np.abs(r['x'][j][self.nq:] - V_REST).min()) for j in r['rest_tests']]      # mpc.py:138
            out.append(r)
            margins.append(min([num.margin] + rest))
        return out, min(margins)

    # ---- the four statements chained in _DeviceGroup's order --------------------------------------------------------------------
    def initial_state(self):
        nq, n, B, Nb = self.nq, self.n_steps, self.B, self.Nb
        d = dict(x_cur=self.x0.copy(), alive=np.ones(B, U8), sa=np.zeros(B, U8), collided=np.zeros(B, U8), ja=np.zeros(B, I64),
                 last_x=np.full(B, n, I64), last_u=np.full(B, n - 1, I64), x_abort=np.zeros((B, Nb + 1, 2 * nq)),
                 u_abort=np.zeros((B, Nb, nq)), step=np.zeros(1, I64), x_log=np.full((n + 1, B, 2 * nq), np.nan),
                 u_log=np.full((n, B, nq), np.nan), r_log=np.full((n, B), -1, I64), resumed=np.zeros(B, U8),
                 r=np.zeros(B, I64), pending=np.zeros(B, U8), u_other=np.zeros((B, nq)), stepping=np.ones(B, U8), u=np.zeros((B, nq)),
                 viable=np.zeros(B, U8), abort=np.zeros(B, U8), any_event=np.zeros(1, I32))
        d['x_log'][0] = self.x0
        return d

    def scripted_step(self, d):
        """the stand-in for the controller's step: u = where(stepping, table, u_other), abort = script & stepping"""
        j = int(d['step'][0])
        stp = d['stepping'].astype(bool)
        return np.where(stp[:, None], self.table[j], d['u_other']), (self.script[j] & stp).astype(U8)

    def events_of(self, d, n_events):
        """(rows, status_c, x_c, u_c) of the events left in d['abort'] -- the backup solves from the instances' current states"""
        rows = np.where(d['abort'])[0].astype(I64)
        sols = []
        for b in rows:
            sols.append(self.backup(int(b), n_events[b], d['x_cur'][b]))
            n_events[b] += 1
        return dict(rows=rows, status_c=np.array([s[0] for s in sols], I32), x_c=np.array([s[1] for s in sols]),
                    u_c=np.array([s[2] for s in sols]))

    def chain(self, quirks):
        """The run as the four statements in the device loop's order: per step loop_pre, the scripted step, classify, the previous
        step's events, loop_post; the last step's events after the loop.  Returns (state, events [(step, instance)])."""
        d = self.initial_state()
        n_events, events, inflight = np.zeros(self.B, int), [], None
        for j in range(self.n_steps):
            d['r'] = self.r_table[j]
            d = loop_pre(d, self.Nb)
            d['u'], d['abort'] = self.scripted_step(d)
            d = classify_aborts(d, quirks)
            if inflight is not None:
                d = apply_backup(dict(d, **inflight), self.Nb)
                inflight = None
            if d['any_event'][0]:
                inflight = self.events_of(d, n_events)
                events += [(j, int(b)) for b in inflight['rows']]
                d['pending'] = d['abort'].copy()
            x_next, ok_next = oracle_next(self.oracle, self.prob, self.par, d['x_cur'], d['u'])
            d = loop_post(d, x_next, ok_next)
        if inflight is not None:
            d = apply_backup(dict(d, **inflight), self.Nb)
        return d, events


def blanked_logs(d):
    """the logs as the reference leaves them: NaN after an instance's last valid row (closed_loop._Group.results)"""
    n = d['u_log'].shape[0]
    x = np.transpose(d['x_log'], (1, 0, 2)).copy()
    u = np.transpose(d['u_log'], (1, 0, 2)).copy()
    steps = np.arange(n + 1)[None, :]
    x[steps > d['last_x'][:, None]] = np.nan
    u[steps[:, :n] > d['last_u'][:, None]] = np.nan
    return x, u


class _ScriptNumerics:
    """what run_closed_loop asks of its numerics, for ONE instance of a Scenario: the CPU oracle's plant and state tests, the
    scripted backup outcomes, and -- as ``step`` -- the table-driven controller.  Keeps the margins of the state tests."""

    def __init__(self, sc, b):
        self.sc, self.b, self.j, self.k = sc, b, 0, 0
        self.margin = np.inf

    def on_step(self, j):
        self.j = j
        self.inst.r = int(self.sc.r_table[j, self.b])

    def step(self, inst, numerics, x):
        sc, j, b = self.sc, self.j, self.b
        inst.x_viable = np.array(x, float)
        abort = bool(sc.script[j, b])
        return sc.table[j, b].copy(), abort

    def plant(self, x, u):
        xn, _ = self.sc.oracle.plant_step(np.asarray(x, float)[None], np.asarray(u, float)[None])
        return xn[0]

    def check_state_bounds(self, x):
        pr, tol = self.sc.prob, self.sc.par.tol_x
        x = np.asarray(x, float)
        self.margin = min(self.margin, float(np.abs(x - (pr.x_min - tol)).min()), float(np.abs(x - (pr.x_max + tol)).min()))
        return bool(np.all(x >= pr.x_min - tol) and np.all(x <= pr.x_max + tol))

    def check_collision(self, x):
        pr, o = self.sc.prob, self.sc.oracle
        x = np.asarray(x, float)
        xg = np.repeat(x[None, None, :], pr.N + 1, 1)
        rows = o.eval_nodes(xg, np.zeros((1, pr.N, pr.nu)), np.zeros((1, pr.N + 1, 5)))['row_val'][0, 0, :len(pr.row_check)]
        self.margin = min(self.margin, float(np.abs(rows - pr.row_check[:, 0]).min()), float(np.abs(rows - pr.row_check[:, 1]).min()))
        ok = bool(np.all(rows >= pr.row_check[:, 0]) and np.all(rows <= pr.row_check[:, 1]))
        assert ok == bool(o.check_trajectory(x[None, None, :], pr.x_min, pr.x_max, 1e30, pr.row_check[:, 0], pr.row_check[:, 1])[0])
        return ok

    def backup_solve(self, xv):
        out = self.sc.backup(self.b, self.k, xv)
        self.k += 1
        return out

    def converged(self, x_last):
        return False
