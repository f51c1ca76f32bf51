"""Shared pieces of the safe-set-network shape tests (test_mlp_shapes_host.py, test_mlp_shapes_gpu.py): seeded networks of any width
and depth for any ``n_dof_safe_set <= nq``, the float64 numpy statement of the network's row, and the yardstick of the error bound.
Not a test module.

The statement is written from the reference's definition of the row (safe_set.py:82-94), not from the kernels:

    v   = qd[:nd] + eps e_0,   s = [(q[:nd] - mean) / std ; v / |v|]            (the network sees the first nd joints only)
    y   = net(s)                                                               (Linear, act, ..., Linear; any depth)
    g   = y (100 - alpha) / 100 - |v|
    dg/dx over all 2 nq state entries: zero in the slots of the joints nd..nq-1, position and velocity alike

Errors are measured in the SPREAD norm: max |a - ref| over the live rows of a case divided by (max - min) of the float64 reference
over those rows -- of the network's share kap y for the value (|v| is float64 arithmetic on both sides and, like the output bias,
would only hide an error of the network behind a large constant), of the block for the gradient's position and velocity blocks.
A case's yardstick E_o is the CPU oracle's fp32 error against float64 in that norm; the engine's bound is max(16 E_o, floor) with
the floors 2e-5 (value) and 2e-4 (gradient) of test_gpu_parity.py."""
import functools

import numpy as np

from conftest import constant_guess, sample_instances

ACTS = ('gelu', 'relu', 'elu', 'tanh', 'silu')
VAL_FLOOR, GRAD_FLOOR, FOLD = 2e-5, 2e-4, 16.0
MIN_Y_SPREAD = 0.1


class PlainNet:
    """weights [out, in] / biases [out] in fp32, an activation name and the state normalisation: what BatchedOcpSolver.set_mlp and
    Oracle(prob, (W, b, act)) take.  Any depth.  The last ``n_ctx`` columns of ``weights[0]`` are context inputs when ctx_mean /
    ctx_std are given (SafeSetNet's convention)."""

    def __init__(self, weights, biases, act, mean, std, ctx_mean=None, ctx_std=None):
        self.weights = [np.ascontiguousarray(w, np.float32) for w in weights]
        self.biases = [np.ascontiguousarray(b, np.float32) for b in biases]
        self.act = act
        self.mean, self.std = np.asarray(mean, np.float64).reshape(-1), np.asarray(std, np.float64).reshape(-1)
        self.dims = [self.weights[0].shape[1]] + [w.shape[0] for w in self.weights]
        self.ctx_mean = np.zeros(0) if ctx_mean is None else np.asarray(ctx_mean, np.float64).reshape(-1)
        self.ctx_std = np.ones(self.ctx_mean.size) if ctx_std is None else np.asarray(ctx_std, np.float64).reshape(-1)
        self.n_ctx = int(self.ctx_mean.size)

    def folded(self, ctx):
        """the plain net this one is for the context ``ctx``: b0 + Wc ((ctx - ctx_mean) / ctx_std) formed in float64, rounded to fp32"""
        ns = self.dims[0] - self.n_ctx
        W0 = self.weights[0].astype(np.float64)
        b0 = self.biases[0].astype(np.float64) + W0[:, ns:] @ ((np.asarray(ctx, np.float64) - self.ctx_mean) / self.ctx_std)
        return PlainNet([self.weights[0][:, :ns]] + self.weights[1:], [b0.astype(np.float32)] + self.biases[1:], self.act, self.mean, self.std)


def make_net(prob, H, L, act='gelu', seed=0, n_ctx=0, gain=2.0, out_bias=3.0):
    """L Linear layers (L - 1 hidden ones of width H) on 2 nd + n_ctx inputs.  Weights U(+-gain / sqrt(fan_in)), biases U(+-0.5): the
    gain keeps the signal alive through six layers, so that the output varies over the rows of a case (MIN_Y_SPREAD, asserted of
    the float64 statement by spreads()); the output bias keeps the set non-empty, as SafeSetNet.synthetic's does."""
    nd = prob.params.n_dof_safe_set
    rng = np.random.default_rng([int(seed), int(H), int(L), ACTS.index(act), int(nd), int(n_ctx)])
    dims = [2 * nd + n_ctx] + [H] * (L - 1) + [1]
    Ws, bs = [], []
    for l in range(L):
        k = gain / np.sqrt(dims[l])
        Ws.append(rng.uniform(-k, k, (dims[l + 1], dims[l])).astype(np.float32))
        bs.append(rng.uniform(-0.5, 0.5, dims[l + 1]).astype(np.float32))
    bs[-1][:] = out_bias
    q_lo, q_hi = prob.x_min[:nd], prob.x_max[:nd]
    ctx = (np.linspace(-0.5, 0.5, n_ctx), np.linspace(0.5, 1.5, n_ctx)) if n_ctx else (None, None)
    return PlainNet(Ws, bs, act, 0.5 * (q_lo + q_hi), (q_hi - q_lo) / np.sqrt(12.0), *ctx)


@functools.lru_cache(maxsize=None)
def shape_problem(controller, nq, nd, N):
    """(par, prob): the Z1 with nq joints of which the network sees nd, the problem's normalisation set as make_net's nets have it"""
    from safe_mpc_amd.parser import Parameters
    from safe_mpc_amd.problem import OcpProblem
    par = Parameters({}, 'z1')
    par.nq, par.n_dof_safe_set, par.net_size, par.N = nq, nd, [2 * nd, 256, 1], N
    prob = OcpProblem(par, controller, 'ext', N=N)
    q_lo, q_hi = prob.x_min[:nd], prob.x_max[:nd]
    prob.set_normalisation(0.5 * (q_lo + q_hi), (q_hi - q_lo) / np.sqrt(12.0))
    return par, prob


# ---- the float64 statement ------------------------------------------------------------------------------------------------------------
def act64(name, a):
    """value and derivative of the activations parser.py offers, as torch.nn defines them, float64"""
    if name == 'relu':
        return np.maximum(a, 0.0), (a > 0).astype(np.float64)
    if name == 'elu':
        e = np.exp(np.minimum(a, 0.0))
        return np.where(a > 0, a, e - 1.0), np.where(a > 0, 1.0, e)
    if name == 'tanh':
        t = np.tanh(a)
        return t, 1.0 - t * t
    if name == 'silu':
        sg = 1.0 / (1.0 + np.exp(-a))
        return a * sg, sg * (1.0 + a * (1.0 - sg))
    if name == 'gelu':          # GELU(approximate='tanh')
        k0, k1 = np.sqrt(2.0 / np.pi), 0.044715
        th = np.tanh(k0 * (a + k1 * a ** 3))
        return 0.5 * a * (1.0 + th), 0.5 * (1.0 + th) + 0.5 * a * (1.0 - th * th) * k0 * (1.0 + 3.0 * k1 * a * a)
    raise ValueError(name)


def mlp64(net, s):
    """y [M] and dy/ds [M, in] of the fp32 weights in float64: forward sweep, then the reverse sweep for the single output"""
    a, ders = np.asarray(s, np.float64), []
    L = len(net.weights)
    for l in range(L):
        z = a @ net.weights[l].astype(np.float64).T + net.biases[l].astype(np.float64)
        if l + 1 < L:
            a, d = act64(net.act, z)
            ders.append(d)
        else:
            a = z
    delta = np.ones((a.shape[0], 1))
    for l in range(L - 1, -1, -1):
        if l + 1 < L:
            delta = delta * ders[l]
        delta = delta @ net.weights[l].astype(np.float64)
    return a[:, 0], delta


def features64(net, x, nq, eps):
    """s [M, 2 nd], v [M, nd], |v| [M] of states x [M, 2 nq]"""
    nd = net.mean.size
    v = x[:, nq:nq + nd].copy()
    v[:, 0] += eps
    vn = np.sqrt((v * v).sum(axis=1))
    return np.hstack([(x[:, :nd] - net.mean) / net.std, v / vn[:, None]]), v, vn


def row64(net, x, nq, eps, alpha):
    """(g [M], dg/dx [M, 2 nq], y [M]) of a plain net on states x [M, 2 nq]; alpha a scalar or [M]"""
    x = np.asarray(x, np.float64).reshape(-1, 2 * nq)
    nd = net.mean.size
    s, v, vn = features64(net, x, nq, eps)
    y, gs = mlp64(net, s)
    kap = (100.0 - np.asarray(alpha, np.float64)) / 100.0 * np.ones(x.shape[0])
    g = y * kap - vn
    dg = np.zeros((x.shape[0], 2 * nq))
    dg[:, :nd] = kap[:, None] * gs[:, :nd] / net.std
    # d(v/|v|)/dv = I/|v| - v v^T/|v|^3 (symmetric), d|v|/dv = v/|v|
    gv = gs[:, nd:]
    dg[:, nq:nq + nd] = kap[:, None] * (gv / vn[:, None] - v * ((gv * v).sum(axis=1) / vn ** 3)[:, None]) - v / vn[:, None]
    return g, dg, y


# ---- a case: a problem, a net, the nodes' states and switches ------------------------------------------------------------------------
class Case:
    """controller 'st' (terminal row: B rows) or 'constraint_everywhere' (the row on the nodes 1..N; ``switched``: about half the
    per-node switches off, the live count not a multiple of 16).  ``seed2``: other states for the second call on one handle."""

    def __init__(self, controller, nq, nd, H, L, B, N, act='gelu', switched=False, seed=0, n_ctx=0):
        self.controller, self.nq, self.nd, self.H, self.L, self.B, self.N = controller, nq, nd, H, L, B, N
        self.act, self.switched, self.seed = act, switched, seed
        self.par, self.prob = shape_problem(controller, nq, nd, N)
        self.net = make_net(self.prob, H, L, act, seed, n_ctx)
        self.name = f'{controller}-nq{nq}-nd{nd}-H{H}-L{L}-{act}-B{B}-N{N}' + ('-switched' if switched else '') + (f'-ctx{n_ctx}' if n_ctx else '')

    @functools.lru_cache(maxsize=None)
    def inputs(self, which=0):
        """(x0, xg, ug, p) -- states off the constant guess, velocities of every joint (the unseen ones included) non-zero"""
        return case_inputs(self.prob, self.B, self.seed + 5 * which + 1, self.switched)

    def live(self, p):
        on = p[:, :, 4] > 0
        on[:, 0] = False
        if self.controller == 'st':
            on[:, :self.N] = False
        return on

    def reference(self, which=0, net=None):
        """float64 (g, dg, y) on the live nodes of inputs(which), in the order of np.nonzero(live)"""
        x0, xg, ug, p = self.inputs(which)
        on = self.live(p)
        return row64(net or self.net, xg[on], self.nq, self.par.eps, p[on][:, 3])


def case_inputs(prob, B, seed, switched=False):
    N = prob.N
    x0 = sample_instances(prob, B, seed=seed, vel_scale=0.3)
    xg, ug, p = constant_guess(prob, x0)
    rng = np.random.default_rng(seed)
    xg[:, 1:] += 0.05 * rng.standard_normal(xg[:, 1:].shape)
    if switched:
        p[:, :, 4] = np.where(rng.uniform(size=p.shape[:2]) < 0.5, 1.0, -1.0)
        if int((p[:, 1:, 4] > 0).sum()) % 16 == 0:
            b, k = np.argwhere(p[:, 1:, 4] > 0)[0]
            p[b, 1 + k, 4] = -1.0
    return x0, xg, ug, p


def spread(a):
    a = np.asarray(a, np.float64)
    return float(a.max() - a.min())


def spreads(case, g, dg, y, p_on):
    """the three norms of a case from its float64 reference: of kap y (value), of the position and the velocity block of dg/dx.
    Asserts the conditions the norms rest on: the network's output varies over the rows, and so does every gradient block."""
    nq, nd = case.nq, case.nd
    kap = (100.0 - p_on[:, 3]) / 100.0
    sy, sv, sq, sd = spread(y), spread(kap * y), spread(dg[:, :nd]), spread(dg[:, nq:nq + nd])
    assert sy >= MIN_Y_SPREAD, (case.name, 'network output too flat over the rows', sy)
    assert sq > 0 and sd > 0, (case.name, sq, sd)
    return sv, sq, sd


def errors(case, val, grad, g, dg, norms):
    """(value error, gradient error) in the spread norm; val [M], grad [M, >= 2 nq] against the reference g, dg"""
    nq, nd = case.nq, case.nd
    sv, sq, sd = norms
    ev = np.abs(val - g).max() / sv
    eg = max(np.abs(grad[:, :nd] - dg[:, :nd]).max() / sq, np.abs(grad[:, nq:nq + nd] - dg[:, nq:nq + nd]).max() / sd)
    return float(ev), float(eg)


def oracle_of(case, net=None):
    from oracle.oracle import Oracle
    net = net or case.net
    return Oracle(case.prob, (net.weights, net.biases, net.act))


@functools.lru_cache(maxsize=None)
def yardstick(case, which=0, ctx=None):
    """(E_o, E_o_grad, value bound, gradient bound, norms) of a case: the CPU oracle's fp32 pass against the float64 statement over
    the live rows, and the bound the engine is held to.  ``ctx``: a context (tuple) the case's net is folded with first."""
    net = case.net.folded(np.array(ctx)) if ctx is not None else case.net
    x0, xg, ug, p = case.inputs(which)
    on = case.live(p)
    g, dg, y = case.reference(which, net)
    norms = spreads(case, g, dg, y, p[on])
    ev = oracle_of(case, net).eval_nodes(xg, ug, p)
    assert np.all(ev['nn_val'][~on] == 0.0) and np.all(ev['nn_grad'][~on] == 0.0)
    e_o, e_og = errors(case, ev['nn_val'][on], ev['nn_grad'][on], g, dg, norms)
    return e_o, e_og, max(FOLD * e_o, VAL_FLOOR), max(FOLD * e_og, GRAD_FLOOR), norms


def rows_reference(prob, net, x, alpha):
    """(g [M] float64, the absolute bound on an fp32 pass's g) of states x [M, 2 nq] for the forward-only consumers: the value
    bound of the spread norm, max(16 E_o, 2e-5) x spread(kap y), with E_o the oracle's error on these very rows (Oracle.nn_row)"""
    from oracle.oracle import Oracle
    nq, par = prob.nq, prob.params
    x = np.asarray(x, np.float64).reshape(-1, 2 * nq)
    alpha = np.asarray(alpha, np.float64) * np.ones(x.shape[0])
    g, dg, y = row64(net, x, nq, par.eps, alpha)
    sv = spread((100.0 - alpha) / 100.0 * y)
    assert spread(y) >= MIN_Y_SPREAD, ('network output too flat over the rows', spread(y))
    o = Oracle(prob, (net.weights, net.biases, net.act))
    e_o = max(abs(o.nn_row(x[m], alpha[m])[0] - g[m]) for m in range(x.shape[0])) / sv
    return g, max(FOLD * e_o, VAL_FLOOR) * sv


# ---- the cases -------------------------------------------------------------------------------------------------------------------------
# nn_dof < nq on the one-kernel passes (256 wide, three hidden layers) and on the layer-by-layer chain (H = 128)
ND_PAIRS = [(6, 5), (6, 3), (5, 4)]
SMALL_SHAPES = [('st', 17, 6, False), ('constraint_everywhere', 9, 7, True)]


@functools.lru_cache(maxsize=None)
def nd_case(family, nq, nd, controller, B, N, switched):
    return Case(controller, nq, nd, 256 if family != 'chain' else 128, 4, B, N, switched=switched, seed=11)


@functools.lru_cache(maxsize=None)
def wave_case(switched):
    return Case('constraint_everywhere', 6, 5, 256, 4, 520, 16, switched=switched, seed=6)


# width and depth through the chain: nq = nd = 6; mode 1 with B = 33, mode 3 with B = 9, N = 15
WIDTH_DEPTH = [(64, 2), (64, 6), (128, 3), (192, 4), (320, 5), (512, 4), (256, 3), (256, 5)]
CHAIN_SHAPES = [('st', 33, 4, False), ('constraint_everywhere', 9, 15, True)]


@functools.lru_cache(maxsize=None)
def chain_case(H, L, controller, B, N, switched, act='gelu', nd=6, n_ctx=0):
    return Case(controller, 6, nd, H, L, B, N, act=act, switched=switched, seed=21, n_ctx=n_ctx)


def all_eval_cases():
    """every case the GPU file runs through eval_nodes (the host file measures the yardstick of each)"""
    out = []
    for nq, nd in ND_PAIRS:
        for shape in SMALL_SHAPES:
            out.append(nd_case('fused', nq, nd, *shape))
            out.append(nd_case('chain', nq, nd, *shape))
    out += [wave_case(False), wave_case(True)]
    for H, L in WIDTH_DEPTH:
        out += [chain_case(H, L, *shape) for shape in CHAIN_SHAPES]
    out += [chain_case(128, 3, *CHAIN_SHAPES[0], act=a) for a in ACTS if a != 'gelu']
    return out


CTX = (0.4, -1.1, 0.9, 2.0, -0.3, 1.7)      # the context of the n_ctx = 6 case: all the room MLP_KPAD leaves behind 2 nd = 10


def context_case(controller, B, N, switched):
    return chain_case(128, 3, controller, B, N, switched, nd=5, n_ctx=6)
