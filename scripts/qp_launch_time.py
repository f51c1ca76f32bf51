"""Launch time of the throughput-form QP solve in the SHIPPED build (or the one SMPC_HIP_LIB names), on the state that
scripts/qp_phase_profile.py profiles: SMPC_B instances (256: lone wavefronts), C1 after 5 closed-loop steps, SMPC_REPS timed solves of
the same inputs (device events around set-up + k_qp_ipm).  The counterpart of the phase profile for builds whose -DQP_PROFILE variant
spills where the shipped one does not (point 6): one number, but of the code that runs.

Usage on the GPU box:  SMPC_B=256 python scripts/qp_launch_time.py     (A/B: once per build, in alternation)
"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import bench
from safe_mpc_amd.solver import BatchedOcpSolver
par, prob, net = bench.build_problem()
s = BatchedOcpSolver(prob, net)
s.set_qp_mode('throughput')
B = int(os.environ.get('SMPC_B', '256')); R = int(os.environ.get('SMPC_REPS', '40'))
x0 = bench.initial_states(s, prob, B, 0)
N = prob.N
xg = np.repeat(x0[:, None, :], N + 1, axis=1); ug = np.zeros((B, N, 6)); p = np.zeros((B, N + 1, 5))
p[:, :, :3], p[:, :, 3], p[:, :, 4] = prob.ee_ref, par.alpha, 1.0
x = x0
for i in range(5):
    xo, uo, st, it = s.solve(x, xg, ug, p)
    xg, ug, ua = s.provide_control((st == 0).astype(np.int32), xo, uo, xg, ug)
    x, _ = s.plant_step(x, ua)
    xg = s.guess_correction(xg, ug)
dev = torch.device('cuda:0')
t = lambda a: torch.tensor(a, dtype=torch.float64, device=dev)
xd, xgd, ugd, pd = t(x), t(xg), t(ug), t(p)
s.enable_timing(True)
ts = []
for r in range(R + 3):
    out = s.solve(xd, xgd, ugd, pd)
    ts.append(s.timing()['time_qp'] * 1e3)
ts = np.array(ts[3:])
it = out[3].cpu().numpy()
print('%s B %d  QP (setup + ipm) ms: min %.4f  median %.4f  max %.4f  (%d solves, mean iterations %.2f, max %d)' % (
    os.environ.get('SMPC_HIP_LIB', 'shipped build'), B, ts.min(), np.median(ts), ts.max(), R, it.mean(), it.max()))
