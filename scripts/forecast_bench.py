#!/usr/bin/env python3
"""What a forecast costs and what it changes (smpc_forecast_scene, run_mpc(forecast=...); profiles/scene_forecast.txt).

1. k_scene_forecast alone (+ nothing else on the stream): B = 4096 (SMPC_B), N = 30, the problem's six rows, a world of T = 131
   columns read at clock 50, each mode: 3 warm-up and 10 timed calls between HIP events on the handle's stream.
2. The closed loop: 'htwa', B = 4096, N = 30, SMPC_STEPS (default 60) steps on turning tracks (problem.turning_scenes, sigma_v = 0.3,
   sigma_a = 3.0), the four arms none / true / hold / cv in alternation, SMPC_ROUNDS (default 2) rounds: ms per closed-loop step
   (run_mpc's own timing) and the lengths of conv_idx, collisions_idx, viable_idx, unconv_idx per arm.
3. k_scene_fit alone beside the CV kernel (profiles/scene_forecast_fit.txt): the shapes of 1, an observed track set, windows 2, 4, 8,
   16, 32 at clock 50 (every window full), the same 3 + 10 calls between HIP events.
4. The closed loop under observation noise: the tracks of 2 seen through observe_tracks (sigma SMPC_OBS_NOISE, default 0.005), the arms
   true (the clairvoyant reference, which observes nothing), cv and fit with windows 4, 8, 16 -- noise against lag by window length.
5. k_scene_poly alone beside k_scene_fit (profiles/scene_forecast_poly.txt): the shapes and the observed track of 3, windows 4, 8, 16,
   32, the line (smpc_forecast_scene_fit) and degrees 0 and 2 (smpc_forecast_scene_poly) window by window.
6. The closed loop on the turning tracks of 2, without observation noise (the controller sees the world) and with it (as 4): the arms
   true, cv, and the polynomial fit of degrees 1, 0 and 2 with windows 4, 8, 16, 32 -- lag against noise by window length and degree.
7. Room for being wrong (profiles/row_bounds.txt): the closed loop of 4 with forecast='cv' under observation noise and
   run_mpc(row_margin=(0, b)) for growth rates b of SMPC_MARGIN_GROWTH (default 0, 0.0005, 0.001, 0.002, 0.004 metres per node), one
   run each: collisions with the true world, abort events and the mean closed-loop cost of the instances that did not collide.
8. What the table costs a solve: smpc_solve_batch at B = 4096, N = 30 with a scene per instance set, without and with a row-bounds
   table (the descriptor's own bounds in every entry: the same QPs), in alternation, SMPC_ROUNDS (default 5) rounds of 10 calls
   between HIP events after 3 warm-up calls.
9. k_fit_margin alone beside the forecast kernel of the same fit (profiles/row_margin_fit.txt): the shapes and the observed track of
   3, windows 4, 8, 16, 32 and degrees 1, 0, 2; per (window, degree) the forecast and smpc_forecast_row_margin in alternation,
   SMPC_ROUNDS (default 3) rounds of 10 calls between HIP events after 3 warm-up calls.
10. A margin that follows the fit: the closed loop of 7 with forecast='fit' (window SMPC_FIT_WINDOW, default 8; degree SMPC_FIT_DEGREE,
   default 1) and run_mpc(row_margin_fit=(z, 0, SMPC_MARGIN_CAP)) for z of SMPC_MARGIN_Z (default 0, 1, 2, 3), next to the arms over b
   of 7 on the CV forecast and on the same fit, all in one session, one run each.
11. k_scene_kalman + k_kalman_margin beside k_scene_poly + k_fit_margin at window 32 (profiles/scene_forecast_kalman.txt): the shapes
   and the observed track of 3, degrees 1, 0, 2, the four calls in alternation, SMPC_ROUNDS (default 3) rounds of 10 calls between HIP
   events after 3 warm-up calls.  The filter advances with every call (a state of B x rows x 256 bytes is read and written).
12. The closed loop with the filter: the tracks of 4, with and without dropouts (problem.occlude_tracks, p SMPC_DROPOUT, default 0.05,
   mean length SMPC_DROPOUT_LEN, default 4): forecast='fit' (window SMPC_FIT_WINDOW, degree SMPC_FIT_DEGREE, with and without
   row_margin_fit z = 2; only without dropouts, a fit carries a NaN) against forecast='kalman' for q / r of SMPC_KALMAN_QR (default
   0.03, 0.1, 0.3) with r = the sensor's sigma, with and without row_margin_kalman z = 2, SMPC_ROUNDS rounds in alternation: ms per
   step, collisions of B and the mean closed-loop cost of the others.
A measurement tool, not a test; it reads nothing outside the repository.

    python scripts/forecast_bench.py [kernel|loop|fit-kernel|fit-loop|poly-kernel|poly-loop|margin-loop|margin-solve|interval-kernel|
                                      interval-loop|kalman-kernel|kalman-loop]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench                                                   # noqa: E402
from safe_mpc_amd import closed_loop as cl                     # noqa: E402
from safe_mpc_amd.problem import FORECAST_MODES, observe_tracks, turning_scenes   # noqa: E402
from safe_mpc_amd.solver import BatchedOcpSolver               # noqa: E402


def kernel_times(B):
    import torch
    par, prob, net = bench.build_problem()
    s = BatchedOcpSolver(prob, net)
    N, T, clock = prob.N, 131, 50
    device = torch.device('cuda', s.device)
    world = torch.tensor(turning_scenes(prob, B, T, 0.3, 3.0, seed=0), dtype=torch.float64, device=device)
    cell = torch.full((1,), clock, dtype=torch.int64, device=device)
    s.set_instance_world_track(world)
    s.set_scene_clock(cell)
    stream = torch.cuda.ExternalStream(s.L.smpc_stream(s.h), device=device)
    wrote = B * (N + 1) * len(prob.rows) * 64 / 1e6
    with torch.cuda.stream(stream):
        for mode in FORECAST_MODES:
            for _ in range(3):
                s.forecast_scene(mode)
            ms = []
            for _ in range(10):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                s.forecast_scene(mode)
                b.record(stream)
                b.synchronize()
                ms.append(a.elapsed_time(b))
            ms = np.array(ms)
            print(f'k_scene_forecast {mode:>4}: mean {1e3 * ms.mean():.1f} us, min {1e3 * ms.min():.1f}, max {1e3 * ms.max():.1f} (10 calls between '
                  f'HIP events); writes {wrote:.1f} MB: {wrote / ms.mean() / 1e3:.2f} TB/s of stores at the mean; B = {B}, N = {N}, '
                  f'{len(prob.rows)} rows, T = {T}, clock {clock}', flush=True)
    s.set_instance_world_track(None)
    s.set_scene_clock(None)
    s.close()


def fit_kernel_times(B, poly=False):
    import torch
    par, prob, net = bench.build_problem()
    s = BatchedOcpSolver(prob, net)
    N, T, clock = prob.N, 131, 50
    device = torch.device('cuda', s.device)
    world = turning_scenes(prob, B, T, 0.3, 3.0, seed=0)
    s.set_instance_world_track(torch.tensor(world, dtype=torch.float64, device=device))
    s.set_instance_observed_track(torch.tensor(observe_tracks(prob, world, 0.005), dtype=torch.float64, device=device))
    cell = torch.full((1,), clock, dtype=torch.int64, device=device)
    s.set_scene_clock(cell)
    stream = torch.cuda.ExternalStream(s.L.smpc_stream(s.h), device=device)
    rec = B * len(prob.rows) * 64 / 1e6                         # MB per column of the table
    with torch.cuda.stream(stream):
        calls = [('k_scene_forecast cv', lambda: s.forecast_scene('cv'), 2)] + \
            [(f'k_scene_fit window {m:2d}', (lambda m=m: s.forecast_scene_fit(m)), m) for m in (2, 4, 8, 16, 32)]
        if poly:        # the line and the two new degrees side by side, window by window
            calls = [c for m in (4, 8, 16, 32) for c in
                     [(f'k_scene_fit window {m:2d}', (lambda m=m: s.forecast_scene_fit(m)), m)] +
                     [(f'k_scene_poly window {m:2d} degree {p}', (lambda m=m, p=p: s.forecast_scene_poly(m, p)), m) for p in (0, 2)]]
        for name, call, cols in calls:
            for _ in range(3):
                call()
            ms = []
            for _ in range(10):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                call()
                b.record(stream)
                b.synchronize()
                ms.append(a.elapsed_time(b))
            ms = np.array(ms)
            print(f'{name}: mean {1e3 * ms.mean():.1f} us, min {1e3 * ms.min():.1f}, max {1e3 * ms.max():.1f} (10 calls between HIP events); '
                  f'reads {cols * rec:.1f} MB, writes {(N + 1) * rec:.1f} MB: {(cols + N + 1) * rec / ms.mean() / 1e3:.2f} TB/s at the mean; '
                  f'B = {B}, N = {N}, {len(prob.rows)} rows, T = {T}, clock {clock}', flush=True)
    s.set_instance_world_track(None)
    s.set_scene_clock(None)
    s.close()


def loop_times(B, noisy=False, poly=False):
    from safe_mpc_amd import controller as C
    par, prob, net = bench.build_problem()
    par.N = prob.N
    steps, rounds = int(os.environ.get('SMPC_STEPS', '60')), int(os.environ.get('SMPC_ROUNDS', '2'))
    probe = BatchedOcpSolver(prob, net)
    x0 = bench.initial_states(probe, prob, B, 0)
    probe.close()
    N = prob.N
    xg, ug = np.repeat(x0[:, None, :], N + 1, axis=1), np.zeros((B, N, prob.nu))
    world = turning_scenes(C.OcpProblem(par, 'htwa', 'ext', N=N), B, steps + 1 + N, 0.3, 3.0, seed=0)
    arms = [None, 'true', 'hold', 'cv']
    kwargs = {a: ({} if a is None else {'forecast': a}) for a in arms}
    if noisy:           # what the controller sees: the world through a sensor; 'true' observes nothing and is the reference
        sigma = float(os.environ.get('SMPC_OBS_NOISE', '0.005'))
        seen = observe_tracks(C.OcpProblem(par, 'htwa', 'ext', N=N), world, sigma, seed=0)
        arms = ['true', 'cv', 'fit4', 'fit8', 'fit16']
        kwargs = {'true': {'forecast': 'true'}, 'cv': {'forecast': 'cv', 'observed': seen}}
        kwargs.update({f'fit{m}': {'forecast': 'fit', 'forecast_window': m, 'observed': seen} for m in (4, 8, 16)})
        print(f'observation noise sigma = {sigma}')
    elif poly:          # the controller sees the world itself: what is left is the lag
        kwargs = {'true': {'forecast': 'true'}, 'cv': {'forecast': 'cv'}}
        print('no observation noise')
    if poly:            # every window with the line, the mean and the parabola
        what = {} if not noisy else {'observed': seen}
        arms = ['true', 'cv'] + [f'fit{m}d{p}' for m in (4, 8, 16, 32) for p in (1, 0, 2)]
        kwargs.update({f'fit{m}d{p}': {'forecast': 'fit', 'forecast_window': m, 'forecast_degree': p, **what}
                       for m in (4, 8, 16, 32) for p in (1, 0, 2)})
    res = {a: [] for a in arms}
    for r in range(rounds + 1):                                 # (round 0 warms everything up)
        for arm in arms:
            tm = {}
            out = cl.run_mpc(par, 'htwa', xg, ug, n_steps=steps, on_device=True, scenes=world, timing=tm, **kwargs[arm])
            counts = tuple(len(out[k]) for k in ('conv_idx', 'collisions_idx', 'viable_idx', 'unconv_idx'))
            if r:
                res[arm].append((tm['ms_per_step'],) + counts)
            print(f'round {r} forecast={arm}: {tm["ms_per_step"]:.3f} ms per step; conv / collisions / viable / unconv = {counts}', flush=True)
    for arm in arms:
        a = np.array(res[arm])
        print(f'forecast={str(arm):>8}: {a[:, 0].mean():.3f} ms per closed-loop step (rounds {a[:, 0].min():.3f} .. {a[:, 0].max():.3f}); '
              f'conv {int(a[0, 1])}, collisions {int(a[0, 2])}, viable {int(a[0, 3])}, unconv {int(a[0, 4])}; B = {B}, N = {N}, {steps} steps')


def interval_kernel_times(B):
    import torch
    par, prob, net = bench.build_problem()
    s = BatchedOcpSolver(prob, net)
    N, T, clock, nr = prob.N, 131, 50, len(prob.rows)
    device = torch.device('cuda', s.device)
    world = turning_scenes(prob, B, T, 0.3, 3.0, seed=0)
    s.set_instance_world_track(torch.tensor(world, dtype=torch.float64, device=device))
    s.set_instance_observed_track(torch.tensor(observe_tracks(prob, world, 0.005), dtype=torch.float64, device=device))
    cell = torch.full((1,), clock, dtype=torch.int64, device=device)
    s.set_scene_clock(cell)
    stream = torch.cuda.ExternalStream(s.L.smpc_stream(s.h), device=device)
    rounds = int(os.environ.get('SMPC_ROUNDS', '3'))
    rec = B * nr * 64 / 1e6                                     # MB per column of the table that was seen
    out_fc, out_mg = (N + 1) * rec, B * (N + 1) * nr * 16 / 1e6
    with torch.cuda.stream(stream):
        for m in (4, 8, 16, 32):
            for p in (1, 0, 2):
                calls = {'forecast': (lambda: s.forecast_scene_poly(m, p)), 'margin': (lambda: s.forecast_row_margin(m, p, 2.0))}
                res = {k: [] for k in calls}
                for r in range(rounds):
                    for name, call in calls.items():
                        for _ in range(3):
                            call()
                        for _ in range(10):
                            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            a.record(stream)
                            call()
                            b.record(stream)
                            b.synchronize()
                            res[name].append(a.elapsed_time(b))
                f, g = np.array(res['forecast']), np.array(res['margin'])
                print(f'window {m:2d} degree {p}: forecast kernel mean {1e3 * f.mean():.1f} us (min {1e3 * f.min():.1f}, max {1e3 * f.max():.1f}), '
                      f'reads {m * rec:.1f} MB, writes {out_fc:.1f} MB | k_fit_margin mean {1e3 * g.mean():.1f} us (min {1e3 * g.min():.1f}, max '
                      f'{1e3 * g.max():.1f}), reads 2 x {m * rec:.1f} MB, writes {out_mg:.1f} MB; {rounds} rounds of 10 calls each in alternation; '
                      f'B = {B}, N = {N}, {nr} rows, T = {T}, clock {clock}', flush=True)
    s.set_instance_row_bounds(None)
    s.set_instance_world_track(None)
    s.set_scene_clock(None)
    s.close()


def interval_loop(B):
    from safe_mpc_amd import controller as C
    par, prob, net = bench.build_problem()
    par.N = prob.N
    steps = int(os.environ.get('SMPC_STEPS', '60'))
    sigma = float(os.environ.get('SMPC_OBS_NOISE', '0.005'))
    window, degree = int(os.environ.get('SMPC_FIT_WINDOW', '8')), int(os.environ.get('SMPC_FIT_DEGREE', '1'))
    cap = float(os.environ.get('SMPC_MARGIN_CAP', '0.15'))
    rates = [float(v) for v in os.environ.get('SMPC_MARGIN_GROWTH', '0,0.0005,0.001,0.002,0.004').split(',')]
    zs = [float(v) for v in os.environ.get('SMPC_MARGIN_Z', '0,1,2,3').split(',')]
    probe = BatchedOcpSolver(prob, net)
    x0 = bench.initial_states(probe, prob, B, 0)
    probe.close()
    N = prob.N
    xg, ug = np.repeat(x0[:, None, :], N + 1, axis=1), np.zeros((B, N, prob.nu))
    ocp = C.OcpProblem(par, 'htwa', 'ext', N=N)
    world = turning_scenes(ocp, B, steps + 1 + N, 0.3, 3.0, seed=0)
    seen = observe_tracks(ocp, world, sigma, seed=0)
    fit = {'forecast': 'fit', 'forecast_window': window, 'forecast_degree': degree}
    print(f'observation noise sigma = {sigma}, turning tracks (sigma_v 0.3, sigma_a 3.0); B = {B}, N = {N}, {steps} steps; the fit: window '
          f'{window}, degree {degree}; cap of the fitted margin {cap} m')
    arms = [(f"forecast='cv', row_margin = (0, {b:g})", {'forecast': 'cv', **({} if b == 0.0 else {'row_margin': (0.0, b)})}) for b in rates]
    arms += [(f"forecast='fit', row_margin = (0, {b:g})", {**fit, 'row_margin': (0.0, b)}) for b in rates if b != 0.0]   # (b = 0 is z = 0 below)
    arms += [(f"forecast='fit', row_margin_fit = ({z:g}, 0, {cap:g})", {**fit, 'row_margin_fit': (z, 0.0, cap)}) for z in zs]
    for name, kw in arms:
        tm = {}
        out = cl.run_mpc(par, 'htwa', xg, ug, n_steps=steps, on_device=True, scenes=world, observed=seen, score=True, timing=tm, **kw)
        alive = np.ones(B, bool)
        alive[out['collisions_idx']] = False
        cost = out['score']['cost'][alive]
        print(f"{name}: collisions with the true world {len(out['collisions_idx'])}, abort events {len(out['x_viable'])}, converged "
              f"{len(out['conv_idx'])}, mean closed-loop cost of the {int(alive.sum())} others {np.nanmean(cost):.6g}; "
              f"{tm['ms_per_step']:.3f} ms per step", flush=True)


def kalman_kernel_times(B):
    import torch
    from safe_mpc_amd.problem import kalman_params
    par, prob, net = bench.build_problem()
    s = BatchedOcpSolver(prob, net)
    N, T, clock, nr = prob.N, 131, 50, len(prob.rows)
    device = torch.device('cuda', s.device)
    world = turning_scenes(prob, B, T, 0.3, 3.0, seed=0)
    s.set_instance_world_track(torch.tensor(world, dtype=torch.float64, device=device))
    s.set_instance_observed_track(torch.tensor(observe_tracks(prob, world, 0.005), dtype=torch.float64, device=device))
    cell = torch.full((1,), clock, dtype=torch.int64, device=device)
    s.set_scene_clock(cell)
    stream = torch.cuda.ExternalStream(s.L.smpc_stream(s.h), device=device)
    rounds = int(os.environ.get('SMPC_ROUNDS', '3'))
    rec = B * nr * 64 / 1e6                                     # MB per column of the table that was seen
    state = s.new_kalman_state(B)
    with torch.cuda.stream(stream):
        for p in (1, 0, 2):
            kp = kalman_params(p, 0.0005, 0.005)
            state.zero_()
            calls = {'k_scene_poly w32': (lambda: s.forecast_scene_poly(32, p)), 'k_fit_margin w32': (lambda: s.forecast_row_margin(32, p, 2.0)),
                     'k_scene_kalman': (lambda: s.forecast_scene_kalman(kp, state)), 'k_kalman_margin': (lambda: s.kalman_row_margin(kp, state, 2.0))}
            res = {k: [] for k in calls}
            for r in range(rounds):
                for name, call in calls.items():
                    for _ in range(3):
                        call()
                    for _ in range(10):
                        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        a.record(stream)
                        call()
                        b.record(stream)
                        b.synchronize()
                        res[name].append(a.elapsed_time(b))
            line = ' | '.join(f'{k} mean {1e3 * np.mean(v):.1f} us (min {1e3 * np.min(v):.1f}, max {1e3 * np.max(v):.1f})' for k, v in res.items())
            print(f'degree {p}: {line}; a column is {rec:.1f} MB, the state {4 * rec:.1f} MB, F {(N + 1) * rec:.1f} MB, a row-bounds table '
                  f'{B * (N + 1) * nr * 16 / 1e6:.1f} MB; {rounds} rounds of 10 calls each in alternation; B = {B}, N = {N}, {nr} rows, T = {T}, '
                  f'clock {clock}', flush=True)
    s.set_instance_row_bounds(None)
    s.set_instance_world_track(None)
    s.set_scene_clock(None)
    s.close()


def kalman_loop(B):
    from safe_mpc_amd import controller as C
    from safe_mpc_amd.problem import occlude_tracks
    par, prob, net = bench.build_problem()
    par.N = prob.N
    steps, rounds = int(os.environ.get('SMPC_STEPS', '60')), int(os.environ.get('SMPC_ROUNDS', '1'))
    sigma = float(os.environ.get('SMPC_OBS_NOISE', '0.005'))
    window, degree = int(os.environ.get('SMPC_FIT_WINDOW', '8')), int(os.environ.get('SMPC_FIT_DEGREE', '1'))
    cap = float(os.environ.get('SMPC_MARGIN_CAP', '0.15'))
    drop = (float(os.environ.get('SMPC_DROPOUT', '0.05')), float(os.environ.get('SMPC_DROPOUT_LEN', '4')))
    ratios = [float(v) for v in os.environ.get('SMPC_KALMAN_QR', '0.03,0.1,0.3').split(',')]
    probe = BatchedOcpSolver(prob, net)
    x0 = bench.initial_states(probe, prob, B, 0)
    probe.close()
    N = prob.N
    xg, ug = np.repeat(x0[:, None, :], N + 1, axis=1), np.zeros((B, N, prob.nu))
    ocp = C.OcpProblem(par, 'htwa', 'ext', N=N)
    world = turning_scenes(ocp, B, steps + 1 + N, 0.3, 3.0, seed=0)
    seen = observe_tracks(ocp, world, sigma, seed=0)
    lost = occlude_tracks(ocp, seen, drop[0], drop[1], seed=0)
    lost[:, 0] = seen[:, 0]                                     # (every obstacle is seen once before it can be lost)
    print(f'observation noise sigma = {sigma}, turning tracks (sigma_v 0.3, sigma_a 3.0); B = {B}, N = {N}, {steps} steps; the fit: window '
          f'{window}, degree {degree}; cap of the margins {cap} m; dropouts p = {drop[0]}, mean length {drop[1]}: '
          f'{100 * np.isnan(lost[:, :, 0, 0]).mean():.1f} % of row 0\'s samples lost')
    fit = {'forecast': 'fit', 'forecast_window': window, 'forecast_degree': degree, 'observed': seen}
    arms = [("forecast='fit'", fit), (f"forecast='fit', row_margin_fit = (2, 0, {cap:g})", {**fit, 'row_margin_fit': (2.0, 0.0, cap)})]
    for obs, tag in ((seen, ''), (lost, ' with dropouts')):
        for ratio in ratios:
            kal = {'forecast': 'kalman', 'forecast_degree': degree, 'kalman': (ratio * sigma, sigma, sigma, sigma, 0.1), 'observed': obs}
            arms += [(f"forecast='kalman' q/r = {ratio:g}{tag}", kal),
                     (f"forecast='kalman' q/r = {ratio:g}{tag}, row_margin_kalman = (2, {cap:g})", {**kal, 'row_margin_kalman': (2.0, cap)})]
    for r in range(rounds):
        for name, kw in arms:
            tm = {}
            out = cl.run_mpc(par, 'htwa', xg, ug, n_steps=steps, on_device=True, scenes=world, score=True, timing=tm, **kw)
            alive = np.ones(B, bool)
            alive[out['collisions_idx']] = False
            cost = out['score']['cost'][alive]
            print(f"round {r} {name}: collisions with the true world {len(out['collisions_idx'])}, abort events {len(out['x_viable'])}, converged "
                  f"{len(out['conv_idx'])}, mean closed-loop cost of the {int(alive.sum())} others {np.nanmean(cost):.6g}; "
                  f"{tm['ms_per_step']:.3f} ms per step", flush=True)


def margin_loop(B):
    from safe_mpc_amd import controller as C
    par, prob, net = bench.build_problem()
    par.N = prob.N
    steps = int(os.environ.get('SMPC_STEPS', '60'))
    sigma = float(os.environ.get('SMPC_OBS_NOISE', '0.005'))
    rates = [float(v) for v in os.environ.get('SMPC_MARGIN_GROWTH', '0,0.0005,0.001,0.002,0.004').split(',')]
    probe = BatchedOcpSolver(prob, net)
    x0 = bench.initial_states(probe, prob, B, 0)
    probe.close()
    N = prob.N
    xg, ug = np.repeat(x0[:, None, :], N + 1, axis=1), np.zeros((B, N, prob.nu))
    ocp = C.OcpProblem(par, 'htwa', 'ext', N=N)
    world = turning_scenes(ocp, B, steps + 1 + N, 0.3, 3.0, seed=0)
    seen = observe_tracks(ocp, world, sigma, seed=0)
    print(f"forecast='cv', observation noise sigma = {sigma}, turning tracks (sigma_v 0.3, sigma_a 3.0); B = {B}, N = {N}, {steps} steps")
    for b in rates:
        kw = {} if b == 0.0 else {'row_margin': (0.0, b)}      # (b = 0: the run without the argument)
        out = cl.run_mpc(par, 'htwa', xg, ug, n_steps=steps, on_device=True, scenes=world, forecast='cv', observed=seen, score=True, **kw)
        alive = np.ones(B, bool)
        alive[out['collisions_idx']] = False
        cost = out['score']['cost'][alive]
        print(f"row_margin = (0, {b:g}): collisions with the true world {len(out['collisions_idx'])}, abort events {len(out['x_viable'])}, "
              f"converged {len(out['conv_idx'])}, mean closed-loop cost of the {int(alive.sum())} others {np.nanmean(cost):.6g}", flush=True)


def margin_solve_times(B):
    import torch
    par, prob, net = bench.build_problem()
    s = BatchedOcpSolver(prob, net)
    N, nr = prob.N, len(prob.rows)
    device = torch.device('cuda', s.device)
    dev = lambda a: torch.tensor(a, dtype=torch.float64, device=device)
    x0 = bench.initial_states(s, prob, B, 0)
    p = np.zeros((B, N + 1, 5))
    p[:, :, :3], p[:, :, 3], p[:, :, 4] = prob.ee_ref, par.alpha, 1.0
    args = [dev(x0), dev(np.repeat(x0[:, None, :], N + 1, axis=1)), dev(np.zeros((B, N, prob.nu))), dev(p)]
    s.set_instance_scene(dev(turning_scenes(prob, B, 1, 0.3, 3.0, seed=0)[:, 0]))
    lo = dev(np.ascontiguousarray(np.broadcast_to(prob.row_lb, (B, N + 1, nr))))
    hi = dev(np.ascontiguousarray(np.broadcast_to(prob.row_ub, (B, N + 1, nr))))
    rounds = int(os.environ.get('SMPC_ROUNDS', '5'))
    stream = torch.cuda.ExternalStream(s.L.smpc_stream(s.h), device=device)
    res = {False: [], True: []}
    with torch.cuda.stream(stream):
        out = s.solve(*args)
        for r in range(rounds):
            for table in (False, True):
                s.set_instance_row_bounds(*((lo, hi) if table else (None, None)))
                for _ in range(3):
                    s.solve(*args, out=out)
                ms = []
                for _ in range(10):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record(stream)
                    s.solve(*args, out=out)
                    b.record(stream)
                    b.synchronize()
                    ms.append(a.elapsed_time(b))
                res[table].append(np.mean(ms))
                print(f'round {r} table={table}: {np.mean(ms):.4f} ms per solve (min {np.min(ms):.4f}, max {np.max(ms):.4f})', flush=True)
    for table in (False, True):
        a = np.array(res[table])
        print(f'smpc_solve_batch with a scene, row-bounds table {"set" if table else "not set"}: mean {a.mean():.4f} ms (rounds {a.min():.4f} .. '
              f'{a.max():.4f}); B = {B}, N = {N}, {nr} rows, {rounds} rounds of 10 calls in alternation')
    s.set_instance_row_bounds(None)
    s.set_instance_scene(None)
    s.close()


def main(argv=None):
    what = (sys.argv[1:] if argv is None else argv) or ['kernel', 'loop']
    B = int(os.environ.get('SMPC_B', '4096'))
    if 'kernel' in what:
        kernel_times(B)
    if 'loop' in what:
        loop_times(B)
    if 'fit-kernel' in what:
        fit_kernel_times(B)
    if 'fit-loop' in what:
        loop_times(B, noisy=True)
    if 'poly-kernel' in what:
        fit_kernel_times(B, poly=True)
    if 'poly-loop' in what:
        loop_times(B, poly=True)
        loop_times(B, noisy=True, poly=True)
    if 'margin-loop' in what:
        margin_loop(B)
    if 'margin-solve' in what:
        margin_solve_times(B)
    if 'interval-kernel' in what:
        interval_kernel_times(B)
    if 'interval-loop' in what:
        interval_loop(B)
    if 'kalman-kernel' in what:
        kalman_kernel_times(B)
    if 'kalman-loop' in what:
        kalman_loop(B)
    return 0


if __name__ == '__main__':
    sys.exit(main())
