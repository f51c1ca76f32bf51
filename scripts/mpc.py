#!/usr/bin/env python3
"""Closed-loop MPC run -- drop-in for the reference's scripts/mpc.py (same flags, config.yaml, guess / result pickles),
with every instance of its outer loop (mpc.py:102) solved at once on the MI355X engine.

    python scripts/mpc.py -c st --horizon 30 --alpha 10 [--noise 5 --control_noise 1] [--scene-jitter SIGMA --scene-seed S]
--scene-jitter SIGMA: every instance runs in a scene of its own -- the scenes stored with the guesses (guess_acados.py
--scene-jitter) if there are any, else every obstacle moved by its own N(0, SIGMA^2) draw per axis (problem.jittered_scenes,
seed --scene-seed, default 0).
--scene-velocity SIGMA: obstacles that move -- every instance gets a constant-velocity track of scenes, n_steps + 1 + horizon time
columns long: the tracks stored with the guesses (guess_acados.py --scene-velocity) continued at their velocity if there are any,
else every obstacle with its own N(0, SIGMA^2) velocity draw per axis (problem.moving_scenes; seed --scene-seed, start positions
jittered by --scene-jitter if that is given too).  A safe-set network with a context (``ctx_select`` in its checkpoint) follows the
track column by column.
--scene-accel SIGMA (needs --scene-velocity): obstacles that change course -- the tracks are drawn by problem.turning_scenes, whose
velocities random-walk with N(0, SIGMA^2) accelerations per obstacle and axis (stored tracks are not continued: they are drawn).
--scene-forecast hold|cv|true (needs --scene-velocity): the track is the WORLD, which only the plant meets; the controller plans
against a forecast of it formed every step from the columns the world has shown (run_mpc(forecast=...)) -- the
frozen world, a constant-velocity extrapolation, or the world itself.  The result file's name gets the suffix ``_fc<mode>``.
--scene-forecast fit [--forecast-window M] (M = 1..32, default 8): the forecast is a least-squares line through the last M columns seen
(run_mpc(forecast='fit', forecast_window=M)); suffix ``_fcfit_w<M>``.
--forecast-degree P (P = 0, 1 or 2, default 1; needs --scene-forecast fit): the fit is a least-squares polynomial of degree P through
those columns (run_mpc(forecast_degree=P)) -- 0 the window mean, 2 a constant-acceleration model; suffix ``_d<P>``
behind ``_w<M>`` for P other than 1.
--scene-obs-noise SIGMA [--scene-obs-seed S] (needs --scene-forecast hold, cv or fit): the controller sees the world through a sensor --
every obstacle's position in every column off by its own N(0, SIGMA^2) draw per axis (problem.observe_tracks, seed S, default 0), and
the forecast is formed from that (run_mpc(observed=...)); the plant meets the true world.  Suffix ``_on<SIGMA>`` for SIGMA > 0.
--row-margin A [--row-margin-growth B] (metres, metres per node; B needs A, default 0): obstacle inflation along the horizon -- node k of
every solve leaves A + B k metres of extra room around the world-fixed obstacles (run_mpc(row_margin=(A, B)));
the outcome tests keep the physical check bounds.  Suffix ``_rm<A>`` and, for B other than 0, ``_g<B>`` behind it.
--row-margin-z Z [--row-margin-prior S] [--row-margin-cap D] (needs --scene-forecast fit; S in metres, default 0; D in metres, default
problem.FIT_MARGIN_CAP): the margin is formed every step from the residuals of the fit -- node k leaves A + B k + Z s g_k metres, at
most D, per instance and row: s the residual standard deviation of the window, at least S, g_k the growth of the forecast's error
(run_mpc(row_margin_fit=(Z, S, D))); --row-margin then gives its base.  Suffix ``_rmf<Z>_p<S>_c<D>``.
--scene-forecast kalman [--forecast-degree P] --kalman-q Q --kalman-r R [--kalman-prior V0 A0] [--kalman-beta B]: the forecast is a
Kalman filter per (instance, row) -- P = 0, 1 (the default here) or 2 its model, Q the process noise, R the sensor noise in metres, V0 and
A0 the prior standard deviations of velocity and acceleration per column (default R each), B in [0, 1] the rate of the innovation scale
(default 0) -- run_mpc(forecast='kalman', kalman=(Q, R, V0, A0, B)), DESIGN.md section 9s.  Suffix ``_fckalman_d<P>_q<Q>_r<R>_v<V0>_a<A0>_b<B>``.
--scene-obs-dropout P [--scene-obs-dropout-len L] (needs --scene-forecast kalman): the sensor loses sight of an obstacle -- per (instance,
obstacle) a visible one starts a burst of missing samples with probability P per column, of mean length L columns (default 4;
problem.occlude_tracks, seed --scene-obs-seed); the filter skips its update there.  Suffix ``_od<P>_l<L>`` behind ``_on``.
--row-margin-z Z [--row-margin-cap D] with --scene-forecast kalman: the margin is formed every step from the filter's predicted covariance
(run_mpc(row_margin_kalman=(Z, D))); --row-margin gives its base; --row-margin-prior does not apply.  Suffix ``_rmk<Z>_c<D>``.
--track 8|circle (or ``track_traj: true`` in config.yaml, which means the "8"): the trajectory-tracking task -- the controller follows
tracking.tracking_trajectory's curve for n_steps_tracking steps, from the warm starts guess_acados.py --track wrote.
--track-jitter SIGMA [--track-scale-jitter S] [--track-seed S] (only with a tracking run): every instance follows a curve of its own --
the curves stored with the guesses (guess_acados.py --track-jitter) if there are any, else tracking.jittered_curves.
--controller-model nominal|plant (default nominal): with ``plant`` (needs --noise > 0) every instance's controller forms its dynamics
with the perturbed link inertials its plant is simulated with -- the matched-model arm of the model-noise study -- and the result
file's name gets the suffix ``_cmplant`` before ``_mpc.pkl``.
Exit code = number of failed instances, as in the reference (mpc.py:317).
"""
import os
import pickle
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from safe_mpc_amd import closed_loop as cl                      # noqa: E402
from safe_mpc_amd.parser import Parameters, parse_args          # noqa: E402


def main(argv=None):
    args = parse_args(argv)
    model_name = args['system']
    params = Parameters(args, model_name, rti=True)
    params.act, params.alpha, params.N = args['activation'], args['alpha'], args['horizon']
    params.back_hor = args['back_hor']
    cont_name = args['controller']
    use_net = None if cont_name in ('naive', 'zerovel') else True          # controller.py:236 / STController
    raw = list(sys.argv[1:] if argv is None else argv)
    traj = cl.tracking_from_cli(params, raw)                # (sets params.n_steps / track_traj: the file names carry the token)
    gfile = cl.guess_file(params, model_name, cont_name, params.N, use_net)
    print(gfile)
    data = pickle.load(open(gfile, 'rb'))
    x_guess, u_guess = data['xg'][:params.test_num], data['ug'][:params.test_num]
    if '--track-jitter' in raw:
        # the warm starts were generated along their own curves; without stored ones, a curve per loaded guess
        traj = data['curves'][:params.test_num] if 'curves' in data else cl.tracking_from_cli(params, raw, n=x_guess.shape[0])
    scenes = None
    if '--scene-jitter' in raw:
        if 'scenes' in data:          # the warm starts were generated in these scenes
            scenes = data['scenes'][:params.test_num]
        else:
            from safe_mpc_amd.problem import OcpProblem, jittered_scenes
            seed = int(raw[raw.index('--scene-seed') + 1]) if '--scene-seed' in raw else 0
            scenes = jittered_scenes(OcpProblem(params, 'naive'), x_guess.shape[0], float(raw[raw.index('--scene-jitter') + 1]), seed)
    opt = lambda flag, default, cast: cast(raw[raw.index(flag) + 1]) if flag in raw else default
    forecast = opt('--scene-forecast', None, str)
    if forecast is not None and forecast not in ('hold', 'cv', 'true', 'fit', 'kalman'):
        raise SystemExit(f'--scene-forecast {forecast}: expected hold, cv or true, or fit, or kalman')
    window, obs_noise = opt('--forecast-window', 8, int), opt('--scene-obs-noise', 0.0, float)
    if '--forecast-window' in raw and forecast != 'fit':
        raise SystemExit('--forecast-window needs --scene-forecast fit: no other forecast has a window')
    if forecast == 'fit' and not 1 <= window <= 32:
        raise SystemExit(f'--forecast-window {window}: expected 1..32')
    degree = opt('--forecast-degree', 1, int)
    if '--forecast-degree' in raw and forecast not in ('fit', 'kalman'):
        raise SystemExit('--forecast-degree needs --scene-forecast fit or kalman: no other forecast has a degree')
    if not 0 <= degree <= 2:
        raise SystemExit(f'--forecast-degree {degree}: expected 0, 1 or 2')
    for flag in ('--scene-obs-noise', '--scene-obs-seed'):
        if flag in raw and forecast not in ('hold', 'cv', 'fit', 'kalman'):
            raise SystemExit(f'{flag} needs --scene-forecast hold, cv or fit, or kalman: nothing else reads what was observed')
    if obs_noise < 0:
        raise SystemExit(f'--scene-obs-noise {obs_noise}: a standard deviation is not negative')
    for flag in ('--kalman-q', '--kalman-r', '--kalman-prior', '--kalman-beta', '--scene-obs-dropout', '--scene-obs-dropout-len'):
        if flag in raw and forecast != 'kalman':
            raise SystemExit(f'{flag} needs --scene-forecast kalman: no other forecast has a filter or skips a missing sample')
    kalman = dropout = None
    if forecast == 'kalman':
        for flag in ('--kalman-q', '--kalman-r'):
            if flag not in raw:
                raise SystemExit(f'--scene-forecast kalman needs {flag}: the filter has no default noise')
        try:
            q, r = opt('--kalman-q', 0.0, float), opt('--kalman-r', 0.0, float)
            v0, a0 = ((float(raw[raw.index('--kalman-prior') + 1]), float(raw[raw.index('--kalman-prior') + 2]))
                      if '--kalman-prior' in raw else (r, r))
        except (ValueError, IndexError):
            raise SystemExit('--kalman-q Q, --kalman-r R, --kalman-prior V0 A0: expected numbers')
        kalman = (q, r, v0, a0, opt('--kalman-beta', 0.0, float))
        from safe_mpc_amd.problem import kalman_params
        try:
            kalman_params(degree, *kalman, who='--kalman')
        except ValueError as e:
            raise SystemExit(str(e))
        if '--scene-obs-dropout-len' in raw and '--scene-obs-dropout' not in raw:
            raise SystemExit('--scene-obs-dropout-len needs --scene-obs-dropout: there is no burst to size')
        if '--scene-obs-dropout' in raw:
            dropout = (opt('--scene-obs-dropout', 0.0, float), opt('--scene-obs-dropout-len', 4.0, float))
            if not (0.0 <= dropout[0] <= 1.0 and 1.0 <= dropout[1] < float('inf')):
                raise SystemExit(f'--scene-obs-dropout {dropout[0]} --scene-obs-dropout-len {dropout[1]}: expected a probability and a mean '
                                 f'length of at least one column')
    for flag in ('--scene-forecast', '--scene-accel'):
        if flag in raw and '--scene-velocity' not in raw:
            raise SystemExit(f'{flag} needs --scene-velocity: there is no track to forecast or to turn')
    if '--scene-velocity' in raw:
        from safe_mpc_amd.problem import OcpProblem, extend_tracks, moving_scenes, turning_scenes
        T = int(params.n_steps) + 1 + int(params.N)
        if '--scene-accel' in raw:
            scenes = turning_scenes(OcpProblem(params, 'naive'), x_guess.shape[0], T, opt('--scene-velocity', 0.0, float),
                                    opt('--scene-accel', 0.0, float), opt('--scene-seed', 0, int), sigma=opt('--scene-jitter', 0.0, float))
        elif 'scenes' in data and data['scenes'].ndim == 4:
            scenes = extend_tracks(data['scenes'][:params.test_num], T)
        else:
            scenes = moving_scenes(OcpProblem(params, 'naive'), x_guess.shape[0], T, opt('--scene-velocity', 0.0, float),
                                   opt('--scene-seed', 0, int), sigma=opt('--scene-jitter', 0.0, float))
    fc_kw, name_kw = ({} if forecast is None else {'forecast': forecast}), ({} if forecast is None else {'forecast': forecast})
    if forecast == 'fit':
        fc_kw['forecast_window'] = name_kw['forecast_window'] = window
    if degree != 1 or forecast == 'kalman':     # (degree 1 is the fit of before: its call and its file name)
        fc_kw['forecast_degree'] = name_kw['forecast_degree'] = degree
    if kalman is not None:
        fc_kw['kalman'] = name_kw['kalman'] = kalman
    if '--scene-obs-noise' in raw:
        from safe_mpc_amd.problem import OcpProblem, observe_tracks
        fc_kw['observed'] = observe_tracks(OcpProblem(params, 'naive'), scenes, obs_noise, opt('--scene-obs-seed', 0, int))
        name_kw['obs_noise'] = obs_noise
    if dropout is not None:
        from safe_mpc_amd.problem import OcpProblem, occlude_tracks
        fc_kw['observed'] = occlude_tracks(OcpProblem(params, 'naive'), fc_kw.get('observed', scenes), dropout[0], dropout[1],
                                           opt('--scene-obs-seed', 0, int))
        name_kw['obs_dropout'] = dropout
    if '--row-margin-growth' in raw and '--row-margin' not in raw:
        raise SystemExit('--row-margin-growth needs --row-margin: there is no margin to grow')
    if '--row-margin' in raw:
        fc_kw['row_margin'] = name_kw['row_margin'] = (opt('--row-margin', 0.0, float), opt('--row-margin-growth', 0.0, float))
        if cont_name == 'parallel':
            raise SystemExit("--row-margin: the 'parallel' policy is not supported")
    for flag in ('--row-margin-prior', '--row-margin-cap'):
        if flag in raw and '--row-margin-z' not in raw:
            raise SystemExit(f'{flag} needs --row-margin-z: there is no fitted margin to bound')
    if '--row-margin-z' in raw:
        from safe_mpc_amd.problem import FIT_MARGIN_CAP
        if forecast not in ('fit', 'kalman'):
            raise SystemExit('--row-margin-z needs --scene-forecast fit or kalman: no other forecast leaves residuals or a covariance')
        if cont_name == 'parallel':
            raise SystemExit("--row-margin-z: the 'parallel' policy is not supported")
        if forecast == 'kalman' and '--row-margin-prior' in raw:
            raise SystemExit("--row-margin-prior goes with --scene-forecast fit: the filter's floor is its own sensor noise, --kalman-r")
        fit = (opt('--row-margin-z', 0.0, float), opt('--row-margin-prior', 0.0, float), opt('--row-margin-cap', FIT_MARGIN_CAP, float))
        if not all(0.0 <= v < float('inf') for v in fit):
            raise SystemExit(f'--row-margin-z, --row-margin-prior, --row-margin-cap: {fit}: expected finite numbers that are not negative')
        if forecast == 'kalman':
            fc_kw['row_margin_kalman'] = name_kw['row_margin_kalman'] = (fit[0], fit[2])
        else:
            fc_kw['row_margin_fit'] = name_kw['row_margin_fit'] = fit
    cmodel = raw[raw.index('--controller-model') + 1] if '--controller-model' in raw else 'nominal'
    if cmodel not in ('nominal', 'plant'):
        raise SystemExit(f'--controller-model {cmodel}: expected nominal or plant')
    tm = {}
    # all loop state in HBM (policy automaton, abort handling, logs); SMPC_HOST_STATE=1 keeps it in numpy arrays instead
    res = cl.run_mpc(params, cont_name, x_guess, u_guess, noise=args['noise'], control_noise=args['control_noise'],
                     callback=True, on_device=os.environ.get('SMPC_HOST_STATE', '0') != '1', timing=tm,
                     collect_times=os.environ.get('SMPC_NO_TIME_STATS', '0') != '1', scenes=scenes, traj=traj,
                     models='plant' if cmodel == 'plant' else None, **fc_kw)
    with_stats = os.environ.get('SMPC_NO_TIME_STATS', '0') != '1'
    print(f"{tm['ms_per_step']:.3f} ms per closed-loop step of {x_guess.shape[0]} instances"
          + (' (eager launches with per-solve HIP events for the time statistics below; SMPC_NO_TIME_STATS=1 replays the step halves as '
             'hipGraphs without them)' if with_stats else ' (step halves replayed as hipGraphs, no per-solve time statistics)'))
    if 'time_stats' in res:      # the block of the reference's mpc.py:300-303 (here one solve = all instances of a group)
        print('99% quantile of the computation time:')
        for field, t in zip(res['time_fields'], res['time_q99']):
            print(f"{field:<20} -> {t}")
    n = x_guess.shape[0]
    print(f"Completed task: {len(res['conv_idx'])}\nCollisions: {len(res['collisions_idx'])}"
          f"\nViable states: {len(res['viable_idx'])}\nNot converged: {n - len(res['conv_idx']) - len(res['collisions_idx'])}")
    cl.save_pickle(cl.result_file(params, model_name, cont_name, params.N, use_net, args['noise'], args['control_noise'],
                                  args['joint_bounds_margin'], args['collision_margin'], controller_model=cmodel,
                                  **name_kw), res)
    return len(res['collisions_idx'])


if __name__ == '__main__':
    sys.exit(main())
