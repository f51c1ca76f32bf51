"""A scene of its own for every instance, without a GPU: the geometry helpers of problem.py, the C ABI's new entry point, and
run_mpc(scenes=...) on the host path through the CPU oracle (scene_cases.SceneOracleSolver: one oracle per scene)."""
import ctypes
import os

import numpy as np
import pytest

import scene_cases as sc
from conftest import make_problem, sample_instances
from fake_solver import OracleSolver
from oracle.oracle import Oracle
from safe_mpc_amd import closed_loop as cl
from safe_mpc_amd import controller as C
from safe_mpc_amd.problem import SCENE_ROW, OcpProblem, jittered_scenes, scenes_from_problems


# ---- 1. geometry ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('system,controller,names', [('z1', 'st', sc.Z1_OBSTACLES), ('fr7', 'constraint_everywhere', sc.FR7_OBSTACLES)])
def test_scene_equals_the_geometry_of_moved_parameters(system, controller, names):
    """scene(moves) == row_geometry() of the problem built from moved parameters, to the bit, for every test shift; the records
    hold C, D, offset, 0; rows of other obstacles and everything a scene does not carry stay as they are"""
    (par, base, net), moved, geom = sc.scene_family(system, controller, 12, 4 if system == 'z1' else 3)
    g0 = base.row_geometry()
    assert g0.shape == (len(base.rows), SCENE_ROW) and np.all(g0[:, 7] == 0.0)
    for r, row in zip(g0, base.rows):
        assert np.array_equal(r[:7], list(row.C) + list(row.D) + [row.offset])
    assert len(base.row_obstacle) == len(base.rows)
    for shift, (_, pm, _), gm in zip(sc.SHIFTS, moved, geom):
        got = base.scene({n: shift for n in names})
        assert np.array_equal(got, pm.row_geometry()) and np.array_equal(got, gm)        # (fr7: the plane's offset column included)
        if any(shift):
            assert not np.array_equal(got, g0)
    assert np.array_equal(base.scene({}), g0)
    if system == 'fr7':
        assert base.row_obstacle == ['ball', 'ball', 'ball', 'floor'] and [r.kind for r in base.rows] == [2, 2, 3, 4]
        # a plane takes the component of the move along its perpendicular axis, and nothing else moves with it
        up = base.scene({'floor': (0.3, -0.2, 0.125)})
        ax = base.rows[3].axis
        assert up[3, 6] == g0[3, 6] + (0.3, -0.2, 0.125)[ax] and np.array_equal(up[:3], g0[:3]) and np.array_equal(up[3, :6], g0[3, :6])
        # sphere rows read C only: D stays zero
        assert np.all(base.scene({'ball': (0.1, 0.2, 0.3)})[:3, 3:6] == 0.0)
    else:
        assert base.row_obstacle == ['fixed1', 'fixed2', 'fixed3'] * 2
        one = base.scene({'fixed2': (0.0, 0.0, 0.1)})
        assert np.array_equal(one[[0, 2, 3, 5]], g0[[0, 2, 3, 5]]) and np.array_equal(one[[1, 4], 2], g0[[1, 4], 2] + 0.1)
    with pytest.raises(ValueError, match='unknown obstacle'):
        base.scene({'no_such_obstacle': (0, 0, 0)})


def test_scenes_from_problems_rejects_what_a_scene_does_not_carry():
    (par, base, net), moved, geom = sc.scene_family('z1', 'st', 12, 4)
    assert geom.shape == (4, 6, SCENE_ROW)
    # other bounds: a thicker obstacle
    par2, _, _ = make_problem('st', N=12)
    par2.obst_capsules[0]['radius'] += 0.01
    with pytest.raises(ValueError, match='lb, ub'):
        scenes_from_problems(base, [OcpProblem(par2, 'st', 'ext', N=12)])
    # other check bounds only
    par3, _, _ = make_problem('st', N=12, tol_obs=1e-3)
    with pytest.raises(ValueError, match='check bounds'):
        scenes_from_problems(base, [OcpProblem(par3, 'st', 'ext', N=12)])
    # other kinds: the fr7 problem is no scene of z1's
    with pytest.raises(ValueError):
        scenes_from_problems(base, [sc.scene_family('fr7', 'constraint_everywhere', 12, 3)[0][1]])
    js = jittered_scenes(base, 5, 0.02, seed=3)
    assert js.shape == (5, 6, SCENE_ROW) and np.array_equal(js, jittered_scenes(base, 5, 0.02, seed=3))
    assert np.array_equal(js[:, 0], js[:, 3]) and not np.array_equal(js[0], js[1])     # one draw per obstacle, another per scene
    assert np.array_equal(jittered_scenes(base, 2, 0.0)[1], base.row_geometry())


# ---- 2. the ABI -----------------------------------------------------------------------------------------------------------------
def test_library_exports_the_entry_point_and_lib_declares_it():
    from safe_mpc_amd import _lib
    assert 'smpc_set_instance_scene' in _lib.SYMBOLS
    assert os.path.exists(_lib.LIB_PATH), 'the engine is built before the tests run (__graft_entry__.build)'
    L = ctypes.CDLL(_lib.LIB_PATH)               # loads without a GPU
    assert hasattr(L, 'smpc_set_instance_scene')
    assert L.smpc_abi_version() == 5
    hdr = open(os.path.join(os.path.dirname(_lib.LIB_PATH), '..', '..', 'include', 'smpc.h')).read()
    assert '#define SMPC_SCENE_ROW 8' in hdr and SCENE_ROW == 8


# ---- 3. the closed loop in two scenes at once ---------------------------------------------------------------------------------------
def _factories(par, N, scene_pars=None, geoms=None, solver_cls=None, log=None):
    """make_controller / make_backup of run_mpc around the CPU oracle; with scene_pars, around SceneOracleSolver"""
    def build(cls, name, cost, horizon, batch):
        ctrl = cls.__new__(cls)
        prob = C.OcpProblem(par, name, cost, N=horizon)
        net = C.SafeSetNet.from_params(par, prob.x_min, prob.x_max)
        prob.set_normalisation(net.mean, net.std)
        if scene_pars is None:
            solver = (solver_cls or OracleSolver)(prob, net)
        else:
            subs = []
            for sp in scene_pars:
                pr = C.OcpProblem(sp, name, cost, N=horizon)
                pr.set_normalisation(net.mean, net.std)
                subs.append(pr)
            solver = (solver_cls or sc.SceneOracleSolver)(prob, net, subs, geoms)
        if log is not None:
            log[name] = solver
        C.AbstractController.__init__(ctrl, par, batch, cost, horizon, solver=solver, net=net)
        return ctrl
    return (lambda name, batch: build(C.CONTROLLERS[name], C.CONTROLLERS[name].cont_name, 'ext', N, batch),
            lambda batch: build(C.SafeBackupController, 'backup', 'zero', par.back_hor, batch))


def _pars(N, n_scenes):
    pars = []
    for shift in sc.SHIFTS[:n_scenes]:
        par, _, _ = make_problem('htwa', N=N)
        par.back_hor = 12
        sc.move_obstacles(par, shift, sc.Z1_OBSTACLES)
        pars.append(par)
    return pars


def test_run_mpc_in_two_scenes_equals_the_per_scene_runs():
    """2 scenes x 3 instances, 'htwa', 15 steps on the host path: bit for bit the two runs on problems built from moved parameters
    (same oracle, same sub-batches, so not even the threading can differ); results carry the scenes"""
    N, steps = 10, 15
    pars = _pars(N, 2)
    base = C.OcpProblem(pars[0], 'htwa', 'ext', N=N)
    geoms = scenes_from_problems(base, [C.OcpProblem(p, 'htwa', 'ext', N=N) for p in pars])
    x0 = sample_instances(base, 6, seed=5, vel_scale=0.1)
    for p in pars[1:]:      # starts that are free in every scene
        pr = C.OcpProblem(p, 'htwa', 'ext', N=N)
        assert Oracle(pr).check_trajectory(x0[:, None, :], pr.x_min, pr.x_max, 0.0, pr.row_lb, pr.row_ub).all()
    xg, ug = np.repeat(x0[:, None, :], N + 1, axis=1), np.zeros((6, N, 6))
    scenes = np.repeat(geoms, 3, axis=0)                        # [A, A, A, B, B, B]
    mk, mkb = _factories(pars[0], N, pars, geoms)
    res = cl.run_mpc(pars[0], 'htwa', xg, ug, make_controller=mk, make_backup=mkb, n_steps=steps, scenes=scenes, score=True)
    assert np.array_equal(res['scenes'], scenes)
    parts = []
    for s, par in enumerate(pars):
        mk1, mkb1 = _factories(par, N)
        parts.append(cl.run_mpc(par, 'htwa', xg[3 * s:3 * s + 3], ug[3 * s:3 * s + 3], make_controller=mk1, make_backup=mkb1,
                                n_steps=steps, score=True))
    for key in ('x', 'u'):
        assert np.array_equal(res[key], np.concatenate([p[key] for p in parts]), equal_nan=True), key
    for key in ('conv_idx', 'collisions_idx', 'viable_idx', 'unconv_idx'):
        assert res[key] == sorted(i + 3 * s for s, p in enumerate(parts) for i in p[key]), key
    for key, val in res['score'].items():
        ref = np.concatenate([p['score'][key] for p in parts])
        if val.dtype.kind == 'f':
            # (the per-instance statement packs the states into other trajectories than the chunked one: the same numbers from
            #  other calls of the oracle)
            assert np.allclose(val, ref, rtol=1e-12, atol=1e-12, equal_nan=True), key
        else:
            assert np.array_equal(val, ref), key
    assert not np.array_equal(parts[0]['x'], parts[1]['x'])
    # and the scenes matter: the second half of the batch in scene A is another run
    mkA, mkbA = _factories(pars[0], N)
    inA = cl.run_mpc(pars[0], 'htwa', xg[3:], ug[3:], make_controller=mkA, make_backup=mkbA, n_steps=steps)
    assert not np.array_equal(inA['u'], res['u'][3:], equal_nan=True)
    with pytest.raises(ValueError, match='scenes'):
        cl.run_mpc(pars[0], 'htwa', xg, ug, make_controller=mk, make_backup=mkb, n_steps=2, scenes=scenes[:5])
    with pytest.raises(ValueError, match='not supported'):
        cl.generate_guess_until(pars[0], 'htwa', 2, scenes=scenes[:2])


# ---- 4. an abort event hands the backup solver the aborting instances' scenes -------------------------------------------------------
def test_backup_solver_gets_exactly_the_scenes_of_the_aborting_instances():
    N = 4
    pars = _pars(N, 2)
    base = C.OcpProblem(pars[0], 'htwa', 'ext', N=N)
    geoms = scenes_from_problems(base, [C.OcpProblem(p, 'htwa', 'ext', N=N) for p in pars])
    B = 5
    scenes = geoms[[0, 1, 0, 1, 1]]
    scenes = scenes + 1e-3 * np.arange(B)[:, None, None] * (np.arange(SCENE_ROW) < 6)     # every instance a scene of its own
    calls = []

    class Recording(OracleSolver):
        """takes a scene and writes down what it was given and when (the numerics stay the base problem's: the test is about the
        hand-over)"""
        def __init__(self, prob, net, subs=None, geoms=None):
            super().__init__(prob, net)

        def set_instance_scene(self, geom=None):
            calls.append((self.problem.controller, 'scene', None if geom is None else np.array(geom, float)))

        def solve(self, x0, xg, ug, p, out=None):
            calls.append((self.problem.controller, 'solve', len(x0)))
            return super().solve(x0, xg, ug, p, out)

    solvers = {}
    mk, mkb = _factories(pars[0], N, pars, geoms, solver_cls=Recording, log=solvers)
    x0 = sample_instances(base, B, seed=5, vel_scale=0.1)
    xg, ug = np.repeat(x0[:, None, :], N + 1, axis=1), np.zeros((B, N, 6))

    # N = 4 consecutive failed solves make instances 1 and 3 abort at step 3 (controller.py:375-388)
    fail = np.array([0, 4, 0, 4, 0], np.int32)

    def mk_scripted(name, batch):
        ctrl = mk(name, batch)
        ctrl.ocp_solver.scripted_status = [fail.copy() for _ in range(N)] + [np.zeros(B, np.int32)] * 4
        return ctrl
    res = cl.run_mpc(pars[0], 'htwa', xg, ug, make_controller=mk_scripted, make_backup=mkb, n_steps=6, scenes=scenes)
    main = [c for c in calls if c[0] == 'htwa']
    assert main[0][1] == 'scene' and np.array_equal(main[0][2], scenes)            # the group's scene, before its first solve
    # ... and no other until the run is over, when the handle is left without one (a reused solver starts clean)
    assert [k for k, c in enumerate(main) if c[1] == 'scene'] == [0, len(main) - 1] and main[-1][2] is None
    back = [c for c in calls if c[0] == 'backup']
    assert [c[1] for c in back] == ['scene', 'solve', 'scene'], back
    assert np.array_equal(back[0][2], scenes[[1, 3]]) and back[1][2] == 2          # rows 1 and 3, in the order of the compact batch
    assert back[2][2] is None
    assert res['x_viable'].shape[0] == 2
    # the parallel policy is refused by name, before anything is built
    with pytest.raises(ValueError, match="'parallel' policy is not supported"):
        cl.run_mpc(pars[0], 'parallel', xg, ug, make_controller=mk, make_backup=mkb, n_steps=2, scenes=scenes)


# ---- 5. the start states of generate_guess(scenes=...) -------------------------------------------------------------------------------
def test_start_states_are_walked_against_each_instances_own_scene():
    """closed_loop._free_starts_per_scene against the plain statement of the walk (candidate by candidate, each tested in the scene of
    the instance it would start), on a scripted table of which candidate is free in which scene; with one scene for everybody it is
    the shared rule x_all[free][:n]; where the candidates run out the tail is reported unfilled"""
    rng = np.random.default_rng(11)
    n_sc, n_cand = 3, 40
    table = rng.uniform(size=(n_sc, n_cand)) > 0.35             # free[scene, candidate]
    cand = np.zeros((n_cand, 12))
    cand[:, 0] = np.arange(n_cand)

    class Scripted:
        def __init__(self):
            self.scene, self.calls = None, 0

        def set_instance_scene(self, geom=None):
            self.scene = None if geom is None else np.asarray(geom)[:, 0, 0].astype(int)

        def check_trajectory(self, x, tol_x=None):
            self.calls += 1
            assert self.scene is not None and len(self.scene) == len(x)
            return table[self.scene, x[:, 0, 0].astype(int)]

    def statement(scene_of):
        x0, c = [], 0
        for sn in scene_of:
            while c < n_cand and not table[sn, c]:
                c += 1
            if c == n_cand:
                break
            x0.append(c)
            c += 1
        return x0

    for scene_of in (rng.integers(0, n_sc, 20), np.zeros(12, int), rng.integers(0, n_sc, 38)):
        scenes = np.zeros((len(scene_of), 6, SCENE_ROW))
        scenes[:, :, 0] = scene_of[:, None]
        sv = Scripted()
        x0, filled = cl._free_starts_per_scene(sv, scenes, cand)
        want = statement(scene_of)
        assert filled.sum() == len(want) and filled[:len(want)].all()
        assert x0[filled, 0].astype(int).tolist() == want
        assert sv.scene is None                                  # the walk leaves no scene behind
        assert sv.calls <= (n_cand - len(want)) + 1              # one call per rejected candidate, plus one
    assert x0[filled, 0].astype(int).tolist() != list(range(int(filled.sum())))    # (candidates were skipped)
    assert not filled.all()                                      # 38 instances, 40 candidates, a third of them colliding
    same = np.zeros(12, int)
    assert statement(same) == np.where(table[0])[0][:12].tolist()
