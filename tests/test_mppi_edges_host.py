"""CPU checks of tests/mppi_edge_cases.py, the inputs tests/test_gpu_mppi_edges.py runs on the device.

CONDITIONS -- every property of the inputs that the GPU tests rely on (collided and free rollouts on every map, windows clipped at
both ends, ties, weights that underflow, a step that is inside the goal radius and collides, a shard whose first rollout carries
noise, ...) is asserted here on the numpy restatement (oracle/mppi.py).
MUTANTS -- ten defects of the kinds the kernels could have, each applied to a COPY of the restatement (one source line of the
function rewritten and compiled in the test; oracle/ stays as it is) or as a wrapper around its noise / update.  On the inputs of
the case family named for it, the mutant's result must leave the bounds the GPU test holds the device to: a case set that could
not tell the defect from the right controller fails here, without a device."""
import inspect
import types

import numpy as np
import pytest

from oracle import geometry as G
from oracle import mppi as OM
from tests import mppi_edge_cases as E


# ---------------------------------------------------------------------------------------------- mutants
def rewritten(module, fn_name, edits, extra=None):
    """A copy of `module` whose function `fn_name` has every (old, new) of `edits` applied to its source (each `old` must stand
    in it exactly once)."""
    src = inspect.getsource(getattr(module, fn_name))
    for old, new in edits:
        assert src.count(old) == 1, (fn_name, old)
        src = src.replace(old, new)
    ns = dict(vars(module))
    ns.update(extra or {})
    exec(compile(src, f"<mutant of {module.__name__}.{fn_name}>", "exec"), ns)
    return ns[fn_name]


def mutant(**fns):
    """A stand-in for oracle.mppi with some functions replaced."""
    m = types.SimpleNamespace(**{k: getattr(OM, k) for k in ("rollout_costs", "rollout_costs_ant", "update", "update_ant")})
    for k, v in fns.items():
        setattr(m, k, v)
    return m


WINDOW_OK = "ok = (w >= 0) & (w <= P - 1)"
ARGMIN = "j = np.argmin(dd, axis=1)"
ARGMIN0 = "i0 = int(np.argmin(d0))"
PROGRESS = "cost = cost + w_progress * (P - 1 - ip).astype(np.float64)"
NOMINAL = "    if k0 == 0:\n        eps[0] = 0.0"
EDITS = {
    "window_hi": [(WINDOW_OK, "ok = (w >= 0) & (w <= np.minimum(ip[idx] + window_fwd, P - 1)[:, None] - 1)")],
    "window_lo": [(WINDOW_OK, "ok = (w >= np.maximum(ip[idx] - window_back, 0)[:, None] + 1) & (w <= P - 1)")],
    "ties_last": [(ARGMIN, "j = dd.shape[1] - 1 - np.argmin(dd[:, ::-1], axis=1)"), (ARGMIN0, "i0 = P - 1 - int(np.argmin(d0[::-1]))")],
    "progress_i0": [(PROGRESS, "cost = cost + w_progress * (P - 1 - np.full(K, i0)).astype(np.float64)")],
    "goal_first": [("only_goal = reached & ~coll", "only_goal = reached"),
                   ("cost[idx[coll]] = cost[idx[coll]] + w_collision\n        flags[idx[coll]] = 2",
                    "cost[idx[coll & ~reached]] = cost[idx[coll & ~reached]] + w_collision\n        flags[idx[coll & ~reached]] = 2")],
    "nominal_in_every_shard": [(NOMINAL, "    if True:\n        eps[0] = 0.0")],
}


def source_mutant(name):
    fns = {fn: rewritten(OM, fn, EDITS[name]) for fn in ("rollout_costs", "rollout_costs_ant")}
    if name == "nominal_in_every_shard":
        fns.update({fn: rewritten(OM, fn, EDITS[name]) for fn in ("update", "update_ant")})
    return mutant(**fns)


def swapped_centre():
    """The map centre taken as (rows / 2, cols / 2): oracle.geometry's ball test with the two centre lines exchanged."""
    ball = rewritten(G, "_ball_collides", [("xc = W / 2 * scale\n    yc = H / 2 * scale", "xc = H / 2 * scale\n    yc = W / 2 * scale")])
    car = rewritten(G, "is_colliding_car", [], extra={"_ball_collides": ball})
    g = types.SimpleNamespace(**{k: getattr(G, k) for k in ("car_step", "goal_reached", "norm2")}, is_colliding_car=car)
    return mutant(rollout_costs=rewritten(OM, "rollout_costs", [], extra={"G": g}))


def last_step_zeroed(eps):
    e = eps.copy()
    if e.shape[1] % 2:
        e[:, -1] = 0.0
    return e


def steps_exchanged(eps):
    """The noise of step t and of step t ^ 1 exchanged (an odd horizon's last step keeps its own)."""
    e = eps.copy()
    T = e.shape[1]
    for t in range(0, T - 1, 2):
        e[:, [t, t + 1]] = e[:, [t + 1, t]]
    return e


def floor_slices_update(case, costs, eps):
    """`per = K // slices`: the rollouts past slices * per never reach the sums (eta, sum w^2, the controls, the weights)."""
    slices = E.slices_of(case.K)[0]
    kept = slices * (case.K // slices)
    beta = float(np.min(costs))
    w = np.exp(-(costs - beta) / case.lam)
    w[kept:] = 0.0
    e = eps.copy()
    if case.k0 == 0:
        e[0] = 0.0
    eta = float(w.sum())
    return case.U + np.tensordot(w, e, axes=(0, 0)) / eta, w / eta, beta, eta, eta * eta / float((w * w).sum())


def result_of(case, om=OM, eps=None, update=None):
    """Deviations of a (mutant) restatement from the restatement, in the GPU test's quantities."""
    eps = case.ref()["eps"] if eps is None else eps
    c, f, i0, _ = case.rollouts(om=om, eps=eps)
    with np.errstate(all="ignore"):
        Un, w, beta, eta, ess = case.update(c, om=om, eps=eps) if update is None else update(case, c, eps)
    return E.deviations(case.ref(), c, f, i0, U=Un, w=w, beta=beta, eta=eta, ess=ess)


def caught(case, **kw):
    return E.outside(result_of(case, **kw), case.ref())


def test_the_restatement_itself_stays_inside_every_bound():
    """The check that rejects the mutants accepts the restatement (and an unedited copy of it)."""
    same = mutant(rollout_costs=rewritten(OM, "rollout_costs", []), update=rewritten(OM, "update", []))
    for case in (E.map_case("Race_Track", "car", "device"), E.horizon_case(5), E.shard_case(), E.window_case(7, (0, 3), "mid")):
        assert caught(case) == [] and caught(case, om=same) == []


# ---------------------------------------------------------------------------------------------- a. non-square maps
@pytest.mark.parametrize("name", E.MAP_NAMES)
@pytest.mark.parametrize("model", ["car", "ant"])
def test_maps_have_collided_and_free_rollouts(name, model):
    for noise in ("device", "tape"):
        case = E.map_case(name, model, noise)
        r = case.ref()
        assert case.K == 512 and case.T == (16 if model == "car" else 5)
        assert (r["flags"] == 2).sum() >= 16 and (r["flags"] != 2).sum() >= 16, np.bincount(r["flags"], minlength=3)
        assert np.isfinite(r["costs"]).all()
    if name != "boxes":
        assert case.maze.shape[0] != case.maze.shape[1]
        assert len(np.unique(case.eps()[1:, 0, 0])) == case.K - 1


@pytest.mark.parametrize("name", ["Race_Track", "narrow_short.T"])
def test_swapped_map_centre_changes_a_quarter_of_the_flags(name):
    om = swapped_centre()
    for noise in ("device", "tape"):
        case = E.map_case(name, "car", noise)
        c, f, i0, _ = case.rollouts(om=om)
        assert (f != case.ref()["flags"]).sum() >= case.K // 4
        assert "flags" in caught(case, om=om)
    square = E.map_case("boxes", "car", "device")                      # the control: a square map cannot tell
    assert caught(square, om=om) == []


def test_executed_steps_have_the_status_they_are_built_for():
    seen = set()
    for name, model, map_name, state, U, goal, status in E.executed_steps():
        maze = E.the_map(map_name)
        if model == "car":
            x, a, st, Un = OM.execute(maze, state, U, goal)
        else:
            x, a, st, Un = OM.execute_ant(maze, state, U, goal, s_global=E.S_GLOBAL)
        assert st == status, (name, st)
        seen.add((map_name, model, status))
        if status == 2:
            assert np.array_equal(x, state) and (Un == 0).all()
        else:
            assert not np.array_equal(x, state) and np.array_equal(Un[:-1], U[1:]) and np.array_equal(Un[-1], U[-1])
    assert {(n, m, 0) for n in E.MAP_NAMES for m in ("car", "ant")} <= seen
    assert ("Race_Track", "car", 1) in seen and ("Race_Track", "car", 2) in seen
    assert np.abs(E.executed_steps()[0][4][0]).max() > 10.0            # the clip of the first control is exercised


# ---------------------------------------------------------------------------------------------- b. horizons
def test_horizons_and_their_rollout_count():
    assert E.HORIZONS == (1, 3, 5, 63, 64)
    for T in E.HORIZONS:
        case = E.horizon_case(T)
        assert case.K == 130 and case.T == T and all((case.K * lanes) % 256 for lanes in E.LANES)
        assert np.isfinite(case.ref()["costs"]).all() and len(np.unique(case.ref()["costs"])) == case.K


@pytest.mark.parametrize("T", [1, 3, 5, 63])
def test_odd_horizon_noise_mutants_are_caught(T):
    case = E.horizon_case(T)
    eps = case.ref()["eps"]
    assert "costs" in caught(case, eps=last_step_zeroed(eps))
    if T > 1:                                                         # T = 1 has no pair of steps to exchange
        assert "costs" in caught(case, eps=steps_exchanged(eps))
    # the exchange on an even horizon is caught too: the pair generation is wrong at any T
    assert "costs" in caught(E.horizon_case(64), eps=steps_exchanged(E.horizon_case(64).ref()["eps"]))


# ---------------------------------------------------------------------------------------------- c. rollout counts
def test_rollout_counts_reach_the_slice_counts_they_are_chosen_for():
    assert [E.slices_of(K)[0] for K in E.COUNTS] == [1, 1, 1, 1, 2, 3]
    assert E.slices_of(257) == (2, 129) and E.slices_of(513) == (3, 171)
    for K in E.COUNTS:
        case = E.count_case(K)
        assert case.T == 5 and np.isfinite(case.ref()["costs"]).all()
    assert any((K * lanes) % 256 for K in (257, 513) for lanes in E.LANES)
    ant = E.ant_count_case()
    assert ant.K == 32769 and ant.T == 3                              # the first size on the 256-thread block, plus one rollout
    r = ant.ref()
    assert (r["flags"] == 2).sum() >= 16 and (r["flags"] != 2).sum() >= 16


def test_floor_division_of_the_slices_is_caught():
    case = E.count_case(257)                                          # per = 128: rollout 256 never reaches the sums
    r = case.ref()
    assert r["w"][256] > 1e-6                                         # it carries weight: dropping it moves eta by more than 1e-9
    out = caught(case, update=floor_slices_update)
    assert "eta" in out and "w" in out
    assert caught(E.count_case(255), update=floor_slices_update) == []   # one slice: nothing to drop


# ---------------------------------------------------------------------------------------------- d. path windows
def all_window_cases():
    return [c for P in E.WINDOW_P for c in E.window_cases(P)]


def test_window_cases_cover_the_edges():
    assert E.WINDOW_P == (1, 2, 7, 65, 66) and E.WINDOWS == ((0, 0), (0, 3), (8, 56), (64, 64))
    first = last = lo_clipped = hi_clipped = inner = 0
    for case in all_window_cases():
        r, P = case.ref(), len(case.path)
        assert case.K == 256 and case.T == 8 and len(case.staged_path()) == P
        want = {"first": 0, "last": P - 1, "mid": P // 2}[case.name.rsplit("/", 1)[1]]
        assert r["i0"] == want, (case, r["i0"])
        assert np.isfinite(r["costs"]).all()
        first += int((r["last_ip"] == 0).any() and P > 1)
        last += int((r["last_ip"] == P - 1).any() and P > 1)
        lo_clipped += int(r["i0"] - case.window[0] < 0)               # the first step's window of every rollout
        hi_clipped += int(r["i0"] + case.window[1] > P - 1)
        inner += int(r["i0"] - case.window[0] >= 0 and r["i0"] + case.window[1] <= P - 1)
    assert min(first, last, lo_clipped, hi_clipped, inner) >= 3, (first, last, lo_clipped, hi_clipped, inner)
    # a window that moves: some rollout ends away from i0, so the window of a later step is not the first one
    moving = E.window_case(66, (8, 56), "first").ref()
    assert (moving["last_ip"] > moving["i0"] + 8).any()


def test_ant_window_widths():
    assert [b + f + 1 for b, f in E.ANT_WINDOWS] == [1, 8, 9, 65]
    for P in (1, 66):
        for case in E.window_cases(P, "ant"):
            assert np.isfinite(case.ref()["costs"]).all() and case.K == 256 and case.T == 8


@pytest.mark.parametrize("name", ["window_hi", "window_lo", "progress_i0"])
def test_window_mutants_are_caught(name):
    om = source_mutant(name)
    hits = [case for case in all_window_cases() if caught(case, om=om)]
    assert len(hits) >= 6, (name, hits)
    if name == "window_hi":                                           # caught where the window is clipped by the path's end
        assert any(c.ref()["i0"] + c.window[1] > len(c.path) - 1 for c in hits)
        assert any(c.ref()["i0"] + c.window[1] <= len(c.path) - 1 for c in hits)
    if name == "window_lo":
        assert any(c.ref()["i0"] - c.window[0] < 0 for c in hits)
    if name != "progress_i0":                                         # and the ant's search is held to the same edges
        assert any(caught(c, om=om) for c in E.window_cases(66, "ant"))


def test_tie_cases_tie_and_the_last_index_mutant_is_caught():
    om = source_mutant("ties_last")
    rep, ret300, ret400 = E.tie_cases()
    assert rep.ref()["i0"] == 40 and (rep.ref()["last_ip"] == 40).sum() >= rep.K // 4       # the repeated point stays the nearest
    for case, other in ((ret300, 300), (ret400, 400)):
        p = case.staged_path()
        assert np.array_equal(p[10], p[other]) and np.array_equal(case.state[:2], p[10]) and case.ref()["i0"] == 10
        c, f, i0, _ = case.rollouts(om=om)
        assert i0 == other
    assert (300 % 256) // 64 == (10 % 256) // 64 and (400 % 256) // 64 != (10 % 256) // 64   # one wave of the block search; two waves
    for case in (rep, ret300, ret400):
        out = caught(case, om=om)
        assert "i0" in out and "costs" in out, (case, out)


# ---------------------------------------------------------------------------------------------- e. the full path table
@pytest.mark.parametrize("model", ["car", "ant"])
def test_full_table_case_stages_4096_points(model):
    case = E.full_table_case(model)
    assert len(case.path) > 4096 and len(case.staged_path()) == 4096 and case.K == 256 and case.T == 16
    assert 4096 * 16 + case.T * case.nu * 8 + 128 + case.maze.size > 64 * 1024        # the launcher's LDS request
    r = case.ref()
    assert 100 < r["i0"] < 3996 and (r["flags"] == 2).any() and (r["flags"] != 2).any()


# ---------------------------------------------------------------------------------------------- f. weights
def test_weight_cases():
    assert E.LAMS == (1e-3, 1.0, 1e3)
    for lam in E.LAMS:
        r = E.lam_case(lam).ref()
        assert (r["flags"] == 2).sum() >= 16 and (r["flags"] != 2).sum() >= 16
        assert np.isfinite(r["w"]).all() and abs(r["w"].sum() - 1) < 1e-12
    r = E.lam_case(1e-3).ref()
    assert (r["w"] == 0).sum() > 256 and r["ess"] < 2
    assert (E.lam_case(1e3).ref()["w"] > 0).all()                      # and the other end: no weight underflows
    r = E.all_collide_case().ref()
    assert (r["flags"] == 2).all() and np.isfinite(r["w"]).all() and abs(r["w"].sum() - 1) < 1e-12
    z = E.zero_tape_case()
    r = z.ref()
    assert (r["costs"] == r["costs"][0]).all() and (r["w"] == 1.0 / z.K).all() and abs(r["ess"] - z.K) < 1e-9 * z.K
    assert np.array_equal(r["U"], z.U) and np.abs(z.U).min() > 0


# ---------------------------------------------------------------------------------------------- g. goal and collision in one step
def test_goal_and_collision_step():
    case = E.goal_on_wall_case()
    r = case.ref()
    both = r["both"]
    assert both.sum() >= 1 and both[0] and (r["flags"][both] == 2).all() and (r["end_step"][both] == 0).all()
    # + w_collision and no - w_goal: the same rollouts without a goal reward cost the same, without a collision cost 1000 less
    no_goal = case.rollouts(w_goal=0.0)[0]
    no_coll = case.rollouts(w_collision=0.0)[0]
    assert np.array_equal(no_goal[both], r["costs"][both])
    assert np.abs(r["costs"][both] - no_coll[both] - 1.0e3).max() < 1e-9
    out = caught(case, om=source_mutant("goal_first"))
    assert "flags" in out and "costs" in out


# ---------------------------------------------------------------------------------------------- h. shards
def test_shard_case_and_the_nominal_rollout_mutant():
    case = E.shard_case()
    assert case.K == 300 and case.k0 == 300
    eps = case.ref()["eps"]
    assert np.abs(eps[0]).min() > 0                                    # the shard's rollout 0 is global rollout 300: it carries noise
    whole = E.Case("whole", "car", "boxes", case.path, case.goal_xy, case.state, case.U, 600, "device", seed=case.seed, counter=case.counter)
    assert np.array_equal(whole.eps()[300:], eps) and np.array_equal(whole.ref()["costs"][300:], case.ref()["costs"])
    assert "costs" in caught(case, om=source_mutant("nominal_in_every_shard"))
