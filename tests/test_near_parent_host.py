"""CPU: the planner's ``near_radius`` where no GPU is needed -- the four entry points in the header, the binding and the library,
the descriptor's layout, the refusals of the planner and the engine by message (nothing of the device is touched before they are
raised), what an engine with and without ``near_radius`` hands to the library (the recorder of
tests/test_engine_dispatch_host.py stands in for it), and the restatement of tests/near_parent_ref.py on designed cases."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from ditreeonlineplanner_amd import _lib
from ditreeonlineplanner_amd import engine as E
from ditreeonlineplanner_amd.planners import RRT as F
from tests.near_parent_ref import NO_BOUND, near_parent_fast, near_parent_ref
from tests.test_engine_dispatch_host import (B, CAP, COUNTS, KINDS, StubContext, check_bound, check_params, check_round_desc,  # noqa: F401
                                             make_engine, rec, round_inputs)
from tests.test_solution_modes_host import _AntEnv, _car_args
from tests.util import REPO

NEW_CALLS = ["ditree_nn_argmin_near", "ditree_forest_nn_argmin_near", "ditree_expand_round_near", "ditree_forest_expand_round_near"]


def test_near_symbols_declared_bound_and_exported():
    hdr = open(os.path.join(REPO, "include", "ditree.h")).read()
    for name in NEW_CALLS:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name), name
    assert _lib.lib().ditree_version() == 400


def test_near_descriptor_layout_matches_the_header():
    hdr = open(os.path.join(REPO, "include", "ditree.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} ditree_near;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(?:const\s+)?(int32_t|double)\s*(\*?)\s*(\w+);", body)
    assert [f[2] for f in fields] == [n for n, _ in _lib.Near._fields_] == ["cost", "radius", "reach"]
    for (typ, star, name), (_, ctype) in zip(fields, _lib.Near._fields_):
        assert ctype is (C.c_void_p if star else C.c_double), name
    assert C.sizeof(_lib.Near) == 3 * 8


# ---------------------------------------------------------------------- refusals
def test_planner_refuses_by_name():
    start, goal, args = _car_args(solution="anytime", near_radius=1.0)
    with pytest.raises(ValueError, match="near_radius needs solution="):
        F.RRT_Planner(start, goal, **dict(args, solution="first"))
    del args["solution"]
    with pytest.raises(ValueError, match="near_radius needs solution="):                 # the default mode
        F.RRT_Planner(start, goal, **args)
    args["solution"] = "anytime"
    for sol in ("best_of_round", "anytime", "anytime_pruned"):
        with pytest.raises(ValueError, match="near_speed belongs to near_radius"):
            F.RRT_Planner(start, goal, **dict(args, solution=sol, near_radius=None, near_speed=5.0))
    for bad in (0, -1.0, float("nan"), float("inf"), "1", True):
        with pytest.raises(ValueError, match="near_radius must be a positive finite number"):
            F.RRT_Planner(start, goal, **dict(args, near_radius=bad))
        with pytest.raises(ValueError, match="near_speed must be a positive finite number"):
            F.RRT_Planner(start, goal, **dict(args, near_speed=bad))
    with pytest.raises(NotImplementedError, match="near_radius: the car only"):
        F.RRT_Planner(np.zeros(29), np.zeros(29), **dict(args, env_id="antmaze", environment=_AntEnv()))
    with pytest.raises(NotImplementedError, match="near_radius: one rank"):
        F.RRT_Planner(start, goal, **dict(args, world_size=2))
    with pytest.raises(NotImplementedError, match="near_radius: run_type 0 only"):
        F.RRT_Planner(start, goal, **dict(args, run_type=2))
    with pytest.raises(NotImplementedError, match="near_radius: a single prop_duration entry"):
        F.RRT_Planner(start, goal, **dict(args, prop_duration=[32, 64]))


def test_engine_refuses_by_name():
    assert E.check_near(None, None, "first") is None
    assert E.check_near(1.5, None, "anytime") == (1.5, E.CAR_REACH) and E.check_near(2, 0.05, "anytime_pruned") == (2.0, 0.05)
    with pytest.raises(ValueError, match="near_reach belongs to near_radius"):
        E.check_near(None, 0.1, "anytime")
    for bad in (0.0, -0.1, float("nan"), float("inf"), "x", True):
        with pytest.raises(ValueError, match="near_radius must be a positive finite number of metres"):
            E.check_near(bad, 0.1, "anytime")
        with pytest.raises(ValueError, match="near_reach must be a positive finite number of metres per path row"):
            E.check_near(1.0, bad, "anytime")
    with pytest.raises(ValueError, match="near_radius needs a solution other than 'first'"):
        E.check_near(1.0, 0.1, "first")
    with pytest.raises(NotImplementedError, match="near_radius: the car only"):
        E.check_near(1.0, 0.1, "anytime", ant=True)
    maze = np.zeros((4, 4), dtype=np.float32)
    with pytest.raises(NotImplementedError, match="near_radius: a single prop_duration entry"):
        E.ExpansionEngine(object(), maze, np.zeros(6), np.zeros(6), emulate_sticky_done=False, solution="anytime",
                          prop_duration=[32, 64], near_radius=1.0)
    with pytest.raises(NotImplementedError, match="one rank"):
        E.ExpansionEngine(object(), maze, np.zeros(6), np.zeros(6), emulate_sticky_done=False, solution="anytime", world_size=2,
                          near_radius=1.0)


# ---------------------------------------------------------------------- what reaches the library
def one_round(rec, eng, forest):
    rec.calls.clear()
    samples, cond, acts, extra = round_inputs(eng, False)
    if forest:
        extra["counts_per_tree"] = COUNTS
    eng.expand_round(samples, cond, inject_actions=acts, **extra)
    assert rec.problems == []
    return samples, cond, acts, extra


@pytest.mark.parametrize("kind", ["single", "forest", "scene"])
@pytest.mark.parametrize("mode", ["first", "best_of_round", "anytime", "anytime_pruned"])
def test_without_near_radius_no_near_entry_is_reached(rec, kind, mode):
    eng, _ = make_engine(rec, kind, mode)
    assert eng.near is None and "near" not in eng.entries.expand
    one_round(rec, eng, KINDS[kind][1])
    assert not any("near" in n for n in rec.names())
    kw = eng.round_settings()
    assert kw["near_radius"] is None and kw["near_reach"] is None


def test_a_planner_without_near_radius_builds_todays_engine(rec):
    """``near_radius=None`` (given or left out): the engine is built without the search, its round calls are those of the
    planner without the kwarg, and no ``*_near`` entry is reached."""
    names = []
    for more in ({}, {"near_radius": None}, {"near_radius": None, "near_speed": None}):
        start, goal, args = _car_args(solution="anytime", ctx=StubContext(rec), batch=8, capacity=64, prop_duration=[16], **more)
        pl = F.RRT_Planner(start, goal, **args)
        assert pl.near_radius is None and pl.near_speed is None and pl.near_reach is None and pl._engine.near is None
        one_round(rec, pl._engine, False)
        names.append(rec.names())
        assert not any("near" in n for n in names[-1]) and "ditree_expand_round" in names[-1]
    assert names[0] == names[1] == names[2]


@pytest.mark.parametrize("kind", ["single", "forest", "scene"])
@pytest.mark.parametrize("mode", ["best_of_round", "anytime", "anytime_pruned"])
def test_with_near_radius_the_round_takes_the_near_entry(rec, kind, mode):
    """The one expand entry of the search: [scenes or NULL], round, parameters, the bound or NULL, the near descriptor on the
    tree's cost column; the accept and the fallback are the mode's own."""
    _, forest, scenes, _ = KINDS[kind]
    eng, _ = make_engine(rec, kind, mode, near_radius=1.5, near_reach=0.05)
    plain, _ = make_engine(rec, kind, mode)
    assert eng.near == (1.5, 0.05)
    samples, cond, acts, extra = one_round(rec, eng, forest)
    name = "ditree_forest_expand_round_near" if forest else "ditree_expand_round_near"
    assert eng.entries.expand == name and eng.entries.accept == plain.entries.accept and eng.entries.fallback == plain.entries.fallback
    pruned = mode == "anytime_pruned"
    roots = [0, CAP] if forest else [0]
    assert rec.names() == (["ditree_bound_keys"] * len(roots) if pruned else []) + [name, plain.entries.accept]
    c = next(c for c in rec.calls if c.name == name)
    k = 3 if forest else 2
    if forest:
        assert (c.raw[k]._obj is eng.sdesc) if scenes else (c.raw[k] is None)
        k += 1
    check_round_desc(c.args[k], eng, 0, B)
    check_params(c, c.args[k + 1], eng, False, 0, B, samples, cond, acts, extra, False)
    if pruned:
        assert c.raw[k + 2]._obj is eng.bound
        check_bound(c.args[k + 2], eng, eng.fstats if forest else eng.tree.stats)
    else:
        assert c.raw[k + 2] is None
    nr = c.args[k + 3]
    assert isinstance(nr, _lib.Near) and (nr.cost, nr.radius, nr.reach) == (eng.tree.cost.data_ptr(), 1.5, 0.05)
    assert len(c.raw) == k + 5 and c.raw[-1] is eng.ctx.stream
    kw = eng.round_settings()
    assert (kw["near_radius"], kw["near_reach"]) == (1.5, 0.05)


def test_the_planner_hands_radius_and_reach_to_its_engine(rec):
    start, goal, args = _car_args(solution="anytime", ctx=StubContext(rec), batch=8, capacity=64, prop_duration=[16])
    pl = F.RRT_Planner(start, goal, **dict(args, near_radius=2))
    assert (pl.near_radius, pl.near_speed) == (2.0, pl.max_v) and pl.near_reach == pl.max_v * pl.env_dt
    assert pl._engine.near == (2.0, pl.near_reach)
    pl = F.RRT_Planner(start, goal, **dict(args, near_radius=0.5, near_speed=2.5, solution="anytime_pruned"))
    assert pl._engine.near == (0.5, 2.5 * pl.env_dt) and pl._engine.reach == pl.max_v * pl.env_dt
    one_round(rec, pl._engine, False)
    assert "ditree_expand_round_near" in rec.names() and "ditree_expand_round_bounded" not in rec.names()
    settings = dict(F._scene_settings(pl))
    assert settings["near_radius"] == 0.5 and settings["near_speed"] == 2.5


# ---------------------------------------------------------------------- the restatement on designed cases
def test_restatement_designed_cases():
    # nodes on integers, reach 1: g = cost + distance, every value exact
    xy = np.array([[0.0, 0.0], [3.0, 4.0], [6.0, 8.0], [0.0, 5.0], [-5.0, 0.0], [np.nan, 1.0]])
    q = np.array([[0.0, 0.0]])
    cost = np.array([20, 10, 4, 15, 15, 0])
    # radius 5: n* = 0 (d 0), near = {0, 1, 3, 4} (d <= 5), g = 20, 15, 20, 20 -> node 1
    p, star, size = near_parent_ref(q, xy, cost, 5.0, 1.0, detail=True)
    assert (p[0], star[0], size[0]) == (1, 0, 4)
    # radius 10: node 2 (d 10, g 14) is just inside; radius 9.99: just outside
    assert near_parent_ref(q, xy, cost, 10.0, 1.0)[0] == 2 and near_parent_ref(q, xy, cost, 9.99, 1.0)[0] == 1
    # equal g with different d2: cost 15 at distance 5 against cost 20 at distance 0 -> the smaller d2
    assert near_parent_ref(q, xy, np.array([20, 30, 40, 15, 15, 0]), 5.0, 1.0)[0] == 0
    # equal g and equal d2 (nodes 3 and 4): the lower index
    assert near_parent_ref(q, xy, np.array([30, 30, 40, 15, 15, 0]), 5.0, 1.0)[0] == 3
    # equal costs: the nearest node; n* closed under the mask: the nearest open node leads
    assert near_parent_ref(q, xy, np.full(6, 7), 50.0, 1.0)[0] == 0
    key = np.array([9, 1, 1, 1, 1, 1])
    p, star, size = near_parent_ref(q, xy, cost, 1.0, 1.0, key=key, U=5, detail=True)
    assert (p[0], star[0], size[0]) == (1, 1, 3)              # n* = 1 (d 5), tau = 6: nodes 1, 3, 4
    # nothing open, or only NaN distances: lo
    assert near_parent_ref(q, xy, cost, 1.0, 1.0, key=key, U=0)[0] == 0
    assert near_parent_ref(q, xy, cost, 1.0, 1.0, lo=5, hi=6)[0] == 5 and near_parent_ref(q, xy, cost, 1.0, 1.0, lo=3, hi=3)[0] == 3
    assert near_parent_ref(np.array([[np.nan, 0.0]]), xy, cost, 1.0, 1.0)[0] == 0
    # a range: only its nodes count
    # a range: only its nodes count -- n* = 3 (the first at distance 5), tau = 10 takes node 2 in: g = 14 against 20 and 20
    p, star, size = near_parent_ref(q, xy, cost, 5.0, 1.0, lo=2, hi=5, detail=True)
    assert (p[0], star[0], size[0]) == (2, 3, 3)


@pytest.mark.parametrize("solution", ["best_of_round", "anytime", "anytime_pruned"])
def test_preconditions_of_the_device_tests(solution):
    """On the restated planner, never on the device: at a radius of one maze cell (1 m) the scenario's seed has rounds whose
    parents are not the plain nearest nodes, every such parent costs less, and the run draws what the run without the rule
    draws."""
    from oracle import rrt as ORRT
    from tests.anytime_pruned_ref import BATCH, ROUNDS, SEED
    from tests.near_parent_ref import near_run
    o = near_run(solution, 1.0)
    moved = [np.asarray(r["parent"]) != r["nearest"] for r in o.rounds]
    assert not moved[0].any() and sum(int(m.sum()) for m in moved[1:]) > 10       # round 1 has the root alone
    for r, m in zip(o.rounds, moved):
        for b in np.nonzero(m)[0]:                                 # farther than n* and still the smaller g: strictly cheaper
            assert o.cost[int(r["parent"][b])] < o.cost[int(r["nearest"][b])]
    assert len(o.rounds) == (2 if solution == "best_of_round" else ROUNDS) and o.incumbent is not None
    tape = ORRT.RandomTape(SEED)
    H, W = o.pl.maze.shape
    for _ in o.rounds:
        tape.draw_round(BATCH, W, H, o.pl.goal_state, goal_sample_rate=o.pl.gsr, goal_conditioning_bias=o.pl.gcb)
    assert tape.py.getstate() == o.tape.py.getstate()
    a, b = tape.np.get_state(), o.tape.np.get_state()
    assert np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def test_precondition_of_the_reuse_test():
    """The room of tests/test_gpu_tree_reuse.py at 0.5 m and 0.5 m/s: the restated plan reaches its goal within four rounds over a
    chain of at least four nodes, with parents that are not the nearest node; at the default speed it does not reach it."""
    from oracle import geometry as G
    from oracle import rrt as ORRT
    from oracle.tapes import ActionTape
    from tests.near_parent_ref import near_run
    from tests.test_gpu_tree_reuse import BATCH, EDGE, ROUNDS, SEED, TAPE, room

    def planner():
        maze = room()
        start = np.array([*G.cell_rowcol_to_xy([7, 2], maze), 0.0, 0, 0, 0])
        goal = np.array([*G.cell_rowcol_to_xy([7, 5], maze), 0, 0, 0, 0])
        return ORRT.OraclePlanner(maze, start, goal, ActionTape(TAPE).sampler(), edge_length=EDGE, emulate_sticky_done=False)
    o = near_run("anytime", 0.5, near_speed=0.5, seed=SEED, rounds=ROUNDS, scenario=("room", planner, BATCH))
    chain, n = [], o.incumbent
    while n is not None and n >= 0:
        chain.append(n)
        n = o.pl.tree.parents[n]
    assert len(chain) >= 4 and sum(int((np.asarray(r["parent"]) != r["nearest"]).sum()) for r in o.rounds) > 0
    assert near_run("anytime", 0.5, seed=SEED, rounds=ROUNDS, scenario=("room", planner, BATCH)).incumbent is None


def test_restatements_agree():
    rng = np.random.RandomState(1)
    xy = rng.uniform(-5, 5, (400, 2))
    xy[7] = xy[3]
    xy[11] = np.nan
    xy[100:140] = np.round(xy[100:140])                         # lattice points: exact ties
    cost = rng.randint(1, 60, 400)
    cost[7] = cost[3]
    q = np.concatenate([rng.uniform(-5, 5, (40, 2)), xy[[3]], [[np.nan, 0.0]], np.round(rng.uniform(-5, 5, (20, 2)))])
    key = rng.randint(0, 100, 400)
    differs = 0
    for radius in (0.25, 1.0, 3.0):
        for reach in (0.1, 1.0):
            for U in (None, 0, 50, NO_BOUND):
                kw = {} if U is None else dict(key=key, U=U)
                for lo, hi in ((0, 400), (0, 1), (90, 150), (200, 200)):
                    a = near_parent_ref(q, xy, cost, radius, reach, lo=lo, hi=hi, detail=True, **kw)
                    b = near_parent_fast(q, xy, cost, radius, reach, lo=lo, hi=hi, detail=True, block=7, **kw)
                    for u, v in zip(a, b):
                        assert np.array_equal(u, v)
                    differs += int((a[0] != a[1]).sum())
    assert differs > 100                                         # the rule is not the nearest node
    same = near_parent_fast(q, xy, np.full(400, 9), 3.0, 0.1, detail=True)
    assert np.array_equal(same[0], same[1])
