"""CPU: the ant scene forest C-ABI is declared, bound and exported; the ant scenario loader on the reference's scenario file
(tests/golden/test_scenarios_ant.csv) gives the reference's starts and goals, held to the reference's own cell indexing;
plan_ant_scenario_runs refuses what it cannot run before it touches a planner or the GPU; and the run scheduler hands every
job's scene id to an ant scene engine."""
import os
import re
import types

import numpy as np
import pytest

from oracle import ant as OA
from ditreeonlineplanner_amd.planners._runs import Job, run_jobs
from tests.test_ant_forest_host import StubAntEngine, StubAntPlanner
from tests.util import REPO

ANT_SCENE_CALLS = ["ditree_forest_expand_round_ant_scenes", "ditree_forest_fallback_goals_ant"]
ANT_CSV = os.path.join(REPO, "tests", "golden", "test_scenarios_ant.csv")


def test_ant_scene_symbols_declared_bound_and_exported():
    from ditreeonlineplanner_amd import _lib
    hdr = open(os.path.join(REPO, "include", "ditree.h")).read()
    assert "ant scene forests" in hdr
    for name in ANT_SCENE_CALLS:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(_lib.lib(), name), name
    assert _lib.lib().ditree_version() == 400


# ---------------------------------------------------------------------- the scenario loader
def test_ant_scenarios_are_the_references_rows():
    """15 scenarios on 7 distinct mazes of 2 299 cells; start = zeros(29) with xy, 0.75, 1.0 and goal = zeros(29) with xy
    (run_scenarios.py:226-233), xy = the cell centre in the map scaled by 4."""
    from ditreeonlineplanner_amd.scenarios import ant_scenarios
    sc = ant_scenarios(ANT_CSV)
    assert len(sc) == 15
    mazes = {s["maze_name"]: s["maze"] for s in sc}
    assert len(mazes) == 7 and sum(m.size for m in mazes.values()) == 2299
    assert [s["name"] for s in sc][:3] == ["random xlarge easy", "boxes", "boxes2"]
    for s in sc:
        H, W = s["maze"].shape
        for key, cell in (("start", s["start_cell"]), ("goal", s["goal_cell"])):
            v = s[key]
            assert v.shape == (29,) and v.dtype == np.float64
            assert v[0] == (cell[1] + 0.5) * 4.0 - W * 4.0 / 2 and v[1] == H * 4.0 / 2 - (cell[0] + 0.5) * 4.0
        assert s["start"][2] == 0.75 and s["start"][3] == 1.0 and not s["start"][4:].any()
        assert not s["goal"][2:].any()
    first = sc[0]
    assert first["maze_name"] == "random_xlarge" and first["start_cell"] == (1, 1) and first["goal_cell"] == (3, 7)
    assert np.array_equal(first["start"][:2], [-20.0, 20.0]) and np.array_equal(first["goal"][:2], [4.0, 12.0])
    # another scale: the same cells
    half = ant_scenarios(ANT_CSV, s_global=2.0)
    assert all(np.array_equal(a["start"][:2], b["start"][:2] / 2) for a, b in zip(half, sc))


def test_ant_scenario_cells_index_back_under_the_references_own_indexing():
    """The cell -> xy map is third party (parity unpinned); it is held to is_colliding_maze's indexing
    (common/map_utils.py:155-159 as oracle/ant.py restates it): every start and goal centre indexes back to its own (row, col),
    lands on a free cell, and the ant does not collide there."""
    from ditreeonlineplanner_amd.scenarios import ant_scenarios
    s = 4.0
    for sc in ant_scenarios(ANT_CSV):
        maze = sc["maze"]
        H, W = maze.shape
        for key, cell in (("start", sc["start_cell"]), ("goal", sc["goal_cell"])):
            x, y = sc[key][:2]
            xc, yc = W / 2.0 * s, H / 2.0 * s
            row, col = int(np.floor((yc - y) / s)), int(np.floor((x + xc) / s))
            assert (row, col) == cell, (sc["name"], key)
            assert maze[row, col] == 0, (sc["name"], key)
            state = sc[key].copy()
            state[3] = 1.0                                        # an upright torso (the goal vector has no quaternion)
            assert not OA.is_colliding_ant(state[None], maze, 1.2, 4.0)[0], (sc["name"], key)
        assert not OA.is_colliding_ant(sc["start"][None], maze, 1.2, 4.0)[0]


# ---------------------------------------------------------------------- plan_ant_scenario_runs argument rules (no GPU)
SAMPLER = types.SimpleNamespace(sample_round=None)
CTX = object()
MODEL_BYTES = b"\x01" * 8


def _fake(**kw):
    eng = types.SimpleNamespace(H=48, A=2, P=16, lm_n=16, lm_scale=0.8, s_global=4.0, k_steps=1, norm=np.arange(70.0), early_exit=1,
                                model=MODEL_BYTES, ball_radius=1.2, goal_radius=1.8)
    p = types.SimpleNamespace(is_ant=True, run_type=0, world_size=1, sampler=SAMPLER, ctx=CTX, batch=16, ant_dynamics="model",
                              _engine=eng)
    for k, v in kw.items():
        if hasattr(eng, k):
            setattr(eng, k, v)
        else:
            setattr(p, k, v)

    def reset(*a, **k):
        raise AssertionError("plan_ant_scenario_runs touched a planner before refusing")
    p.reset = reset
    return p


def test_plan_ant_scenario_runs_refuses_without_touching_the_gpu():
    from ditreeonlineplanner_amd.planners.RRT import plan_ant_scenario_runs, plan_scenario_runs
    with pytest.raises(NotImplementedError, match="antmaze planners only") as e:
        plan_ant_scenario_runs([_fake(), _fake(is_ant=False)], [[1], [2]])
    assert "plan_scenario_runs" in str(e.value)
    with pytest.raises(NotImplementedError, match="host"):
        plan_ant_scenario_runs([_fake(), _fake(ant_dynamics="host")], [[1], [2]])
    with pytest.raises(NotImplementedError, match="run_type 0"):
        plan_ant_scenario_runs([_fake(), _fake(run_type=1)], [[1], [2]])
    with pytest.raises(NotImplementedError, match="one rank"):
        plan_ant_scenario_runs([_fake(world_size=2)], [[1]])
    with pytest.raises(NotImplementedError, match="plain-callable"):
        plan_ant_scenario_runs([_fake(sampler=lambda *a: None)], [[1]])
    with pytest.raises(ValueError, match="one list per planner"):
        plan_ant_scenario_runs([_fake(), _fake()], [[1]])
    for kw, name in ((dict(sampler=types.SimpleNamespace(sample_round=None)), "sampler"), (dict(ctx=object()), "ctx"),
                     (dict(H=24), "edge_length"), (dict(A=4), "action_horizon"), (dict(P=32), "pred_horizon"),
                     (dict(lm_n=20), "local map size"), (dict(lm_scale=0.2), "local map scale"), (dict(s_global=2.0), "s_global"),
                     (dict(k_steps=4), "k_steps"), (dict(norm=np.ones(70)), "norm"), (dict(early_exit=0), "early_exit"),
                     (dict(batch=8), "batch"), (dict(ant_dynamics="tape"), "ant_dynamics"), (dict(model=b"\x02" * 8), "ant_model"),
                     (dict(ball_radius=1.0), "ball_radius"), (dict(goal_radius=1.0), "goal_radius")):
        with pytest.raises(ValueError, match=f"plan_ant_scenario_runs: planner 2 differs from planner 0 in {name}"):
            plan_ant_scenario_runs([_fake(), _fake(), _fake(**kw)], [[1], [2], [3]])
    # the first difference is the one named
    with pytest.raises(ValueError, match="in action_horizon"):
        plan_ant_scenario_runs([_fake(), _fake(A=4, batch=8)], [[1], [2]])
    assert plan_ant_scenario_runs([], []) == []
    # the car's function keeps refusing ant planners, and names this one
    with pytest.raises(NotImplementedError, match="car") as e:
        plan_scenario_runs([_fake()], [[1]])
    assert "plan_ant_scenario_runs" in str(e.value)


# ---------------------------------------------------------------------- the run scheduler on a stub ant scene engine
def test_run_loop_hands_every_jobs_scene_to_the_ant_scene_engine():
    """Four jobs of two scenarios (scene ids 0 and 1, as plan_ant_scenario_runs queues them) on two trees: reset_tree gets the
    job's scene id, a freed tree takes the next job whatever its scene, and the tape slices stay per run."""
    pa, pb = StubAntPlanner(100.0, 5, 0.1), StubAntPlanner(200.0, 3, 0.25)
    eng = StubAntEngine()
    res = [[None, None], [None, None]]
    jobs = [Job(pl, seed, (res[i], k), (i,)) for i, pl in enumerate((pa, pb)) for k, seed in enumerate((10 + i, 20 + i))]
    out = run_jobs(eng, jobs, 4, "cpu")
    assert out == res[0] + res[1] and all(r is not None for r in out)
    assert [(t, a) for t, a in eng.resets] == [(0, (0,)), (1, (0,)), (0, (1,)), (1, (1,))]
    assert [r["seed"] for r in out] == [10, 20, 11, 21]
    for counts, s, acts, tape, scenes in eng.rounds:              # StubAntEngine.tag_of holds what reset_tree received: the scene
        lo = 0
        for t, n in enumerate(counts):
            if n:
                pl = (pa, pb)[scenes[t]]
                assert (tape[lo:lo + n, 0, 0, 1] == pl.tag).all() and (acts[lo:lo + n, 0, 0, 1] == pl.tag).all()
                first = tape[lo, 0, 0, 0]
                assert np.array_equal(tape[lo:lo + n, 0, 0, 0], np.arange(first, first + n))
                lo += n
    assert pa.tape_calls == [(0, 4), (0, 4), (4, 1), (4, 1)] and pb.tape_calls == [(0, 3), (0, 3)]
    assert [r["number_of_nodes"] for r in out] == [6, 6, 4, 4]
