"""GPU: a scene forest (ditreeonlineplanner_amd/forest.py SceneForestEngine, include/ditree.h "scene forests") grows every tree
exactly as its own single-tree engine does on its own maze, start and goal -- bit for bit -- and plan_scenario_runs equals
sequential seeded plan() calls of every scenario, run by run."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

from oracle import geometry as G
from oracle import rrt as ORRT
from oracle.tapes import ActionTape
from tests.test_gpu_forest import _rng_states, _same_states, _sampler, car_net, compare_tree, ctx, dev, net_ctx  # noqa: F401
from tests.util import load_maze

pytestmark = pytest.mark.gpu

H = 32
# (maze, start cell, start deg, goal cell): scene 0 is test_gpu_forest's boxes scenario (its tree of seed 200 reaches the goal in
# its first round of 3), scene 3 a second start / goal on the same maze; narrow_short and random_huge differ in shape and size.
SCENES = [("boxes", (18, 8), 0.0, (18, 10)), ("narrow_short", (1, 1), 0.0, (4, 9)), ("random_huge", (19, 21), 90.0, (15, 25)),
          ("boxes", (17, 2), 45.0, (2, 17))]
SEEDS = [200, 31, 32, 33]
COUNTS = [[3, 6, 1, 5], [5, 0, 7, 6], [2, 4, 0, 1]]


def scene(k):
    name, (sr, sc), deg, (gr, gc) = SCENES[k]
    maze = load_maze(name)
    start = np.array([*G.cell_rowcol_to_xy([sr, sc], maze), np.deg2rad(deg), 0, 0, 0])
    goal = np.array([*G.cell_rowcol_to_xy([gr, gc], maze), 0, 0, 0, 0])
    return maze, start, goal


def tape_rows(rt, at, n, drawn, maze, goal, n_chunks):
    s, c = rt.draw_round(n, maze.shape[1], maze.shape[0], goal)
    a = np.stack([at.actions(np.arange(drawn, drawn + n), j) for j in range(n_chunks)], axis=1)
    return s, c, a


def run_tape_rounds(ctx, forest, scene_of, early_exit, counts_list=COUNTS, singles=None, wrong=None):
    """Rounds of uneven per-tree counts on action tapes; every tree compared with its own engine after every round.  ``wrong``:
    engines that read scene 0's maze and goal for every tree (what a kernel ignoring the scene would compute)."""
    from ditreeonlineplanner_amd.engine import CNT_GOAL, ExpansionEngine
    T = forest.T
    if singles is None:
        singles = [ExpansionEngine(ctx, *scene(scene_of[t]), edge_length=H, batch=64, capacity=forest.C, early_exit=early_exit)
                   for t in range(T)]
    rts = [ORRT.RandomTape(s) for s in SEEDS[:T]]
    ats = [ActionTape(s + 1000) for s in SEEDS[:T]]
    drawn, done, last_lo, statuses, diverged = [0] * T, [False] * T, [0] * T, [], False
    for counts in counts_list:
        counts = [0 if done[t] else c for t, c in enumerate(counts)]
        S, Cg, Ac = [], [], []
        for t in range(T):
            if counts[t]:
                maze, _, goal = scene(scene_of[t])
                s, c, a = tape_rows(rts[t], ats[t], counts[t], drawn[t], maze, goal, forest.n_chunks)
                S.append(s), Cg.append(c), Ac.append(a)
                singles[t].expand_round(dev(s), dev(c), inject_actions=dev(a))
                statuses.append(singles[t].rb.status[:counts[t]].cpu().numpy() & 0xff)
                if wrong is not None and scene_of[t] != 0:
                    wrong[t].expand_round(dev(s), dev(c), inject_actions=dev(a))
                    diverged |= not torch.equal(wrong[t].rb.status[:counts[t]], singles[t].rb.status[:counts[t]])
        cnt = forest.expand_round(dev(np.concatenate(S)), dev(np.concatenate(Cg)), inject_actions=dev(np.concatenate(Ac)),
                                  counts_per_tree=counts)
        off = np.concatenate([[0], np.cumsum(counts)])
        for t in range(T):
            if counts[t]:
                last_lo[t] = off[t]
            compare_tree(forest, t, singles[t], (off[t], off[t + 1]) if counts[t] else (0, 0), last_lo[t])
            drawn[t] += counts[t]
            done[t] = done[t] or int(cnt[t, CNT_GOAL]) >= 0
    return singles, np.concatenate(statuses), diverged


@pytest.mark.parametrize("early_exit", [False, True])
def test_tape_scene_forest_rounds_equal_single_tree_rounds(ctx, early_exit):
    """Four trees on three mazes (two trees on boxes with different starts and goals), three rounds of uneven counts (incl. 0
    and 1): every tree bit-identical to its own engine on its own scene -- through a goal and collisions -- and a kernel that
    read scene 0's maze and goal for every row would not be."""
    from ditreeonlineplanner_amd import _lib
    from ditreeonlineplanner_amd.engine import CNT_GOAL, ExpansionEngine
    from ditreeonlineplanner_amd.forest import SceneForestEngine
    scene_of = [0, 1, 2, 3]
    forest = SceneForestEngine(ctx, [scene(k) for k in range(len(SCENES))], 4, 24, edge_length=H, batch=64, early_exit=early_exit)
    for t, k in enumerate(scene_of):
        forest.reset_tree(t, k)
    m0, _, g0 = scene(0)
    wrong = [ExpansionEngine(ctx, m0, scene(k)[1], g0, edge_length=H, batch=64, capacity=24, early_exit=early_exit)
             for k in scene_of]
    singles, st, diverged = run_tape_rounds(ctx, forest, scene_of, early_exit, wrong=wrong)
    assert (st == _lib.ST_COLLIDED).any() and (st == _lib.ST_GOAL).any()
    assert forest.goal_node(0) is not None and diverged
    # path and fallback per tree, each against its own scene's goal
    fb = forest.fallback_nodes()
    for t in range(forest.T):
        g = forest.goal_node(t)
        node = g if g is not None else fb[t]
        ref = singles[t].goal_node if singles[t].goal_node is not None else singles[t].fallback_node()
        assert node == ref, t
        if node is not None:
            p, a = forest.path_to(t, node)
            rp, ra = singles[t].path_to(ref)
            assert np.array_equal(p, rp) and np.array_equal(a, ra)
    # slot reuse: tree 1 goes from narrow_short to random_huge and grows like a fresh engine of that scene
    forest.reset_tree(1, 2)
    assert forest.tree_scene(1) == 2 and forest.n_nodes_host[1] == 1
    fresh = ExpansionEngine(ctx, *scene(2), edge_length=H, batch=64, capacity=24, early_exit=early_exit)
    rt, at = ORRT.RandomTape(77), ActionTape(1077)
    maze, _, goal = scene(2)
    s, c, a = tape_rows(rt, at, 6, 0, maze, goal, forest.n_chunks)
    fresh.expand_round(dev(s), dev(c), inject_actions=dev(a))
    forest.expand_round(dev(s), dev(c), inject_actions=dev(a), counts_per_tree=[0, 6, 0, 0])
    compare_tree(forest, 1, fresh, (0, 6))
    assert int(forest.counters(1)[CNT_GOAL]) < 0 or forest.goal_node(1) is not None


@pytest.mark.parametrize("early_exit", [False, True])
def test_denoiser_scene_forest_rounds_equal_single_tree_rounds(net_ctx, early_exit):
    """Three trees on three mazes x 32 candidates x 2 rounds through the f16x3 network: each scene's local map feeds the
    network, and every tree is bit-identical to its own engine's rounds."""
    from ditreeonlineplanner_amd.engine import ExpansionEngine
    from ditreeonlineplanner_amd.forest import SceneForestEngine
    ctx = net_ctx
    scenes = [scene(3), scene(1), scene(2)]
    T, B, Cp = 3, 32, 128
    kw = dict(edge_length=64, early_exit=early_exit)
    forest = SceneForestEngine(ctx, scenes, T, Cp, batch=T * B, **kw)
    for t in range(T):
        forest.reset_tree(t, t)
    singles = [ExpansionEngine(ctx, *scenes[t], batch=B, capacity=Cp, **kw) for t in range(T)]
    rts = [ORRT.RandomTape(60 + t) for t in range(T)]
    gen = torch.Generator(device="cuda").manual_seed(11)
    for _ in range(2):
        S, Cg = zip(*[rts[t].draw_round(B, scenes[t][0].shape[1], scenes[t][0].shape[0], scenes[t][2]) for t in range(T)])
        noise = torch.randn((T * B, forest.n_chunks, forest.P, 2), generator=gen, device="cuda")
        for t in range(T):
            singles[t].expand_round(dev(S[t]), dev(Cg[t]), noise=noise[t * B:(t + 1) * B].contiguous())
        forest.expand_round(dev(np.concatenate(S)), dev(np.concatenate(Cg)), noise=noise, counts_per_tree=[B] * T)
        for t in range(T):
            compare_tree(forest, t, singles[t], (t * B, (t + 1) * B))


def test_scene_calls_refuse_bad_arguments_without_launching(ctx):
    """Scene id out of range, no scene table, too many scenes, an oversized atlas and a missing goals array give an error that
    names them; a scene forest needs no single maze, and its round is untouched by a refused call."""
    from ditreeonlineplanner_amd import _lib
    from ditreeonlineplanner_amd.forest import SceneForestEngine
    from ditreeonlineplanner_amd.ops import Context
    L = _lib.lib()
    ctx2 = Context(0)                                      # no single maze is ever uploaded to this ctx
    ctx2.upload_maze = lambda *a, **k: None
    try:
        h = ctx2._h
        forest = SceneForestEngine(ctx2, [scene(0), scene(1)], 2, 8, edge_length=H, batch=8)
        rb = forest.rb
        rb.node_id.fill_(-7)
        rd = rb.desc(0, 2)
        forest.off_dev.copy_(torch.tensor([0, 1, 2], dtype=torch.int32))
        for i, v in enumerate((0, 1, 2)):
            forest.off_host[i] = v
        rp = _lib.RoundParams()

        def expand(sdesc, handle=h):
            return L.ditree_forest_expand_round_scenes(handle, C.byref(forest.tree.desc), C.byref(forest.fdesc), C.byref(sdesc),
                                                       C.byref(rd), C.byref(rp), ctx2.stream)
        bad = _lib.ForestScenes(forest.tree_scene_dev.data_ptr(), (C.c_int32 * 2)(0, 2))
        assert expand(bad) == -1 and b"tree 1 has scene id 2, out of range [0, 2)" in L.ditree_last_error(h)
        assert expand(_lib.ForestScenes(None, None)) == -1 and b"scene descriptor incomplete" in L.ditree_last_error(h)
        ctx3 = Context(0)                                  # no scene table uploaded
        try:
            assert expand(forest.sdesc, ctx3._h) == -3 and b"no scene table uploaded" in L.ditree_last_error(ctx3._h)
        finally:
            ctx3.close()
        out = torch.empty(2, dtype=torch.int32, device="cuda")
        assert L.ditree_forest_fallback_goals(h, C.byref(forest.tree.desc), C.byref(forest.fdesc), None, out.data_ptr(),
                                              ctx2.stream) == -1
        assert b"goals array" in L.ditree_last_error(h)
        assert (rb.node_id == -7).all()
        m = load_maze("boxes")
        with pytest.raises(_lib.DitreeError, match="65 scenes"):
            ctx2.upload_scenes([m] * 65, np.zeros((65, 2)))
        with pytest.raises(_lib.DitreeError, match="16401 cells"):
            ctx2.upload_scenes([m] * 41 + [m[:1, :1]], np.zeros((42, 2)))
        with pytest.raises(ValueError, match="1..64 scenes"):
            SceneForestEngine(ctx2, [scene(0)] * 65, 2, 8, edge_length=H, batch=8)
        # the forest's own table back; a tape round and its accept run without a single maze and grow like their own engines
        forest.upload_scenes()
        forest.reset_tree(1, 1)
        from ditreeonlineplanner_amd.engine import ExpansionEngine
        singles = [ExpansionEngine(ctx, *scene(k), edge_length=H, batch=8, capacity=8) for k in (0, 1)]
        run_tape_rounds(ctx2, forest, [0, 1], False, counts_list=[[2, 3]], singles=singles)
    finally:
        ctx2.close()


# ---------------------------------------------------------------------- the facade
def _scenario_planner(sampler, k, **kw):
    from ditreeonlineplanner_amd.car_env import CarEnv
    from ditreeonlineplanner_amd.planners.RRT import RRT_Planner
    maze, start, goal = scene(k)
    env = CarEnv(maze_map=maze, collision_checking=False)
    args = dict(env_id="carmaze", environment=env, sampler=sampler, action_horizon=8, local_map_size=20, local_map_scale=0.2,
                global_map_scale=1.0, goal_conditioning_bias=0.85, prop_duration=[32], time_budget=600)
    args.update(kw)
    return RRT_Planner(start, goal, **args)


def check_scenario_runs_equal_sequential(planners, seeds, concurrent):
    from ditreeonlineplanner_amd.common import map_utils
    from ditreeonlineplanner_amd.planners.RRT import plan_scenario_runs
    seq = []
    for pl, ss in zip(planners, seeds):
        seq.append([])
        for s in ss:
            random.seed(s)
            np.random.seed(s)
            torch.manual_seed(s)
            map_utils.cc_calls = 0
            pl.reset()
            path, actions = pl.plan()
            seq[-1].append(dict(pl.results, path=path, actions=actions, cc_calls=map_utils.cc_calls,
                                goal=pl._engine.goal_node is not None))
    random.seed(123)
    np.random.seed(456)
    torch.manual_seed(789)
    before = _rng_states()
    map_utils.cc_calls = 0
    runs = plan_scenario_runs(planners, seeds, concurrent=concurrent)
    assert _same_states(before, _rng_states())
    assert map_utils.cc_calls == sum(r["cc_calls"] for q in seq for r in q)
    for rs, qs, ss in zip(runs, seq, seeds):
        assert [r["seed"] for r in rs] == list(ss)
        for r, q in zip(rs, qs):
            for k in ("iterations", "number_of_nodes", "cc_calls"):
                assert r[k] == q[k], (r["seed"], k, r[k], q[k])
            assert r["success"] == (q["path"] is not None) and r["goal_reached"] == q["goal"]
            for k in ("path", "actions"):
                assert (r[k] is None) == (q[k] is None) and (r[k] is None or np.array_equal(r[k], q[k])), (r["seed"], k)
            if q["path"] is not None:
                assert r["path_time"] == q["path_time"]
    return runs


def test_plan_scenario_runs_equals_sequential_seeded_plans_network(car_net):
    sampler = _sampler(car_net)
    planners = [_scenario_planner(sampler, k, batch=16, max_candidates=48) for k in (3, 1, 2)]
    runs = check_scenario_runs_equal_sequential(planners, [[1, 2], [3, 4, 5], [6, 7]], concurrent=3)
    assert all(r["iterations"] > 0 for rs in runs for r in rs)


def test_plan_scenario_runs_equals_sequential_seeded_plans_tape():
    class Tape:
        def __init__(self):
            self.tape = ActionTape(5)

        def sample_round(self, first, B, n_chunks, P):
            return np.stack([self.tape.actions(np.arange(first, first + B), j) for j in range(n_chunks)], axis=1)
    sampler = Tape()
    planners = [_scenario_planner(sampler, k, batch=8, max_candidates=40) for k in (0, 1, 2)]
    runs = check_scenario_runs_equal_sequential(planners, [[11, 12], [13, 14], [15]], concurrent=2)
    assert any(r["goal_reached"] for r in runs[0])


def test_plan_scenario_runs_of_one_planner_equals_its_plan_runs():
    """The shared run loop on both engine kinds: ``plan_scenario_runs([pl], [seeds])`` (a SceneForestEngine) equals
    ``pl.plan_runs(seeds)`` (a ForestEngine) run for run -- both are tied to sequential ``plan()`` by the tests above and in
    test_gpu_forest."""
    from ditreeonlineplanner_amd.planners.RRT import plan_scenario_runs

    class Tape:
        def __init__(self):
            self.tape = ActionTape(5)

        def sample_round(self, first, B, n_chunks, P):
            return np.stack([self.tape.actions(np.arange(first, first + B), j) for j in range(n_chunks)], axis=1)
    pl = _scenario_planner(Tape(), 0, batch=8, max_candidates=40)
    seeds = [11, 12, 13, 14]
    want = pl.plan_runs(seeds, concurrent=2)
    (got,) = plan_scenario_runs([pl], [seeds], concurrent=2)
    assert [r["seed"] for r in got] == seeds == [r["seed"] for r in want]
    for r, q in zip(got, want):
        for k in ("iterations", "number_of_nodes", "cc_calls", "success", "goal_reached"):
            assert r[k] == q[k], (r["seed"], k, r[k], q[k])
        for k in ("path", "actions"):
            assert (r[k] is None) == (q[k] is None) and (r[k] is None or np.array_equal(r[k], q[k])), (r["seed"], k)
    assert all(r["iterations"] > 0 for r in got) and any(r["goal_reached"] for r in got)
