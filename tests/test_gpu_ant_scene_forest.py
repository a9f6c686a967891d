"""GPU: an ant scene forest (forest.AntSceneForestEngine, include/ditree.h "ant scene forests") grows every tree exactly as its
own AntExpansionEngine does on its own scene's maze, start, goal and desired goal -- bit for bit, node histories included -- on
tape and on model dynamics and with the ant denoiser in the loop; its calls refuse bad arguments before anything is launched;
and plan_ant_scenario_runs equals sequential seeded plan() calls of every scenario, run by run."""
import ctypes as C
import os
import random

import numpy as np
import pytest
import torch

from oracle import ant as OA
from oracle import geometry as G
from oracle import rrt as ORRT
from tests.test_gpu_ant_facade import AntEnv, TapeSampler
from tests.test_gpu_ant_forest import _sampler, ant_net_ctx, ant_policy_net, compare_ant_tree  # noqa: F401
from tests.test_gpu_ant_round import ant_norm
from tests.test_gpu_forest import _rng_states, _same_states, ctx, dev  # noqa: F401
from tests.util import REPO

pytestmark = pytest.mark.gpu

ANT_CSV = os.path.join(REPO, "tests", "golden", "test_scenarios_ant.csv")
# Four scenes of the reference's ant scenario set on three mazes of different dims -- boxes 20 x 20, narrow_short 6 x 11,
# random_large 9 x 12; `boxes` and `boxes3` share a maze but neither start nor goal.  Five trees; trees 0 and 4 share scene 0.
SCENE_NAMES = ["boxes", "narrow", "random large2", "boxes3"]
SCENE_OF = [0, 1, 2, 3, 0]
# Per tree: its own RandomTape (samples), action tape and observation tape (candidate k of tree t is a pure function of
# (SEEDS[t], k)); GOAL_EVERY[t] bends every such candidate of the tree's observation tape towards its scene's desired goal (0:
# none).  The streams, COUNTS, CAP and the desired goals were chosen with the CPU oracle (oracle/ant.py) so that the four rounds
# hold, on both dynamics: a goal that retires a tree, rounds of 1 and 0 candidates, a tree that runs past its CAP node slots, and
# in every round a candidate whose outcome under another tree's scene differs from its own (computed and asserted below).
SEEDS = [154, 32, 23, 205, 200]
GOAL_EVERY = [7, 0, 5, 0, 11]
COUNTS = [[6, 3, 4, 12, 3], [6, 0, 6, 12, 5], [6, 1, 0, 12, 2], [6, 2, 5, 12, 7]]
CAP = 24
TAPE_DESIRED_NOISE = [(0.2, -0.15), (-0.1, 0.2), (0.15, 0.1), (-0.2, -0.1)]      # what a gym env adds to the goal cell's centre
MODEL_DESIRED_OFFSET = [(5.0, 4.0), (4.0, -3.0), (3.0, -5.0), (-4.0, 5.0)]     # model dynamics: this far from the start


def ant_scene(k, dynamics):
    """-> (maze, start (29,), goal (29,), desired_goal (2,)) of scene k."""
    from ditreeonlineplanner_amd.scenarios import ant_scenarios
    sc = {s["name"]: s for s in ant_scenarios(ANT_CSV)}[SCENE_NAMES[k]]
    if dynamics == "tape":
        desired = sc["goal"][:2] + np.array(TAPE_DESIRED_NOISE[k])
    else:
        desired = sc["start"][:2] + np.array(MODEL_DESIRED_OFFSET[k])
    return np.asarray(sc["maze"], dtype=np.float32), sc["start"], sc["goal"], desired


class SceneStreams:
    """The rows one tree feeds its engine on its scene (tests.test_gpu_ant_forest.TreeStreams with the scene as an argument)."""

    def __init__(self, seed, goal_every, maze, goal, desired):
        self.rt = ORRT.RandomTape(seed)
        self.at = OA.AntActionTape(seed + 1000, 16)
        self.ot = OA.AntObsTape(seed + 2000, maze, 4.0, 24, 2, desired_xy=desired, goal_every=goal_every, step=0.12)
        self.maze, self.goal, self.drawn = maze, goal, 0

    def rows(self, n):
        H, W = self.maze.shape
        s, c = np.zeros((n, 29)), np.zeros((n, 2))
        for i in range(n):
            s[i], c[i] = OA.draw_candidate_ant(self.rt, W, H, 4.0, self.goal)
        cand = np.arange(self.drawn, self.drawn + n)
        acts = np.stack([self.at.actions(cand, j) for j in range(24)], axis=1)
        self.drawn += n
        return s, c, acts, self.ot.rows(cand)


def first_chunk(state, acts, obs, scene, dynamics):
    """oracle.ant.ant_rollout_chunk of chunk 0 from ``state`` on ``scene``'s maze and desired goal -> (status, n_steps)."""
    if dynamics == "tape":
        step = lambda i, cur, act, rows: obs[rows, 0, i]                      # noqa: E731
    else:
        step = lambda i, cur, act, rows: OA.ant_model_step(cur, act)          # noqa: E731
    r = OA.ant_rollout_chunk(state, acts[:, 0], step, scene[0], scene[3], 4.0, A=2)
    return r["status"], r["n_steps"]


def other_scene_outcomes_differ(single, n, rows, own, scenes, dynamics):
    """Tree rows of one round: chunk 0 from the parents the engine chose, by the CPU oracle on the tree's own scene (must be
    what the device ran) and on every other scene -> True when another scene gives some row another status or step count."""
    _, _, a, o = rows
    parent = single.rb.parent[:n].cpu().numpy()
    state = single.tree.state.cpu().numpy()[parent]
    st, ns = first_chunk(state, a, o, scenes[own], dynamics)
    assert np.array_equal(single.rb.chunk_steps[:n, 0].cpu().numpy(), ns)
    differs = False
    for k, sc in enumerate(scenes):
        if k != own:
            st2, ns2 = first_chunk(state, a, o, sc, dynamics)
            differs |= bool((st2 != st).any() or (ns2 != ns).any())
    return differs


@pytest.mark.parametrize("dynamics", ["tape", "model"])
def test_ant_scene_forest_rounds_equal_single_tree_rounds(ctx, dynamics):
    """Five trees on four scenes (three mazes of different dims; two trees share a scene, two scenes share a maze), four rounds
    of uneven per-tree counts (incl. 0 and 1) on injected actions: every tree bit-identical to its own AntExpansionEngine on
    its scene -- through a goal that retires a tree and a full tree -- and in every round a kernel that read another tree's
    scene would have computed something else."""
    from ditreeonlineplanner_amd.engine import CNT_GOAL, CNT_OVERFLOW, CNT_PHANTOM, CNT_STICKY, AntExpansionEngine
    from ditreeonlineplanner_amd.forest import AntSceneForestEngine
    scenes = [ant_scene(k, dynamics) for k in range(len(SCENE_NAMES))]
    assert len({sc[0].shape for sc in scenes}) == 3 and np.array_equal(scenes[0][0], scenes[3][0])
    assert not np.array_equal(scenes[0][1], scenes[3][1]) and not np.array_equal(scenes[0][2], scenes[3][2])
    T = len(SEEDS)
    kw = dict(norm=ant_norm(), dynamics=dynamics)
    forest = AntSceneForestEngine(ctx, scenes, T, CAP, batch=64, **kw)
    for t, k in enumerate(SCENE_OF):
        forest.reset_tree(t, k)
    assert [forest.tree_scene(t) for t in range(T)] == SCENE_OF

    def single_of(k):
        maze, start, goal, desired = scenes[k]
        return AntExpansionEngine(ctx, maze, start, goal, desired_goal=desired, batch=64, capacity=CAP, **kw)
    singles = [single_of(k) for k in SCENE_OF]
    streams = [SceneStreams(SEEDS[t], GOAL_EVERY[t], scenes[k][0], scenes[k][2], scenes[k][3]) for t, k in enumerate(SCENE_OF)]
    done = [False] * T
    for counts in COUNTS:
        counts = [0 if done[t] else c for t, c in enumerate(counts)]
        rows = [streams[t].rows(counts[t]) if counts[t] else None for t in range(T)]
        differs = False
        for t in range(T):
            if counts[t]:
                s, c, a, o = rows[t]
                singles[t].expand_round(dev(s), dev(c), inject_actions=dev(a), next_obs_tape=dev(o) if dynamics == "tape" else None)
                differs |= other_scene_outcomes_differ(singles[t], counts[t], rows[t], SCENE_OF[t], scenes, dynamics)
        assert differs, "no candidate of this round tells its own scene from another tree's"
        S, Cg, Ac, Ob = (np.concatenate([r[i] for r in rows if r is not None]) for i in range(4))
        cnt = forest.expand_round(dev(S), dev(Cg), inject_actions=dev(Ac), counts_per_tree=counts,
                                  next_obs_tape=dev(Ob) if dynamics == "tape" else None)
        off = np.concatenate([[0], np.cumsum(counts)])
        for t in range(T):
            compare_ant_tree(forest, t, singles[t], (off[t], off[t + 1]) if counts[t] else (0, 0))
            done[t] = done[t] or int(cnt[t, CNT_GOAL]) >= 0
    cnt = np.stack([forest.counters(t) for t in range(T)])
    assert (cnt[:, CNT_STICKY] == 0).all() and (cnt[:, CNT_PHANTOM] == -1).all()
    retired = [t for t in range(T) if done[t] and streams[t].drawn < sum(c[t] for c in COUNTS)]
    assert retired, "no tree was retired by a goal"
    full = [t for t in range(T) if cnt[t, CNT_OVERFLOW] == 1]
    assert full and all(forest.n_nodes_host[t] == CAP for t in full), "no tree ran past its node slots"
    # path and fallback per tree, each against its own scene's goal_state
    fb = forest.fallback_nodes()
    assert fb == [s.fallback_node() for s in singles]
    for t in range(T):
        g = forest.goal_node(t)
        assert g == singles[t].goal_node
        node = g if g is not None else fb[t]
        if node is not None:
            p, a = forest.path_to(t, node)
            rp, ra = singles[t].path_to(node)
            assert np.array_equal(p, rp) and np.array_equal(a, ra) and p.shape[1] == 29 and a.shape[1] == 8
    # slot reuse across scenes: a retired tree goes to another scene -- root state and history rows from that scene's start --
    # and grows like a fresh engine of that scene; the other trees are untouched
    t = retired[0]
    k2 = (SCENE_OF[t] + 1) % len(scenes)
    others = [k for k in range(T * CAP) if k // CAP != t]
    names = ("state", "hist", "hist_n", "parent", "last_action", "has_prev", "edge_nstates")
    before = {nm: getattr(forest.tree, nm)[others].clone() for nm in names}
    forest.reset_tree(t, k2)
    r = t * CAP
    assert forest.tree_scene(t) == k2 and forest.n_nodes_host[t] == 1 and forest.goal_node(t) is None
    assert np.array_equal(forest.tree.hist[r].cpu().numpy(), np.stack([np.zeros(29), np.zeros(29), scenes[k2][1]]))
    assert int(forest.tree.hist_n[r]) == 1 and np.array_equal(forest.tree.state[r].cpu().numpy(), scenes[k2][1])
    for nm in names:
        assert torch.equal(getattr(forest.tree, nm)[others], before[nm]), nm
    fresh = single_of(k2)
    st = SceneStreams(77, 3, scenes[k2][0], scenes[k2][2], scenes[k2][3])
    s, c, a, o = st.rows(5)
    tape = dict(next_obs_tape=dev(o)) if dynamics == "tape" else {}
    fresh.expand_round(dev(s), dev(c), inject_actions=dev(a), **tape)
    forest.expand_round(dev(s), dev(c), inject_actions=dev(a), counts_per_tree=[5 if i == t else 0 for i in range(T)], **tape)
    compare_ant_tree(forest, t, fresh, (0, 5))


# ---------------------------------------------------------------------- the denoiser in the loop
@pytest.mark.parametrize("early_exit", [False, True])
def test_ant_denoiser_scene_forest_rounds_equal_single_tree_rounds(ant_net_ctx, early_exit):
    """Three trees on three mazes x 32 candidates x 2 rounds through the ant network in f16x3 on model dynamics: each scene's
    local map (cut with its own dims) feeds the network, the early-exit rounds are pool-scheduled launches on index lists, and
    every tree is bit-identical to its own engine's rounds of 32."""
    from ditreeonlineplanner_amd.engine import AntExpansionEngine
    from ditreeonlineplanner_amd.forest import AntSceneForestEngine
    ctx = ant_net_ctx
    scenes = [ant_scene(k, "model") for k in (3, 1, 2)]
    T, B, Cp = 3, 32, 80
    kw = dict(norm=ant_norm(), dynamics="model", early_exit=early_exit)
    forest = AntSceneForestEngine(ctx, scenes, T, Cp, batch=T * B, **kw)
    for t in range(T):
        forest.reset_tree(t, t)
    singles = [AntExpansionEngine(ctx, sc[0], sc[1], sc[2], desired_goal=sc[3], batch=B, capacity=Cp, **kw) for sc in scenes]
    rts = [ORRT.RandomTape(40 + t) for t in range(T)]
    gen = torch.Generator(device="cuda").manual_seed(9)
    for _ in range(2):
        S, Cg = np.zeros((T, B, 29)), np.zeros((T, B, 2))
        for t in range(T):
            H, W = scenes[t][0].shape
            for i in range(B):
                S[t, i], Cg[t, i] = OA.draw_candidate_ant(rts[t], W, H, 4.0, scenes[t][2])
        noise = torch.randn((T * B, forest.n_chunks, forest.P, 8), generator=gen, device="cuda")
        for t in range(T):
            singles[t].expand_round(dev(S[t]), dev(Cg[t]), noise=noise[t * B:(t + 1) * B].contiguous())
        forest.expand_round(dev(S.reshape(T * B, 29)), dev(Cg.reshape(T * B, 2)), noise=noise, counts_per_tree=[B] * T)
        for t in range(T):
            compare_ant_tree(forest, t, singles[t], (t * B, (t + 1) * B))
    assert all(int(n) > 1 for n in forest.n_nodes_host)


# ---------------------------------------------------------------------- refusals
def test_ant_scene_calls_refuse_bad_arguments_without_launching(ctx):
    """No scene table, a scene id out of range, a NULL descriptor part, a car tree, a sharded round and dynamics that is
    neither tape nor model: DITREE_E_STATE / DITREE_E_ARG with a message, the round buffers and the output untouched; the car's
    per-tree-goal fallback keeps refusing an ant tree; and an ant scene forest needs no single maze."""
    from ditreeonlineplanner_amd import _lib
    from ditreeonlineplanner_amd.engine import AntExpansionEngine, ExpansionEngine
    from ditreeonlineplanner_amd.forest import AntSceneForestEngine
    from ditreeonlineplanner_amd.ops import Context, _dbl
    from tests.test_gpu_forest import scenario
    L = _lib.lib()
    scenes = [ant_scene(0, "tape"), ant_scene(1, "tape")]
    ctx2 = Context(0)                                      # no single maze is ever uploaded to this ctx
    ctx2.upload_maze = lambda *a, **k: None
    try:
        h = ctx2._h
        forest = AntSceneForestEngine(ctx2, scenes, 2, 8, batch=8, norm=ant_norm(), dynamics="tape")
        rb = forest.rb
        B = 2
        for name in ("node_id", "parent", "status", "chunks_run"):
            getattr(rb, name).fill_(-7)
        rb.end_state.fill_(-7.0)
        rd = rb.desc(0, B)
        forest._set_offsets([1, 1])
        samples, cg = dev(np.zeros((B, 29))), dev(np.zeros((B, 2)))
        acts, tape = dev(np.zeros((B, 24, forest.P, 8))), dev(np.zeros((B, 24, 2, 29)))
        rp, keep = forest._params(samples, cg, None, acts, 0, B, tape, None, None)
        out = torch.full((2,), -9, dtype=torch.int32, device="cuda")
        ga, gp = _dbl(np.array([[1.0, 2.0], [3.0, 4.0]]))
        tree, fd = forest.tree.desc, forest.fdesc

        def expand(tree=tree, fd=fd, sdesc=forest.sdesc, rd=rd, rp=rp, handle=h):
            rc = L.ditree_forest_expand_round_ant_scenes(handle, C.byref(tree), C.byref(fd), C.byref(sdesc), C.byref(rd), C.byref(rp),
                                                         ctx2.stream)
            return rc, L.ditree_last_error(handle)

        def fallback(tree=tree, fd=fd, goals=gp, o=out.data_ptr()):
            return L.ditree_forest_fallback_goals_ant(h, C.byref(tree), C.byref(fd), goals, o, ctx2.stream), L.ditree_last_error(h)
        ctx3 = Context(0)                                  # no scene table uploaded
        try:
            rc, err = expand(handle=ctx3._h)
            assert rc == -3 and b"forest_expand_round_ant_scenes: no scene table uploaded" in err
        finally:
            ctx3.close()
        rc, err = expand(sdesc=_lib.ForestScenes(forest.tree_scene_dev.data_ptr(), (C.c_int32 * 2)(0, 2)))
        assert rc == -1 and b"forest_expand_round_ant_scenes: tree 1 has scene id 2, out of range [0, 2)" in err
        rc, err = expand(sdesc=_lib.ForestScenes(forest.tree_scene_dev.data_ptr(), None))
        assert rc == -1 and b"scene descriptor incomplete" in err
        rc, err = expand(sdesc=_lib.ForestScenes(None, forest.tree_scene_host))
        assert rc == -1 and b"scene descriptor incomplete" in err
        rc, err = expand(fd=_lib.Forest(2, 8, None, forest.off_dev.data_ptr(), forest.off_host))
        assert rc == -1 and b"forest descriptor incomplete" in err
        rc, err = expand(fd=_lib.Forest(2, 8, forest.fcounters.data_ptr(), forest.off_dev.data_ptr(), None))
        assert rc == -1 and b"forest offsets" in err
        maze, start, goal = scenario()
        car = ExpansionEngine(ctx, maze, start, goal, edge_length=8, batch=8, capacity=16)
        for call in (expand, fallback):
            rc, err = call(tree=car.tree.desc)
            assert rc == -1 and b"an ant forest is an ant tree" in err
        sharded = rb.desc(0, B, shard=1)
        rc, err = expand(rd=sharded)
        assert rc == -1 and b"no shards" in err
        rp.dynamics = 7
        rc, err = expand()
        assert rc == -1 and b"dynamics must be DITREE_ANT_DYN_TAPE or DITREE_ANT_DYN_MODEL" in err
        rp.dynamics = _lib.ANT_DYN_TAPE
        rp.next_obs_tape = None
        rc, err = expand()
        assert rc == -1 and b"without next_obs_tape" in err
        rp.next_obs_tape = tape.data_ptr()
        rc, err = fallback(goals=None)
        assert rc == -1 and b"forest_fallback_goals_ant: goals array" in err
        rc, err = fallback(o=None)
        assert rc == -1 and b"forest_fallback_goals_ant: out_node missing" in err
        # the car's per-tree-goal fallback still takes a car tree only
        assert L.ditree_forest_fallback_goals(h, C.byref(tree), C.byref(fd), gp, out.data_ptr(), ctx2.stream) == -1
        assert b"car tree" in L.ditree_last_error(h)
        torch.cuda.synchronize()
        for name in ("node_id", "parent", "status", "chunks_run"):
            assert (getattr(rb, name) == -7).all(), name
        assert (rb.end_state == -7.0).all() and (out == -9).all()
        del keep, ga
        # a tape round and its accept run without a single maze (and without p->desired_goal) and grow like their own engines
        forest.reset_tree(1, 1)
        singles = [AntExpansionEngine(ctx, sc[0], sc[1], sc[2], desired_goal=sc[3], batch=8, capacity=8, norm=ant_norm(), dynamics="tape")
                   for sc in scenes]
        streams = [SceneStreams(300 + t, 3, scenes[t][0], scenes[t][2], scenes[t][3]) for t in range(2)]
        rows = [streams[0].rows(2), streams[1].rows(3)]
        for t in range(2):
            s, c, a, o = rows[t]
            singles[t].expand_round(dev(s), dev(c), inject_actions=dev(a), next_obs_tape=dev(o))
        S, Cg, Ac, Ob = (np.concatenate([r[i] for r in rows]) for i in range(4))
        forest.expand_round(dev(S), dev(Cg), inject_actions=dev(Ac), counts_per_tree=[2, 3], next_obs_tape=dev(Ob))
        compare_ant_tree(forest, 0, singles[0], (0, 2))
        compare_ant_tree(forest, 1, singles[1], (2, 5))
    finally:
        ctx2.close()


# ---------------------------------------------------------------------- the facade
# (maze, start, desired goal offset from the start) of the two scenarios: the stand-in crawler is slow, so the desired goal sits
# close to the start
PLAN_SCENES = [(0, (4.0, 8.0)), (2, (3.0, -5.0))]


def _scenario_planner(sampler, k, ant_dynamics, **kw):
    from ditreeonlineplanner_amd.planners.RRT import RRT_Planner
    scene, offset = PLAN_SCENES[k]
    maze, start, goal, _ = ant_scene(scene, "model")
    desired = start[:2] + np.array(offset)
    env = AntEnv(maze, 4.0, desired)
    if ant_dynamics == "tape":
        ot = OA.AntObsTape(77 + k, maze, 4.0, 24, 2, desired_xy=desired, goal_every=29, step=0.12)
        kw["next_obs_tape_fn"] = lambda first, B: ot.rows(np.arange(first, first + B))
    return RRT_Planner(start, goal, env_id="antmaze", environment=env, sampler=sampler, prediction_type="actions", action_horizon=2,
                       local_map_size=16, local_map_scale=0.8, global_map_scale=4.0, goal_conditioning_bias=0.85, prop_duration=[48],
                       time_budget=1e9, max_iter=300, verbose=False, capacity=1024, ant_dynamics=ant_dynamics, **kw)


def check_ant_scenario_runs_equal_sequential(planners, seeds, concurrent):
    from ditreeonlineplanner_amd.common import map_utils
    from ditreeonlineplanner_amd.planners.RRT import plan_ant_scenario_runs
    seq = []
    for pl, ss in zip(planners, seeds):
        seq.append([])
        for s in ss:
            random.seed(s)
            np.random.seed(s)
            torch.manual_seed(s)
            pl.reset()
            path, actions = pl.plan()
            seq[-1].append(dict(pl.results, path=path, actions=actions, goal=pl._engine.goal_node is not None))
    random.seed(123)
    np.random.seed(456)
    torch.manual_seed(789)
    before = _rng_states()
    map_utils.cc_calls = 0
    runs = plan_ant_scenario_runs(planners, seeds, concurrent=concurrent)
    assert _same_states(before, _rng_states())
    assert map_utils.cc_calls == 0                          # is_colliding_ant does not count its calls
    for rs, qs, ss in zip(runs, seq, seeds):
        assert [r["seed"] for r in rs] == list(ss)
        for r, q in zip(rs, qs):
            for k in ("iterations", "number_of_nodes"):
                assert r[k] == q[k], (r["seed"], k, r[k], q[k])
            assert r["cc_calls"] == 0
            assert r["success"] == (q["path"] is not None) and r["goal_reached"] == q["goal"]
            for k in ("path", "actions"):
                assert (r[k] is None) == (q[k] is None) and (r[k] is None or np.array_equal(r[k], q[k])), (r["seed"], k)
            if q["path"] is not None:
                assert r["path_time"] == q["path_time"] and r["path"].shape[1] == 29 and r["actions"].shape[1] == 8
    return runs


def _tape_sampler():
    return TapeSampler(OA.AntActionTape(31, 16))


@pytest.mark.parametrize("ant_dynamics", ["model", "tape"])
def test_plan_ant_scenario_runs_equals_sequential_seeded_plans_action_tape(ant_dynamics):
    """Two scenarios x two seeds on two trees (a freed tree takes a run of the other scenario): the action tape at batch 8 and
    40 candidates, on model and on tape dynamics."""
    sampler = _tape_sampler()
    planners = [_scenario_planner(sampler, k, ant_dynamics, batch=8, max_candidates=40) for k in range(2)]
    runs = check_ant_scenario_runs_equal_sequential(planners, [[1, 2], [3, 10]], concurrent=2)
    assert all(r["iterations"] > 0 and r["success"] for rs in runs for r in rs)


def test_plan_ant_scenario_runs_equals_sequential_seeded_plans_network(ant_policy_net):
    """The network sampler + model dynamics at batch 16 and 32 candidates: each run's start noise from its own generator."""
    sampler = _sampler(ant_policy_net)
    planners = [_scenario_planner(sampler, k, "model", batch=16, max_candidates=32) for k in range(2)]
    runs = check_ant_scenario_runs_equal_sequential(planners, [[21, 22], [23, 24]], concurrent=2)
    assert all(r["iterations"] > 0 for rs in runs for r in rs)


def test_plan_ant_scenario_runs_of_one_planner_equals_its_plan_runs():
    """The shared run loop on both ant engine kinds: ``plan_ant_scenario_runs([pl], [seeds])`` (an AntSceneForestEngine) equals
    ``pl.plan_runs(seeds)`` (an AntForestEngine) run for run."""
    from ditreeonlineplanner_amd.planners.RRT import plan_ant_scenario_runs
    pl = _scenario_planner(_tape_sampler(), 0, "model", batch=8, max_candidates=40)
    seeds = [1, 2, 3, 10]
    want = pl.plan_runs(seeds, concurrent=2)
    (got,) = plan_ant_scenario_runs([pl], [seeds], concurrent=2)
    assert [r["seed"] for r in got] == seeds == [r["seed"] for r in want]
    for r, q in zip(got, want):
        for k in ("iterations", "number_of_nodes", "cc_calls", "success", "goal_reached"):
            assert r[k] == q[k], (r["seed"], k, r[k], q[k])
        for k in ("path", "actions"):
            assert (r[k] is None) == (q[k] is None) and (r[k] is None or np.array_equal(r[k], q[k])), (r["seed"], k)
    assert all(r["iterations"] > 0 for r in got)
