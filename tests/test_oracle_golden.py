"""CPU: the oracle restatement against the golden vectors captured from the reference."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import geometry as G
from oracle import rrt as ORRT
from oracle import sampler as OS
from oracle.tapes import ActionTape
from tests.util import load_maze, golden


def test_collision_matches_reference():
    g = golden("geometry")
    for name in ("Race_Track", "boxes", "random_huge", "narrow_short"):
        got = G.is_colliding_car(g[f"collision_{name}_poses"], load_maze(name))
        assert np.array_equal(got, g[f"collision_{name}_expected"]), name


def test_local_map_matches_reference():
    g = golden("geometry")
    for name in ("Race_Track", "boxes", "random_huge"):
        maze = load_maze(name).astype(np.float32)
        H, W = maze.shape
        for tag, (n, scale, sg) in {"car": (20, 0.2, 1.0), "ant": (16, 0.8, 4.0)}.items():
            poses = g[f"localmap_{name}_{tag}_poses"]
            th = poses[:, 2] if tag == "car" else np.zeros(len(poses))
            got = G.create_local_map(maze, poses[:, 0] * sg, poses[:, 1] * sg, th, n, scale, sg,
                                     (W / 2 * sg, H / 2 * sg))
            exp = np.unpackbits(g[f"localmap_{name}_{tag}_expected"])[: got.size].reshape(got.shape)
            assert np.array_equal(got.astype(np.uint8), exp), (name, tag)


def test_lidar_matches_reference():
    g = golden("geometry")
    maze = load_maze("boxes")
    poses = g["lidar_boxes_poses"]
    vis_all = np.unpackbits(g["lidar_boxes_visited"])[: len(poses) * maze.size].reshape(len(poses), *maze.shape)
    for i in range(0, len(poses), 4):
        d, e, v, h = G.lidar_scan(poses[i], maze)
        assert np.array_equal(d, g["lidar_boxes_dist"][i])
        assert np.array_equal(e, g["lidar_boxes_end"][i])
        vis = np.zeros(maze.shape, dtype=np.uint8)
        vis[v[:, 1], v[:, 0]] = 1
        assert np.array_equal(vis, vis_all[i])


def test_lidar_on_every_bundled_maze_fails_where_the_reference_fails():
    """tests/golden/lidar_nonsquare.json (make_lidar_nonsquare.py): what the reference's Lidar2DSim did at 8 free poses of
    every bundled car maze, "ok" or the exception type it raised.  The oracle's default extents fail in the same way at the
    same poses (on every non-square maze, never on a square one); extents="map" scans every pose, every ray ends on a wall
    and every visited cell lies inside the map."""
    with open(os.path.join(os.path.dirname(__file__), "golden", "lidar_nonsquare.json")) as f:
        rec = json.load(f)["mazes"]
    assert {"Race_Track", "narrow_short", "random_large", "shapes", "boxes"} <= set(rec)
    raised = set()
    for name, r in rec.items():
        maze = load_maze(name)
        assert list(maze.shape) == r["shape"] and len(r["poses"]) == len(r["result"]) == 8
        square = maze.shape[0] == maze.shape[1]
        for pose, exp in zip(r["poses"], r["result"]):
            assert maze[int(pose[1]), int(pose[0])] == 0
            try:
                G.lidar_scan(pose, maze)
                got = "ok"
            except Exception as e:                                   # noqa: BLE001 -- the type is what is compared
                got = type(e).__name__
            assert got == exp, (name, pose, got, exp)
            assert (exp == "ok") == square, (name, pose, exp)
            raised.add(exp)
            d, e, v, h = G.lidar_scan(pose, maze, extents="map")
            assert h.all() and (d > 0).all(), (name, pose)
            assert (v[:, 0] >= 0).all() and (v[:, 0] < maze.shape[1]).all(), (name, pose)
            assert (v[:, 1] >= 0).all() and (v[:, 1] < maze.shape[0]).all(), (name, pose)
            if square:
                d0, e0, v0, h0 = G.lidar_scan(pose, maze)
                assert np.array_equal(d, d0) and np.array_equal(e, e0) and np.array_equal(v, v0) and np.array_equal(h, h0)
    assert raised == {"ok", "IndexError", "TypeError"}


def test_kdtree_matches_scipy():
    g = golden("geometry")
    for n in (1, 17, 1000):
        assert np.array_equal(G.nn_argmin(g[f"kdtree_{n}_queries"], g[f"kdtree_{n}_nodes"]), g[f"kdtree_{n}_expected"])


def test_dynamics_known_answers():
    g = golden("geometry")
    cur = g["dyn_s0"].copy()
    for i in range(64):
        cur = G.car_step(cur, g["dyn_actions"][:, i])
        assert np.abs(cur - g["dyn_traj_expected"][:, i + 1]).max() < 1e-9
    # closed forms (car_env.py:376-390): v = 0 -> pose frozen, D/delta integrate the clipped action
    s = np.array([1.0, 2.0, 0.3, 0.0, 0.0, 0.0])
    n = G.car_step(s, np.array([25.0, -7.0]))
    assert np.array_equal(n[:4], s[:4]) and n[4] == 10.0 / 50.0 and n[5] == -2.0 / 50.0
    # delta = 0: straight line along psi
    s = np.array([0.0, 0.0, np.pi / 2, 2.0, 0.0, 0.0])
    n = G.car_step(s, np.zeros(2))
    assert abs(n[0]) < 1e-15 and abs(n[1] - 0.04) < 1e-15 and n[2] == s[2]


def test_dynamics_from_reference_source_text():
    """Vectors produced by CarEnv.step / _update_state / _check_done taken from the TEXT of the reference's car_env.py
    (ast, tests/golden/make_golden.py::gen_dynamics_from_text; MX.tanh bound to math.tanh): expression order, action
    clipping, the goal radius and the frozen-after-success rule -- bit for bit."""
    g = golden("geometry")
    S0, A, goals = g["dyntext_s0"], g["dyntext_actions"], g["dyntext_goals"]
    for b in range(len(S0)):
        cur, done = S0[b].copy(), False
        for i in range(A.shape[1]):
            if not done:
                cur = G.car_step(cur[None], A[b, i][None])[0]
                done = bool(G.goal_reached(cur, goals[b]))
            assert np.array_equal(cur, g["dyntext_traj_expected"][b, i + 1]), (b, i)
            assert done == bool(g["dyntext_success"][b, i])


def test_ant_sampler_preprocessing_matches_reference():
    """oracle.sampler.ant_cond_vector == the reference's DiffusionSampler.forward (antmaze branch) on the recorded cases."""
    g = golden("network")
    nh = g["sampler_ant_n_hist"]
    for i in range(len(nh)):
        h = int(nh[i])
        got = OS.ant_cond_vector(g["sampler_ant_obs"][i:i + 1, 3 - h:], g["sampler_ant_prev"][i:i + 1],
                                 g["sampler_ant_has_prev"][i:i + 1], g["sampler_ant_goals"][i])
        assert got.shape == (1, 97) and np.abs(got[0] - g["sampler_ant_cond_expected"][i]).max() < 2e-7


def test_prop_duration_schedule_trace():
    """The oracle planner with prop_duration = [128, 64, 32] rebuilds the reference planner's tree (golden sched_*)."""
    g = golden("traces")
    from tests.util import load_maze
    pl = ORRT.OraclePlanner(load_maze("boxes"), g["sched_start"], g["sched_goal"], ActionTape(int(g["sched_seed"])).sampler(),
                            prop_duration=[int(v) for v in g["sched_schedule"]])
    pl.plan(ORRT.RandomTape(42), int(g["sched_budget"]), batch=1)
    assert np.array_equal(np.array(pl.tree.parents, dtype=np.int32), g["sched_parents"])
    assert np.array_equal(np.array(pl.tree.states), g["sched_states"])
    assert pl.iterations == int(g["sched_iterations"])


def test_sampler_pre_post_matches_reference():
    g = golden("network")
    cond = OS.car_cond_vector(g["sampler_states"], g["sampler_prev"], g["sampler_has_prev"], g["sampler_goals"])
    assert np.abs(cond - g["sampler_cond_expected"]).max() < 2e-7
    x1 = g["sampler_noise"] + (0.25 * g["sampler_noise"] + 0.5)
    assert np.abs(OS.unnormalize_actions(x1.astype(np.float32)) - g["sampler_actions_expected"]).max() < 1e-6


def test_timesteps_match_reference(golden_dir):
    ref = json.load(open(os.path.join(golden_dir, "timesteps.json")))["get_timesteps_exp_4"]
    for k, v in ref.items():
        t0, dt = OS.get_timesteps("exp", int(k), 4.0)
        assert [float(x) for x in t0] == v["t0"] and [float(x) for x in dt] == v["dt"]
    from ditreeonlineplanner_amd.common.fm_utils import get_timesteps
    for k, v in ref.items():
        t0, dt = get_timesteps("exp", int(k), 4.0)
        assert [float(x) for x in t0] == v["t0"] and [float(x) for x in dt] == v["dt"]


@pytest.mark.parametrize("tag,inp,gcd", [("car", 2, 407)])
def test_unet_matches_reference(tag, inp, gcd):
    from oracle import denoiser as OD
    g = golden("network")
    torch.manual_seed(7)
    net = OD.OracleUnet1D(inp, gcd).eval()
    assert sum(p.numel() for p in net.parameters()) == int(g[f"unet_{tag}_nparams"])
    wsum = sum(float(v.double().sum()) for v in net.state_dict().values())
    assert abs(wsum - float(g[f"unet_{tag}_wsum"])) < 1e-6
    with torch.no_grad():
        y = net(torch.tensor(g[f"unet_{tag}_x"]), torch.tensor(g[f"unet_{tag}_t"]), torch.tensor(g[f"unet_{tag}_cond"]))
    assert np.abs(y.numpy() - g[f"unet_{tag}_y_expected"]).max() < 1e-5


@pytest.mark.parametrize("tag", ["race", "boxes", "rlarge2", "easy"])
def test_planner_trace_matches_reference(tag):
    g = golden("traces")
    maze = load_maze(str(g[f"trace_{tag}_maze_name"]))
    sr, sc, sdeg, gr, gc = [int(v) for v in g[f"trace_{tag}_scenario"]]
    start = np.array([*G.cell_rowcol_to_xy([sr, sc], maze), np.deg2rad(float(sdeg)), 0, 0, 0])
    goal = np.array([*G.cell_rowcol_to_xy([gr, gc], maze), 0, 0, 0, 0])
    pl = ORRT.OraclePlanner(maze, start, goal, ActionTape(int(g[f"trace_{tag}_tape_seed"])).sampler())
    reached, path, actions = pl.plan(ORRT.RandomTape(42), int(g[f"trace_{tag}_budget"]), batch=1)
    assert reached == bool(g[f"trace_{tag}_reached"])
    assert np.array_equal(np.array(pl.tree.parents), g[f"trace_{tag}_parents"])
    assert np.array_equal(np.array(pl.tree.states), g[f"trace_{tag}_states"])
    assert np.array_equal(path, g[f"trace_{tag}_path"]) and np.array_equal(actions, g[f"trace_{tag}_actions"])
    assert pl.iterations == int(g[f"trace_{tag}_iterations"]) and not pl.sticky_triggered


def test_run_type1_trace_matches_reference():
    """run_type 1: obstacle-ahead known answers and the two-stage trace of the reference planner
    (RRT.py:61-111,134-140,202-254)."""
    g = golden("traces")
    maze = load_maze("boxes")
    poses = g["rt1_ahead_poses"]
    st = np.concatenate([poses, np.zeros((len(poses), 3))], axis=1)
    assert np.array_equal(G.check_obstacle_ahead(st, maze), g["rt1_ahead_expected"])
    start, goal, seed = g["rt1_start"], g["rt1_goal"], int(g["rt1_seed"])
    n1, n2 = [int(v) for v in g["rt1_budgets"]]
    pl = ORRT.OraclePlanner(maze, start, goal, ActionTape(seed).sampler(), run_type=1)
    _, path1, act1 = pl.plan(ORRT.RandomTape(42), n1, batch=1)
    assert np.array_equal(np.array(pl.tree.parents), g["rt1_parents1"])
    assert np.array_equal(np.array(pl.tree.states), g["rt1_states1"])
    assert np.array_equal(path1, g["rt1_path1"]) and np.array_equal(act1, g["rt1_actions1"])
    pl2 = ORRT.OraclePlanner(g["rt1_maze2"], start, goal, ActionTape(seed).sampler(), run_type=1, init_main_path=path1)
    _, path2, act2 = pl2.plan(ORRT.RandomTape(42), n2, batch=1)
    assert np.array_equal(np.array(pl2.tree.parents), g["rt1_parents2"])
    assert np.array_equal(np.array(pl2.tree.states), g["rt1_states2"])
    if bool(g["rt1_has_path2"]):
        assert np.array_equal(path2, g["rt1_path2"]) and np.array_equal(act2, g["rt1_actions2"])
    else:
        assert path2 is None
    assert not pl.sticky_triggered and not pl2.sticky_triggered


def test_probability_maps_match_reference():
    """run_type >= 2: EDT prior, gaussian_map, combine_log_blend (prob_sampling_utils.py:50-94,146-165) --
    the oracle and the product's host module against the reference's outputs, bit for bit."""
    from oracle import prob_maps as PM
    from ditreeonlineplanner_amd import prob_sampling_utils as PSU
    g = golden("geometry")
    mazes, priors = g["probmap_mazes"], g["probmap_priors"]
    for m, pr in zip(mazes, priors):
        assert np.array_equal(PM.edt_prior(m), pr) and np.array_equal(PSU.edt_prior(m), pr)
    for i, (rx, ry, gx, gy) in enumerate(g["probmap_pairs"]):
        for mod in (PM, PSU):
            pdf, _, _ = mod.gaussian_map((rx, ry), (gx, gy))
            assert np.array_equal(pdf, g["probmap_gauss"][i]), (mod.__name__, i)
            assert np.array_equal(mod.combine_log_blend(priors[i % len(priors)], pdf), g["probmap_blend"][i])
    # degenerate blends fall back to the prior, then to uniform
    z = np.zeros((20, 20))
    for mod in (PM, PSU):
        assert np.allclose(mod.combine_log_blend(z, g["probmap_gauss"][0]).sum(), 1.0)


@pytest.mark.parametrize("rt", [2, 3])
def test_run_type23_trace_matches_reference(rt):
    g = golden("traces")
    maze = load_maze("boxes")
    start, goal = g["rt1_start"], g["rt1_goal"]
    pl = ORRT.OraclePlanner(maze, start, goal, ActionTape(int(g[f"rt{rt}_seed"])).sampler(), run_type=rt)
    assert np.array_equal(pl.sampling_map(), g[f"rt{rt}_prob_map"])
    _, path, act = pl.plan(ORRT.RandomTape(42), int(g[f"rt{rt}_budget"]), batch=1)
    assert np.array_equal(np.array(pl.tree.parents), g[f"rt{rt}_parents"])
    assert np.array_equal(np.array(pl.tree.states), g[f"rt{rt}_states"])
    assert np.array_equal(path, g[f"rt{rt}_path"]) and np.array_equal(act, g[f"rt{rt}_actions"])


@pytest.mark.parametrize("rt", [2, 3])
def test_car_env_sampling_map_wiring(rt):
    """The product's CarEnv (host part only, no kernel call) keeps the reference's per-run_type map wiring
    (car_env.py:100-137): equal to the CarEnv restatement the reference planner was run against."""
    from ditreeonlineplanner_amd.car_env import CarEnv
    g = golden("traces")
    maze = load_maze("boxes")
    start, goal = g["rt1_start"], g["rt1_goal"]
    env, oenv = CarEnv(maze_map=maze.copy(), collision_checking=False, run_type=rt), ORRT.OracleCarEnv(maze.copy(), run_type=rt)
    assert np.array_equal(env.prob_map, oenv.prob_map)
    opts = {"reset_cell": env.cell_xy_to_rowcol(start[:2]), "reset_deg": np.rad2deg(start[2]),
            "goal_cell": env.cell_xy_to_rowcol(goal[:2])}
    env.reset(options=opts)
    oenv.reset(options=opts)
    if rt >= 3:
        env.update_prob_map_by_loc()
        oenv.update_prob_map_by_loc()
    assert np.array_equal(env.prob_map, g[f"rt{rt}_prob_map"]) and np.array_equal(oenv.prob_map, env.prob_map)
    m2 = g["rt1_maze2"]
    env.maze_map = m2
    oenv.maze_map = m2
    assert np.array_equal(env.prob_map, oenv.prob_map) and not np.array_equal(env.prob_map, g[f"rt{rt}_prob_map"])


@pytest.mark.parametrize("tag", ["visible", "free", "goal", "collision", "hidden", "track"])
def test_online_loop_matches_reference(tag):
    """run_scenarios_with_lidar_DiTree.py:112-127,158-181,470-506 (oracle/online.py) vs the reference-driven loop."""
    from oracle import online as OO
    g = golden("online")
    k = lambda n: g[f"online_{tag}_{n}"]
    known, scanned = k("known0").copy(), k("scanned0").copy()
    o = OO.follow_plan(k("start"), k("actions"), 0, k("path"), known, k("true"), scanned, k("goal_xy"))
    assert [o["event"], o["action_idx"], o["obstacle_idx"]] == [int(v) for v in k("result")]
    assert np.array_equal(o["executed"], k("executed")) and np.array_equal(o["state"], k("state"))
    assert np.array_equal(known, k("known1")) and np.array_equal(scanned, k("scanned1"))


def test_online_path_check_known_answers():
    from oracle import online as OO
    g = golden("online")
    maze, path = g["online_free_maze"], g["online_free_path"]
    for marks, exp in zip(g["online_check_marks"], g["online_check_expected"]):
        sc = maze.copy()
        sc[marks[:, 0], marks[:, 1]] = 1
        assert OO.check_no_obstacles_in_path(sc, path) == int(exp)


def test_rounds_reduce_to_sequential_when_independent():
    """B > 1 rounds: every candidate's parent index must refer to the round-start snapshot."""
    maze = load_maze("boxes")
    start = np.array([*G.cell_rowcol_to_xy([17, 2], maze), np.deg2rad(45.0), 0, 0, 0])
    goal = np.array([*G.cell_rowcol_to_xy([2, 17], maze), 0, 0, 0, 0])
    pl = ORRT.OraclePlanner(maze, start, goal, ActionTape(5).sampler())
    tape = ORRT.RandomTape(42)
    n_before = 1
    for _ in range(6):
        s, c = tape.draw_round(32, maze.shape[1], maze.shape[0], goal)
        r = pl.expand_round(s, c)
        assert (r["parent"] < n_before).all()
        ids = r["accepted"]
        assert ids == list(range(n_before, n_before + len(ids)))
        n_before = len(pl.tree)
