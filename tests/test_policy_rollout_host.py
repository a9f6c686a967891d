"""CPU: the host side of the policy roll-out -- the reference-shaped trajectory rebuilt from per-episode results, the refusals
that need no device, and the reference's validation scenario file read through ``scenarios.car_scenarios``."""
import os

import numpy as np
import pytest

from oracle import geometry as G
from tests import policy_rollout_ref as R
from tests.util import DATA, REPO, load_maze

FIXTURE = os.path.join(REPO, "tests", "golden", "validation_scenarios_car.csv")


def _episodes(n_steps, terminated, M, seed=0):
    rng = np.random.default_rng(seed)
    N = len(n_steps)
    rows = rng.normal(size=(N, M, 8))
    for i, n in enumerate(n_steps):
        rows[i, n:] = 0.0                                   # the device leaves rows it never wrote at zero
    return dict(rows=rows, n_steps=np.array(n_steps), terminated=np.array(terminated, dtype=bool),
                final_state=rng.normal(size=(N, 6)))


@pytest.mark.parametrize("n_steps,terminated,M", [
    ([5, 12, 1, 12], [True, False, True, False], 12),      # the loop ran out of steps: T = max_episode_steps
    ([5, 9, 1, 9], [True, True, True, True], 12),          # everybody ended: T = 9 < max_episode_steps, rows 10.. stay zero
    ([3], [True], 8), ([8], [False], 8), ([8], [True], 8),
    ([1, 1], [True, True], 1),
])
def test_reference_trajectory_is_the_loops_fill_forward(n_steps, terminated, M):
    from ditreeonlineplanner_amd.policy_rollout import reference_trajectory
    ep = _episodes(n_steps, terminated, M)
    traj = reference_trajectory(ep["rows"], ep["n_steps"], ep["terminated"], ep["final_state"], M)
    assert traj.shape == (len(n_steps), M + 1, 8) and traj.dtype == np.float64
    assert np.array_equal(traj, R.fill_forward(ep, M))
    T = max(n_steps)
    for i, (n, t) in enumerate(zip(n_steps, terminated)):
        assert np.array_equal(traj[i, :n], ep["rows"][i, :n])
        if t:                                               # the last written row, up to and including row T
            assert (traj[i, n:T + 1] == ep["rows"][i, n - 1]).all()
        else:                                               # [final state, 0, 0] at row T
            assert np.array_equal(traj[i, T], np.concatenate([ep["final_state"][i], [0.0, 0.0]]))
        assert not traj[i, T + 1:].any()


def test_reference_trajectory_refuses_impossible_results():
    from ditreeonlineplanner_amd.policy_rollout import reference_trajectory
    ep = _episodes([5, 12], [True, False], 12)
    with pytest.raises(ValueError, match="did not end all stop"):
        reference_trajectory(ep["rows"], [5, 11], [False, False], ep["final_state"], 12)
    with pytest.raises(ValueError, match="before its first step"):
        reference_trajectory(ep["rows"], [0, 12], [True, False], ep["final_state"], 12)
    with pytest.raises(ValueError, match=r"\[0, max_episode_steps\]"):
        reference_trajectory(ep["rows"], [5, 13], [True, False], ep["final_state"], 12)


def test_rollout_refuses_by_name_without_a_device():
    from ditreeonlineplanner_amd.rollout_manager import check_rollout_arguments, rollout
    check_rollout_arguments("carmaze")
    for kw, msg in ((dict(env_id="antmaze"), "only the car"), (dict(env_id="PointMaze"), "only the car"),
                    (dict(env_id="drone"), "only the car"), (dict(env_id="car_forest"), "only the car"),
                    (dict(prediction_type="observations"), "prediction_type='observations'"),
                    (dict(obs_history=3), "obs_history=3"), (dict(action_history=2), "action_history=2"),
                    (dict(position_conditioned=True), "position_conditioned=True"),
                    (dict(goal_conditioned=False), "goal_conditioned=False"),
                    (dict(local_map_conditioned=False), "local_map_conditioned=False"), (dict(world_size=2), "2 ranks")):
        args = dict(env_id="carmaze")
        args.update(kw)
        with pytest.raises(NotImplementedError, match=msg):
            check_rollout_arguments(**args)
    # the public function refuses before it reads a file, builds a sampler or opens the device
    with pytest.raises(NotImplementedError, match="prediction_type='observations'"):
        rollout("carmaze", "flow_matching", None, None, prediction_type="observations", scenarios_file="/nonexistent.csv")
    with pytest.raises(NotImplementedError, match="only the car"):
        rollout("antmaze", "flow_matching", None, None)


def test_validation_scenarios_read_through_car_scenarios():
    from ditreeonlineplanner_amd.rollout_manager import validation_episodes
    from ditreeonlineplanner_amd.scenarios import car_scenarios
    sc = car_scenarios(FIXTURE, DATA)
    want = [("val_maze_small", "val_maze_7", (1, 5), 180.0, (5, 3)), ("val_maze_large", "val_maze_10", (1, 3), 180.0, (7, 1)),
            ("val_maze_xlarge", "val_maze_15", (1, 5), 270.0, (13, 4))]
    assert len(sc) == 3
    for s, (name, maze_name, start, deg, goal) in zip(sc, want):
        maze = load_maze(maze_name)
        assert s["name"] == name and s["maze_name"] == maze_name and np.array_equal(s["maze"], maze)
        assert s["start_cell"] == start and s["goal_cell"] == goal
        assert np.array_equal(s["start"], [*G.cell_rowcol_to_xy(list(start), maze), np.deg2rad(deg), 0, 0, 0])
        assert np.array_equal(s["goal"], [*G.cell_rowcol_to_xy(list(goal), maze), 0, 0, 0, 0])
        assert maze[start] == 0 and maze[goal] == 0
    scenes, starts, scene_of = validation_episodes(sc, 4)
    assert starts.shape == (12, 6) and starts.dtype == np.float64 and list(scene_of) == [0] * 4 + [1] * 4 + [2] * 4
    for k, s in enumerate(sc):
        assert np.array_equal(scenes[k][0], s["maze"]) and np.array_equal(scenes[k][1], s["goal"][:2])
        f32 = np.zeros(6, dtype=np.float32)                 # CarEnv.reset: a float32 state
        f32[:3] = s["start"][:3]
        assert (starts[4 * k: 4 * k + 4] == f32.astype(np.float64)).all()
    assert starts[8, 2] == np.float64(np.float32(np.deg2rad(270.0))) != np.deg2rad(270.0)


def test_restatement_reproduces_the_constructed_cases():
    """From rest at full throttle the car covers 0.0277 m after 8 steps, 0.2471 after 16 and 0.5252 after 21: from cell (1, 5) of
    val_maze_7 at 180 deg the goal cell (1, 4) is reached at step index 20; a zero tape never ends."""
    maze = load_maze("val_maze_7")
    s = np.array([*G.cell_rowcol_to_xy([1, 5], maze), np.pi, 0, 0, 0])
    x0, at = s[0], {}
    for t in range(21):
        s = G.car_step(s, np.array([10.0, 0.0]))
        at[t + 1] = x0 - s[0]
    assert abs(at[8] - 0.0277) < 1e-4 and abs(at[16] - 0.2471) < 1e-4 and abs(at[21] - 0.5252) < 1e-4
    goal = G.cell_rowcol_to_xy([1, 4], maze)
    start = np.array([*G.cell_rowcol_to_xy([1, 5], maze), np.pi, 0, 0, 0])
    full = R.tape_actions(lambda c, N, P: np.tile([10.0, 0.0], (N, P, 1)), 2, 16)
    for M, succ in ((20, -1), (21, 20), (40, 20)):
        r = R.run_episodes([maze], [goal], np.stack([start, start]), [0, 0], full, 8, M)
        assert list(r["success_step"]) == [succ, succ] and list(r["n_steps"]) == [min(M, 21)] * 2
    r = R.run_episodes([maze], [goal], start[None], [0], R.tape_actions(lambda c, N, P: np.zeros((N, P, 2)), 1, 16), 8, 40)
    assert not r["terminated"][0] and r["n_steps"][0] == 40 and r["chunks"] == 5
