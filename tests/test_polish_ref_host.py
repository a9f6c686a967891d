"""CPU: the numpy restatement of plan polishing (tests/polish_ref.py) alone on the golden `easy` tape and on the GPU tests' cases,
and the argument refusals of polish_plans that need no device."""
import numpy as np
import pytest

from tests import polish_cases as PC
from tests import polish_ref as R

K, N = 256, 12
SETTINGS = dict(sigma=(1.0, 0.1), hold=8, seed=1)


@pytest.fixture(scope="module")
def easy_run():
    maze, x0, goal, tape = PC.easy_plan()
    return R.polish(maze, x0, goal, tape.astype(np.float64), K, N, **SETTINGS)


def test_the_easy_tape_replays_to_the_goal_at_45_rows():
    maze, x0, goal, tape = PC.easy_plan()
    rp = R.replay(maze, x0, goal, tape.astype(np.float64))
    assert rp["status"] == R.OK and rp["rows"] == 45 == len(tape)
    assert 44.0 <= rp["tau"] < 45.0
    assert rp["states"].shape == (46, 6) and np.array_equal(rp["states"][0], x0)
    # the last rows move fast enough for the 1e-6 bound on tau (>= 0.2 m/s: >= 4 mm a row)
    assert rp["states"][-3:, 3].min() >= 0.2
    # the replay reproduces the plan row for row: the golden trace's path ends where the tape's roll ends
    assert np.abs(rp["states"][-1] - golden_path_end()).max() < 1e-5


def golden_path_end():
    from tests.util import golden
    return np.asarray(golden("traces")["trace_easy_path"][-1], dtype=np.float64)


def test_polishing_shortens_the_easy_tape_and_never_lengthens_it(easy_run):
    out = easy_run
    assert out["status"] == R.OK and out["rows"] < 45
    rows = [45] + [t["rows"] for t in out["trace"]]
    taus = [out["arrival_in"]] + [t["tau_star"] for t in out["trace"]]
    assert all(b <= a for a, b in zip(rows, rows[1:]))
    assert all(b <= a for a, b in zip(taus, taus[1:]))
    assert out["arrival_out"] == taus[-1] < out["arrival_in"]
    for t, before in zip(out["trace"], taus):
        assert t["accepted"] == (t["winner"] >= 0 and t["tau"] < before)
        assert t["tau_star"] == (t["tau"] if t["accepted"] else before)
    # the result is a rolled, collision-free, arriving, f32-exact tape
    maze, x0, goal, _ = PC.easy_plan()
    rp = R.replay(maze, x0, goal, out["tape"])
    assert rp["status"] == R.OK and rp["rows"] == out["rows"] == len(out["tape"]) and rp["tau"] == out["arrival_out"]
    assert np.array_equal(rp["states"], out["states"])
    assert np.array_equal(out["tape"].astype(np.float32).astype(np.float64), out["tape"])


def test_sigma_zero_returns_the_input():
    maze, x0, goal, tape = PC.easy_plan()
    out = R.polish(maze, x0, goal, tape.astype(np.float64), 64, 3, (0.0, 0.0), 4, seed=5)
    assert out["rows"] == 45 and np.array_equal(out["tape"], tape.astype(np.float64))
    assert out["arrival_out"] == out["arrival_in"]
    assert all(not t["accepted"] and t["arriving"] == 64 and t["winner"] == 0 for t in out["trace"])


def test_refused_plans():
    maze, x0, goal, tape = PC.corridor_plan()
    assert R.replay(maze, x0, goal, PC.colliding_tape().astype(np.float64))["status"] == R.COLLIDES
    assert R.replay(maze, x0, goal, tape[:40].astype(np.float64))["status"] == R.NO_ARRIVAL
    inside = x0.copy()
    inside[:2] = goal + [0.3, 0.0]
    assert R.replay(maze, inside, goal, tape.astype(np.float64))["status"] == R.START_IN_GOAL
    bad = tape.astype(np.float64)
    bad[3, 0] += 1e-12
    assert R.replay(maze, x0, goal, bad)["status"] == R.NOT_F32
    out = R.polish(maze, x0, goal, PC.colliding_tape().astype(np.float64), 64, 2, (1.0, 0.1), 4, seed=0)
    assert out["status"] == R.COLLIDES and out["trace"] == [] and np.array_equal(out["tape"], PC.colliding_tape())


def test_the_corridor_tape_is_cut_at_its_arrival():
    maze, x0, goal, tape = PC.corridor_plan()
    rp = R.replay(maze, x0, goal, tape.astype(np.float64))
    assert rp["status"] == R.OK and rp["rows"] < len(tape) and maze.shape == (5, 9)
    assert rp["states"][-3:, 3].min() >= 0.2


def test_the_hash_of_the_first_row_and_the_given_first_rows():
    a = R.first_rows(7, 3, 256, 45)
    assert a.min() >= 0 and a.max() < 45 and len(np.unique(a)) > 20
    assert np.array_equal(a, R.first_rows(7, 3, 256, 45)) and not np.array_equal(a, R.first_rows(7, 4, 256, 45))
    assert np.array_equal(R.given_first_rows([0, 44, 45, 100, -1, -45, -46], 45), [0, 44, 0, 10, 44, 0, 0])


@pytest.mark.parametrize("case", PC.KERNEL_CASES, ids=lambda c: f"{c[0]}-K{c[1]}-hold{c[2]}")
def test_the_gpu_cases_need_no_exemption(case):
    """No candidate of the GPU tests' cases comes within 1e-9 of the goal radius or of a wall on the oracle, iteration 1 is one
    in which nothing arrives, and the candidates that start at row 0 and at the last row are there."""
    name, K_, hold, N_, seed = case
    maze, x0, goal, tape = PC.PLANS[name]()
    noise, first_row = PC.case_inputs(*case)
    out = R.polish(maze, x0, goal, tape.astype(np.float64), K_, N_, PC.SIGMA, hold, seed, noise=noise, first_row=first_row,
                   critical=True)
    assert out["status"] == R.OK
    assert [t["critical"] for t in out["trace"]] == [0] * N_
    assert out["trace"][1]["arriving"] == 0 and out["trace"][1]["winner"] == -1 and not out["trace"][1]["accepted"]
    assert out["trace"][0]["arriving"] > 0
    T = out["trace"][0]["rows"]
    assert list(R.given_first_rows(first_row[2, :2], T)) == [0, T - 1]


def test_polish_plans_refuses_bad_settings_without_a_device():
    from ditreeonlineplanner_amd.polish import check_settings, polish_plans
    maze, x0, goal, tape = PC.easy_plan()
    for bad, word in ((dict(rollouts=0), "multiple of 64"), (dict(rollouts=100), "multiple of 64"), (dict(iterations=-1), "iterations"),
                      (dict(hold=0), "hold"), (dict(sigma=(1.0, float("nan"))), "sigma"), (dict(sigma=(-1.0, 0.1)), "sigma"),
                      (dict(sigma=(float("inf"), 0.1)), "sigma"), (dict(sigma=(1.0,)), "sigma")):
        kw = dict(rollouts=64, iterations=1, sigma=(1.0, 0.1), hold=4)
        kw.update(bad)
        with pytest.raises(ValueError, match=word):
            polish_plans(None, maze, x0[None], goal[None], [tape], **kw)
    assert check_settings(128, 0, (0.0, 0.0), 1) == (128, 0, (0.0, 0.0), 1)
    with pytest.raises(ValueError, match="starts and goals"):
        polish_plans(None, maze, np.zeros((2, 6)), np.zeros((2, 2)), [tape], rollouts=64, iterations=1)
    with pytest.raises(ValueError, match="empty tape"):
        polish_plans(None, maze, x0[None], goal[None], [np.zeros((0, 2))], rollouts=64, iterations=1)
    big = np.zeros((200, 200))
    with pytest.raises(ValueError, match="staged in LDS"):
        polish_plans(None, big, x0[None], goal[None], [tape], rollouts=64, iterations=1)


def test_polish_refuses_the_ant():
    from ditreeonlineplanner_amd.planners.RRT import RRT_Planner, polish_runs
    pl = RRT_Planner.__new__(RRT_Planner)
    pl.is_ant = True
    with pytest.raises(NotImplementedError):
        pl.polish()
    with pytest.raises(NotImplementedError):
        polish_runs(pl, [])
