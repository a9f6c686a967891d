"""The plans and the caller-supplied noise of the plan-polishing tests, shared by the CPU test (which checks on the oracle that no
candidate of these cases sits within 1e-9 of the goal radius or of a wall) and the GPU tests (which then compare exactly)."""
from __future__ import annotations

import functools

import numpy as np

from oracle import geometry as G
from tests.util import golden, load_maze


@functools.lru_cache(maxsize=None)
def easy_plan():
    """The golden trace `easy` (val_maze_7, 7 x 7): maze, start state, env goal, the plan's 45 float32 actions."""
    g = golden("traces")
    maze = load_maze(str(g["trace_easy_maze_name"]))
    sr, sc, sdeg, gr, gc = [int(v) for v in g["trace_easy_scenario"]]
    x0 = np.array([*G.cell_rowcol_to_xy([sr, sc], maze), np.deg2rad(float(sdeg)), 0, 0, 0])
    goal = np.array(G.cell_rowcol_to_xy([gr, gc], maze), dtype=np.float64)
    return maze, x0, goal, np.asarray(g["trace_easy_actions"], dtype=np.float32)


@functools.lru_cache(maxsize=None)
def corridor_plan():
    """A non-square 5 x 9 corridor (walls on the border) driven end to end: the tape arrives at 108 rows at 3.9 m/s and carries
    12 more rows behind its arrival, which the replay cuts."""
    maze = np.zeros((5, 9))
    maze[0] = maze[-1] = 1
    maze[:, 0] = maze[:, -1] = 1
    x0 = np.array([*G.cell_rowcol_to_xy([2, 1], maze), 0.0, 0, 0, 0])
    goal = np.array(G.cell_rowcol_to_xy([2, 7], maze), dtype=np.float64)
    t = np.arange(120)
    tape = np.stack([np.where(t < 30, 2.0, 0.0), 0.002 * np.sin(t / 5.0)], axis=1).astype(np.float32)
    return maze, x0, goal, tape


def colliding_tape():
    """On the corridor: steers into the wall."""
    t = np.arange(200)
    return np.stack([np.full(200, 2.0), np.where(t < 10, 0.1, 0.0)], axis=1).astype(np.float32)


PLANS = {"easy": easy_plan, "corridor": corridor_plan}

# (plan, K, hold, iterations, seed): K = 64 one wave, 192 three waves of one work-group, 320 crosses a work-group; hold 1, 4 and
# past the tape's rows
KERNEL_CASES = [("easy", 64, 1, 4, 11), ("easy", 192, 4, 4, 12), ("easy", 320, 100, 3, 13), ("corridor", 320, 4, 3, 14),
                ("corridor", 64, 1000, 3, 15)]
SIGMA = (1.0, 0.1)


def case_inputs(name, K, hold, N, seed):
    """-> (noise (N, K, NB, 2), first_row (N, K)).  Candidates 0 and 1 of every iteration start at row 0 and at the last row (-1);
    iteration 1 is one in which nothing arrives: every candidate brakes (dD - 100 -> clipped to -10) from row 0 on."""
    tape = PLANS[name]()[3]
    rng = np.random.default_rng(seed)
    nb = (len(tape) + hold - 1) // hold
    noise = rng.normal(size=(N, K, nb, 2)) * np.asarray(SIGMA)
    first_row = rng.integers(0, 1 << 20, size=(N, K)).astype(np.int32)
    first_row[:, 0] = 0
    first_row[:, 1] = -1
    noise[1, :, :, 0] = -100.0
    first_row[1] = 0
    return noise, first_row
