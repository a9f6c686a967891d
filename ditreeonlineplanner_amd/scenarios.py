"""The scenario sets of the reference benchmark: one maze, start and goal per row of a scenario file.

The car: data/test_scenarios_car.csv.

``car_scenarios()`` returns what run_scenarios.py:203-246 builds for the car from every row -- the maze from ``<maze_name>.csv``,
``start = [x, y, deg2rad(start_deg), 0, 0, 0]`` and ``goal = [x, y, 0, 0, 0, 0]`` with x, y from ``CarEnv.cell_rowcol_to_xy`` --
so that a scenario set can be planned at once (``planners.RRT.plan_scenario_runs``).

The ant: ``ant_scenarios(csv_path)`` reads a file in the layout of the reference's experiments/test_scenarios_ant.csv
(run_scenarios.py:202-233) for ``planners.RRT.plan_ant_scenario_runs``; the file itself is not packaged.
"""
from __future__ import annotations

import csv
import os

import numpy as np

DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data")


def car_scenarios(csv_path=None, mazes_dir=None):
    """-> list of dicts ``name``, ``maze_name``, ``maze`` (float64 map as np.loadtxt reads it), ``start`` (6,), ``goal`` (6,),
    ``start_cell`` / ``goal_cell`` (row, col), in file order.  A row whose maze file is missing is skipped, as the reference
    skips it."""
    from .car_env import CarEnv
    csv_path = os.path.join(DATA, "test_scenarios_car.csv") if csv_path is None else csv_path
    mazes_dir = DATA if mazes_dir is None else mazes_dir
    out, mazes = [], {}
    with open(csv_path, newline="") as f:
        rows = csv.reader(f)
        next(rows)                                                   # the header
        for row in rows:
            if not row:
                continue
            name, maze_name, start_row, start_col, start_deg, goal_row, goal_col = row
            path = os.path.join(mazes_dir, f"{maze_name}.csv")
            if not os.path.exists(path):
                continue
            if maze_name not in mazes:
                mazes[maze_name] = np.loadtxt(path, delimiter=",")
            maze = mazes[maze_name]
            env = CarEnv(maze_map=maze, collision_checking=False)
            start_xy = env.cell_rowcol_to_xy(np.array([int(start_row), int(start_col)]))
            goal_xy = env.cell_rowcol_to_xy(np.array([int(goal_row), int(goal_col)]))
            out.append(dict(name=name, maze_name=maze_name, maze=maze.copy(),
                            start=np.array([start_xy[0], start_xy[1], np.deg2rad(float(start_deg)), 0.0, 0.0, 0.0]),
                            goal=np.array([goal_xy[0], goal_xy[1], 0.0, 0.0, 0.0, 0.0]),
                            start_cell=(int(start_row), int(start_col)), goal_cell=(int(goal_row), int(goal_col))))
    return out


def ant_scenarios(csv_path, mazes_dir=None, s_global=4.0):
    """The antmaze scenario set of ``csv_path`` (rows ``name, maze_name, start_row, start_col, goal_row, goal_col``;
    run_scenarios.py:202-233) -> list of dicts ``name``, ``maze_name``, ``maze``, ``start`` (29,), ``goal`` (29,),
    ``start_cell`` / ``goal_cell`` (row, col), in file order: ``start = zeros(29)`` with ``[:2] = xy``, ``[2] = 0.75`` (torso
    height), ``[3] = 1.0`` (qw); ``goal = zeros(29)`` with ``[:2] = xy`` (:226-233).  A row whose maze file is missing is
    skipped, as the reference skips it.  ``mazes_dir``: where ``<maze_name>.csv`` lives (default: the packaged maps).

    PARITY UNPINNED: the cell -> xy map, ``xy = ((col + 0.5) s - W s / 2, H s / 2 - (row + 0.5) s)`` with s = ``s_global``, is
    gymnasium-robotics' ``Maze.cell_rowcol_to_xy`` (third party, not in the reference tree), restated here.  It is held to the
    reference's own indexing: every cell centre indexes back to its (row, col) under ``is_colliding_maze``
    (common/map_utils.py:155-159), which the tests check on the reference's file."""
    mazes_dir = DATA if mazes_dir is None else mazes_dir
    s = float(s_global)
    out, mazes = [], {}
    with open(csv_path, newline="") as f:
        rows = csv.reader(f)
        next(rows)                                                   # the header
        for row in rows:
            if not row:
                continue
            name, maze_name, start_row, start_col, goal_row, goal_col = row
            path = os.path.join(mazes_dir, f"{maze_name}.csv")
            if not os.path.exists(path):
                continue
            if maze_name not in mazes:
                mazes[maze_name] = np.loadtxt(path, delimiter=",")
            maze = mazes[maze_name]
            H, W = maze.shape

            def xy(r, c):
                return np.array([(c + 0.5) * s - W * s / 2, H * s / 2 - (r + 0.5) * s])

            start_cell, goal_cell = (int(start_row), int(start_col)), (int(goal_row), int(goal_col))
            start, goal = np.zeros(29), np.zeros(29)
            start[:2] = xy(*start_cell)
            start[2], start[3] = 0.75, 1.0
            goal[:2] = xy(*goal_cell)
            out.append(dict(name=name, maze_name=maze_name, maze=maze.copy(), start=start, goal=goal, start_cell=start_cell,
                            goal_cell=goal_cell))
    return out
