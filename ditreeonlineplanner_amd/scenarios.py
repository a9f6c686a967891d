"""The car scenario set of the reference benchmark: data/test_scenarios_car.csv, one maze, start and goal per row.

``car_scenarios()`` returns what run_scenarios.py:203-246 builds for the car from every row -- the maze from ``<maze_name>.csv``,
``start = [x, y, deg2rad(start_deg), 0, 0, 0]`` and ``goal = [x, y, 0, 0, 0, 0]`` with x, y from ``CarEnv.cell_rowcol_to_xy`` --
so that a scenario set can be planned at once (``planners.RRT.plan_scenario_runs``).
"""
from __future__ import annotations

import csv
import os

import numpy as np

DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data")


def car_scenarios(csv_path=None, mazes_dir=None):
    """-> list of dicts ``name``, ``maze_name``, ``maze`` (float64 map as np.loadtxt reads it), ``start`` (6,), ``goal`` (6,), in
    file order.  A row whose maze file is missing is skipped, as the reference skips it."""
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
                            goal=np.array([goal_xy[0], goal_xy[1], 0.0, 0.0, 0.0, 0.0])))
    return out
