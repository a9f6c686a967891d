"""Record what the reference's Lidar2DSim does on every bundled car maze, square or not.

Runs ONLY in the build container (imports the reference's lidar_sim/lidar_2d_sim.py unmodified); what it writes,
tests/golden/lidar_nonsquare.json, is data: per maze its shape, 8 seeded poses in free cells (x_col, y_row, yaw) and, per
pose, "ok" or the name of the exception type ``Lidar2DSim().scan`` raised.  tests/test_oracle_golden.py holds the oracle's
default (``extents="reference"``) to these outcomes and requires ``extents="map"`` to scan every pose.

    python tests/golden/make_lidar_nonsquare.py
"""
import glob
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, REPO)
sys.path.insert(0, REF)

from lidar_sim.lidar_2d_sim import Lidar2DSim as RefLidar           # noqa: E402

DATA = os.path.join(REPO, "ditreeonlineplanner_amd", "data")
SEED, POSES = 20, 8


def free_poses(rng, maze, n):
    """n poses in free cells: fractional offsets in [0.05, 0.95], yaw uniform in [-pi, pi)."""
    free = np.argwhere(maze == 0)
    rc = free[rng.choice(len(free), n, replace=len(free) < n)]
    off = rng.uniform(0.05, 0.95, (n, 2))
    yaw = rng.uniform(-np.pi, np.pi, n)
    return np.stack([rc[:, 1] + off[:, 0], rc[:, 0] + off[:, 1], yaw], axis=1)


def main():
    rng = np.random.default_rng(SEED)
    lidar = RefLidar()
    out = {}
    for path in sorted(glob.glob(os.path.join(DATA, "*.csv"))):
        name = os.path.splitext(os.path.basename(path))[0]
        if name.startswith("test_scenarios"):
            continue
        maze = np.loadtxt(path, delimiter=",")
        ref_maze = np.loadtxt(os.path.join(REF, "maps", "mazes", name + ".csv"), delimiter=",")
        assert np.array_equal(maze, ref_maze), name
        poses = free_poses(rng, maze, POSES)
        results = []
        for p in poses:
            try:
                lidar.scan(p, maze)
                results.append("ok")
            except Exception as e:                                   # noqa: BLE001 -- the type is what is recorded
                results.append(type(e).__name__)
        out[name] = {"shape": list(maze.shape), "poses": poses.tolist(), "result": results}
        print(f"{name} {maze.shape}: {results}")
    with open(os.path.join(HERE, "lidar_nonsquare.json"), "w") as f:
        json.dump({"seed": SEED, "mazes": out}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
