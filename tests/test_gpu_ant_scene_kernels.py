"""GPU: the ant scene rollout (ant_rollout_kernel<.., SCENES>) and the per-tree-goal fallback of ant forests against an
independent reference at the scene table's limits: 64 scenes in an atlas of more than 15 000 cells, the last map at an offset
that is no multiple of 16, a 1 x N and an N x 1 map among them.  Every candidate of ditree_forest_expand_round_ant_scenes is
compared with oracle.ant.ant_rollout_chunk on its own scene's maze and desired goal, from the parent the device chose among its
tree's nodes: exactly on tape dynamics; status and steps exactly and states within 1e-9 on model dynamics (the bound the
single-maze model kernel is held to)."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import ant as OA
from oracle import geometry as G
from tests.test_gpu_ant_round import ant_norm
from tests.test_gpu_forest import ctx, dev  # noqa: F401
from tests.test_gpu_forest_kernels import limit_scenes, nn_ref, norm_rule

pytestmark = pytest.mark.gpu

S_GLOBAL, A_STEPS, T, CAP = 4.0, 8, 64, 8


def cell_xy(rc, maze):
    H, W = maze.shape
    return np.array([(rc[1] + 0.5) * S_GLOBAL - W * S_GLOBAL / 2, H * S_GLOBAL / 2 - (rc[0] + 0.5) * S_GLOBAL])


def ant_limit_scene(maze, rng):
    """Start: an upright ant near the centre of a free cell (interior where there is one); desired goal: near the centre of a
    neighbouring cell; goal_state: that cell's centre."""
    H, W = maze.shape
    free = np.argwhere(maze == 0)
    if not len(free):                                              # a border row: every cell a wall
        free = np.argwhere(maze >= 0)
    inner = [rc for rc in free if 0 < rc[0] < H - 1 and 0 < rc[1] < W - 1]
    rc = np.array(inner[rng.integers(len(inner))] if inner else free[rng.integers(len(free))])
    nb = [rc + d for d in ((0, 1), (1, 0), (0, -1), (-1, 0)) if 0 <= (rc + d)[0] < H and 0 <= (rc + d)[1] < W]
    goal_rc = nb[rng.integers(len(nb))] if nb else rc
    start, goal = np.zeros(29), np.zeros(29)
    start[:2] = cell_xy(rc, maze) + rng.uniform(-0.5, 0.5, 2)
    start[2], start[3] = 0.75, 1.0
    goal[:2] = cell_xy(goal_rc, maze)
    return maze, start, goal, goal[:2] + rng.uniform(-0.4, 0.4, 2)


def walk_tape(rng, from_xy, towards, n):
    """(n, 1, A, 29) observations: per candidate a walk of 0.5-unit steps from its parent's xy, every third one bent towards
    its row of ``towards`` (n, 2); plausible torso heights, unit quaternions that tip over now and then."""
    o = rng.normal(0.0, 0.6, (n, 1, A_STEPS, 29))
    for b in range(n):
        heading = rng.uniform(-np.pi, np.pi) + np.cumsum(rng.normal(0.0, 0.3, A_STEPS))
        xy = from_xy[b] + np.cumsum(0.5 * np.stack([np.cos(heading), np.sin(heading)], axis=1), axis=0)
        if b % 3 == 0:
            w = (np.arange(1, A_STEPS + 1) / A_STEPS)[:, None]
            xy = (1 - w) * xy + w * (towards[b] + rng.uniform(-0.5, 0.5, 2))
        ang = np.cumsum(rng.normal(0.0, 0.5 if rng.random() < 0.1 else 0.1, A_STEPS))
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        o[b, 0, :, 0:2] = xy
        o[b, 0, :, 2] = rng.uniform(0.45, 0.8, A_STEPS)
        o[b, 0, :, 3] = np.cos(ang / 2)
        o[b, 0, :, 4:7] = np.sin(ang / 2)[:, None] * axis
    return o


def round_inputs(rng, mazes, scenes, xy, sizes, P):
    """One round of 1 - 3 candidates per tree: counts, offsets, samples (B, 29), actions (B, 1, P, 8), the parents a segmented
    nearest-node search must choose, and an observation tape that walks on from those parents."""
    counts = rng.integers(1, 4, T)
    off = np.concatenate([[0], np.cumsum(counts)])
    B = int(off[-1])
    tree_of_row = np.searchsorted(off, np.arange(B), "right") - 1
    samples = np.zeros((B, 29))
    for b, t in enumerate(tree_of_row):
        H, W = mazes[t].shape
        samples[b, :2] = rng.uniform(-W * 2.0, W * 2.0), rng.uniform(-H * 2.0, H * 2.0)
    acts = np.zeros((B, 1, P, 8))
    acts[:, 0, :A_STEPS] = rng.uniform(-1.2, 1.2, (B, A_STEPS, 8))
    want_parent = nn_ref(xy, samples[:, :2], off, CAP, sizes)
    desired = np.stack([scenes[t][3] for t in tree_of_row])
    return counts, off, samples, acts, want_parent, walk_tape(rng, xy[want_parent], desired, B)


@pytest.mark.parametrize("dynamics", ["tape", "model"])
def test_ant_scene_forest_on_a_full_scene_table(ctx, dynamics):
    """64 ant trees, one per scene of the 64-scene atlas, two rounds of 1 - 3 candidates per tree on injected actions; then the
    per-tree-goal fallback against the first smallest np.linalg.norm over each tree's nodes 1.."""
    from ditreeonlineplanner_amd import _lib
    from ditreeonlineplanner_amd.forest import AntSceneForestEngine, atlas_layout
    from ditreeonlineplanner_amd.ops import _dbl
    rng = np.random.default_rng(78)
    mazes = limit_scenes()
    offsets, dims, cells = atlas_layout(mazes)
    assert len(mazes) == T and cells == sum(m.size for m in mazes), "two scenes share a map"
    assert 15000 <= cells <= 16384 and offsets[-1] > 14000 and offsets[-1] % 16 != 0, (cells, offsets[-1])
    assert any(m.shape[0] == 1 for m in mazes) and any(m.shape[1] == 1 for m in mazes)
    scenes = [ant_limit_scene(m, rng) for m in mazes]
    forest = AntSceneForestEngine(ctx, scenes, T, CAP, batch=3 * T, norm=ant_norm(), dynamics=dynamics, edge_length=A_STEPS,
                                  action_horizon=A_STEPS)
    assert forest.n_chunks == 1
    for t in range(T):
        forest.reset_tree(t, t)
    seen, differs = set(), 0
    for rnd in range(2):
        xy = forest.tree.xy.cpu().numpy()
        state = forest.tree.state.cpu().numpy()
        sizes = [int(v) for v in forest.n_nodes_host]
        counts, off, samples, acts, want_parent, tape = round_inputs(rng, mazes, scenes, xy, sizes, forest.P)
        B = int(off[-1])
        forest.expand_round(dev(samples), dev(samples[:, :2]), inject_actions=dev(acts), counts_per_tree=counts,
                            next_obs_tape=dev(tape) if dynamics == "tape" else None)
        rb = forest.rb
        parent = rb.parent[:B].cpu().numpy()
        assert np.array_equal(parent, want_parent)
        status, steps = rb.status[:B].cpu().numpy(), rb.chunk_steps[:B, 0].cpu().numpy()
        states, end = rb.states[:B, 0].cpu().numpy(), rb.end_state[:B].cpu().numpy()
        out_acts = rb.actions[:B, 0].cpu().numpy()
        for t in range(T):
            rows = slice(off[t], off[t + 1])
            obs = tape[rows]
            if dynamics == "tape":
                step = lambda i, cur, act, r, obs=obs: obs[r, 0, i]                       # noqa: E731
            else:
                step = lambda i, cur, act, r: OA.ant_model_step(cur, act)                # noqa: E731
            exp = OA.ant_rollout_chunk(state[parent[rows]], acts[rows, 0], step, mazes[t], scenes[t][3], S_GLOBAL, A=A_STEPS)
            assert np.array_equal(status[rows] & 0xff, exp["status"]), (t, status[rows], exp["status"])
            assert np.array_equal(steps[rows], exp["n_steps"]), t
            assert np.array_equal(out_acts[rows], exp["actions"]), t
            if dynamics == "tape":
                assert np.array_equal(states[rows], exp["states"]) and np.array_equal(end[rows], exp["end_state"]), t
            else:
                assert np.abs(states[rows] - exp["states"]).max() < 1e-9, t
                assert np.abs(end[rows] - exp["end_state"]).max() < 1e-9, t
            seen.update(exp["status"].tolist())
            if t > 0:                                             # scene 0's record for this row would give another outcome
                e0 = OA.ant_rollout_chunk(state[parent[rows]], acts[rows, 0], step, mazes[0], scenes[0][3], S_GLOBAL, A=A_STEPS)
                differs += int((e0["status"] != exp["status"]).any() or (e0["n_steps"] != exp["n_steps"]).any())
    print("ant scene table", dynamics, "statuses seen", sorted(seen), "trees whose rows differ under scene 0:", differs)
    assert {G.STATUS_OK, G.STATUS_COLLIDED} <= seen and differs >= 20, (seen, differs)
    if dynamics == "tape":
        assert G.STATUS_GOAL in seen
    # ---- the fallback with one goal per tree: first smallest norm over the tree's nodes 1.., -1 for a root alone
    xy = forest.tree.xy.cpu().numpy()
    sizes = [int(v) for v in forest.n_nodes_host]
    goals = np.stack([scenes[t][2][:2] + rng.uniform(-3.0, 3.0, 2) for t in range(T)])
    ref = [-1 if n < 2 else 1 + int(np.argmin(norm_rule(xy[t * CAP + 1:t * CAP + n], goals[t]))) for t, n in enumerate(sizes)]
    out = torch.full((T,), -9, dtype=torch.int32, device="cuda")
    ga, gp = _dbl(goals)
    _lib.check(ctx._h, _lib.lib().ditree_forest_fallback_goals_ant(ctx._h, C.byref(forest.tree.desc), C.byref(forest.fdesc), gp,
                                                                   out.data_ptr(), ctx.stream), "forest_fallback_goals_ant")
    got = [int(v) if v < 0 else int(v) - t * CAP for t, v in enumerate(out.cpu().numpy())]
    assert got == ref
    assert sum(v > 0 for v in ref) >= T // 2
    # the engine's surface: each tree against its own scene's goal_state
    ref = [None if n < 2 else 1 + int(np.argmin(norm_rule(xy[t * CAP + 1:t * CAP + n], scenes[t][2][:2]))) for t, n in enumerate(sizes)]
    assert forest.fallback_nodes() == ref
