"""CPU: the scene-forest C-ABI is declared, bound and exported, its ctypes descriptor matches the header, the atlas stores every
distinct maze of the scenario set once, the scenario loader gives the reference's starts and goals, and plan_scenario_runs
refuses what it does not cover before touching a GPU."""
import ctypes as C
import csv
import os
import re
import types

import numpy as np
import pytest

from tests.util import DATA, REPO

SCENE_CALLS = ["ditree_upload_scenes", "ditree_forest_expand_round_scenes", "ditree_forest_fallback_goals"]


def test_scene_symbols_declared_bound_and_exported():
    from ditreeonlineplanner_amd import _lib
    hdr = open(os.path.join(REPO, "include", "ditree.h")).read()
    for name in SCENE_CALLS:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(_lib.lib(), name), name
    assert _lib.lib().ditree_version() == 400
    assert int(re.search(r"#define DITREE_MAX_SCENES (\d+)", hdr).group(1)) == _lib.MAX_SCENES
    assert int(re.search(r"#define DITREE_MAX_ATLAS_CELLS (\d+)", hdr).group(1)) == _lib.MAX_ATLAS_CELLS


def test_scene_descriptor_layout_matches_the_header():
    from ditreeonlineplanner_amd import _lib
    hdr = open(os.path.join(REPO, "include", "ditree.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} ditree_forest_scenes;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(const\s+)?(int32_t)\s*(\*?)\s*(\w+);", body)
    assert [f[3] for f in fields] == [n for n, _ in _lib.ForestScenes._fields_] == ["tree_scene", "tree_scene_host"]
    assert all(f[2] == "*" for f in fields)
    assert C.sizeof(_lib.ForestScenes) == 16 and _lib.ForestScenes.tree_scene_host.offset == 8


def _expected_scenarios():
    """run_scenarios.py:207-246 for the car, written out: cell centre x = (col + 0.5) - W / 2, y = H / 2 - (row + 0.5)."""
    out = []
    with open(os.path.join(DATA, "test_scenarios_car.csv"), newline="") as f:
        rows = csv.reader(f)
        next(rows)
        for name, maze_name, sr, sc, deg, gr, gc in rows:
            maze = np.loadtxt(os.path.join(DATA, f"{maze_name}.csv"), delimiter=",")
            H, W = maze.shape

            def xy(r, c):
                return (int(c) + 0.5) - W / 2, H / 2 - (int(r) + 0.5)
            out.append((name, maze, np.array([*xy(sr, sc), np.deg2rad(float(deg)), 0, 0, 0]), np.array([*xy(gr, gc), 0, 0, 0, 0])))
    return out


def test_car_scenarios_give_the_reference_starts_and_goals():
    from ditreeonlineplanner_amd.scenarios import car_scenarios
    got = car_scenarios()
    want = _expected_scenarios()
    assert len(got) == len(want) == 15
    for g, (name, maze, start, goal) in zip(got, want):
        assert g["name"] == name
        assert np.array_equal(g["maze"], maze)
        assert np.array_equal(g["start"], start), name
        assert np.array_equal(g["goal"], goal), name


def test_car_scenarios_skip_a_row_whose_maze_is_missing(tmp_path):
    from ditreeonlineplanner_amd.scenarios import car_scenarios
    p = tmp_path / "s.csv"
    p.write_text("scenario_name,maze_name,start_row,start_col,start_deg,goal_row,goal_col\n"
                 "a,boxes,17,2,45,2,17\nb,no_such_maze,1,1,0,2,2\n")
    got = car_scenarios(str(p))
    assert [g["name"] for g in got] == ["a"]


def test_atlas_stores_each_distinct_maze_once():
    from ditreeonlineplanner_amd.forest import atlas_layout, cell_codes
    from ditreeonlineplanner_amd.scenarios import car_scenarios
    sc = car_scenarios()
    mazes = [s["maze"] for s in sc]
    off, dims, cells = atlas_layout(mazes)
    # seven distinct mazes: Race_Track 7x13, random_xlarge 13x13, narrow_short 6x11, boxes 20x20, shapes 21x24, random_large 9x12,
    # random_huge 31x31 -- 2 299 cells, each stored at its first scene's offset
    assert cells == 91 + 169 + 66 + 400 + 504 + 108 + 961 == 2299
    assert [tuple(d) for d in dims] == [m.shape for m in mazes]
    first = {}
    used = 0
    for s, o, m in zip(sc, off, mazes):
        if s["maze_name"] not in first:
            first[s["maze_name"]] = used
            used += m.size
        assert o == first[s["maze_name"]], s["name"]
    assert used == cells
    # identical codes share bytes, a single changed cell does not; the codes follow ditree_upload_maze's rule
    a = np.zeros((3, 4))
    b = a.copy()
    b[1, 2] = 1
    off, _, cells = atlas_layout([a, b, a.copy(), a.reshape(4, 3)])
    assert list(off) == [0, 12, 0, 24] and cells == 36
    assert list(cell_codes(np.array([[0.0, 1.0, 2.5, -1.0, 300.0]]))[0]) == [0, 1, 255, 255, 255]


# ---------------------------------------------------------------------- plan_scenario_runs argument rules (no GPU)
def _fake(**kw):
    eng = types.SimpleNamespace(A=8, P=64, lm_n=20, lm_scale=0.2, s_global=1.0, k_steps=1, norm=np.arange(16.0), sticky=1,
                                early_exit=1, schedule=[64])
    p = types.SimpleNamespace(is_ant=False, run_type=0, world_size=1, sampler=SAMPLER, ctx=CTX, batch=16, _engine=eng)
    for k, v in kw.items():
        if hasattr(eng, k):
            setattr(eng, k, v)
        else:
            setattr(p, k, v)

    def reset(*a, **k):
        raise AssertionError("plan_scenario_runs touched a planner before refusing")
    p.reset = reset
    return p


SAMPLER = types.SimpleNamespace(sample_round=None)
CTX = object()


def test_plan_scenario_runs_refuses_without_touching_the_gpu():
    from ditreeonlineplanner_amd.planners.RRT import plan_scenario_runs
    with pytest.raises(NotImplementedError, match="car"):
        plan_scenario_runs([_fake(), _fake(is_ant=True)], [[1], [2]])
    with pytest.raises(NotImplementedError, match="run_type 0"):
        plan_scenario_runs([_fake(), _fake(run_type=2)], [[1], [2]])
    with pytest.raises(NotImplementedError, match="one rank"):
        plan_scenario_runs([_fake(world_size=2)], [[1]])
    with pytest.raises(NotImplementedError, match="plain-callable"):
        plan_scenario_runs([_fake(sampler=lambda *a: None)], [[1]])
    with pytest.raises(ValueError, match="one list per planner"):
        plan_scenario_runs([_fake(), _fake()], [[1]])
    for kw, name in ((dict(sampler=types.SimpleNamespace(sample_round=None)), "sampler"), (dict(ctx=object()), "ctx"),
                     (dict(A=16), "action_horizon"), (dict(P=32), "pred_horizon"), (dict(lm_n=16), "local map size"),
                     (dict(lm_scale=0.8), "local map scale"), (dict(s_global=4.0), "s_global"), (dict(k_steps=4), "k_steps"),
                     (dict(norm=np.ones(16)), "norm"), (dict(sticky=0), "emulate_sticky_done"), (dict(early_exit=0), "early_exit"),
                     (dict(schedule=[32, 64]), "prop_duration"), (dict(batch=8), "batch")):
        with pytest.raises(ValueError, match=f"planner 2 differs from planner 0 in {name}"):
            plan_scenario_runs([_fake(), _fake(), _fake(**kw)], [[1], [2], [3]])
    # the first difference is the one named
    with pytest.raises(ValueError, match="in action_horizon"):
        plan_scenario_runs([_fake(), _fake(A=16, batch=8)], [[1], [2]])
    assert plan_scenario_runs([], []) == []


# ---------------------------------------------------------------------- generated code of the scene kernels
def _function(text, name):
    start = text.index(name + ":")
    return text[start:text.index(".Lfunc_end", start)].splitlines()


def _loop_lines(body):
    """Every line of a basic block that the compiler marks as part of a loop ('Loop Header' / 'in Loop:' on its label)."""
    out, inside = [], False
    for line in body:
        if re.match(r"\s*(\.LBB\w+:|; %bb\.\d+:)", line):
            inside = "Loop Header" in line or "in Loop:" in line
        elif inside:
            out.append(line)
    return out


def test_scene_kernels_spill_nothing_and_load_their_scene_outside_the_step_loop(tmp_path):
    """The scene instantiations of the rollout (every G / LOCKSTEP / STAGE) and the scene local map have no scratch traffic, and
    the rollout reads a lane's scene record before its step loop: its loops hold exactly the global loads of the single-maze
    instantiation (the design rule of car_rollout_kernel -- nothing fetched per step but the staged action burst)."""
    import subprocess
    src = os.path.join(REPO, "ditreeonlineplanner_amd", "csrc", "geom_kernels.hip")
    out = tmp_path / "gk.s"
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "-S", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", src,
                    "-o", str(out)], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    text = out.read_text()
    tail = "EEvPKhiiPdPKdlPiiiddS2_14ditree_stridesS2_S6_S5_lS5_S2_PhPKiiS9_i12ChunkStrides"
    n = 0
    for g in (1, 2):
        for lock in (0, 1):
            for stage in (0, 1):
                scn = _function(text, f"_Z18car_rollout_kernelILi{g}ELb{lock}ELb{stage}ELb1{tail}")
                one = _function(text, f"_Z18car_rollout_kernelILi{g}ELb{lock}ELb{stage}ELb0{tail}")
                assert not any("scratch_" in l for l in scn), (g, lock, stage)
                loads = [sum(bool(re.search(r"\bglobal_load", l)) for l in _loop_lines(b)) for b in (scn, one)]
                assert loads[0] == loads[1], (g, lock, stage, loads)
                assert any("ds_read" in l or "ds_load" in l for l in scn)       # the maze is read from LDS
                n += 1
    assert n == 8
    lm = _function(text, "_Z16local_map_kernelILb1EEvPKhiiPKdiPKiS5_i7AxisArgdiPf")
    assert not any("scratch_" in l for l in lm)
