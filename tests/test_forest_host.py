"""CPU: the forest C-ABI is declared, bound and exported, its ctypes descriptor matches the header, and the per-run random
streams of RRT_Planner.plan_runs draw what sequential seeded runs draw while leaving the caller's generators alone; the run
scheduler both forests share (planners/_runs.py run_jobs) on a stub engine and stub planners."""
import ctypes as C
import os
import random
import re
import types

import numpy as np
import pytest

from ditreeonlineplanner_amd.planners import RRT as F
from ditreeonlineplanner_amd.planners._runs import Job, RunStreams, caller_states_kept, draw_runs, run_jobs
from tests.test_draw_round import fake_planner, same_state, states
from tests.util import REPO

FOREST_CALLS = ["ditree_forest_expand_round", "ditree_forest_accept", "ditree_forest_chunk_budget", "ditree_forest_nn_argmin",
                "ditree_forest_fallback"]


def test_forest_symbols_declared_bound_and_exported():
    from ditreeonlineplanner_amd import _lib
    hdr = open(os.path.join(REPO, "include", "ditree.h")).read()
    for name in FOREST_CALLS:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(_lib.lib(), name), name
    assert _lib.lib().ditree_version() == 400


def test_forest_descriptor_layout_matches_the_header():
    from ditreeonlineplanner_amd import _lib
    hdr = open(os.path.join(REPO, "include", "ditree.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} ditree_forest;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(const\s+)?(int32_t)\s*(\*?)\s*(\w+);", body)
    assert [f[3] for f in fields] == [n for n, _ in _lib.Forest._fields_]
    for (_, _, star, name), (_, ctype) in zip(fields, _lib.Forest._fields_):
        if star:
            assert ctype in (C.c_void_p, C.POINTER(C.c_int32)), name
        else:
            assert ctype is C.c_int32, name
    assert C.sizeof(_lib.Forest) == 4 + 4 + 3 * 8
    assert _lib.Forest.counters.offset == 8 and _lib.Forest.off_host.offset == 24


def _planner():
    p = fake_planner(0)
    p.draw_round = types.MethodType(F.RRT_Planner.draw_round, p)
    return p


def test_run_streams_start_where_seeding_the_globals_leaves_them():
    with caller_states_kept():
        random.seed(17)
        np.random.seed(17)
        want = states()
    st = RunStreams(17)
    with caller_states_kept():
        with st.active():
            assert same_state(states(), want)


def test_per_run_draws_equal_sequential_seeded_draws_and_keep_the_caller_states():
    """Three runs with uneven rounds (incl. 0 and 1 candidates, bulk and single draws) interleaved round by round: each run's
    samples and conditioning goals equal what a sequential run seeded with its seed draws, round for round."""
    p = _planner()
    seeds = [3, 7, 11]
    rounds = [[5, 1, 0], [2, 4, 3], [0, 1, 6], [9, 0, 1]]
    random.seed(99)
    np.random.seed(99)
    caller = states()
    streams = [RunStreams(s) for s in seeds]
    got = [[] for _ in seeds]
    with caller_states_kept():
        for sizes in rounds:
            for i, d in enumerate(draw_runs([p.draw_round] * len(seeds), streams, sizes)):
                if d is not None:
                    got[i].append(d)
    assert same_state(states(), caller)
    for i, s in enumerate(seeds):
        random.seed(s)
        np.random.seed(s)
        want = [p.draw_round(r[i]) for r in rounds if r[i] > 0]
        assert len(want) == len(got[i])
        for (ws, wc), (gs, gc) in zip(want, got[i]):
            assert np.array_equal(ws, gs) and np.array_equal(wc, gc)
        end = states()
        with caller_states_kept():
            with streams[i].active():
                assert same_state(states(), end)          # the run's streams sit where the sequential run's do


def test_plan_runs_refuses_without_touching_the_gpu():
    def stub(**kw):
        p = types.SimpleNamespace(is_ant=False, run_type=0, world_size=1, sampler=types.SimpleNamespace(sample_round=None))
        p.__dict__.update(kw)
        return p
    with pytest.raises(NotImplementedError, match="car"):
        F.RRT_Planner.plan_runs(stub(is_ant=True), [1])
    with pytest.raises(NotImplementedError, match="run_type 0"):
        F.RRT_Planner.plan_runs(stub(run_type=2), [1])
    with pytest.raises(NotImplementedError, match="one rank"):
        F.RRT_Planner.plan_runs(stub(world_size=2), [1])
    with pytest.raises(NotImplementedError, match="plain-callable"):
        F.RRT_Planner.plan_runs(stub(sampler=lambda *a: None), [1])


# ---------------------------------------------------------------------- the run scheduler on stubs
class StubPlanner:
    """What run_jobs reads of a planner.  Draws come from the global generators; ``tag`` marks whose draw_round / _host_actions
    produced a row."""

    def __init__(self, tag, max_candidates, env_dt):
        self.tag, self.max_candidates, self.env_dt, self.time_budget = tag, max_candidates, env_dt, 600.0
        self.sampler = types.SimpleNamespace(sample_round=None)

    def draw_round(self, B):
        s = np.random.rand(B, 6)
        c = np.array([[random.random(), self.tag] for _ in range(B)])
        return s, c

    def _host_actions(self, first, B):
        import torch
        a = torch.zeros(B, 2, 4, 2, dtype=torch.float64)
        a[:, 0, 0, 0] = torch.arange(first, first + B)
        a[:, 0, 0, 1] = self.tag
        return a


class StubEngine:
    """The public surface run_jobs uses of a forest engine: every candidate becomes a node and costs two iterations and
    chunk_steps (3, tree + 1); the run reset with ``goal_tag`` reaches the goal (node 7) in its second round."""
    T, n_chunks, P, ACTION_DIM, ddpm = 2, 2, 4, 2, None

    def __init__(self, goal_tag):
        import torch
        self.goal_tag = goal_tag
        self.rb = types.SimpleNamespace(chunk_steps=torch.zeros(8, 2, dtype=torch.int32))
        self.n_nodes_host = np.ones(2, dtype=np.int64)
        self.iters, self.rounds_of, self.tag_of, self.goal = [0, 0], [0, 0], [None, None], [None, None]
        self.resets, self.rounds = [], []

    def reset_tree(self, t, *args):
        self.resets.append((t, args))
        self.tag_of[t], self.iters[t], self.rounds_of[t], self.goal[t] = args[0], 0, 0, None
        self.n_nodes_host[t] = 1

    def expand_round(self, s, c, noise=None, inject_actions=None, counts_per_tree=None, step_noise=None):
        assert noise is None and step_noise is None
        self.rounds.append((list(counts_per_tree), s.numpy().copy(), c.numpy().copy(), inject_actions.numpy().copy(),
                            list(self.tag_of)))
        cnt = np.zeros((2, 8), dtype=np.int32)
        cnt[:, 1] = -1
        lo = 0
        for t, n in enumerate(counts_per_tree):
            if n:
                self.rounds_of[t] += 1
                self.iters[t] += 2 * n
                self.n_nodes_host[t] += n
                self.rb.chunk_steps[lo:lo + n, 0] = 3
                self.rb.chunk_steps[lo:lo + n, 1] = t + 1
                lo += n
                if self.tag_of[t] == self.goal_tag and self.rounds_of[t] == 2:
                    self.goal[t] = 7
                    cnt[t, 1] = 1000 + t
        return cnt

    def counters(self, t):
        row = np.zeros(8, dtype=np.int32)
        row[3] = self.iters[t]
        return row

    def goal_node(self, t):
        return self.goal[t]

    def fallback_node(self, t):
        return int(self.n_nodes_host[t]) - 1

    def path_to(self, t, node):
        return np.zeros((node + 1, 6), dtype=np.float32), np.zeros((node, 2), dtype=np.float32)


def test_run_loop_on_a_stub_engine_and_stub_planners(monkeypatch):
    """Five jobs of two planners (max_candidates 5 and 12 at batch 4) on two trees, on the CPU: queue order, slot reuse, the
    extra reset_tree arguments, each round's counts, each run's own draws and candidate offsets in tree order, goal and
    fallback endings, the per-job results, the caller's generator states and the single add_cc_calls."""
    from ditreeonlineplanner_amd.common import map_utils
    added = []
    monkeypatch.setattr(map_utils, "add_cc_calls", added.append)
    pa, pb = StubPlanner(100.0, 5, 0.1), StubPlanner(200.0, 12, 0.25)
    eng = StubEngine(goal_tag="d")
    out = [None] * 5
    spec = [(pa, 10, "a"), (pb, 11, "b"), (pa, 12, "c"), (pb, 13, "d"), (pa, 14, "e")]
    jobs = [Job(pl, seed, (out, i), (tag,)) for i, (pl, seed, tag) in enumerate(spec)]
    random.seed(99)
    np.random.seed(99)
    caller = states()
    res = run_jobs(eng, jobs, 4, "cpu")
    assert same_state(states(), caller)
    assert res == out and all(r is not None for r in out)
    # queue order; a finished tree takes the next job with that job's reset_tree arguments
    assert eng.resets == [(0, ("a",)), (1, ("b",)), (0, ("c",)), (1, ("d",)), (0, ("e",))]
    # min(batch, what is left) for active runs, 0 for the idle tree once the queue is empty
    assert [r[0] for r in eng.rounds] == [[4, 4], [1, 4], [4, 4], [1, 4], [4, 4], [1, 0]]
    # the rows of every round: each run's own seeded draws through its own planner, and its own candidate offsets, in tree order
    by_tag = {tag: (pl, seed) for pl, seed, tag in spec}
    want, drawn = {}, {tag: 0 for tag in by_tag}
    with caller_states_kept():
        for tag, (pl, seed) in by_tag.items():
            random.seed(seed)
            np.random.seed(seed)
            left, want[tag] = pl.max_candidates if tag != "d" else 8, []
            while left:
                want[tag].append(pl.draw_round(min(4, left)))
                left -= min(4, left)
    for counts, s, c, acts, tags in eng.rounds:
        lo = 0
        for t, n in enumerate(counts):
            if n:
                ws, wc = want[tags[t]].pop(0)
                assert np.array_equal(s[lo:lo + n], ws) and np.array_equal(c[lo:lo + n], wc), (tags[t], lo)
                assert np.array_equal(acts[lo:lo + n, 0, 0, 0], np.arange(drawn[tags[t]], drawn[tags[t]] + n))
                assert (acts[lo:lo + n, 0, 0, 1] == by_tag[tags[t]][0].tag).all()
                drawn[tags[t]] += n
                lo += n
        assert lo == len(s) == len(c) == len(acts)
    assert all(not w for w in want.values())
    # results: from the job's own tree and planner
    cands = [5, 12, 5, 8, 5]
    tree = [0, 1, 0, 1, 0]
    for i, (r, (pl, seed, tag)) in enumerate(zip(out, spec)):
        assert r["seed"] == seed and r["success"] and r["goal_reached"] == (tag == "d")
        assert r["iterations"] == 2 * cands[i] and r["number_of_nodes"] == cands[i] + 1
        node = 7 if tag == "d" else cands[i]                      # the goal node, else the fallback node (the last one)
        assert len(r["path"]) == node + 1 and len(r["actions"]) == node
        assert r["path_time"] == (node + 1) * pl.env_dt
        assert r["cc_calls"] == cands[i] * (3 + tree[i] + 1)
        assert r["time"] >= 0.0
    assert added == [sum(r["cc_calls"] for r in out)] == [20 + 60 + 20 + 40 + 20]
