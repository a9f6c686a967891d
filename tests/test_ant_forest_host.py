"""CPU: the ant forest C-ABI is declared, bound and exported; which planners ``check_forest_scope`` admits; and the ant branch
of the run scheduler (planners/_runs.py run_jobs) on a stub ant engine and stub ant planners: per-run tape slices by each
run's own candidate offset in tree order, no collision-check count, the caller's generator states."""
import os
import random
import re
import types

import numpy as np
import pytest

from ditreeonlineplanner_amd.planners._runs import Job, check_forest_scope, run_jobs
from tests.test_draw_round import same_state, states
from tests.util import REPO

ANT_FOREST_CALLS = ["ditree_forest_expand_round_ant", "ditree_forest_accept_ant", "ditree_forest_fallback_ant"]


def test_ant_forest_symbols_declared_bound_and_exported():
    from ditreeonlineplanner_amd import _lib
    hdr = open(os.path.join(REPO, "include", "ditree.h")).read()
    for name in ANT_FOREST_CALLS:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(_lib.lib(), name), name
    assert _lib.lib().ditree_version() == 400


def _stub(**kw):
    p = types.SimpleNamespace(is_ant=True, run_type=0, world_size=1, sampler=types.SimpleNamespace(sample_round=None))
    p.__dict__.update(kw)
    return p


def test_forest_scope_admits_the_ant_with_device_dynamics_only():
    check_forest_scope(_stub(ant_dynamics="model"), "plan_runs")
    check_forest_scope(_stub(ant_dynamics="tape"), "plan_runs")
    for refused in (_stub(ant_dynamics="host"), _stub()):               # no ant_dynamics: read as the default, "host"
        with pytest.raises(NotImplementedError, match="car") as e:
            check_forest_scope(refused, "plan_runs")
        assert "host" in str(e.value) and "plan_runs" in str(e.value)
    # the other rules hold for the ant as for the car
    with pytest.raises(NotImplementedError, match="run_type 0"):
        check_forest_scope(_stub(ant_dynamics="model", run_type=1), "plan_runs")
    with pytest.raises(NotImplementedError, match="one rank"):
        check_forest_scope(_stub(ant_dynamics="tape", world_size=2), "plan_runs")
    with pytest.raises(NotImplementedError, match="plain-callable"):
        check_forest_scope(_stub(ant_dynamics="model", sampler=lambda *a: None), "plan_runs")


def test_plan_scenario_runs_stays_the_cars():
    from ditreeonlineplanner_amd.planners.RRT import plan_scenario_runs
    for dyn in ("model", "tape"):
        with pytest.raises(NotImplementedError, match="car"):
            plan_scenario_runs([_stub(ant_dynamics=dyn)], [[1]])


# ---------------------------------------------------------------------- the run scheduler's ant branch on stubs
N_CHUNKS, A, P = 2, 2, 4


class StubAntPlanner:
    """What run_jobs reads of an ant planner with tape dynamics.  ``tag`` marks whose draw_round / _host_actions / tape
    function produced a row; the tape row of candidate k of this planner's run carries (k, tag)."""
    is_ant, ant_dynamics = True, "tape"

    def __init__(self, tag, max_candidates, env_dt):
        self.tag, self.max_candidates, self.env_dt, self.time_budget = tag, max_candidates, env_dt, 600.0
        self.sampler = types.SimpleNamespace(sample_round=None)
        self.tape_calls = []

    def draw_round(self, B):
        s = np.random.rand(B, 29)
        c = np.array([[random.random(), self.tag] for _ in range(B)])
        return s, c

    def _host_actions(self, first, B):
        import torch
        a = torch.zeros(B, N_CHUNKS, P, 8, dtype=torch.float64)
        a[:, 0, 0, 0] = torch.arange(first, first + B)
        a[:, 0, 0, 1] = self.tag
        return a

    def _tape_fn(self, first, B):
        self.tape_calls.append((first, B))
        tape = np.zeros((B, N_CHUNKS, A, 29))
        tape[:, 0, 0, 0] = np.arange(first, first + B)
        tape[:, 0, 0, 1] = self.tag
        return tape


class StubAntEngine:
    """The surface run_jobs uses of an AntForestEngine: every candidate becomes a node and costs two iterations; chunk_steps
    are filled (an ant run must not count them).  ``expand_round`` has the ant engine's keyword arguments."""
    T, n_chunks, P, ACTION_DIM, ddpm = 2, N_CHUNKS, P, 8, None

    def __init__(self):
        import torch
        self.rb = types.SimpleNamespace(chunk_steps=torch.full((8, N_CHUNKS), 5, dtype=torch.int32))
        self.n_nodes_host = np.ones(2, dtype=np.int64)
        self.iters, self.tag_of = [0, 0], [None, None]
        self.resets, self.rounds = [], []

    def reset_tree(self, t, *args):
        self.resets.append((t, args))
        self.tag_of[t], self.iters[t] = args[0], 0
        self.n_nodes_host[t] = 1

    def expand_round(self, s, c, noise=None, inject_actions=None, counts_per_tree=None, step_noise=None, accept=True,
                     next_obs_tape=None, cond_out=None):
        assert noise is None and step_noise is None and cond_out is None
        self.rounds.append((list(counts_per_tree), s.numpy().copy(), inject_actions.numpy().copy(), next_obs_tape.numpy().copy(),
                            list(self.tag_of)))
        cnt = np.zeros((2, 8), dtype=np.int32)
        cnt[:, 1] = -1
        for t, n in enumerate(counts_per_tree):
            self.iters[t] += 2 * n
            self.n_nodes_host[t] += n
        return cnt

    def counters(self, t):
        row = np.zeros(8, dtype=np.int32)
        row[3] = self.iters[t]
        return row

    def goal_node(self, t):
        return None

    def fallback_node(self, t):
        return int(self.n_nodes_host[t]) - 1

    def path_to(self, t, node):
        return np.zeros((node + 1, 29), dtype=np.float32), np.zeros((node, 8), dtype=np.float32)


def test_ant_run_loop_tape_slices_no_cc_calls_and_caller_states(monkeypatch):
    """Three ant jobs of two planners (max_candidates 5 and 9 at batch 4) on two trees: every round's tape is each active
    run's own ``next_obs_tape_fn(its first candidate, n)`` in tree order (so are the action rows), the runs report cc_calls 0
    and nothing is added to the module counter, and the caller's generator states are kept."""
    from ditreeonlineplanner_amd.common import map_utils
    added = []
    monkeypatch.setattr(map_utils, "add_cc_calls", added.append)
    before = map_utils.cc_calls
    pa, pb = StubAntPlanner(100.0, 5, 0.1), StubAntPlanner(200.0, 9, 0.25)
    eng = StubAntEngine()
    out = [None] * 3
    spec = [(pa, 10, "a"), (pb, 11, "b"), (pa, 12, "c")]
    jobs = [Job(pl, seed, (out, i), (tag,)) for i, (pl, seed, tag) in enumerate(spec)]
    random.seed(99)
    np.random.seed(99)
    caller = states()
    res = run_jobs(eng, jobs, 4, "cpu")
    assert same_state(states(), caller)
    assert res == out and all(r is not None for r in out)
    assert eng.resets == [(0, ("a",)), (1, ("b",)), (0, ("c",))]
    assert [r[0] for r in eng.rounds] == [[4, 4], [1, 4], [4, 1], [1, 0]]
    by_tag = {tag: pl for pl, _, tag in spec}
    drawn = {tag: 0 for tag in by_tag}
    for counts, s, acts, tape, tags in eng.rounds:
        assert tape.shape == (sum(counts), N_CHUNKS, A, 29)
        lo = 0
        for t, n in enumerate(counts):
            if n:
                first = drawn[tags[t]]
                assert np.array_equal(tape[lo:lo + n, 0, 0, 0], np.arange(first, first + n)), (tags[t], lo)
                assert (tape[lo:lo + n, 0, 0, 1] == by_tag[tags[t]].tag).all()
                assert np.array_equal(acts[lo:lo + n, 0, 0, 0], np.arange(first, first + n))
                drawn[tags[t]] += n
                lo += n
        assert lo == len(s) == len(acts) == len(tape)
    # the tape function was asked once per (run, round), with the run's own offset: runs a and c share planner pa
    assert pa.tape_calls == [(0, 4), (4, 1), (0, 4), (4, 1)] and pb.tape_calls == [(0, 4), (4, 4), (8, 1)]
    for r, cands in zip(out, [5, 9, 5]):
        assert r["success"] and not r["goal_reached"] and r["iterations"] == 2 * cands and r["number_of_nodes"] == cands + 1
        assert r["cc_calls"] == 0
    assert added == [] and map_utils.cc_calls == before
