"""Per-run random streams and the run scheduler of ``RRT_Planner.plan_runs`` / ``plan_scenario_runs``: run i draws what ``random.seed(s); np.random.seed(s);
torch.manual_seed(s); planner.reset(); planner.plan()`` draws, s = seeds[i], while several runs share one forest.

The reference draws its samples from the GLOBAL ``random`` / ``np.random`` generators (planners/base_planner.py:162-207,
planners/RRT.py:134-140,153-156), and ``planners/_draw.py`` works on them too.  So each run keeps its own two states and swaps
them in around its draws; the caller's states are put back when ``plan_runs`` returns.  The start noise (and the DDPM step
noise) of a run comes from its own device ``torch.Generator``, seeded as ``torch.manual_seed(s)`` seeds the default one, and
is drawn with the same shapes in the same order as ``plan()`` draws it.  ``run_jobs`` is the scheduler both forests share; it
touches the engine only through its public surface and takes the device as an argument, so it runs on the CPU on stubs.
"""
from __future__ import annotations

import random
import time
from contextlib import contextmanager
from typing import NamedTuple

import numpy as np


class RunStreams:
    """The generator states one seeded run owns.  ``device``: where its torch generator lives (None: no torch generator)."""

    def __init__(self, seed, device=None):
        self.seed = int(seed)
        self.py = random.Random(self.seed).getstate()                 # what random.seed(s) leaves
        self.np = np.random.RandomState(self.seed).get_state()        # what np.random.seed(s) leaves
        self.gen = None
        if device is not None:
            import torch
            self.gen = torch.Generator(device=device)
            self.gen.manual_seed(self.seed)                            # what torch.manual_seed(s) leaves on that device

    @contextmanager
    def active(self):
        """The global ``random`` / ``np.random`` hold this run's states inside the block; the run keeps where they end."""
        random.setstate(self.py)
        np.random.set_state(self.np)
        try:
            yield self
        finally:
            self.py = random.getstate()
            self.np = np.random.get_state()


@contextmanager
def caller_states_kept():
    """Whatever runs inside, the caller's global ``random`` / ``np.random`` states are restored on the way out."""
    py, npst = random.getstate(), np.random.get_state()
    try:
        yield
    finally:
        random.setstate(py)
        np.random.set_state(npst)


def draw_runs(draws, streams, sizes):
    """One round of several runs: ``draws[i](B) -> (samples, cond_goals)`` on the global generators (run i's own planner's
    ``RRT_Planner.draw_round``), called for every run with ``sizes[i] > 0`` under that run's states.  -> list of (s, c) or
    None per run.  The caller keeps its own states around the whole loop (``caller_states_kept``)."""
    out = []
    for draw, st, B in zip(draws, streams, sizes):
        if B <= 0:
            out.append(None)
            continue
        with st.active():
            out.append(draw(int(B)))
    return out


class Job(NamedTuple):
    """One seeded run of a forest: ``planner`` draws for it and owns its budgets, ``slot`` = (container, index) receives its
    result dict, ``reset_args`` are the extra arguments of the engine's ``reset_tree`` (none in a plain forest, the scene id
    in a scene forest)."""
    planner: object
    seed: int
    slot: tuple
    reset_args: tuple = ()


def run_jobs(eng, jobs, batch, device):
    """The run scheduler of ``RRT_Planner.plan_runs`` and ``plan_scenario_runs``: ``jobs`` in queue order on the trees of the
    forest engine ``eng``, at most ``eng.T`` in flight, a finished run's tree taking the next job.  Every round gives each
    active run min(batch, what is left of its planner's max_candidates) candidates, drawn through its planner's
    ``draw_round`` on its own streams, and the noise of its own generator in ``plan()``'s order (start noise, then the DDPM
    step noise); ``time_budget`` counts from the run's own start.  Fills every job's slot with a ``plan_runs``-shaped dict,
    adds the summed collision-check count to ``common.map_utils.cc_calls`` once, leaves the caller's ``random`` /
    ``np.random`` states as they were, and returns the dicts in job order.

    Ant jobs (``planner.is_ant``; an ``AntForestEngine``): with tape dynamics every run's
    ``next_obs_tape_fn(the run's first candidate, n)`` rows, concatenated in tree order, go to ``expand_round``; and since
    ``is_colliding_ant`` does not count its calls (``plan()`` adds nothing for the ant) the runs report ``cc_calls`` 0 and
    ``common.map_utils.cc_calls`` stays as it is.

    ``planner.solution`` (one value for all jobs): with "first" and "best_of_round" a run finishes with its first goal-reaching
    round, with "anytime" on its own budgets only; a finished run's node is its tree's goal node -- for the two new modes the
    incumbent -- else the fallback.  Every dict carries ``solutions`` (goal nodes appended) and ``first_solution_candidates``
    (the run's candidates up to and including its first goal-reaching round, or None).  "anytime_pruned" is "anytime" with one
    more ending: a run whose tree has no open node left after a round (``eng.exhausted(t)``) finishes there with its incumbent,
    and its tree takes the next job; its dict carries ``pruned_candidates``, ``closed_nodes`` and ``bound_exhausted`` too.
    ``planner.sparse_cell`` (one value for all jobs): every dict carries ``dominated_candidates``, ``retired_nodes`` and
    ``active_nodes`` of its tree as of the run's last accept."""
    import torch
    from ..common import map_utils
    from ..engine import ANYTIME, CNT_GOAL, CNT_ITERS
    if not jobs:
        return []
    T = eng.T
    network = hasattr(jobs[0].planner.sampler, "ensure_bound")
    ant = bool(getattr(jobs[0].planner, "is_ant", False))
    tape = ant and getattr(jobs[0].planner, "ant_dynamics", "host") == "tape"
    K = len(eng.ddpm[0]) if (network and eng.ddpm is not None) else 0
    solution = getattr(jobs[0].planner, "solution", "first")
    first = solution == "first"
    anytime = solution in ANYTIME
    pruned = solution == "anytime_pruned"
    sparse = getattr(jobs[0].planner, "sparse_cell", None) is not None
    results = [None] * len(jobs)
    queue = list(range(len(jobs)))[::-1]
    slots = [None] * T                    # per tree: [job index, RunStreams, drawn, start time, first_solution_candidates]
    steps_dev = torch.zeros(T, dtype=torch.int64, device=device)
    solutions_dev = None if first else torch.zeros(T, dtype=torch.int64, device=device)
    total_cc = 0

    def start(t):
        slots[t] = None
        if queue:
            i = queue.pop()
            eng.reset_tree(t, *jobs[i].reset_args)
            steps_dev[t] = 0
            if not first:
                solutions_dev[t] = 0
            slots[t] = [i, RunStreams(jobs[i].seed, device), 0, time.time(), None]

    def finish(t, goal):
        nonlocal total_cc
        i, _, _, t0, first_at = slots[t]
        job = jobs[i]
        row = eng.counters(t)
        node = goal if goal is not None else eng.fallback_node(t)          # RRT.py:227-254
        elapsed = time.time() - t0
        path = actions = None
        if node is not None:
            path, actions = eng.path_to(t, node)
        cc = 0 if ant else int(steps_dev[t].item())          # is_colliding_ant does not count its calls (map_utils.py:126-136)
        total_cc += cc
        results[i] = job.slot[0][job.slot[1]] = {
            "seed": job.seed, "success": path is not None, "goal_reached": goal is not None, "iterations": int(row[CNT_ITERS]),
            "time": elapsed, "path": path, "actions": actions, "number_of_nodes": int(eng.n_nodes_host[t]),
            "path_time": None if path is None else len(path) * job.planner.env_dt, "cc_calls": cc,
            "solutions": (0 if goal is None else 1) if first else int(solutions_dev[t].item()),
            "first_solution_candidates": first_at}
        if pruned:
            results[i].update(pruned_candidates=eng.pruned_candidates(t), closed_nodes=eng.closed_nodes(t),
                              bound_exhausted=bool(eng.exhausted(t)))
        if sparse:
            results[i].update(dominated_candidates=eng.dominated_candidates(t), retired_nodes=eng.retired_nodes(t),
                              active_nodes=eng.active_nodes(t))
        start(t)

    with caller_states_kept():
        for t in range(T):
            start(t)
        while True:
            # the loop head of plan(): a run goes on while its own wall-clock budget and candidate budget last
            sizes = [0] * T
            for t in range(T):
                while slots[t] is not None:
                    i, _, drawn, t0, _ = slots[t]
                    pl = jobs[i].planner
                    if (time.time() - t0) < pl.time_budget and (pl.max_candidates is None or drawn < pl.max_candidates):
                        sizes[t] = batch if pl.max_candidates is None else min(batch, pl.max_candidates - drawn)
                        break
                    finish(t, None if first else eng.goal_node(t))          # the budgets ended: an anytime run's incumbent
            if not any(sizes):
                break
            active = [t for t in range(T) if sizes[t] > 0]
            planners = [jobs[slots[t][0]].planner for t in active]
            drawn_sc = draw_runs([pl.draw_round for pl in planners], [slots[t][1] for t in active], [sizes[t] for t in active])
            s = torch.as_tensor(np.concatenate([d[0] for d in drawn_sc]), device=device)
            c = torch.as_tensor(np.concatenate([d[1] for d in drawn_sc]), device=device)
            B = int(sum(sizes))
            noise = acts = step_noise = None
            if network:
                noise = torch.empty((B, eng.n_chunks, eng.P, eng.ACTION_DIM), dtype=torch.float32, device=device)
                if K:
                    step_noise = torch.empty((B, eng.n_chunks, K, eng.P, eng.ACTION_DIM), dtype=torch.float32, device=device)
                lo = 0
                for t in active:
                    g = slots[t][1].gen
                    noise[lo:lo + sizes[t]].normal_(generator=g)
                    if K:
                        step_noise[lo:lo + sizes[t]].normal_(generator=g)
                    lo += sizes[t]
            else:
                acts = torch.cat([pl._host_actions(slots[t][2], sizes[t]) for pl, t in zip(planners, active)])
            extra = {}                                          # the ant engine's own keyword arguments, for ant jobs only
            if tape:
                extra["next_obs_tape"] = torch.as_tensor(np.ascontiguousarray(np.concatenate(
                    [pl._tape_fn(slots[t][2], sizes[t]) for pl, t in zip(planners, active)])), device=device)
            cnt = eng.expand_round(s, c, noise=noise, inject_actions=acts, counts_per_tree=sizes, step_noise=step_noise, **extra)
            if not ant:
                tree_of = torch.as_tensor(np.repeat(np.arange(T), sizes), device=device)
                steps_dev.index_add_(0, tree_of, eng.rb.chunk_steps[:B].sum(dim=1, dtype=torch.int64))
            if not first:
                solutions_dev += eng.round_solutions(B)
            for t in active:
                slots[t][2] += sizes[t]
                if int(cnt[t, CNT_GOAL]) >= 0:
                    if slots[t][4] is None:
                        slots[t][4] = slots[t][2]
                    if not anytime or (pruned and eng.exhausted(t)):
                        finish(t, eng.goal_node(t))
    if not ant:
        map_utils.add_cc_calls(total_cc)        # the counter the drivers read (run_scenarios.py:338,343), once
    return results


def check_forest_scope(pl, who):
    """What a planner must be to join a forest (``who``: the refusing function's name, for its messages)."""
    if pl.is_ant:
        if getattr(pl, "ant_dynamics", "host") not in ("model", "tape"):
            raise NotImplementedError(f"{who}: the car (carmaze), or the ant with ant_dynamics 'model' or 'tape' -- with "
                                      "ant_dynamics='host' the caller's simulator steps one candidate at a time on the host, "
                                      "so it bounds such a run and a forest buys nothing there")
    if pl.run_type != 0:
        raise NotImplementedError(f"{who}: run_type 0 only (the online re-planning driver plans one run at a time)")
    if pl.world_size > 1:
        raise NotImplementedError(f"{who}: one rank (a forest is not sharded)")
    if not hasattr(pl.sampler, "ensure_bound") and not hasattr(pl.sampler, "sample_round"):
        raise NotImplementedError(f"{who}: a plain-callable sampler draws from its own generator and cannot be split per run; "
                                  "give it a sample_round(first_candidate, B, n_chunks, pred_horizon) method")
