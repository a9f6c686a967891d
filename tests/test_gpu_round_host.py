"""The host half of the planning rounds (csrc/ditree_api.hip) where no other test goes: the stepped ant API with early exit (its
own compaction step), its refusals out of order, and the per-context round scratch as rounds of both robots grow it in turn."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import ant as OA
from oracle import rrt as ORRT
from tests.test_gpu_ant_round import _engine, _model_inputs, ant_norm, dev
from tests.test_oracle_ant import trace_setup
from tests.util import load_maze

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -3            # include/ditree.h DITREE_E_ARG, DITREE_E_STATE


@pytest.fixture(scope="module")
def ctx():
    from ditreeonlineplanner_amd.ops import Context
    c = Context(0)
    yield c
    c.close()


def _draw_ant(B, goal_state, seed):
    tape = ORRT.RandomTape(seed)
    s, c = np.zeros((B, 29)), np.zeros((B, 2))
    for i in range(B):
        s[i], c[i] = OA.draw_candidate_ant(tape, 20, 20, 4.0, goal_state)
    return s, c


def _seed_nodes(eng, N0):
    """A synthetic snapshot as in test_ant_round_full_size_through_accept: N0 nodes in free cells of `boxes`, some 0.1 from a
    wall, with 3-row histories and previous actions."""
    rng = np.random.default_rng(11)
    _, nodes, _ = _model_inputs(N0, 1, seed=12)
    t = eng.tree
    nd = dev(nodes)
    t.state[:N0] = nd
    t.xy[:N0] = nd[:, :2]
    t.parent[:N0] = torch.arange(-1, N0 - 1, device="cuda", dtype=torch.int32).clamp(min=0)
    t.parent[0] = -1
    t.has_prev[1:N0] = 1
    t.last_action[1:N0] = dev(rng.uniform(-1, 1, (N0 - 1, 8)))
    hist = np.repeat(nodes[:, None, :], 3, axis=1)
    hist[:, :2, 7:] += rng.normal(0, 0.05, (N0, 2, 22))
    t.hist[:N0] = dev(hist)
    t.hist_n[:N0] = 3
    t.hist_n[0] = 1
    t.counters[0] = N0
    t.n_nodes_host = N0


def test_ant_host_stepped_round_with_early_exit_is_bit_identical(ctx):
    """dynamics='host' with early_exit: ditree_ant_chunk_sample compacts the alive candidates itself and both halves of the chunk
    run on that list.  The setup of test_ant_host_stepped_round_equals_the_model_round (RandomTape(7), noise seed 5) on a tree
    seeded with nodes next to walls -- from the trace's start alone the random network walks no candidate into a wall (60 pairs
    of seeds tried), and then no chunk runs on a compacted list.  The round's outputs and the tree equal the early_exit=False
    round bit for bit, and some chunk ran on 0 < n < B rows."""
    from ditreeonlineplanner_amd import _lib
    from ditreeonlineplanner_amd.engine import AntExpansionEngine
    from ditreeonlineplanner_amd.model import NoisePredNet
    g, pre, pl, atape, otape, m = trace_setup("model_boxes")
    net = NoisePredNet(input_dim=8, additional_global_cond_dim=97, pred_horizon=16, local_map_size=16, seed=0)
    net.bind(ctx, precision=_lib.PREC_F32, max_batch=32)
    B = 24
    s, c = _draw_ant(B, g[pre + "goal"], 7)
    noise = torch.randn(B, 24, 16, 8, generator=torch.Generator().manual_seed(5)).cuda()
    res, calls = [], []
    for ee in (False, True):
        calls.append([])

        def step_fn(chunk, start, actions, rows):
            calls[-1].append((chunk, rows.tolist()))
            cur, out = start.copy(), np.zeros((len(rows), 2, 29))
            for i in range(2):
                cur = OA.ant_model_step(cur, actions[:, i])
                out[:, i] = cur
            return out
        eng = AntExpansionEngine(ctx, m["maze"], g[pre + "start"], g[pre + "goal"], desired_goal=g[pre + "desired"], norm=ant_norm(),
                                 batch=B, capacity=256, dynamics="host", early_exit=ee)
        _seed_nodes(eng, 64)
        eng.expand_round(dev(s), dev(c), noise=noise, step_fn=step_fn)
        snap = eng.tree_snapshot()
        res.append([t[:B].cpu().numpy() for t in (eng.rb.status, eng.rb.chunk_steps, eng.rb.chunks_run, eng.rb.states, eng.rb.actions)] +
                   [snap["parents"], snap["states"], snap["counters"]])
    for a, b in zip(*res):
        assert np.array_equal(a, b)
    assert calls[0] == calls[1]
    assert calls[1][0] == (0, list(range(B)))
    assert any(0 < len(rows) < B for _, rows in calls[1]), [len(rows) for _, rows in calls[1]]    # the compacted list was used


def test_ant_stepped_api_out_of_order():
    """ditree_ant_chunk_sample / _chunk_step on a context that has seen no ditree_ant_round_begin, and chunk indices outside
    [0, n_chunks): refused by name, nothing launched."""
    from ditreeonlineplanner_amd import _lib
    from ditreeonlineplanner_amd.ops import Context
    g, pre, pl, atape, otape, m = trace_setup("model_boxes")
    L = _lib.lib()
    B = 4
    fresh = Context(0)
    try:
        eng = _engine(fresh, g, pre, m, B, "host")
        eng.ensure_maze()
        s, c = _draw_ant(B, g[pre + "goal"], 7)
        s, c = dev(s), dev(c)
        acts = dev(np.stack([atape.actions(np.arange(B), j) for j in range(eng.n_chunks)], axis=1))
        obs = torch.zeros(B, eng.A, 29, dtype=torch.float64, device="cuda")
        rp, keep = eng._params(s, c, None, acts, 0, B)
        rd = eng.rb.desc(0, B)
        h, t, st = fresh._h, C.byref(eng.tree.desc), fresh.stream
        eng.rb.status.fill_(-7)

        def sample(j):
            return L.ditree_ant_chunk_sample(h, t, C.byref(rd), C.byref(rp), j, st), L.ditree_last_error(h)

        def step(j):
            return L.ditree_ant_chunk_step(h, t, C.byref(rd), C.byref(rp), j, obs.data_ptr(), st), L.ditree_last_error(h)
        assert sample(0) == (E_STATE, b"ant_chunk_sample: call ditree_ant_round_begin first")
        assert step(0) == (E_STATE, b"ant_chunk_step: call ditree_ant_round_begin first")
        for j in (-1, eng.n_chunks):
            assert sample(j) == (E_ARG, b"ant_chunk_sample: chunk index out of range")
            assert step(j) == (E_ARG, b"ant_chunk_step: chunk index out of range")
        torch.cuda.synchronize()
        assert bool((eng.rb.status == -7).all()) and not bool(eng.rb.actions.any())
        del keep
    finally:
        fresh.close()


def _ant_tape_round(ctx, B):
    """One ant round of B candidates from the root on an action tape and an observation tape, cond_out requested (so the local
    map and the conditioning buffers are used): every output of the round and the tree."""
    g, pre, pl, atape, otape, m = trace_setup("tape_boxes")
    eng = _engine(ctx, g, pre, m, B, "tape")
    s, c = _draw_ant(B, g[pre + "goal"], 42)
    cand = np.arange(B)
    acts = np.stack([atape.actions(cand, j) for j in range(eng.n_chunks)], axis=1)
    cond = torch.zeros(B, eng.n_chunks, 97, dtype=torch.float32, device="cuda")
    eng.expand_round(dev(s), dev(c), inject_actions=dev(acts), next_obs_tape=dev(otape.rows(cand)), cond_out=cond)
    snap = eng.tree_snapshot()
    rb = eng.rb
    return [t.cpu().numpy() for t in (rb.status, rb.chunks_run, rb.chunk_steps, rb.parent, rb.end_state, rb.states, rb.actions, cond)] + \
           [snap["parents"], snap["states"], snap["counters"], eng.tree.hist[: len(snap["parents"])].cpu().numpy()]


def _car_tape_round(ctx, B):
    """One car round of B candidates from the root on an action tape."""
    from ditreeonlineplanner_amd.engine import ExpansionEngine
    from oracle import geometry as G
    maze = load_maze("boxes")
    start = np.array([*G.cell_rowcol_to_xy([17, 2], maze), np.deg2rad(45.0), 0, 0, 0])
    goal = np.array([*G.cell_rowcol_to_xy([2, 17], maze), 0, 0, 0, 0])
    eng = ExpansionEngine(ctx, maze, start, goal, edge_length=32, action_horizon=8, batch=B, capacity=256)
    samples, cond = ORRT.RandomTape(42).draw_round(B, maze.shape[1], maze.shape[0], goal)
    rng = np.random.default_rng(9)
    acts = np.stack([rng.normal(0.45, 1.0, (B, eng.n_chunks, eng.P)), rng.normal(0.0, 0.92, (B, eng.n_chunks, eng.P))], axis=3).copy()
    eng.expand_round(dev(samples), dev(cond), inject_actions=dev(acts))
    snap = eng.tree_snapshot()
    rb = eng.rb
    return [t.cpu().numpy() for t in (rb.status, rb.chunks_run, rb.chunk_steps, rb.parent, rb.end_state, rb.states, rb.actions)] + \
           [snap["parents"], snap["states"], snap["counters"]]


def test_round_scratch_growth_across_robots():
    """One context: an ant round at B = 8, a car round at B = 8, an ant round at B = 40 (the ant's scratch grows after the car's
    was made).  Every output equals the same round on a context of its own, bit for bit."""
    from ditreeonlineplanner_amd.ops import Context
    rounds = ((_ant_tape_round, 8), (_car_tape_round, 8), (_ant_tape_round, 40))
    shared = Context(0)
    try:
        got = [fn(shared, B) for fn, B in rounds]
    finally:
        shared.close()
    for (fn, B), out in zip(rounds, got):
        own = Context(0)
        try:
            ref = fn(own, B)
        finally:
            own.close()
        assert len(ref) == len(out)
        for k, (a, b) in enumerate(zip(ref, out)):
            assert a.shape == b.shape and np.array_equal(a, b), (fn.__name__, B, k)
    assert (got[2][1] > 1).sum() > 3 and np.abs(got[2][7]).max() > 0       # edges of several chunks; cond_out was written
