"""GPU: a forest of independent trees (ditreeonlineplanner_amd/forest.py, include/ditree.h "forests") grows every tree exactly
as its own single-tree engine does when fed the same rows -- bit for bit -- and RRT_Planner.plan_runs equals sequential seeded
plan() calls, run by run."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

from oracle import denoiser as OD
from oracle import geometry as G
from oracle import rrt as ORRT
from oracle.tapes import ActionTape
from tests.util import load_maze

pytestmark = pytest.mark.gpu

# One maze / start / goal for every tree (the goal test lives in the rollout).  The per-tree streams (sample seed, action-tape
# seed) and candidate counts were chosen with the CPU oracle so that the four rounds hold: tree 0 a sticky-done phantom in
# round 1, tree 1 rounds of 1 and 0 candidates, trees 2 and 1 a goal in round 3, tree 4 a goal in round 1 (then no more
# candidates), tree 3 running past its C = 24 slots.
MAZE, START, GOAL, H = "boxes", ((18, 8), 0.0), (18, 10), 32
SEEDS = [154, 221, 213, 205, 200]
COUNTS = [[16, 1, 4, 12, 3], [16, 0, 6, 12, 5], [16, 1, 0, 12, 2], [16, 1, 5, 12, 7]]
CAP = 24


@pytest.fixture(scope="module")
def ctx():
    from ditreeonlineplanner_amd.ops import Context
    c = Context(0)
    yield c
    c.close()


def dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def scenario():
    maze = load_maze(MAZE)
    (sr, sc), deg = START
    start = np.array([*G.cell_rowcol_to_xy([sr, sc], maze), np.deg2rad(deg), 0, 0, 0])
    goal = np.array([*G.cell_rowcol_to_xy(list(GOAL), maze), 0, 0, 0, 0])
    return maze, start, goal


def compare_tree(forest, t, single, rows, phantom_base=None):
    """Tree t of the forest against its own engine: node arrays, edges, counter row and the round's rows (``rows``: the tree's
    range in this round; ``phantom_base``: its first row in the last round it had candidates)."""
    from ditreeonlineplanner_amd.engine import CNT_GOAL, CNT_PHANTOM
    Cp, ft, st = forest.C, forest.tree, single.tree
    n = int(forest.n_nodes_host[t])
    assert n == st.n_nodes_host
    sl = slice(t * Cp, t * Cp + n)
    par = ft.parent[sl].cpu().numpy()
    assert np.array_equal(np.where(par < 0, par, par - t * Cp), st.parent[:n].cpu().numpy())
    for name in ("state", "xy", "last_action", "has_prev", "edge_nstates", "edge_nactions"):
        assert torch.equal(getattr(ft, name)[sl], getattr(st, name)[:n]), (t, name)
    # num_visit over the tree's whole slot range (atomics from the accept land only on the tree's own nodes)
    assert torch.equal(ft.num_visit[t * Cp:(t + 1) * Cp], st.num_visit[:Cp]), (t, "num_visit")
    for k in range(1, n):
        ns, na = int(st.edge_nstates[k]), int(st.edge_nactions[k])
        assert torch.equal(ft.edge_states[t * Cp + k, :ns], st.edge_states[k, :ns]), (t, k)
        assert torch.equal(ft.edge_actions[t * Cp + k, :na], st.edge_actions[k, :na]), (t, k)
    row = forest.counters(t).astype(np.int64)
    ref = st.counters.cpu().numpy().astype(np.int64)
    lo, hi = rows
    if row[CNT_GOAL] >= 0:
        row[CNT_GOAL] -= t * Cp
    if row[CNT_PHANTOM] >= 0:
        row[CNT_PHANTOM] -= lo if phantom_base is None else phantom_base
    assert np.array_equal(row, ref), (t, row, ref)
    if hi > lo:
        nid = forest.rb.node_id[lo:hi].cpu().numpy().astype(np.int64)
        nid = np.where(nid < 0, nid, nid - t * Cp)
        assert np.array_equal(nid, single.rb.node_id[:hi - lo].cpu().numpy())
        for name in ("status", "chunks_run", "parent"):
            f = getattr(forest.rb, name)[lo:hi].cpu().numpy().astype(np.int64)
            s = getattr(single.rb, name)[:hi - lo].cpu().numpy().astype(np.int64)
            if name == "parent":
                f = f - t * Cp
            assert np.array_equal(f, s), (t, name)


def test_tape_forest_rounds_equal_single_tree_rounds(ctx):
    """Five trees, four rounds of uneven per-tree counts (incl. 0 and 1) on action tapes: every tree bit-identical to its own
    ExpansionEngine fed the same rows -- through a goal that retires a tree, a sticky-done phantom and a full tree."""
    from ditreeonlineplanner_amd.engine import CNT_GOAL, CNT_OVERFLOW, CNT_STICKY, ExpansionEngine
    from ditreeonlineplanner_amd.forest import ForestEngine
    maze, start, goal = scenario()
    T = len(SEEDS)
    forest = ForestEngine(ctx, maze, start, goal, T, CAP, edge_length=H, batch=64)
    singles = [ExpansionEngine(ctx, maze, start, goal, edge_length=H, batch=64, capacity=CAP) for _ in range(T)]
    rts = [ORRT.RandomTape(s) for s in SEEDS]
    ats = [ActionTape(s + 1000) for s in SEEDS]
    drawn = [0] * T
    done = [False] * T
    last_lo = [0] * T
    W, L = maze.shape[1], maze.shape[0]
    for counts in COUNTS:
        counts = [0 if done[t] else c for t, c in enumerate(counts)]
        S, Cg, Ac = [], [], []
        for t in range(T):
            if counts[t]:
                s, c = rts[t].draw_round(counts[t], W, L, goal)
                a = np.stack([ats[t].actions(np.arange(drawn[t], drawn[t] + counts[t]), j) for j in range(forest.n_chunks)], axis=1)
                S.append(s), Cg.append(c), Ac.append(a)
                singles[t].expand_round(dev(s), dev(c), inject_actions=dev(a))
        cnt = forest.expand_round(dev(np.concatenate(S)), dev(np.concatenate(Cg)), inject_actions=dev(np.concatenate(Ac)),
                                  counts_per_tree=counts)
        off = np.concatenate([[0], np.cumsum(counts)])
        for t in range(T):
            if counts[t]:
                last_lo[t] = off[t]
            compare_tree(forest, t, singles[t], (off[t], off[t + 1]) if counts[t] else (0, 0), last_lo[t])
            drawn[t] += counts[t]
            done[t] = done[t] or int(cnt[t, CNT_GOAL]) >= 0
    cnt = np.stack([forest.counters(t) for t in range(T)])
    assert cnt[0, CNT_STICKY] == 1 and cnt[0, CNT_GOAL] >= 0                      # the phantom
    assert (cnt[[1, 2, 4], CNT_GOAL] >= 0).all() and (cnt[[1, 2, 4], CNT_STICKY] == 0).all()
    assert cnt[3, CNT_OVERFLOW] == 1 and forest.n_nodes_host[3] == CAP
    assert drawn[4] == 3 + 5                                                     # tree 4 left after its goal in round 1
    # path and fallback per tree, local numbering
    for t in range(T):
        g = forest.goal_node(t)
        node = g if g is not None else forest.fallback_node(t)
        ref = singles[t].goal_node if singles[t].goal_node is not None else singles[t].fallback_node()
        assert node == ref
        p, a = forest.path_to(t, node)
        rp, ra = singles[t].path_to(ref)
        assert np.array_equal(p, rp) and np.array_equal(a, ra)
    # a retired tree's slot takes a new run: back to its root, the others untouched
    before = forest.tree.state[:CAP].clone()
    forest.reset_tree(4)
    assert forest.n_nodes_host[4] == 1 and forest.goal_node(4) is None and torch.equal(forest.tree.state[:CAP], before)


@pytest.fixture(scope="module")
def net_ctx(ctx):
    from ditreeonlineplanner_amd import _lib
    from ditreeonlineplanner_amd.model import NoisePredNet
    torch.manual_seed(0)
    onet = OD.init_noise_pred_net().eval()
    net = NoisePredNet(init=False)
    net.load_state_dict(onet.state_dict())
    net.bind(ctx, precision=_lib.PREC_F16X3, max_batch=256)
    return ctx


@pytest.mark.parametrize("early_exit,schedule", [(False, None), (True, None), (True, [32, 64])])
def test_denoiser_forest_rounds_equal_single_tree_rounds(net_ctx, early_exit, schedule):
    """Four trees x 64 candidates x 3 rounds through the default f16x3 network: a sample's result does not depend on its
    batch, so every tree is bit-identical to its own engine's rounds of 64."""
    from ditreeonlineplanner_amd.engine import ExpansionEngine
    from ditreeonlineplanner_amd.forest import ForestEngine
    ctx = net_ctx
    maze = load_maze("boxes")
    start = np.array([*G.cell_rowcol_to_xy([17, 2], maze), np.deg2rad(45.0), 0, 0, 0])
    goal = np.array([*G.cell_rowcol_to_xy([2, 17], maze), 0, 0, 0, 0])
    T, B, Cp = 4, 64, 256
    kw = dict(edge_length=64, prop_duration=schedule, early_exit=early_exit)
    forest = ForestEngine(ctx, maze, start, goal, T, Cp, batch=T * B, **kw)
    singles = [ExpansionEngine(ctx, maze, start, goal, batch=B, capacity=Cp, **kw) for _ in range(T)]
    rts = [ORRT.RandomTape(40 + t) for t in range(T)]
    gen = torch.Generator(device="cuda").manual_seed(9)
    for _ in range(3):
        S, Cg = zip(*[rt.draw_round(B, 20, 20, goal) for rt in rts])
        noise = torch.randn((T * B, forest.n_chunks, forest.P, 2), generator=gen, device="cuda")
        for t in range(T):
            singles[t].expand_round(dev(S[t]), dev(Cg[t]), noise=noise[t * B:(t + 1) * B].contiguous())
        forest.expand_round(dev(np.concatenate(S)), dev(np.concatenate(Cg)), noise=noise, counts_per_tree=[B] * T)
        for t in range(T):
            compare_tree(forest, t, singles[t], (t * B, (t + 1) * B))


def test_forest_calls_refuse_bad_arguments_without_launching(ctx):
    """Non-monotone offsets, off[T] != B and T * C > capacity give DITREE_E_ARG with a message, and the round is untouched."""
    from ditreeonlineplanner_amd import _lib
    from ditreeonlineplanner_amd.engine import ExpansionEngine
    from ditreeonlineplanner_amd.forest import ForestEngine
    maze, start, goal = scenario()
    forest = ForestEngine(ctx, maze, start, goal, 3, 8, edge_length=H, batch=8)
    h, L = ctx._h, _lib.lib()
    forest.rb.node_id.fill_(-7)
    rd = forest.rb.desc(0, 4)

    def accept_with(off, n_trees=3, cap=8):
        off_host = (C.c_int32 * len(off))(*off)
        fd = _lib.Forest(n_trees, cap, forest.fcounters.data_ptr(), forest.off_dev.data_ptr(), off_host)
        return L.ditree_forest_accept(h, C.byref(forest.tree.desc), C.byref(fd), C.byref(rd), 1, ctx.stream)
    for off, n_trees, cap, msg in (([0, 3, 2, 4], 3, 8, b"not monotone"), ([0, 1, 2, 3], 3, 8, b"off[T] = 3"),
                                   ([0, 1, 2, 4], 3, 9, b"exceeds the tree's capacity"), ([1, 2, 3, 4], 3, 8, b"off[0]")):
        assert accept_with(off, n_trees, cap) == -1
        assert msg in L.ditree_last_error(h)
    assert (forest.rb.node_id == -7).all()
    with pytest.raises(ValueError, match="one entry per tree"):
        forest.expand_round(dev(np.zeros((2, 6))), dev(np.zeros((2, 2))), inject_actions=dev(np.zeros((2, 4, 64, 2))),
                            counts_per_tree=[1, 1])
    # an ant-shaped tree is not a forest
    single = ExpansionEngine(ctx, maze, start, goal, edge_length=H, batch=8, capacity=24)
    single.tree.desc.state_dim = 29
    fd = _lib.Forest(3, 8, forest.fcounters.data_ptr(), forest.off_dev.data_ptr(), (C.c_int32 * 4)(0, 1, 2, 4))
    assert L.ditree_forest_accept(h, C.byref(single.tree.desc), C.byref(fd), C.byref(rd), 0, ctx.stream) == -1
    assert b"car tree" in L.ditree_last_error(h)


# ---------------------------------------------------------------------- the facade
def _planner(sampler, **kw):
    from ditreeonlineplanner_amd.car_env import CarEnv
    from ditreeonlineplanner_amd.planners.RRT import RRT_Planner
    maze = load_maze("boxes")
    env = CarEnv(maze_map=maze, collision_checking=False)
    start = np.array([*env.cell_rowcol_to_xy(np.array([18, 13])), 0.0, 0.0, 0.0, 0.0])
    goal = np.array([*env.cell_rowcol_to_xy(np.array([18, 17])), 0, 0, 0, 0.0])
    args = dict(env_id="carmaze", environment=env, sampler=sampler, action_horizon=8, local_map_size=20, local_map_scale=0.2,
                global_map_scale=1.0, goal_conditioning_bias=0.85, prop_duration=[32], time_budget=600)
    args.update(kw)
    return RRT_Planner(start, goal, **args)


def _rng_states():
    return (random.getstate(), np.random.get_state()[1].copy(), np.random.get_state()[2], torch.get_rng_state().clone(),
            torch.cuda.get_rng_state().clone())


def _same_states(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2] == b[2] and torch.equal(a[3], b[3]) and torch.equal(a[4], b[4])


def check_plan_runs_equals_sequential(pl, seeds, concurrent):
    from ditreeonlineplanner_amd.common import map_utils
    seq = []
    for s in seeds:
        random.seed(s)
        np.random.seed(s)
        torch.manual_seed(s)
        map_utils.cc_calls = 0
        pl.reset()
        path, actions = pl.plan()
        seq.append(dict(pl.results, path=path, actions=actions, cc_calls=map_utils.cc_calls,
                        goal=pl._engine.goal_node is not None))
    random.seed(123)
    np.random.seed(456)
    torch.manual_seed(789)
    before = _rng_states()
    map_utils.cc_calls = 0
    runs = pl.plan_runs(seeds, concurrent=concurrent)
    assert _same_states(before, _rng_states())
    assert map_utils.cc_calls == sum(r["cc_calls"] for r in seq)
    assert [r["seed"] for r in runs] == list(seeds)
    for r, q in zip(runs, seq):
        for k in ("iterations", "number_of_nodes", "cc_calls"):
            assert r[k] == q[k], (r["seed"], k, r[k], q[k])
        assert r["success"] == (q["path"] is not None) and r["goal_reached"] == q["goal"]
        for k in ("path", "actions"):
            assert (r[k] is None) == (q[k] is None) and (r[k] is None or np.array_equal(r[k], q[k])), (r["seed"], k)
        if q["path"] is not None:
            assert r["path_time"] == q["path_time"]
    return runs


@pytest.fixture(scope="module")
def car_net():
    from ditreeonlineplanner_amd.train_diffusion_policy import init_noise_pred_net
    torch.manual_seed(0)
    onet = OD.init_noise_pred_net().eval()
    net = init_noise_pred_net(input_dim=2, action_dim=2, obs_dim=3, obs_history=1, action_history=1, goal_conditioned=True,
                              goal_dim=2, local_map_conditioned=True, local_map_encoder="resnet", local_map_embedding_dim=400,
                              local_map_size=20, down_dims=[512, 1024, 2048])
    net.load_state_dict(onet.state_dict())
    return net


def _sampler(net, scheduler=None, k=1):
    from ditreeonlineplanner_amd.policies.fm_policy import DiffusionSampler
    return DiffusionSampler(net, scheduler, "carmaze", policy="diffusion" if scheduler is not None else "flow_matching",
                            pred_horizon=64, action_dim=2, prediction_type="actions", obs_history=1, action_history=1,
                            goal_conditioned=True, num_diffusion_iters=k, local_map_size=20).eval()


def test_plan_runs_equals_sequential_seeded_plans_network(car_net):
    pl = _planner(_sampler(car_net), batch=16, max_candidates=64)
    runs = check_plan_runs_equals_sequential(pl, [1, 2, 3, 4, 5, 6], concurrent=3)
    assert all(r["iterations"] > 0 for r in runs)


def test_plan_runs_equals_sequential_seeded_plans_tape_and_ddpm(car_net):
    from ditreeonlineplanner_amd.ddpm import DDPMScheduler

    class Tape:
        def __init__(self):
            self.tape = ActionTape(5)

        def sample_round(self, first, B, n_chunks, P):
            return np.stack([self.tape.actions(np.arange(first, first + B), j) for j in range(n_chunks)], axis=1)
    check_plan_runs_equals_sequential(_planner(Tape(), batch=8, max_candidates=40), [11, 12, 13, 14], concurrent=2)
    sch = DDPMScheduler(num_train_timesteps=4, beta_schedule="squaredcos_cap_v2", clip_sample=True, prediction_type="epsilon")
    check_plan_runs_equals_sequential(_planner(_sampler(car_net, sch, 4), batch=16, max_candidates=32), [21, 22, 23],
                                      concurrent=None)


def test_plan_runs_refuses_what_it_does_not_cover(car_net):
    class OneAction:                                          # a plain callable: its own generator, not split per run
        def __call__(self, *a, **k):
            return np.array([[4.0, 0.1]])
    with pytest.raises(NotImplementedError, match="plain-callable"):
        _planner(OneAction(), batch=4, max_candidates=4).plan_runs([1, 2])
    with pytest.raises(NotImplementedError, match="run_type 0"):
        _planner(_sampler(car_net), batch=4, max_candidates=4, run_type=1).plan_runs([1, 2])
