"""GPU: an ant forest (forest.AntForestEngine, include/ditree.h "ant forests") grows every tree exactly as its own
AntExpansionEngine does when fed the same rows -- bit for bit, node histories included -- on tape and on model dynamics, with
the ant denoiser in the loop, and RRT_Planner(env_id='antmaze').plan_runs equals sequential seeded plan() calls, run by run."""
import numpy as np
import pytest
import torch

from oracle import ant as OA
from oracle import rrt as ORRT
from tests.test_gpu_ant_facade import AntEnv, TapeSampler
from tests.test_gpu_ant_round import ant_norm, make_ant_net
from tests.test_gpu_forest import check_plan_runs_equals_sequential, compare_tree, ctx, dev  # noqa: F401
from tests.test_oracle_ant import trace_setup

pytestmark = pytest.mark.gpu

# The `tape_boxes` scenario (maze, start, goal) for every tree.  Per tree: its own RandomTape (samples), action tape and
# observation tape; GOAL_EVERY[t] bends every such candidate of the tree's observation tape towards the goal (0: none).  The
# streams, counts, CAP and MODEL_DESIRED were chosen with the CPU oracle (oracle/ant.py) so that the four rounds hold, on
# both dynamics: a goal that retires a tree (it gets no more candidates), a tree with rounds of 1 and 0 candidates, and a tree
# that runs past its CAP node slots.
SEEDS = [154, 221, 213, 205, 200]
GOAL_EVERY = [7, 0, 5, 0, 11]
COUNTS = [[6, 1, 4, 12, 3], [6, 0, 6, 12, 5], [6, 1, 0, 12, 2], [6, 1, 5, 12, 7]]
CAP = 24
MODEL_DESIRED_OFFSET = (5.0, 4.0)          # model dynamics: the desired goal sits this far from the start (the crawler is slow)


class TreeStreams:
    """The rows tree t feeds its engine: candidate k of the tree is a pure function of (SEEDS[t], k)."""

    def __init__(self, t, maze, goal, desired):
        s = SEEDS[t]
        self.rt = ORRT.RandomTape(s)
        self.at = OA.AntActionTape(s + 1000, 16)
        self.ot = OA.AntObsTape(s + 2000, maze, 4.0, 24, 2, desired_xy=desired, goal_every=GOAL_EVERY[t], step=0.12)
        self.maze, self.goal, self.drawn = maze, goal, 0

    def rows(self, n):
        H, W = self.maze.shape
        s, c = np.zeros((n, 29)), np.zeros((n, 2))
        for i in range(n):
            s[i], c[i] = OA.draw_candidate_ant(self.rt, W, H, 4.0, self.goal)
        cand = np.arange(self.drawn, self.drawn + n)
        acts = np.stack([self.at.actions(cand, j) for j in range(24)], axis=1)
        self.drawn += n
        return s, c, acts, self.ot.rows(cand)


def forest_scenario(dynamics):
    g, pre, _, _, _, m = trace_setup("tape_boxes")
    start, goal = g[pre + "start"], g[pre + "goal"]
    desired = g[pre + "desired"] if dynamics == "tape" else start[:2] + np.array(MODEL_DESIRED_OFFSET)
    return m["maze"], start, goal, desired


def compare_ant_tree(forest, t, single, rows):
    """tests.test_gpu_forest.compare_tree (node arrays, edges, num_visit, counter row, the round's ids) plus what the ant
    adds: every node's history rows and their count, and the round's trajectories, end states and step counts."""
    compare_tree(forest, t, single, rows)
    Cp, ft, st = forest.C, forest.tree, single.tree
    n = int(forest.n_nodes_host[t])
    assert torch.equal(ft.hist_n[t * Cp:t * Cp + n], st.hist_n[:n]), (t, "hist_n")
    hn = st.hist_n[:n].cpu().numpy()
    assert set(hn.tolist()) <= {1, 2, 3} and hn[0] == 1
    for k in range(n):
        assert torch.equal(ft.hist[t * Cp + k, 3 - hn[k]:], st.hist[k, 3 - hn[k]:]), (t, k, "hist")
    lo, hi = rows
    if hi > lo:
        for name in ("end_state", "chunk_steps"):
            assert torch.equal(getattr(forest.rb, name)[lo:hi], getattr(single.rb, name)[:hi - lo]), (t, name)
        run = single.rb.chunks_run[:hi - lo].cpu().numpy()
        for b in range(hi - lo):
            for name in ("states", "actions"):
                assert torch.equal(getattr(forest.rb, name)[lo + b, :run[b]], getattr(single.rb, name)[b, :run[b]]), (t, b, name)


@pytest.mark.parametrize("dynamics", ["tape", "model"])
def test_ant_forest_rounds_equal_single_tree_rounds(ctx, dynamics):
    """Five trees, four rounds of uneven per-tree counts (incl. 0 and 1) on injected actions: every tree bit-identical to its
    own AntExpansionEngine fed the same rows -- through a goal that retires a tree and a full tree."""
    from ditreeonlineplanner_amd.engine import CNT_GOAL, CNT_OVERFLOW, CNT_PHANTOM, CNT_STICKY, AntExpansionEngine
    from ditreeonlineplanner_amd.forest import AntForestEngine
    maze, start, goal, desired = forest_scenario(dynamics)
    T = len(SEEDS)
    kw = dict(desired_goal=desired, norm=ant_norm(), dynamics=dynamics)
    forest = AntForestEngine(ctx, maze, start, goal, T, CAP, batch=64, **kw)
    singles = [AntExpansionEngine(ctx, maze, start, goal, batch=64, capacity=CAP, **kw) for _ in range(T)]
    streams = [TreeStreams(t, maze, goal, desired) for t in range(T)]
    done = [False] * T
    for counts in COUNTS:
        counts = [0 if done[t] else c for t, c in enumerate(counts)]
        rows = [streams[t].rows(counts[t]) if counts[t] else None for t in range(T)]
        for t in range(T):
            if counts[t]:
                s, c, a, o = rows[t]
                singles[t].expand_round(dev(s), dev(c), inject_actions=dev(a), next_obs_tape=dev(o) if dynamics == "tape" else None)
        S, Cg, Ac, Ob = (np.concatenate([r[i] for r in rows if r is not None]) for i in range(4))
        cnt = forest.expand_round(dev(S), dev(Cg), inject_actions=dev(Ac), counts_per_tree=counts,
                                  next_obs_tape=dev(Ob) if dynamics == "tape" else None)
        off = np.concatenate([[0], np.cumsum(counts)])
        for t in range(T):
            compare_ant_tree(forest, t, singles[t], (off[t], off[t + 1]) if counts[t] else (0, 0))
            done[t] = done[t] or int(cnt[t, CNT_GOAL]) >= 0
    cnt = np.stack([forest.counters(t) for t in range(T)])
    assert (cnt[:, CNT_STICKY] == 0).all() and (cnt[:, CNT_PHANTOM] == -1).all()       # the ant env has no sticky-done latch
    retired = [t for t in range(T) if done[t] and streams[t].drawn < sum(c[t] for c in COUNTS)]
    assert retired, "no tree was retired by a goal"
    assert cnt[3, CNT_OVERFLOW] == 1 and forest.n_nodes_host[3] == CAP
    assert cnt[[0, 1, 2, 4], CNT_OVERFLOW].sum() == 0
    # path and fallback per tree, local numbering
    assert forest.fallback_nodes() == [s.fallback_node() for s in singles]
    for t in range(T):
        g = forest.goal_node(t)
        assert g == singles[t].goal_node
        node = g if g is not None else forest.fallback_node(t)
        ref = singles[t].goal_node if singles[t].goal_node is not None else singles[t].fallback_node()
        assert node == ref
        p, a = forest.path_to(t, node)
        rp, ra = singles[t].path_to(ref)
        assert np.array_equal(p, rp) and np.array_equal(a, ra) and p.shape[1] == 29 and a.shape[1] == 8
    # a retired tree's slot takes a new run: back to its root (history included), the others untouched
    t = retired[0]
    others = [k for k in range(T * CAP) if k // CAP != t]
    names = ("state", "hist", "hist_n", "parent", "last_action", "has_prev", "edge_nstates")
    before = {nm: getattr(forest.tree, nm)[others].clone() for nm in names}
    cnt_before = forest.fcounters.clone()
    forest.reset_tree(t)
    r = t * CAP
    assert forest.n_nodes_host[t] == 1 and forest.goal_node(t) is None
    assert np.array_equal(forest.tree.hist[r].cpu().numpy(), np.stack([np.zeros(29), np.zeros(29), start]))
    assert int(forest.tree.hist_n[r]) == 1 and int(forest.tree.parent[r]) == -1 and int(forest.tree.has_prev[r]) == 0
    assert forest.fcounters[t].tolist() == [1, -1, 0, 0, 0, 0, 0, -1]
    for nm in names:
        assert torch.equal(getattr(forest.tree, nm)[others], before[nm]), nm
    keep = [k for k in range(T) if k != t]
    assert torch.equal(forest.fcounters[keep], cnt_before[keep])


# ---------------------------------------------------------------------- the denoiser in the loop
@pytest.fixture(scope="module")
def ant_net_ctx(ctx):
    from ditreeonlineplanner_amd import _lib
    from ditreeonlineplanner_amd.model import NoisePredNet
    onet = make_ant_net()
    net = NoisePredNet(input_dim=8, additional_global_cond_dim=97, pred_horizon=16, local_map_size=16, init=False)
    net.load_state_dict(onet.state_dict())
    net.bind(ctx, precision=_lib.PREC_F16X3, max_batch=128)
    return ctx


@pytest.mark.parametrize("early_exit", [False, True])
def test_ant_denoiser_forest_rounds_equal_single_tree_rounds(ant_net_ctx, early_exit):
    """Four trees x 32 candidates x 2 rounds through the ant network in f16x3 on model dynamics: a sample's result does not
    depend on its batch, so every tree is bit-identical to its own engine's rounds of 32."""
    from ditreeonlineplanner_amd.engine import AntExpansionEngine
    from ditreeonlineplanner_amd.forest import AntForestEngine
    ctx = ant_net_ctx
    maze, start, goal, desired = forest_scenario("model")
    T, B, Cp = 4, 32, 80
    kw = dict(desired_goal=desired, norm=ant_norm(), dynamics="model", early_exit=early_exit)
    forest = AntForestEngine(ctx, maze, start, goal, T, Cp, batch=T * B, **kw)
    singles = [AntExpansionEngine(ctx, maze, start, goal, batch=B, capacity=Cp, **kw) for _ in range(T)]
    rts = [ORRT.RandomTape(40 + t) for t in range(T)]
    gen = torch.Generator(device="cuda").manual_seed(9)
    H, W = maze.shape
    for _ in range(2):
        S, Cg = np.zeros((T, B, 29)), np.zeros((T, B, 2))
        for t in range(T):
            for i in range(B):
                S[t, i], Cg[t, i] = OA.draw_candidate_ant(rts[t], W, H, 4.0, goal)
        noise = torch.randn((T * B, forest.n_chunks, forest.P, 8), generator=gen, device="cuda")
        for t in range(T):
            singles[t].expand_round(dev(S[t]), dev(Cg[t]), noise=noise[t * B:(t + 1) * B].contiguous())
        forest.expand_round(dev(S.reshape(T * B, 29)), dev(Cg.reshape(T * B, 2)), noise=noise, counts_per_tree=[B] * T)
        for t in range(T):
            compare_ant_tree(forest, t, singles[t], (t * B, (t + 1) * B))
    assert all(int(n) > 1 for n in forest.n_nodes_host)


# ---------------------------------------------------------------------- the facade
PLAN_DESIRED_OFFSET = (4.0, 8.0)
# found with oracle/ant.py (OracleAntPlanner.plan on RandomTape(seed), 40 candidates in rounds of 8, the stand-in model and the
# `model_boxes` action tape): seeds 2 and 3 reach the goal (candidates 38 and 20), seeds 1 and 10 end by fallback
PLAN_SEEDS = [1, 2, 3, 10]


def _planner(sampler, ant_dynamics, **kw):
    from ditreeonlineplanner_amd.planners.RRT import RRT_Planner
    g, pre, _, atape, otape, m = trace_setup("model_boxes")
    start, goal = g[pre + "start"], g[pre + "goal"]
    desired = start[:2] + np.array(PLAN_DESIRED_OFFSET)
    env = AntEnv(m["maze"], 4.0, desired)
    if sampler is None:
        sampler = TapeSampler(atape)
    if ant_dynamics == "tape":
        ot = OA.AntObsTape(77, m["maze"], 4.0, 24, 2, desired_xy=desired, goal_every=29, step=0.12)
        kw["next_obs_tape_fn"] = lambda first, B: ot.rows(np.arange(first, first + B))
    if ant_dynamics is not None:
        kw["ant_dynamics"] = ant_dynamics
    return RRT_Planner(start, goal, env_id="antmaze", environment=env, sampler=sampler, prediction_type="actions", action_horizon=2,
                       local_map_size=16, local_map_scale=0.8, global_map_scale=4.0, goal_conditioning_bias=0.85, prop_duration=[48],
                       time_budget=1e9, max_iter=300, verbose=False, capacity=1024, **kw)


def test_ant_plan_runs_equals_sequential_seeded_plans_action_tape():
    """(a) the action tape + model dynamics, batch 8, 40 candidates, four seeds on two trees (slot reuse): both endings occur;
    (b) the same with tape dynamics and a next_obs_tape_fn."""
    runs = check_plan_runs_equals_sequential(_planner(None, "model", batch=8, max_candidates=40), PLAN_SEEDS, concurrent=2)
    assert any(r["goal_reached"] for r in runs) and any(r["success"] and not r["goal_reached"] for r in runs)
    assert all(r["cc_calls"] == 0 and r["path"].shape[1] == 29 and r["actions"].shape[1] == 8 for r in runs)
    runs = check_plan_runs_equals_sequential(_planner(None, "tape", batch=8, max_candidates=40), PLAN_SEEDS, concurrent=2)
    assert all(r["iterations"] > 0 and r["cc_calls"] == 0 for r in runs)


@pytest.fixture(scope="module")
def ant_policy_net():
    from ditreeonlineplanner_amd.train_diffusion_policy import init_noise_pred_net
    torch.manual_seed(0)
    return init_noise_pred_net(input_dim=8, action_dim=8, obs_dim=29, obs_history=3, action_history=1, goal_conditioned=True,
                               goal_dim=2, local_map_conditioned=True, local_map_encoder="resnet", local_map_embedding_dim=400,
                               local_map_size=16, down_dims=[512, 1024, 2048])


def _sampler(net, scheduler=None, k=1):
    from ditreeonlineplanner_amd.policies.fm_policy import DiffusionSampler
    return DiffusionSampler(net, scheduler, "antmaze", policy="diffusion" if scheduler is not None else "flow_matching",
                            pred_horizon=16, action_dim=8, prediction_type="actions", obs_history=3, action_history=1,
                            goal_conditioned=True, num_diffusion_iters=k, local_map_size=16)


def test_ant_plan_runs_equals_sequential_seeded_plans_network(ant_policy_net):
    """(c) the network sampler + model dynamics, batch 16, 32 candidates, three seeds at once: each run's start noise from its
    own generator at ACTION_DIM 8."""
    runs = check_plan_runs_equals_sequential(_planner(_sampler(ant_policy_net), "model", batch=16, max_candidates=32), [21, 22, 23],
                                             concurrent=None)
    assert all(r["iterations"] > 0 and r["cc_calls"] == 0 for r in runs)


def test_ant_plan_runs_equals_sequential_seeded_plans_ddpm(ant_policy_net):
    """(d) the same with the sampler's DDPM branch (K = 4): start noise, then step noise, from each run's own generator."""
    from ditreeonlineplanner_amd.ddpm import DDPMScheduler
    sch = DDPMScheduler(num_train_timesteps=4, beta_schedule="squaredcos_cap_v2", clip_sample=True, prediction_type="epsilon")
    runs = check_plan_runs_equals_sequential(_planner(_sampler(ant_policy_net, sch, 4), "model", batch=16, max_candidates=32),
                                             [21, 22, 23], concurrent=None)
    assert all(r["iterations"] > 0 for r in runs)


def test_ant_forest_facade_refusals():
    """plan_runs with the default host dynamics (the caller's simulator), plan_scenario_runs with ant planners."""
    from ditreeonlineplanner_amd.planners.RRT import plan_scenario_runs
    with pytest.raises(NotImplementedError, match="car") as e:
        _planner(None, None, batch=4, max_candidates=4).plan_runs([1, 2])
    assert "host" in str(e.value)
    pls = [_planner(None, "model", batch=4, max_candidates=4) for _ in range(2)]
    with pytest.raises(NotImplementedError, match="car"):
        plan_scenario_runs(pls, [[1], [2]])
