"""GPU: the reference's five small local-map encoders (identity, mlp, max, grid, cnn; local_map_encoder.py:137-218) on the
device, against tests/golden/encoders*.npz -- embeddings, parameters and d_ref from the reference's own classes
(tests/golden/make_encoder_golden.py, which also asserts that the reference's whole network equals
OracleUnet1D(cat(embedding, cond)): the expectation of the whole-network and round tests here).

Embedding bound: identity and max bit for bit; mlp, grid and cnn within 16 x d_ref, d_ref = the reference's own
fp32-vs-float64 difference per case (1.5e-8 .. 1.7e-7).  The margin covers another summation order and the device's exp /
division in Mish, a few ulp each.

On the MI355X the kernels deviate from the fixture by 1.2 x d_ref (mlp, grid at N = 20) to 2.5 x d_ref (cnn, N = 16), the
same multiples as the same source run on host threads.  Each case prints its figure as an ENCODER_DEVIATION line.
"""
import numpy as np
import pytest
import torch

from oracle import sampler as OS
from tests import encoder_util as EU
from tests.test_gpu_denoiser import TOL, rel

pytestmark = pytest.mark.gpu
MARGIN = 16.0
CAR_CASE = {"identity": "identity_20", "mlp": "mlp_20", "max": "max_20_k3", "grid": "grid_20", "cnn": "cnn_20"}


@pytest.fixture(scope="module")
def ctx():
    from ditreeonlineplanner_amd.ops import Context
    c = Context(0)
    yield c
    c.close()


def _inputs(case, B, seed=5):
    """(noise, cond) rows for the case's network; row b is the same whatever B (a prefix of one seeded draw)."""
    _, _, n, _ = EU.CASE[case]
    D, G, P = EU.shape_of(n)
    g = torch.Generator().manual_seed(seed)
    noise = torch.randn(65, P, D, generator=g)
    cond = torch.randn(65, G, generator=g) * 0.7
    return noise[:B].contiguous(), cond[:B].contiguous()


def _run(ctx, case, rows, want_emb=True):
    """One flow step on the given fixture map rows -> (x1, map_emb) as numpy."""
    _, _, n, _ = EU.CASE[case]
    noise, cond = _inputs(case, 65)
    idx = torch.as_tensor(rows)
    lm = torch.tensor(EU.maps(n))[idx].contiguous()
    D = noise.shape[2]
    unit = np.concatenate([np.zeros(D), np.ones(D)])       # x1 is read normalised; the table only has to be D wide (8 for the ant)
    x1 = ctx.denoise(noise[idx].contiguous().cuda(), lm.cuda(), cond[idx].contiguous().cuda(), act_norm=unit, want_actions=False)
    emb = ctx.debug_read("map_emb", len(rows))[:, 0, :].cpu().numpy() if want_emb else None
    return x1.cpu().numpy(), emb


@pytest.mark.parametrize("case", [c[0] for c in EU.CASES])
def test_embeddings_match_the_reference(ctx, case):
    """Every fixture case at B in {1, 3, 65} through ctx.denoise and the "map_emb" tap; N = 16 on an ant-shaped net."""
    _, kind, n, E = EU.CASE[case]
    fx = EU.fixture()
    want, d_ref = fx[f"{case}/emb"], float(fx[f"{case}/d_ref"])
    net, _ = EU.make_pair(case)
    net.bind(ctx, precision=1, max_batch=65)
    D, G, P = EU.shape_of(n)
    assert ctx.denoise_dims() == (P, D, n, G, E)
    worst = 0.0
    for B in (1, 3, 65):
        x1, emb = _run(ctx, case, list(range(B)))
        assert emb.shape == (B, E) and emb.dtype == np.float32 and np.isfinite(x1).all()
        if kind in ("identity", "max"):
            assert np.array_equal(emb, want[:B]), (case, B)
        else:
            worst = max(worst, float(np.abs(emb.astype(np.float64) - want[:B]).max()))
    if kind not in ("identity", "max"):
        print(f"ENCODER_DEVIATION {case}: max |engine - reference| {worst:.3g} = {worst / d_ref:.2f} x d_ref ({d_ref:.3g})")
        assert worst <= MARGIN * d_ref, (case, worst, d_ref, worst / d_ref)


@pytest.mark.parametrize("kind", EU.SMALL)
def test_a_sample_does_not_depend_on_its_batch(ctx, kind):
    """Row b of a B = 65 call == the B = 1 call on that map, bit for bit: embedding and x1.  Rows on both sides of the mlp
    kernel's 8-sample tiles, the last row of a partial tile, and the constant maps."""
    case = CAR_CASE[kind]
    net, _ = EU.make_pair(case)
    net.bind(ctx, precision=1, max_batch=65)
    x_all, e_all = _run(ctx, case, list(range(65)))
    for b in (0, 1, 7, 8, 37, 64):
        x_one, e_one = _run(ctx, case, [b])
        assert np.array_equal(e_one[0], e_all[b]), (kind, b)
        assert np.array_equal(x_one[0], x_all[b]), (kind, b)


def test_embedding_bits_do_not_depend_on_the_precision(ctx):
    """The small encoders run in f32 in every instantiation: PREC_F32 and PREC_F16X3 give the same embedding bits."""
    from ditreeonlineplanner_amd._lib import PREC_F16X3, PREC_F32
    net, _ = EU.make_pair("cnn_20", dims=(256, 512, 1024))
    embs = []
    for prec in (PREC_F32, PREC_F16X3):
        net.bind(ctx, precision=prec, max_batch=65)
        embs.append(_run(ctx, "cnn_20", list(range(65)))[1])
    assert np.array_equal(embs[0], embs[1])
    assert np.abs(embs[0]).max() > 0


ROWS = [0, 1, 2, 10, 20, 30, 40, 64]


@pytest.mark.parametrize("kind,prec,dims", [(k, 1, (64, 128, 256)) for k in EU.SMALL] + [("cnn", 2, (256, 512, 1024))])
def test_whole_network_against_the_composed_oracle(ctx, kind, prec, dims):
    """x1 of one flow step against OracleUnet1D(cat(fixture embedding, cond)); 'max' (E = 9, cond_dim 272) and the car 'cnn'
    (E = 576, cond_dim 839) are the narrowest and the widest FiLM input."""
    case = CAR_CASE[kind]
    _, _, n, E = EU.CASE[case]
    net, ounet = EU.make_pair(case, dims=dims)
    net.bind(ctx, precision=prec, max_batch=len(ROWS))
    noise, cond = _inputs(case, 65)
    emb = torch.tensor(EU.fixture()[f"{case}/emb"][ROWS])
    oracle = EU.ComposedNet(ounet, lambda lm: emb)
    x_ref = OS.flow_sample(oracle, noise[ROWS], EU.maps(n)[ROWS], cond[ROWS], k_steps=1)
    x1, _ = _run(ctx, case, ROWS, want_emb=False)
    r = rel(x1, x_ref)
    print(f"WHOLE_NETWORK {kind} prec {prec}: rel {r:.3g} (bound {2 * TOL[prec]['l2']:.3g}), cond_dim {256 + E + 7}")
    assert r < 2 * TOL[prec]["l2"], (kind, prec, r)
    assert rel(noise[ROWS].numpy(), x_ref) > 1e-2            # the step moved the sample: the comparison is not vacuous


def test_reuse_encoder_keeps_the_embedding(ctx):
    case = "mlp_20"
    net, _ = EU.make_pair(case)
    net.bind(ctx, precision=1, max_batch=8)
    noise, cond = _inputs(case, 8)
    lm = torch.tensor(EU.maps(20)[6:14]).cuda()
    other = torch.tensor(EU.maps(20)[20:28]).cuda()
    x, c = noise.cuda(), cond.cuda()
    x2 = (noise * 0.5 + 0.1).cuda()
    ctx.denoise_eval(x, lm, c, 3.0)
    again = ctx.denoise_eval(x2, lm, c, 2.0, reuse_encoder=True).cpu().numpy()
    kept = ctx.denoise_eval(x2, other, c, 2.0, reuse_encoder=True).cpu().numpy()       # the maps are not read again
    fresh = ctx.denoise_eval(x2, lm, c, 2.0).cpu().numpy()
    assert np.array_equal(again, fresh) and np.array_equal(kept, fresh)
    assert not np.array_equal(ctx.denoise_eval(x2, other, c, 2.0).cpu().numpy(), fresh)


def test_one_round_with_a_cnn_net(ctx):
    """8 candidates, H = 32, boxes: ExpansionEngine.expand_round against the oracle round (tests/test_gpu_round_precision.py)
    whose net is (restated cnn encoder + OracleUnet1D)."""
    from tests import test_gpu_round_precision as RP
    from ditreeonlineplanner_amd.engine import CNT_GOAL, CNT_LATCH, CNT_NODES, ExpansionEngine
    Bc, prec = 8, 1
    net, ounet = EU.make_pair("cnn_20")
    params = EU.case_params("cnn_20")
    oracle = EU.ComposedNet(ounet, lambda lm: EU.restated_encoder("cnn", lm, params, 576))
    # the seed: the first after 20260301 whose oracle round mixes survivors with collisions in chunks 1, 2 and 3 and keeps every
    # local-map sample point > 1e-4 from an occupancy-changing cell boundary (map_margin; 20260301 has one at 3e-6) -- properties
    # of the oracle round alone
    maze, nodes, goal, samples, cond, noise = RP.make_inputs(Bc, 20260303)
    pl = RP._oracle_planner(lambda sample, local_map, timestep, global_cond: oracle(sample, local_map, timestep, global_cond),
                            maze, nodes, goal, noise)
    ref = pl.expand_round(samples, cond)
    assert pl.goal_node is None
    ref["tree_parents"], ref["tree_states"] = np.array(pl.tree.parents), np.array(pl.tree.states)
    run = np.arange(RP.H // RP.A)[None, :] < ref["chunks_run"][:, None]
    mm = np.full(run.shape, np.inf)
    mm[run] = RP.map_margin(maze, ref["states"][:, :, 0][run])
    ref["map_margin"] = mm.min(axis=1)
    assert (ref["status"] == 0).sum() >= 2 and (ref["status"] == 2).sum() >= 2 and ref["chunks_run"].sum() > 2 * Bc
    assert ref["map_margin"].min() > 1e-4

    net.bind(ctx, precision=prec, max_batch=Bc)
    st = dict(B=Bc, rounds=1, maze=maze, nodes=nodes, goal=goal, samples=samples, cond=cond, noise=noise)
    N0, dev = RP.N0, ctx.device
    eng = ExpansionEngine(ctx, maze, nodes[0], goal, edge_length=RP.H, action_horizon=RP.A, pred_horizon=RP.P, batch=Bc,
                          capacity=N0 + Bc, emulate_sticky_done=False)
    assert ctx.weights_owner is net                     # the engine ran OUR net, not a re-bound default
    t = eng.tree
    nd = torch.as_tensor(nodes, device=dev)
    t.state[:N0] = nd
    t.xy[:N0] = nd[:, :2]
    t.parent[:N0] = torch.arange(-1, N0 - 1, device=dev, dtype=torch.int32).clamp(min=0)
    t.parent[0] = -1
    t.has_prev[1:N0] = 1
    t.counters[CNT_NODES] = N0
    t.counters[CNT_GOAL] = -1
    t.counters[CNT_LATCH] = 0
    t.n_nodes_host = N0
    eng.expand_round(torch.as_tensor(samples, device=dev), torch.as_tensor(cond, device=dev), noise=noise.to(dev))
    rb, snap = eng.rb, eng.tree_snapshot()
    got = dict(status=rb.status[:Bc].cpu().numpy() & 0xFF, parent=rb.parent[:Bc].cpu().numpy(),
               end_state=rb.end_state[:Bc].cpu().numpy(), states=rb.states[:Bc].cpu().numpy(),
               chunks_run=rb.chunks_run[:Bc].cpu().numpy(), chunk_steps=rb.chunk_steps[:Bc].cpu().numpy(),
               tree_parents=snap["parents"], tree_states=snap["states"])
    dv = RP.deviation(got, ref)
    print("ROUND cnn", dv)
    tol = RP.BOUND[prec][0]
    assert dv["flips"] == 0 and dv["n_agree"] == Bc, dv                  # statuses, chunk counts, executed steps: exact
    assert dv["nn_parent_mismatches"] == 0 and dv["tree_parent_mismatches"] == 0, dv
    assert dv["map_sensitive"] == 0, dv                                   # (a property of the seeded oracle round)
    assert dv["max_abs_trajectory_state"] < tol and dv["max_abs_tree_node_state"] < tol, dv


def test_planner_facade_with_the_default_identity_encoder(ctx):
    """init_noise_pred_net's own default, local_map_encoder='identity', through DiffusionSampler and RRT_Planner.plan()."""
    import random
    from ditreeonlineplanner_amd.car_env import CarEnv
    from ditreeonlineplanner_amd.planners.RRT import RRT_Planner
    from ditreeonlineplanner_amd.policies.fm_policy import DiffusionSampler
    from ditreeonlineplanner_amd.train_diffusion_policy import init_noise_pred_net
    from oracle import geometry as G
    from tests.util import load_maze
    net = init_noise_pred_net(input_dim=2, action_dim=2, obs_dim=3, obs_history=1, action_history=1, goal_conditioned=True,
                              goal_dim=2, local_map_size=20, down_dims=[256, 512, 1024])
    assert net.encoder_name == "identity" and net.embedding_dim == 400
    smp = DiffusionSampler(net, None, "carmaze", policy="flow_matching", pred_horizon=64, action_dim=2, prediction_type="actions",
                           obs_history=1, action_history=1, goal_conditioned=True, num_diffusion_iters=1, local_map_size=20).eval()
    maze = load_maze("boxes")
    env = CarEnv(maze_map=maze, collision_checking=False)
    start = np.array([*G.cell_rowcol_to_xy([17, 2], maze), 0.7, 0, 0, 0])
    goal = np.array([*G.cell_rowcol_to_xy([2, 17], maze), 0, 0, 0, 0])
    random.seed(3)
    np.random.seed(3)
    torch.manual_seed(3)
    pl = RRT_Planner(start, goal, env_id="carmaze", environment=env, sampler=smp, action_horizon=8, local_map_size=20,
                     local_map_scale=0.2, global_map_scale=1.0, prop_duration=[32], time_budget=60, batch=16,
                     max_candidates=32)
    pl.plan()
    assert pl.results["iterations"] > 0 and pl.results["number_of_nodes"] > 1
    assert pl._engine.ctx.denoise_dims()[4] == 400


def test_unsupported_encoder_manifests_are_clean_errors(ctx):
    """What the loader cannot serve comes back through ditree_last_error, not an abort."""
    from ditreeonlineplanner_amd._lib import DitreeError
    from ditreeonlineplanner_amd.weights import pack_state_dict
    net, _ = EU.make_pair("max_20_k3")
    sd = net.state_dict()
    for enc, E, msg in (("cnn", 9, "produces 576"), ("max", 10, "perfect square"), ("mlp", 400, "cond_dim")):
        blob, manifest = pack_state_dict(sd, pred_horizon=64, local_map_size=20, checksum=False, encoder=enc, embedding_dim=E)
        with pytest.raises(DitreeError, match=msg):
            ctx.load_weights(blob, manifest)
    blob, manifest = pack_state_dict(sd, pred_horizon=64, local_map_size=20, checksum=False, encoder="max", embedding_dim=9)
    with pytest.raises(DitreeError, match="unknown encoder"):
        ctx.load_weights(blob, manifest.replace("#encoder max 9", "#encoder vit 9"))
    # a 'grid' manifest whose blob lacks the conv parameters: refused when the plan is built
    sd = {k: v for k, v in EU.make_pair("grid_20")[0].state_dict().items() if not k.startswith("encoder.")}
    blob, manifest = pack_state_dict(sd, pred_horizon=64, local_map_size=20, checksum=False, encoder="grid", embedding_dim=144)
    ctx.load_weights(blob, manifest)
    with pytest.raises(DitreeError, match="missing parameter encoder.conv1.weight"):
        ctx.denoise_reserve(8, 1)
