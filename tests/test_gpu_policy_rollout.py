"""GPU: closed-loop policy roll-outs (ditreeonlineplanner_amd/policy_rollout.py, include/ditree.h "policy roll-outs") against the
numpy restatement of the reference loop (tests/policy_rollout_ref.py), against the expansion round whose kernels the goldens
pin, against separate denoiser calls, against the oracle network, and ``rollout_manager.rollout`` on the reference's
validation scenario file."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from oracle import denoiser as OD
from oracle import geometry as G
from oracle.tapes import ActionTape
from tests import policy_rollout_ref as R
from tests.test_gpu_forest import car_net, ctx, dev, net_ctx  # noqa: F401
from tests.util import DATA, REPO, load_maze

pytestmark = pytest.mark.gpu

A, P_TAPE, P_NET = 8, 16, 64
MAZES = ("val_maze_7", "val_maze_10", "val_maze_15")
FIXTURE = os.path.join(REPO, "tests", "golden", "validation_scenarios_car.csv")


@functools.lru_cache(maxsize=None)
def mazes():
    return tuple(load_maze(n) for n in MAZES)


def cell_xy(k, r, c):
    return G.cell_rowcol_to_xy([r, c], mazes()[k])


def start_state(k, r, c, deg, v=0.0):
    """car_env.py:216-230: [x, y, deg2rad(deg), 0, 0, 0] rounded to float32 and widened; ``v`` set afterwards."""
    s = np.zeros(6, dtype=np.float32)
    s[:2], s[2] = cell_xy(k, r, c), np.deg2rad(deg)
    s = s.astype(np.float64)
    s[3] = v
    return s


def tape_cases():
    """Three validation mazes x 4 episodes.  Scene 0 (val_maze_7, goal cell (1, 4)): 0 = from cell (1, 5) at 180 deg at full
    throttle (success at step index 20), 1 = the same start at 0 deg, facing the wall cell (1, 6) (collides between steps 16
    and 21), 2 = that with v = 3 (collides inside chunk 0), 3 = a zero tape (never ends).  Scene 2's goal sits on the face of
    the wall above cell (1, 5) and episode 8 starts 0.2 m below it at v = 3, heading up: its first step is inside the goal
    radius AND collides -- both flags from one step.  (From a goal CELL this cannot be built: the centre of a free cell is 0.5 m
    from the wall, the two-ball test fires 0.175 m from it, and a step covers centimetres.)  The others run ActionTape rows."""
    goals = [cell_xy(0, 1, 4), cell_xy(1, 7, 1), cell_xy(2, 1, 5) + np.array([0.0, 0.5])]
    both = start_state(2, 1, 5, 90, 3.0)
    both[1] += 0.30
    starts = np.array([start_state(0, 1, 5, 180), start_state(0, 1, 5, 0), start_state(0, 1, 5, 0, 3.0), start_state(0, 1, 3, 180),
                       start_state(1, 1, 3, 180), start_state(1, 1, 3, 180, 2.0), start_state(1, 3, 3, 0, 1.0),
                       start_state(1, 5, 4, 180, 1.5),
                       both, start_state(2, 1, 5, 270), start_state(2, 1, 5, 270, 2.0), start_state(2, 3, 7, 0, 1.0)])
    scene_of = np.repeat([0, 1, 2], 4)
    at = ActionTape(77, pred_horizon=P_TAPE)

    def tape_fn(c, N, P):
        a = at.actions(np.arange(N), c).astype(np.float64)
        a[[0, 1, 2, 8]] = [10.0, 0.0]
        a[3] = 0.0
        return a
    return goals, starts, scene_of, tape_fn


@functools.lru_cache(maxsize=None)
def tape_reference(M):
    goals, starts, scene_of, tape_fn = tape_cases()
    return R.run_episodes(mazes(), goals, starts, scene_of, R.tape_actions(tape_fn, len(starts), P_TAPE), A, M)


def tape_engine(ctx, goals, starts, scene_of, tape_fn, P=P_TAPE):
    from ditreeonlineplanner_amd.policy_rollout import PolicyRolloutEngine
    return PolicyRolloutEngine(ctx, list(zip(mazes(), goals)), starts, scene_of, tape_fn=tape_fn, action_horizon=A, pred_horizon=P)


class BoundSampler:
    """What PolicyRolloutEngine reads of a sampler, for the network that ``net_ctx`` has bound already."""
    def __init__(self, k=1, tables=None):
        from ditreeonlineplanner_amd.ops import CAR_NORM
        self.norm, self.num_diffusion_iters, self._tables = CAR_NORM, k, tables
        self.policy = "diffusion" if tables is not None else "flow_matching"

    def ddpm_tables(self):
        return self._tables


def net_engine(ctx, goals, starts, scene_of, k=1, tables=None):
    from ditreeonlineplanner_amd.policy_rollout import PolicyRolloutEngine
    return PolicyRolloutEngine(ctx, list(zip(mazes(), goals)), starts, scene_of, sampler=BoundSampler(k, tables), action_horizon=A,
                               pred_horizon=P_NET)


def same_results(a, b, rows=None):
    for k in ("n_steps", "success_step", "collided", "status", "best_dist", "rows", "final_state"):
        x, y = (a[k], b[k]) if rows is None else (a[k][rows], b[k])
        assert np.array_equal(x, y), k


# ---------------------------------------------------------------------- tape episodes against the restatement
@pytest.mark.parametrize("M", [20, 21, 40])
def test_tape_episodes_equal_the_restatement(ctx, M):
    from ditreeonlineplanner_amd import _lib
    ref = tape_reference(M)
    n, ss = ref["n_steps"], ref["success_step"]
    # what the case set must hold, asserted from the restatement
    assert ref["collided"][1] and not ref["succeeded"][1] and n[1] > A                         # a collision, beyond chunk 0
    assert ref["collided"][2] and n[2] <= A                                                    # a collision inside chunk 0
    assert not ref["terminated"][3] and n[3] == M                                              # an episode that never ends
    assert ref["both"][8] and n[8] == 1 and ss[8] == 0                                         # both flags from one step
    if M == 20:
        assert not ref["succeeded"][0] and n[0] == 20                                          # not reached with 20 steps
    else:
        assert ref["succeeded"][0] and not ref["collided"][0] and ss[0] == 20 and n[0] == 21   # a success ...
    if M == 21:
        assert ss[0] == M - 1                                                                  # ... on the very last allowed step
    goals, starts, scene_of, tape_fn = tape_cases()
    eng = tape_engine(ctx, goals, starts, scene_of, tape_fn)
    res = eng.run(M)
    assert eng.chunks_run == ref["chunks"]
    assert np.array_equal(res["n_steps"], n) and np.array_equal(res["success_step"], ss)
    assert np.array_equal(res["collided"], ref["collided"])
    code = res["status"] & 0xFF
    assert np.array_equal((code == _lib.EP_SUCCESS) | (code == _lib.EP_COLLIDED), ref["terminated"])
    assert np.array_equal((res["status"] & _lib.ST_FLAG_GOAL_AT_COLLISION) != 0, ref["both"])
    assert np.array_equal(code == _lib.EP_OUT_OF_STEPS, ~ref["terminated"])
    for k in ("rows", "final_state", "best_dist"):
        err = np.abs(res[k] - ref[k]).max()
        print(f"POLICY_ROLLOUT_TAPE M={M} {k} max |d| = {err:.3e}")
        assert err < 1e-9, (k, err)
    assert np.array_equal(eng.trajectory(res), R.fill_forward(dict(ref, rows=res["rows"], final_state=res["final_state"]), M))
    # a second run of the same engine starts from scratch
    same_results(eng.run(M), res)


# ---------------------------------------------------------------------- an episode is an expansion candidate from the root
def round_cases():
    """Per scene ONE start (the root of that scene's tree) and a goal cell; E = 4 episodes per scene differ by their tape /
    noise rows.  Scene 0 is the full-throttle run into the goal cell (success at step 20 < 32)."""
    goals = [cell_xy(0, 1, 4), cell_xy(1, 1, 1), cell_xy(2, 3, 5)]
    roots = [start_state(0, 1, 5, 180), start_state(1, 1, 3, 180, 2.0), start_state(2, 1, 5, 270, 2.0)]
    return goals, roots


def check_episodes_equal_round_edges(ctx, res, goals, roots, early_exit, P, inject=None, noise=None):
    from ditreeonlineplanner_amd import _lib
    from ditreeonlineplanner_amd.engine import ExpansionEngine
    E, M, nC = 4, 32, 4
    seen = set()
    for k, maze in enumerate(mazes()):
        goal_state = np.array([*goals[k], 0, 0, 0, 0])
        eng = ExpansionEngine(ctx, maze, roots[k], goal_state, edge_length=M, action_horizon=A, pred_horizon=P, batch=E,
                              capacity=16, early_exit=early_exit)
        assert np.array_equal(eng.env_goal, goals[k])
        sl = slice(k * E, (k + 1) * E)
        kw = dict(inject_actions=inject[sl].contiguous()) if inject is not None else dict(noise=noise[sl].contiguous())
        eng.expand_round(dev(np.tile(roots[k], (E, 1))), dev(np.tile(goals[k], (E, 1))), accept=False, **kw)
        rb = eng.rb
        st, cs = rb.status[:E].cpu().numpy(), rb.chunk_steps[:E].cpu().numpy()
        states, actions, end = rb.states[:E].cpu().numpy(), rb.actions[:E].cpu().numpy(), rb.end_state[:E].cpu().numpy()
        for e in range(E):
            i = k * E + e
            n = int(res["n_steps"][i])
            want = res["status"][i] if (res["status"][i] & 0xFF) != _lib.EP_OUT_OF_STEPS else _lib.ST_OK
            assert st[e] == want, (i, st[e], want)
            seen.add(int(st[e]) & 0xFF)
            assert np.array_equal(cs[e], np.clip(n - A * np.arange(nC), 0, A)), i
            assert np.array_equal(end[e], res["final_state"][i]), i
            after = np.concatenate([res["rows"][i, :n, :6], res["final_state"][i][None]])      # the state after step t - 1 at row t
            for j in range(nC):
                s = int(cs[e, j])
                if s == 0:
                    continue
                assert np.array_equal(states[e, j, :s + 1], after[A * j: A * j + s + 1]), (i, j)
                assert np.array_equal(actions[e, j, :s], res["rows"][i, A * j: A * j + s, 6:]), (i, j)
    return seen


@pytest.mark.parametrize("early_exit", [False, True])
def test_tape_episodes_equal_single_tree_round_edges(ctx, early_exit):
    from ditreeonlineplanner_amd import _lib
    goals, roots = round_cases()
    at = ActionTape(78, pred_horizon=P_TAPE)
    N = 12
    tapes = np.stack([at.actions(np.arange(N), c).astype(np.float64) for c in range(4)], axis=1)       # (N, n_chunks, P, 2)
    tapes[0] = [10.0, 0.0]
    eng = tape_engine(ctx, goals, np.repeat(np.array(roots), 4, axis=0), np.repeat([0, 1, 2], 4), lambda c, n, p: tapes[:, c])
    res = eng.run(32)
    seen = check_episodes_equal_round_edges(ctx, res, goals, roots, early_exit, P_TAPE, inject=dev(tapes))
    assert {_lib.ST_GOAL, _lib.ST_COLLIDED} <= seen


@pytest.mark.parametrize("early_exit", [False, True])
def test_network_episodes_equal_single_tree_round_edges(net_ctx, early_exit):
    goals, roots = round_cases()
    gen = torch.Generator(device="cuda").manual_seed(21)
    noise = torch.randn((12, 4, P_NET, 2), generator=gen, device="cuda")
    eng = net_engine(net_ctx, goals, np.repeat(np.array(roots), 4, axis=0), np.repeat([0, 1, 2], 4))
    res = eng.run(32, noise_fn=lambda c: noise[:, c].contiguous())
    check_episodes_equal_round_edges(net_ctx, res, goals, roots, early_exit, P_NET, noise=noise)


# ---------------------------------------------------------------------- the network path equals a tape of separate sampler calls
def net_cases():
    """Mixed starts on the three mazes; episodes 2 and 8 face a wall 0.5 m ahead at v = 3 (they end in chunk 0 unless the policy
    brakes or steers hard)."""
    goals = [cell_xy(0, 5, 3), cell_xy(1, 7, 1), cell_xy(2, 13, 4)]                             # the fixture's goal cells
    starts = np.array([start_state(0, 1, 5, 180), start_state(0, 1, 5, 180, 1.0), start_state(0, 1, 5, 0, 3.0),
                       start_state(0, 3, 3, 0, 2.0),
                       start_state(1, 1, 3, 180), start_state(1, 1, 3, 180, 2.0), start_state(1, 3, 3, 0, 1.0),
                       start_state(1, 5, 4, 180, 1.5),
                       start_state(2, 1, 5, 90, 3.0), start_state(2, 1, 5, 270), start_state(2, 1, 5, 270, 2.0),
                       start_state(2, 3, 7, 0, 1.0)])
    return goals, starts, np.repeat([0, 1, 2], 4)


def separate_sampler_call(ctx, eng, noise, k, tables=None, z=None):
    """The chunk's actions for the WHOLE batch from the public single ops on the engine's current state: one local-map call per
    maze, one conditioning call, one denoiser call."""
    from ditreeonlineplanner_amd.common.fm_utils import get_timesteps
    from ditreeonlineplanner_amd.ops import CAR_NORM
    lm = torch.empty(eng.N, 20, 20, dtype=torch.float32, device="cuda")
    for s, maze in enumerate(mazes()):
        rows = torch.as_tensor(np.nonzero(eng.scene_of == s)[0], device="cuda")
        ctx.upload_maze(maze)
        lm[rows] = ctx.local_map(eng.state[rows].contiguous(), n=20, scale=0.2, s_global=1.0, scaled=True)
    cond = ctx.cond_vector(eng.state, eng.last_action, eng.has_prev, eng.goal_xy, 20, CAR_NORM)
    if tables is not None:
        return ctx.denoise_ddpm(noise, z, lm, cond, tables[0], tables[1], act_norm=CAR_NORM[12:16])
    t0, dt = get_timesteps("exp", k, 4.0)
    return ctx.denoise(noise, lm, cond, t0=t0.numpy(), dt=dt.numpy(), act_norm=CAR_NORM[12:16])


@pytest.mark.parametrize("k,ddpm", [(1, False), (4, False), (4, True)])
def test_network_path_equals_a_tape_of_separate_sampler_calls(net_ctx, k, ddpm):
    ctx = net_ctx
    tables = None
    if ddpm:
        from ditreeonlineplanner_amd.ddpm import DDPMScheduler, ddpm_tables
        tables = ddpm_tables(DDPMScheduler(num_train_timesteps=k, beta_schedule="squaredcos_cap_v2", clip_sample=True,
                                           prediction_type="epsilon"), k)
    goals, starts, scene_of = net_cases()
    M = 16
    from ditreeonlineplanner_amd.ops import Context
    eng = net_engine(ctx, goals, starts, scene_of, k, tables)
    ctx2 = Context(0)                                  # a ctx follows one batch at a time: the tape twin lives on its own
    try:
        twin = tape_engine(ctx2, goals, starts, scene_of, lambda *a: None, P=P_NET)      # driven chunk by chunk below
        gen = torch.Generator(device="cuda").manual_seed(31 + k)
        eng.begin(M)
        twin.begin(M)
        for c in range(M // A):
            noise = torch.randn((eng.N, P_NET, 2), generator=gen, device="cuda")
            z = torch.randn((eng.N, k, P_NET, 2), generator=gen, device="cuda") if ddpm else None
            acts = separate_sampler_call(ctx, eng, noise, k, tables, z)
            n_a, n_b = eng.chunk(noise=noise, step_noise=z), twin.chunk(tape=acts.contiguous())
            assert n_a == n_b
            same_results(eng.results(), twin.results())
            if n_a == 0:
                break
        assert eng.results()["n_steps"].max() > A      # a second chunk saw the previous action
    finally:
        ctx2.close()


# ---------------------------------------------------------------------- the network path against the oracle network
def test_network_episodes_match_the_oracle_network(net_ctx):
    """16 steps = two chunks: flags exact, states within the 1e-5 that tests/test_gpu_round_precision.py holds chained chunks
    to.  (No further: a closed loop amplifies the 1e-6 deviation of the denoiser.)"""
    torch.manual_seed(0)
    onet = OD.init_noise_pred_net().eval()             # the weights net_ctx bound
    goals, starts, scene_of = net_cases()
    M = 16
    noise = torch.randn((2, len(starts), P_NET, 2), generator=torch.Generator().manual_seed(41))
    ref = R.run_episodes(mazes(), goals, starts, scene_of, R.oracle_actions(onet)(lambda c: noise[c].numpy()), A, M)
    eng = net_engine(net_ctx, goals, starts, scene_of)
    res = eng.run(M, noise_fn=lambda c: noise[c].cuda().contiguous())
    assert np.array_equal(res["n_steps"], ref["n_steps"]) and np.array_equal(res["success_step"], ref["success_step"])
    assert np.array_equal(res["collided"], ref["collided"])
    err = max(np.abs(res["rows"][..., :6] - ref["rows"][..., :6]).max(), np.abs(res["final_state"] - ref["final_state"]).max())
    print(f"POLICY_ROLLOUT_ORACLE max |d state| = {err:.3e}")
    assert err < 1e-5, err


# ---------------------------------------------------------------------- skipping terminated episodes changes nobody else
def test_skipping_terminated_episodes_changes_nobody_else(net_ctx):
    goals, starts, scene_of = net_cases()
    M = 24
    noise = torch.randn((3, len(starts), P_NET, 2), generator=torch.Generator(device="cuda").manual_seed(51), device="cuda")
    res = net_engine(net_ctx, goals, starts, scene_of).run(M, noise_fn=lambda c: noise[c].contiguous())
    alone = np.nonzero(res["n_steps"] == M)[0]
    early = np.nonzero(res["n_steps"] <= A)[0]
    assert 0 < len(alone) < len(starts) and len(early) > 0       # someone left the batch after chunk 0, someone ran to the end
    sub = net_engine(net_ctx, goals, starts[alone], scene_of[alone])
    idx = torch.as_tensor(alone, device="cuda")
    same_results(res, sub.run(M, noise_fn=lambda c: noise[c][idx].contiguous()), rows=alone)


# ---------------------------------------------------------------------- rollout(...) on the reference's validation file
def test_rollout_on_the_validation_scenarios(car_net, monkeypatch):
    from ditreeonlineplanner_amd import policy_rollout as PR
    from ditreeonlineplanner_amd.rollout_manager import rollout
    E, M = 4, 24
    captured = []
    run = PR.PolicyRolloutEngine.run

    def spy(self, *a, **k):
        captured.append((self, run(self, *a, **k)))
        return captured[-1][1]
    monkeypatch.setattr(PR.PolicyRolloutEngine, "run", spy)
    torch.manual_seed(5)
    before = torch.cuda.get_rng_state().clone()
    out, frames = rollout("carmaze", "flow_matching", car_net, None, max_episode_steps=M, num_diffusion_iters=1, local_map_size=20,
                          scale=0.2, pred_horizon=P_NET, action_horizon=A, envs_per_scenario=E, render=True,
                          scenarios_file=FIXTURE, maps_folder=DATA)
    after = torch.cuda.get_rng_state().clone()
    eng, res = captured[0]
    assert frames == [] and [o["scenario_name"] for o in out] == ["val_maze_small", "val_maze_large", "val_maze_xlarge"]
    keys = ["scenario_name", "maze", "start_rowcol", "goal_rowcol", "start_position", "goal_position", "best_dist",
            "step_to_completion", "trajectory", "collision_count"]
    cells = [((1, 5), (5, 3)), ((1, 3), (7, 1)), ((1, 5), (13, 4))]
    for k, o in enumerate(out):
        assert list(o.keys()) == keys
        assert o["start_rowcol"] == cells[k][0] and o["goal_rowcol"] == cells[k][1]
        assert np.array_equal(o["maze"], mazes()[k])
        assert np.array_equal(o["start_position"], cell_xy(k, *cells[k][0]))
        assert np.array_equal(o["goal_position"], cell_xy(k, *cells[k][1]))
        for name, shape in (("best_dist", (E,)), ("step_to_completion", (E,)), ("collision_count", (E,)),
                            ("trajectory", (E, M + 1, 8))):
            assert o[name].shape == shape and o[name].dtype == np.float64, name
        assert set(np.unique(o["collision_count"])) <= {0.0, 1.0} and (o["step_to_completion"] >= -1).all()
    # the start rows are CarEnv.reset's float32 values, the same for every env of a scenario
    assert np.array_equal(out[0]["trajectory"][:, 0, :6], np.tile(start_state(0, 1, 5, 180), (E, 1)))
    # trajectory = the restatement's fill-forward of the per-episode results
    code = res["status"] & 0xFF
    ref = dict(res, terminated=(code == 1) | (code == 2))
    assert np.array_equal(np.concatenate([o["trajectory"] for o in out]), R.fill_forward(ref, M))
    assert np.array_equal(np.concatenate([o["step_to_completion"] for o in out]), res["success_step"].astype(np.float64))
    # the generator is where one (N, P, 2) randn per executed chunk leaves it
    chunks = -(-int(res["n_steps"].max()) // A)
    assert eng.chunks_run == chunks
    torch.cuda.set_rng_state(before)
    for _ in range(chunks):
        torch.randn((3 * E, P_NET, 2), device="cuda")
    assert torch.equal(torch.cuda.get_rng_state(), after)


# ---------------------------------------------------------------------- refusals and bad arguments: nothing launched
def test_refusals_and_bad_arguments_launch_nothing(net_ctx):
    from ditreeonlineplanner_amd import _lib
    from ditreeonlineplanner_amd.model import NoisePredNet
    from ditreeonlineplanner_amd.ops import CAR_NORM, Context
    from ditreeonlineplanner_amd.rollout_manager import rollout
    L = _lib.lib()
    goals, starts, scene_of, tape_fn = tape_cases()
    eng = tape_engine(net_ctx, goals, starts, scene_of, tape_fn, P=P_NET)
    eng.begin(16)
    arrays = (eng.state, eng.rows, eng.n_steps, eng.success_step, eng.collided, eng.status, eng.best_dist, eng.last_action,
              eng.goal_xy)
    for t in arrays:
        t.fill_(-7)
    tape = torch.zeros(eng.N, P_NET, 2, dtype=torch.float64, device="cuda")
    noise = torch.zeros(eng.N, P_NET, 2, dtype=torch.float32, device="cuda")
    n = C.c_int32(-5)
    keep = []

    def params(**kw):
        pp = _lib.PolicyParams()
        pp.step_limit, pp.P, pp.K, pp.lm_n, pp.lm_size, pp.s_global = 16, P_NET, 1, 20, 20.0, 1.0
        for name, arr, ty in (("t0", [0.0], C.c_float), ("dt", [1.0], C.c_float), ("norm", CAR_NORM, C.c_double),
                              ("axis", eng.axis, C.c_double)):
            a = np.ascontiguousarray(arr, dtype=np.float32 if ty is C.c_float else np.float64)
            keep.append(a)
            setattr(pp, name, a.ctypes.data_as(C.POINTER(ty)))
        pp.noise = noise.data_ptr()
        for k, v in kw.items():
            setattr(pp, k, v)
        return pp

    def chunk(desc, pp, h=net_ctx._h, stream=None):
        rc = L.ditree_policy_chunk(h, C.byref(desc), C.byref(pp), C.byref(n), net_ctx.stream if stream is None else stream)
        return rc, L.ditree_last_error(h)

    def batch(**kw):
        d = _lib.PolicyBatch.from_buffer_copy(eng.desc)
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    for desc, pp, code, msg in (
            (batch(), params(P=32), -1, b"pred_horizon 32 / local map 20 do not match the loaded denoiser (P 64, action_dim 2"),
            (batch(), params(lm_n=16), -1, b"do not match the loaded denoiser"),
            (batch(), params(P=4, noise=None, tape=tape.data_ptr()), -1,
             b"need 1 <= A <= 64, A <= P and 1 <= step_limit <= max_steps"),
            (batch(), params(step_limit=17), -1, b"step_limit 17, max_steps 16"),
            (batch(A=65), params(), -1, b"need 1 <= A <= 64"),
            (batch(rows=None), params(), -1, b"batch descriptor incomplete"),
            (batch(scene_host=(C.c_int32 * eng.N)(*([0] * 5 + [3] + [0] * 6))), params(), -1,
             b"episode 5 has scene id 3, out of range [0, 3)"),
            (batch(), params(noise=None), -1, b"neither noise nor an action tape"),
            (batch(), params(t0=None), -1, b"flow schedule missing"),
            (batch(), params(ddpm_coef=params().t0, K=2), -1, b"the DDPM branch needs step_noise"),
            (batch(idx=eng.n_steps.data_ptr()), params(), -3, b"call ditree_policy_begin on this batch first")):
        rc, err = chunk(desc, pp)
        assert rc == code and msg in err, (rc, err, msg)
    bad = batch(scene_host=(C.c_int32 * eng.N)(*([0] * 11 + [-1])))
    assert L.ditree_policy_begin(net_ctx._h, C.byref(bad), net_ctx.stream) == -1
    assert b"policy_begin: episode 11 has scene id -1" in L.ditree_last_error(net_ctx._h)
    torch.cuda.synchronize()
    assert n.value == -5 and all(bool((t == -7).all()) for t in arrays)
    # no scene table; a denoiser that is not the car's
    other = Context(0)
    try:
        rc = L.ditree_policy_chunk(other._h, C.byref(eng.desc), C.byref(params()), C.byref(n), other.stream)
        assert rc == -3 and b"policy_chunk: no scene table uploaded" in L.ditree_last_error(other._h)
        other.upload_scenes(list(mazes()), np.stack(goals))
        NoisePredNet(input_dim=8, additional_global_cond_dim=97, pred_horizon=16, local_map_size=16, seed=0).bind(
            other, precision=_lib.PREC_F16X3, max_batch=1)
        rc = L.ditree_policy_chunk(other._h, C.byref(eng.desc), C.byref(params(P=16, lm_n=16)), C.byref(n), other.stream)
        assert rc == -1 and b"action_dim 8, map 16, cond 97; the car's is action_dim 2, cond 7" in L.ditree_last_error(other._h)
    finally:
        other.close()
    torch.cuda.synchronize()
    assert n.value == -5 and all(bool((t == -7).all()) for t in arrays)
    # the Python surface: every refusal by name, before the sampler or the engine exist
    for kw, msg in ((dict(env_id="antmaze"), "only the car"), (dict(env_id="pointmaze"), "only the car"),
                    (dict(env_id="drone_forest"), "only the car"),
                    (dict(prediction_type="observations"), "prediction_type='observations'"), (dict(obs_history=2), "obs_history=2"),
                    (dict(action_history=0), "action_history=0"), (dict(position_conditioned=True), "position_conditioned=True"),
                    (dict(local_map_conditioned=False), "local_map_conditioned=False")):
        args = dict(env_id="carmaze", policy="flow_matching", ema_noise_pred_net=None, noise_scheduler=None)
        args.update(kw)
        with pytest.raises(NotImplementedError, match=msg):
            rollout(**args, scenarios_file="/nonexistent.csv")
    with pytest.raises(ValueError, match="exactly one of sampler / tape_fn"):
        from ditreeonlineplanner_amd.policy_rollout import PolicyRolloutEngine
        PolicyRolloutEngine(net_ctx, list(zip(mazes(), goals)), starts, scene_of)
    with pytest.raises(ValueError, match=r"every id must lie in \[0, 3\)"):
        tape_engine(net_ctx, goals, starts, np.repeat([0, 1, 3], 4), tape_fn)
    torch.cuda.synchronize()
    assert all(bool((t == -7).all()) for t in arrays)
