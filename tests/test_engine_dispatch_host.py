"""CPU: what each of the seven engine classes hands to the library for one round and one fallback -- the entry points and their
order, the descriptors and the trailing arguments -- and the one root row every reset writes.  No device: the library handle
``_lib.lib()`` returns is a recorder for the test (every call noted with its by-reference structures copied at call time,
since the fake returns before anything is read), the context is a stub on CPU tensors."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from ditreeonlineplanner_amd import _lib
from ditreeonlineplanner_amd import engine as E
from ditreeonlineplanner_amd import forest as F

BYREF = type(C.byref(C.c_int()))
T, CAP, COUNTS = 2, 8, [3, 1]
B = sum(COUNTS)
PD_ROWS = {"ditree_fallback_select": 1, "ditree_forest_fallback": 1, "ditree_forest_fallback_ant": 1,
           "ditree_forest_fallback_goals": T, "ditree_forest_fallback_goals_ant": T}


class Call(types.SimpleNamespace):
    """One library call: ``name``, ``raw`` (the arguments as given), ``args`` (by-reference structures copied), ``goal`` (the
    two doubles behind the parameter block's goal field), ``off`` (a forest's host offsets), ``pd`` (a fallback's goal rows)."""


class Recorder:
    """Stands in for the ctypes handle: notes every call, makes the argument check ctypes would make, returns 0 (12 for
    ditree_record_doubles)."""

    def __init__(self):
        self.calls, self.problems = [], []

    def event(self, name, **kw):
        self.calls.append(Call(name=name, raw=(), args=(), **kw))

    def __getattr__(self, name):
        if name not in _lib.SIGNATURES:
            raise AttributeError(name)
        argtypes = _lib.SIGNATURES[name][1]

        def fn(*raw):
            call = Call(name=name, raw=raw, args=[], goal=None, off=None, pd=None)
            if len(raw) != len(argtypes):
                self.problems.append(f"{name}: {len(raw)} arguments, the signature lists {len(argtypes)}")
            for i, (a, ty) in enumerate(zip(raw, argtypes)):
                try:
                    ty.from_param(a)
                except (TypeError, C.ArgumentError) as e:
                    self.problems.append(f"{name}: argument {i} ({a!r}) is no {ty.__name__}: {e}")
                if isinstance(a, BYREF):
                    obj = a._obj
                    a = type(obj).from_buffer_copy(obj)
                    if isinstance(obj, (_lib.RoundParams, _lib.AntRoundParams)):
                        g = obj.goal_xy if isinstance(obj, _lib.RoundParams) else obj.desired_goal
                        call.goal = (g[0], g[1])
                    if isinstance(obj, _lib.Forest):
                        call.off = [obj.off_host[k] for k in range(obj.n_trees + 1)]
                elif ty is _lib._pd and a is not None and name in PD_ROWS and call.pd is None:
                    call.pd = [a[k] for k in range(2 * PD_ROWS[name])]
                call.args.append(a)
            self.calls.append(call)
            return 12 if name == "ditree_record_doubles" else 0
        return fn

    def names(self):
        return [c.name for c in self.calls if c.name != "ditree_record_doubles"]


class StubContext:
    def __init__(self, rec):
        self.device, self._h, self.stream = torch.device("cpu"), C.c_void_p(0x1000), None
        self.maze_owner = self.scenes_owner = None
        self.rec = rec

    def upload_maze(self, maze, owner=None):
        self.rec.event("upload_maze", owner=owner)
        self.maze_owner = owner

    def upload_scenes(self, mazes, goal_xy, owner=None):
        self.rec.event("upload_scenes", owner=owner)
        self.scenes_owner = owner


@pytest.fixture
def rec(monkeypatch):
    r = Recorder()
    monkeypatch.setattr(_lib, "_LIB", r)                       # restored afterwards
    return r


# ---------------------------------------------------------------------- the engines under test
MAZE = np.zeros((6, 6), dtype=np.float32)
MAZE[2, 3] = 1
MAZE2 = np.zeros((6, 6), dtype=np.float32)
MAZE2[4, 1] = 1
CAR_START, CAR_GOAL = np.array([-2.2, -2.1, 0.3, 0, 0, 0.0]), np.array([2.2, 2.3, 0, 0, 0, 0.0])
CAR_START2, CAR_GOAL2 = np.array([-1.2, 2.1, 0.1, 0, 0, 0.0]), np.array([1.4, -2.3, 0, 0, 0, 0.0])
ANT_START, ANT_GOAL = np.arange(29) * 0.01 - 4.0, np.arange(29) * 0.02 + 3.0
ANT_START2, ANT_GOAL2 = np.arange(29) * 0.03 - 6.0, np.arange(29) * 0.01 + 5.0
CAR_KW = dict(action_horizon=8, pred_horizon=16, local_map_size=10, batch=8, k_steps=2, early_exit=True)
ANT_KW = dict(norm=np.linspace(0.5, 1.5, 70), edge_length=4, action_horizon=2, pred_horizon=4, local_map_size=6, batch=8,
              k_steps=2, early_exit=True, ball_radius=1.1)
CAR_SCENES = [(MAZE, CAR_START, CAR_GOAL, None), (MAZE2, CAR_START2, CAR_GOAL2, np.array([1.25, -2.75]))]
ANT_SCENES = [(MAZE, ANT_START, ANT_GOAL, None), (MAZE2, ANT_START2, ANT_GOAL2, np.array([5.5, 6.5]))]

# kind -> (class, forest, scenes, ant)
KINDS = {"single": (E.ExpansionEngine, False, False, False), "forest": (F.ForestEngine, True, False, False),
         "scene": (F.SceneForestEngine, True, True, False), "ant": (E.AntExpansionEngine, False, False, True),
         "ant_forest": (F.AntForestEngine, True, False, True), "ant_scene": (F.AntSceneForestEngine, True, True, True)}

#        kind, solution / dynamics, schedule, expand entries, accept entry, accept's trailing argument, fallback entry
TABLE = [
    ("single", "first", False, ["ditree_expand_round"], "ditree_accept", "sticky", "ditree_fallback_select"),
    ("single", "first", True, ["ditree_chunk_budget", "ditree_expand_round"], "ditree_accept", "sticky", "ditree_fallback_select"),
    ("single", "best_of_round", False, ["ditree_expand_round"], "ditree_accept_best", "cost", "ditree_fallback_select"),
    ("single", "anytime", True, ["ditree_chunk_budget", "ditree_expand_round"], "ditree_accept_best", "cost", "ditree_fallback_select"),
    ("single", "anytime_pruned", False, ["ditree_expand_round_bounded"], "ditree_accept_bounded", "bound", "ditree_fallback_select"),
    ("forest", "first", False, ["ditree_forest_expand_round"], "ditree_forest_accept", "sticky", "ditree_forest_fallback"),
    ("forest", "first", True, ["ditree_forest_chunk_budget", "ditree_forest_expand_round"], "ditree_forest_accept", "sticky",
     "ditree_forest_fallback"),
    ("forest", "best_of_round", True, ["ditree_forest_chunk_budget", "ditree_forest_expand_round"], "ditree_forest_accept_best",
     "cost", "ditree_forest_fallback"),
    ("forest", "anytime", False, ["ditree_forest_expand_round"], "ditree_forest_accept_best", "cost", "ditree_forest_fallback"),
    ("forest", "anytime_pruned", False, ["ditree_forest_expand_round_bounded"], "ditree_forest_accept_bounded", "bound",
     "ditree_forest_fallback"),
    ("scene", "first", False, ["ditree_forest_expand_round_scenes"], "ditree_forest_accept", "sticky",
     "ditree_forest_fallback_goals"),
    ("scene", "best_of_round", False, ["ditree_forest_expand_round_scenes"], "ditree_forest_accept_best", "cost",
     "ditree_forest_fallback_goals"),
    ("scene", "anytime", True, ["ditree_forest_chunk_budget", "ditree_forest_expand_round_scenes"], "ditree_forest_accept_best",
     "cost", "ditree_forest_fallback_goals"),
    ("scene", "anytime_pruned", False, ["ditree_forest_expand_round_bounded"], "ditree_forest_accept_bounded", "bound",
     "ditree_forest_fallback_goals"),
    ("ant", "tape", False, ["ditree_expand_round_ant"], "ditree_accept", "sticky", "ditree_fallback_select"),
    ("ant", "model", False, ["ditree_expand_round_ant"], "ditree_accept", "sticky", "ditree_fallback_select"),
    ("ant", "host", False, ["ditree_ant_round_begin"] + ["ditree_ant_chunk_sample", "ditree_ant_chunk_step"] * 2, "ditree_accept",
     "sticky", "ditree_fallback_select"),
    ("ant_forest", "tape", False, ["ditree_forest_expand_round_ant"], "ditree_forest_accept_ant", None, "ditree_forest_fallback_ant"),
    ("ant_scene", "tape", False, ["ditree_forest_expand_round_ant_scenes"], "ditree_forest_accept_ant", None,
     "ditree_forest_fallback_goals_ant"),
]


def make_engine(rec, kind, mode, schedule=False, **more):
    cls, forest, scenes, ant = KINDS[kind]
    ctx = StubContext(rec)
    if ant:
        kw = dict(ANT_KW, dynamics=mode, **more)
        single = (MAZE, ANT_START, ANT_GOAL)
    else:
        kw = dict(CAR_KW, solution=mode, emulate_sticky_done=mode == "first", **more)
        kw["prop_duration" if schedule else "edge_length"] = [8, 16] if schedule else 16
        single = (MAZE, CAR_START, CAR_GOAL)
    if scenes:
        eng = cls(ctx, ANT_SCENES if ant else CAR_SCENES, T, CAP, **kw)
    elif forest:
        eng = cls(ctx, *single, T, CAP, **kw)
    else:
        eng = cls(ctx, *single, capacity=2 * CAP, **kw)
    return eng, ctx


def round_inputs(eng, ant, n=B):
    S, D = eng.STATE_DIM, eng.ACTION_DIM
    g = torch.Generator().manual_seed(3)
    samples = torch.rand(n, S, dtype=torch.float64, generator=g)
    cond = torch.rand(n, 2, dtype=torch.float64, generator=g)
    acts = torch.rand(n, eng.n_chunks, eng.P, D, dtype=torch.float64, generator=g)
    extra = {}
    if ant and eng.dynamics == "tape":
        extra["next_obs_tape"] = torch.rand(n, eng.n_chunks, eng.A, 29, dtype=torch.float64, generator=g)
    if ant and eng.dynamics == "host":
        extra["step_fn"] = lambda j, start, actions, rows: np.zeros((rows.size, actions.shape[1], 29))
    return samples, cond, acts, extra


def ptr(t, lo=0):
    return t[lo:].data_ptr()


def as_int(v):
    return v.value if isinstance(v, C.c_void_p) else v


def check_round_desc(rd, eng, lo, n, own=None, shard=0):
    own_lo, own_n = (0, n) if own is None else own
    assert (rd.B, rd.own_lo, rd.own_n, rd.shard) == (n, own_lo, own_n, shard)
    assert rd.parent == ptr(eng.rb.parent, lo) and rd.status == ptr(eng.rb.status, lo) and rd.node_id == ptr(eng.rb.node_id, lo)
    assert rd.states == ptr(eng.rb.states, lo) and rd.actions == ptr(eng.rb.actions, lo)


def check_params(call, rp, eng, ant, lo, n, samples, cond, acts, extra, schedule, n_nodes=1):
    assert isinstance(rp, _lib.AntRoundParams if ant else _lib.RoundParams)
    assert (rp.n_nodes, rp.P, rp.K, rp.lm_n, rp.early_exit) == (n_nodes, eng.P, 2, eng.lm_n, 1)
    assert rp.samples == ptr(samples, lo) and rp.cond_goal == ptr(cond, lo) and rp.inject_actions == ptr(acts, lo)
    assert rp.noise is None and not rp.ddpm_coef
    assert rp.step_noise is None
    assert call.goal == tuple(float(v) for v in eng.env_goal[:2])
    assert rp.lm_size == float(eng.goal_scale) and rp.s_global == float(eng.s_global)
    if ant:
        assert rp.goal_radius == 0.45 * 4.0 and rp.ball_radius == 1.1
        assert rp.dynamics == (_lib.ANT_DYN_MODEL if eng.dynamics == "model" else _lib.ANT_DYN_TAPE)
        tape = extra.get("next_obs_tape")
        assert rp.next_obs_tape == (None if tape is None else ptr(tape, lo))
        assert rp.cond_out is None
    else:
        assert rp.chunk_budget == (ptr(eng._budget, lo) if schedule else None)


def check_bound(bd, eng, stats):
    assert (bd.cost, bd.key, bd.stats) == (eng.tree.cost.data_ptr(), eng.tree.key.data_ptr(), stats.data_ptr())
    assert bd.goal_radius == 0.5 and bd.reach == E.CAR_REACH


def check_forest_desc(call, fd, eng, counts):
    assert (fd.n_trees, fd.tree_capacity) == (T, CAP)
    assert fd.counters == eng.fcounters.data_ptr() and fd.off == eng.off_dev.data_ptr()
    assert call.off == [0] + list(np.cumsum(counts))


def check_leading(call, eng, forest):
    """Context handle, the engine's own tree descriptor, then the forest descriptor; the stream last."""
    assert call.raw[0] is eng.ctx._h and call.raw[1]._obj is eng.tree.desc and call.raw[-1] is eng.ctx.stream
    assert bytes(call.args[1]) == bytes(eng.tree.desc)
    if forest:
        assert call.raw[2]._obj is eng.fdesc
        check_forest_desc(call, call.args[2], eng, COUNTS)


@pytest.mark.parametrize("kind,mode,schedule,expand,accept,trailing,fallback", TABLE,
                         ids=[f"{r[0]}-{r[1]}{'-schedule' if r[2] else ''}" for r in TABLE])
def test_one_round_and_one_fallback_reach_the_library_as_at_the_parent(rec, kind, mode, schedule, expand, accept, trailing,
                                                                       fallback):
    _, forest, scenes, ant = KINDS[kind]
    eng, ctx = make_engine(rec, kind, mode, schedule)
    pruned = mode == "anytime_pruned"
    roots = [0, CAP] if forest else [0]                         # the roots the constructor's reset wrote
    if scenes:
        eng.reset_tree(1, 1)                                    # tree 1 on the second scene
        roots.append(CAP)
    upload = "upload_scenes" if scenes else "upload_maze"
    assert any(c.name == upload and c.owner is eng for c in rec.calls)
    ctx.maze_owner = ctx.scenes_owner = None                    # someone else's upload since
    rec.calls.clear()
    samples, cond, acts, extra = round_inputs(eng, ant)
    if forest:
        extra["counts_per_tree"] = COUNTS
    cnt = eng.expand_round(samples, cond, inject_actions=acts, **extra)
    assert cnt.shape == ((T, 8) if forest else (8,))
    if forest:
        eng.n_nodes_host[:] = 3
        eng.fallback_nodes()
    else:
        eng.tree.n_nodes_host = 3
        eng.fallback_node()
    assert rec.problems == []
    # the sequence: this engine's upload before the first launch, the keys of the reset roots, expand, accept, fallback
    names = rec.names()
    assert names[0] == upload and rec.calls[0].owner is eng
    keys = ["ditree_bound_keys"] * len(roots) if pruned else []
    assert names[1:] == (expand[:-1] if schedule else []) + keys + (expand[-1:] if schedule else expand) + [accept, fallback]
    calls = {c.name: c for c in rec.calls}
    stats = eng.fstats if forest else eng.tree.stats
    for c in rec.calls:
        if c.name.startswith("upload") or c.name == "ditree_bound_keys":
            continue
        check_leading(c, eng, forest and c.name != "ditree_bound_keys")
    if pruned:
        got = [c for c in rec.calls if c.name == "ditree_bound_keys"]
        assert [c.raw[3:6] for c in got] == [(r, 1, CAP if forest else 0) for r in roots]
        for c in got:
            assert c.raw[1]._obj is eng.tree.desc and c.raw[2]._obj is eng.bound
            check_bound(c.args[2], eng, stats)
    # chunk budget: the whole round's samples, before its expand
    if schedule:
        c = calls[expand[0]]
        k = 3 if forest else 2
        assert c.raw[k] == samples.data_ptr() and c.raw[k + 1] == B
        if not forest:
            assert c.raw[k + 2] == 1                             # n_nodes
        assert list(c.raw[-5]) == [1, 2] and c.raw[-4] == 2
        assert c.raw[-3] == eng._budget_parent.data_ptr() and c.raw[-2] == eng._budget.data_ptr()
    # the expand calls: [scenes], round, parameters, [bound]
    for name in dict.fromkeys(expand[1:] if schedule else expand):
        c = calls[name]
        k = 3 if forest else 2
        if name in ("ditree_forest_expand_round_scenes", "ditree_forest_expand_round_ant_scenes"):
            assert c.raw[k]._obj is eng.sdesc
            k += 1
        elif name == "ditree_forest_expand_round_bounded":
            assert (c.raw[k]._obj is eng.sdesc) if scenes else (c.raw[k] is None)
            k += 1
        check_round_desc(c.args[k], eng, 0, B)
        check_params(c, c.args[k + 1], eng, ant, 0, B, samples, cond, acts, extra, schedule)
        if pruned:
            assert c.raw[k + 2]._obj is eng.bound
            check_bound(c.args[k + 2], eng, stats)
    if scenes:
        assert [eng.sdesc.tree_scene_host[t] for t in range(T)] == [0, 1]
        assert eng.sdesc.tree_scene == eng.tree_scene_dev.data_ptr()
    # accept: the round descriptor of all rows, then the sticky flag / the cost column / the bound / nothing
    c = calls[accept]
    k = 3 if forest else 2
    check_round_desc(c.args[k], eng, 0, B)
    assert len(c.raw) == k + (2 if trailing is None else 3)
    if trailing == "sticky":
        assert c.raw[k + 1] == (0 if ant else 1)
    elif trailing == "cost":
        assert c.raw[k + 1] == eng.tree.cost.data_ptr()
    elif trailing == "bound":
        assert c.raw[k + 1]._obj is eng.bound
        check_bound(c.args[k + 1], eng, stats)
    # fallback: each tree's goal_state[:2]
    c = calls[fallback]
    if not forest:
        assert c.raw[2] == 3 and c.raw[4] is None and c.raw[5] == 0
        assert c.pd == list(eng.goal_state[:2])
    elif scenes:
        assert c.pd == [*eng.scene_goals[0][:2], *eng.scene_goals[1][:2]]
    else:
        assert c.pd == list(eng.goal_state[:2])


@pytest.mark.parametrize("kind,mode", [("forest", "first"), ("forest", "anytime_pruned"), ("scene", "best_of_round"),
                                       ("ant_forest", "tape"), ("ant_scene", "model")])
def test_a_forest_round_without_candidates_calls_nothing(rec, kind, mode):
    eng, _ = make_engine(rec, kind, mode)
    ant = KINDS[kind][3]
    samples, cond, acts, extra = round_inputs(eng, ant, n=0)
    rec.calls.clear()
    before = eng.cnt_host.copy()
    cnt = eng.expand_round(samples, cond, inject_actions=acts, counts_per_tree=[0, 0], **extra)
    assert cnt is not eng.cnt_host and np.array_equal(cnt, before)
    assert eng.expand_round(samples, cond, inject_actions=acts, counts_per_tree=[0, 0], accept=False, **extra) is None
    assert rec.calls == []


@pytest.mark.parametrize("n,expect", [(4, ["ditree_expand_round", "ditree_round_pack", "allgather", "ditree_round_unpack", "ditree_accept"]),
                                      (1, ["allgather", "ditree_round_unpack", "ditree_accept"])])
def test_a_sharded_round_expands_its_own_rows_and_accepts_all(rec, monkeypatch, n, expect):
    """Rank 1 of 2: its launch covers rows [lo, hi) of every per-candidate array, the exchange and the accept cover the whole
    round with ``own`` / ``shard`` set; with an empty shard (one candidate, which is rank 0's) only the launch is skipped."""
    monkeypatch.setattr(E, "allgather_round_fields", lambda fields, per, rank, world, group=None: rec.event(
        "allgather", per=per, rank=rank, world=world))
    monkeypatch.delenv("DITREE_GATHER_EDGES", raising=False)
    eng, _ = make_engine(rec, "single", "first", rank=1, world_size=2)
    rec.calls.clear()
    samples, cond, acts, extra = round_inputs(eng, False, n=n)
    eng.expand_round(samples, cond, inject_actions=acts)
    assert rec.problems == [] and rec.names() == expect
    per = (n + 1) // 2
    lo, own_n = min(per, n), n - min(per, n)
    calls = {c.name: c for c in rec.calls}
    if own_n:
        c = calls["ditree_expand_round"]
        check_round_desc(c.args[2], eng, lo, own_n)
        check_params(c, c.args[3], eng, False, lo, own_n, samples, cond, acts, extra, False)
        check_round_desc(calls["ditree_round_pack"].args[2], eng, lo, own_n)
        assert calls["ditree_round_pack"].raw[3] == eng.rb.records[per:].data_ptr()
    rd = calls["ditree_round_unpack"].args[2]
    check_round_desc(rd, eng, 0, n, shard=per)
    assert rd.last_action == eng.rb.last_action.data_ptr() and rd.first_action == eng.rb.first_action.data_ptr()
    check_round_desc(calls["ditree_accept"].args[2], eng, 0, n, own=(lo, own_n), shard=per)
    assert (calls["allgather"].per, calls["allgather"].rank, calls["allgather"].world) == (per, 1, 2)


def test_an_action_tape_round_of_a_ddpm_engine_takes_the_flow_schedule(rec):
    eng, _ = make_engine(rec, "single", "first")
    eng.ddpm = (np.arange(5, dtype=np.float32), np.ones((5, 5), dtype=np.float32))
    samples, cond, acts, _ = round_inputs(eng, False)
    rec.calls.clear()
    eng.expand_round(samples, cond, inject_actions=acts)
    rp = next(c for c in rec.calls if c.name == "ditree_expand_round").args[3]
    assert rp.K == 2 and not rp.ddpm_coef and rp.step_noise is None and bool(rp.t0) and bool(rp.dt)
    assert eng.ddpm is not None


def test_refusals_of_a_round_keep_their_type_and_text(rec):
    eng, _ = make_engine(rec, "forest", "first")
    samples, cond, acts, _ = round_inputs(eng, False)
    with pytest.raises(ValueError, match="counts_per_tree is required"):
        eng.expand_round(samples, cond, inject_actions=acts)
    with pytest.raises(ValueError, match=r"sum\(counts_per_tree\) = 3 rows"):
        eng.expand_round(samples, cond, inject_actions=acts, counts_per_tree=[2, 1])
    with pytest.raises(ValueError, match="exceeds engine batch 8"):
        eng.expand_round(samples.repeat(3, 1), cond.repeat(3, 1), inject_actions=acts.repeat(3, 1, 1, 1), counts_per_tree=[6, 6])
    ant, _ = make_engine(rec, "ant", "host")
    samples, cond, acts, _ = round_inputs(ant, True)
    with pytest.raises(ValueError, match="step_fn is required"):
        ant.expand_round(samples, cond, inject_actions=acts)
    with pytest.raises(ValueError, match=r"samples must be \(B, 29\)"):
        ant.expand_round(samples[:, :6], cond, inject_actions=acts)
    tape, _ = make_engine(rec, "ant_forest", "tape")
    with pytest.raises(ValueError, match="dynamics='tape': next_obs_tape must be"):
        tape.expand_round(samples, cond, inject_actions=acts, counts_per_tree=COUNTS)


# ---------------------------------------------------------------------- the root row
TREE_FIELDS = ("state", "xy", "parent", "last_action", "has_prev", "num_visit", "edge_states", "edge_actions", "edge_nstates",
               "edge_nactions", "edge_owner", "hist", "hist_n", "cost", "key")


def scribble(tree, skip=()):
    """Rows written into every slot of the tree."""
    for name in TREE_FIELDS:
        t = getattr(tree, name)
        if t is not None and name not in skip:
            t.copy_((torch.arange(t.numel()).reshape(t.shape) % 5 + 2).to(t.dtype))


def columns(tree):
    return {name: getattr(tree, name).clone() for name in TREE_FIELDS if getattr(tree, name) is not None}


def check_root(got, r, span, start, ant, with_cost):
    """The root row at slot ``r`` of a tree of ``span`` slots, field by field."""
    s = torch.as_tensor(np.asarray(start, dtype=np.float64))
    assert torch.equal(got["state"][r], s) and torch.equal(got["xy"][r], s[:2])
    assert got["parent"][r] == -1 and got["has_prev"][r] == 0 and not got["last_action"][r].any()
    assert not got["num_visit"][r:r + span].any()
    assert got["edge_nstates"][r] == 0 and got["edge_nactions"][r] == 0 and got["edge_owner"][r] == -1
    if ant:
        assert not got["hist"][r, :2].any() and torch.equal(got["hist"][r, 2], s) and got["hist_n"][r] == 1
    if with_cost:
        assert got["cost"][r] == 1


@pytest.mark.parametrize("kind,mode", [("single", "first"), ("single", "anytime_pruned"), ("ant", "tape")])
def test_reset_writes_the_root_row_of_a_single_tree(rec, kind, mode):
    eng, _ = make_engine(rec, kind, mode)
    ant = KINDS[kind][3]
    tr = eng.tree
    scribble(tr, skip=("edge_owner",))                           # a single tree's root is never another rank's
    tr._cnt_buf.fill_(9)
    start = (ANT_START if ant else CAR_START) + 0.5
    eng.reset(start, ANT_GOAL if ant else CAR_GOAL)
    check_root(columns(tr), 0, tr.capacity, start, ant, mode != "first" and not ant)
    assert tr.counters.tolist() == [1, -1, 0, 0, 0, 0, 0, -1] and tr.n_nodes_host == 1
    if mode == "anytime_pruned":
        assert tr.stats.tolist() == list(E.STATS_ROOT) and list(tr.stats_host) == list(E.STATS_ROOT)


@pytest.mark.parametrize("kind,mode", [("forest", "first"), ("forest", "anytime"), ("forest", "anytime_pruned"),
                                       ("scene", "anytime_pruned"), ("ant_forest", "tape"), ("ant_scene", "tape")])
def test_reset_tree_leaves_what_reset_leaves_for_a_single_tree_of_that_capacity(rec, kind, mode):
    _, _, scenes, ant = KINDS[kind]
    eng, ctx = make_engine(rec, kind, mode)
    tr, r = eng.tree, CAP
    scribble(tr)
    eng._fcnt_buf.fill_(9)
    eng.cnt_host[:] = 9
    eng.n_nodes_host[:] = 5
    before = columns(tr)
    if scenes:
        start = (ANT_SCENES if ant else CAR_SCENES)[1][1]
        eng.reset_tree(1, 1)
    else:
        start = (ANT_START if ant else CAR_START) + 0.25
        eng.reset_tree(1, start)
    after = columns(tr)
    with_cost = mode != "first" and not ant
    check_root(after, r, CAP, start, ant, with_cost)
    # what DeviceTree.reset leaves for a single tree of that capacity, on the same rows
    one = E.DeviceTree(ctx, CAP, eng.n_chunks, eng.A, state_dim=eng.STATE_DIM, action_dim=eng.ACTION_DIM, hist=ant,
                       cost=with_cost, key=mode == "anytime_pruned")
    for name in TREE_FIELDS:
        t = getattr(one, name)
        if t is not None and name != "edge_owner":
            t.copy_(before[name][r:r + CAP])
    one.reset(start)
    for name, col in columns(one).items():
        if name == "num_visit":
            assert torch.equal(after[name][r:r + CAP], col)
        else:
            assert torch.equal(after[name][r], col[0]), name
    # the tree's counter and stats rows and their host copies; the other tree's slots and rows untouched
    assert eng.fcounters[1].tolist() == one.counters.tolist() == eng.cnt_host[1].tolist() and eng.n_nodes_host[1] == 1
    assert eng.fcounters[0].tolist() == [9] * 8 and eng.cnt_host[0].tolist() == [9] * 8 and eng.n_nodes_host[0] == 5
    if mode == "anytime_pruned":
        assert eng.fstats[1].tolist() == list(E.STATS_ROOT) == list(eng.stats_host[1]) and eng.fstats[0].tolist() == [9] * 4
    for name in after:
        keep = torch.ones(tr.capacity, dtype=torch.bool)
        keep[r:r + CAP if name == "num_visit" else r + 1] = False
        assert torch.equal(after[name][keep], before[name][keep]), name
