"""GPU: MPPI missions on the device (`ditree_mppi_missions`; facades `MPPI.follow`, `online.follow_reference`,
`mppi.follow_fleet`) against the STEPWISE path, bit for bit.

The reference of every test is the MPPI driver's loop (`run_scenarios_with_lidar_MPPI.py:417-452`) written out below with
`MPPI.step`, `MPPI.is_done` and `online.scan_and_update_maze(mppi, ...)` on a second controller with the same seed: expected
events, counts, traces, mazes and controller state all come from that loop, never from the code under test, and every
comparison is `np.array_equal` (K <= 256 is the stepwise controller's one-slice case, whose summation order the mission kernel
reproduces).  Inputs are the ones tests/test_gpu_mppi.py builds: boxes.csv, its L-shaped reference path, its wall-facing
collision state, and a true maze that is boxes plus one occupied cell on the path three cells ahead of the start, absent
from the known maze.  They were picked with the CPU restatement (oracle/mppi.py + oracle/online.py) so that the stepwise loop
sees every event code, a known-maze change by a scan, and controller steps (with collided rollouts) after it; the assertions
on that are made on the device stepwise loop.  dt = 0.02, scan_time = 0.2: a scan falls on every 11th executed step."""
import numpy as np
import pytest
import torch

from oracle import geometry as G
from tests.test_gpu_mppi import make
from tests.util import load_maze

pytestmark = pytest.mark.gpu
STEPS_DONE, GOAL, TRIALS = 0, 1, 2           # include/ditree.h DITREE_MEV_*
LAST_KEYS = ("beta", "eta", "nearest_path_index", "collided_rollouts", "effective_samples")


@pytest.fixture(scope="module")
def ctx():
    from ditreeonlineplanner_amd.ops import Context
    c = Context(0)
    yield c
    c.close()


def scenario(kind):
    """-> dict(state, truth, max_steps, allowed, U0): the mission's start state, true maze, call budget, ALLOWED_TRIALS and the
    nominal controls it starts from (None = rest)."""
    from tests.test_gpu_mppi import l_path
    maze = load_maze("boxes")
    path, _ = l_path(maze)
    truth = maze.copy()
    U0 = None
    if kind == "free":                       # along the bottom corridor at speed: 50 executed steps, scans at 11, 22, 33, 44
        state, max_steps, allowed = np.array([path[50, 0], path[50, 1], 0.0, 2.0, 0.3, 0.0]), 50, 1
    elif kind == "hidden":                   # the cell three ahead of the start is occupied in the TRUE maze only
        truth[18, 4] = 1
        state, max_steps, allowed = np.array([path[0, 0], path[0, 1], 0.0, 1.5, 0.3, 0.0]), 55, 2
    elif kind == "near_goal":                # about eleven steps short of the goal radius, heading at it
        state, max_steps, allowed = np.array([path[-52, 0], path[-52, 1], np.pi / 2, 2.5, 0.4, 0.0]), 40, 1
    elif kind in ("collision1", "collision3"):
        # nose 0.12 from the bottom wall, fast, heading into it: the executed step collides whatever the controls are
        wall_y = G.cell_rowcol_to_xy([18, 5], maze)[1] - 0.5
        state = np.array([path[300, 0], wall_y + 0.19, -np.pi / 2, 5.0, 1.0, 0.0])
        max_steps, allowed, U0 = 20, int(kind[-1]), 1.0
    else:
        raise KeyError(kind)
    return dict(state=state, truth=truth, max_steps=max_steps, allowed=allowed, U0=U0)


def controller(ctx, K, T, seed, sc, path_slice=slice(None)):
    m, maze, path, _ = make(ctx, K, T, seed=seed)
    if path_slice != slice(None):
        m.set_ref_path(path[path_slice])
    if sc["U0"] is not None:
        m._U.fill_(sc["U0"])
    return m, maze


def stepwise(m, state, known, truth, scanned, max_steps, allowed, t_acc=0.0, trials=0):
    """run_scenarios_with_lidar_MPPI.py:417-452 with at most `max_steps` controller calls."""
    from ditreeonlineplanner_amd import online
    state = np.asarray(state, dtype=np.float64).copy()
    ex_s, ex_a = [], []
    calls = scans = 0
    changed_at = None                        # the controller call whose scan first changed the known maze
    while calls < max_steps and not m.is_done(state) and trials < allowed:
        nxt, action, done = m.step(state)
        calls += 1
        if done is None:
            trials += 1
            continue
        trials = 0
        state = nxt
        m.env.set_state(state)
        ex_s.append(state.copy())
        ex_a.append(action.copy())
        t_acc += m.env.dt
        if t_acc > m.env.lidar2dsim.scan_time:
            before = known.copy()
            online.scan_and_update_maze(m, known, truth, scanned)
            scans += 1
            if changed_at is None and not np.array_equal(before, known):
                changed_at = calls
            t_acc = 0.0
    event = GOAL if m.is_done(state) else (TRIALS if trials >= allowed else STEPS_DONE)
    return dict(state=state, ex_s=np.array(ex_s).reshape(-1, 6), ex_a=np.array(ex_a).reshape(-1, 2), event=event, calls=calls,
                scans=scans, t_acc=t_acc, trials=trials, changed_at=changed_at)


def same_controller_state(f, s):
    """The fused controller `f` is where the stepwise controller `s` is."""
    assert f.counter == s.counter
    assert np.array_equal(f._U.cpu().numpy(), s._U.cpu().numpy())
    assert np.array_equal(f._state.cpu().numpy(), s._state.cpu().numpy())
    assert (f._state_host is None) == (s._state_host is None)
    if s._state_host is not None:
        assert np.array_equal(f._state_host, s._state_host)
    assert set(f.last) == set(s.last)
    for k in s.last:
        assert np.array_equal(f.last[k], s.last[k]), (k, f.last[k], s.last[k])
    assert np.array_equal(f.env.state, s.env.state) and f.env.done == s.env.done
    assert f.maze.dtype == s.maze.dtype and np.array_equal(f.maze, s.maze)
    assert np.array_equal(f.env.maze_map, s.env.maze_map)


def same_mission(out, ref, mazes_f, mazes_s):
    state, ex_s, ex_a, event, info = out
    assert event == ref["event"], (event, ref["event"])
    assert ex_s.shape == ref["ex_s"].shape and np.array_equal(ex_s, ref["ex_s"])
    assert ex_a.shape == ref["ex_a"].shape and np.array_equal(ex_a, ref["ex_a"])
    assert np.array_equal(state, ref["state"])
    assert info["controller_calls"] == ref["calls"] and info["scans"] == ref["scans"]
    assert info["trials"] == ref["trials"] and info["action_time_count"] == ref["t_acc"]
    for a, b in zip(mazes_f, mazes_s):
        assert np.array_equal(a, b)


def run_pair(ctx, K, T, kind, seed=3):
    sc = scenario(kind)
    s, maze = controller(ctx, K, T, seed, sc)
    known_s, scanned_s = maze.copy(), maze.copy()
    ref = stepwise(s, sc["state"], known_s, sc["truth"], scanned_s, sc["max_steps"], sc["allowed"])
    f, _ = controller(ctx, K, T, seed, sc)
    known_f, scanned_f = maze.copy(), maze.copy()
    out = f.follow(sc["state"], known_f, sc["truth"], scanned_f, sc["max_steps"], allowed_trials=sc["allowed"])
    same_mission(out, ref, (known_f, scanned_f), (known_s, scanned_s))
    same_controller_state(f, s)
    return ref, maze, known_s, f, s


@pytest.mark.parametrize("K,T", [(20, 16), (20, 8), (64, 8), (256, 16), (1, 8)])
def test_fused_mission_equals_the_stepwise_loop_at_every_size(ctx, K, T):
    """The hidden-obstacle mission at the driver's sizes (K = 20 is no multiple of the 64 lanes), a full work-group and the
    noise-free nominal rollout alone: a scan changes the known maze and controller steps follow the change."""
    ref, maze, known, _, _ = run_pair(ctx, K, T, "hidden")
    assert ref["scans"] >= 4 and ref["changed_at"] is not None and ref["changed_at"] < ref["calls"]
    assert known[18, 4] == 1 and maze[18, 4] == 0


@pytest.mark.parametrize("kind", ["free", "hidden", "near_goal", "collision1", "collision3"])
def test_fused_mission_equals_the_stepwise_loop_in_every_scenario(ctx, kind):
    ref, maze, known, f, s = run_pair(ctx, 64, 8, kind)
    if kind == "free":
        assert ref["event"] == STEPS_DONE and ref["scans"] >= 4 and ref["calls"] == 50 and np.array_equal(known, maze)
    elif kind == "hidden":
        assert not np.array_equal(known, maze) and ref["changed_at"] < ref["calls"]        # steps after the maze changed
        assert s.last["collided_rollouts"] >= 0
    elif kind == "near_goal":
        assert ref["event"] == GOAL and 0 < ref["calls"] < 40 and s.env.done is True
    else:
        allowed = int(kind[-1])
        assert ref["event"] == TRIALS and ref["calls"] == allowed and ref["trials"] == allowed and len(ref["ex_s"]) == 0
        assert (f._U.cpu().numpy() == 0).all()


def test_resumed_mission_equals_the_uncut_one(ctx):
    """follow(N) + follow(N) from the returned info = follow(2N); N = 25: the cut falls between the scans of steps 22 and 33
    with a part-filled scan clock, which the second call must take over."""
    sc = scenario("hidden")
    N = 25
    a, maze = controller(ctx, 64, 8, 5, sc)
    ka, sa = maze.copy(), maze.copy()
    whole = a.follow(sc["state"], ka, sc["truth"], sa, 2 * N, allowed_trials=2)
    b, _ = controller(ctx, 64, 8, 5, sc)
    kb, sb = maze.copy(), maze.copy()
    first = b.follow(sc["state"], kb, sc["truth"], sb, N, allowed_trials=2)
    assert first[3] == STEPS_DONE and 0.0 < first[4]["action_time_count"] < 0.2 and first[4]["scans"] == 2
    second = b.follow(first[0], kb, sc["truth"], sb, N, allowed_trials=2, action_time_count=first[4]["action_time_count"],
                      trials=first[4]["trials"])
    assert np.array_equal(np.concatenate([first[1], second[1]]), whole[1])
    assert np.array_equal(np.concatenate([first[2], second[2]]), whole[2])
    assert np.array_equal(second[0], whole[0]) and second[3] == whole[3]
    assert second[4]["action_time_count"] == whole[4]["action_time_count"] and second[4]["trials"] == whole[4]["trials"]
    assert first[4]["scans"] + second[4]["scans"] == whole[4]["scans"] >= 4
    assert np.array_equal(ka, kb) and np.array_equal(sa, sb)
    same_controller_state(b, a)


def test_mission_longer_than_one_launch_is_chained_by_the_facade(ctx, monkeypatch):
    """A launch is bounded in controller calls; the facade issues further launches and carries counter, scan clock and trial
    count across them.  With the bound lowered to 16 calls the hidden mission (up to 55 calls) takes three or four launches,
    cut between scans with a part-filled scan clock, and still equals the stepwise loop."""
    from ditreeonlineplanner_amd import mppi
    monkeypatch.setattr(mppi, "MISSION_MAX_STEPS", 16)
    ref, _, _, _, _ = run_pair(ctx, 20, 8, "hidden")
    assert ref["calls"] > 32 and ref["scans"] >= 3


def test_start_inside_the_goal_radius_runs_nothing(ctx):
    sc = scenario("free")
    m, maze = controller(ctx, 64, 8, 3, sc)
    m._U.fill_(0.25)
    m.counter = 7
    state = np.array([m.env.goal[0] - 0.3, m.env.goal[1] + 0.2, 0.3, 1.0, 0.2, 0.0])
    assert m.is_done(state)
    known, scanned = maze.copy(), maze.copy()
    env_state, env_done, last = m.env.state, m.env.done, dict(m.last)
    out = m.follow(state, known, sc["truth"], scanned, 30)
    assert out[3] == GOAL and out[1].shape == (0, 6) and out[2].shape == (0, 2) and np.array_equal(out[0], state)
    assert out[4]["controller_calls"] == 0 and out[4]["scans"] == 0 and out[4]["action_time_count"] == 0.0
    assert m.counter == 7 and (m._U.cpu().numpy() == 0.25).all() and m.last == last
    assert np.array_equal(known, maze) and np.array_equal(scanned, maze) and np.array_equal(m.maze, np.float32(maze))
    assert np.array_equal(m.env.state, env_state) and m.env.done == env_done


def fleet_members(ctx):
    """Five missions that differ in seed, start, reference-path length and true maze; (kind, seed, path slice, max_steps)."""
    return [("hidden", 11, slice(None), 30), ("near_goal", 12, slice(400, None), 40), ("collision3", 13, slice(None), 20),
            ("free", 14, slice(0, 1200), 17), ("hidden", 15, slice(None, None, 2), 41)]


def build_fleet(ctx, members):
    cs, states, known, truth, scanned, steps, allowed = [], [], [], [], [], [], []
    for kind, seed, sl, n in members:
        sc = scenario(kind)
        m, maze = controller(ctx, 64, 8, seed, sc, sl)
        cs.append(m)
        states.append(sc["state"])
        known.append(maze.copy())
        truth.append(sc["truth"])
        scanned.append(maze.copy())
        steps.append(n)
        allowed.append(sc["allowed"])
    return cs, states, known, truth, scanned, steps, allowed


def test_fleet_of_five_equals_each_mission_alone(ctx):
    from ditreeonlineplanner_amd import mppi
    members = fleet_members(ctx)
    alone = []
    cs1, st1, kn1, tr1, sc1, steps, allowed = build_fleet(ctx, members)
    for i in range(len(members)):
        alone.append(cs1[i].follow(st1[i], kn1[i], tr1[i], sc1[i], steps[i], allowed_trials=allowed[i]))
    cs, st, kn, tr, scn, steps, allowed = build_fleet(ctx, members)
    outs = mppi.follow_fleet(cs, st, kn, tr, scn, steps, allowed_trials=allowed)
    assert len({int(c._path.shape[0]) for c in cs}) >= 4 and len({int(c.params.seed) for c in cs}) == 5
    for i, (o, a) in enumerate(zip(outs, alone)):
        assert o[3] == a[3] and np.array_equal(o[0], a[0]) and np.array_equal(o[1], a[1]) and np.array_equal(o[2], a[2]), i
        assert o[4] == a[4], (i, o[4], a[4])
        assert np.array_equal(kn[i], kn1[i]) and np.array_equal(scn[i], sc1[i]), i
        same_controller_state(cs[i], cs1[i])
    # the single runs are held to the stepwise loop by the tests above; what they were is asserted on a stepwise run of each
    events, calls = [], []
    for kind, seed, sl, n in members:
        sc = scenario(kind)
        s, maze = controller(ctx, 64, 8, seed, sc, sl)
        ref = stepwise(s, sc["state"], maze.copy(), sc["truth"], maze.copy(), n, sc["allowed"])
        events.append(ref["event"])
        calls.append(ref["calls"])
    assert events == [o[3] for o in outs] and calls == [o[4]["controller_calls"] for o in outs]
    assert events.count(GOAL) == 1 and events.count(TRIALS) == 1 and events.count(STEPS_DONE) == 3
    assert len({c for c, e in zip(calls, events) if e == STEPS_DONE}) == 3            # ended after different step counts


def test_fleet_larger_than_the_device_equals_its_members(ctx):
    """300 missions on 256 compute units: two distinct missions alternate, 30 controller calls each."""
    from ditreeonlineplanner_amd import mppi
    two = [("hidden", 21, slice(None), 30), ("free", 22, slice(0, 1200), 30)]
    cs1, st1, kn1, tr1, sc1, steps1, al1 = build_fleet(ctx, two)
    alone = [cs1[i].follow(st1[i], kn1[i], tr1[i], sc1[i], 30, allowed_trials=al1[i]) for i in range(2)]
    assert not np.array_equal(alone[0][1], alone[1][1]) and alone[0][4]["scans"] == 2
    scs = [scenario(k) for k, _, _, _ in two]
    maze = load_maze("boxes")
    cs = []
    for i in range(300):
        m, _ = controller(ctx, 64, 8, two[i % 2][1], scs[i % 2], two[i % 2][2])
        cs.append(m)
    kn = [maze.copy() for _ in range(300)]
    scn = [maze.copy() for _ in range(300)]
    outs = mppi.follow_fleet(cs, [scs[i % 2]["state"] for i in range(300)], kn, [scs[i % 2]["truth"] for i in range(300)], scn, 30,
                             allowed_trials=[scs[i % 2]["allowed"] for i in range(300)])
    U = [c._U.cpu().numpy() for c in cs1]
    for i, o in enumerate(outs):
        a = alone[i % 2]
        assert o[3] == a[3] and np.array_equal(o[0], a[0]) and np.array_equal(o[1], a[1]) and np.array_equal(o[2], a[2]), i
        assert o[4] == a[4], i
        assert np.array_equal(kn[i], kn1[i % 2]) and np.array_equal(scn[i], sc1[i % 2]), i
        assert cs[i].counter == cs1[i % 2].counter and cs[i].last == cs1[i % 2].last, i
    for i in (0, 1, 255, 256, 257, 298, 299):
        assert np.array_equal(cs[i]._U.cpu().numpy(), U[i % 2]), i
        assert np.array_equal(cs[i]._state.cpu().numpy(), alone[i % 2][0]), i


def test_state_left_behind(ctx):
    """After follow, one more step() does what it does after the stepwise loop, and the ctx's own maze copy is the mission's
    final known maze: a collision probe on the cell the scans added collides without any upload."""
    sc = scenario("hidden")
    s, maze = controller(ctx, 64, 8, 9, sc)
    known_s, scanned_s = maze.copy(), maze.copy()
    ref = stepwise(s, sc["state"], known_s, sc["truth"], scanned_s, 40, 2)
    f, _ = controller(ctx, 64, 8, 9, sc)
    ctx.upload_maze(maze)                                      # the ctx holds the maze WITHOUT the hidden cell
    known_f, scanned_f = maze.copy(), maze.copy()
    out = f.follow(sc["state"], known_f, sc["truth"], scanned_f, 40, allowed_trials=2)
    assert ctx.maze_owner is f
    probe = np.argwhere(known_f != maze)
    assert len(probe) == 1 and tuple(probe[0]) == (18, 4)
    xy = G.cell_rowcol_to_xy(probe[0], maze)
    st = torch.as_tensor(np.array([[xy[0], xy[1], 0.0, 0, 0, 0]]), device=ctx.device)
    status, _, _, _ = ctx.car_rollout(st, torch.zeros(1, 1, 2, dtype=torch.float64, device=ctx.device), np.array([1e6, 1e6]), A=1)
    assert int(status.item()) & 0xFF == 2
    same_mission(out, ref, (known_f, scanned_f), (known_s, scanned_s))
    rf = f.step(out[0])
    rs = s.step(ref["state"])
    assert np.array_equal(rf[0], rs[0]) and np.array_equal(rf[1], rs[1]) and rf[2] is rs[2]
    same_controller_state(f, s)


def test_follow_reference_keeps_the_driver_semantics(ctx):
    """online.follow_reference: the caller's numpy mazes are updated IN PLACE (the driver keeps using its own arrays), the
    controller's env carries the new state / done flag / known maze, and the result equals MPPI.follow's."""
    from ditreeonlineplanner_amd import online
    sc = scenario("near_goal")
    a, maze = controller(ctx, 64, 8, 3, sc)
    b, _ = controller(ctx, 64, 8, 3, sc)
    known, scanned = maze.copy(), maze.copy()
    known_id, scanned_id = id(known), id(scanned)
    k2, s2 = maze.copy(), maze.copy()
    ref = b.follow(sc["state"], k2, sc["truth"], s2, 40)
    out = online.follow_reference(a, sc["state"], known, sc["truth"], scanned, 40)
    assert id(known) == known_id and id(scanned) == scanned_id and known.dtype == maze.dtype
    assert np.array_equal(known, k2) and np.array_equal(scanned, s2) and bool((scanned == 2).any()) == (out[4]["scans"] > 0)
    assert out[3] == GOAL == ref[3] and np.array_equal(out[0], ref[0]) and np.array_equal(out[1], ref[1]) and np.array_equal(out[2], ref[2])
    assert out[4] == ref[4] and set(out[4]) >= {"action_time_count", "trials"}
    assert a.env.done is True and np.array_equal(a.env.state, out[0]) and a.is_done(out[0])
    assert a.env.maze_map is known and np.array_equal(a.maze, np.float32(known)) and a.counter == out[4]["controller_calls"]
    same_controller_state(a, b)


def test_refusals(ctx):
    from ditreeonlineplanner_amd import _lib, mppi
    from ditreeonlineplanner_amd.mppi import MPPI
    sc = scenario("free")
    maze = load_maze("boxes")
    args = lambda: (sc["state"], maze.copy(), sc["truth"], maze.copy(), 5)
    big, _ = controller(ctx, 257, 8, 0, sc)
    with pytest.raises(ValueError, match="K = 257 > 256"):
        big.follow(*args())
    assert big.counter == 0
    m, _ = controller(ctx, 64, 8, 0, sc)
    m.world = 2
    with pytest.raises(ValueError, match="sharded"):
        m.follow(*args())
    m.world = 1
    with pytest.raises(ValueError, match="noise tape"):
        m.follow(*args(), noise=torch.zeros(64, 8, 2, dtype=torch.float64, device=ctx.device))
    ant = MPPI(maze_data=maze, T=8, K=16, nx=29, nu=8, ctx=ctx)
    with pytest.raises(NotImplementedError, match="AntMPPI"):
        ant.follow(*args())
    with pytest.raises(NotImplementedError, match="AntMPPI"):
        mppi.follow_fleet([ant], [sc["state"]], [maze.copy()], [maze.copy()], [maze.copy()], 5)
    bare = MPPI(maze_data=maze, T=8, K=16, ctx=ctx)
    with pytest.raises(_lib.DitreeError, match="set_ref_path"):
        bare.follow(*args())
    other, _ = controller(ctx, 64, 16, 0, sc)
    with pytest.raises(ValueError, match="differs from controller 0 in T"):
        mppi.follow_fleet([m, other], [sc["state"]] * 2, [maze.copy(), maze.copy()], [maze.copy()] * 2, [maze.copy(), maze.copy()], 5)
    stale = maze.copy()
    assert stale[18, 9] == 0
    stale[18, 9] = 1
    with pytest.raises(ValueError, match="not the controller's known maze"):
        m.follow(sc["state"], stale, sc["truth"], maze.copy(), 5)
    assert m.counter == 0 and m.last == {}
    # the C entry point names its limits too
    h = _lib.lib()
    p = _lib.MppiParams.from_buffer_copy(m.params)
    one = torch.zeros(64, dtype=torch.float64, device=ctx.device)
    ptr = one.data_ptr()

    def call(params, M=1, P_max=16, rows=20, cols=20, first=ptr):
        rc = h.ditree_mppi_missions(ctx._h, params, M, first, ptr, ptr, ptr, ptr, ptr, ptr, P_max, ptr, ptr, ptr, ptr, rows, cols, ptr, 0,
                                    ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, -1, ctx.stream)
        return rc, h.ditree_last_error(ctx._h).decode()
    for change, kw, word in ((dict(K=257), {}, "K <= 256"), (dict(T=65), {}, "T <= 64"), ({}, dict(P_max=4097), "P <= 4096"),
                             ({}, dict(rows=120, cols=120), "13104"), (dict(k_offset=64), {}, "k_offset"), ({}, dict(M=0), "M < 1"),
                             ({}, dict(first=None), "null pointer")):
        q = _lib.MppiParams.from_buffer_copy(p)
        for k, v in change.items():
            setattr(q, k, v)
        rc, msg = call(q, **kw)
        assert rc == -1 and word in msg, (rc, msg, word)
