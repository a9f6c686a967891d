"""GPU: ditree_polish_plans against the numpy restatement (tests/polish_ref.py), iteration by iteration from the device's own
incumbent.  Noise and first rows are supplied by the caller, so candidate tapes are bit-equal by construction; tests/
test_polish_ref_host.py checks on the oracle that no candidate of these cases sits within 1e-9 of the goal radius or of a wall.

The 1e-6 on an arrival time: tau = (s - 1) + (d_{s-1} - 0.5) / (d_{s-1} - d_s); the states are pinned to 1e-9, so numerator and
denominator move by at most 2e-9, and the tapes here cross the radius at >= 0.2 m/s, a denominator of >= 4 mm a row:
2 * 2e-9 / 4e-3 = 1e-6."""
import numpy as np
import pytest

from tests import polish_cases as PC
from tests import polish_ref as R

pytestmark = pytest.mark.gpu

TAU_TOL = 1e-6
STATE_TOL = 1e-9


@pytest.fixture(scope="module")
def ctx():
    from ditreeonlineplanner_amd.ops import Context
    return Context(0)


def _polish(ctx, maze, x0, goal, tape, **kw):
    from ditreeonlineplanner_amd.polish import polish_plans
    return polish_plans(ctx, np.asarray(maze), np.asarray(x0)[None], np.asarray(goal)[None], [tape], **kw)[0]


def _same(a, b):
    """Two polish_plans results, bit for bit."""
    assert a["status"] == b["status"] and a["rows_in"] == b["rows_in"] and a["rows_out"] == b["rows_out"]
    assert a["arrival_in"] == b["arrival_in"] and a["arrival_out"] == b["arrival_out"]
    assert np.array_equal(a["actions"], b["actions"])
    assert (a["path64"] is None) == (b["path64"] is None)
    if a["path64"] is not None:
        assert np.array_equal(a["path64"], b["path64"]) and np.array_equal(a["path"], b["path"])
    for c in a["trace"]:
        assert np.array_equal(a["trace"][c], b["trace"][c]), c


@pytest.mark.parametrize("case", PC.KERNEL_CASES, ids=lambda c: f"{c[0]}-K{c[1]}-hold{c[2]}")
def test_every_iteration_matches_the_restatement_from_the_devices_own_incumbent(ctx, case):
    name, K, hold, N, seed = case
    maze, x0, goal, tape0 = PC.PLANS[name]()
    noise, first_row = PC.case_inputs(*case)
    kw = dict(rollouts=K, sigma=PC.SIGMA, hold=hold, seed=seed)
    tape = tape0
    chain = []
    for n in range(N):
        dev = _polish(ctx, maze, x0, goal, tape, iterations=1, noise=noise[n:n + 1], first_row=first_row[n:n + 1], **kw)
        chain.append(dev)
        rp = R.replay(maze, x0, goal, tape.astype(np.float64))
        assert dev["status"] == "ok" and rp["status"] == R.OK
        assert dev["rows_in"] == len(tape) and abs(dev["arrival_in"] - rp["tau"]) <= TAU_TOL
        T = rp["rows"]
        if n == 0:
            assert T < len(tape0) or name == "easy"              # the corridor tape carries rows behind its arrival: cut
        it = R.iterate(maze, x0, goal, tape[:T].astype(np.float64), rp["tau"], R.given_first_rows(first_row[n], T), noise[n], hold,
                       critical=True)
        tr = {c: v[0] for c, v in dev["trace"].items()}
        ncrit = int(it["critical"].sum())
        k = int(tr["winner"])
        print(f"{name} K={K} hold={hold} n={n}: device k={k} tau={tr['tau']!r} accepted={bool(tr['accepted'])} rows={int(tr['rows'])} "
              f"arriving={int(tr['arriving'])} | reference k={it['winner']} tau={it['tau'].min()!r} arriving={int(it['arrived'].sum())} "
              f"critical={ncrit}")
        assert abs(int(tr["arriving"]) - int(it["arrived"].sum())) <= min(1, ncrit)
        if k >= 0:
            assert it["arrived"][k] and abs(it["tau"][k] - tr["tau"]) <= TAU_TOL       # the device's winner has the reference's tau
            assert it["tau"].min() >= tr["tau"] - TAU_TOL                              # and no reference candidate beats it
        else:
            assert not it["arrived"].any() and np.isinf(tr["tau"])
        assert bool(tr["accepted"]) == it["accepted"]
        assert int(tr["rows"]) == len(it["tape"]) == dev["rows_out"]
        assert abs(tr["arrival"] - it["tau_star"]) <= TAU_TOL and tr["arrival"] == dev["arrival_out"]
        if it["accepted"]:
            s = int(it["rows"][k])
            assert np.array_equal(dev["actions"].astype(np.float64), it["tapes"][k, :s])   # bit-equal by construction
            assert np.abs(dev["path64"] - R.roll(maze, x0, goal, it["tapes"][k:k + 1, :s])["states"][0]).max() <= STATE_TOL
        else:
            assert np.array_equal(dev["actions"], tape[:T])
            assert np.abs(dev["path64"] - rp["states"]).max() <= STATE_TOL
        assert dev["rows_out"] <= T and dev["arrival_out"] <= dev["arrival_in"]
        tape = dev["actions"]
    assert chain[1]["trace"]["arriving"][0] == 0 and chain[1]["trace"]["winner"][0] == -1      # the iteration in which nothing arrives
    assert chain[0]["trace"]["arriving"][0] > 0
    # all N iterations in one call (T* and tau* never leave the device) = the chain of single iterations, bit for bit
    whole = _polish(ctx, maze, x0, goal, tape0, iterations=N, noise=noise, first_row=first_row, **kw)
    assert whole["rows_out"] == chain[-1]["rows_out"] and whole["arrival_out"] == chain[-1]["arrival_out"]
    assert np.array_equal(whole["actions"], chain[-1]["actions"]) and np.array_equal(whole["path64"], chain[-1]["path64"])
    for n in range(N):
        for c in whole["trace"]:
            assert whole["trace"][c][n] == chain[n]["trace"][c][0], (c, n)
    assert whole["arrival_in"] == chain[0]["arrival_in"]


def test_sigma_zero_returns_the_replayed_plan(ctx):
    maze, x0, goal, tape = PC.corridor_plan()
    rp = R.replay(maze, x0, goal, tape.astype(np.float64))
    dev = _polish(ctx, maze, x0, goal, tape, rollouts=192, iterations=3, sigma=(0.0, 0.0), hold=4, seed=9)
    assert dev["status"] == "ok" and dev["rows_in"] == len(tape) and dev["rows_out"] == rp["rows"] < len(tape)
    assert np.array_equal(dev["actions"], tape[:rp["rows"]]) and dev["arrival_out"] == dev["arrival_in"]
    assert np.abs(dev["path64"] - rp["states"]).max() <= STATE_TOL
    assert not dev["trace"]["accepted"].any() and (dev["trace"]["arriving"] == 192).all() and (dev["trace"]["winner"] == 0).all()
    assert (dev["trace"]["tau"] == dev["arrival_in"]).all()          # a candidate from X*[a] = the whole tape's roll, bit for bit


def test_refused_plans_leave_their_buffers_untouched(ctx):
    from ditreeonlineplanner_amd.polish import polish_plans
    maze, x0, goal, tape = PC.corridor_plan()
    inside = x0.copy()
    inside[:2] = goal + [0.3, 0.0]
    tapes = [PC.colliding_tape(), tape, tape[:40], tape]
    starts = np.stack([x0, inside, x0, x0])
    out = polish_plans(ctx, maze, starts, np.tile(goal, (4, 1)), tapes, rollouts=64, iterations=2, sigma=PC.SIGMA, hold=4, seed=3)
    assert [r["status"] for r in out] == ["collides", "start_in_goal", "no_arrival", "ok"]
    for r, t in zip(out[:3], tapes[:3]):
        assert r["path"] is None and np.array_equal(r["actions"], t) and r["rows_out"] == r["rows_in"] == len(t)
        raw = r["raw"]
        assert raw["rows"] == len(t) and np.array_equal(raw["tape"][:len(t)], t.astype(np.float64)) and not raw["tape"][len(t):].any()
        assert not raw["states"].any() and not raw["trace"].any() and not raw["arrival"].any()
    # the plan next to them is polished as it is alone
    _same(out[3], _polish(ctx, maze, x0, goal, tape, rollouts=64, iterations=2, sigma=PC.SIGMA, hold=4, seed=3))


def test_two_plans_with_different_mazes_equal_each_alone_and_a_second_call(ctx):
    from ditreeonlineplanner_amd.polish import polish_plans
    plans = [PC.easy_plan(), PC.corridor_plan()]
    kw = dict(rollouts=320, iterations=4, sigma=PC.SIGMA, hold=4, seed=21)

    def both():
        return polish_plans(ctx, [p[0] for p in plans], np.stack([p[1] for p in plans]), np.stack([p[2] for p in plans]),
                            [p[3] for p in plans], **kw)
    a, b = both(), both()
    for i, p in enumerate(plans):
        _same(a[i], b[i])
        _same(a[i], _polish(ctx, p[0], p[1], p[2], p[3], **kw))
    assert a[0]["rows_out"] <= 45 and a[0]["arrival_out"] < a[0]["arrival_in"]


def test_the_on_device_generator_keeps_the_guarantees(ctx):
    """No overrides: the result, rolled by the oracle on the CPU, arrives at exactly rows_out without a collision, with no more
    rows and no later arrival than the plan that went in; rows and arrival never grow along the trace."""
    maze, x0, goal, tape = PC.easy_plan()
    dev = _polish(ctx, maze, x0, goal, tape, rollouts=256, iterations=12, sigma=(1.0, 0.1), hold=8, seed=1)
    assert dev["status"] == "ok" and dev["rows_in"] == 45
    rp = R.replay(maze, x0, goal, dev["actions"].astype(np.float64))
    assert rp["status"] == R.OK and rp["rows"] == dev["rows_out"] == len(dev["actions"]) <= dev["rows_in"]
    assert dev["arrival_out"] <= dev["arrival_in"] and abs(rp["tau"] - dev["arrival_out"]) <= TAU_TOL
    assert np.abs(dev["path64"] - rp["states"]).max() <= STATE_TOL and len(dev["path"]) == dev["rows_out"] + 1
    rows = np.concatenate([[45], dev["trace"]["rows"]])
    taus = np.concatenate([[dev["arrival_in"]], dev["trace"]["arrival"]])
    assert (np.diff(rows) <= 0).all() and (np.diff(taus) <= 0).all()
    assert dev["trace"]["arriving"].max() > 0
    # reported, not asserted: the restatement with the same generator and hash (the device's log / sincos may differ from numpy's
    # in the last place, so a candidate tape is not bit-equal by construction here)
    ref = R.polish(maze, x0, goal, tape.astype(np.float64), 256, 12, (1.0, 0.1), 8, 1)
    print("device rows", list(dev["trace"]["rows"]), "arrival", dev["arrival_out"], "| reference rows", [t["rows"] for t in ref["trace"]],
          "arrival", ref["arrival_out"])


def test_the_c_abi_refuses_by_name(ctx):
    import ctypes as C
    import torch
    from ditreeonlineplanner_amd import _lib
    maze, x0, goal, tape = PC.corridor_plan()
    ctx.upload_maze(maze)
    dev = ctx.device
    cap = len(tape)
    t = {"x0": torch.as_tensor(x0[None], device=dev), "goal_xy": torch.as_tensor(goal[None], device=dev),
         "tape": torch.as_tensor(tape.astype(np.float64)[None], device=dev).contiguous(),
         "rows": torch.full((1,), cap, dtype=torch.int32, device=dev), "states": torch.zeros(1, cap + 1, 6, dtype=torch.float64, device=dev),
         "arrival": torch.zeros(1, 2, dtype=torch.float64, device=dev), "status": torch.full((1,), -1, dtype=torch.int32, device=dev),
         "trace": torch.zeros(1, 2, _lib.POLISH_TRACE, dtype=torch.float64, device=dev)}

    def call(**over):
        d = _lib.Polish()
        d.n_plans, d.state_dim, d.action_dim, d.capacity, d.K, d.N, d.hold = 1, 6, 2, cap, 64, 2, 4
        d.sigma[0], d.sigma[1] = 1.0, 0.1
        rows_host = (C.c_int32 * 1)(over.pop("rows_host", cap))
        d.rows_host = rows_host
        for name, v in t.items():
            setattr(d, name, v.data_ptr())
        for name, v in over.items():
            if name == "sigma":
                d.sigma[0], d.sigma[1] = v
            else:
                setattr(d, name, v)
        rc = _lib.lib().ditree_polish_plans(ctx._h, C.byref(d), ctx.stream)
        return rc, _lib.lib().ditree_last_error(ctx._h).decode()

    for over, word in ((dict(K=0), "multiple of 64"), (dict(K=96), "multiple of 64"), (dict(N=-1), "N < 0"), (dict(hold=0), "hold < 1"),
                       (dict(sigma=(float("nan"), 0.1)), "sigma"), (dict(sigma=(1.0, -0.5)), "sigma"),
                       (dict(sigma=(float("inf"), 0.1)), "sigma"), (dict(rows_host=cap + 1), "capacity"),
                       (dict(state_dim=29, action_dim=8), "ant"), (dict(n_plans=0), "n_plans"), (dict(tape=None), "null pointer")):
        rc, msg = call(**over)
        assert rc == -1 and word in msg, (over, rc, msg)
    torch.cuda.synchronize()
    assert int(t["status"].item()) == -1 and not t["states"].any().item()      # nothing was launched
    rc, msg = call()
    assert rc == 0, msg
    torch.cuda.synchronize()
    assert int(t["status"].item()) == 0
