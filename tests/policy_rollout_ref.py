"""CPU restatement of the closed-loop policy roll-out (rollout_manager.py:706-838 for the car, with a terminated episode frozen)
in numpy, built from the pinned oracle functions only: ``oracle.geometry.car_step`` / ``is_colliding_car`` / ``create_local_map``,
``oracle.sampler.car_cond_vector`` / ``flow_sample`` and the oracle network.  Test infrastructure for
tests/test_gpu_policy_rollout.py, tests/test_policy_rollout_host.py and profiles/policy_rollout_probe.py."""
import numpy as np

from oracle import geometry as G
from oracle import sampler as OS


def oracle_actions(net, k_steps=1, local_map_size=20, local_map_scale=0.2, s_global=1.0):
    """``actions_fn`` of ``run_episodes`` for the oracle network: the reference's sampler call on the given episodes
    (fm_policy.py:53-212, flow matching).  ``noise_fn(chunk) -> (N, P, 2)`` float32 for the WHOLE batch."""
    def make(noise_fn):
        def actions_fn(chunk, rows, mazes, scene_of, state, prev_action, has_prev, goal):
            noise = np.asarray(noise_fn(chunk), dtype=np.float32)[rows]
            lm = np.empty((len(rows), local_map_size, local_map_size), dtype=np.float32)
            for k, maze in enumerate(mazes):                                   # rollout_manager.py:718-735, per maze
                m = scene_of[rows] == k
                if m.any():
                    center = (s_global * maze.shape[1] / 2, s_global * maze.shape[0] / 2)          # :641
                    lm[m] = G.create_local_map(maze, state[m, 0], state[m, 1], state[m, 2], local_map_size, local_map_scale,
                                               s_global, center)
            cond = OS.car_cond_vector(state, prev_action, has_prev, goal, local_map_size=local_map_size)
            x = OS.flow_sample(net, noise, OS.scale_local_map(lm), cond, k_steps=k_steps)
            return OS.unnormalize_actions(x)
        return actions_fn
    return make


def tape_actions(tape_fn, N, P):
    """``actions_fn`` for an action tape ``tape_fn(chunk, N, P) -> (N, P, 2)``."""
    def actions_fn(chunk, rows, mazes, scene_of, state, prev_action, has_prev, goal):
        return np.asarray(tape_fn(chunk, N, P), dtype=np.float64)[rows]
    return actions_fn


def run_episodes(mazes, goals, starts, scene_of, actions_fn, action_horizon, max_episode_steps):
    """The chunk loop.  ``actions_fn(chunk, rows, mazes, scene_of, state[rows], prev_action[rows], has_prev[rows], goal[rows])``
    -> (len(rows), >= A, 2) float64 for the episodes still running.  -> dict of per-episode results + ``chunks`` run."""
    starts = np.asarray(starts, dtype=np.float64)
    scene_of = np.asarray(scene_of)
    N, A, M = starts.shape[0], int(action_horizon), int(max_episode_steps)
    goal = np.asarray(goals, dtype=np.float64)[scene_of]
    state = starts.copy()
    rows = np.zeros((N, M, 8))
    n_steps = np.zeros(N, dtype=np.int64)
    success_step = np.full(N, -1, dtype=np.int64)
    collided = np.zeros(N, dtype=bool)
    succeeded = np.zeros(N, dtype=bool)
    both = np.zeros(N, dtype=bool)
    best = np.full(N, np.inf)
    prev_action = np.zeros((N, 2))
    has_prev = np.zeros(N, dtype=bool)
    done = np.zeros(N, dtype=bool)
    step, chunks = 0, 0
    while step < M and not done.all():
        run = np.nonzero(~done)[0]
        acts = np.asarray(actions_fn(chunks, run, mazes, scene_of, state[run], prev_action[run], has_prev[run], goal[run]),
                          dtype=np.float64)
        chunks += 1
        for j in range(A):
            for q, i in enumerate(run):
                if done[i]:
                    continue
                a = acts[q, j]
                rows[i, step, :6], rows[i, step, 6:] = state[i], a
                state[i] = G.car_step(state[i], a)
                d = state[i, :2] - goal[i]
                ok = bool(np.linalg.norm(d) < 0.5)                                             # car_env.py:341-350
                hit = bool(G.is_colliding_car(state[i][None], np.asarray(mazes[scene_of[i]]))[0])   # car_env.py:267-268
                best[i] = np.minimum(best[i], np.sqrt(d[0] * d[0] + d[1] * d[1]))              # rollout_manager.py:800-801
                n_steps[i] = step + 1
                prev_action[i], has_prev[i] = a, True
                if ok and success_step[i] < 0:
                    success_step[i] = step
                succeeded[i] |= ok
                collided[i] |= hit
                both[i] |= ok and hit
                done[i] = ok or hit
            step += 1
            if step >= M or done.all():
                break
    return dict(n_steps=n_steps, success_step=success_step, collided=collided, succeeded=succeeded, both=both, best_dist=best,
                rows=rows, final_state=state, terminated=done.copy(), chunks=chunks)


def fill_forward(res, max_episode_steps):
    """The reference's ``traj`` (rollout_manager.py:702,767-768,813-815), written the way its loop writes it: step by step."""
    N, M = res["n_steps"].shape[0], int(max_episode_steps)
    traj = np.zeros((N, M + 1, 8))
    T = int(res["n_steps"].max())
    for t in range(T):
        live = res["n_steps"] > t
        traj[live, t] = res["rows"][live, t]
        traj[~live, t] = traj[~live, t - 1]
    traj[:, T] = np.concatenate([res["final_state"], np.zeros((N, 2))], axis=-1)
    traj[res["terminated"], T] = traj[res["terminated"], T - 1]
    return traj
