"""``rollout`` with the reference's signature (rollout_manager.py:545-838): the closed-loop policy roll-out that
train_diffusion_policy.py runs before training, every few epochs and at the end -- ``envs_per_scenario`` cars on every row of
the validation scenario file, each driven by the sampler alone for up to ``max_episode_steps`` steps -- as ONE batch of
episodes on the device (``policy_rollout.PolicyRolloutEngine``).  Car only.

Three departures from the reference loop, parity unpinned: a terminated episode is frozen instead of
re-reset by stable-baselines3's DummyVecEnv (``collision_count`` is 0 or 1, every quantity comes from the float64 env state);
terminated episodes are left out of later sampler calls; ``best_dist`` takes the success test's fused norm.
"""
from __future__ import annotations

import numpy as np

SCENARIOS_FILE = "experiments/validation_scenarios_car.csv"          # rollout_manager.py:606-607
MAPS_FOLDER = "maps/mazes"


def check_rollout_arguments(env_id, prediction_type="actions", obs_history=1, action_history=1, position_conditioned=False,
                            goal_conditioned=True, local_map_conditioned=True, world_size=1):
    """Everything ``rollout`` refuses, by name, before anything touches the device."""
    e = str(env_id).lower()
    if "car" not in e or "ant" in e or "point" in e or "drone" in e or "forest" in e:
        raise NotImplementedError(f"rollout: env_id {env_id!r}: only the car's roll-out runs on the device (the ant, point and "
                                  "drone envs are third-party physics or absent from the reference tree)")
    if prediction_type != "actions":
        raise NotImplementedError(f"rollout: prediction_type={prediction_type!r}: only 'actions' (the 'observations' branch drives "
                                  "a PD controller on the host)")
    if obs_history != 1 or action_history != 1:
        raise NotImplementedError(f"rollout: obs_history={obs_history}, action_history={action_history}: the car's sampler is "
                                  "conditioned on one observation and one previous action")
    if position_conditioned:
        raise NotImplementedError("rollout: position_conditioned=True is not built (the conditioning vector drops x, y, psi)")
    if not goal_conditioned:
        raise NotImplementedError("rollout: goal_conditioned=False is not built")
    if not local_map_conditioned:
        raise NotImplementedError("rollout: local_map_conditioned=False is not built (the network reads a local map)")
    if int(world_size) != 1:
        raise NotImplementedError(f"rollout: {world_size} ranks: a policy roll-out runs on one rank")


def validation_episodes(scenarios, envs_per_scenario):
    """The batch the reference builds from its scenario rows (rollout_manager.py:624-661, car_env.py:216-230): per row the maze,
    ``env.goal`` = the goal cell's centre, and ``envs_per_scenario`` start states ``[x, y, deg2rad(deg), 0, 0, 0]`` rounded to
    float32 and widened, as ``CarEnv.reset`` leaves them.  ``scenarios``: ``scenarios.car_scenarios`` rows.
    -> (scenes [(maze, goal_xy)], starts (S * E, 6), scene_of (S * E,))."""
    E = int(envs_per_scenario)
    if E < 1:
        raise ValueError("envs_per_scenario must be >= 1")
    scenes, starts, scene_of = [], [], []
    for k, sc in enumerate(scenarios):
        scenes.append((sc["maze"], np.asarray(sc["goal"], dtype=np.float64)[:2]))
        s0 = np.zeros(6, dtype=np.float32)
        s0[:3] = np.asarray(sc["start"], dtype=np.float64)[:3]
        starts += [s0.astype(np.float64)] * E
        scene_of += [k] * E
    return scenes, np.array(starts, dtype=np.float64).reshape(-1, 6), np.array(scene_of, dtype=np.int32)


def rollout(env_id, policy, ema_noise_pred_net, noise_scheduler, max_episode_steps=250, render_mode="rgb_array",
            num_diffusion_iters=100, prediction_type="actions", obs_history=1, action_history=1, position_conditioned=False,
            goal_conditioned=True, local_map_conditioned=True, local_map_size=10, scale=0.2, pred_horizon=16, action_horizon=8,
            envs_per_scenario=32, render=False, *, scenarios_file=None, maps_folder=None, ctx=None, precision=None):
    """rollout_manager.py:545-838 for the car -> ``(results_per_scenario, [])``: per scenario row a dict with the reference's
    keys (:825-836) -- ``scenario_name``, ``maze``, ``start_rowcol``, ``goal_rowcol``, ``start_position``, ``goal_position``,
    ``best_dist`` (E,), ``step_to_completion`` (E,) float with -1 = never, ``trajectory`` (E, max_episode_steps + 1, 8),
    ``collision_count`` (E,) float.  ``render`` is ignored, as the reference forces it off (:564).  Keyword-only:
    ``scenarios_file`` / ``maps_folder`` (defaults: the reference's relative paths), ``ctx``, ``precision`` (the sampler's)."""
    import torch.distributed as dist
    world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
    check_rollout_arguments(env_id, prediction_type, obs_history, action_history, position_conditioned, goal_conditioned,
                            local_map_conditioned, world)
    from .policies.fm_policy import DiffusionSampler
    from .policy_rollout import PolicyRolloutEngine
    from .scenarios import car_scenarios
    scenarios_file = SCENARIOS_FILE if scenarios_file is None else scenarios_file
    maps_folder = MAPS_FOLDER if maps_folder is None else maps_folder
    scenarios = car_scenarios(scenarios_file, maps_folder)
    if not scenarios:
        raise FileNotFoundError(f"rollout: no scenario of {scenarios_file} has its maze under {maps_folder}")
    sampler = DiffusionSampler(ema_noise_pred_net, noise_scheduler, env_id, policy, pred_horizon, 2, prediction_type, obs_history,
                               action_history, num_diffusion_iters, local_map_size=local_map_size, ctx=ctx, precision=precision)
    scenes, starts, scene_of = validation_episodes(scenarios, envs_per_scenario)
    eng = PolicyRolloutEngine(sampler.ctx, scenes, starts, scene_of, sampler=sampler, action_horizon=action_horizon,
                              pred_horizon=pred_horizon, local_map_size=local_map_size, local_map_scale=scale, s_global=1.0)
    res = eng.run(max_episode_steps)
    traj = eng.trajectory(res)
    step_to_completion = res["success_step"].astype(np.float64)                     # -1 = never (:817)
    collision_count = res["collided"].astype(np.float64)
    E = int(envs_per_scenario)
    out = []
    for i, sc in enumerate(scenarios):
        sl = slice(i * E, (i + 1) * E)
        out.append({
            "scenario_name": sc["name"], "maze": sc["maze"], "start_rowcol": sc["start_cell"], "goal_rowcol": sc["goal_cell"],
            "start_position": np.asarray(sc["start"], dtype=np.float64)[:2].copy(),
            "goal_position": np.asarray(sc["goal"], dtype=np.float64)[:2].copy(),
            "best_dist": res["best_dist"][sl].copy(), "step_to_completion": step_to_completion[sl].copy(),
            "trajectory": traj[sl].copy(), "collision_count": collision_count[sl].copy()})
    return out, []
