"""Episodes/s and ms per chunk of the closed-loop policy roll-out (ditreeonlineplanner_amd/policy_rollout.py) on the reference's
validation scenario file (tests/golden/validation_scenarios_car.csv: S = 3 mazes): E = 32 cars per scenario -- the reference's
size (rollout_manager.py:559) -- and E = 1024, ``max_episode_steps`` = 250, the config-2 car network (seeded random weights) in
f16x3, K = 1, after a warm-up run, best of ``--reps``; the host clock ends in a device synchronise.  Then the E = 32 batch for
``--cpu-steps`` steps on the device and through the CPU restatement (tests/policy_rollout_ref.py, the oracle network on at most
16 host threads) -- a bounded sample of the same loop, the two drawing their own noise.  Prints one JSON line (and writes it
to --out).

    timeout -k 10 600 python profiles/policy_rollout_probe.py --out out/r10_policy_rollout_probe.json
"""
import argparse
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

FIXTURE = os.path.join(REPO, "tests", "golden", "validation_scenarios_car.csv")
A, P = 8, 64


def sampler():
    from ditreeonlineplanner_amd.policies.fm_policy import DiffusionSampler
    from ditreeonlineplanner_amd.train_diffusion_policy import init_noise_pred_net
    from oracle import denoiser as OD
    torch.manual_seed(0)
    onet = OD.init_noise_pred_net().eval()
    net = init_noise_pred_net(input_dim=2, action_dim=2, obs_dim=3, obs_history=1, action_history=1, goal_conditioned=True,
                              goal_dim=2, local_map_conditioned=True, local_map_encoder="resnet", local_map_embedding_dim=400,
                              local_map_size=20, down_dims=[512, 1024, 2048])
    net.load_state_dict(onet.state_dict())
    smp = DiffusionSampler(net, None, "carmaze", policy="flow_matching", pred_horizon=P, action_dim=2, prediction_type="actions",
                           obs_history=1, action_history=1, goal_conditioned=True, num_diffusion_iters=1, local_map_size=20)
    return smp, onet


def episodes(E):
    from ditreeonlineplanner_amd.rollout_manager import validation_episodes
    from ditreeonlineplanner_amd.scenarios import DATA, car_scenarios
    return validation_episodes(car_scenarios(FIXTURE, DATA), E)


def device_run(smp, E, M, reps):
    from ditreeonlineplanner_amd.policy_rollout import PolicyRolloutEngine
    scenes, starts, scene_of = episodes(E)
    eng = PolicyRolloutEngine(smp.ctx, scenes, starts, scene_of, sampler=smp, action_horizon=A, pred_horizon=P)
    torch.manual_seed(1)
    eng.run(M)                                                   # warm-up: bind, reserve, first launches
    times = []
    for _ in range(reps):
        torch.manual_seed(1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = eng.run(M)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    t = min(times)
    return {"scenarios": len(scenes), "envs_per_scenario": E, "episodes": eng.N, "max_episode_steps": M, "seconds": times,
            "chunks": eng.chunks_run, "ms_per_chunk": 1e3 * t / eng.chunks_run, "episodes_per_s": eng.N / t,
            "env_steps": int(res["n_steps"].sum()), "succeeded": int((res["success_step"] >= 0).sum()),
            "collided": int(res["collided"].sum())}


def cpu_run(onet, E, M):
    from tests import policy_rollout_ref as R
    torch.set_num_threads(min(16, torch.get_num_threads()))
    scenes, starts, scene_of = episodes(E)
    gen = torch.Generator().manual_seed(1)
    actions_fn = R.oracle_actions(onet)(lambda c: torch.randn((len(starts), P, 2), generator=gen).numpy())
    t0 = time.perf_counter()
    res = R.run_episodes([m for m, _ in scenes], [g for _, g in scenes], starts, scene_of, actions_fn, A, M)
    t = time.perf_counter() - t0
    return {"scenarios": len(scenes), "envs_per_scenario": E, "episodes": len(starts), "max_episode_steps": M, "seconds": t,
            "threads": torch.get_num_threads(), "chunks": res["chunks"], "ms_per_chunk": 1e3 * t / res["chunks"],
            "episodes_per_s": len(starts) / t, "env_steps": int(res["n_steps"].sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--steps", type=int, default=250)
    ap.add_argument("--cpu-steps", type=int, default=40)
    a = ap.parse_args()
    smp, onet = sampler()
    out = {"probe": "policy_rollout_probe", "device": torch.cuda.get_device_name(0), "precision": "f16x3", "k_steps": 1,
           "action_horizon": A, "pred_horizon": P,
           "device_E32": device_run(smp, 32, a.steps, a.reps), "device_E1024": device_run(smp, 1024, a.steps, a.reps),
           "device_E32_bounded": device_run(smp, 32, a.cpu_steps, a.reps),
           "cpu_restatement_E32_bounded": cpu_run(onet, 32, a.cpu_steps)}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
