#!/usr/bin/env python
"""Closed-loop cost of the continuous-command path against the action-id path (SPEC a15b).

For each config (default C3 and C2, the presets' env counts) one FFMPVec runs, with single-step
graphs on (FFMPVec.use_graphs), K closed-loop steps of
    step(policy_reactive(out=action_buffer))      the id path  (bench.py's closed_loop step_graph row)
    step(policy_field(out=command_buffer))        the command path
each timed after >= 30 ms of its own untimed steps (bench.py's warm-up discipline: after an idle gap
the first few ms of steps run slow), and K back-to-back launches of each policy kernel alone.
Prints one JSON line per config.  A first measurement: no threshold.

    python tools/command_path_timing.py [--configs C3,C2] [--steps 200] [--repeats 3]
"""
import argparse
import json
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C3,C2")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3, help="timed regions per path, interleaved; all are reported")
    ap.add_argument("--envs", type=int, default=0, help="override the preset's env count")
    ap.add_argument("--no-autotune", action="store_true")
    args = ap.parse_args()
    import torch
    from flow_field_based_motion_planner_amd.config import PRESETS, preset
    from flow_field_based_motion_planner_amd.vec_env import FFMPVec

    K = max(200, args.steps)
    for name in args.configs.split(","):
        n = args.envs or PRESETS[name]["n_envs"]
        env = FFMPVec(n, preset(name), device="cuda:0", autotune=not args.no_autotune)
        env.reset()
        env.use_graphs(True)
        paths = {"ids_policy_reactive": lambda: env.step(env.policy_reactive(out=env.action_buffer)),
                 "cmd_policy_field": lambda: env.step(env.policy_field(out=env.command_buffer))}

        def loop(body, k):
            for _ in range(k):
                body()

        def timed(body, k):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loop(body, k)
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        warm = {}
        for key, body in paths.items():
            loop(body, env.graph_period() + 1)  # every ring position's graph of this kind captured
            warm[key] = max(8, int(math.ceil(30.0 / max(timed(body, 8) * 1e3 / 8, 1e-3))))
        runs = {key: [] for key in paths}
        for _ in range(args.repeats):
            for key, body in paths.items():
                loop(body, warm[key])  # >= 30 ms of this path's own steps right before its timed region
                runs[key].append(timed(body, K))
        out = {"config": name, "n_envs": n, "steps": K, "fused": env.fused, "ring": env.ring,
               "frame_window": env.frame_window, "graphs": "single-step", "warm_steps": warm}
        for key, ts in runs.items():
            out[key] = {"env_steps_per_s": [round(n * K / t) for t in ts],
                        "ms_per_step": [round(t * 1e3 / K, 4) for t in ts]}
        med = {key: sorted(ts)[len(ts) // 2] for key, ts in runs.items()}
        out["cmd_over_ids"] = round(med["ids_policy_reactive"] / med["cmd_policy_field"], 4)
        # the policy kernels alone: K back-to-back launches between two events
        for key, fn, buf in (("policy_reactive_kernel_us", env.policy_reactive, env.action_buffer),
                             ("policy_field_kernel_us", env.policy_field, env.command_buffer)):
            loop(lambda: fn(out=buf), 50)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            loop(lambda: fn(out=buf), K)
            e1.record()
            torch.cuda.synchronize()
            out[key] = round(e0.elapsed_time(e1) * 1e3 / K, 3)
        env.check_errors()
        print(json.dumps(out), flush=True)
        env.close()
        del env, paths


if __name__ == "__main__":
    main()
