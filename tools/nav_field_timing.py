#!/usr/bin/env python
"""Cost of the navigation field (include/ffmp.h ffmp_nav_field) beside the env step.

For each config (default C2: 4,096 x 128^2 with 8 static discs, and C3: 256^2 with 16 discs, the
preset's env counts unless --envs) one FFMPVec is reset and stepped a few times with the reactive
controller (so the frames are ordinary mid-episode frames), then K back-to-back calls between two
HIP events are timed, after `--warm` untimed calls of the same kind, `--repeats` regions per kind,
interleaved:
    step            step(actions) — the env step the field is quoted against
    nav_cmd         ffmp_nav_field writing cmd only (policy_nav into a preallocated tensor)
    nav_planes      ffmp_nav_field writing the cost and dir planes (+ target, geo_cost)
Appends one JSON line per config to profiles/nav_field_timing.jsonl (--out) and prints it.  The field
is opt-in and off the hot path: a record, no threshold.

    python tools/nav_field_timing.py [--configs C2,C3] [--calls 5] [--repeats 3] [--envs N]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C2,C3")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3, help="timed regions per kind, interleaved; all are reported")
    ap.add_argument("--envs", type=int, default=0, help="override the preset's env count")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nav_field_timing.jsonl"))
    args = ap.parse_args()
    import torch
    from flow_field_based_motion_planner_amd.config import PRESETS, preset
    from flow_field_based_motion_planner_amd.vec_env import FFMPVec

    for name in args.configs.split(","):
        n = args.envs or PRESETS[name]["n_envs"]
        env = FFMPVec(n, preset(name), device="cuda:0", autotune=False)
        G = env.cfg.grid
        env.reset()
        for _ in range(8):
            env.step(env.policy_reactive())
        actions = env.policy_reactive().clone()
        kn = dict(FFMPVec.NAV_DEFAULTS)
        cmd = torch.empty((n, 2), dtype=torch.float64, device=env.device)
        cost = torch.empty((n, G, G), dtype=torch.uint16, device=env.device)
        dirs = torch.empty((n, G, G), dtype=torch.uint8, device=env.device)
        target = torch.empty((n, 2), dtype=torch.int32, device=env.device)
        geo = torch.empty(n, dtype=torch.int32, device=env.device)
        kinds = {"step": lambda: env.step(actions),
                 "nav_cmd": lambda: env._nav_launch("nav_field", **kn, cmd=cmd),
                 "nav_planes": lambda: env._nav_launch("nav_field", **kn, cost=cost, direction=dirs, target=target, geo_cost=geo)}

        def timed(body, k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(k):
                body()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / k  # ms per call

        runs = {key: [] for key in kinds}
        for _ in range(args.repeats):
            for key, body in kinds.items():
                timed(body, args.warm)
                runs[key].append(round(timed(body, args.calls), 4))
        med = {key: sorted(ts)[len(ts) // 2] for key, ts in runs.items()}
        reach = int((geo >= 0).sum())
        out = {"config": name, "n_envs": n, "grid": G, "n_obst": env.cfg.n_obst, "calls": args.calls, "warm": args.warm,
               "knobs": kn, "reachable_envs": reach, "ms_per_call": runs,
               "nav_cmd_over_step": round(med["nav_cmd"] / med["step"], 2),
               "nav_planes_over_step": round(med["nav_planes"] / med["step"], 2)}
        env.check_errors()
        line = json.dumps(out)
        print(line, flush=True)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
        env.close()
        del env, kinds, cost, dirs


if __name__ == "__main__":
    main()
