#!/usr/bin/env python
"""The crossing family (tests/flow_predict_ref.py: a disc crossing the robot's line to the goal, 24 scenes) in closed
loop on the GPU, planned from ground truth and from the scan alone.  Legs:
    plain            policy_nav() over the newest frame
    predicted        policy_nav(predict=dict(steps=24, slack=3)): the newest frame and obs["flow"]
    lidar_plain      L = 180: policy_nav(lidar=True), the map made from the scan, unknown cells free
    lidar_predicted  L = 180: a LidarFlow(lag=4) updated every step, policy_nav(predict=dict(flow=holder, other=0)) —
                     its scan frame (unknown cells free, as in the plain leg) and its estimated flow
Appends one JSON line per leg to profiles/flow_predict_crossing.jsonl (--out) and prints it: the outcome per scene
(1 goal, 2 collision, 3 truncated, 0 none), the step it happened at, the counts, and for the lidar legs the share of
live env-steps in which the holder had an estimate (more than `lag` updates).  A record, no threshold.

    python tools/flow_predict_crossing.py [--lag 4] [--beams 180]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lag", type=int, default=4)
    ap.add_argument("--beams", type=int, default=180)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flow_predict_crossing.jsonl"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from flow_field_based_motion_planner_amd.config import FFMPConfig
    from flow_field_based_motion_planner_amd.vec_env import FFMPVec
    from tests import flow_predict_ref as R
    from tests import nav_field_ref as NR

    sc = R.crossing_scenes()
    n = len(sc["pose"])
    for leg in ("plain", "predicted", "lidar_plain", "lidar_predicted"):
        lidar = leg.startswith("lidar")
        cfg = FFMPConfig(**dict(R.CROSS_CFG, n_beams=args.beams if lidar else 0))
        env = FFMPVec(n, cfg, device="cuda:0", autotune=False)
        env.reset()
        env.set_scenarios(**sc)
        env.check_errors()
        holder = env.lidar_flow(lag=args.lag) if leg == "lidar_predicted" else None
        flags, live_steps, with_estimate = [], 0, 0
        for _ in range(R.CROSS_STEPS):
            if holder is not None:
                holder.update()
                live = NR._outcomes(flags)[0] == 0 if flags else np.ones(n, bool)
                live_steps += int(live.sum())
                with_estimate += int(((holder.updates.cpu().numpy() > args.lag) & live).sum())
                cmd = env.policy_nav(predict=dict(flow=holder, other=0))
            elif leg == "lidar_plain":
                cmd = env.policy_nav(lidar=True)
            else:
                cmd = env.policy_nav(predict=dict(steps=24, slack=3) if leg == "predicted" else False)
            env.step(cmd)
            flags.append((env.is_goal.cpu().numpy().copy(), env.collision.cpu().numpy().copy(), env.truncated.cpu().numpy().copy()))
            if (NR._outcomes(flags)[0] != 0).all():
                break
        env.check_errors()
        env.close()
        o, t = NR._outcomes(flags)
        col, goal, neither, mean = R.summary(o, t)
        line = {"leg": leg, "n_beams": cfg.n_beams, "lag": args.lag if holder is not None else None,
                "outcomes": "".join(map(str, o.tolist())), "steps": t.tolist(), "collisions": col, "goals": goal, "neither": neither,
                "steps_per_reached_goal": None if goal == 0 else round(mean, 1),
                "estimate_share": round(with_estimate / live_steps, 3) if live_steps else None}
        print(json.dumps(line), flush=True)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
