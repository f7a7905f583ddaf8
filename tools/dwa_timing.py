#!/usr/bin/env python
"""Cost of one rollout-planner launch (include/ffmp.h ffmp_dwa) beside the launches it stands next to.

For each config (default C2, C3 and C5's share of 16,384 envs, all with moving discs and the flow planes switched
on) and each format (f32, u8f16) one FFMPVec is reset and stepped with the reactive controller.  Two warm-up calls
of every kind, then `--launches` calls per kind, each between two HIP events of its own, the kinds interleaved:
    dwa         ffmp_dwa alone over a cost plane made once: the default table (28 candidates, horizon 18), the
                newest frame and obs["flow"], every output
    predict     predicted_frames(out=): ffmp_flow_predict's launch, the point of comparison
    nav_cost    ffmp_nav_field with the cost plane as its only output: the launch policy_dwa shares with policy_nav
    policy_nav  policy_nav(out=)
    policy_dwa  policy_dwa(out=): nav_cost + dwa
Writes one JSON document (--out, default profiles/dwa_launch.json) with one record per (config, format): the
median, minimum and maximum ms per launch, and the bytes the dwa launch has to move — the frame cells within
src_reach of the robot, the flow of the source cells among them, A H cost cells, the table, the outputs.  The pass
is opt-in and off the step's path: a record, no threshold.

    python tools/dwa_timing.py [--configs C2,C3,C5] [--formats f32,u8f16] [--launches 24] [--envs N] [--out FILE]
"""
import argparse
import ctypes as C
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHARE = {"C5": 16384}  # envs of the preset one GPU holds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C2,C3,C5")
    ap.add_argument("--formats", default="f32,u8f16")
    ap.add_argument("--launches", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--envs", type=int, default=0, help="override the env count (default: the preset's, per GPU)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dwa_launch.json"))
    args = ap.parse_args()
    import torch
    from flow_field_based_motion_planner_amd import _abi
    from flow_field_based_motion_planner_amd.config import PRESETS, preset
    from flow_field_based_motion_planner_amd.vec_env import FFMPVec

    records = []
    for name in args.configs.split(","):
        for fmt in args.formats.split(","):
            n = args.envs or SHARE.get(name) or PRESETS[name]["n_envs"] // max(PRESETS[name]["gpus"], 1)
            cfg = preset(name).replace(moving=True, flow=True)
            env = FFMPVec(n, cfg, device="cuda:0", autotune=False, obs_format=fmt)
            G = env.cfg.grid
            env.reset()
            for _ in range(8):
                env.step(env.policy_reactive())
            cmd = torch.empty((n, 2), dtype=torch.float64, device=env.device)
            det = env.policy_dwa(detail=True)  # the table, the cost plane and every output, once
            cost, H = det["cost"], det["horizon"]
            _, traj, cmds = env._dwa_table(24, 1, 0.325)
            A = int(cmds.shape[0])
            frame, flow = env.state_m[:, 1], env.flow
            cps = float(torch.tensor(env.cfg.dt / env.cfg.res, dtype=torch.float32))
            reach = min(G // 2, 31 + int(math.ceil(H * cps * env.DWA_SPEED)))  # policy_dwa's default
            ffmt = _abi.OBS_F32 if frame.dtype == torch.float32 else _abi.OBS_U8F16
            vfmt = _abi.OBS_F32 if flow.dtype == torch.float32 else _abi.OBS_U8F16
            pred = torch.empty((n, G, G), dtype=torch.uint8, device=env.device)
            plane = torch.empty((n, G, G), dtype=torch.uint16, device=env.device)

            def dwa():
                _abi.check(env.lib.ffmp_dwa(C.byref(env._cfg_c), n, cost.data_ptr(), G * G, frame.data_ptr(), frame.stride(0), ffmt,
                                            flow.data_ptr(), flow.stride(0), vfmt, cps, reach, traj.data_ptr(), cmds.data_ptr(), A, H,
                                            None, 0.0, 0.0, None, det["choice"].data_ptr(), cmd.data_ptr(), det["score"].data_ptr(),
                                            det["n_adm"].data_ptr(), det["blocked_at"].data_ptr(), env._stream()), "ffmp_dwa")

            kinds = {"dwa": dwa,
                     "predict": lambda: env.predicted_frames(out=pred),
                     "nav_cost": lambda: env._nav_launch("nav_field", 2, 40, 4, 0.25, cost=plane),
                     "policy_nav": lambda: env.policy_nav(out=cmd),
                     "policy_dwa": lambda: env.policy_dwa(out=cmd)}
            for body in kinds.values():
                for _ in range(args.warmup):
                    body()
            torch.cuda.synchronize()
            assert torch.equal(cmd, det["cmd"])  # the launch timed is the launch policy_dwa makes
            pairs = {key: [] for key in kinds}
            for _ in range(args.launches):
                for key, body in kinds.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    body()
                    e1.record()
                    pairs[key].append((e0, e1))
            torch.cuda.synchronize()
            ms = {key: sorted(e0.elapsed_time(e1) for e0, e1 in evs) for key, evs in pairs.items()}
            stat = {key: {"median": round(t[len(t) // 2], 4), "min": round(t[0], 4), "max": round(t[-1], 4)} for key, t in ms.items()}
            c = G // 2
            lo, hi = max(c - reach, 0), min(c + reach, G - 1)
            region = frame[:, lo:hi + 1, lo:hi + 1]
            sources = int((region == 255).sum())
            fes, ves = frame.element_size(), flow.element_size()
            side = hi - lo + 1
            nbytes = {"frame_region": n * side * side * fes, "flow_of_sources": sources * 2 * ves, "cost_cells": n * A * H * 2,
                      "table": A * (H + 1) * 4 + A * 16, "outputs": n * (4 + 16 + 4 + 4 + A)}
            nbytes["total"] = sum(nbytes.values())
            full = n * G * G
            rec = {"config": name, "format": fmt, "n_envs": n, "grid": G, "n_obst": env.cfg.n_obst, "candidates": A, "horizon": H,
                   "src_reach": reach, "cps": cps, "launches": args.launches, "warmup": args.warmup, "ms_per_launch": stat,
                   "dwa_bytes": nbytes, "dwa_gb_per_s": round(nbytes["total"] / (stat["dwa"]["median"] * 1e-3) / 1e9, 1),
                   "predict_bytes": full * (fes + 1), "nav_cost_bytes": full * (fes + 2),
                   "source_cells_in_region_per_env": round(sources / n, 1),
                   "admissible_per_env": round(float(det["n_adm"].float().mean()), 2),
                   "none_admissible_share": round(float((det["choice"] < 0).float().mean()), 4),
                   "dwa_over_predict": round(stat["dwa"]["median"] / stat["predict"]["median"], 3),
                   "dwa_share_of_policy_dwa": round(stat["dwa"]["median"] / stat["policy_dwa"]["median"], 3)}
            env.check_errors()
            print(json.dumps(rec), flush=True)
            records.append(rec)
            env.close()
            del env, kinds, det, cost, plane, pred, cmd, frame, flow, region, pairs
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/dwa_timing.py", "unit": "ms per launch, HIP events round each launch", "records": records}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
