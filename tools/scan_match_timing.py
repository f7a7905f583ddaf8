#!/usr/bin/env python
"""Cost of scan-to-map matching (include/ffmp.h ffmp_scan_match) beside the world map's update it precedes.

For each config (default C2 with a 180-beam lidar, C3 and C5's share of 16,384 envs) a child process of its own resets
one FFMPVec and steps it 8 times with the reactive controller, updating the world map after every step.  Two warm-up
calls of every kind, then `--launches` calls per kind, each between two HIP events of its own, the kinds interleaved:
    match_R4T4   ffmp_scan_match at WorldMap.match's default knobs (radius 4, 4 turns)
    match_R2T2   the same at the localizer's knobs (radius 2, 2 turns)
    world_map    ffmp_world_map alone on the same plane, in place: the yardstick
(the library calls the holders make, without their bookkeeping; the prior is the env's own pose; pose_out and info are
written, the volume is not).  The presets' worlds are open — a handful of discs, the walls out of range — so their own
scans have few returns; every match kind is therefore timed twice, on the env's scan and, with the suffix _dense, on a
synthetic scan in which every beam returns (ranges uniform in 0.2 .. 0.9 of range_max): the two ends of the load.
Writes one JSON document (--out, default profiles/scan_match_launch.json) with one record
per config: the median, minimum and maximum ms per launch, the byte gathers of a launch — candidates x the valid beams of
every env, an upper bound: beams whose endpoint is off the plane gather nothing — and the gathers per second that gives
at the median, and each launch relative to the world map's update.  The pass is opt-in and off the step's path: a record, no threshold.

    python tools/scan_match_timing.py [--configs C2,C3,C5] [--launches 24] [--envs N] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHARE = {"C5": 16384}  # envs of the preset one GPU holds
KNOBS = {"R4T4": (4, 4), "R2T2": (2, 2)}


def one(name, args):
    import torch
    from flow_field_based_motion_planner_amd import _abi
    from flow_field_based_motion_planner_amd.config import PRESETS, beam_dirs, preset, turn_table
    from flow_field_based_motion_planner_amd.vec_env import FFMPVec

    n = args.envs or SHARE.get(name) or PRESETS[name]["n_envs"] // max(PRESETS[name]["gpus"], 1)
    cfg = preset(name)
    if cfg.n_beams == 0:
        cfg = cfg.replace(n_beams=180)
    env = FFMPVec(n, cfg, device="cuda:0", autotune=False)
    L = env.cfg.n_beams
    env.reset()
    wm = env.world_map()
    wm.update()
    for _ in range(8):
        env.step(env.policy_reactive())
        wm.update()
    lib, cfg_c, rec_t, lidar = env.lib, C.byref(env._cfg_c), env.record, env.lidar
    sectors, none = env._sectors(L), torch.zeros(n, dtype=torch.uint8, device=env.device)
    beams = torch.as_tensor(beam_dirs(L)).to(env.device).contiguous()
    dth = env.cfg.res / env.cfg.lidar_range
    W2, rm = wm.cells * wm.cells, wm.knobs[1]
    pose_out = torch.empty((n, 4), dtype=torch.float32, device=env.device)
    info = torch.zeros((n, 8), dtype=torch.int32, device=env.device)
    tables = {key: torch.as_tensor(turn_table(T, dth)).to(env.device).contiguous() for key, (R, T) in KNOBS.items()}

    gen = torch.Generator(device=env.device).manual_seed(1)
    dense = ((0.2 + 0.7 * torch.rand((n, L), generator=gen, device=env.device)) * rm).to(torch.float32).contiguous()

    def match(key, flags, rows):
        R, T = KNOBS[key]

        def body():
            _abi.check(lib.ffmp_scan_match(cfg_c, n, rows.data_ptr(), rows.stride(0), L, beams.data_ptr(), rec_t.data_ptr(),
                                           rec_t.stride(0), None, wm.log_odds.data_ptr(), W2, wm.cells, tables[key].data_ptr(), T, R, rm,
                                           max(8, L // 6), 0, pose_out.data_ptr(), info.data_ptr(), None, flags, env._stream()),
                       "ffmp_scan_match")
        return body

    def world_map():
        _abi.check(lib.ffmp_world_map(cfg_c, n, lidar.data_ptr(), lidar.stride(0), L, sectors.data_ptr(), rec_t.data_ptr(),
                                      rec_t.stride(0), None, none.data_ptr(), wm.log_odds.data_ptr(), W2, wm.cells, *wm.knobs, 0,
                                      env._stream()), "ffmp_world_map")

    kinds = {}
    for key in KNOBS:
        for rows, tag in ((lidar, ""), (dense, "_dense")):
            kinds[f"match_{key}{tag}"] = match(key, 0, rows)
    kinds["world_map"] = world_map
    for body in kinds.values():
        for _ in range(args.warmup):
            body()
    torch.cuda.synchronize()
    match("R4T4", 0, lidar)()
    valid = int(info[:, 6].sum())
    matched = round(float((info[:, 0] == 1).float().mean()), 4)
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
    gathers = {key + tag: (2 * T + 1) * (2 * R + 1) ** 2 * v for key, (R, T) in KNOBS.items() for tag, v in (("", valid), ("_dense", n * L))}
    of = lambda k: k.split("_")[1] + ("_dense" if k.endswith("_dense") else "")  # noqa: E731
    per_s = {k: round(gathers[of(k)] / (stat[k]["median"] * 1e-3) / 1e12, 3) for k in kinds if k != "world_map"}
    rec = {"config": name, "n_envs": n, "grid": env.cfg.grid, "n_beams": L, "cells": wm.cells, "map_bytes": wm.bytes, "range_max": rm,
           "dtheta": dth, "launches": args.launches, "warmup": args.warmup, "ms_per_launch": stat,
           "valid_beams_per_env": round(valid / n, 1), "byte_gathers": gathers, "tera_gathers_per_s": per_s,
           "over_world_map": {k: round(stat[k]["median"] / stat["world_map"]["median"], 3) for k in kinds if k != "world_map"},
           "matched_share": matched}
    env.check_errors()
    env.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C2,C3,C5")
    ap.add_argument("--launches", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--envs", type=int, default=0, help="override the env count (default: the preset's, per GPU)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scan_match_launch.json"))
    ap.add_argument("--child", default="", help="CONFIG — time that one config in this process and print its record")
    args = ap.parse_args()
    if args.child:
        print("RECORD " + json.dumps(one(args.child, args)), flush=True)
        return
    records = []
    for name in args.configs.split(","):  # one process per config: nothing of one run is warm in the next
        cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--launches", str(args.launches),
               "--warmup", str(args.warmup), "--envs", str(args.envs)]
        done = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if done.returncode:  # stop here: nothing more is started after a child that failed
            sys.exit(f"{name} failed ({done.returncode}):\n{done.stdout[-2000:]}\n{done.stderr[-4000:]}")
        line = [ln for ln in done.stdout.splitlines() if ln.startswith("RECORD ")][-1]
        print(line[7:], flush=True)
        records.append(json.loads(line[7:]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/scan_match_timing.py", "unit": "ms per launch, HIP events round each launch", "records": records},
                  f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
