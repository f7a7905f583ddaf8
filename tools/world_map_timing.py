#!/usr/bin/env python
"""Cost of the world-fixed scan map's two launches (include/ffmp.h ffmp_world_map / ffmp_world_frame)
beside the re-sampled map's one (ffmp_scan_map).

For each config (default C2 with a 180-beam lidar, C3 and C5's share of 16,384 envs) and each format (f32, u8f16)
a child process of its own resets one FFMPVec and steps it 8 times with the reactive controller, updating both maps
after every step.  Two warm-up calls of every kind, then `--launches` calls per kind, each between two HIP events of
its own, the kinds interleaved:
    world_map    ffmp_world_map alone on the WorldMap's plane, in place, default cells (the arena plus four cells a side)
    world_frame  ffmp_world_frame alone, the view at the env's pose
    scan_map     ffmp_scan_map alone on the LidarMap's pair of planes, with its frame: the point of comparison
(the library calls the holders make, without their bookkeeping copies; no env restarts in the timed calls).
Writes one JSON document (--out, default profiles/world_map_launch.json) with one record per (config, format): the
median, minimum and maximum ms per launch, the bytes each launch has to move and the TB/s that gives at the median.
world_map: the cells of every env's box (the sensor disc's bounding box clipped to the plane, columns rounded out to
multiples of 4) read and written once, and the scan; world_frame: one map byte per ego cell and the frame;
scan_map: a byte read, a byte written and a frame element per cell, and the scan.  The passes are opt-in and off
the step's path: a record, no threshold.

    python tools/world_map_timing.py [--configs C2,C3,C5] [--formats f32,u8f16] [--launches 24] [--envs N] [--out FILE]
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


def box_cells(pose, cells, res, range_max):
    """Cells of every env's box as world_map_kernel takes it (csrc/ffmp_worldmap.hip), summed; pose (n, 4) float32."""
    import numpy as np
    wh = float(np.float32(cells * res / 2.0))
    resf = float(np.float32(res))
    p = pose.astype(np.float64)
    reach = (range_max / np.hypot(p[:, 2], p[:, 3])) * (1.0 + 1e-5) + resf

    def span(at):
        lo = np.clip(np.floor((at - reach + wh) / resf) - 1.0, 0, cells)
        hi = np.clip(np.ceil((at + reach + wh) / resf) + 1.0, -1, cells - 1)
        return lo.astype(np.int64), hi.astype(np.int64)

    p0, p1 = span(p[:, 0])
    q0, q1 = span(p[:, 1])
    q0, q1 = q0 & ~3, q1 | 3
    return int((np.maximum(p1 - p0 + 1, 0) * np.maximum(q1 - q0 + 1, 0)).sum())


def one(name, fmt, args):
    import torch
    from flow_field_based_motion_planner_amd import _abi
    from flow_field_based_motion_planner_amd.config import PRESETS, preset
    from flow_field_based_motion_planner_amd.vec_env import FFMPVec

    n = args.envs or SHARE.get(name) or PRESETS[name]["n_envs"] // max(PRESETS[name]["gpus"], 1)
    cfg = preset(name)
    if cfg.n_beams == 0:
        cfg = cfg.replace(n_beams=180)
    env = FFMPVec(n, cfg, device="cuda:0", autotune=False, obs_format=fmt)
    G, L = env.cfg.grid, env.cfg.n_beams
    env.reset()
    wm, lm = env.world_map(), env.lidar_map()
    view = torch.empty((n, G, G), dtype=env._frame_dtype, device=env.device)
    wm.update()
    lm.update()
    for _ in range(8):
        env.step(env.policy_reactive())
        wm.update()
        lm.update()
    lib, cfg_c, rec_t, lidar = env.lib, C.byref(env._cfg_c), env.record, env.lidar
    sectors, none = env._sectors(L), torch.zeros(n, dtype=torch.uint8, device=env.device)
    W2 = wm.cells * wm.cells
    src, dst = lm._planes[lm._cur], lm._planes[1 - lm._cur]

    def world_map():
        _abi.check(lib.ffmp_world_map(cfg_c, n, lidar.data_ptr(), lidar.stride(0), L, sectors.data_ptr(), rec_t.data_ptr(),
                                      rec_t.stride(0), None, none.data_ptr(), wm.log_odds.data_ptr(), W2, wm.cells, *wm.knobs, 0,
                                      env._stream()), "ffmp_world_map")

    def world_frame():
        _abi.check(lib.ffmp_world_frame(cfg_c, n, rec_t.data_ptr(), rec_t.stride(0), wm.log_odds.data_ptr(), W2, wm.cells,
                                        view.data_ptr(), G * G, *wm.view, env._stream()), "ffmp_world_frame")

    def scan_map():
        _abi.check(lib.ffmp_scan_map(cfg_c, n, lidar.data_ptr(), lidar.stride(0), L, sectors.data_ptr(), rec_t.data_ptr(),
                                     rec_t.stride(0), lm._pose.data_ptr(), 4, None, none.data_ptr(), src.data_ptr(), dst.data_ptr(),
                                     G * G, lm.frame.data_ptr(), G * G, *lm.knobs, 0, env._stream()), "ffmp_scan_map")

    kinds = {"world_map": world_map, "world_frame": world_frame, "scan_map": scan_map}
    for body in kinds.values():
        for _ in range(args.warmup):
            body()
    torch.cuda.synchronize()
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
    fes = view.element_size()
    scan = n * L * 4 + L * 8
    visited = box_cells(env.record[:, 0:4].cpu().numpy(), wm.cells, env.cfg.res, env.cfg.lidar_range)
    nbytes = {"world_map": 2 * visited + scan, "world_frame": n * G * G * (1 + fes) + n * 16, "scan_map": n * G * G * (2 + fes) + scan + n * 32}
    f = view.cpu()
    rec = {"config": name, "format": fmt, "n_envs": n, "grid": G, "n_beams": L, "cells": wm.cells, "map_bytes": wm.bytes,
           "range_max": env.cfg.lidar_range, "launches": args.launches, "warmup": args.warmup, "ms_per_launch": stat,
           "box_cells_per_env": round(visited / n, 1), "bytes": nbytes,
           "tb_per_s": {k: round(nbytes[k] / (stat[k]["median"] * 1e-3) / 1e12, 3) for k in kinds},
           "world_map_over_scan_map": round(stat["world_map"]["median"] / stat["scan_map"]["median"], 3),
           "view_shares": {"occupied": round(float((f == 255).float().mean()), 4), "free": round(float((f == 0).float().mean()), 4)}}
    env.check_errors()
    env.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C2,C3,C5")
    ap.add_argument("--formats", default="f32,u8f16")
    ap.add_argument("--launches", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--envs", type=int, default=0, help="override the env count (default: the preset's, per GPU)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "world_map_launch.json"))
    ap.add_argument("--child", default="", help="CONFIG:FORMAT — time that one pair in this process and print its record")
    args = ap.parse_args()
    if args.child:
        name, fmt = args.child.split(":")
        print("RECORD " + json.dumps(one(name, fmt, args)), flush=True)
        return
    records = []
    for name in args.configs.split(","):
        for fmt in args.formats.split(","):  # one process per config and format: nothing of one run is warm in the next
            cmd = [sys.executable, os.path.abspath(__file__), "--child", f"{name}:{fmt}", "--launches", str(args.launches),
                   "--warmup", str(args.warmup), "--envs", str(args.envs)]
            done = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            if done.returncode:  # stop here: nothing more is started after a child that failed
                sys.exit(f"{name}:{fmt} failed ({done.returncode}):\n{done.stdout[-2000:]}\n{done.stderr[-4000:]}")
            out = done.stdout
            line = [ln for ln in out.splitlines() if ln.startswith("RECORD ")][-1]
            print(line[7:], flush=True)
            records.append(json.loads(line[7:]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/world_map_timing.py", "unit": "ms per launch, HIP events round each launch", "records": records},
                  f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
