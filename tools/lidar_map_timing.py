#!/usr/bin/env python
"""Cost of one update of the accumulated scan map (include/ffmp.h ffmp_scan_map) beside the
single-scan launch it extends (lidar_frames(newest_only=True), whose kernel it leaves as it was).

For each config (default C2 — with C3's 180 beams, it has none of its own —, C3 and one GPU's share of
C5, unless --envs) and each frame format (f32, u8f16) one FFMPVec is reset and stepped a few times with
the reactive controller (ordinary mid-episode scans), the kinds are called alternately until `--warm-ms` (default 30) have passed, and then
`--repeats` regions of `--calls` back-to-back calls between two HIP events are timed per kind,
interleaved:
    scan          lidar_frames(out=, newest_only=True): the yardstick
    update        LidarMap.update(pose=) with the pose alternating between the env's own and one turned
                  by 0.1 rad and moved by (2.3, -1.7) cells, so every update gathers through a rotation
    update_still  LidarMap.update(): the pose has not changed, the gather is the identity
    update_plain  `update` with FFMP_SCAN_PLAIN
    update_nofrm  `update` on a holder made with frame=False: the planes alone
Each kind stands beside the bytes it moves (frame store; + 1 byte read and 1 written per cell for the
map) and their time at the 8 TB/s HBM spec.  Appends one JSON line per (config, format) to
profiles/lidar_map_timing.jsonl (--out) and prints it.  The pass is opt-in and off the step's path: a
record, no threshold.

    python tools/lidar_map_timing.py [--configs C2,C3,C5] [--formats f32,u8f16] [--calls 5] [--repeats 3] [--envs N]
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_SPEC = 8.0e12  # bytes per second


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C2,C3,C5")
    ap.add_argument("--formats", default="f32,u8f16")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warm-ms", type=float, default=30.0)
    ap.add_argument("--repeats", type=int, default=3, help="timed regions per kind, interleaved; all are reported")
    ap.add_argument("--envs", type=int, default=0, help="override the env count (default: the preset's, per GPU)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lidar_map_timing.jsonl"))
    args = ap.parse_args()
    import torch
    from flow_field_based_motion_planner_amd.config import PRESETS, preset
    from flow_field_based_motion_planner_amd.vec_env import FFMPVec

    for name in args.configs.split(","):
        for fmt in args.formats.split(","):
            n = args.envs or PRESETS[name]["n_envs"] // max(PRESETS[name]["gpus"], 1)
            cfg = preset(name)
            if cfg.n_beams == 0:  # C2 has no lidar of its own: give it C3's
                cfg = cfg.replace(n_beams=180)
            env = FFMPVec(n, cfg, device="cuda:0", autotune=False, obs_format=fmt)
            G, L = env.cfg.grid, env.cfg.n_beams
            env.reset()
            for _ in range(8):
                env.step(env.policy_reactive())
            newest = torch.empty((n, G, G), dtype=env._frame_dtype, device=env.device)
            pose_a = env.record[:, 0:4].contiguous()
            c, s = math.cos(0.1), math.sin(0.1)
            pose_b = pose_a.clone()
            pose_b[:, 0] += 2.3 * env.cfg.res
            pose_b[:, 1] -= 1.7 * env.cfg.res
            pose_b[:, 2] = pose_a[:, 2] * c - pose_a[:, 3] * s
            pose_b[:, 3] = pose_a[:, 3] * c + pose_a[:, 2] * s
            never = torch.zeros(n, dtype=torch.bool, device=env.device)
            m, still, bare = env.lidar_map(), env.lidar_map(), env.lidar_map(frame=False)
            turn = {id(m): 0, id(bare): 0}

            def moving(holder, plain=False):
                turn[id(holder)] ^= 1
                holder.update(pose=pose_b if turn[id(holder)] else pose_a, first=never, plain=plain)

            kinds = {"scan": lambda: env.lidar_frames(out=newest, newest_only=True),
                     "update": lambda: moving(m),
                     "update_still": lambda: still.update(),
                     "update_plain": lambda: moving(m, plain=True),
                     "update_nofrm": lambda: moving(bare)}
            frame_bytes = newest.numel() * newest.element_size()
            nbytes = {k: frame_bytes + 2 * n * G * G for k in kinds}
            nbytes["scan"] = frame_bytes
            nbytes["update_nofrm"] = 2 * n * G * G

            def timed(body, k):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(k):
                    body()
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1) / k  # ms per call

            t0 = time.perf_counter()
            while (time.perf_counter() - t0) * 1e3 < args.warm_ms:
                for body in kinds.values():
                    body()
                torch.cuda.synchronize()
            runs = {key: [] for key in kinds}
            for _ in range(args.repeats):
                for key, body in kinds.items():
                    runs[key].append(round(timed(body, args.calls), 4))
            med = {key: sorted(ts)[len(ts) // 2] for key, ts in runs.items()}
            share = {k: round(float((m.frame == v).float().mean()), 4) for k, v in (("free", 0), ("unknown", 128), ("occupied", 255))}
            out = {"config": name, "format": fmt, "n_envs": n, "grid": G, "n_beams": L, "calls": args.calls,
                   "warm_ms": args.warm_ms, "cell_shares": share, "ms_per_call": runs, "bytes_moved": nbytes,
                   "hbm_ms": {k: round(b / HBM_SPEC * 1e3, 4) for k, b in nbytes.items()},
                   "fraction_of_hbm_spec": {k: round(nbytes[k] / HBM_SPEC * 1e3 / med[k], 3) for k in nbytes},
                   "over_scan": {k: round(med[k] / med["scan"], 3) for k in kinds if k != "scan"}}
            env.check_errors()
            line = json.dumps(out)
            print(line, flush=True)
            os.makedirs(os.path.dirname(args.out), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")
            env.close()
            del env, kinds, newest, m, still, bare
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
