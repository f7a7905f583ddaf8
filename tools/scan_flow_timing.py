#!/usr/bin/env python
"""Cost of one update of the flow estimated from the scan (include/ffmp.h ffmp_scan_flow) beside
the launches it stands next to.

For each config (default C2 — with C3's 180 beams, it has none of its own — and C3, unless --envs) and each
format (f32, u8f16) one FFMPVec is reset and stepped with the reactive controller; the scan and the pose are
saved, the env is stepped `lag` more times and they are saved again.  Two warm-up calls of every kind, then
`--repeats` regions of `--calls` back-to-back calls between two HIP events per kind, interleaved:
    update        LidarFlow.update(ranges=, pose=) fed the two saved scans in runs of `lag`, so the frame of
                  `lag` updates ago is always the other scan: every update searches as a live one does
    scan_launch   its first launch alone: ffmp_scan_frames, newest only, uint8, into a ring slot
    flow_launch   its second launch alone: ffmp_scan_flow on the two saved frames and poses
    scan          lidar_frames(out=, newest_only=True) in the env's frame format
    map_update    LidarMap.update()
    step          FFMPVec.step() with the reactive controller's actions
    fill          torch's fill_ of the flow tensor: the pure-store floor of the flow planes
Appends one JSON line per (config, format) to profiles/scan_flow_timing.jsonl (--out) and prints it: the
times, the hit cells per env and the kinds of the timed frames, the ratio of `update` and `flow_launch` to
`fill` and to `map_update`.  The pass is opt-in and off the step's path: a record, no threshold.

    python tools/scan_flow_timing.py [--configs C2,C3] [--formats f32,u8f16] [--calls 5] [--repeats 3] [--envs N] [--lag 4]
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_SPEC = 8.0e12  # bytes per second


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C2,C3")
    ap.add_argument("--formats", default="f32,u8f16")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3, help="timed regions per kind, interleaved; all are reported")
    ap.add_argument("--envs", type=int, default=0, help="override the env count (default: the preset's, per GPU)")
    ap.add_argument("--lag", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scan_flow_timing.jsonl"))
    args = ap.parse_args()
    import torch
    from flow_field_based_motion_planner_amd import _abi
    from flow_field_based_motion_planner_amd.config import PRESETS, preset
    from flow_field_based_motion_planner_amd.vec_env import FFMPVec

    for name in args.configs.split(","):
        for fmt in args.formats.split(","):
            n = args.envs or PRESETS[name]["n_envs"] // max(PRESETS[name]["gpus"], 1)
            cfg = preset(name)
            if cfg.n_beams == 0:  # C2 has no lidar of its own: give it C3's
                cfg = cfg.replace(n_beams=180)
            env = FFMPVec(n, cfg, device="cuda:0", autotune=False, obs_format=fmt)
            G, L, lag = env.cfg.grid, env.cfg.n_beams, args.lag
            G2 = G * G
            env.reset()
            for _ in range(8):
                env.step(env.policy_reactive())
            scans, poses = [env.lidar.clone()], [env.record[:, 0:4].contiguous()]
            for _ in range(lag):
                env.step(env.policy_reactive())
            scans.append(env.lidar.clone())
            poses.append(env.record[:, 0:4].contiguous())
            actions = env.policy_reactive()
            never = torch.zeros(n, dtype=torch.bool, device=env.device)
            m, lmap = env.lidar_flow(lag=lag), env.lidar_map()
            newest = torch.empty((n, G, G), dtype=env._frame_dtype, device=env.device)
            frames = torch.empty((2, n, G, G), dtype=torch.uint8, device=env.device)
            for k in range(2):
                env._scan_launch(scans[k], None, frames[k].data_ptr(), G2, _abi.OBS_U8F16, *m.scan_knobs)
            calls = {"update": 0}

            def update():
                k = (calls["update"] // lag) & 1
                calls["update"] += 1
                m.update(ranges=scans[k], pose=poses[k], first=never)

            def flow_launch():
                _abi.check(env.lib.ffmp_scan_flow(C.byref(env._cfg_c), n, frames[1].data_ptr(), frames[0].data_ptr(), G2,
                                                  poses[1].data_ptr(), 4, poses[0].data_ptr(), 4, None, None, m.flow.data_ptr(),
                                                  2 * G2, m.kind.data_ptr(), G2, *m.knobs, env._stream()), "ffmp_scan_flow")

            kinds = {"update": update,
                     "scan_launch": lambda: env._scan_launch(scans[1], None, frames[1].data_ptr(), G2, _abi.OBS_U8F16, *m.scan_knobs),
                     "flow_launch": flow_launch,
                     "scan": lambda: env.lidar_frames(out=newest, newest_only=True),
                     "map_update": lambda: lmap.update(),
                     "step": lambda: env.step(actions),
                     "fill": lambda: m.flow.fill_(0)}

            def timed(body, k):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(k):
                    body()
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1) / k  # ms per call

            for _ in range(max(args.warmup, 2 * lag)):  # the ring of `update` holds both scans from here on
                update()
            for key, body in kinds.items():
                for _ in range(args.warmup):
                    body()
            torch.cuda.synchronize()
            runs = {key: [] for key in kinds}
            for _ in range(args.repeats):
                for key, body in kinds.items():
                    runs[key].append(round(timed(body, args.calls), 4))
            med = {key: sorted(ts)[len(ts) // 2] for key, ts in runs.items()}
            flow_launch()
            torch.cuda.synchronize()
            hits = float((frames[1] == 255).sum()) / n
            kshare = {str(v): round(float((m.kind == v).sum()) / n, 2) for v in (1, 2)}
            flow_bytes = m.flow.numel() * m.flow.element_size()
            nbytes = {"fill": flow_bytes, "flow_launch": flow_bytes + 3 * n * G2, "scan_launch": n * G2,
                      "update": flow_bytes + 4 * n * G2}
            out = {"config": name, "format": fmt, "n_envs": n, "grid": G, "n_beams": L, "lag": lag, "knobs": list(m.knobs[2:]),
                   "calls": args.calls, "warmup": args.warmup, "hit_cells_per_env": round(hits, 1),
                   "cells_per_env_by_kind": kshare, "ms_per_call": runs, "bytes_moved": nbytes,
                   "hbm_ms": {k: round(b / HBM_SPEC * 1e3, 4) for k, b in nbytes.items()},
                   "over_fill": {k: round(med[k] / med["fill"], 3) for k in ("update", "flow_launch")},
                   "over_map_update": {k: round(med[k] / med["map_update"], 3) for k in ("update", "flow_launch")},
                   "over_step": {k: round(med[k] / med["step"], 3) for k in ("update", "flow_launch")}}
            env.check_errors()
            line = json.dumps(out)
            print(line, flush=True)
            os.makedirs(os.path.dirname(args.out), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")
            env.close()
            del env, kinds, newest, frames, m, lmap, scans, poses
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
