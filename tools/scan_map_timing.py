#!/usr/bin/env python
"""Cost of the frames built from the lidar scan (include/ffmp.h ffmp_scan_frames) beside the env step.

For each config (default C3: 32,768 x 256^2 with 180 beams, and one GPU's share of C5: 16,384 x 512^2
with 360 beams, unless --envs) and each frame format (f32, u8f16) one FFMPVec is reset and stepped a
few times with the reactive controller (so the scans are ordinary mid-episode scans), then K
back-to-back calls between two HIP events are timed, after `--warm` untimed calls of the same kind,
`--repeats` regions per kind, interleaved:
    step            step(actions) — the env step the pass is quoted against
    both            lidar_frames(out=) into a preallocated (N, 2, G, G) block: the in-place shift
    newest          lidar_frames(out=, newest_only=True) into a preallocated (N, G, G) plane
    both_plain, newest_plain   the same with FFMP_SCAN_PLAIN (the SPEC's bisection for every cell)
    visible_newest  visible_frames(out=, newest_only=True): the ground-truth pass at the same config
    fill_both, fill_newest     torch's fill_ of the same tensors: what a pure store stream takes there
Each kind stands beside the bytes it writes (the shift also reads one frame) and their time at the
8 TB/s HBM spec ("hbm_ms"); the ratios to the fill, to visible_frames and to the step are derived from
the medians.  Appends one JSON line per (config, format) to profiles/scan_map_timing.jsonl (--out)
and prints it.  The pass is opt-in and off the step's path: a record, no threshold.

    python tools/scan_map_timing.py [--configs C3,C5] [--formats f32,u8f16] [--calls 5] [--repeats 3] [--envs N]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_SPEC = 8.0e12  # bytes per second


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C3,C5")
    ap.add_argument("--formats", default="f32,u8f16")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3, help="timed regions per kind, interleaved; all are reported")
    ap.add_argument("--envs", type=int, default=0, help="override the env count (default: the preset's, per GPU)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scan_map_timing.jsonl"))
    args = ap.parse_args()
    import torch
    from flow_field_based_motion_planner_amd.config import PRESETS, preset
    from flow_field_based_motion_planner_amd.vec_env import FFMPVec

    for name in args.configs.split(","):
        for fmt in args.formats.split(","):
            n = args.envs or PRESETS[name]["n_envs"] // max(PRESETS[name]["gpus"], 1)
            env = FFMPVec(n, preset(name), device="cuda:0", autotune=False, obs_format=fmt)
            G, L = env.cfg.grid, env.cfg.n_beams
            env.reset()
            for _ in range(8):
                env.step(env.policy_reactive())
            actions = env.policy_reactive().clone()
            both = torch.empty((n, 2, G, G), dtype=env._frame_dtype, device=env.device)
            newest = torch.empty((n, G, G), dtype=env._frame_dtype, device=env.device)
            kinds = {"step": lambda: env.step(actions),
                     "both": lambda: env.lidar_frames(out=both),
                     "newest": lambda: env.lidar_frames(out=newest, newest_only=True),
                     "both_plain": lambda: env.lidar_frames(out=both, plain=True),
                     "newest_plain": lambda: env.lidar_frames(out=newest, newest_only=True, plain=True),
                     "visible_newest": lambda: env.visible_frames(out=newest, newest_only=True),
                     "fill_both": lambda: both.fill_(0), "fill_newest": lambda: newest.fill_(0)}
            nbytes = {"both": both.numel() * both.element_size(), "newest": newest.numel() * newest.element_size()}
            for k in ("both_plain", "fill_both"):
                nbytes[k] = nbytes["both"]
            for k in ("newest_plain", "visible_newest", "fill_newest"):
                nbytes[k] = nbytes["newest"]

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
            env.lidar_frames(out=newest, newest_only=True)
            torch.cuda.synchronize()
            share = {k: round(float((newest == v).float().mean()), 4) for k, v in (("free", 0), ("unknown", 128), ("occupied", 255))}
            out = {"config": name, "format": fmt, "n_envs": n, "grid": G, "n_beams": L, "calls": args.calls, "warm": args.warm,
                   "cell_shares": share, "ms_per_call": runs, "bytes_written": nbytes,
                   "hbm_ms": {k: round(b / HBM_SPEC * 1e3, 4) for k, b in nbytes.items()},
                   "fraction_of_hbm_spec": {k: round(nbytes[k] / HBM_SPEC * 1e3 / med[k], 3) for k in nbytes},
                   "over_step": {k: round(med[k] / med["step"], 3) for k in nbytes},
                   "over_fill": {"both": round(med["both"] / med["fill_both"], 2),
                                 "newest": round(med["newest"] / med["fill_newest"], 2)},
                   "over_visible": {"newest": round(med["newest"] / med["visible_newest"], 2)},
                   "plain_over_shortcut": {"both": round(med["both_plain"] / med["both"], 2),
                                           "newest": round(med["newest_plain"] / med["newest"], 2)}}
            env.check_errors()
            line = json.dumps(out)
            print(line, flush=True)
            os.makedirs(os.path.dirname(args.out), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")
            env.close()
            del env, kinds, both, newest
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
