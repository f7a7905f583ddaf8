#!/usr/bin/env python
"""Cost of the sensor-visible frames (include/ffmp.h ffmp_visible_frames) beside the env step.

For each config (default C2: 4,096 x 128^2 with 8 discs, and C3: 32,768 x 256^2 with 16 discs, the
preset's env counts unless --envs) and each frame format (f32, u8f16) one FFMPVec is reset and stepped
a few times with the reactive controller (so the records are ordinary mid-episode records), then K
back-to-back calls between two HIP events are timed, after `--warm` untimed calls of the same kind,
`--repeats` regions per kind, interleaved:
    step            step(actions) — the env step the pass is quoted against
    both            visible_frames() into a preallocated (N, 2, G, G) block
    newest          visible_frames(newest_only=True) into a preallocated (N, G, G) plane
    both_nocull, newest_nocull   the same with FFMP_VISIBLE_NOCULL (every disc for every cell)
    fill_both, fill_newest       torch's fill_ of the same tensors: what a pure store stream takes there
Each kind stands beside the bytes it writes and their time at the 8 TB/s HBM spec ("hbm_ms"); the
achieved fraction of that spec and the NOCULL / culled ratio are derived from the medians.  Appends
one JSON line per (config, format) to profiles/visible_frames_timing.jsonl (--out) and prints it.
The pass is opt-in and off the step's path: a record, no threshold.

    python tools/visible_timing.py [--configs C2,C3] [--formats f32,u8f16] [--calls 5] [--repeats 3] [--envs N]
    python tools/visible_timing.py --configs C3 --formats f32 --discs 0     # the cost with no disc at all
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
    ap.add_argument("--configs", default="C2,C3")
    ap.add_argument("--formats", default="f32,u8f16")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3, help="timed regions per kind, interleaved; all are reported")
    ap.add_argument("--envs", type=int, default=0, help="override the preset's env count")
    ap.add_argument("--discs", type=int, default=None, help="override the preset's disc count (0: what the pass costs with nothing to cull)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "visible_frames_timing.jsonl"))
    args = ap.parse_args()
    import torch
    from flow_field_based_motion_planner_amd.config import PRESETS, preset
    from flow_field_based_motion_planner_amd.vec_env import FFMPVec

    for name in args.configs.split(","):
        for fmt in args.formats.split(","):
            n = args.envs or PRESETS[name]["n_envs"]
            cfg = preset(name) if args.discs is None else preset(name).replace(n_obst=args.discs)
            env = FFMPVec(n, cfg, device="cuda:0", autotune=False, obs_format=fmt)
            G = env.cfg.grid
            env.reset()
            for _ in range(8):
                env.step(env.policy_reactive())
            actions = env.policy_reactive().clone()
            both = torch.empty((n, 2, G, G), dtype=env._frame_dtype, device=env.device)
            newest = torch.empty((n, G, G), dtype=env._frame_dtype, device=env.device)
            kinds = {"step": lambda: env.step(actions),
                     "both": lambda: env.visible_frames(out=both),
                     "newest": lambda: env.visible_frames(out=newest, newest_only=True),
                     "both_nocull": lambda: env.visible_frames(out=both, nocull=True),
                     "newest_nocull": lambda: env.visible_frames(out=newest, newest_only=True, nocull=True),
                     "fill_both": lambda: both.fill_(0), "fill_newest": lambda: newest.fill_(0)}
            nbytes = {"both": both.numel() * both.element_size(), "newest": newest.numel() * newest.element_size()}
            nbytes["both_nocull"], nbytes["newest_nocull"] = nbytes["both"], nbytes["newest"]
            nbytes["fill_both"], nbytes["fill_newest"] = nbytes["both"], nbytes["newest"]

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
            env.visible_frames(out=both)
            torch.cuda.synchronize()
            out = {"config": name, "format": fmt, "n_envs": n, "grid": G, "n_obst": env.cfg.n_obst, "calls": args.calls,
                   "warm": args.warm, "unknown_fraction": round(float((both == 128).float().mean()), 4), "ms_per_call": runs,
                   "bytes_written": nbytes, "hbm_ms": {k: round(b / HBM_SPEC * 1e3, 4) for k, b in nbytes.items()},
                   "fraction_of_hbm_spec": {k: round(nbytes[k] / HBM_SPEC * 1e3 / med[k], 3) for k in nbytes},
                   "over_step": {k: round(med[k] / med["step"], 3) for k in nbytes},
                   "nocull_over_culled": {"both": round(med["both_nocull"] / med["both"], 2),
                                          "newest": round(med["newest_nocull"] / med["newest"], 2)},
                   "over_fill": {"both": round(med["both"] / med["fill_both"], 2),
                                 "newest": round(med["newest"] / med["fill_newest"], 2)}}
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
