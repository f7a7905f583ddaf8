#!/usr/bin/env python
"""Cost of one predicted-occupancy pass (include/ffmp.h ffmp_flow_predict) beside the launches it
stands next to.

For each config (default C2 and C3, both with moving discs and the flow planes switched on) and each format
(f32, u8f16) one FFMPVec is reset and stepped with the reactive controller.  Two warm-up calls of every kind,
then `--repeats` regions of `--calls` back-to-back calls between two HIP events per kind, interleaved:
    predict     predicted_frames(out=) over the newest frame and obs["flow"]: the launch alone
    nav         policy_nav(frames=) over that plane: the navigation field alone on the same frames
    step        FFMPVec.step() with the reactive controller's actions
    fill        torch's fill_ of the uint8 output: the pure-store floor
    copy        torch's copy_ of the newest frame into a uint8 tensor: the frame read plus the store, without
                the flow — the floor of a pass that skips the flow of every group without a source
Appends one JSON line per (config, format) to profiles/flow_predict_timing.jsonl (--out) and prints it: the
times, the share of 16-cell groups that hold a source (whose flow is loaded), the swept cells per env, the
ratio of `predict` to `copy`, `fill`, `nav` and `step`.  The pass is opt-in and off the step's path: a record,
no threshold.

--horizons 1,64 also times predicted_frames(steps=H) — what the sources' walks cost — and --tag labels the line,
e.g. with a probe build of the library under FFMP_LIB (profiles/flow_predict_variants.jsonl).

    python tools/flow_predict_timing.py [--configs C2,C3] [--formats f32,u8f16] [--calls 5] [--repeats 3] [--envs N]
                                        [--horizons 1,64] [--tag NAME]
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
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3, help="timed regions per kind, interleaved; all are reported")
    ap.add_argument("--envs", type=int, default=0, help="override the env count (default: the preset's, per GPU)")
    ap.add_argument("--horizons", default="", help="also time predicted_frames(steps=H) for these H, e.g. 1,64: what the walks cost")
    ap.add_argument("--tag", default="", help="a label for the line, e.g. the library variant under FFMP_LIB")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flow_predict_timing.jsonl"))
    args = ap.parse_args()
    import torch
    from flow_field_based_motion_planner_amd.config import PRESETS, preset
    from flow_field_based_motion_planner_amd.vec_env import FFMPVec

    for name in args.configs.split(","):
        for fmt in args.formats.split(","):
            n = args.envs or PRESETS[name]["n_envs"] // max(PRESETS[name]["gpus"], 1)
            cfg = preset(name).replace(moving=True, flow=True)
            env = FFMPVec(n, cfg, device="cuda:0", autotune=False, obs_format=fmt)
            G = env.cfg.grid
            G2 = G * G
            env.reset()
            for _ in range(8):
                env.step(env.policy_reactive())
            actions = env.policy_reactive()
            out = torch.empty((n, G, G), dtype=torch.uint8, device=env.device)
            floor = torch.empty((n, G, G), dtype=torch.uint8, device=env.device)
            cmd = torch.empty((n, 2), dtype=torch.float64, device=env.device)
            kinds = {"predict": lambda: env.predicted_frames(out=out),
                     "nav": lambda: env.policy_nav(frames=out, out=cmd),
                     "step": lambda: env.step(actions),
                     "fill": lambda: floor.fill_(0),
                     "copy": lambda: floor.copy_(env.state_m[:, 1])}
            for h in [int(x) for x in args.horizons.split(",") if x]:
                kinds[f"predict_steps_{h}"] = lambda h=h: env.predicted_frames(out=out, steps=h)

            def timed(body, k):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(k):
                    body()
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1) / k  # ms per call

            for key, body in kinds.items():
                for _ in range(args.warmup):
                    body()
            torch.cuda.synchronize()
            runs = {key: [] for key in kinds}
            for _ in range(args.repeats):
                for key, body in kinds.items():
                    runs[key].append(round(timed(body, args.calls), 4))
            med = {key: sorted(ts)[len(ts) // 2] for key, ts in runs.items()}
            _, n_swept = env.predicted_frames(out=out, count=True)
            frame = env.state_m[:, 1]
            src = (frame == 255).reshape(n, G2 // 16, 16)
            groups = float(src.any(dim=2).float().mean())
            fes, ves = frame.element_size(), env.flow.element_size()
            nbytes = {"fill": n * G2, "copy": n * G2 * (fes + 1),
                      "predict": int(n * G2 * (fes + 1 + 2 * ves * groups)), "predict_all_flow": n * G2 * (fes + 1 + 2 * ves)}
            out_line = {"tag": args.tag, "config": name, "format": fmt, "n_envs": n, "grid": G, "n_obst": env.cfg.n_obst,
                        "knobs": {"steps": 24, "slack": 3, "pace": 6, "cps": 2.0}, "calls": args.calls, "warmup": args.warmup,
                        "source_cells_share": round(float(src.float().mean()), 4), "source_groups_share": round(groups, 4),
                        "swept_cells_per_env": round(float(n_swept.float().mean()), 1), "ms_per_call": runs, "bytes_moved": nbytes,
                        "hbm_ms": {k: round(b / HBM_SPEC * 1e3, 4) for k, b in nbytes.items()},
                        "predict_over": {k: round(med["predict"] / med[k], 3) for k in ("copy", "fill", "nav", "step")}}
            env.check_errors()
            line = json.dumps(out_line)
            print(line, flush=True)
            os.makedirs(os.path.dirname(args.out), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")
            env.close()
            del env, kinds, out, floor, cmd, frame, src, n_swept
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
