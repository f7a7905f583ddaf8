#!/usr/bin/env python
"""Cost of one frame-potential pass (include/ffmp.h ffmp_frame_potential) beside a plain fill of the
bytes it stores.

For each config (default C2, C3 and C5's one-GPU share) and each format (f32: float32 frames and a float32
potential plane; u8f16: uint8 frames and a binary16 plane) one FFMPVec is reset and stepped with the reactive
controller.  Warm-up calls of every kind, then `--repeats` regions of `--calls` back-to-back calls between two
HIP events per kind, interleaved:
    potential   the launch of frame_potential() over the newest frame: the plane, the gradient and robot_d2
    all         the same with the dist2 plane as well
    grad        the launch of frame_potential(potential=False): the gradient and robot_d2 alone, what
                policy_field(lidar=True) adds
    fill        torch's fill_ of the potential plane: the pure-store floor of `potential`
    fill_all    fill_ of the potential and the dist2 planes: the floor of `all`
    step        FFMPVec.step() with the reactive controller's actions, for scale
Appends one JSON line per (config, format) to profiles/frame_potential_timing.jsonl (--out) and prints it: the
times, the share of obstacle cells and of cells within reach of one, the bytes each kind moves and the ratio of
each pass to its fill.  The pass is opt-in and off the step's path: a record, no threshold.

    python tools/frame_potential_timing.py [--configs C2,C3,C5] [--formats f32,u8f16] [--calls 10] [--repeats 5]
                                           [--envs N] [--occ-min 255] [--reach R] [--tag NAME]
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
    ap.add_argument("--configs", default="C2,C3,C5")
    ap.add_argument("--formats", default="f32,u8f16")
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5, help="timed regions per kind, interleaved; all are reported")
    ap.add_argument("--envs", type=int, default=0, help="override the env count (default: the preset's, per GPU)")
    ap.add_argument("--occ-min", type=int, default=255)
    ap.add_argument("--reach", type=int, default=0, help="0: ceil(rho0 / res)")
    ap.add_argument("--tag", default="", help="a label for the line, e.g. the library variant under FFMP_LIB")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frame_potential_timing.jsonl"))
    args = ap.parse_args()
    import torch
    from flow_field_based_motion_planner_amd.config import PRESETS, preset
    from flow_field_based_motion_planner_amd.vec_env import FFMPVec

    for name in args.configs.split(","):
        for fmt in args.formats.split(","):
            n = args.envs or PRESETS[name]["n_envs"] // max(PRESETS[name]["gpus"], 1)
            env = FFMPVec(n, preset(name), device="cuda:0", autotune=False, obs_format=fmt)
            G = env.cfg.grid
            G2 = G * G
            env.reset()
            for _ in range(8):
                env.step(env.policy_reactive())
            actions = env.policy_reactive()
            pdt = torch.float32 if fmt == "f32" else torch.float16
            reach = args.reach or None
            small = {"grad": torch.empty((n, 2), device=env.device), "robot_d2": torch.empty(n, dtype=torch.int32, device=env.device)}
            pot = torch.empty((n, G, G), dtype=pdt, device=env.device)
            d2 = torch.empty((n, G, G), dtype=torch.uint16, device=env.device)
            d2_bytes = d2.view(torch.uint8)
            knobs = dict(occ_min=args.occ_min, reach=reach, dtype=pdt)
            cells = env._potential_reach("frame_potential", reach, True)

            def launch(**planes):  # the launch alone, without the (N,) clearance the public call derives
                env._potential_launch(None, None, args.occ_min, cells, grad=small["grad"],
                                      robot_d2=small["robot_d2"], **planes)

            def fill_all():
                pot.fill_(0)
                d2_bytes.fill_(0)

            kinds = {"potential": lambda: launch(potential=pot),
                     "all": lambda: launch(potential=pot, dist2=d2),
                     "grad": lambda: launch(),
                     "fill": lambda: pot.fill_(0),
                     "fill_all": fill_all,
                     "step": lambda: env.step(actions)}

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
            res = env.frame_potential(out=dict(small, potential=pot, dist2=d2), **knobs)
            frame = env.state_m[:, 1]
            fes, pes = frame.element_size(), pot.element_size()
            # the share of cells in reach of an obstacle, on a sample of envs (uint16 has few torch ops: through int32)
            sample = res["dist2"][:min(n, 256)].view(torch.int16).to(torch.int32) & 0xFFFF
            nbytes = {"fill": n * G2 * pes, "fill_all": n * G2 * (pes + 2), "potential": n * G2 * (fes + pes),
                      "all": n * G2 * (fes + pes + 2), "grad": n * G * min(G, 3 + 2 * cells) * fes}
            out_line = {"tag": args.tag, "config": name, "format": fmt, "n_envs": n, "grid": G, "n_obst": env.cfg.n_obst,
                        "knobs": {"occ_min": args.occ_min, "reach": cells},
                        "calls": args.calls, "warmup": args.warmup,
                        "obstacle_cells_share": round(float((sample == 0).float().mean()), 4),
                        "cells_in_reach_share": round(float((sample != 65535).float().mean()), 4),
                        "robots_in_reach_share": round(float((res["robot_d2"] >= 0).float().mean()), 4),
                        "ms_per_call": runs, "ms_median": med, "bytes_moved": nbytes,
                        "hbm_ms": {k: round(b / HBM_SPEC * 1e3, 4) for k, b in nbytes.items()},
                        "over_fill": {"potential": round(med["potential"] / med["fill"], 3), "all": round(med["all"] / med["fill_all"], 3),
                                      "grad": round(med["grad"] / med["fill"], 3)},
                        "potential_over_step": round(med["potential"] / med["step"], 3)}
            env.check_errors()
            line = json.dumps(out_line)
            print(line, flush=True)
            os.makedirs(os.path.dirname(args.out), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")
            env.close()
            del env, kinds, pot, d2, d2_bytes, small, frame, res, sample
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
