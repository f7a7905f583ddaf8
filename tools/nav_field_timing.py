#!/usr/bin/env python
"""Cost of the navigation field (include/ffmp.h ffmp_nav_field) beside the env step.

For each config (default C2: 4,096 x 128^2 with 8 static discs, and C3: 256^2 with 16 discs, the
preset's env counts unless --envs) one FFMPVec is reset and stepped a few times with the reactive
controller (so the frames are ordinary mid-episode frames), then K back-to-back calls between two
HIP events are timed, after `--warm` untimed calls of the same kind, `--repeats` regions per kind,
interleaved:
    step            step(actions) — the env step the field is quoted against
    nav_cmd         ffmp_nav_field writing cmd only (policy_nav into a preallocated tensor)
    nav_planes      ffmp_nav_field writing the cost and dir planes (+ target, geo_cost)
With --tile T (0 = the library's default tile), and always on a grid above 256 x 256, the tiled kernel
(ffmp_nav_field_tiled: the plane in HBM, tiles through LDS) is timed as well, on the same frames:
    nav_cmd_tiled, nav_planes_tiled
so that at C3 with --tile 256 (one tile per env) the two kernels stand side by side: the difference
is the cost of going through HBM.  "C5share" is C5's share of one GPU, 16,384 x 512^2.
Appends one JSON line per config to profiles/nav_field_timing.jsonl (--out; by default
profiles/nav_field_tiled_timing.jsonl when a tiled kind is timed) and prints it.  The field is opt-in
and off the hot path: a record, no threshold.

    python tools/nav_field_timing.py [--configs C2,C3] [--calls 5] [--repeats 3] [--envs N]
    python tools/nav_field_timing.py --configs C5share,C3 --tile 256
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C2,C3")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3, help="timed regions per kind, interleaved; all are reported")
    ap.add_argument("--envs", type=int, default=0, help="override the preset's env count")
    ap.add_argument("--tile", type=int, default=None, help="also time the tiled kernel with this tile (0 = its default)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from flow_field_based_motion_planner_amd.config import PRESETS, preset
    from flow_field_based_motion_planner_amd.vec_env import FFMPVec

    shares = {"C5share": ("C5", 16384)}  # a multi-GPU preset's share of one GPU
    for name in args.configs.split(","):
        base, share = shares.get(name, (name, 0))
        n = args.envs or share or PRESETS[base]["n_envs"]
        env = FFMPVec(n, preset(base), device="cuda:0", autotune=False)
        G = env.cfg.grid
        tile = args.tile if args.tile is not None else (0 if G > 256 else None)
        out_path = args.out or os.path.join(ROOT, "profiles", "nav_field_timing.jsonl" if tile is None
                                            else "nav_field_tiled_timing.jsonl")
        env.reset()
        for _ in range(8):
            env.step(env.policy_reactive())
        actions = env.policy_reactive().clone()
        kn = dict(FFMPVec.NAV_DEFAULTS)
        cmd = torch.empty((n, 2), dtype=torch.float64, device=env.device)
        cost = torch.empty((n, G, G), dtype=torch.uint16, device=env.device)
        dirs = torch.empty((n, G, G), dtype=torch.uint8, device=env.device)
        target = torch.empty((n, 2), dtype=torch.int32, device=env.device)
        geo = torch.empty(n, dtype=torch.int32, device=env.device)
        kinds = {"step": lambda: env.step(actions)}
        if G <= 256:
            kinds["nav_cmd"] = lambda: env._nav_launch("nav_field", **kn, cmd=cmd)
            kinds["nav_planes"] = lambda: env._nav_launch("nav_field", **kn, cost=cost, direction=dirs, target=target,
                                                          geo_cost=geo)
        if tile is not None:
            kinds["nav_cmd_tiled"] = lambda: env._nav_launch("nav_field", **kn, cmd=cmd, tile=tile)
            kinds["nav_planes_tiled"] = lambda: env._nav_launch("nav_field", **kn, cost=cost, direction=dirs, target=target,
                                                                geo_cost=geo, tile=tile)

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
        reach = int((geo >= 0).sum())
        out = {"config": name, "n_envs": n, "grid": G, "n_obst": env.cfg.n_obst, "calls": args.calls, "warm": args.warm,
               "knobs": kn, "reachable_envs": reach, "ms_per_call": runs}
        for key in kinds:
            if key != "step":
                out[key + "_over_step"] = round(med[key] / med["step"], 2)
        if tile is not None:
            out["tile"] = tile
            out["workspace_bytes"] = env.nav_workspace_bytes()
            if "nav_cmd" in kinds:
                out["tiled_over_untiled"] = {"cmd": round(med["nav_cmd_tiled"] / med["nav_cmd"], 3),
                                             "planes": round(med["nav_planes_tiled"] / med["nav_planes"], 3)}
        env.check_errors()
        line = json.dumps(out)
        print(line, flush=True)
        os.makedirs(os.path.dirname(out_path), exist_ok=True)
        with open(out_path, "a") as f:
            f.write(line + "\n")
        env.close()
        del env, kinds, cost, dirs


if __name__ == "__main__":
    main()
