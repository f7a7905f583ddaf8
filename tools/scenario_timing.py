#!/usr/bin/env python
"""Cost of putting every env into a caller's episode against resetting every env (SPEC a16b).

For each config (default C3, the preset's env count) one FFMPVec is reset, its episodes are taken
with scenarios() (device float64 tensors: set_scenarios converts nothing), and K back-to-back calls
between two HIP events are timed, after `--warm` untimed calls of the same kind, `--repeats` regions
per kind, interleaved:
    reset()                         the full reset: env kernel (Philox sampler) + both-frames raster
    reset(mask=all)                 the masked reset, the path set_scenarios follows
    set_scenarios(**scenarios)      env kernel (episode read from the arrays) + both-frames raster
and the env-side kernels alone (ffmp_reset / ffmp_set_scenario over all envs, no raster).
`--reset-only` times the reset rows alone (a tree without set_scenarios, e.g. the parent commit).
Prints one JSON line per config.  Injection is not on the hot path: a record, no threshold.

    python tools/scenario_timing.py [--configs C3] [--calls 50] [--repeats 3] [--reset-only]
"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C3")
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warm", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3, help="timed regions per kind, interleaved; all are reported")
    ap.add_argument("--envs", type=int, default=0, help="override the preset's env count")
    ap.add_argument("--reset-only", action="store_true")
    ap.add_argument("--no-autotune", action="store_true")
    args = ap.parse_args()
    import torch
    from flow_field_based_motion_planner_amd import _abi
    from flow_field_based_motion_planner_amd.config import PRESETS, preset
    from flow_field_based_motion_planner_amd.vec_env import FFMPVec

    for name in args.configs.split(","):
        n = args.envs or PRESETS[name]["n_envs"]
        env = FFMPVec(n, preset(name), device="cuda:0", autotune=not args.no_autotune)
        env.reset()
        every = torch.ones(n, dtype=torch.bool, device=env.device)
        lib, cfg_c, st, ob = env.lib, C.byref(env._cfg_c), C.byref(env._state_c), C.byref(env._obs_c)

        def reset_kernel():
            _abi.check(lib.ffmp_reset(cfg_c, n, env.env_offset, None, 0, st, ob, env._stream()), "ffmp_reset")

        kinds = {"reset": lambda: env.reset(), "reset_masked_all": lambda: env.reset(mask=every),
                 "reset_kernel": reset_kernel}
        if not args.reset_only:
            sc = env.scenarios()

            def scenario_kernel():
                _abi.check(lib.ffmp_set_scenario(cfg_c, n, env.env_offset, None, sc["pose"].data_ptr(),
                                                 sc["goal"].data_ptr(), sc["obst"].data_ptr(), sc["obst_r"].data_ptr(),
                                                 sc["episode"].data_ptr(), st, ob, env._stream()), "ffmp_set_scenario")

            kinds["set_scenarios"] = lambda: env.set_scenarios(**sc)
            kinds["set_scenario_kernel"] = scenario_kernel

        def timed(body, k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(k):
                body()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) * 1e3 / k  # us per call

        runs = {key: [] for key in kinds}
        for _ in range(args.repeats):
            for key, body in kinds.items():
                timed(body, args.warm)
                runs[key].append(round(timed(body, args.calls), 2))
        out = {"config": name, "n_envs": n, "calls": args.calls, "warm": args.warm, "fused": env.fused,
               "ring": env.ring, "frame_window": env.frame_window, "us_per_call": runs}
        med = {key: sorted(ts)[len(ts) // 2] for key, ts in runs.items()}
        if not args.reset_only:
            out["set_scenarios_over_masked_reset"] = round(med["set_scenarios"] / med["reset_masked_all"], 4)
            out["scenario_kernel_over_reset_kernel"] = round(med["set_scenario_kernel"] / med["reset_kernel"], 4)
        env.check_errors()
        print(json.dumps(out), flush=True)
        env.close()
        del env, kinds


if __name__ == "__main__":
    main()
