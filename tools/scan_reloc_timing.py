#!/usr/bin/env python
"""Cost of relocalisation without a prior (include/ffmp.h ffmp_scan_relocalize) at C3's plane: the whole
plane (Wc = 520, R = 260) and the full circle (T = 90: 181 rotations), on maps the env built.

For each env count (default 1, 16 and 256) a child process of its own resets one C3 FFMPVec and steps it 8 times with
the reactive controller, updating the world map after every step.  Then, per block size B (default 4, 8 and 16), two
warm-up calls and `--launches` calls of every kind, each between two HIP events of its own, the kinds interleaved:
    reloc_B<B>       ffmp_scan_relocalize, the default form: the prior is the plane's centre with yaw 0
    exh_B<B>         the same call with FFMP_RELOC_EXHAUSTIVE (n <= 16 only, `--exh-launches` calls): a cross-check
    match_R16T32     ffmp_scan_match at its own limits on the same buffers, the prior the env's pose: the yardstick
(the library calls the holder makes, without its bookkeeping; pose_out and info are written, the bounds are not).  The
yardstick's time per candidate times (2T+1)(2R+1)^2 is what the exhaustive search of the whole window would cost; each
record gives that extrapolation and how far under it the pruned call comes, with the refined counts (info[7]).
--phases adds, per env count and at B = 8, one more child under `rocprofv3 --kernel-trace --stats` that makes the
default call only: the mean time of each of the six kernels, summed into the three phases (the sliding maximum; the
bounds; select and refine).  Writes one JSON document (--out, default profiles/scan_reloc_timing.json).  The pass is
opt-in and off the step's path: a record, no threshold.

    python tools/scan_reloc_timing.py [--envs 1,16,256] [--blocks 4,8,16] [--launches 12] [--phases] [--out FILE]
"""
import argparse
import csv
import ctypes as C
import glob
import json
import math
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T_FULL = 90
MATCH_R, MATCH_T = 16, 32
PHASES = {"reloc_xmax_kernel": "sliding_max", "reloc_coarse_kernel": "bounds", "reloc_seed_kernel": "select_refine",
          "reloc_compact_kernel": "select_refine", "reloc_refine_kernel": "select_refine", "reloc_final_kernel": "select_refine"}


def one(n, args):
    import torch
    from flow_field_based_motion_planner_amd import _abi
    from flow_field_based_motion_planner_amd.config import beam_dirs, preset, turn_table
    from flow_field_based_motion_planner_amd.vec_env import FFMPVec

    cfg = preset("C3")
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
    dev = env.device
    beams = torch.as_tensor(beam_dirs(L)).to(dev).contiguous()
    W2, rm, Wc = wm.cells * wm.cells, wm.knobs[1], wm.cells
    R, T = Wc // 2, T_FULL
    K = 2 * T + 1
    centre = torch.zeros((n, 4), dtype=torch.float32, device=dev)
    centre[:, 2] = 1.0
    pose_out = torch.empty((n, 4), dtype=torch.float32, device=dev)
    info = torch.zeros((n, 8), dtype=torch.int32, device=dev)
    full = torch.as_tensor(turn_table(T, 2.0 * math.pi / K)).to(dev).contiguous()
    small = torch.as_tensor(turn_table(MATCH_T, env.cfg.res / env.cfg.lidar_range)).to(dev).contiguous()
    blocks = [int(b) for b in args.blocks.split(",")]
    per_env = {B: int(lib.ffmp_scan_relocalize_work(Wc, R, T, B)) for B in blocks}
    work = torch.empty((n * max(per_env.values()),), dtype=torch.uint8, device=dev)

    def reloc(B, flags):
        def body():
            _abi.check(lib.ffmp_scan_relocalize(cfg_c, n, lidar.data_ptr(), lidar.stride(0), L, beams.data_ptr(), centre.data_ptr(), 4, None,
                                                wm.log_odds.data_ptr(), W2, Wc, full.data_ptr(), T, R, B, rm, max(8, L // 6), 0, -2 ** 31,
                                                pose_out.data_ptr(), info.data_ptr(), None, work.data_ptr(), work.numel(), flags,
                                                env._stream()), "ffmp_scan_relocalize")
        return body

    def match():
        _abi.check(lib.ffmp_scan_match(cfg_c, n, lidar.data_ptr(), lidar.stride(0), L, beams.data_ptr(), rec_t.data_ptr(), rec_t.stride(0),
                                       None, wm.log_odds.data_ptr(), W2, Wc, small.data_ptr(), MATCH_T, MATCH_R, rm, max(8, L // 6), 0,
                                       pose_out.data_ptr(), info.data_ptr(), None, 0, env._stream()), "ffmp_scan_match")

    kinds = {f"reloc_B{B}": (reloc(B, 0), args.launches) for B in blocks}
    if args.only_default:
        for body, count in kinds.values():
            for _ in range(args.warmup + count):
                body()
        torch.cuda.synchronize()
        env.close()
        return {"n_envs": n}
    if n <= 16:
        kinds.update({f"exh_B{B}": (reloc(B, _abi.RELOC_EXHAUSTIVE), args.exh_launches) for B in blocks})
    kinds["match_R16T32"] = (match, args.launches)
    refined, status, answers = {}, {}, {}
    for key, (body, _) in kinds.items():
        for _ in range(args.warmup if not key.startswith("exh") else 1):
            body()
        torch.cuda.synchronize()
        if key != "match_R16T32":
            refined[key] = {"min": int(info[:, 7].min()), "median": int(info[:, 7].median()), "max": int(info[:, 7].max())}
            status[key] = round(float((info[:, 0] == 1).float().mean()), 4)
            answers[key] = (pose_out.clone(), info[:, 0:7].clone())
    for B in blocks:  # the cross-check gives the same answer
        if f"exh_B{B}" in answers:
            assert torch.equal(answers[f"exh_B{B}"][0].view(torch.int32), answers[f"reloc_B{B}"][0].view(torch.int32))
            assert torch.equal(answers[f"exh_B{B}"][1], answers[f"reloc_B{B}"][1])
    valid = int(info[:, 6].sum())
    pairs = {key: [] for key in kinds}
    for i in range(args.launches):
        for key, (body, count) in kinds.items():
            if i >= count:
                continue
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            body()
            e1.record()
            pairs[key].append((e0, e1))
    torch.cuda.synchronize()
    ms = {key: sorted(e0.elapsed_time(e1) for e0, e1 in evs) for key, evs in pairs.items()}
    stat = {key: {"median": round(t[len(t) // 2], 4), "min": round(t[0], 4), "max": round(t[-1], 4), "calls": len(t)} for key, t in ms.items()}
    cand_match = (2 * MATCH_T + 1) * (2 * MATCH_R + 1) ** 2
    cand_full = K * (2 * R + 1) ** 2
    extrapolated = stat["match_R16T32"]["median"] / cand_match * cand_full
    rec = {"config": "C3", "n_envs": n, "n_beams": L, "cells": Wc, "radius": R, "n_turns": T, "range_max": rm, "launches": args.launches,
           "warmup": args.warmup, "valid_beams_per_env": round(valid / n, 1), "workspace_bytes_per_env": per_env,
           "blocks_total": {f"B{B}": K * ((2 * R + B) // B) ** 2 for B in blocks}, "refined_blocks": refined, "found_share": status,
           "ms_per_call": stat, "ms_per_env": {k: round(v["median"] / n, 5) for k, v in stat.items()},
           "candidates": {"match_R16T32": cand_match, "whole_window": cand_full},
           "exhaustive_extrapolated_ms": round(extrapolated, 2),
           "times_under_extrapolation": {k: round(extrapolated / v["median"], 1) for k, v in stat.items() if k.startswith("reloc")}}
    env.check_errors()
    env.close()
    return rec


def phases(n, args):
    """The default call at B = 8 under the kernel trace: mean microseconds per kernel and per phase."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "run", "--output-format", "csv", "--", sys.executable,
               os.path.abspath(__file__), "--child", str(n), "--blocks", "8", "--only-default", "--launches", str(args.launches),
               "--warmup", str(args.warmup)]
        done = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if done.returncode:
            sys.exit(f"phases n={n} failed ({done.returncode}):\n{done.stdout[-2000:]}\n{done.stderr[-4000:]}")
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            sys.exit(f"phases n={n}: no kernel_stats.csv under {d}")
        kernels, split = {}, {}
        for row in csv.DictReader(open(files[0])):
            for name, phase in PHASES.items():
                if name in row["Name"]:
                    us = float(row["AverageNs"]) / 1e3
                    kernels[name] = {"calls": int(row["Calls"]), "mean_us": round(us, 2)}
                    split[phase] = round(split.get(phase, 0.0) + us, 2)
        return {"block": 8, "kernels": kernels, "phase_us": split}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", default="1,16,256")
    ap.add_argument("--blocks", default="4,8,16")
    ap.add_argument("--launches", type=int, default=12)
    ap.add_argument("--exh-launches", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--phases", action="store_true", help="add the per-kernel split from a rocprofv3 kernel trace (B = 8)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scan_reloc_timing.json"))
    ap.add_argument("--child", type=int, default=0, help="N — time that env count in this process and print its record")
    ap.add_argument("--only-default", action="store_true", help="child: make the default calls only (the traced run)")
    args = ap.parse_args()
    if args.child:
        print("RECORD " + json.dumps(one(args.child, args)), flush=True)
        return
    records = []
    for n in (int(v) for v in args.envs.split(",")):  # one process per env count: nothing of one run is warm in the next
        cmd = [sys.executable, os.path.abspath(__file__), "--child", str(n), "--blocks", args.blocks, "--launches", str(args.launches),
               "--exh-launches", str(args.exh_launches), "--warmup", str(args.warmup)]
        done = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if done.returncode:  # stop here: nothing more is started after a child that failed
            sys.exit(f"n={n} failed ({done.returncode}):\n{done.stdout[-2000:]}\n{done.stderr[-4000:]}")
        line = [ln for ln in done.stdout.splitlines() if ln.startswith("RECORD ")][-1]
        rec = json.loads(line[7:])
        if args.phases:
            rec["phases"] = phases(n, args)
        print(json.dumps(rec), flush=True)
        records.append(rec)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/scan_reloc_timing.py", "unit": "ms per call, HIP events round each call", "records": records},
                  f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
