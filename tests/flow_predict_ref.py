"""Predicted-occupancy frames (include/ffmp.h ffmp_flow_predict) restated in NumPy — the
checker of tests/test_flow_predict_host.py and tests/test_gpu_flow_predict.py, and, run as a script, the
closed-loop table of DESIGN §10.8.  Nothing here is shared with the kernel.

    python tests/flow_predict_ref.py                   the crossing family: plain, predicted, gate off
    python tests/flow_predict_ref.py --write-golden    and record the first two in tests/golden/flow_predict_crossing.json
"""
from __future__ import annotations

import os

import numpy as np

F32 = np.float32
DEFAULTS = dict(steps=24, slack=3, swept=254, other=128)


def arrival(G: int, pace: int) -> np.ndarray:
    """ka (G, G) int64: the earliest prediction step at which the robot can stand on a cell — the chamfer
    5-7 distance from the robot cell (G/2, G/2), `pace` units per step, integer division."""
    c = G // 2
    a = np.abs(np.arange(G) - c)
    m = np.maximum(a[:, None], a[None, :])
    n = np.minimum(a[:, None], a[None, :])
    return (5 * m + 2 * n) // int(pace)


def host_knobs(dt: float, res: float, speed: float = 0.6):
    """(cps, pace) as FFMPVec.predicted_frames derives them: cps = float32(dt / res),
    pace = max(1, rint(5 * speed * dt / res))."""
    return F32(dt / res), max(1, int(np.rint(5.0 * speed * dt / res)))


def flow_predict_one(frame, vx, vy, steps, cps, pace, slack, swept=254, other=128):
    """One env: frame (G, G) float32 or uint8, vx / vy (G, G) float32 or float16 -> (out (G, G) uint8, n_swept)."""
    frame = np.asarray(frame)
    G = frame.shape[0]
    with np.errstate(invalid="ignore"):
        occ = frame > 0          # a NaN compares false
        src = frame == 255
    cps = F32(cps)
    vx = np.asarray(vx).astype(F32)  # binary16 is converted to float32 first
    vy = np.asarray(vy).astype(F32)
    bit = np.zeros((G, G), dtype=bool)
    ii, jj = np.nonzero(src)
    if ii.size:
        with np.errstate(all="ignore"):
            su = vx[ii, jj] * cps    # one float32 multiply each
            sv = vy[ii, jj] * cps
        ok = np.isfinite(su) & np.isfinite(sv) & ~((su == 0) & (sv == 0))
        ii, jj, su, sv = ii[ok], jj[ok], su[ok], sv[ok]
        ka = arrival(G, pace)
        for k in range(1, int(steps) + 1):
            with np.errstate(all="ignore"):
                ru = np.rint(F32(k) * su)  # float32 product, half to even
                rv = np.rint(F32(k) * sv)
            # |r| >= G (an overflow to inf included) leaves the grid from any row: no integer is formed for it
            near = (np.abs(ru) < G) & (np.abs(rv) < G)
            ti = ii[near] + ru[near].astype(np.int64)
            tj = jj[near] + rv[near].astype(np.int64)
            inside = (ti >= 0) & (ti < G) & (tj >= 0) & (tj < G)
            ti, tj = ti[inside], tj[inside]
            if slack >= 0:
                gate = np.abs(k - ka[ti, tj]) <= slack
                ti, tj = ti[gate], tj[gate]
            bit[ti, tj] = True
    out = np.where(src, 255, np.where(occ, int(other), np.where(bit, int(swept), 0))).astype(np.uint8)
    return out, int((bit & ~occ).sum())


def flow_predict(frames, flow, steps=24, cps=F32(2.0), pace=6, slack=3, swept=254, other=128, mask=None, out_in=None,
                 n_swept_in=None):
    """Batch form: frames (N, G, G), flow (N, 2, G, G) [vx, vy] -> (out (N, G, G) uint8, n_swept (N,) int32).
    mask: envs with 0 keep their cells of out_in and their n_swept_in."""
    frames = np.asarray(frames)
    flow = np.asarray(flow)
    n, G = frames.shape[0], frames.shape[-1]
    out = np.zeros((n, G, G), np.uint8) if out_in is None else np.array(out_in, dtype=np.uint8)
    cnt = np.zeros(n, np.int32) if n_swept_in is None else np.array(n_swept_in, dtype=np.int32)
    for e in range(n):
        if mask is not None and not mask[e]:
            continue
        out[e], cnt[e] = flow_predict_one(frames[e], flow[e, 0], flow[e, 1], steps, cps, pace, slack, swept, other)
    return out, cnt


# ------------------------------------------------------------------ the crossing family
CROSS_CFG = dict(grid=64, n_obst=2, n_beams=0, moving=True, flow=True, obst_vmax=1.0, world_half=2.0, max_steps=120,
                 autoreset=False)
CROSS_V = (0.2, 0.3, 0.4, 0.5)
CROSS_Y0 = (-0.3, -0.5, -0.7, -0.9, -1.1, -1.3)
CROSS_STEPS = 120
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "flow_predict_crossing.json")


def crossing_scenes():
    """24 scenes: robot (-1, 0, yaw 0), goal (1, 0); disc 0 of r = 0.25 at (0, y0) moving at (0, v); disc 1
    parked with r = 0."""
    cases = [(v, y0) for v in CROSS_V for y0 in CROSS_Y0]
    n = len(cases)
    obst = np.zeros((n, 2, 4))
    obst_r = np.zeros((n, 2))
    for e, (v, y0) in enumerate(cases):
        obst[e, 0] = (0.0, y0, 0.0, v)
        obst[e, 1] = (1.7, 1.7, 0.0, 0.0)
    obst_r[:, 0] = 0.25
    return dict(pose=np.tile([-1.0, 0.0, 0.0], (n, 1)), goal=np.tile([1.0, 0.0], (n, 1)), obst=obst, obst_r=obst_r)


_LOOPS = {}


def crossing_closed_loop(predict=None, steps=CROSS_STEPS):
    """The untouched NumPy oracle on the crossing family, driven by tests/nav_field_ref.py's planner and
    follower: (outcome (24,), step it happened at (24,)), codes 0 none, 1 goal, 2 collision, 3 truncated.
    predict: None plans over the newest frame; a dict of flow_predict's knobs (steps, slack, ...) plans over
    the predicted plane of the newest frame and the ground-truth flow.  Computed once per setting."""
    key = (None if predict is None else tuple(sorted(predict.items())), steps)
    if key in _LOOPS:
        return _LOOPS[key]
    import pytest
    from flow_field_based_motion_planner_amd.config import FFMPConfig
    from oracle import ffmp_oracle
    from tests import nav_field_ref as NR
    from tests.test_gpu_scenarios import _oracle_inject
    cfg = FFMPConfig(**CROSS_CFG)
    sc = crossing_scenes()
    n = len(sc["pose"])
    cps, pace = host_knobs(cfg.dt, cfg.res)
    mp = pytest.MonkeyPatch()
    try:
        ref = ffmp_oracle.OracleVecEnv(cfg, n)
        cv, cw = NR._PerEnv(), NR._PerEnv()
        mp.setattr(ffmp_oracle, "CMD_V", cv)
        mp.setattr(ffmp_oracle, "CMD_W", cw)
        ref.reset()
        _oracle_inject(ref, sc, 1)
        flags = []
        zeros = np.zeros(n, dtype=np.int64)
        for _ in range(steps):
            plane = ref.state_m[:, 1]
            if predict is not None:
                plane = flow_predict(plane, ref.flow, cps=cps, pace=pace, **dict(DEFAULTS, **predict))[0]
            c = NR.nav_field(plane, ref.record[:, 8:10], cfg)["cmd"]
            cv.value, cw.value = NR._clip(c)
            ref.step(zeros)
            flags.append((ref.is_goal.copy(), ref.collision.copy(), ref.truncated.copy()))
            if (NR._outcomes(flags)[0] != 0).all():
                break
    finally:
        mp.undo()
    _LOOPS[key] = NR._outcomes(flags)
    return _LOOPS[key]


def summary(outcome, when):
    """(collisions, goals, neither, mean steps per reached goal)."""
    goal = outcome == 1
    return int((outcome == 2).sum()), int(goal.sum()), int(((outcome != 1) & (outcome != 2)).sum()), \
        float(when[goal].mean()) if goal.any() else float("nan")


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if "--write-golden" in sys.argv:  # the record tests/test_gpu_flow_predict.py compares the GPU's closed loop with
        import json
        gold = {}
        for name, predict in (("plain", None), ("predicted", dict(steps=24, slack=3))):
            o, t = crossing_closed_loop(predict)
            gold[name] = {"outcome": o.tolist(), "step": t.tolist()}
        with open(GOLDEN, "w") as f:
            json.dump(gold, f)
            f.write("\n")
    for name, predict in (("plain policy_nav", None), ("predicted, steps 24, slack 3", dict(steps=24, slack=3)),
                          ("predicted, gate off (slack -1)", dict(steps=24, slack=-1))):
        o, t = crossing_closed_loop(predict)
        col, goal, neither, mean = summary(o, t)
        print(f"{name}: collisions {col} of {len(o)}, goals {goal}, neither {neither}, steps per reached goal {mean:.1f}")
        print("   outcomes", "".join(str(x) for x in o.tolist()), "at", t.tolist())
