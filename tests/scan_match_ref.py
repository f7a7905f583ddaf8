"""Scan-to-map matching (include/ffmp.h ffmp_scan_match) restated in NumPy, operation for
operation — the checker of tests/test_gpu_scan_match.py.

Every float array is float32 and every line is one float32 operation per element (NumPy never fuses
a*b + c), in the SPEC's order; np.rint rounds half to even as rintf does; comparisons are NumPy's, so a NaN
is off the plane.  The scores are int32 sums, so the order of the beams does not show.  match() gathers all
(2R + 1)^2 shifts of one rotation at once from a plane padded with zeros; match_loops() is the SPEC read
literally, three Python loops, for tiny sizes.  The winner is picked by a lexicographic sort of the SPEC's
tie order, not by the kernel's packed key.

localize_step() restates the WorldMap.localizer holder's step (float64 composition of the map <- odom
transform, match, the transform recomputed, the map updated at the matched pose).

`python tests/scan_match_ref.py` prints the drift table and the single-shot recovery figures of DESIGN §10.12."""
import math
import os
import sys

import numpy as np

if __name__ == "__main__":  # run as a script: the repository root is not on the path yet
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from flow_field_based_motion_planner_amd.config import FFMPConfig, beam_table
from oracle.ffmp_oracle import Cfg
from tests import world_map_ref as W

F32 = np.float32
FLT_MAX = np.finfo(np.float32).max


def beam_dirs(L: int) -> np.ndarray:
    """(L, 2) float32: the rounding of config.beam_table(L)."""
    return beam_table(L).astype(F32)


def turn_table(T: int, dtheta: float) -> np.ndarray:
    """(2T + 1, 2) float32 {cos, sin} of (k - T) dtheta, float64 then rounded; entry T is exactly (1, 0)."""
    out = np.zeros((2 * T + 1, 2), F32)
    for k in range(2 * T + 1):
        out[k] = (math.cos((k - T) * dtheta), math.sin((k - T) * dtheta))
    return out


def _cells(cfg: Cfg, Wc: int, ranges, pose, beams, turns, R: int, range_max):
    """valid (n, L) bool; fp, fq (n, K, L) float32; on (n, K, L) bool; ck, sk (n, K) float32."""
    n, L = ranges.shape
    res, wh = F32(cfg.f["res_f"]), W.half_of(cfg, Wc)
    px, py, c, s = (pose[:, k].reshape(n, 1) for k in range(4))
    with np.errstate(all="ignore"):
        r = ranges
        valid = (r > F32(0.0)) & (r <= F32(range_max)) & (r <= FLT_MAX)
        bx = r * beams[:, 0].reshape(1, L)
        by = r * beams[:, 1].reshape(1, L)
        rc, rs = turns[:, 0].reshape(1, -1), turns[:, 1].reshape(1, -1)
        p0 = c * rc
        p1 = s * rs
        ck = p0 - p1  # (n, K)
        q0 = s * rc
        q1 = c * rs
        sk = q0 + q1
        ckb, skb = ck[:, :, None], sk[:, :, None]
        bxb, byb = bx[:, None, :], by[:, None, :]
        t0 = ckb * bxb
        t1 = skb * byb
        wx = t0 - t1
        wx = wx + px[:, :, None]
        u0 = skb * bxb
        u1 = ckb * byb
        wy = u0 + u1
        wy = wy + py[:, :, None]
        fp = wx + wh
        fp = fp / res
        fp = np.rint(fp)
        fq = wy + wh
        fq = fq / res
        fq = np.rint(fq)
        lo, hi = F32(-R), F32(Wc - 1 + R)
        on = valid[:, None, :] & (fp >= lo) & (fp <= hi) & (fq >= lo) & (fq <= hi)
    assert fp.dtype == F32 and fq.dtype == F32 and ck.dtype == F32
    finite = np.isfinite(pose).all(axis=1)
    on = on & finite.reshape(n, 1, 1)
    return valid, fp, fq, on, ck, sk


def _finish(cfg: Cfg, pose, vol, valid, ck, sk, R: int, T: int, min_valid: int, min_gain: int):
    n = pose.shape[0]
    res = F32(cfg.f["res_f"])
    A = 2 * R + 1
    kk, aa, bb = np.meshgrid(np.arange(-T, T + 1), np.arange(-R, R + 1), np.arange(-R, R + 1), indexing="ij")
    kk, aa, bb = kk.ravel(), aa.ravel(), bb.ravel()
    finite = np.isfinite(pose).all(axis=1)
    nvalid = valid.sum(axis=1).astype(np.int32)
    pose_out = pose.copy()
    info = np.zeros((n, 8), np.int32)
    for e in range(n):
        S = vol[e].ravel().astype(np.int64)
        w = np.lexsort((bb, aa, kk, np.abs(kk), aa * aa + bb * bb, -S))[0]
        k, a, b = int(kk[w]), int(aa[w]), int(bb[w])
        best, zero = int(S[w]), int(vol[e, T, R, R])
        ok = bool(finite[e]) and nvalid[e] >= min_valid and best - zero >= min_gain and (k, a, b) != (0, 0, 0)
        if not finite[e]:
            best = zero = 0
        info[e] = (1, k, a, b, best, zero, nvalid[e], 0) if ok else (0, 0, 0, 0, best, zero, nvalid[e], 0)
        if ok:
            da = F32(a) * res
            db = F32(b) * res
            pose_out[e] = (pose[e, 0] + da, pose[e, 1] + db, ck[e, k + T], sk[e, k + T])
    assert pose_out.dtype == F32
    return pose_out, info


def _prep(m, ranges, pose, R, T, dtheta, beams, turns):
    m = np.asarray(m, np.int8)
    ranges = np.asarray(ranges, F32)
    n, L = ranges.shape
    pose = np.ascontiguousarray(np.asarray(pose, F32).reshape(n, -1)[:, 0:4])
    beams = beam_dirs(L) if beams is None else np.asarray(beams, F32)
    turns = turn_table(T, dtheta) if turns is None else np.asarray(turns, F32)
    assert turns.shape == (2 * T + 1, 2) and beams.shape == (L, 2) and 0 <= R <= 16 and 0 <= T <= 32
    return m, ranges, pose, beams, turns


def match(cfg: Cfg, m, ranges, pose, R: int, T: int, dtheta: float = 0.0, range_max=np.inf, min_valid: int = 0,
          min_gain: int = 0, beams=None, turns=None):
    """One ffmp_scan_match call on the planes m (n, Wc, Wc) int8: (pose_out (n, 4) float32, info (n, 8) int32,
    volume (n, 2T+1, 2R+1, 2R+1) int32)."""
    m, ranges, pose, beams, turns = _prep(m, ranges, pose, R, T, dtheta, beams, turns)
    n, Wc, _ = m.shape
    valid, fp, fq, on, ck, sk = _cells(cfg, Wc, ranges, pose, beams, turns, R, range_max)
    A, K = 2 * R + 1, 2 * T + 1
    pad = 2 * R  # fp in -R .. Wc-1+R and a in -R .. R: fp + a in -2R .. Wc-1+2R
    mp = np.zeros((n, Wc + 2 * pad, Wc + 2 * pad), np.int8)
    mp[:, pad:pad + Wc, pad:pad + Wc] = m
    gp = np.where(on, fp, F32(0.0)).astype(np.int64) + pad  # converted only where on holds
    gq = np.where(on, fq, F32(0.0)).astype(np.int64) + pad
    sh = np.arange(-R, R + 1)
    e = np.arange(n).reshape(n, 1, 1, 1)
    vol = np.zeros((n, K, A, A), np.int32)
    for k in range(K):
        p = gp[:, k, :, None, None] + sh.reshape(1, 1, A, 1)
        q = gq[:, k, :, None, None] + sh.reshape(1, 1, 1, A)
        got = mp[e, p, q].astype(np.int32) * on[:, k, :, None, None]
        vol[:, k] = got.sum(axis=1, dtype=np.int32)
    pose_out, info = _finish(cfg, pose, vol, valid, ck, sk, R, T, min_valid, min_gain)
    return pose_out, info, vol


def match_loops(cfg: Cfg, m, ranges, pose, R: int, T: int, dtheta: float = 0.0, range_max=np.inf, min_valid: int = 0,
                min_gain: int = 0, beams=None, turns=None):
    """match() as the SPEC reads: a loop per rotation, shift and beam.  Tiny sizes only."""
    m, ranges, pose, beams, turns = _prep(m, ranges, pose, R, T, dtheta, beams, turns)
    n, Wc, _ = m.shape
    valid, fp, fq, on, ck, sk = _cells(cfg, Wc, ranges, pose, beams, turns, R, range_max)
    L = ranges.shape[1]
    vol = np.zeros((n, 2 * T + 1, 2 * R + 1, 2 * R + 1), np.int32)
    for e in range(n):
        for k in range(2 * T + 1):
            for l in range(L):
                if not on[e, k, l]:
                    continue
                p, q = int(fp[e, k, l]), int(fq[e, k, l])
                for a in range(-R, R + 1):
                    for b in range(-R, R + 1):
                        if 0 <= p + a <= Wc - 1 and 0 <= q + b <= Wc - 1:
                            vol[e, k, a + R, b + R] += int(m[e, p + a, q + b])
    pose_out, info = _finish(cfg, pose, vol, valid, ck, sk, R, T, min_valid, min_gain)
    return pose_out, info, vol


# ---------------------------------------------------------------- the localizer holder, restated
def compose(tf: np.ndarray, odom: np.ndarray) -> np.ndarray:
    """The prior T o odom: tf (n, 3) float64 {tx, ty, theta}, odom (n, 4) float32 words -> (n, 4) float32."""
    o = np.asarray(odom, F32).astype(np.float64)
    ct, st = np.cos(tf[:, 2]), np.sin(tf[:, 2])
    x = ct * o[:, 0] - st * o[:, 1] + tf[:, 0]
    y = st * o[:, 0] + ct * o[:, 1] + tf[:, 1]
    c = ct * o[:, 2] - st * o[:, 3]
    s = st * o[:, 2] + ct * o[:, 3]
    return np.stack([x, y, c, s], axis=1).astype(F32)


def transform_of(matched: np.ndarray, odom: np.ndarray) -> np.ndarray:
    """The map <- odom transform (n, 3) float64 that takes the odometry pose to the matched pose."""
    mt = np.asarray(matched, F32).astype(np.float64)
    o = np.asarray(odom, F32).astype(np.float64)
    th = np.arctan2(mt[:, 3], mt[:, 2]) - np.arctan2(o[:, 3], o[:, 2])
    th = np.arctan2(np.sin(th), np.cos(th))
    ct, st = np.cos(th), np.sin(th)
    tx = mt[:, 0] - (ct * o[:, 0] - st * o[:, 1])
    ty = mt[:, 1] - (st * o[:, 0] + ct * o[:, 1])
    return np.stack([tx, ty, th], axis=1)


def localize_step(config: FFMPConfig, m, tf, odom, ranges, first, R: int = 2, T: int = 2, dtheta=None, min_valid=None,
                  min_gain: int = 0, range_max=None, update: bool = True):
    """One step of the holder: (matched pose (n, 4) float32, the new transform (n, 3), the new planes, info).
    Envs flagged first get T = 0 and are not matched (their map is empty)."""
    cfg = Cfg.from_config(config)
    ranges = np.asarray(ranges, F32)
    n, L = ranges.shape
    first = np.asarray(first).reshape(n) != 0
    dtheta = config.res / config.lidar_range if dtheta is None else dtheta
    min_valid = max(8, L // 6) if min_valid is None else min_valid
    range_max = config.lidar_range if range_max is None else range_max
    tf = np.where(first.reshape(n, 1), 0.0, np.asarray(tf, np.float64))
    prior = compose(tf, odom)
    matched, info, _ = match(cfg, m, ranges, prior, R, T, dtheta, range_max, min_valid, min_gain)
    matched[first] = prior[first]
    info[first] = 0
    tf = np.where(first.reshape(n, 1), 0.0, transform_of(matched, odom))
    if update:
        m = W.from_config(config, m, ranges, matched, first=first, range_max=range_max)
    return matched, tf, m, info


# ---------------------------------------------------------------- the physical tie
def tie_config(**kw) -> FFMPConfig:
    from tests.lidar_map_ref import LONG
    return FFMPConfig(**dict(LONG[64], lidar_max=4.0, **kw))


def drift_of(pose: np.ndarray, k: int, step=0.005, turn=0.008) -> np.ndarray:
    """The true pose (n, 4) seen through an odometry frame that has drifted for k steps: turned by k turn about
    the world's origin and moved by k step along x."""
    tf = np.tile(np.array([[k * step, 0.0, k * turn]]), (pose.shape[0], 1))
    return compose(tf, pose)


def pose_errors(est: np.ndarray, true: np.ndarray):
    e, t = est.astype(np.float64), true.astype(np.float64)
    d = np.hypot(e[:, 0] - t[:, 0], e[:, 1] - t[:, 1])
    yaw = np.arctan2(e[:, 3], e[:, 2]) - np.arctan2(t[:, 3], t[:, 2])
    return d, np.abs(np.arctan2(np.sin(yaw), np.cos(yaw)))


def drift_run(seed: int = 1, n: int = 24, steps: int = 40, matching: bool = True, R: int = 2, T: int = 2, dtheta=0.0125,
              config=None, step_fn=None):
    """The drift run: (position error (kept,), yaw error (kept,), contradiction share of the ego view, kept count).
    step_fn(k, odom, ranges, first) -> matched pose replaces the restated holder (the GPU test's hook)."""
    from oracle.ffmp_oracle import OracleVecEnv
    config = tie_config() if config is None else config
    cfg = Cfg.from_config(config)
    Wc = W.default_cells(config) + 24
    env = OracleVecEnv(config, n, with_potential=False)
    env.reset()
    rng = np.random.default_rng(seed)
    m = np.zeros((n, Wc, Wc), np.int8)
    tf = np.zeros((n, 3))
    alive = np.ones(n, bool)
    episode = env.episode.copy()
    est = None
    for k in range(steps + 1):
        if k:
            env.step(rng.integers(7, 28, n))
            alive &= (env.episode == episode) & (env.record[:, 10] == 0)
        true = env.record[:, 0:4].astype(F32)
        odom = drift_of(true, k)
        first = np.full(n, k == 0)
        if step_fn is not None:
            est = step_fn(k, odom, env.lidar, first)
        elif matching:
            est, tf, m, _ = localize_step(config, m, tf, odom, env.lidar, first, R, T, dtheta)
        else:
            est = odom
            m = W.from_config(config, m, env.lidar, odom, first=first)
    d, yaw = pose_errors(est, true)
    bad = None
    if step_fn is None:
        frame = W.ego_frame(cfg, m, est, outside=128)
        bad, _ = W.quality(frame[alive], env.state_m[alive, 1])
    return d[alive], yaw[alive], bad, int(alive.sum())


def single_shot(seed: int, n: int = 32, steps: int = 30, R: int = 4, T: int = 4, dtheta=0.0125, config=None):
    """Single-shot recovery: (kept, per-env |recovered - displaced| in (a, b, k) (kept, 3), valid beams (kept,))."""
    from oracle.ffmp_oracle import OracleVecEnv
    config = tie_config() if config is None else config
    cfg = Cfg.from_config(config)
    Wc = W.default_cells(config) + 24
    env = OracleVecEnv(config, n, with_potential=False)
    env.reset()
    rng = np.random.default_rng(seed)
    m = np.zeros((n, Wc, Wc), np.int8)
    alive = np.ones(n, bool)
    episode = env.episode.copy()
    for k in range(steps + 1):
        if k:
            env.step(rng.integers(0, 28, n))
            alive &= (env.episode == episode) & (env.record[:, 10] == 0)
        if k < steps:
            m = W.from_config(config, m, env.lidar, env.record[:, 0:4], first=np.full(n, k == 0))
    true = env.record[:, 0:4].astype(F32)
    a, b = rng.integers(-(R - 1), R, n), rng.integers(-(R - 1), R, n)
    kk = rng.integers(-(T - 1), T, n)
    res = float(config.res)
    yaw = np.arctan2(true[:, 3].astype(np.float64), true[:, 2].astype(np.float64)) + kk * dtheta
    moved = np.stack([true[:, 0] + a * res, true[:, 1] + b * res, np.cos(yaw), np.sin(yaw)], axis=1).astype(F32)
    _, info, _ = match(cfg, m, env.lidar, moved, R, T, dtheta, config.lidar_range, max(8, env.lidar.shape[1] // 6), 0)
    miss = np.abs(np.stack([info[:, 2] + a, info[:, 3] + b, info[:, 1] + kk], axis=1))
    return int(alive.sum()), miss[alive], info[alive, 6]


if __name__ == "__main__":
    for moving in (False, True):
        kw = dict(moving=True, obst_vmax=0.5) if moving else {}
        print("moving discs (obst_vmax 0.5)" if moving else "static discs", flush=True)
        for seed in (1, 2, 3):
            kept, miss, nv = single_shot(seed, config=tie_config(**kw))
            within = (miss <= 1).all(axis=1)
            exact = (miss == 0).all(axis=1)
            print(f"  single shot seed {seed}: kept {kept}/32, within one cell and step {within.sum()}/{kept}, exact "
                  f"{100 * exact.mean():.0f} %, valid beams >= {nv.min()}", flush=True)
        if moving:
            break
        for seed in (1, 2):
            for matching in (False, True):
                d, yaw, bad, kept = drift_run(seed, matching=matching)
                name = "matched before every update" if matching else "map updated at the odometry pose"
                print(f"  drift seed {seed}, {name}: kept {kept}/24, position error median {np.median(d):.3f} max {d.max():.3f} m, "
                      f"yaw error max {yaw.max():.4f} rad, known cells contradicting truth {100 * bad:.1f} %", flush=True)
