"""The world-fixed scan map and its ego view (include/ffmp.h ffmp_world_map / ffmp_world_frame, DESIGN §3
a19e) restated in NumPy, operation for operation — the checker of tests/test_gpu_world_map.py.

Every float array is float32 and every line is one float32 operation per element (NumPy never fuses
a*b + c), in the SPEC's order.  The classification is tests/scan_map_ref.py's bisection and known / free /
occ tests, restated here over per-env (ex, ey) arrays instead of the grid's cell coordinates; the restatement
visits every cell of the plane, not a box (a cell the scan does not reach keeps its value either way).
np.rint rounds half to even as rintf does; comparisons are NumPy's, so a NaN is outside.

`python tests/world_map_ref.py` prints the map-quality figures of DESIGN §10.11: a static preset at G = 64,
200 steps of the oracle under policy_nav's restated follower, the world map's ego view against the
re-sampled map of tests/lidar_map_ref.py."""
import os
import sys

import numpy as np

if __name__ == "__main__":  # run as a script: the repository root is not on the path yet
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from flow_field_based_motion_planner_amd.config import FFMPConfig, sector_table
from oracle.ffmp_oracle import Cfg, cell_coords

F32 = np.float32
KNOBS = dict(l_hit=8, l_free=4, l_max=64, decay=0)


def default_cells(config: FFMPConfig) -> int:
    """FFMPVec.world_map's default: the arena plus four cells a side, rounded up to a multiple of 4."""
    return 4 * int(np.ceil((2.0 * config.W / config.res + 8.0) / 4.0))


def half_of(cfg: Cfg, cells: int) -> np.float32:
    """wh_f: Wc * res / 2 in float64, rounded."""
    return F32(float(cells) * float(cfg.res) / 2.0)


def origin_of(cfg: Cfg, cells: int) -> float:
    """World coordinate of cell 0's centre (both axes)."""
    return -float(half_of(cfg, cells))


def classes(ex: np.ndarray, ey: np.ndarray, ranges: np.ndarray, u: np.ndarray, th, range_max):
    """(known, free, occ) bool arrays of ex's shape (n, ...): ffmp_scan_frames' classification at the points
    (ex, ey) float32 of env e under the row ranges[e] (n, L) and the sector table u (L, 2)."""
    ex, ey = np.asarray(ex, F32), np.asarray(ey, F32)
    ranges = np.asarray(ranges, F32)
    u = np.asarray(u, F32)
    n, L = ranges.shape
    H = (L + 1) // 2
    with np.errstate(all="ignore"):
        p0 = u[0, 0] * ey
        p1 = u[0, 1] * ex
        c0 = p0 - p1
        first = c0 >= F32(0.0)
        lo = np.where(first, 0, H - 1)
        hi = np.where(first, H, L)
        while True:
            act = hi - lo > 1
            if not act.any():
                break
            mid = np.where(act, (lo + hi) >> 1, 0)
            p0 = u[mid, 0] * ey
            p1 = u[mid, 1] * ex
            t = p0 - p1
            ge = t >= F32(0.0)
            lo = np.where(act & ge, mid, lo)
            hi = np.where(act & ~ge, mid, hi)
        e = np.arange(n).reshape((n,) + (1,) * (ex.ndim - 1))
        r = ranges[e, lo]
        bx = ex * ex
        by = ey * ey
        b = bx + by
        rm = F32(range_max)
        mm = rm * rm
        th = F32(th)
        lo_r = r - th
        hi_r = r + th
        known = (b <= mm) & (r > F32(0.0))
        free = (lo_r > F32(0.0)) & (b < lo_r * lo_r)
        occ = b <= hi_r * hi_r
    assert b.dtype == F32
    return known, free, occ


def update(cfg: Cfg, m: np.ndarray, ranges: np.ndarray, pose: np.ndarray, first=None, mask=None, thickness=None,
           range_max=np.inf, l_hit=8, l_free=4, l_max=64, decay=0, u=None) -> np.ndarray:
    """One ffmp_world_map call on m (n, Wc, Wc) int8: the new planes (m itself is not written)."""
    m = np.asarray(m, np.int8)
    n, Wc, _ = m.shape
    ranges = np.asarray(ranges, F32)
    pose = np.asarray(pose, F32).reshape(n, -1)[:, 0:4]
    u = sector_table(ranges.shape[1]) if u is None else np.asarray(u, F32)
    res, wh = F32(cfg.f["res_f"]), half_of(cfg, Wc)
    idx = np.arange(Wc).astype(F32)
    w = idx * res
    w = w - wh  # (Wc,) world coordinate of row p / column q
    sh = (n, 1, 1)
    px, py, c, s = (pose[:, k].reshape(sh) for k in range(4))
    with np.errstate(all="ignore"):
        dx = w.reshape(1, Wc, 1) - px
        dy = w.reshape(1, 1, Wc) - py
        a0 = c * dx
        a1 = s * dy
        ex = a0 + a1
        b0 = c * dy
        b1 = s * dx
        ey = b0 - b1
    assert ex.dtype == F32 and ey.dtype == F32
    known, free, occ = classes(ex, ey, ranges, u, cfg.f["res_f"] if thickness is None else thickness, range_max)
    restart = np.zeros(n, bool) if first is None else np.asarray(first).reshape(n) != 0
    M = np.where(restart.reshape(sh), 0, m.astype(np.int32))
    hit = np.clip(M + l_hit, -l_max, l_max)
    fre = np.clip(M - l_free, -l_max, l_max)
    none = M - np.sign(M) * np.minimum(np.abs(M), decay)
    out = np.where(~known, M, np.where(free, fre, np.where(occ, hit, none)))
    finite = np.isfinite(pose).all(axis=1)
    out = np.where(finite.reshape(sh), out, M)
    assert out.min() >= -128 and out.max() <= 127
    out = out.astype(np.int8)
    if mask is not None:
        keep = np.asarray(mask).reshape(n) == 0
        out[keep] = m[keep]
    return out


def ego_frame(cfg: Cfg, m: np.ndarray, pose: np.ndarray, unknown: int = 128, outside: int = 255, occ_thr: int = 8,
              free_thr: int = 4) -> np.ndarray:
    """One ffmp_world_frame call: (n, G, G) uint8."""
    m = np.asarray(m, np.int8)
    n, Wc, _ = m.shape
    G = cfg.grid
    pose = np.asarray(pose, F32).reshape(n, -1)[:, 0:4]
    res, wh = F32(cfg.f["res_f"]), half_of(cfg, Wc)
    co = cell_coords(cfg, np.arange(G)).astype(F32)
    ex, ey = co.reshape(1, G, 1), co.reshape(1, 1, G)
    sh = (n, 1, 1)
    px, py, c, s = (pose[:, k].reshape(sh) for k in range(4))
    with np.errstate(all="ignore"):
        a0 = c * ex
        a1 = s * ey
        wx = a0 - a1
        wx = wx + px
        b0 = s * ex
        b1 = c * ey
        wy = b0 + b1
        wy = wy + py
        fp = wx + wh
        fp = fp / res
        fp = np.rint(fp)
        fq = wy + wh
        fq = fq / res
        fq = np.rint(fq)
        inside = (fp >= F32(0.0)) & (fp <= F32(Wc - 1)) & (fq >= F32(0.0)) & (fq <= F32(Wc - 1))
    assert fp.dtype == F32 and fq.dtype == F32
    gp = np.where(inside, fp, F32(0.0)).astype(np.int64)
    gq = np.where(inside, fq, F32(0.0)).astype(np.int64)
    e = np.arange(n).reshape(sh)
    M = m[e, gp, gq].astype(np.int32)
    val = np.where(~inside, outside, np.where(M >= occ_thr, 255, np.where(M <= -free_thr, 0, unknown)))
    finite = np.isfinite(pose).all(axis=1)
    return np.where(finite.reshape(sh), val, unknown).astype(np.uint8)


def from_config(config: FFMPConfig, m, ranges, pose, thickness=None, range_max=None, **kw) -> np.ndarray:
    """update with the Python surface's defaults: thickness = res, range_max = cfg.lidar_range."""
    return update(Cfg.from_config(config), m, ranges, pose, thickness=config.res if thickness is None else thickness,
                  range_max=config.lidar_range if range_max is None else range_max, **kw)


def quality(frame: np.ndarray, truth: np.ndarray, unknown: int = 128):
    """(share of the cells the map calls known that contradict the ground-truth frame, share of the
    ground-truth cells the map knows); cells the view marks outside the plane count as not known."""
    tocc = truth > 0
    free, occ = frame == 0, frame == 255
    known = free | occ
    wrong = (free & tocc) | (occ & ~tocc)
    return float(wrong.sum() / max(int(known.sum()), 1)), float(known.mean())


def compare_on_oracle(config: FFMPConfig, n: int = 16, steps: int = 200, cells=None):
    """Drive the NumPy oracle under policy_nav's restated follower, updating both maps after the reset and
    after every step: ((contradiction, coverage) of the world map's ego view, the same of lidar_map_ref)."""
    from oracle import ffmp_oracle
    from tests import lidar_map_ref, nav_field_ref
    cfg = Cfg.from_config(config)
    G = config.grid
    Wc = default_cells(config) if cells is None else cells
    wm = np.zeros((n, Wc, Wc), np.int8)
    lm = np.zeros((n, G, G), np.int8)
    lframe = None
    # the commands go in through the oracle's CMD_V / CMD_W tables, as nav_field_ref.oracle_closed_loop does
    saved = ffmp_oracle.CMD_V, ffmp_oracle.CMD_W
    cv, cw = nav_field_ref._PerEnv(), nav_field_ref._PerEnv()
    ffmp_oracle.CMD_V, ffmp_oracle.CMD_W = cv, cw
    try:
        env = ffmp_oracle.OracleVecEnv(config, n, with_potential=False)
        env.reset()
        pose, episode = env.record[:, 0:4].copy(), env.episode.copy()
        for k in range(steps + 1):
            if k:
                cmd = nav_field_ref.nav_field(env.state_m[:, 1], env.record[:, 8:10], config)["cmd"]
                cv.value, cw.value = nav_field_ref._clip(cmd)
                env.step(np.zeros(n, dtype=np.int64))
            first = (env.episode != episode) | (env.record[:, 10] != 0) | (k == 0)
            now = env.record[:, 0:4].copy()
            wm = from_config(config, wm, env.lidar, now, first=first)
            lm, lframe = lidar_map_ref.from_config(config, lm, env.lidar, now, pose, first=first)
            pose, episode = now, env.episode.copy()
    finally:
        ffmp_oracle.CMD_V, ffmp_oracle.CMD_W = saved
    wframe = ego_frame(cfg, wm, pose, outside=128)
    truth = env.state_m[:, 1]
    return quality(wframe, truth), quality(lframe, truth)


if __name__ == "__main__":
    from tests.lidar_map_ref import LONG
    (wbad, wknown), (lbad, lknown) = compare_on_oracle(FFMPConfig(**LONG[64]))
    print(f"LONG[64], 16 envs, 200 steps under the field follower, cells = {default_cells(FFMPConfig(**LONG[64]))}:")
    print(f"  world map ego view: known cells contradicting the ground truth {100 * wbad:.2f} %, cells known {100 * wknown:.1f} %")
    print(f"  re-sampled ego map: known cells contradicting the ground truth {100 * lbad:.2f} %, cells known {100 * lknown:.1f} %")
