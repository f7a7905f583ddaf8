"""Motion flow estimated from the scan (include/ffmp.h ffmp_scan_flow) restated in NumPy,
step for step — the checker of tests/test_gpu_scan_flow.py — and the bookkeeping of LidarFlow restated on
the host (RefFlow), driven on the NumPy oracle or beside a live env.

The warp is tests/lidar_map_ref.prior_of applied to the plane of the earlier frame's hits (so the motion,
the restart rule and the rounding are that restatement's, already pinned against ffmp_scan_map); the
frames are tests/scan_map_ref.scan_frame's.  Everything else is integer: the planes are padded with
zeros by radius + block + 1 cells, a block sum is two passes of shifted additions, and the search visits
the displacements in the SPEC's order, keeping the first strictly smaller cost.

`python tests/scan_flow_ref.py` prints the quantities tests/test_scan_flow_host.py asserts: on the NumPy
oracle (TIE: G = 64, 8 moving discs, L = 180), 16 envs, 16 steps of random actions with an update after
the reset and after every step, the estimate against the ground-truth flow, with the ego motion and with
the identity warp in its place."""
import os
import sys

import numpy as np

if __name__ == "__main__":  # run as a script: the repository root is not on the path yet
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from flow_field_based_motion_planner_amd.config import FFMPConfig
from oracle.ffmp_oracle import Cfg
from tests import lidar_map_ref as M
from tests.scan_map_ref import dilate8, scan_frame

F32 = np.float32
KNOBS = dict(radius=4, block=3, gate=1, min_hits=3)
# the set-up of the physical tie: world_half = 0.45 * G * res, so the walls lie inside the map
TIE = {64: dict(grid=64, n_obst=8, n_beams=180, moving=True, flow=True, obst_vmax=0.5, world_half=0.45 * 64 * 0.05,
                goal_min=0.6, goal_max=1.3, max_steps=200, seed=31),
       100: dict(grid=100, n_obst=8, n_beams=180, moving=True, flow=True, obst_vmax=0.5, world_half=0.45 * 100 * 0.05,
                 goal_min=0.8, goal_max=2.0, max_steps=200, seed=12)}


def displacements(R: int):
    """The visiting order: |du|, |dv| <= R by ascending (du*du + dv*dv, du, dv)."""
    return sorted(((du, dv) for du in range(-R, R + 1) for dv in range(-R, R + 1)), key=lambda d: (d[0] * d[0] + d[1] * d[1], d[0], d[1]))


def hit_planes(cfg: Cfg, cur, prev, pose_now, pose_prev, first=None):
    """(Hc, Hp (n, G, G) bool, restart (n,) bool)."""
    cur, prev = np.asarray(cur, np.uint8), np.asarray(prev, np.uint8)
    n = cur.shape[0]
    bad = M.motion(cfg, pose_now, pose_prev)[4]
    restart = bad if first is None else bad | (np.asarray(first).reshape(n) != 0)
    hp = M.prior_of(cfg, (prev == 255).astype(np.int8), pose_now, pose_prev, first) != 0
    return cur == 255, hp, restart


def _box(f: np.ndarray, B: int, G: int) -> np.ndarray:
    """f (n, G + 2B, G + 2B) on the indices -B .. G+B-1: (n, G, G) sums over a, b in -B..B, as int16."""
    f = f.astype(np.int16)
    rows = sum(f[:, a:a + G, :] for a in range(2 * B + 1))
    return sum(rows[:, :, b:b + G] for b in range(2 * B + 1))


def scan_flow(cfg: Cfg, cur, prev, pose_now, pose_prev, scale, first=None, mask=None, radius=4, block=3, gate=1, min_hits=3,
              half=False, flow_in=None, kind_in=None):
    """One ffmp_scan_flow call: (flow (n, 2, G, G) float32, or float16 with half; kind (n, G, G) uint8).  An env
    with mask 0 keeps its cells of flow_in / kind_in (zeros when not given)."""
    G, R, B = cfg.grid, int(radius), int(block)
    hc, hp, restart = hit_planes(cfg, cur, prev, pose_now, pose_prev, first)
    n = hc.shape[0]
    P = R + B + 1
    pad = ((0, 0), (P, P), (P, P))
    pc, pp = np.pad(hc, pad), np.pad(hp, pad)
    grid = np.pad(np.ones((1, G, G), bool), pad)  # a cell index outside 0..G-1 reads 0 in every plane
    dc, dp = dilate8(pc) & grid, dilate8(pp) & grid

    def dom(x, di, dj):  # x[i + di][j + dj] for i, j in -B .. G+B-1
        return x[:, P - B + di:P + B + di + G, P - B + dj:P + B + dj + G]

    hcd = dom(pc, 0, 0)
    nc = _box(hcd, B, G)
    c0 = _box(dom(pc & ~dp, 0, 0), B, G) + _box(dom(pp & ~dc, 0, 0), B, G)
    best = np.full((n, G, G), 1000, np.int16)
    du = np.zeros((n, G, G), np.int32)
    dv = np.zeros((n, G, G), np.int32)
    for d in displacements(R):
        q = dom(pp, -d[0], -d[1])
        npd = _box(q, B, G)
        cost = _box(hcd ^ q, B, G)
        better = (npd >= min_hits) & (cost < best)
        best = np.where(better, cost, best)
        du = np.where(better, d[0], du)
        dv = np.where(better, d[1], dv)
    found = best < 1000
    live = hc & ~restart.reshape(n, 1, 1) & (nc >= min_hits)
    kind = np.where(live, np.where(c0 <= gate, 1, np.where(found, 2, 0)), 0).astype(np.uint8)
    s = F32(scale)
    vx = np.where(kind == 2, du.astype(F32) * s, F32(0.0)).astype(F32)
    vy = np.where(kind == 2, dv.astype(F32) * s, F32(0.0)).astype(F32)
    flow = np.stack([vx, vy], axis=1)
    if half:
        with np.errstate(over="ignore"):
            flow = flow.astype(np.float16)  # round to nearest even
    if mask is not None:
        keep = np.asarray(mask).reshape(n) == 0
        flow[keep] = 0 if flow_in is None else np.asarray(flow_in)[keep]
        kind[keep] = 0 if kind_in is None else np.asarray(kind_in)[keep]
    return flow, kind


class RefFlow:
    """LidarFlow's bookkeeping restated on the host: the ring of lag + 1 frames with the pose words and the
    episode id beside each (-1: no frame of this env in the slot), the updates since the restart, the
    outputs.  warp(pose_now, pose_prev) -> (pose_now, pose_prev): a deliberately wrong motion."""

    def __init__(self, config: FFMPConfig, n: int, lag=4, radius=4, block=3, gate=1, min_hits=3, thickness=None, range_max=None,
                 half=False, warp=None):
        G = config.grid
        self.config, self.cfg, self.n, self.lag, self.half, self.warp = config, Cfg.from_config(config), n, lag, half, warp
        self.knobs = dict(radius=radius, block=block, gate=gate, min_hits=min_hits)
        self.thickness = config.res if thickness is None else thickness
        self.range_max = config.lidar_range if range_max is None else range_max
        self.scale = F32(config.res / (lag * config.dt))
        self.frames = np.zeros((lag + 1, n, G, G), np.uint8)
        self.poses = np.zeros((lag + 1, n, 4), F32)
        self.episodes = np.full((lag + 1, n), -1, np.int64)
        self.pos = 0
        self.updates = np.zeros(n, np.int64)
        self.flow = np.zeros((n, 2, G, G), np.float16 if half else F32)
        self.kind = np.zeros((n, G, G), np.uint8)

    @property
    def frame(self):
        return self.frames[self.pos]

    def reset(self, mask=None):
        sel = np.ones(self.n, bool) if mask is None else np.asarray(mask).reshape(self.n) != 0
        self.episodes[:, sel] = -1
        self.updates[sel] = 0
        self.flow[sel] = 0
        self.kind[sel] = 0

    def update(self, lidar, record=None, episode=None, pose=None, first=None, mask=None):
        """lidar (n, L); record (n, >= 11) and episode (n,) as the env's, or pose (n, 4) [and first].  Returns
        the `first` bytes the kernel got."""
        n, lag = self.n, self.lag
        last = self.episodes[self.pos]
        if pose is None:
            pose = np.asarray(record, F32)[:, 0:4]
            episode = np.asarray(episode).astype(np.int64)
            if first is None:
                first = (episode != last) | (np.asarray(record)[:, 10] != 0)
        else:
            pose = np.asarray(pose, F32)
            episode = np.zeros(n, np.int64)
        never = last < 0
        restart = never if first is None else (np.asarray(first).reshape(n) != 0) | never
        sel = np.ones(n, bool) if mask is None else np.asarray(mask).reshape(n) != 0
        restart = restart & sel
        self.episodes[:, restart] = -1
        slot = (self.pos + 1) % (lag + 1)
        old = (slot + 1) % (lag + 1)
        new = scan_frame(self.cfg, lidar, 128, self.thickness, self.range_max)
        self.frames[slot][sel] = new[sel]
        self.episodes[slot] = np.where(sel, episode, -1)
        kfirst = self.episodes[old] != self.episodes[slot]
        now, prev = pose, self.poses[old]
        if self.warp is not None:
            now, prev = self.warp(now, prev)
        self.flow, self.kind = scan_flow(self.cfg, self.frames[slot], self.frames[old], now, prev, self.scale, first=kfirst,
                                         mask=None if mask is None else sel, half=self.half, flow_in=self.flow, kind_in=self.kind,
                                         **self.knobs)
        self.poses[slot] = pose
        self.updates = np.where(sel, np.where(restart, 1, self.updates + 1), self.updates)
        self.pos = slot
        return kfirst


# ---------------------------------------------------------------------------------------- the physical tie
def near_flow(flow: np.ndarray, reach: int = 2):
    """The ground-truth flow dilated by `reach` cells: per cell the flow of the nearest cell (squared
    distance, then row, then column offset) within the (2*reach+1)² neighbourhood that lies on a moving
    disc (flow != 0), and whether there is one.  (n, 2, G, G) float32, (n, G, G) bool."""
    n, _, G, _ = flow.shape
    on = (flow[:, 0] != 0) | (flow[:, 1] != 0)
    pad = ((0, 0), (reach, reach), (reach, reach))
    pon, px, py = np.pad(on, pad), np.pad(flow[:, 0], pad), np.pad(flow[:, 1], pad)
    out = np.zeros_like(flow)
    has = np.zeros((n, G, G), bool)
    for di, dj in displacements(reach):
        sl = (slice(None), slice(reach + di, reach + di + G), slice(reach + dj, reach + dj + G))
        take = pon[sl] & ~has
        out[:, 0] = np.where(take, px[sl], out[:, 0])
        out[:, 1] = np.where(take, py[sl], out[:, 1])
        has |= pon[sl]
    return out, has


def tie_on_oracle(config: FFMPConfig, n: int = 16, steps: int = 16, seed: int = 1, identity: bool = False, lag: int = 4, **knobs):
    """Drive the NumPy oracle with default_rng(seed) actions, a RefFlow updated after the reset and after every
    step.  Over every update and every env with an estimate (not restarting) counts, among the hit cells:
      moving: kind 1 or 2 and within two cells of a moving disc — how many lie within 2 quanta (either
              component) of the dilated ground-truth flow;
      static: farther than two cells from every disc — how many have flow exactly zero.
    identity: the earlier pose is replaced by the current one (no ego-motion compensation).
    Returns (moving good, moving all, static zero, static all)."""
    from oracle.ffmp_oracle import OracleVecEnv
    env = OracleVecEnv(config, n, with_potential=False)
    env.reset()
    warp = (lambda now, prev: (now, now)) if identity else None
    ref = RefFlow(config, n, lag=lag, warp=warp, **knobs)
    rng = np.random.default_rng(seed)
    q2 = 2.0 * float(ref.scale) + 1e-6
    tally = np.zeros(4, np.int64)
    for k in range(steps + 1):
        if k:
            env.step(rng.integers(0, 28, n))
        first = ref.update(env.lidar, env.record, env.episode)
        live = ~first.reshape(n, 1, 1)
        hit = (ref.frame == 255) & live
        truth, on = near_flow(env.flow)
        disc = discs_near(env, config)
        err = np.maximum(np.abs(ref.flow[:, 0] - truth[:, 0]), np.abs(ref.flow[:, 1] - truth[:, 1]))
        mov = hit & on & (ref.kind > 0)
        sta = hit & ~disc
        zero = (ref.flow[:, 0] == 0) & (ref.flow[:, 1] == 0)
        tally += (int((mov & (err <= q2)).sum()), int(mov.sum()), int((sta & zero).sum()), int(sta.sum()))
    return tuple(int(t) for t in tally)


def discs_near(env, config: FFMPConfig, reach: int = 2) -> np.ndarray:
    """(n, G, G) bool: within `reach` cells of an occupied cell that is not the world's wall — the newest
    ground-truth frame without the cells outside the world."""
    from oracle.ffmp_oracle import cell_coords, outside_world
    cfg = env.cfg
    G = cfg.grid
    c = cell_coords(cfg, np.arange(G)).astype(F32)
    wall = outside_world(cfg, env.record[:, 0:4].astype(F32), c.reshape(1, G, 1), c.reshape(1, 1, G))
    m = (env.state_m[:, 1] > 0) & ~wall
    for _ in range(reach):
        m = dilate8(m)
    return m


if __name__ == "__main__":
    for G in (64, 100):
        for seed in (1, 2):
            for identity in (False, True):
                g, a, z, s = tie_on_oracle(FFMPConfig(**TIE[G]), seed=seed, identity=identity)
                print(f"TIE[{G}] seed {seed} {'identity warp' if identity else 'ego compensated'}: moving within 2 quanta "
                      f"{g} of {a} ({g / max(a, 1):.3f}), static exactly zero {z} of {s} ({z / max(s, 1):.3f})")
