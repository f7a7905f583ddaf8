"""FFMPConfig — the one POD-like configuration of the batched FFMP environment.

Reference constants it carries (YoshitakaNagai/flow_field_based_motion_planner):
  MAP_RESOLUTION 0.05, ROBOT_RSIZE 0.13, GOAL_THRESHOLHD 0.5, MAP_GRID_NUM 100,
  MAP_RANGE 5.0                       src/gym_ffmp/envs/ffmp.py:14-19
  MAX_STEPS 200                       src/train.py:60
  RobotAction.cmd[28]                 src/gym_ffmp/envs/robot/config.py:25-55
Everything else (dt, world size, obstacle model, potential-field constants,
lidar) has no reference implementation (Gazebo / external BEV nodes)
and is this framework's own specification — see DESIGN.md §SPEC.

This module is pure host logic (no torch, no GPU) so it is testable on CPU.
"""
from __future__ import annotations

import dataclasses
import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np

COLLIDE_FOOTPRINT = 1
COLLIDE_LIDAR = 2
MAX_OBST = 64
MAX_FOOT = 128
MAX_BEAMS = 1024
N_ACTIONS = 28
REC_HDR = 16

# RobotAction.cmd (config.py:28-55) as literals: cmd[7*vi + wi] = (CMD_V[vi], CMD_W[wi]).
CMD_V = (0.0, 0.2, 0.4, 0.6)
CMD_W = (-0.6, -0.4, -0.2, 0.0, 0.2, 0.4, 0.6)


def action_table() -> List[Tuple[float, float]]:
    return [(v, w) for v in CMD_V for w in CMD_W]


ROLLOUT_MAX = 28  # |cell offset| a rollout table may hold (include/ffmp.h ffmp_dwa: 28 + 3 footprint cells = 31)


def _rollouts(cfg, v, w, horizon: int, stride: int, probe: float):
    """The unicycle (DESIGN §3 "Unicycle") rolled forward from ego pose (0, 0, 0) per candidate
    m = len(w) * vi + wi, float64 with math.cos / math.sin: (cells (A, H, 2), probes (A, H, 2), cmds (A, 2)) —
    cells[m][k-1] the cell offset after k * stride env steps, probes[m][k-1] that of the point `probe` metres
    ahead of it along the heading at that moment."""
    horizon, stride, probe = int(horizon), int(stride), float(probe)
    if horizon < 1 or stride < 1:
        raise ValueError(f"rollout_table: horizon and stride must be >= 1, got {horizon}, {stride}")
    if not (math.isfinite(probe) and probe >= 0):
        raise ValueError(f"rollout_table: probe must be finite and >= 0, got {probe}")
    v, w = [float(a) for a in v], [float(a) for a in w]
    if not v or not w or not all(math.isfinite(a) for a in v + w):
        raise ValueError("rollout_table: v and w must be non-empty lists of finite numbers")
    res, dt = float(cfg.res), float(cfg.dt)
    cmds = np.array([(vm, wm) for vm in v for wm in w], dtype=np.float64)
    cells = np.zeros((len(cmds), horizon, 2), dtype=np.float64)
    probes = np.zeros_like(cells)
    for m, (vm, wm) in enumerate(cmds.tolist()):
        x = y = yaw = 0.0
        for k in range(1, horizon + 1):
            for _ in range(stride):
                x += (vm * math.cos(yaw)) * dt
                y += (vm * math.sin(yaw)) * dt
                yaw += wm * dt
            cells[m, k - 1] = (x / res, y / res)
            probes[m, k - 1] = ((x + probe * math.cos(yaw)) / res, (y + probe * math.sin(yaw)) / res)
    return np.rint(cells), np.rint(probes), cmds


def rollout_table(cfg, v=(0, .2, .4, .6), w=(-.6, -.4, -.2, 0, .2, .4, .6), horizon: int = 24, stride: int = 1,
                  probe: float = 0.325):
    """The candidate table of the rollout planner (include/ffmp.h ffmp_dwa): (traj int16 (A, H + 1, 2),
    cmds float64 (A, 2)).  Candidate m = len(w) * vi + wi is the command (v[vi], w[wi]) — with the default
    lists the reference's action id (RobotAction.cmd, config.py:28-55).  traj[m][k-1], k = 1..H, is the cell
    offset (rint(x / res), rint(y / res)) of the unicycle after k * stride env steps of that command from ego
    pose (0, 0, 0); traj[m][H] is the probe, the endpoint pushed `probe` metres forward along the final
    heading (the forward point of ROS's dwa_local_planner: what lets a turn on the spot score a heading).
    All trigonometry is here, float64; the kernel sees integers.  ValueError if any |offset| exceeds 28
    (ROLLOUT_MAX) — at res 0.05, dt 0.1 the default lists fit up to horizon 18 (rollout_horizon)."""
    cells, probes, cmds = _rollouts(cfg, v, w, horizon, stride, probe)
    traj = np.concatenate([cells, probes[:, -1:]], axis=1)
    worst = float(np.abs(traj).max())
    if not worst <= ROLLOUT_MAX:  # a NaN (res or dt of 0) fails too
        raise ValueError(f"rollout_table: a rollout reaches {worst:.0f} cells from the robot, more than {ROLLOUT_MAX} "
                         f"(horizon {horizon}, stride {stride}, probe {probe}, dt {cfg.dt}, res {cfg.res}): shorten it")
    return traj.astype(np.int16), cmds


def rollout_horizon(cfg, v=(0, .2, .4, .6), w=(-.6, -.4, -.2, 0, .2, .4, .6), horizon: int = 24, stride: int = 1,
                    probe: float = 0.325) -> int:
    """The longest horizon H <= `horizon` at which rollout_table(cfg, v, w, H, stride, probe) stays within
    its 28 cells; ValueError if not even H = 1 does."""
    cells, probes, _ = _rollouts(cfg, v, w, horizon, stride, probe)
    for H in range(int(horizon), 0, -1):
        if max(np.abs(cells[:, :H]).max(), np.abs(probes[:, H - 1]).max()) <= ROLLOUT_MAX:
            return H
    raise ValueError(f"rollout_horizon: no horizon keeps the rollouts within {ROLLOUT_MAX} cells "
                     f"(stride {stride}, probe {probe}, dt {cfg.dt}, res {cfg.res})")


def footprint_offsets(grid: int, res: float = 0.05, robot_r: float = 0.13) -> List[Tuple[int, int]]:
    """robot_grids of FFMP.is_collision (ffmp.py:87-94), generalised to any G.

    Cell (i, j) belongs to the footprint iff
        sqrt(pow(i*res - 0.5*R, 2) + pow(j*res - 0.5*R, 2)) <= robot_r,  R = G*res,
    evaluated in float64 exactly as the reference does (for G=100, R = 5.0 =
    MAP_RANGE).  Returned as offsets from (G//2, G//2), in the reference's
    (i, j) scan order.  Only a window around the centre can qualify.
    """
    map_range = grid * res
    c = grid // 2
    w = int(math.ceil(robot_r / res)) + 2
    out = []
    for i in range(max(0, c - w), min(grid, c + w + 1)):
        for j in range(max(0, c - w), min(grid, c + w + 1)):
            xp = math.pow(i * res - 0.5 * map_range, 2)
            yp = math.pow(j * res - 0.5 * map_range, 2)
            if math.sqrt(xp + yp) <= robot_r:
                out.append((i - c, j - c))
    return out


def beam_table(n_beams: int) -> np.ndarray:
    """(L, 2) float64 {cos, sin} of beam angles -pi + l*2pi/L (robot frame)."""
    out = np.zeros((n_beams, 2), dtype=np.float64)
    if n_beams:
        step = 2.0 * math.pi / n_beams
        for l in range(n_beams):
            th = -math.pi + l * step
            out[l, 0] = math.cos(th)
            out[l, 1] = math.sin(th)
    return out


def beam_dirs(n_beams: int) -> np.ndarray:
    """(L, 2) float32: beam_table rounded — the `beams` table of ffmp_scan_match (include/ffmp.h)."""
    return beam_table(n_beams).astype(np.float32)


def turn_table(turns: int, dtheta: float) -> np.ndarray:
    """(2T + 1, 2) float32 {cos, sin} of (k - T) * dtheta, math.cos / math.sin of the float64 angle rounded:
    the rotation steps of ffmp_scan_match (include/ffmp.h).  Entry T is exactly (1, 0)."""
    turns = int(turns)
    if turns < 0:
        raise ValueError(f"turns must be >= 0, got {turns}")
    out = np.zeros((2 * turns + 1, 2), dtype=np.float32)
    for k in range(2 * turns + 1):
        th = (k - turns) * float(dtheta)
        out[k, 0] = math.cos(th)
        out[k, 1] = math.sin(th)
    return out


def sector_table(n_beams: int) -> np.ndarray:
    """(L, 2) float32 {cos, sin} of the cone boundaries -pi + (m - 1/2)*2pi/L (robot frame), each the
    float32 rounding of math.cos / math.sin of the float64 angle: sector m, from boundary m to
    boundary m + 1, is the cone of beam m (include/ffmp.h ffmp_scan_frames)."""
    out = np.zeros((n_beams, 2), dtype=np.float32)
    if n_beams:
        step = 2.0 * math.pi / n_beams
        for m in range(n_beams):
            th = -math.pi + (m - 0.5) * step
            out[m, 0] = math.cos(th)
            out[m, 1] = math.sin(th)
    return out


@dataclass
class FFMPConfig:
    grid: int = 100                 # G (MAP_GRID_NUM, ffmp.py:15)
    n_obst: int = 4                 # K
    n_beams: int = 180              # L (0 disables lidar)
    max_steps: int = 200            # MAX_STEPS (train.py:60)
    moving: bool = False
    autoreset: bool = True
    collide_mode: Optional[int] = None  # default: footprint | (lidar if L > 0)
    res: float = 0.05               # MAP_RESOLUTION (ffmp.py:18)
    dt: float = 0.1                 # s per env step (SPEC)
    robot_r: float = 0.13           # ROBOT_RSIZE (ffmp.py:17)
    goal_thr: float = 0.5           # GOAL_THRESHOLHD (ffmp.py:19)
    world_half: Optional[float] = None   # default G*res (world side 2*G*res)
    lidar_max: Optional[float] = None    # default G*res/2
    goal_min: float = 1.0
    goal_max: Optional[float] = None     # default G*res/2
    obst_rmin: float = 0.10
    obst_rmax: float = 0.30
    obst_vmax: float = 0.5
    start_clear: float = 0.5
    goal_clear: float = 0.5
    k_att: float = 1.0
    k_rep: float = 0.1
    rho0: float = 0.5
    rho_min: Optional[float] = None      # default res/2
    cull_margin: float = 0.1
    flow: bool = False              # also raster the BEV motion-flow planes
    seed: int = 0

    # ---- derived -----------------------------------------------------------
    def __post_init__(self):
        self.validate()

    def validate(self):
        G = self.grid
        if G < 8 or G > 4096 or G % 4:
            raise ValueError(f"grid must be a multiple of 4 in [8, 4096], got {G}")
        if not 0 <= self.n_obst <= MAX_OBST:
            raise ValueError(f"n_obst must be in [0, {MAX_OBST}], got {self.n_obst}")
        if not 0 <= self.n_beams <= MAX_BEAMS:
            raise ValueError(f"n_beams must be in [0, {MAX_BEAMS}], got {self.n_beams}")
        # the physical constants (DESIGN.md §SPEC "Which constants are free"): finite, on the side of
        # zero the kernels assume, and a cull margin above the float32 rounding of the culls
        for name, v in (("res", self.res), ("dt", self.dt), ("robot_r", self.robot_r), ("goal_thr", self.goal_thr),
                        ("world_half", self.world_half), ("lidar_max", self.lidar_max), ("k_att", self.k_att),
                        ("k_rep", self.k_rep), ("rho0", self.rho0), ("rho_min", self.rho_min),
                        ("cull_margin", self.cull_margin)):
            if v is not None and not math.isfinite(v):
                raise ValueError(f"{name} must be finite, got {v}")
        if self.res <= 0 or self.dt < 0:
            raise ValueError("res must be > 0 and dt >= 0")
        if self.rho0 <= 0:
            raise ValueError(f"rho0 must be > 0, got {self.rho0}")
        if self.lidar_max is not None and self.lidar_max < 0:
            raise ValueError(f"lidar_max must be >= 0, got {self.lidar_max}")
        if self.robot_r < 0:
            raise ValueError(f"robot_r must be >= 0, got {self.robot_r}")
        if not self.cull_margin >= self.cull_floor():
            raise ValueError(f"cull_margin must be >= {self.cull_floor():.3g} (cull_floor(): 2^-16 of the scene's "
                             f"extent), got {self.cull_margin}")
        if not 0 <= self.seed < 2 ** 64:
            raise ValueError("seed must fit in uint64")
        if len(self.footprint) > MAX_FOOT:
            raise ValueError("footprint too large")

    def cull_floor(self) -> float:
        """The smallest cull_margin (metres) at which the raster's and the sensors' culls are exact:
        2^-16 S with S = G res / 2 + world_half + rho0 + obst_rmax, a bound on every distance the
        culls compare.  Fewer than 16 float32 roundings of at most 2^-24 each separate a cull's
        distance from the cell test's, less than 2^-20 S; the floor leaves a factor of 16
        (DESIGN.md §5 "The cull margin's floor")."""
        return 2.0 ** -16 * (0.5 * (self.grid * self.res) + self.W + self.rho0 + self.obst_rmax)

    @property
    def W(self) -> float:
        return self.grid * self.res if self.world_half is None else float(self.world_half)

    @property
    def lidar_range(self) -> float:
        return 0.5 * self.grid * self.res if self.lidar_max is None else float(self.lidar_max)

    @property
    def goal_hi(self) -> float:
        return 0.5 * self.grid * self.res if self.goal_max is None else float(self.goal_max)

    @property
    def rho_lo(self) -> float:
        return 0.5 * self.res if self.rho_min is None else float(self.rho_min)

    @property
    def mode(self) -> int:
        if self.collide_mode is not None:
            return int(self.collide_mode)
        return COLLIDE_FOOTPRINT | (COLLIDE_LIDAR if self.n_beams > 0 else 0)

    @property
    def footprint(self) -> List[Tuple[int, int]]:
        return footprint_offsets(self.grid, self.res, self.robot_r)

    def f32_constants(self) -> Dict[str, np.float32]:
        """The float32 raster constants, each = (float)(double expression)."""
        f = np.float32
        return {
            "res_f": f(self.res),
            "half_f": f(0.5 * (self.grid * self.res)),
            "world_half_f": f(self.W),
            "half_ka_f": f(0.5 * self.k_att),
            "half_kr_f": f(0.5 * self.k_rep),
            "rho0_f": f(self.rho0),
            "inv_rho0_f": f(1.0 / self.rho0),
            "rho_min_f": f(self.rho_lo),
            "inv_2res_f": f(1.0 / (2.0 * self.res)),
            "cull_margin_f": f(self.cull_margin),
        }

    def record_len(self) -> int:
        return REC_HDR + 12 * self.n_obst

    def replace(self, **kw) -> "FFMPConfig":
        return dataclasses.replace(self, **kw)

    def to_dict(self) -> dict:
        return dataclasses.asdict(self)


# Benchmark configurations (BASELINE.json:configs; SURVEY §8 "Config shorthand").
# n_envs is the TOTAL env count; gpus the GPU count the config is quoted on.
PRESETS: Dict[str, dict] = {
    "C1": dict(n_envs=1, gpus=0, cfg=dict(grid=64, n_obst=4, moving=False, n_beams=0)),
    "C2": dict(n_envs=4096, gpus=1, cfg=dict(grid=128, n_obst=8, moving=False, n_beams=0)),
    "C3": dict(n_envs=32768, gpus=1, cfg=dict(grid=256, n_obst=16, moving=True, n_beams=180)),
    "C4": dict(n_envs=65536, gpus=8, cfg=dict(grid=256, n_obst=16, moving=True, n_beams=180)),
    "C5": dict(n_envs=131072, gpus=8, cfg=dict(grid=512, n_obst=32, moving=True, n_beams=360)),
}


def preset(name: str, **overrides) -> FFMPConfig:
    if name not in PRESETS:
        raise KeyError(f"unknown preset {name!r}; known: {sorted(PRESETS)}")
    kw = dict(PRESETS[name]["cfg"])
    kw.update(overrides)
    return FFMPConfig(**kw)


def bytes_per_env_step(cfg: FFMPConfig, potential: bool = True, window: int = 2,
                       seamless: bool = False, obs_format: str = "f32") -> Dict[str, int]:
    """Algorithmic HBM bytes of one env step.

    raster kernel: writes the new float32 frame of state_m (4 G^2), the older one too on the
    steps where the frame window wraps (every W-1 steps; every step for W = 2; never with the
    seamless ring) — plus, not
    counted here, the older frame of each env reset on the other steps —, the float32 potential
    plane (4 G^2) and, with cfg.flow, the two float32 flow planes (8 G^2); reads the raster
    record (64 + 48 K).  state kernel: reads/writes pose, goal, d0, t, episode, obstacles and
    writes the small obs, lidar and the record.  obs_format "u8f16" (FFMPVec): 1-byte frames and
    a 2-byte potential plane (and 2-byte flow planes) instead.
    """
    G2 = cfg.grid * cfg.grid
    K, L = cfg.n_obst, cfg.n_beams
    rec = 4 * cfg.record_len()
    fb, pb = {"f32": (4, 4), "u8f16": (1, 2)}[obs_format]
    frames = fb * G2 + (0 if seamless and window > 2 else (fb * G2) // (max(int(window), 2) - 1))
    raster = frames + (pb * G2 if potential else 0) + (2 * pb * G2 if cfg.flow else 0) + rec
    state_rw = 2 * (24 + 16 + 8 + 4 + 4 + 40 * K)  # pose, goal, d0, t, episode, obst(32)+r(8)
    small_obs = 4 * (2 + 2 + 1 + 2) + 4 * L + rec + 8 + 4 + 4  # g, v, t, grad, lidar, record, action, reward, flags
    return {"raster": raster, "state": state_rw + small_obs, "total": raster + state_rw + small_obs}
