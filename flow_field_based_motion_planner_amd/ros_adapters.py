"""ROS-message adapters: the batched env's tensors <-> the messages the reference loop consumed
and produced (src/train.py:82-165), for a sim-to-real bridge.

No rospy here (not installed; nothing runs a ROS graph): messages are duck-typed — any object
with the fields rospy messages have works, and `Msg` is a minimal stand-in for tests.  The
conversions keep the reference's exact semantics:

  laser_callback (:145-150)          ranges_to_scan_data: keep r with `r != inf and r` — NaN
                                     is kept, 0.0 and +inf are dropped — appended to a list
                                     that starts as [None] (:97) and grows across callbacks
  LaserScan -> the env's lidar row    scan_to_lidar_row: a scan of any field of view and ray count
                                     resampled onto the env's L-beam circle, the `ranges=` row
                                     of FFMPVec.lidar_frames (the map built from the scan)
  temporal_bev_image_callback        image_to_map: mono8 image (H, W) -> float32 (1, H, W),
    (:116-121)                       raw 0..255 (kornia.image_to_tensor(keepdim=True).float())
  robot_position_extractor           odometry_to_pose: (x, y, yaw) with yaw from the quaternion
    (:157-165)                       (tf euler_from_quaternion, axes 'sxyz'), stamp -> seconds
  Odometry -> the map's pose words    odom_to_pose_row: {x, y, cos yaw, sin yaw} float32, the `pose=`
                                     row of LidarMap.update (the accumulated scan map)
  pose_array_callback (:126-132)     pose_array_to_start_goal: poses[0], poses[1];
                                     pose_array_to_scenario: that start / goal plus the discs as
                                     the arrays FFMPVec.set_scenarios / FFMP.reset(options=) take
  relative_goal_calculator           relative_goal: [sqrt(dx^2 + dy^2), pi_to_pi(atan2(dy, dx)
    (:167-180)                       - yaw)] in float64, the `relative_goal_info` rewarder2 takes
  cmd_vel_publisher (:134-143)       action_to_twist: RobotAction.cmd[a] -> linear.x, angular.z;
                                     command_to_twist: a continuous (v, w) -> the same Twist;
                                     twist_to_command: the way back, a /cmd_vel Twist -> (v, w)
                                     for FFMPVec.step / FFMP.step

and the other direction, env -> messages: lidar_to_ranges, frame_to_image, pose_to_odometry,
world_map_to_occupancy_grid (one env's WorldMap plane as a dict shaped like nav_msgs/OccupancyGrid) and
map_to_odom_transform (the map -> odom transform a localisation node publishes, from the pose
WorldMap.match found, as a dict shaped like geometry_msgs/TransformStamped).
Host-side (numpy): a bridge talks to one robot at a time.
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence, Tuple

import numpy as np

from .config import action_table


class Msg:
    """Minimal attribute bag standing in for a rospy message (nested via keyword dicts)."""

    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, Msg(**v) if isinstance(v, dict) else v)

    def __repr__(self):
        return f"Msg({', '.join(f'{k}={v!r}' for k, v in vars(self).items())})"


# ----------------------------------------------------------------------------- sensor -> env
def ranges_to_scan_data(ranges: Sequence[float], scan_data: Optional[List] = None) -> List:
    """laser_callback (train.py:145-150): append every range that is `!= inf` and truthy."""
    out = [None] if scan_data is None else scan_data
    for r in ranges:
        if r != float("inf") and r:
            out.append(r)
    return out


def scan_to_lidar_row(msg_or_ranges, n_beams: int, angle_min: Optional[float] = None,
                      angle_increment: Optional[float] = None, range_min: float = 0.0,
                      range_max: float = float("inf")) -> np.ndarray:
    """A LaserScan (or its bare `ranges`) resampled onto the env's L-beam full circle: (L,) float32 in
    the lidar's convention, the `ranges=` row FFMPVec.lidar_frames / ffmp_scan_frames take.

    Ray k of the scan points at angle_min + k * angle_increment (taken from the message when not
    given; a bare sequence defaults to a full circle from -pi).  Env beam l takes the rays whose
    wrapped angle falls in its cone [-pi + (l - 1/2) 2pi/L, -pi + (l + 1/2) 2pi/L) — the cone
    ffmp_scan_frames paints with that beam's range — and of several the nearest finite range.
    Per ray: NaN, a range <= 0 or below range_min is no data (NaN); one above range_max is no return
    (+inf).  A message's own range_min / range_max narrow the two arguments.  A cone no ray falls
    into, or with no usable ray, is NaN (no data: the map keeps `unknown` there), so a 270 degree scan
    leaves the rear cones NaN and an odd ray count needs no care.
    scan_to_lidar_row(lidar_to_ranges(row, rm), L, -pi, 2 pi / L) gives `row` back except that -inf
    (the origin inside a disc, published as 0.0) comes back as NaN: both mean no data to the map."""
    L = int(n_beams)
    if L < 1:
        raise ValueError("n_beams must be >= 1")
    if hasattr(msg_or_ranges, "ranges"):
        msg = msg_or_ranges
        vals = np.asarray(msg.ranges, dtype=np.float64).reshape(-1)
        if angle_min is None:
            angle_min = float(msg.angle_min)
        if angle_increment is None:
            angle_increment = float(msg.angle_increment)
        range_min = max(float(range_min), float(getattr(msg, "range_min", range_min)))
        range_max = min(float(range_max), float(getattr(msg, "range_max", range_max)))
    else:
        vals = np.asarray(msg_or_ranges, dtype=np.float64).reshape(-1)
        if angle_min is None:
            angle_min = -math.pi
        if angle_increment is None:
            angle_increment = 2.0 * math.pi / max(len(vals), 1)
    step = 2.0 * math.pi / L
    ang = float(angle_min) + np.arange(len(vals), dtype=np.float64) * float(angle_increment)
    cone = np.floor((ang + math.pi) / step + 0.5).astype(np.int64) % L
    with np.errstate(invalid="ignore"):
        dead = np.isnan(vals) | (vals <= 0.0) | (vals < range_min)
        none = ~dead & (vals > range_max)
    hit = ~dead & ~none
    row = np.full(L, np.nan)
    row[cone[none]] = np.inf
    best = np.full(L, np.inf)
    np.minimum.at(best, cone[hit], vals[hit])
    has = np.zeros(L, dtype=bool)
    has[cone[hit]] = True
    row[has] = best[has]
    return row.astype(np.float32)


def image_to_map(img: np.ndarray) -> np.ndarray:
    """temporal_bev_image_callback (train.py:116-121): mono8 (H, W) -> float32 (1, H, W), 0..255."""
    a = np.asarray(img)
    if a.ndim == 2:
        a = a[None]
    elif a.ndim == 3:
        a = np.transpose(a, (2, 0, 1))  # HWC -> CHW, as kornia.image_to_tensor
    else:
        raise ValueError("image must be (H, W) or (H, W, C)")
    return a.astype(np.float32)


def quaternion_to_yaw(x: float, y: float, z: float, w: float) -> float:
    """Yaw of tf.transformations.euler_from_quaternion([x, y, z, w]) (static 'sxyz' axes):
    atan2(M[1,0], M[0,0]) of the normalised rotation matrix, 0 in gimbal lock or for a
    (near-)zero quaternion (tf returns the identity matrix there).  tf is not installed here,
    so this restates its published algorithm (ulp-level agreement; parity unpinned)."""
    eps = 4.0 * float(np.finfo(float).eps)  # tf's _EPS
    n = x * x + y * y + z * z + w * w
    if n < eps:
        return 0.0
    s = 2.0 / n
    m10 = s * (x * y + z * w)
    m00 = 1.0 - s * (y * y + z * z)
    if math.sqrt(m00 * m00 + m10 * m10) > eps:
        return math.atan2(m10, m00)
    return 0.0


def odometry_to_pose(msg) -> Tuple[float, float, float, float]:
    """robot_position_extractor (train.py:157-165): (x, y, yaw, stamp seconds)."""
    p = msg.pose.pose.position
    q = msg.pose.pose.orientation
    st = msg.header.stamp
    t = float(st.to_sec()) if hasattr(st, "to_sec") else float(st.secs) + 1e-9 * float(st.nsecs)
    return float(p.x), float(p.y), quaternion_to_yaw(q.x, q.y, q.z, q.w), t


def odom_to_pose_row(msg) -> np.ndarray:
    """nav_msgs/Odometry -> the four float32 pose words {x, y, cos yaw, sin yaw} of record words 0..3:
    one row of the `pose=` tensor LidarMap.update / ffmp_scan_map take.  The yaw is quaternion_to_yaw's
    (which normalises: a non-unit quaternion gives the yaw of its direction, a (near-)zero one yaw 0),
    cos and sin are math.cos / math.sin of it rounded to float32.  A non-finite position or
    quaternion gives non-finite words, and the map restarts that env (include/ffmp.h ffmp_scan_map)."""
    p = msg.pose.pose.position
    q = msg.pose.pose.orientation
    quat = (float(q.x), float(q.y), float(q.z), float(q.w))
    yaw = quaternion_to_yaw(*quat) if all(math.isfinite(v) for v in quat) else float("nan")
    return np.array([float(p.x), float(p.y), math.cos(yaw), math.sin(yaw)], dtype=np.float32)


def pose_array_to_start_goal(msg) -> Tuple[Tuple[float, float], Tuple[float, float]]:
    """pose_array_callback (train.py:126-132): start = poses[0], goal = poses[1] (x, y)."""
    s, g = msg.poses[0].position, msg.poses[1].position
    return (float(s.x), float(s.y)), (float(g.x), float(g.y))


def pose_array_to_scenario(start, goal, obstacles=(), cfg=None) -> dict:
    """An episode arriving from outside — the start and goal of /start_goal_points
    (pose_array_callback, train.py:113-132; e.g. pose_array_to_start_goal's pair) plus the discs the
    simulator holds — as the arrays FFMPVec.set_scenarios / FFMP.reset(options={"scenario": ...})
    take, one row each: pose (1, 3), goal (1, 2), obst (1, K, 4), obst_r (1, K), float64.
    start: (x, y) or (x, y, yaw) (yaw 0.0 if absent); goal: (x, y); obstacles: a sequence of
    (x, y, r) or (x, y, r, vx, vy).  cfg (an FFMPConfig): K = cfg.n_obst, the rest padded with parked
    discs as the sampler's (r = 0 at (3 W, 3 W)), ValueError if more than K are given; without cfg,
    K = len(obstacles)."""
    s = [float(v) for v in start]
    g = [float(v) for v in goal]
    if len(s) not in (2, 3) or len(g) != 2:
        raise ValueError("start must be (x, y) or (x, y, yaw) and goal (x, y)")
    discs = []
    for o in obstacles:
        o = [float(v) for v in o]
        if len(o) not in (3, 5):
            raise ValueError("an obstacle must be (x, y, r) or (x, y, r, vx, vy)")
        discs.append(o + [0.0, 0.0] if len(o) == 3 else o)
    K = len(discs) if cfg is None else int(cfg.n_obst)
    if len(discs) > K:
        raise ValueError(f"{len(discs)} obstacles given, the config holds n_obst = {K}")
    park = 0.0 if cfg is None else 3.0 * float(cfg.W)
    obst = np.zeros((1, K, 4), dtype=np.float64)
    obst[0, :, 0:2] = park
    obst_r = np.zeros((1, K), dtype=np.float64)
    for k, (x, y, r, vx, vy) in enumerate(discs):
        obst[0, k] = (x, y, vx, vy)
        obst_r[0, k] = r
    return {"pose": np.array([[s[0], s[1], s[2] if len(s) == 3 else 0.0]], dtype=np.float64),
            "goal": np.array([g], dtype=np.float64), "obst": obst, "obst_r": obst_r}


def _wrap_pi(a: float) -> float:
    """ROSNode.pi_to_pi (train.py:167-172): subtract 2pi while >= pi, then add 2pi while <= -pi
    (so both +pi and -pi end at +pi); iterative on purpose — a remainder differs in the last bits."""
    two_pi = 2 * math.pi
    while a >= math.pi:
        a -= two_pi
    while a <= -math.pi:
        a += two_pi
    return a


def relative_goal(x: float, y: float, yaw: float, goal_x: float, goal_y: float) -> np.ndarray:
    """relative_goal_calculator (train.py:174-180) on a pose (e.g. from odometry_to_pose) and the
    goal of pose_array_to_start_goal: float64 [dist, orientation], the `relative_goal_info` that
    FFMP.rewarder / rewarder2 consume (train.py:536, :577)."""
    dx, dy = goal_x - x, goal_y - y
    return np.array([math.sqrt(dx * dx + dy * dy), _wrap_pi(math.atan2(dy, dx) - yaw)])


def action_to_twist(action: int) -> Msg:
    """cmd_vel_publisher(commander(a)) (train.py:134-143, :668-673)."""
    v, w = action_table()[int(action)]
    return Msg(linear={"x": v, "y": 0.0, "z": 0.0}, angular={"x": 0.0, "y": 0.0, "z": w})


def command_to_twist(v: float, w: float) -> Msg:
    """cmd_vel_publisher (train.py:134-143) for a continuous command: linear.x = v, angular.z = w.
    command_to_twist(*action_table()[a]) is action_to_twist(a), field for field."""
    return Msg(linear={"x": float(v), "y": 0.0, "z": 0.0}, angular={"x": 0.0, "y": 0.0, "z": float(w)})


def twist_to_command(msg) -> Tuple[float, float]:
    """The way back from a /cmd_vel Twist (train.py:134-143 sets only linear.x and angular.z) to the
    (v, w) command FFMPVec.step / FFMP.step take (clipped there to the action Box, ffmp.py:29-32)."""
    return float(msg.linear.x), float(msg.angular.z)


# ----------------------------------------------------------------------------- env -> messages
def lidar_to_ranges(lidar_row: np.ndarray, range_max: float) -> List[float]:
    """One env's lidar (L,) as LaserScan.ranges: no return (+inf) stays inf (dropped by
    laser_callback), a beam starting inside a disc (-inf) becomes 0.0 (also dropped, as
    is_collision2 skips falsy ranges), everything else is the float32 range."""
    r = np.asarray(lidar_row, dtype=np.float32)
    out = np.where(np.isneginf(r), 0.0, r).astype(np.float64)
    out = np.where(out > range_max, np.inf, out)
    return [float(v) for v in out]


def frame_to_image(frame: np.ndarray) -> np.ndarray:
    """One (G, G) occupancy frame (0/255 float) as a mono8 image (H = G rows)."""
    f = np.asarray(frame)
    if f.ndim != 2:
        raise ValueError("frame must be (G, G)")
    return np.clip(f, 0, 255).astype(np.uint8)


def yaw_to_quaternion(yaw: float) -> Tuple[float, float, float, float]:
    """(x, y, z, w) of a rotation by `yaw` about z (tf quaternion_from_euler(0, 0, yaw))."""
    return 0.0, 0.0, math.sin(0.5 * yaw), math.cos(0.5 * yaw)


def pose_to_odometry(x: float, y: float, yaw: float, stamp: float) -> Msg:
    qx, qy, qz, qw = yaw_to_quaternion(yaw)
    secs = int(math.floor(stamp))
    return Msg(header={"stamp": {"secs": secs, "nsecs": int(round((stamp - secs) * 1e9))}},
               pose={"pose": {"position": {"x": x, "y": y, "z": 0.0},
                              "orientation": {"x": qx, "y": qy, "z": qz, "w": qw}}})


def world_map_to_occupancy_grid(log_odds_row: np.ndarray, resolution: float, origin, occ_thr: int = 8, free_thr: int = 4) -> dict:
    """One env's plane of a WorldMap (`log_odds[e]`, (cells, cells) int8, row p world x, column q world
    y) as a plain dict shaped like nav_msgs/OccupancyGrid.  `data` is int8, -1 unknown, 0 free (log-odds
    <= -free_thr), 100 occupied (>= occ_thr), in the row-major order ROS expects, x fastest:
    data[y * width + x] is cell (x, y) — the plane TRANSPOSED and then flattened, since the plane's
    rows are x.  `origin`: WorldMap.origin, the world coordinate of the CENTRE of cell (0, 0) (a scalar
    for both axes, or (x, y)); info.origin.position is the lower-left CORNER of that cell, as ROS defines
    it, half a cell less.  The map's axes are the world's: the orientation is the identity."""
    m = np.asarray(log_odds_row)
    if m.ndim != 2 or m.shape[0] != m.shape[1]:
        raise ValueError("log_odds_row must be (cells, cells)")
    if not 1 <= int(occ_thr) <= 127 or not 1 <= int(free_thr) <= 127:
        raise ValueError("occ_thr and free_thr must be in [1, 127]")
    ox, oy = (origin, origin) if np.ndim(origin) == 0 else origin
    m = m.astype(np.int32)
    val = np.where(m >= int(occ_thr), 100, np.where(m <= -int(free_thr), 0, -1)).astype(np.int8)
    res = float(resolution)
    return {"header": {"frame_id": "map"},
            "info": {"resolution": res, "width": int(m.shape[0]), "height": int(m.shape[1]),
                     "origin": {"position": {"x": float(ox) - 0.5 * res, "y": float(oy) - 0.5 * res, "z": 0.0},
                                "orientation": {"x": 0.0, "y": 0.0, "z": 0.0, "w": 1.0}}},
            "data": np.ascontiguousarray(val.T).reshape(-1)}


def map_to_odom_transform(odom_row, matched_row, stamp: float) -> dict:
    """The `map -> odom` transform of a localisation node as a plain dict shaped like
    geometry_msgs/TransformStamped: the rigid motion that takes the odometry pose `odom_row` to the pose
    `matched_row` that WorldMap.match / the localizer found for the same instant — both rows of four words
    {x, y, cos yaw, sin yaw} (odom_to_pose_row's layout).  yaw = yaw(matched) - yaw(odom), wrapped into
    (-pi, pi]; translation = matched position - R(yaw) odom position; the rotation is yaw_to_quaternion's.
    Composed with the odometry pose it gives the matched pose back; equal rows give the identity."""
    o = np.asarray(odom_row, dtype=np.float64).reshape(-1)
    m = np.asarray(matched_row, dtype=np.float64).reshape(-1)
    if o.shape[0] < 4 or m.shape[0] < 4:
        raise ValueError("odom_row and matched_row must hold the four words {x, y, cos yaw, sin yaw}")
    yaw = _wrap_pi(math.atan2(m[3], m[2]) - math.atan2(o[3], o[2]))
    c, s = math.cos(yaw), math.sin(yaw)
    qx, qy, qz, qw = yaw_to_quaternion(yaw)
    secs = int(math.floor(stamp))
    return {"header": {"stamp": {"secs": secs, "nsecs": int(round((stamp - secs) * 1e9))}, "frame_id": "map"},
            "child_frame_id": "odom",
            "transform": {"translation": {"x": float(m[0] - (c * o[0] - s * o[1])), "y": float(m[1] - (s * o[0] + c * o[1])), "z": 0.0},
                          "rotation": {"x": qx, "y": qy, "z": qz, "w": qw}}}
