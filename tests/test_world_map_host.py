"""The world-fixed scan map, without a GPU: the NumPy restatement (tests/world_map_ref.py, the checker of
tests/test_gpu_world_map.py) has the SPEC's properties (include/ffmp.h ffmp_world_map / ffmp_world_frame,
DESIGN §3 a19e) and remembers what the re-sampled map of tests/lidar_map_ref.py forgets; the four symbols
are declared, bound and exported consistently inside ABI 9, and every argument check answers before any
launch."""
import ctypes as C
import inspect
import math
import re

import numpy as np
import pytest

from flow_field_based_motion_planner_amd import _abi, ros_adapters
from flow_field_based_motion_planner_amd.config import MAX_BEAMS, FFMPConfig
from oracle.ffmp_oracle import Cfg
from tests import lidar_map_ref as M
from tests import scan_map_ref as S
from tests import world_map_ref as W

F32 = np.float32
INF = float("inf")
NAN = float("nan")
G = 64
CONFIG = FFMPConfig(grid=G, n_obst=0, n_beams=0)
CFG = Cfg.from_config(CONFIG)
WC = W.default_cells(CONFIG)  # world_half = G res: 2 G + 8 cells
OFF = (WC - G) // 2           # world cell of ego cell 0 for a robot at the origin with yaw 0


def _pose(x, y, yaw, n=1):
    return np.tile(np.array([[x, y, math.cos(yaw), math.sin(yaw)]], F32), (n, 1))


def _random_map(n, cells=WC, seed=0):
    return np.random.default_rng(seed).integers(-128, 128, (n, cells, cells)).astype(np.int8)


def test_default_cells_and_cell_centres():
    assert WC == 136 and OFF == 36
    assert W.default_cells(FFMPConfig(grid=256, n_obst=0, n_beams=0)) == 520
    assert W.default_cells(FFMPConfig(grid=64, n_obst=0, n_beams=0, world_half=3.0)) == 128
    assert W.default_cells(FFMPConfig(grid=64, n_obst=0, n_beams=0, world_half=3.01)) == 132  # rounded up to a multiple of 4
    assert W.half_of(CFG, WC) == F32(WC * CONFIG.res / 2.0) and W.origin_of(CFG, WC) == -float(F32(3.4))


# ------------------------------------------------------------------ 1. known answers
@pytest.mark.parametrize("yaw", [0.0, 0.7, -2.0])
def test_standing_still_saturates_and_leaves_the_rest(yaw):
    """A ring of hits at 0.8 m seen from a robot that stands still: hit cells reach +l_max after
    ceil(l_max / l_hit) updates and stay, free cells -l_max after ceil(l_max / l_free); a cell beyond range_max,
    or in a cone without data, keeps whatever it held."""
    p = _pose(0.35, -0.6, yaw)
    rows = np.full((1, 90), 0.8, F32)
    rows[0, 10:20] = NAN  # cones without data
    start = _random_map(1, seed=3)
    kn = dict(l_hit=9, l_free=5, l_max=64, decay=0, range_max=1.0)
    one = W.update(CFG, np.zeros_like(start), rows, p, **kn)
    hit, fre = one[0] == 9, one[0] == -5
    assert hit.sum() > 50 and fre.sum() > 200 and ((one[0] == 0) | hit | fre).all()
    m = np.zeros_like(start)
    n_hit, n_free = math.ceil(64 / 9), math.ceil(64 / 5)
    for k in range(1, n_free + 2):
        m = W.update(CFG, m, rows, p, **kn)
        assert (m[0][hit] == min(9 * k, 64)).all() and (m[0][fre] == -min(5 * k, 64)).all()
        assert ((m[0][hit] == 64).all()) == (k >= n_hit) and ((m[0][fre] == -64).all()) == (k >= n_free)
    # the rest of the plane: unchanged, bit for bit, whatever it held — the cells beyond range_max ...
    out = W.update(CFG, start, rows, p, l_hit=9, l_free=5, l_max=127, decay=7, range_max=1.0)
    idx = (np.arange(WC) * F32(CONFIG.res) - W.half_of(CFG, WC)).astype(np.float64)
    d = np.hypot(idx.reshape(WC, 1) - float(p[0, 0]), idx.reshape(1, WC) - float(p[0, 1]))
    far = d > 1.0 + 1e-4
    assert far.mean() > 0.8 and np.array_equal(out[0][far], start[0][far])
    # ... and those in a cone without data; every other cell within range has changed class-wise
    untouched = out[0] == start[0]
    near = d < 0.7
    assert (untouched & near).sum() > 20 and ((~untouched) & near).sum() > 200
    assert (out[0][fre & (start[0] > -100)] == np.clip(start[0][fre & (start[0] > -100)].astype(int) - 5, -127, 127)).all()


def test_decay_mask_first_and_bad_poses():
    p = _pose(0.0, 0.0, 0.4, n=3)
    rows = np.full((3, 90), 0.8, F32)
    one = W.update(CFG, np.zeros((3, WC, WC), np.int8), rows, p, l_hit=1, l_free=1, range_max=1.2)
    hit, fre = one[0] == 1, one[0] == -1
    idx = (np.arange(WC) * F32(CONFIG.res) - W.half_of(CFG, WC)).astype(np.float64)
    d = np.hypot(idx.reshape(WC, 1), idx.reshape(1, WC))
    shell = (d > 0.95) & (d < 1.15)  # known, neither a hit nor free: the decay's cells
    assert not (hit | fre)[shell].any() and shell.sum() > 100
    start = np.zeros((3, WC, WC), np.int8)
    start[:, :, 0::3], start[:, :, 1::3], start[:, :, 2::3] = 5, -2, -128
    out = W.update(CFG, start, rows, p, l_hit=0, l_free=0, l_max=127, decay=3, range_max=1.2)
    exp = np.where(start[0] == 5, 2, np.where(start[0] == -2, 0, -125))
    assert np.array_equal(out[0][shell], exp[shell]) and np.array_equal(out[0][d > 1.3], start[0][d > 1.3])
    # mask 0 keeps every byte, first zeroes the whole plane before the update
    m = _random_map(3, seed=5)
    out = W.update(CFG, m, rows, p, mask=np.array([1, 0, 1]), first=np.array([0, 1, 1]), l_max=127, range_max=1.2)
    assert np.array_equal(out[1], m[1])
    assert (out[2][d > 1.3] == 0).all() and (out[2][hit] == 8).all() and (out[2][fre] == -4).all()
    assert np.array_equal(out[0][d > 1.3], m[0][d > 1.3]) and not np.array_equal(out[0], m[0])
    # a non-finite pose word: the plane as it is — as it is after the zeroing where first is set
    for word, v in ((0, NAN), (1, INF), (2, NAN), (3, -INF)):
        bad = p.copy()
        bad[:, word] = v
        out = W.update(CFG, m, rows, bad, first=np.array([0, 1, 0]), range_max=1.2)
        assert np.array_equal(out[0], m[0]) and (out[1] == 0).all() and np.array_equal(out[2], m[2])
        assert (W.ego_frame(CFG, m, bad, unknown=77) == 77).all()
    # a huge but finite pose: no cell is within range, nothing changes, and the view is all `outside`
    big = p.copy()
    big[:, 0] = 1e30
    assert np.array_equal(W.update(CFG, m, rows, big, range_max=1.2), m)
    assert (W.ego_frame(CFG, m, big, outside=9) == 9).all()


def test_ego_frame_thresholds_and_outside():
    lv = np.zeros((1, WC, WC), np.int8)
    lv[0] = (np.arange(WC) - 68).reshape(1, WC)  # the log-odds of column q is q - 68
    f = W.ego_frame(CFG, lv, _pose(0.0, 0.0, 0.0), unknown=9, outside=200, occ_thr=3, free_thr=5)
    q = np.arange(G) + OFF - 68
    exp = np.where(q >= 3, 255, np.where(q <= -5, 0, 9))
    assert np.array_equal(f[0], np.broadcast_to(exp, (G, G)))
    # the robot near the plane's edge: the part of the window beyond it reads `outside`
    f = W.ego_frame(CFG, lv, _pose(3.0, 0.0, 0.0), unknown=9, outside=200, occ_thr=3, free_thr=5)
    rows_in = np.arange(G) + OFF + 60 <= WC - 1
    assert (f[0][~rows_in] == 200).all() and np.array_equal(f[0][rows_in], np.broadcast_to(exp, (G, G))[rows_in])
    assert 0 < rows_in.sum() < G


# ------------------------------------------------------------------ 2. memory beyond the window
def test_a_wall_is_remembered_beyond_range_and_window():
    """Update 1 sees a wall ahead at 0.8 m; the robot then drives 2.5 m on — the wall is 1.7 m behind it,
    outside range_max (1.0 m) and outside the 3.2 m ego window — and comes back without seeing it again (no
    data in any cone).  The world map still holds the wall's log-odds and ego_frame shows it; the re-sampled
    ego map of tests/lidar_map_ref.py, fed the same sequence, has lost it."""
    L = 90
    wall = np.full((1, L), NAN, F32)
    wall[0, 35:56] = 0.8  # the 21 cones around the bearing 0 (ahead)
    blind = np.full((1, L), NAN, F32)
    here, there = _pose(0.0, 0.0, 0.0), _pose(2.5, 0.0, 0.0)
    kn = dict(l_hit=8, l_free=4, l_max=64, decay=0)
    wm = W.update(CFG, np.zeros((1, WC, WC), np.int8), wall, here, range_max=1.0, first=np.ones(1), **kn)
    lm, lf = M.update(CFG, np.zeros((1, G, G), np.int8), wall, here, here, first=np.ones(1), range_max=1.0, occ_thr=8, free_thr=4, **kn)
    seen = wm[0] == 8
    assert seen.sum() > 20 and (lf == 255).sum() > 20
    f0 = W.ego_frame(CFG, wm, here)
    assert np.array_equal(f0[0] == 255, seen[OFF:OFF + G, OFF:OFF + G]) and (f0 == 255).sum() == seen.sum()
    assert ((f0 == 255) & (lf == 255)).sum() >= 0.9 * (lf == 255).sum()  # the same wall in both maps
    free_there = np.full((1, L), INF, F32)  # at the far end the scan sees free space out to range_max
    wm2 = W.update(CFG, wm, free_there, there, range_max=1.0, **kn)
    lm2, lf2 = M.update(CFG, lm, free_there, there, here, range_max=1.0, occ_thr=8, free_thr=4, **kn)
    assert np.array_equal(wm2[0][seen], wm[0][seen]) and (wm2[0] == -4).sum() > 500  # kept, and the far end mapped
    assert (W.ego_frame(CFG, wm2, there, outside=128) == 255).sum() == 0  # out of the window there
    wm3 = W.update(CFG, wm2, blind, here, range_max=1.0, **kn)
    lm3, lf3 = M.update(CFG, lm2, blind, here, there, range_max=1.0, occ_thr=8, free_thr=4, **kn)
    back = W.ego_frame(CFG, wm3, here)
    assert np.array_equal(back == 255, f0 == 255)  # the wall again, cell for cell
    assert (lf3 == 255).sum() == 0 and (lm3 > 0).sum() == 0  # the ego map has forgotten it


# ------------------------------------------------------------------ 3. the quarter turn of the view
@pytest.mark.parametrize("at", [(0.0, 0.0), (0.5, -0.25), (2.9, 2.9)])
def test_quarter_turn_views_are_rotations_of_each_other(at):
    """(c, s) = (0, 1): wx = -ey + px, wy = ex + py, so ego cell (i, j) of the turned robot is ego cell
    (G - j, i) of the robot with yaw 0 — an exact rotation wherever G - j is inside the window (j >= 1)."""
    m = _random_map(1, seed=11)
    ident = W.ego_frame(CFG, m, np.array([[at[0], at[1], 1.0, 0.0]], F32), outside=200)[0]
    turned = W.ego_frame(CFG, m, np.array([[at[0], at[1], 0.0, 1.0]], F32), outside=200)[0]
    i, j = np.meshgrid(np.arange(G), np.arange(1, G), indexing="ij")
    assert np.array_equal(turned[i, j], ident[G - j, i])
    assert np.array_equal(turned[:, 1:], np.rot90(ident[1:, :], k=-1))
    assert len(np.unique(ident)) >= 3


# ------------------------------------------------------------------ 4. the OccupancyGrid dict
def test_occupancy_grid_dict():
    m = np.zeros((8, 8), np.int8)
    m[1, 2], m[3, 0], m[7, 7], m[0, 5], m[4, 4] = 8, -4, 127, 7, -3
    d = ros_adapters.world_map_to_occupancy_grid(m, 0.05, -0.2, occ_thr=8, free_thr=4)
    assert set(d) == {"header", "info", "data"} and d["header"]["frame_id"] == "map"
    info = d["info"]
    assert info["resolution"] == 0.05 and info["width"] == 8 and info["height"] == 8
    assert info["origin"]["position"] == {"x": pytest.approx(-0.225), "y": pytest.approx(-0.225), "z": 0.0}
    assert info["origin"]["orientation"] == {"x": 0.0, "y": 0.0, "z": 0.0, "w": 1.0}
    data = d["data"]
    assert data.dtype == np.int8 and data.shape == (64,)
    # x fastest: data[y * width + x] is cell (x, y) = plane[x][y] — the transpose of the plane, flattened
    assert data[2 * 8 + 1] == 100 and data[0 * 8 + 3] == 0 and data[7 * 8 + 7] == 100
    assert data[5 * 8 + 0] == -1 and data[4 * 8 + 4] == -1 and (data == -1).sum() == 61
    assert np.array_equal(data.reshape(8, 8), np.where(m.T >= 8, 100, np.where(m.T <= -4, 0, -1)))
    d = ros_adapters.world_map_to_occupancy_grid(m, 0.1, (1.0, -2.0), occ_thr=7, free_thr=3)
    assert d["data"][5 * 8 + 0] == 100 and d["data"][4 * 8 + 4] == 0
    assert d["info"]["origin"]["position"]["x"] == pytest.approx(0.95) and d["info"]["origin"]["position"]["y"] == pytest.approx(-2.05)
    with pytest.raises(ValueError):
        ros_adapters.world_map_to_occupancy_grid(np.zeros((8, 4), np.int8), 0.05, 0.0)
    with pytest.raises(ValueError):
        ros_adapters.world_map_to_occupancy_grid(m, 0.05, 0.0, occ_thr=0)


# ------------------------------------------------------------------ 5. the C surface and its refusals
SIGS = (("ffmp_world_map", 21), ("ffmp_world_map_check", 10), ("ffmp_world_frame", 15), ("ffmp_world_frame_check", 7))


def test_header_binding_and_library_agree(lib):
    h = open(_abi.HEADER_PATH).read()
    assert int(re.search(r"#define FFMP_ABI_VERSION (\d+)", h).group(1)) == 9 == _abi.ABI_VERSION
    code = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    for name, count in SIGS:
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, code)
        assert m, name
        params = [p.strip() for p in m.group(1).split(",")]
        res, args = _abi._SIGS[name]
        assert res is C.c_int and len(args) == len(params) == count, (name, params)
        assert hasattr(lib, name)
    decl = h.index("int ffmp_world_map(")
    comment = h[h.rindex("/*", 0, decl):decl]
    for word in ("[unpinned]", "wh_f = (float)(Wc * res / 2)", "wx = (float)p * res_f - wh_f", "dx = wx - px;  dy = wy - py",
                 "ex = c*dx + s*dy;  ey = c*dy - s*dx", "M unchanged", "clamp(M + l_hit, -l_max, l_max)",
                 "clamp(M - l_free, -l_max, l_max)", "M - sgn(M) * min(|M|, decay)", "superset", "first[e] != 0", "mask[e] == 0",
                 "wx = (c*ex - s*ey) + px;  wy = (s*ex + c*ey) + py", "rintf((wx + wh_f) / res_f)", "a NaN is outside",
                 "!inside ? outside", "overlap"):
        assert word in comment, word
    from flow_field_based_motion_planner_amd import env, vec_env
    sig = inspect.signature(vec_env.FFMPVec.world_map)
    names = ("cells", "unknown", "outside", "thickness", "range_max", "l_hit", "l_free", "l_max", "decay", "occ_thr", "free_thr")
    assert [k for k in sig.parameters][1:] == list(names)
    assert [sig.parameters[k].default for k in names] == [None, 128, 255, None, None, 8, 4, 64, 0, 8, 4]
    sig = inspect.signature(vec_env.WorldMap.update)
    assert [sig.parameters[k].default for k in ("ranges", "pose", "first", "mask", "plain")] == [None, None, None, None, False]
    sig = inspect.signature(vec_env.WorldMap.ego_frame)
    assert [sig.parameters[k].default for k in ("pose", "out")] == [None, None]
    for attr in ("log_odds", "origin", "resolution", "bytes"):
        assert isinstance(getattr(vec_env.WorldMap, attr), property), attr
    assert callable(vec_env.WorldMap.reset) and callable(env.FFMP.world_map)


P = 1 << 24  # never dereferenced: every call below is refused, or has n == 0
W2 = WC * WC
G2 = G * G
KNOBS = dict(l_hit=8, l_free=4, l_max=64, decay=0)


def _update(lib, cfg, n=4, ranges=P, stride=None, L=180, sectors=P, pose=P, pose_stride=16, mask=None, first=None, map_=P,
            map_stride=W2, cells=WC, th=0.05, rm=INF, flags=0, **knobs):
    k = dict(KNOBS, **knobs)
    return lib.ffmp_world_map(C.byref(cfg), n, ranges, L if stride is None else stride, L, sectors, pose, pose_stride, mask, first,
                              map_, map_stride, cells, th, rm, k["l_hit"], k["l_free"], k["l_max"], k["decay"], flags, None)


def _view(lib, cfg, n=4, pose=P, pose_stride=16, map_=P, map_stride=W2, cells=WC, frame=P + (1 << 22), frame_stride=G2, fmt=0,
          unknown=128, outside=255, occ_thr=8, free_thr=4):
    return lib.ffmp_world_frame(C.byref(cfg), n, pose, pose_stride, map_, map_stride, cells, frame, frame_stride, fmt, unknown,
                                outside, occ_thr, free_thr, None)


def test_update_argument_checks_without_a_launch(lib):
    cfg = _abi.make_cfg(FFMPConfig(grid=G, n_obst=4, n_beams=0))
    E = -1  # FFMP_E_ARG
    chk = lambda *a: lib.ffmp_world_map_check(C.byref(cfg), *a)  # noqa: E731
    good = (180, WC, 0.05, INF, 8, 4, 64, 0, 0)
    assert chk(*good) == 0
    knob_cases = [(dict(l_hit=-1), b"l_hit"), (dict(l_hit=128), b"l_hit"), (dict(l_free=-1), b"l_free"), (dict(l_free=128), b"l_free"),
                  (dict(l_max=0), b"l_max"), (dict(l_max=128), b"l_max"), (dict(decay=-1), b"decay"), (dict(decay=128), b"decay")]
    cases = knob_cases + [
        (dict(cells=4, map_stride=1 << 23), b"cells"), (dict(cells=2052, map_stride=1 << 23), b"cells"), (dict(cells=134), b"cells"),
        (dict(cells=0), b"cells"), (dict(L=0), b"n_beams"), (dict(L=MAX_BEAMS + 1), b"n_beams"), (dict(th=NAN), b"thickness"),
        (dict(th=-0.01), b"thickness"), (dict(th=INF), b"thickness"), (dict(rm=NAN), b"range_max"), (dict(rm=0.0), b"range_max"),
        (dict(rm=-1.0), b"range_max"), (dict(flags=2), b"flags"), (dict(flags=-1), b"flags"),
        (dict(ranges=None), b"ranges is NULL"), (dict(sectors=None), b"sectors is NULL"), (dict(pose=None), b"pose is NULL"),
        (dict(map_=None), b"map is NULL"), (dict(stride=179), b"ranges_stride"), (dict(pose_stride=3), b"pose_stride"),
        (dict(map_stride=W2 - 4), b"map_env_stride"), (dict(map_=P + 2), b"map alignment"), (dict(map_=P + 1), b"map alignment"),
        (dict(map_stride=W2 + 2), b"map alignment"), (dict(n=-1), b"negative n"), (dict(n=1 << 40), b"too large"),
        (dict(n=1 << 31, rm=0.5), b"too large"), (dict(n=1 << 30), b"too large")]
    for kw, word in cases:
        assert _update(lib, cfg, **kw) == E, kw
        assert word in lib.ffmp_last_error(), (kw, lib.ffmp_last_error())
        assert lib.ffmp_last_error().startswith(b"ffmp_world_map:")
    for kw, word in knob_cases:
        k = dict(KNOBS, **kw)
        assert chk(180, WC, 0.05, INF, k["l_hit"], k["l_free"], k["l_max"], k["decay"], 0) == E and word in lib.ffmp_last_error()
    assert chk(180, 6, 0.05, INF, 8, 4, 64, 0, 0) == E and b"cells" in lib.ffmp_last_error()
    assert chk(0, WC, 0.05, INF, 8, 4, 64, 0, 0) == E and b"n_beams" in lib.ffmp_last_error()
    assert chk(180, WC, 0.05, INF, 8, 4, 64, 0, 4) == E and b"flags" in lib.ffmp_last_error()
    assert lib.ffmp_world_map_check(None, *good) == E and b"cfg is NULL" in lib.ffmp_last_error()
    assert lib.ffmp_world_map(None, 0, P, 180, 180, P, P, 4, None, None, P, W2, WC, 0.05, INF, 8, 4, 64, 0, 0, None) == E
    bad = _abi.make_cfg(FFMPConfig(grid=G, n_obst=4, n_beams=0))
    bad.res_f = 0.0
    assert _update(lib, bad) == E and b"res_f" in lib.ffmp_last_error()
    # the bounds themselves pass the checks: n == 0 launches nothing
    for kw in (dict(l_hit=0, l_free=0, decay=0), dict(l_hit=127, l_free=127, l_max=127, decay=127), dict(l_max=1), dict(flags=1),
               dict(mask=P), dict(first=P), dict(pose_stride=4), dict(stride=1000), dict(L=1), dict(L=MAX_BEAMS), dict(map_=P + 4),
               dict(map_stride=W2 + 4), dict(th=0.0), dict(rm=1e-3), dict(rm=1e30), dict(cells=8), dict(cells=2048, map_stride=1 << 22)):
        assert _update(lib, cfg, n=0, **kw) == 0, (kw, lib.ffmp_last_error())


def test_view_argument_checks_without_a_launch(lib):
    cfg = _abi.make_cfg(FFMPConfig(grid=G, n_obst=4, n_beams=0))
    E = -1
    chk = lambda *a: lib.ffmp_world_frame_check(C.byref(cfg), *a)  # noqa: E731
    assert chk(WC, 0, 128, 255, 8, 4) == 0 and chk(WC, 1, 0, 0, 1, 127) == 0
    knob_cases = [(dict(fmt=2), b"format"), (dict(fmt=-1), b"format"), (dict(unknown=-1), b"unknown"), (dict(unknown=256), b"unknown"),
                  (dict(outside=-1), b"outside"), (dict(outside=256), b"outside"), (dict(occ_thr=0), b"occ_thr"),
                  (dict(occ_thr=128), b"occ_thr"), (dict(free_thr=0), b"free_thr"), (dict(free_thr=128), b"free_thr"),
                  (dict(cells=4), b"cells"), (dict(cells=2052), b"cells"), (dict(cells=134), b"cells")]
    big = dict(map_stride=1 << 23, frame=P + (1 << 28))
    cases = [(dict(big, **kw), word) for kw, word in knob_cases] + [
        (dict(pose=None), b"pose is NULL"), (dict(map_=None), b"map is NULL"), (dict(frame=None), b"frame_out is NULL"),
        (dict(pose_stride=3), b"pose_stride"), (dict(map_stride=W2 - 4), b"map_env_stride"), (dict(frame_stride=G2 - 4), b"frame_env_stride"),
        (dict(frame=P + (1 << 22) + 4), b"frame alignment"), (dict(frame=P + (1 << 22) + 2, fmt=1), b"frame alignment"),
        (dict(frame_stride=G2 + 2), b"frame alignment"),
        # a frame whose bytes meet the map's: at its start, inside it, one byte into its end, and the map inside the frames
        (dict(frame=P), b"overlap"), (dict(frame=P + 4 * W2 - 16), b"overlap"), (dict(frame=P - 16 * G2 + 16), b"overlap"),
        (dict(frame=P + W2, fmt=1), b"overlap"), (dict(frame=P - 4 * G2 + 4, fmt=1), b"overlap"),
        (dict(n=-1), b"negative n"), (dict(n=1 << 40), b"too large"), (dict(n=1 << 31), b"too large")]
    for kw, word in cases:
        assert _view(lib, cfg, **kw) == E, kw
        assert word in lib.ffmp_last_error(), (kw, lib.ffmp_last_error())
        assert lib.ffmp_last_error().startswith(b"ffmp_world_frame:")
    for kw, word in knob_cases:
        k = dict(cells=WC, fmt=0, unknown=128, outside=255, occ_thr=8, free_thr=4)
        k.update(kw)
        assert chk(k["cells"], k["fmt"], k["unknown"], k["outside"], k["occ_thr"], k["free_thr"]) == E and word in lib.ffmp_last_error()
    for g in (4, 4100, 66, 0):
        bad = _abi.make_cfg(FFMPConfig(grid=G, n_obst=4, n_beams=0))
        bad.grid = g
        assert _view(lib, bad, frame_stride=1 << 30, frame=P + (1 << 28)) == E and b"grid" in lib.ffmp_last_error(), g
        assert lib.ffmp_world_frame_check(C.byref(bad), WC, 0, 128, 255, 8, 4) == E and b"grid" in lib.ffmp_last_error()
    assert lib.ffmp_world_frame_check(None, WC, 0, 128, 255, 8, 4) == E and b"cfg is NULL" in lib.ffmp_last_error()
    wide = _abi.make_cfg(FFMPConfig(grid=256, n_obst=4, n_beams=0))  # 4 blocks per env: n * 4 passes 2^31 before n does
    assert _view(lib, wide, n=(1 << 31) - 1, frame_stride=256 * 256, frame=P + (1 << 40)) == E and b"too large" in lib.ffmp_last_error()
    # the bounds themselves pass the checks: n == 0 launches nothing
    for kw in (dict(n=0, frame=P + 4 * W2), dict(n=0, frame=P - 16 * G2), dict(n=0, frame=P + 4 * W2, fmt=1), dict(n=0, frame=P),
               dict(n=0, unknown=0, outside=0, occ_thr=1, free_thr=1), dict(n=0, occ_thr=127, free_thr=127), dict(n=0, pose_stride=4),
               dict(n=0, frame_stride=G2 + 4), dict(n=0, map_stride=W2 + 4), dict(n=0, cells=8), dict(n=0, cells=2048, map_stride=1 << 22)):
        assert _view(lib, cfg, **kw) == 0, (kw, lib.ffmp_last_error())


def test_the_classification_is_the_scan_frames_one():
    """tests/world_map_ref.classes at the ego grid's own cell coordinates is tests/scan_map_ref.scan_frame."""
    rng = np.random.default_rng(4)
    rows = rng.uniform(0.2, 1.5, (3, 90)).astype(F32)
    rows[rng.integers(0, 8, rows.shape) == 0] = INF
    rows[rng.integers(0, 8, rows.shape) == 0] = NAN
    rows[rng.integers(0, 8, rows.shape) == 0] = -1.0
    from flow_field_based_motion_planner_amd.config import sector_table
    from oracle.ffmp_oracle import cell_coords
    co = cell_coords(CFG, np.arange(G)).astype(F32)
    ex = np.broadcast_to(co.reshape(1, G, 1), (3, G, G))
    ey = np.broadcast_to(co.reshape(1, 1, G), (3, G, G))
    for th, rm in ((None, INF), (0.12, 1.0), (0.0, 0.7)):
        known, free, occ = W.classes(ex, ey, rows, sector_table(90), CFG.f["res_f"] if th is None else th, rm)
        val = np.where(~known, 128, np.where(free, 0, np.where(occ, 255, 128)))
        assert np.array_equal(val, S.scan_frame(CFG, rows, 128, th, rm))
