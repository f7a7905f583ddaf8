"""Frames built from the lidar scan, without a GPU: ffmp_scan_frames / ffmp_scan_frames_check are
declared, bound and exported consistently inside ABI 9; every argument check answers before any
launch; config.sector_table and ros_adapters.scan_to_lidar_row do what the SPEC (include/ffmp.h,
DESIGN §3 a19b) says; and the NumPy restatement (tests/scan_map_ref.py, the checker of
tests/test_gpu_scan_map.py) has the SPEC's properties and is tied to the oracle's ground truth."""
import ctypes as C
import inspect
import math
import re

import numpy as np
import pytest

from flow_field_based_motion_planner_amd import _abi, ros_adapters
from flow_field_based_motion_planner_amd.config import MAX_BEAMS, FFMPConfig, beam_table, sector_table
from oracle.ffmp_oracle import Cfg, cell_coords
from tests import scan_map_ref as S

SYMBOLS = ("ffmp_scan_frames", "ffmp_scan_frames_check")
INF = float("inf")
NAN = float("nan")


def test_header_binding_and_library_agree(lib):
    h = open(_abi.HEADER_PATH).read()
    assert int(re.search(r"#define FFMP_ABI_VERSION (\d+)", h).group(1)) == 9 == _abi.ABI_VERSION
    assert lib.ffmp_abi_version() == 9
    code = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    for name in SYMBOLS:
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, code)
        assert m, name
        params = [p.strip() for p in m.group(1).split(",")]
        res, args = _abi._SIGS[name]
        assert res is C.c_int and len(args) == len(params), (name, params)
        assert hasattr(lib, name)
    assert int(re.search(r"#define FFMP_SCAN_PLAIN (\d+)", h).group(1)) == _abi.SCAN_PLAIN
    decl = h.index("int ffmp_scan_frames(")
    comment = h[h.rindex("/*", 0, decl):decl]
    for word in ("[unpinned]", "c0 >= 0 ? (0, H) : (H - 1, L)", "mid = (lo + hi) >> 1", "known = (b <= mm) && (r > 0)",
                 "free  = (lo_r > 0) && (b < lo_r*lo_r)", "occ   = b <= hi_r*hi_r", "left to right", "(m - 1/2)*2pi/L"):
        assert word in comment, word
    # no struct changed
    assert len(_abi.StateT._fields_) == 11 and len(_abi.ObsT._fields_) == 12 and len(_abi.OutT._fields_) == 5
    assert len(_abi.CfgT._fields_) == 37 and len(_abi.ObsTagsT._fields_) == 3
    _abi.verify_layout(lib)


def _call(lib, cfg, p, n=4, ranges="p", stride=None, L=180, sectors="p", mask=None, first=None, older="p", newest="q",
          env_stride=None, fmt=0, unknown=128, th=0.05, rm=INF, flags=0):
    """older defaults to p, newest to one plane above it (stride 2 G*G): the contiguous (n, 2, G, G) block."""
    G2 = cfg.grid * cfg.grid
    es = 4 if fmt == 0 else 1
    pick = lambda v: p if v == "p" else (p + G2 * es if v == "q" else v)  # noqa: E731
    return lib.ffmp_scan_frames(C.byref(cfg), n, pick(ranges), L if stride is None else stride, L, pick(sectors), mask, first,
                                pick(older), pick(newest), 2 * G2 if env_stride is None else env_stride, fmt, unknown, th, rm,
                                flags, None)


def test_argument_checks_without_a_launch(lib):
    cfg = _abi.make_cfg(FFMPConfig(grid=64, n_obst=4, n_beams=0))
    G2 = 64 * 64
    p = 1 << 20  # never dereferenced: every call below is refused, or has n == 0
    E = -1  # FFMP_E_ARG
    for g in (4, 4100, 66, 0):  # outside 8..4096, or not a multiple of 4
        bad = _abi.make_cfg(FFMPConfig(grid=64, n_obst=4, n_beams=0))
        bad.grid = g
        assert _call(lib, bad, p, env_stride=1 << 30) == E and b"grid" in lib.ffmp_last_error(), g
        assert lib.ffmp_scan_frames_check(C.byref(bad), 180, 0, 128, 0.05, INF, 0) == E and b"grid" in lib.ffmp_last_error()
    for kw, word in ((dict(L=0), b"n_beams"), (dict(L=-3), b"n_beams"), (dict(L=MAX_BEAMS + 1), b"n_beams"),
                     (dict(fmt=2), b"format"), (dict(fmt=-1), b"format"), (dict(unknown=-1), b"unknown"),
                     (dict(unknown=256), b"unknown"), (dict(th=NAN), b"thickness"), (dict(th=-0.01), b"thickness"),
                     (dict(th=INF), b"thickness"), (dict(rm=NAN), b"range_max"), (dict(rm=0.0), b"range_max"),
                     (dict(rm=-1.0), b"range_max"), (dict(rm=-INF), b"range_max"), (dict(flags=2), b"flags"),
                     (dict(flags=-1), b"flags"), (dict(ranges=None), b"ranges is NULL"), (dict(sectors=None), b"sectors is NULL"),
                     (dict(stride=179), b"ranges_stride"), (dict(older=None, newest=None), b"both NULL"),
                     (dict(env_stride=G2 - 4, newest=None), b"out_env_stride"),
                     (dict(older=p + 4), b"alignment"), (dict(newest=p + 4 * G2 + 8), b"alignment"),
                     (dict(older=p + 2, fmt=1), b"alignment"), (dict(env_stride=2 * G2 + 2), b"alignment"),
                     (dict(env_stride=2 * G2 + 1, fmt=1), b"alignment"),
                     # the two planes closer than G*G elements, either way round, and across envs
                     (dict(newest="p"), b"overlap"), (dict(newest=p + 4 * (G2 - 4)), b"overlap"),
                     (dict(older=p + 4 * (G2 - 4), newest="p"), b"overlap"), (dict(newest=p + G2 - 4, fmt=1), b"overlap"),
                     (dict(env_stride=G2), b"overlap"), (dict(env_stride=2 * G2 - 4), b"overlap"),
                     (dict(newest=p + 4 * (3 * G2 + 8), env_stride=2 * G2 + 16), b"overlap"),
                     (dict(n=-1), b"negative n"), (dict(n=1 << 40), b"too large")):
        assert _call(lib, cfg, p, **kw) == E, kw
        assert word in lib.ffmp_last_error(), (kw, lib.ffmp_last_error())
        assert lib.ffmp_last_error().startswith(b"ffmp_scan_frames:")
    assert lib.ffmp_scan_frames(None, 0, p, 180, 180, p, None, None, p, p + 4 * G2, 2 * G2, 0, 128, 0.05, INF, 0, None) == E
    # the bounds themselves pass the checks: n == 0 launches nothing
    for kw in (dict(unknown=0), dict(unknown=255), dict(th=0.0), dict(rm=1e-3), dict(rm=INF), dict(flags=1), dict(older=None),
               dict(newest=None), dict(fmt=1), dict(older=p + 4, newest=p + 4 + G2, fmt=1), dict(env_stride=2 * G2 + 4),
               dict(mask=p), dict(first=p), dict(stride=1000), dict(L=1), dict(L=MAX_BEAMS), dict(env_stride=G2, newest=None),
               # a slot-major pair: the planes of one frame side by side, the other frame after all of them
               dict(newest=p + 4 * 4 * G2, env_stride=G2), dict(older=p + 4 * 4 * G2, newest="p", env_stride=G2)):
        assert _call(lib, cfg, p, n=0, **kw) == 0, (kw, lib.ffmp_last_error())
    # ... which n = 4 envs fill exactly and n = 5 would overrun (refused before any launch)
    assert _call(lib, cfg, p, n=5, newest=p + 4 * 4 * G2, env_stride=G2) == E and b"overlap" in lib.ffmp_last_error()
    for g, beams in ((8, 1), (100, 360), (4096, 1024)):
        ok = _abi.make_cfg(FFMPConfig(grid=g, n_obst=1, n_beams=0))
        assert _call(lib, ok, p, n=0, L=beams) == 0
        assert lib.ffmp_scan_frames_check(C.byref(ok), beams, 0, 128, 0.05, INF, 0) == 0
        assert lib.ffmp_scan_frames_check(C.byref(ok), beams, 1, 0, 0.0, 2.5, 1) == 0
    chk = lambda *a: lib.ffmp_scan_frames_check(C.byref(cfg), *a)  # noqa: E731
    assert chk(180, 2, 128, 0.05, INF, 0) == E and b"format" in lib.ffmp_last_error()
    assert chk(0, 0, 128, 0.05, INF, 0) == E and b"n_beams" in lib.ffmp_last_error()
    assert chk(180, 0, 300, 0.05, INF, 0) == E and chk(180, 0, 128, -1.0, INF, 0) == E and chk(180, 0, 128, 0.05, 0.0, 0) == E
    assert chk(180, 0, 128, 0.05, INF, 4) == E and b"flags" in lib.ffmp_last_error()
    assert lib.ffmp_scan_frames_check(None, 180, 0, 128, 0.05, INF, 0) == E


def test_python_surface_names_the_feature():
    from flow_field_based_motion_planner_amd import env, vec_env
    sig = inspect.signature(vec_env.FFMPVec.lidar_frames)
    names = ("out", "unknown", "thickness", "range_max", "newest_only", "shift", "ranges", "mask", "plain")
    assert [sig.parameters[k].default for k in names] == [None, 128, None, None, False, True, None, None, False]
    assert callable(env.FFMP.lidar_frames)
    for fn in (vec_env.FFMPVec.nav_field, vec_env.FFMPVec.policy_nav):
        ps = inspect.signature(fn).parameters
        assert ps["lidar"].default is False and ps["visible"].default is False and ps["frames"].default is None
    sig = inspect.signature(ros_adapters.scan_to_lidar_row)
    assert [sig.parameters[k].default for k in ("angle_min", "angle_increment", "range_min", "range_max")] == [None, None, 0.0, INF]


# ------------------------------------------------------------------ the sector table and the search
LS = (1, 2, 7, 45, 180, 360, 1023, 1024)


def test_sector_table():
    for L in LS:
        u = sector_table(L)
        assert u.dtype == np.float32 and u.shape == (L, 2)
        for m in (0, L // 2, L - 1):
            a = -math.pi + (m - 0.5) * (2.0 * math.pi / L)
            assert u[m, 0] == np.float32(math.cos(a)) and u[m, 1] == np.float32(math.sin(a))
        # beam m (config.beam_table) is the axis of cone m: half a step past boundary m
        if L > 2:
            bt = beam_table(L)
            cross = u[:, 0].astype(np.float64) * bt[:, 1] - u[:, 1].astype(np.float64) * bt[:, 0]
            assert np.allclose(cross, math.sin(math.pi / L), atol=1e-6)
    assert sector_table(0).shape == (0, 2)


@pytest.mark.parametrize("G", [8, 64, 100])
def test_sectors_agree_with_atan2_away_from_the_boundaries(G):
    cfg = Cfg.from_config(FFMPConfig(grid=G, n_obst=0, n_beams=0))
    for L in LS:
        got = S.sectors_of(cfg, sector_table(L))
        assert got.min() >= 0 and got.max() <= L - 1
        sec, d = S.atan2_sectors(cfg, L)
        clear = d > 1e-4
        assert clear.sum() >= 0.75 * G * G  # the check is about nearly every cell
        assert np.array_equal(got[clear], sec[clear]), (G, L, int((got != sec)[clear].sum()))
    if G == 64:  # the procedure is the definition: on the boundaries the two differ
        assert (S.sectors_of(cfg, sector_table(180)) != S.atan2_sectors(cfg, 180)[0]).sum() > 0


# ------------------------------------------------------------------ the restatement's properties
def _b(cfg):
    c = cell_coords(cfg, np.arange(cfg.grid)).astype(np.float32)
    ex, ey = c.reshape(-1, 1), c.reshape(1, -1)
    return ex * ex + ey * ey


@pytest.mark.parametrize("L", [1, 7, 180])
def test_empty_and_dead_scans(L):
    cfg = Cfg.from_config(FFMPConfig(grid=64, n_obst=0, n_beams=0))
    b = _b(cfg)
    # nothing in range: a free disc of radius range_max, unknown outside it
    rm = 1.0
    got = S.scan_frame(cfg, np.full((1, L), np.inf, np.float32), unknown=77, range_max=rm)[0]
    disc = b <= np.float32(rm) * np.float32(rm)
    assert disc.any() and not disc.all()
    assert (got[disc] == 0).all() and (got[~disc] == 77).all()
    assert (S.scan_frame(cfg, np.full((1, L), np.inf, np.float32), unknown=77)[0] == 0).all()  # range_max = inf
    # no data at all
    for dead in (NAN, 0.0, -INF, -1.0):
        got = S.scan_frame(cfg, np.full((1, L), dead, np.float32), unknown=77, range_max=rm)
        assert (got == 77).all(), dead


def test_thickness_and_the_three_values():
    cfg = Cfg.from_config(FFMPConfig(grid=64, n_obst=0, n_beams=0))
    b = _b(cfg)
    L = 90
    # r < th: no free cell in that cone, the hit's disc reaches the origin
    rows = np.full((1, L), 0.03, np.float32)
    got = S.scan_frame(cfg, rows, thickness=0.05)[0]
    assert (got != 0).all() and got[32, 32] == 255 and (got == 128).any()
    # one cone with r < th among long ones
    rows = np.full((1, L), 1.0, np.float32)
    rows[0, 17] = 0.04
    lo = S.sectors_of(cfg, sector_table(L))
    got = S.scan_frame(cfg, rows, thickness=0.05)[0]
    assert (lo == 17).sum() > 5 and (got[lo == 17] != 0).all() and (got[lo != 17] == 0).any()
    # a ring: free inside r - th, occupied within th of r, unknown beyond (float32 comparisons on b)
    r, th = np.float32(0.8), np.float32(0.1)
    got = S.scan_frame(cfg, np.full((1, L), r, np.float32), thickness=th)[0]
    free = b < (r - th) * (r - th)
    occ = ~free & (b <= (r + th) * (r + th))
    assert np.array_equal(got == 0, free) and np.array_equal(got == 255, occ) and np.array_equal(got == 128, ~free & ~occ)
    assert free.sum() > 100 and occ.sum() > 100 and (~free & ~occ).sum() > 100
    # thickness 0: only cells exactly at the range are occupied
    got0 = S.scan_frame(cfg, np.full((1, L), r, np.float32), thickness=0.0)[0]
    assert np.array_equal(got0 == 0, b < r * r) and np.array_equal(got0 == 255, b == r * r)
    # unknown only recolours
    for u in (0, 255):
        other = S.scan_frame(cfg, np.full((1, L), r, np.float32), unknown=u, thickness=th)[0]
        assert np.array_equal(other[got != 128], got[got != 128]) and (other[got == 128] == u).all()


def test_a_beam_paints_its_own_cone():
    """Beam l's range lands on the cells about bearing -pi + l 2pi/L — in the raster's frame, cell (i, j)
    at (ex, ey) = (i, j) * res - half: a hit straight ahead (+x, beam L/2) is in the rows above the centre."""
    cfg = Cfg.from_config(FFMPConfig(grid=64, n_obst=0, n_beams=0))
    L, c = 180, 32
    for l, (di, dj) in ((90, (1, 0)), (135, (0, 1)), (45, (0, -1)), (0, (-1, 0))):
        rows = np.full((1, L), np.inf, np.float32)
        rows[0, l] = 0.5  # 10 cells
        got = S.scan_frame(cfg, rows, thickness=0.05)[0]
        assert got[c + 10 * di, c + 10 * dj] == 255 and got[c + 5 * di, c + 5 * dj] == 0
        assert got[c + 14 * di, c + 14 * dj] == 128 and got[c - 10 * di, c - 10 * dj] == 0
        assert (got == 255).sum() <= 4


# ------------------------------------------------------------------ ros_adapters.scan_to_lidar_row
def test_scan_to_lidar_row_round_trip():
    L = 180
    config, env = S.oracle_state(64, n=5)
    rm = config.lidar_range
    for row in env.lidar:
        back = ros_adapters.scan_to_lidar_row(ros_adapters.lidar_to_ranges(row, rm), L, -math.pi, 2 * math.pi / L)
        assert back.dtype == np.float32 and back.shape == (L,)
        assert np.array_equal(back, row.astype(np.float32), equal_nan=True)
    assert np.isfinite(env.lidar).any() and np.isposinf(env.lidar).any()
    row = np.array([0.5, -INF, INF, 1.25, -INF, 2.0], np.float32)  # -inf (inside a disc) is published as 0.0: no data
    back = ros_adapters.scan_to_lidar_row(ros_adapters.lidar_to_ranges(row, 3.0), 6, -math.pi, 2 * math.pi / 6)
    assert np.array_equal(back, np.array([0.5, NAN, INF, 1.25, NAN, 2.0], np.float32), equal_nan=True)
    # a bare sequence defaults to the full circle from -pi
    assert np.array_equal(ros_adapters.scan_to_lidar_row([0.5, 0.0, INF, 1.25, 0.0, 2.0], 6), back, equal_nan=True)


def test_scan_to_lidar_row_partial_and_odd_scans():
    # 270 degrees, 1081 rays (an odd count), as a message: the rear quarter has no ray
    k = 1081
    amin, inc = -0.75 * math.pi, 1.5 * math.pi / (k - 1)
    ang = amin + np.arange(k) * inc
    rng = 1.0 + 0.5 * np.cos(3 * ang)
    msg = ros_adapters.Msg(ranges=list(rng), angle_min=amin, angle_increment=inc, range_min=0.1, range_max=30.0)
    L = 180
    row = ros_adapters.scan_to_lidar_row(msg, L)
    beams = -math.pi + np.arange(L) * 2 * math.pi / L
    inside = np.abs(beams) <= 0.75 * math.pi - 1e-9
    outside = np.abs(beams) > 0.75 * math.pi + math.pi / L
    assert np.isnan(row[outside]).all() and outside.sum() >= 40 and np.isfinite(row[inside]).all()
    # several rays per cone: the nearest; it is within the cone's spread of the curve at the beam's angle
    assert np.abs(row[inside] - (1.0 + 0.5 * np.cos(3 * beams[inside]))).max() < 1.5 * (math.pi / L) * 1.01
    for l in (60, 90, 133):
        mine = np.floor((ang + math.pi) / (2 * math.pi / L) + 0.5).astype(int) % L == l
        assert mine.sum() >= 4 and row[l] == np.float32(rng[mine].min())
    # range_min / range_max: below -> NaN, above -> +inf; a finite ray beats an inf one, an inf one a dead one
    vals = [0.05, 0.5, 40.0, NAN, 2.0, INF, 0.0, 40.0, 1.5, 0.02]
    row = ros_adapters.scan_to_lidar_row(vals, 5, range_min=0.1, range_max=30.0)  # 10 rays: cones get (0, 9), (1, 2), ...
    #   cone 0: rays 0 (dead), 1?  ray k at -pi + k*2pi/10 falls in cone floor(k/2 + 0.5) % 5
    cones = [int(math.floor(k / 2 + 0.5)) % 5 for k in range(10)]
    assert cones == [0, 1, 1, 2, 2, 3, 3, 4, 4, 0]
    assert np.array_equal(row, np.array([NAN, 0.5, 2.0, INF, 1.5], np.float32), equal_nan=True)
    # wrapped angles: a scan that runs 0 .. 2 pi lands on the same beams as -pi .. pi
    a = ros_adapters.scan_to_lidar_row(np.arange(1, 9, dtype=float), 8, angle_min=-math.pi, angle_increment=math.pi / 4)
    bb = ros_adapters.scan_to_lidar_row(np.roll(np.arange(1, 9, dtype=float), -4), 8, angle_min=0.0, angle_increment=math.pi / 4)
    assert np.array_equal(a, bb) and np.array_equal(a, np.arange(1, 9, dtype=np.float32))
    # fewer rays than beams: the cones between them hold no data
    sparse = ros_adapters.scan_to_lidar_row([1.0, 2.0, 3.0], 12)
    assert np.isfinite(sparse).sum() == 3 and np.isnan(sparse).sum() == 9 and sparse[0] == 1.0 and sparse[4] == 2.0


# ------------------------------------------------------------------ the physical tie to the oracle
@pytest.mark.parametrize("G", [64, 100])
def test_the_map_agrees_with_the_ground_truth(G):
    """OracleVecEnv, n = 65, 4 steps of default_rng(1) actions on LIVE[G] with 180 / 360 beams: the map of
    the env's own scan against state_m's newest frame.  A transposed or mirrored map fails the 1 % cap by
    a factor of twenty, so a frame-convention error that ref and kernel could share cannot pass."""
    config, env = S.oracle_state(G)
    assert config.n_beams == {64: 180, 100: 360}[G] and env.n == 65
    scan = S.from_config(config, env.lidar)
    truth = env.state_m[:, 1]
    S.assert_preconditions(scan, truth, f"LIVE[{G}]")
    for other in (scan.transpose(0, 2, 1), scan[:, :, ::-1], scan[:, ::-1]):
        _, _, nfree, bad, _, _ = S.truth_stats(np.ascontiguousarray(other), truth)
        assert bad > 0.1 * nfree
