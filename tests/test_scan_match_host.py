"""Scan-to-map matching, without a GPU: the NumPy restatement (tests/scan_match_ref.py, the checker of
tests/test_gpu_scan_match.py) has the SPEC's known answers (include/ffmp.h ffmp_scan_match);
the two symbols are declared, bound and exported consistently inside ABI 9; every argument check answers
before any launch; and the physical tie: on the oracle's scans the matcher recovers a displaced pose and holds
a drifting odometry to the map (DESIGN §10.12 — the figures asserted are the restatement's, never the kernel's)."""
import ctypes as C
import inspect
import math
import re
import warnings

import numpy as np
import pytest

from flow_field_based_motion_planner_amd import _abi, config as config_mod
from flow_field_based_motion_planner_amd.config import MAX_BEAMS, FFMPConfig
from oracle.ffmp_oracle import Cfg
from tests import scan_match_ref as R
from tests import world_map_ref as W

F32 = np.float32
INF = float("inf")
NAN = float("nan")
G = 64
CONFIG = FFMPConfig(grid=G, n_obst=0, n_beams=0)
CFG = Cfg.from_config(CONFIG)
WC = W.default_cells(CONFIG)  # 136
RES = float(CONFIG.res)


def _pose(x, y, yaw, n=1):
    return np.tile(np.array([[x, y, math.cos(yaw), math.sin(yaw)]], F32), (n, 1))


def _room_scan(x, y, yaw, L=180, half=1.0):
    """Ranges (1, L) float32 of a robot at (x, y, yaw) inside the square room |wx|, |wy| <= half."""
    b = config_mod.beam_table(L)
    th = np.arctan2(b[:, 1], b[:, 0]) + yaw
    dx, dy = np.cos(th), np.sin(th)
    with np.errstate(divide="ignore"):
        tx = np.where(dx > 0, (half - x) / dx, np.where(dx < 0, (-half - x) / dx, np.inf))
        ty = np.where(dy > 0, (half - y) / dy, np.where(dy < 0, (-half - y) / dy, np.inf))
    return np.minimum(tx, ty).astype(F32).reshape(1, L)


def test_tables():
    assert np.array_equal(config_mod.beam_dirs(180), R.beam_dirs(180)) and config_mod.beam_dirs(7).dtype == F32
    assert np.array_equal(config_mod.beam_dirs(180), config_mod.beam_table(180).astype(F32))
    t = config_mod.turn_table(4, 0.0125)
    assert t.shape == (9, 2) and t.dtype == F32 and np.array_equal(t, R.turn_table(4, 0.0125))
    assert tuple(t[4]) == (1.0, 0.0) and t[5, 1] == F32(math.sin(0.0125)) and t[3, 1] == -t[5, 1] and t[0, 0] == F32(math.cos(0.05))
    assert config_mod.turn_table(0, 0.3).tolist() == [[1.0, 0.0]]
    with pytest.raises(ValueError):
        config_mod.turn_table(-1, 0.1)


# ------------------------------------------------------------------ 1. known answers
def test_an_empty_map_keeps_the_prior_bit_for_bit():
    rows = _room_scan(0.0, 0.0, 0.0).repeat(2, axis=0)
    pose = np.array([[0.3, -0.2, 0.6, 0.8], [-0.0, 0.25, -0.0, 1.0]], F32)
    out, info, vol = R.match(CFG, np.zeros((2, WC, WC), np.int8), rows, pose, 3, 2, 0.02)
    assert (vol == 0).all() and vol.shape == (2, 5, 7, 7)
    assert np.array_equal(info, np.array([[0, 0, 0, 0, 0, 0, 180, 0]] * 2))
    assert np.array_equal(out.view(np.uint32), pose.view(np.uint32))
    assert np.signbit(out[1, 0]) and np.signbit(out[1, 2])


def test_whole_cell_shifts_are_recovered():
    """A map from one scan of a room with its walls in range; the same scan matched from the pose moved by every
    whole-cell (a, b), |a|, |b| <= R - 1, with T = 0, finds (-a, -b) within one cell."""
    Rr = 4
    x, y, yaw = 0.12, -0.07, 0.3
    rows = _room_scan(x, y, yaw)
    p = _pose(x, y, yaw)
    m = W.update(CFG, np.zeros((1, WC, WC), np.int8), rows, p, first=np.ones(1), range_max=2.0)
    assert (m == 8).sum() > 100 and (m == -4).sum() > 1000
    sh = np.arange(-(Rr - 1), Rr)
    aa, bb = (v.ravel() for v in np.meshgrid(sh, sh, indexing="ij"))
    n = aa.size
    moved = np.tile(p, (n, 1))
    moved[:, 0] = p[0, 0] + (aa * RES).astype(F32)
    moved[:, 1] = p[0, 1] + (bb * RES).astype(F32)
    out, info, vol = R.match(CFG, np.tile(m, (n, 1, 1)), np.tile(rows, (n, 1)), moved, Rr, 0, 0.0, 2.0)
    assert np.abs(info[:, 2] + aa).max() <= 1 and np.abs(info[:, 3] + bb).max() <= 1 and (info[:, 1] == 0).all()
    exact = (info[:, 2] == -aa) & (info[:, 3] == -bb)
    assert exact.mean() >= 0.8
    moving = (aa != 0) | (bb != 0)
    assert (info[moving & exact, 0] == 1).all() and info[~moving, 0].tolist() == [0]
    assert (info[:, 4] >= info[:, 5]).all() and (info[:, 6] == 180).all()
    # status 1: the pose moved by whole cells, (c, s) the prior's at T = 0; status 0: the prior's bits
    ok = info[:, 0] == 1
    assert np.array_equal(out[ok, 0], moved[ok, 0] + info[ok, 2].astype(F32) * F32(CFG.f["res_f"]))
    assert np.array_equal(out[ok, 1], moved[ok, 1] + info[ok, 3].astype(F32) * F32(CFG.f["res_f"]))
    assert np.array_equal(out[ok, 2:], moved[ok, 2:]) and np.array_equal(out[~ok].view(np.uint32), moved[~ok].view(np.uint32))
    # a rotation is found too: the pose turned by two steps comes back by two steps
    turned = _pose(x, y, yaw + 2 * 0.02)
    out, info, _ = R.match(CFG, m, rows, turned, 1, 3, 0.02, 2.0)
    assert info[0, 0] == 1 and abs(info[0, 1] + 2) <= 1 and abs(info[0, 2]) <= 1 and abs(info[0, 3]) <= 1
    t = R.turn_table(3, 0.02)[info[0, 1] + 3]
    assert out[0, 2] == turned[0, 2] * t[0] - turned[0, 3] * t[1] and out[0, 3] == turned[0, 3] * t[0] + turned[0, 2] * t[1]


def _winner(vol, R_, T_):
    n = vol.shape[0]
    pose = _pose(0.0, 0.0, 0.0, n)
    one = np.ones((n, 1), F32)
    _, info = R._finish(CFG, pose, vol.astype(np.int32), np.ones((n, 4), bool), one.repeat(2 * T_ + 1, 1), 0 * one.repeat(2 * T_ + 1, 1),
                        R_, T_, 0, 0)
    return [tuple(int(v) for v in row[1:4]) for row in info], info


def test_the_tie_order():
    R_, T_ = 2, 2
    def vol_of(cands, base=0, top=9):
        v = np.full((1, 2 * T_ + 1, 2 * R_ + 1, 2 * R_ + 1), base)
        for k, a, b in cands:
            v[0, k + T_, a + R_, b + R_] = top
        return v
    pick = lambda cands: _winner(vol_of(cands), R_, T_)[0][0]  # noqa: E731
    assert _winner(np.zeros((1, 5, 5, 5)), R_, T_)[0][0] == (0, 0, 0)                 # everything ties: no move
    assert pick([(0, 2, 0), (2, 1, 1), (-2, 1, 0)]) == (-2, 1, 0)                     # the smaller a^2 + b^2 first
    assert pick([(2, 1, 0), (-1, 0, 1), (-2, 0, -1)]) == (-1, 0, 1)                   # then the smaller |k|
    assert pick([(1, 1, 0), (-1, 0, 1)]) == (-1, 0, 1)                                # then the smaller k
    assert pick([(1, 1, 0), (1, 0, 1), (1, -1, 0), (1, 0, -1)]) == (1, -1, 0)         # then the smaller a
    assert pick([(1, 0, 1), (1, 0, -1)]) == (1, 0, -1)                                # then the smaller b
    assert pick([(2, 2, 2)]) == (2, 2, 2) and _winner(vol_of([(2, 2, 2)], top=-1), R_, T_)[0][0] == (0, 0, 0)
    # a score beats every tie-break
    v = vol_of([(0, 0, 0)], top=9)
    v[0, 4, 4, 4] = 10
    names, info = _winner(v, R_, T_)
    assert names[0] == (2, 2, 2) and info[0].tolist() == [1, 2, 2, 2, 10, 9, 4, 0]
    # a plane of one value scores every candidate alike where no endpoint leaves it: the prior stays
    rows = _room_scan(0.0, 0.0, 0.0)
    out, info, vol = R.match(CFG, np.full((1, WC, WC), 5, np.int8), rows, _pose(0.02, 0.01, 0.4), 3, 3, 0.01)
    assert (vol == 5 * 180).all() and info[0].tolist() == [0, 0, 0, 0, 900, 900, 180, 0]


def test_the_gate():
    x, y, yaw = 0.12, -0.07, 0.3
    rows = _room_scan(x, y, yaw)
    m = W.update(CFG, np.zeros((1, WC, WC), np.int8), rows, _pose(x, y, yaw), first=np.ones(1), range_max=2.0)
    moved = _pose(x + 2 * RES, y - RES, yaw)
    _, info, _ = R.match(CFG, m, rows, moved, 3, 0, 0.0, 2.0)
    gain = int(info[0, 4] - info[0, 5])
    assert info[0, 0] == 1 and gain > 0 and info[0, 6] == 180
    for kw, status in ((dict(min_valid=180), 1), (dict(min_valid=181), 0), (dict(min_gain=gain), 1), (dict(min_gain=gain + 1), 0)):
        out, inf2, _ = R.match(CFG, m, rows, moved, 3, 0, 0.0, 2.0, **kw)
        assert inf2[0, 0] == status and np.array_equal(inf2[0, 4:], info[0, 4:])
        assert (inf2[0, 1:4] == 0).all() == (status == 0)
        assert np.array_equal(out.view(np.uint32), moved.view(np.uint32)) == (status == 0)
    # a non-finite pose word: status 0, both scores 0, the words copied, the valid beams still counted
    for word, v in ((0, NAN), (1, INF), (2, -INF), (3, NAN)):
        bad = moved.copy()
        bad[0, word] = v
        out, inf2, vol = R.match(CFG, m, rows, bad, 3, 1, 0.01, 2.0)
        assert inf2[0].tolist() == [0, 0, 0, 0, 0, 0, 180, 0] and (vol == 0).all()
        assert np.array_equal(out.view(np.uint32), bad.view(np.uint32))


def test_beams_without_a_return_are_not_counted():
    m = np.full((1, WC, WC), 3, np.int8)
    rows = np.full((1, 12), 0.5, F32)
    rows[0, :8] = (NAN, 0.0, -0.0, -1.0, INF, -INF, 0.8, 0.7000001)
    _, info, vol = R.match(CFG, m, rows, _pose(0.0, 0.0, 0.2), 1, 1, 0.05, range_max=0.7)
    assert info[0, 6] == 4 and (vol == 12).all()
    _, info, vol = R.match(CFG, m, rows, _pose(0.0, 0.0, 0.2), 1, 1, 0.05, range_max=INF)
    assert info[0, 6] == 6 and (vol == 18).all()  # +inf is no return with range_max = +inf either
    rows[0, 0] = np.finfo(F32).max  # valid, and its endpoint is far off the plane
    _, info, vol = R.match(CFG, m, rows, _pose(0.0, 0.0, 0.2), 1, 1, 0.05, range_max=INF)
    assert info[0, 6] == 7 and (vol == 18).all()


def test_endpoints_off_the_plane_count_zero_and_convert_nothing():
    m = np.full((3, WC, WC), 2, np.int8)
    rows = np.full((3, 16), 0.1, F32)  # two cells: some endpoints are off the plane, all within R of it
    wh = float(W.half_of(CFG, WC))
    pose = np.concatenate([_pose(wh - RES, wh - RES, 0.1), _pose(-wh, wh - RES, 2.0), _pose(1e30, -1e30, 0.5)])
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # a float beyond int64 converted would warn
        out, info, vol = R.match(CFG, m, rows, pose, 2, 1, 0.03)
    assert (vol[2] == 0).all() and info[2].tolist() == [0, 0, 0, 0, 0, 0, 16, 0]
    for e in (0, 1):  # the corner: shifts into the plane see more of it than shifts out of it
        assert 0 <= vol[e].min() < vol[e, 1, 2, 2] < vol[e].max() == 2 * 16 and info[e, 0] == 1
    assert info[0, 1:4].tolist() == [0, -2, -2] and info[1, 1:4].tolist() == [0, 2, -2]
    assert np.array_equal(vol, R.match_loops(CFG, m, rows, pose, 2, 1, 0.03)[2])


def test_the_vectorised_restatement_is_the_triple_loop():
    rng = np.random.default_rng(5)
    cfg8 = Cfg.from_config(FFMPConfig(grid=8, n_obst=0, n_beams=0))
    n = 6
    m = rng.integers(-128, 128, (n, 8, 8)).astype(np.int8)
    rows = rng.uniform(0.02, 0.3, (n, 7)).astype(F32)
    rows[1, 2], rows[2, 0], rows[3, 6] = NAN, 0.0, INF
    yaw = rng.uniform(-3.2, 3.2, n)
    pose = np.stack([rng.uniform(-0.2, 0.2, n), rng.uniform(-0.2, 0.2, n), np.cos(yaw), np.sin(yaw)], axis=1).astype(F32)
    pose[4, 0], pose[5, 2:] = 0.3, 0.0
    seen = set()
    for kw in (dict(), dict(range_max=0.2, min_valid=6), dict(min_gain=40)):
        a, b = R.match(cfg8, m, rows, pose, 2, 1, 0.2, **kw), R.match_loops(cfg8, m, rows, pose, 2, 1, 0.2, **kw)
        for x, y in zip(a, b):
            assert x.dtype == y.dtype and np.array_equal(x.view(np.uint32) if x.dtype == F32 else x, y.view(np.uint32) if y.dtype == F32 else y)
        assert a[2].shape == (n, 3, 5, 5)
        seen.update(a[1][:, 0].tolist())
    assert seen == {0, 1}  # the gate shut and open among the cases


def test_the_transform_takes_the_odometry_to_the_matched_pose():
    rng = np.random.default_rng(2)
    n = 9
    def poses():
        yaw = rng.uniform(-3.1, 3.1, n)
        return np.stack([rng.uniform(-2, 2, n), rng.uniform(-2, 2, n), np.cos(yaw), np.sin(yaw)], axis=1).astype(F32)
    odom, matched = poses(), poses()
    tf = R.transform_of(matched, odom)
    assert np.abs(R.compose(tf, odom).astype(np.float64) - matched).max() < 1e-6 and (np.abs(tf[:, 2]) <= math.pi).all()
    assert np.abs(R.transform_of(odom, odom)).max() < 1e-12
    assert np.array_equal(R.compose(np.zeros((n, 3)), odom), odom)


# ------------------------------------------------------------------ 2. the C surface and its refusals
SIGS = (("ffmp_scan_match", 23), ("ffmp_scan_match_check", 9))


def test_header_binding_and_library_agree(lib):
    h = open(_abi.HEADER_PATH).read()
    assert int(re.search(r"#define FFMP_ABI_VERSION (\d+)", h).group(1)) == 9 == _abi.ABI_VERSION
    assert int(re.search(r"#define FFMP_MATCH_GLOBAL (\d+)", h).group(1)) == _abi.MATCH_GLOBAL == 1
    code = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    for name, count in SIGS:
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, code)
        assert m, name
        params = [p.strip() for p in m.group(1).split(",")]
        res, args = _abi._SIGS[name]
        assert res is C.c_int and len(args) == len(params) == count, (name, params)
        assert hasattr(lib, name)
    decl = h.index("int ffmp_scan_match(")
    comment = h[h.rindex("/*", 0, decl):decl]
    for word in ("[unpinned]", "valid_l = (r > 0) && (r <= range_max) && (r <= FLT_MAX)", "bx = r*beams[l].x;  by = r*beams[l].y",
                 "ck = c*rc - s*rs;  sk = s*rc + c*rs", "wx = (ck*bx - sk*by) + px;  wy = (sk*bx + ck*by) + py",
                 "rintf((wx + wh_f) / res_f)", "fp >= -R && fp <= Wc-1+R", "S(k, a, b)", "a*a + b*b", "then the smaller |k|",
                 "S_best - S(0,0,0) < min_gain", "bit for bit", "px + (float)a*res_f", "{status, k, a, b, S_best, S(0,0,0), valid, 0}",
                 "mask[e] == 0", "FFMP_MATCH_GLOBAL", "overlap", "an addition within ABI 9"):
        assert word in comment, word
    from flow_field_based_motion_planner_amd import ros_adapters, vec_env
    sig = inspect.signature(vec_env.WorldMap.match)
    names = ("ranges", "pose", "radius", "turns", "dtheta", "min_valid", "min_gain", "range_max", "detail", "volume", "out", "mask")
    assert [k for k in sig.parameters][1:1 + len(names)] == list(names)
    assert [sig.parameters[k].default for k in names] == [None, None, 4, 4, None, None, 0, None, False, False, None, None]
    sig = inspect.signature(vec_env.WorldMap.localizer)
    assert [sig.parameters[k].default for k in ("radius", "turns", "dtheta")] == [2, 2, None]
    sig = inspect.signature(vec_env.Localizer.step)
    assert [k for k in sig.parameters][1:] == ["odom", "ranges", "first", "update"]
    assert [sig.parameters[k].default for k in ("ranges", "first", "update")] == [None, None, True]
    assert isinstance(vec_env.Localizer.transform, property) and callable(ros_adapters.map_to_odom_transform)


P = 1 << 24  # never dereferenced: every call below is refused, or has n == 0
W2 = WC * WC
FAR = P + (1 << 28)


def _match(lib, cfg, n=4, ranges=P, stride=None, L=180, beams=P, pose=P, pose_stride=16, mask=None, map_=P, map_stride=W2, cells=WC,
           turns=P, T=4, R_=4, rm=INF, min_valid=8, min_gain=0, pose_out=FAR, info=FAR + (1 << 20), volume=FAR + (1 << 21), flags=0):
    return lib.ffmp_scan_match(C.byref(cfg), n, ranges, L if stride is None else stride, L, beams, pose, pose_stride, mask, map_,
                               map_stride, cells, turns, T, R_, rm, min_valid, min_gain, pose_out, info, volume, flags, None)


def test_argument_checks_without_a_launch(lib):
    cfg = _abi.make_cfg(FFMPConfig(grid=G, n_obst=4, n_beams=0))
    E = -1  # FFMP_E_ARG
    chk = lambda *a: lib.ffmp_scan_match_check(C.byref(cfg), *a)  # noqa: E731
    good = dict(L=180, cells=WC, R_=4, T=4, rm=INF, min_valid=8, min_gain=0, flags=0)
    order = ("L", "cells", "R_", "T", "rm", "min_valid", "min_gain", "flags")
    assert chk(*[good[k] for k in order]) == 0
    knob_cases = [(dict(R_=-1), b"radius"), (dict(R_=17), b"radius"), (dict(T=-1), b"n_turns"), (dict(T=33), b"n_turns"),
                  (dict(min_valid=-1), b"min_valid"), (dict(min_gain=-1), b"min_gain"), (dict(flags=2), b"flags"), (dict(flags=-1), b"flags"),
                  (dict(cells=4), b"cells"), (dict(cells=2052), b"cells"), (dict(cells=134), b"cells"), (dict(cells=0), b"cells"),
                  (dict(L=0), b"n_beams"), (dict(L=MAX_BEAMS + 1), b"n_beams"), (dict(rm=NAN), b"range_max"), (dict(rm=0.0), b"range_max"),
                  (dict(rm=-1.0), b"range_max")]
    big = dict(map_stride=1 << 23)
    cases = [(dict(big, **kw), word) for kw, word in knob_cases] + [
        (dict(ranges=None), b"ranges is NULL"), (dict(beams=None), b"beams is NULL"), (dict(pose=None), b"pose is NULL"),
        (dict(map_=None), b"map is NULL"), (dict(turns=None), b"turns is NULL"),
        (dict(pose_out=None, info=None, volume=None), b"all NULL"),
        (dict(stride=179), b"ranges_stride"), (dict(pose_stride=3), b"pose_stride"), (dict(map_stride=W2 - 4), b"map_env_stride"),
        (dict(map_=P + 2), b"map alignment"), (dict(map_stride=W2 + 2), b"map alignment"),
        (dict(pose_out=FAR + 4), b"output alignment"), (dict(pose_out=FAR + 8), b"output alignment"), (dict(info=FAR + 4), b"output alignment"),
        (dict(volume=FAR + 2), b"output alignment"),
        # an output whose bytes meet the map's: at its start, one row into its end, and ending one byte inside it
        (dict(pose_out=P), b"pose_out overlaps"), (dict(pose_out=P + 4 * W2 - 16), b"pose_out overlaps"), (dict(pose_out=P - 48), b"pose_out overlaps"),
        (dict(info=P + 32), b"info overlaps"), (dict(info=P - 4 * 32 + 16), b"info overlaps"),
        (dict(volume=P + 4 * W2 - 4), b"volume overlaps"), (dict(volume=P - 4 * 4 * 9 * 81 + 4), b"volume overlaps"),
        (dict(n=-1), b"negative n"), (dict(n=1 << 40), b"too large"), (dict(n=1 << 31), b"too large")]
    for kw, word in cases:
        assert _match(lib, cfg, **kw) == E, kw
        assert word in lib.ffmp_last_error(), (kw, lib.ffmp_last_error())
        assert lib.ffmp_last_error().startswith(b"ffmp_scan_match:")
    for kw, word in knob_cases:
        k = dict(good, **kw)
        assert chk(*[k[key] for key in order]) == E and word in lib.ffmp_last_error(), kw
    assert lib.ffmp_scan_match_check(None, *[good[k] for k in order]) == E and b"cfg is NULL" in lib.ffmp_last_error()
    bad = _abi.make_cfg(FFMPConfig(grid=G, n_obst=4, n_beams=0))
    bad.res_f = 0.0
    assert _match(lib, bad) == E and b"res_f" in lib.ffmp_last_error()
    # the bounds themselves pass the checks (n == 0 launches nothing), as do outputs that end where the map starts
    for kw in (dict(R_=0, T=0), dict(R_=16, T=32), dict(min_valid=0), dict(min_valid=1 << 30, min_gain=1 << 30), dict(flags=1), dict(mask=P),
               dict(pose_stride=4), dict(stride=1000), dict(L=1), dict(L=MAX_BEAMS), dict(map_=P + 4), dict(map_stride=W2 + 4),
               dict(rm=1e-3), dict(rm=1e30), dict(cells=8), dict(cells=2048, map_stride=1 << 22), dict(pose_out=None),
               dict(pose_out=None, info=None), dict(info=None, volume=None), dict(pose_out=P), dict(volume=P + 4)):
        assert _match(lib, cfg, n=0, **kw) == 0, (kw, lib.ffmp_last_error())


# ------------------------------------------------------------------ 3. the physical tie
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_single_shot_recovery(seed):
    """LONG[64] with lidar_max = 4.0, static discs, 32 envs: 30 random steps with an update after the reset and
    after each step but the last; the last pose displaced by a random (a, b, k), |a|, |b| < R = 4, |k| < T = 4,
    dtheta = 0.0125.  Measured by the restatement, seeds 1-3: 29 of 32 kept, all within one cell and one step,
    100 % exact, >= 141 valid beams."""
    kept, miss, valid = R.single_shot(seed)
    print(f"seed {seed}: kept {kept}, within {(miss <= 1).all(axis=1).sum()}, exact {(miss == 0).all(axis=1).mean():.3f}, valid >= {valid.min()}")
    assert kept >= 24
    assert (miss <= 1).all()
    assert (miss == 0).all(axis=1).mean() >= 0.85


def test_drift_run():
    """The drift run of DESIGN §10.12 at seed 1: odometry that drifts by 5 mm and 0.008 rad a step, 24 envs, 40
    steps of actions 7..27, the map plane default_cells + 24, search +-2 cells and +-2 x 0.0125 rad.  Measured by
    the restatement: 17 envs kept; matched max 0.065 m / 0.020 rad; unmatched median 0.509 m."""
    d, yaw, bad, kept = R.drift_run(1, matching=True)
    d0, yaw0, bad0, kept0 = R.drift_run(1, matching=False)
    print(f"matched: kept {kept}, max {d.max():.4f} m, {yaw.max():.4f} rad, contradiction {bad:.4f}; "
          f"control: median {np.median(d0):.4f} m, {yaw0.max():.4f} rad, contradiction {bad0:.4f}")
    assert kept >= 16 and kept0 == kept
    assert d.max() <= 0.15
    assert yaw.max() <= 0.04
    assert np.median(d0) >= 0.4
