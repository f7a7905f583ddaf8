"""Motion flow estimated from the scan, without a GPU: the NumPy restatement (tests/scan_flow_ref.py, the
checker of tests/test_gpu_scan_flow.py) has the SPEC's properties with known answers (include/ffmp.h
ffmp_scan_flow) and is tied to the oracle's ground-truth flow; ffmp_scan_flow /
ffmp_scan_flow_check are declared, bound and exported consistently inside ABI 9, and every argument check
answers before any launch."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest

from flow_field_based_motion_planner_amd import _abi
from flow_field_based_motion_planner_amd.config import FFMPConfig
from oracle.ffmp_oracle import Cfg
from tests import scan_flow_ref as R

F32 = np.float32
INF = float("inf")
NAN = float("nan")
G = 64
H = G // 2
CFG = Cfg.from_config(FFMPConfig(grid=G, n_obst=0, n_beams=0))
RES = float(F32(CFG.f["res_f"]))
Z = np.array([[0.0, 0.0, 1.0, 0.0]], F32)  # a pose: identity when used for both frames
SCALE = F32(0.125)


def _poses(n, p=Z):
    return np.tile(np.asarray(p, F32), (n, 1))


def _shifted(m, du, dv):
    """s[i][j] = m[i - du][j - dv], 0 where that leaves the plane."""
    out = np.zeros_like(m)
    g = m.shape[-1]
    out[..., max(du, 0):g + min(du, 0), max(dv, 0):g + min(dv, 0)] = m[..., max(-du, 0):g + min(-du, 0), max(-dv, 0):g + min(-dv, 0)]
    return out


def _blobs(seed=0, first=8, step=15, count=4):
    """A (G, G) uint8 frame of asymmetric blobs: at every lattice site a random non-empty subset of 3 x 3 cells.
    Blobs lie >= 13 cells apart: no block (+-3) or search window (+-7) around a cell of one blob, shifted by
    up to 4 cells, reaches another."""
    rng = np.random.default_rng(seed)
    m = np.zeros((G, G), np.uint8)
    for a in range(count):
        for b in range(count):
            while True:
                blob = rng.integers(0, 2, (3, 3))
                if blob.sum() >= 2 and not np.array_equal(blob, blob[::-1, ::-1]):
                    break
            i, j = first + step * a, first + step * b
            m[i:i + 3, j:j + 3] = 255 * blob
    return m


# ------------------------------------------------------------------ 1. a shifted pattern is recovered
def test_every_shift_of_a_blob_pattern_is_recovered_exactly():
    """prev = blobs, cur = blobs shifted by (du, dv), identity pose, radius 4, block 3, gate 0, min_hits 1.
    A shift within one cell (|du|, |dv| <= 1) lies inside the 3 x 3 dilation of the static gate: c0 = 0 and
    every hit cell is static (kind 1, flow 0).  Any other shift: the blob's leading cell lies outside
    D(Hp), so c0 >= 1 > gate, the true displacement costs 0 and no other one does (a blob of width <= 3 in a
    block of width 7 never equals its own translate): kind 2 and (du, dv) exactly, for every hit cell whose
    block and source block lie inside the grid."""
    rad, B = 4, 3
    shifts = [(du, dv) for du in range(-rad, rad + 1) for dv in range(-rad, rad + 1)]
    prev = np.tile(_blobs(), (len(shifts), 1, 1))
    cur = np.stack([_shifted(prev[0], du, dv) for du, dv in shifts])
    flow, kind = R.scan_flow(CFG, cur, prev, _poses(len(shifts)), _poses(len(shifts)), SCALE, radius=rad, block=B, gate=0, min_hits=1)
    ii, jj = np.meshgrid(np.arange(G), np.arange(G), indexing="ij")
    hits = left_out = 0
    for k, (du, dv) in enumerate(shifts):
        hit = cur[k] == 255
        inside = (ii - B >= 0) & (ii + B < G) & (jj - B >= 0) & (jj + B < G) & \
                 (ii - du - B >= 0) & (ii - du + B < G) & (jj - dv - B >= 0) & (jj - dv + B < G)
        hits += int(hit.sum())
        left_out += int((hit & ~inside).sum())
        sel = hit & inside
        assert sel.sum() >= 30, (du, dv)
        if max(abs(du), abs(dv)) <= 1:
            assert (kind[k][sel] == 1).all() and (flow[k][:, sel] == 0).all(), (du, dv)
        else:
            assert (kind[k][sel] == 2).all(), (du, dv, np.unique(kind[k][sel]))
            assert (flow[k, 0][sel] == F32(du) * SCALE).all() and (flow[k, 1][sel] == F32(dv) * SCALE).all(), (du, dv)
        assert (kind[k][~hit] == 0).all() and (flow[k][:, ~hit] == 0).all()
    assert 4 * left_out <= hits, (left_out, hits)


# ------------------------------------------------------------------ 2. a static pattern under ego motion
def _walls(seed=1):
    """A static scene: a rectangle of walls two cells thick and a few random thick dots."""
    rng = np.random.default_rng(seed)
    m = np.zeros((G, G), np.uint8)
    m[14:16, 14:50] = m[48:50, 14:50] = m[14:50, 14:16] = m[14:50, 48:50] = 255
    for _ in range(12):
        i, j = rng.integers(18, 44, 2)
        m[i:i + 2, j:j + 2] = 255
    return m


@pytest.mark.parametrize("k,axis", [(1, 0), (-3, 0), (2, 1), (-4, 1)])
def test_static_pattern_under_a_whole_cell_translation(k, axis):
    """The robot moves k cells along ego x (axis 0) or ego y (axis 1), yaw 0: the cell now at (i, j) was at
    (i + k, j); the warp moves the earlier frame onto the current one, so nothing moves."""
    prev = _walls()
    cur = _shifted(prev, -k if axis == 0 else 0, -k if axis == 1 else 0)  # cur[i][j] = prev[i + k][j]
    now = Z.copy()
    now[0, axis] = F32(k * RES)
    flow, kind = R.scan_flow(CFG, cur[None], prev[None], now, Z, SCALE)
    hit = cur == 255
    assert (flow == 0).all() and np.isin(kind, (0, 1)).all()
    assert (kind[0][hit] == 1).mean() > 0.95 and (kind[0][~hit] == 0).all()
    # without the compensation the same pair moves (|k| >= 2) — the estimator sees the shift
    f2, k2 = R.scan_flow(CFG, cur[None], prev[None], Z, Z, SCALE)
    if abs(k) >= 2:
        assert (k2 == 2).sum() > 50 and (f2 != 0).any()


def test_static_pattern_under_a_quarter_turn():
    """The robot turns left by 90 degrees on the spot: the cell now at offsets (a, b) was at (-b, a)
    (tests/test_lidar_map_host.py test_quarter_turn)."""
    prev = _walls(seed=2)
    a, b = np.meshgrid(np.arange(G) - H, np.arange(G) - H, indexing="ij")
    ok = -b <= H - 1
    cur = np.where(ok, prev[np.where(ok, -b + H, 0), a + H], 0).astype(np.uint8)
    now = np.array([[0.3, 0.4, 0.0, 1.0]], F32)
    was = np.array([[0.3, 0.4, 1.0, 0.0]], F32)
    flow, kind = R.scan_flow(CFG, cur[None], prev[None], now, was, SCALE)
    assert (flow == 0).all() and np.isin(kind, (0, 1)).all() and (kind[0][cur == 255] == 1).mean() > 0.95
    f2, k2 = R.scan_flow(CFG, cur[None], prev[None], was, was, SCALE)
    assert (k2 == 2).any() and (f2 != 0).any()  # uncompensated, the dots move (the square of walls maps onto itself)


# ------------------------------------------------------------------ 3. gate, min_hits, first, mask
def _one(cells_cur, cells_prev, n=1, **kw):
    cur = np.zeros((n, G, G), np.uint8)
    prev = np.zeros((n, G, G), np.uint8)
    for i, j in cells_cur:
        cur[:, i, j] = 255
    for i, j in cells_prev:
        prev[:, i, j] = 255
    kw.setdefault("pose_now", _poses(n))
    return R.scan_flow(CFG, cur, prev, kw.pop("pose_now"), _poses(n), SCALE, **kw)


def test_gate_min_hits_first_and_mask():
    # one cell that moved 3 columns: itself unmatched and its source unmatched inside the block, c0 = 2
    flow, kind = _one([(30, 33)], [(30, 30)], gate=1, min_hits=1)
    assert kind[0, 30, 33] == 2 and flow[0, 0, 30, 33] == 0 and flow[0, 1, 30, 33] == F32(3) * SCALE
    assert kind.sum() == 2 and np.count_nonzero(flow) == 1
    flow, kind = _one([(30, 33)], [(30, 30)], gate=2, min_hits=1)
    assert kind[0, 30, 33] == 1 and (flow == 0).all()
    # with block 2 the source is outside the block: c0 = 1
    assert _one([(30, 33)], [(30, 30)], gate=1, min_hits=1, block=2)[1][0, 30, 33] == 1
    assert _one([(30, 33)], [(30, 30)], gate=0, min_hits=1, block=2)[1][0, 30, 33] == 2
    # bytes other than 255 are no hits
    cur = np.full((1, G, G), 128, np.uint8)
    cur[0, 30, 33] = 255
    prev = np.full((1, G, G), 254, np.uint8)
    prev[0, 30, 30] = 255
    flow, kind = R.scan_flow(CFG, cur, prev, Z, Z, SCALE, min_hits=1)
    assert kind.sum() == 2 and flow[0, 1, 30, 33] == F32(3) * SCALE
    # min_hits: the current block has one hit; and a displacement whose source block has too few is skipped
    assert _one([(30, 33)], [(30, 30)], min_hits=2)[1].sum() == 0
    flow, kind = _one([(30, 33), (30, 34)], [(30, 30), (30, 31), (33, 36)], min_hits=2, gate=0)
    assert kind[0, 30, 33] == 2 and kind[0, 30, 34] == 2 and (flow[0, 1][[30, 30], [33, 34]] == F32(3) * SCALE).all()
    assert _one([(30, 33), (30, 34)], [(30, 30)], min_hits=2, gate=0)[1].sum() == 0  # no source block has two hits
    # the radius bounds the search: a source 5 cells away is found with radius 5 only
    assert _one([(30, 35)], [(30, 30)], min_hits=1, gate=0, radius=4)[0][0, 1, 30, 35] != F32(5) * SCALE
    flow, kind = _one([(30, 35)], [(30, 30)], min_hits=1, gate=0, radius=5)
    assert kind[0, 30, 35] == 2 and flow[0, 1, 30, 35] == F32(5) * SCALE
    # first, or a pose word that is not finite: kind 0 and flow 0 everywhere; mask 0 keeps what was there
    n = 4
    now = _poses(n)
    now[2, 1] = NAN
    fin = np.full((n, 2, G, G), 7, F32)
    kin = np.full((n, G, G), 9, np.uint8)
    flow, kind = _one([(30, 33)], [(30, 30)], n=n, pose_now=now, min_hits=1, first=np.array([0, 1, 0, 0]), mask=np.array([1, 1, 1, 0]),
                      flow_in=fin, kind_in=kin)
    assert kind[0, 30, 33] == 2 and kind[1].sum() == 0 and kind[2].sum() == 0 and (flow[1] == 0).all() and (flow[2] == 0).all()
    assert (flow[3] == 7).all() and (kind[3] == 9).all()
    # binary16 under the compact format
    f16, _ = _one([(30, 33)], [(30, 30)], min_hits=1, half=True)
    assert f16.dtype == np.float16 and f16[0, 1, 30, 33] == np.float16(F32(3) * SCALE)
    # the sign: a negative scale gives -0.0 for a kind-2 component with displacement 0, as (float)0 * scale does
    fneg, _ = R.scan_flow(CFG, *[x for x in _frames_pair()], Z, Z, F32(-0.125), min_hits=1)
    assert np.signbit(fneg[0, 0, 30, 33]) and fneg[0, 1, 30, 33] == F32(-0.375)


def _frames_pair():
    cur = np.zeros((1, G, G), np.uint8)
    prev = np.zeros((1, G, G), np.uint8)
    cur[0, 30, 33] = prev[0, 30, 30] = 255
    return cur, prev


# ------------------------------------------------------------------ 4. the visiting order
def test_ties_go_to_the_smaller_norm_then_du_then_dv():
    """One current hit at (32, 32), block 1, radius 4; earlier hits at the 8 cells 4 away along the axes and
    the diagonals, >= 4 cells apart: each candidate's block holds exactly its own hit, so every candidate costs
    0.  The winner is the first in the order (du*du + dv*dv, du, dv); taking it away promotes the next."""
    cand = [(du, dv) for du in (-4, 0, 4) for dv in (-4, 0, 4) if (du, dv) != (0, 0)]
    order = sorted(cand, key=lambda d: (d[0] * d[0] + d[1] * d[1], d[0], d[1]))
    assert order[:4] == [(-4, 0), (0, -4), (0, 4), (4, 0)] and order[4:] == [(-4, -4), (-4, 4), (4, -4), (4, 4)]
    assert [d for d in R.displacements(4) if d in cand] == order
    left = list(order)
    while left:
        flow, kind = _one([(32, 32)], [(32 - du, 32 - dv) for du, dv in left], gate=0, min_hits=1, block=1, radius=4)
        du, dv = left.pop(0)
        assert kind[0, 32, 32] == 2
        assert (flow[0, 0, 32, 32], flow[0, 1, 32, 32]) == (F32(du) * SCALE, F32(dv) * SCALE), (du, dv)
    assert R.displacements(1) == [(0, 0), (-1, 0), (0, -1), (0, 1), (1, 0), (-1, -1), (-1, 1), (1, -1), (1, 1)]
    assert len(R.displacements(5)) == 121


# ------------------------------------------------------------------ 5. the bookkeeping
def test_refflow_restarts_until_it_has_lag_frames():
    config = FFMPConfig(**R.TIE[64])
    n, lag = 3, 2
    ref = R.RefFlow(config, n, lag=lag)
    rng = np.random.default_rng(0)
    lidar = rng.uniform(0.3, 1.4, (n, 180)).astype(F32)
    rec = np.zeros((n, 16), F32)
    rec[:, 2] = 1.0
    ep = np.zeros(n, np.int64)
    firsts = []
    for k in range(6):
        if k == 4:
            ep[1] += 1  # env 1 starts a new episode
        firsts.append(ref.update(lidar, rec, ep).copy())
    assert [f.tolist() for f in firsts] == [[True] * 3, [True] * 3, [False] * 3, [False] * 3, [False, True, False],
                                            [False, True, False]]
    assert ref.updates.tolist() == [6, 2, 6]
    assert ref.update(lidar, rec, ep).tolist() == [False, False, False]
    ref.update(lidar, rec, ep, mask=np.array([1, 0, 1]))  # env 1 is left out: it loses its history
    assert ref.update(lidar, rec, ep).tolist() == [False, True, False] and ref.updates.tolist() == [9, 1, 9]
    ref.reset(np.array([1, 0, 0]))
    assert ref.update(lidar, rec, ep).tolist() == [True, True, False]
    assert float(ref.scale) == float(F32(config.res / (lag * config.dt)))


# ------------------------------------------------------------------ 6. the C surface and its refusals
def test_header_binding_and_library_agree(lib):
    h = open(_abi.HEADER_PATH).read()
    assert int(re.search(r"#define FFMP_ABI_VERSION (\d+)", h).group(1)) == 9 == _abi.ABI_VERSION
    assert lib.ffmp_abi_version() == 9
    code = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    for name, count in (("ffmp_scan_flow", 22), ("ffmp_scan_flow_check", 7)):
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, code)
        assert m, name
        params = [p.strip() for p in m.group(1).split(",")]
        res, args = _abi._SIGS[name]
        assert res is C.c_int and len(args) == len(params) == count, (name, params)
        assert hasattr(lib, name)
    decl = h.index("int ffmp_scan_flow(")
    comment = h[h.rindex("/*", 0, decl):decl]
    for word in ("[unpinned]", "Hc[i][j]   = cur[i][j] == 255", "Hp[i][j]   = inside && prev[(int)ru + G/2][(int)rv + G/2] == 255",
                 "D(X)[i][j] = OR of X over the 3 x 3 neighbourhood", "nc < min_hits", "c0 <= gate", "(du*du + dv*dv, du, dv)",
                 "np_d < min_hits is skipped", "strictly smaller", "vx = (float)du * scale", "round-to-nearest-even", "aperture",
                 "ffmp_scan_map's"):
        assert word in comment, word
    assert "ffmp_scan_flow      ->" in h[:h.index("#ifndef FFMP_H")]
    from flow_field_based_motion_planner_amd import env, vec_env
    sig = inspect.signature(vec_env.FFMPVec.lidar_flow)
    names = ("lag", "radius", "block", "gate", "min_hits", "thickness", "range_max", "kind")
    assert [sig.parameters[k].default for k in names] == [4, 4, 3, 1, 3, None, None, True]
    sig = inspect.signature(vec_env.LidarFlow.update)
    assert [sig.parameters[k].default for k in ("ranges", "pose", "first", "mask")] == [None, None, None, None]
    sig = inspect.signature(vec_env.LidarFlow.bev_image)
    assert [sig.parameters[k].default for k in ("occ", "out")] == [None, None]
    assert callable(env.FFMP.lidar_flow) and callable(vec_env.LidarFlow.reset)


P = 1 << 20  # never dereferenced: every call below is refused, or has n == 0
G2 = G * G
KNOBS = dict(radius=4, block=3, gate=1, min_hits=3)


def _call(lib, cfg, n=4, cur=P, prev=P + 4 * G2, frame_stride=G2, now=P, now_stride=16, was=P, was_stride=4, mask=None, first=None,
          flow=P + (1 << 20), flow_stride=2 * G2, kind=P + (2 << 20), kind_stride=G2, fmt=0, scale=0.125, **knobs):
    k = dict(KNOBS, **knobs)
    return lib.ffmp_scan_flow(C.byref(cfg), n, cur, prev, frame_stride, now, now_stride, was, was_stride, mask, first, flow,
                              flow_stride, kind, kind_stride, fmt, scale, k["radius"], k["block"], k["gate"], k["min_hits"], None)


def test_argument_checks_without_a_launch(lib):
    cfg = _abi.make_cfg(FFMPConfig(grid=G, n_obst=4, n_beams=0))
    E = -1  # FFMP_E_ARG
    chk = lambda *a: lib.ffmp_scan_flow_check(C.byref(cfg), *a)  # noqa: E731
    good = (0, 0.125, 4, 3, 1, 3)
    assert chk(*good) == 0
    for g in (4, 516, 1024, 66, 0):
        bad = _abi.make_cfg(FFMPConfig(grid=G, n_obst=4, n_beams=0))
        bad.grid = g
        assert _call(lib, bad, frame_stride=1 << 30, flow_stride=1 << 30, kind_stride=1 << 30) == E and b"grid" in lib.ffmp_last_error(), g
        assert lib.ffmp_scan_flow_check(C.byref(bad), *good) == E and b"grid" in lib.ffmp_last_error()
    knob_cases = [(dict(radius=0), b"radius"), (dict(radius=6), b"radius"), (dict(block=0), b"block"), (dict(block=4), b"block"),
                  (dict(gate=-1), b"gate"), (dict(gate=99), b"gate"), (dict(min_hits=0), b"min_hits"), (dict(min_hits=50), b"min_hits")]
    F = P + (1 << 20)
    cases = knob_cases + [
        (dict(fmt=2), b"format"), (dict(fmt=-1), b"format"), (dict(scale=NAN), b"scale"), (dict(scale=INF), b"scale"),
        (dict(scale=-INF), b"scale"),
        (dict(cur=None), b"cur is NULL"), (dict(prev=None), b"prev is NULL"), (dict(now=None), b"pose_now is NULL"),
        (dict(was=None), b"pose_prev is NULL"), (dict(flow=None), b"flow_out is NULL"),
        (dict(now_stride=3), b"pose_now_stride"), (dict(was_stride=0), b"pose_prev_stride"),
        (dict(frame_stride=G2 - 4), b"frame_env_stride"), (dict(flow_stride=2 * G2 - 4), b"flow_env_stride"),
        (dict(kind_stride=G2 - 4), b"kind_env_stride"),
        (dict(cur=P + 2), b"frame alignment"), (dict(prev=P + 4 * G2 + 1), b"frame alignment"), (dict(frame_stride=G2 + 2), b"frame alignment"),
        (dict(flow=F + 8), b"flow alignment"), (dict(flow=F + 4, fmt=1), b"flow alignment"), (dict(flow_stride=2 * G2 + 2), b"flow alignment"),
        (dict(kind=P + (2 << 20) + 2), b"kind alignment"), (dict(kind_stride=G2 + 2), b"kind alignment"),
        # flow_out and kind_out share bytes, either way round; an output on top of a frame
        (dict(kind=F), b"overlap"), (dict(kind=F + 4 * (8 * G2) - 4), b"overlap"), (dict(kind=F - 4 * G2 + 4), b"overlap"),
        (dict(kind=F + 2 * (8 * G2) - 4, fmt=1), b"overlap"),
        (dict(flow=P), b"overlap"), (dict(flow=P + 8 * G2 - 16), b"overlap"), (dict(kind=P + 4 * G2), b"overlap"),
        (dict(n=-1), b"negative n"), (dict(n=1 << 40), b"too large")]
    for kw, word in cases:
        assert _call(lib, cfg, **kw) == E, kw
        assert word in lib.ffmp_last_error(), (kw, lib.ffmp_last_error())
        assert lib.ffmp_last_error().startswith(b"ffmp_scan_flow:")
    for kw, word in knob_cases:
        k = dict(KNOBS, **kw)
        assert chk(0, 0.125, k["radius"], k["block"], k["gate"], k["min_hits"]) == E and word in lib.ffmp_last_error()
    assert chk(2, 0.125, 4, 3, 1, 3) == E and b"format" in lib.ffmp_last_error()
    assert chk(0, NAN, 4, 3, 1, 3) == E and b"scale" in lib.ffmp_last_error()
    assert lib.ffmp_scan_flow_check(None, *good) == E
    assert lib.ffmp_scan_flow(None, 0, P, P, G2, P, 4, P, 4, None, None, P, 2 * G2, None, 0, 0, 0.125, 4, 3, 1, 3, None) == E
    # the bounds themselves pass the checks: n == 0 launches nothing
    for kw in (dict(radius=1, block=1, gate=0, min_hits=1), dict(radius=5, block=3, gate=98, min_hits=49), dict(kind=None),
               dict(kind=None, kind_stride=0), dict(fmt=1), dict(fmt=1, flow=F + 8), dict(mask=P), dict(first=P), dict(now_stride=4),
               dict(scale=0.0), dict(scale=-3.0), dict(scale=1e30), dict(frame_stride=G2 + 4), dict(flow_stride=2 * G2 + 4),
               dict(kind_stride=G2 + 4), dict(cur=P, prev=P)):
        assert _call(lib, cfg, n=0, **kw) == 0, (kw, lib.ffmp_last_error())
    for g in (8, 36, 100, 512):
        ok = _abi.make_cfg(FFMPConfig(grid=g, n_obst=1, n_beams=0))
        assert _call(lib, ok, n=0, frame_stride=g * g, flow_stride=2 * g * g, kind_stride=g * g) == 0
        assert lib.ffmp_scan_flow_check(C.byref(ok), 1, -0.5, 5, 1, 98, 1) == 0


# ------------------------------------------------------------------ 7. the physical tie to the oracle
def test_the_estimate_agrees_with_the_ground_truth_flow():
    """OracleVecEnv on TIE[64] (flow=True, 8 moving discs, vmax 0.5 m/s, world_half = 0.45 G res, L = 180), 16 envs,
    16 steps of default_rng(1) actions, lag 4, radius 4, block 3, gate 1, min_hits 3, an update after the reset
    and after every step; one quantum is res / (lag dt) = 0.125 m/s.  Among the hit cells of the envs that have
    an estimate:
      moving — kind 1 or 2, within two cells of a moving disc: the share within 2 quanta (either component)
               of the ground-truth flow dilated by two cells;
      static — farther than two cells from every disc (the world's walls): the share with flow exactly zero.
    Measured (python tests/scan_flow_ref.py), seeds 1 and 2:
        G = 64:  moving 0.883, 0.883 of 13,836 / 13,991 cells; static 0.823, 0.827 of 21,912 / 22,354 cells;
                 with the identity warp in place of the ego motion: moving 0.406, 0.369; static 0.445, 0.408.
        G = 100: moving 0.943, 0.938; static 0.866, 0.870; identity warp: moving 0.384, 0.338; static 0.491, 0.457.
    Caps: moving >= 0.80, static >= 0.75, and the identity warp below 0.55 on both — they separate an
    estimator that compensates the ego motion from one that does not."""
    config = FFMPConfig(**R.TIE[64])
    assert config.flow and config.moving and config.n_obst == 8 and config.n_beams == 180 and config.obst_vmax == 0.5
    assert abs(config.W - 0.45 * 64 * config.res) < 1e-12 and config.res / (4 * config.dt) == 0.125
    good, moving, zero, static = R.tie_on_oracle(config, n=16, steps=16, seed=1)
    print(f"ego compensated: moving {good} of {moving} ({good / moving:.3f}), static {zero} of {static} ({zero / static:.3f})")
    assert moving >= 5000 and static >= 5000
    assert good / moving >= 0.80
    assert zero / static >= 0.75
    good, moving, zero, static = R.tie_on_oracle(config, n=16, steps=16, seed=1, identity=True)
    print(f"identity warp: moving {good} of {moving} ({good / moving:.3f}), static {zero} of {static} ({zero / static:.3f})")
    assert moving >= 5000 and static >= 5000
    assert good / moving < 0.55
    assert zero / static < 0.55
