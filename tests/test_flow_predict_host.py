"""Predicted-occupancy frames, without a GPU: the NumPy restatement (tests/flow_predict_ref.py, the checker of
tests/test_gpu_flow_predict.py) has the SPEC's properties with known answers (include/ffmp.h ffmp_flow_predict,
DESIGN §3 a16d) and is tied to the oracle by a closed loop in which it matters; ffmp_flow_predict /
ffmp_flow_predict_check are declared, bound and exported consistently inside ABI 9, and every argument check
answers before any launch."""
import ctypes as C
import functools
import inspect
import json
import re

import numpy as np
import pytest

from flow_field_based_motion_planner_amd import _abi
from flow_field_based_motion_planner_amd.config import FFMPConfig
from tests import flow_predict_cases as K
from tests import flow_predict_ref as R

F32 = np.float32
INF = float("inf")
NAN = float("nan")
G = 64
H = G // 2
OFF = dict(pace=6, slack=-1)  # the gate off


def _one(cells, su, sv, steps, frame=None, cps=F32(1.0), **kw):
    """Sources at `cells` (255), all with flow (su, sv) in cells per step (cps = 1) -> (out, n_swept) of one env."""
    f = np.zeros((G, G), F32) if frame is None else frame.copy()
    flow = np.zeros((2, G, G), F32)
    for i, j in cells:
        f[i, j] = 255
    flow[0], flow[1] = su, sv
    out, cnt = R.flow_predict(f[None], flow[None], steps=steps, cps=cps, **kw)
    return out[0], int(cnt[0])


def _cells(out, value):
    return sorted((int(i), int(j)) for i, j in zip(*np.nonzero(out == value)))


# ------------------------------------------------------------------ 1. known answers
def test_known_answers():
    # one cell per step along ego x: exactly the cells (21..28, 20)
    out, cnt = _one([(20, 20)], 1.0, 0.0, 8, **OFF)
    assert _cells(out, 254) == [(i, 20) for i in range(21, 29)] and cnt == 8
    assert _cells(out, 255) == [(20, 20)] and np.isin(out, (0, 254, 255)).all() and out.dtype == np.uint8
    # half a cell per step: rintf goes half to even — offsets 0, 1, 2, 2, 2, 3, 4, 4; the source cell stays 255
    assert [int(np.rint(F32(k) * F32(0.5))) for k in range(1, 9)] == [0, 1, 2, 2, 2, 3, 4, 4]
    out, cnt = _one([(20, 20)], 0.5, 0.0, 8, **OFF)
    assert _cells(out, 254) == [(21, 20), (22, 20), (23, 20), (24, 20)] and out[20, 20] == 255 and cnt == 4
    # the multiply by cps is the SPEC's: 0.25 m/s at 2 cells per m/s per step is the same track
    out2, _ = _one([(20, 20)], 0.25, 0.0, 8, cps=F32(2.0), **OFF)
    assert np.array_equal(out, out2)
    # both axes, negative components
    out, _ = _one([(20, 20)], -1.0, 2.0, 3, **OFF)
    assert _cells(out, 254) == [(17, 26), (18, 24), (19, 22)]
    # targets that leave the grid are dropped, the rest kept
    out, cnt = _one([(60, 5)], 1.0, -1.0, 8, **OFF)
    assert _cells(out, 254) == [(61, 4), (62, 3), (63, 2)] and cnt == 3
    out, cnt = _one([(0, 0)], -1.0, 0.0, 8, **OFF)
    assert cnt == 0 and _cells(out, 254) == []
    # a displacement far beyond the grid, up to an overflow of (float)k * su, is outside and nothing else
    for big in (1e3, 3e9, 3e38):
        out, cnt = _one([(20, 20)], big, 0.0, 8, **OFF)
        assert cnt == 0 and _cells(out, 255) == [(20, 20)]
    # NaN, inf or zero flow makes no source; -0.0 is zero
    for su, sv in ((NAN, 1.0), (1.0, NAN), (INF, 0.0), (0.0, -INF), (0.0, 0.0), (-0.0, 0.0), (-0.0, -0.0)):
        out, cnt = _one([(20, 20)], su, sv, 8, **OFF)
        assert cnt == 0 and _cells(out, 255) == [(20, 20)] and (out[out != 255] == 0).all(), (su, sv)
    # a finite flow times cps that overflows is no source either
    assert _one([(20, 20)], 3e38, 0.0, 8, cps=F32(100.0), **OFF)[1] == 0
    # one zero component is a source
    assert _one([(20, 20)], 0.0, 1.0, 2, **OFF)[1] == 2


def test_other_values_sources_and_the_count():
    f = np.zeros((G, G), F32)
    f[20, 24] = 128      # occupied, never a source: `other`, and under a set bit still `other`
    f[20, 30] = 255      # a 255 cell under a set bit stays 255
    f[40, 40] = 128      # with a flow of its own: still no source
    f[41, 41] = NAN      # a NaN compares false: free
    f[42, 42] = -3.0     # not > 0: free
    f[43, 43] = 0.5      # > 0: occupied
    out, cnt = _one([(20, 20)], 0.0, 1.0, 12, frame=f, other=77, swept=9, **OFF)
    assert out[20, 24] == 77 and out[20, 30] == 255 and out[40, 40] == 77 and out[43, 43] == 77
    assert out[41, 41] == 0 and out[42, 42] == 0
    # the 255 cell at (20, 30) is a source too and sweeps (20, 31..42): n_swept counts every free cell with a bit, once
    bit_free = ({(20, j) for j in range(21, 33)} | {(20, j) for j in range(31, 43)}) - {(20, 24), (20, 30)}
    assert _cells(out, 9) == sorted(bit_free) and cnt == len(bit_free) == 20
    # uint8 frames and binary16 flow give the same plane
    fu = np.zeros((1, G, G), np.uint8)
    fu[0, 20, 20] = fu[0, 20, 30] = 255
    fu[0, 20, 24] = fu[0, 40, 40] = 128
    fu[0, 43, 43] = 1
    flow = np.zeros((1, 2, G, G), F32)
    flow[0, 1] = 1.0
    a = R.flow_predict(fu, flow, steps=12, cps=F32(1.0), other=77, swept=9, **OFF)
    b = R.flow_predict(fu, flow.astype(np.float16), steps=12, cps=F32(1.0), other=77, swept=9, **OFF)
    assert np.array_equal(a[0], out[None]) and np.array_equal(b[0], a[0]) and a[1][0] == b[1][0] == cnt
    # swept = 0 leaves the plane as it was but still counts
    out0, cnt0 = _one([(20, 20)], 0.0, 1.0, 12, frame=f, other=77, swept=0, **OFF)
    assert cnt0 == cnt and _cells(out0, 9) == [] and (out0 != 0).sum() == 5


# ------------------------------------------------------------------ 2. the gate
@pytest.mark.parametrize("pace,slack,steps,cell,ka", [(6, 3, 24, (H + 6, H), 5), (6, 0, 24, (H + 6, H), 5), (6, -1, 24, (H + 6, H), 5),
                                                      (6, 3, 24, (H - 4, H + 5), 5), (1, 3, 40, (H + 6, H), 30),
                                                      (1024, 3, 24, (H + 6, H), 0), (1024, 0, 24, (H + 6, H), 0),
                                                      (6, 255, 24, (H + 6, H), 5)])
def test_a_cell_is_blocked_only_near_the_robots_arrival(pace, slack, steps, cell, ka):
    """A source on row ti moving one cell per step along ego y passes through `cell` at step k0 = the distance it
    starts at.  ka of the cell is the chamfer 5-7 distance over the pace: the cell is blocked for k0 in
    ka - slack .. ka + slack and at no other k0 (every k0 <= steps with the gate off)."""
    ti, tj = cell
    assert int(R.arrival(G, pace)[ti, tj]) == ka
    assert R.arrival(G, 6)[H, H] == 0 and R.arrival(G, 6)[H + 3, H - 2] == (15 + 4) // 6 and R.arrival(G, 1)[0, 0] == 7 * H
    for k0 in range(1, min(tj, steps + 6) + 1):
        out, _ = _one([(ti, tj - k0)], 0.0, 1.0, steps, pace=pace, slack=slack)
        want = k0 <= steps and (slack < 0 or abs(k0 - ka) <= slack)
        assert (out[ti, tj] == 254) == want, (k0, out[ti, tj])


# ------------------------------------------------------------------ 3. a rigid blob is translated rigidly
def _shifted(m, du, dv):
    """s[i][j] = m[i - du][j - dv], False where that leaves the plane."""
    out = np.zeros_like(m)
    g = m.shape[-1]
    if abs(du) < g and abs(dv) < g:
        out[max(du, 0):g + min(du, 0), max(dv, 0):g + min(dv, 0)] = m[max(-du, 0):g + min(-du, 0), max(-dv, 0):g + min(-dv, 0)]
    return out


@pytest.mark.parametrize("su,sv", [(1.0, 0.0), (0.5, 0.5), (0.7, -0.4), (-0.3, 1.0), (-1.0, -1.0), (0.13, 0.0), (2.5, -1.5)])
def test_a_rigid_blob_is_translated_rigidly_at_every_k(su, sv):
    rng = np.random.default_rng(3)
    blob = np.zeros((G, G), bool)
    blob[28:35, 26:33] = rng.random((7, 7)) < 0.7
    solid = np.zeros((G, G), bool)
    solid[40:45, 10:15] = True
    for m in (blob, solid):
        steps = 30
        out, cnt = _one(list(zip(*np.nonzero(m))), su, sv, steps, **OFF)
        union = np.zeros_like(m)
        for k in range(1, steps + 1):
            union |= _shifted(m, int(np.rint(F32(k) * F32(su))), int(np.rint(F32(k) * F32(sv))))
        assert np.array_equal(out == 254, union & ~m) and np.array_equal(out == 255, m) and cnt == (union & ~m).sum()
    if max(abs(su), abs(sv)) <= 1.0:
        # no holes inside the swept image of a solid blob at <= 1 cell per step: every row and every column of it is one run
        region = (out != 0)
        for line in list(region) + list(region.T):
            idx = np.nonzero(line)[0]
            assert idx.size == 0 or idx[-1] - idx[0] + 1 == idx.size


# ------------------------------------------------------------------ 4. mask
def test_mask_keeps_a_poisoned_out():
    f = np.zeros((3, G, G), F32)
    f[:, 20, 20] = 255
    flow = np.zeros((3, 2, G, G), F32)
    flow[:, 0] = 1.0
    poison = np.full((3, G, G), 7, np.uint8)
    out, cnt = R.flow_predict(f, flow, steps=4, cps=F32(1.0), mask=np.array([1, 0, 1]), out_in=poison, n_swept_in=np.full(3, -5), **OFF)
    assert (out[1] == 7).all() and cnt.tolist() == [4, -5, 4] and cnt.dtype == np.int32
    assert np.array_equal(out[0], out[2]) and _cells(out[0], 254) == [(i, 20) for i in range(21, 25)]


# ------------------------------------------------------------------ 4b. the GPU ladder's cases show what they are for
def _edges(sw):
    """Swept cells of (n, G, G) in the first 8 rows, the last 8 rows, the first 8 columns, the last 8 columns: (n, 4)."""
    return np.stack([sw[:, :8].sum(axis=(1, 2)), sw[:, -8:].sum(axis=(1, 2)), sw[:, :, :8].sum(axis=(1, 2)),
                     sw[:, :, -8:].sum(axis=(1, 2))], axis=1)


@functools.lru_cache(maxsize=None)
def _restated(G, n, which, ft, vt, knob):
    """(swept mask, n_swept) of a ladder case in one format pair: computed once per session."""
    f, v = K.cast(*K.case_planes(G, n, which), ft, vt)
    out, cnt = R.flow_predict(f, v, **dict(K.KNOBS, **K.knobs(knob, G)))
    assert cnt.sum() == (out == 254).sum()
    return out == 254, cnt


LADDER_CASES = [(G, n, knob, which, fmts) for knob, which, fmts, sizes in K.GPU_LADDER for G, n in K.LADDER if G in sizes]
LADDER_CASES.append(K.MANY + ("open", "overflow", K.ENDS[1:]))
LADDER_CASES += [(G, n, "open", "overflow", K.ENDS) for G, n in K.CORRECTED]


@pytest.mark.parametrize("G,n,knob,which,fmts", LADDER_CASES, ids=lambda v: v if isinstance(v, (int, str)) else str(len(v)))
def test_ladder_cases_put_bits_where_they_are_meant_to(G, n, knob, which, fmts):
    """Conditions on the restatement's output for every (G, knob set, density, format pair) that
    tests/test_gpu_flow_predict.py runs.  Not measurements: a generator that misses one gets another seed or
    density.  Measured with these planes, per case and format pair: open, the fewest swept cells in an 8-cell edge
    band of one env 438 on overflow and 19 on listed, the last 16 flat cells hit at every size; far gate, 384 or
    more swept cells per edge band of a case on overflow and 21 or more on listed, gated / open counts 0.23 to 0.39;
    moving sources per env 1,427 to 7,744 on overflow and 290 to 744 on listed."""
    for ft, vt in fmts:
        f, v = K.cast(*K.case_planes(G, n, which), ft, vt)
        moving = K.moving_sources(f, v)
        assert ((moving < K.LIST) if which == "listed" else (moving > K.LIST)).all(), (ft, vt, moving)
        sw, cnt = _restated(G, n, which, ft, vt, knob)
        edges = _edges(sw)
        if knob == "open":
            assert (edges > 0).all(), (ft, vt, edges)
            assert sw.reshape(n, -1)[:, -16:].any(), (ft, vt)
        elif knob == "far":
            assert (edges.sum(axis=0) > 0).all(), (ft, vt, edges)
            wide = _restated(G, n, which, ft, vt, "open")[1].sum()
            assert 0 < cnt.sum() < wide, (ft, vt, cnt.sum(), wide)
        else:  # default: why the other two exist
            assert G >= 128 and cnt.sum() > 0 and (edges == 0).all(), (ft, vt, edges)


@pytest.mark.parametrize("G,n", [s for s in K.LADDER if s[0] >= 128])
def test_default_knobs_reach_no_border_at_the_benchmark_grids_and_above(G, n):
    f, v = K.cast(*K.case_planes(G, n, "overflow"), np.float32, np.float32)
    out, cnt = R.flow_predict(f, v, **K.KNOBS)
    assert cnt.sum() > 0 and not _edges(out == 254).any()
    ii = np.nonzero(out == 254)
    assert max(np.abs(ii[1] - G // 2).max(), np.abs(ii[2] - G // 2).max()) <= 33  # (5 * 33) // 6 = 27 = steps + slack


def test_the_row_correction_runs_only_at_the_sizes_chosen_for_it():
    """pred_walk recovers the row of a flat cell as (int)((float)q * (1.0f / G)) and corrects it by one either way.
    Restated in float32: the correction downwards is never needed, the one upwards at 15 grids, none of them on the
    ladder; K.CORRECTED holds two, and their planes have moving sources on such cells in every env — sources that
    a kernel without the correction would walk from column G of the row above."""
    needing = {}
    for G in range(8, 516, 4):
        high, low = K.uncorrected_cells(G)
        assert not len(high), G
        if len(low):
            assert (low % G == 0).all()
            needing[G] = len(low)
    assert sorted(needing) == [164, 188, 220, 244, 328, 332, 376, 388, 428, 436, 440, 460, 484, 488, 492]
    assert not set(needing) & set(K.SIZES)
    for G, n in K.CORRECTED:
        assert needing[G] > 200 and (K.lds_bytes(G) > 65536) == (G == 460)
        for ft, vt in K.ENDS:
            f, v = K.cast(*K.case_planes(G, n, "overflow"), ft, vt)
            with np.errstate(all="ignore"):
                su, sv = v[:, 0].astype(F32) * K.KNOBS["cps"], v[:, 1].astype(F32) * K.KNOBS["cps"]
                moving = (f == 255) & np.isfinite(su) & np.isfinite(sv) & ~((su == 0) & (sv == 0))
            on = moving.reshape(n, -1)[:, K.uncorrected_cells(G)[1]].sum(axis=1)
            assert (on >= 20).all(), (G, ft, vt, on)


def test_ladder_sizes_sit_on_both_sides_of_the_lds_cap():
    assert [K.lds_bytes(g) for g in (404, 408, 508, 512)] == [65304, 66520, 100872, 102400]
    assert K.lds_bytes(404) <= 65536 < K.lds_bytes(408) and [g * g % 32 for g in (100, 260, 404, 508)] == [16] * 4
    assert K.knobs("far", 512)["pace"] == 28 and K.knobs("far", 100)["pace"] == 6
    # the moved generator at its default density is the one the earlier random test used
    a = K.planes(100, 3, seed=103)
    b = K.planes(100, 3, seed=103, density=0.03)
    assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b)) and K.moving_sources(*a).max() < K.LIST


# ------------------------------------------------------------------ 5. the C surface and its refusals
def test_header_binding_and_library_agree(lib):
    h = open(_abi.HEADER_PATH).read()
    assert int(re.search(r"#define FFMP_ABI_VERSION (\d+)", h).group(1)) == 9 == _abi.ABI_VERSION
    assert lib.ffmp_abi_version() == 9
    code = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    for name, count in (("ffmp_flow_predict", 19), ("ffmp_flow_predict_check", 9)):
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, code)
        assert m, name
        params = [p.strip() for p in m.group(1).split(",")]
        res, args = _abi._SIGS[name]
        assert res is C.c_int and len(args) == len(params) == count, (name, params)
        assert hasattr(lib, name)
    decl = h.index("int ffmp_flow_predict(")
    comment = h[h.rindex("/*", 0, decl):decl]
    for word in ("[unpinned]", "occ[a]  = F[a] > 0", "src[a]  = F[a] == 255", "su = vx[a] * cps", "(int)rintf((float)k * su)",
                 "ka = (5*m + 2*n) / pace", "|k - ka| <= slack", "F[a] == 255 ? 255 : occ[a] ? other : bit[a] ? swept : 0",
                 "n_swept = number of cells with bit && !occ", "slack = -1", "constant-velocity", "footprint dilation",
                 "straight-line bound"):
        assert word in comment, word
    assert "ffmp_flow_predict   ->" in h[:h.index("#ifndef FFMP_H")]
    from flow_field_based_motion_planner_amd import env, vec_env
    sig = inspect.signature(vec_env.FFMPVec.predicted_frames)
    names = ("flow", "frames", "steps", "slack", "dt", "speed", "swept", "other", "out", "mask", "count")
    assert [sig.parameters[k].default for k in names] == [None, None, 24, 3, None, 0.6, 254, 128, None, None, False]
    for fn in (vec_env.FFMPVec.nav_field, vec_env.FFMPVec.policy_nav):
        assert inspect.signature(fn).parameters["predict"].default is False
    assert callable(env.FFMP.predicted_frames)
    cfg = FFMPConfig()
    assert R.host_knobs(cfg.dt, cfg.res) == (F32(2.0), 6)


P = 1 << 20  # never dereferenced: every call below is refused, or has n == 0
G2 = G * G
KNOBS = dict(steps=24, cps=2.0, pace=6, slack=3, swept=254, other=128)
FLOW = P + (1 << 20)
OUT = P + (2 << 20)


def _call(lib, cfg, n=4, frame=P, frame_stride=G2, ffmt=0, flow=FLOW, flow_stride=2 * G2, vfmt=0, mask=None, out=OUT, out_stride=G2,
          n_swept=None, **knobs):
    k = dict(KNOBS, **knobs)
    return lib.ffmp_flow_predict(C.byref(cfg), n, frame, frame_stride, ffmt, flow, flow_stride, vfmt, mask, out, out_stride, n_swept,
                                 k["steps"], k["cps"], k["pace"], k["slack"], k["swept"], k["other"], None)


def test_argument_checks_without_a_launch(lib):
    cfg = _abi.make_cfg(FFMPConfig(grid=G, n_obst=4, n_beams=0))
    E = -1  # FFMP_E_ARG

    def chk(c=cfg, ffmt=0, vfmt=0, **knobs):
        k = dict(KNOBS, **knobs)
        return lib.ffmp_flow_predict_check(C.byref(c), ffmt, vfmt, k["steps"], k["cps"], k["pace"], k["slack"], k["swept"], k["other"])

    assert chk() == 0
    for g in (4, 516, 1024, 66, 0):
        bad = _abi.make_cfg(FFMPConfig(grid=G, n_obst=4, n_beams=0))
        bad.grid = g
        assert _call(lib, bad, frame_stride=1 << 30, flow_stride=1 << 30, out_stride=1 << 30) == E and b"grid" in lib.ffmp_last_error(), g
        assert chk(bad) == E and b"grid" in lib.ffmp_last_error()
    knob_cases = [(dict(steps=0), b"steps"), (dict(steps=65), b"steps"), (dict(pace=0), b"pace"), (dict(pace=1025), b"pace"),
                  (dict(slack=-2), b"slack"), (dict(slack=256), b"slack"), (dict(swept=-1), b"swept"), (dict(swept=256), b"swept"),
                  (dict(other=-1), b"other"), (dict(other=256), b"other"), (dict(cps=NAN), b"cps"), (dict(cps=INF), b"cps"),
                  (dict(cps=-INF), b"cps"), (dict(cps=-0.5), b"cps"), (dict(ffmt=2), b"frame_format"), (dict(ffmt=-1), b"frame_format"),
                  (dict(vfmt=2), b"flow_format"), (dict(vfmt=-1), b"flow_format")]
    cases = knob_cases + [
        (dict(frame=None), b"frame is NULL"), (dict(flow=None), b"flow is NULL"), (dict(out=None), b"out is NULL"),
        (dict(frame_stride=G2 - 4), b"frame_env_stride"), (dict(flow_stride=2 * G2 - 4), b"flow_env_stride"),
        (dict(out_stride=G2 - 4), b"out_env_stride"),
        (dict(frame=P + 2), b"frame alignment"), (dict(frame=P + 1, ffmt=1), b"frame alignment"), (dict(frame_stride=G2 + 2), b"frame alignment"),
        (dict(flow=FLOW + 2), b"flow alignment"), (dict(flow=FLOW + 2, vfmt=1), b"flow alignment"), (dict(flow_stride=2 * G2 + 2), b"flow alignment"),
        (dict(out=OUT + 2), b"out alignment"), (dict(out_stride=G2 + 2), b"out alignment"), (dict(n_swept=P - 2), b"n_swept"),
        # out on top of the frame or the flow, either way round, at its first or last byte
        (dict(out=P), b"overlap"), (dict(out=P + 4 * (4 * G2) - 4), b"overlap"), (dict(out=P - 4 * G2 + 4), b"overlap"),
        (dict(out=P + 4 * G2 - 4, ffmt=1), b"overlap"), (dict(out=FLOW), b"overlap"), (dict(out=FLOW + 4 * (8 * G2) - 4), b"overlap"),
        (dict(out=FLOW + 2 * (8 * G2) - 4, vfmt=1), b"overlap"), (dict(n_swept=OUT + 8), b"overlap"), (dict(n_swept=P + 8), b"overlap"),
        (dict(n=-1), b"negative n"), (dict(n=1 << 40), b"too large")]
    for kw, word in cases:
        assert _call(lib, cfg, **kw) == E, kw
        assert word in lib.ffmp_last_error(), (kw, lib.ffmp_last_error())
        assert lib.ffmp_last_error().startswith(b"ffmp_flow_predict:")
    for kw, word in knob_cases:
        assert chk(**kw) == E and word in lib.ffmp_last_error(), kw
    assert lib.ffmp_flow_predict_check(None, 0, 0, 24, 2.0, 6, 3, 254, 128) == E
    assert lib.ffmp_flow_predict(None, 0, P, G2, 0, FLOW, 2 * G2, 0, None, OUT, G2, None, 24, 2.0, 6, 3, 254, 128, None) == E
    # the bounds themselves pass the checks: n == 0 launches nothing
    for kw in (dict(steps=1), dict(steps=64), dict(pace=1), dict(pace=1024), dict(slack=-1), dict(slack=255), dict(swept=0, other=0),
               dict(swept=255, other=255), dict(cps=0.0), dict(cps=1e30), dict(ffmt=1), dict(vfmt=1), dict(ffmt=1, vfmt=1),
               dict(frame=P + 4), dict(frame=P + 4, ffmt=1), dict(flow=FLOW + 4), dict(flow=FLOW + 4, vfmt=1), dict(out=OUT + 4),
               dict(mask=P), dict(n_swept=P), dict(frame_stride=G2 + 4), dict(flow_stride=2 * G2 + 4), dict(out_stride=G2 + 4),
               dict(out=P)):
        assert _call(lib, cfg, n=0, **kw) == 0, (kw, lib.ffmp_last_error())
    for g in (8, 36, 100, 512):
        ok = _abi.make_cfg(FFMPConfig(grid=g, n_obst=1, n_beams=0))
        assert _call(lib, ok, n=0, frame_stride=g * g, flow_stride=2 * g * g, out_stride=g * g) == 0
        assert chk(ok, 1, 1, steps=64, cps=0.0, pace=1024, slack=-1, swept=0, other=255) == 0


# ------------------------------------------------------------------ 6. the physical tie to the oracle
def test_the_predicted_plan_passes_behind_a_crossing_disc():
    """The untouched NumPy oracle in closed loop with tests/nav_field_ref.py's planner and follower on the crossing
    family (R.CROSS_CFG: G = 64, flow=True, world_half 2.0, 120 steps, no autoreset; robot (-1, 0, yaw 0), goal
    (1, 0); a disc of r = 0.25 at (0, y0) moving at (0, v), v in 0.2..0.5 m/s, y0 in -0.3..-1.3 m: 24 scenes),
    planning over the newest frame (plain) and over the predicted plane of the newest frame and the ground-truth
    flow (steps 24, slack 3, pace 6, cps 2).  Measured (python tests/flow_predict_ref.py), outcomes per scene
    (1 goal, 2 collision, 3 truncated):
        plain            112111112211111221111222   8 collisions, 16 goals, 36.1 steps per reached goal
        predicted        112111111111111111111111   1 collision, 23 goals, 43.8 steps per reached goal
        gate off (-1)    111121111133111111111111   1 collision, 21 goals, 2 not there after 120 steps, 52.1 steps
    Caps: the plain planner collides in at least 6 scenes, the predicted one in at most 3 and reaches the goal in
    all the others."""
    cfg = FFMPConfig(**R.CROSS_CFG)
    assert R.host_knobs(cfg.dt, cfg.res) == (F32(2.0), 6) and len(R.crossing_scenes()["pose"]) == 24
    o0, t0 = R.crossing_closed_loop(None)
    o1, t1 = R.crossing_closed_loop(dict(steps=24, slack=3))
    print("plain    ", "".join(map(str, o0.tolist())), t0.tolist(), R.summary(o0, t0))
    print("predicted", "".join(map(str, o1.tolist())), t1.tolist(), R.summary(o1, t1))
    assert (o0 == 2).sum() >= 6
    assert (o1 == 2).sum() <= 3
    assert ((o1 == 1) | (o1 == 2)).all()
    # the record the GPU's closed loop is compared with (tests/test_gpu_flow_predict.py) is this run
    with open(R.GOLDEN) as f:
        gold = json.load(f)
    assert gold == {"plain": {"outcome": o0.tolist(), "step": t0.tolist()}, "predicted": {"outcome": o1.tolist(), "step": t1.tolist()}}
