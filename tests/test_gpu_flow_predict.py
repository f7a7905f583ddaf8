"""Predicted-occupancy frames on the GPU (include/ffmp.h ffmp_flow_predict) against
their NumPy restatement (tests/flow_predict_ref.py), bit for bit:

1. random planes in the four frame x flow formats at G = 8, 64, 100 and n = 1, 3, 70 — about 3 % sources, flows
   within +-2 cells per step, NaN / inf / -0.0 flows, sources on all four borders pointing outward —, and a
   plane whose every cell is a source;
2. the corners of the knobs;
3. mask=, env strides of a larger buffer, and bases aligned to 4 but not 16 bytes (the 4-byte loads and stores);
3b. the size ladder of tests/flow_predict_cases.py — G = 100, 128, 256, 260, 404, 408, 508, 512: both benchmark
   grids, both sides of the 64 KiB cap of dynamic LDS, the half-used last bit word — with the gate off and with a
   gate that reaches the border, below and above 1,024 moving sources per env (gate off and above in the four
   formats, the rest in float32 / float32 and uint8 / binary16); the default knobs at 256 and 512; 256 with n = 70;
   244 and 460, where pred_walk's row correction runs; the 4-byte paths at 408; mask= at 512.
   tests/test_flow_predict_host.py proves on the restatement that these cases sweep the borders and the last word;
4. FFMPVec.predicted_frames over the env's own frame and flow and over a LidarFlow, nav_field / policy_nav
   with predict=, the errors; the surface on live envs at G = 256 (untiled planner) and 260 (tiled);
5. the crossing family in closed loop: the outcomes of the CPU run, scene by scene and step by step;
6. inside a graph capture of the caller's; in a fresh process (tests/first_capture_child.py), the first launch above
   64 KiB of LDS made while capturing, for ffmp_flow_predict, ffmp_frame_potential and ffmp_scan_flow."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from flow_field_based_motion_planner_amd import _abi
from flow_field_based_motion_planner_amd.config import FFMPConfig
from flow_field_based_motion_planner_amd.env import FFMP
from flow_field_based_motion_planner_amd.vec_env import FFMPVec
from tests import flow_predict_cases as K
from tests import flow_predict_ref as R
from tests import nav_field_ref as NR
from tests.scan_flow_ref import TIE

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
KNOBS, FORMATS = K.KNOBS, K.FORMATS
_planes = K.planes


def _t(x):
    return torch.as_tensor(np.ascontiguousarray(x), device=DEV)


def _cfg(G):
    return _abi.make_cfg(FFMPConfig(grid=G, n_obst=1, n_beams=0))


def _launch(lib, G, frame, flow, out, n_swept=None, mask=None, frame_stride=None, flow_stride=None, out_stride=None, n=None,
            **knobs):
    """ffmp_flow_predict over device tensors (any view whose env planes are dense) on the default stream."""
    k = dict(KNOBS, **knobs)
    cfg = _cfg(G)
    fmt = lambda t: _abi.OBS_F32 if t.dtype == torch.float32 else _abi.OBS_U8F16  # noqa: E731
    rc = lib.ffmp_flow_predict(C.byref(cfg), frame.shape[0] if n is None else n, frame.data_ptr(),
                               frame.stride(0) if frame_stride is None else frame_stride, fmt(frame), flow.data_ptr(),
                               flow.stride(0) if flow_stride is None else flow_stride, fmt(flow),
                               None if mask is None else mask.data_ptr(), out.data_ptr(),
                               out.stride(0) if out_stride is None else out_stride,
                               None if n_swept is None else n_swept.data_ptr(), int(k["steps"]), float(k["cps"]), int(k["pace"]),
                               int(k["slack"]), int(k["swept"]), int(k["other"]), None)
    assert rc == 0, lib.ffmp_last_error()
    torch.cuda.synchronize()


def _same(got, exp, where):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.dtype == exp.dtype and got.shape == exp.shape, (where, got.dtype, got.shape)
    bad = np.nonzero(got != exp)
    assert not len(bad[0]), (where, len(bad[0]), [b[:5] for b in bad], got[bad][:5], exp[bad][:5])


def _run(lib, G, frame, flow, ft, vt, where, **knobs):
    n = frame.shape[0]
    with np.errstate(over="ignore"):
        f, v = frame.astype(ft), flow.astype(vt)
        exp, cnt = R.flow_predict(f, v, **dict(KNOBS, **knobs))
    out = torch.full((n, G, G), 7, dtype=torch.uint8, device=DEV)
    n_swept = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    _launch(lib, G, _t(f), _t(v), out, n_swept, **knobs)
    _same(out, exp, (where, "out"))
    _same(n_swept, cnt, (where, "n_swept"))
    return exp, cnt


# ------------------------------------------------------------------ 1. random and dense planes
@pytest.mark.parametrize("G", [8, 64, 100])
@pytest.mark.parametrize("n", [1, 3, 70])
def test_random_planes_equal_the_restatement(lib, G, n):
    frame, flow = _planes(G, n, seed=G + n)
    f32 = frame.copy()  # values only a float32 frame can hold
    f32[:, 1, 1::5] = np.nan
    f32[:, 2, 1::5] = -4.0
    f32[:, 3, 1::5] = 0.25
    f32[:, 4, 1::5] = 255.5
    swept = others = 0
    for ft, vt in FORMATS:
        with np.errstate(over="ignore"):
            exp, cnt = _run(lib, G, f32 if ft is np.float32 else frame, flow, ft, vt, (G, n, ft.__name__, vt.__name__))
        swept += int(cnt.sum())
        others += int((exp == 128).sum())
        assert cnt.sum() == (exp == 254).sum()
    assert swept > 0 and (others > 0 or G == 8)  # the case shows something


def test_every_cell_a_source(lib):
    frame, flow = _planes(64, 3, seed=5, dense=True)
    for ft, vt in FORMATS:
        exp, cnt = _run(lib, 64, frame, flow, ft, vt, ("dense", ft.__name__, vt.__name__), slack=-1)
        assert (exp == 255).all() and (cnt == 0).all()
    # the same crowd of sources onto free cells: every second row a row of sources
    frame[:, 1::2] = 0
    for slack in (-1, 3):
        exp, cnt = _run(lib, 64, frame, flow, np.float32, np.float32, ("rows", slack), slack=slack)
        assert (cnt > 0).all()


# ------------------------------------------------------------------ 2. the corners of the knobs
def test_knob_corners(lib):
    frame, flow = _planes(64, 3, seed=9)
    seen = set()
    for steps in (1, 64):
        for slack in (-1, 0, 255):
            for pace in (1, 1024):
                exp, cnt = _run(lib, 64, frame, flow, np.float32, np.float32, (steps, slack, pace), steps=steps, slack=slack, pace=pace)
                seen.add(int(cnt.sum()))
    assert len(seen) >= 3
    _run(lib, 64, frame, flow, np.uint8, np.float16, "bytes", swept=0, other=255)
    _run(lib, 64, frame, flow, np.uint8, np.float16, "bytes", swept=255, other=0)
    exp, cnt = _run(lib, 64, frame, flow, np.float32, np.float32, "cps 0", cps=F32(0.0))
    assert (cnt == 0).all()
    _run(lib, 64, frame, flow, np.float32, np.float32, "cps large", cps=F32(1e30))
    _run(lib, 64, frame, flow, np.float32, np.float32, "cps fraction", cps=F32(0.37))


# ------------------------------------------------------------------ 3. mask, strides, alignment
def test_mask_strides_and_unaligned_bases(lib):
    G, n = 64, 5
    G2 = G * G
    frame, flow = _planes(G, n, seed=11)
    exp, cnt = R.flow_predict(frame, flow, **KNOBS)
    with np.errstate(over="ignore"):
        cast = {(ft, vt): (frame.astype(ft), flow.astype(vt)) for ft, vt in FORMATS}  # 3e38 is inf in binary16
    # mask=: the envs left out keep their poisoned cells and their count
    mask = np.array([1, 0, 1, 1, 0], np.uint8)
    out = torch.full((n, G, G), 7, dtype=torch.uint8, device=DEV)
    n_swept = torch.full((n,), -9, dtype=torch.int32, device=DEV)
    _launch(lib, G, _t(frame), _t(flow), out, n_swept, mask=_t(mask))
    m = mask.astype(bool)
    _same(out, np.where(m[:, None, None], exp, 7).astype(np.uint8), "mask out")
    _same(n_swept, np.where(m, cnt, -9).astype(np.int32), "mask n_swept")
    # the frame as state_m[:, 1] of a frame pair, the flow and the output out of larger buffers
    for ft, vt in FORMATS:
        pair = torch.full((n, 2, G, G), 255, dtype=torch.float32 if ft is np.float32 else torch.uint8, device=DEV)
        fc, vc = cast[ft, vt]
        pair[:, 1] = _t(fc)
        big = torch.full((n, 3, G, G), 1.0, dtype=torch.float32 if vt is np.float32 else torch.float16, device=DEV)
        big[:, :2] = _t(vc)
        wide = torch.full((n, G2 + 16), 7, dtype=torch.uint8, device=DEV)
        e2, c2 = R.flow_predict(fc, vc, **KNOBS)
        _launch(lib, G, pair[:, 1], big, wide)
        assert pair[:, 1].stride(0) == 2 * G2 and big.stride(0) == 3 * G2
        _same(wide[:, :G2].reshape(n, G, G), e2, ("strides", ft.__name__, vt.__name__))
        assert (wide[:, G2:] == 7).all()
        # bases aligned to 4 but not to 16 bytes, env strides that are no multiple of 16 bytes: 4-byte loads and stores
        fe = 4 // np.dtype(ft).itemsize  # elements in 4 bytes
        fbuf = torch.zeros(n * (G2 + 4) + fe, dtype=pair.dtype, device=DEV)
        fv = fbuf[fe:].reshape(n, G2 + 4)
        fv[:, :G2] = _t(fc).reshape(n, G2)
        ve = 4 // np.dtype(vt).itemsize
        vbuf = torch.zeros(n * (2 * G2 + 4) + ve, dtype=big.dtype, device=DEV)
        vv = vbuf[ve:].reshape(n, 2 * G2 + 4)
        vv[:, :2 * G2] = _t(vc).reshape(n, 2 * G2)
        obuf = torch.full((n * (G2 + 4) + 4,), 7, dtype=torch.uint8, device=DEV)
        ov = obuf[4:].reshape(n, G2 + 4)
        assert fv.data_ptr() % 16 == 4 and vv.data_ptr() % 16 == 4 and ov.data_ptr() % 16 == 4
        _launch(lib, G, fv, vv, ov)
        _same(ov[:, :G2].reshape(n, G, G), e2, ("unaligned", ft.__name__, vt.__name__))
        assert (ov[:, G2:] == 7).all() and (obuf[:4] == 7).all()
    # n == 0 launches nothing
    out = torch.full((n, G, G), 7, dtype=torch.uint8, device=DEV)
    _launch(lib, G, _t(frame), _t(flow), out, n=0)
    assert (out == 7).all()


# ------------------------------------------------------------------ 3b. the size ladder (tests/flow_predict_cases.py)
def _ladder(lib, G, n, knob, which, fmts):
    """A ladder case in the given format pairs against the restatement; tests/test_flow_predict_host.py holds the proof
    that the case puts bits at the borders, in the last word and on the stated side of the list."""
    frame, flow = K.case_planes(G, n, which)
    for ft, vt in fmts:
        f, v = K.cast(frame, flow, ft, vt)
        exp, cnt = _run(lib, G, f, v, ft, vt, (G, n, knob, which, ft.__name__, vt.__name__), **K.knobs(knob, G))
        assert cnt.sum() == (exp == 254).sum() and cnt.sum() > 0


@pytest.mark.parametrize("G,n", K.LADDER)
@pytest.mark.parametrize("knob,which,fmts", [c[:3] for c in K.GPU_LADDER[:4]], ids=lambda v: v if isinstance(v, str) else str(len(v)))
def test_ladder_equals_the_restatement(lib, G, n, knob, which, fmts):
    _ladder(lib, G, n, knob, which, fmts)


@pytest.mark.parametrize("G", K.GPU_LADDER[4][3])
def test_ladder_default_knobs_at_the_timed_grids(lib, G):
    knob, which, fmts, _ = K.GPU_LADDER[4]
    _ladder(lib, G, dict(K.LADDER)[G], knob, which, fmts)


def test_ladder_many_envs_at_256(lib):
    _ladder(lib, *K.MANY, "open", "overflow", K.ENDS[1:])


@pytest.mark.parametrize("G,n", K.CORRECTED)
def test_sizes_at_which_the_row_correction_runs(lib, G, n):
    """No ladder size makes pred_walk's float quotient miss the row (tests/test_flow_predict_host.py); these two do."""
    _ladder(lib, G, n, "open", "overflow", K.ENDS)


def test_unaligned_bases_and_padded_strides_at_408(lib):
    """The 4-byte loads and stores on the opt-in branch: bases at 4 mod 16 bytes, env strides of G*G + 4 elements."""
    G, n = 408, 2
    G2 = G * G
    frame, flow = K.case_planes(G, n, "overflow")
    knobs = K.knobs("open", G)
    for ft, vt in K.ENDS:
        fc, vc = K.cast(frame, flow, ft, vt)
        exp, cnt = R.flow_predict(fc, vc, **dict(KNOBS, **knobs))
        fe = 4 // np.dtype(ft).itemsize  # elements in 4 bytes
        fbuf = torch.zeros(n * (G2 + 4) + fe, dtype=torch.float32 if ft is np.float32 else torch.uint8, device=DEV)
        fv = fbuf[fe:].reshape(n, G2 + 4)
        fv[:, :G2] = _t(fc).reshape(n, G2)
        ve = 4 // np.dtype(vt).itemsize
        vbuf = torch.zeros(n * (2 * G2 + 4) + ve, dtype=torch.float32 if vt is np.float32 else torch.float16, device=DEV)
        vv = vbuf[ve:].reshape(n, 2 * G2 + 4)
        vv[:, :2 * G2] = _t(vc).reshape(n, 2 * G2)
        obuf = torch.full((n * (G2 + 4) + 4,), 7, dtype=torch.uint8, device=DEV)
        ov = obuf[4:].reshape(n, G2 + 4)
        n_swept = torch.full((n,), -1, dtype=torch.int32, device=DEV)
        assert fv.data_ptr() % 16 == 4 and vv.data_ptr() % 16 == 4 and ov.data_ptr() % 16 == 4
        _launch(lib, G, fv, vv, ov, n_swept, **knobs)
        _same(ov[:, :G2].reshape(n, G, G), exp, ("unaligned 408", ft.__name__, vt.__name__))
        _same(n_swept, cnt, ("unaligned 408 n_swept", ft.__name__, vt.__name__))
        assert (ov[:, G2:] == 7).all() and (obuf[:4] == 7).all()
        assert cnt.sum() == (exp == 254).sum() and cnt.sum() > 0


def test_mask_at_512(lib):
    G, n = 512, 2
    frame, flow = K.cast(*K.case_planes(G, n, "overflow"), np.float32, np.float32)
    knobs = K.knobs("open", G)
    exp, cnt = R.flow_predict(frame, flow, **dict(KNOBS, **knobs))
    out = torch.full((n, G, G), 7, dtype=torch.uint8, device=DEV)
    n_swept = torch.full((n,), -9, dtype=torch.int32, device=DEV)
    _launch(lib, G, _t(frame), _t(flow), out, n_swept, mask=_t(np.array([1, 0], np.uint8)), **knobs)
    _same(out[0], exp[0], "mask 512, env 0")
    assert (out[1] == 7).all() and n_swept.tolist() == [int(cnt[0]), -9]
    assert cnt[0] == (exp[0] == 254).sum() and cnt[0] > 0


# ------------------------------------------------------------------ 4. FFMPVec
def _expect(env, frame=None, flow=None, **kw):
    cps, pace = R.host_knobs(kw.pop("dt", env.cfg.dt), env.cfg.res, kw.pop("speed", 0.6))
    frame = env.state_m[:, 1] if frame is None else frame
    flow = env.obs["flow"] if flow is None else flow
    return R.flow_predict(frame.cpu().numpy(), flow.cpu().numpy(), cps=cps, pace=pace, **dict(R.DEFAULTS, **kw))


@pytest.mark.parametrize("fmt", ["f32", "u8f16"])
def test_predicted_frames_of_a_live_env(fmt):
    cfg = FFMPConfig(**TIE[64])
    n = 6
    env = FFMPVec(n, cfg, device=DEV, autotune=False, obs_format=fmt)
    with pytest.raises(RuntimeError, match="reset"):
        env.predicted_frames()
    env.reset()
    lf = env.lidar_flow(lag=2)
    lf.update()
    rng = np.random.default_rng(2)
    for _ in range(5):
        env.step(torch.as_tensor(rng.integers(21, 28, n), device=DEV))
        lf.update()
    assert env.obs["flow"].dtype == (torch.float16 if fmt == "u8f16" else torch.float32)
    exp, cnt = _expect(env)
    assert cnt.sum() > 0
    got = env.predicted_frames()
    assert got.dtype == torch.uint8 and tuple(got.shape) == (n, 64, 64)
    _same(got, exp, (fmt, "own flow"))
    out = torch.empty_like(got)
    res = env.predicted_frames(out=out, count=True)
    assert res[0] is out and res[1].dtype == torch.int32
    _same(out, exp, (fmt, "out="))
    _same(res[1], cnt, (fmt, "count"))
    # knobs, dt and speed
    kw = dict(steps=10, slack=1, dt=0.2, speed=0.3, swept=9, other=200)
    _same(env.predicted_frames(**kw), _expect(env, **kw)[0], (fmt, "knobs"))
    assert R.host_knobs(0.2, cfg.res, 0.3) == (F32(4.0), 6) and R.host_knobs(cfg.dt, cfg.res, 0.0)[1] == 1
    _same(env.predicted_frames(speed=0.0, slack=-1), _expect(env, speed=0.0, slack=-1)[0], (fmt, "pace 1"))
    # mask
    mask = torch.as_tensor([True, False, True, True, False, True], device=DEV)
    poisoned = torch.full_like(got, 7)
    env.predicted_frames(out=poisoned, mask=mask)
    _same(poisoned, np.where(mask.cpu().numpy()[:, None, None], exp, 7).astype(np.uint8), (fmt, "mask"))
    # the estimated flow over the scan frame, and a flow / frame of the caller's
    assert (lf.flow != 0).any()
    e2, c2 = _expect(env, frame=lf.frame, flow=lf.flow)
    got2, n2 = env.predicted_frames(flow=lf, count=True)
    _same(got2, e2, (fmt, "LidarFlow"))
    _same(n2, c2, (fmt, "LidarFlow count"))
    assert c2.sum() > 0
    _same(env.predicted_frames(flow=lf.flow), _expect(env, flow=lf.flow)[0], (fmt, "flow tensor"))
    _same(env.predicted_frames(flow=lf.flow.float(), frames=lf.frame), e2, (fmt, "uint8 frame, float32 flow"))
    _same(env.predicted_frames(frames=lf.frame.float().contiguous()), _expect(env, frame=lf.frame)[0], (fmt, "frames="))
    # the planner over the predicted plane
    for kw, plane in ((dict(predict=True), got), (dict(predict=dict(steps=10, slack=1)), env.predicted_frames(steps=10, slack=1)),
                      (dict(predict=lf), got2)):
        assert torch.equal(env.policy_nav(**kw), env.policy_nav(frames=plane))
        a, b = env.nav_field(cost=True, **kw), env.nav_field(cost=True, frames=plane)
        assert all(torch.equal(a[k], b[k]) for k in ("cost", "target", "geo_cost"))
    goals = env.record[:, 8:10].cpu().numpy()
    _same(env.policy_nav(predict=True), NR.nav_field(exp, goals, cfg)["cmd"], (fmt, "policy_nav(predict=True)"))
    assert torch.equal(env.policy_nav(predict=False), env.policy_nav())
    # the errors
    for what in (env.policy_nav, env.nav_field):
        for kw in (dict(frames=got), dict(visible=True), dict(lidar=True), dict(lidar_map=env.lidar_map())):
            with pytest.raises(ValueError, match="pass one of frames, visible=True, lidar=True, lidar_map and predict"):
                what(predict=True, **kw)
        for bad in (3, "yes", dict(out=out), dict(count=True)):
            with pytest.raises(ValueError, match="predict"):
                what(predict=bad)
    other_env = FFMPVec(n, cfg, device=DEV, autotune=False, obs_format=fmt)
    other_env.reset()
    with pytest.raises(ValueError, match="LidarFlow of this env"):
        other_env.predicted_frames(flow=lf)
    other_env.close()
    for kw, word in ((dict(dt=0.0), "dt"), (dict(dt=-1.0), "dt"), (dict(dt=float("nan")), "dt"), (dict(dt=1e300), "res"),
                     (dict(speed=-1.0), "speed"), (dict(speed=1e6), "speed"), (dict(flow=lf.flow[:, :1]), "flow"),
                     (dict(flow=lf.flow.double()), "flow"), (dict(frames=got[:, :32]), "frames"), (dict(out=got[:3]), "out"),
                     (dict(out=got.float()), "out")):
        with pytest.raises(ValueError, match=word):
            env.predicted_frames(**kw)
    for kw in (dict(steps=0), dict(steps=65), dict(slack=-2), dict(slack=256), dict(swept=256), dict(other=-1)):
        with pytest.raises(_abi.FFMPBackendError):
            env.predicted_frames(**kw)
    env.close()


@pytest.mark.parametrize("fmt", ["f32", "u8f16"])
@pytest.mark.parametrize("G", [256, 260])
def test_predicted_frames_at_the_benchmark_grid_and_above(G, fmt):
    """C3's grid, where the planner holds the plane in LDS, and 256 + 4, where it goes through ffmp_nav_field_tiled:
    the surface over a real frame ring's strides, the far-reaching call, and the planner over the predicted plane."""
    cfg = FFMPConfig(grid=G, n_obst=12, n_beams=0, moving=True, flow=True, world_half=3.0, goal_min=1.0, goal_max=3.5,
                     obst_rmax=0.6, obst_vmax=1.0, max_steps=50, seed=8)
    n = 2
    env = FFMPVec(n, cfg, device=DEV, autotune=False, obs_format=fmt)
    env.reset()
    for a in (24, 3, 25):
        env.step(torch.full((n,), a, dtype=torch.int64, device=DEV))
    assert (env._nav_tiled(None) is not None) == (G > 256)
    exp, cnt = _expect(env)
    assert cnt.sum() > 0
    _same(env.predicted_frames(), exp, (G, fmt, "own flow"))
    got, n_swept = env.predicted_frames(count=True)
    _same(got, exp, (G, fmt, "count=True"))
    _same(n_swept, cnt, (G, fmt, "count"))
    far, far_cnt = _expect(env, slack=-1, steps=64)
    assert far_cnt.sum() > cnt.sum()
    got_far, n_far = env.predicted_frames(slack=-1, steps=64, count=True)
    _same(got_far, far, (G, fmt, "gate off, 64 steps"))
    _same(n_far, far_cnt, (G, fmt, "gate off, 64 steps, count"))
    goals = env.record[:, 8:10].cpu().numpy()
    _same(env.policy_nav(predict=True), NR.nav_field(exp, goals, cfg)["cmd"], (G, fmt, "policy_nav(predict=True)"))
    for kw, plane in ((dict(predict=True), got), (dict(predict=dict(slack=-1, steps=64)), got_far)):
        a, b = env.nav_field(cost=True, **kw), env.nav_field(cost=True, frames=plane)
        assert all(torch.equal(a[k], b[k]) for k in ("cost", "target", "geo_cost")), (G, fmt, kw)
    env.close()


def test_without_flow_planes_and_the_single_env():
    cfg = FFMPConfig(grid=64, n_obst=4, n_beams=0, moving=True)
    env = FFMPVec(2, cfg, device=DEV, autotune=False)
    env.reset()
    with pytest.raises(ValueError, match="flow=True"):
        env.predicted_frames()
    with pytest.raises(ValueError, match="flow=True"):
        env.policy_nav(predict=True)
    flow = torch.zeros((2, 2, 64, 64), device=DEV)
    flow[:, 0] = 0.5
    _same(env.predicted_frames(flow=flow), _expect(env, flow=flow)[0], "a flow of the caller's")
    env.close()
    one = FFMP(FFMPConfig(**TIE[64]), device=DEV, verbose=False)
    with pytest.raises(RuntimeError):
        one.predicted_frames()
    one.reset()
    one.step(24)
    got, cnt = one.predicted_frames(count=True)
    exp, c = _expect(one._vec_env())
    _same(got, exp, "single env")
    _same(cnt, c, "single env count")
    one.close()


# ------------------------------------------------------------------ 5. the crossing family in closed loop
def _gpu_closed_loop(predict):
    cfg = FFMPConfig(**R.CROSS_CFG)
    sc = R.crossing_scenes()
    env = FFMPVec(len(sc["pose"]), cfg, device=DEV, autotune=False)
    env.reset()
    env.set_scenarios(**sc)
    env.check_errors()
    flags = []
    for _ in range(R.CROSS_STEPS):
        env.step(env.policy_nav(predict=predict))
        flags.append((env.is_goal.cpu().numpy().copy(), env.collision.cpu().numpy().copy(), env.truncated.cpu().numpy().copy()))
        if (NR._outcomes(flags)[0] != 0).all():
            break
    env.check_errors()
    env.close()
    return NR._outcomes(flags)


def test_crossing_family_equals_the_cpu_closed_loop():
    """The 24 crossing scenes (tests/flow_predict_ref.py) through set_scenarios, stepped with
    policy_nav(predict=dict(steps=24, slack=3)) and with plain policy_nav(): the per-env outcome and the step it
    happened at equal the CPU run (the NumPy oracle driven by the restatements), recorded in
    tests/golden/flow_predict_crossing.json and recomputed by tests/test_flow_predict_host.py.  Every link is
    bit-exact, so equality is the assertion."""
    with open(R.GOLDEN) as f:
        gold = json.load(f)
    for name, predict in (("predicted", dict(steps=24, slack=3)), ("plain", False)):
        o, t = _gpu_closed_loop(predict)
        print(name, "".join(map(str, o.tolist())), t.tolist())
        assert o.tolist() == gold[name]["outcome"] and t.tolist() == gold[name]["step"], name
    assert sum(x == 2 for x in gold["plain"]["outcome"]) >= 6 and sum(x == 2 for x in gold["predicted"]["outcome"]) <= 3


# ------------------------------------------------------------------ 6. inside a graph capture
def test_first_opt_in_launch_of_a_process_inside_a_capture():
    """tests/first_capture_child.py in a fresh process: for ffmp_flow_predict, ffmp_frame_potential and ffmp_scan_flow
    the first call of the process above 64 KiB of dynamic LDS (grid 512) is made while a stream is capturing, and the
    replay equals the restatement.  One child, no retries: a non-zero exit or the time limit is the failure."""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "first_capture_child.py")
    done = subprocess.run([sys.executable, child], capture_output=True, text=True, timeout=120)
    print(done.stdout, done.stderr)
    assert done.returncode == 0, (done.returncode, done.stdout[-2000:], done.stderr[-2000:])
    seen = [json.loads(line) for line in done.stdout.splitlines() if line.startswith("{")]
    assert [(r["pass"], r["outcome"]) for r in seen] == [("ffmp_flow_predict", "match"), ("ffmp_frame_potential", "match"),
                                                        ("ffmp_scan_flow", "match")], seen


def test_graph_capture():
    cfg = FFMPConfig(**TIE[64])
    n = 4
    env = FFMPVec(n, cfg, device=DEV, autotune=False, frame_window=2)
    env.reset()
    env.step(torch.full((n,), 24, device=DEV))
    out = torch.empty((n, 64, 64), dtype=torch.uint8, device=DEV)
    eager = env.predicted_frames().clone()  # one eager call
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=torch.cuda.Stream(device=DEV)):
        assert env.predicted_frames(out=out) is out
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    seen = [eager]
    for a in (25, 22):
        for _ in range(3):
            env.step(torch.full((n,), a, device=DEV))
        out.fill_(7)
        g.replay()
        torch.cuda.synchronize()
        now = env.predicted_frames()
        assert torch.equal(out, now)
        _same(out, _expect(env)[0], ("replay", a))
        assert not any(torch.equal(now, s) for s in seen)
        seen.append(now.clone())
    env.close()
