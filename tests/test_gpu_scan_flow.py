"""Motion flow estimated from the scan on the GPU (include/ffmp.h ffmp_scan_flow) against
the NumPy restatement (tests/scan_flow_ref.py): `flow` as bits and `kind` as bytes, torch.equal.

1. the raw entry point: random frames with 2-30 % hits plus oracle-driven frames, random poses with a restart
   by NaN, G = 8 (the block and the search reach past every edge), 36 (rows end inside a 32-bit word), 64,
   100, 256 with n = 3 and 512 with n = 2 (the LDS limit);
2. knob corners; formats and layout (float32 / binary16, kind_out NULL, padded strides, mask and first per
   env); isolation at n = 65;
3. LidarFlow against the restated bookkeeping on a live config with auto-resets inside the window, both
   obs formats, the single-env surface; nothing else moves."""
import ctypes as C

import numpy as np
import pytest
import torch

from flow_field_based_motion_planner_amd import _abi
from flow_field_based_motion_planner_amd.config import FFMPConfig
from flow_field_based_motion_planner_amd.env import FFMP
from flow_field_based_motion_planner_amd.vec_env import FFMPVec, LidarFlow
from oracle.ffmp_oracle import Cfg, bev_image
from tests import scan_flow_ref as R
from tests import scan_map_ref as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
F32 = np.float32
SCALE = F32(0.125)


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def _bits(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32 if a.dtype == F32 else np.int16 if a.dtype == np.float16 else a.dtype))


def _same(got: torch.Tensor, exp: np.ndarray, where):
    g = got.cpu().contiguous()
    g = g.view(torch.int32) if g.dtype == torch.float32 else g.view(torch.int16) if g.dtype == torch.float16 else g
    e = _bits(exp)
    assert g.shape == e.shape and g.dtype == e.dtype, (where, g.shape, e.shape, g.dtype, e.dtype)
    if not torch.equal(g, e):
        bad = torch.nonzero(g != e)
        raise AssertionError((where, len(bad), bad[:5].tolist(), got.cpu()[tuple(bad[:5].T)].tolist(), exp[tuple(bad[:5].T.numpy())].tolist()))


def _raw(G, cur, prev, now, was, first=None, mask=None, half=False, kind=True, frame_stride=None, flow_stride=None,
         kind_stride=None, scale=SCALE, fill=0, **knobs):
    """One ffmp_scan_flow call on device copies of the arrays: (flow (n, 2, G, G), kind (n, G, G) or None) as torch
    tensors, cut out of buffers with the given env strides that were filled with `fill` first."""
    lib = _abi.load()
    cfg = _abi.make_cfg(FFMPConfig(grid=G, n_obst=0, n_beams=0))
    n, G2 = cur.shape[0], G * G
    fs, ws, ks = frame_stride or G2, flow_stride or 2 * G2, kind_stride or G2
    k = dict(R.KNOBS, **knobs)

    def strided(a, stride):  # (n, ...) -> a device buffer with `stride` elements per env
        buf = torch.zeros((n, stride), dtype=a.dtype, device=DEV)
        buf[:, :a[0].numel()] = a.reshape(n, -1)
        return buf

    dcur, dprev = strided(_t(cur), fs), strided(_t(prev), fs)
    dnow, dwas = _t(np.asarray(now, F32)), _t(np.asarray(was, F32))
    flow = torch.full((n, ws), fill, dtype=torch.float16 if half else torch.float32, device=DEV)
    kd = torch.full((n, ks), fill, dtype=torch.uint8, device=DEV) if kind else None
    dfirst = None if first is None else _t(np.asarray(first, np.uint8))
    dmask = None if mask is None else _t(np.asarray(mask, np.uint8))
    rc = lib.ffmp_scan_flow(C.byref(cfg), n, dcur.data_ptr(), dprev.data_ptr(), fs, dnow.data_ptr(), dnow.stride(0), dwas.data_ptr(),
                            dwas.stride(0), None if dmask is None else dmask.data_ptr(), None if dfirst is None else dfirst.data_ptr(),
                            flow.data_ptr(), ws, None if kd is None else kd.data_ptr(), ks, 1 if half else 0, float(scale),
                            k["radius"], k["block"], k["gate"], k["min_hits"], None)
    assert rc == 0, lib.ffmp_last_error()
    torch.cuda.synchronize()
    if ws > 2 * G2:
        assert (flow[:, 2 * G2:] == fill).all()
    if kd is not None and ks > G2:
        assert (kd[:, G2:] == fill).all()
    return flow[:, :2 * G2].reshape(n, 2, G, G), None if kd is None else kd[:, :G2].reshape(n, G, G)


def _random_case(G, n, seed):
    """Frames with 2-30 % hits: the current one is the earlier one moved by a few cells where the density is low
    (so the search finds things), independent noise elsewhere; poses with small motions, env 1 of three or more restarts by NaN."""
    rng = np.random.default_rng(seed)
    dens = np.linspace(0.02, 0.30, n)
    prev = np.stack([np.where(rng.random((G, G)) < d, 255, rng.integers(0, 255, (G, G))) for d in dens]).astype(np.uint8)
    cur = np.stack([np.roll(prev[e], (int(rng.integers(-3, 4)), int(rng.integers(-3, 4))), (0, 1)) if e % 2 == 0 else
                    np.where(rng.random((G, G)) < dens[e], 255, 0) for e in range(n)]).astype(np.uint8)
    res = 0.05
    yaw0 = rng.uniform(-3, 3, n)
    yaw1 = yaw0 + rng.uniform(-0.08, 0.08, n)
    p0 = rng.uniform(-1, 1, (n, 2))
    p1 = p0 + rng.uniform(-2.5 * res, 2.5 * res, (n, 2))
    was = np.stack([p0[:, 0], p0[:, 1], np.cos(yaw0), np.sin(yaw0)], axis=1).astype(F32)
    now = np.stack([p1[:, 0], p1[:, 1], np.cos(yaw1), np.sin(yaw1)], axis=1).astype(F32)
    now[0], was[0] = (0, 0, 1, 0), (0, 0, 1, 0)  # env 0: the identity
    if n > 2:
        now[1, int(rng.integers(0, 4))] = NAN
    return cur, prev, now, was


_ORACLE = {}


def _oracle_case(G, n=6, lag=4):
    """Scan frames of the NumPy oracle on TIE[G], `lag` steps apart, with their poses (computed once)."""
    if G not in _ORACLE:
        from oracle.ffmp_oracle import OracleVecEnv
        config = FFMPConfig(**R.TIE[G])
        env = OracleVecEnv(config, n, with_potential=False)
        env.reset()
        rng = np.random.default_rng(3)
        prev, was = S.from_config(config, env.lidar), env.record[:, 0:4].astype(F32).copy()
        for _ in range(lag):
            env.step(rng.integers(0, 28, n))
        _ORACLE[G] = (S.from_config(config, env.lidar), prev, env.record[:, 0:4].astype(F32).copy(), was)
    return _ORACLE[G]


def _cfg(G):
    return Cfg.from_config(FFMPConfig(grid=G, n_obst=0, n_beams=0))


# ------------------------------------------------------------------ 1. the raw entry point
@pytest.mark.parametrize("G,n", [(8, 5), (36, 5), (64, 6), (100, 5), (256, 3), (512, 2)])
def test_kernel_equals_restatement_on_random_frames(G, n):
    cur, prev, now, was = _random_case(G, n, seed=G)
    exp_f, exp_k = R.scan_flow(_cfg(G), cur, prev, now, was, SCALE)
    flow, kind = _raw(G, cur, prev, now, was, fill=7)
    _same(kind, exp_k, (G, "kind"))
    _same(flow, exp_f, (G, "flow"))
    if n > 2:
        assert exp_k[1].sum() == 0  # the NaN pose
    if G >= 36:
        assert all((exp_k == v).any() for v in (0, 1, 2))


@pytest.mark.parametrize("G", [64, 100])
def test_kernel_equals_restatement_on_oracle_frames(G):
    cur, prev, now, was = _oracle_case(G)
    exp_f, exp_k = R.scan_flow(_cfg(G), cur, prev, now, was, SCALE)
    assert (exp_k == 1).sum() > 100 and (exp_k == 2).sum() > 100
    flow, kind = _raw(G, cur, prev, now, was, fill=7)
    _same(kind, exp_k, (G, "kind"))
    _same(flow, exp_f, (G, "flow"))


# ------------------------------------------------------------------ 2. knobs, formats, layout, isolation
@pytest.mark.parametrize("knobs", [dict(radius=1, block=1), dict(radius=5, block=3), dict(radius=4, block=3), dict(gate=0), dict(gate=98),
                                   dict(min_hits=1), dict(min_hits=49), dict(radius=5, block=2, gate=3, min_hits=2)],
                         ids=lambda k: "-".join(f"{a}{b}" for a, b in k.items()))
def test_knob_corners(knobs):
    G = 64
    rc, rp, rn, rw = _random_case(G, 6, seed=11)
    oc, op, on, ow = _oracle_case(G)
    cur, prev, now, was = np.concatenate([rc, oc]), np.concatenate([rp, op]), np.concatenate([rn, on]), np.concatenate([rw, ow])
    if knobs.get("min_hits") == 49:  # a full 7 x 7 block of hits, moved by (1, 2)
        prev[0, 20:36, 20:36] = 255
        cur[0] = np.roll(prev[0], (1, 2), (0, 1))
    exp_f, exp_k = R.scan_flow(_cfg(G), cur, prev, now, was, SCALE, **knobs)
    flow, kind = _raw(G, cur, prev, now, was, **knobs)
    _same(kind, exp_k, (knobs, "kind"))
    _same(flow, exp_f, (knobs, "flow"))
    assert (exp_k > 0).any()
    if knobs.get("gate") == 98:
        assert not (exp_k == 2).any()  # c0 <= 2 * 49: everything with enough hits is static
    if knobs.get("gate") == 0:
        assert (exp_k == 2).sum() > (R.scan_flow(_cfg(G), cur, prev, now, was, SCALE)[1] == 2).sum()


@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
def test_formats_layout_mask_and_first(half):
    G = 36
    cur, prev, now, was = _random_case(G, 7, seed=5)
    n, G2 = len(cur), G * G
    first = np.array([0, 0, 1, 0, 0, 0, 1], np.uint8)
    mask = np.array([1, 1, 1, 0, 1, 0, 1], np.uint8)
    scale = F32(0.3)  # not a power of two: binary16 rounds
    kw = dict(first=first, mask=mask, half=half, scale=scale)
    fin = np.full((n, 2, G, G), 7, np.float16 if half else F32)
    kin = np.full((n, G, G), 7, np.uint8)
    exp_f, exp_k = R.scan_flow(_cfg(G), cur, prev, now, was, scale, first=first, mask=mask, half=half, flow_in=fin, kind_in=kin)
    assert (exp_f[3] == 7).all() and (exp_k[5] == 7).all() and exp_k[2].sum() == 0 and (exp_k == 2).any()
    if half:
        assert (exp_f.astype(F32) != R.scan_flow(_cfg(G), cur, prev, now, was, scale, first=first, mask=mask, flow_in=fin)[0]).any()
    flow, kind = _raw(G, cur, prev, now, was, fill=7, **kw)
    _same(kind, exp_k, "dense kind")
    _same(flow, exp_f, "dense flow")
    # padded env strides on every plane; kind_out NULL
    flow, kind = _raw(G, cur, prev, now, was, fill=7, frame_stride=G2 + 12, flow_stride=2 * G2 + 20, kind_stride=G2 + 4, **kw)
    _same(kind, exp_k, "padded kind")
    _same(flow, exp_f, "padded flow")
    flow, kind = _raw(G, cur, prev, now, was, fill=7, kind=False, flow_stride=2 * G2 + 8, **kw)
    assert kind is None
    _same(flow, exp_f, "flow without kind")


def test_an_env_does_not_depend_on_its_neighbours():
    G, n = 64, 65
    cur, prev, now, was = _random_case(G, n, seed=9)
    exp_f, exp_k = R.scan_flow(_cfg(G), cur, prev, now, was, SCALE)
    flow, kind = _raw(G, cur, prev, now, was)
    _same(kind, exp_k, "batch kind")
    _same(flow, exp_f, "batch flow")
    for e in (0, 31, 64):
        f1, k1 = _raw(G, cur[e:e + 1], prev[e:e + 1], now[e:e + 1], was[e:e + 1])
        assert torch.equal(f1[0].view(torch.int32), flow[e].view(torch.int32)) and torch.equal(k1[0], kind[e]), e


# ------------------------------------------------------------------ 3. the holder
class LiveRef:
    """RefFlow fed from a live FFMPVec."""

    def __init__(self, env: FFMPVec, **kw):
        self.env = env
        self.ref = R.RefFlow(env.cfg, env.num_envs, half=env.obs_format == "u8f16", **kw)

    def update(self, **kw):
        env = self.env
        return self.ref.update(env.lidar.cpu().numpy(), env.record.cpu().numpy(), env.episode.cpu().numpy(), **kw)


def _check(m: LidarFlow, ref: R.RefFlow, where):
    _same(m.kind, ref.kind, (where, "kind"))
    _same(m.flow, ref.flow, (where, "flow"))
    _same(m.frame, ref.frame, (where, "frame"))
    assert m.updates.cpu().tolist() == ref.updates.tolist(), where


@pytest.mark.parametrize("fmt", ["f32", "u8f16"])
def test_holder_against_the_restated_bookkeeping(fmt):
    n, lag = 9, 2
    cfg = FFMPConfig(**S.LIVE[64])
    env = FFMPVec(n, cfg, device=DEV, autotune=False, obs_format=fmt)
    env.reset()
    m, live = env.lidar_flow(lag=lag), LiveRef(env, lag=lag)
    ref = live.ref
    assert m.flow.dtype == (torch.float16 if fmt == "u8f16" else torch.float32) and m.kind.dtype == torch.uint8
    assert tuple(m._frames.shape) == (lag + 1, n, 64, 64) and m._frames.dtype == torch.uint8
    assert m.scale == float(F32(cfg.res / (lag * cfg.dt)))
    rng = np.random.default_rng(2)
    step = lambda: env.step(torch.as_tensor(rng.integers(0, 28, n), device=DEV))  # noqa: E731
    restarts = moving = images = 0
    for k in range(2 * lag + 3 + 1):
        if k:
            step()
        first = live.update()
        assert m.update() is m.flow
        _check(m, ref, (fmt, k))
        restarts += int(first.sum()) if k > lag else 0
        moving += int((ref.kind == 2).sum())
        if (ref.kind == 2).any() and images < 2:  # the 4-channel image from sensor data alone
            images += 1
            want = bev_image(ref.frame, ref.flow.astype(F32), cfg.obst_vmax)
            img = m.bev_image()
            assert img.dtype == env._frame_dtype and tuple(img.shape) == (n, 4, 64, 64)
            assert np.array_equal(img.cpu().numpy().astype(F32), want)
            assert (want[:, 1] != 128).any() and (want[:, 3] != 0).any() and (want[:, 0] == 255).any()
            occ = env.lidar_frames(newest_only=True)
            out = torch.empty_like(img)
            assert m.bev_image(occ=occ, out=out) is out and torch.equal(out, img)
            with pytest.raises(ValueError):
                m.bev_image(occ=occ[:, :32])
    assert restarts >= 3 and moving > 50 and images == 2  # max_steps 6: auto-resets fall inside the window
    # a second update in the same step: the same scan again, the earlier frame one slot younger
    live.update()
    m.update()
    _check(m, ref, (fmt, "twice"))
    # mask=: the envs left out keep their outputs and lose their history
    step()
    mask = np.arange(n) % 3 != 1
    live.update(mask=mask)
    m.update(mask=torch.as_tensor(mask, device=DEV))
    _check(m, ref, (fmt, "masked"))
    for _ in range(lag + 1):
        step()
        first = live.update()
        m.update()
        _check(m, ref, (fmt, "after the mask"))
    # reset(mask)
    sel = np.arange(n) % 4 == 0
    m.reset(torch.as_tensor(sel, device=DEV))
    ref.reset(sel)
    assert (m.flow[sel] == 0).all() and (m.kind[sel] == 0).all()
    step()
    first = live.update()
    m.update()
    assert first[sel].all()
    _check(m, ref, (fmt, "reset(mask)"))
    m.reset()
    assert (m.flow == 0).all() and (m.kind == 0).all() and (m.updates == 0).all()
    env.check_errors()
    env.close()


def test_pose_and_ranges_on_an_env_without_a_lidar():
    n, G, lag = 5, 36, 1
    cfg = FFMPConfig(grid=G, n_obst=2, n_beams=0, world_half=0.02 * G, seed=3)
    env = FFMPVec(n, cfg, device=DEV, autotune=False)
    env.reset()
    m = env.lidar_flow(lag=lag, min_hits=1, kind=False)
    ref = R.RefFlow(cfg, n, lag=lag, min_hits=1)
    assert m.kind is None
    with pytest.raises(ValueError, match="n_beams"):
        m.update()
    rng = np.random.default_rng(4)
    yaw = rng.uniform(-3, 3, n)
    pose = np.stack([rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), np.cos(yaw), np.sin(yaw)], axis=1).astype(F32)
    for k in range(4):
        rows = rng.uniform(0.2, 0.8, (n, 40)).astype(F32)
        pose = pose.copy()
        pose[:, 0] += F32(0.03)
        first = np.arange(n) == k if k >= 2 else None
        ref.update(rows, pose=pose, first=first)
        m.update(ranges=_t(rows), pose=_t(pose), first=None if first is None else _t(first))
        _same(m.flow, ref.flow, ("pose=", k))
        _same(m.frame, ref.frame, ("pose= frame", k))
    assert (ref.kind == 2).any()
    for bad in (dict(pose=torch.zeros((n, 4), dtype=torch.float64, device=DEV)), dict(pose=torch.zeros((n, 3), device=DEV)),
                dict(ranges=torch.zeros((n + 1, 7), device=DEV))):
        with pytest.raises((ValueError, _abi.FFMPBackendError)):
            m.update(**bad)
    for kw in (dict(lag=0), dict(lag=17)):
        with pytest.raises(ValueError):
            env.lidar_flow(**kw)
    for kw in (dict(radius=6), dict(block=0), dict(gate=99), dict(min_hits=0), dict(thickness=-1.0)):
        with pytest.raises(_abi.FFMPBackendError):
            env.lidar_flow(**kw)
    env.close()


def test_single_env_surface():
    one = FFMP(FFMPConfig(**dict(S.LIVE[64], autoreset=False)), device=DEV)
    with pytest.raises(RuntimeError):
        one.lidar_flow()
    one.reset()
    m = one.lidar_flow(lag=1)
    assert isinstance(m, LidarFlow) and m.env is one._vec_env()
    live = LiveRef(m.env, lag=1)
    for a in (None, 24, 24):
        if a is not None:
            one.step(a)
        live.update()
        m.update()
    assert tuple(m.flow.shape) == (1, 2, 64, 64) and tuple(m.kind.shape) == (1, 64, 64)
    _check(m, live.ref, "single env")
    one.close()


def test_nothing_else_moves():
    n = 7
    cfg = FFMPConfig(**S.LIVE[64])
    envs = [FFMPVec(n, cfg, device=DEV, autotune=False, frame_window=3) for _ in range(2)]
    for env in envs:
        env.reset()
    m = envs[0].lidar_flow(lag=2)
    m.update()
    rng = np.random.default_rng(6)
    names = ("state_m", "lidar", "record", "episode", "frame_tags", "reward", "done", "state_g", "state_v")
    for _ in range(5):
        a = torch.as_tensor(rng.integers(0, 28, n), device=DEV)
        for env in envs:
            env.step(a)
        m.update()
        seen = 0
        for k in names:
            x, y = getattr(envs[0], k, None), getattr(envs[1], k, None)
            if x is None:
                continue
            seen += 1
            ix = torch.int32 if x.dtype == torch.float32 else torch.int64 if x.dtype == torch.float64 else x.dtype
            assert torch.equal(x.view(ix), y.view(ix)), k
        assert seen >= 6
    for env in envs:
        env.check_errors()
        env.close()
