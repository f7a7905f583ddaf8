"""The accumulated scan map on the GPU (include/ffmp.h ffmp_scan_map) against the NumPy
restatement (tests/lidar_map_ref.py): both log-odds planes and the frame, bit for bit.

1. live: 65 envs on LIVE[8], LIVE[64], LIVE[100] (max_steps 6: auto-resets fall inside the run) and the
   long-episode G = 64 config, 12 steps with an update after every step and once after a skipped one, both
   frame formats, four knob sets, plain=True;
2. synthetic pose pairs (translations, the quarter turn, half-cell ties, NaN / inf / 1e30 words), scans
   with +-inf, NaN, 0 and negatives, L in {1, 7, 1024}, M_in holding every int8 value, a mask, G = 100
   (G % 64 != 0), G = 64 and 128 (tiled), one env at G = 512;
3. the holder: two updates in one step, reset(mask), an auto-reset caught through the episode id,
   ranges= / pose= on an n_beams = 0 env, nav_field(lidar_map=m), the step untouched;
4. refusals: overlapping and misaligned planes; the env still steps afterwards."""
import ctypes as C

import numpy as np
import pytest
import torch

from flow_field_based_motion_planner_amd import _abi
from flow_field_based_motion_planner_amd.config import FFMPConfig
from flow_field_based_motion_planner_amd.env import FFMP
from flow_field_based_motion_planner_amd.vec_env import FFMPVec, LidarMap
from oracle.ffmp_oracle import Cfg
from tests import lidar_map_ref as M
from tests import scan_map_ref as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INF = float("inf")
NAN = float("nan")
F32 = np.float32
CONFIGS = {"8": S.LIVE[8], "64": S.LIVE[64], "100": S.LIVE[100], "long64": M.LONG[64]}
KNOB_SETS = (dict(), dict(decay=1), dict(l_hit=127, l_max=127), dict(l_free=0, decay=4))


def _frame_np(m: LidarMap) -> np.ndarray:
    want = torch.uint8 if m.env.obs_format == "u8f16" else torch.float32
    assert m.frame.dtype == want
    f = m.frame.cpu().numpy()
    assert np.array_equal(f, f.astype(np.uint8))  # float32 frames hold whole bytes
    return f.astype(np.uint8)


def _same(got: np.ndarray, exp: np.ndarray, where):
    assert got.shape == exp.shape and got.dtype == exp.dtype, (where, got.shape, exp.shape, got.dtype, exp.dtype)
    bad = np.nonzero(got != exp)
    assert not len(bad[0]), (where, len(bad[0]), [b[:5] for b in bad], got[bad][:5], exp[bad][:5])


class RefMap:
    """The holder's bookkeeping restated on the host: the plane, the frame, the pose words and episode
    ids of the last update."""

    def __init__(self, env: FFMPVec, unknown=128, **knobs):
        n, G = env.num_envs, env.cfg.grid
        self.env, self.unknown, self.knobs = env, unknown, knobs
        self.m = np.zeros((n, G, G), np.int8)
        self.frame = np.full((n, G, G), unknown, np.uint8)
        self.pose = np.zeros((n, 4), F32)
        self.episode = np.full(n, -1, np.int64)

    def update(self, mask=None):
        env = self.env
        rec, ep = env.record.cpu().numpy(), env.episode.cpu().numpy().astype(np.int64)
        first = (ep != self.episode) | (rec[:, 10] != 0)
        self.m, self.frame = M.from_config(env.cfg, self.m, env.lidar.cpu().numpy(), rec[:, 0:4], self.pose, first=first,
                                           mask=mask, unknown=self.unknown, frame_in=self.frame, **self.knobs)
        sel = np.ones(len(ep), bool) if mask is None else np.asarray(mask) != 0
        self.pose[sel], self.episode[sel] = rec[sel, 0:4], ep[sel]
        return first


def _check(m: LidarMap, ref: RefMap, where, before=None):
    _same(m.log_odds.cpu().numpy(), ref.m, (where, "log-odds"))
    _same(_frame_np(m), ref.frame, (where, "frame"))
    if before is not None:  # the other plane of the pair is the input, unchanged
        _same(m._planes[1 - m._cur].cpu().numpy(), before, (where, "input plane"))


# ------------------------------------------------------------------ 1. live
@pytest.mark.parametrize("fmt", ["f32", "u8f16"])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_kernel_equals_restatement_on_live_runs(name, fmt):
    n = 65
    cfg = FFMPConfig(**CONFIGS[name])
    env = FFMPVec(n, cfg, device=DEV, autotune=False, obs_format=fmt)
    env.reset()
    maps = [env.lidar_map(**kw) for kw in KNOB_SETS]
    refs = [RefMap(env, **kw) for kw in KNOB_SETS]
    plain = env.lidar_map()
    rng = np.random.default_rng(1)
    restarts = moved = 0
    for k in range(13):
        if k:
            env.step(torch.as_tensor(rng.integers(0, 28, n), device=DEV))
        if k == 6:
            continue  # a skipped update: the next one spans two steps
        for m, ref in zip(maps, refs):
            before = ref.m
            first = ref.update()
            assert m.update() is m.frame
            _check(m, ref, (name, fmt, k, ref.knobs), before)
        plain.update(plain=True)
        _check(plain, refs[0], (name, fmt, k, "plain"))
        restarts += int(first.sum()) if k else 0
        moved += int((~first).sum())
    if name == "long64":
        assert moved >= 8 * n  # long episodes: the warp carries the map along
    else:
        assert restarts >= n  # max_steps 6: every env restarted inside the run
        assert moved >= 3 * n or name == "8"  # (on LIVE[8] the goal lies within reach: every step ends an episode)
    if name != "8":
        last = refs[0]
        assert all((last.frame == v).mean() > 0.01 for v in (0, 128)) and (last.frame == 255).any()
        assert (last.m != np.where(last.frame == 255, 8, np.where(last.frame == 0, -4, 0))).any()  # more than one scan deep
    env.check_errors()
    env.close()


# ------------------------------------------------------------------ 2. synthetic
def _mixed_rows(n, L, seed):
    rng = np.random.default_rng(seed)
    rows = rng.uniform(0.05, 2.0, (n, L)).astype(F32)
    kind = rng.integers(0, 12, (n, L))
    for k, v in enumerate((INF, NAN, -INF, 0.0, -0.7)):
        rows[kind == k] = v
    return rows


def _pose_pairs(res: float):
    """(now, prev, first) rows: the host test's translations and quarter turn, half-cell ties, words that
    are not finite, a huge one, and general motions."""
    r = float(F32(res))
    z = (0.0, 0.0, 1.0, 0.0)
    c, s = float(np.cos(0.3)), float(np.sin(0.3))
    pairs = [((F32(1 * r), 0, 1, 0), z, 0), ((F32(-3 * r), 0, 1, 0), z, 0), ((0, F32(1 * r), 1, 0), z, 0),
             ((0, F32(-3 * r), 1, 0), z, 0), ((0.3, 0.4, 0, 1), (0.3, 0.4, 1, 0), 0), ((0.3, 0.4, 1, 0), (0.3, 0.4, 0, 1), 0),
             ((F32(r) * F32(0.5), 0, 1, 0), z, 0), ((0, F32(r) * F32(-0.5), 1, 0), z, 0),
             ((F32(r) * F32(2.5), F32(r) * F32(-1.5), 1, 0), z, 0),
             ((NAN, 0, 1, 0), z, 0), (z, (0, 0, NAN, 0), 0), ((0, INF, 1, 0), z, 0), ((0, 0, 1, -INF), z, 0),
             ((1e30, 0, 1, 0), z, 0), ((0, -1e30, c, s), z, 0), ((1e38, 1e38, 1, 0), (-1e38, -1e38, 1, 0), 0),
             ((0.21, -0.13, c, s), (0.05, 0.02, 1, 0), 0), ((0.0, 0.0, -1, 0), (0.11, 0.07, c, -s), 0),
             ((0.21, -0.13, c, s), (0.05, 0.02, 1, 0), 1), (z, z, 0), (z, z, 1)]
    now = np.array([p[0] for p in pairs], F32)
    prev = np.array([p[1] for p in pairs], F32)
    return now, prev, np.array([p[2] for p in pairs], bool)


def _every_int8(n, G, seed):
    m = np.random.default_rng(seed).integers(-128, 128, (n, G, G)).astype(np.int8)
    m.reshape(n, -1)[:, :256] = np.arange(-128, 128).astype(np.int8)  # every value, whatever the draw
    return m


@pytest.mark.parametrize("fmt", ["f32", "u8f16"])
@pytest.mark.parametrize("G", [64, 100, 128])
def test_synthetic_poses_scans_and_planes(G, fmt):
    """On an env without a lidar (n_beams = 0): everything comes in through ranges=, pose= and first=."""
    cfg = FFMPConfig(grid=G, n_obst=2, n_beams=0, world_half=0.02 * G, seed=3)
    now, prev, first = _pose_pairs(cfg.res)
    n = len(now)
    env = FFMPVec(n, cfg, device=DEV, autotune=False, obs_format=fmt)
    env.reset()
    ocfg = Cfg.from_config(cfg)
    cr, sr, tx, ty, bad = M.motion(ocfg, now, prev)
    assert bad.sum() == 5 and (tx == F32(0.5)).any() and (ty == F32(-0.5)).any() and (np.abs(tx) > 1e30).any()
    with pytest.raises(ValueError, match="n_beams"):
        env.lidar_map().update()
    t = lambda a, dt=None: torch.as_tensor(a, device=DEV) if dt is None else torch.as_tensor(a, device=DEV).to(dt)  # noqa: E731
    mask = np.ones(n, np.uint8)
    mask[[2, 16]] = 0
    for L, kw in ((1, dict()), (7, dict(unknown=0, decay=3, l_max=127)), (1024, dict(unknown=255, thickness=0.12, range_max=0.9, l_hit=127,
                                                                                    l_free=0, l_max=100, occ_thr=127, free_thr=1))):
        rows = _mixed_rows(n, L, seed=L)
        if L == 1:
            rows[:, 0] = np.resize(np.array([0.8, INF, NAN, -INF, 0.0, -0.7, 1.5], F32), n)
        m_in = _every_int8(n, G, seed=L)
        m = env.lidar_map(**kw)
        m.update(ranges=t(rows), pose=t(prev), first=t(np.ones(n, bool)))  # sets the holder's previous pose
        m.log_odds.copy_(t(m_in))
        m.frame.fill_(77)
        for msk, plain in ((None, False), (mask, False), (None, True)):
            other = m._planes[1 - m._cur]
            other.fill_(55)
            m.log_odds.copy_(t(m_in))
            m._pose.copy_(t(prev))
            frame_in = _frame_np(m)
            got = m.update(ranges=t(rows), pose=t(now), first=t(first), mask=None if msk is None else t(msk), plain=plain)
            assert got is m.frame
            rkw = {k: v for k, v in kw.items() if k not in ("thickness", "range_max")}
            exp_m, exp_f = M.from_config(cfg, m_in, rows, now, prev, first=first, mask=msk, frame_in=frame_in,
                                         thickness=kw.get("thickness"), range_max=kw.get("range_max"), **rkw)
            _same(m.log_odds.cpu().numpy(), exp_m, (G, fmt, L, "map", plain))
            _same(_frame_np(m), exp_f, (G, fmt, L, "frame", plain))
            _same(m._planes[1 - m._cur].cpu().numpy(), m_in, (G, fmt, L, "input"))
            if msk is not None:  # a masked env keeps its saved pose: the motion is not lost
                kept = m._pose.cpu().numpy()
                assert np.array_equal(kept[[2, 16]], prev[[2, 16]], equal_nan=True) and np.array_equal(kept[3], now[3])
        if L == 7:
            assert len(np.unique(exp_m)) > 200
    env.check_errors()
    env.close()


def test_grid_512_two_updates():
    """One env: cell indices pass 65,536 and an env spans 16 blocks."""
    cfg = FFMPConfig(grid=512, n_obst=32, n_beams=360, moving=False, world_half=12.0, obst_rmax=1.0, seed=11)
    env = FFMPVec(1, cfg, device=DEV, autotune=False)
    env.reset()
    m, ref = env.lidar_map(), RefMap(env)
    for k, a in enumerate((None, 26)):
        if a is not None:
            for _ in range(2):
                env.step(torch.as_tensor([a], device=DEV))
        before = ref.m
        first = ref.update()
        m.update()
        _check(m, ref, ("512", k), before)
    assert not first.any() and (ref.m == -8).any() and (ref.m == 16).any() and (ref.frame == 128).mean() > 0.05
    env.close()


# ------------------------------------------------------------------ 3. the holder
@pytest.mark.parametrize("fmt", ["f32", "u8f16"])
def test_holder_bookkeeping(fmt):
    n = 65
    cfg = FFMPConfig(**S.LIVE[64])
    env = FFMPVec(n, cfg, device=DEV, autotune=False, obs_format=fmt, frame_window=3)
    env.reset()
    ocfg = Cfg.from_config(cfg)
    m, ref = env.lidar_map(unknown=0), RefMap(env, unknown=0)
    rng = np.random.default_rng(5)
    step = lambda: env.step(torch.as_tensor(rng.integers(0, 28, n), device=DEV))  # noqa: E731
    m.update()
    ref.update()
    step()
    m.update()
    ref.update()
    _check(m, ref, "one step")
    # a second update in the same step: the identity warp, one more scan on the same cells
    once = ref.m
    pose = env.record[:, 0:4].cpu().numpy()
    assert np.array_equal(M.prior_of(ocfg, once, pose, pose), once.astype(np.int32))
    twice, _ = M.from_config(cfg, once, env.lidar.cpu().numpy(), pose, pose, unknown=0)
    watched = {k: getattr(env, k).clone() for k in ("state_m", "lidar", "record", "episode", "frame_tags")
               if getattr(env, k, None) is not None}
    assert len(watched) >= 4
    m.update()
    ref.update()
    _check(m, ref, "twice")
    _same(m.log_odds.cpu().numpy(), twice, "warp-free double update")
    for k, v in watched.items():  # the step's own state is untouched
        assert torch.equal(getattr(env, k).view(torch.int32 if v.dtype == torch.float32 else v.dtype),
                           v.view(torch.int32 if v.dtype == torch.float32 else v.dtype)), k
    # planning on the map
    d = env.nav_field(cost=True, direction=True, lidar_map=m)
    d2 = env.nav_field(cost=True, direction=True, frames=m.frame)
    for k in ("cost", "dir", "target", "geo_cost"):
        assert torch.equal(d[k], d2[k]), k
    assert torch.equal(env.policy_nav(lidar_map=m), env.policy_nav(frames=m.frame))
    assert not torch.equal(d["cost"], env.nav_field(cost=True)["cost"])
    for kw in (dict(frames=m.frame), dict(visible=True), dict(lidar=True)):
        with pytest.raises(ValueError):
            env.nav_field(lidar_map=m, **kw)
        with pytest.raises(ValueError):
            env.policy_nav(lidar_map=m, **kw)
    with pytest.raises(ValueError):
        env.nav_field(lidar_map=env.lidar_map(frame=False))
    with pytest.raises(ValueError):
        env.nav_field(lidar_map=m.frame)
    # reset(mask): the selected envs start anew, the others go on
    sel = np.arange(n) % 4 == 1
    m.reset(torch.as_tensor(sel, device=DEV))
    assert (m.log_odds[sel] == 0).all() and (m.frame[sel] == 0).all() and (m.log_odds[~sel] != 0).any()
    ref.m[sel], ref.frame[sel], ref.episode[sel] = 0, 0, -1
    step()
    m.update()
    first = ref.update()
    _check(m, ref, "reset(mask)")
    assert first[sel].all()
    # skipped steps across an auto-reset: record word 10 is back to 0, the episode id tells
    for _ in range(8):
        step()
    ep, word = env.episode.cpu().numpy(), env.record[:, 10].cpu().numpy()
    assert ((ep != ref.episode) & (word == 0)).sum() >= 5
    m.update()
    first = ref.update()
    assert first.all()  # max_steps 6: every env has reset since
    _check(m, ref, "missed auto-resets")
    # a masked update leaves the env's map, frame and saved pose alone
    step()
    mask = np.arange(n) % 3 != 0
    m.update(mask=torch.as_tensor(mask, device=DEV))
    ref.update(mask=mask.astype(np.uint8))
    _check(m, ref, "masked")
    step()
    m.update()
    ref.update()
    _check(m, ref, "after the mask")
    # reset() forgets everything
    m.reset()
    assert (m.log_odds == 0).all() and (m.frame == 0).all()
    # frame=False: the planes alone
    bare, bref = env.lidar_map(frame=False, decay=2), RefMap(env, decay=2)
    assert bare.update() is None and bare.frame is None
    bref.update()
    _same(bare.log_odds.cpu().numpy(), bref.m, "frame=False")
    env.check_errors()
    env.close()


def test_single_env_surface():
    one = FFMP(FFMPConfig(**dict(S.LIVE[64], autoreset=False)), device=DEV)
    with pytest.raises(RuntimeError):
        one.lidar_map()
    one.reset()
    m = one.lidar_map(decay=1)
    assert isinstance(m, LidarMap) and m.env is one._vec_env()
    ref = RefMap(m.env, decay=1)
    m.update()
    ref.update()
    one.step(24)
    m.update()
    ref.update()
    assert tuple(m.frame.shape) == (1, 64, 64) and m.log_odds.dtype == torch.int8
    _check(m, ref, "single env")
    one.close()


# ------------------------------------------------------------------ 4. refusals
@pytest.mark.parametrize("fmt", ["f32", "u8f16"])
def test_overlapping_and_misaligned_planes_are_refused(fmt):
    n, G2 = 3, 64 * 64
    env = FFMPVec(n, FFMPConfig(**S.LIVE[64]), device=DEV, autotune=False, obs_format=fmt)
    env.reset()
    m = env.lidar_map()
    buf = torch.full((2 * n * G2 + 64,), 9, dtype=torch.int8, device=DEV)
    frame = torch.full((n * G2 + 16,), 9, dtype=env._frame_dtype, device=DEV)
    p, f = buf.data_ptr(), frame.data_ptr()
    first = torch.ones(n, dtype=torch.uint8, device=DEV)
    sectors = env._sectors(env.lidar.shape[1])

    def launch(map_in, map_out, map_stride=G2, frame_ptr=f, frame_stride=G2):
        return env.lib.ffmp_scan_map(C.byref(env._cfg_c), n, env.lidar.data_ptr(), env.lidar.stride(0), env.lidar.shape[1],
                                     sectors.data_ptr(), env.record.data_ptr(), env.record.stride(0), m._pose.data_ptr(), 4, None,
                                     first.data_ptr(), map_in, map_out, map_stride, frame_ptr, frame_stride, *m.knobs, 0,
                                     env._stream())

    es = env._fes
    for args, word in (((p, p), "overlap"), ((p, p + G2 - 4), "overlap"), ((p + G2 - 4, p), "overlap"), ((p, p + 2 * G2), "overlap"),
                       ((p, p + 3 * G2 + 8, G2 + 8), "overlap"), ((p + 1, p + 3 * G2), "map alignment"),
                       ((p, p + 3 * G2 + 2), "map alignment"), ((p, p + 3 * G2 + 8, G2 + 2), "map alignment"),
                       ((p, p + 3 * G2, G2, f + es), "frame alignment"), ((p, p + 3 * G2, G2, f, G2 + 2), "frame alignment"),
                       ((p, p + 3 * G2, G2 - 4), "map_env_stride"), ((None, p), "map_in is NULL"), ((p, None), "map_out is NULL")):
        assert launch(*args) == -1, args
        assert word in env.lib.ffmp_last_error().decode(), (args, env.lib.ffmp_last_error())
    torch.cuda.synchronize()
    assert (buf == 9).all() and (frame == 9).all()
    for kw in (dict(l_max=0), dict(l_hit=128), dict(decay=-1), dict(occ_thr=0), dict(free_thr=200), dict(unknown=256),
               dict(thickness=-1.0), dict(range_max=0.0)):
        with pytest.raises(_abi.FFMPBackendError):
            env.lidar_map(**kw)
    for bad in (dict(pose=torch.zeros((n, 4), dtype=torch.float64, device=DEV)), dict(pose=torch.zeros((n, 3), device=DEV)),
                dict(pose=torch.zeros((n, 4))), dict(ranges=torch.zeros((n + 1, 7), device=DEV)),
                dict(ranges=torch.zeros((n, 1025), device=DEV))):
        with pytest.raises((ValueError, _abi.FFMPBackendError)):
            m.update(**bad)
    # the well-formed call on the same buffers goes through, and the env still steps
    assert launch(p, p + 3 * G2) == 0, env.lib.ffmp_last_error()
    ref = RefMap(env)
    ref.update()
    _same(buf[3 * G2:6 * G2].reshape(n, 64, 64).cpu().numpy(), ref.m, "raw call")
    assert (buf[6 * G2:] == 9).all() and (buf[:3 * G2] == 9).all() and (frame[n * G2:] == 9).all()
    env.step(torch.as_tensor([3, 10, 24], device=DEV))
    m.update()
    m.update()
    env.check_errors()
    fresh = FFMPVec(2, FFMPConfig(**S.LIVE[8]), device=DEV, autotune=False)
    with pytest.raises(RuntimeError, match="reset"):
        fresh.lidar_map().update()
    fresh.close()
    env.close()
