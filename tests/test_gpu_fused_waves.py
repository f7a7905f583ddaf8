"""FFMP_RASTER_WAVES (the tagged float32 kernels at a forced occupancy): an env stepped
with the flag against the same env stepped without it, both with granule tags, and a third env
with sparse_frames=False.  torch.equal on bit patterns after every step: every physical ring
slot, frame_tags, the potential, the record, the small observations, reward and flags; and the tag
invariant (tag 0 => the granule is all zero).  Grids 64 (TILE4: one column band, four waves per
band), 128 (two bands), 256 (four bands, the C3 mapping) and 96 (tile flags fall back to row runs);
1 and 16 discs; worlds in which some envs have a wall in their plane's reach and others have not
(robots start at the world's middle: it depends on their yaw) and worlds with no wall in any plane;
resets inside every run (the older frame written per env); every ring layout; NT / PLAIN, with and
without XCD; ids and commands; a masked reset; a captured graph; the two-launch raster; and the flag
where it is ignored.  ffmp_raster_waves says which kernel a launch takes: the flagged env's launches must
answer 6 (not the plain kernel) and the others 0."""
import ctypes as C

import numpy as np
import pytest
import torch

from flow_field_based_motion_planner_amd import _abi
from flow_field_based_motion_planner_amd.config import FFMPConfig
from flow_field_based_motion_planner_amd.vec_env import FFMPVec

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
A = _abi
WAVES = (A.RASTER_WAVES,)
# today's flags of the one-launch step / (cells per block, flags) of the two-launch raster
BASE = [A.RASTER_NT | A.RASTER_TILE4, A.RASTER_PLAIN | A.RASTER_XCD | A.RASTER_TILE4, A.RASTER_NT | A.RASTER_XCD | A.RASTER_TILE2,
        A.RASTER_PLAIN, A.RASTER_NT | A.RASTER_XCD, A.RASTER_PLAIN | A.RASTER_TILE2, A.RASTER_NT]
CELLS = [4096, 16384, 2048, 1024, 8192, 65536, 3072]
KEYS = ("potential", "record", "state_g", "state_v", "state_t", "grad", "lidar", "reward", "done", "is_goal",
        "collision", "truncated", "pose", "obst", "t", "episode")
RINGS = {"seamless4": dict(frame_window=4, seamless=True), "wrap3": dict(frame_window=3, seamless=False),
         "pair2": dict(frame_window=2)}


def _cfg(G, K, **kw):
    return FFMPConfig(**dict(dict(grid=G, n_obst=K, n_beams=16, moving=True, max_steps=5, seed=11), **kw))


def _trio(n, cfg, ring, **kw):
    kw = dict(dict(device=DEV, autotune=False, fused=False), **RINGS[ring], **kw)
    a, b = FFMPVec(n, cfg, sparse_frames=True, **kw), FFMPVec(n, cfg, sparse_frames=True, **kw)
    c = FFMPVec(n, cfg, sparse_frames=False, **kw)
    assert a.frame_tags is not None and b.frame_tags is not None and c.frame_tags is None
    return a, b, c


def _slots(env):
    G2 = env.cfg.grid ** 2
    if env.frame_window == 2:
        return env._frames.reshape(env.num_envs, 2, G2).transpose(0, 1)
    return env._frames[:env.frame_window].reshape(env.frame_window, env.num_envs, G2)


def _bits(t):
    return t.contiguous().view(torch.uint8)


def _same(a, b, c, what):
    torch.cuda.synchronize()
    assert torch.equal(a.frame_tags, b.frame_tags), (what, "frame_tags")
    for o, name in ((b, "tagged"), (c, "dense")):
        assert torch.equal(_bits(_slots(a)), _bits(_slots(o))), (what, name, "frames")
        assert torch.equal(_bits(a.state_m), _bits(o.state_m)), (what, name, "state_m")
        for k in KEYS:
            va, vo = getattr(a, k), getattr(o, k)
            if vo is not None:
                assert torch.equal(_bits(va), _bits(vo)), (what, name, k)
    f = _slots(a)
    S, N, G2 = f.shape
    T = a.frame_tags.shape[2]
    nz = torch.zeros(S, N, T * 64, dtype=torch.bool, device=f.device)
    nz[:, :, :G2] = f != 0
    assert not bool((nz.view(S, N, T, 64).any(dim=3) & (a.frame_tags == 0)).any()), (what, "tag 0 over a non-zero cell")


def _sees_walls(env):
    """Per env: a corner of the plane outside world_half - cull_margin, so some wave task of the env
    draws wall cells or at least runs the wall test's slow side (float64: envs at the very boundary may
    differ from the kernel's float32, the counts below do not depend on them)."""
    cfg = env.cfg
    h = 0.5 * cfg.grid * cfg.res
    p = env.pose.double()
    c, s = torch.cos(p[:, 2]), torch.sin(p[:, 2])
    out = torch.zeros(env.num_envs, dtype=torch.bool, device=p.device)
    for ex in (-h, h):
        for ey in (-h, h):
            wx, wy = p[:, 0] + c * ex - s * ey, p[:, 1] + s * ex + c * ey
            out |= (wx.abs() > cfg.W - cfg.cull_margin) | (wy.abs() > cfg.W - cfg.cull_margin)
    return out


def _set(envs, i, kind):
    """Step i's launch form: kind 0 one-launch, 1 two-launch; envs[0] gets the flag."""
    base, cells = BASE[i % len(BASE)], CELLS[i % len(CELLS)]
    for j, e in enumerate(envs):
        f = base | (WAVES[i % len(WAVES)] if j == 0 else 0)
        e.fused = kind == 0
        e.fused_flags = f
        e.raster_shape = e.raster_shape_newest = (cells, f)
    # the flagged env's launch takes the forced-occupancy kernel, the other two the plain ones
    assert [_kernel_waves(e, e.fused_flags) for e in envs] == [6, 0, 0]


def _kernel_waves(env, flags):
    """The library's own answer for a launch of this env with these flags (no launch)."""
    return env.lib.ffmp_raster_waves(C.byref(env._cfg_c), C.cast(C.byref(env._obs_c), C.POINTER(A.ObsT)), flags)


def _act(rng, n, cmd):
    if cmd:
        return torch.as_tensor(rng.uniform([-0.1, -0.7], [0.7, 0.7], (n, 2)), device=DEV)
    return torch.as_tensor(rng.integers(0, 28, n), device=DEV)


# world: world_half in plane sides.  Robots start at the middle, the plane's corners reach 0.5 (yaw 0)
# to 0.71 (yaw 45 deg) plane sides: 0.65 -> some envs of a launch see walls and others do not; 1.0
# (the default, C3's) -> no env does.
@pytest.mark.parametrize("G,K,n,ring,world", [
    (64, 1, 37, "seamless4", 0.65), (64, 16, 37, "wrap3", 0.65), (64, 16, 37, "pair2", 1.0),
    (128, 16, 37, "seamless4", 0.65), (128, 1, 37, "pair2", 0.65), (128, 16, 37, "wrap3", 1.0),
    (256, 16, 5, "seamless4", 1.0), (256, 1, 5, "wrap3", 0.65), (256, 16, 5, "pair2", 0.65),
    (96, 16, 37, "seamless4", 0.65), (96, 1, 37, "wrap3", 1.0),
])
def test_every_launch_form(G, K, n, ring, world):
    cfg = _cfg(G, K, world_half=world * G * 0.05)
    envs = _trio(n, cfg, ring)
    a, b, c = envs
    rng = np.random.default_rng(G + K + n)
    for e in envs:
        e.reset()
    _same(a, b, c, "reset")
    seen = torch.zeros(2, dtype=torch.int64)
    for i in range(14):
        _set(envs, i, (i // 2) % 2 if i % 5 else 0)
        act = _act(rng, n, i % 3 == 1)
        for e in envs:
            e.step(act)
        _same(a, b, c, i)
        w = _sees_walls(a)
        seen += torch.tensor([int(w.sum()), int((~w).sum())])
    assert int(a.episode.sum()) >= n          # auto-resets: the older frame written for single envs
    if world >= 1.0:
        assert int(seen[0]) == 0, seen                        # no wall in any plane
    elif n >= 37:
        assert int(seen[0]) > 0 and int(seen[1]) > 0, seen   # planes with and without walls in every launch
    a.check_errors()
    for e in envs:
        e.close()


@pytest.mark.parametrize("ring", ["seamless4", "wrap3", "pair2"])
def test_masked_reset_and_graph(ring):
    n, G, K = 37, 128, 16
    cfg = _cfg(G, K, world_half=0.65 * G * 0.05)
    envs = _trio(n, cfg, ring)
    a, b, c = envs
    rng = np.random.default_rng(4)
    for e in envs:
        e.reset()
    _set(envs, 0, 0)
    for i in range(3):
        act = _act(rng, n, False)
        for e in envs:
            e.step(act)
        _same(a, b, c, ("warm", i))
    m = torch.as_tensor(rng.integers(0, 2, n).astype(bool), device=DEV)
    for e in envs:
        e.reset(mask=m)
    _same(a, b, c, "reset(mask)")
    _set(envs, 1, 1)
    for e in envs:
        e.raster(mask=~m)
    _same(a, b, c, "raster(mask)")
    # a captured graph of one-launch steps with the flag, replayed twice
    _set(envs, 0, 0)
    per = a.graph_period()
    g = a.capture(per, skewed=False, pipelined=False)
    for r in range(2):
        acts = torch.as_tensor(rng.integers(0, 28, (per, n)), device=DEV)
        g.replay(acts)
        for i in range(per):
            b.step(acts[i])
            c.step(acts[i])
        _same(a, b, c, ("replay", r))
    a.check_errors()
    for e in envs:
        e.close()


@pytest.mark.parametrize("kw", [dict(obs_format="u8f16"), dict(sparse_frames=False), dict(sparse_frames=False, flow=True),
                                dict(sparse_frames=True, flow=True)])
def test_flag_ignored_where_it_does_not_apply(kw):
    """The compact format, no tags, flow planes: with the flag the launch is today's."""
    n = 16
    kw = dict(kw)
    cfg = _cfg(64, 4, flow=kw.pop("flow", False))
    envs = [FFMPVec(n, cfg, device=DEV, autotune=False, fused=False, frame_window=3, **kw) for _ in range(2)]
    rng = np.random.default_rng(1)
    for e in envs:
        e.reset()
    for i in range(8):
        base = (A.RASTER_NT | A.RASTER_TILE4, A.RASTER_PLAIN)[i % 2]
        for j, e in enumerate(envs):
            f = base | (WAVES[i % len(WAVES)] if j == 0 else 0)
            e.fused, e.fused_flags = i % 4 < 2, f
            e.raster_shape = e.raster_shape_newest = (4096, f)
            assert _kernel_waves(e, f) == 0
        act = _act(rng, n, i % 3 == 1)
        for e in envs:
            e.step(act)
        torch.cuda.synchronize()
        x, y = envs
        assert torch.equal(_bits(x._frames), _bits(y._frames)), i
        for k in KEYS + ("flow", "frame_tags"):
            if getattr(y, k) is not None:
                assert torch.equal(_bits(getattr(x, k)), _bits(getattr(y, k))), (i, k)
    for e in envs:
        e.close()
