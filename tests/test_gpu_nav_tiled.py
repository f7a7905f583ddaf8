"""The tiled navigation field on the GPU (include/ffmp.h ffmp_nav_field_tiled) against the
NumPy restatement of the SPEC (tests/nav_field_ref.py), bit for bit in cost, dir, target, geo_cost
and cmd:

1. forced small tiles on live env frames (2 x 2, 3 x 3 and ragged 4 x 4 tiles; negative frame stride;
   uint8 frames; more envs than one);
2. synthetic planes at the same shapes, the serpentine maze crossing a tile edge in every corridor;
3. a single tile equals the untiled kernel, also with more envs than the persistent grid has slots;
4. real sizes: G = 260 (256 + 4) and G = 512, live frames and the mazes up to the cost cap;
5. any subset of the outputs, and the scalar loads of an unaligned frame;
6. capture(policy="nav") equals step(policy_nav()); the workspace's lifetime; the trap's closed loop."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from flow_field_based_motion_planner_amd import _abi
from flow_field_based_motion_planner_amd.config import FFMPConfig
from flow_field_based_motion_planner_amd.vec_env import FFMPVec
from tests import nav_field_ref as R
from tests.parity_util import gpu_snapshot

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = ("cost", "dir", "target", "geo_cost", "cmd")


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.int64) if x.dtype == np.float64 else x


def _gpu(env, rows=slice(None), tile=None, **knobs):
    """Every output of the kernel for the current observation (two launches: planes + cmd)."""
    field_kn = {k: v for k, v in knobs.items() if k != "turn_sin"}
    d = env.nav_field(cost=True, direction=True, tile=tile, **field_kn)
    out = {k: d[k].cpu().numpy()[rows] for k in ("cost", "dir", "target", "geo_cost")}  # (no uint16 indexing on the device)
    out["cmd"] = env.policy_nav(tile=tile, **knobs).cpu().numpy()[rows]
    gd = d["geo_dist"].cpu().numpy()[rows]
    assert np.array_equal(gd, np.where(out["geo_cost"] < 0, np.inf, out["geo_cost"] * (env.cfg.res / 5.0)))
    return out


def _expect(env, rows=slice(None), **knobs):
    frames = env.state_m[:, 1].cpu().numpy()[rows]
    goals = env.record[:, 8:10].cpu().numpy()[rows]
    return R.nav_field(frames, goals, env.cfg, **knobs)


def _assert_same(got, exp, where):
    for k in KEYS:
        assert got[k].dtype == exp[k].dtype and got[k].shape == exp[k].shape, (where, k, got[k].dtype, got[k].shape)
        bad = np.nonzero(_bits(got[k]) != _bits(exp[k]))
        assert not len(bad[0]), (where, k, [b[:5] for b in bad], got[k][bad][:5], exp[k][bad][:5])


# ------------------------------------------------------------------ 1. forced tiles on live frames
FORMS = {
    "f32_seamless8": dict(frame_window=8, seamless=True),
    "u8f16_w2": dict(frame_window=2, obs_format="u8f16"),
}
LIVE = {  # the parameters of tests/test_gpu_nav_field.py's LIVE configs (96: those of 100)
    64: dict(grid=64, n_obst=8, n_beams=0, moving=True, world_half=1.3, goal_min=0.6, goal_max=1.5, obst_rmax=0.4,
             obst_vmax=1.0, max_steps=6, seed=31),
    96: dict(grid=96, n_obst=12, n_beams=0, moving=True, world_half=2.0, goal_min=0.8, goal_max=2.4, obst_rmax=0.5,
             obst_vmax=1.0, max_steps=6, seed=12),
    100: dict(grid=100, n_obst=12, n_beams=0, moving=True, world_half=2.0, goal_min=0.8, goal_max=2.4, obst_rmax=0.5,
              obst_vmax=1.0, max_steps=6, seed=12),
}
SHAPES = [64, 96, 100]  # at tile 32: 2 x 2 tiles; 3 x 3 (one tile with all 8 neighbours); 4 x 4, the last 4 cells wide


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("n", [1, 65])
@pytest.mark.parametrize("G", SHAPES)
def test_forced_tiles_equal_restatement_on_live_frames(G, n, form):
    """W + 2 steps at least (the ring wraps; the seamless ring's wrap step reaches the newest frame
    through a NEGATIVE frame stride), resets inside (max_steps 6).  n = 1: every step is compared;
    n = 65: at the reset observation and the two steps around the wrap, every fourth env at the wrap
    step and three envs at the other two against the restatement (it is the cost), and every env
    against the untiled kernel."""
    cfg = FFMPConfig(**LIVE[G])
    env = FFMPVec(n, cfg, device=DEV, autotune=False, **FORMS[form])
    W = env.frame_window
    if env.ring == "seamless":
        env.WRAP_VIA_ALIAS = False
    env.reset()
    rng = np.random.default_rng(G + n)
    steps = max(W + 2, 7)
    checked = negative = 0
    for k in range(steps + 1):
        if n == 1 or k in (0, W - 1, W):
            rows = slice(None) if n == 1 else (list(range(0, n, 4)) if k == W else [0, 32, 64])
            got = _gpu(env, tile=32)
            _assert_same({key: v[rows] for key, v in got.items()}, _expect(env, rows), (k,))
            if n > 1:  # every env against the untiled kernel (tests/test_gpu_nav_field.py holds that to the restatement)
                _assert_same(got, _gpu(env), (k, "untiled"))
            checked += 1
            negative += int(env._obs_c.state_m_frame_stride < 0)
        if k < steps:
            env.step(torch.as_tensor(rng.integers(0, 28, n), device=DEV))
    assert checked >= 3
    if env.ring == "seamless":
        assert negative >= 1
    if n == 65:
        assert int(env.episode.sum()) > 0
    env.check_errors()
    env.close()


# ------------------------------------------------------------------ 2. synthetic planes
def _scenes(G):
    """name -> (frame, goal float32 (2,)): the scenes of tests/test_gpu_nav_field.py."""
    cfg = FFMPConfig(grid=G, n_obst=0, n_beams=0)
    f = cfg.f32_constants()
    c = G // 2
    at = lambda cell: R.cell_to_goal(cell, f["half_f"], f["res_f"])  # noqa: E731
    z = np.zeros((G, G), np.float32)
    ring = z.copy()
    ring[c - 6:c + 7, c - 6] = ring[c - 6:c + 7, c + 6] = ring[c - 6, c - 6:c + 7] = ring[c + 6, c - 6:c + 7] = 255.0
    blob = z.copy()
    blob[c + 10:c + 16, c - 12:c - 4] = 255.0
    maze, maze_cell = R.serpentine(G)
    return cfg, {"empty": (z, at((G - 3, 5))), "full": (np.full((G, G), 255.0, np.float32), at((c + 9, c))),
                 "ringed": (ring, at((c + 20, c - 3))), "goal_on_hard": (blob, at((c + 12, c - 8))),
                 "nan_goal": (blob, np.float32([np.nan, 0.3])), "maze": (maze, at(maze_cell))}


def _set_scene(env, e, frame, goal):
    env.state_m[e, 1].copy_(torch.as_tensor(frame, device=DEV))
    env.record[e, 8:10].copy_(torch.as_tensor(goal, device=DEV))


MAZE = {64: (2355, 18257), 96: (5407, 44125), 100: (5680, 46024)}  # geo_cost: margin 0, defaults (the restatement's)


@pytest.mark.parametrize("G", SHAPES)
def test_synthetic_planes_through_forced_tiles(G):
    """The serpentine's corridors run the width of the plane on an 8-cell pitch, so every one of them
    crosses every vertical tile edge, and the path takes them all: each tile comes due many times."""
    cfg, scenes = _scenes(G)
    env = FFMPVec(3, cfg, device=DEV, autotune=False, frame_window=2)
    env.reset()
    seen = {}
    for names, knobs in ((("empty", "full", "ringed"), {}), (("goal_on_hard", "nan_goal", "maze"), {}),
                         (("goal_on_hard", "nan_goal", "maze"), dict(margin=0))):
        for e, name in enumerate(names):
            _set_scene(env, e, *scenes[name])
        got, exp = _gpu(env, tile=32, **knobs), _expect(env, **knobs)
        _assert_same(got, exp, (names, knobs))
        for e, name in enumerate(names):
            seen[name, bool(knobs)] = int(got["geo_cost"][e]), tuple(got["target"][e]), int((got["cost"][e] < 65535).sum())
    print(G, seen)
    assert seen["empty", False][0] > 0 and seen["empty", False][2] == G * G
    assert seen["full", False] == (-1, (0, 0), 1)  # both cleared cells stand alone: only the goal's own 0
    assert seen["ringed", False][:2] == (-1, (0, 0)) and seen["ringed", False][2] > G
    assert seen["goal_on_hard", False][0] == -1 and seen["goal_on_hard", True][0] == -1
    assert seen["nan_goal", False] == (-1, (0, 0), 0)
    assert (seen["maze", True][0], seen["maze", False][0]) == MAZE[G]
    env.close()


# ------------------------------------------------------------------ 3. one tile == the untiled kernel
@pytest.mark.parametrize("G", [64, 256])
def test_single_tile_equals_untiled_kernel(G):
    cfg = FFMPConfig(**dict(LIVE[64], grid=G, seed=5))
    env = FFMPVec(3, cfg, device=DEV, autotune=False, frame_window=3)
    env.reset()
    for a in (3, 24):
        env.step(torch.full((3,), a, dtype=torch.int64, device=DEV))
    maze, cell = R.serpentine(G)
    f = cfg.f32_constants()
    _set_scene(env, 2, maze, R.cell_to_goal(cell, f["half_f"], f["res_f"]))
    for knobs in ({}, dict(margin=0)):
        tiled, plain = _gpu(env, tile=256, **knobs), _gpu(env, **knobs)
        _assert_same(tiled, plain, (G, knobs))
    assert env.nav_workspace_bytes() > 0
    env.close()


def test_more_envs_than_slots():
    """At tile 256 a workgroup takes nearly all of a CU's LDS, so the persistent grid has one slot per
    CU and 44 envs more than slots make the first 44 workgroups plan a second env in the same slot and
    the same LDS — one of them after an env with a NaN goal, which leaves the slot untouched.  Every
    env equals the untiled kernel; a first-round and two second-round envs equal the restatement."""
    G = 256
    cfg = FFMPConfig(**dict(LIVE[64], grid=G, world_half=3.0, goal_max=3.0, seed=17))
    probe = C.c_size_t()
    lib = _abi.load()
    c = _abi.make_cfg(cfg)
    _abi.check(lib.ffmp_nav_field_tiled_workspace(C.byref(c), 1 << 20, 256, 1, C.byref(probe)), "workspace")
    one = C.c_size_t()
    _abi.check(lib.ffmp_nav_field_tiled_workspace(C.byref(c), 1, 256, 1, C.byref(one)), "workspace")
    slots = probe.value // one.value
    assert 64 <= slots <= 2048
    n = slots + 44
    env = FFMPVec(n, cfg, device=DEV, autotune=False, frame_window=2, obs_format="u8f16")
    env.reset()
    env.step(torch.full((n,), 24, dtype=torch.int64, device=DEV))
    env.record[5, 8] = float("nan")  # env slots + 5 follows it in slot 5
    tiled, plain = _gpu(env, tile=256), _gpu(env)
    _assert_same(tiled, plain, "untiled")
    assert tiled["geo_cost"][5] == -1 and (tiled["cost"][5] == 65535).all()
    rows = [3, slots + 5, n - 1]
    _assert_same({k: v[rows] for k, v in tiled.items()}, _expect(env, rows), "restatement")
    assert (tiled["geo_cost"] > 0).mean() > 0.5  # ordinary frames: most goals are reachable
    env.close()


# ------------------------------------------------------------------ 4. real sizes
def test_grid_260_default_tile_on_live_frames():
    """256 + 4: the default tile leaves a last row and column of tiles 4 cells wide."""
    cfg = FFMPConfig(grid=260, n_obst=12, n_beams=0, moving=True, world_half=3.0, goal_min=1.0, goal_max=3.5, obst_rmax=0.6,
                     obst_vmax=1.0, max_steps=50, seed=8)
    env = FFMPVec(2, cfg, device=DEV, autotune=False, frame_window=2)
    env.reset()
    for a in (24, 3):
        env.step(torch.full((2,), a, dtype=torch.int64, device=DEV))
    _assert_same(_gpu(env), _expect(env), 260)
    with pytest.raises(RuntimeError, match="grid"):  # the untiled entry keeps refusing it
        _abi.check(env.lib.ffmp_nav_field_check(C.byref(env._cfg_c), env._fmt, 2, 40, 4), "ffmp_nav_field_check")
    env.close()


@pytest.fixture(scope="module")
def env512():
    cfg = FFMPConfig(grid=512, n_obst=32, n_beams=0, moving=True, max_steps=50, seed=2)
    env = FFMPVec(2, cfg, device=DEV, autotune=False, frame_window=2)
    env.reset()
    yield env
    env.close()


def test_grid_512_on_stepped_frames(env512):
    env = env512
    for a in (24, 10, 3):
        env.step(torch.full((2,), a, dtype=torch.int64, device=DEV))
    assert env.state_m[:, 1].count_nonzero() > 0
    _assert_same(_gpu(env, [0]), _expect(env, [0]), 512)


@pytest.mark.parametrize("pitch,knobs,geo", [(32, dict(margin=0), 36805), (32, {}, 37211), (16, {}, -1)])
def test_grid_512_serpentine(env512, pitch, knobs, geo):
    """pitch 32: the path takes every corridor of the plane, 36,805 with margin 0 and 37,211 with the
    defaults.  pitch 16: twice the corridors, the costs run into the cap: the largest reachable cost
    is 65,534 and the robot cell is beyond it."""
    env = env512
    cfg = env.cfg
    f = cfg.f32_constants()
    maze, cell = R.serpentine(512, pitch)
    _set_scene(env, 1, maze, R.cell_to_goal(cell, f["half_f"], f["res_f"]))
    got, exp = _gpu(env, [1], **knobs), _expect(env, [1], **knobs)
    _assert_same(got, exp, (pitch, knobs))
    assert int(got["geo_cost"][0]) == geo
    if geo < 0:
        assert int(got["cost"][got["cost"] < 65535].max()) == 65534


# ------------------------------------------------------------------ 5. NULL outputs, scalar loads
def test_any_subset_of_outputs_through_forced_tiles():
    cfg = FFMPConfig(**LIVE[64])
    n, G = 5, 64
    env = FFMPVec(n, cfg, device=DEV, autotune=False, frame_window=3)
    env.nav_tile = 32
    env.reset()
    env.step(torch.as_tensor([3, 10, 24, 27, 0], device=DEV))
    kn = dict(FFMPVec.NAV_DEFAULTS)

    def buffers():
        return dict(cost=torch.full((n, G, G), 0xABCD, dtype=torch.uint16, device=DEV),
                    direction=torch.full((n, G, G), 0x5A, dtype=torch.uint8, device=DEV),
                    target=torch.full((n, 2), -77, dtype=torch.int32, device=DEV),
                    geo_cost=torch.full((n,), -77, dtype=torch.int32, device=DEV),
                    cmd=torch.full((n, 2), -7.5, dtype=torch.float64, device=DEV))

    full = buffers()
    env._nav_launch("nav_field", **kn, **full)
    ref = {k: v.cpu().numpy() for k, v in full.items()}
    exp = _expect(env)
    _assert_same({("dir" if k == "direction" else k): v for k, v in ref.items()}, exp, "all outputs")
    names = list(full)
    for r in range(len(names)):
        for subset in itertools.combinations(names, r):
            b = buffers()
            env._nav_launch("nav_field", **kn, **{k: b[k] for k in subset})
            for k in names:
                got = b[k].cpu().numpy()
                want = ref[k] if k in subset else buffers()[k].cpu().numpy()  # not passed: never touched
                assert np.array_equal(_bits(got), _bits(want)), (subset, k)
    env.close()


@pytest.mark.parametrize("fmt", ["f32", "u8f16"])
def test_unaligned_frames_take_the_scalar_loads(fmt):
    """Frames one element off a 16-byte boundary, with strides of their own, straight through the C ABI."""
    cfg = FFMPConfig(**LIVE[64])
    n, G, tile = 3, 64, 32
    env = FFMPVec(n, cfg, device=DEV, autotune=False, frame_window=3, obs_format=fmt)
    env.reset()
    env.step(torch.as_tensor([24, 10, 3], device=DEV))
    exp = _expect(env)
    newest = env.state_m[:, 1]
    es, stride, frame = newest.element_size(), G * G + 8, 5 * G * G
    buf = torch.zeros(n * stride + 1, dtype=newest.dtype, device=DEV)
    buf[1:].view(n, stride)[:, :G * G].copy_(newest.reshape(n, -1))
    assert (buf.data_ptr() + es) % 16 != 0
    ob = _abi.ObsT()
    C.memmove(C.byref(ob), C.byref(env._obs_c), C.sizeof(ob))
    ob.state_m = buf.data_ptr() + es - frame * es  # the older frame's (never read) address: the newest is `frame` past it
    ob.state_m_stride, ob.state_m_frame_stride = stride, frame
    goals = torch.zeros((n, 5), dtype=torch.float32, device=DEV)
    goals[:, :2] = env.record[:, 8:10]
    got = dict(cost=torch.empty((n, G, G), dtype=torch.uint16, device=DEV), dir=torch.empty((n, G, G), dtype=torch.uint8, device=DEV),
               target=torch.empty((n, 2), dtype=torch.int32, device=DEV), geo_cost=torch.empty(n, dtype=torch.int32, device=DEV),
               cmd=torch.empty((n, 2), dtype=torch.float64, device=DEV))
    nbytes = C.c_size_t()
    _abi.check(env.lib.ffmp_nav_field_tiled_workspace(C.byref(env._cfg_c), n, tile, 1, C.byref(nbytes)), "workspace")
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=DEV)
    assert ws.data_ptr() % 256 == 0
    _abi.check(env.lib.ffmp_nav_field_tiled(C.byref(env._cfg_c), n, C.byref(ob), goals.data_ptr(), 5, 2, 40, 4, 0.25,
                                            *[got[k].data_ptr() for k in KEYS], tile, ws.data_ptr(), ws.numel(),
                                            env._stream()), "ffmp_nav_field_tiled")
    _assert_same({k: v.cpu().numpy() for k, v in got.items()}, exp, fmt)
    # a workspace one byte short of what the launch's slots take is refused
    assert env.lib.ffmp_nav_field_tiled(C.byref(env._cfg_c), n, C.byref(ob), goals.data_ptr(), 5, 2, 40, 4, 0.25,
                                        *[got[k].data_ptr() for k in KEYS], tile, ws.data_ptr(), ws.numel() - 1,
                                        env._stream()) == -1
    assert b"workspace too small" in env.lib.ffmp_last_error()
    env.close()


# ------------------------------------------------------------------ 6. capture, workspace, closed loop
def _same(a, b, where):
    sa, sb = gpu_snapshot(a), gpu_snapshot(b)
    for k in sb:
        if sb[k] is None:
            assert sa[k] is None, (where, k)
        else:
            assert np.array_equal(sa[k], sb[k], equal_nan=sb[k].dtype.kind == "f"), (where, k)


@pytest.mark.parametrize("G,n,nav_tile", [(260, 2, None), (64, 48, 32)])
def test_nav_capture_equals_step_loop(G, n, nav_tile):
    """The tiled launch inside a step graph (run on its own, the G = 260 case raises the kernel's LDS
    cap and asks for its occupancy for the first time in capture()'s preparation, before the capture
    begins): W + 2 steps of the graph equal the step(policy_nav()) loop."""
    cfg = FFMPConfig(**dict(LIVE[64], grid=G, moving=False, max_steps=11))
    a, b = (FFMPVec(n, cfg, device=DEV, autotune=False, frame_window=2) for _ in range(2))
    a.nav_tile = b.nav_tile = nav_tile
    a.reset()
    b.reset()
    steps = a.frame_window + 2
    assert a.nav_workspace_bytes() == 0
    g = a.capture(steps, policy="nav")
    held = a.nav_workspace_bytes()
    assert held > 0  # allocated before the capture began; the graph holds its pointer
    for r in range(2):
        g.replay()
        for k in range(steps):
            b.step(b.policy_nav())
        torch.cuda.synchronize()
        _same(a, b, r)
    assert a.nav_workspace_bytes() == held
    assert float(b.pose[:, :2].abs().sum()) > 0
    _assert_same(_gpu(a, [0]), _expect(a, [0]), "after the replays")
    a.close()
    b.close()


def test_workspace_lifetime():
    cfg = FFMPConfig(**LIVE[64])
    env = FFMPVec(4, cfg, device=DEV, autotune=False)
    env.reset()
    env.policy_nav()  # G = 64, no tile: the untiled kernel, no workspace
    assert env.nav_workspace_bytes() == 0
    env.policy_nav(tile=32)
    one = env.nav_workspace_bytes()
    assert one > 0
    env.policy_nav(tile=32)
    assert env.nav_workspace_bytes() == one  # cached
    env.nav_field(cost=True, tile=32)  # the caller's plane: a smaller workspace of its own
    two = env.nav_workspace_bytes()
    assert one < two < 2 * one
    env.nav_tile = 64
    env.policy_nav()
    assert env.nav_workspace_bytes() > two
    with pytest.raises(RuntimeError, match="tile"):
        env.policy_nav(tile=48)
    env.close()
    assert env.nav_workspace_bytes() == 0
    with pytest.raises(RuntimeError):
        env.policy_nav(tile=32)


def test_trap_nav_reaches_every_goal_through_forced_tiles():
    """tests/test_gpu_nav_field.py's trap (the U-shaped cup of tests/nav_field_ref.py, 8 / 8 goals for
    the restatement driving the NumPy oracle, the last at step 105) with every plan made by the tiled
    kernel at tile 32."""
    cfg = FFMPConfig(**R.TRAP_CFG)
    n = len(R.TRAP_YAWS)
    env = FFMPVec(n, cfg, device=DEV, autotune=False)
    env.nav_tile = 32
    env.reset()
    env.set_scenarios(**R._trap())
    env.check_errors()
    flags = []
    for _ in range(120):
        env.step(env.policy_nav())
        flags.append((env.is_goal.cpu().numpy().copy(), env.collision.cpu().numpy().copy(), env.truncated.cpu().numpy().copy()))
    env.check_errors()
    assert env.nav_workspace_bytes() > 0
    env.close()
    outcome, when = R._outcomes(flags)
    print("trap nav, tile 32: outcomes", outcome.tolist(), "at steps", when.tolist())
    assert (outcome == 1).all()  # every goal reached before any collision or truncation
