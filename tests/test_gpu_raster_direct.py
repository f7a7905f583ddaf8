"""FFMP_RASTER_DIRECT (the tagged float32 raster whose blocks use no LDS, no barrier and one memory round
trip): an env whose two-launch raster carries the flag against the same env with FFMP_RASTER_WAVES (the
staged twin), torch.equal on bit patterns after every step: every physical ring slot, the granule tags,
the potential, the pair view and the record; the tag invariant; and the NumPy oracle through
parity_util.compare.  ffmp_raster_direct says which kernel a launch takes: the flagged env's launches
must answer 1 and the twin's 0 (and ffmp_raster_waves 6 for the twin)."""
import ctypes as C

import numpy as np
import pytest
import torch

from flow_field_based_motion_planner_amd import _abi
from flow_field_based_motion_planner_amd.config import FFMPConfig
from flow_field_based_motion_planner_amd.vec_env import FFMPVec
from oracle.ffmp_oracle import OracleVecEnv
from tests import parity_util, physics_cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
A = _abi
N = 5  # not a multiple of anything
RINGS = {"seamless3": dict(frame_window=3, seamless=True), "pair2": dict(frame_window=2)}
# store flavour and block placement of step i (the deal comes from the test's parameters)
BASE = [A.RASTER_NT, A.RASTER_PLAIN | A.RASTER_XCD, A.RASTER_NT | A.RASTER_XCD, A.RASTER_PLAIN]
CELLS = [2048, 4096, 65536]  # 65536: a whole plane of the grids used here (the launch rounds it down)
KEYS = ("potential", "record", "state_g", "state_v", "state_t", "grad", "lidar", "reward", "done", "is_goal",
        "collision", "truncated", "pose", "obst", "t", "episode")


def _cfg(G, K, **kw):
    return FFMPConfig(**dict(dict(grid=G, n_obst=K, n_beams=16, moving=True, max_steps=5, seed=23), **kw))


def _pair(n, cfg, ring, **kw):
    kw = dict(dict(device=DEV, autotune=False, fused=False, sparse_frames=True), **RINGS[ring], **kw)
    a, b = FFMPVec(n, cfg, **kw), FFMPVec(n, cfg, **kw)
    assert a.frame_tags is not None and b.frame_tags is not None
    return a, b


def _slots(env):
    G2 = env.cfg.grid ** 2
    if env.frame_window == 2:
        return env._frames.reshape(env.num_envs, 2, G2).transpose(0, 1)
    return env._frames[:env.frame_window].reshape(env.frame_window, env.num_envs, G2)


def _bits(t):
    return t.contiguous().view(torch.uint8)


def _same(a, b, what):
    torch.cuda.synchronize()
    assert torch.equal(a.frame_tags, b.frame_tags), (what, "frame_tags")
    assert torch.equal(_bits(_slots(a)), _bits(_slots(b))), (what, "frames")
    assert torch.equal(_bits(a.state_m), _bits(b.state_m)), (what, "state_m")
    for k in KEYS:
        va, vb = getattr(a, k), getattr(b, k)
        if vb is not None:
            assert torch.equal(_bits(va), _bits(vb)), (what, k)
    f = _slots(a)
    S, n, G2 = f.shape
    T = a.frame_tags.shape[2]
    nz = torch.zeros(S, n, T * 64, dtype=torch.bool, device=f.device)
    nz[:, :, :G2] = f != 0
    assert not bool((nz.view(S, n, T, 64).any(dim=3) & (a.frame_tags == 0)).any()), (what, "tag 0 over a non-zero cell")


def _query(env, cells, flags):
    """(ffmp_raster_direct, ffmp_raster_waves): the library's own answer for a launch of this env (no launch)."""
    cfg, obs = C.byref(env._cfg_c), C.cast(C.byref(env._obs_c), C.POINTER(A.ObsT))
    return env.lib.ffmp_raster_direct(cfg, obs, cells, flags), env.lib.ffmp_raster_waves(cfg, obs, flags)


def _set(a, b, i, deal):
    """Step i's two-launch shape: a gets the direct form, b its staged twin."""
    base, cells = BASE[i % len(BASE)] | deal, CELLS[i % len(CELLS)]
    a.raster_shape = a.raster_shape_newest = (cells, base | A.RASTER_DIRECT)
    b.raster_shape = b.raster_shape_newest = (cells, base | A.RASTER_WAVES)
    assert _query(a, cells, base | A.RASTER_DIRECT) == (1, 0)
    assert _query(b, cells, base | A.RASTER_WAVES) == (0, 6)


def _act(rng, n, cmd=False):
    if cmd:
        return torch.as_tensor(rng.uniform([-0.1, -0.7], [0.7, 0.7], (n, 2)), device=DEV)
    return torch.as_tensor(rng.integers(0, 28, n), device=DEV)


# G = 64: one column band of 4-row tiles (four waves per band) and row runs; G = 128: one band of 2-row
# tiles.  Blocks of 2,048 and 4,096 cells and whole planes, cycled over the steps with the store flavour.
@pytest.mark.parametrize("ring", ["seamless3", "pair2"])
@pytest.mark.parametrize("K", [0, 1, 16, 64])
@pytest.mark.parametrize("G,deal", [(64, A.RASTER_TILE4), (64, 0), (128, A.RASTER_TILE2)])
def test_equals_the_staged_twin_and_the_oracle(G, deal, K, ring):
    cfg = _cfg(G, K, world_half=0.65 * G * 0.05)  # some planes reach a wall, others do not
    a, b = _pair(N, cfg, ring)
    ref = OracleVecEnv(cfg, N)
    rng = np.random.default_rng(G + K)
    a.reset()
    b.reset()
    ref.reset()
    _same(a, b, "reset")
    bad = []
    for i in range(13):
        _set(a, b, i, deal)
        act = rng.integers(0, 28, N)
        for e in (a, b):
            e.step(torch.as_tensor(act, device=DEV))
        ref.step(act)
        _same(a, b, i)
        bad += parity_util.compare(parity_util.gpu_snapshot(a), parity_util.oracle_snapshot(ref), f"step {i}")
    assert not bad, bad[:5]
    assert int(a.episode.sum()) >= N  # auto-resets: the older frame written for single envs of a newest-only launch
    a.check_errors()
    a.close()
    b.close()


def _scenario(rng, n, K):
    pose = np.concatenate([rng.uniform(-0.5, 0.5, (n, 2)), rng.uniform(-3.0, 3.0, (n, 1))], 1)
    goal = rng.uniform(1.0, 2.0, (n, 2))
    obst = np.concatenate([rng.uniform(-3.0, 3.0, (n, K, 2)), rng.uniform(-0.5, 0.5, (n, K, 2))], 2)
    return dict(pose=pose, goal=goal, obst=obst, obst_r=rng.uniform(0.1, 0.4, (n, K)))


@pytest.mark.parametrize("ring", ["seamless3", "pair2"])
def test_launch_variants(ring):
    """A mask that skips envs, envs reset in the middle of a run, the command step and an injected
    scenario followed by a step."""
    G, K, deal = 128, 16, A.RASTER_TILE2
    cfg = _cfg(G, K, world_half=0.65 * G * 0.05)
    a, b = _pair(N, cfg, ring)
    rng = np.random.default_rng(7)
    a.reset()
    b.reset()
    for i in range(4):
        _set(a, b, i, deal)
        act = _act(rng, N, cmd=i % 2 == 1)  # (v, w) commands on the odd steps
        for e in (a, b):
            e.step(act)
        _same(a, b, ("warm", i))
    m = torch.as_tensor(np.array([1, 0, 1, 1, 0], bool), device=DEV)
    for e in (a, b):
        e.reset(mask=m)  # reset envs beside stepped ones: header word 10 decides per env
    _same(a, b, "reset(mask)")
    _set(a, b, 5, deal)
    for e in (a, b):
        e.step(_act(np.random.default_rng(8), N))
    _same(a, b, "step after reset(mask)")
    # the masked raster with the tags as the steps left them, then through the public call
    mu8 = (~m).contiguous().view(torch.uint8)
    for full in (False, True):
        for e in (a, b):
            e._raster_launch(full, mu8)
        _same(a, b, ("masked launch", full))
    for e in (a, b):
        e.raster(mask=~m)
    _same(a, b, "raster(mask)")
    sc = _scenario(rng, N, K)
    for e in (a, b):
        e.set_scenarios(**sc, mask=m)
    _same(a, b, "set_scenarios")
    for i in range(6, 9):
        _set(a, b, i, deal)
        act = _act(rng, N, cmd=i % 2 == 1)
        for e in (a, b):
            e.step(act)
        _same(a, b, ("after scenario", i))
    a.check_errors()
    a.close()
    b.close()


@pytest.mark.parametrize("deal", [A.RASTER_TILE2, A.RASTER_TILE4, 0])
def test_margin_at_the_floor(deal):
    """physics_cases' thin_margin (the cull margin at the least value a config may carry), without its
    flow planes: the band cull of the direct form keeps what the staged one keeps."""
    cfg, n, steps = physics_cases.PHYSICS["thin_margin"]
    cfg = cfg.replace(flow=False)
    assert cfg.cull_margin == cfg.cull_floor()
    a, b = _pair(n, cfg, "seamless3")
    ref = OracleVecEnv(cfg, n)
    rng = np.random.default_rng(3)
    a.reset()
    b.reset()
    ref.reset()
    bad = []
    for i in range(steps):
        _set(a, b, i, deal)
        act = rng.integers(0, 28, n)
        for e in (a, b):
            e.step(torch.as_tensor(act, device=DEV))
        ref.step(act)
        _same(a, b, i)
        bad += parity_util.compare(parity_util.gpu_snapshot(a), parity_util.oracle_snapshot(ref), f"step {i}")
    assert not bad, bad[:5]
    a.close()
    b.close()


@pytest.mark.parametrize("G,deal,K", [(64, A.RASTER_TILE4, 16), (128, A.RASTER_TILE2, 64), (64, 0, 1)])
def test_unaligned_record_and_tags(G, deal, K):
    """A record base 4 bytes off a 16-B boundary takes the 4-B disc loads; a tag base and an env stride that
    are no multiples of 16 are read byte by byte anyway: the same planes and tag bytes as the staged twin
    on the same odd buffers, and as the env's own aligned launch."""
    cfg = _cfg(G, K, world_half=0.65 * G * 0.05)
    a, b = _pair(N, cfg, "pair2")
    rng = np.random.default_rng(G + K)
    a.reset()
    b.reset()
    for i in range(3):
        _set(a, b, i, deal)
        act = _act(rng, N)
        for e in (a, b):
            e.step(act)
    _same(a, b, "warm")
    T = a.frame_tags.shape[2]
    stride = T + 5
    out = []
    for env, flag in ((a, A.RASTER_DIRECT), (b, A.RASTER_WAVES)):
        rec = torch.zeros(env.record.numel() + 5, dtype=torch.float32, device=DEV)
        off = 1 + (-(rec.data_ptr() // 4) % 4)  # 4 bytes past a 16-B boundary
        rec[off:off + env.record.numel()] = env.record.reshape(-1)
        assert (rec.data_ptr() + 4 * off) % 16 == 4
        # tags of the caller's own, 1 = unknown: the newest-only launch leaves exact tags in the newest
        # slot's, which the full launch then reads
        tags = torch.ones(2, N * stride + 32, dtype=torch.uint8, device=DEV)
        toff = 3 + (-tags.data_ptr() % 16)
        view = tags[:, toff:toff + N * stride].view(2, N, stride)
        ob = A.ObsTagsT.from_buffer_copy(env._obs_c)
        ob.tags_older = tags[0].data_ptr() + toff
        ob.tags_newest = tags[1].data_ptr() + toff
        ob.tags_env_stride = stride
        assert ob.tags_older % 16 and ob.tags_newest % 16 and stride % 16
        base = A.RASTER_NT | deal
        obp = C.cast(C.byref(ob), C.POINTER(A.ObsT))
        assert env.lib.ffmp_raster_direct(C.byref(env._cfg_c), obp, 2048, base | flag) == int(flag == A.RASTER_DIRECT)
        for newest in (A.RASTER_NEWEST, 0):
            A.check(env.lib.ffmp_raster_ex(C.byref(env._cfg_c), N, rec.data_ptr() + 4 * off, None, C.byref(ob), 2048,
                                           base | flag | newest, env._stream()), "ffmp_raster")
        torch.cuda.synchronize()
        out.append((_bits(_slots(env)).clone(), view[:, :, :T].clone(), view[:, :, T:].clone(), env.potential.clone()))
    for x, y in zip(*out):
        assert torch.equal(x, y)
    assert bool((out[0][2] == 1).all())  # the bytes between the envs' tags are untouched
    # and the env's own, aligned launch of the same record gives the same planes
    _set(a, b, 0, deal)
    for e in (a, b):
        e._raster_launch(True)
    _same(a, b, "aligned")
    assert torch.equal(_bits(_slots(a)), out[0][0])
    a.close()
    b.close()


@pytest.mark.parametrize("ring", ["seamless3", "pair2"])
def test_captured_graph_replays_equal_to_eager_steps(ring):
    G, K, deal = 128, 16, A.RASTER_TILE2
    cfg = _cfg(G, K, world_half=0.65 * G * 0.05)
    a, b = _pair(N, cfg, ring)
    rng = np.random.default_rng(5)
    a.reset()
    b.reset()
    _set(a, b, 1, deal)
    for i in range(3):
        act = _act(rng, N)
        for e in (a, b):
            e.step(act)
    _same(a, b, "warm")
    per = 2 * a.graph_period()
    g = a.capture(per, skewed=False, pipelined=False)
    for r in range(2):
        acts = torch.as_tensor(rng.integers(0, 28, (per, N)), device=DEV)
        g.replay(acts)
        for i in range(per):
            b.step(acts[i])
        _same(a, b, ("replay", r))
    a.check_errors()
    a.close()
    b.close()


@pytest.mark.parametrize("kw,flags,cells,G", [
    (dict(sparse_frames=False), A.RASTER_NT | A.RASTER_TILE4, 4096, 64),                  # no tags
    (dict(sparse_frames=True, flow=True), A.RASTER_NT | A.RASTER_TILE4, 4096, 64),        # flow planes
    (dict(obs_format="u8f16"), A.RASTER_NT | A.RASTER_TILE4, 4096, 64),                   # compact format
    (dict(sparse_frames=True), A.RASTER_NT | A.RASTER_TILE8, 4096, 64),                   # 8-row tiles
    (dict(sparse_frames=True), A.RASTER_NT | A.RASTER_TILE16, 4096, 64),                  # 16-row tiles
])
def test_flag_ignored_where_it_does_not_apply(kw, flags, cells, G):
    """As FFMP_RASTER_WAVES: where the form does not apply the launch is the one without the flag, and
    ffmp_raster_direct answers 0."""
    kw = dict(kw)
    cfg = _cfg(G, 4, flow=kw.pop("flow", False))
    x, y = (FFMPVec(16, cfg, device=DEV, autotune=False, fused=False, frame_window=3, **kw) for _ in range(2))
    rng = np.random.default_rng(1)
    x.reset()
    y.reset()
    for i in range(6):
        for e, f in ((x, flags | A.RASTER_DIRECT | (A.RASTER_WAVES if i % 2 else 0)), (y, flags | (A.RASTER_WAVES if i % 2 else 0))):
            e.raster_shape = e.raster_shape_newest = (cells, f)
            assert _query(e, cells, f)[0] == 0
        assert _query(x, cells, x.raster_shape[1])[1] == _query(y, cells, y.raster_shape[1])[1]
        act = _act(rng, 16, i % 3 == 1)
        x.step(act)
        y.step(act)
        torch.cuda.synchronize()
        assert torch.equal(_bits(x._frames), _bits(y._frames)), i
        for k in KEYS + ("flow", "frame_tags"):
            if getattr(y, k) is not None:
                assert torch.equal(_bits(getattr(x, k)), _bits(getattr(y, k))), (i, k)
    x.close()
    y.close()
