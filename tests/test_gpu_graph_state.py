"""Captured graphs against the host state that keeps changing underneath them.  A HIP graph freezes
its launches' arguments by value: the config struct (the seed that keys the auto-reset RNG), device
pointers, ring-slot addresses, host arrays such as temporal_maps' lag offsets.  The reference is a
twin FFMPVec of the same config driven by plain step() calls (pinned to the oracle by
tests/test_gpu_parity.py); everything is compared bit for bit.

1. a config change (reset(seed=s), seed(s), load_state_dict of another seed) makes StepGraph.replay()
   raise, for every graph form, and a fresh capture equals the twin; the unchanged seed, a bare
   reset() do not; replay() and capture() after close() raise;
2. state changes that leave a graph valid: masked resets, a reload of an own checkpoint, raster(),
   a poisoned ring slot + invalidate_frame_tags(), launch shapes and tuning changed after the
   capture, a period of single-step graphs in between, invalid ids / NaN commands inside a block;
3. the frame history through replays: temporal_maps(k) for every k after every replay, after a
   partial graph and after interleaved step() calls;
4. the sensor, planner and follower entry points captured into a graph of the caller's on a stream
   of the caller's, writing into guarded out= tensors, replayed after whole ring periods; a callable
   closed-loop policy over lidar_frames.

max_steps = 7: every env is reset inside every block of eight steps or more, so the seed is read."""
import numpy as np
import pytest
import torch

from flow_field_based_motion_planner_amd import _abi
from flow_field_based_motion_planner_amd.config import FFMPConfig
from flow_field_based_motion_planner_amd.vec_env import FFMPVec

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CFG = dict(grid=64, n_obst=8, n_beams=48, moving=True, obst_rmax=0.45, obst_vmax=1.0, world_half=2.4,
           goal_min=0.6, goal_max=1.5, max_steps=7, seed=31)
N = 96

# graph form -> (FFMPVec arguments, capture() arguments)
W8 = dict(frame_window=8, seamless=True, fused=False)
PLAIN = dict(pipelined=False, skewed=False)
FORMS = {
    "seamless8": (W8, PLAIN),
    "seamless3": (dict(frame_window=3, seamless=True, fused=False), PLAIN),
    "wrap4": (dict(frame_window=4, seamless=False, fused=False), PLAIN),
    "pair2": (dict(frame_window=2, fused=False), PLAIN),
    "one_launch": (dict(frame_window=8, seamless=True, fused=True), PLAIN),
    "pipelined": (W8, dict(pipelined=True)),
    "skewed": (W8, dict(skewed=True)),
    "reactive": (dict(frame_window=4, seamless=False, fused=False), dict(policy="reactive")),
    "field": (W8, dict(policy="field")),
    "nav": (dict(frame_window=3, seamless=True, fused=False), dict(policy="nav")),
    "commands": (dict(frame_window=4, seamless=False, fused=False), dict(commands=True)),
}
POLICY = {"reactive": FFMPVec.policy_reactive, "field": FFMPVec.policy_field, "nav": FFMPVec.policy_nav}


def _snap(env):
    d = {k: v.detach().cpu().numpy().copy() for k, v in env.obs.items()}  # state_m and the potential plane included
    for k in ("reward", "done", "is_goal", "collision", "truncated", "pose", "goal", "obst", "t", "episode", "record"):
        d[k] = getattr(env, k).detach().cpu().numpy().copy()
    return d


def _same(a, b, where):
    torch.cuda.synchronize()
    sa, sb = _snap(a), _snap(b)
    for k in sb:
        assert np.array_equal(sa[k], sb[k], equal_nan=True), (where, k)


def _pair(form, **kw):
    cfg = FFMPConfig(**CFG)
    kw = dict(dict(device=DEV, autotune=False), **FORMS[form][0], **kw)
    return FFMPVec(N, cfg, **kw), FFMPVec(N, cfg, **kw)


class _Drive:
    """One graph form on env `a` against plain steps of its twin `b`."""

    def __init__(self, form, a, b, seed=5):
        self.form, self.a, self.b = form, a, b
        self.cap = FORMS[form][1]
        per = a.graph_period()
        self.steps = per * -(-8 // per)  # >= 8 steps: every env is reset (max_steps 7) inside a block
        self.rng = np.random.default_rng(seed)
        self.g = None

    def capture(self):
        self.g = self.a.capture(self.steps, **self.cap)
        assert self.g.chainable and self.g.steps == self.steps
        assert self.g.pipelined == bool(self.cap.get("pipelined")) and self.g.skewed == bool(self.cap.get("skewed"))
        return self.g

    def inputs(self):
        """The block a replay takes: ids, commands, or None for a closed loop."""
        if self.cap.get("policy"):
            return None
        if self.cap.get("commands"):
            return torch.as_tensor(self.rng.uniform([-0.1, -0.7], [0.7, 0.7], (self.steps, N, 2)), device=DEV)
        return torch.as_tensor(self.rng.integers(0, 28, (self.steps, N)), device=DEV)

    def twin(self, blk):
        for i in range(self.steps):
            self.b.step(POLICY[self.cap["policy"]](self.b) if blk is None else blk[i])

    def block(self, where, blk=None, check=True):
        """One replay on `a`, the same steps on `b`; auto-resets happened inside; equal afterwards."""
        before = int(self.a.episode.sum())
        blk = self.inputs() if blk is None else blk
        self.g.replay(blk)
        self.twin(blk)
        if check:
            _same(self.a, self.b, (self.form, where))
        assert int(self.a.episode.sum()) >= before + N, (self.form, where)  # the seed was read

    def refused(self, where):
        """The replay raises, names the cause and the remedy, and runs nothing."""
        with pytest.raises(RuntimeError, match=r"config changed since capture.*captured again"):
            self.g.replay(self.inputs())
        _same(self.a, self.b, (self.form, where, "refused"))

    def both(self, fn):
        fn(self.a)
        fn(self.b)


# ------------------------------------------------------------------ 1. config changes invalidate
@pytest.mark.parametrize("form", list(FORMS))
def test_config_change_refuses_replay(form):
    a, b = _pair(form)
    d = _Drive(form, a, b)
    d.both(lambda e: e.reset())
    assert a._wpos == 0
    g0 = d.capture()
    d.block("first")
    # the unchanged seed and a bare reset(): the same config, the graph stays valid
    d.both(lambda e: e.reset(seed=CFG["seed"]))
    d.block("reset(seed=same)")
    d.both(lambda e: e.reset())
    d.block("reset()")
    assert d.g is g0 and a._cfg_gen == 0
    # a new seed through a full reset: the frame position is the capture's, only the config differs
    d.both(lambda e: e.reset(seed=77))
    assert a._wpos == g0.wpos
    d.refused("reset(seed=77)")
    assert d.capture() is not g0
    d.block("reset(seed=77) 1")
    d.block("reset(seed=77) 2")
    with pytest.raises(RuntimeError, match="config changed"):  # the old graph stays refused
        g0.replay(d.inputs())
    # seed() alone: nothing moves but the config
    d.both(lambda e: e.seed(79))
    d.refused("seed(79)")
    d.capture()
    d.block("seed(79) 1")
    d.block("seed(79) 2")
    # a checkpoint of an env with another seed
    c = FFMPVec(N, FFMPConfig(**dict(CFG, seed=78)), device=DEV, autotune=False, **FORMS[form][0])
    c.reset()
    sd = c.state_dict()
    c.close()
    d.both(lambda e: e.load_state_dict(sd))
    assert a.cfg.seed == 78
    d.refused("load_state_dict(seed 78)")
    d.capture()
    d.block("load_state_dict 1")
    d.block("load_state_dict 2")
    gen = a._cfg_gen
    d.both(lambda e: e.seed(78))  # the seed it has: no new generation
    assert a._cfg_gen == gen == 3
    d.block("seed(same)")
    a.close()
    with pytest.raises(RuntimeError, match="closed"):
        d.g.replay(d.inputs())
    with pytest.raises(RuntimeError, match="closed"):
        a.capture(d.steps, **d.cap)
    b.close()


def test_use_graphs_cache_is_dropped_and_refilled():
    """The single-step graphs keep their behaviour: dropped by a new seed and re-captured lazily,
    kept by the same seed."""
    a, b = _pair("seamless3")
    a.use_graphs(True)
    rng = np.random.default_rng(3)
    acts = torch.as_tensor(rng.integers(0, 28, (27, N)), device=DEV)
    for e in (a, b):
        e.reset()
    for k in range(9):
        a.step(acts[k])
        b.step(acts[k])
    assert len(a._graphs) == 3
    for e in (a, b):
        e.reset(seed=CFG["seed"])
    assert len(a._graphs) == 3 and a._cfg_gen == 0
    for e in (a, b):
        e.seed(77)
    assert len(a._graphs) == 0 and a._cfg_gen == 1
    for k in range(9, 18):
        a.step(acts[k])
        b.step(acts[k])
        _same(a, b, ("seed(77)", k))
    assert len(a._graphs) == 3 and int(b.episode.sum()) >= N
    a.close()
    b.close()


# ------------------------------------------------------------------ 2. state changes that keep a graph valid
@pytest.mark.parametrize("form", list(FORMS))
def test_state_changes_keep_the_graph(form):
    a, b = _pair(form)
    assert a.sparse_frames and b.sparse_frames
    d = _Drive(form, a, b, seed=11)
    d.both(lambda e: e.reset())
    g = d.capture()
    rec_ptr = a.record.data_ptr()
    W = a.frame_window
    d.block("first")

    # a masked reset with an arbitrary mask
    m = torch.as_tensor(np.random.default_rng(1).integers(0, 2, N).astype(bool), device=DEV)
    assert 0 < int(m.sum()) < N
    d.both(lambda e: e.reset(mask=m))
    _same(a, b, (form, "reset(mask)"))
    d.block("reset(mask) 1")
    d.block("reset(mask) 2")

    # an own checkpoint from one block earlier (the pipelined and skewed replays go through two record buffers)
    sda, sdb = a.state_dict(), b.state_dict()
    d.block("past the checkpoint")
    a.load_state_dict(sda)
    b.load_state_dict(sdb)
    assert a.record.data_ptr() == rec_ptr and a._state_c.record == rec_ptr
    assert a._cfg_gen == 0
    _same(a, b, (form, "load_state_dict"))
    d.block("load_state_dict 1")
    d.block("load_state_dict 2")

    # a re-raster
    d.both(lambda e: e.raster())
    _same(a, b, (form, "raster"))
    d.block("raster 1")
    d.block("raster 2")

    # garbage in a ring slot outside the current pair, tags invalidated: the replays' rasters store every cell
    if W > 2:
        slot = (a._wpos + 2) % W
        for e in (a, b):
            e._frames[slot].fill_(3.0)
            e.invalidate_frame_tags(slot)
        d.block("poisoned slot 1")
        d.block("poisoned slot 2")
        assert not bool((a._frames[:W] == 3.0).any())  # frames hold 0 / 255: the slot was rewritten whole

    # launch shapes and tuning changed on `a` after the capture: baked into the graph, the same bits anyway
    a.raster_shape = a.raster_shape_newest = (2048, _abi.RASTER_NT | _abi.RASTER_XCD)
    a.fused_flags = _abi.RASTER_PLAIN | _abi.RASTER_XCD
    d.block("shapes 1")
    d.block("shapes 2")
    waves, lanes = _abi.set_tuning(_abi.TUNE_ENV_WAVES, 1), _abi.set_tuning(_abi.TUNE_ENV_LANES, 16)
    try:
        d.block("tuning 1")
        d.block("tuning 2")
    finally:
        _abi.set_tuning(_abi.TUNE_ENV_WAVES, waves)
        _abi.set_tuning(_abi.TUNE_ENV_LANES, lanes)

    # a whole period of single-step graphs between two replays
    a.use_graphs(True)
    acts = torch.as_tensor(d.rng.integers(0, 28, (a.graph_period(), N)), device=DEV)
    for k in range(a.graph_period()):
        a.step(acts[k])
        b.step(acts[k])
    _same(a, b, (form, "use_graphs period"))
    assert a._wpos == g.wpos
    d.block("use_graphs 1")
    a.use_graphs(False)
    d.block("use_graphs 2")

    # invalid ids (NaN commands) inside a replayed block: the error bit on both, cleared, and on they go
    blk = d.inputs()
    if blk is not None:
        if blk.is_floating_point():
            blk[2, 5, 1] = float("nan")
        else:
            blk[2, 5], blk[d.steps - 1, 17] = 99, -1
        d.block("bad input", blk)
        for e in (a, b):
            with pytest.raises(ValueError):
                e.check_errors()
        d.block("after bad input")
    for e in (a, b):
        e.check_errors()
    assert d.g is g  # one graph served all of it
    a.close()
    b.close()


# ------------------------------------------------------------------ 3. frame history through replays
RINGS = {"seamless6": dict(frame_window=6, seamless=True), "wrap5": dict(frame_window=5, seamless=False),
         "u8f16": dict(frame_window=6, seamless=True, obs_format="u8f16")}


def _history_same(a, b, where):
    assert a.max_temporal_frames == b.max_temporal_frames, where
    assert a._hist_from_reset == b._hist_from_reset and len(a._hist) == len(b._hist), (where, a._hist, b._hist)
    for k in range(1, a.max_temporal_frames + 1):
        ma, mb = a.temporal_maps(k), b.temporal_maps(k)
        assert ma.shape == (N, k, 64, 64) and torch.equal(ma, mb), (where, k)
    _same(a, b, where)


@pytest.mark.parametrize("ring,cap", [("seamless6", "plain"), ("seamless6", "skewed"), ("seamless6", "pipelined"),
                                      ("wrap5", "plain"), ("wrap5", "skewed"), ("wrap5", "pipelined"),
                                      ("u8f16", "plain"), ("u8f16", "pipelined")])
def test_frame_history_follows_replays(ring, cap):
    cfg = FFMPConfig(**CFG)
    kw = dict(device=DEV, autotune=False, fused=False, **RINGS[ring])
    a, b = FFMPVec(N, cfg, **kw), FFMPVec(N, cfg, **kw)
    per = a.graph_period()
    assert per % 2 == 0 and a.max_temporal_frames == (4 if ring == "wrap5" else 6)
    rng = np.random.default_rng(21)

    def acts(k):
        return torch.as_tensor(rng.integers(0, 28, (k, N)), device=DEV)

    def steps(blk):
        for row in blk:
            a.step(row)
            b.step(row)

    for e in (a, b):
        e.reset()
    _history_same(a, b, "reset")
    steps(acts(2))  # the capture starts mid-ring, the history still short of the ring
    g = a.capture(per, pipelined=cap == "pipelined", skewed=cap == "skewed")
    assert g.chainable and g.skewed == (cap == "skewed") and g.pipelined == (cap == "pipelined")
    ep0 = int(a.episode.sum())
    for r in range(3):
        blk = acts(per)
        g.replay(blk)
        for row in blk:
            b.step(row)
        _history_same(a, b, ("replay", r))
    assert int(a.episode.sum()) >= ep0 + N  # 3 periods >= 12 steps: every env was reset inside the replays
    # a partial graph leaves the ring off the capture's position; step() calls bring it back
    part = a.capture(per - 1, pipelined=False, skewed=False)
    assert not part.chainable
    blk = acts(per - 1)
    part.replay(blk)
    for row in blk:
        b.step(row)
    _history_same(a, b, "partial")
    with pytest.raises(RuntimeError, match="frame position"):
        g.replay(acts(per))
    steps(acts(1))
    _history_same(a, b, "step after partial")
    for r in range(2):  # whole periods of step() calls interleaved with replays
        blk = acts(per)
        g.replay(blk)
        for row in blk:
            b.step(row)
        _history_same(a, b, ("replay after steps", r))
        steps(acts(per))
        _history_same(a, b, ("steps after replay", r))
    a.close()
    b.close()


# ------------------------------------------------------------------ 4. entry points inside a caller's graph
GUARD, POISON, PAD = 0xA5, 0x5A, 4096


class _Guarded:
    """A tensor in the middle of a larger buffer filled with a guard byte."""

    def __init__(self, shape, dtype):
        nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        self.buf = torch.full((2 * PAD + nbytes,), GUARD, dtype=torch.uint8, device=DEV)
        self.bytes = self.buf[PAD:PAD + nbytes]
        self.t = self.bytes.view(dtype).view(shape)
        assert self.t.data_ptr() % 16 == 0

    def intact(self):
        return bool((self.buf[:PAD] == GUARD).all()) and bool((self.buf[PAD + self.bytes.numel():] == GUARD).all())


def _entries(env):
    """name -> (shapes and dtypes of the out= tensors, call(env, outs) -> the tensors to compare)."""
    n, G, fd = env.num_envs, env.cfg.grid, env._frame_dtype
    pair, one, cmd = [((n, 2, G, G), fd)], [((n, G, G), fd)], [((n, 2), torch.float64)]

    def nav(tile):
        def call(e, o):
            d = e.nav_field(cost=True, direction=True, tile=tile)
            return [d[k] for k in ("target", "geo_cost", "cost", "dir", "geo_dist")]
        return call

    return {
        "visible": (pair, lambda e, o: [e.visible_frames(out=o[0])]),
        "visible_range": (pair, lambda e, o: [e.visible_frames(out=o[0], max_range=1.0)]),
        "visible_newest": (one, lambda e, o: [e.visible_frames(out=o[0], newest_only=True)]),
        "visible_newest_range": (one, lambda e, o: [e.visible_frames(out=o[0], newest_only=True, max_range=1.0, unknown=7)]),
        "lidar": (pair, lambda e, o: [e.lidar_frames(out=o[0], shift=False)]),
        "lidar_shift": (pair, lambda e, o: [e.lidar_frames(out=o[0], shift=True)]),
        "nav_field": ([], nav(None)),
        "nav_field_tiled": ([], nav(32)),
        "policy_nav": (cmd, lambda e, o: [e.policy_nav(out=o[0])]),
        "policy_nav_tiled": (cmd, lambda e, o: [e.policy_nav(out=o[0], tile=32)]),
        "policy_nav_visible": (cmd, lambda e, o: [e.policy_nav(out=o[0], visible=True)]),
        "policy_nav_lidar": (cmd, lambda e, o: [e.policy_nav(out=o[0], lidar=True)]),
        "policy_field": (cmd, lambda e, o: [e.policy_field(out=o[0])]),
        "policy_reactive": ([((n,), torch.int64)], lambda e, o: [e.policy_reactive(out=o[0])]),
        "temporal_maps3": ([((n, 3, G, G), fd)], lambda e, o: [e.temporal_maps(3, out=o[0])]),
    }


def _bytes(t):
    return t.detach().contiguous().cpu().numpy().view(np.uint8)


@pytest.mark.parametrize("fmt", ["f32", "u8f16"])
def test_entry_points_in_a_callers_graph(fmt):
    """Every entry point: one eager call (the warm-up the docstrings ask for), one call captured on a
    stream of the caller's into guarded out= tensors, then after each whole ring period the replay
    equals a fresh eager call, and no byte around the outputs moved."""
    cfg = FFMPConfig(**CFG)
    W = 6
    env = FFMPVec(N, cfg, device=DEV, autotune=False, frame_window=W, seamless=True, fused=False, obs_format=fmt)
    assert env.graph_period() == W
    rng = np.random.default_rng(2)

    def steps(k):
        for _ in range(k):
            env.step(torch.as_tensor(rng.integers(0, 28, N), device=DEV))

    env.reset()
    steps(W + 1)  # mid-ring, the history as deep as the ring
    entries = _entries(env)
    graphs = {}
    for name, (specs, call) in entries.items():
        outs = [_Guarded(s, dt) for s, dt in specs]
        call(env, [_Guarded(s, dt).t for s, dt in specs])  # eager once: sector table, workspaces
        if name == "lidar_shift":  # its pair is state: the previous call's newest frame is the next older one
            env.lidar_frames(out=outs[0].t, shift=False)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=torch.cuda.Stream(device=DEV)):
            res = call(env, [o.t for o in outs])
        for o, r in zip(outs, res):
            assert r is o.t
        graphs[name] = (g, outs, res)
    shift_ref = graphs["lidar_shift"][1][0].t.clone()
    ep0 = int(env.episode.sum())
    for period in range(2):
        steps(W)
        first = env.record[:, 10] != 0
        for name, (g, outs, res) in graphs.items():
            specs, call = entries[name]
            if name == "lidar_shift":
                prev_newest = outs[0].t[:, 1].clone()
            else:
                for o in outs:
                    o.bytes.fill_(POISON)
                for r in res[len(outs):]:  # tensors the call made itself (inside the capture)
                    r.view(torch.uint8).fill_(POISON)
            g.replay()
            torch.cuda.synchronize()
            if name == "lidar_shift":
                want = [env.lidar_frames(out=shift_ref, shift=True)]
                older, newest = outs[0].t[:, 0], outs[0].t[:, 1]
                assert torch.equal(older[~first], prev_newest[~first]), (period, name, "older is the last newest")
                assert torch.equal(older[first], newest[first]), (period, name, "first observation")
                assert int((~first).sum()) > 0
            else:
                want = call(env, [_Guarded(s, dt).t for s, dt in specs])
            assert len(want) == len(res)
            for i, (r, w) in enumerate(zip(res, want)):
                assert r.shape == w.shape and r.dtype == w.dtype, (period, name, i)
                assert np.array_equal(_bytes(r), _bytes(w)), (period, name, i)
            for o in outs:
                assert o.intact(), (period, name, "guard bytes")
    assert int(env.episode.sum()) >= ep0 + N  # 12 steps: every env was reset between the replays
    # the outputs are not trivial: frames with hidden / occupied cells, reachable goals, turning commands
    torch.cuda.synchronize()
    assert bool((graphs["visible"][2][0] == 128).any()) and bool((graphs["lidar"][2][0] == 255).any())
    assert bool((graphs["nav_field"][2][1] > 0).any()) and bool((graphs["policy_nav"][2][0] != 0).any())
    env.close()


@pytest.mark.parametrize("fmt", ["f32", "u8f16"])
def test_closed_loop_over_lidar_frames(fmt):
    """capture(policy=fn), fn making its ids from the map of the scan (lidar_frames into a buffer of
    its own, torch ops on the device): stop and turn when a window of cells ahead holds a hit."""
    cfg = FFMPConfig(**CFG)
    kw = dict(device=DEV, autotune=False, frame_window=8, seamless=True, fused=False, obs_format=fmt)
    a, b = FFMPVec(N, cfg, **kw), FFMPVec(N, cfg, **kw)
    G, c = cfg.grid, cfg.grid // 2
    table = torch.as_tensor([24, 6], device=DEV)  # ahead at full speed; stop and turn left
    bufs = {id(e): torch.zeros((N, G, G), dtype=e._frame_dtype, device=DEV) for e in (a, b)}
    seen = []

    def fn(env):
        buf = env.lidar_frames(unknown=0, newest_only=True, out=bufs[id(env)])
        blocked = (buf[:, c + 3:c + 10, c - 1:c + 2] == 255).flatten(1).any(1)
        if env is b:
            seen.append(blocked)
        return table[blocked.to(torch.int64)]

    for e in (a, b):
        e.reset()
    ids = fn(a)  # eager once before the capture: the sector table is built on the host
    assert ids.shape == (N,) and ids.dtype == torch.int64
    g = a.capture(policy=fn)
    assert g.steps == 8 and callable(g.policy)
    for r in range(2):
        g.replay()
        for k in range(g.steps):
            b.step(fn(b))
        _same(a, b, (fmt, r))
        assert torch.equal(bufs[id(a)], bufs[id(b)]), (fmt, r)
    assert int(a.episode.sum()) >= N
    blocked = torch.stack(seen)
    assert 0 < int(blocked.sum()) < blocked.numel()  # both rows of the table were used
    a.close()
    b.close()
