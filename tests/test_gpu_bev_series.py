"""The 12-channel BEV option on the GPU (src/train.py:66 "(occupancy(MONO) + flow(RGB)) * series(3
steps)", :474-486 make_temporal_maps, src/gym_ffmp/envs/ffmp.py:16): ffmp_bev_image against the
oracle's bev_image bit for bit (the stated RGB encoding: parity unpinned against the reference, whose
encoding lived outside its repository); FFMPVec(bev_series=3).bev_maps() against the oracle env's
images fed through the reference's map_memory (TemporalStack, is_first = a reset); the replay
memory's BEV series against what the env emitted; Brain(input_channels=12) updating."""
import ctypes as C

import numpy as np
import pytest
import torch

from flow_field_based_motion_planner_amd import FFMPConfig, _abi
from flow_field_based_motion_planner_amd.replay import ReplayMemory
from flow_field_based_motion_planner_amd.vec_env import FFMPVec
from oracle.ffmp_oracle import Cfg, OracleVecEnv, Record, TemporalStack, bev_image, raster
from tests import series_cases

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CFG = FFMPConfig(grid=64, n_obst=8, n_beams=32, moving=True, max_steps=4, obst_rmax=0.5, obst_vmax=1.2,
                 world_half=3.2, goal_max=2.0, flow=True, seed=31)


def _direct(occ, flow, vmax, compact):
    n, plane = occ.shape[0], occ.shape[1]
    out = torch.full((n, 4, plane), 7, dtype=occ.dtype, device=DEV)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _abi.check(_abi.load().ffmp_bev_image(n, int(compact), occ.data_ptr(), plane, flow.data_ptr(), plane, vmax,
                                          out.data_ptr(), 4 * plane, s), "ffmp_bev_image")
    return out


@pytest.mark.parametrize("plane", [4096, 9801])  # 4 cells per thread / 1 (a plane not a multiple of 4)
@pytest.mark.parametrize("compact", [False, True])
def test_bev_image_equals_oracle(plane, compact):
    vmax = 1.2
    v = np.float32(vmax)
    rng = np.random.default_rng(plane + compact)
    n = 5
    fx = rng.uniform(-1.3, 1.3, (n, plane)).astype(np.float32) * v
    fy = rng.uniform(-1.3, 1.3, (n, plane)).astype(np.float32) * v
    # exact halves of the R / G / B grids, zero, +-vmax and beyond: the rounding mode's cases
    specials = np.array([0.0, v, -v, 2 * v, v / 255, v * 3 / 255, -v / 255, v / 510, -v / 510], np.float32)
    fx[:, :specials.size], fy[:, :specials.size] = specials, specials[::-1]
    occ = (rng.random((n, plane)) < 0.3).astype(np.float32) * 255
    flow = np.stack([fx, fy], 1)
    if compact:
        flow = flow.astype(np.float16)
        got = _direct(torch.as_tensor(occ.astype(np.uint8), device=DEV), torch.as_tensor(flow, device=DEV),
                      vmax, True).cpu().numpy().astype(np.float32)
    else:
        got = _direct(torch.as_tensor(occ, device=DEV), torch.as_tensor(flow, device=DEV), vmax, False).cpu().numpy()
    want = bev_image(occ.reshape(n, 1, plane), flow.astype(np.float32).reshape(n, 2, 1, plane), vmax)
    assert np.array_equal(got, want.reshape(n, 4, plane))


OCC_STRIDES = {"plane": lambda p: p, "2*plane": lambda p: 2 * p, "plane+4": lambda p: p + 4, "plane+1": lambda p: p + 1}
OUT_STRIDES = {"4*plane": lambda p: 4 * p, "12*plane": lambda p: 12 * p, "4*plane+1": lambda p: 4 * p + 1}
# (out_env_stride, the destination's channel offset): the env's ring slot, the replay's k = 3 series layout at
# each of its three images, and a stride that is no multiple of 4
OUT_LAYOUTS = (("4*plane", 0), ("12*plane", 0), ("12*plane", 4), ("12*plane", 8), ("4*plane+1", 0))


@pytest.mark.parametrize("compact", [False, True])
@pytest.mark.parametrize("n", [1, 3, 70])
@pytest.mark.parametrize("plane", [4, 1020, 1024, 1025, 1028, 10000])
def test_bev_image_at_replay_strides(plane, n, compact):
    """ffmp_bev_image at the strides its callers pass, not only the packed ones: the replay's occupancy is the
    newest frame of an [older, newest] pair (occ_env_stride = 2 * plane) and its destination one image of a
    12-channel series (out_env_stride = 12 * plane, at channel 0, 4 or 8).  The planes sit around one block of the
    4-cells-per-thread kernel (1024 cells) and at one thread's worth (4); 1025 takes the 1-cell kernel, and so must
    a stride of plane + 1 or 4 * plane + 1 while the plane itself is a multiple of 4.  Everything outside the four
    written planes of each env keeps the sentinel `out` was filled with."""
    vmax = 1.2
    v = np.float32(vmax)
    rng = np.random.default_rng([plane, n, int(compact)])
    fx = rng.uniform(-1.3, 1.3, (n, plane)).astype(np.float32) * v
    fy = rng.uniform(-1.3, 1.3, (n, plane)).astype(np.float32) * v
    # the rounding mode's cases of test_bev_image_equals_oracle (as many as the plane holds)
    specials = np.array([0.0, v, -v, 2 * v, v / 255, v * 3 / 255, -v / 255, v / 510, -v / 510], np.float32)
    m = min(plane, specials.size)
    fx[:, :m], fy[:, :m] = specials[:m], specials[::-1][:m]
    flow = np.stack([fx, fy], 1)
    if compact:
        flow = flow.astype(np.float16)
    odt, sentinel = (np.uint8, 165) if compact else (np.float32, -3.0)
    occ_all = rng.integers(0, 256, n * (2 * plane + 4)).astype(odt)  # any stored value is copied, not only 0 / 255
    d_occ, d_flow = torch.as_tensor(occ_all, device=DEV), torch.as_tensor(flow, device=DEV)
    lib = _abi.load()
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    want_of = {}
    for occ_name, occ_of in OCC_STRIDES.items():
        occ_stride = occ_of(plane)
        if occ_stride not in want_of:
            occ = np.stack([occ_all[e * occ_stride:e * occ_stride + plane] for e in range(n)])
            want_of[occ_stride] = bev_image(occ.astype(np.float32).reshape(n, 1, plane),
                                            flow.astype(np.float32).reshape(n, 2, 1, plane), vmax).reshape(n, 4 * plane)
        want = want_of[occ_stride]
        for out_name, ch in OUT_LAYOUTS:
            out_stride = OUT_STRIDES[out_name](plane)
            assert ch * plane + 4 * plane <= out_stride and occ_stride * (n - 1) + plane <= occ_all.size
            out = torch.full((n * out_stride,), sentinel, dtype=d_occ.dtype, device=DEV)
            _abi.check(lib.ffmp_bev_image(n, int(compact), d_occ.data_ptr(), occ_stride, d_flow.data_ptr(), plane, vmax,
                                          out.data_ptr() + ch * plane * out.element_size(), out_stride, s),
                       "ffmp_bev_image")
            got = out.cpu().numpy().reshape(n, out_stride)
            tag = f"occ stride {occ_name}, out stride {out_name} at channel {ch}"
            assert np.array_equal(got[:, ch * plane:(ch + 4) * plane].astype(np.float32), want), tag
            assert (got[:, :ch * plane] == sentinel).all() and (got[:, (ch + 4) * plane:] == sentinel).all(), tag


def _ref_images(ref, vmax, compact):
    flow = ref.flow.astype(np.float16).astype(np.float32) if compact else ref.flow
    return bev_image(ref.state_m[:, 1], flow, vmax)


BEV_ROWS = [("f32", 4), ("u8f16", 2)]


# the present cases keep their ids; the mixed-ages configs of tests/series_cases.py (flow=True) take both rows: a
# float32 image of 10000, 1296, 144 and 64 sixteen-byte vectors, a uint8 one of 2500, 324, 36 and 16
@pytest.mark.parametrize("case,fmt,window",
                         [pytest.param(None, *row, id=f"{row[0]}-{row[1]}") for row in BEV_ROWS]
                         + [pytest.param(name, *row, id=f"{name}-{row[0]}-{row[1]}")
                            for name in ("G100", "G36", "G12", "G8") for row in BEV_ROWS])
def test_bev_maps_match_reference_map_memory(case, fmt, window):
    n, steps, k = 24, 18, 3
    cfg = CFG if case is None else series_cases.config(case, flow=True)
    G = cfg.grid
    mix = series_cases.AgeMix()
    env = FFMPVec(n, cfg, device=DEV, frame_window=window, obs_format=fmt, autotune=False, bev_series=k)
    ref = OracleVecEnv(cfg, n)
    env.reset()
    ref.reset()
    stacks = {kk: [TemporalStack(kk) for _ in range(n)] for kk in (1, 2, 3)}

    def push(first):
        img = _ref_images(ref, cfg.obst_vmax, fmt == "u8f16")
        for kk, per_env in stacks.items():
            for e, st in enumerate(per_env):
                st.push(img[e], bool(first[e]))

    def check(tag):
        for kk, per_env in stacks.items():
            got = env.bev_maps(kk).cpu().numpy().astype(np.float32)
            want = np.stack([np.concatenate(st.mem, axis=0) for st in per_env])
            assert got.shape == (n, 4 * kk, G, G) and got.shape == want.shape
            bad = np.argwhere((got != want).any(axis=(2, 3)))
            assert bad.size == 0, f"{tag} k={kk}: (env, channel) mismatches {bad[:8].tolist()}"

    push(np.ones(n, bool))
    check("reset")
    rng = np.random.default_rng(4)
    resets = 0
    for s in range(steps):
        a = rng.integers(0, 28, n)
        env.step(torch.as_tensor(a, device=DEV))
        ref.step(a)
        push(ref.done)
        resets += int(ref.done.sum())
        mix.note(ref)
        check(f"step {s}")
    assert resets > n
    if case is not None:  # the envs' ages differ (tests/test_series_cases_host.py)
        mix.check(n, ref.state_m[:, 1])
    # a moving disc colours its cells: the flow channels are not constant
    img = env.bev_maps(1)
    assert int((img[:, 3] > 0).sum()) > 0 and int((img[:, 1] != 128).sum()) > 0
    with pytest.raises(ValueError):
        env.bev_maps(4)


def test_bev_maps_errors_and_reload():
    with pytest.raises(ValueError, match="flow=True"):
        FFMPVec(4, CFG.replace(flow=False), device=DEV, bev_series=3)
    env = FFMPVec(8, CFG, device=DEV, autotune=False, bev_series=3)
    with pytest.raises(RuntimeError, match="reset"):
        env.bev_maps(3)
    env.reset()
    for _ in range(2):
        env.step(torch.zeros(8, dtype=torch.int64, device=DEV))
    sd = env.state_dict()
    env2 = FFMPVec(8, CFG, device=DEV, autotune=False, bev_series=3)
    env2.load_state_dict(sd)
    assert torch.equal(env2.bev_maps(1), env.bev_maps(1))
    with pytest.raises(RuntimeError, match="known images"):
        env2.bev_maps(2)  # the older images are not part of a state_dict
    env2.step(torch.zeros(8, dtype=torch.int64, device=DEV))
    env.step(torch.zeros(8, dtype=torch.int64, device=DEV))
    assert torch.equal(env2.bev_maps(2), env.bev_maps(2))
    out = torch.empty(8, 8, 64, 64, device=DEV)
    assert env.bev_maps(2, out=out) is out
    with pytest.raises(ValueError):
        env.bev_maps(2, out=torch.empty(8, 4, 64, 64, device=DEV))


@pytest.mark.parametrize("case,obs_format",
                         [pytest.param(None, f, id=f) for f in ("f32", "u8f16")]
                         + [pytest.param(name, f, id=f"{name}-{f}") for name in ("G100", "G12") for f in ("f32", "u8f16")])
def test_replay_bev_series_reproduces_the_env(case, obs_format):
    """ReplayMemory(series=3, bev=True): the state series re-rastered and coloured from the stored
    records equals env.bev_maps(3) before the step; the observation series equals it after the step,
    or for an env that reset, the state series slid by one with the terminal image appended.  In the
    compact layout the env colours binary16 flow planes, and so must the replay.  G100 / G12: the
    mixed-ages configs of tests/series_cases.py, where the stored steps-since-reset differ across the envs of a
    step."""
    cfg = FFMPConfig(grid=64, n_obst=12, n_beams=32, moving=True, max_steps=5, obst_rmax=0.5, obst_vmax=1.2,
                     world_half=2.4, goal_min=0.6, goal_max=1.5, flow=True, seed=23)
    if case is not None:
        cfg = series_cases.config(case, flow=True)
    G = cfg.grid
    N, T, k = 32, 11, 3
    env = FFMPVec(N, cfg, device=DEV, keep_terminal=True, bev_series=k, obs_format=obs_format)
    mem = ReplayMemory(env, capacity=N * T, series=k, bev=True)
    env.reset()
    rng = np.random.default_rng(2)
    before, after, term, dones, ages, early = [], [], [], [], [], 0
    for _ in range(T):
        before.append(env.bev_maps(k).float())
        ages.append(env.t.clone())
        mem.push_begin()
        a = torch.as_tensor(rng.integers(0, 28, N), device=DEV)
        env.step(a)
        mem.push_end(a)
        after.append(env.bev_maps(k).float())
        term.append(env.term_record.clone())
        dones.append(env.done.clone())
        early += int((env.done & ~env.truncated).sum())
    done_all = torch.cat(dones)
    assert 0 < int(done_all.sum()) < N * T
    # s_since is the state's steps since reset, clamped to the k - 1 records kept and to the steps pushed
    seen = torch.arange(T, device=DEV).repeat_interleave(N)
    assert torch.equal(mem.s_since.long(), torch.minimum(torch.cat(ages).long(), seen).clamp(max=k - 1))
    if case is not None:
        assert torch.cat(ages).unique().numel() >= series_cases.MIN_AGES and early >= N
        assert mem.s_since[-N:].unique().tolist() == list(range(k))  # every clamp among the envs of one step
    tr, ex = mem.sample(0, index=torch.arange(N * T, device=DEV), potential=True)
    assert tr.state_m.shape == (N * T, 4 * k, G, G) and "flow" not in ex
    s_want = torch.cat(before)
    assert torch.equal(tr.state_m, s_want)
    nd = ~done_all
    assert torch.equal(tr.observe_m[nd], torch.cat(after)[nd])
    assert torch.equal(tr.observe_m[done_all][:, :-4], s_want[done_all][:, 4:])
    oc = Cfg.from_config(cfg)
    sm, _, flow = raster(oc, Record.unpack(torch.cat(term)[done_all].cpu().numpy(), cfg.n_obst), False)
    if obs_format == "u8f16":
        flow = flow.astype(np.float16).astype(np.float32)
    newest = bev_image(sm[:, 1], flow, cfg.obst_vmax)
    assert np.array_equal(tr.observe_m[done_all][:, -4:].cpu().numpy(), newest)
    mem2 = ReplayMemory(env, capacity=N * T, series=k, bev=True)
    mem2.load_state_dict(mem.state_dict())
    tr2, _ = mem2.sample(0, index=torch.arange(N * T, device=DEV))
    assert torch.equal(tr2.state_m, tr.state_m) and torch.equal(tr2.observe_m, tr.observe_m)
    with pytest.raises(ValueError):
        ReplayMemory(env, capacity=N * T, series=k).load_state_dict(mem.state_dict())


@pytest.mark.parametrize("amp", [False, True])
def test_brain_twelve_channels_updates(amp):
    from flow_field_based_motion_planner_amd.learner import Brain
    cfg = FFMPConfig(grid=100, n_obst=6, n_beams=0, moving=True, max_steps=20, flow=True, seed=41)
    n = 16
    env = FFMPVec(n, cfg, device=DEV, keep_terminal=True, bev_series=3, autotune=False)
    brain = Brain(env, capacity=256, batch_size=32, input_channels=12, amp=amp, seed=3)
    assert brain.main_q_network.conv1.in_channels == 12 and brain.memory.bev
    obs = env.reset()
    losses = []
    for _ in range(4):
        a = brain.decide_action(obs, env.episode)
        assert a.shape == (n,)
        brain.memory.push_begin()
        obs, _, _, _ = env.step(a)
        brain.memory.push_end(a)
        loss = brain.replay()
        if loss is not None:
            losses.append(float(loss))
    assert losses and all(np.isfinite(losses))
    with pytest.raises(ValueError, match="bev_series"):
        Brain(FFMPVec(n, cfg, device=DEV, keep_terminal=True, autotune=False), input_channels=12)


def test_bev_ring_counts_against_the_hbm_budget():
    """the BEV image ring is an arena buffer — a budget that holds the planes but not the
    ring is refused at construction, and an instance built within a budget holds the ring inside it."""
    cfg = FFMPConfig(grid=64, n_obst=4, n_beams=0, moving=True, max_steps=20, flow=True, seed=3)
    N, k = 4096, 3
    ring = k * N * 4 * 64 * 64 * 4  # 768 MiB
    planes = N * 64 * 64 * 4 * (2 + 1 + 2)  # frames (W = 2), potential, flow: 320 MiB
    with pytest.raises(ValueError):
        FFMPVec(N, cfg, device=DEV, bev_series=k, hbm_budget=planes + ring // 2, autotune=False)
    env = FFMPVec(N, cfg, device=DEV, bev_series=k, hbm_budget=planes + ring + (64 << 20), autotune=False)
    assert env.hbm_bytes() <= planes + ring + (64 << 20)
    a0 = env._arena_buf.data_ptr()
    assert a0 <= env.bev.data_ptr() < a0 + env._arena_buf.numel()
    env.reset()
    env.step(torch.zeros(N, dtype=torch.int64, device=DEV))
    assert env.bev_maps(k).shape == (N, 4 * k, 64, 64)
    env.close()
