"""Device replay memory (replay.py): what sample() materialises is bit-identical to what the env
emitted (state before the step, observation after it — the terminal one for envs that reset),
and the ring follows the reference ReplayMemory's push / len / sample semantics
(src/train.py:212-228).

The cases named G100 / G12 run the mixed-ages configs of tests/series_cases.py: the envs of one step differ in
their steps since reset, so a memory that stored s_since (or a history record) of the wrong slot shows."""
import numpy as np
import pytest
import torch

from flow_field_based_motion_planner_amd import FFMPConfig
from flow_field_based_motion_planner_amd.replay import ReplayMemory, Transition
from flow_field_based_motion_planner_amd.vec_env import FFMPVec
from oracle.ffmp_oracle import Cfg, Record, bev_image, raster
from tests import series_cases

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


class _RefRing:
    """src/train.py:212-228 ReplayMemory.push / __len__, restated over transition ids."""

    def __init__(self, capacity):
        self.capacity, self.memory, self.index = capacity, [], 0

    def push(self, item):
        if len(self.memory) < self.capacity:
            self.memory.append(None)
        self.memory[self.index] = item
        self.index = (self.index + 1) % self.capacity


def _snap(env):
    return {"state_m": env.state_m.clone(), "small": torch.cat([env.state_g, env.state_v, env.state_t], 1).clone(),
            "potential": env.potential.clone() if env.potential is not None else None,
            "flow": env.flow.clone() if env.flow is not None else None, "record": env.record.clone()}


def _cases(values):
    """The present cases under their ids, then G100 and G12 of tests/series_cases.py for each of them."""
    return ([pytest.param(None, v, id=str(v)) for v in values]
            + [pytest.param(name, v, id=f"{name}-{v}") for name in ("G100", "G12") for v in values])


@pytest.mark.parametrize("case,flow", _cases([False, True]))
def test_sample_reproduces_env_observations(case, flow):
    cfg = FFMPConfig(grid=64, n_obst=12, n_beams=32, moving=True, max_steps=5, obst_rmax=0.5, obst_vmax=1.2,
                     world_half=2.4, goal_min=0.6, goal_max=1.5, flow=flow, seed=21)
    N, T = 48, 9
    if case is not None:  # 12 steps: at least N episodes end by a collision or a goal (test_series_cases_host.py)
        cfg, T = series_cases.config(case, flow), 12
    G = cfg.grid
    env = FFMPVec(N, cfg, device=DEV, keep_terminal=True)
    mem = ReplayMemory(env, capacity=N * T)
    env.reset()
    rng = np.random.default_rng(0)
    before, after, term, dones, ages, early = [], [], [], [], [], 0
    for _ in range(T):
        before.append(_snap(env))
        ages.append(env.t.clone())
        mem.push_begin()
        a = torch.as_tensor(rng.integers(0, 28, N), device=DEV)
        env.step(a)
        mem.push_end(a)
        after.append(_snap(env))
        term.append((env.term_record.clone(), env.term_obs.clone()))
        dones.append(env.done.clone())
        early += int((env.done & ~env.truncated).sum())
    assert len(mem) == N * T
    done_all = torch.cat(dones)
    assert 0 < int(done_all.sum()) < N * T  # both kinds of transition are present
    if case is not None:  # the pair keeps no s_since: the ages of the stored states themselves
        assert torch.cat(ages).unique().numel() >= series_cases.MIN_AGES and early >= N, (early, N)
    idx = torch.arange(N * T, device=DEV)
    tr, ex = mem.sample(0, index=idx, potential=True)
    assert isinstance(tr, Transition) and tr.state_m.shape == (N * T, 2, G, G)
    assert tr.action.shape == (N * T, 1) and tr.reward.shape == (N * T,)
    assert torch.equal(tr.state_m, torch.cat([b["state_m"] for b in before]))
    assert torch.equal(ex["potential"], torch.cat([b["potential"] for b in before]))
    s_small = torch.cat([tr.state_g, tr.state_v, tr.state_t], 1)
    assert torch.equal(s_small, torch.cat([b["small"] for b in before]))
    o_small = torch.cat([tr.observe_g, tr.observe_v, tr.observe_t], 1)
    assert torch.equal(o_small, torch.cat([t[1] for t in term]))
    if flow:
        assert torch.equal(ex["flow"], torch.cat([b["flow"] for b in before]))
    # not-done transitions: observation == what the env returned after the step
    nd = ~done_all
    assert torch.equal(tr.observe_m[nd], torch.cat([a_["state_m"] for a_ in after])[nd])
    assert torch.equal(ex["observe_potential"][nd], torch.cat([a_["potential"] for a_ in after])[nd])
    assert torch.equal(o_small[nd], torch.cat([a_["small"] for a_ in after])[nd])
    assert torch.equal(ex["done"], done_all)
    # done transitions: the terminal frame (the oracle raster of the terminal record), not the reset one
    oc = Cfg.from_config(cfg)
    recs = torch.cat([t[0] for t in term])[done_all].cpu().numpy()
    sm_ref = raster(oc, Record.unpack(recs, cfg.n_obst), False)[0]
    got = tr.observe_m[done_all].cpu().numpy()
    assert np.array_equal(got, sm_ref)
    reset_frames = torch.cat([a_["state_m"] for a_ in after])[done_all].cpu().numpy()
    assert not np.array_equal(got, reset_frames)


def test_ring_semantics_and_sampling():
    cfg = FFMPConfig(grid=32, n_obst=4, n_beams=0, moving=True, max_steps=4, seed=22)
    N, cap, T = 16, 100, 10
    env = FFMPVec(N, cfg, device=DEV, keep_terminal=True)
    mem = ReplayMemory(env, capacity=cap, seed=5)
    ref = _RefRing(cap)
    env.reset()
    rng = np.random.default_rng(1)
    recs, acts = {}, {}
    for s in range(T):
        rec_before = env.record.clone()
        mem.push_begin()
        a = rng.integers(0, 28, N)
        env.step(torch.as_tensor(a, device=DEV))
        mem.push_end(torch.as_tensor(a, device=DEV))
        for e in range(N):
            ref.push((s, e))
            recs[(s, e)], acts[(s, e)] = rec_before[e], int(a[e])
        assert len(mem) == len(ref.memory) and mem.index == ref.index
    for slot, key in enumerate(ref.memory):
        assert torch.equal(mem.s_record[slot], recs[key]), slot
        assert int(mem.action[slot]) == acts[key]
    idx = mem.sample_indices(64)
    assert idx.unique().numel() == 64 and int(idx.max()) < cap
    assert mem.sample_indices(500, replacement=True).numel() == 500
    with pytest.raises(ValueError):
        mem.sample_indices(cap + 1)
    tr, ex = mem.sample(32)
    assert tr.state_m.shape == (32, 2, 32, 32) and ex["index"].unique().numel() == 32
    sd = mem.state_dict()
    mem2 = ReplayMemory(env, capacity=cap)
    mem2.load_state_dict(sd)
    tr2, _ = mem2.sample(32, index=ex["index"])
    assert torch.equal(tr2.state_m, tr.state_m) and torch.equal(tr2.observe_m, tr.observe_m)
    with pytest.raises(ValueError):
        ReplayMemory(FFMPVec(N, cfg, device=DEV), capacity=cap)  # needs keep_terminal
    with pytest.raises(RuntimeError):
        mem.push_end(torch.zeros(N, dtype=torch.int64, device=DEV))


def _run_series(cfg, N, T, k, obs_format="f32", capacity=None, bev=False, seed=2):
    """Step an env T times through a ReplayMemory(series=k).  Returns (env, mem, before, after, term, dones, ages,
    early): the env's series before and after every step (float32), the terminal records, the done flags, the
    ages of the stored states and the number of episodes that ended by something other than the truncation."""
    env = FFMPVec(N, cfg, device=DEV, keep_terminal=True, obs_format=obs_format,
                  **(dict(bev_series=k) if bev else dict(frame_window=k + 1)))
    mem = ReplayMemory(env, capacity=N * T if capacity is None else capacity, series=k, bev=bev)
    series = lambda: (env.bev_maps(k) if bev else env.temporal_maps(k)).to(torch.float32, copy=True)  # noqa: E731
    env.reset()
    rng = np.random.default_rng(seed)
    before, after, term, dones, ages, early = [], [], [], [], [], 0
    for _ in range(T):
        before.append(series())
        ages.append(env.t.clone())
        mem.push_begin()
        a = torch.as_tensor(rng.integers(0, 28, N), device=DEV)
        env.step(a)
        mem.push_end(a)
        after.append(series())
        term.append(env.term_record.clone())
        dones.append(env.done.clone())
        early += int((env.done & ~env.truncated).sum())
    return env, mem, before, after, term, dones, ages, early


def _check_since(mem, ages, N, T, H, mixed):
    """s_since of every slot of an unwrapped ring: the state's steps since reset, clamped to the H records kept and
    to the steps pushed before it.  (The clamp leaves H + 1 values, so "at least 4 distinct" is asked of the ages
    themselves, and of s_since that the envs of one step take every value it can hold.)"""
    seen = torch.arange(T, device=DEV).repeat_interleave(N)
    assert torch.equal(mem.s_since.long(), torch.minimum(torch.cat(ages).long(), seen).clamp(max=H))
    if mixed:
        assert torch.cat(ages).unique().numel() >= series_cases.MIN_AGES
        assert mem.s_since[-N:].unique().tolist() == list(range(H + 1))


def _check_series(cfg, mem, N, T, k, before, after, term, dones):
    G = cfg.grid
    done_all = torch.cat(dones)
    assert 0 < int(done_all.sum()) < N * T
    tr, ex = mem.sample(0, index=torch.arange(N * T, device=DEV), potential=True)
    assert tr.state_m.shape == (N * T, k, G, G) and tr.state_m.dtype == torch.float32
    s_want = torch.cat(before)
    assert torch.equal(tr.state_m, s_want)
    nd = ~done_all
    assert torch.equal(tr.observe_m[nd], torch.cat(after)[nd])
    assert torch.equal(tr.observe_m[done_all][:, :-1], s_want[done_all][:, 1:])
    oc = Cfg.from_config(cfg)
    recs = torch.cat(term)[done_all].cpu().numpy()
    newest = raster(oc, Record.unpack(recs, cfg.n_obst), False)[0][:, 1]
    assert np.array_equal(tr.observe_m[done_all][:, -1].cpu().numpy(), newest)
    return tr


@pytest.mark.parametrize("case,k", _cases([3, 4]))
def test_series_sample_reproduces_temporal_maps(case, k):
    """ReplayMemory(series=k): the k-frame state series re-rastered from the stored records equals
    env.temporal_maps(k) before the step; the observation series equals it after the step, or for
    an env that reset, the state series slid by one with the terminal frame appended (the reference
    appends the observed frame to map_memory; is_first refills it only on the next iteration)."""
    cfg = FFMPConfig(grid=64, n_obst=12, n_beams=32, moving=True, max_steps=5, obst_rmax=0.5, obst_vmax=1.2,
                     world_half=2.4, goal_min=0.6, goal_max=1.5, seed=23)
    if case is not None:
        cfg = series_cases.config(case)
    N, T = 32, 11
    env, mem, before, after, term, dones, ages, early = _run_series(cfg, N, T, k)
    _check_since(mem, ages, N, T, k - 2, case is not None)
    assert case is None or early >= N, (early, N)
    tr = _check_series(cfg, mem, N, T, k, before, after, term, dones)
    sd = mem.state_dict()
    mem2 = ReplayMemory(env, capacity=N * T, series=k)
    mem2.load_state_dict(sd)
    tr2, _ = mem2.sample(0, index=torch.arange(N * T, device=DEV))
    assert torch.equal(tr2.state_m, tr.state_m) and torch.equal(tr2.observe_m, tr.observe_m)


@pytest.mark.parametrize("case", ["G100", "G12"])
def test_series_sample_from_a_compact_env(case):
    """A u8f16 env, mono series k = 3: the replay rasters float32 frames, and they equal the env's uint8 series
    (temporal_maps(3).float()) at mixed ages."""
    cfg, N, T, k = series_cases.config(case), 32, 11, 3
    env, mem, before, after, term, dones, ages, early = _run_series(cfg, N, T, k, obs_format="u8f16")
    assert env.temporal_maps(k).dtype == torch.uint8
    _check_since(mem, ages, N, T, k - 2, True)
    assert early >= N, (early, N)
    _check_series(cfg, mem, N, T, k, before, after, term, dones)


@pytest.mark.parametrize("k,bev", [(4, False), (3, True)])
def test_series_ring_wraps_mid_step(k, bev):
    """capacity = 5 N + 7, 9 steps: the ring wraps inside a step (the split copy of s_hist and s_since in
    push_begin, of the rest in push_end), and later steps overwrite the oldest.  Every live slot's state and
    observation series equal what the env emitted for the (step, env) the reference ring keeps there; so do they
    after a state_dict round trip.  Then odd batches: 37 indices drawn with replacement, and one index, each row
    equal to the row of the full sample at that index."""
    cfg = series_cases.config("G12", flow=bev)
    G, N, T = cfg.grid, 24, 9
    cap = 5 * N + 7
    env, mem, before, after, term, dones, ages, early = _run_series(cfg, N, T, k, capacity=cap, bev=bev, seed=6)
    assert early >= N and torch.cat(ages).unique().numel() >= series_cases.MIN_AGES
    ref = _RefRing(cap)
    for s_ in range(T):
        for e in range(N):
            ref.push((s_, e))
    assert len(mem) == len(ref.memory) == cap and mem.index == ref.index == (N * T) % cap
    # the step that straddles the end of the ring
    assert ref.memory[cap - 1] == (5, 6) and ref.memory[0] == (5, 7)
    st = torch.tensor([key[0] for key in ref.memory], device=DEV)
    en = torch.tensor([key[1] for key in ref.memory], device=DEV)
    flat = st * N + en
    H = k - 1 if bev else k - 2
    assert torch.equal(mem.s_since.long(), torch.minimum(torch.cat(ages).long()[flat], st).clamp(max=H))
    s_want, o_after, done = torch.cat(before)[flat], torch.cat(after)[flat], torch.cat(dones)[flat]
    assert 0 < int(done.sum()) < cap
    c = 4 if bev else 1  # channels per step of the series
    out = raster(Cfg.from_config(cfg), Record.unpack(torch.cat(term)[flat][done].cpu().numpy(), cfg.n_obst), False)
    newest = bev_image(out[0][:, 1], out[2], cfg.obst_vmax) if bev else out[0][:, 1:2]

    def check(m):
        tr, ex = m.sample(0, index=torch.arange(cap, device=DEV))
        assert tr.state_m.shape == (cap, c * k, G, G)
        bad = (tr.state_m != s_want).flatten(1).any(1).nonzero().flatten().tolist()
        assert not bad, f"state series of slots {bad[:8]} (step, env) {[ref.memory[b] for b in bad[:8]]}"
        assert torch.equal(ex["done"], done)
        assert torch.equal(tr.observe_m[~done], o_after[~done])
        assert torch.equal(tr.observe_m[done][:, :-c], s_want[done][:, c:])
        # the terminal frame (the oracle's raster of the terminal record), not the reset one the env showed
        assert np.array_equal(tr.observe_m[done][:, -c:].cpu().numpy(), newest)
        assert not torch.equal(tr.observe_m[done][:, -c:], o_after[done][:, -c:])
        return tr.state_m.clone(), tr.observe_m.clone()

    full_s, full_o = check(mem)
    mem2 = ReplayMemory(env, capacity=cap, series=k, bev=bev)
    mem2.load_state_dict(mem.state_dict())
    assert len(mem2) == cap and mem2.index == mem.index
    s2, o2 = check(mem2)
    assert torch.equal(s2, full_s) and torch.equal(o2, full_o)
    gen = np.random.default_rng(9)
    for index in (gen.integers(0, cap, 37), np.array([cap - 1]), np.array([0])):
        assert index.size == 1 or np.unique(index).size < index.size  # drawn with replacement: duplicates
        idx = torch.as_tensor(index, device=DEV)
        tr, ex = mem.sample(0, index=idx)
        assert tr.state_m.shape == (index.size, c * k, G, G) and torch.equal(ex["index"], idx)
        assert torch.equal(tr.state_m, full_s[idx]) and torch.equal(tr.observe_m, full_o[idx])
        assert torch.equal(tr.action.flatten(), mem.action[idx]) and torch.equal(tr.reward, mem.reward[idx])
