"""The kernels at physical constants off their defaults (tests/physics_cases.py), against the NumPy
oracle and the restatements, which take every constant from the config:

a. the step in every launch form against the oracle, step by step (tests/parity_util.py's
   tolerances, unchanged), the float32 forms bit-identical to each other, the tag invariant, the
   oracle's event counts from the GPU's flags, the tile shapes of the two-launch raster at the
   least cull margin;
b. visible_frames, lidar_frames, lidar_map, lidar_flow, nav_field / policy_nav, policy_field and
   policy_reactive against their restatements, bit for bit, after 3 and after 8 steps;
c. ReplayMemory, which builds its own ffmp_cfg_t, re-rasters what the env showed.

Every FFMPVec is built with autotune=False."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from flow_field_based_motion_planner_amd import _abi
from flow_field_based_motion_planner_amd.replay import ReplayMemory
from flow_field_based_motion_planner_amd.vec_env import FFMPVec
from oracle.ffmp_oracle import OracleVecEnv
from tests import nav_field_ref as R
from tests import scan_map_ref as S
from tests import visible_ref as V
from tests.parity_util import compare, gpu_snapshot, oracle_snapshot, policy_reactive_np
from tests.physics_cases import PHYSICS, SCALES, actions, check_floors, count_events
from tests.test_gpu_lidar_map import RefMap
from tests.test_gpu_lidar_map import _check as _check_map
from tests.test_gpu_nav_field import _assert_same as _same_nav
from tests.test_gpu_nav_field import _expect as _expect_nav
from tests.test_gpu_nav_field import _gpu as _gpu_nav
from tests.test_gpu_scan_flow import LiveRef
from tests.test_gpu_scan_flow import _check as _check_flow
from tests.test_gpu_scan_map import _same as _same_frames
from tests.test_gpu_sparse_frames import _invariant

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INF = float("inf")

TILED = _abi.RASTER_NT | _abi.RASTER_TILE4
FORMS = {
    # name: (FFMPVec arguments, fused flags)
    "two_launch": (dict(fused=False, frame_window=4), None),
    "fused": (dict(fused=True, frame_window=4), TILED),
    "fused_waves": (dict(fused=True, frame_window=4), TILED | _abi.RASTER_WAVES),
    "dense": (dict(fused=False, frame_window=4, sparse_frames=False), None),
    "no_potential": (dict(fused=False, frame_window=4, potential=False), None),
    "u8f16": (dict(fused=False, frame_window=4, obs_format="u8f16"), None),
}
F32_FORMS = ("two_launch", "fused", "fused_waves", "dense")
STEP_PARAMS = [(name, form) for name in PHYSICS for form in FORMS if name != "dt0" or form == "two_launch"]

_ORACLE = {}


def _oracle(name):
    """(snapshots after the reset and after every step, event counts) of the NumPy oracle on a case:
    computed once, kept for the case's forms (one case at a time), never written."""
    if name not in _ORACLE:
        _ORACLE.clear()
        cfg, n, steps = PHYSICS[name]
        ref = OracleVecEnv(cfg, n)
        ref.reset()
        snaps, counts = [copy.deepcopy(oracle_snapshot(ref))], {}
        for a in actions(n, steps):
            ref.step(a)
            snaps.append(copy.deepcopy(oracle_snapshot(ref)))
            count_events(counts, ref.done, ref.collision, ref.is_goal, ref.truncated, ref.lidar if cfg.n_beams else None)
        _ORACLE[name] = (snaps, counts)
    return _ORACLE[name]


def _env(name, form):
    cfg, n, _ = PHYSICS[name]
    kw, flags = FORMS[form]
    env = FFMPVec(n, cfg, device=DEV, autotune=False, keep_terminal=True, **kw)
    if flags is not None:
        env.fused_flags = flags
    return env


def _kernel_waves(env):
    return env.lib.ffmp_raster_waves(C.byref(env._cfg_c), C.cast(C.byref(env._obs_c), C.POINTER(_abi.ObsT)), env.fused_flags)


def _half_bits(a):
    return np.ascontiguousarray(a).view(np.uint16)


def _compare(form, g, o, where):
    """The mismatches of one snapshot against the oracle's, by the form's rule."""
    if form == "no_potential":  # frames and flow only
        bad = [] if np.array_equal(g["state_m"], o["state_m"]) else [f"{where} state_m differs"]
        if o["flow"] is not None and not np.array_equal(g["flow"], o["flow"]):
            bad.append(f"{where} flow differs")
        return bad
    if form == "u8f16":  # as test_gpu_compact.py::test_compact_vs_oracle: uint8 frames, the planes rounded to binary16
        bad = []
        if g["state_m"].dtype != np.uint8 or not np.array_equal(g["state_m"], o["state_m"].astype(np.uint8)):
            bad.append(f"{where} state_m (uint8) differs")
        if not np.array_equal(_half_bits(g["potential"]), _half_bits(o["potential"].astype(np.float16))):
            bad.append(f"{where} potential (binary16) differs")
        if o["flow"] is not None and not np.array_equal(_half_bits(g["flow"]), _half_bits(o["flow"].astype(np.float16))):
            bad.append(f"{where} flow (binary16) differs")
        g = dict(g, state_m=o["state_m"], potential=None, flow=o["flow"])
        return bad + compare(g, o, where)
    return compare(g, o, where)


# ------------------------------------------------------------------ a. the step in every launch form
@pytest.mark.parametrize("name,form", STEP_PARAMS)
def test_step_parity(name, form):
    """Step by step against the oracle.  The float32 observations are held to the absolute 1e-5 of
    tests/parity_util.py at every scale, `metres` (goal distances of tens of metres) included."""
    cfg, n, steps = PHYSICS[name]
    snaps, want = _oracle(name)
    env = _env(name, form)
    assert env.fused == FORMS[form][0]["fused"] and env.frame_window == 4
    tagged = env.frame_tags is not None
    assert tagged == (form not in ("dense", "u8f16"))
    if form == "fused_waves":  # the 6-waves kernel applies to tagged float32 frames without flow planes
        assert _kernel_waves(env) == (0 if cfg.flow else 6)
    elif form == "fused":
        assert _kernel_waves(env) == 0
    env.reset()
    torch.cuda.synchronize()
    problems = _compare(form, gpu_snapshot(env), snaps[0], "reset")
    counts = {}
    for s, a in enumerate(actions(n, steps)):
        env.step(torch.as_tensor(a, device=DEV))
        torch.cuda.synchronize()
        g = gpu_snapshot(env)
        problems += _compare(form, g, snaps[s + 1], f"step {s}")
        count_events(counts, g["done"], g["collision"], g["is_goal"], g["truncated"], g["lidar"])
        if tagged and s % 4 == 3:
            _invariant(env, (name, form, s))
    assert not problems, "\n".join(problems[:20])
    print(name, form, counts)
    assert counts == want, (counts, want)  # the oracle's events, from the GPU's flags
    check_floors(name, counts)
    if name == "dt0":
        assert counts["truncated"] == n and counts["collision"] == 0  # nothing moves: every episode runs out
    env.check_errors()
    env.close()


@pytest.mark.parametrize("name", [k for k in PHYSICS if k != "dt0"])
def test_float32_forms_identical(name):
    """Every float32 form writes the same planes, record, small observations and flags, torch.equal."""
    cfg, n, steps = PHYSICS[name]
    keys = ("state_m", "potential", "flow", "record", "state_g", "state_v", "state_t", "grad", "lidar", "reward", "done",
            "is_goal", "collision", "truncated", "t", "episode", "term_record", "term_obs")
    acts = torch.as_tensor(actions(n, steps), device=DEV)
    want = None
    for form in F32_FORMS:
        env = _env(name, form)
        env.reset()
        got = []
        for s in range(steps):
            env.step(acts[s])
            got.append({k: getattr(env, k).clone() for k in keys if getattr(env, k) is not None})
        if want is None:
            want = got
            assert "potential" in got[0] and ("flow" in got[0]) == bool(cfg.flow) and ("lidar" in got[0]) == (cfg.n_beams > 0)
        for s in range(steps):
            assert got[s].keys() == want[s].keys()
            for k in want[s]:
                a, b = got[s][k], want[s][k]
                if a.is_floating_point():  # NaN-safe: a term_obs no episode has filled yet
                    assert torch.equal(a.isnan(), b.isnan()), (form, s, k)
                    a, b = a.nan_to_num(nan=0.0, posinf=INF, neginf=-INF), b.nan_to_num(nan=0.0, posinf=INF, neginf=-INF)
                assert torch.equal(a, b), (form, s, k)
        env.close()


def test_thin_margin_tile_shapes():
    """The column-band cull of the two-launch raster at the least cull margin, with flow planes: the
    2-D tile shapes against the oracle (frames and flow bit for bit, the potential to its tolerance)."""
    name = "thin_margin"
    cfg, n, steps = PHYSICS[name]
    assert cfg.flow and cfg.cull_margin == cfg.cull_floor()
    snaps, _ = _oracle(name)
    for shape in ((2048, _abi.RASTER_TILE2), (4096, _abi.RASTER_TILE4 | _abi.RASTER_XCD), (4096, _abi.RASTER_TILE8)):
        env = FFMPVec(n, cfg, device=DEV, autotune=False, keep_terminal=True, fused=False, frame_window=4)
        env.raster_shape = env.raster_shape_newest = shape
        env.reset()
        problems = compare(gpu_snapshot(env), snaps[0], "reset")
        for s, a in enumerate(actions(n, steps)):
            env.step(torch.as_tensor(a, device=DEV))
            torch.cuda.synchronize()
            problems += compare(gpu_snapshot(env), snaps[s + 1], f"step {s}")
        assert not problems, (shape, problems[:10])
        _invariant(env, shape)
        env.close()


# ------------------------------------------------------------------ b. sensors, planners and policies
def _walk(name, marks=(3, 8), **kw):
    """The case's env, yielded after each step in `marks` of the case's actions: (env, step)."""
    cfg, n, _ = PHYSICS[name]
    env = FFMPVec(n, cfg, device=DEV, autotune=False, **kw)
    env.reset()
    for s, a in enumerate(actions(n, max(marks)), start=1):
        env.step(torch.as_tensor(a, device=DEV))
        if s in marks:
            yield env, s
    env.check_errors()
    env.close()


@pytest.mark.parametrize("name", list(SCALES))
def test_visible_frames(name):
    for env, s in _walk(name):
        rec = env.record.cpu().numpy()
        for mr in (None, 0.6 * env.cfg.lidar_range):
            exp = V.from_packed(env.cfg, rec, 128, INF if mr is None else mr)
            _same_frames(env.visible_frames(max_range=mr), exp, env, (name, s, mr))
        if s == 8:
            assert (exp == 128).any() and (exp == 255).any()


@pytest.mark.parametrize("name", list(SCALES))
def test_lidar_frames(name):
    """thickness = res and range_max = lidar_range, the defaults.  `coarse` and `metres`: the range ends
    inside the plane; `fine`: most hits lie beyond it."""
    for env, s in _walk(name):
        exp = S.from_config(env.cfg, env.lidar.cpu().numpy())
        got = env.lidar_frames()
        _same_frames(got[:, 1], exp, env, (name, s))
        assert torch.equal(got[:, 0], got[:, 1])
        _same_frames(env.lidar_frames(newest_only=True, plain=True), exp, env, (name, s, "plain"))
        assert all((exp == v).any() for v in (0, 128, 255)), (name, s)


@pytest.mark.parametrize("name", list(SCALES))
def test_lidar_map(name):
    """Four consecutive updates (after steps 3..6) and one that spans two steps (after step 8): both
    log-odds planes and the frame."""
    m = ref = None
    for env, s in _walk(name, marks=(3, 4, 5, 6, 8)):
        if m is None:
            m, ref = env.lidar_map(), RefMap(env)
        before = ref.m
        ref.update()
        assert m.update() is m.frame
        _check_map(m, ref, (name, s), before)
    assert (ref.frame == 255).any() and (ref.frame == 0).any()


@pytest.mark.parametrize("name", list(SCALES))
def test_lidar_flow(name):
    """lag = 1: one quantum is res / dt m/s.  Updates after steps 3..6 and after step 8."""
    q = SCALES[name]["quantum"]
    m = live = None
    estimated = 0
    for env, s in _walk(name, marks=(3, 4, 5, 6, 8)):
        if m is None:
            m, live = env.lidar_flow(lag=1), LiveRef(env, lag=1)
            assert m.scale == q
        live.update()
        assert m.update() is m.flow
        _check_flow(m, live.ref, (name, s))
        steps_of_q = live.ref.flow.astype(np.float64) / q
        assert np.array_equal(steps_of_q, np.rint(steps_of_q)) and np.abs(steps_of_q).max() <= 4
        estimated += int((live.ref.kind != 0).sum())
    assert estimated > 0


@pytest.mark.parametrize("name", list(SCALES))
def test_nav_field_and_followers(name):
    """nav_field's planes, target and cost, policy_nav's commands (they divide by dt) and
    policy_field's, bit for bit."""
    moving = 0
    for env, s in _walk(name):
        got = _gpu_nav(env)
        _same_nav(got, _expect_nav(env), (name, s))
        moving += int((got["cmd"] != 0).any(axis=1).sum())
        c = env.policy_field().cpu().numpy()
        exp = R._field_np(env.grad.cpu().numpy(), env.cfg.dt)
        assert np.array_equal(c.view(np.int64), exp.view(np.int64)), (name, s)
        assert np.isfinite(c).all() and (c != 0).any()
    assert moving > 0


@pytest.mark.parametrize("name", list(SCALES))
def test_policy_reactive(name):
    """As test_gpu_closed_loop.py::test_policy_reactive_matches_restatement drives it: the policy's own
    actions, every third step the case's random ones, over the case's steps.  On the NumPy oracle this
    walk blocks 42 / 245 / 2 / 43 times in the four cases (`metres`: the ray is the one cell just
    outside a 2.6-cell footprint, so a disc is rarely on it without a collision)."""
    cfg, n, steps = PHYSICS[name]
    assert min(3 + int(round(0.25 / cfg.res)), cfg.grid // 2 - 1) == SCALES[name]["lookahead"]
    env = FFMPVec(n, cfg, device=DEV, autotune=False)
    env.reset()
    blocked = 0
    for s, rand in enumerate(actions(n, steps)):
        a = env.policy_reactive()
        exp = policy_reactive_np(cfg, env.state_m[:, 1].cpu().numpy(), env.state_g.cpu().numpy())
        assert np.array_equal(a.cpu().numpy(), exp), (name, s)
        blocked += int((exp // 7 == 0).sum())
        env.step(torch.as_tensor(rand, device=DEV) if s % 3 == 2 else a)
    assert blocked > 0  # some env has taken the blocked branch
    env.check_errors()
    env.close()


def test_dt_zero_refused_where_it_divides():
    cfg, n, _ = PHYSICS["dt0"]
    env = FFMPVec(n, cfg, device=DEV, autotune=False)
    env.reset()
    env.step(torch.zeros(n, dtype=torch.int64, device=DEV))
    for call in (env.policy_field, env.policy_nav, lambda: env.lidar_flow(lag=1)):
        with pytest.raises(ValueError, match="dt"):
            call()
    d = env.nav_field(cost=True)  # the planes need no dt
    assert int((d["geo_cost"] >= 0).sum()) > 0
    env.policy_reactive()
    env.check_errors()
    env.close()


# ------------------------------------------------------------------ c. replay
def test_replay_reproduces_env_observations():
    """ReplayMemory builds its own ffmp_cfg_t from the env's config: sample(index=arange) gives back
    state_m, the potential and the not-done observe_m bit for bit
    (test_gpu_replay.py::test_sample_reproduces_env_observations, at the `coarse` constants)."""
    cfg, N, _ = PHYSICS["coarse"]
    T = 9
    env = FFMPVec(N, cfg, device=DEV, autotune=False, keep_terminal=True)
    mem = ReplayMemory(env, capacity=N * T)
    env.reset()
    before, after, dones = [], [], []
    for a in actions(N, T):
        before.append((env.state_m.clone(), env.potential.clone()))
        mem.push_begin()
        a = torch.as_tensor(a, device=DEV)
        env.step(a)
        mem.push_end(a)
        after.append((env.state_m.clone(), env.potential.clone()))
        dones.append(env.done.clone())
    done_all = torch.cat(dones)
    assert 0 < int(done_all.sum()) < N * T
    tr, ex = mem.sample(0, index=torch.arange(N * T, device=DEV), potential=True)
    assert torch.equal(tr.state_m, torch.cat([b[0] for b in before]))
    assert torch.equal(ex["potential"], torch.cat([b[1] for b in before]))
    nd = ~done_all
    assert torch.equal(tr.observe_m[nd], torch.cat([a_[0] for a_ in after])[nd])
    assert torch.equal(ex["observe_potential"][nd], torch.cat([a_[1] for a_ in after])[nd])
    assert torch.equal(ex["done"], done_all)
    assert bool((tr.state_m > 0).any())
    env.close()
