"""The rollout planner on the GPU (include/ffmp.h ffmp_dwa) against its NumPy restatement
(tests/dwa_ref.py), every output bit for bit, blocked_at included:

1. random planes at G = 8, 64, 100 with n = 1, 3, 70 and G = 256, 260, 512 with n = 3 — cost planes with 65535
   speckle, frames with 255 blobs round the robot, flows with 0, NaN, +-inf and displacements of G cells and more —
   over the knob grid A in 1, 28, 64 x H in 1, 24, 32 x R in 0, 31, G (the whole grid for n <= 3, four corners of it
   at n = 70), the two frame and the two flow formats taking turns;
2. every cell a source (the list overflows); padded env strides and bases aligned to 4 but not 16 bytes; mask=; the
   velocity window with a NaN row; frame = flow = NULL; single outputs;
3. FFMPVec.policy_dwa on live envs in f32 and u8f16 at G = 64 and 256: detail=True against the restatement run on
   the env's own tensors, actions=True ids stepping to the state the commands step to; the single env; the errors;
4. the crossing family in closed loop: the outcomes of the CPU run, scene by scene and step by step;
5. inside a graph capture of the caller's, after one eager call."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from flow_field_based_motion_planner_amd import _abi
from flow_field_based_motion_planner_amd.config import FFMPConfig, rollout_table
from flow_field_based_motion_planner_amd.env import FFMP
from flow_field_based_motion_planner_amd.vec_env import FFMPVec
from tests import dwa_ref as D
from tests import flow_predict_ref as R
from tests import nav_field_ref as NR
from tests.scan_flow_ref import TIE

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
FORMATS = [(np.float32, np.float32), (np.uint8, np.float16), (np.float32, np.float16), (np.uint8, np.float32)]
OUTS = ("choice", "cmd", "score", "n_adm", "blocked_at")
CPS = F32(2.0)


def _t(x):
    return torch.as_tensor(np.ascontiguousarray(x), device=DEV)


def _pycfg(G):
    return FFMPConfig(grid=G, n_obst=1, n_beams=0)


def planes(G, n, seed, dense=False):
    """(cost (n, G, G) uint16, frame (n, G, G) float32 of values a uint8 frame holds too, flow (n, 2, G, G) float32):
    5 % of the cost plane 65535 with the 3 x 3 cells round the robot free in two envs of three; discs of 255 (and a few
    cells of 128) within 40 cells of the robot; flows within +-1.5 m/s with zeros, -0.0, NaN, +-inf and 3e38, 1e3
    (a displacement beyond any grid) sprinkled over them."""
    rng = np.random.default_rng(seed)
    c = G // 2
    cost = rng.integers(0, 4000, (n, G, G)).astype(np.uint16)
    cost[rng.random((n, G, G)) < 0.05] = 65535
    cost[::3, c - 1:c + 2, c - 1:c + 2] = 7
    cost[1::3, c - 1:c + 2, c - 1:c + 2] = 9
    frame = np.zeros((n, G, G), F32)
    ii, jj = np.mgrid[:G, :G]
    for e in range(n):
        for _ in range(6):
            ci, cj = c + rng.integers(-min(c, 40), min(c, 40), 2)
            r = rng.integers(0, 4)
            frame[e][(ii - ci) ** 2 + (jj - cj) ** 2 <= r * r] = 255
        frame[e][rng.random((G, G)) < 0.01] = 128
    if dense:
        frame[:] = 255
    flow = rng.uniform(-1.5, 1.5, (n, 2, G, G)).astype(F32)
    u = rng.random((n, 2, G, G))
    for lo, v in ((0.00, 0.0), (0.10, -0.0), (0.14, np.nan), (0.16, np.inf), (0.18, -np.inf), (0.20, 3e38), (0.22, 1e3)):
        flow[(u >= lo) & (u < lo + 0.02)] = v
    flow[:, :, ::7] *= 0.1  # slow rows: sources that stay near where they are
    return cost, frame, flow


def table(A, H, seed, spread=28):
    """A table of the caller's: walks of -1..2 cells per step and axis clipped to +-spread, a probe up to 7 cells from
    the endpoint (clipped too), random commands — candidate 0 stays on the robot cell."""
    rng = np.random.default_rng(seed)
    steps = rng.integers(-1, 3, (A, H, 2)) * rng.choice([-1, 1], (A, 1, 2))
    cells = np.clip(np.cumsum(steps, axis=1), -spread, spread)
    cells[0] = 0
    probe = np.clip(cells[:, -1:] + rng.integers(-7, 8, (A, 1, 2)), -spread, spread)
    return np.concatenate([cells, probe], axis=1).astype(np.int16), rng.normal(size=(A, 2))


def _same(got, exp, where):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.dtype == exp.dtype and got.shape == exp.shape, (where, got.dtype, got.shape, exp.dtype, exp.shape)
    bad = np.nonzero(got.view(np.uint64) != exp.view(np.uint64)) if got.dtype == np.float64 else np.nonzero(got != exp)
    assert not len(bad[0]), (where, len(bad[0]), [b[:5] for b in bad], got[bad][:5], exp[bad][:5])


def _poison(n, A):
    return dict(choice=torch.full((n,), -7, dtype=torch.int32, device=DEV), cmd=torch.full((n, 2), 9.5, dtype=torch.float64, device=DEV),
                score=_t(np.full(n, 77, np.uint32)), n_adm=torch.full((n,), -3, dtype=torch.int32, device=DEV),
                blocked_at=torch.full((n, A), 200, dtype=torch.uint8, device=DEV))


def _launch(lib, G, cost, frame, flow, traj, cmds, out, reach, cps=CPS, vel=None, dv_max=0.0, dw_max=0.0, mask=None, n=None):
    """ffmp_dwa over device tensors (any view whose env planes are dense) on the default stream."""
    cfg = _abi.make_cfg(_pycfg(G))
    fmt = lambda t: _abi.OBS_U8F16 if t is not None and t.dtype in (torch.uint8, torch.float16) else _abi.OBS_F32  # noqa: E731
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    A, H = traj.shape[0], traj.shape[1] - 1
    rc = lib.ffmp_dwa(C.byref(cfg), cost.shape[0] if n is None else n, cost.data_ptr(), cost.stride(0), ptr(frame),
                      0 if frame is None else frame.stride(0), fmt(frame), ptr(flow), 0 if flow is None else flow.stride(0), fmt(flow),
                      float(cps), int(reach), traj.data_ptr(), cmds.data_ptr(), A, H, ptr(vel), float(dv_max), float(dw_max), ptr(mask),
                      *[ptr(out.get(k)) for k in OUTS], None)
    assert rc == 0, lib.ffmp_last_error()
    torch.cuda.synchronize()


def _run(lib, G, cost, frame, flow, traj, cmds, reach, where, **kw):
    """One launch into poisoned outputs against the restatement; returns the restatement's outputs."""
    n = cost.shape[0]
    exp = D.dwa(cost, frame, flow, CPS, reach, traj, cmds, _pycfg(G).footprint, **kw)
    out = _poison(n, traj.shape[0])
    dev = {k: _t(v) for k, v in kw.items() if k in ("vel", "mask")}
    _launch(lib, G, _t(cost), None if frame is None else _t(frame), None if flow is None else _t(flow), _t(traj), _t(cmds), out, reach,
            dv_max=kw.get("dv_max", 0.0), dw_max=kw.get("dw_max", 0.0), **dev)
    for k in OUTS:
        _same(out[k], exp[k], (where, k))
    return exp


# ------------------------------------------------------------------ 1. random planes over the knob grid
GRID = [(A, H, Rk) for A in (1, 28, 64) for H in (1, 24, 32) for Rk in (0, 31, "G")]
CORNERS = [(64, 32, "G"), (28, 24, 31), (1, 1, 0), (64, 24, 31)]  # at n = 70: one per format pair


@pytest.mark.parametrize("G,n", [(G, n) for G in (8, 64, 100) for n in (1, 3, 70)] + [(256, 3), (260, 3), (512, 3)])
def test_random_planes_equal_the_restatement(lib, G, n):
    cost, frame, flow = planes(G, n, seed=G + n)
    spread = 28 if G >= 64 else 5  # at G = 8 most of a +-28 table is outside the grid; +-5 is on both sides of the border
    tables = {(A, H): table(A, H, seed=A * 100 + H, spread=spread) for A in (1, 28, 64) for H in (1, 24, 32)}
    cast = {}
    with np.errstate(over="ignore"):
        for ft, vt in FORMATS:
            cast[ft, vt] = (frame.astype(ft), flow.astype(vt))  # 3e38 and 1e3 * cps are inf in binary16
    met = adm = blocked = 0
    for idx, (A, H, Rk) in enumerate(GRID if n <= 3 else CORNERS):
        reach = min(G, Rk) if Rk != "G" else G  # R = 31 is outside 0..G at G = 8: G there
        ft, vt = FORMATS[idx % 4]
        f, v = cast[ft, vt]
        traj, cmds = tables[A, H]
        exp = _run(lib, G, cost, f, v, traj, cmds, reach, (G, n, A, H, reach, ft.__name__, vt.__name__))
        adm += int(exp["n_adm"].sum())
        blocked += int(((exp["blocked_at"] > 0) & (exp["blocked_at"] <= H)).sum())
        if Rk != 0:
            still = D.dwa(cost, None, None, CPS, reach, traj, cmds, _pycfg(G).footprint)
            met += int((still["blocked_at"] != exp["blocked_at"]).sum())
    assert adm > 0 and blocked > 0 and met > 0, (adm, blocked, met)  # the case shows something: candidates of both kinds, and moving sources that block


# ------------------------------------------------------------------ 2. further cases
def test_every_cell_a_source(lib):
    G, n = 64, 3
    cost, frame, flow = planes(G, n, seed=5, dense=True)
    traj, cmds = table(28, 24, seed=1)
    with np.errstate(over="ignore"):
        for ft, vt in FORMATS:
            exp = _run(lib, G, cost, frame.astype(ft), flow.astype(vt), traj, cmds, G, ("dense", ft.__name__, vt.__name__))
    still = D.dwa(cost, None, None, CPS, G, traj, cmds, _pycfg(G).footprint)
    assert (exp["blocked_at"] != still["blocked_at"]).sum() > 20 and (frame == 255).all()


def test_padded_strides_and_unaligned_bases(lib):
    G, n = 64, 5
    G2 = G * G
    cost, frame, flow = planes(G, n, seed=11)
    traj, cmds = table(28, 24, seed=2)
    foot = _pycfg(G).footprint
    for ft, vt in FORMATS:
        with np.errstate(over="ignore"):
            fc, vc = frame.astype(ft), flow.astype(vt)
        exp = D.dwa(cost, fc, vc, CPS, 31, traj, cmds, foot)
        tf = torch.float32 if ft is np.float32 else torch.uint8
        tv = torch.float32 if vt is np.float32 else torch.float16
        # the frame as state_m[:, 1] of a frame pair, the flow out of a larger buffer, the cost plane with an odd env stride
        pair = torch.full((n, 2, G, G), 255, dtype=tf, device=DEV)
        pair[:, 1] = _t(fc)
        big = torch.full((n, 3, G, G), 1.0, dtype=tv, device=DEV)
        big[:, :2] = _t(vc)
        cbuf = torch.full((n * (G2 + 1) + 1,), 65535, dtype=torch.uint16, device=DEV)
        cv = cbuf[1:].reshape(n, G2 + 1)
        cv[:, :G2] = _t(cost).reshape(n, G2)
        assert cv.data_ptr() % 4 == 2 and cv.stride(0) == G2 + 1 and pair[:, 1].stride(0) == 2 * G2
        out = _poison(n, 28)
        _launch(lib, G, cv, pair[:, 1], big, _t(traj), _t(cmds), out, 31)
        for k in OUTS:
            _same(out[k], exp[k], ("strides", ft.__name__, vt.__name__, k))
        # bases aligned to 4 but not to 16 bytes, env strides that are no multiple of 16 bytes: the 4-byte loads
        fe = 4 // np.dtype(ft).itemsize
        fbuf = torch.zeros(n * (G2 + 4) + fe, dtype=tf, device=DEV)
        fv = fbuf[fe:].reshape(n, G2 + 4)
        fv[:, :G2] = _t(fc).reshape(n, G2)
        ve = 4 // np.dtype(vt).itemsize
        vbuf = torch.zeros(n * (2 * G2 + 4) + ve, dtype=tv, device=DEV)
        vv = vbuf[ve:].reshape(n, 2 * G2 + 4)
        vv[:, :2 * G2] = _t(vc).reshape(n, 2 * G2)
        tbuf = torch.zeros(traj.size + 2, dtype=torch.int16, device=DEV)
        tbuf[2:] = _t(traj).reshape(-1)
        assert fv.data_ptr() % 16 == 4 and vv.data_ptr() % 16 == 4 and tbuf[2:].data_ptr() % 16 == 4
        out = _poison(n, 28)
        _launch(lib, G, _t(cost), fv, vv, tbuf[2:].reshape(traj.shape), _t(cmds), out, 31)
        for k in OUTS:
            _same(out[k], exp[k], ("unaligned", ft.__name__, vt.__name__, k))


def test_mask_window_null_frame_and_single_outputs(lib):
    G, n = 64, 6
    cost, frame, flow = planes(G, n, seed=21)
    traj, cmds = rollout_table(_pycfg(G), horizon=18)
    foot = _pycfg(G).footprint
    # mask=: the envs left out keep every poisoned word (the restatement starts from the same poison)
    mask = np.array([1, 0, 1, 1, 0, 1], np.uint8)
    prev = {k: v.cpu().numpy() for k, v in _poison(n, 28).items()}
    exp = D.dwa(cost, frame, flow, CPS, 32, traj, cmds, foot, mask=mask, prev=prev)
    out = _poison(n, 28)
    _launch(lib, G, _t(cost), _t(frame), _t(flow), _t(traj), _t(cmds), out, 32, mask=_t(mask))
    for k in OUTS:
        _same(out[k], exp[k], ("mask", k))
    assert out["choice"][1] == -7 and (out["blocked_at"][4] == 200).all() and out["choice"][0] != -7
    # the velocity window: rows inside, on the edge, outside every command, and NaN rows
    vel = np.array([[0.2, 0.0], [0.4, 0.2], [5.0, 0.0], [np.nan, 0.0], [0.0, np.nan], [0.6, -0.6]])
    for dv, dw in ((0.2, 0.2), (0.0, 0.0), (np.inf, np.inf), (0.2000001, 0.1999999)):
        exp = _run(lib, G, cost, frame, flow, traj, cmds, 32, ("vel", dv, dw), vel=vel, dv_max=dv, dw_max=dw)
        assert exp["n_adm"][3] == 0 and exp["n_adm"][4] == 0 and not exp["blocked_at"][3:5].any()  # a NaN is in no window
        assert exp["n_adm"][2] == 0 or dv == np.inf  # 5 m/s is within an infinite window alone
    assert exp["blocked_at"][0].astype(bool).sum() == 3  # the last window round (0.2, 0): v in 0, 0.2, 0.4 and w = 0 alone
    # frame = flow = NULL: static only
    exp = _run(lib, G, cost, None, None, traj, cmds, 32, "null")
    assert exp["n_adm"].sum() > 0
    # each output alone, the others NULL
    full = D.dwa(cost, frame, flow, CPS, 32, traj, cmds, foot)
    for k in OUTS:
        out = {k: _poison(n, 28)[k]}
        _launch(lib, G, _t(cost), _t(frame), _t(flow), _t(traj), _t(cmds), out, 32)
        _same(out[k], full[k], ("alone", k))
    # n == 0 launches nothing
    out = _poison(n, 28)
    _launch(lib, G, _t(cost), _t(frame), _t(flow), _t(traj), _t(cmds), out, 32, n=0)
    assert (out["choice"] == -7).all() and (out["blocked_at"] == 200).all()


# ------------------------------------------------------------------ 3. FFMPVec
def _expect(env, det, flow="own", **kw):
    """The restatement on the env's own tensors: the cost plane of this call, the newest frame, obs["flow"]."""
    H, cps, reach = D.host_knobs(env.cfg, kw.get("horizon", 24), kw.get("stride", 1), kw.get("src_reach"), kw.get("probe", 0.325))
    traj, cmds = rollout_table(env.cfg, horizon=H, stride=kw.get("stride", 1), probe=kw.get("probe", 0.325))
    assert det["horizon"] == H
    frame = vflow = None
    if flow == "own":
        frame, vflow = env.state_m[:, 1].cpu().numpy(), env.obs["flow"].cpu().numpy()
    elif flow is not None:
        frame, vflow = flow.frame.cpu().numpy(), flow.flow.cpu().numpy()
    vel = kw.get("vel")
    dv, dw = kw.get("accel", (0.0, 0.0))
    return D.dwa(det["cost"].cpu().numpy(), frame, vflow, cps, reach, traj, cmds, env.cfg.footprint,
                 vel=None if vel is None else vel.cpu().numpy(), dv_max=dv, dw_max=dw)


def _check_detail(env, where, flow="own", **kw):
    call = dict(kw)
    if flow != "own":
        call["flow"] = flow
    det = env.policy_dwa(detail=True, **call)
    exp = _expect(env, det, flow=flow, **kw)
    for k in OUTS:
        _same(det[k], exp[k], (where, k))
    stop = np.where(exp["choice"] < 0, 3, exp["choice"]).astype(np.int64)
    _same(det["action"], stop, (where, "action"))
    return det, exp


@pytest.mark.parametrize("fmt", ["f32", "u8f16"])
@pytest.mark.parametrize("G", [64, 256])
def test_policy_dwa_of_a_live_env(G, fmt):
    if G == 64:
        cfg, n = FFMPConfig(**TIE[64]), 6
    else:
        cfg, n = FFMPConfig(grid=G, n_obst=12, n_beams=0, moving=True, flow=True, world_half=3.0, goal_min=1.0, goal_max=3.5,
                            obst_rmax=0.6, obst_vmax=1.0, max_steps=50, seed=8), 3
    env = FFMPVec(n, cfg, device=DEV, autotune=False, obs_format=fmt)
    twin = FFMPVec(n, cfg, device=DEV, autotune=False, obs_format=fmt)
    with pytest.raises(RuntimeError, match="reset"):
        env.policy_dwa()
    env.reset()
    twin.reset()
    rng = np.random.default_rng(2)
    for _ in range(4):
        a = torch.as_tensor(rng.integers(14, 28, n), device=DEV)
        env.step(a)
        twin.step(a)
    met = 0
    for step in range(6):
        det, exp = _check_detail(env, (G, fmt, step))
        cmd = env.policy_dwa()
        assert cmd.dtype == torch.float64 and tuple(cmd.shape) == (n, 2) and torch.equal(cmd, det["cmd"])
        ids = env.policy_dwa(actions=True)
        assert ids.dtype == torch.int64 and torch.equal(ids, det["action"])
        cost = env.nav_field(cost=True)["cost"]
        assert torch.equal(cost.view(torch.int16), det["cost"].view(torch.int16))
        still = env.policy_dwa(flow=None, detail=True)
        met += int((still["blocked_at"] != det["blocked_at"]).sum())
        # the ids fed to step() give the state the commands give
        env.step(cmd)
        twin.step(ids)
        for name in ("pose", "state_m", "reward", "done"):
            assert torch.equal(getattr(env, name), getattr(twin, name)), (G, fmt, step, name)
    assert met > 0  # the flow blocked something the static plane does not
    # the other arguments
    out = torch.empty((n, 2), dtype=torch.float64, device=DEV)
    assert env.policy_dwa(out=out) is out and torch.equal(out, env.policy_dwa())
    ids = torch.empty(n, dtype=torch.int64, device=DEV)
    assert env.policy_dwa(out=ids, actions=True) is ids
    _check_detail(env, (G, fmt, "static"), flow=None)
    _check_detail(env, (G, fmt, "knobs"), horizon=9, stride=2, probe=0.2, src_reach=20)
    vel = torch.as_tensor([[0.2, 0.0]] * (n - 1) + [[float("nan"), 0.0]], dtype=torch.float64, device=DEV)
    det, exp = _check_detail(env, (G, fmt, "window"), vel=vel, accel=(0.2, 0.2))
    assert exp["n_adm"][-1] == 0 and (exp["n_adm"][:-1] <= 9).all() and det["action"][-1] == 3
    if cfg.n_beams:
        lf = env.lidar_flow(lag=2)
        lf.update()
        env.step(env.policy_dwa())
        lf.update()
        _check_detail(env, (G, fmt, "LidarFlow"), flow=lf)
        det = env.policy_dwa(lidar=True, detail=True)
        assert torch.equal(det["cost"].view(torch.int16), env.nav_field(cost=True, lidar=True)["cost"].view(torch.int16))
    # the table is kept per (horizon, stride, probe) and dropped with the config
    assert set(env._dwa_tables) >= {(24, 1, 0.325), (9, 2, 0.2)}
    env.seed(99)
    assert env._dwa_tables is None
    # the errors
    for kw, word in ((dict(flow=3), "flow"), (dict(vel=vel), "go together"), (dict(accel=(0.1, 0.1)), "go together"),
                     (dict(vel=vel.float(), accel=(0.1, 0.1)), "vel"), (dict(out=out[:1]), "out"), (dict(out=out, actions=True), "out"),
                     (dict(probe=1.5), "28"), (dict(horizon=0), "horizon")):
        with pytest.raises(ValueError, match=word):
            env.policy_dwa(**kw)
    for kw in (dict(src_reach=-1), dict(src_reach=G + 1), dict(vel=vel, accel=(-0.1, 0.1))):
        with pytest.raises(_abi.FFMPBackendError):
            env.policy_dwa(**kw)
    if cfg.n_beams:
        with pytest.raises(ValueError, match="LidarFlow of this env"):
            twin.policy_dwa(flow=lf)
    env.close()
    twin.close()


def test_without_flow_planes_and_the_single_env():
    cfg = FFMPConfig(grid=64, n_obst=4, n_beams=0, moving=True)
    env = FFMPVec(2, cfg, device=DEV, autotune=False)
    env.reset()
    with pytest.raises(ValueError, match="flow=True"):
        env.policy_dwa()
    _check_detail(env, "no flow planes", flow=None)
    env.close()
    one = FFMP(FFMPConfig(**TIE[64]), device=DEV, verbose=False)
    with pytest.raises(RuntimeError):
        one.policy_dwa()
    one.reset()
    one.step(24)
    det, exp = _check_detail(one._vec_env(), "single env")
    assert torch.equal(one.policy_dwa(), det["cmd"]) and tuple(one.policy_dwa(actions=True).shape) == (1,)
    one.close()


# ------------------------------------------------------------------ 4. the crossing family in closed loop
def test_crossing_family_equals_the_cpu_closed_loop():
    """The 24 crossing scenes (tests/flow_predict_ref.py) through set_scenarios, stepped with policy_dwa(): the per-env
    outcome and the step it happened at equal the CPU run (the NumPy oracle driven by the restatements), recorded in
    tests/golden/dwa_crossing.json and recomputed by tests/test_dwa_host.py.  Every link is bit-exact, so equality is
    the assertion."""
    with open(D.GOLDEN) as f:
        gold = json.load(f)["dwa"]
    cfg = FFMPConfig(**R.CROSS_CFG)
    sc = R.crossing_scenes()
    env = FFMPVec(len(sc["pose"]), cfg, device=DEV, autotune=False)
    env.reset()
    env.set_scenarios(**sc)
    env.check_errors()
    flags = []
    for _ in range(R.CROSS_STEPS):
        env.step(env.policy_dwa())
        flags.append((env.is_goal.cpu().numpy().copy(), env.collision.cpu().numpy().copy(), env.truncated.cpu().numpy().copy()))
        if (NR._outcomes(flags)[0] != 0).all():
            break
    env.check_errors()
    env.close()
    o, t = NR._outcomes(flags)
    print("dwa", "".join(map(str, o.tolist())), t.tolist())
    assert o.tolist() == gold["outcome"] and t.tolist() == gold["step"]
    with open(R.GOLDEN) as f:
        plain = json.load(f)["plain"]["outcome"]
    assert sum(x == 2 for x in gold["outcome"]) <= sum(x == 2 for x in plain)


# ------------------------------------------------------------------ 5. inside a graph capture
def test_graph_capture():
    cfg = FFMPConfig(**TIE[64])
    n = 4
    env = FFMPVec(n, cfg, device=DEV, autotune=False, frame_window=2)
    env.reset()
    env.step(torch.full((n,), 24, device=DEV))
    out = torch.empty((n, 2), dtype=torch.float64, device=DEV)
    eager = env.policy_dwa().clone()  # one eager call: the table goes to the device here
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=torch.cuda.Stream(device=DEV)):
        assert env.policy_dwa(out=out) is out
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    for a in (25, 22):
        for _ in range(3):
            env.step(torch.full((n,), a, device=DEV))
        out.fill_(7.0)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, env.policy_dwa())
        _check_detail(env, ("replay", a))
    env.close()
