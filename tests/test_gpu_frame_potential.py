"""The potential field of an occupancy frame on the GPU (include/ffmp.h ffmp_frame_potential, DESIGN §3 a18b /
§5.15) against its NumPy restatement (tests/frame_potential_ref.py), bit for bit (a NaN equal to any NaN: its
sign and payload are the machine's):

1. random planes in the four frame x potential formats at G = 8, 36, 64, 100, 260 and n = 1, 3, 70, reach 1, 10,
   32 and occ_min 255, 128, 1 dealt over them, G = 512 once — about 3 % hits and 3 % other values, obstacles on
   every border, an all-obstacle and an empty env, a NaN and an inf goal;
2. mask=, env strides of a larger buffer, bases aligned to 4 but not 16 bytes, every output alone;
3. FFMPVec.frame_potential over state_m, lidar=True, a LidarMap and predict=True, FFMP.frame_potential, the errors;
4. policy_field(grad=...) against the float64 restatement of the follower, policy_field(lidar=True), and plain
   policy_field() against an env that never touched the feature;
5. inside a graph capture of the caller's."""
import ctypes as C

import numpy as np
import pytest
import torch

from flow_field_based_motion_planner_amd import _abi
from flow_field_based_motion_planner_amd.config import FFMPConfig
from flow_field_based_motion_planner_amd.env import FFMP
from flow_field_based_motion_planner_amd.vec_env import FFMPVec
from tests import frame_potential_ref as R
from tests.scan_flow_ref import TIE

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
KEYS = ("dist2", "potential", "grad", "robot_d2")
TORCH = {np.float32: torch.float32, np.float16: torch.float16, np.uint8: torch.uint8}


def _t(x):
    return torch.as_tensor(np.ascontiguousarray(x)).to(DEV)


def _config(G):
    return FFMPConfig(grid=G, n_obst=1, n_beams=0)


def _planes(G, n, seed):
    """(frame float32 with values a uint8 holds, goals): about 3 % hits and 3 % other values, obstacles on every
    border and in the corners, env 1 all obstacle and env 2 empty (n >= 3), a NaN and an inf goal (n >= 3)."""
    rng = np.random.default_rng(seed)
    u = rng.random((n, G, G))
    frame = np.zeros((n, G, G), F32)
    frame[u < 0.03] = 255
    other = (u >= 0.03) & (u < 0.06)
    frame[other] = rng.integers(1, 255, int(other.sum()))
    frame[:, 0, ::4] = frame[:, G - 1, 1::4] = frame[:, 2::4, 0] = frame[:, 3::4, G - 1] = 255
    frame[:, 0, 0] = frame[:, G - 1, G - 1] = 255
    goal = rng.uniform(-3.0, 3.0, (n, 2)).astype(F32)
    if n >= 3:
        frame[1] = 255
        frame[2] = 0
        goal[0, 1] = np.nan
        goal[n - 1, 0] = np.inf
    return frame, goal


def _launch(lib, G, frame, goal, occ_min, reach, dist2=None, potential=None, grad=None, robot_d2=None, mask=None, goal_stride=2,
            dist2_stride=None, pot_stride=None, n=None):
    """ffmp_frame_potential over device tensors (any view whose env planes are dense) on the default stream."""
    cfg = _abi.make_cfg(_config(G))
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    pfmt = _abi.OBS_U8F16 if potential is not None and potential.dtype == torch.float16 else _abi.OBS_F32
    rc = lib.ffmp_frame_potential(C.byref(cfg), frame.shape[0] if n is None else n, frame.data_ptr(), frame.stride(0),
                                  _abi.OBS_F32 if frame.dtype == torch.float32 else _abi.OBS_U8F16, goal.data_ptr(), goal_stride, p(mask),
                                  occ_min, reach, p(dist2), G * G if dist2_stride is None else dist2_stride, p(potential),
                                  G * G if pot_stride is None else pot_stride, pfmt, p(grad), p(robot_d2), None)
    assert rc == 0, lib.ffmp_last_error()
    torch.cuda.synchronize()


def _np(t):
    return t.cpu().numpy() if isinstance(t, torch.Tensor) else t


def _same(got, exp, where):
    got = _np(got)
    ok = R.same_bits(got, exp)
    bad = np.nonzero(~ok)
    assert not len(bad[0]), (where, len(bad[0]), [b[:5] for b in bad], got[bad][:5], exp[bad][:5])


def _fresh(n, G, pdt):
    """Poisoned outputs: a launch has to write every word."""
    return dict(dist2=_t(np.full((n, G, G), 7, np.uint16)), potential=torch.full((n, G, G), -3.0, dtype=TORCH[pdt], device=DEV),
                grad=torch.full((n, 2), -3.0, device=DEV), robot_d2=torch.full((n,), -9, dtype=torch.int32, device=DEV))


def _run(lib, G, frame, goal, occ_min, reach, pdt, where):
    exp = R.frame_potential(frame, goal, _config(G), occ_min=occ_min, reach=reach, dtype=pdt)
    out = _fresh(frame.shape[0], G, pdt)
    _launch(lib, G, _t(frame), _t(goal), occ_min, reach, **out)
    for k in KEYS:
        _same(out[k], exp[k], (where, k))
    return exp


# ------------------------------------------------------------------ 1. random planes
CASES = [(8, 1, 1, 255), (8, 3, 32, 1), (8, 70, 10, 128), (36, 1, 10, 128), (36, 3, 1, 255), (36, 70, 32, 1), (64, 1, 32, 255),
         (64, 3, 10, 1), (64, 70, 1, 128), (100, 1, 10, 1), (100, 3, 32, 255), (100, 70, 10, 255), (260, 1, 32, 128), (260, 3, 10, 255),
         (260, 70, 1, 1), (512, 1, 32, 255)]


@pytest.mark.parametrize("G,n,reach,occ_min", CASES)
def test_random_planes_equal_the_restatement(lib, G, n, reach, occ_min):
    frame, goal = _planes(G, n, seed=G + n)
    f32 = frame.copy()  # values only a float32 frame can hold
    sel = [e for e in range(n) if e not in (1, 2)]  # not the all-obstacle and the empty env
    f32[sel, 1, 1::5] = np.nan
    f32[sel, 2, 1::5] = -4.0
    f32[sel, 3, 1::5] = 0.25
    f32[sel, 4, 1::5] = 255.5
    f32[sel, 5, 1::5] = 127.5
    for ft in (np.float32, np.uint8):
        fr = f32 if ft is np.float32 else frame.astype(np.uint8)
        for pdt in (np.float32, np.float16):
            exp = _run(lib, G, fr, goal, occ_min, reach, pdt, (G, n, reach, occ_min, ft.__name__, pdt.__name__))
        near = (exp["dist2"] != 65535) & (exp["dist2"] != 0)
        assert near.any() and (exp["dist2"] == 0).any()  # the case shows something
        if n >= 3:
            assert (exp["dist2"][1] == 0).all() and (exp["dist2"][2] == 65535).all() and exp["robot_d2"][2] == -1
            assert np.isnan(exp["potential"][0]).all() and np.isnan(exp["grad"][0]).all() and np.isnan(exp["grad"][n - 1, 0])
        if reach * 0.05 < 0.5 and G > 8:
            assert (exp["dist2"] == 65535).any()


# ------------------------------------------------------------------ 2. mask, strides, alignment, every output alone
@pytest.mark.parametrize("G", [36, 64])
def test_mask_strides_unaligned_bases_and_single_outputs(lib, G):
    n, reach = 5, 10
    G2 = G * G
    frame, goal = _planes(G, n, seed=11)
    cfg = _config(G)
    exp = {pdt: R.frame_potential(frame, goal, cfg, reach=reach, dtype=pdt) for pdt in (np.float32, np.float16)}
    # mask=: the envs left out keep every poisoned word
    mask = np.array([1, 0, 1, 1, 0], np.uint8)
    out = _fresh(n, G, np.float32)
    poison = {k: v.cpu().numpy() for k, v in out.items()}
    _launch(lib, G, _t(frame), _t(goal), 255, reach, mask=_t(mask), **out)
    want = R.frame_potential(frame, goal, cfg, reach=reach, mask=mask, **{k + "_in": poison[k] for k in KEYS})
    for k in KEYS:
        _same(out[k], want[k], ("mask", k))
        assert (out[k][1].cpu().numpy() == poison[k][1]).all()
    # every output alone, and the gradient with the clearance but without a plane (only the rows it needs are worked on)
    for keys in (("dist2",), ("potential",), ("grad",), ("robot_d2",), ("grad", "robot_d2"), ("dist2", "grad")):
        for pdt in (np.float32, np.float16):
            out = {k: v for k, v in _fresh(n, G, pdt).items() if k in keys}
            _launch(lib, G, _t(frame.astype(np.uint8)), _t(goal), 255, reach, **out)
            for k in keys:
                _same(out[k], exp[pdt][k], ("alone", keys, k))
    # a reach below the default one: the gradient is that of the cut-off field, with or without the plane
    short = R.frame_potential(frame, goal, cfg, reach=1)
    out = {"grad": torch.zeros((n, 2), device=DEV), "robot_d2": torch.zeros(n, dtype=torch.int32, device=DEV)}
    _launch(lib, G, _t(frame), _t(goal), 255, 1, **out)
    _same(out["grad"], short["grad"], "reach 1 grad")
    _same(out["robot_d2"], short["robot_d2"], "reach 1 robot_d2")
    for ft in (np.float32, np.uint8):
        for pdt in (np.float32, np.float16):
            fc = frame.astype(ft)
            # the frame as state_m[:, 1] of a frame pair, the goal as words 8..9 of a record, the planes out of larger buffers
            pair = torch.full((n, 2, G, G), 255, dtype=TORCH[ft], device=DEV)
            pair[:, 1] = _t(fc)
            record = torch.full((n, 28), 5.0, device=DEV)
            record[:, 8:10] = _t(goal)
            wide_d = _t(np.full((n, G2 + 16), 7, np.uint16))
            wide_p = torch.full((n, G2 + 16), -3.0, dtype=TORCH[pdt], device=DEV)
            grad = torch.zeros((n, 2), device=DEV)
            rd2 = torch.zeros(n, dtype=torch.int32, device=DEV)
            assert pair[:, 1].stride(0) == 2 * G2
            _launch(lib, G, pair[:, 1], record[:, 8:10], 255, reach, dist2=wide_d, potential=wide_p, grad=grad, robot_d2=rd2,
                    goal_stride=28, dist2_stride=G2 + 16, pot_stride=G2 + 16)
            where = ("strides", ft.__name__, pdt.__name__)
            _same(_np(wide_d)[:, :G2].reshape(n, G, G), exp[pdt]["dist2"], where)
            _same(_np(wide_p)[:, :G2].reshape(n, G, G), exp[pdt]["potential"], where)
            _same(grad, exp[pdt]["grad"], where)
            _same(rd2, exp[pdt]["robot_d2"], where)
            assert (_np(wide_d)[:, G2:] == 7).all() and (_np(wide_p)[:, G2:] == -3).all()
            # bases aligned to 4 but not to 8 or 16 bytes, env strides that are no multiple of 16 bytes: the 4-byte accesses
            fe = 4 // np.dtype(ft).itemsize  # elements in 4 bytes
            fbuf = torch.zeros(n * (G2 + 4) + fe, dtype=TORCH[ft], device=DEV)
            fv = fbuf[fe:].reshape(n, G2 + 4)
            fv[:, :G2] = _t(fc).reshape(n, G2)
            dbuf = _t(np.full(n * (G2 + 4) + 2, 7, np.uint16))
            dv = dbuf[2:].reshape(n, G2 + 4)
            pe = 4 // np.dtype(pdt).itemsize
            pbuf = torch.full((n * (G2 + 4) + pe,), -3.0, dtype=TORCH[pdt], device=DEV)
            pv = pbuf[pe:].reshape(n, G2 + 4)
            assert fv.data_ptr() % 16 == 4 and dv.data_ptr() % 8 == 4 and pv.data_ptr() % 8 == 4
            grad.zero_()
            _launch(lib, G, fv, _t(goal), 255, reach, dist2=dv, potential=pv, grad=grad, dist2_stride=G2 + 4, pot_stride=G2 + 4)
            where = ("unaligned", ft.__name__, pdt.__name__)
            _same(_np(dbuf)[2:].reshape(n, G2 + 4)[:, :G2].reshape(n, G, G), exp[pdt]["dist2"], where)
            _same(_np(pbuf)[pe:].reshape(n, G2 + 4)[:, :G2].reshape(n, G, G), exp[pdt]["potential"], where)
            _same(grad, exp[pdt]["grad"], where)
            assert (_np(dbuf)[2:].reshape(n, G2 + 4)[:, G2:] == 7).all() and (_np(pbuf)[pe:].reshape(n, G2 + 4)[:, G2:] == -3).all()
            assert (_np(dbuf)[:2] == 7).all() and (_np(pbuf)[:pe] == -3).all()
    # n == 0 launches nothing
    out = _fresh(n, G, np.float32)
    _launch(lib, G, _t(frame), _t(goal), 255, reach, n=0, **out)
    assert (out["potential"] == -3).all() and (out["robot_d2"] == -9).all()


# ------------------------------------------------------------------ 3. FFMPVec
def _expect(env, plane=None, goal=None, **kw):
    plane = env.state_m[:, 1] if plane is None else plane
    goal = env.record[:, 8:10] if goal is None else goal
    dtype = np.float16 if kw.pop("dtype", torch.float32) == torch.float16 else np.float32
    return R.frame_potential(plane.cpu().numpy(), goal.cpu().numpy(), env.cfg, dtype=dtype, **kw)


def _same_dict(got, exp, res, where):
    for k in KEYS:
        if k in got:
            _same(got[k], exp[k], (where, k))
    _same(got["clearance"], R.clearance(exp["robot_d2"], res), (where, "clearance"))


@pytest.mark.parametrize("fmt", ["f32", "u8f16"])
def test_frame_potential_of_a_live_env(fmt):
    cfg = FFMPConfig(**TIE[64])
    n, G = 6, 64
    env = FFMPVec(n, cfg, device=DEV, autotune=False, obs_format=fmt)
    with pytest.raises(RuntimeError, match="reset"):
        env.frame_potential()
    env.reset()
    lm = env.lidar_map(unknown=0)
    lm.update()
    rng = np.random.default_rng(2)
    for _ in range(5):
        env.step(torch.as_tensor(rng.integers(21, 28, n), device=DEV))
        lm.update()
    before = {k: v.clone() for k, v in env.obs.items()}
    # the newest frame of the window: walls and discs repel
    got = env.frame_potential(distance=True)
    assert set(got) == {"grad", "robot_d2", "clearance", "potential", "dist2"}
    assert got["potential"].dtype == torch.float32 and got["dist2"].dtype == torch.uint16 and got["clearance"].dtype == torch.float64
    assert tuple(got["potential"].shape) == (n, G, G) and tuple(got["grad"].shape) == (n, 2)
    exp = _expect(env)
    _same_dict(got, exp, cfg.res, (fmt, "state_m"))
    assert (exp["dist2"] == 0).any() and (exp["dist2"] == 65535).any()
    half = env.frame_potential(dtype=torch.float16)
    assert half["potential"].dtype == torch.float16 and "dist2" not in half
    _same_dict(half, _expect(env, dtype=torch.float16), cfg.res, (fmt, "float16"))
    only = env.frame_potential(potential=False, distance=True, reach=3)
    assert "potential" not in only
    _same_dict(only, _expect(env, reach=3), cfg.res, (fmt, "clearance alone"))
    # knobs, a goal of the caller's, out= and mask=
    goal = torch.as_tensor([[0.5, -0.25]] * n, dtype=torch.float32, device=DEV)
    _same_dict(env.frame_potential(goal=goal, occ_min=1, reach=12), _expect(env, goal=goal, occ_min=1, reach=12), cfg.res, (fmt, "knobs"))
    out = {"potential": torch.full((n, G, G), -3.0, device=DEV), "grad": torch.full((n, 2), -3.0, device=DEV),
           "robot_d2": torch.full((n,), -9, dtype=torch.int32, device=DEV), "dist2": _t(np.full((n, G, G), 7, np.uint16))}
    mask = torch.as_tensor([True, False, True, True, False, True], device=DEV)
    res = env.frame_potential(out=out, mask=mask)
    assert all(res[k] is out[k] for k in KEYS)
    m = mask.cpu().numpy()
    want = R.frame_potential(env.state_m[:, 1].cpu().numpy(), env.record[:, 8:10].cpu().numpy(), cfg, mask=m,
                             dist2_in=np.full((n, G, G), 7, np.uint16), potential_in=np.full((n, G, G), -3.0, F32),
                             grad_in=np.full((n, 2), -3.0, F32), robot_d2_in=np.full(n, -9))
    for k in KEYS:
        _same(res[k], want[k], (fmt, "out= and mask", k))
    # the sensor planes: the scan frame, the accumulated map, the predicted plane, a plane of the caller's
    scan = env.lidar_frames(unknown=0, newest_only=True)
    _same_dict(env.frame_potential(lidar=True), _expect(env, plane=scan), cfg.res, (fmt, "lidar"))
    assert (scan == 255).any()
    _same_dict(env.frame_potential(lidar_map=lm, distance=True), _expect(env, plane=lm.frame), cfg.res, (fmt, "lidar_map"))
    pred = env.predicted_frames()
    _same_dict(env.frame_potential(predict=True, occ_min=254), _expect(env, plane=pred, occ_min=254), cfg.res, (fmt, "predict"))
    vis = env.visible_frames(unknown=0, newest_only=True)
    _same_dict(env.frame_potential(visible=True), _expect(env, plane=vis), cfg.res, (fmt, "visible"))
    _same_dict(env.frame_potential(frames=pred), _expect(env, plane=pred), cfg.res, (fmt, "frames="))
    # the follower over a sensed plane is the follower over that plane's gradient
    g = env.frame_potential(lidar=True, potential=False)["grad"]
    _same(env.policy_field(lidar=True), R.policy_field(g.cpu().numpy(), cfg.dt), (fmt, "policy_field(lidar=True)"))
    assert torch.equal(env.policy_field(lidar_map=lm), env.policy_field(grad=env.frame_potential(lidar_map=lm)["grad"]))
    # nothing of the observation moved
    assert all(torch.equal(before[k], env.obs[k]) for k in before)
    # the errors
    for kw in (dict(frames=pred, lidar=True), dict(visible=True, lidar=True), dict(predict=True, lidar_map=lm)):
        with pytest.raises(ValueError, match="pass"):
            env.frame_potential(**kw)
    with pytest.raises(ValueError, match="rho0.*res|res.*rho0"):
        env.frame_potential(reach=9)
    env.frame_potential(reach=9, potential=False)
    for kw, word in ((dict(dtype=torch.float64), "dtype"), (dict(goal=goal[:3]), "goal"), (dict(goal=goal.double()), "goal"),
                     (dict(frames=pred[:, :32]), "frames"), (dict(out={"potential": out["potential"].half()}), "potential"),
                     (dict(out={"grad": out["grad"][:2]}), "grad"), (dict(out={"cost": out["grad"]}), "cost"),
                     (dict(grad=g, lidar=True), "not both")):
        with pytest.raises(ValueError, match=word):
            (env.policy_field if "grad" in kw else env.frame_potential)(**kw)
    for kw in (dict(occ_min=0), dict(occ_min=256), dict(reach=33), dict(reach=0, potential=False)):
        with pytest.raises(_abi.FFMPBackendError):
            env.frame_potential(**kw)
    env.close()


def test_a_rho0_beyond_the_window_and_the_single_env():
    cfg = FFMPConfig(grid=64, n_obst=4, n_beams=0, rho0=2.0)  # 40 cells
    env = FFMPVec(2, cfg, device=DEV, autotune=False)
    env.reset()
    for call in (env.frame_potential, env.policy_field):
        with pytest.raises(ValueError, match="rho0.*res"):
            call(frames=env.state_m[:, 1].contiguous())
    with pytest.raises(ValueError, match="rho0.*res"):
        env.frame_potential(reach=32)
    got = env.frame_potential(reach=32, potential=False, distance=True)
    _same_dict(got, _expect(env, reach=32), cfg.res, "clearance at reach 32")
    env.close()
    one = FFMP(FFMPConfig(**TIE[64]), device=DEV, verbose=False)
    with pytest.raises(RuntimeError):
        one.frame_potential()
    one.reset()
    one.step(24)
    got = one.frame_potential(distance=True)
    assert tuple(got["potential"].shape) == (1, 64, 64)
    _same_dict(got, _expect(one._vec_env()), one.cfg.res, "single env")
    one.close()


# ------------------------------------------------------------------ 4. the follower
def test_policy_field_over_a_gradient_and_untouched_without_one():
    cfg = FFMPConfig(**TIE[64])
    n = 64
    env = FFMPVec(n, cfg, device=DEV, autotune=False)
    twin = FFMPVec(n, cfg, device=DEV, autotune=False)  # never touches the feature
    env.reset()
    twin.reset()
    rng = np.random.default_rng(4)
    grads = rng.normal(0.0, 1.0, (n, 2)).astype(F32)
    grads[0] = 0.0
    grads[1] = (np.nan, 1.0)
    grads[2] = (np.inf, 0.0)
    grads[3] = (-1.0, 0.0)   # straight ahead
    grads[4] = (1.0, 0.0)    # straight behind: turn on the spot
    grads[5] = (1.0, 1e-3)
    grads[6] = (0.0, -1e-30)
    grads[7] = (1e30, 1e30)  # the squared norm is finite in float64
    _same(env.policy_field(grad=_t(grads)), R.policy_field(grads, cfg.dt), "policy_field(grad=)")
    out = torch.empty((n, 2), dtype=torch.float64, device=DEV)
    assert env.policy_field(out=out, grad=_t(grads)) is out
    _same(out, R.policy_field(grads, cfg.dt), "policy_field(out=, grad=)")
    for step in range(4):
        env.frame_potential(distance=True)
        env.policy_field(grad=_t(grads))
        a, b = env.policy_field(), twin.policy_field()
        assert torch.equal(a, b), step
        _same(a, R.policy_field(env.obs["grad"].cpu().numpy(), cfg.dt), ("policy_field()", step))
        env.step(a)
        twin.step(b)
        assert all(torch.equal(env.obs[k], twin.obs[k]) for k in env.obs)
    with pytest.raises(ValueError, match="grad"):
        env.policy_field(grad=_t(grads).double())
    with pytest.raises(ValueError, match="grad"):
        env.policy_field(grad=_t(grads)[:3])
    env.close()
    twin.close()


# ------------------------------------------------------------------ 5. inside a graph capture
def test_graph_capture():
    cfg = FFMPConfig(**TIE[64])
    n = 4
    env = FFMPVec(n, cfg, device=DEV, autotune=False, frame_window=2)
    env.reset()
    env.step(torch.full((n,), 24, device=DEV))
    out = {"potential": torch.empty((n, 64, 64), device=DEV), "dist2": torch.empty((n, 64, 64), dtype=torch.uint16, device=DEV),
           "grad": torch.empty((n, 2), device=DEV), "robot_d2": torch.empty(n, dtype=torch.int32, device=DEV)}
    cmd = torch.empty((n, 2), dtype=torch.float64, device=DEV)
    eager = {k: v.clone() for k, v in env.frame_potential(distance=True).items()}  # one eager call
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=torch.cuda.Stream(device=DEV)):
        res = env.frame_potential(out=out)
        env.policy_field(out=cmd, grad=res["grad"])
    g.replay()
    torch.cuda.synchronize()
    assert all(R.same_bits(out[k].cpu().numpy(), eager[k].cpu().numpy()).all() for k in KEYS)
    seen = [eager["potential"]]
    for a in (25, 22):
        for _ in range(3):
            env.step(torch.full((n,), a, device=DEV))
        for k in ("potential", "grad"):
            out[k].fill_(7)
        g.replay()
        torch.cuda.synchronize()
        exp = _expect(env)
        for k in KEYS:
            _same(out[k], exp[k], ("replay", a, k))
        _same(cmd, R.policy_field(exp["grad"], cfg.dt), ("replay cmd", a))
        assert not any(torch.equal(out["potential"], s) for s in seen)
        seen.append(out["potential"].clone())
    env.close()
