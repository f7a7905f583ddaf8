"""Continuous (v, w) commands (SPEC a15b) without a GPU: the four ABI-9 entry points are declared,
bound and exported consistently; their argument checks answer before any launch; the ROS adapters
round-trip a command; FFMPVec / FFMP validate the shape and dtype of what step() is given."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from flow_field_based_motion_planner_amd import _abi, ros_adapters
from flow_field_based_motion_planner_amd.config import FFMPConfig, action_table
from flow_field_based_motion_planner_amd.env import FFMP
from flow_field_based_motion_planner_amd.vec_env import FFMPVec

CMD_SYMBOLS = ("ffmp_step_state_cmd", "ffmp_step_fused_cmd", "ffmp_step_cmd", "ffmp_policy_field")


def _header():
    return open(_abi.HEADER_PATH).read()


def test_header_binding_and_library_agree(lib):
    h = _header()
    assert int(re.search(r"#define FFMP_ABI_VERSION (\d+)", h).group(1)) == 9 == _abi.ABI_VERSION
    assert lib.ffmp_abi_version() == 9
    code = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    for name in CMD_SYMBOLS:
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, code)
        assert m, name
        params = [p.strip() for p in m.group(1).split(",")]
        res, args = _abi._SIGS[name]
        assert res is C.c_int and len(args) == len(params), (name, params)
        assert hasattr(lib, name)
        # the command array is a double*, const for the steps that read it
        cmd = [p for p in params if re.search(r"\bcmd$", p)]
        assert cmd == (["double* cmd"] if name == "ffmp_policy_field" else ["const double* cmd"]), (name, cmd)
    # the id entry points and their command forms take the same arguments, the array aside
    for ids, cmd in (("ffmp_step_state", "ffmp_step_state_cmd"), ("ffmp_step_fused", "ffmp_step_fused_cmd"),
                     ("ffmp_step", "ffmp_step_cmd"), ("ffmp_policy_reactive", "ffmp_policy_field")):
        assert _abi._SIGS[ids] == _abi._SIGS[cmd]
    # the header's convention: the comment above an entry point cites the reference lines it stands for
    for name in CMD_SYMBOLS:
        decl = h.index("int %s(" % name)
        comment = h[h.rindex("/*", 0, decl):decl]
        assert "ffmp.py:29-32" in comment and "train.py:134-143" in comment, name
    # the structs did not change (existing callers build them positionally)
    assert len(_abi.StateT._fields_) == 11 and len(_abi.ObsT._fields_) == 12 and len(_abi.OutT._fields_) == 5
    _abi.verify_layout(lib)


def _host_structs():
    dummy = (C.c_double * 16)()
    p = C.cast(dummy, C.c_void_p).value
    p += (-p) % 16
    st = _abi.StateT(p, p, p, p, p, p, p, p, p)
    ob = _abi.ObsT(p, p, p, p, p, p, p)
    out = _abi.OutT(p, p, p, p, p)
    return dummy, p, st, ob, out


def test_argument_checks_without_a_launch(lib):
    cfg = _abi.make_cfg(FFMPConfig(grid=64, n_obst=4, n_beams=0))
    keep, p, st, ob, out = _host_structs()
    R = C.byref
    steps = ((lib.ffmp_step_state_cmd, ()), (lib.ffmp_step_fused_cmd, (0,)), (lib.ffmp_step_cmd, ()))
    for fn, extra in steps:
        # NULL cmd
        assert fn(R(cfg), 4, 0, None, R(st), R(ob), R(out), *extra, None) == -1
        assert b"cmd" in lib.ffmp_last_error() and b"NULL" in lib.ffmp_last_error()
        # 8-byte aligned only: each env's pair is one 16-byte load
        assert fn(R(cfg), 4, 0, p + 8, R(st), R(ob), R(out), *extra, None) == -1
        assert b"16-byte aligned" in lib.ffmp_last_error()
        # n == 0: a no-op success, nothing launched
        assert fn(R(cfg), 0, 0, p, R(st), R(ob), R(out), *extra, None) == 0
        # the checks every step makes still answer first
        assert fn(R(cfg), -1, 0, p, R(st), R(ob), R(out), *extra, None) == -1
        bad = _abi.make_cfg(FFMPConfig(grid=64, n_obst=4, n_beams=0))
        bad.grid = 66
        assert fn(R(bad), 0, 0, p, R(st), R(ob), R(out), *extra, None) == -3
    # the follower
    assert lib.ffmp_policy_field(R(cfg), 4, R(ob), None, None) == -1
    assert b"cmd is NULL" in lib.ffmp_last_error()
    assert lib.ffmp_policy_field(R(cfg), 4, R(ob), p + 8, None) == -1
    assert b"16-byte aligned" in lib.ffmp_last_error()
    no_grad = _abi.ObsT(p, p, p, p, p, None, p)
    assert lib.ffmp_policy_field(R(cfg), 4, R(no_grad), p, None) == -1
    assert b"obs.grad" in lib.ffmp_last_error()
    assert lib.ffmp_policy_field(R(cfg), 4, None, p, None) == -1
    assert lib.ffmp_policy_field(R(cfg), 0, R(ob), p, None) == 0
    assert lib.ffmp_policy_field(R(cfg), -1, R(ob), p, None) == -1
    # the id entry points answer as before
    assert lib.ffmp_step_state(R(cfg), 4, 0, None, R(st), R(ob), R(out), None) == -1
    assert b"action is NULL" in lib.ffmp_last_error()
    assert lib.ffmp_step_state(R(cfg), 0, 0, p + 8, R(st), R(ob), R(out), None) == 0
    del keep


def test_ros_command_adapters():
    tw = ros_adapters.command_to_twist(0.31, -0.27)
    assert (tw.linear.x, tw.linear.y, tw.linear.z) == (0.31, 0.0, 0.0)
    assert (tw.angular.x, tw.angular.y, tw.angular.z) == (0.0, 0.0, -0.27)
    assert ros_adapters.twist_to_command(tw) == (0.31, -0.27)
    for a, (v, w) in enumerate(action_table()):
        x, y = ros_adapters.command_to_twist(*action_table()[a]), ros_adapters.action_to_twist(a)
        for part in ("linear", "angular"):
            for axis in ("x", "y", "z"):
                fx, fy = getattr(getattr(x, part), axis), getattr(getattr(y, part), axis)
                assert fx == fy and type(fx) is type(fy) and np.signbit(fx) == np.signbit(fy), (a, part, axis)
        assert ros_adapters.twist_to_command(y) == (v, w)
    # duck-typed: any object with linear.x / angular.z; the other fields are not read
    m = ros_adapters.Msg(linear={"x": np.float32(0.5)}, angular={"z": 1})
    v, w = ros_adapters.twist_to_command(m)
    assert (v, w) == (0.5, 1.0) and type(v) is float and type(w) is float


def _vec_shell(n):
    """An FFMPVec with only what the input validation reads (no device, no library)."""
    env = object.__new__(FFMPVec)
    env.num_envs, env.device = n, torch.device("cpu")
    return env


def test_vec_env_input_dispatch():
    env = _vec_shell(4)
    a, is_cmd = env._act_in(torch.tensor([1, 2, 3, 4]))
    assert not is_cmd and a.dtype == torch.int64 and a.shape == (4,)
    a, is_cmd = env._act_in(np.array([[1], [2], [3], [4]], dtype=np.int32))  # N integers in any shape, as before
    assert not is_cmd and a.tolist() == [1, 2, 3, 4]
    a, is_cmd = env._act_in([5, 6, 7, 8])
    assert not is_cmd and a.tolist() == [5, 6, 7, 8]
    c32 = torch.tensor([[0.1, -0.3], [0.6, 0.6], [0.25, 0.0], [-1.0, 2.0]], dtype=torch.float32)
    c, is_cmd = env._act_in(c32)
    assert is_cmd and c.dtype == torch.float64 and c.shape == (4, 2) and c.is_contiguous()
    assert torch.equal(c, c32.double()) and c.data_ptr() % 16 == 0  # float32 widened exactly
    c64 = c32.double()
    c, is_cmd = env._act_in(c64)
    assert is_cmd and c.data_ptr() == c64.data_ptr()  # already in the kernel's layout: no copy
    c, _ = env._act_in(np.asarray(c64))
    assert torch.equal(c, c64)
    t = torch.arange(16, dtype=torch.float64).reshape(4, 4)[:, 1:3]  # a strided view is made contiguous
    c, _ = env._act_in(t)
    assert c.is_contiguous() and torch.equal(c, t)
    flat = torch.zeros(10, dtype=torch.float64)  # an 8-byte aligned view is moved to a 16-byte boundary
    odd = flat[1:9].view(4, 2) if flat.data_ptr() % 16 == 0 else flat[0:8].view(4, 2)
    odd = flat[1:9].view(4, 2) if odd.data_ptr() % 16 == 0 else odd
    c, _ = env._act_in(odd)
    assert c.data_ptr() % 16 == 0 and torch.equal(c, odd)
    for bad in (torch.zeros(4, dtype=torch.float64),          # float ids
                torch.zeros((4, 3), dtype=torch.float64),
                torch.zeros((2, 4), dtype=torch.float64),
                torch.zeros((8,), dtype=torch.float32),       # N * 2 elements, not (N, 2)
                torch.zeros((4, 2), dtype=torch.float16),
                torch.zeros((3, 2), dtype=torch.float64),
                torch.zeros((4, 2), dtype=torch.complex64),
                torch.zeros(5, dtype=torch.int64),
                torch.zeros((4, 2), dtype=torch.int64)):      # 2N integers are not N ids
        with pytest.raises(ValueError):
            env._act_in(bad)
    # N = 2: the dtype decides between two ids and ... nothing else: a float (2,) is not (N, 2)
    two = _vec_shell(2)
    assert not two._act_in(torch.tensor([3, 4]))[1]
    with pytest.raises(ValueError):
        two._act_in(torch.tensor([0.3, 0.4]))
    assert two._act_in(torch.tensor([[0.3, 0.4], [0.1, 0.2]]))[1]


def test_command_spaces():
    env = _vec_shell(3)
    one, many = env.single_command_space, env.command_space
    assert one.dtype == np.float32 and one.shape == (2,) and many.shape == (3, 2) and many.dtype == np.float32
    assert np.array_equal(one.low, np.float32([0.0, -0.6])) and np.array_equal(one.high, np.float32([0.6, 0.6]))
    assert np.array_equal(many.low, np.tile(one.low, (3, 1))) and np.array_equal(many.high, np.tile(one.high, (3, 1)))
    lo, hi = action_table()[0], action_table()[27]
    assert np.array_equal(one.low, np.float32(lo)) and np.array_equal(one.high, np.float32(hi))
    s = many.sample()
    assert s.shape == (3, 2) and s.dtype == np.float32 and many.contains(s)
    assert env._act_in(s)[1]  # a sample is what step() takes
    from flow_field_based_motion_planner_amd._spaces import Discrete, MultiDiscrete
    assert isinstance(env.single_action_space, Discrete) and isinstance(env.action_space, MultiDiscrete)


def test_single_env_input_validation():
    env = FFMP(FFMPConfig(grid=32, n_obst=0, n_beams=0), device="cpu")
    assert FFMP._action_in(5) == (5, None)
    assert FFMP._action_in(np.int64(27)) == (27, None)
    assert FFMP._action_in(np.array([4])) == (4, None)
    for bad in (28, -1):
        with pytest.raises(IndexError):
            FFMP._action_in(bad)
    s = env.action_space.sample()
    assert s.shape == (2,) and s.dtype == np.float32
    a, cmd = FFMP._action_in(s)
    assert a is None and cmd.shape == (1, 2) and cmd.dtype == np.float64 and np.array_equal(cmd[0], s.astype(np.float64))
    for form in ([0.2, -0.4], (0.2, -0.4), np.array([0.2, -0.4]), torch.tensor([0.2, -0.4], dtype=torch.float64)):
        a, cmd = FFMP._action_in(form)
        assert a is None and np.array_equal(cmd, [[0.2, -0.4]])
    a, cmd = FFMP._action_in(np.array([np.inf, -np.inf]))  # clipped by the step, not refused
    assert a is None and np.isinf(cmd).all()
    for nan in ([np.nan, 0.1], [0.2, np.nan]):
        with pytest.raises(ValueError, match="NaN"):
            FFMP._action_in(nan)
    for bad in ([0.1, 0.2, 0.3], [1, 2], np.zeros((2, 2))):
        with pytest.raises(ValueError):
            FFMP._action_in(bad)
    with pytest.raises(RuntimeError):  # the reset check still comes first
        env.step(s)
