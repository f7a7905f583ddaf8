"""Injected episodes (SPEC a16b), the host side: the header's new entry point within ABI 9, its
ctypes binding, ros_adapters.pose_array_to_scenario and set_scenarios' argument check
(vec_env.scenario_tensors) — none of it needs a GPU."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from flow_field_based_motion_planner_amd import _abi
from flow_field_based_motion_planner_amd.config import FFMPConfig
from flow_field_based_motion_planner_amd.ros_adapters import pose_array_to_scenario
from flow_field_based_motion_planner_amd.vec_env import FFMPVec, scenario_tensors


def _header():
    with open(_abi.HEADER_PATH) as f:
        return f.read()


def test_header_declares_set_scenario_within_abi_9():
    h = _header()
    assert re.search(r"#define\s+FFMP_ABI_VERSION\s+9\b", h)
    m = re.search(r"\bint\s+ffmp_set_scenario\s*\(([^;]*)\)\s*;", h)
    assert m, "ffmp_set_scenario is not declared"
    args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    names = [a.split()[-1].lstrip("*") for a in args.split(",")]
    assert names == ["cfg", "n", "env_offset", "mask", "pose", "goal", "obst", "obst_r", "episode", "state", "obs",
                     "stream"]
    assert "within ABI 9" in h
    assert "value 4: bad scenario" in h


def test_abi_binds_set_scenario():
    assert _abi.ABI_VERSION == 9
    res, args = _abi._SIGS["ffmp_set_scenario"]
    assert res is C.c_int and len(args) == 12
    assert args[0] == C.POINTER(_abi.CfgT) and args[9] == C.POINTER(_abi.StateT) and args[10] == C.POINTER(_abi.ObsT)
    assert args[1] is C.c_int64 and args[2] is C.c_int64 and all(a is C.c_void_p for a in args[3:9] + [args[11]])
    assert callable(FFMPVec.set_scenarios) and callable(FFMPVec.scenarios)


# ------------------------------------------------------------------ pose_array_to_scenario
def test_pose_array_to_scenario_pads_with_parked_discs():
    cfg = FFMPConfig(grid=64, n_obst=4, n_beams=48, world_half=2.4)
    sc = pose_array_to_scenario((0.5, -0.25, 1.0), (1.5, 0.75), [(1.0, 1.0, 0.3), (-1.0, 0.5, 0.2, 0.1, -0.2)], cfg=cfg)
    assert {k: (v.shape, v.dtype) for k, v in sc.items()} == {
        "pose": ((1, 3), np.float64), "goal": ((1, 2), np.float64), "obst": ((1, 4, 4), np.float64),
        "obst_r": ((1, 4), np.float64)}
    assert sc["pose"].tolist() == [[0.5, -0.25, 1.0]] and sc["goal"].tolist() == [[1.5, 0.75]]
    assert sc["obst"][0, 0].tolist() == [1.0, 1.0, 0.0, 0.0] and sc["obst"][0, 1].tolist() == [-1.0, 0.5, 0.1, -0.2]
    assert sc["obst_r"][0].tolist() == [0.3, 0.2, 0.0, 0.0]
    park = 3.0 * cfg.W  # the sampler's parked disc: r = 0 at (3 W, 3 W), at rest
    assert sc["obst"][0, 2:].tolist() == [[park, park, 0.0, 0.0]] * 2


def test_pose_array_to_scenario_defaults_and_errors():
    sc = pose_array_to_scenario((1, 2), (3, 4))  # integers, no yaw, no config: K = 0
    assert sc["pose"].tolist() == [[1.0, 2.0, 0.0]] and sc["pose"].dtype == np.float64
    assert sc["obst"].shape == (1, 0, 4) and sc["obst_r"].shape == (1, 0)
    assert pose_array_to_scenario((0, 0), (1, 1), [(1, 1, 0.5)])["obst"].shape == (1, 1, 4)
    cfg = FFMPConfig(grid=64, n_obst=1, n_beams=48)
    with pytest.raises(ValueError, match="2 obstacles given.*n_obst = 1"):
        pose_array_to_scenario((0, 0), (1, 1), [(1, 1, 0.5), (2, 2, 0.5)], cfg=cfg)
    with pytest.raises(ValueError):
        pose_array_to_scenario((0, 0, 0, 0), (1, 1))
    with pytest.raises(ValueError):
        pose_array_to_scenario((0, 0), (1, 1), [(1, 1)])
    # the adapter's output is what the argument check takes
    out = scenario_tensors(1, 1, **pose_array_to_scenario((0, 0), (1, 1), [(1, 1, 0.5)], cfg=cfg))
    assert out["obst"].shape == (1, 1, 4) and out["episode"] is None


# ------------------------------------------------------------------ set_scenarios' argument check
def _args(n, K, dtype=np.float64):
    return dict(pose=np.zeros((n, 3), dtype), goal=np.ones((n, 2), dtype), obst=np.zeros((n, K, 4), dtype),
                obst_r=np.zeros((n, K), dtype))


def test_scenario_tensors_widens_float32_exactly():
    a = _args(5, 3, np.float32)
    a["pose"][:] = np.float32(0.1)
    out = scenario_tensors(5, 3, **a, episode=np.arange(5))
    assert all(out[k].dtype == torch.float64 and out[k].is_contiguous() for k in ("pose", "goal", "obst", "obst_r"))
    assert out["pose"][0, 0].item() == float(np.float32(0.1))
    assert out["episode"].dtype == torch.int32 and out["episode"].tolist() == [0, 1, 2, 3, 4]
    t = scenario_tensors(5, 3, **{k: torch.as_tensor(v) for k, v in a.items()})  # tensors as well as arrays
    assert torch.equal(t["pose"], out["pose"])
    assert scenario_tensors(5, 3, **{k: v[:, ::1] for k, v in _args(5, 3).items()})["obst_r"].shape == (5, 3)


def test_scenario_tensors_without_discs():
    out = scenario_tensors(2, 0, np.zeros((2, 3)), np.zeros((2, 2)))
    assert out["obst"] is None and out["obst_r"] is None
    scenario_tensors(2, 0, np.zeros((2, 3)), np.zeros((2, 2)), np.zeros((2, 0, 4)), np.zeros((2, 0)))
    with pytest.raises(ValueError, match="obst"):
        scenario_tensors(2, 0, np.zeros((2, 3)), np.zeros((2, 2)), np.zeros((2, 1, 4)), np.zeros((2, 1)))


@pytest.mark.parametrize("key,bad", [
    ("pose", np.zeros((4, 2))), ("pose", np.zeros((5, 3))), ("pose", np.zeros(12)), ("goal", np.zeros((4, 3))),
    ("obst", np.zeros((4, 3, 3))), ("obst", np.zeros((4, 2, 4))), ("obst_r", np.zeros((4, 3, 1))),
    ("obst", None), ("obst_r", None),
    ("pose", np.zeros((4, 3), np.int64)), ("goal", np.zeros((4, 2), np.float16)), ("obst_r", np.zeros((4, 3), bool)),
    ("episode", np.zeros(3, np.int64)), ("episode", np.zeros(4)), ("episode", np.zeros((4, 1), np.int32))])
def test_scenario_tensors_rejects_bad_shapes_and_dtypes(key, bad):
    a = _args(4, 3)
    a[key] = bad
    with pytest.raises(ValueError, match=key):
        scenario_tensors(4, 3, **a)
