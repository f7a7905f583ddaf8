"""The physics cases (tests/physics_cases.py) on the CPU: the C oracle equals the NumPy oracle bit
for bit at every case, every case shows the events it is there for (on the NumPy oracle alone), and
FFMPConfig / check_cfg refuse the constants no kernel is safe at."""
import ctypes as C
import math

import numpy as np
import pytest

from flow_field_based_motion_planner_amd import _abi
from flow_field_based_motion_planner_amd.config import FFMPConfig
from oracle import ffmp_oracle_c as oc
from oracle.ffmp_oracle import OracleVecEnv
from tests.parity_util import same_bits
from tests.physics_cases import PHYSICS, SCALES, actions, check_floors, count_events


@pytest.fixture(scope="module")
def oracle_runs():
    """name -> event counts of the NumPy oracle over the case's run, each case run once on first use
    (with the C oracle beside it, compared bit for bit at every step)."""
    oc.build()
    cache = {}

    def run(name):
        if name not in cache:
            cfg, n, steps = PHYSICS[name]
            ref = OracleVecEnv(cfg, n)
            got = oc.COracleVecEnv(cfg, n, threads=3)
            ref.reset()
            got.reset()
            same_bits(got, ref, f"{name} reset")
            counts = {}
            for k, a in enumerate(actions(n, steps)):
                ref.step(a)
                got.step(a)
                same_bits(got, ref, f"{name} step {k}")
                count_events(counts, ref.done, ref.collision, ref.is_goal, ref.truncated,
                             ref.lidar if cfg.n_beams else None)
            cache[name] = counts
        return cache[name]
    return run


@pytest.mark.parametrize("name", list(PHYSICS))
def test_c_oracle_equals_numpy_oracle(name, oracle_runs):
    oracle_runs(name)


@pytest.mark.parametrize("name", list(PHYSICS))
def test_case_is_not_vacuous(name, oracle_runs):
    counts = oracle_runs(name)
    print(name, counts)
    check_floors(name, counts)
    cfg, n, steps = PHYSICS[name]
    if name in SCALES:
        assert len(cfg.footprint) == SCALES[name]["n_foot"]
        assert math.isclose(cfg.res / cfg.dt, SCALES[name]["quantum"], rel_tol=1e-12)
        assert min(3 + round(0.25 / cfg.res), cfg.grid // 2 - 1) == SCALES[name]["lookahead"]
    if name == "dt0":  # nothing but the step counter moves: every episode runs into max_steps
        assert counts["truncated"] == n * (steps // cfg.max_steps) and counts["collision"] == counts["goal"] == 0
    if name == "thin_margin":
        assert cfg.cull_margin == cfg.cull_floor() and 1e-4 < cfg.cull_margin < 2e-4
    if name == "all_reach":  # rho0 beyond the plane's diagonal plus every disc: no cell is out of any disc's reach
        assert cfg.rho0 > cfg.grid * cfg.res and cfg.rho_lo == 4 * cfg.res


def test_collide_modes_differ(oracle_runs):
    assert oracle_runs("mode1")["collision"] != oracle_runs("mode2")["collision"]


# ---------------------------------------------------------------- refusals
FINITE_FIELDS = ("res", "dt", "robot_r", "goal_thr", "world_half", "lidar_max", "k_att", "k_rep", "rho0", "rho_min",
                 "cull_margin")


@pytest.mark.parametrize("field", FINITE_FIELDS)
@pytest.mark.parametrize("value", [float("nan"), float("inf"), float("-inf")])
def test_config_refuses_non_finite(field, value):
    with pytest.raises(ValueError, match=field):
        FFMPConfig(grid=64, **{field: value})


@pytest.mark.parametrize("field,value", [("rho0", 0.0), ("rho0", -0.5), ("lidar_max", -1.0), ("robot_r", -0.1),
                                         ("cull_margin", 0.0), ("cull_margin", -0.1), ("cull_margin", 1e-5)])
def test_config_refuses_unsafe(field, value):
    with pytest.raises(ValueError, match=field):
        FFMPConfig(grid=64, **{field: value})


def test_cull_floor_scales():
    """2^-16 (G res / 2 + world_half + rho0 + obst_rmax): 3e-4 m at C3, 1.5e-3 m at `metres`; the
    floor itself passes, one part in a thousand below it does not, the default passes everywhere."""
    from flow_field_based_motion_planner_amd.config import preset
    c3 = preset("C3")
    assert c3.cull_floor() == 2.0 ** -16 * (6.4 + 12.8 + 0.5 + 0.3) and 2.9e-4 < c3.cull_floor() < 3.2e-4
    assert 1.4e-3 < PHYSICS["metres"][0].cull_floor() < 1.6e-3
    for cfg, _, _ in PHYSICS.values():
        assert cfg.cull_floor() < 0.1
        ok = cfg.replace(cull_margin=cfg.cull_floor())
        assert ok.cull_margin == cfg.cull_floor()
        with pytest.raises(ValueError, match="cull_margin"):
            cfg.replace(cull_margin=cfg.cull_floor() * 0.999)
    FFMPConfig(grid=4096, n_beams=0)  # the largest grid at the default margin


def test_dt_zero_is_a_valid_step_config():
    assert FFMPConfig(grid=32, dt=0.0).dt == 0.0
    with pytest.raises(ValueError):
        FFMPConfig(grid=32, dt=-0.1)


def _check(lib, c):
    """check_cfg through an entry point that launches nothing."""
    return lib.ffmp_step_skewed_check(C.byref(c), _abi.OBS_F32, 0)


def test_library_accepts_every_case(lib):
    for name, (cfg, _, _) in PHYSICS.items():
        c = _abi.make_cfg(cfg.replace(flow=False, n_beams=0))  # the skewed step takes no flow planes; no beam table here
        assert _check(lib, c) == 0, (name, lib.ffmp_last_error())


LIB_BAD = [(f, v, f.encode()) for f in ("res", "dt", "robot_r", "goal_thr", "world_half", "lidar_max")
           for v in (float("nan"), float("inf"))] + \
          [("half_ka_f", float("nan"), b"k_att"), ("half_kr_f", float("inf"), b"k_rep"),
           ("rho0_f", float("nan"), b"rho0"), ("rho0_f", float("inf"), b"rho0"), ("rho0_f", 0.0, b"rho0"),
           ("rho0_f", -0.5, b"rho0"), ("rho_min_f", float("nan"), b"rho_min"),
           ("cull_margin_f", float("nan"), b"cull_margin"), ("cull_margin_f", float("inf"), b"cull_margin"),
           ("cull_margin_f", 0.0, b"cull_margin"), ("cull_margin_f", -0.1, b"cull_margin"),
           ("cull_margin_f", 1e-5, b"cull_margin"), ("lidar_max", -1.0, b"lidar_max"), ("robot_r", -0.1, b"robot_r"),
           ("res", 0.0, b"res"), ("dt", -0.1, b"dt")]


@pytest.mark.parametrize("field,value,word", LIB_BAD)
def test_library_refuses_unsafe(lib, field, value, word):
    c = _abi.make_cfg(FFMPConfig(grid=64, n_obst=4, n_beams=0))
    assert _check(lib, c) == 0
    setattr(c, field, value)
    assert _check(lib, c) == -3, (field, value)
    assert word in lib.ffmp_last_error(), lib.ffmp_last_error()


def test_library_floor_is_not_stricter_than_the_config(lib):
    """A margin FFMPConfig accepts passes check_cfg (which knows rho0 and the margin as float32
    only), at every case's scale; half the floor does not."""
    for name, (cfg, _, _) in PHYSICS.items():
        c = _abi.make_cfg(cfg.replace(flow=False, n_beams=0, cull_margin=cfg.cull_floor()))
        assert _check(lib, c) == 0, (name, lib.ffmp_last_error())
        c.cull_margin_f = 0.5 * cfg.cull_floor()
        assert _check(lib, c) == -3 and b"cull_margin" in lib.ffmp_last_error(), name


def test_library_refuses_dt_zero_where_it_divides(lib):
    """ffmp_policy_field and the follower of ffmp_nav_field / ffmp_nav_field_tiled divide by dt: with
    dt = 0 they return FFMP_E_CFG before any launch; the planes of ffmp_nav_field alone do not need
    dt, and ffmp_scan_flow refuses the infinite scale res / (lag dt)."""
    cfg = _abi.make_cfg(PHYSICS["dt0"][0].replace(n_beams=0))
    assert _check(lib, cfg) == 0
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p).value
    p += (-p) % 16
    ob = _abi.ObsT(p, p, p, p, p, p, p)
    assert lib.ffmp_policy_field(C.byref(cfg), 4, C.byref(ob), p, None) == -3
    assert b"dt" in lib.ffmp_last_error()
    assert lib.ffmp_nav_field(C.byref(cfg), 4, C.byref(ob), p, 2, 2, 40, 4, 0.25, None, None, None, None, p, None) == -3
    assert b"dt" in lib.ffmp_last_error()
    assert lib.ffmp_nav_field(C.byref(cfg), 0, C.byref(ob), p, 2, 2, 40, 4, 0.25, None, None, None, None, None, None) == 0
    ws = (C.c_char * 1024)()
    w = C.cast(ws, C.c_void_p).value
    w += (-w) % 256
    assert lib.ffmp_nav_field_tiled(C.byref(cfg), 4, C.byref(ob), p, 2, 2, 40, 4, 0.25, None, None, None, None, p, 0, w,
                                    512, None) == -3
    assert b"dt" in lib.ffmp_last_error()
    assert lib.ffmp_scan_flow_check(C.byref(cfg), _abi.OBS_F32, float("inf"), 4, 3, 1, 3) == -1
    assert b"scale" in lib.ffmp_last_error()
    ok = _abi.make_cfg(PHYSICS["dt0"][0].replace(n_beams=0, dt=0.1))
    assert lib.ffmp_policy_field(C.byref(ok), 0, C.byref(ob), p, None) == 0
