"""The tiled navigation field without a GPU: ffmp_nav_field_tiled / _check / _workspace are declared,
bound and exported consistently inside ABI 9; every argument check answers before any launch; the
workspace grows without the caller's cost plane and is bounded by n; and the NumPy model of the
kernel's tile schedule (tests/nav_tiled_model.py) ends on the plane of tests/nav_field_ref.py."""
import ctypes as C
import re

import numpy as np
import pytest

from flow_field_based_motion_planner_amd import _abi
from flow_field_based_motion_planner_amd.config import FFMPConfig
from tests import nav_field_ref as R
from tests import nav_tiled_model as M

TILED_SYMBOLS = ("ffmp_nav_field_tiled", "ffmp_nav_field_tiled_check", "ffmp_nav_field_tiled_workspace")
E = -1  # FFMP_E_ARG


def test_header_binding_and_library_agree(lib):
    h = open(_abi.HEADER_PATH).read()
    assert int(re.search(r"#define FFMP_ABI_VERSION (\d+)", h).group(1)) == 9 == _abi.ABI_VERSION
    code = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    for name in TILED_SYMBOLS:
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, code)
        assert m, name
        params = [p.strip() for p in m.group(1).split(",")]
        res, args = _abi._SIGS[name]
        assert res is C.c_int and len(args) == len(params), (name, params)
        assert hasattr(lib, name)
    # ffmp_nav_field's arguments, then tile, workspace, workspace_bytes, with the stream last
    old, new = _abi._SIGS["ffmp_nav_field"][1], _abi._SIGS["ffmp_nav_field_tiled"][1]
    assert new[:len(old) - 1] == old[:-1] and new[len(old) - 1:] == [C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p]
    # the comment states the tiling, the workspace and the limits, and cites the SPEC rather than repeating it
    decl = h.index("int ffmp_nav_field_tiled(")
    comment = h[h.rindex("/*", 0, decl):decl]
    for word in ("SPEC above ffmp_nav_field", "512", "halo", "multiple of 32 in [32, 256]", "256-byte aligned", "slots",
                 "No workgroup waits on another"):
        assert word in comment, word
    assert "(1,0) (-1,0)" not in comment
    _abi.verify_layout(lib)


def _host_args():
    keep = (C.c_double * 80)()
    p = C.cast(keep, C.c_void_p).value
    p += (-p) % 256
    return keep, p, _abi.ObsT(p, p, p, p, p, p, p)


def _call(lib, cfg, ob, p, n=4, goal="p", stride=2, margin=2, pen=40, look=4, ts=0.25, cost=None, dirs=None, cmd=None,
          tile=0, ws="p", ws_bytes=1 << 40):
    return lib.ffmp_nav_field_tiled(C.byref(cfg), n, C.byref(ob) if ob is not None else None, p if goal == "p" else goal,
                                    stride, margin, pen, look, ts, cost, dirs, None, None, cmd, tile,
                                    p if ws == "p" else ws, ws_bytes, None)


def test_argument_checks_without_a_launch(lib):
    cfg = _abi.make_cfg(FFMPConfig(grid=64, n_obst=4, n_beams=0))
    keep, p, ob = _host_args()
    for g in (4, 516, 1024, 66):  # outside 8..512, or not a multiple of 4
        bad = _abi.make_cfg(FFMPConfig(grid=64, n_obst=4, n_beams=0))
        bad.grid = g
        assert _call(lib, bad, ob, p) == E and b"grid" in lib.ffmp_last_error(), g
        assert lib.ffmp_nav_field_tiled_check(C.byref(bad), 0, 2, 40, 4, 0) == E
    # everything the untiled entry refuses, and the tile and the workspace
    for kw, word in ((dict(margin=-1), b"margin"), (dict(margin=9), b"margin"), (dict(pen=-1), b"soft_pen"),
                     (dict(pen=16385), b"soft_pen"), (dict(look=0), b"lookahead"), (dict(look=65), b"lookahead"),
                     (dict(ts=float("nan")), b"turn_sin"), (dict(ts=-0.1), b"turn_sin"), (dict(goal=None), b"goal_ego"),
                     (dict(stride=1), b"goal_stride"), (dict(cmd=p + 8), b"16-byte aligned"), (dict(n=-1), b"negative n"),
                     (dict(cost=p + 4), b"8-byte aligned"), (dict(dirs=p + 2), b"4-byte aligned"),
                     (dict(tile=16), b"tile"), (dict(tile=48), b"tile"), (dict(tile=288), b"tile"), (dict(tile=-32), b"tile"),
                     (dict(ws=None), b"workspace is NULL"), (dict(ws=p + 128), b"256-byte aligned"),
                     (dict(ws_bytes=0), b"workspace too small"), (dict(ws_bytes=4096), b"workspace too small")):
        assert _call(lib, cfg, ob, p, **kw) == E, kw
        assert word in lib.ffmp_last_error(), (kw, lib.ffmp_last_error())
        assert lib.ffmp_last_error().startswith(b"ffmp_nav_field_tiled:")
    no_frames = _abi.ObsT(None, p, p, p, p, p, p)
    assert _call(lib, cfg, no_frames, p) == E and b"state_m" in lib.ffmp_last_error()
    assert _call(lib, cfg, None, p) == E
    # the bounds themselves pass the checks: n == 0 launches nothing
    for kw in (dict(margin=0), dict(margin=8), dict(pen=0), dict(pen=16384), dict(look=1), dict(look=64), dict(ts=0.0),
               dict(cmd=p), dict(cost=p, dirs=p), dict(tile=0), dict(tile=32), dict(tile=256), dict(tile=96), dict(ws_bytes=0)):
        assert _call(lib, cfg, ob, p, n=0, **kw) == 0, kw
    for tile, ok in ((0, True), (32, True), (256, True), (16, False), (48, False), (288, False)):
        assert (lib.ffmp_nav_field_tiled_check(C.byref(cfg), 0, 2, 40, 4, tile) == 0) == ok, tile
    assert lib.ffmp_nav_field_tiled_check(C.byref(cfg), 2, 2, 40, 4, 0) == E and b"format" in lib.ffmp_last_error()
    assert lib.ffmp_nav_field_tiled_check(C.byref(cfg), 0, 9, 40, 4, 0) == E
    assert lib.ffmp_nav_field_tiled_check(None, 0, 2, 40, 4, 0) == E
    del keep


def test_large_grids_pass_the_tiled_check_and_not_the_untiled(lib):
    keep, p, ob = _host_args()
    for g in (8, 100, 256, 260, 512):
        cfg = _abi.make_cfg(FFMPConfig(grid=g, n_obst=0, n_beams=0))
        for tile in (0, 32, 256):
            assert lib.ffmp_nav_field_tiled_check(C.byref(cfg), 0, 2, 40, 4, tile) == 0, (g, tile, lib.ffmp_last_error())
            assert lib.ffmp_nav_field_tiled_check(C.byref(cfg), 1, 0, 0, 1, tile) == 0
        assert _call(lib, cfg, ob, p, n=0) == 0
        assert (lib.ffmp_nav_field_check(C.byref(cfg), 0, 2, 40, 4) == 0) == (g <= 256), g
    del keep


def _workspace(lib, g, n, tile, with_cost):
    cfg = _abi.make_cfg(FFMPConfig(grid=g, n_obst=0, n_beams=0))
    b = C.c_size_t(12345)
    assert lib.ffmp_nav_field_tiled_workspace(C.byref(cfg), n, tile, with_cost, C.byref(b)) == 0, lib.ffmp_last_error()
    return b.value


def test_workspace_bytes(lib):
    for g in (64, 260, 512):
        words = g * ((g + 31) // 32)
        masks, plane = -(-2 * 4 * words // 256) * 256, -(-2 * g * g // 256) * 256
        for tile in (0, 32):
            assert _workspace(lib, g, 0, tile, 0) == 0
            assert _workspace(lib, g, 1, tile, 1) == masks      # one slot: the two masks
            assert _workspace(lib, g, 1, tile, 0) == masks + plane  # and the plane the caller does not give
            for n in (3, 1 << 20):
                with_cost, without = _workspace(lib, g, n, tile, 1), _workspace(lib, g, n, tile, 0)
                slots = with_cost // masks
                assert 1 <= slots <= min(n, 2048) and with_cost == slots * masks and without == slots * (masks + plane)
            assert _workspace(lib, g, 3, tile, 0) == 3 * (masks + plane)  # bounded by n
    cfg = _abi.make_cfg(FFMPConfig(grid=64, n_obst=0, n_beams=0))
    b = C.c_size_t()
    assert lib.ffmp_nav_field_tiled_workspace(C.byref(cfg), 4, 48, 0, C.byref(b)) == E and b"tile" in lib.ffmp_last_error()
    assert lib.ffmp_nav_field_tiled_workspace(C.byref(cfg), -1, 0, 0, C.byref(b)) == E
    assert lib.ffmp_nav_field_tiled_workspace(C.byref(cfg), 4, 0, 0, None) == E
    assert lib.ffmp_nav_field_tiled_workspace(None, 4, 0, 0, C.byref(b)) == E


def test_python_surface_takes_a_tile():
    import inspect
    from flow_field_based_motion_planner_amd import vec_env
    for name in ("nav_field", "policy_nav"):
        assert inspect.signature(getattr(vec_env.FFMPVec, name)).parameters["tile"].default is None
    assert vec_env.FFMPVec.nav_tile is None and callable(vec_env.FFMPVec.nav_workspace_bytes)
    assert "512 x 512" in vec_env.FFMPVec.nav_field.__doc__


# ------------------------------------------------------------------ the schedule's model
def _ringed(G):
    c = G // 2
    m = np.zeros((G, G), np.float32)
    m[c - 6:c + 7, c - 6] = m[c - 6:c + 7, c + 6] = m[c - 6, c - 6:c + 7] = m[c + 6, c - 6:c + 7] = 255.0
    return m, (c + 20, c - 3)


@pytest.mark.parametrize("scene,G,tile", [("serpentine", 64, 32), ("serpentine", 100, 32), ("ringed", 64, 32),
                                          ("serpentine", 64, 0)])
@pytest.mark.parametrize("knobs", [dict(margin=0, soft_pen=40), dict(margin=2, soft_pen=40)])
def test_tile_schedule_model_reaches_the_fixed_point(scene, G, tile, knobs):
    """Tile-local fixed points against read-only halos, the kernel's work-list and dirty rule: the
    plane is Dijkstra's bit for bit, within the kernel's bound on tile visits.  G = 100 at tile 32:
    4 x 4 tiles, the last row and column 4 cells wide; tile 0 at G = 64: one tile, one visit."""
    cfg = FFMPConfig(grid=G, n_obst=0, n_beams=0)
    frame, q = R.serpentine(G) if scene == "serpentine" else _ringed(G)
    hard, soft = R.cell_classes(frame, cfg.footprint, knobs["margin"], q)
    want = R.cost_to_go(hard, soft, q, knobs["soft_pen"])
    got, visits, order = M.tiled_cost_to_go(hard, soft, q, knobs["soft_pen"], tile)
    nt = -(-G // M.tile_edge(G, tile))
    print(scene, G, tile, knobs, "tiles", nt * nt, "visits", visits)
    assert got.dtype == want.dtype and np.array_equal(got, want)
    assert visits < M.visit_bound(G) and order[0] == (q[0] // M.tile_edge(G, tile)) * nt + q[1] // M.tile_edge(G, tile)
    if nt == 1:
        assert visits == 1
    else:
        assert visits > nt * nt or scene == "ringed"  # the maze's corridors cross tile edges: tiles come due again
