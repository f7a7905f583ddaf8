"""FFMP_RASTER_DIRECT without a GPU: the header and the binding agree on the bit, the bit is free, the
library holds the kernels and picks them only where the form applies, FFMPVec offers the new shapes only to
float32 envs with granule tags (and never to the one-launch step), and tuning() carries the flag."""
import ctypes as C
import json
import re

from flow_field_based_motion_planner_amd import _abi
from flow_field_based_motion_planner_amd.config import FFMPConfig
from flow_field_based_motion_planner_amd.vec_env import FFMPVec

NEW = _abi.RASTER_DIRECT


def _defines():
    code = re.sub(r"/\*.*?\*/", "", open(_abi.HEADER_PATH).read(), flags=re.S)
    return {k: int(v) for k, v in re.findall(r"#define FFMP_RASTER_(\w+) (\d+)", code)}


def test_header_and_binding_agree():
    d = _defines()
    assert d["DIRECT"] == 2048 == _abi.RASTER_DIRECT
    # the next free bit: every raster flag is a bit of its own, DIRECT the highest
    vals = sorted(d.values())
    assert len(set(vals)) == len(vals) and all(v & (v - 1) == 0 for v in vals) and vals[-1] == NEW
    assert "ffmp_raster_direct" in _abi._SIGS


def _host_env(obs_format, tags, flow=False):
    """The candidate lists need only these attributes: no device, no library."""
    e = object.__new__(FFMPVec)
    e.obs_format = obs_format
    e.frame_tags = object() if tags else None
    e.cfg = FFMPConfig(grid=64, n_obst=4, n_beams=0, flow=flow)
    return e


def test_offered_only_with_tags_in_f32_and_only_to_the_raster():
    on = _host_env("f32", True)
    shapes = on._shape_candidates()
    new = [sh for sh in shapes if sh[1] & NEW]
    assert new == list(FFMPVec.DIRECT_SHAPES)
    # each beside its staged twin (the same shape with RASTER_WAVES in the flag's place): row runs, TILE2, TILE4
    for cells, f in new:
        assert not f & _abi.RASTER_WAVES and (cells, f & ~NEW | _abi.RASTER_WAVES) in shapes, (cells, f)
    assert {f & (_abi.RASTER_TILE2 | _abi.RASTER_TILE4) for _, f in new} == {0, _abi.RASTER_TILE2, _abi.RASTER_TILE4}
    assert not [f for f in on._fused_candidates() if f & NEW]
    assert on._offered(_abi.RASTER_NT | NEW)
    for env in (_host_env("f32", False), _host_env("u8f16", False), _host_env("f32", True, flow=True)):
        assert not [sh for sh in env._shape_candidates() if sh[1] & NEW]
        assert not [f for f in env._fused_candidates() if f & NEW]
        assert not env._offered(_abi.RASTER_NT | NEW)
    # the lists without the new shapes are the ones from before the flag
    assert [sh for sh in shapes if not sh[1] & NEW] == [sh for sh in FFMPVec.RASTER_SHAPES if on._offered(sh[1])]
    assert not [sh for sh in FFMPVec.RASTER_SHAPES if sh[1] & NEW] and not [f for f in FFMPVec.FUSED_FLAGS if f & NEW]


def test_tuning_round_trip():
    """tuning() -> JSON -> _apply_tuning keeps the flag in both launch kinds (bench.py --save-tuning / --tuning)."""
    e = _host_env("f32", True)
    e.pipeline_slices, e._fused_req = 1, None
    e.raster_shape, e.raster_shape_newest = (4096, _abi.RASTER_NT | NEW), FFMPVec.DIRECT_SHAPES[2]
    e.fused, e.fused_flags = False, _abi.RASTER_NT | _abi.RASTER_WAVES
    t = json.loads(json.dumps(e.tuning()))
    o = _host_env("f32", True)
    o.pipeline_slices, o._fused_req = 1, None
    o._apply_tuning(t)
    assert o.raster_shape == e.raster_shape and o.raster_shape_newest == e.raster_shape_newest
    assert o.raster_shape_newest[1] & NEW and o.fused is False and o.fused_flags == e.fused_flags
    assert o.tuning() == e.tuning()
    assert o.placement["shape_newest"]["flags"] & NEW


def test_library_holds_and_picks_the_kernels(lib):
    """The direct kernels are in the library (store flavour x XCD remap x record alignment), and the launch's
    own decision (ffmp_raster_direct: no launch, nothing dereferenced) takes them for a tagged float32 obs
    with the flag, in row runs and 2- / 4-row tiles of the column-band-major deal, in blocks of at most
    65,536 cells, and for nothing else."""
    blob = open(_abi.LIB_PATH, "rb").read()
    names = set(re.findall(rb"_Z20raster_direct_kernelILb([01])ELb([01])ELb([01])EE", blob))
    assert len(names) == 8, names
    keep = (C.c_double * 16)()
    p = C.cast(keep, C.c_void_p).value
    p += (-p) % 16

    def ask(cfg, cells, flags, tags=True, fmt=_abi.OBS_F32):
        ob = _abi.ObsTagsT(p, p, p, p, p, p, p)
        ob.format = fmt
        if tags:
            ob.reserved = _abi.OBS_EXT_TAGS
            ob.tags_older, ob.tags_newest, ob.tags_env_stride = p, p + 8, 1 << 20
        obp = C.cast(C.byref(ob), C.POINTER(_abi.ObsT))
        return lib.ffmp_raster_direct(C.byref(cfg), obp, cells, flags), lib.ffmp_raster_waves(C.byref(cfg), obp, flags)

    def cfg(G, **kw):
        return _abi.make_cfg(FFMPConfig(grid=G, n_obst=4, n_beams=0, **kw))

    T2, T4, T8, T16, NT, W = (_abi.RASTER_TILE2, _abi.RASTER_TILE4, _abi.RASTER_TILE8, _abi.RASTER_TILE16,
                              _abi.RASTER_NT, _abi.RASTER_WAVES)
    c64, c256 = cfg(64), cfg(256)
    # the flag alone selects the form; ffmp_raster_waves keeps answering for RASTER_WAVES alone
    assert ask(c64, 4096, NT | T4 | NEW) == (1, 0) and ask(c64, 4096, NT | T4 | NEW | W) == (1, 6)
    assert ask(c64, 4096, NT | T4 | W) == (0, 6) and ask(c64, 4096, NT | T4) == (0, 0)
    for cells, f in FFMPVec.DIRECT_SHAPES + ((0, NEW), (2048, T2 | NEW), (65536, T4 | NEW | _abi.RASTER_XCD | _abi.RASTER_PLAIN)):
        assert ask(c256, cells, f)[0] == 1, (cells, f)
    # where the form does not apply: no tags, flow planes, the compact format, 8- and 16-row tiles, ...
    assert ask(c64, 4096, NT | T4 | NEW, tags=False)[0] == 0
    assert ask(c64, 4096, NT | T4 | NEW, tags=False, fmt=_abi.OBS_U8F16)[0] == 0
    assert ask(cfg(64, flow=True), 4096, NT | T4 | NEW)[0] == 0
    assert ask(c256, 16384, NT | T8 | NEW)[0] == 0 and ask(c256, 16384, NT | T16 | NEW)[0] == 0
    # ... blocks of more granules than a wave's 64 tasks hold, and tiles outside the column-band-major deal
    assert ask(cfg(512), 65536, NT | T4 | NEW)[0] == 1 and ask(cfg(512), 131072, NT | T4 | NEW)[0] == 0
    assert ask(cfg(384), 6144, NT | T2 | NEW)[0] == 0      # 3 column bands of 128
    assert ask(cfg(384), 6144, NT | NEW)[0] == 1           # its row runs
    assert ask(cfg(96), 4096, NT | T4 | NEW)[0] == 1       # tiles do not split the plane: row runs
    assert ask(cfg(768), 12288, NT | T4 | NEW)[0] == 1     # 12 column bands of 64, three per wave
    # bad arguments are refused as by the launch
    assert ask(c64, 1000, NT | NEW)[0] == -1 and b"cells_per_block" in lib.ffmp_last_error()
    ob = _abi.ObsTagsT(p, p, p, p, p, p, p)
    ob.reserved = _abi.OBS_EXT_TAGS
    assert lib.ffmp_raster_direct(C.byref(c64), C.cast(C.byref(ob), C.POINTER(_abi.ObsT)), 0, NEW) == -1
    assert b"FFMP_OBS_EXT_TAGS" in lib.ffmp_last_error()
    del keep
