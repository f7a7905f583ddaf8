"""Granule tags (ffmp_obs_tags_t, FFMP_OBS_EXT_TAGS) without a GPU: the extension leaves ABI 9, every
existing struct and every existing ffmp_layout value as they were; the new selectors agree with the
ctypes struct; a plain ffmp_obs_t with reserved == 0 passes the argument checks as before, and the
flag's own checks answer before any launch."""
import ctypes as C
import re

from flow_field_based_motion_planner_amd import _abi
from flow_field_based_motion_planner_amd.config import FFMPConfig

# ffmp_layout(0 .. 9) of ABI 9 as released: sizeof cfg / state / obs / out, four cfg offsets,
# sizeof(ffmp_episode_t), offsetof(ffmp_obs_t, format)
LAYOUT_ABI9 = {0: 1224, 1: 88, 2: 88, 3: 40, 4: 1064, 5: 1168, 6: 1208, 7: 1216, 8: 72, 9: 80}

RASTERING = ("ffmp_raster", "ffmp_raster_ex", "ffmp_step", "ffmp_step_cmd", "ffmp_step_fused", "ffmp_step_fused_cmd",
             "ffmp_step_skewed")


def _code():
    return re.sub(r"/\*.*?\*/", "", open(_abi.HEADER_PATH).read(), flags=re.S)


def test_abi_version_and_existing_layout_unchanged(lib):
    code = _code()
    assert int(re.search(r"#define FFMP_ABI_VERSION (\d+)", code).group(1)) == 9 == _abi.ABI_VERSION
    assert lib.ffmp_abi_version() == 9
    assert C.sizeof(_abi.ObsT) == 88 == lib.ffmp_layout(2)
    for k, v in LAYOUT_ABI9.items():
        assert lib.ffmp_layout(k) == v, k
    # the ctypes structs say the same (CfgT through verify_layout's offsets)
    assert (C.sizeof(_abi.CfgT), C.sizeof(_abi.StateT), C.sizeof(_abi.OutT), C.sizeof(_abi.EpisodeT)) == \
        (LAYOUT_ABI9[0], LAYOUT_ABI9[1], LAYOUT_ABI9[3], LAYOUT_ABI9[8])
    assert len(_abi.ObsT._fields_) == 12 and _abi.ObsT._fields_[-1][0] == "reserved"
    # the selectors between the old ones and the extension's stay unknown
    for k in list(range(10, 20)) + [22, -1]:
        assert lib.ffmp_layout(k) == -1, k
    _abi.verify_layout(lib)


def test_new_selectors_agree_with_the_binding(lib):
    T = _abi.ObsTagsT
    assert lib.ffmp_layout(20) == C.sizeof(T) == 88 + 24
    assert lib.ffmp_layout(21) == T.tags_older.offset == 88
    assert (T.tags_newest.offset, T.tags_env_stride.offset) == (96, 104)
    # the ffmp_obs_t is the first member: every ObsT field sits where it sits in an ObsT
    for name, _ in _abi.ObsT._fields_:
        assert getattr(T, name).offset == getattr(_abi.ObsT, name).offset, name
    code = _code()
    m = re.search(r"typedef struct ffmp_obs_tags \{(.*?)\} ffmp_obs_tags_t;", code, re.S)
    members = [ln.strip().rstrip(";") for ln in m.group(1).strip().splitlines() if ln.strip()]
    assert members == ["ffmp_obs_t obs", "uint8_t* tags_older", "uint8_t* tags_newest", "int64_t tags_env_stride"]
    assert int(re.search(r"#define FFMP_OBS_EXT_TAGS (\d+)", code).group(1)) == 1 == _abi.OBS_EXT_TAGS
    assert int(re.search(r"#define FFMP_TAG_CELLS (\d+)", code).group(1)) == 64 == _abi.TAG_CELLS
    # no entry point changed its signature for it
    for name in RASTERING:
        assert _abi._SIGS[name][1].count(C.POINTER(_abi.ObsT)) == 1, name


def _host_args():
    dummy = (C.c_double * 16)()
    p = C.cast(dummy, C.c_void_p).value
    p += (-p) % 16
    st = _abi.StateT(p, p, p, p, p, p, p, p, p)
    out = _abi.OutT(p, p, p, p, p)
    return dummy, p, st, out


def _calls(lib, cfg, n, p, st, ob, out):
    """Every launch that rasters, with host pointers: only n == 0 or a failing check is safe."""
    R = C.byref
    return {
        "ffmp_raster": lambda: lib.ffmp_raster(R(cfg), n, p, None, R(ob), None),
        "ffmp_raster_ex": lambda: lib.ffmp_raster_ex(R(cfg), n, p, None, R(ob), 0, 0, None),
        "ffmp_step": lambda: lib.ffmp_step(R(cfg), n, 0, p, R(st), R(ob), R(out), None),
        "ffmp_step_cmd": lambda: lib.ffmp_step_cmd(R(cfg), n, 0, p, R(st), R(ob), R(out), None),
        "ffmp_step_fused": lambda: lib.ffmp_step_fused(R(cfg), n, 0, p, R(st), R(ob), R(out), 0, None),
        "ffmp_step_fused_cmd": lambda: lib.ffmp_step_fused_cmd(R(cfg), n, 0, p, R(st), R(ob), R(out), 0, None),
        "ffmp_step_skewed": lambda: lib.ffmp_step_skewed(R(cfg), n, 0, p, R(st), R(ob), R(out), p + 64, 0, 0, None),
    }


def test_plain_obs_passes_the_checks_as_before(lib):
    """A C caller's stand-alone ffmp_obs_t, reserved = 0: nothing behind it is looked at."""
    cfg = _abi.make_cfg(FFMPConfig(grid=64, n_obst=4, n_beams=0))
    keep, p, st, out = _host_args()
    ob = _abi.ObsT(p, p, p, p, p, p, p)
    assert ob.reserved == 0 and C.sizeof(ob) == 88
    for name, call in _calls(lib, cfg, 0, p, st, ob, out).items():
        assert call() == 0, (name, lib.ffmp_last_error())
    del keep


def test_flag_checks_answer_before_any_launch(lib):
    cfg = _abi.make_cfg(FFMPConfig(grid=64, n_obst=4, n_beams=0))
    keep, p, st, out = _host_args()
    T = 64 * 64 // 64

    def tagged(older, newest, stride, fmt=_abi.OBS_F32):
        ob = _abi.ObsTagsT(p, p, p, p, p, p, p)
        ob.format, ob.reserved = fmt, _abi.OBS_EXT_TAGS
        ob.tags_older, ob.tags_newest, ob.tags_env_stride = older, newest, stride
        return ob

    # well-formed: accepted (n == 0: nothing launched)
    for name, call in _calls(lib, cfg, 0, p, st, tagged(p, p + 8, T), out).items():
        assert call() == 0, (name, lib.ffmp_last_error())
    # a NULL tag pointer, a stride below the tags of one frame, the compact format: FFMP_E_ARG, n > 0 included
    for n in (0, 4):
        for ob, word in ((tagged(None, p, T), b"NULL"), (tagged(p, None, T), b"NULL"),
                         (tagged(p, p, T - 1), b"tags_env_stride"), (tagged(p, p, T, _abi.OBS_U8F16), b"FFMP_OBS_F32")):
            for name, call in _calls(lib, cfg, n, p, st, ob, out).items():
                if name == "ffmp_step_skewed" and ob.format != _abi.OBS_F32:
                    assert call() == -1  # (its own format check answers first)
                    continue
                assert call() == -1, name
                msg = lib.ffmp_last_error()
                assert b"FFMP_OBS_EXT_TAGS" in msg and word in msg, (name, msg)
    del keep
