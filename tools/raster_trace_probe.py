"""Where a two-launch raster block's time goes before its first wave task: wall-clock stamps (100 MHz)
from a probe build of libffmp (-DFFMP_TRACE: `make probe V=trace DEFS=-DFFMP_TRACE`; never the shipped
library).  Stamps of thread 0 of each of the first 65,536 blocks: 3 kernel entry, 0 old tags staged
(staged form only), 1 record read (staged form: behind the barrier; FFMP_RASTER_DIRECT: behind its one
wait), 2 block done; and of lane 0 of each wave on either side of the staged form's barrier.  Every stamp
drains the wave's memory counters first, so the build runs slower than the shipped one and the gaps are
the chain's latency.  Prints, per launch form, the prologue's share of a block's life and the waves' wait
at the barrier.
usage: FFMP_LIB=tools/_probe/libffmp_trace.so python tools/raster_trace_probe.py [preset] [n_envs] [cells] [flags ...]"""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from flow_field_based_motion_planner_amd import _abi  # noqa: E402
from flow_field_based_motion_planner_amd.config import PRESETS, preset  # noqa: E402
from flow_field_based_motion_planner_amd.vec_env import FFMPVec  # noqa: E402

name = sys.argv[1] if len(sys.argv) > 1 else "C3"
n = int(sys.argv[2]) if len(sys.argv) > 2 else PRESETS[name]["n_envs"]
cells = int(sys.argv[3]) if len(sys.argv) > 3 else 16384
base = _abi.RASTER_NT | _abi.RASTER_TILE2
forms = [int(a) for a in sys.argv[4:]] or [base | _abi.RASTER_WAVES, base | _abi.RASTER_DIRECT]
lib = _abi.load()
lib.ffmp_trace_read.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
lib.ffmp_trace_read_waves.argtypes = [C.c_void_p, C.c_int]
env_t = np.zeros((4096, 12), np.uint64)
ras_t = np.zeros((65536, 4), np.uint64)
wav_t = np.zeros((65536, 4, 2), np.uint64)


def read():
    lib.ffmp_trace_read(env_t.ctypes.data, ras_t.ctypes.data, 1)
    lib.ffmp_trace_read_waves(wav_t.ctypes.data, 1)


def line(nm, d):
    d = d * 0.01  # ticks -> us
    print(f"   {nm:34s} median {np.median(d):7.2f}  p10 {np.percentile(d, 10):7.2f}  p90 {np.percentile(d, 90):7.2f}  "
          f"max {d.max():7.2f} us")


env = FFMPVec(n, preset(name), device="cuda:0",
              tuning={"shape": [cells, forms[0]], "shape_newest": [cells, forms[0]], "fused": False, "fused_flags": _abi.RASTER_NT})
assert env.frame_tags is not None, "the probe is about the tagged raster"
gen = torch.Generator(device="cuda:0").manual_seed(1000)
acts = torch.randint(0, 28, (2 * env.frame_window + 2, n), device="cuda:0", dtype=torch.int64, generator=gen)
print(f"{name}, {n} envs, W = {env.frame_window} ({env.ring}), {cells}-cell blocks; two eager steps per form after "
      f"{2 * env.frame_window} warm-up steps", flush=True)
for flags in forms:
    env.raster_shape = env.raster_shape_newest = (cells, flags)
    obs = C.cast(C.byref(env._obs_c), C.POINTER(_abi.ObsT))
    direct = env.lib.ffmp_raster_direct(C.byref(env._cfg_c), obs, cells, flags)
    waves = env.lib.ffmp_raster_waves(C.byref(env._cfg_c), obs, flags)
    env.reset()
    for k in range(2 * env.frame_window):
        env.step(acts[k])
    torch.cuda.synchronize()
    read()
    for rep in range(2):
        env.step(acts[2 * env.frame_window + rep])
        torch.cuda.synchronize()
        read()
        R = ras_t.astype(np.int64)
        R = R[(R[:, 2] > 0) & (R[:, 3] > 0)]
        life, pro = R[:, 2] - R[:, 3], R[:, 1] - R[:, 3]
        print(f"flags {flags} ({'direct' if direct else 'staged'} form, W = {waves}) step {rep}: launch span "
              f"{(R[:, 2].max() - R[:, 3].min()) * 0.01:.1f} us over {len(R)} stamped blocks")
        line("block life (entry -> done)", life)
        line("prologue (entry -> record read)", pro)
        if not direct:
            line("  entry -> old tags staged", R[:, 0] - R[:, 3])
            line("  tags staged -> behind the barrier", R[:, 1] - R[:, 0])
        print(f"   prologue share of block life: {pro.sum() / life.sum():.3f}")
        if not direct:
            Wv = wav_t.astype(np.int64)
            Wv = Wv[(Wv[:, :, 0] > 0).all(1) & (Wv[:, :, 1] > 0).all(1)]
            wait = Wv[:, :, 1] - Wv[:, :, 0]
            for w in range(4):
                line(f"wave {w}: wait at the barrier", wait[:, w])
            line("arrival spread (last - first wave)", Wv[:, :, 0].max(1) - Wv[:, :, 0].min(1))
            print(f"   mean wait per wave {wait.mean() * 0.01:.2f} us = {wait.mean() / life.mean():.3f} of a block's life")
env.close()
