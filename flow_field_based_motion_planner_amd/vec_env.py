"""FFMPVec — N batched FFMP environments resident in HBM, stepped by libffmp.

This is the new batched surface the north star asks for (the reference's
`FFMP` has no step()/reset(): src/gym_ffmp/envs/ffmp.py:77-83 is commented out
and src/train.py drives Gazebo over ROS instead, train.py:523-693).  One call of
`step(actions)` is one iteration of the reference main loop for every env:

    publish cmd_vel(commander(action))       train.py:668-673  -> unicycle integrator
    Gazebo / BEV nodes produce the next obs   train.py:116-165  -> raster + lidar kernels
    make_temporal_maps                        train.py:474-486  -> state_m [older, newest]
    rewarder2 / rewarder                      ffmp.py:167-188   -> collision, goal, reward, done
    step == MAX_STEPS -> done                 train.py:607-608  -> truncated
    done -> /episode_manager reset            train.py:611-664  -> auto-reset (Philox)

`actions` is either the N action ids (an integer tensor: commander's table) or N continuous
(v, w) commands (a floating (N, 2) tensor: the action Box of ffmp.py:29-32, any Twist of
cmd_vel_publisher, train.py:134-143), clipped to the Box by the env kernel (SPEC a15b).

Observation tensors keep the consumer layout of train.py:44,543-557 with a
leading N: state_m (N,2,G,G) f32, state_g (N,2), state_v (N,2), state_t (N,1);
extras: potential (N,G,G), grad (N,2), lidar (N,L).

Every entry point goes through the HIP library; there is no CPU path.  The
returned obs dict holds the env's own device buffers (overwritten in place by
the next step/reset) unless `copy=True`.  With a frame ring (frame_window > 2)
`state_m` is a view of the current pair of ring slots, so take it from each
step's return value (or `env.state_m`) rather than keeping the first one.
"""
from __future__ import annotations

import ctypes as C
import math
import os
import weakref
from typing import Dict, Optional, Tuple, Union

import numpy as np
import torch

from . import _abi
from .config import (PRESETS, FFMPConfig, beam_dirs, beam_table, preset, rollout_horizon, rollout_table, sector_table,
                     turn_table)


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def scenario_tensors(num_envs: int, n_obst: int, pose, goal, obst=None, obst_r=None, episode=None,
                     device="cpu") -> Dict[str, Optional[torch.Tensor]]:
    """set_scenarios' host-side argument check (no GPU needed with device="cpu"): the arrays as
    contiguous float64 tensors on `device` — pose (N, 3), goal (N, 2), obst (N, K, 4), obst_r (N, K)
    (both None where K == 0) — and episode (N,) int32 or None.  Tensors or arrays, float32 (widened
    exactly) or float64, from any device; a wrong shape or a dtype of another kind is a ValueError."""
    N, K = int(num_envs), int(n_obst)

    def f64(name, x, shape):
        t = torch.as_tensor(x)
        if not t.is_floating_point() or t.dtype not in (torch.float32, torch.float64):
            raise ValueError(f"{name} must be float32 or float64, got {t.dtype}")
        if tuple(t.shape) != shape:
            raise ValueError(f"{name} must have shape {shape}, got {tuple(t.shape)}")
        return t.to(device=device, dtype=torch.float64).contiguous()

    out = {"pose": f64("pose", pose, (N, 3)), "goal": f64("goal", goal, (N, 2)), "obst": None, "obst_r": None,
           "episode": None}
    if K > 0:
        if obst is None or obst_r is None:
            raise ValueError(f"obst and obst_r are needed with n_obst = {K}")
        out["obst"], out["obst_r"] = f64("obst", obst, (N, K, 4)), f64("obst_r", obst_r, (N, K))
    else:
        for name, x, shape in (("obst", obst, (N, 0, 4)), ("obst_r", obst_r, (N, 0))):
            if x is not None and tuple(torch.as_tensor(x).shape) != shape:
                raise ValueError(f"{name} must have shape {shape} with n_obst = 0, got {tuple(torch.as_tensor(x).shape)}")
    if episode is not None:
        ep = torch.as_tensor(episode)
        if ep.is_floating_point() or ep.is_complex() or ep.dtype == torch.bool:
            raise ValueError(f"episode must be an integer tensor, got {ep.dtype}")
        if tuple(ep.shape) != (N,):
            raise ValueError(f"episode must have shape {(N,)}, got {tuple(ep.shape)}")
        out["episode"] = ep.to(device=device, dtype=torch.int32).contiguous()
    return out


class FFMPVec:
    """Batched FFMP env on one GPU.

    Args:
        num_envs: envs held by THIS process (a shard of the global batch).
        config: FFMPConfig or preset name ("C1".."C5").
        device: a cuda device (default: current).
        env_offset: global index of env 0 (shard start); RNG streams are keyed
            by the global index so trajectories do not depend on sharding.
        potential: also raster the potential plane (default True).
        keep_terminal: also keep every env's post-step state before auto-reset
            (`term_record` (N, record_len) and `term_obs` (N, 5) = state_g, state_v, state_t):
            what a transition store needs for envs that just finished (ReplayMemory).
        frame_window: W >= 2 frames per env kept in HBM.  W > 2: a slot-major ring `frames`
            (W, N, G, G) and `state_m` = the (N,2,G,G) view frames[p:p+2].transpose(0, 1) of the
            current [older, newest] pair.  Each step slides the pair by one slot and writes only
            the new frame (plus the older one of envs that reset): the temporal stack of
            make_temporal_maps (train.py:474-486) kept in place instead of re-written, as one
            contiguous plane per slot.  Every W-1 steps the pair wraps to slot 0 (both frames
            written).  W = 2: the contiguous (N,2,G,G) layout, both frames written every step.
            None: 8 for large batches when HBM allows, else 2.
        seamless: W > 2 only.  True: the ring is HIP virtual memory with one extra virtual slot
            mapped onto slot 0's pages (include/ffmp.h ffmp_ring_create), so the pair never
            wraps and every step writes only the new frame; `frames` is (W+1, N, G, G) with
            frames[W] aliasing frames[0].  None (default): seamless when the device supports
            it, else the wrapping ring.  False: always the wrapping ring.
        fused: True: every step is ONE launch (ffmp_step_fused: one block per env steps the env,
            then rasters its plane); False: the env kernel, then the raster; None (default): the
            autotune times both on this instance and keeps the faster (small batches: False).
        tuning: a previous instance's `tuning()` (launch shapes, one- or two-launch step): used
            instead of the autotune (e.g. for profiling runs that should contain only timed
            launches); the seamless ring's slot repair still runs.
        hbm_budget: bytes of HBM this instance may hold, at steady state and while it is built
            (autotune placement tries and the ring's pairing candidates included): caps the frame
            window W, the ring's extra pairing pieces (FFMP_TUNE_RING_EXTRA) and the relocation /
            placement retries (each holds another arena + a spacer).  None: W and the retries are
            sized from free HBM (60 % for the ring).  Pieces a closed instance's ring left in the
            process pool are reused by later rings and are not charged to this one.  `hbm_bytes()`
            / `hbm_peak_bytes` report what it holds / held at most.
        obs_format: "f32" (default): the reference consumer layout, state_m float32 0/255
            (train.py:543-545) and a float32 potential plane.  "u8f16": the compact layout
            (include/ffmp.h FFMP_OBS_U8F16) for consumers that convert on load — state_m uint8
            with the same 0/255 values (`state_m.float()` is the f32 layout bit for bit) and the
            potential plane as float16 (the float32 value rounded to nearest even): 3 instead of
            8 bytes per cell of a step's raster.  With cfg.flow the flow planes are float16 too.
        bev_series: k > 0 (needs cfg.flow): also keep the last k 4-channel BEV images [occupancy,
            R, G, B] of every env (ffmp_bev_image: the newest frame and its motion flow as colour),
            a ring `bev` (k, N, 4, G, G) written after every step / reset; bev_maps() is the input of
            the reference's 12-channel option (train.py:66: "(occupancy(MONO) + flow(RGB)) *
            series(3 steps)", k = 3).  One extra elementwise launch per step.
        info_format: "dict" (default): step()'s info is one dict of (N,) device tensors (is_goal,
            collision, truncated, step, episode).  "list": gym 0.17/0.18 VectorEnv's form, a tuple
            of N per-env dicts of Python scalars (one device -> host copy per step).
        sparse_frames: keep one tag per 64-cell granule of every (ring slot, env) — `frame_tags`
            (slots, N, ceil(G*G/64)) uint8 in the arena, tag 0 = the granule holds zeros — and let
            the raster skip the frame stores that would write zeros over zeros (include/ffmp.h
            ffmp_obs_tags_t): about half the bytes of a C3 step, every value unchanged.  None
            (default): on for obs_format="f32" with pipeline == 1 (pipelined slices and the
            compact format store densely; asking for it there raises ValueError).  The frame
            ring is then read-only for consumers: a caller that writes into it calls
            invalidate_frame_tags() before the next step (`frames` does so each time it is taken).
    """

    def __init__(self, num_envs: int, config: Union[FFMPConfig, str] = "C3",
                 device: Optional[Union[str, torch.device]] = None, env_offset: int = 0,
                 potential: bool = True, seed: Optional[int] = None, arena: bool = True,
                 autotune: bool = True, pipeline: Optional[int] = None, keep_terminal: bool = False,
                 frame_window: Optional[int] = None, seamless: Optional[bool] = None,
                 fused: Optional[bool] = None, tuning: Optional[dict] = None, obs_format: str = "f32",
                 hbm_budget: Optional[int] = None, bev_series: int = 0, info_format: str = "dict",
                 sparse_frames: Optional[bool] = None):
        if isinstance(config, str):
            config = preset(config)
        if seed is not None:
            config = config.replace(seed=int(seed))
        self.cfg: FFMPConfig = config
        self.lib = _abi.load()
        if not torch.cuda.is_available():
            raise _abi.FFMPBackendError("FFMPVec needs a ROCm GPU (torch.cuda.is_available() is False)")
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if self.device.type != "cuda":
            raise ValueError(f"FFMPVec runs on a GPU device, got {self.device}")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.num_envs = int(num_envs)
        if self.num_envs <= 0:
            raise ValueError("num_envs must be positive")
        if obs_format not in self.OBS_FORMATS:
            raise ValueError(f"obs_format must be one of {sorted(self.OBS_FORMATS)}, got {obs_format!r}")
        self.obs_format = obs_format
        if info_format not in self.INFO_FORMATS:
            raise ValueError(f"info_format must be one of {self.INFO_FORMATS}, got {info_format!r}")
        self.info_format = info_format
        self._fmt, self._frame_dtype, self._pot_dtype = self.OBS_FORMATS[obs_format]
        self._fes = torch.empty((), dtype=self._frame_dtype).element_size()  # bytes per frame cell
        self._pes = torch.empty((), dtype=self._pot_dtype).element_size()    # bytes per potential cell
        # granule tags (include/ffmp.h ffmp_obs_tags_t): the raster skips the frame stores that would
        # write zeros over zeros.  float32 frames, the serial step (pipelined slices launch their
        # rasters per env slice through plain ffmp_obs_t structs: they run dense)
        slices = 1 if pipeline is None else max(1, min(int(pipeline), self.num_envs))
        if sparse_frames and (obs_format != "f32" or slices > 1):
            raise ValueError("sparse_frames=True needs obs_format='f32' and pipeline=1")
        self.sparse_frames = (obs_format == "f32" and slices == 1) if sparse_frames is None else bool(sparse_frames)
        self.env_offset = int(env_offset)
        self.with_potential = bool(potential)
        self.hbm_budget = None if hbm_budget is None else int(hbm_budget)
        self.hbm_peak_bytes = 0
        self.arena = bool(arena)
        self.keep_terminal = bool(keep_terminal)
        self.placement = None
        self.raster_shape = (0, 0)  # (cells per block, FFMP_RASTER_* flags); 0, 0 = library default
        self.raster_shape_newest = (0, 0)  # the same for newest-only launches (frame ring)
        # the BEV image ring (bev_series) is an arena buffer like the planes: counted by the HBM
        # budget, the auto frame window and the ring's pairing spare
        self.bev_series = int(bev_series)
        if self.bev_series:
            if not self.cfg.flow:
                raise ValueError("bev_series needs FFMPConfig(flow=True) (the flow planes it colours)")
            if not 1 <= self.bev_series <= _abi.MAX_SERIES:
                raise ValueError(f"bev_series must be in [1, {_abi.MAX_SERIES}]")
        self.frame_window = self._pick_window(frame_window)
        self._seamless_req = seamless if self.frame_window > 2 else False
        if seamless and self.frame_window == 2:
            raise ValueError("seamless=True needs frame_window > 2")
        self.ring = "contiguous" if self.frame_window == 2 else "wrap"  # or "seamless" (set by _alloc)
        self.ring_meta = None
        self.fused = bool(fused) if fused is not None else False  # autotune may switch it on
        self._fused_req = fused
        self.fused_flags = _abi.RASTER_NT
        self._wpos = 0  # frame slot of state_m[:, 0]
        # temporal_maps(k): physical ring slots of the newest frames, newest first (lag 0, 1, ...),
        # and whether every env's lags beyond them are clamped away (a full reset) or unknown
        # (a checkpoint reload re-rasters only the [older, newest] pair)
        self._hist = []
        self._hist_from_reset = False
        self._alloc()
        self._bev_pos = 0       # ring slot of the newest image
        self._bev_hist = []     # slots of the newest images, newest first (as _hist)
        self._bev_from_reset = False
        G2 = self.cfg.grid * self.cfg.grid
        if pipeline is None:
            pipeline = 1  # measured: no net gain on MI355X (profiles/r01_pipeline.txt, r03b_pipeline.txt)
        self.pipeline_slices = max(1, min(int(pipeline), self.num_envs))
        if self.pipeline_slices > 1 and fused:
            raise ValueError("pipeline > 1 and fused=True are exclusive")
        if self.pipeline_slices > 1:
            self._fused_req = False
        plane_bytes = self.num_envs * G2 * (2 * self._fes + (self._pes if potential else 0) +
                                            (2 * self._pes if self.cfg.flow else 0))
        paired = self.ring == "seamless" and self.with_potential
        if paired and plane_bytes >= self.RELOCATE_MIN_BYTES and (tuning is not None or autotune):
            self._relocate_partner(self.PARTNER_TRIES if plane_bytes >= self.REPLACE_MIN_BYTES
                                   else self.PARTNER_TRIES_SMALL)
        self._build_structs()
        if tuning is not None:
            self._apply_tuning(tuning)
            if paired and plane_bytes >= self.RELOCATE_MIN_BYTES:
                self._repair_slots()
                self.placement = dict(self.placement, ring=self.ring_meta)
        elif autotune and plane_bytes >= self.AUTOTUNE_MIN_BYTES:
            self._autotune_raster()
            # the seamless ring already paired its slots with the potential plane; a new arena
            # would undo that
            if self.arena and plane_bytes >= self.REPLACE_MIN_BYTES and not paired:
                self._retry_placement()
            if paired and plane_bytes >= self.RELOCATE_MIN_BYTES:
                self._repair_slots()
                self._recheck_fused()
            if self.placement is not None and self.ring_meta is not None:
                self.placement = dict(self.placement, ring=self.ring_meta)
        self.pool_released_bytes = 0
        if self.ring == "seamless":
            # the pairing references of the planes this instance paired against and then dropped
            # (relocation tries): those planes are freed, a later plane may take their address
            self._forget_partners(keep=self.potential)
        if self.release_pool and self.ring == "seamless":
            # the pairing candidates this instance did not choose, the rings its relocation /
            # repair dropped: their memory goes back to the device (addresses stay reserved)
            torch.cuda.synchronize(self.device)
            self.pool_released_bytes = _abi.ring_pool_trim(self.device.index, self.pool_keep_bytes)
            if self.ring_meta is not None:
                self.ring_meta = dict(self.ring_meta, pool_released_bytes=self.pool_released_bytes)
                if self.placement is not None and "ring" in self.placement:
                    self.placement = dict(self.placement, ring=self.ring_meta)
        self._needs_reset = True

    # ------------------------------------------------------------------ setup
    # After construction (and on close) the frame-ring pieces parked in the process pool — pairing
    # candidates not chosen, rings dropped by the relocation / slot repair — are released
    # (ffmp_ring_pool_trim): at C3 they were ~65 GB beside the instance's 77 GB (round 3).  A
    # process that builds envs in a loop may keep a floor of pieces for the next one (reused first).
    release_pool = True
    pool_keep_bytes = 0
    _pair_partners = ()  # potential-plane addresses this instance's rings were paired against

    @staticmethod
    def _forget_at_exit(device: int, box: list) -> None:
        """weakref.finalize of an instance dropped without close(): its planes' pairing references
        go with it (a later instance whose plane lands at the same address — torch's caching
        allocator hands it out again — must not be judged against another plane's probe)."""
        for ptr in box:
            _abi.ring_pair_forget(device, ptr)
        box.clear()

    def _note_partner(self) -> None:
        if self.potential is not None:
            self._pair_partners = tuple(set(self._pair_partners) | {self.potential.data_ptr()})
            box = getattr(self, "_partner_box", None)
            if box is None:
                import weakref
                box = self._partner_box = []
                weakref.finalize(self, FFMPVec._forget_at_exit, self.device.index, box)
            box[:] = list(self._pair_partners)

    def _forget_partners(self, keep: Optional[torch.Tensor] = None) -> None:
        """Forget the ring-pairing references of the partner planes this instance no longer holds
        (trimming the pool had erased every instance's)."""
        k = None if keep is None else keep.data_ptr()
        for ptr in self._pair_partners:
            if ptr != k:
                _abi.ring_pair_forget(self.device.index, ptr)
        self._pair_partners = () if k is None else (k,)
        box = getattr(self, "_partner_box", None)
        if box is not None:
            box[:] = list(self._pair_partners)

    OBS_FORMATS = {"f32": (_abi.OBS_F32, torch.float32, torch.float32),
                   "u8f16": (_abi.OBS_U8F16, torch.uint8, torch.float16)}
    _ARENA_ALIGN = 2 << 20
    WINDOW_DEFAULT = 8
    WINDOW_HBM_FRACTION = 0.6  # auto window: frames + other planes within this share of free HBM

    def _arena_estimate(self, with_frames: bool) -> int:
        """Bytes of the arena _alloc carves (2 MiB-aligned buffers)."""
        off = 0
        for _, shape, dtype in self._buffer_specs(with_frames=with_frames):
            off = -(-off // self._ARENA_ALIGN) * self._ARENA_ALIGN + self._nbytes(shape, dtype)
        return -(-off // self._ARENA_ALIGN) * self._ARENA_ALIGN

    @staticmethod
    def _ring_piece(slot_bytes: int) -> int:
        """Piece size of a seamless ring slot (ffmp_ring.hip ring_geom; 2 MiB granularity)."""
        g = 2 << 20
        slot = -(-slot_bytes // g) * g
        return (1 << 30) if slot >= (2 << 30) else slot

    def _ring_stride(self, slot_bytes: int) -> int:
        piece = self._ring_piece(slot_bytes)
        return -(-slot_bytes // piece) * piece

    def _pick_window(self, w: Optional[int]) -> int:
        cfg, N = self.cfg, self.num_envs
        G2 = cfg.grid * cfg.grid
        plane = N * G2 * self._fes
        budget = self.hbm_budget
        if budget is not None:  # what fits: the arena (other planes, state) + W ring slots
            rest = budget - self._arena_estimate(with_frames=False)  # (holds the tags of 2 slots)
            tag_slot = N * self._tags_per_frame() if self.sparse_frames else 0
            w_fit = (rest + 2 * tag_slot) // (self._ring_stride(plane) + tag_slot)
            if rest < 2 * plane:
                raise ValueError(f"hbm_budget {budget} B cannot hold {N} envs' planes "
                                 f"({self._arena_estimate(with_frames=False) + 2 * plane} B at W = 2)")
        if w is not None:
            if int(w) < 2:
                raise ValueError("frame_window must be >= 2")
            if budget is not None and int(w) > 2 and int(w) > w_fit:
                raise ValueError(f"frame_window={w} does not fit hbm_budget={budget} (at most {w_fit})")
            return int(w)
        if N * G2 * 12 < self.AUTOTUNE_MIN_BYTES:  # (the f32 layout's bytes: same choice for both formats)
            return 2
        other = N * G2 * ((self._pes if self.with_potential else 0) + (2 * self._pes if cfg.flow else 0) +
                          4 * self.bev_series * self._fes)
        free, _ = torch.cuda.mem_get_info(self.device)
        free += max(0, int(self.lib.ffmp_ring_pool_bytes(self.device.index)))  # parked pieces are reused
        room = self.WINDOW_HBM_FRACTION * free - other
        wmax = self.WINDOW_DEFAULT if budget is None else min(self.WINDOW_DEFAULT, w_fit)
        W = int(max(2, min(wmax, room // plane)))
        return 2 if W < 3 else W

    def _buffer_specs(self, with_frames: bool = True):
        """(name, shape, dtype) of every per-shard device buffer."""
        cfg, N = self.cfg, self.num_envs
        G, K, L = cfg.grid, cfg.n_obst, cfg.n_beams
        f32, f64, i32, b = torch.float32, torch.float64, torch.int32, torch.bool
        specs = [
            # observation planes first: the big, hot, write-streamed buffers
            ("frames", (N, 2, G, G) if getattr(self, "frame_window", 2) == 2 else (self.frame_window, N, G, G),
             self._frame_dtype),
            ("potential", (N, G, G), self._pot_dtype),
            ("flow", (N, 2, G, G), self._pot_dtype),  # float16 in the compact layout, like the potential
            # sparse_frames: one tag per 64-cell granule of every (physical frame slot, env)
            ("frame_tags", (max(getattr(self, "frame_window", 2), 2), N, self._tags_per_frame()), torch.uint8),
            # state
            ("pose", (N, 3), f64), ("goal", (N, 2), f64), ("d0", (N,), f64),
            ("obst", (N, max(K, 1), 4), f64), ("obst_r", (N, max(K, 1)), f64),
            ("t", (N,), i32), ("episode", (N,), i32), ("record", (N, cfg.record_len()), f32),
            ("err", (1,), i32),
            # small obs + outputs
            ("state_g", (N, 2), f32), ("state_v", (N, 2), f32), ("state_t", (N, 1), f32),
            ("grad", (N, 2), f32), ("lidar", (N, L), f32),
            ("reward", (N,), f32), ("done", (N,), b), ("is_goal", (N,), b), ("collision", (N,), b),
            ("truncated", (N,), b),
            # optional: post-step state before auto-reset (ffmp_state_t.term_*)
            ("term_record", (N, cfg.record_len()), f32), ("term_obs", (N, 5), f32),
            # optional: the last bev_series 4-channel BEV images of every env (ffmp_bev_image)
            ("bev", (max(getattr(self, "bev_series", 0), 1), N, 4, G, G), self._frame_dtype),
        ]
        if not self.with_potential:
            specs = [sp for sp in specs if sp[0] != "potential"]
        if not cfg.flow:
            specs = [sp for sp in specs if sp[0] != "flow"]
        if not getattr(self, "sparse_frames", False):
            specs = [sp for sp in specs if sp[0] != "frame_tags"]
        if L == 0:
            specs = [sp for sp in specs if sp[0] != "lidar"]
        if not self.keep_terminal:
            specs = [sp for sp in specs if not sp[0].startswith("term_")]
        if not getattr(self, "bev_series", 0):
            specs = [sp for sp in specs if sp[0] != "bev"]
        if not with_frames:
            specs = [sp for sp in specs if sp[0] != "frames"]
        return specs

    def _tags_per_frame(self) -> int:
        """Granule tags per frame plane: ceil(G * G / 64) (include/ffmp.h FFMP_TAG_CELLS)."""
        return -(-self.cfg.grid * self.cfg.grid // _abi.TAG_CELLS)

    frame_tags = None  # (slots, N, ceil(G*G/64)) uint8, sparse_frames only
    _frames = None

    @property
    def frames(self) -> Optional[torch.Tensor]:
        """The frame ring itself: (W, N, G, G) slot-major ((W + 1, ...) for the seamless ring, slot W
        aliasing slot 0), or (N, 2, G, G) with W = 2.  This is the handle through which a caller can
        write frame memory, so with sparse_frames taking it counts as a write: every tag is set to
        unknown (invalidate_frame_tags()), and the next raster into each slot stores all of its
        cells.  Take it to inspect or to overwrite the ring, not in the step loop; `state_m`,
        temporal_maps() and bev_maps() read the ring without that cost."""
        self.invalidate_frame_tags()
        return self._frames

    @frames.setter
    def frames(self, t: Optional[torch.Tensor]) -> None:
        self._frames = t

    def invalidate_frame_tags(self, slots=None) -> None:
        """Mark the frames of the physical ring slots `slots` (an index, a list or a slice of
        frame_tags' first dimension; None: all) as unknown, so that the next raster into them stores
        every cell.  The frame ring is read-only for consumers: whoever writes frame memory behind
        the raster's back (torch ops on `frames` / `state_m`, a new or re-mapped ring) calls this
        before the next step, or a granule tagged all-zero keeps whatever was written into it.
        A no-op without sparse_frames."""
        if self.frame_tags is None:
            return
        if slots is None:
            self.frame_tags.fill_(1)
        else:
            self.frame_tags[slots] = 1

    def frame_tag_density(self) -> float:
        """Mean tag of the newest frame's slot: the share of that frame's granules that hold a
        non-zero cell (or are unknown) — a diagnostic, computed with torch outside any timed
        region (it synchronizes); NaN without tags.  C3: about 0.04."""
        if self.frame_tags is None:
            return float("nan")
        slot = (self._wpos + 1) % self.frame_tags.shape[0]
        return float(self.frame_tags[slot].ne(0).float().mean().item())

    NO_VMM = "has no virtual memory management"  # ffmp_ring_create's message (ffmp_ring.hip ring_geom)

    def _alloc_ring(self) -> bool:
        """The seamless frame ring (HIP VMM, virtual slot W aliasing slot 0), if requested and
        the device supports it; its slots are built to pair well with the potential plane the
        raster writes beside them (include/ffmp.h ffmp_ring_create)."""
        N, G = self.num_envs, self.cfg.grid
        torch.cuda.synchronize(self.device)  # the pairing probes write the potential plane on their own stream
        prev_extra = None
        try:
            partner = self.potential if self.PAIR_SLOTS else None
            if self.hbm_budget is not None:  # pairing candidates beyond need only within the budget
                slot = N * G * G * self._fes
                spare = self.hbm_budget - self._arena_used - self.frame_window * self._ring_stride(slot)
                prev_extra = _abi.set_tuning(_abi.TUNE_RING_EXTRA, 1 + max(0, spare // self._ring_piece(slot)))
            try:
                self._ring = _abi.SeamlessRing(self.device.index, (N, G, G), self.frame_window, bits=8 * self._fes,
                                               partner=partner)
            except _abi.FFMPBackendError as e:
                if self.NO_VMM in str(e):
                    raise
                # the ring's pieces come from outside torch's caching allocator: give its cached
                # blocks back to the device and try once more
                torch.cuda.empty_cache()
                self._ring = _abi.SeamlessRing(self.device.index, (N, G, G), self.frame_window, bits=8 * self._fes,
                                               partner=partner)
            self._frames = self._ring.tensor
            self.ring_meta = self._ring.info()
            if partner is not None:
                self._note_partner()
        except _abi.FFMPBackendError as e:
            # only a device without virtual memory management falls back to the wrapping ring;
            # any other failure (out of memory, a fault) is the caller's to see
            if self._seamless_req or self.NO_VMM not in str(e):
                raise
            self._seamless_req = False  # no VMM here: the wrapping ring from now on
            return False
        finally:
            if prev_extra is not None:
                _abi.set_tuning(_abi.TUNE_RING_EXTRA, prev_extra)
        self.ring = "seamless"
        self._note_hbm()
        return True

    def _note_hbm(self, extra: int = 0) -> None:
        """Track the most HBM this instance has held (hbm_peak_bytes); `extra` = bytes held beside
        the current buffers (placement tries, spacers)."""
        self.hbm_peak_bytes = max(self.hbm_peak_bytes, self.hbm_bytes() + int(extra))

    def _budget_allows(self, held_extra: int, more: int) -> bool:
        """Under hbm_budget: may the instance hold `more` bytes beside its buffers and `held_extra`?"""
        return self.hbm_budget is None or self.hbm_bytes() + held_extra + more <= self.hbm_budget

    def _alloc(self, keep_ring: bool = False):
        """All per-shard buffers, zero-initialised.  With arena=True (default) they are views
        into ONE device allocation carved at 2 MiB boundaries, planes first.  The seamless frame
        ring, when used, is its own VMM allocation, made after the arena so that its slots can
        be paired with the potential plane (keep_ring: re-allocate everything else)."""
        dev = self.device
        keep = keep_ring and self.ring == "seamless"
        want_ring = keep or self._seamless_req is not False
        if not keep:
            self._frames = None
            self._ring = None
            self.ring_meta = None
        specs = self._buffer_specs(with_frames=not want_ring)
        self.potential = None
        self.lidar = None
        self.flow = None
        self.frame_tags = None
        self.term_record = None
        self.term_obs = None
        self.bev = None
        if self.arena:
            self._arena_offs, off = [], 0
            for _, shape, dtype in specs:
                off = -(-off // self._ARENA_ALIGN) * self._ARENA_ALIGN
                self._arena_offs.append(off)
                off += self._nbytes(shape, dtype)
            self._arena_used = -(-off // self._ARENA_ALIGN) * self._ARENA_ALIGN
            self._arena_buf = torch.zeros(max(self._arena_used, 1), dtype=torch.uint8, device=dev)
            self._carve(0, specs)
        else:
            self._arena_buf = None
            self._arena_used = 0
            for name, shape, dtype in specs:
                setattr(self, name, torch.zeros(shape, dtype=dtype, device=dev))
        if want_ring and not keep and not self._alloc_ring():
            return self._alloc()  # no VMM: the wrapping ring, frames in the arena
        if self.potential is not None:
            self.potential.zero_()  # the pairing probe wrote into it
        L = self.cfg.n_beams
        self.beam_cs = torch.as_tensor(beam_table(L), dtype=torch.float64).to(dev) if L > 0 else None
        if self.frame_tags is not None:
            if self.ring == "seamless":
                self.invalidate_frame_tags()  # a ring's contents are undefined (new) or stale (kept)
            else:
                self.frame_tags.zero_()       # the frames were allocated as zeros: tag 0 holds
        self._note_hbm()

    @staticmethod
    def _nbytes(shape, dtype) -> int:
        n = 1
        for d in shape:
            n *= d
        return n * torch.empty((), dtype=dtype).element_size()

    def _carve(self, base: int, specs) -> None:
        """Point every buffer of `specs` into the arena, starting `base` bytes in."""
        self._arena_base = base
        for (name, shape, dtype), o in zip(specs, self._arena_offs):
            nb = self._nbytes(shape, dtype)
            setattr(self, name, self._arena_buf[base + o:base + o + nb].view(dtype).view(shape))

    # Raster launch-shape autotune (profiles/r01_placement.txt, r01_raster_tuning.txt).  The
    # raster's three concurrent 16-B store streams run anywhere from 5.7 to 7.3 TB/s depending
    # on where the planes land in HBM (fixed per allocation, identical virtual layouts) and on
    # the launch shape, and the best shape differs between allocations (e.g. 4096-cell blocks
    # 7.1-7.3 TB/s on some allocations and 5.7 on others, where 2048-cell blocks give 6.8).
    # So the shape is chosen per instance: the raster is timed on this instance's own buffers,
    # after a real reset, for each candidate, and the fastest is kept.  Results are identical
    # for every shape.
    AUTOTUNE_MIN_BYTES = 256 << 20
    # Newest-only launches (frame ring) move 2/3 of the bytes per block of a full launch, so they
    # want bigger blocks (profiles/r01_window.txt: 16384-cell blocks 7.1 TB/s vs 6.7 at 4096);
    # the two launch kinds are tuned independently from the same timed cycles.
    RASTER_SHAPES = (
        (4096, _abi.RASTER_PLAIN), (2048, _abi.RASTER_PLAIN), (2048, _abi.RASTER_PLAIN | _abi.RASTER_XCD),
        (4096, _abi.RASTER_PLAIN | _abi.RASTER_XCD), (3072, _abi.RASTER_PLAIN | _abi.RASTER_XCD),
        (2048, _abi.RASTER_NT), (4096, _abi.RASTER_NT), (2048, _abi.RASTER_NT | _abi.RASTER_XCD),
        (8192, _abi.RASTER_NT), (8192, _abi.RASTER_NT | _abi.RASTER_XCD), (16384, _abi.RASTER_NT),
        (8192, _abi.RASTER_PLAIN), (16384, _abi.RASTER_PLAIN),
        # 2-D wave tiles (compact cull box, fewer disc evaluations; identical results)
        (16384, _abi.RASTER_NT | _abi.RASTER_TILE4), (8192, _abi.RASTER_NT | _abi.RASTER_TILE4),
        (8192, _abi.RASTER_NT | _abi.RASTER_XCD | _abi.RASTER_TILE4), (16384, _abi.RASTER_NT | _abi.RASTER_TILE2),
        (16384, _abi.RASTER_NT | _abi.RASTER_TILE8), (4096, _abi.RASTER_PLAIN | _abi.RASTER_TILE4),
        # smaller tiled blocks for small planes (C2's 0.09 ms launches lose ~10 % to their last blocks)
        (4096, _abi.RASTER_NT | _abi.RASTER_TILE4), (2048, _abi.RASTER_NT | _abi.RASTER_TILE4),
        # round 3: 4,096-cell tiled blocks with the XCD remap — at C3 the fastest shape in the step loop
        # (2.265 ms against 2.345 without the remap and 2.39 for 8,192-cell blocks;
        # profiles/r03b_transient_shapes.txt, steady state)
        (4096, _abi.RASTER_NT | _abi.RASTER_XCD | _abi.RASTER_TILE4), (4096, _abi.RASTER_NT | _abi.RASTER_XCD | _abi.RASTER_TILE2),
        # granule tags only: the tagged kernel held to 6 waves per SIMD (RASTER_WAVES)
        (4096, _abi.RASTER_NT | _abi.RASTER_XCD | _abi.RASTER_TILE4 | _abi.RASTER_WAVES),
        (8192, _abi.RASTER_NT | _abi.RASTER_TILE4 | _abi.RASTER_WAVES),
        (16384, _abi.RASTER_NT | _abi.RASTER_TILE2 | _abi.RASTER_WAVES), (4096, _abi.RASTER_NT | _abi.RASTER_WAVES),
        # 16,384-cell tiled blocks with the XCD remap, plain and held to 6 waves per SIMD: at C3 with tags the
        # 4-row tiles run 1.51-1.53 ms per newest-only launch against 1.57-1.59 without the remap
        # (profiles/raster_direct_variants.json)
        (16384, _abi.RASTER_NT | _abi.RASTER_XCD | _abi.RASTER_TILE4), (16384, _abi.RASTER_NT | _abi.RASTER_XCD | _abi.RASTER_TILE2),
        (16384, _abi.RASTER_NT | _abi.RASTER_XCD | _abi.RASTER_TILE4 | _abi.RASTER_WAVES),
        (16384, _abi.RASTER_NT | _abi.RASTER_XCD | _abi.RASTER_TILE2 | _abi.RASTER_WAVES),
    )

    # Granule tags only, the two-launch raster: the tagged kernel at 6 waves per SIMD whose blocks use no
    # LDS and no barrier and make one memory round trip (RASTER_DIRECT), beside each of its staged twins
    # above.  A list of its own: the flag stands without RASTER_WAVES, and the one-launch step ignores it.
    DIRECT_SHAPES = (
        (4096, _abi.RASTER_NT | _abi.RASTER_XCD | _abi.RASTER_TILE4 | _abi.RASTER_DIRECT),
        (8192, _abi.RASTER_NT | _abi.RASTER_TILE4 | _abi.RASTER_DIRECT),
        (16384, _abi.RASTER_NT | _abi.RASTER_TILE2 | _abi.RASTER_DIRECT), (4096, _abi.RASTER_NT | _abi.RASTER_DIRECT),
        (16384, _abi.RASTER_NT | _abi.RASTER_XCD | _abi.RASTER_TILE4 | _abi.RASTER_DIRECT),
        (16384, _abi.RASTER_NT | _abi.RASTER_XCD | _abi.RASTER_TILE2 | _abi.RASTER_DIRECT),
    )

    def _raster_gbs_steady(self, steps: int = 3) -> Dict[bool, Tuple[float, float]]:
        """Raster (GB/s, ms per launch) per launch kind (full: True, newest-only: False) in the
        real regime: whole steps (env kernel, then raster), raster launches timed with HIP
        events.  (Back-to-back rasters alone can read up to 15 % higher for some shapes than
        they sustain inside the step loop.)"""
        a = torch.full((self.num_envs,), 10, dtype=torch.int64, device=self.device)
        self.step(a)
        t = []
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(steps):
            self.step(a, timing=t)
        ev[1].record()
        torch.cuda.synchronize(self.device)
        out = {}
        for full in (True, False):
            sel = [r for r in t if r[4] == full]
            if sel:
                ms = sum(r[0].elapsed_time(r[1]) for r in sel)
                out[full] = (sum(r[3] for r in sel) / (ms * 1e-3) / 1e9, ms / len(sel))
        out["step_ms"] = ev[0].elapsed_time(ev[1]) / steps
        return out

    # Placement retries.  Two planes written in lockstep (a frame slot and the potential plane)
    # stream at ~7.1 TB/s or ~5.3-6.2 depending on where each landed in physical memory — a
    # property of the PAIR (tools/region_probe.hip, profiles/r01_ring.txt §6) — so with the
    # seamless ring one slow slot/plane pair makes one step in W ~25 % slower.  Allocating again
    # while the earlier arenas and a spacer are still held (so the allocator must return
    # different memory) often lands fast: below the threshold, up to PLACEMENT_RETRIES further
    # arenas are timed over one whole ring cycle and the fastest kept; bounded by free HBM.
    REPLACE_MIN_BYTES = 4 << 30
    PLACEMENT_FAST_GBS = 6800.0
    PLACEMENT_FAST_GBS_SEAMLESS = 7000.0  # newest-only launches only: every slot paired well
    PLACEMENT_RETRIES = 8
    PLACEMENT_SPACER = 1 << 30

    def _retry_placement(self) -> None:
        """Below the fast threshold, allocate the arena again (the seamless ring is kept: rings are
        never unmapped) while the previous ones and a growing spacer are held, time one ring
        cycle with the tuned shapes, keep the fastest; then re-tune the shapes on the winner."""
        names = [n for n, _, _ in self._buffer_specs()]  # includes "frames" (arena or ring)
        keep = [(self.placement["gbs"], self._arena_buf, {n: getattr(self, n) for n in names})]
        spacers = []
        tries = [round(self.placement["gbs"], 1)]
        fast = self.PLACEMENT_FAST_GBS_SEAMLESS if self.ring == "seamless" else self.PLACEMENT_FAST_GBS
        for k in range(self.PLACEMENT_RETRIES):
            if max(c[0] for c in keep) >= fast:
                break
            free, _ = torch.cuda.mem_get_info(self.device)
            if free < 1.2 * self._arena_buf.numel() + (k + 1) * self.PLACEMENT_SPACER + (1 << 30):
                break
            held = sum(c[1].numel() for c in keep[1:]) + sum(t.numel() for t in spacers)
            if not self._budget_allows(held, self._arena_buf.numel() + (k + 1) * self.PLACEMENT_SPACER):
                break
            spacers.append(torch.empty((k + 1) * self.PLACEMENT_SPACER, dtype=torch.uint8, device=self.device))
            self._alloc(keep_ring=True)
            self._note_hbm(held + spacers[-1].numel())
            self._build_structs()
            gbs = self._placement_gbs()
            tries.append(round(gbs, 1))
            keep.append((gbs, self._arena_buf, {n: getattr(self, n) for n in names}))
        best = max(range(len(keep)), key=lambda i: keep[i][0])
        _, buf, views = keep[best]
        self._arena_buf = buf
        for n, v in views.items():
            setattr(self, n, v)
        self.invalidate_frame_tags()  # a kept ring was written under the other arenas' tags
        self._build_structs()
        del keep, spacers, views, buf
        torch.cuda.empty_cache()
        if best > 0:
            self._autotune_raster()
        self.placement = dict(self.placement, placement_tries=tries, placement_kept=best)

    # Slot repair (seamless ring).  The pairing probe at ring creation predicts most, not all,
    # slow slot/potential pairings; the step loop itself is the judge: time every slot's
    # newest-only raster over two ring cycles (after SLOT_WARMUP_CYCLES untimed ones) and rebuild
    # the ring with new pieces for slots more than SLOW_SLOT above the fastest (ffmp_ring_rebuild),
    # up to REPAIR_ROUNDS times, keeping the rebuilt ring only if its cycle is faster; a reverted
    # rebuild does not end the repair — the next round draws other pieces (round 6: one C3 box kept a
    # slot 15 % slow after its single rebuild came out worse, 13.41 vs 13.71 M on the same box,
    # profiles/r06g_bench_default_*.json).  (The 12 % threshold of rounds 1-3 guarded against rebuilds
    # judged on post-idle timings; with the warm-up, 6 %: profiles/r04h_slot_repair.txt.)
    SLOW_SLOT = 1.06
    REPAIR_ROUNDS = 3
    PAIR_SLOTS = True  # build the ring's slots from pieces probed against the potential plane

    # untimed ring cycles before the slot timing: the timing follows host work (construction, a
    # rebuild's pairing probes) that left the GPU idle, and after such a gap the raster runs slow
    # for about one ring cycle while the GPU warms up again (profiles/r03b_transient_*.txt); timed
    # straight after a rebuild, kept slots read 4-7 % slow and good rebuilds were reverted
    # (profiles/r04h_slot_repair.txt)
    SLOT_WARMUP_CYCLES = 2

    def _slot_ms(self) -> Dict[int, float]:
        """Median newest-only raster ms per physical slot written, over two ring cycles."""
        W = self.frame_window
        self.reset()
        a = torch.full((self.num_envs,), 10, dtype=torch.int64, device=self.device)
        for _ in range(self.SLOT_WARMUP_CYCLES * W):
            self.step(a)
        t = []
        for _ in range(2 * W):
            self.step(a, timing=t)
        torch.cuda.synchronize(self.device)
        per: Dict[int, list] = {}
        S = self.pipeline_slices  # timing entries per step (one raster launch per env slice)
        for k in range(len(t) // S):
            per.setdefault(self._slot_written(k), []).append(sum(r[0].elapsed_time(r[1]) for r in t[k * S:(k + 1) * S]))
        self._clear_after_tuning()
        return {i: float(np.median(v)) for i, v in per.items()}

    def _slot_written(self, k: int) -> int:
        """Physical ring slot whose newest frame step k (0-based) after a full reset writes: the
        reset leaves the window at [0, 1], step k slides it to [k+1, k+2] and writes the newest
        frame, virtual slot k+2 -> physical (k+2) % W (virtual slot W is slot 0)."""
        return (k + 2) % self.frame_window

    # Partner relocation (seamless ring).  The ring's pieces are probed against the potential
    # plane; when no probe reaches PAIR_FAST_GBS the plane itself sits where nothing pairs well
    # (round-1 C5 and some C3 boxes: every probe 4.9-5.5 TB/s).  Then the arena (with the potential
    # plane) is allocated again elsewhere — the earlier arenas and a growing spacer stay held so
    # the allocator must return different memory — and a ring is paired against the new plane
    # (the losing rings' pieces return to the pool and are probed again first); the pair with the
    # fastest probe is kept.
    # Small planes too (round 2, profiles/r02_env_chain.txt): at C2 (0.5 GB of planes, 256-MiB
    # ring pieces) every first probe paired at 5.3-5.6 TB/s and the raster ran 0.106 ms; the third
    # relocation found a 6.8 TB/s pair on each of three fresh runs, raster 0.089 ms (+16 % env-steps/s).
    # Below REPLACE_MIN_BYTES a try is cheap (a < 4 GiB arena, a few 256-MiB probes), so more are allowed.
    PAIR_FAST_GBS = 6200.0  # ffmp_ring.hip kPairFastGBs
    PARTNER_TRIES = 3
    PARTNER_TRIES_SMALL = 6
    RELOCATE_MIN_BYTES = 512 << 20  # planes of C2 size up (the ring pairs pieces of >= 256 MiB)

    def _relocate_partner(self, max_tries: int) -> None:
        meta = self.ring_meta or {}
        if not meta.get("pair_probes") or meta.get("pair_gbs_max", 0.0) >= self.PAIR_FAST_GBS:
            return
        names = [n for n, _, _ in self._buffer_specs(with_frames=False)]

        def snap():
            return {"gbs": self.ring_meta["pair_gbs_max"], "arena": self._arena_buf, "ring": self._ring,
                    "meta": self.ring_meta, "views": {n: getattr(self, n) for n in names}}

        best = snap()
        tries, held = [best["gbs"]], []
        ring_bytes = self.frame_window * self._ring.slot_stride
        for k in range(max_tries):
            free, _ = torch.cuda.mem_get_info(self.device)
            if free < self._arena_used + (k + 1) * self.PLACEMENT_SPACER + ring_bytes + (16 << 30):
                break
            # under hbm_budget: the arenas held so far (the best's among them) + this try's spacer,
            # arena and ring beside the best ring
            held_b = sum(t.numel() for t in held)
            if self.hbm_budget is not None and ring_bytes + max(held_b, self._arena_used) + self._arena_used + \
                    (k + 1) * self.PLACEMENT_SPACER + ring_bytes > self.hbm_budget:
                break
            held.append(self._arena_buf)
            held.append(torch.empty((k + 1) * self.PLACEMENT_SPACER, dtype=torch.uint8, device=self.device))
            self._ring = self._frames = None  # the best ring stays referenced by `best`
            try:
                self._alloc()
            except _abi.FFMPBackendError:
                break
            if self.ring != "seamless" or self._ring is None:
                break
            self.hbm_peak_bytes = max(self.hbm_peak_bytes, ring_bytes + sum(t.numel() for t in held) +
                                      self._arena_used + self.frame_window * self._ring.slot_stride)
            cur = snap()
            tries.append(cur["gbs"])
            if cur["gbs"] > best["gbs"]:
                best = cur
            cur = None
            if best["gbs"] >= self.PAIR_FAST_GBS:
                break
        self._arena_buf, self._ring, self.ring = best["arena"], best["ring"], "seamless"
        for n, v in best["views"].items():
            setattr(self, n, v)
        self._frames = self._ring.tensor
        self._arena_used = self._arena_buf.numel()
        torch.cuda.synchronize(self.device)
        del held
        self.potential.zero_()
        self._frames[:self.frame_window].zero_()
        self.invalidate_frame_tags()
        self.ring_meta = dict(best["meta"], partner_tries=[round(g, 1) for g in tries])
        best = None
        torch.cuda.empty_cache()

    def _adopt_ring_tensor(self) -> None:
        self._frames = self._ring.tensor
        self.potential.zero_()
        self.invalidate_frame_tags()  # rebuilt / reverted slots: other pieces, written by probes
        self._build_structs()

    def _repair_slots(self) -> None:
        """Rebuild slow slots and keep whichever ring cycles faster: a rebuild maps every slot at
        new addresses and has left kept slots slower than before (round-1 repair logs), so the
        old ring stays alive until the new one has been timed (SeamlessRing.rebuild keep_old)."""
        history = []
        ms = self._slot_ms()
        for _ in range(self.REPAIR_ROUNDS):
            fast = min(ms.values())
            slow = [i for i, v in ms.items() if v > self.SLOW_SLOT * fast]
            history.append({"slot_ms": [round(ms[i], 3) for i in sorted(ms)], "slow": slow})
            if not slow:
                break
            # the tuning launches (and _clear_after_tuning's memsets) must be done before the
            # rebuild's pairing probes write the potential plane on their own stream
            torch.cuda.synchronize(self.device)
            try:
                self._ring.rebuild(sum(1 << i for i in slow), partner=self.potential, keep_old=True)
            except _abi.FFMPBackendError as err:
                # the rebuild maps the new pieces beside the old ring: with the HBM shared (several
                # ranks on one device) it can run out; the current ring is whole and stays, and the
                # pieces the rebuild took went back to the pool (trimmed below / in __init__)
                history.append({"skipped": str(err)[:200]})
                break
            self._adopt_ring_tensor()
            new = self._slot_ms()
            if sum(new.values()) < sum(ms.values()):
                torch.cuda.synchronize(self.device)
                self._ring.drop_previous()
                ms = new
            else:  # the rebuilt ring cycles slower: back to the previous one, then another round
                history.append({"slot_ms": [round(new[i], 3) for i in sorted(new)], "reverted": True})
                torch.cuda.synchronize(self.device)
                self._ring.revert()
                self._adopt_ring_tensor()
                self._clear_after_tuning()
        else:  # every round rebuilt: the kept ring's timing (slots still slow if the last rebuilds lost)
            fast = min(ms.values())
            history.append({"slot_ms": [round(ms[i], 3) for i in sorted(ms)],
                            "slow": [i for i, v in ms.items() if v > self.SLOW_SLOT * fast]})
        self.ring_meta = dict(self.ring_meta or {}, **self._ring.info(), repair=history)

    def tuning(self) -> dict:
        """The launch choices of this instance (pass as FFMPVec(tuning=...) to skip the autotune)."""
        return {"shape": list(self.raster_shape), "shape_newest": list(self.raster_shape_newest),
                "fused": bool(self.fused), "fused_flags": int(self.fused_flags)}

    def _apply_tuning(self, t: dict) -> None:
        self.raster_shape = tuple(t["shape"])
        self.raster_shape_newest = tuple(t.get("shape_newest", t["shape"]))
        self.fused = bool(t.get("fused", False)) and self.pipeline_slices == 1 and self._fused_req is not False
        self.fused_flags = int(t.get("fused_flags", _abi.RASTER_NT))
        self.placement = {"shape": {"cells_per_block": self.raster_shape[0], "flags": self.raster_shape[1]},
                          "shape_newest": {"cells_per_block": self.raster_shape_newest[0],
                                           "flags": self.raster_shape_newest[1]},
                          "from": "tuning", "fused": {"chosen": self.fused, "flags": self.fused_flags}}

    def _tune_steps(self) -> int:
        """Timed steps per measurement: >= ~10 ms of raster, in whole ring cycles — the wrapping
        ring's W-1 steps (one full raster), or the seamless ring's W steps: every slot is written
        once, and the potential plane streams beside each slot at its own rate (one slow
        slot/plane pairing makes one step in W ~25 % slower, profiles/r01_ring.txt §6), so a
        placement check must see all of them."""
        plane_bytes = self.state_m.numel() * (self._fes + (self._pes / 2 if self.with_potential else 0.0) +
                                              (float(self._pes) if self.flow is not None else 0.0))
        steps = 3 if plane_bytes >= (8 << 30) else 12
        cyc = {"wrap": self.frame_window - 1, "seamless": self.frame_window}.get(self.ring, 1)
        return -(-steps // cyc) * cyc

    def _cycle_gbs(self, ms_full: Optional[float], ms_newest: Optional[float]) -> float:
        """Raster bandwidth of one ring cycle from per-launch times of the two kinds: one full
        launch + W-2 newest-only ones (wrapping ring), full launches only (W = 2) or newest-only
        ones only (seamless ring)."""
        n_new, n_full = self.frame_window - 2, 1
        if self.ring == "seamless":
            n_new, n_full = 1, 0
        b = n_full * self._raster_bytes(self.num_envs, True) + n_new * self._raster_bytes(self.num_envs, False)
        ms = (ms_full if n_full else 0.0) + (n_new * ms_newest if n_new else 0.0)
        return b / (ms * 1e-3) / 1e9

    def _clear_after_tuning(self) -> None:
        if self._arena_buf is not None:
            self._arena_buf.zero_()
        if self.ring == "seamless":
            self._frames[:self.frame_window].zero_()
        if self.frame_tags is not None:
            if self._arena_buf is not None or self.ring == "seamless":
                self.frame_tags.zero_()  # every frame was just zeroed: tag 0 holds for every granule
            else:
                self.invalidate_frame_tags()
        self._needs_reset = True

    def _autotune_raster(self) -> None:
        self.reset()  # a real state (a zeroed record would stack every disc on the robot cell)
        self._warm_tags()
        results = []
        steps = self._tune_steps()
        for shape in self._shape_candidates():
            self.raster_shape = self.raster_shape_newest = shape
            results.append((self._raster_gbs_steady(steps), shape))
        best = {}
        for kind in (True, False):
            got = [(r[kind][0], r[kind][1], shape) for r, shape in results if kind in r]
            if got:
                best[kind] = max(got)
        if True in best:
            self.raster_shape = best[True][2]
        else:  # seamless ring: steps never write both frames; resets use the newest-only winner
            self.raster_shape = best[False][2]
        self.raster_shape_newest = best[False][2] if False in best else self.raster_shape
        gbs = self._cycle_gbs(best[True][1] if True in best else None, best[False][1] if False in best else None)
        fused = self._tune_fused(steps)
        self.placement = {"shape": {"cells_per_block": self.raster_shape[0], "flags": self.raster_shape[1]},
                          "shape_newest": ({"cells_per_block": self.raster_shape_newest[0],
                                            "flags": self.raster_shape_newest[1]} if False in best else None),
                          "gbs": round(gbs, 1),
                          "candidates": [[c, f] + [round(r[k][0], 1) for k in (True, False) if k in r]
                                         for r, (c, f) in results],
                          "fused": fused}
        self._clear_after_tuning()

    # Fused-step candidates (ffmp_step_fused flags; a block is a whole plane, so no cells/block)
    FUSED_FLAGS = (
        _abi.RASTER_NT, _abi.RASTER_PLAIN, _abi.RASTER_NT | _abi.RASTER_XCD, _abi.RASTER_PLAIN | _abi.RASTER_XCD,
        _abi.RASTER_NT | _abi.RASTER_TILE4, _abi.RASTER_NT | _abi.RASTER_XCD | _abi.RASTER_TILE4,
        _abi.RASTER_PLAIN | _abi.RASTER_TILE4, _abi.RASTER_NT | _abi.RASTER_TILE2,
        _abi.RASTER_NT | _abi.RASTER_XCD | _abi.RASTER_TILE2, _abi.RASTER_NT | _abi.RASTER_TILE8,
        # granule tags only: the TILE4 / TILE2 / row-run candidates again, held to 6 waves per SIMD
        # (RASTER_WAVES; profiles/fused_waves_variants.json)
        _abi.RASTER_NT | _abi.RASTER_TILE4 | _abi.RASTER_WAVES,
        _abi.RASTER_NT | _abi.RASTER_XCD | _abi.RASTER_TILE4 | _abi.RASTER_WAVES,
        _abi.RASTER_PLAIN | _abi.RASTER_TILE4 | _abi.RASTER_WAVES, _abi.RASTER_NT | _abi.RASTER_TILE2 | _abi.RASTER_WAVES,
        _abi.RASTER_NT | _abi.RASTER_XCD | _abi.RASTER_TILE2 | _abi.RASTER_WAVES, _abi.RASTER_NT | _abi.RASTER_WAVES,
    )

    # The compact format (obs_format="u8f16") writes 3 bytes per cell and is bound by the per-task
    # cull / wall / index work rather than by HBM (tools/compact_probe.py): 16 cells per lane
    # (1024-cell wave tasks) by default, tiles R x 1024/R; NARROW = the 4-cells-per-lane kernel.
    # (round 2: the 16-cells-per-lane tiles hoist their columns' work out of the tile loop;
    # tools/compact_shapes.py: whole-plane blocks, 4- or 16-cell lanes, 1.46-1.55 ms at C3)
    COMPACT_SHAPES = (
        (65536, _abi.RASTER_NT | _abi.RASTER_TILE4 | _abi.RASTER_NARROW),
        (32768, _abi.RASTER_NT | _abi.RASTER_TILE4 | _abi.RASTER_NARROW),
        (16384, _abi.RASTER_NT | _abi.RASTER_TILE4 | _abi.RASTER_NARROW),
        (65536, _abi.RASTER_PLAIN | _abi.RASTER_TILE16), (32768, _abi.RASTER_NT | _abi.RASTER_TILE16),
        (16384, _abi.RASTER_NT | _abi.RASTER_TILE16), (65536, _abi.RASTER_NT | _abi.RASTER_TILE4),
        (16384, _abi.RASTER_NT | _abi.RASTER_TILE8), (16384, _abi.RASTER_PLAIN | _abi.RASTER_TILE16),
        (32768, _abi.RASTER_PLAIN | _abi.RASTER_TILE4 | _abi.RASTER_NARROW),
        # round 3: 4-cell lanes in 2 x 128-cell tiles or 256-cell rows, so that a wave's uint8 frame
        # stores cover whole 128-byte lines (TILE4's 64-cell rows write half lines: PMC 1.02x)
        (32768, _abi.RASTER_NT | _abi.RASTER_TILE2 | _abi.RASTER_NARROW),
        (65536, _abi.RASTER_NT | _abi.RASTER_TILE2 | _abi.RASTER_NARROW),
        (32768, _abi.RASTER_NT | _abi.RASTER_NARROW),
        # round 3: 8 cells per lane (an 8-B frame and a 16-B potential store per lane), 4 x 128-cell
        # tiles, 6 waves per SIMD: 0.954-0.985 ms against the 4-cell tiles' 1.00-1.03 at C3
        # (profiles/r03b_ct8_shapes.txt)
        (65536, _abi.RASTER_NT | _abi.RASTER_TILE4 | _abi.RASTER_MID8),
        (32768, _abi.RASTER_NT | _abi.RASTER_TILE4 | _abi.RASTER_MID8),
        (65536, _abi.RASTER_NT | _abi.RASTER_TILE8 | _abi.RASTER_MID8),
        (65536, _abi.RASTER_NT | _abi.RASTER_XCD | _abi.RASTER_TILE4 | _abi.RASTER_MID8),
    )
    COMPACT_FUSED_FLAGS = (
        _abi.RASTER_NT | _abi.RASTER_TILE16, _abi.RASTER_NT | _abi.RASTER_TILE8, _abi.RASTER_NT | _abi.RASTER_TILE4,
        _abi.RASTER_NT | _abi.RASTER_TILE4 | _abi.RASTER_NARROW, _abi.RASTER_PLAIN | _abi.RASTER_TILE16,
        _abi.RASTER_NT | _abi.RASTER_XCD | _abi.RASTER_TILE16, _abi.RASTER_NT,
        _abi.RASTER_NT | _abi.RASTER_TILE2 | _abi.RASTER_NARROW,
        _abi.RASTER_NT | _abi.RASTER_TILE4 | _abi.RASTER_MID8,
    )

    XCD_SHAPES = True  # autotune candidates include the XCD-aware block remap

    # With granule tags the 8-row tiles (32-cell row segments, half a granule) store every cell and
    # leave tag 1 behind, which would also make the next candidate's first ring cycle dense: dropped.
    # The RASTER_WAVES forms select a kernel of their own only with tags (float32 frames, no flow
    # planes); elsewhere the library ignores the flag, so they would time a candidate twice: dropped.
    # RASTER_DIRECT likewise, and only in the two-launch raster (the one-launch step ignores it).
    def _offered(self, flags: int) -> bool:
        tags = self.frame_tags is not None
        if flags & (_abi.RASTER_WAVES | _abi.RASTER_DIRECT) and not (tags and self.obs_format == "f32" and not self.cfg.flow):
            return False
        return (self.XCD_SHAPES or not flags & _abi.RASTER_XCD) and not (tags and flags & _abi.RASTER_TILE8)

    def _shape_candidates(self):
        shapes = self.COMPACT_SHAPES if self.obs_format == "u8f16" else self.RASTER_SHAPES + self.DIRECT_SHAPES
        return [sh for sh in shapes if self._offered(sh[1])]

    def _fused_candidates(self):
        flags = self.COMPACT_FUSED_FLAGS if self.obs_format == "u8f16" else self.FUSED_FLAGS
        return [f for f in flags if self._offered(f) and not f & _abi.RASTER_DIRECT]

    def _warm_tags(self) -> None:
        """One untimed ring cycle of real steps, so that every slot a timed step overwrites holds a
        stepped frame with exact tags (after a reset the slots beyond the pair hold zeros or unknown
        tags, and re-rastering one record would make old and new discs coincide: about half the
        granules a real step stores).  The shape ranking, the placement check and the one- /
        two-launch recheck then time the raster under the tags of the steady state."""
        if self.frame_tags is None:
            return
        a = torch.full((self.num_envs,), 10, dtype=torch.int64, device=self.device)
        for _ in range(self.frame_window):
            self.step(a)

    def _tune_fused(self, steps: int) -> Optional[dict]:
        """Time whole steps of the two-launch path (the tuned raster shapes) against the fused
        step for each FUSED_FLAGS candidate; keep the faster (fused=None), or the best fused flags
        (fused=True)."""
        if self._fused_req is False or self.pipeline_slices > 1:
            self.fused = False
            return None
        self.fused = False
        sep = self._raster_gbs_steady(steps)["step_ms"]
        self.fused = True
        res = []
        for f in self._fused_candidates():
            self.fused_flags = f
            res.append((self._raster_gbs_steady(steps)["step_ms"], f))
        best_ms, best_f = min(res)
        self.fused_flags = best_f
        self.fused = bool(self._fused_req) or best_ms < 0.995 * sep
        return {"chosen": self.fused, "two_launch_step_ms": round(sep, 4), "fused_step_ms": round(best_ms, 4),
                "flags": best_f, "candidates": [[f, round(m, 4)] for m, f in res]}

    def _recheck_fused(self) -> None:
        """The one- or two-launch decision again, on the repaired ring.  _autotune_raster makes it
        before the slot repair, whose rebuilt slots change the step time by 5-10 %, and the two
        kinds are within ~2 % of each other at C3: on three fresh runs of one box the pre-repair
        choice kept the two-launch step at 2.48-2.50 ms where the one-launch step ran 2.44 ms
        (profiles/r02_fused_recheck.txt).  Two alternating rounds of two ring cycles each, the
        better of each kind; the autotune's best fused flags; the two-launch step only if it is
        0.5 % faster."""
        tf = (self.placement or {}).get("fused")
        if self._fused_req is not None or self.pipeline_slices > 1 or not tf:
            return
        self.reset()
        self._warm_tags()
        steps = 2 * self._tune_steps()
        rounds = 2
        if max(tf.get("two_launch_step_ms", 1.0), tf.get("fused_step_ms", 1.0)) < self.SHORT_STEP_MS:
            # short steps (C2: ~0.1 ms) vary by several % between rounds of a few steps, and the
            # one- and two-launch steps are within that of each other (a 2-round pick
            # kept a path 3 % slower): more and longer alternating rounds, compared by their medians
            rounds = self.SHORT_STEP_ROUNDS
            cyc = max(1, self.graph_period())
            steps = max(steps, -(-self.SHORT_STEP_MIN_STEPS // cyc) * cyc)
        ms = {False: [], True: []}
        for _ in range(rounds):
            for kind in (False, True):
                self.fused = kind
                self.fused_flags = tf["flags"]
                ms[kind].append(self._raster_gbs_steady(steps)["step_ms"])
        pick = min if rounds <= 2 else (lambda v: float(np.median(v)))
        sep, fus = pick(ms[False]), pick(ms[True])
        # ties go to the one-launch step: on the repaired ring it was the faster one on every box
        # measured (0.3-1.4 %), the two-launch step only ahead on poorly paired rings
        self.fused = not (sep < 0.995 * fus)
        self._clear_after_tuning()
        self.placement = dict(self.placement, fused=dict(tf, chosen=self.fused, recheck={
            "two_launch_step_ms": round(sep, 4), "fused_step_ms": round(fus, 4), "rounds": rounds,
            "steps_per_round": steps, "statistic": "min" if rounds <= 2 else "median",
            "two_launch_rounds_ms": [round(v, 4) for v in ms[False]],
            "fused_rounds_ms": [round(v, 4) for v in ms[True]]}))

    SHORT_STEP_MS = 0.5        # below this, the one- / two-launch recheck takes SHORT_STEP_ROUNDS rounds ...
    SHORT_STEP_ROUNDS = 8      # ... alternating, of >= SHORT_STEP_MIN_STEPS steps each (whole ring cycles)
    SHORT_STEP_MIN_STEPS = 50

    def _placement_gbs(self) -> float:
        """Cycle bandwidth of the current buffers with the current launch shapes."""
        self.reset()
        self._warm_tags()
        r = self._raster_gbs_steady(self._tune_steps())
        gbs = self._cycle_gbs(r[True][1] if True in r else None, r[False][1] if False in r else None)
        self._clear_after_tuning()
        return gbs

    def _build_structs(self):
        self._cfg_c = _abi.make_cfg(self.cfg, _ptr(self.beam_cs) or 0)
        self._state_c = _abi.StateT(self.pose.data_ptr(), self.goal.data_ptr(), self.d0.data_ptr(),
                                    self.obst.data_ptr(), self.obst_r.data_ptr(), self.t.data_ptr(),
                                    self.episode.data_ptr(), self.record.data_ptr(), self.err.data_ptr(),
                                    _ptr(self.term_record), _ptr(self.term_obs))
        G2 = self.cfg.grid * self.cfg.grid
        obs_t = _abi.ObsT if self.frame_tags is None else _abi.ObsTagsT
        self._obs_c = obs_t(self.state_m.data_ptr(), self.state_g.data_ptr(), self.state_v.data_ptr(),
                            self.state_t.data_ptr(), _ptr(self.potential), self.grad.data_ptr(),
                            _ptr(self.lidar), _ptr(self.flow), *self._sm_strides(), self._fmt)
        self._set_tags(self._wpos)
        self._out_c = _abi.OutT(self.reward.data_ptr(), self.done.data_ptr(), self.is_goal.data_ptr(),
                                self.collision.data_ptr(), self.truncated.data_ptr())
        self._build_slices()

    # Optional pipelined step (pipeline=S > 1): the env kernel of slice s+1 runs on a
    # high-priority side stream while the raster of slice s runs on the caller's stream.
    # Results are identical; on MI355X it did not pay (the raster fills every CU, the slices
    # add kernel tails), so the default is the serial step.

    def _build_slices(self):
        N, S = self.num_envs, self.pipeline_slices
        bounds = [N * k // S for k in range(S + 1)]

        def off(t, e0):
            return None if t is None else t.data_ptr() + e0 * t.stride(0) * t.element_size()

        self._slices = []
        for k in range(S):
            a, n = bounds[k], bounds[k + 1] - bounds[k]
            st = _abi.StateT(off(self.pose, a), off(self.goal, a), off(self.d0, a), off(self.obst, a),
                             off(self.obst_r, a), off(self.t, a), off(self.episode, a), off(self.record, a),
                             self.err.data_ptr(), off(self.term_record, a), off(self.term_obs, a))
            ob = _abi.ObsT(off(self.state_m, a), off(self.state_g, a), off(self.state_v, a), off(self.state_t, a),
                           off(self.potential, a), off(self.grad, a), off(self.lidar, a), off(self.flow, a), 0, 0,
                           self._fmt)
            out = _abi.OutT(off(self.reward, a), off(self.done, a), off(self.is_goal, a), off(self.collision, a),
                            off(self.truncated, a))
            self._slices.append((a, n, st, ob, out, off(self.record, a)))
        if S > 1 and getattr(self, "_side", None) is None:
            lo, hi = torch.cuda.Stream.priority_range()
            self._side = torch.cuda.Stream(self.device, priority=hi)  # env kernels first
            self._ev_go = torch.cuda.Event()
        if S > 1 and len(getattr(self, "_ev_slice", ())) != S:
            self._ev_slice = [torch.cuda.Event() for _ in range(S)]

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    # ------------------------------------------------------------ frame window
    @property
    def state_m(self) -> torch.Tensor:
        """(N, 2, G, G) [older, newest] view of the frame window (contiguous iff W == 2).
        Read-only for consumers, like `frames`: with sparse_frames the raster skips stores into
        granules it knows to be zero, so a caller that writes into the ring must call
        invalidate_frame_tags() before the next step."""
        if self.frame_window == 2:
            return self._frames
        return self._frames[self._wpos:self._wpos + 2].transpose(0, 1)

    def _sm_strides(self):
        """(env stride, frame stride) of state_m in elements, for ffmp_obs_t."""
        G2 = self.cfg.grid * self.cfg.grid
        if self.frame_window == 2:
            return (2 * G2, G2)
        return (G2, self._frames.stride(0))

    # Seamless ring, wrap step (pair [W-1, W]): the newest frame goes to physical slot 0, which
    # virtual slots 0 and W both map.  WRAP_VIA_ALIAS False: the raster writes it through slot
    # 0's own addresses (negative frame stride from slot W-1); the state_m view still reads it
    # through slot W.  Same bytes either way.
    WRAP_VIA_ALIAS = True

    def _set_tags(self, p: int) -> None:
        """Point the launch struct at the tags of the PHYSICAL slots of the pair [p, p + 1]: the
        seamless ring's virtual slot W is slot 0 (through the alias or the negative frame stride
        alike); the wrapping ring and the contiguous pair never leave [0, slots)."""
        tg = self.frame_tags
        if tg is None:
            return
        o, slots = self._obs_c, tg.shape[0]
        o.reserved = _abi.OBS_EXT_TAGS
        o.tags_older = tg.data_ptr() + (p % slots) * tg.stride(0)
        o.tags_newest = tg.data_ptr() + ((p + 1) % slots) * tg.stride(0)
        o.tags_env_stride = tg.stride(1)

    def _set_window(self, p: int) -> None:
        self._wpos = p
        self._set_tags(p)
        self._obs_c.state_m = self._frames.data_ptr() + p * self._frames.stride(0) * self._fes
        if self.ring == "seamless":
            W, fs = self.frame_window, self._frames.stride(0)
            wrap = p == W - 1 and not self.WRAP_VIA_ALIAS
            self._obs_c.state_m_frame_stride = -(W - 1) * fs if wrap else fs

    def _note_window(self, full: bool) -> None:
        """Frame history after a raster at the current window: the newest frame's slot first;
        a full raster also rewrote the older slot (with the previous newest frame)."""
        if self.frame_window == 2:
            return
        W = self.frame_window
        new, old = (self._wpos + 1) % W, self._wpos % W
        prev = self._hist
        if full:
            self._hist = [new, old] + [s for s in prev[1:] if s not in (new, old)]
        else:
            self._hist = [new] + [s for s in prev if s != new]
        del self._hist[W:]
        if len(self._hist) < len(prev) + 1:
            # a frame of the history was overwritten: lags beyond the list are no longer
            # guaranteed to be clamped away
            self._hist_from_reset = False

    @property
    def max_temporal_frames(self) -> int:
        """The largest k temporal_maps(k) can serve at every step: W for the seamless ring and the
        contiguous pair, W - 1 for the wrapping ring (its wrap re-rasters the newest frame into slot 0,
        so after the first wrap it holds W - 1 distinct frames)."""
        return self.frame_window - 1 if self.ring == "wrap" else self.frame_window

    def _bev_push(self, advance: bool, restart: bool = False) -> None:
        """Write the current BEV image of every env into the ring (bev_series): a new slot after a
        step (advance), the current one again after a re-raster or masked reset, slot 0 after a full
        reset (restart: every env's older lags are clamped away)."""
        if self.bev is None:
            return
        S = self.bev.shape[0]
        if restart:
            self._bev_pos, self._bev_hist, self._bev_from_reset = 0, [0], True
        elif advance:
            self._bev_pos = (self._bev_pos + 1) % S
            self._bev_hist = ([self._bev_pos] + self._bev_hist)[:S]
        elif not self._bev_hist:
            self._bev_hist = [self._bev_pos]
        G2 = self.cfg.grid * self.cfg.grid
        sm = self.state_m
        with torch.cuda.device(self.device):
            self._bev_launch(sm, G2)

    def _bev_launch(self, sm: torch.Tensor, G2: int) -> None:
        _abi.check(self.lib.ffmp_bev_image(self.num_envs, 1 if self.obs_format == "u8f16" else 0,
                                           sm[:, 1].data_ptr(), sm.stride(0), self.flow.data_ptr(), G2,
                                           float(np.float32(self.cfg.obst_vmax)), self.bev[self._bev_pos].data_ptr(),
                                           4 * G2, self._stream()), "ffmp_bev_image")

    def bev_maps(self, k: Optional[int] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """make_temporal_maps over the last k 4-channel BEV images (bev_series): (N, 4k, G, G),
        oldest image first, each [occupancy, R, G, B] (include/ffmp.h ffmp_bev_image), every env's
        lags clamped to its episode start as in temporal_maps (is_first refills map_memory) — the
        reference's INPUT_CHANNELS = 12 option at k = 3 (train.py:66, ffmp.py:16).  Gathered by
        ffmp_temporal_maps from the ring into `out` (or a new tensor; frames' dtype)."""
        self._check_open()
        if self.bev is None:
            raise RuntimeError("bev_maps() needs FFMPVec(..., bev_series=k)")
        S = self.bev.shape[0]
        k = S if k is None else int(k)
        if not 1 <= k <= S:
            raise ValueError(f"k must be in [1, {S}] (bev_series={S})")
        if self._needs_reset:
            raise RuntimeError("call reset() before bev_maps()")
        if len(self._bev_hist) < k and not self._bev_from_reset:
            raise RuntimeError(f"the BEV ring holds {len(self._bev_hist)} known images since the last reload; "
                               f"bev_maps({k}) needs {k} (step {k - len(self._bev_hist)} more times, or reset())")
        N, G = self.num_envs, self.cfg.grid
        plane = 4 * G * G
        hist = self._bev_hist
        offs = [hist[min(d, len(hist) - 1)] * N * plane for d in range(k)]
        if out is None:
            out = torch.empty(N, 4 * k, G, G, dtype=self.bev.dtype, device=self.device)
        elif out.shape != (N, 4 * k, G, G) or out.dtype != self.bev.dtype or not out.is_contiguous() \
                or out.device != self.device:
            raise ValueError(f"out must be a contiguous {self.bev.dtype} tensor of shape {(N, 4 * k, G, G)} on {self.device}")
        lag = (C.c_int64 * k)(*offs)
        _abi.check(self.lib.ffmp_temporal_maps(N, self.bev.data_ptr(), lag, k, plane, plane, self._fes,
                                               self.t.data_ptr(), out.data_ptr(), self._stream()), "ffmp_temporal_maps")
        return out

    def temporal_maps(self, k: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """make_temporal_maps (src/train.py:474-486) over the last k frames: (N, k, G, G), oldest
        first, each env's lags clamped to its episode start (is_first refills the reference's
        map_memory with the first frame) — the reference's INPUT_CHANNELS = k with a mono BEV
        image (train.py:66-69).  k <= 2: a view of state_m.  k > 2: gathered from the frame ring
        (k <= frame_window) by ffmp_temporal_maps into `out` (or a new tensor)."""
        self._check_open()
        k = int(k)
        if k < 1:
            raise ValueError("k must be >= 1")
        if k <= 2 and out is None:
            return self.state_m[:, 2 - k:]
        if k > self.max_temporal_frames or k > _abi.MAX_SERIES:
            raise ValueError(f"temporal_maps({k}) needs at most {self.max_temporal_frames} frames here "
                             f"(frame_window={self.frame_window}, ring={self.ring}: a wrapping ring re-rasters "
                             f"its newest frame into slot 0 and keeps W - 1 distinct frames; at most "
                             f"{_abi.MAX_SERIES})")
        if self._needs_reset:
            raise RuntimeError("call reset() before temporal_maps()")
        N, G = self.num_envs, self.cfg.grid
        if self.frame_window == 2:
            offs = [G * G, 0]  # contiguous (N, 2, G, G): newest, older
            env_stride = 2 * G * G
        else:
            if len(self._hist) < k and not self._hist_from_reset:
                raise RuntimeError(f"the frame ring holds {len(self._hist)} known frames since the last reload; "
                                   f"temporal_maps({k}) needs {k} (step {k - len(self._hist)} more times, or reset())")
            # lags the ring has not seen since a full reset are never read (every env's lag is
            # clamped to its steps since that reset): any valid slot stands in
            offs = [self._hist[min(d, len(self._hist) - 1)] * self._frames.stride(0) for d in range(k)]
            env_stride = G * G
        offs = (offs + [offs[-1]] * k)[:k]
        if out is None:
            out = torch.empty(N, k, G, G, dtype=self._frames.dtype, device=self.device)
        elif out.shape != (N, k, G, G) or out.dtype != self._frames.dtype or not out.is_contiguous() \
                or out.device != self.device:
            raise ValueError(f"out must be a contiguous {self._frames.dtype} tensor of shape {(N, k, G, G)} on {self.device}")
        lag = (C.c_int64 * k)(*offs)
        _abi.check(self.lib.ffmp_temporal_maps(N, self._frames.data_ptr(), lag, k, env_stride, G * G, self._fes,
                                               self.t.data_ptr(), out.data_ptr(), self._stream()), "ffmp_temporal_maps")
        return out

    def _raster_bytes(self, n: int, full: bool) -> int:
        """Algorithmic bytes of one raster launch over n envs (excluding the older frames of envs
        reset during a newest-only launch: one frame each, added by bench.py from the episode counts)."""
        G2 = self.cfg.grid * self.cfg.grid
        per = (2 if full else 1) * self._fes * G2 + (self._pes * G2 if self.potential is not None else 0) + \
            (2 * self._pes * G2 if self.flow is not None else 0) + 4 * self.cfg.record_len()
        return n * per

    def _raster_launch(self, full: bool, mask=None, timing: Optional[list] = None) -> None:
        self._check_open()
        cpb, flags = self.raster_shape if full else self.raster_shape_newest
        flags |= 0 if full else _abi.RASTER_NEWEST
        if timing is not None:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        _abi.check(self.lib.ffmp_raster_ex(C.byref(self._cfg_c), self.num_envs, self.record.data_ptr(), _ptr(mask),
                                           C.byref(self._obs_c), cpb, flags, self._stream()), "ffmp_raster")
        if timing is not None:
            e1.record()
            timing.append((e0, e1, self.num_envs, self._raster_bytes(self.num_envs, full), full))

    # --------------------------------------------------------------- gym API
    @property
    def obs(self) -> Dict[str, torch.Tensor]:
        d = {"state_m": self.state_m, "state_g": self.state_g, "state_v": self.state_v, "state_t": self.state_t,
             "grad": self.grad}
        if self.potential is not None:
            d["potential"] = self.potential
        if self.lidar is not None:
            d["lidar"] = self.lidar
        if self.flow is not None:
            d["flow"] = self.flow
        return d

    def _obs_out(self, copy: bool):
        o = self.obs
        return {k: v.clone() for k, v in o.items()} if copy else o

    def reset(self, seed: Optional[int] = None, mask: Optional[torch.Tensor] = None, copy: bool = False):
        """Reset all envs (mask None: new episodes 0 from `seed`) or only masked ones."""
        self._check_open()
        with torch.cuda.device(self.device):
            if seed is not None:
                self._set_cfg(self.cfg.replace(seed=int(seed)))
            m = None
            if mask is not None:
                m = mask.to(device=self.device, dtype=torch.bool).contiguous().view(torch.uint8)
                if m.numel() != self.num_envs:
                    raise ValueError("mask must have num_envs elements")
            initial = 1 if (mask is None) else 0
            s = self._stream()
            if mask is None:
                self._set_window(0)
                self._hist, self._hist_from_reset = [], True
                self._note_window(True)
            _abi.check(self.lib.ffmp_reset(C.byref(self._cfg_c), self.num_envs, self.env_offset, _ptr(m), initial,
                                           C.byref(self._state_c), C.byref(self._obs_c), s), "ffmp_reset")
            self._raster_launch(True, m)
            self._mask_keepalive = m
            self._bev_push(advance=False, restart=mask is None)
        self._needs_reset = False
        return self._obs_out(copy)

    # ------------------------------------------------ injected episodes (SPEC a16b)
    def set_scenarios(self, pose, goal, obst=None, obst_r=None, mask=None, episode=None, copy: bool = False):
        """Put the masked envs (mask None: all) into the caller's episodes (include/ffmp.h
        ffmp_set_scenario): the masked reset with the sampled start / goal / discs replaced by
        `pose` (N, 3) x, y, yaw, `goal` (N, 2), `obst` (N, K, 4) x, y, vx, vy and `obst_r` (N, K)
        — tensors or arrays, float32 (widened exactly) or float64, on any device; with K == 0 the
        obst arguments may be omitted.  `episode` (N,) integers: the envs' new episode counters (None:
        episode + 1, as a masked reset) — a later auto-reset samples (seed, episode + 1, env).  An env
        with a non-finite word, a negative radius or |yaw| > 1024 stays as it was and sets error bit
        4 (check_errors: "bad scenario").  The frame window does not move (so step graphs captured
        before stay valid); needs a prior reset().  Returns the observation, like reset()."""
        self._check_open()
        if self._needs_reset:
            raise RuntimeError("call reset() before set_scenarios()")
        sc = scenario_tensors(self.num_envs, self.cfg.n_obst, pose, goal, obst, obst_r, episode, self.device)
        with torch.cuda.device(self.device):
            m = None
            if mask is not None:
                m = torch.as_tensor(mask).to(device=self.device, dtype=torch.bool).contiguous().view(torch.uint8)
                if m.numel() != self.num_envs:
                    raise ValueError("mask must have num_envs elements")
            _abi.check(self.lib.ffmp_set_scenario(C.byref(self._cfg_c), self.num_envs, self.env_offset, _ptr(m),
                                                  sc["pose"].data_ptr(), sc["goal"].data_ptr(), _ptr(sc["obst"]),
                                                  _ptr(sc["obst_r"]), _ptr(sc["episode"]), C.byref(self._state_c),
                                                  C.byref(self._obs_c), self._stream()), "ffmp_set_scenario")
            self._raster_launch(True, m)
            self._mask_keepalive, self._scenario_keepalive = m, sc
            self._bev_push(advance=False)
        return self._obs_out(copy)

    def scenarios(self, mask=None) -> Dict[str, torch.Tensor]:
        """The envs' episodes as set_scenarios takes them: clones of pose (N, 3), goal (N, 2), obst
        (N, K, 4), obst_r (N, K) and episode (N,) — of the masked envs only (M rows, in env order)
        with `mask`.  Fed back at t == 0 (straight after a reset or an injection) they reproduce the
        env, later auto-resets included."""
        self._check_open()
        K = self.cfg.n_obst
        d = {"pose": self.pose, "goal": self.goal, "obst": self.obst[:, :K], "obst_r": self.obst_r[:, :K],
             "episode": self.episode}
        if mask is None:
            return {k: v.clone() for k, v in d.items()}
        m = torch.as_tensor(mask).to(device=self.device, dtype=torch.bool).reshape(-1)
        if m.numel() != self.num_envs:
            raise ValueError("mask must have num_envs elements")
        return {k: v[m].clone() for k, v in d.items()}

    def _actions(self, actions) -> torch.Tensor:
        a = torch.as_tensor(actions)
        if a.device != self.device or a.dtype != torch.int64:
            a = a.to(device=self.device, dtype=torch.int64)
        a = a.reshape(-1)
        if a.numel() != self.num_envs:
            raise ValueError(f"expected {self.num_envs} actions, got {a.numel()}")
        return a.contiguous()

    def _commands(self, cmds) -> torch.Tensor:
        """(N, 2) float64 (v, w) commands on the device, contiguous and 16-byte aligned (the env
        kernel reads each row as one 16-byte load); float32 is widened exactly."""
        c = torch.as_tensor(cmds)
        if not c.is_floating_point() or tuple(c.shape) != (self.num_envs, 2):
            raise ValueError(f"commands must be a floating tensor of shape ({self.num_envs}, 2), got "
                             f"{c.dtype} {tuple(c.shape)}")
        if c.dtype not in (torch.float32, torch.float64):
            raise ValueError(f"commands must be float32 or float64, got {c.dtype}")
        if c.device != self.device or c.dtype != torch.float64:
            c = c.to(device=self.device, dtype=torch.float64)
        c = c.contiguous()
        if c.data_ptr() % 16:
            c = c.clone()
        return c

    def _act_in(self, actions) -> Tuple[torch.Tensor, bool]:
        """step()'s input dispatch (SPEC a15b): an integer tensor of N elements -> (ids (N,) int64,
        False), today's path; a floating tensor of shape (N, 2) -> ((N, 2) float64 (v, w) commands,
        True); anything else raises ValueError."""
        a = torch.as_tensor(actions)
        if a.is_floating_point():
            return self._commands(a), True
        if a.is_complex():
            raise ValueError("actions must be integer ids (N,) or floating (v, w) commands (N, 2)")
        return self._actions(a), False

    def step_state(self, actions: torch.Tensor) -> None:
        """Kernel 1 of a step: dynamics, lidar, reward/done, auto-reset, record."""
        self._check_open()
        a, is_cmd = self._act_in(actions)
        self._act_keepalive = a
        fn, what = (self.lib.ffmp_step_state_cmd, "ffmp_step_state_cmd") if is_cmd else \
            (self.lib.ffmp_step_state, "ffmp_step_state")
        _abi.check(fn(C.byref(self._cfg_c), self.num_envs, self.env_offset, a.data_ptr(), C.byref(self._state_c),
                      C.byref(self._obs_c), C.byref(self._out_c), self._stream()), what)

    def raster(self, mask: Optional[torch.Tensor] = None) -> None:
        """Re-raster the current observation (both frames, potential, flow) from the record."""
        self._check_open()
        m = None if mask is None else mask.to(device=self.device, dtype=torch.bool).contiguous().view(torch.uint8)
        if self.frame_tags is not None:
            # an explicit re-raster rewrites the pair whatever it holds (a reloaded checkpoint, a
            # caller that wrote into state_m): no store of it is skipped
            slots = self.frame_tags.shape[0]
            self.invalidate_frame_tags([self._wpos % slots, (self._wpos + 1) % slots])
        self._raster_launch(True, m)
        self._bev_push(advance=False)

    def _next_window(self) -> bool:
        """Slide the [older, newest] pair by one slot for the next raster; True if that raster
        must write both frames (the wrapping ring's wrap, or W = 2)."""
        p = self._wpos + 1
        if self.ring == "seamless":  # virtual slot W is slot 0: the pair slides forever
            full = False
            p %= self.frame_window
        else:
            full = p > self.frame_window - 2
        self._set_window(0 if full else p)
        self._note_window(full)
        return full

    def _state_bytes(self, n: int) -> int:
        """Algorithmic bytes of the env step itself over n envs (state read + write, small obs,
        lidar, record write, action, reward and flags; config.bytes_per_env_step "state")."""
        from .config import bytes_per_env_step
        return n * bytes_per_env_step(self.cfg, potential=self.potential is not None)["state"]

    def _step_fused(self, actions, timing: Optional[list] = None) -> None:
        """Env step + raster in one launch (ffmp_step_fused): one block per env."""
        self._check_open()
        a, is_cmd = self._act_in(actions)
        self._act_keepalive = a
        full = self._next_window()
        flags = self.fused_flags | (0 if full else _abi.RASTER_NEWEST)
        if timing is not None:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        fn, what = (self.lib.ffmp_step_fused_cmd, "ffmp_step_fused_cmd") if is_cmd else \
            (self.lib.ffmp_step_fused, "ffmp_step_fused")
        _abi.check(fn(C.byref(self._cfg_c), self.num_envs, self.env_offset, a.data_ptr(), C.byref(self._state_c),
                      C.byref(self._obs_c), C.byref(self._out_c), flags, self._stream()), what)
        if timing is not None:
            e1.record()
            n = self.num_envs
            timing.append((e0, e1, n, self._raster_bytes(n, full) + self._state_bytes(n), full))

    def raster_step(self, timing: Optional[list] = None) -> None:
        """Kernel 2 of a step (the HBM-bound hot kernel): slide the frame pair by one and raster
        the new frame + potential (+ flow), or both frames when the window wraps or W == 2."""
        self._check_open()
        full = self._next_window()
        self._raster_launch(full, None, timing)

    def _step_pipelined(self, actions, timing) -> None:
        self._check_open()
        a, is_cmd = self._act_in(actions)
        self._act_keepalive = a
        main = torch.cuda.current_stream(self.device)
        side = self._side
        self._ev_go.record(main)
        side.wait_event(self._ev_go)
        sp = C.c_void_p(side.cuda_stream)
        # a slice's inputs start a0 ids (8 B each) or a0 (v, w) rows (16 B each) into the array
        fn, what, esz = (self.lib.ffmp_step_state_cmd, "ffmp_step_state_cmd", 16) if is_cmd else \
            (self.lib.ffmp_step_state, "ffmp_step_state", 8)
        for k, (a0, n, st, ob, out, rec) in enumerate(self._slices):
            _abi.check(fn(C.byref(self._cfg_c), n, self.env_offset + a0, a.data_ptr() + a0 * esz, C.byref(st),
                          C.byref(ob), C.byref(out), sp), what)
            self._ev_slice[k].record(side)
        # the raster of slice k on the main stream once its env slice is done: the env kernels of the
        # later slices run beside it.  The frame pair slides as in raster_step (ring or contiguous).
        full = self._next_window()
        cpb, flags = self.raster_shape if full else self.raster_shape_newest
        flags |= 0 if full else _abi.RASTER_NEWEST
        sm0, sm_stride, sm_frame = self._obs_c.state_m, self._obs_c.state_m_stride, self._obs_c.state_m_frame_stride
        mp = C.c_void_p(main.cuda_stream)
        for k, (a0, n, st, ob, out, rec) in enumerate(self._slices):
            ob.state_m = sm0 + a0 * sm_stride * self._fes
            ob.state_m_stride, ob.state_m_frame_stride = sm_stride, sm_frame
            main.wait_event(self._ev_slice[k])
            if timing is not None:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(main)
            _abi.check(self.lib.ffmp_raster_ex(C.byref(self._cfg_c), n, rec, None, C.byref(ob), cpb, flags, mp),
                       "ffmp_raster")
            if timing is not None:
                e1.record(main)
                timing.append((e0, e1, n, self._raster_bytes(n, full), full))

    def step(self, actions, copy: bool = False, timing: Optional[list] = None
             ) -> Tuple[Dict[str, torch.Tensor], torch.Tensor, torch.Tensor, dict]:
        """Advance every env one step. Returns (obs, reward f32[N], done bool[N], info).

        `timing`: optional list; (start, end, n_envs, algorithmic bytes, full) per raster launch
        (HIP events on the caller's stream) are appended to it.  With use_graphs(True) (and no
        `timing`) the step's launches run as the replay of a single-step HIP graph (step_graphs)."""
        self._check_open()
        if self._needs_reset:
            raise RuntimeError("call reset() before step()")
        with torch.cuda.device(self.device):
            if self._graphs is not None and timing is None:
                self._step_graph(actions)
            elif self.pipeline_slices > 1:
                self._step_pipelined(actions, timing)
            elif self.fused:
                self._step_fused(actions, timing)
            else:
                self.step_state(actions)
                self.raster_step(timing)
            self._bev_push(advance=True)
        if self.info_format == "list":
            info = self._info_list()
        else:
            info = {"is_goal": self.is_goal, "collision": self.collision, "truncated": self.truncated,
                    "step": self.t, "episode": self.episode}
            if copy:
                info = {k: v.clone() for k, v in info.items()}
        if copy:
            return self._obs_out(True), self.reward.clone(), self.done.clone(), info
        return self.obs, self.reward, self.done, info

    # ------------------------------------------------ info in gym 0.17/0.18's per-env form
    # "dict" (default): one dict of (N,) device tensors, the batched form (nothing leaves the GPU).
    # "list": gym.vector.VectorEnv.step_wait's form in gym 0.17/0.18 — a tuple of N dicts of Python
    # scalars, one per env (costs one device -> host copy of the five (N,) flags per step).
    info_format = "dict"
    INFO_FORMATS = ("dict", "list")

    def _info_list(self) -> tuple:
        keys = ("is_goal", "collision", "truncated", "t", "episode")  # info key "step" is the counter t
        cols = torch.stack([getattr(self, k).to(torch.int64) for k in keys]).cpu().tolist()
        return tuple({"is_goal": bool(g), "collision": bool(c), "truncated": bool(tr), "step": int(st),
                      "episode": int(ep)} for g, c, tr, st, ep in zip(*cols))

    # ------------------------------------------------ single-step graphs for step()
    # A closed-loop caller (each action computed from the previous observation, train.py:572-577)
    # cannot use capture()'s multi-step graphs.  use_graphs(True): every step() replays a HIP graph of
    # ONE step (its env kernel + raster, or the one-launch step), captured lazily for each frame-ring
    # position (graph_period() of them), reading the actions from a static device buffer
    # (`action_buffer`; step(env.action_buffer) skips the copy into it).  Bit-identical to the plain
    # launches (tests/test_gpu_closed_loop.py).
    _graphs = None

    def use_graphs(self, on: bool = True) -> None:
        """Run step() as single-step graph replays (on) or plain launches (off).  Not with pipeline
        slices or a BEV image ring (their steps need per-step host work)."""
        self._check_open()
        if not on:
            self._graphs = None
            return
        if self.pipeline_slices > 1 or self.bev is not None:
            raise ValueError("use_graphs() needs pipeline=1 and no bev_series")
        if self._graphs is None:
            self._graphs = {}
            if getattr(self, "action_buffer", None) is None:
                self.action_buffer = torch.zeros(self.num_envs, dtype=torch.int64, device=self.device)
            if getattr(self, "command_buffer", None) is None:
                self.command_buffer = torch.zeros((self.num_envs, 2), dtype=torch.float64, device=self.device)

    action_buffer = None
    command_buffer = None  # (N, 2) float64: the static (v, w) block of the command steps' graphs

    def _step_graph(self, actions) -> None:
        # ids and commands have a static buffer and graphs of their own: the cache is keyed by the kind
        if isinstance(actions, torch.Tensor) and actions.data_ptr() == self.command_buffer.data_ptr():
            buf, kind = self.command_buffer, "cmd"
        elif isinstance(actions, torch.Tensor) and actions.data_ptr() == self.action_buffer.data_ptr():
            buf, kind = self.action_buffer, "ids"
        else:
            a, is_cmd = self._act_in(actions)
            buf, kind = (self.command_buffer, "cmd") if is_cmd else (self.action_buffer, "ids")
            buf.copy_(a, non_blocking=True)
        key = (self._wpos, self.fused, kind)
        g = self._graphs.get(key)
        if g is None:
            g = torch.cuda.CUDAGraph()
            snap = (self._wpos, list(self._hist), self._hist_from_reset)
            stream = torch.cuda.Stream(device=self.device)
            stream.wait_stream(torch.cuda.current_stream(self.device))
            try:
                with torch.cuda.graph(g, stream=stream):
                    if self.fused:
                        self._step_fused(buf)
                    else:
                        self.step_state(buf)
                        self.raster_step()
            finally:
                # nothing ran: the host bookkeeping goes back to where the GPU state is
                self._set_window(snap[0])
                self._hist, self._hist_from_reset = snap[1], snap[2]
            self._graphs[key] = g
        g.replay()
        self._next_window()

    # ------------------------------------------------ closed-loop controller
    def policy_reactive(self, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The next actions (N,) int64 from the current observation, on the device
        (include/ffmp.h ffmp_policy_reactive: steer towards the goal, stop and turn when the newest
        frame is occupied just ahead) — a scripted controller for closed-loop runs (bench.py's
        closed_loop leg), not the reference's Q-network.  `out`: write into this (N,) int64 tensor
        (e.g. action_buffer) instead of a new one."""
        self._check_open()
        if self._needs_reset:
            raise RuntimeError("call reset() before policy_reactive()")
        if out is None:
            out = torch.empty(self.num_envs, dtype=torch.int64, device=self.device)
        elif out.shape != (self.num_envs,) or out.dtype != torch.int64 or not out.is_contiguous() \
                or out.device != self.device:
            raise ValueError(f"out must be a contiguous int64 tensor of shape ({self.num_envs},) on {self.device}")
        with torch.cuda.device(self.device):
            _abi.check(self.lib.ffmp_policy_reactive(C.byref(self._cfg_c), self.num_envs, C.byref(self._obs_c),
                                                     out.data_ptr(), self._stream()), "ffmp_policy_reactive")
        return out

    def policy_field(self, out: Optional[torch.Tensor] = None, grad: Optional[torch.Tensor] = None,
                     frames: Optional[torch.Tensor] = None, visible: bool = False, lidar: bool = False,
                     lidar_map: Optional["LidarMap"] = None, predict=False) -> torch.Tensor:
        """The next (v, w) commands (N, 2) float64 from the current observation, on the device
        (include/ffmp.h ffmp_policy_field): descend the potential field along its gradient at the
        robot cell (obs["grad"]) — full speed along the descent direction's heading component, turn
        towards it, turn on the spot when it points behind.  A scripted controller for closed-loop
        runs over commands, as policy_reactive is over action ids.  `out`: write into this (N, 2)
        float64 tensor (e.g. command_buffer) instead of a new one.
        grad: follow this contiguous (N, 2) float32 device tensor instead of obs["grad"] (e.g.
        frame_potential(...)["grad"]).  frames / visible / lidar / lidar_map / predict: follow the
        field of that plane — frame_potential's gradient with its defaults (one more launch, plus
        the plane's own), the follower a robot with nothing but its scan can run.  With none of
        them the call is what it always was."""
        self._check_open()
        if self._needs_reset:
            raise RuntimeError("call reset() before policy_field()")
        if not self.cfg.dt > 0:
            raise ValueError("policy_field: dt must be > 0 (the turn rate divides by it)")
        if out is None:
            out = torch.empty((self.num_envs, 2), dtype=torch.float64, device=self.device)
        elif tuple(out.shape) != (self.num_envs, 2) or out.dtype != torch.float64 or not out.is_contiguous() \
                or out.device != self.device or out.data_ptr() % 16:
            raise ValueError(f"out must be a contiguous, 16-byte aligned float64 tensor of shape "
                             f"({self.num_envs}, 2) on {self.device}")
        obs_c = self._obs_c
        sensed = frames is not None or visible or lidar or lidar_map is not None or (predict is not False and predict is not None)
        if grad is not None and sensed:
            raise ValueError("policy_field: pass grad or a plane (frames, visible, lidar, lidar_map, predict), not both")
        if sensed:
            grad = torch.empty((self.num_envs, 2), dtype=torch.float32, device=self.device)
            plane = self._plane_source("policy_field", frames, visible, lidar, lidar_map, predict)
            self._potential_launch(plane, None, 255, self._potential_reach("policy_field", None, True), grad=grad)
        elif grad is not None and (not isinstance(grad, torch.Tensor) or tuple(grad.shape) != (self.num_envs, 2)
                                   or grad.dtype != torch.float32 or not grad.is_contiguous() or grad.device != self.device):
            raise ValueError(f"grad must be a contiguous float32 tensor of shape ({self.num_envs}, 2) on {self.device}")
        if grad is not None:
            obs_c = _abi.ObsT()
            C.memmove(C.byref(obs_c), C.byref(self._obs_c), C.sizeof(obs_c))
            obs_c.grad, obs_c.reserved = grad.data_ptr(), 0  # a plain ffmp_obs_t: only grad is read
        with torch.cuda.device(self.device):
            _abi.check(self.lib.ffmp_policy_field(C.byref(self._cfg_c), self.num_envs, C.byref(obs_c),
                                                  out.data_ptr(), self._stream()), "ffmp_policy_field")
        return out

    # ------------------------------------------------ navigation field
    NAV_DEFAULTS = dict(margin=2, soft_pen=40, lookahead=4, turn_sin=0.25)

    nav_tile: Optional[int] = None  # set (0 = the library's default tile) to plan through the tiled kernel on any grid
    _nav_ws = None                  # (tile, with_cost) -> the tiled kernel's workspace, a device tensor

    def _nav_tiled(self, tile: Optional[int]) -> Optional[int]:
        """The tile of the tiled kernel (ffmp_nav_field_tiled; 0 = its default), or None for the
        kernel that holds the whole plane in LDS: tiled when `tile` or the attribute nav_tile is
        given, or when the grid is larger than 256 x 256."""
        if tile is None:
            tile = self.nav_tile
        if tile is None:
            return 0 if self.cfg.grid > 256 else None
        return int(tile)

    def _nav_workspace(self, tile: int, with_cost: bool) -> torch.Tensor:
        """The workspace of the tiled kernel for this env count, allocated on first use and kept
        until close(), per (tile, with_cost)."""
        if self._nav_ws is None:
            self._nav_ws = {}
        key = (tile, bool(with_cost))
        ws = self._nav_ws.get(key)
        if ws is None:
            nbytes = C.c_size_t()
            with torch.cuda.device(self.device):
                _abi.check(self.lib.ffmp_nav_field_tiled_workspace(C.byref(self._cfg_c), self.num_envs, tile, int(with_cost),
                                                                   C.byref(nbytes)), "ffmp_nav_field_tiled_workspace")
            buf = torch.empty(nbytes.value + 256, dtype=torch.uint8, device=self.device)
            off = (-buf.data_ptr()) % 256
            ws = self._nav_ws[key] = buf[off:off + nbytes.value]
        return ws

    def nav_workspace_bytes(self) -> int:
        """Device bytes held by the tiled navigation kernel's workspaces (0 before the first tiled
        call; freed by close())."""
        return sum(int(ws.numel()) for ws in (self._nav_ws or {}).values())

    def _nav_plane_obs(self, frames: torch.Tensor) -> "_abi.ObsT":
        """A copy of the launch struct whose newest frame is the caller's (N, G, G) plane: state_m
        is the (never read) address one plane before it, the frame stride one plane."""
        n, G = self.num_envs, self.cfg.grid
        fmts = {torch.float32: _abi.OBS_F32, torch.uint8: _abi.OBS_U8F16}
        if not isinstance(frames, torch.Tensor) or tuple(frames.shape) != (n, G, G) or frames.dtype not in fmts \
                or not frames.is_contiguous() or frames.device != self.device:
            raise ValueError(f"frames must be a contiguous float32 or uint8 tensor of shape ({n}, {G}, {G}) on {self.device}")
        ob = _abi.ObsT()
        C.memmove(C.byref(ob), C.byref(self._obs_c), C.sizeof(ob))
        ob.state_m = frames.data_ptr() - G * G * frames.element_size()
        ob.state_m_stride, ob.state_m_frame_stride = G * G, G * G
        ob.format, ob.reserved = fmts[frames.dtype], 0
        return ob

    def _plane_source(self, what: str, frames, visible: bool, lidar: bool, lidar_map, predict) -> Optional[torch.Tensor]:
        """The plane a caller of nav_field's conventions asks for — frames=, visible=True, lidar=True,
        lidar_map= or predict=, at most one — or None for the newest frame of the window."""
        if predict is not False and predict is not None:
            if frames is not None or visible or lidar or lidar_map is not None:
                raise ValueError(f"{what}: pass one of frames, visible=True, lidar=True, lidar_map and predict")
            if predict is True:
                kw = {}
            elif isinstance(predict, dict):
                kw = dict(predict)
                if kw.get("count") or kw.get("out") is not None:
                    raise ValueError(f"{what}: predict takes predicted_frames' knobs, not out= or count=")
            elif isinstance(predict, LidarFlow):
                kw = {"flow": predict}
            else:
                raise ValueError(f"{what}: predict must be False, True, a dict of predicted_frames' keyword arguments "
                                 f"or a LidarFlow of this env")
            frames = self.predicted_frames(**kw)
        if visible:
            if frames is not None:
                raise ValueError(f"{what}: pass frames or visible=True, not both")
            frames = self.visible_frames(unknown=0, newest_only=True)
        if lidar:
            if frames is not None:
                raise ValueError(f"{what}: pass one of frames, visible=True and lidar=True")
            frames = self.lidar_frames(unknown=0, newest_only=True)
        if lidar_map is not None:
            if frames is not None:
                raise ValueError(f"{what}: pass one of frames, visible=True, lidar=True and lidar_map")
            if not isinstance(lidar_map, LidarMap) or lidar_map.env is not self or lidar_map.frame is None:
                raise ValueError(f"{what}: lidar_map must be a LidarMap of this env that keeps a frame")
            frames = lidar_map.frame
        return frames

    def _nav_launch(self, what: str, margin: int, soft_pen: int, lookahead: int, turn_sin: float,
                    cost=None, direction=None, target=None, geo_cost=None, cmd=None, tile: Optional[int] = None,
                    frames: Optional[torch.Tensor] = None, visible: bool = False, lidar: bool = False,
                    lidar_map: Optional["LidarMap"] = None, predict=False) -> None:
        """One ffmp_nav_field (or, see _nav_tiled, ffmp_nav_field_tiled) launch over the current
        observation: the newest frame through the window's strides and format, the ego goal from
        record words 8..9.  frames: plan over this (N, G, G) plane instead of the newest frame;
        visible: over visible_frames(newest_only=True, unknown=0); lidar: over
        lidar_frames(newest_only=True, unknown=0); lidar_map: over that LidarMap's frame; predict:
        over predicted_frames() (True), predicted_frames(**predict) (a dict) or
        predicted_frames(flow=predict) (a LidarFlow)."""
        self._check_open()
        if self._needs_reset:
            raise RuntimeError(f"call reset() before {what}()")
        frames = self._plane_source(what, frames, visible, lidar, lidar_map, predict)
        obs_c, fmt = self._obs_c, self._fmt
        if frames is not None:
            obs_c = self._nav_plane_obs(frames)
            fmt = obs_c.format
        knobs = (int(margin), int(soft_pen), int(lookahead))
        tile = self._nav_tiled(tile)
        if tile is not None:
            _abi.check(self.lib.ffmp_nav_field_tiled_check(C.byref(self._cfg_c), fmt, *knobs, tile),
                       "ffmp_nav_field_tiled_check")
            ws = self._nav_workspace(tile, cost is not None)
            with torch.cuda.device(self.device):
                _abi.check(self.lib.ffmp_nav_field_tiled(C.byref(self._cfg_c), self.num_envs, C.byref(obs_c),
                                                         self.record.data_ptr() + 8 * 4, self.record.stride(0), *knobs,
                                                         float(turn_sin), _ptr(cost), _ptr(direction), _ptr(target),
                                                         _ptr(geo_cost), _ptr(cmd), tile, ws.data_ptr(), ws.numel(),
                                                         self._stream()), "ffmp_nav_field_tiled")
            return
        _abi.check(self.lib.ffmp_nav_field_check(C.byref(self._cfg_c), fmt, *knobs), "ffmp_nav_field_check")
        with torch.cuda.device(self.device):
            _abi.check(self.lib.ffmp_nav_field(C.byref(self._cfg_c), self.num_envs, C.byref(obs_c),
                                               self.record.data_ptr() + 8 * 4, self.record.stride(0), *knobs,
                                               float(turn_sin), _ptr(cost), _ptr(direction), _ptr(target),
                                               _ptr(geo_cost), _ptr(cmd), self._stream()), "ffmp_nav_field")

    # ------------------------------------------------ sensor-visible frames
    def _visible_launch(self, record: torch.Tensor, older: Optional[int], newest: Optional[int], env_stride: int,
                        fmt: int, unknown: int, max_range: Optional[float], mask=None, flags: int = 0) -> None:
        """One ffmp_visible_frames launch over `record` (n, R) on the current stream; older / newest
        are device addresses (None: that frame is not computed)."""
        mr = float("inf") if max_range is None else float(max_range)
        _abi.check(self.lib.ffmp_visible_frames_check(C.byref(self._cfg_c), fmt, int(unknown), mr, int(flags)),
                   "ffmp_visible_frames_check")
        with torch.cuda.device(self.device):
            _abi.check(self.lib.ffmp_visible_frames(C.byref(self._cfg_c), record.shape[0], record.data_ptr(),
                                                    record.stride(0), _ptr(mask), older, newest, int(env_stride), fmt,
                                                    int(unknown), mr, int(flags), self._stream()), "ffmp_visible_frames")

    def visible_frames(self, out: Optional[torch.Tensor] = None, unknown: int = 128, max_range: Optional[float] = None,
                       newest_only: bool = False, mask: Optional[torch.Tensor] = None, nocull: bool = False) -> torch.Tensor:
        """What a sensor at the robot can see of the frame pair, on the device (include/ffmp.h
        ffmp_visible_frames): state_m with every cell an obstacle disc hides from the ego origin — and
        every cell farther than `max_range` metres, when given — set to `unknown` (a byte; 0 is the
        image of a hit-based estimator, where hidden things are simply absent).  (N, 2, G, G)
        [older, newest], or (N, G, G) with newest_only, in the env's frame dtype (float32, or uint8
        with obs_format="u8f16").  Computed from `record` on the current stream by one launch, so a
        caller can capture it into a graph of their own; the step and its frames are untouched.
        out: write into this contiguous tensor instead of a new one; mask: (N,) bool or uint8, envs
        with 0 keep their cells of `out`; nocull: the kernel without its culls (the same bits)."""
        self._check_open()
        if self._needs_reset:
            raise RuntimeError("call reset() before visible_frames()")
        n, G = self.num_envs, self.cfg.grid
        shape = (n, G, G) if newest_only else (n, 2, G, G)
        if out is None:
            out = torch.empty(shape, dtype=self._frame_dtype, device=self.device)
        elif tuple(out.shape) != shape or out.dtype != self._frame_dtype or not out.is_contiguous() \
                or out.device != self.device:
            raise ValueError(f"out must be a contiguous {self._frame_dtype} tensor of shape {shape} on {self.device}")
        if mask is not None:
            mask = torch.as_tensor(mask, device=self.device).reshape(n).to(torch.uint8).contiguous()
        G2 = G * G
        if newest_only:
            older, newest, stride = None, out.data_ptr(), G2
        else:
            older, newest, stride = out.data_ptr(), out.data_ptr() + G2 * self._fes, 2 * G2
        self._visible_launch(self.record, older, newest, stride, self._fmt, unknown, max_range, mask,
                             _abi.VISIBLE_NOCULL if nocull else 0)
        return out

    # ------------------------------------------------ frames built from the lidar scan
    _sector_cache = None  # L -> (L, 2) float32 device tensor (config.sector_table)

    def _sectors(self, L: int) -> torch.Tensor:
        if self._sector_cache is None:
            self._sector_cache = {}
        if L not in self._sector_cache:
            self._sector_cache[L] = torch.as_tensor(sector_table(L)).to(self.device).contiguous()
        return self._sector_cache[L]

    def _scan_launch(self, ranges: torch.Tensor, older: Optional[int], newest: Optional[int], env_stride: int, fmt: int,
                     unknown: int, thickness: float, range_max: float, mask=None, first=None, flags: int = 0) -> None:
        """One ffmp_scan_frames launch over `ranges` (n, L) float32 on the current stream; older / newest
        are device addresses (None: that frame is not written)."""
        L = int(ranges.shape[1])
        knobs = (fmt, int(unknown), float(thickness), float(range_max), int(flags))
        _abi.check(self.lib.ffmp_scan_frames_check(C.byref(self._cfg_c), L, *knobs), "ffmp_scan_frames_check")
        sectors = self._sectors(L)
        with torch.cuda.device(self.device):
            _abi.check(self.lib.ffmp_scan_frames(C.byref(self._cfg_c), ranges.shape[0], ranges.data_ptr(), ranges.stride(0), L,
                                                 sectors.data_ptr(), _ptr(mask), _ptr(first), older, newest, int(env_stride),
                                                 *knobs, self._stream()), "ffmp_scan_frames")

    def lidar_frames(self, out: Optional[torch.Tensor] = None, unknown: int = 128, thickness: Optional[float] = None,
                     range_max: Optional[float] = None, newest_only: bool = False, shift: bool = True,
                     ranges: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None,
                     plain: bool = False) -> torch.Tensor:
        """The occupancy frames a robot can build from its own scan, on the device (include/ffmp.h
        ffmp_scan_frames): per cell, the range of the beam whose cone holds the cell decides between
        free (0, nearer than the hit), occupied (255, within `thickness` metres of the hit; default
        res) and `unknown` (a byte: behind the hit, beyond `range_max` metres — default
        cfg.lidar_range — or in a cone without data).  (N, 2, G, G) [older, newest], or (N, G, G)
        with newest_only, in the env's frame dtype.  One launch on the current stream (the in-place
        shift adds the comparison that makes its `first` bytes); the step, its frames and its lidar
        are untouched.
        ranges: a contiguous (N, L') float32 device tensor in the lidar's convention (+inf no return,
        -inf / NaN / <= 0 no data) instead of the env's own `lidar`; L' need not be cfg.n_beams.
        out=None allocates, and both frames are the current scan.  out: write into this contiguous
        tensor instead.  With out given and shift=True the pair is advanced in place as
        make_temporal_maps does: older takes what newest held, newest the current scan; an env on
        the first observation of an episode (record word 10 != 0: it has just reset) gets two equal
        frames, as state_m does.  shift=False writes the current scan into both frames.
        mask: (N,) bool or uint8, envs with 0 keep all their cells of `out`; plain: the kernel
        without its search shortcut (the same bits).
        Inside a graph capture of the caller's: call it once eagerly first — the sector table of a
        beam count is built on the host and copied to the device at the first call for that count,
        a host-to-device copy that has no place in a capture; afterwards the call is one launch (two
        with the shift)."""
        self._check_open()
        if self._needs_reset:
            raise RuntimeError("call reset() before lidar_frames()")
        n, G = self.num_envs, self.cfg.grid
        if ranges is None:
            if self.lidar is None:
                raise ValueError("lidar_frames: the env has n_beams == 0, pass ranges=")
            ranges = self.lidar
        elif not isinstance(ranges, torch.Tensor) or ranges.dim() != 2 or ranges.shape[0] != n or ranges.dtype != torch.float32 \
                or not ranges.is_contiguous() or ranges.device != self.device:
            raise ValueError(f"ranges must be a contiguous float32 tensor of shape ({n}, L) on {self.device}")
        shape = (n, G, G) if newest_only else (n, 2, G, G)
        first = None
        if out is None:
            out = torch.empty(shape, dtype=self._frame_dtype, device=self.device)
        elif tuple(out.shape) != shape or out.dtype != self._frame_dtype or not out.is_contiguous() \
                or out.device != self.device:
            raise ValueError(f"out must be a contiguous {self._frame_dtype} tensor of shape {shape} on {self.device}")
        elif shift and not newest_only:
            first = self.record[:, 10] != 0  # bool: one byte per env, 0 or 1
        if mask is not None:
            mask = torch.as_tensor(mask, device=self.device).reshape(n).to(torch.uint8).contiguous()
        G2 = G * G
        if newest_only:
            older, newest, stride = None, out.data_ptr(), G2
        else:
            older, newest, stride = out.data_ptr(), out.data_ptr() + G2 * self._fes, 2 * G2
        self._scan_launch(ranges, older, newest, stride, self._fmt, unknown,
                          self.cfg.res if thickness is None else thickness,
                          self.cfg.lidar_range if range_max is None else range_max, mask, first,
                          _abi.SCAN_PLAIN if plain else 0)
        return out

    # ------------------------------------------------ the accumulated scan map
    def lidar_map(self, unknown: int = 128, thickness: Optional[float] = None, range_max: Optional[float] = None,
                  l_hit: int = 8, l_free: int = 4, l_max: int = 64, decay: int = 0, occ_thr: int = 8, free_thr: int = 4,
                  frame: bool = True) -> "LidarMap":
        """A map of the scan that remembers (include/ffmp.h ffmp_scan_map): an int8 log-odds plane per
        env, ego-centric, moved along with the robot and updated from the scan by every
        LidarMap.update() — a hit adds `l_hit`, a free cell subtracts `l_free`, saturating at
        +-`l_max`; a cell the scan says nothing about keeps its value, less `decay` toward 0.  The
        frame holds 255 where the log-odds are >= `occ_thr`, 0 where <= -`free_thr`, else `unknown`.
        thickness, range_max: as for lidar_frames.  frame=False keeps no frame.  Known limits: a
        moving obstacle leaves a trail of stale hits until the beam sweeps it free again or `decay`
        fades it, and the nearest-neighbour re-sampling jitters edges by up to a cell."""
        self._check_open()
        return LidarMap(self, unknown, self.cfg.res if thickness is None else thickness,
                        self.cfg.lidar_range if range_max is None else range_max, l_hit, l_free, l_max, decay, occ_thr,
                        free_thr, frame)

    # ------------------------------------------------ the world-fixed scan map
    def world_map(self, cells: Optional[int] = None, unknown: int = 128, outside: int = 255, thickness: Optional[float] = None,
                  range_max: Optional[float] = None, l_hit: int = 8, l_free: int = 4, l_max: int = 64, decay: int = 0,
                  occ_thr: int = 8, free_thr: int = 4) -> "WorldMap":
        """The /map of occupancy-grid mapping (include/ffmp.h ffmp_world_map / ffmp_world_frame): an int8
        log-odds plane per env with one cell per WORLD cell, `cells` x `cells` of them centred on the world's
        origin, integrated in place from the scan and the pose by every WorldMap.update() and never re-sampled
        — edges do not jitter, and what leaves the ego window is remembered.  WorldMap.ego_frame() cuts the
        window around the robot out and rotates it into the ego frame: 255 where the log-odds are >=
        `occ_thr`, 0 where <= -`free_thr`, `unknown` elsewhere and `outside` beyond the plane — a plane for
        nav_field / policy_nav / policy_dwa / frame_potential through frames=.  cells: a multiple of 4 in
        [8, 2048]; by default the arena [-world_half, world_half] plus four cells a side.  thickness,
        range_max, l_hit, l_free, l_max, decay: as for lidar_map, but a cell the scan does not reach
        (beyond range_max, or in a cone without data) keeps its value with no decay.  Memory: cells^2
        bytes per env.  Known limit: a moving obstacle leaves a trail of stale hits until the beam
        sweeps it free again."""
        self._check_open()
        if cells is None:
            cells = 4 * int(math.ceil((2.0 * self.cfg.W / self.cfg.res + 8.0) / 4.0))
        cells = int(cells)
        if cells > 2048:
            raise ValueError(f"world_map: cells = {cells} is above 2048 ({self.num_envs} envs x {cells}^2 bytes = "
                             f"{self.num_envs * cells * cells / 1e9:.2f} GB of log-odds); use a coarser res or a smaller world_half")
        holder = WorldMap(self, cells, unknown, outside, self.cfg.res if thickness is None else thickness,
                          self.cfg.lidar_range if range_max is None else range_max, l_hit, l_free, l_max, decay, occ_thr,
                          free_thr)
        if self._world_maps is None:
            self._world_maps = []
        self._world_maps.append(weakref.ref(holder))
        return holder

    # ------------------------------------------------ motion flow estimated from the scan
    def lidar_flow(self, lag: int = 4, radius: int = 4, block: int = 3, gate: int = 1, min_hits: int = 3,
                   thickness: Optional[float] = None, range_max: Optional[float] = None, kind: bool = True) -> "LidarFlow":
        """The motion flow a robot can estimate from its own scan (include/ffmp.h ffmp_scan_flow): the
        sensor-side counterpart of obs["flow"].  Every LidarFlow.update() builds the scan frame, moves
        the frame of `lag` updates ago into the current ego frame and matches the
        (2*block+1) x (2*block+1) block of hits around every hit cell against it, over displacements
        of up to `radius` cells: (N, 2, G, G) [vx, vy] in the env's flow dtype, world velocity in the
        current ego axes in m/s, a multiple of res / (lag * dt).  A block within `gate` unmatched
        cells of the warped earlier frame is static (flow 0); one with fewer than `min_hits` hits is
        not estimated.  thickness, range_max: as for lidar_frames.  kind=False keeps no kind plane
        (0 no estimate, 1 static, 2 moving).  Known limits: integer displacements of a
        two-cell-thick arc — one quantum is res / (lag * dt); a straight wall shows no motion along
        itself (the aperture problem; the gate hides most of it); a disc that reflects off a wall
        inside the lag gets the net displacement; an env in its first `lag` updates has no flow."""
        self._check_open()
        return LidarFlow(self, lag, radius, block, gate, min_hits, self.cfg.res if thickness is None else thickness,
                         self.cfg.lidar_range if range_max is None else range_max, kind)

    # ------------------------------------------------ predicted-occupancy frames
    def predicted_frames(self, flow=None, frames: Optional[torch.Tensor] = None, steps: int = 24, slack: int = 3,
                         dt: Optional[float] = None, speed: float = 0.6, swept: int = 254, other: int = 128,
                         out: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None, count: bool = False):
        """The newest frame with the cells a moving obstacle is predicted to cover when the robot can be
        there marked occupied, on the device (include/ffmp.h ffmp_flow_predict): (N, G, G) uint8 — 255
        where the frame is 255, `other` where it holds another value > 0, `swept` where a predicted cell
        is free now, else 0 — the plane nav_field(predict=...) plans over.  Every 255 cell with a
        velocity is moved along it for k = 1..`steps` prediction steps of `dt` seconds (default
        cfg.dt) and blocks its target cell if the robot, covering `speed` m/s, could reach that cell
        within `slack` steps of step k (its chamfer distance from the robot cell at
        pace = max(1, rint(5 * speed * dt / res)) units per step); slack=-1 blocks the whole swept
        corridor.  Present occupancy always stays.
        flow: None — the env's own obs["flow"] over the newest frame (the env must have been made
        with flow=True); a contiguous (N, 2, G, G) float32 or float16 device tensor [vx, vy] in m/s
        in the current ego axes; or a LidarFlow of this env — its .flow over its .frame.  frames: a
        contiguous (N, G, G) float32 or uint8 device tensor instead of that frame.  out: write into
        this contiguous (N, G, G) uint8 tensor; mask: (N,) bool or uint8, envs with 0 keep their
        cells of `out`; count=True: also return n_swept (N,) int32, the free cells newly blocked.
        One launch on the current stream, so a caller can capture it into a graph of their own; the
        step and its frames are untouched.  Known limits: constant velocities (no wall reflection, no
        reaction to the robot); a thin arc faster than about two cells per step leaves one-cell gaps
        that nav_field's footprint dilation closes; the arrival time is a straight-line bound."""
        self._check_open()
        if self._needs_reset:
            raise RuntimeError("call reset() before predicted_frames()")
        n, G = self.num_envs, self.cfg.grid
        G2 = G * G
        plane = None
        if isinstance(flow, LidarFlow):
            if flow.env is not self:
                raise ValueError("predicted_frames: flow must be a LidarFlow of this env")
            plane, flow = flow.frame, flow.flow
        elif flow is None:
            if self.flow is None:
                raise ValueError("predicted_frames: the env was made without flow=True, pass flow=")
            flow = self.flow
        elif not isinstance(flow, torch.Tensor) or tuple(flow.shape) != (n, 2, G, G) \
                or flow.dtype not in (torch.float32, torch.float16) or not flow.is_contiguous() or flow.device != self.device:
            raise ValueError(f"flow must be a contiguous float32 or float16 tensor of shape ({n}, 2, {G}, {G}) on {self.device}, "
                             f"or a LidarFlow of this env")
        fmts = {torch.float32: _abi.OBS_F32, torch.uint8: _abi.OBS_U8F16}
        if frames is not None:
            if not isinstance(frames, torch.Tensor) or tuple(frames.shape) != (n, G, G) or frames.dtype not in fmts \
                    or not frames.is_contiguous() or frames.device != self.device:
                raise ValueError(f"frames must be a contiguous float32 or uint8 tensor of shape ({n}, {G}, {G}) on {self.device}")
            plane = frames
        elif plane is None:
            plane = self.state_m[:, 1]  # a view: the env stride of the window
        if dt is None:
            dt = self.cfg.dt
        dt, res, speed = float(dt), float(self.cfg.res), float(speed)
        if not (math.isfinite(dt) and dt > 0):
            raise ValueError(f"predicted_frames: dt must be finite and > 0, got {dt}")
        with np.errstate(over="ignore"):
            cps = float(np.float32(dt / res))
        if not (math.isfinite(cps) and cps > 0):
            raise ValueError(f"predicted_frames: dt / res = {dt} / {res} is not a finite positive float32 (res)")
        if not (math.isfinite(speed) and speed >= 0):
            raise ValueError(f"predicted_frames: speed must be finite and >= 0, got {speed}")
        pace = 5.0 * speed * dt / res
        if not pace <= 1024:
            raise ValueError(f"predicted_frames: speed * dt / res gives a pace of {pace:.6g} chamfer units per step, above 1024 (speed)")
        pace = max(1, int(np.rint(pace)))
        knobs = (int(steps), cps, pace, int(slack), int(swept), int(other))
        ffmt, vfmt = fmts[plane.dtype], _abi.OBS_F32 if flow.dtype == torch.float32 else _abi.OBS_U8F16
        _abi.check(self.lib.ffmp_flow_predict_check(C.byref(self._cfg_c), ffmt, vfmt, *knobs), "ffmp_flow_predict_check")
        if out is None:
            out = torch.empty((n, G, G), dtype=torch.uint8, device=self.device)
        elif not isinstance(out, torch.Tensor) or tuple(out.shape) != (n, G, G) or out.dtype != torch.uint8 \
                or not out.is_contiguous() or out.device != self.device:
            raise ValueError(f"out must be a contiguous uint8 tensor of shape ({n}, {G}, {G}) on {self.device}")
        if mask is not None:
            mask = torch.as_tensor(mask, device=self.device).reshape(n).to(torch.uint8).contiguous()
        n_swept = torch.zeros(n, dtype=torch.int32, device=self.device) if count else None
        with torch.cuda.device(self.device):
            _abi.check(self.lib.ffmp_flow_predict(C.byref(self._cfg_c), n, plane.data_ptr(), plane.stride(0), ffmt,
                                                  flow.data_ptr(), flow.stride(0), vfmt, _ptr(mask), out.data_ptr(), G2,
                                                  _ptr(n_swept), *knobs, self._stream()), "ffmp_flow_predict")
        return (out, n_swept) if count else out

    # ------------------------------------------------ potential field of a frame
    def _potential_reach(self, what: str, reach: Optional[int], exact: bool) -> int:
        """The window of ffmp_frame_potential in cells: ceil(rho0 / res) by default; a given reach
        that cuts the repulsive term short of rho0 is refused when the field has to be exact."""
        need = int(math.ceil(self.cfg.rho0 / self.cfg.res))
        if reach is None:
            if need > 32:
                raise ValueError(f"{what}: rho0 / res = {self.cfg.rho0} / {self.cfg.res} needs a reach of {need} cells, "
                                 f"above 32 (lower rho0 or raise res)")
            return need
        reach = int(reach)
        if exact and reach < need:
            raise ValueError(f"{what}: reach = {reach} cells covers {reach * self.cfg.res:.6g} m, short of rho0 = {self.cfg.rho0} "
                             f"at res = {self.cfg.res} ({need} cells): the potential would be cut off inside rho0 "
                             f"(potential=False gives the clearance alone at any reach)")
        return reach

    def _potential_launch(self, plane: Optional[torch.Tensor], goal: Optional[torch.Tensor], occ_min: int, reach: int,
                          dist2=None, potential=None, grad=None, robot_d2=None, mask=None) -> None:
        """One ffmp_frame_potential launch on the current stream.  plane: an (N, G, G) float32 or
        uint8 device tensor whose env planes are dense (None: the newest frame, a view of the
        window); goal: a contiguous (N, 2) float32 device tensor (None: record words 8..9)."""
        n, G = self.num_envs, self.cfg.grid
        fmts = {torch.float32: _abi.OBS_F32, torch.uint8: _abi.OBS_U8F16}
        if plane is None:
            plane = self.state_m[:, 1]  # a view: the env stride of the window
        elif not isinstance(plane, torch.Tensor) or tuple(plane.shape) != (n, G, G) or plane.dtype not in fmts \
                or not plane.is_contiguous() or plane.device != self.device:
            raise ValueError(f"frames must be a contiguous float32 or uint8 tensor of shape ({n}, {G}, {G}) on {self.device}")
        if goal is None:
            goal_ptr, goal_stride = self.record.data_ptr() + 8 * 4, self.record.stride(0)
        elif not isinstance(goal, torch.Tensor) or tuple(goal.shape) != (n, 2) or goal.dtype != torch.float32 \
                or not goal.is_contiguous() or goal.device != self.device:
            raise ValueError(f"goal must be a contiguous float32 tensor of shape ({n}, 2) on {self.device}")
        else:
            goal_ptr, goal_stride = goal.data_ptr(), 2
        pfmt = _abi.OBS_U8F16 if potential is not None and potential.dtype == torch.float16 else _abi.OBS_F32
        _abi.check(self.lib.ffmp_frame_potential_check(C.byref(self._cfg_c), fmts[plane.dtype], pfmt, int(occ_min), reach),
                   "ffmp_frame_potential_check")
        with torch.cuda.device(self.device):
            _abi.check(self.lib.ffmp_frame_potential(C.byref(self._cfg_c), n, plane.data_ptr(), plane.stride(0), fmts[plane.dtype],
                                                     goal_ptr, goal_stride, _ptr(mask), int(occ_min), reach, _ptr(dist2), G * G,
                                                     _ptr(potential), G * G, pfmt, _ptr(grad), _ptr(robot_d2), self._stream()),
                       "ffmp_frame_potential")

    def frame_potential(self, frames: Optional[torch.Tensor] = None, visible: bool = False, lidar: bool = False,
                        lidar_map: Optional["LidarMap"] = None, predict=False, goal: Optional[torch.Tensor] = None,
                        occ_min: int = 255, reach: Optional[int] = None, distance: bool = False, potential: bool = True,
                        dtype: torch.dtype = torch.float32, out: Optional[Dict[str, torch.Tensor]] = None,
                        mask: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        """The potential field of an occupancy frame, on the device (include/ffmp.h
        ffmp_frame_potential): what obs["potential"] and obs["grad"] are to the simulator's disc
        list, for any plane a sensor can give.  Every cell >= `occ_min` is an obstacle (255: hits
        only, unknown cells do not repel; 1: nav_field's occupancy; a predicted plane marks its
        swept cells 254).  Returns
          grad      (N, 2) float32: the central difference of the potential at the robot cell, the
                    layout policy_field(grad=...) reads
          robot_d2  (N,) int32: the squared distance in cells from the robot cell to the nearest
                    obstacle cell within `reach` cells along either axis, -1 when there is none
          clearance (N,) float64 metres = sqrt(robot_d2) * res, inf where -1
          potential (N, G, G) `dtype` (float32 or float16) with potential=True: the attractive term of
                    the raster plus Khatib's repulsive term of the NEAREST obstacle cell — not the sum
                    over discs of obs["potential"]; walls and anything else in the frame repel
          dist2     (N, G, G) uint16 with distance=True: the squared clearance of every cell in cells,
                    65535 where no obstacle lies within the window
        The plane: the newest frame state_m[:, 1], or one of frames= (a contiguous (N, G, G) float32
        or uint8 device tensor), visible=True, lidar=True, lidar_map=, predict= as for nav_field.
        goal: a contiguous (N, 2) float32 device tensor of ego goals instead of the env's own.
        reach: the window in cells, 1..32; None is ceil(rho0 / res), the smallest at which the field
        is exact out to rho0 — a smaller one is refused unless potential=False (the clearance alone
        may use any reach, and `grad` is then of the cut-off field).  out: a dict of tensors to
        write into, any of "grad", "robot_d2", "potential", "dist2" (contiguous, of the shapes and
        dtypes above; a plane given there is computed); mask: (N,) bool or uint8, envs with 0 keep
        every word.  One launch on the current stream, so a caller can capture it into a graph of
        their own (visible=, lidar= and predict= add theirs); with `out` supplying the planes it
        allocates only the (N,) clearance.  The step and its observation are untouched."""
        self._check_open()
        if self._needs_reset:
            raise RuntimeError("call reset() before frame_potential()")
        n, G = self.num_envs, self.cfg.grid
        if dtype not in (torch.float32, torch.float16):
            raise ValueError(f"frame_potential: dtype must be torch.float32 or torch.float16, got {dtype}")
        out = dict(out) if out else {}
        unknown = set(out) - {"grad", "robot_d2", "potential", "dist2"}
        if unknown:
            raise ValueError(f"frame_potential: out has no plane named {sorted(unknown)}")
        potential = bool(potential) or "potential" in out
        distance = bool(distance) or "dist2" in out
        reach = self._potential_reach("frame_potential", reach, exact=potential)
        spec = {"grad": ((n, 2), torch.float32), "robot_d2": ((n,), torch.int32)}
        if potential:
            spec["potential"] = ((n, G, G), dtype)
        if distance:
            spec["dist2"] = ((n, G, G), torch.uint16)
        res = {}
        for key, (shape, dt) in spec.items():
            t = out.get(key)
            if t is None:
                t = torch.empty(shape, dtype=dt, device=self.device)
            elif not isinstance(t, torch.Tensor) or tuple(t.shape) != shape or t.dtype != dt or not t.is_contiguous() \
                    or t.device != self.device:
                raise ValueError(f"out[{key!r}] must be a contiguous {dt} tensor of shape {shape} on {self.device}")
            res[key] = t
        if mask is not None:
            mask = torch.as_tensor(mask, device=self.device).reshape(n).to(torch.uint8).contiguous()
        plane = self._plane_source("frame_potential", frames, visible, lidar, lidar_map, predict)
        self._potential_launch(plane, goal, occ_min, reach, dist2=res.get("dist2"),
                               potential=res.get("potential"), grad=res["grad"], robot_d2=res["robot_d2"], mask=mask)
        rd = res["robot_d2"].to(torch.float64)
        res["clearance"] = torch.where(rd < 0, torch.full_like(rd, float("inf")), torch.sqrt(rd.clamp(min=0)) * self.cfg.res)
        return res

    def nav_field(self, cost: bool = False, direction: bool = False, margin: int = 2, soft_pen: int = 40,
                  lookahead: int = 4, tile: Optional[int] = None, frames: Optional[torch.Tensor] = None,
                  visible: bool = False, lidar: bool = False, lidar_map: Optional["LidarMap"] = None,
                  predict=False) -> Dict[str, torch.Tensor]:
        """The navigation field of the current observation, on the device (include/ffmp.h
        ffmp_nav_field): the cost-to-go from the goal cell over the traversable cells of the newest
        ego frame (hard = the footprint-dilated occupancy; a `margin`-cell zone around it costs
        `soft_pen` extra per cell) and the direction per cell.  Returns
          target   (N, 2) int32: the cell `lookahead` moves down the path, as offsets from the robot cell
          geo_cost (N,) int32: the cost at the robot cell, -1 when the goal is unreachable
          geo_dist (N,) float64 metres = geo_cost * res / 5, inf when unreachable — the chamfer 5-7
                   approximation of the geodesic length (it overestimates a straight line by up to
                   ~8 %), with the zone's penalties included
          cost (N, G, G) uint16 (65535: hard or unreachable) with cost=True
          dir  (N, G, G) uint8 (neighbour index 0..7, 8 at the goal, 255 unreachable) with direction=True
        A static plan over the plane it is given: obstacle velocities are looked at only with
        predict= (below).  Grids up to 512 x 512: up to
        256 x 256 one workgroup holds an env's whole plane in LDS; above that, or when `tile` (or the
        attribute nav_tile) is given, the plane lives in a workspace on the device and is relaxed in
        tiles of `tile` x `tile` cells (0 = the library's default, 256; else a multiple of 32 in
        [32, 256]) — the same bits either way (include/ffmp.h ffmp_nav_field_tiled).  The workspace
        is allocated on the first such call and kept until close() (nav_workspace_bytes()).
        frames: plan over this contiguous (N, G, G) float32 or uint8 device tensor instead of the
        newest frame; visible=True: over visible_frames(newest_only=True, unknown=0), what the robot
        can see with hidden cells taken as free (the usual free-space assumption); lidar=True: over
        lidar_frames(newest_only=True, unknown=0), the map made from the scan alone, what a real
        robot has; lidar_map=m: over m.frame, the accumulated map of a LidarMap of this env (make it
        with unknown=0 to count unknown cells as free; the caller updates it); predict: over
        predicted_frames(), the newest frame with the cells a moving obstacle is predicted to cover
        when the robot can be there marked occupied — True for its defaults, a dict of its keyword
        arguments, or a LidarFlow of this env for that holder's frame and estimated flow (grids up to
        512 x 512; one more launch).  At most one of the five.
        Inside a graph capture of the caller's: call it once eagerly first, with the same tile and
        cost= (the tiled kernel's workspace is allocated and its kernel set up at the first such
        call; lidar=True also builds lidar_frames' sector table then)."""
        n, G = self.num_envs, self.cfg.grid
        out = {"target": torch.empty((n, 2), dtype=torch.int32, device=self.device),
               "geo_cost": torch.empty(n, dtype=torch.int32, device=self.device)}
        if cost:
            out["cost"] = torch.empty((n, G, G), dtype=torch.uint16, device=self.device)
        if direction:
            out["dir"] = torch.empty((n, G, G), dtype=torch.uint8, device=self.device)
        self._nav_launch("nav_field", margin, soft_pen, lookahead, self.NAV_DEFAULTS["turn_sin"],
                         cost=out.get("cost"), direction=out.get("dir"), target=out["target"], geo_cost=out["geo_cost"],
                         tile=tile, frames=frames, visible=visible, lidar=lidar, lidar_map=lidar_map, predict=predict)
        gc =out["geo_cost"].to(torch.float64)
        out["geo_dist"] = torch.where(gc < 0, torch.full_like(gc, float("inf")), gc * (self.cfg.res / 5.0))
        return out

    def policy_nav(self, out: Optional[torch.Tensor] = None, margin: int = 2, soft_pen: int = 40, lookahead: int = 4,
                   turn_sin: float = 0.25, tile: Optional[int] = None, frames: Optional[torch.Tensor] = None,
                   visible: bool = False, lidar: bool = False, lidar_map: Optional["LidarMap"] = None,
                   predict=False) -> torch.Tensor:
        """The next (v, w) commands (N, 2) float64 from the navigation field of the current
        observation, on the device (include/ffmp.h ffmp_nav_field's follower): head for the cell
        `lookahead` moves down the cheapest path, turning on the spot while it lies more than
        asin(turn_sin) off the heading.  Complete on a static scene (it has no local minima, unlike
        policy_field); stateless, so on an exactly symmetric scene it can dither between two equal
        routes; obstacle velocities are looked at only with predict= (as for nav_field: the plan
        then passes behind a crossing obstacle instead of steering for the gap it is about to fill).
        (0, 0) when the goal is unreachable.  `out`:
        write into this (N, 2) float64 tensor (e.g. command_buffer) instead of a new one.  `tile`: as
        for nav_field (grids above 256 x 256 always take the tiled kernel); `frames`, `visible`, `lidar`,
        `lidar_map`: as for nav_field (plan over a plane of the caller's, over what the robot can see,
        over the map made from its scan, or over the accumulated map).  Inside a graph capture of the
        caller's: call it once eagerly first, as for nav_field."""
        self._check_open()
        if self._needs_reset:
            raise RuntimeError("call reset() before policy_nav()")
        if not self.cfg.dt > 0:
            raise ValueError("policy_nav: dt must be > 0 (the follower's turn rate divides by it)")
        if out is None:
            out = torch.empty((self.num_envs, 2), dtype=torch.float64, device=self.device)
        elif tuple(out.shape) != (self.num_envs, 2) or out.dtype != torch.float64 or not out.is_contiguous() \
                or out.device != self.device or out.data_ptr() % 16:
            raise ValueError(f"out must be a contiguous, 16-byte aligned float64 tensor of shape "
                             f"({self.num_envs}, 2) on {self.device}")
        self._nav_launch("policy_nav", margin, soft_pen, lookahead, turn_sin, cmd=out, tile=tile, frames=frames,
                         visible=visible, lidar=lidar, lidar_map=lidar_map, predict=predict)
        return out

    # ------------------------------------------------ the rollout planner
    DWA_STOP = 3       # the action id of the command (0, 0): what actions=True answers when nothing is admissible
    DWA_SPEED = 0.5    # m/s, the sampler's top obstacle speed: what the default src_reach allows for
    _dwa_tables = None  # (horizon, stride, probe) -> (H, traj, cmds) on the device
    _dwa_cost = None    # the cost plane between the two launches, kept from call to call

    def _dwa_table(self, horizon: int, stride: int, probe: float):
        """The device copy of config.rollout_table for this config, cut to the longest horizon <= `horizon`
        that keeps the table within its 28 cells (config.rollout_horizon); made once per
        (horizon, stride, probe) and dropped when the config changes."""
        key = (int(horizon), int(stride), float(probe))
        if self._dwa_tables is None:
            self._dwa_tables = {}
        t = self._dwa_tables.get(key)
        if t is None:
            H = rollout_horizon(self.cfg, horizon=key[0], stride=key[1], probe=key[2])
            traj, cmds = rollout_table(self.cfg, horizon=H, stride=key[1], probe=key[2])
            t = self._dwa_tables[key] = (H, torch.as_tensor(traj, device=self.device), torch.as_tensor(cmds, device=self.device))
        return t

    def policy_dwa(self, out: Optional[torch.Tensor] = None, horizon: int = 24, stride: int = 1, probe: float = 0.325,
                   flow=True, vel: Optional[torch.Tensor] = None, accel=None, src_reach: Optional[int] = None,
                   actions: bool = False, detail: bool = False, margin: int = 2, soft_pen: int = 40,
                   tile: Optional[int] = None, frames: Optional[torch.Tensor] = None, visible: bool = False,
                   lidar: bool = False, lidar_map: Optional["LidarMap"] = None):
        """The next (v, w) commands (N, 2) float64 from a dynamic-window / trajectory-rollout planner, on the
        device (include/ffmp.h ffmp_dwa): the reference's 28 commands (4 speeds x 7 turn rates) are each rolled
        forward through the robot's own unicycle for up to `horizon` steps of `stride` env steps, rejected
        where they leave the grid, stand on a hard cell of the navigation field, or meet a moving obstacle AT THE
        STEP the robot is there (every 255 cell with a velocity moved along it, step by step, against the
        robot's footprint), and the admissible one that ends lowest on the field — cost at the endpoint plus
        cost at the probe, the point `probe` metres ahead of it along the final heading — is chosen; (0, 0)
        when none is admissible.  Two launches: nav_field's (cost=True, with `margin`, `soft_pen`, `tile`, and
        `frames` / `visible` / `lidar` / `lidar_map` by nav_field's conventions) and ffmp_dwa's.
        horizon: an upper bound — the table holds cell offsets of at most 28, so the rollouts are cut to the
        longest horizon that fits (config.rollout_horizon: 18 at res 0.05, dt 0.1; detail=True reports it).
        flow: True — the env's own flow planes over the newest frame (ValueError if the env was made without
        flow=True); None or False — static only; a LidarFlow of this env — its estimate over its frame.
        src_reach: moving sources are looked for within this many cells of the robot (per axis); default
        min(G // 2, 31 + ceil(H * cps * 0.5)) with cps = float32(stride * dt / res) — what an obstacle at the
        sampler's top speed of 0.5 m/s can bring into the rollouts' 31 cells within the horizon.
        accel=(dv_max, dw_max) with vel, a contiguous (N, 2) float64 device tensor of the robot's present
        (v, w): only the commands within that window of it are candidates (the dynamic window).
        out: write the commands into this (N, 2) float64 tensor (e.g. command_buffer).  actions=True: return
        (N,) int64 action ids instead — the candidate number is the reference's action id; id 3 = (0, 0) when
        none is admissible.  detail=True: a dict with cmd, action, choice (N,) int32 (-1: none), score (N,)
        uint32 (0xFFFFFFFF: none), n_adm (N,) int32, blocked_at (N, 28) uint8 (the first blocked step per
        candidate, horizon + 1 if free, 0 outside the window), cost (N, G, G) uint16 and horizon.
        Known limits: present occupancy stays hard at every step (the cost plane holds it); constant-velocity
        prediction; nothing is checked between successive steps; the candidate set is discrete.  Inside a
        graph capture of the caller's: call it once eagerly first with the same arguments (the table is
        copied to the device, and nav_field's workspace made, at the first call)."""
        self._check_open()
        if self._needs_reset:
            raise RuntimeError("call reset() before policy_dwa()")
        n, G = self.num_envs, self.cfg.grid
        if isinstance(flow, LidarFlow):
            if flow.env is not self:
                raise ValueError("policy_dwa: flow must be a LidarFlow of this env")
            src, vflow = flow.frame, flow.flow
        elif flow is True:
            if self.flow is None:
                raise ValueError("policy_dwa: the env was made without flow=True; pass flow=None (static only) or a LidarFlow")
            src, vflow = self.state_m[:, 1], self.flow  # a view: the env stride of the window
        elif flow is None or flow is False:
            src = vflow = None
        else:
            raise ValueError("policy_dwa: flow must be True, None / False or a LidarFlow of this env")
        if (vel is None) != (accel is None):
            raise ValueError("policy_dwa: vel and accel=(dv_max, dw_max) go together")
        dv_max = dw_max = 0.0
        if vel is not None:
            if not isinstance(vel, torch.Tensor) or tuple(vel.shape) != (n, 2) or vel.dtype != torch.float64 \
                    or not vel.is_contiguous() or vel.device != self.device:
                raise ValueError(f"vel must be a contiguous float64 tensor of shape ({n}, 2) on {self.device}")
            dv_max, dw_max = (float(a) for a in accel)
        if actions:
            if out is not None and (tuple(out.shape) != (n,) or out.dtype != torch.int64 or not out.is_contiguous()
                                    or out.device != self.device):
                raise ValueError(f"out must be a contiguous int64 tensor of shape ({n},) on {self.device} with actions=True")
            ids, out = out, None
        if out is None:
            out = torch.empty((n, 2), dtype=torch.float64, device=self.device)
        elif tuple(out.shape) != (n, 2) or out.dtype != torch.float64 or not out.is_contiguous() \
                or out.device != self.device or out.data_ptr() % 16:
            raise ValueError(f"out must be a contiguous, 16-byte aligned float64 tensor of shape ({n}, 2) on {self.device}")
        H, traj, cmds = self._dwa_table(horizon, stride, probe)
        A = int(cmds.shape[0])
        cps = float(np.float32(int(stride) * self.cfg.dt / self.cfg.res))
        if src_reach is None:
            src_reach = min(G // 2, 31 + int(math.ceil(H * cps * self.DWA_SPEED)))
        fmts = {torch.float32: _abi.OBS_F32, torch.uint8: _abi.OBS_U8F16}
        ffmt = fmts[src.dtype] if src is not None else _abi.OBS_F32
        vfmt = _abi.OBS_U8F16 if vflow is not None and vflow.dtype == torch.float16 else _abi.OBS_F32
        _abi.check(self.lib.ffmp_dwa_check(C.byref(self._cfg_c), ffmt, vfmt, cps, int(src_reach), A, H, dv_max, dw_max),
                   "ffmp_dwa_check")
        if detail or self._dwa_cost is None or tuple(self._dwa_cost.shape) != (n, G, G):
            cost = torch.empty((n, G, G), dtype=torch.uint16, device=self.device)
            if not detail:
                self._dwa_cost = cost
        else:
            cost = self._dwa_cost
        self._nav_launch("policy_dwa", margin, soft_pen, self.NAV_DEFAULTS["lookahead"], self.NAV_DEFAULTS["turn_sin"],
                         cost=cost, tile=tile, frames=frames, visible=visible, lidar=lidar, lidar_map=lidar_map)
        choice = torch.empty(n, dtype=torch.int32, device=self.device) if actions or detail else None
        more = {}
        if detail:
            more = dict(score=torch.empty(n, dtype=torch.uint32, device=self.device),
                        n_adm=torch.empty(n, dtype=torch.int32, device=self.device),
                        blocked_at=torch.empty((n, A), dtype=torch.uint8, device=self.device))
        with torch.cuda.device(self.device):
            _abi.check(self.lib.ffmp_dwa(C.byref(self._cfg_c), n, cost.data_ptr(), G * G, _ptr(src),
                                         src.stride(0) if src is not None else 0, ffmt, _ptr(vflow),
                                         vflow.stride(0) if vflow is not None else 0, vfmt, cps, int(src_reach),
                                         traj.data_ptr(), cmds.data_ptr(), A, H, _ptr(vel), dv_max, dw_max, None,
                                         _ptr(choice), out.data_ptr(), _ptr(more.get("score")), _ptr(more.get("n_adm")),
                                         _ptr(more.get("blocked_at")), self._stream()), "ffmp_dwa")
        if actions or detail:
            act = torch.where(choice < 0, torch.full_like(choice, self.DWA_STOP), choice).to(torch.int64)
            if actions and ids is not None:
                act = ids.copy_(act)
        if detail:
            return dict(more, cmd=out, action=act, choice=choice, cost=cost, horizon=H)
        return act if actions else out

    # ------------------------------------------------ HIP graph of whole steps
    def graph_period(self) -> int:
        """Steps after which the frame pair is back on the same ring slots (so one captured
        sequence of steps can be replayed forever): W with the seamless ring, W - 1 with the
        wrapping ring (its wrap step writes both frames), 1 with W = 2."""
        if self.ring == "seamless":
            return self.frame_window
        return self.frame_window - 1 if self.frame_window > 2 else 1

    def capture(self, steps: Optional[int] = None, pipelined: Optional[bool] = None,
                skewed: Optional[bool] = None, policy=None, commands: bool = False) -> "StepGraph":
        """Capture `steps` consecutive steps (default graph_period(); a multiple of it) into one HIP
        graph (torch.cuda.CUDAGraph: hipGraph on ROCm).  StepGraph.replay(actions) then runs them as
        ONE launch from the host — every kernel of every step, the same launches step() makes, with
        no host work or launch gaps between them; the actions are read from a static device block the
        replay fills first.  The host's frame bookkeeping is advanced by the replay, not by the
        capture (nothing runs while capturing).  `pipelined` (two-launch steps, an even count; off by
        default, StepGraph.PIPELINE_DEFAULT): the env kernel of step i + 1 runs beside the raster of
        step i (see StepGraph).  `skewed` (float32 frames, no flow planes, the two-launch step, an even
        count; by default where the env step's blocks fit the CUs once, StepGraph._skew_pays): the
        raster of step i and the env step of step i + 1 in ONE launch (ffmp_step_skewed).
        `policy` (closed loop): "reactive" (policy_reactive) or a callable env -> (N,) int64 device
        tensor, captured too: each step's actions are computed inside the graph from the previous
        step's observation (the first from the observation before the replay), and replay() takes
        no actions — the device-resident form of train.py:572-577's act-then-publish loop.  Plain
        two-launch (or one-launch) steps only: the policy reads the raster's frame.
        Continuous (v, w) commands (SPEC a15b): policy="field" (policy_field) or policy="nav"
        (policy_nav with its defaults; the static block is
        (steps, N, 2) float64 and replay() takes no actions), or commands=True for an open loop whose
        replay(cmds) takes a (steps, N, 2) block.  Command graphs run plain steps: pipelined=True or
        skewed=True raises ValueError (the skewed launch reads ids a step ahead), and their defaults
        resolve to off.
        The graph holds the config (the seed included) by value: after reset(seed=s), seed(s) or a
        load_state_dict() with another seed its replay() raises RuntimeError and the steps have to be
        captured again; the same seed, reset(), reset(mask=), raster() and set_scenarios() leave it
        valid.
        Warm-up: a capture runs nothing and copies nothing from the host, so whatever a callable
        policy calls must have run once before — lidar_frames() builds its sector table on the host
        at its first call for a beam count, and the tiled nav_field() / policy_nav() allocates its
        workspace and sets its kernel up at its first call (policy="nav" does that here, before the
        capture begins).  Call the policy once eagerly, then capture."""
        return StepGraph(self, steps, pipelined, skewed, policy, commands)

    # ------------------------------------------------ gym.vector.VectorEnv surface
    is_vector_env = True

    @property
    def single_action_space(self):
        """The action id train.py feeds to RobotAction.commander (train.py:343-345, 668-673);
        the reference's Box (ffmp.py:29-32) describes the (v, w) it maps to."""
        from ._spaces import Discrete
        return Discrete(28)

    @property
    def action_space(self):
        from ._spaces import MultiDiscrete
        return MultiDiscrete([28] * self.num_envs)

    @property
    def single_command_space(self):
        """The (v, w) command step() also takes (SPEC a15b): the reference's action Box
        [0, -0.6] .. [0.6, 0.6] (ffmp.py:29-32), float32."""
        from ._spaces import Box
        from .config import CMD_V, CMD_W
        return Box(np.array([CMD_V[0], CMD_W[0]], dtype=np.float32),
                   np.array([CMD_V[-1], CMD_W[-1]], dtype=np.float32), dtype=np.float32)

    @property
    def command_space(self):
        from ._spaces import Box
        one = self.single_command_space
        return Box(np.broadcast_to(one.low, (self.num_envs, 2)), np.broadcast_to(one.high, (self.num_envs, 2)),
                   dtype=np.float32)

    def _obs_space(self, lead):
        """Keys/dtypes of the train.py consumer contract (train.py:543-557), bounds per key."""
        from ._spaces import Box, Dict as DictSpace
        G, L = self.cfg.grid, self.cfg.n_beams
        inf = np.inf

        def box(lo, hi, shape, dtype=np.float32):
            lo = np.broadcast_to(np.asarray(lo, dtype=dtype), lead + shape)
            hi = np.broadcast_to(np.asarray(hi, dtype=dtype), lead + shape)
            return Box(lo, hi, dtype=dtype)

        compact = self.obs_format == "u8f16"
        sp = {"state_m": box(0, 255, (2, G, G), np.uint8) if compact else box(0.0, 255.0, (2, G, G)),
              "state_g": box([0.0, -np.pi], [inf, np.pi], (2,)),   # [dist, orient]
              "state_v": box([0.0, -np.pi], [inf, np.pi], (2,)),   # [|dxy|, wrap(dyaw)] per step
              "state_t": box(0.0, inf, (1,)),
              "grad": box(-inf, inf, (2,))}
        if self.potential is not None:
            sp["potential"] = box(0.0, inf, (G, G), np.float16 if compact else np.float32)
        if L:
            sp["lidar"] = box(-inf, inf, (L,))
        if self.flow is not None:
            sp["flow"] = box(-inf, inf, (2, G, G), np.float16 if compact else np.float32)
        return DictSpace(sp)

    @property
    def single_observation_space(self):
        return self._obs_space(())

    @property
    def observation_space(self):
        return self._obs_space((self.num_envs,))

    def seed(self, seed: int) -> None:
        """gym 0.17-style: the seed of the next full reset()."""
        self._set_cfg(self.cfg.replace(seed=int(seed)))

    _cfg_gen = 0  # config generation: counts the configs that differed from their predecessor

    def _set_cfg(self, cfg: FFMPConfig) -> None:
        """A new config after construction (a new seed): the launch struct is rebuilt and the
        config generation moves on.  Graphs captured the old struct by value: the single-step
        graphs are dropped (re-captured on use), a StepGraph of an older generation refuses to
        replay.  A config equal to the current one (reset(seed=<the same seed>)) changes nothing."""
        if cfg == self.cfg:
            return
        self.cfg = cfg
        self._cfg_c = _abi.make_cfg(self.cfg, _ptr(self.beam_cs) or 0)
        self._cfg_gen += 1
        self._dwa_tables = None  # rollout tables hold the old config's dt and res
        if self._graphs is not None:
            self._graphs = {}

    def step_async(self, actions) -> None:
        self._pending_actions = actions

    def step_wait(self, **kw):
        a, self._pending_actions = self._pending_actions, None
        if a is None:
            raise RuntimeError("step_wait() without step_async()")
        return self.step(a, **kw)

    def close(self) -> None:
        """Release the device buffers (the object is unusable afterwards: every entry point that
        would launch a kernel raises RuntimeError)."""
        if self._closed:
            return
        self._closed = True
        self._needs_reset = True
        torch.cuda.synchronize(self.device)
        self._graphs = None  # their kernels' arguments point into the buffers freed below
        self.action_buffer = None
        self.command_buffer = None
        for name, _, _ in self._buffer_specs():
            setattr(self, name, None)
        # the launch structs hold raw device pointers into the freed buffers
        self._state_c = self._obs_c = self._out_c = None
        self._slices = []
        self._arena_buf = None
        self._record_alt = None
        self._nav_ws = None
        self._dwa_tables = self._dwa_cost = None
        for ref in self._world_maps or ():
            holder = ref()
            if holder is not None:
                holder._release()
        self._world_maps = None
        self.bev = None
        had_ring = self.ring == "seamless"
        self._ring = None  # the seamless ring's pieces return to the process pool ...
        self._forget_partners()  # the potential plane is freed: its pairing references go
        torch.cuda.empty_cache()
        if had_ring and self.release_pool:
            import gc
            gc.collect()  # ... once the last tensor view of the ring is gone
            _abi.ring_pool_trim(self.device.index, self.pool_keep_bytes)  # ... and their memory to the device

    _closed = False
    _world_maps = None  # weak references to the WorldMap holders of world_map(): close() releases their planes
    bev = None  # the BEV image ring (bev_series); a class default: _alloc's HBM accounting runs first

    def _check_open(self) -> None:
        if self._closed:
            raise RuntimeError("FFMPVec is closed")

    # ------------------------------------------------------------ utilities
    def check_errors(self) -> None:
        """Raise if any step saw an action id outside 0..27 (bit 1; it was run as action 3) or a NaN
        command (bit 2; it was run as (0, 0)), or set_scenarios a bad scenario (bit 4: a non-finite
        word, a negative radius or |yaw| > 1024; the env was left as it was).  Clears the bits."""
        v = int(self.err.item())
        if v:
            self.err.zero_()
            if v == 1:  # the ids path alone: its message as it always was
                raise ValueError(f"invalid action id(s) passed to FFMPVec.step (error bits {v:#x})")
            if v & 4:
                step = ([] if not v & 1 else ["invalid action id(s)"]) + ([] if not v & 2 else ["NaN command(s)"])
                raise ValueError("bad scenario(s) passed to FFMPVec.set_scenarios (non-finite word, negative radius "
                                 "or |yaw| > 1024: those envs were left unchanged)" +
                                 (f" and {' and '.join(step)} passed to FFMPVec.step" if step else "") +
                                 f" (error bits {v:#x})")
            what = ([] if not v & 1 else ["invalid action id(s)"]) + ([] if not v & 2 else ["NaN command(s)"])
            raise ValueError(f"{' and '.join(what) or 'errors'} passed to FFMPVec.step (error bits {v:#x}; "
                             "bit 2: NaN command)")

    # simulator state, then the per-env observations and outputs the env kernel wrote (the planes
    # are re-rastered from the record on load)
    _SD_STATE = ("pose", "goal", "d0", "obst", "obst_r", "t", "episode", "record")
    _SD_OBS = ("state_g", "state_v", "state_t", "grad", "lidar", "reward", "done", "is_goal", "collision",
               "truncated", "term_record", "term_obs")

    def state_dict(self) -> Dict[str, torch.Tensor]:
        """Checkpoint: the simulator state plus the small observations and step outputs (the
        planes are re-derived from the record by load_state_dict's raster())."""
        self._check_open()
        sd = {k: getattr(self, k).clone() for k in self._SD_STATE}
        for k in self._SD_OBS:
            v = getattr(self, k)
            if v is not None:
                sd[k] = v.clone()
        sd["seed"] = torch.tensor(self.cfg.seed, dtype=torch.int64)
        return sd

    def load_state_dict(self, sd: Dict[str, torch.Tensor]) -> None:
        """Restore a state_dict() of an env of the same config and num_envs (a fresh instance
        included): every observation key of the saved env is reproduced."""
        self._check_open()
        for k in self._SD_STATE:
            getattr(self, k).copy_(sd[k])
        for k in self._SD_OBS:
            v = getattr(self, k)
            if v is not None and k in sd:
                v.copy_(sd[k])
        seed = int(sd["seed"])
        if seed != self.cfg.seed:
            self._set_cfg(self.cfg.replace(seed=seed))
        self.raster()
        self._hist, self._hist_from_reset = [], False  # older frames than the pair are not restored
        self._note_window(True)
        self._bev_hist, self._bev_from_reset = [self._bev_pos], False  # likewise older BEV images
        self._needs_reset = False

    def hbm_bytes(self) -> int:
        """HBM this instance holds now: its arena plus the seamless ring's W physical slots (the
        alias slot maps slot 0's pages again and holds nothing)."""
        ring = 0
        if self.ring == "seamless" and getattr(self, "_ring", None) is not None:
            ring = self.frame_window * self._ring.slot_stride
        alt = getattr(self, "_record_alt", None)  # a pipelined step graph's second record buffer
        if self._arena_buf is not None:
            return self._arena_buf.numel() + ring + (0 if alt is None else alt.numel() * alt.element_size())
        return ring + sum(t.numel() * t.element_size() for t in vars(self).values()
                          if isinstance(t, torch.Tensor) and not (ring and t is self._frames))

    def __repr__(self):
        c = self.cfg
        return (f"FFMPVec(num_envs={self.num_envs}, G={c.grid}, K={c.n_obst}, L={c.n_beams}, "
                f"moving={c.moving}, device={self.device}, env_offset={self.env_offset}, "
                f"frame_window={self.frame_window}, ring={self.ring}, obs_format={self.obs_format})")


__all__ = ["FFMPVec", "PRESETS"]


class LidarMap:
    """The accumulated scan map of an FFMPVec (FFMPVec.lidar_map; include/ffmp.h ffmp_scan_map, DESIGN §3
    a19c): two (N, G, G) int8 log-odds planes used as a ping-pong pair, the (N, G, G) frame in the env's
    frame dtype, and the pose words and episode ids of the last update — the previous pose is the
    holder's own, so an update after any number of steps uses the right motion, a second update in
    the same step is an identity warp, and a missed auto-reset is still caught through the episode id.
    The step, its frames, its lidar and its record are never written."""

    def __init__(self, env: FFMPVec, unknown: int, thickness: float, range_max: float, l_hit: int, l_free: int, l_max: int,
                 decay: int, occ_thr: int, free_thr: int, frame: bool = True):
        self.env = env
        self.knobs = (env._fmt, int(unknown), float(thickness), float(range_max), int(l_hit), int(l_free), int(l_max),
                      int(decay), int(occ_thr), int(free_thr))
        _abi.check(env.lib.ffmp_scan_map_check(C.byref(env._cfg_c), 1, *self.knobs, 0), "ffmp_scan_map_check")
        n, G = env.num_envs, env.cfg.grid
        self._planes = torch.zeros((2, n, G, G), dtype=torch.int8, device=env.device)
        self._cur = 0
        self.frame = torch.full((n, G, G), int(unknown), dtype=env._frame_dtype, device=env.device) if frame else None
        self._pose = torch.zeros((n, 4), dtype=torch.float32, device=env.device)
        self._episode = torch.full((n,), -1, dtype=torch.int32, device=env.device)  # no episode: every env restarts

    @property
    def log_odds(self) -> torch.Tensor:
        """The current (N, G, G) int8 plane: 0 nothing known, positive occupied, negative free."""
        return self._planes[self._cur]

    def _mask(self, mask) -> Optional[torch.Tensor]:
        if mask is None:
            return None
        return torch.as_tensor(mask, device=self.env.device).reshape(self.env.num_envs).to(torch.uint8).contiguous()

    def reset(self, mask: Optional[torch.Tensor] = None) -> None:
        """Forget the map of the selected envs (mask: (N,) bool or uint8; None = all): log-odds 0, the
        frame `unknown`, and the next update restarts them."""
        if mask is None:
            self.log_odds.zero_()
            self._episode.fill_(-1)
            if self.frame is not None:
                self.frame.fill_(self.knobs[1])
            return
        sel = self._mask(mask).bool()
        self.log_odds[sel] = 0
        self._episode[sel] = -1
        if self.frame is not None:
            self.frame[sel] = self.knobs[1]

    def update(self, ranges: Optional[torch.Tensor] = None, pose: Optional[torch.Tensor] = None,
               first: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None, plain: bool = False
               ) -> Optional[torch.Tensor]:
        """Move the map into the current ego frame and add the current scan: one launch on the current
        stream, then two tiny copies (the pose words and episode ids) on the same stream.  Returns
        the frame.
        ranges: a contiguous (N, L') float32 device tensor instead of the env's `lidar`, as in
        lidar_frames.  pose: a contiguous (N, 4) float32 device tensor {x, y, cos yaw, sin yaw}
        instead of record words 0..3 (ros_adapters.odom_to_pose_row makes a row).  first: (N,) bool,
        the envs whose map starts anew; by default the envs whose episode id has changed since the
        last update or whose record says it has just reset — with pose= given the env's own
        bookkeeping is not looked at, and without first= no env restarts (but those never updated or
        reset()).  mask: (N,) bool or uint8, envs with 0 keep their map, their frame and their saved
        pose.  plain: the kernel without its search shortcut (the same bits)."""
        env = self.env
        env._check_open()
        if env._needs_reset:
            raise RuntimeError("call reset() before LidarMap.update()")
        n, G = env.num_envs, env.cfg.grid
        if ranges is None:
            if env.lidar is None:
                raise ValueError("LidarMap.update: the env has n_beams == 0, pass ranges=")
            ranges = env.lidar
        elif not isinstance(ranges, torch.Tensor) or ranges.dim() != 2 or ranges.shape[0] != n or ranges.dtype != torch.float32 \
                or not ranges.is_contiguous() or ranges.device != env.device:
            raise ValueError(f"ranges must be a contiguous float32 tensor of shape ({n}, L) on {env.device}")
        never = self._episode < 0
        if pose is None:
            pose = env.record
            if first is None:
                first = (env.episode != self._episode) | (env.record[:, 10] != 0)
            episode = env.episode
        else:
            if not isinstance(pose, torch.Tensor) or tuple(pose.shape) != (n, 4) or pose.dtype != torch.float32 \
                    or not pose.is_contiguous() or pose.device != env.device:
                raise ValueError(f"pose must be a contiguous float32 tensor of shape ({n}, 4) on {env.device}")
            episode = torch.zeros_like(self._episode)
        if first is None:
            first = never
        else:
            first = torch.as_tensor(first, device=env.device).reshape(n).bool() | never
        mask = self._mask(mask)
        L = int(ranges.shape[1])
        flags = _abi.SCAN_PLAIN if plain else 0
        _abi.check(env.lib.ffmp_scan_map_check(C.byref(env._cfg_c), L, *self.knobs, flags), "ffmp_scan_map_check")
        sectors = env._sectors(L)
        src, dst = self._planes[self._cur], self._planes[1 - self._cur]
        with torch.cuda.device(env.device):
            _abi.check(env.lib.ffmp_scan_map(C.byref(env._cfg_c), n, ranges.data_ptr(), ranges.stride(0), L,
                                             sectors.data_ptr(), pose.data_ptr(), pose.stride(0), self._pose.data_ptr(), 4,
                                             _ptr(mask), first.data_ptr(), src.data_ptr(), dst.data_ptr(), G * G,
                                             _ptr(self.frame), G * G, *self.knobs, flags, env._stream()), "ffmp_scan_map")
        if mask is None:
            self._pose.copy_(pose[:, 0:4])
            self._episode.copy_(episode)
        else:
            sel = mask.bool()
            self._pose.copy_(torch.where(sel.unsqueeze(1), pose[:, 0:4], self._pose))
            self._episode.copy_(torch.where(sel, episode, self._episode))
        self._cur = 1 - self._cur
        return self.frame


class WorldMap:
    """The world-fixed scan map of an FFMPVec (FFMPVec.world_map; include/ffmp.h ffmp_world_map /
    ffmp_world_frame): one (N, cells, cells) int8 log-odds plane, row p world x and
    column q world y, cell (p, q) centred on (origin + p * resolution, origin + q * resolution), updated
    in place — no second plane — and the episode ids of the last update, so a missed auto-reset still
    restarts the env.  The step, its frames, its lidar and its record are never written; the env's
    close() releases the plane."""

    def __init__(self, env: FFMPVec, cells: int, unknown: int, outside: int, thickness: float, range_max: float, l_hit: int,
                 l_free: int, l_max: int, decay: int, occ_thr: int, free_thr: int):
        self.env = env
        self.cells = int(cells)
        self.knobs = (float(thickness), float(range_max), int(l_hit), int(l_free), int(l_max), int(decay))
        self.view = (env._fmt, int(unknown), int(outside), int(occ_thr), int(free_thr))
        _abi.check(env.lib.ffmp_world_map_check(C.byref(env._cfg_c), 1, self.cells, *self.knobs, 0), "ffmp_world_map_check")
        _abi.check(env.lib.ffmp_world_frame_check(C.byref(env._cfg_c), self.cells, *self.view), "ffmp_world_frame_check")
        n = env.num_envs
        self._plane = torch.zeros((n, self.cells, self.cells), dtype=torch.int8, device=env.device)
        self._episode = torch.full((n,), -1, dtype=torch.int32, device=env.device)  # no episode: every env restarts

    @property
    def log_odds(self) -> torch.Tensor:
        """The (N, cells, cells) int8 plane: 0 nothing known, positive occupied, negative free."""
        self._check()
        return self._plane

    @property
    def resolution(self) -> float:
        """Metres per cell: the env's res."""
        return float(self.env.cfg.res)

    @property
    def origin(self) -> float:
        """World coordinate (both axes) of the centre of cell (0, 0): -(float32)(cells * res / 2)."""
        return -float(np.float32(self.cells * self.env.cfg.res / 2.0))

    @property
    def bytes(self) -> int:
        """Device bytes of the log-odds plane."""
        return self.env.num_envs * self.cells * self.cells

    def _check(self) -> None:
        if self._plane is None:
            raise RuntimeError("the WorldMap's env is closed")

    def _release(self) -> None:
        self._plane = self._episode = None

    def _mask(self, mask) -> Optional[torch.Tensor]:
        if mask is None:
            return None
        return torch.as_tensor(mask, device=self.env.device).reshape(self.env.num_envs).to(torch.uint8).contiguous()

    def _pose(self, pose) -> torch.Tensor:
        env = self.env
        if pose is None:
            return env.record
        n = env.num_envs
        if not isinstance(pose, torch.Tensor) or tuple(pose.shape) != (n, 4) or pose.dtype != torch.float32 \
                or not pose.is_contiguous() or pose.device != env.device:
            raise ValueError(f"pose must be a contiguous float32 tensor of shape ({n}, 4) on {env.device}")
        return pose

    def reset(self, mask: Optional[torch.Tensor] = None) -> None:
        """Forget the map of the selected envs (mask: (N,) bool or uint8; None = all): log-odds 0, and the
        next update restarts them."""
        self._check()
        if mask is None:
            self._plane.zero_()
            self._episode.fill_(-1)
            return
        sel = self._mask(mask).bool()
        self._plane[sel] = 0
        self._episode[sel] = -1

    def update(self, ranges: Optional[torch.Tensor] = None, pose: Optional[torch.Tensor] = None,
               first: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None, plain: bool = False) -> torch.Tensor:
        """Add the current scan at the current pose: one launch on the current stream, in place, then one
        tiny copy (the episode ids) on the same stream.  Returns the log-odds plane.
        ranges, pose, first, mask, plain: LidarMap.update's conventions — ranges a contiguous (N, L')
        float32 device tensor instead of the env's `lidar`; pose a contiguous (N, 4) float32 device tensor
        {x, y, cos yaw, sin yaw} instead of record words 0..3, and then the env's own bookkeeping is not
        looked at: without first= no env restarts (but those never updated or reset()); first: (N,)
        bool, the envs whose map starts anew, by default those whose episode id has changed since the
        last update or whose record says it has just reset; mask: envs with 0 keep their map."""
        env = self.env
        env._check_open()
        self._check()
        if env._needs_reset:
            raise RuntimeError("call reset() before WorldMap.update()")
        n = env.num_envs
        if ranges is None:
            if env.lidar is None:
                raise ValueError("WorldMap.update: the env has n_beams == 0, pass ranges=")
            ranges = env.lidar
        elif not isinstance(ranges, torch.Tensor) or ranges.dim() != 2 or ranges.shape[0] != n or ranges.dtype != torch.float32 \
                or not ranges.is_contiguous() or ranges.device != env.device:
            raise ValueError(f"ranges must be a contiguous float32 tensor of shape ({n}, L) on {env.device}")
        never = self._episode < 0
        if pose is None:
            if first is None:
                first = (env.episode != self._episode) | (env.record[:, 10] != 0)
            episode = env.episode
        else:
            episode = torch.zeros_like(self._episode)
        pose = self._pose(pose)
        if first is None:
            first = never
        else:
            first = torch.as_tensor(first, device=env.device).reshape(n).bool() | never
        mask = self._mask(mask)
        L = int(ranges.shape[1])
        flags = _abi.SCAN_PLAIN if plain else 0
        _abi.check(env.lib.ffmp_world_map_check(C.byref(env._cfg_c), L, self.cells, *self.knobs, flags), "ffmp_world_map_check")
        sectors = env._sectors(L)
        with torch.cuda.device(env.device):
            _abi.check(env.lib.ffmp_world_map(C.byref(env._cfg_c), n, ranges.data_ptr(), ranges.stride(0), L, sectors.data_ptr(),
                                              pose.data_ptr(), pose.stride(0), _ptr(mask), first.data_ptr(),
                                              self._plane.data_ptr(), self.cells * self.cells, self.cells, *self.knobs, flags,
                                              env._stream()), "ffmp_world_map")
        if mask is None:
            self._episode.copy_(episode)
        else:
            self._episode.copy_(torch.where(mask.bool(), episode, self._episode))
        return self._plane

    def ego_frame(self, pose: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The map as the robot at `pose` (by default the env's current pose) sees it: (N, G, G) in the
        env's frame dtype — one launch on the current stream, read-only on the map.  out: a contiguous
        tensor of that shape and dtype to write into."""
        env = self.env
        env._check_open()
        self._check()
        if pose is None and env._needs_reset:
            raise RuntimeError("call reset() before WorldMap.ego_frame()")
        pose = self._pose(pose)
        n, G = env.num_envs, env.cfg.grid
        if out is None:
            out = torch.empty((n, G, G), dtype=env._frame_dtype, device=env.device)
        elif not isinstance(out, torch.Tensor) or tuple(out.shape) != (n, G, G) or out.dtype != env._frame_dtype \
                or not out.is_contiguous() or out.device != env.device:
            raise ValueError(f"out must be a contiguous {env._frame_dtype} tensor of shape ({n}, {G}, {G}) on {env.device}")
        with torch.cuda.device(env.device):
            _abi.check(env.lib.ffmp_world_frame(C.byref(env._cfg_c), n, pose.data_ptr(), pose.stride(0), self._plane.data_ptr(),
                                                self.cells * self.cells, self.cells, out.data_ptr(), G * G, *self.view,
                                                env._stream()), "ffmp_world_frame")
        return out

    _match_tables = None  # (L or (T, dtheta)) -> device tensor: config.beam_dirs / config.turn_table

    def _match_table(self, key, make) -> torch.Tensor:
        if self._match_tables is None:
            self._match_tables = {}
        if key not in self._match_tables:
            self._match_tables[key] = torch.as_tensor(make()).to(self.env.device).contiguous()
        return self._match_tables[key]

    def match(self, ranges: Optional[torch.Tensor] = None, pose: Optional[torch.Tensor] = None, radius: int = 4, turns: int = 4,
              dtheta: Optional[float] = None, min_valid: Optional[int] = None, min_gain: int = 0,
              range_max: Optional[float] = None, detail: bool = False, volume: bool = False, out: Optional[torch.Tensor] = None,
              mask: Optional[torch.Tensor] = None, flags: int = 0):
        """The pose corrected against the map (include/ffmp.h ffmp_scan_match): the scan's endpoints scored on
        the plane at every whole-cell shift within `radius` cells and every rotation of up to `turns` steps of
        `dtheta` round the prior `pose`, and the best candidate's pose — (N, 4) float32 {x, y, cos yaw, sin yaw},
        what update(pose=) and ego_frame(pose=) take; an env the gate refuses keeps its prior bit for bit.  One
        launch on the current stream, read-only on the map.
        ranges, pose: as update() takes them (by default the env's lidar and record words 0..3).  dtheta: by
        default res / lidar_range, one cell of arc at full range; min_valid: the fewest valid beams an env is
        matched on, by default max(8, L // 6); min_gain: the least the best score must exceed the prior's by;
        range_max: by default the map's.  detail: also return info (N, 8) int32 {status, k, a, b, S_best,
        S(0,0,0), valid, 0}; volume: also return every score (N, 2 turns + 1, 2 radius + 1, 2 radius + 1) int32.
        out: a contiguous (N, 4) float32 tensor to write the pose into; mask: envs with 0 keep their row of
        out (with out=None: their prior).  flags: ffmp_scan_match's (_abi.MATCH_GLOBAL: accepted, no effect)."""
        env = self.env
        env._check_open()
        self._check()
        if pose is None and env._needs_reset:
            raise RuntimeError("call reset() before WorldMap.match()")
        n = env.num_envs
        if ranges is None:
            if env.lidar is None:
                raise ValueError("WorldMap.match: the env has n_beams == 0, pass ranges=")
            ranges = env.lidar
        elif not isinstance(ranges, torch.Tensor) or ranges.dim() != 2 or ranges.shape[0] != n or ranges.dtype != torch.float32 \
                or not ranges.is_contiguous() or ranges.device != env.device:
            raise ValueError(f"ranges must be a contiguous float32 tensor of shape ({n}, L) on {env.device}")
        pose = self._pose(pose)
        L, R, T = int(ranges.shape[1]), int(radius), int(turns)
        dtheta = env.cfg.res / env.cfg.lidar_range if dtheta is None else float(dtheta)
        min_valid = max(8, L // 6) if min_valid is None else int(min_valid)
        rm = self.knobs[1] if range_max is None else float(range_max)
        _abi.check(env.lib.ffmp_scan_match_check(C.byref(env._cfg_c), L, self.cells, R, T, rm, min_valid, int(min_gain), int(flags)),
                   "ffmp_scan_match_check")
        mask = self._mask(mask)
        if out is None:
            out = torch.empty((n, 4), dtype=torch.float32, device=env.device)
            if mask is not None:
                out.copy_(pose[:, 0:4])
        elif not isinstance(out, torch.Tensor) or tuple(out.shape) != (n, 4) or out.dtype != torch.float32 \
                or not out.is_contiguous() or out.device != env.device:
            raise ValueError(f"out must be a contiguous float32 tensor of shape ({n}, 4) on {env.device}")
        info = torch.zeros((n, 8), dtype=torch.int32, device=env.device) if detail else None
        vol = torch.zeros((n, 2 * T + 1, 2 * R + 1, 2 * R + 1), dtype=torch.int32, device=env.device) if volume else None
        beams = self._match_table(L, lambda: beam_dirs(L))
        table = self._match_table((T, dtheta), lambda: turn_table(T, dtheta))
        with torch.cuda.device(env.device):
            _abi.check(env.lib.ffmp_scan_match(C.byref(env._cfg_c), n, ranges.data_ptr(), ranges.stride(0), L, beams.data_ptr(),
                                               pose.data_ptr(), pose.stride(0), _ptr(mask), self._plane.data_ptr(),
                                               self.cells * self.cells, self.cells, table.data_ptr(), T, R, rm, min_valid,
                                               int(min_gain), out.data_ptr(), _ptr(info), _ptr(vol), int(flags), env._stream()),
                       "ffmp_scan_match")
        if not detail and not volume:
            return out
        return (out,) + ((info,) if detail else ()) + ((vol,) if volume else ())

    _reloc_work = None  # the relocalisation's workspace, kept by its size

    def relocalize(self, ranges: Optional[torch.Tensor] = None, pose: Optional[torch.Tensor] = None, radius: Optional[int] = None,
                   turns: int = 90, dtheta: Optional[float] = None, block: int = 8, min_valid: Optional[int] = None,
                   min_score: Optional[int] = None, min_gain: int = 0, range_max: Optional[float] = None, refine: bool = True,
                   detail: bool = False, bounds: bool = False, out: Optional[torch.Tensor] = None,
                   mask: Optional[torch.Tensor] = None, flags: int = 0):
        """The pose found again on the map over a wide window or with no prior at all (include/ffmp.h
        ffmp_scan_relocalize): match()'s winner over `radius` up to 1024 cells and `turns` up to 512 steps of
        `dtheta`, by a pruned two-level search with blocks of `block` x `block` shifts — the same bits as the
        exhaustive search.  Six launches on the current stream, read-only on the map; (N, 4) float32.
        pose=None: no prior — the plane's centre with yaw 0, radius cells // 2 and dtheta 2 pi / (2 turns + 1),
        the whole plane and the full circle.  With a pose: radius 32 and match()'s dtheta by default.
        ranges, min_valid, min_gain, range_max, out, mask: match()'s.  min_score: the least score that is believed
        (None: no such rule).  refine: follow the search with one match() launch at its answer on the envs of
        status 1 — radius 2, match()'s default dtheta, turns = min(32, ceil(dtheta / fine / 2)) — which recovers
        the angular resolution the coarse rotation step gave up.  detail: also return the search's info (N, 8)
        int32 {status, k, a, b, S_best, S(0,0,0), valid, refined blocks}; bounds: also return every U
        (N, 2 turns + 1, nb, nb) int32.  flags: _abi.RELOC_EXHAUSTIVE refines every block (the same pose)."""
        env = self.env
        env._check_open()
        self._check()
        n = env.num_envs
        if ranges is None:
            if env.lidar is None:
                raise ValueError("WorldMap.relocalize: the env has n_beams == 0, pass ranges=")
            if env._needs_reset:
                raise RuntimeError("call reset() before WorldMap.relocalize()")
            ranges = env.lidar
        elif not isinstance(ranges, torch.Tensor) or ranges.dim() != 2 or ranges.shape[0] != n or ranges.dtype != torch.float32 \
                or not ranges.is_contiguous() or ranges.device != env.device:
            raise ValueError(f"ranges must be a contiguous float32 tensor of shape ({n}, L) on {env.device}")
        L, T, B = int(ranges.shape[1]), int(turns), int(block)
        fine = env.cfg.res / env.cfg.lidar_range
        if pose is None:
            pose = self._match_table("centre", lambda: np.tile(np.array([[0.0, 0.0, 1.0, 0.0]], np.float32), (n, 1)))
            R = self.cells // 2 if radius is None else int(radius)
            dtheta = 2.0 * math.pi / (2 * T + 1) if dtheta is None else float(dtheta)
        else:
            pose = self._pose(pose)
            R = 32 if radius is None else int(radius)
            dtheta = fine if dtheta is None else float(dtheta)
        min_valid = max(8, L // 6) if min_valid is None else int(min_valid)
        min_score = -2 ** 31 if min_score is None else int(min_score)
        rm = self.knobs[1] if range_max is None else float(range_max)
        _abi.check(env.lib.ffmp_scan_relocalize_check(C.byref(env._cfg_c), L, self.cells, R, T, B, rm, min_valid, int(min_gain),
                                                      int(flags)), "ffmp_scan_relocalize_check")
        mask = self._mask(mask)
        if out is None:
            out = torch.empty((n, 4), dtype=torch.float32, device=env.device)
            if mask is not None:
                out.copy_(pose[:, 0:4])
        elif not isinstance(out, torch.Tensor) or tuple(out.shape) != (n, 4) or out.dtype != torch.float32 \
                or not out.is_contiguous() or out.device != env.device:
            raise ValueError(f"out must be a contiguous float32 tensor of shape ({n}, 4) on {env.device}")
        info = torch.zeros((n, 8), dtype=torch.int32, device=env.device) if (detail or refine) else None
        nb = (2 * R + B) // B
        U = torch.zeros((n, 2 * T + 1, nb, nb), dtype=torch.int32, device=env.device) if bounds else None
        per_env = int(env.lib.ffmp_scan_relocalize_work(self.cells, R, T, B))
        if per_env < 0:
            _abi.check(per_env, "ffmp_scan_relocalize_work")
        if self._reloc_work is None or self._reloc_work.numel() != n * per_env:
            self._reloc_work = None
            self._reloc_work = torch.empty((n * per_env,), dtype=torch.uint8, device=env.device)
        work = self._reloc_work
        beams = self._match_table(L, lambda: beam_dirs(L))
        table = self._match_table((T, dtheta), lambda: turn_table(T, dtheta))
        with torch.cuda.device(env.device):
            _abi.check(env.lib.ffmp_scan_relocalize(C.byref(env._cfg_c), n, ranges.data_ptr(), ranges.stride(0), L, beams.data_ptr(),
                                                    pose.data_ptr(), pose.stride(0), _ptr(mask), self._plane.data_ptr(),
                                                    self.cells * self.cells, self.cells, table.data_ptr(), T, R, B, rm, min_valid,
                                                    int(min_gain), min_score, out.data_ptr(), _ptr(info), _ptr(U), work.data_ptr(),
                                                    work.numel(), int(flags), env._stream()), "ffmp_scan_relocalize")
        if refine:
            found = info[:, 0] == 1
            if mask is not None:
                found = found & mask.bool()
            self.match(ranges=ranges, pose=out.clone(), radius=2, turns=min(32, max(0, math.ceil(dtheta / fine / 2.0))),
                       min_valid=min_valid, range_max=rm, out=out, mask=found)
        if not detail and not bounds:
            return out
        return (out,) + ((info,) if detail else ()) + ((U,) if bounds else ())

    def localizer(self, radius: int = 2, turns: int = 2, dtheta: Optional[float] = None, min_valid: Optional[int] = None,
                  min_gain: int = 0, range_max: Optional[float] = None) -> "Localizer":
        """A holder that keeps the per-env map <- odom transform and corrects every odometry pose against this
        map before the scan is integrated (Localizer.step)."""
        self._check()
        return Localizer(self, radius, turns, dtheta, min_valid, min_gain, range_max)


class Localizer:
    """Scan-to-map localisation over a WorldMap (WorldMap.localizer): `transform` (N, 3)
    float64 {tx, ty, theta} on the device, the rigid motion that takes an odometry pose into the map's frame.
    step() composes the prior from it, matches, recomputes it, and updates the map at the matched pose."""

    def __init__(self, world_map: WorldMap, radius: int, turns: int, dtheta, min_valid, min_gain: int, range_max):
        self.map = world_map
        self.knobs = dict(radius=int(radius), turns=int(turns), dtheta=dtheta, min_valid=min_valid, min_gain=int(min_gain),
                          range_max=range_max)
        env = world_map.env
        self._tf = torch.zeros((env.num_envs, 3), dtype=torch.float64, device=env.device)
        self._seen = torch.zeros((env.num_envs,), dtype=torch.bool, device=env.device)

    @property
    def transform(self) -> torch.Tensor:
        """(N, 3) float64 {tx, ty, theta}: map <- odom."""
        return self._tf

    def step(self, odom: torch.Tensor, ranges: Optional[torch.Tensor] = None, first: Optional[torch.Tensor] = None,
             update: bool = True) -> torch.Tensor:
        """odom: a contiguous (N, 4) float32 device tensor {x, y, cos yaw, sin yaw}, the odometry poses.  The prior
        is transform o odom (float64, rounded to the four float32 words); the matched pose (N, 4) float32 is
        returned, `transform` is recomputed from it and the odometry, and with `update` the scan is integrated at
        it (WorldMap.update(pose=matched, first=...)).  Envs flagged `first` ((N,) bool) and envs never stepped
        get transform 0 and are not matched on this call: their map is empty."""
        wm = self.map
        env = wm.env
        if odom is None:
            raise ValueError("Localizer.step: odom is required")
        odom = wm._pose(odom)
        n = env.num_envs
        fresh = ~self._seen
        if first is not None:
            fresh = fresh | torch.as_tensor(first, device=env.device).reshape(n).bool()
        tf = torch.where(fresh.reshape(n, 1), torch.zeros_like(self._tf), self._tf)
        o = odom.to(torch.float64)
        ct, st = torch.cos(tf[:, 2]), torch.sin(tf[:, 2])
        prior = torch.stack([ct * o[:, 0] - st * o[:, 1] + tf[:, 0], st * o[:, 0] + ct * o[:, 1] + tf[:, 1],
                             ct * o[:, 2] - st * o[:, 3], st * o[:, 2] + ct * o[:, 3]], dim=1).to(torch.float32).contiguous()
        matched = wm.match(ranges=ranges, pose=prior, mask=~fresh, **self.knobs)
        m = matched.to(torch.float64)
        th = torch.atan2(m[:, 3], m[:, 2]) - torch.atan2(o[:, 3], o[:, 2])
        th = torch.atan2(torch.sin(th), torch.cos(th))
        ct, st = torch.cos(th), torch.sin(th)
        new = torch.stack([m[:, 0] - (ct * o[:, 0] - st * o[:, 1]), m[:, 1] - (st * o[:, 0] + ct * o[:, 1]), th], dim=1)
        self._tf.copy_(torch.where(fresh.reshape(n, 1), torch.zeros_like(new), new))
        self._seen.fill_(True)
        if update:
            wm.update(ranges=ranges, pose=matched, first=fresh)
        return matched

    def relocalize(self, odom: torch.Tensor, ranges: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None,
                   **knobs) -> Tuple[torch.Tensor, torch.Tensor]:
        """Recovery for the envs of `mask` ((N,) bool or uint8; None = all) whose transform is lost: the pose is
        searched on the whole map with no prior (WorldMap.relocalize(pose=None, **knobs)) and the `transform` rows
        of the envs that came back with status 1 are recomputed from it and `odom`, with step()'s float64
        formulas; every other row stays as it was, and the map is not updated.  Returns (pose (N, 4) float32 —
        the rows not searched or not found hold the plane's centre —, status (N,) int32)."""
        wm = self.map
        env = wm.env
        if odom is None:
            raise ValueError("Localizer.relocalize: odom is required")
        odom = wm._pose(odom)
        n = env.num_envs
        knobs = dict(knobs, detail=True, bounds=False)
        pose, info = wm.relocalize(ranges=ranges, pose=None, mask=mask, **knobs)[0:2]
        found = info[:, 0] == 1
        if mask is not None:
            found = found & wm._mask(mask).bool()
        o = odom.to(torch.float64)
        m = pose.to(torch.float64)
        th = torch.atan2(m[:, 3], m[:, 2]) - torch.atan2(o[:, 3], o[:, 2])
        th = torch.atan2(torch.sin(th), torch.cos(th))
        ct, st = torch.cos(th), torch.sin(th)
        new = torch.stack([m[:, 0] - (ct * o[:, 0] - st * o[:, 1]), m[:, 1] - (st * o[:, 0] + ct * o[:, 1]), th], dim=1)
        self._tf.copy_(torch.where(found.reshape(n, 1), new, self._tf))
        self._seen.copy_(self._seen | found)
        return pose, torch.where(found, torch.ones_like(info[:, 0]), torch.zeros_like(info[:, 0]))


class LidarFlow:
    """The motion flow estimated from the scan of an FFMPVec (FFMPVec.lidar_flow; include/ffmp.h
    ffmp_scan_flow): a ring of lag + 1 uint8 scan frames (lag + 1, N, G, G) — uint8
    whatever the env's obs_format — with the pose words and the episode id saved beside every frame
    (-1: the env has no frame in that slot), `updates` (N,) int32, the updates of every env since
    its restart, and the outputs: `flow` (N, 2, G, G) [vx, vy] in the env's flow dtype and `kind`
    (N, G, G) uint8 (0 no estimate, 1 static, 2 moving) or None.  An env restarts — flow 0 and kind 0
    until it has `lag` earlier frames again — when its episode id differs from the one saved at
    the last update, when its record says it has just reset, or when the last update left it out
    (mask=): the ring advances for all envs at once, so an env that skips an update loses its
    history.  The step, its frames, its lidar and its record are never written."""

    MAX_LAG = 16

    def __init__(self, env: FFMPVec, lag: int, radius: int, block: int, gate: int, min_hits: int, thickness: float,
                 range_max: float, kind: bool = True):
        lag = int(lag)
        if not 1 <= lag <= self.MAX_LAG:
            raise ValueError(f"lag must be in [1, {self.MAX_LAG}], got {lag}")
        if not env.cfg.dt > 0:
            raise ValueError("lidar_flow: dt must be > 0 (a velocity is a displacement over lag * dt)")
        self.env, self.lag = env, lag
        self.scale = float(np.float32(env.cfg.res / (lag * env.cfg.dt)))
        self.knobs = (env._fmt, self.scale, int(radius), int(block), int(gate), int(min_hits))
        self.scan_knobs = (128, float(thickness), float(range_max))
        _abi.check(env.lib.ffmp_scan_flow_check(C.byref(env._cfg_c), *self.knobs), "ffmp_scan_flow_check")
        _abi.check(env.lib.ffmp_scan_frames_check(C.byref(env._cfg_c), 1, _abi.OBS_U8F16, *self.scan_knobs, 0),
                   "ffmp_scan_frames_check")
        n, G, dev = env.num_envs, env.cfg.grid, env.device
        self._frames = torch.zeros((lag + 1, n, G, G), dtype=torch.uint8, device=dev)
        self._poses = torch.zeros((lag + 1, n, 4), dtype=torch.float32, device=dev)
        self._episodes = torch.full((lag + 1, n), -1, dtype=torch.int32, device=dev)
        self._pos = 0
        self.updates = torch.zeros(n, dtype=torch.int32, device=dev)
        self.flow = torch.zeros((n, 2, G, G), dtype=env._pot_dtype, device=dev)
        self.kind = torch.zeros((n, G, G), dtype=torch.uint8, device=dev) if kind else None

    @property
    def frame(self) -> torch.Tensor:
        """The newest (N, G, G) uint8 scan frame of the ring (lidar_frames(newest_only=True)'s bytes)."""
        return self._frames[self._pos]

    def _mask(self, mask) -> Optional[torch.Tensor]:
        if mask is None:
            return None
        return torch.as_tensor(mask, device=self.env.device).reshape(self.env.num_envs).to(torch.uint8).contiguous()

    def reset(self, mask: Optional[torch.Tensor] = None) -> None:
        """Forget the frames of the selected envs (mask: (N,) bool or uint8; None = all): flow 0, kind 0,
        and the next update restarts them."""
        if mask is None:
            self._episodes.fill_(-1)
            self.updates.zero_()
            self.flow.zero_()
            if self.kind is not None:
                self.kind.zero_()
            return
        sel = self._mask(mask).bool()
        self._episodes[:, sel] = -1
        self.updates[sel] = 0
        self.flow[sel] = 0
        if self.kind is not None:
            self.kind[sel] = 0

    def update(self, ranges: Optional[torch.Tensor] = None, pose: Optional[torch.Tensor] = None,
               first: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Build the current scan frame into the next ring slot and estimate the flow against the frame
        of `lag` updates ago: two launches on the current stream (ffmp_scan_frames, ffmp_scan_flow) and
        the small bookkeeping copies on the same stream.  Returns `flow`.
        ranges: a contiguous (N, L') float32 device tensor instead of the env's `lidar`, as in
        lidar_frames.  pose: a contiguous (N, 4) float32 device tensor {x, y, cos yaw, sin yaw}
        instead of record words 0..3 (ros_adapters.odom_to_pose_row makes a row).  first: (N,) bool,
        the envs that start anew; by default the envs whose episode id has changed since the last
        update or whose record says it has just reset — with pose= given the env's own bookkeeping
        is not looked at, and without first= no env restarts (but those never updated, left out of
        the last update or reset()).  mask: (N,) bool or uint8, envs with 0 keep their flow and kind,
        and lose their history."""
        env = self.env
        env._check_open()
        if env._needs_reset:
            raise RuntimeError("call reset() before LidarFlow.update()")
        n, G, lag = env.num_envs, env.cfg.grid, self.lag
        if ranges is None:
            if env.lidar is None:
                raise ValueError("LidarFlow.update: the env has n_beams == 0, pass ranges=")
            ranges = env.lidar
        elif not isinstance(ranges, torch.Tensor) or ranges.dim() != 2 or ranges.shape[0] != n or ranges.dtype != torch.float32 \
                or not ranges.is_contiguous() or ranges.device != env.device:
            raise ValueError(f"ranges must be a contiguous float32 tensor of shape ({n}, L) on {env.device}")
        last = self._episodes[self._pos]
        if pose is None:
            pose = env.record
            episode = env.episode
            if first is None:
                first = (episode != last) | (env.record[:, 10] != 0)
        else:
            if not isinstance(pose, torch.Tensor) or tuple(pose.shape) != (n, 4) or pose.dtype != torch.float32 \
                    or not pose.is_contiguous() or pose.device != env.device:
                raise ValueError(f"pose must be a contiguous float32 tensor of shape ({n}, 4) on {env.device}")
            episode = torch.zeros_like(last)
        never = last < 0
        restart = never if first is None else torch.as_tensor(first, device=env.device).reshape(n).bool() | never
        mask = self._mask(mask)
        sel = None if mask is None else mask.bool()
        if sel is not None:
            restart = restart & sel
        self._episodes.masked_fill_(restart.unsqueeze(0), -1)
        slot = (self._pos + 1) % (lag + 1)
        old = (slot + 1) % (lag + 1)  # the slot of `lag` updates ago
        G2 = G * G
        env._scan_launch(ranges, None, self._frames[slot].data_ptr(), G2, _abi.OBS_U8F16, *self.scan_knobs, mask)
        self._episodes[slot] = episode if sel is None else torch.where(sel, episode, torch.full_like(episode, -1))
        kfirst = self._episodes[old] != self._episodes[slot]  # bool: one byte per env
        with torch.cuda.device(env.device):
            _abi.check(env.lib.ffmp_scan_flow(C.byref(env._cfg_c), n, self._frames[slot].data_ptr(), self._frames[old].data_ptr(),
                                              G2, pose.data_ptr(), pose.stride(0), self._poses[old].data_ptr(), 4, _ptr(mask),
                                              kfirst.data_ptr(), self.flow.data_ptr(), 2 * G2, _ptr(self.kind), G2,
                                              *self.knobs, env._stream()), "ffmp_scan_flow")
        self._poses[slot] = pose[:, 0:4]
        one = torch.ones_like(self.updates)
        nxt = torch.where(restart, one, self.updates + 1)
        self.updates.copy_(nxt if sel is None else torch.where(sel, nxt, self.updates))
        self._pos = slot
        return self.flow

    def bev_image(self, occ: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The 4-channel [occupancy, R, G, B] image (include/ffmp.h ffmp_bev_image) with the estimated
        flow in place of obs["flow"]: (N, 4, G, G) in the env's frame dtype, vmax = cfg.obst_vmax —
        the reference's 12-channel input from sensor data alone, a ring of these images going
        through temporal_maps as the ground-truth ones do.  occ: a contiguous (N, G, G) device tensor
        in the env's frame dtype; by default the newest scan frame of the ring.  out: write into
        this contiguous tensor instead of a new one."""
        env = self.env
        env._check_open()
        n, G = env.num_envs, env.cfg.grid
        G2 = G * G
        if occ is None:
            occ = self.frame if env._frame_dtype == torch.uint8 else self.frame.to(env._frame_dtype)
        elif not isinstance(occ, torch.Tensor) or tuple(occ.shape) != (n, G, G) or occ.dtype != env._frame_dtype \
                or not occ.is_contiguous() or occ.device != env.device:
            raise ValueError(f"occ must be a contiguous {env._frame_dtype} tensor of shape ({n}, {G}, {G}) on {env.device}")
        shape = (n, 4, G, G)
        if out is None:
            out = torch.empty(shape, dtype=env._frame_dtype, device=env.device)
        elif tuple(out.shape) != shape or out.dtype != env._frame_dtype or not out.is_contiguous() or out.device != env.device:
            raise ValueError(f"out must be a contiguous {env._frame_dtype} tensor of shape {shape} on {env.device}")
        with torch.cuda.device(env.device):
            _abi.check(env.lib.ffmp_bev_image(n, 1 if env.obs_format == "u8f16" else 0, occ.data_ptr(), G2, self.flow.data_ptr(), G2,
                                              float(np.float32(env.cfg.obst_vmax)), out.data_ptr(), 4 * G2, env._stream()),
                       "ffmp_bev_image")
        return out


class StepGraph:
    """`steps` consecutive FFMPVec steps captured as one HIP graph (FFMPVec.capture).

    The env kernel + raster (or the one-launch step) of each step are recorded with the frame-ring
    slots that step writes; when `steps` is a multiple of graph_period() the ring is back on its
    starting slots after a replay and the same graph is valid for the next one (other counts replay
    whenever the frame position is back where the capture started).  replay(actions)
    copies the (steps, N) action block into the graph's static block (one device copy), replays,
    then advances the env's host-side frame bookkeeping exactly as `steps` calls of step() would.
    Results are those of `steps` step() calls with the same actions, bit for bit
    (tests/test_gpu_graph.py).  Not with pipeline slices or a BEV image ring (their launches need
    per-step host work), and the env must not be stepped or reset between capture and replay except
    through whole replays or whole periods of step() calls (checked: the frame position).

    The graph holds the env's config struct (the seed that keys the auto-reset RNG included) by
    value.  A config change after the capture — reset(seed=s), seed(s) or load_state_dict() of a
    checkpoint with another seed — makes replay() raise RuntimeError: capture again (it is not done
    silently).  What does not change the config leaves the graph valid: reset(), reset(seed=<the
    same seed>), reset(mask=), set_scenarios(), raster(), invalidate_frame_tags(), a load_state_dict()
    with the same seed (all at the capture's frame position), and launch shapes or tuning changed
    later (the captured launches keep theirs; the results are the same bits).
    (tests/test_gpu_graph_state.py.)

    Pipelined (two-launch steps, an even step count): the raster of step i reads only the record
    its env kernel wrote, and the env kernel reads none of the raster's outputs, so with two record
    buffers — step i's env kernel writes buffer (i + 1) % 2, the current record being buffer 0 —
    the env kernel of step i + 1 runs on a second stream beside the raster of step i, waiting only
    for the raster of step i - 1 (the last reader of its buffer).  The graph's intermediate steps'
    small outputs (reward, done, state_g, ...) are overwritten one step early, which nobody sees: a
    replay's observation is its last step's, written in the same order as step() writes it, and the
    frames, potential and record are bit-identical (tests/test_gpu_graph.py).

    Skewed (the default where skew_supported() and the one-off trial in _skew_pays() say it pays):
    the same two record buffers, but the raster of step i and the env kernel of step i + 1 are ONE
    launch (ffmp_step_skewed: env blocks first, raster blocks after), so a k-step replay is k + 1
    dispatches on one stream instead of 2k and no env kernel waits on a raster tail.  Same results,
    bit for bit (tests/test_gpu_graph.py, tests/timed_path_check.py)."""

    # Off by default: the overlap happens (rocprofv3 trace, profiles/r05n_pipelined_graph.txt) but the
    # raster beside an env kernel runs ~12 % longer and the graph leaves ~10 us between two rasters on
    # different queues — C2 38.5-38.7 vs 38.9-39.2 M serial, C3 14.01-14.03 vs 13.88-14.03 M
    # (profiles/r05m_pipelined_graph.txt).  FFMP_GRAPH_PIPELINE=1 makes it the default.
    PIPELINE_DEFAULT = os.environ.get("FFMP_GRAPH_PIPELINE", "0") == "1"
    SKEW_DEFAULT = os.environ.get("FFMP_GRAPH_SKEW", "1") != "0"  # A/B knob

    @staticmethod
    def skew_supported(env: FFMPVec, k: int) -> bool:
        """Does ffmp_step_skewed take this instance's steps?  The library answers
        (ffmp_step_skewed_check: float32 frames, no flow planes, its env waves' LDS against the
        device's limit) for both raster shapes the graph uses; the two-launch step and an even k."""
        if env.fused or k % 2 or env.obs_format != "f32" or env.flow is not None:
            return False
        return all(env.lib.ffmp_step_skewed_check(C.byref(env._cfg_c), env._fmt, flags) == 0
                   for flags in {env.raster_shape[1], env.raster_shape_newest[1]})

    @staticmethod
    def _skew_pays(env: FFMPVec) -> bool:
        """The default: skew while the env step's blocks (4 waves each) fit the CUs once — they are
        dispatched first, and more of them delay the raster's stores (C2's 128 blocks: 39.6 -> 41.2 M
        env-steps/s; C3's 2,048: 14.0 -> 13.9 M; profiles/r05r_skewed_graph.txt).  bench.py times both."""
        K = env.cfg.n_obst
        lpe = 8 if K <= 8 else 16 if K <= 16 else 32 if K <= 32 else 64
        blocks = -(-env.num_envs // (4 * (64 // lpe)))
        return blocks <= torch.cuda.get_device_properties(env.device).multi_processor_count

    def __init__(self, env: FFMPVec, steps: Optional[int] = None, pipelined: Optional[bool] = None,
                 skewed: Optional[bool] = None, policy=None, commands: bool = False):
        env._check_open()
        if policy is not None:
            if pipelined or skewed:
                raise ValueError("a closed-loop graph (policy) runs plain steps: the policy reads each raster's frame")
            if policy not in ("reactive", "field", "nav") and not callable(policy):
                raise ValueError("policy must be 'reactive', 'field', 'nav' or a callable env -> (N,) int64 tensor")
            pipelined = skewed = False
        # (v, w) commands instead of ids: the field follower's closed loop, or an open loop (commands=True)
        self.commands = bool(commands) or policy in ("field", "nav")
        if self.commands:
            if callable(policy):
                raise ValueError("commands=True takes policy='field', 'nav' or no policy (a callable policy returns ids)")
            if policy == "reactive":
                raise ValueError("policy='reactive' computes action ids, not commands")
            if pipelined or skewed:
                raise ValueError("a command graph runs plain steps: the pipelined and skewed forms read action ids")
            pipelined = skewed = False
        self.policy = policy
        if env._needs_reset:
            raise RuntimeError("call reset() before capture()")
        if env.pipeline_slices > 1 or env.bev is not None:
            raise ValueError("capture() needs pipeline=1 and no bev_series")
        per = env.graph_period()
        k = per if steps is None else int(steps)
        if k <= 0:
            raise ValueError("steps must be positive")
        # a multiple of the period ends on the slots it started from, so it replays back to back;
        # any other count is replayable once the frame position is back at the capture's
        self.chainable = k % per == 0
        self.env, self.steps = env, k
        # the static block the captured steps read: ids (k, N) int64, or commands (k, N, 2) float64
        self.actions = torch.zeros((k, env.num_envs, 2), dtype=torch.float64, device=env.device) if self.commands \
            else torch.zeros((k, env.num_envs), dtype=torch.int64, device=env.device)
        can_pipe = not env.fused and k % 2 == 0
        if pipelined is None:
            pipelined = can_pipe and self.PIPELINE_DEFAULT
        if pipelined and not can_pipe:
            raise ValueError("a pipelined graph needs the two-launch step and an even step count")
        self.pipelined = bool(pipelined)
        can_skew = not self.pipelined and self.skew_supported(env, k)
        if skewed is None:
            skewed = can_skew and self.SKEW_DEFAULT and self._skew_pays(env)
        if skewed and not can_skew:
            raise ValueError("a skewed graph needs the two-launch step, an even step count, float32 frames "
                             "without flow planes, and no pipelining")
        self.skewed = bool(skewed)
        snap = (env._wpos, list(env._hist), env._hist_from_reset)
        self.wpos = env._wpos
        self.cfg_gen = env._cfg_gen  # the launches below hold this generation's config struct by value
        self.graph = torch.cuda.CUDAGraph()
        stream = torch.cuda.Stream(device=env.device)
        if policy == "nav" and env._nav_tiled(None) is not None:
            env._nav_workspace(env._nav_tiled(None), False)  # allocated before the capture: the graph holds its pointer
        torch.cuda.synchronize(env.device)
        rec0 = env.record
        if self.pipelined or self.skewed:
            if getattr(env, "_record_alt", None) is None or env._record_alt.shape != rec0.shape:
                env._record_alt = torch.empty_like(rec0)
            bufs = (rec0, env._record_alt)
        if self.pipelined:
            self._side = torch.cuda.Stream(device=env.device)
        try:
            with torch.cuda.device(env.device), torch.cuda.graph(self.graph, stream=stream):
                if self.pipelined:
                    self._capture_pipelined(k, bufs)
                elif self.skewed:
                    self._capture_skewed(k, bufs)
                else:
                    for i in range(k):
                        if policy is not None:
                            self._act(i)
                        if env.fused:
                            env._step_fused(self.actions[i])
                        else:
                            env.step_state(self.actions[i])
                            env.raster_step()
        finally:
            env.record = rec0
            env._state_c.record = rec0.data_ptr()
            # nothing ran: the host bookkeeping goes back to where the GPU state is
            env._set_window(snap[0])
            env._hist, env._hist_from_reset = snap[1], snap[2]
        if env._wpos != self.wpos:
            raise RuntimeError("frame position changed during capture")

    def _act(self, i: int) -> None:
        """Closed loop: step i's actions from the current observation, into the static block."""
        if self.policy == "reactive":
            self.env.policy_reactive(out=self.actions[i])
        elif self.policy == "field":
            self.env.policy_field(out=self.actions[i])
        elif self.policy == "nav":
            self.env.policy_nav(out=self.actions[i])
        else:
            a = self.policy(self.env)
            if not (isinstance(a, torch.Tensor) and a.numel() == self.env.num_envs):
                raise ValueError("policy must return an (N,) tensor of action ids")
            self.actions[i].copy_(a.reshape(-1))

    def _capture_pipelined(self, k: int, bufs) -> None:
        env, side = self.env, self._side
        cap = torch.cuda.current_stream(env.device)
        fork = torch.cuda.Event()
        fork.record(cap)
        side.wait_event(fork)
        ev_env = [torch.cuda.Event() for _ in range(k)]
        ev_ras = [torch.cuda.Event() for _ in range(k)]
        for i in range(k):
            buf = bufs[(i + 1) % 2]  # k even: the last step writes buffer 0, the current record
            env.record = buf
            env._state_c.record = buf.data_ptr()
            with torch.cuda.stream(side):
                if i >= 2:
                    side.wait_event(ev_ras[i - 2])  # the last raster that read this buffer
                env.step_state(self.actions[i])
                ev_env[i].record(side)
            cap.wait_event(ev_env[i])
            env.raster_step()
            ev_ras[i].record(cap)
        # the side stream's last work (env kernel k - 1) is joined by the last raster's wait

    def _capture_skewed(self, k: int, bufs) -> None:
        """env(0); then for i < k - 1 ONE launch of raster(i) + env(i + 1); then raster(k - 1).  env(i)
        writes record buffer (i + 1) % 2, raster(i) reads it (k even: the last is buffer 0)."""
        env = self.env
        env.record = bufs[1]
        env._state_c.record = bufs[1].data_ptr()
        env.step_state(self.actions[0])
        for i in range(k - 1):
            full = env._next_window()
            cpb, flags = env.raster_shape if full else env.raster_shape_newest
            flags |= 0 if full else _abi.RASTER_NEWEST
            rec_r, rec_w = bufs[(i + 1) % 2], bufs[(i + 2) % 2]
            env.record = rec_w
            env._state_c.record = rec_w.data_ptr()
            _abi.check(env.lib.ffmp_step_skewed(C.byref(env._cfg_c), env.num_envs, env.env_offset,
                                                self.actions[i + 1].data_ptr(), C.byref(env._state_c),
                                                C.byref(env._obs_c), C.byref(env._out_c), rec_r.data_ptr(), cpb,
                                                flags, env._stream()), "ffmp_step_skewed")
        env.record = bufs[0]
        env._state_c.record = bufs[0].data_ptr()
        env.raster_step()

    def replay(self, actions: Optional[torch.Tensor] = None) -> None:
        """Run the captured steps; actions (steps, N) int64 — or, for a commands=True graph,
        (steps, N, 2) float32 / float64 (v, w) commands — (None: the block the last replay used)."""
        env = self.env
        env._check_open()
        if env._needs_reset:
            raise RuntimeError("call reset() before replay()")
        if env._cfg_gen != self.cfg_gen:
            raise RuntimeError("the env's config changed since capture (a new seed through reset(seed=), seed() or "
                               "load_state_dict()): the graph holds the old one and has to be captured again "
                               "(env.capture())")
        if env._wpos != self.wpos:
            raise RuntimeError("the env's frame position moved since capture (step() a whole graph_period())")
        if actions is not None:
            if self.policy is not None:
                raise ValueError("a closed-loop graph computes its own actions (replay() takes none)")
            a = torch.as_tensor(actions)
            if a.shape != self.actions.shape:
                raise ValueError(f"actions must have shape {tuple(self.actions.shape)}")
            if self.commands and a.dtype not in (torch.float32, torch.float64):
                raise ValueError(f"commands must be float32 or float64, got {a.dtype}")
            self.actions.copy_(a, non_blocking=True)
        with torch.cuda.device(env.device):
            self.graph.replay()
        for _ in range(self.steps):  # the host side of each step (frame pair, history), no launch
            env._next_window()
