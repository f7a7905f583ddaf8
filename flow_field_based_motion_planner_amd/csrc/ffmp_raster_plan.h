// ffmp_raster_plan.h — how a raster is launched, decided once.  raster_plan() turns (cfg, obs, cells per
// block, FFMP_RASTER_* flags, n) into a RasterPlan or refuses them; ffmp_raster_ex, the one-launch step and
// the skewed step launch what it says, and ffmp_raster_waves / ffmp_raster_direct / ffmp_step_skewed_check
// report it.  Host only and pure: no HIP call, no access through a pointer of the batch (only the
// ffmp_obs_t header and its tag extension are read), so a host program can include it without the kernels.
#pragma once
#include "ffmp.h"

namespace ffmp {

// Observation format of a raster instantiation: FMT_F32 (reference layout), FMT_CT4 (compact
// FFMP_OBS_U8F16, 4 cells per lane) or FMT_CT16 (compact, 16 cells per lane: a wave task is
// 1024 cells, so the per-task cull / wall / index work is spread over 4x the cells — the compact
// raster writes 3 bytes per cell and is bound by that per-task work, not by HBM; needs G % 16 == 0).
// FMT_CT8 (FFMP_RASTER_MID8, G % 8 == 0): 8 cells per lane, an 8-B frame store and a 16-B potential
// store per lane (512-cell wave tasks).
constexpr int FMT_F32 = 0, FMT_CT4 = 1, FMT_CT16 = 2, FMT_CT8 = 3;
constexpr int kTagLdsCap = 1024;       // granules of one slot a block stages (a whole 256 x 256 plane)
constexpr int kRasterWaves = 6;        // FFMP_RASTER_WAVES: waves per SIMD of the tagged float32 kernels

// Who launches: ffmp_raster_ex (every form), the one-launch step (a block is one whole plane, whatever
// cells_per_block says; no direct form) or the skewed step (float32 frames without flow planes only; neither
// FFMP_RASTER_WAVES nor FFMP_RASTER_DIRECT).
enum class RasterUse { kTwoLaunch, kOneLaunch, kSkewed };

// How a refusal is reported: ffmp_detail::fail (sets ffmp_last_error(), returns the code), handed in so that
// this header needs no other.  GCC checks the format strings below through the attribute, clang does not
// through a pointer: tests/test_raster_plan_host.py pins every text.
typedef int (*RefuseFn)(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

// The granule tags behind an ffmp_obs_t with FFMP_OBS_EXT_TAGS (include/ffmp.h ffmp_obs_tags_t), env 0.
struct RasterTags {
  uint8_t* older;
  uint8_t* newest;
  int64_t env_stride;
};

struct RasterPlan {
  int fmt;                      // FMT_*
  bool ct, flow, tagged;        // compact planes; flow planes; granule tags
  RasterTags tags;              // tagged only
  bool nt, xcd;                 // nontemporal stores; each XCD walks its own block range
  int32_t newest;               // 1: only the newest frame is written
  int cpb, bpe;                 // cells per block, blocks per env
  int32_t tile_log2r;           // log2 of the rows of a 2-D wave tile, 0 = 1-D chunks
  int waves;                    // kRasterWaves: the tagged float32 kernel held to that many waves per SIMD, else 0
  bool direct;                  // ffmp_raster_ex launches raster_direct_kernel
  int64_t sm_stride, sm_frame;  // state_m strides in elements, defaults filled in (n > 0 only)
};

// log2 of the rows of a 2-D wave tile (FFMP_RASTER_TILE*), 0 = 1-D chunks
inline int32_t tile_rows_log2(int32_t flags) {
  return (flags & FFMP_RASTER_TILE16) ? 4 : (flags & FFMP_RASTER_TILE8) ? 3 : (flags & FFMP_RASTER_TILE4) ? 2
       : (flags & FFMP_RASTER_TILE2) ? 1 : 0;
}

// The raster instantiation for an obs format: compact planes use 16 cells per lane when every
// lane's 16 cells stay in one row (G % 16 == 0) unless FFMP_RASTER_NARROW asks for 4.
inline int raster_format(bool compact, int grid, int32_t flags) {
  if (!compact) return FMT_F32;
  if (flags & FFMP_RASTER_NARROW) return FMT_CT4;
  if ((flags & FFMP_RASTER_MID8) && grid % 8 == 0) return FMT_CT8;
  return grid % 16 == 0 ? FMT_CT16 : FMT_CT4;
}

// FFMP_RASTER_WAVES -> the W of the tagged float32 kernel to launch (0: the plain one).  Without tags, in
// the compact format or with flow planes the flag is ignored.
inline int raster_waves(int32_t flags, bool tagged, bool ct, bool flow) {
  if (!tagged || ct || flow) return 0;
  return (flags & FFMP_RASTER_WAVES) ? kRasterWaves : 0;
}

// FFMP_RASTER_DIRECT -> does ffmp_raster_ex launch raster_direct_kernel?  Where FFMP_RASTER_WAVES would select
// the tagged float32 kernel (tags, float32 frames, no flow planes), for row runs and 2- / 4-row tiles in the
// column-band-major deal (tile_log2r as the launch settled it), in blocks whose old tags the staged form
// would stage too.  Elsewhere the flag is ignored.
inline bool raster_direct(int32_t flags, bool tagged, bool ct, bool flow, int grid, int cpb, int32_t tile_log2r) {
  if (!(flags & FFMP_RASTER_DIRECT) || !tagged || ct || flow || tile_log2r > 2) return false;
  const int G2 = grid * grid;
  if (((cpb < G2 ? cpb : G2) + 63) / 64 > kTagLdsCap) return false;
  if (tile_log2r == 0) return true;
  const int ncb = grid / (256 >> tile_log2r);
  return ncb > 0 && ((4 % ncb) == 0 || (ncb % 4) == 0);
}

// The launch shape: cells per block (cells_per_block 0: 4096; a plane below one block: the plane, rounded up
// to 1024), and the 2-D wave tiles (R rows x (cells per wave task)/R columns) where the
// plane and the block split into them, else 0: the 1-D chunks (identical results).
inline void raster_shape(int grid, int32_t cells_per_block, int fmt, int32_t flags, int* cpb_out, int32_t* tile_log2r_out) {
  const int G2 = grid * grid;
  const int cpb_max = cells_per_block ? cells_per_block : 4096;
  const int cpb = G2 < cpb_max ? ((G2 + 1023) / 1024) * 1024 : cpb_max;
  int32_t tile_log2r = tile_rows_log2(flags);
  if (tile_log2r) {
    const int C = (fmt == FMT_CT16 ? 1024 : fmt == FMT_CT8 ? 512 : 256) >> tile_log2r, R = 1 << tile_log2r;
    const bool whole_bands = cpb >= G2 || (cpb % (grid * R)) == 0;
    if ((grid % C) != 0 || !whole_bands) tile_log2r = 0;
  }
  *cpb_out = cpb;
  *tile_log2r_out = tile_log2r;
}

// The plan's tag step: p->tagged and p->tags from obs (checked; tagged = false without FFMP_OBS_EXT_TAGS).
inline int plan_tags(const ffmp_cfg_t* cfg, const ffmp_obs_t* o, RasterPlan* p, RefuseFn fail) {
  p->tagged = (o->reserved & FFMP_OBS_EXT_TAGS) != 0;
  if (!p->tagged) return FFMP_OK;
  const ffmp_obs_tags_t* x = reinterpret_cast<const ffmp_obs_tags_t*>(o);
  if (o->format != FFMP_OBS_F32)
    return fail(FFMP_E_ARG, "FFMP_OBS_EXT_TAGS: granule tags need format FFMP_OBS_F32, got %d", o->format);
  if (!x->tags_older || !x->tags_newest) return fail(FFMP_E_ARG, "FFMP_OBS_EXT_TAGS: tags_older / tags_newest is NULL");
  const int64_t T = ((int64_t)cfg->grid * cfg->grid + FFMP_TAG_CELLS - 1) / FFMP_TAG_CELLS;
  if (x->tags_env_stride < T)
    return fail(FFMP_E_ARG, "FFMP_OBS_EXT_TAGS: tags_env_stride %lld < %lld tags per frame",
                (long long)x->tags_env_stride, (long long)T);
  p->tags = RasterTags{x->tags_older, x->tags_newest, x->tags_env_stride};
  return FFMP_OK;
}

// Fills *p for a raster of n envs of a checked cfg into obs, or refuses the arguments.  cells_per_block: 0
// (4096) or a multiple of 1024.  n == 0: everything but the strides, which are not checked (nothing is
// written).
inline int raster_plan(RasterUse use, const ffmp_cfg_t* cfg, const ffmp_obs_t* obs, int32_t cells_per_block,
                       int32_t flags, int64_t n, RasterPlan* p, RefuseFn fail) {
  const int G2 = cfg->grid * cfg->grid;
  const bool two = use == RasterUse::kTwoLaunch, skewed = use == RasterUse::kSkewed;
  if (use == RasterUse::kOneLaunch) cells_per_block = ((G2 + 1023) / 1024) * 1024;
  if (cells_per_block != 0 && (cells_per_block < 1024 || cells_per_block % 1024 != 0))
    return fail(FFMP_E_ARG, "cells_per_block must be 0 or a multiple of 1024, got %d", cells_per_block);
  if ((flags & FFMP_RASTER_NT) && (flags & FFMP_RASTER_PLAIN)) return fail(FFMP_E_ARG, "NT and PLAIN both set");
  if (obs->format != FFMP_OBS_F32 && obs->format != FFMP_OBS_U8F16)
    return fail(FFMP_E_ARG, "unknown obs.format %d", obs->format);
  p->ct = obs->format == FFMP_OBS_U8F16;
  p->flow = cfg->flow != 0;
  if (skewed && (p->ct || p->flow)) return fail(FFMP_E_ARG, "ffmp_step_skewed: float32 frames without flow planes only");
  if (int rc = plan_tags(cfg, obs, p, fail)) return rc;
  p->fmt = raster_format(p->ct, cfg->grid, flags);
  raster_shape(cfg->grid, cells_per_block, p->fmt, flags, &p->cpb, &p->tile_log2r);
  p->bpe = (G2 + p->cpb - 1) / p->cpb;
  p->nt = (flags & FFMP_RASTER_NT) ? true : (flags & FFMP_RASTER_PLAIN) ? false : (G2 <= 16384);
  p->xcd = (flags & FFMP_RASTER_XCD) != 0;
  p->newest = (flags & FFMP_RASTER_NEWEST) ? 1 : 0;
  p->waves = skewed ? 0 : raster_waves(flags, p->tagged, p->ct, p->flow);
  p->direct = two && raster_direct(flags, p->tagged, p->ct, p->flow, cfg->grid, p->cpb, p->tile_log2r);
  if (n == 0) return FFMP_OK;
  p->sm_stride = obs->state_m_stride ? obs->state_m_stride : 2 * (int64_t)G2;
  p->sm_frame = obs->state_m_frame_stride ? obs->state_m_frame_stride : (int64_t)G2;
  const int64_t sm_frame_abs = p->sm_frame < 0 ? -p->sm_frame : p->sm_frame;  // negative: newest in a lower slot
  if (p->sm_stride < (int64_t)G2 || sm_frame_abs < (int64_t)G2 ||
      (p->sm_stride < 2 * (int64_t)G2 && sm_frame_abs < n * (int64_t)G2))
    return fail(FFMP_E_ARG, "state_m strides overlap: env %lld, frame %lld elements (G*G = %d)",
                (long long)p->sm_stride, (long long)p->sm_frame, G2);
  return FFMP_OK;
}

}  // namespace ffmp
