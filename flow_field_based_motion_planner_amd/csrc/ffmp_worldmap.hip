// ffmp_worldmap.hip — the world-fixed lidar map: one int8 log-odds cell per world cell, integrated from
// the scan and the pose in place, and its ego view (include/ffmp.h ffmp_world_map / ffmp_world_frame carry
// the SPEC).
//
// world_map_kernel.  The class of a cell that the scan does not reach is "not known" and leaves the cell as
// it is, so an env's blocks visit only a box around the sensor disc: rows p0 .. p0 + h - 1, columns
// q0 .. q0 + 4 w4 - 1 (q0 a multiple of 4), clipped to the plane.  The box is linearised in groups of 4
// cells, group g = row g / w4, columns 4 (g % w4) ..: a lane owns one group per pass (one 32-bit load, one
// 32-bit store of its own bytes), a wave 64 consecutive groups — 256 consecutive bytes of a row, or the
// tail of one row and the head of the next — and the env's bpe blocks stride over the box together.  No
// cell is touched by two lanes, so there is no LDS traffic beyond the staged scan, and one barrier (after
// the staging).  An env that restarts (first[e] != 0) takes the whole plane as its region: groups outside
// the box store zeros, groups inside it update a prior of 0 — the lanes that zero are the lanes that update.
// The grid is sized for the box of a unit (c, s) at range_max; a pose whose (c, s) is shorter than a unit
// vector only makes the box larger than that, and the stride loop covers it.
//
// The box is a superset of every cell the SPEC can call known.  known needs b = ex*ex + ey*ey <= mm in
// float32, where (ex, ey) is (dx, dy) turned and scaled by (c, s): b >= |cs|^2 d^2 (1 - 2^-19) for the float32
// d = |(dx, dy)|, mm <= rm^2 (1 + 2^-23), and the float32 cell centre differs from p res_f - wh_f by less
// than 2^-22 Wc res.  So a known cell has |p res_f - wh_f - px| <= (rm / |cs|)(1 + 1e-5) + res in exact
// arithmetic, which the box (float64, rounded outwards by a further cell) contains.  A range_max whose
// float32 square overflows is the exception: mm = +inf admits every cell, a b of +inf included, so the
// region is then the whole plane, as for range_max = +inf.
//
// The per-cell search is ffmp_scan.hip's, restated (that file's kernels keep their code objects): the
// SPEC's bisection for a lane's first cell, and for the second to fourth the predicate at the previous
// cell's cone and its neighbours inside the cell's own half-turn, bisecting when none of the three has it.
// The proof at the head of ffmp_scan.hip does not use where the cells lie, only that (ex, ey) is the
// point the predicate is evaluated at, so it holds for the rotated coordinates here.
//
// world_frame_kernel: one byte gathered per ego cell, 4 consecutive cells of an ego row per lane (1,024
// consecutive cells per block of 256 threads, no loop, no LDS, no barrier), one 16-byte (float32) or 4-byte
// (uint8) store per lane.  The stores are whole lines; the loads are not: a wave's 256 consecutive ego cells
// lie on a line through the plane at the env's yaw, so one byte-load instruction touches up to 64 different
// rows of it.  Measured at C3 float32: 8.14 ms, against ffmp_scan_map's 6.29 in the same run, whose gather
// turns by the motion of one step only.  scan_kernel's shape (blocks of 16,384 cells, wave tasks of 4 x 64
// tiles) was measured too and is no faster, 8.38 ms: it is not the 2 M small workgroups.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "ffmp_device.h"
#include "ffmp_host.h"

#pragma clang fp contract(off)

namespace {

using namespace ffmp;

constexpr int kWmThreads = 256;
constexpr int kWmBlockCells = 8192;  // cells of the largest box per block: 8 groups per lane
constexpr int kWfBlockCells = 1024;  // ego cells per block of the view: one group of 4 per lane

struct WorldMapArgs {
  const float* ranges;
  int64_t ranges_stride;  // floats
  const float* sectors;   // (L, 2)
  const float* pose;      // {px, py, cos yaw, sin yaw} per env
  int64_t pose_stride;
  const uint8_t* mask;    // or NULL
  const uint8_t* first;   // or NULL
  int8_t* map;
  int64_t map_stride;     // bytes
  int32_t L, bpe, Wc, plain;
  float th, rm, mm, wh;   // thickness, range_max, range_max^2, the world coordinate of cell 0 negated
  int32_t l_hit, l_free, l_max, decay;
};

typedef float wm_f32x4 __attribute__((ext_vector_type(4)));

// q / d for 0 <= q < 2^24, 1 <= d: the float quotient is within one of it
FFMP_DEV int wm_div(int q, int d, float invd) {
  int i = (int)((float)q * invd);
  if (i * d > q) --i;
  if ((i + 1) * d <= q) ++i;
  return i;
}

FFMP_DEV float wm_cross(float2 u, float ex, float ey) { return u.x * ey - u.y * ex; }

FFMP_DEV int wm_search(const float2* s_u, int lo, int hi, float ex, float ey) {
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (wm_cross(s_u[mid], ex, ey) >= 0.0f) lo = mid; else hi = mid;
  }
  return lo;
}

// the bisection's predicate at m with the ends of the half-turn standing for true and false (the read is
// clamped into the table, its value then unused)
FFMP_DEV bool wm_pred(const float2* s_u, int m, int LO, int HI, int L, float ex, float ey) {
  const float t = wm_cross(s_u[min(max(m, 0), L - 1)], ex, ey);
  return (m <= LO) | ((m < HI) & (t >= 0.0f));
}

FFMP_DEV bool wm_finite(float v) { return v - v == 0.0f; }

// [lo, hi] of the cell indices within `reach` of centre `at`, clipped to 0 .. Wc - 1 (lo > hi: none)
FFMP_DEV void wm_span(double at, double reach, double wh, double res, int Wc, int* lo, int* hi) {
  double a = floor((at - reach + wh) / res) - 1.0, b = ceil((at + reach + wh) / res) + 1.0;
  if (!(a >= 0.0)) a = 0.0;  // a NaN (inf - inf) takes the whole plane
  if (!(b <= (double)(Wc - 1))) b = (double)(Wc - 1);
  if (a > (double)Wc) a = (double)Wc;
  if (b < -1.0) b = -1.0;
  *lo = (int)a;
  *hi = (int)b;
}

__global__ __launch_bounds__(kWmThreads) void world_map_kernel(ffmp_cfg_t cfg, WorldMapArgs a) {
  __shared__ float2 s_u[FFMP_MAX_BEAMS];
  __shared__ float s_r[FFMP_MAX_BEAMS];

  const int L = a.L, Wc = a.Wc;
  const int tid = threadIdx.x;
  const uint32_t lb = blockIdx.x, bpe = (uint32_t)a.bpe;  // 32-bit division: the grid has < 2^31 blocks
  const int64_t e = lb / bpe;
  const int tile = (int)(lb - (uint32_t)e * bpe);
  if (a.mask && a.mask[e] == 0) return;  // block-uniform, as everything up to the loop
  const bool restart = a.first && a.first[e] != 0;
  const float* ps = a.pose + e * a.pose_stride;
  const float px = ps[0], py = ps[1], pc = ps[2], psn = ps[3];
  const bool finite = wm_finite(px) && wm_finite(py) && wm_finite(pc) && wm_finite(psn);
  if (!finite && !restart) return;

  // the box of the sensor disc (see the head of the file)
  int p0 = 0, p1 = -1, q0 = 0, q1 = -1;
  if (finite) {
    const double nrm = sqrt((double)pc * (double)pc + (double)psn * (double)psn);
    // nrm == 0 or rm = inf: +inf; and a range_max whose float32 square overflows admits every cell, b = +inf included
    const double rm = a.mm > 3.0e38f ? __builtin_inf() : (double)a.rm;
    const double reach = (rm / nrm) * (1.0 + 1e-5) + (double)cfg.res_f;
    wm_span((double)px, reach, (double)a.wh, (double)cfg.res_f, Wc, &p0, &p1);
    wm_span((double)py, reach, (double)a.wh, (double)cfg.res_f, Wc, &q0, &q1);
    q0 &= ~3;
    q1 |= 3;  // Wc % 4 == 0: still <= Wc - 1
  }
  const bool empty = p1 < p0 || q1 < q0;
  if (empty && !restart) return;
  // the region this env's blocks cover: the box, or the whole plane for an env that restarts
  const int r_p0 = restart ? 0 : p0, r_q0 = restart ? 0 : q0;
  const int r_h = restart ? Wc : p1 - p0 + 1, r_w4 = restart ? (Wc >> 2) : ((q1 - q0 + 1) >> 2);
  const int total = r_h * r_w4;  // <= 2^20 groups

  if (!empty) {
    const float* rg = a.ranges + e * a.ranges_stride;
    for (int l = tid; l < L; l += kWmThreads) {
      s_u[l] = make_float2(a.sectors[2 * l], a.sectors[2 * l + 1]);
      s_r[l] = rg[l];
    }
  }
  __syncthreads();

  const int H = (L + 1) >> 1;
  const float2 u0 = s_u[0];
  const bool plain = a.plain != 0;
  const float inv_w4 = 1.0f / (float)r_w4;
  int8_t* mp = a.map + e * a.map_stride;

  for (int g = tile * kWmThreads + tid; g < total; g += (int)bpe * kWmThreads) {
    const int row = wm_div(g, r_w4, inv_w4);
    const int p = r_p0 + row, q = r_q0 + 4 * (g - row * r_w4);
    uint32_t* cell = reinterpret_cast<uint32_t*>(mp + (int64_t)p * Wc + q);
    const bool inbox = !empty && p >= p0 && p <= p1 && q >= q0 && q <= q1;
    if (!inbox) {  // only in a restarting env
      *cell = 0u;
      continue;
    }
    const uint32_t old = restart ? 0u : *cell;
    const float wx = (float)p * cfg.res_f - a.wh;
    const float dx = wx - px;
    uint32_t out = 0;
    int lo = 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float wy = (float)(q + u) * cfg.res_f - a.wh;
      const float dy = wy - py;
      const float ex = pc * dx + psn * dy;
      const float ey = pc * dy - psn * dx;
      const bool fh = wm_cross(u0, ex, ey) >= 0.0f;  // the first half-turn
      const int LO = fh ? 0 : H - 1, HI = fh ? H : L;
      if (u > 0 && !plain) {
        const int c = min(max(lo, LO), HI - 1);
        const bool t0 = wm_pred(s_u, c - 1, LO, HI, L, ex, ey), t1 = wm_pred(s_u, c, LO, HI, L, ex, ey);
        const bool t2 = wm_pred(s_u, c + 1, LO, HI, L, ex, ey), t3 = wm_pred(s_u, c + 2, LO, HI, L, ex, ey);
        const bool found = t1 ? !(t2 & t3) : t0;
        lo = t1 ? (t2 ? c + 1 : c) : c - 1;
        if (!found) lo = wm_search(s_u, LO, HI, ex, ey);
      } else {
        lo = wm_search(s_u, LO, HI, ex, ey);
      }
      const float r = s_r[lo];
      const float b = ex * ex + ey * ey;
      const float lo_r = r - a.th, hi_r = r + a.th;
      const bool known = (b <= a.mm) && (r > 0.0f);
      const bool fre = (lo_r > 0.0f) && (b < lo_r * lo_r);
      const bool occ = b <= hi_r * hi_r;
      const int m = (int)(int8_t)(old >> (8 * u));
      const int am = m < 0 ? -m : m, d = min(am, a.decay);
      const int faded = m > 0 ? m - d : m + d;  // m == 0: d == 0
      const int hit = min(max(m + a.l_hit, -a.l_max), a.l_max);
      const int fr = min(max(m - a.l_free, -a.l_max), a.l_max);
      const int mo = !known ? m : fre ? fr : occ ? hit : faded;
      out |= (uint32_t)(mo & 255) << (8 * u);
    }
    *cell = out;
  }
}

struct WorldFrameArgs {
  const float* pose;
  int64_t pose_stride;
  const int8_t* map;
  int64_t map_stride;  // bytes
  void* frame;
  int64_t frame_stride;  // elements
  int32_t bpe, Wc;
  int32_t unknown, outside, occ_thr, free_thr;
  float wh;
};

template <int FMT>
__global__ __launch_bounds__(kWmThreads) void world_frame_kernel(ffmp_cfg_t cfg, WorldFrameArgs a) {
  const int G = cfg.grid, G2 = G * G, Wc = a.Wc;
  const uint32_t lb = blockIdx.x, bpe = (uint32_t)a.bpe;
  const int64_t e = lb / bpe;
  const int tile = (int)(lb - (uint32_t)e * bpe);
  const int cq = tile * kWfBlockCells + 4 * (int)threadIdx.x;
  if (cq >= G2) return;  // G2 % 16 == 0: a lane's 4 cells are all in the plane or all outside it
  const int i = wm_div(cq, G, 1.0f / (float)G);  // G % 4 == 0: the 4 cells share row i
  const int j = cq - i * G;
  const float* ps = a.pose + e * a.pose_stride;
  const float px = ps[0], py = ps[1], pc = ps[2], psn = ps[3];
  const bool finite = wm_finite(px) && wm_finite(py) && wm_finite(pc) && wm_finite(psn);
  const int8_t* mp = a.map + e * a.map_stride;
  const float hi_f = (float)(Wc - 1);
  const float ex = cell_coord(cfg, i);
  uint32_t val[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const float ey = cell_coord(cfg, j + u);
    const float wx = (pc * ex - psn * ey) + px;
    const float wy = (psn * ex + pc * ey) + py;
    const float fp = rintf((wx + a.wh) / cfg.res_f);
    const float fq = rintf((wy + a.wh) / cfg.res_f);
    const bool inside = (fp >= 0.0f) && (fp <= hi_f) && (fq >= 0.0f) && (fq <= hi_f);
    const int gp = inside ? (int)fp : 0, gq = inside ? (int)fq : 0;  // in 0..Wc-1 either way
    const int m = (int)mp[gp * Wc + gq];
    const uint32_t v = !inside ? (uint32_t)a.outside : m >= a.occ_thr ? 255u : m <= -a.free_thr ? 0u : (uint32_t)a.unknown;
    val[u] = finite ? v : (uint32_t)a.unknown;
  }
  const int64_t at = e * a.frame_stride + cq;
  if (FMT == FFMP_OBS_F32) {
    wm_f32x4 v;
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = (float)val[u];
    *reinterpret_cast<wm_f32x4*>(reinterpret_cast<float*>(a.frame) + at) = v;
  } else {
    *reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(a.frame) + at) =
        val[0] | (val[1] << 8) | (val[2] << 16) | (val[3] << 24);
  }
}

int wm_plane_check(const char* who, const ffmp_cfg_t* cfg, int32_t cells) {
  if (!cfg) return fail(FFMP_E_ARG, "%s: cfg is NULL", who);
  if (cells < 8 || cells > 2048 || (cells % 4) != 0)
    return fail(FFMP_E_ARG, "%s: cells must be a multiple of 4 in [8,2048], got %d", who, cells);
  if (!(cfg->res_f > 0.0f) || isinf(cfg->res_f)) return fail(FFMP_E_ARG, "%s: cfg.res_f must be > 0 and finite", who);
  return FFMP_OK;
}

int world_map_check(const char* who, const ffmp_cfg_t* cfg, int32_t n_beams, int32_t cells, float thickness, float range_max,
                    int32_t l_hit, int32_t l_free, int32_t l_max, int32_t decay, int32_t flags) {
  if (int rc = wm_plane_check(who, cfg, cells)) return rc;
  if (n_beams < 1 || n_beams > FFMP_MAX_BEAMS)
    return fail(FFMP_E_ARG, "%s: n_beams must be in [1,%d], got %d", who, FFMP_MAX_BEAMS, n_beams);
  if (!(thickness >= 0.0f) || isinf(thickness)) return fail(FFMP_E_ARG, "%s: thickness must be >= 0 and finite", who);
  if (!(range_max > 0.0f)) return fail(FFMP_E_ARG, "%s: range_max must be > 0 (or +inf) and not NaN", who);
  if (l_hit < 0 || l_hit > 127) return fail(FFMP_E_ARG, "%s: l_hit must be in [0,127], got %d", who, l_hit);
  if (l_free < 0 || l_free > 127) return fail(FFMP_E_ARG, "%s: l_free must be in [0,127], got %d", who, l_free);
  if (l_max < 1 || l_max > 127) return fail(FFMP_E_ARG, "%s: l_max must be in [1,127], got %d", who, l_max);
  if (decay < 0 || decay > 127) return fail(FFMP_E_ARG, "%s: decay must be in [0,127], got %d", who, decay);
  if (flags & ~FFMP_SCAN_PLAIN) return fail(FFMP_E_ARG, "%s: unknown flags 0x%x", who, flags);
  return FFMP_OK;
}

int world_frame_check(const char* who, const ffmp_cfg_t* cfg, int32_t cells, int32_t format, int32_t unknown, int32_t outside,
                      int32_t occ_thr, int32_t free_thr) {
  if (int rc = wm_plane_check(who, cfg, cells)) return rc;
  if (cfg->grid < 8 || cfg->grid > 4096 || (cfg->grid % 4) != 0)
    return fail(FFMP_E_ARG, "%s: grid must be a multiple of 4 in [8,4096], got %d", who, cfg->grid);
  if (format != FFMP_OBS_F32 && format != FFMP_OBS_U8F16) return fail(FFMP_E_ARG, "%s: unknown format %d", who, format);
  if (unknown < 0 || unknown > 255) return fail(FFMP_E_ARG, "%s: unknown must be a byte 0..255, got %d", who, unknown);
  if (outside < 0 || outside > 255) return fail(FFMP_E_ARG, "%s: outside must be a byte 0..255, got %d", who, outside);
  if (occ_thr < 1 || occ_thr > 127) return fail(FFMP_E_ARG, "%s: occ_thr must be in [1,127], got %d", who, occ_thr);
  if (free_thr < 1 || free_thr > 127) return fail(FFMP_E_ARG, "%s: free_thr must be in [1,127], got %d", who, free_thr);
  return FFMP_OK;
}

// wh_f of the SPEC: Wc * res / 2 in float64, rounded
float wm_half(const ffmp_cfg_t* cfg, int32_t cells) { return (float)((double)cells * cfg->res / 2.0); }

// blocks per env of the update: the box of a unit (c, s) at range_max, clipped to the plane
int64_t wm_blocks_per_env(const ffmp_cfg_t* cfg, int32_t cells, float range_max) {
  double side = 2.0 * (((double)range_max * (1.0 + 1e-5)) / (double)cfg->res_f + 1.0) + 4.0;
  if (!(side <= (double)cells)) side = (double)cells;  // +inf and NaN: the plane
  const int64_t h = (int64_t)ceil(side), w = (h + 7) & ~(int64_t)3;
  const int64_t hc = h < cells ? h : cells, wc = w < cells ? w : cells;
  const int64_t bpe = (hc * wc + kWmBlockCells - 1) / kWmBlockCells;
  return bpe < 1 ? 1 : bpe;
}

}  // namespace

extern "C" {

int ffmp_world_map_check(const ffmp_cfg_t* cfg, int32_t n_beams, int32_t cells, float thickness, float range_max, int32_t l_hit,
                         int32_t l_free, int32_t l_max, int32_t decay, int32_t flags) {
  return world_map_check("ffmp_world_map", cfg, n_beams, cells, thickness, range_max, l_hit, l_free, l_max, decay, flags);
}

int ffmp_world_map(const ffmp_cfg_t* cfg, int64_t n, const float* ranges, int64_t ranges_stride, int32_t n_beams,
                   const float* sectors, const float* pose, int64_t pose_stride, const uint8_t* mask, const uint8_t* first,
                   int8_t* map, int64_t map_env_stride, int32_t cells, float thickness, float range_max, int32_t l_hit,
                   int32_t l_free, int32_t l_max, int32_t decay, int32_t flags, void* stream) {
  const char* who = "ffmp_world_map";
  if (int rc = world_map_check(who, cfg, n_beams, cells, thickness, range_max, l_hit, l_free, l_max, decay, flags)) return rc;
  if (n < 0) return fail(FFMP_E_ARG, "%s: negative n", who);
  if (!ranges) return fail(FFMP_E_ARG, "%s: ranges is NULL", who);
  if (!sectors) return fail(FFMP_E_ARG, "%s: sectors is NULL", who);
  if (!pose) return fail(FFMP_E_ARG, "%s: pose is NULL", who);
  if (!map) return fail(FFMP_E_ARG, "%s: map is NULL", who);
  if (ranges_stride < n_beams)
    return fail(FFMP_E_ARG, "%s: ranges_stride %lld < n_beams = %d", who, (long long)ranges_stride, n_beams);
  if (pose_stride < 4) return fail(FFMP_E_ARG, "%s: pose_stride %lld < 4", who, (long long)pose_stride);
  const int64_t W2 = (int64_t)cells * cells;
  if (map_env_stride < W2)
    return fail(FFMP_E_ARG, "%s: map_env_stride %lld < cells*cells = %lld", who, (long long)map_env_stride, (long long)W2);
  if (((uintptr_t)map & 3u) != 0 || (map_env_stride % 4) != 0)
    return fail(FFMP_E_ARG, "%s: the map must be 4-byte aligned with map_env_stride a multiple of 4 (map alignment)", who);
  const int64_t bpe = wm_blocks_per_env(cfg, cells, range_max);
  if (n > 0x7fffffffLL || n * bpe > 0x7fffffffLL) return fail(FFMP_E_ARG, "%s: n too large for one launch: %lld", who, (long long)n);
  if (n == 0) return FFMP_OK;

  WorldMapArgs a;
  a.ranges = ranges;
  a.ranges_stride = ranges_stride;
  a.sectors = sectors;
  a.pose = pose;
  a.pose_stride = pose_stride;
  a.mask = mask;
  a.first = first;
  a.map = map;
  a.map_stride = map_env_stride;
  a.L = n_beams;
  a.bpe = (int32_t)bpe;
  a.Wc = cells;
  a.plain = (flags & FFMP_SCAN_PLAIN) ? 1 : 0;
  a.th = thickness;
  a.rm = range_max;
  a.mm = range_max * range_max;
  a.wh = wm_half(cfg, cells);
  a.l_hit = l_hit;
  a.l_free = l_free;
  a.l_max = l_max;
  a.decay = decay;
  hipLaunchKernelGGL(world_map_kernel, dim3((unsigned)(n * bpe)), dim3(kWmThreads), 0, (hipStream_t)stream, *cfg, a);
  return launch_ok(who);
}

int ffmp_world_frame_check(const ffmp_cfg_t* cfg, int32_t cells, int32_t format, int32_t unknown, int32_t outside,
                           int32_t occ_thr, int32_t free_thr) {
  return world_frame_check("ffmp_world_frame", cfg, cells, format, unknown, outside, occ_thr, free_thr);
}

int ffmp_world_frame(const ffmp_cfg_t* cfg, int64_t n, const float* pose, int64_t pose_stride, const int8_t* map,
                     int64_t map_env_stride, int32_t cells, void* frame_out, int64_t frame_env_stride, int32_t format,
                     int32_t unknown, int32_t outside, int32_t occ_thr, int32_t free_thr, void* stream) {
  const char* who = "ffmp_world_frame";
  if (int rc = world_frame_check(who, cfg, cells, format, unknown, outside, occ_thr, free_thr)) return rc;
  if (n < 0) return fail(FFMP_E_ARG, "%s: negative n", who);
  if (!pose) return fail(FFMP_E_ARG, "%s: pose is NULL", who);
  if (!map) return fail(FFMP_E_ARG, "%s: map is NULL", who);
  if (!frame_out) return fail(FFMP_E_ARG, "%s: frame_out is NULL", who);
  if (pose_stride < 4) return fail(FFMP_E_ARG, "%s: pose_stride %lld < 4", who, (long long)pose_stride);
  const int64_t W2 = (int64_t)cells * cells, G2 = (int64_t)cfg->grid * cfg->grid;
  if (map_env_stride < W2)
    return fail(FFMP_E_ARG, "%s: map_env_stride %lld < cells*cells = %lld", who, (long long)map_env_stride, (long long)W2);
  if (frame_env_stride < G2)
    return fail(FFMP_E_ARG, "%s: frame_env_stride %lld < G*G = %lld", who, (long long)frame_env_stride, (long long)G2);
  const uintptr_t am = format == FFMP_OBS_F32 ? 15u : 3u;
  if (((uintptr_t)frame_out & am) != 0 || (frame_env_stride % 4) != 0)
    return fail(FFMP_E_ARG, "%s: frame_out must be %d-byte aligned with frame_env_stride a multiple of 4 elements (frame alignment)",
                who, (int)am + 1);
  const int64_t bpe = (G2 + kWfBlockCells - 1) / kWfBlockCells;
  if (n > 0x7fffffffLL || n * bpe > 0x7fffffffLL) return fail(FFMP_E_ARG, "%s: n too large for one launch: %lld", who, (long long)n);
  if (n > 0) {  // the bytes the launch reads against the bytes it writes
    const uint64_t es = format == FFMP_OBS_F32 ? 4u : 1u;
    const uintptr_t m0 = (uintptr_t)map, m1 = m0 + (uint64_t)(n - 1) * (uint64_t)map_env_stride + (uint64_t)W2;
    const uintptr_t f0 = (uintptr_t)frame_out, f1 = f0 + ((uint64_t)(n - 1) * (uint64_t)frame_env_stride + (uint64_t)G2) * es;
    if (m0 < f1 && f0 < m1) return fail(FFMP_E_ARG, "%s: frame_out overlaps the map", who);
  }
  if (n == 0) return FFMP_OK;

  WorldFrameArgs a;
  a.pose = pose;
  a.pose_stride = pose_stride;
  a.map = map;
  a.map_stride = map_env_stride;
  a.frame = frame_out;
  a.frame_stride = frame_env_stride;
  a.bpe = (int32_t)bpe;
  a.Wc = cells;
  a.unknown = unknown;
  a.outside = outside;
  a.occ_thr = occ_thr;
  a.free_thr = free_thr;
  a.wh = wm_half(cfg, cells);
  hipStream_t s = (hipStream_t)stream;
  if (format == FFMP_OBS_F32)
    hipLaunchKernelGGL((world_frame_kernel<FFMP_OBS_F32>), dim3((unsigned)(n * bpe)), dim3(kWmThreads), 0, s, *cfg, a);
  else
    hipLaunchKernelGGL((world_frame_kernel<FFMP_OBS_U8F16>), dim3((unsigned)(n * bpe)), dim3(kWmThreads), 0, s, *cfg, a);
  return launch_ok(who);
}

}  // extern "C"
