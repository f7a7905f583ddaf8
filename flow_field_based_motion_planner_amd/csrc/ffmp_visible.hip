// ffmp_visible.hip — sensor-visible occupancy frames: the raster's occupancy with line of sight
// from the robot applied (include/ffmp.h ffmp_visible_frames carries the SPEC).
//
// visible_kernel: the raster's shape.  A block of 256 threads serves up to 16,384 consecutive cells of
// one frame of one env; a wave task is 256 cells, 4 per lane (one 16-byte store for float32 frames,
// one 4-byte store for uint8 ones): 256 consecutive cells, or with G % 64 == 0 a tile of 4 rows x 64
// columns (the raster's FFMP_RASTER_TILE4).  The frame's header and discs are staged in LDS
// once per block, with oo = ox*ox + oy*oy and q = oo - r2 per disc (the SPEC's own operations, done
// once).  Lane k keeps disc k in registers and two culls run lane-parallel per wave task, each ending
// in one __ballot that gives the wave-uniform list of discs the per-cell loop visits:
//   inside cull   box_dist2(centre, task box) <= r2.  The box's bounds are cell coordinates (the same
//                 float32 expression, monotone in the index), float32 subtraction, squaring and
//                 addition are monotone, so box_dist2 <= the dx*dx + dy*dy of every cell of the box:
//                 a disc the test drops has `inside` false in every cell.  No margin is needed.
//   shadow cull   a cell p that disc o hides satisfies a > 0, a < b and q b <= a^2 (a = p.o, b = p.p),
//                 so p lies in the wedge of half-angle asin(r / |o|) about o — the intersection of the
//                 half-planes r a -+ sqrt(q) c >= 0 (c = p.o_perp) bounded by the two tangent lines
//                 from the sensor — and beyond the chord through the tangent points, a > q.  All three
//                 are linear in p, so a box reaches them iff one of its corners does.  Float32: the
//                 per-cell test can pass up to ~10 eps oo b past the exact boundary, so the cull uses
//                 q' = q - 1e-5 oo (a wider wedge; r' = 1.01 sqrt(oo - q'), since the float32 oo is
//                 within 2 eps oo of |o|^2 and oo - q' >= 1e-5 oo), tests a > 0.9999 q' and gives
//                 every corner value a slack of 1e-5 times its scale (eps = 6e-8: a factor > 10).
//                 A disc with q <= 2e-5 oo (the sensor inside it or on its rim) or with a non-finite
//                 word always passes.
// FFMP_VISIBLE_NOCULL replaces both lists by "every disc" (and tests the walls in every cell): the
// SPEC evaluated as written, to compare the culled path with.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "ffmp_device.h"
#include "ffmp_host.h"

#pragma clang fp contract(off)

namespace {

using namespace ffmp;

constexpr int kVisThreads = 256;
constexpr int kVisTask = 256;                     // cells of a wave task: 4 per lane
constexpr int kVisBlockCells = 4 * 16 * kVisTask;  // 4 waves x 16 tasks: the block's prologue (record -> LDS) is paid once

struct VisArgs {
  const float* record;
  int64_t rec_stride;  // floats
  const uint8_t* mask;
  void* out[2];        // the frames this launch computes, nf of them
  int32_t newest[2];   // out[s] is the newest frame (header words 0..3, current discs)
  int64_t env_stride;  // elements
  int32_t nf, bpe;     // frames per env, blocks per frame plane
  int32_t unknown, nocull;
  float rr;            // max_range * max_range
};

typedef float vis_f32x4 __attribute__((ext_vector_type(4)));

FFMP_DEV float vis_box_dist2(float px, float py, float x0, float x1, float y0, float y1) {
  const float dx = fmaxf(fmaxf(x0 - px, px - x1), 0.0f);
  const float dy = fmaxf(fmaxf(y0 - py, py - y1), 0.0f);
  return dx * dx + dy * dy;
}

// all of a box whose four corners pass lies inside the world (the world is convex, the ego -> world
// map is affine), cull_margin_f away from its walls: far more than the float32 error of the map
FFMP_DEV bool vis_corner_inside(const ffmp_cfg_t& cfg, const FrameHdr& h, float ex, float ey) {
  const float wx = h.px + (h.c * ex - h.s * ey);
  const float wy = h.py + (h.s * ex + h.c * ey);
  const float W = cfg.world_half_f - cfg.cull_margin_f;
  return (fabsf(wx) <= W) && (fabsf(wy) <= W);
}

// q / G for 0 <= q < 2^24 (G <= 4096): the float quotient is within one of it
FFMP_DEV int vis_div(int q, int G, float invG) {
  int i = (int)((float)q * invG);
  if (i * G > q) --i;
  if ((i + 1) * G <= q) ++i;
  return i;
}

template <int FMT>
__global__ __launch_bounds__(kVisThreads) void visible_kernel(ffmp_cfg_t cfg, VisArgs a) {
  __shared__ float4 s_d[FFMP_MAX_OBST];  // ox, oy, r2, r
  __shared__ float2 s_q[FFMP_MAX_OBST];  // oo, q
  __shared__ float s_h[4];

  const int K = cfg.n_obst, G = cfg.grid, G2 = G * G;
  const int tid = threadIdx.x;
  const uint32_t lb = blockIdx.x, bpe = (uint32_t)a.bpe, nf = (uint32_t)a.nf;  // 32-bit divisions: the grid has < 2^31 blocks
  const uint32_t ef = lb / bpe;
  const int tile = (int)(lb - ef * bpe);
  const int64_t e = ef / nf;
  const int slot = (int)(ef - (uint32_t)e * nf);
  if (a.mask && a.mask[e] == 0) return;  // block-uniform

  const bool newest = a.newest[slot] != 0;
  const float* rec = a.record + e * a.rec_stride;
  if (tid < 4) s_h[tid] = rec[(newest ? 0 : 4) + tid];
  if (tid < K) {
    const float* d = rec + FFMP_REC_HDR + 4 * ((newest ? 0 : K) + tid);
    const float4 o = make_float4(d[0], d[1], d[2], d[3]);
    const float oo = o.x * o.x + o.y * o.y;
    s_d[tid] = o;
    s_q[tid] = make_float2(oo, oo - o.z);
  }
  __syncthreads();

  const FrameHdr h{s_h[0], s_h[1], s_h[2], s_h[3]};
  const float res = cfg.res_f, half = cfg.half_f;
  const float invG = 1.0f / (float)G;
  const int wave = tid >> 6, lane = tid & 63;
  const bool nocull = a.nocull != 0;

  // lane k's disc: the operands of the two culls
  const bool has = lane < K;
  const float4 o = has ? s_d[lane] : make_float4(0.f, 0.f, 0.f, 0.f);
  const float2 oq = has ? s_q[lane] : make_float2(0.f, 0.f);
  const bool casts = has && o.z > 0.0f;                 // the SPEC's r2 > 0
  const bool always = !(oq.y > 2e-5f * oq.x);           // the sensor in or on the disc, or a non-finite word
  const float qw = oq.y - 1e-5f * oq.x;                 // q'
  const float sw = 0.9999f * sqrtf(fmaxf(qw, 0.0f));    // sqrt(q'), rounded towards the wider wedge
  const float rw = 1.01f * sqrtf(fmaxf(oq.x - qw, 0.0f));  // r'

  const int qbeg = tile * kVisBlockCells;
  const int qend = min(qbeg + kVisBlockCells, G2);
  float* of = reinterpret_cast<float*>(a.out[slot]) + e * a.env_stride;
  uint8_t* ob = reinterpret_cast<uint8_t*>(a.out[slot]) + e * a.env_stride;
  const float unk = (float)a.unknown;

  // G % 64 == 0: task t is the tile of 4 rows x 64 columns number t in band-major order instead of cells
  // [256 t, 256 t + 256) — the same task count, a compact box (C3: 0.2 m x 3.2 m, not 0.05 m x 12.8 m),
  // so fewer discs pass the culls; a row of a tile is 16 lanes' worth of contiguous stores.
  const bool tiled = (G & 63) == 0;
  const int ncb = G >> 6;

  for (int q0 = qbeg + wave * kVisTask; q0 < qend; q0 += 4 * kVisTask) {  // wave-uniform
    // the task's box: rows i0..i1, and its columns when it lies in one row
    int i0, i1, j0, j1;
    if (tiled) {
      const int t = q0 >> 8, band = vis_div(t, ncb, 1.0f / (float)ncb);
      i0 = 4 * band;
      i1 = i0 + 3;
      j0 = 64 * (t - band * ncb);
      j1 = j0 + 63;
    } else {
      const int ql = min(q0 + kVisTask, qend) - 1;
      i0 = vis_div(q0, G, invG);
      i1 = vis_div(ql, G, invG);
      j0 = i0 == i1 ? q0 - i0 * G : 0;
      j1 = i0 == i1 ? ql - i1 * G : G - 1;
    }
    const float bx0 = (float)i0 * res - half, bx1 = (float)i1 * res - half;
    const float by0 = (float)j0 * res - half, by1 = (float)j1 * res - half;

    uint64_t mi, ms;
    bool walls;
    if (nocull) {
      mi = __ballot(has);
      ms = __ballot(casts);
      walls = true;
    } else {
      mi = __ballot(has && vis_box_dist2(o.x, o.y, bx0, bx1, by0, by1) <= o.z);
      // corners (x0,y0) (x0,y1) (x1,y0) (x1,y1): a = p.o, c = p.o_perp, o_perp = (-oy, ox)
      const float a00 = bx0 * o.x + by0 * o.y, a01 = bx0 * o.x + by1 * o.y;
      const float a10 = bx1 * o.x + by0 * o.y, a11 = bx1 * o.x + by1 * o.y;
      const float c00 = by0 * o.x - bx0 * o.y, c01 = by1 * o.x - bx0 * o.y;
      const float c10 = by0 * o.x - bx1 * o.y, c11 = by1 * o.x - bx1 * o.y;
      const float amax = fmaxf(fmaxf(a00, a01), fmaxf(a10, a11));
      const float l1 = fmaxf(fmaxf(rw * a00 - sw * c00, rw * a01 - sw * c01),
                             fmaxf(rw * a10 - sw * c10, rw * a11 - sw * c11));
      const float l2 = fmaxf(fmaxf(rw * a00 + sw * c00, rw * a01 + sw * c01),
                             fmaxf(rw * a10 + sw * c10, rw * a11 + sw * c11));
      const float pm = fmaxf(fabsf(bx0), fabsf(bx1)) + fmaxf(fabsf(by0), fabsf(by1));  // >= |p| in the box
      const float ml = 1e-5f * (oq.x * pm) + 1e-30f;
      const bool reach = amax + 1e-5f * (oq.x + pm * pm) > 0.9999f * qw && l1 >= -ml && l2 >= -ml;
      ms = __ballot(casts && (always || reach));
      const uint64_t wb = __ballot(lane >= 4 || vis_corner_inside(cfg, h, (lane & 2) ? bx1 : bx0, (lane & 1) ? by1 : by0));
      walls = (wb & 0xFull) != 0xFull;
    }

    int q = q0 + 4 * lane, i, j;
    if (tiled) {
      i = i0 + (lane >> 4);
      j = j0 + 4 * (lane & 15);
      q = i * G + j;
    } else {
      if (q >= qend) continue;  // G2 % 16 == 0: a lane's 4 cells are all in the plane or all outside it
      i = vis_div(q, G, invG);  // G % 4 == 0: the 4 cells share row i
      j = q - i * G;
    }
    const float ex = cell_coord(cfg, i);
    float ey[4], b[4];
    bool occ[4], hid[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      ey[u] = cell_coord(cfg, j + u);
      b[u] = ex * ex + ey[u] * ey[u];
      occ[u] = walls & outside_world(cfg, h, ex, ey[u]);
      hid[u] = b[u] > a.rr;
    }
    for (uint64_t m = mi | ms; m; m &= m - 1) {
      const int k = __builtin_ctzll(m);
      const float4 d = s_d[k];
      const float2 dq = s_q[k];
      const bool sh = (ms >> k) & 1ull;  // wave-uniform
      const float dx = ex - d.x;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float dy = ey[u] - d.y;
        const bool inside = dx * dx + dy * dy <= d.z;
        occ[u] = occ[u] | inside;
        if (sh) {  // bitwise: every operand is evaluated, no branch per cell
          const float av = ex * d.x + ey[u] * d.y;
          const bool cone = (av > 0.0f) & (av < b[u]) & (dq.x * b[u] - av * av <= d.z * b[u]);
          hid[u] = hid[u] | (!inside & ((dq.y <= 0.0f) | cone));
        }
      }
    }
    if (FMT == FFMP_OBS_F32) {
      vis_f32x4 v;
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = hid[u] ? unk : (occ[u] ? 255.0f : 0.0f);
      *reinterpret_cast<vis_f32x4*>(of + q) = v;
    } else {
      uint32_t v = 0;
#pragma unroll
      for (int u = 0; u < 4; ++u) v |= (hid[u] ? (uint32_t)a.unknown : (occ[u] ? 255u : 0u)) << (8 * u);
      *reinterpret_cast<uint32_t*>(ob + q) = v;
    }
  }
}

int visible_check(const ffmp_cfg_t* cfg, int32_t format, int32_t unknown, float max_range, int32_t flags) {
  const char* who = "ffmp_visible_frames";
  if (!cfg) return fail(FFMP_E_ARG, "%s: cfg is NULL", who);
  if (cfg->grid < 8 || cfg->grid > 4096 || (cfg->grid % 4) != 0)
    return fail(FFMP_E_ARG, "%s: grid must be a multiple of 4 in [8,4096], got %d", who, cfg->grid);
  if (cfg->n_obst < 0 || cfg->n_obst > FFMP_MAX_OBST) return fail(FFMP_E_ARG, "%s: n_obst out of range: %d", who, cfg->n_obst);
  if (format != FFMP_OBS_F32 && format != FFMP_OBS_U8F16) return fail(FFMP_E_ARG, "%s: unknown format %d", who, format);
  if (unknown < 0 || unknown > 255) return fail(FFMP_E_ARG, "%s: unknown must be a byte 0..255, got %d", who, unknown);
  if (!(max_range >= 0.0f)) return fail(FFMP_E_ARG, "%s: max_range must be >= 0 and not NaN", who);
  if (flags & ~FFMP_VISIBLE_NOCULL) return fail(FFMP_E_ARG, "%s: unknown flags 0x%x", who, flags);
  return FFMP_OK;
}

}  // namespace

extern "C" {

int ffmp_visible_frames_check(const ffmp_cfg_t* cfg, int32_t format, int32_t unknown, float max_range, int32_t flags) {
  return visible_check(cfg, format, unknown, max_range, flags);
}

int ffmp_visible_frames(const ffmp_cfg_t* cfg, int64_t n, const float* record, int64_t record_stride,
                        const uint8_t* mask, void* out_older, void* out_newest, int64_t out_env_stride,
                        int32_t format, int32_t unknown, float max_range, int32_t flags, void* stream) {
  const char* who = "ffmp_visible_frames";
  if (int rc = visible_check(cfg, format, unknown, max_range, flags)) return rc;
  if (n < 0) return fail(FFMP_E_ARG, "%s: negative n", who);
  if (!record) return fail(FFMP_E_ARG, "%s: record is NULL", who);
  const int64_t rec_len = FFMP_REC_HDR + 12 * (int64_t)cfg->n_obst;
  if (record_stride < rec_len)
    return fail(FFMP_E_ARG, "%s: record_stride %lld < %lld floats of a record", who, (long long)record_stride, (long long)rec_len);
  if (!out_older && !out_newest) return fail(FFMP_E_ARG, "%s: out_older and out_newest are both NULL", who);
  const int64_t G2 = (int64_t)cfg->grid * cfg->grid;
  if (out_env_stride < G2)
    return fail(FFMP_E_ARG, "%s: out_env_stride %lld < G*G = %lld", who, (long long)out_env_stride, (long long)G2);
  const uintptr_t am = format == FFMP_OBS_F32 ? 15u : 3u;
  if ((((uintptr_t)out_older | (uintptr_t)out_newest) & am) != 0 || (out_env_stride % 4) != 0)
    return fail(FFMP_E_ARG, "%s: outputs must be %d-byte aligned with out_env_stride a multiple of 4 elements (alignment)", who,
                (int)am + 1);
  if (n == 0) return FFMP_OK;

  VisArgs a;
  a.record = record;
  a.rec_stride = record_stride;
  a.mask = mask;
  a.nf = 0;
  a.out[0] = a.out[1] = nullptr;
  a.newest[0] = a.newest[1] = 0;
  if (out_older) { a.out[a.nf] = out_older; a.newest[a.nf++] = 0; }
  if (out_newest) { a.out[a.nf] = out_newest; a.newest[a.nf++] = 1; }
  a.env_stride = out_env_stride;
  a.bpe = (int32_t)((G2 + kVisBlockCells - 1) / kVisBlockCells);
  a.unknown = unknown;
  a.nocull = (flags & FFMP_VISIBLE_NOCULL) ? 1 : 0;
  a.rr = max_range * max_range;
  const int64_t blocks = n * a.nf * a.bpe;
  if (n > 0x7fffffffLL || blocks > 0x7fffffffLL) return fail(FFMP_E_ARG, "%s: n too large for one launch: %lld", who, (long long)n);
  hipStream_t s = (hipStream_t)stream;
  if (format == FFMP_OBS_F32)
    hipLaunchKernelGGL((visible_kernel<FFMP_OBS_F32>), dim3((unsigned)blocks), dim3(kVisThreads), 0, s, *cfg, a);
  else
    hipLaunchKernelGGL((visible_kernel<FFMP_OBS_U8F16>), dim3((unsigned)blocks), dim3(kVisThreads), 0, s, *cfg, a);
  return launch_ok(who);
}

}  // extern "C"
