// ffmp_scan.hip — occupancy frames built from the lidar scan: the inverse sensor model
// (include/ffmp.h ffmp_scan_frames carries the SPEC).  Below it scan_map_kernel, the
// accumulated map: the same classification added to an int8 log-odds plane that is first moved into the
// current ego frame (include/ffmp.h ffmp_scan_map).
//
// scan_kernel: visible_kernel's shape.  A block of 256 threads serves up to 16,384 consecutive cells of
// one env; a wave task is 256 cells, 4 per lane (one 16-byte store for float32 frames, one 4-byte store
// for uint8 ones): 256 consecutive cells, or with G % 64 == 0 a tile of 4 rows x 64 columns.  The env's
// L ranges and the L sector vectors are staged in LDS once per block (12 KiB at L = 1024).  A cell's
// cone is found by the SPEC's bisection over the sector vectors: at most ceil(log2 L) dependent 8-byte
// LDS reads.  One block writes both frames of its cells, so the lane that moves the previous newest
// value into the older frame is the lane that overwrites it.
//
// The shortcut (every cell after a lane's first; FFMP_SCAN_PLAIN turns it off).  Let t(m) =
// u[m].x*ey - u[m].y*ex, the float32 cross product of sector vector m with the cell.  The SPEC picks
// the half-turn (LO, HI) = (0, H) or (H - 1, L) from the sign of t(0) and bisects to an index lo in
// [LO, HI) such that
//     (lo == LO or t(lo) >= 0)  and  (lo + 1 == HI or t(lo + 1) < 0):                         (P)
// LO stands for "true" and HI for "false" without being evaluated, and each step keeps a true lo and a
// false hi.  Inside one half-turn the vectors u[LO + 1 .. HI - 1] turn by less than pi, so in exact
// arithmetic t(m) = |p| sin(bearing - angle_m) is >= 0 up to the cell's cone and < 0 after it: the
// predicate is monotone in m, there is exactly one index with (P), and every bisection order ends on
// it.  In float32 the sign of t(m) is exact wherever |sin| exceeds a few 2^-24, i.e. everywhere but at
// the one boundary the cell lies on (if any) — a single uncertain m between a run of true and a run of
// false leaves the sequence monotone whichever way it rounds — and, for even L, at m = H for a cell on
// boundary 0, where t(H) = -t(0) bit for bit when u[H] = -u[0] (float32 products and differences round
// symmetrically), which is true exactly when the SPEC takes the second half-turn.  So ANY index of
// the cell's own half-turn that has (P) is the SPEC's answer.  A lane's cells are neighbours along a
// row and mostly share a cone or lie in adjacent ones, so cells 2..4 take the previous cell's lo,
// clamped into this cell's half-turn (which is taken from this cell's own t(0)), as c and evaluate the
// predicate at c - 1, c, c + 1, c + 2 — four independent LDS reads, no branch — with the ends of the
// half-turn standing for true and false as in the bisection.  If one of c - 1, c, c + 1 has (P) it is
// the answer; otherwise (next to the origin, mostly) the cell bisects.  Two variants with branches were
// measured first and are slower than no shortcut at all, C3 newest frame, no shortcut 4.17-4.24 ms:
// "test (P) at the old lo, else bisect" 4.73 ms (in nearly every wave some lane's cell has moved on to
// the next cone, and then the whole wave pays for the bisection), "walk down or up from the old lo, at
// most three steps" 4.41 ms (a divergent loop iteration costs as much as two of the bisection's).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "ffmp_device.h"
#include "ffmp_host.h"

#pragma clang fp contract(off)

namespace {

using namespace ffmp;

constexpr int kScanThreads = 256;
constexpr int kScanTask = 256;                       // cells of a wave task: 4 per lane
constexpr int kScanBlockCells = 4 * 16 * kScanTask;  // 4 waves x 16 tasks: the staging of the scan is paid once

struct ScanArgs {
  const float* ranges;
  int64_t ranges_stride;  // floats
  const float* sectors;   // (L, 2)
  const uint8_t* mask;
  const uint8_t* first;
  void* older;            // or NULL
  void* newest;           // or NULL
  int64_t env_stride;     // elements
  int32_t L, bpe;         // beams, blocks per env
  int32_t unknown, plain;
  float th, mm;           // thickness, range_max * range_max
};

typedef float scan_f32x4 __attribute__((ext_vector_type(4)));

// q / G for 0 <= q < 2^24 (G <= 4096): the float quotient is within one of it
FFMP_DEV int scan_div(int q, int G, float invG) {
  int i = (int)((float)q * invG);
  if (i * G > q) --i;
  if ((i + 1) * G <= q) ++i;
  return i;
}

FFMP_DEV float scan_cross(float2 u, float ex, float ey) { return u.x * ey - u.y * ex; }

// the SPEC's bisection from (lo, hi)
FFMP_DEV int scan_search(const float2* s_u, int lo, int hi, float ex, float ey) {
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (scan_cross(s_u[mid], ex, ey) >= 0.0f) lo = mid; else hi = mid;
  }
  return lo;
}

// the bisection's predicate at m, the ends of the half-turn included: true at and below LO, false at and
// above HI, t(m) >= 0 between them (the read is clamped into the table, its value then unused)
FFMP_DEV bool scan_pred(const float2* s_u, int m, int LO, int HI, int L, float ex, float ey) {
  const float t = scan_cross(s_u[min(max(m, 0), L - 1)], ex, ey);
  return (m <= LO) | ((m < HI) & (t >= 0.0f));
}

template <int FMT>
__global__ __launch_bounds__(kScanThreads) void scan_kernel(ffmp_cfg_t cfg, ScanArgs a) {
  __shared__ float2 s_u[FFMP_MAX_BEAMS];
  __shared__ float s_r[FFMP_MAX_BEAMS];

  const int L = a.L, G = cfg.grid, G2 = G * G;
  const int tid = threadIdx.x;
  const uint32_t lb = blockIdx.x, bpe = (uint32_t)a.bpe;  // 32-bit division: the grid has < 2^31 blocks
  const int64_t e = lb / bpe;
  const int tile = (int)(lb - (uint32_t)e * bpe);
  if (a.mask && a.mask[e] == 0) return;  // block-uniform

  const float* rg = a.ranges + e * a.ranges_stride;
  for (int l = tid; l < L; l += kScanThreads) {
    s_u[l] = make_float2(a.sectors[2 * l], a.sectors[2 * l + 1]);
    s_r[l] = rg[l];
  }
  __syncthreads();

  const bool shift = a.older && a.newest && a.first && a.first[e] == 0;  // older <- the previous newest
  const float invG = 1.0f / (float)G;
  const int wave = tid >> 6, lane = tid & 63;
  const int H = (L + 1) >> 1;
  const float2 u0 = s_u[0];
  const bool plain = a.plain != 0;

  const int qbeg = tile * kScanBlockCells;
  const int qend = min(qbeg + kScanBlockCells, G2);
  const int64_t base = e * a.env_stride;
  const bool tiled = (G & 63) == 0;
  const int ncb = G >> 6;

  for (int q0 = qbeg + wave * kScanTask; q0 < qend; q0 += 4 * kScanTask) {  // wave-uniform
    int q = q0 + 4 * lane, i, j;
    if (tiled) {  // task t: the tile of 4 rows x 64 columns number t in band-major order
      const int t = q0 >> 8, band = scan_div(t, ncb, 1.0f / (float)ncb);
      i = 4 * band + (lane >> 4);
      j = 64 * (t - band * ncb) + 4 * (lane & 15);
      q = i * G + j;
    } else {
      if (q >= qend) continue;  // G2 % 16 == 0: a lane's 4 cells are all in the plane or all outside it
      i = scan_div(q, G, invG);  // G % 4 == 0: the 4 cells share row i
      j = q - i * G;
    }
    const float ex = cell_coord(cfg, i);
    uint32_t val[4];
    int lo = 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float ey = cell_coord(cfg, j + u);
      const bool fh = scan_cross(u0, ex, ey) >= 0.0f;  // the first half-turn
      const int LO = fh ? 0 : H - 1, HI = fh ? H : L;
      if (u > 0 && !plain) {
        // the previous cell's cone and its neighbours (see the head of the file); s_u is read at
        // indices clamped into 0..L-1
        const int c = min(max(lo, LO), HI - 1);
        const bool p0 = scan_pred(s_u, c - 1, LO, HI, L, ex, ey), p1 = scan_pred(s_u, c, LO, HI, L, ex, ey);
        const bool p2 = scan_pred(s_u, c + 1, LO, HI, L, ex, ey), p3 = scan_pred(s_u, c + 2, LO, HI, L, ex, ey);
        const bool found = p1 ? !(p2 & p3) : p0;
        lo = p1 ? (p2 ? c + 1 : c) : c - 1;
        if (!found) lo = scan_search(s_u, LO, HI, ex, ey);
      } else {
        lo = scan_search(s_u, LO, HI, ex, ey);
      }
      const float r = s_r[lo];
      const float b = ex * ex + ey * ey;
      const float lo_r = r - a.th, hi_r = r + a.th;
      const bool known = (b <= a.mm) && (r > 0.0f);
      const bool fre = (lo_r > 0.0f) && (b < lo_r * lo_r);
      const bool occ = b <= hi_r * hi_r;
      val[u] = !known ? (uint32_t)a.unknown : fre ? 0u : occ ? 255u : (uint32_t)a.unknown;
    }
    if (FMT == FFMP_OBS_F32) {
      scan_f32x4 v;
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = (float)val[u];
      float* nw = a.newest ? reinterpret_cast<float*>(a.newest) + base + q : nullptr;
      if (a.older) {
        const scan_f32x4 ov = shift ? *reinterpret_cast<const scan_f32x4*>(nw) : v;
        *reinterpret_cast<scan_f32x4*>(reinterpret_cast<float*>(a.older) + base + q) = ov;
      }
      if (nw) *reinterpret_cast<scan_f32x4*>(nw) = v;
    } else {
      const uint32_t v = val[0] | (val[1] << 8) | (val[2] << 16) | (val[3] << 24);
      uint8_t* nw = a.newest ? reinterpret_cast<uint8_t*>(a.newest) + base + q : nullptr;
      if (a.older) {
        const uint32_t ov = shift ? *reinterpret_cast<const uint32_t*>(nw) : v;
        *reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(a.older) + base + q) = ov;
      }
      if (nw) *reinterpret_cast<uint32_t*>(nw) = v;
    }
  }
}

// ---------------------------------------------------------------- the accumulated map
struct ScanMapArgs {
  const float* ranges;
  int64_t ranges_stride;  // floats
  const float* sectors;   // (L, 2)
  const float* pose_now;  // {px, py, cos yaw, sin yaw} per env
  int64_t pose_now_stride;
  const float* pose_prev;
  int64_t pose_prev_stride;
  const uint8_t* mask;
  const uint8_t* first;   // or NULL
  const int8_t* map_in;
  int8_t* map_out;
  int64_t map_stride;     // bytes
  void* frame;            // or NULL
  int64_t frame_stride;   // elements
  int32_t L, bpe;
  int32_t unknown, plain;
  float th, mm;
  int32_t l_hit, l_free, l_max, decay, occ_thr, free_thr;
};

// The class of a lane's 4 cells (row i, columns j .. j + 3) under the staged scan: scan_kernel's loop body,
// word for word, ending in f(u, known, fre, occ) instead of a value.  scan_kernel keeps its own copy: called
// from there, this function changes that kernel's register allocation (its code object must stay as it is).
template <class F>
FFMP_DEV void scan_classes(const ffmp_cfg_t& cfg, const float2* s_u, const float* s_r, int L, int H, float2 u0, bool plain,
                           float th, float mm, int i, int j, F&& f) {
  const float ex = cell_coord(cfg, i);
  int lo = 0;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const float ey = cell_coord(cfg, j + u);
    const bool fh = scan_cross(u0, ex, ey) >= 0.0f;  // the first half-turn
    const int LO = fh ? 0 : H - 1, HI = fh ? H : L;
    if (u > 0 && !plain) {
      const int c = min(max(lo, LO), HI - 1);
      const bool p0 = scan_pred(s_u, c - 1, LO, HI, L, ex, ey), p1 = scan_pred(s_u, c, LO, HI, L, ex, ey);
      const bool p2 = scan_pred(s_u, c + 1, LO, HI, L, ex, ey), p3 = scan_pred(s_u, c + 2, LO, HI, L, ex, ey);
      const bool found = p1 ? !(p2 & p3) : p0;
      lo = p1 ? (p2 ? c + 1 : c) : c - 1;
      if (!found) lo = scan_search(s_u, LO, HI, ex, ey);
    } else {
      lo = scan_search(s_u, LO, HI, ex, ey);
    }
    const float r = s_r[lo];
    const float b = ex * ex + ey * ey;
    const float lo_r = r - th, hi_r = r + th;
    const bool known = (b <= mm) && (r > 0.0f);
    const bool fre = (lo_r > 0.0f) && (b < lo_r * lo_r);
    const bool occ = b <= hi_r * hi_r;
    f(u, known, fre, occ);
  }
}

// scan_kernel's shape (blocks, tasks, staging).  Per lane: four 1-byte loads of the previous plane at the
// warped cells (a 4 x 64 tile reads a rotated box of about that size: the cache lines are shared by the
// wave), one 4-byte store of the new plane, one 16- or 4-byte store of the frame.  The blocks of an env
// whose mask byte is 0 copy its plane with 4-byte loads and stores.
template <int FMT>
__global__ __launch_bounds__(kScanThreads) void scan_map_kernel(ffmp_cfg_t cfg, ScanMapArgs a) {
  __shared__ float2 s_u[FFMP_MAX_BEAMS];
  __shared__ float s_r[FFMP_MAX_BEAMS];

  const int L = a.L, G = cfg.grid, G2 = G * G;
  const int tid = threadIdx.x;
  const uint32_t lb = blockIdx.x, bpe = (uint32_t)a.bpe;
  const int64_t e = lb / bpe;
  const int tile = (int)(lb - (uint32_t)e * bpe);
  const int qbeg = tile * kScanBlockCells;
  const int qend = min(qbeg + kScanBlockCells, G2);
  const int8_t* min_ = a.map_in + e * a.map_stride;
  int8_t* mout = a.map_out + e * a.map_stride;
  if (a.mask && a.mask[e] == 0) {  // block-uniform: the plane as it is, no warp, no frame
    for (int q = qbeg + 4 * tid; q < qend; q += 4 * kScanThreads)
      *reinterpret_cast<uint32_t*>(mout + q) = *reinterpret_cast<const uint32_t*>(min_ + q);
    return;
  }

  const float* rg = a.ranges + e * a.ranges_stride;
  for (int l = tid; l < L; l += kScanThreads) {
    s_u[l] = make_float2(a.sectors[2 * l], a.sectors[2 * l + 1]);
    s_r[l] = rg[l];
  }
  __syncthreads();

  // the env's motion: float64 from eight float32 words, rounded to float32 (every thread, block-uniform)
  const float* p1 = a.pose_now + e * a.pose_now_stride;
  const float* p0 = a.pose_prev + e * a.pose_prev_stride;
  const double c0 = (double)p0[2], s0 = (double)p0[3], c1 = (double)p1[2], s1 = (double)p1[3];
  const double dx = (double)p1[0] - (double)p0[0], dy = (double)p1[1] - (double)p0[1];
  const float cr = (float)(c0 * c1 + s0 * s1);
  const float sr = (float)(c0 * s1 - s0 * c1);
  const float tx = (float)((c0 * dx + s0 * dy) / (double)cfg.res_f);
  const float ty = (float)((c0 * dy - s0 * dx) / (double)cfg.res_f);
  const bool finite = (cr - cr == 0.0f) && (sr - sr == 0.0f) && (tx - tx == 0.0f) && (ty - ty == 0.0f);
  const bool restart = (a.first && a.first[e] != 0) || !finite;

  const float invG = 1.0f / (float)G;
  const int wave = tid >> 6, lane = tid & 63;
  const int H = (L + 1) >> 1, hg = G >> 1;
  const float lo_f = (float)(-hg), hi_f = (float)(hg - 1);
  const float2 u0 = s_u[0];
  const bool plain = a.plain != 0;
  const int64_t fbase = e * a.frame_stride;
  const bool tiled = (G & 63) == 0;
  const int ncb = G >> 6;

  for (int q0 = qbeg + wave * kScanTask; q0 < qend; q0 += 4 * kScanTask) {  // wave-uniform
    int q = q0 + 4 * lane, i, j;
    if (tiled) {
      const int t = q0 >> 8, band = scan_div(t, ncb, 1.0f / (float)ncb);
      i = 4 * band + (lane >> 4);
      j = 64 * (t - band * ncb) + 4 * (lane & 15);
      q = i * G + j;
    } else {
      if (q >= qend) continue;
      i = scan_div(q, G, invG);
      j = q - i * G;
    }
    // the nearest-neighbour gather of the prior: cell (i, j + u) of this frame is cell (ru, rv) of the previous one
    const float fa = (float)(i - hg);
    int prior[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float fb = (float)(j + u - hg);
      const float wu = (cr * fa - sr * fb) + tx;
      const float wv = (sr * fa + cr * fb) + ty;
      const float ru = rintf(wu), rv = rintf(wv);
      const bool inside = (ru >= lo_f) && (ru <= hi_f) && (rv >= lo_f) && (rv <= hi_f) && !restart;
      const int gi = inside ? (int)ru + hg : 0, gj = inside ? (int)rv + hg : 0;  // in 0..G-1 either way
      const int m = (int)min_[gi * G + gj];
      prior[u] = inside ? m : 0;
    }
    int mo[4];
    scan_classes(cfg, s_u, s_r, L, H, u0, plain, a.th, a.mm, i, j, [&](int u, bool known, bool fre, bool occ) {
      const int p = prior[u];
      const int ap = p < 0 ? -p : p, d = min(ap, a.decay);
      const int faded = p > 0 ? p - d : p + d;  // p == 0: d == 0
      const int hit = min(max(p + a.l_hit, -a.l_max), a.l_max);
      const int fr = min(max(p - a.l_free, -a.l_max), a.l_max);
      mo[u] = !known ? faded : fre ? fr : occ ? hit : faded;
    });
    *reinterpret_cast<uint32_t*>(mout + q) =
        (uint32_t)(mo[0] & 255) | ((uint32_t)(mo[1] & 255) << 8) | ((uint32_t)(mo[2] & 255) << 16) | ((uint32_t)(mo[3] & 255) << 24);
    if (a.frame) {
      uint32_t val[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) val[u] = mo[u] >= a.occ_thr ? 255u : mo[u] <= -a.free_thr ? 0u : (uint32_t)a.unknown;
      if (FMT == FFMP_OBS_F32) {
        scan_f32x4 v;
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = (float)val[u];
        *reinterpret_cast<scan_f32x4*>(reinterpret_cast<float*>(a.frame) + fbase + q) = v;
      } else {
        *reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(a.frame) + fbase + q) =
            val[0] | (val[1] << 8) | (val[2] << 16) | (val[3] << 24);
      }
    }
  }
}

// plane e of one array against plane e' of the other (elements of es bytes, S elements between envs): they
// overlap iff |d + (e - e') S| < G*G
bool scan_planes_overlap(const void* pa, const void* pb, uint64_t es, int64_t stride, int64_t G2, int64_t n) {
  const uintptr_t po = (uintptr_t)pa, pn = (uintptr_t)pb;
  const uint64_t d = (po > pn ? po - pn : pn - po) / es, S = (uint64_t)stride;
  const uint64_t k = d / S, r = d - k * S, last = n > 0 ? (uint64_t)(n - 1) : 0u;
  return d < (uint64_t)G2 || (k <= last && r < (uint64_t)G2) || (k + 1 <= last && S - r < (uint64_t)G2);
}

int scan_check(const char* who, const ffmp_cfg_t* cfg, int32_t n_beams, int32_t format, int32_t unknown, float thickness,
               float range_max, int32_t flags) {
  if (!cfg) return fail(FFMP_E_ARG, "%s: cfg is NULL", who);
  if (cfg->grid < 8 || cfg->grid > 4096 || (cfg->grid % 4) != 0)
    return fail(FFMP_E_ARG, "%s: grid must be a multiple of 4 in [8,4096], got %d", who, cfg->grid);
  if (n_beams < 1 || n_beams > FFMP_MAX_BEAMS)
    return fail(FFMP_E_ARG, "%s: n_beams must be in [1,%d], got %d", who, FFMP_MAX_BEAMS, n_beams);
  if (format != FFMP_OBS_F32 && format != FFMP_OBS_U8F16) return fail(FFMP_E_ARG, "%s: unknown format %d", who, format);
  if (unknown < 0 || unknown > 255) return fail(FFMP_E_ARG, "%s: unknown must be a byte 0..255, got %d", who, unknown);
  if (!(thickness >= 0.0f) || isinf(thickness)) return fail(FFMP_E_ARG, "%s: thickness must be >= 0 and finite", who);
  if (!(range_max > 0.0f)) return fail(FFMP_E_ARG, "%s: range_max must be > 0 (or +inf) and not NaN", who);
  if (flags & ~FFMP_SCAN_PLAIN) return fail(FFMP_E_ARG, "%s: unknown flags 0x%x", who, flags);
  return FFMP_OK;
}

int scan_map_check(const char* who, const ffmp_cfg_t* cfg, int32_t n_beams, int32_t format, int32_t unknown, float thickness,
                   float range_max, int32_t l_hit, int32_t l_free, int32_t l_max, int32_t decay, int32_t occ_thr,
                   int32_t free_thr, int32_t flags) {
  if (int rc = scan_check(who, cfg, n_beams, format, unknown, thickness, range_max, flags)) return rc;
  if (l_hit < 0 || l_hit > 127) return fail(FFMP_E_ARG, "%s: l_hit must be in [0,127], got %d", who, l_hit);
  if (l_free < 0 || l_free > 127) return fail(FFMP_E_ARG, "%s: l_free must be in [0,127], got %d", who, l_free);
  if (l_max < 1 || l_max > 127) return fail(FFMP_E_ARG, "%s: l_max must be in [1,127], got %d", who, l_max);
  if (decay < 0 || decay > 127) return fail(FFMP_E_ARG, "%s: decay must be in [0,127], got %d", who, decay);
  if (occ_thr < 1 || occ_thr > 127) return fail(FFMP_E_ARG, "%s: occ_thr must be in [1,127], got %d", who, occ_thr);
  if (free_thr < 1 || free_thr > 127) return fail(FFMP_E_ARG, "%s: free_thr must be in [1,127], got %d", who, free_thr);
  return FFMP_OK;
}

}  // namespace

extern "C" {

int ffmp_scan_frames_check(const ffmp_cfg_t* cfg, int32_t n_beams, int32_t format, int32_t unknown, float thickness,
                           float range_max, int32_t flags) {
  return scan_check("ffmp_scan_frames", cfg, n_beams, format, unknown, thickness, range_max, flags);
}

int ffmp_scan_frames(const ffmp_cfg_t* cfg, int64_t n, const float* ranges, int64_t ranges_stride, int32_t n_beams,
                     const float* sectors, const uint8_t* mask, const uint8_t* first, void* out_older, void* out_newest,
                     int64_t out_env_stride, int32_t format, int32_t unknown, float thickness, float range_max,
                     int32_t flags, void* stream) {
  const char* who = "ffmp_scan_frames";
  if (int rc = scan_check(who, cfg, n_beams, format, unknown, thickness, range_max, flags)) return rc;
  if (n < 0) return fail(FFMP_E_ARG, "%s: negative n", who);
  if (!ranges) return fail(FFMP_E_ARG, "%s: ranges is NULL", who);
  if (!sectors) return fail(FFMP_E_ARG, "%s: sectors is NULL", who);
  if (ranges_stride < n_beams)
    return fail(FFMP_E_ARG, "%s: ranges_stride %lld < n_beams = %d", who, (long long)ranges_stride, n_beams);
  if (!out_older && !out_newest) return fail(FFMP_E_ARG, "%s: out_older and out_newest are both NULL", who);
  const int64_t G2 = (int64_t)cfg->grid * cfg->grid;
  if (out_env_stride < G2)
    return fail(FFMP_E_ARG, "%s: out_env_stride %lld < G*G = %lld", who, (long long)out_env_stride, (long long)G2);
  const uintptr_t am = format == FFMP_OBS_F32 ? 15u : 3u;
  if ((((uintptr_t)out_older | (uintptr_t)out_newest) & am) != 0 || (out_env_stride % 4) != 0)
    return fail(FFMP_E_ARG, "%s: outputs must be %d-byte aligned with out_env_stride a multiple of 4 elements (alignment)", who,
                (int)am + 1);
  const int64_t bpe = (G2 + kScanBlockCells - 1) / kScanBlockCells;
  if (n > 0x7fffffffLL || n * bpe > 0x7fffffffLL) return fail(FFMP_E_ARG, "%s: n too large for one launch: %lld", who, (long long)n);
  if (out_older && out_newest) {
    if (scan_planes_overlap(out_older, out_newest, format == FFMP_OBS_F32 ? 4u : 1u, out_env_stride, G2, n))
      return fail(FFMP_E_ARG, "%s: the older and newest planes overlap (they must lie G*G = %lld elements apart)", who,
                  (long long)G2);
  }
  if (n == 0) return FFMP_OK;

  ScanArgs a;
  a.ranges = ranges;
  a.ranges_stride = ranges_stride;
  a.sectors = sectors;
  a.mask = mask;
  a.first = first;
  a.older = out_older;
  a.newest = out_newest;
  a.env_stride = out_env_stride;
  a.L = n_beams;
  a.bpe = (int32_t)bpe;
  a.unknown = unknown;
  a.plain = (flags & FFMP_SCAN_PLAIN) ? 1 : 0;
  a.th = thickness;
  a.mm = range_max * range_max;
  const int64_t blocks = n * bpe;
  hipStream_t s = (hipStream_t)stream;
  if (format == FFMP_OBS_F32)
    hipLaunchKernelGGL((scan_kernel<FFMP_OBS_F32>), dim3((unsigned)blocks), dim3(kScanThreads), 0, s, *cfg, a);
  else
    hipLaunchKernelGGL((scan_kernel<FFMP_OBS_U8F16>), dim3((unsigned)blocks), dim3(kScanThreads), 0, s, *cfg, a);
  return launch_ok(who);
}

int ffmp_scan_map_check(const ffmp_cfg_t* cfg, int32_t n_beams, int32_t format, int32_t unknown, float thickness,
                        float range_max, int32_t l_hit, int32_t l_free, int32_t l_max, int32_t decay, int32_t occ_thr,
                        int32_t free_thr, int32_t flags) {
  return scan_map_check("ffmp_scan_map", cfg, n_beams, format, unknown, thickness, range_max, l_hit, l_free, l_max, decay,
                        occ_thr, free_thr, flags);
}

int ffmp_scan_map(const ffmp_cfg_t* cfg, int64_t n, const float* ranges, int64_t ranges_stride, int32_t n_beams,
                  const float* sectors, const float* pose_now, int64_t pose_now_stride, const float* pose_prev,
                  int64_t pose_prev_stride, const uint8_t* mask, const uint8_t* first, const int8_t* map_in, int8_t* map_out,
                  int64_t map_env_stride, void* frame_out, int64_t frame_env_stride, int32_t format, int32_t unknown,
                  float thickness, float range_max, int32_t l_hit, int32_t l_free, int32_t l_max, int32_t decay,
                  int32_t occ_thr, int32_t free_thr, int32_t flags, void* stream) {
  const char* who = "ffmp_scan_map";
  if (int rc = scan_map_check(who, cfg, n_beams, format, unknown, thickness, range_max, l_hit, l_free, l_max, decay, occ_thr,
                              free_thr, flags))
    return rc;
  if (n < 0) return fail(FFMP_E_ARG, "%s: negative n", who);
  if (!ranges) return fail(FFMP_E_ARG, "%s: ranges is NULL", who);
  if (!sectors) return fail(FFMP_E_ARG, "%s: sectors is NULL", who);
  if (!pose_now) return fail(FFMP_E_ARG, "%s: pose_now is NULL", who);
  if (!pose_prev) return fail(FFMP_E_ARG, "%s: pose_prev is NULL", who);
  if (!map_in) return fail(FFMP_E_ARG, "%s: map_in is NULL", who);
  if (!map_out) return fail(FFMP_E_ARG, "%s: map_out is NULL", who);
  if (ranges_stride < n_beams)
    return fail(FFMP_E_ARG, "%s: ranges_stride %lld < n_beams = %d", who, (long long)ranges_stride, n_beams);
  if (pose_now_stride < 4) return fail(FFMP_E_ARG, "%s: pose_now_stride %lld < 4", who, (long long)pose_now_stride);
  if (pose_prev_stride < 4) return fail(FFMP_E_ARG, "%s: pose_prev_stride %lld < 4", who, (long long)pose_prev_stride);
  const int64_t G2 = (int64_t)cfg->grid * cfg->grid;
  if (map_env_stride < G2)
    return fail(FFMP_E_ARG, "%s: map_env_stride %lld < G*G = %lld", who, (long long)map_env_stride, (long long)G2);
  if ((((uintptr_t)map_in | (uintptr_t)map_out) & 3u) != 0 || (map_env_stride % 4) != 0)
    return fail(FFMP_E_ARG, "%s: map planes must be 4-byte aligned with map_env_stride a multiple of 4 (map alignment)", who);
  if (frame_out) {
    if (frame_env_stride < G2)
      return fail(FFMP_E_ARG, "%s: frame_env_stride %lld < G*G = %lld", who, (long long)frame_env_stride, (long long)G2);
    const uintptr_t am = format == FFMP_OBS_F32 ? 15u : 3u;
    if (((uintptr_t)frame_out & am) != 0 || (frame_env_stride % 4) != 0)
      return fail(FFMP_E_ARG, "%s: frame_out must be %d-byte aligned with frame_env_stride a multiple of 4 elements (frame alignment)",
                  who, (int)am + 1);
  }
  const int64_t bpe = (G2 + kScanBlockCells - 1) / kScanBlockCells;
  if (n > 0x7fffffffLL || n * bpe > 0x7fffffffLL) return fail(FFMP_E_ARG, "%s: n too large for one launch: %lld", who, (long long)n);
  if (scan_planes_overlap(map_in, map_out, 1u, map_env_stride, G2, n))
    return fail(FFMP_E_ARG, "%s: the map_in and map_out planes overlap (they must lie G*G = %lld bytes apart)", who, (long long)G2);
  if (n == 0) return FFMP_OK;

  ScanMapArgs a;
  a.ranges = ranges;
  a.ranges_stride = ranges_stride;
  a.sectors = sectors;
  a.pose_now = pose_now;
  a.pose_now_stride = pose_now_stride;
  a.pose_prev = pose_prev;
  a.pose_prev_stride = pose_prev_stride;
  a.mask = mask;
  a.first = first;
  a.map_in = map_in;
  a.map_out = map_out;
  a.map_stride = map_env_stride;
  a.frame = frame_out;
  a.frame_stride = frame_env_stride;
  a.L = n_beams;
  a.bpe = (int32_t)bpe;
  a.unknown = unknown;
  a.plain = (flags & FFMP_SCAN_PLAIN) ? 1 : 0;
  a.th = thickness;
  a.mm = range_max * range_max;
  a.l_hit = l_hit;
  a.l_free = l_free;
  a.l_max = l_max;
  a.decay = decay;
  a.occ_thr = occ_thr;
  a.free_thr = free_thr;
  const int64_t blocks = n * bpe;
  hipStream_t s = (hipStream_t)stream;
  if (format == FFMP_OBS_F32)
    hipLaunchKernelGGL((scan_map_kernel<FFMP_OBS_F32>), dim3((unsigned)blocks), dim3(kScanThreads), 0, s, *cfg, a);
  else
    hipLaunchKernelGGL((scan_map_kernel<FFMP_OBS_U8F16>), dim3((unsigned)blocks), dim3(kScanThreads), 0, s, *cfg, a);
  return launch_ok(who);
}

}  // extern "C"
