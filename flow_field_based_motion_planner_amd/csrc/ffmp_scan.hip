// ffmp_scan.hip — occupancy frames built from the lidar scan: the inverse sensor model
// (include/ffmp.h ffmp_scan_frames carries the SPEC).
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

#pragma clang fp contract(off)

namespace ffmp_detail {
int fail(int code, const char* fmt, ...);  // ffmp_kernels.hip (sets ffmp_last_error())
}
using ffmp_detail::fail;

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

int scan_check(const ffmp_cfg_t* cfg, int32_t n_beams, int32_t format, int32_t unknown, float thickness, float range_max,
               int32_t flags) {
  const char* who = "ffmp_scan_frames";
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

}  // namespace

extern "C" {

int ffmp_scan_frames_check(const ffmp_cfg_t* cfg, int32_t n_beams, int32_t format, int32_t unknown, float thickness,
                           float range_max, int32_t flags) {
  return scan_check(cfg, n_beams, format, unknown, thickness, range_max, flags);
}

int ffmp_scan_frames(const ffmp_cfg_t* cfg, int64_t n, const float* ranges, int64_t ranges_stride, int32_t n_beams,
                     const float* sectors, const uint8_t* mask, const uint8_t* first, void* out_older, void* out_newest,
                     int64_t out_env_stride, int32_t format, int32_t unknown, float thickness, float range_max,
                     int32_t flags, void* stream) {
  const char* who = "ffmp_scan_frames";
  if (int rc = scan_check(cfg, n_beams, format, unknown, thickness, range_max, flags)) return rc;
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
    // plane e of one frame against plane e' of the other: they overlap iff |d + (e - e') S| < G*G
    const uintptr_t po = (uintptr_t)out_older, pn = (uintptr_t)out_newest;
    const uint64_t es = format == FFMP_OBS_F32 ? 4u : 1u;
    const uint64_t d = (po > pn ? po - pn : pn - po) / es, S = (uint64_t)out_env_stride;
    const uint64_t k = d / S, r = d - k * S, last = n > 0 ? (uint64_t)(n - 1) : 0u;
    if (d < (uint64_t)G2 || (k <= last && r < (uint64_t)G2) || (k + 1 <= last && S - r < (uint64_t)G2))
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
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return fail(FFMP_E_HIP, "%s: HIP launch failed: %s", who, hipGetErrorString(err));
  return FFMP_OK;
}

}  // extern "C"
