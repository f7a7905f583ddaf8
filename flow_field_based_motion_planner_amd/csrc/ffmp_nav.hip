// ffmp_nav.hip — the navigation field of libffmp (include/ffmp.h ffmp_nav_field): per env, the
// cost-to-go from the goal over the traversable cells of the newest ego frame (integer chamfer 5-7
// costs), the direction per cell, and a follower that tracks the descent path from the robot cell.
// No reference counterpart.
//
// nav_field_kernel: one workgroup per env, everything in LDS —
//   cost   uint16 [G + 2][G + 2]  a halo of 65535 all round (no bounds checks on neighbour reads); the
//                                row stride is an odd number of dwords, so the lanes of a row sweep
//                                (lane = row, one column at a time) land on distinct banks
//   A, B, C  bit masks [G][ceil(G / 32)] words: occupancy -> zone ping-pong, hard, zone / soft
// G = 256: 130 KiB + 3 x 8 KiB of the CU's 160 KiB.
// Schedule: directional sweeps.  A pass is a row sweep (lane t walks row t left to right and back,
// relaxing every cell against all 8 neighbours in place) and a column sweep (lane t walks column t
// down and back); a corridor of any length along an axis is crossed in one pass.  Values only
// decrease and every stored value is the cost of a real path, so the unsynchronised 2-byte LDS
// updates inside a sweep are safe; the pass that changes nothing read only final values, which makes
// its plane the SPEC's unique fixed point.  The loop carries a hard bound of 2 G^2 passes.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <atomic>
#include <type_traits>

#include "ffmp.h"

#pragma clang fp contract(off)

namespace ffmp_detail {
int fail(int code, const char* fmt, ...);  // ffmp_kernels.hip (sets ffmp_last_error())
}
using ffmp_detail::fail;

namespace {

constexpr int kNavThreads = 256;
constexpr int kNavMaxGrid = 256;
constexpr size_t kNavLdsLimit = 159 * 1024;  // gfx950: 160 KiB of LDS per CU, all of it open to one workgroup; 1 KiB left for static LDS
constexpr uint32_t kInf = 65535u;

struct NavFoot {
  int16_t di[FFMP_MAX_FOOT], dj[FFMP_MAX_FOOT];
};

struct NavArgs {
  int32_t G, n_foot, margin, soft_pen, lookahead;
  int64_t env_stride, goal_stride;  // elements
  double half, res, dt, turn_sin;
  uint16_t* cost;
  uint8_t* dir;
  int32_t* target;
  int32_t* geo_cost;
  double* cmd;
};

size_t nav_lds_bytes(int G) {
  const size_t cost = (size_t)(G + 2) * (G + 2) * 2, mask = (size_t)G * ((G + 31) / 32) * 4;
  return ((cost + 15) & ~(size_t)15) + 3 * mask;
}

// bits [p, p + 32) of a mask row of `wpr` words; bits outside the row read 0
__device__ __forceinline__ uint32_t row_bits(const uint32_t* row, int wpr, int p) {
  const int w0 = p >> 5, sh = p & 31;
  const uint32_t lo = (w0 >= 0 && w0 < wpr) ? row[w0] : 0u;
  if (sh == 0) return lo;
  const uint32_t hi = (w0 + 1 >= 0 && w0 + 1 < wpr) ? row[w0 + 1] : 0u;
  return (lo >> sh) | (hi << (32 - sh));
}

__device__ __forceinline__ uint32_t mask_bit(const uint32_t* m, int wpr, int i, int j) {
  return (m[i * wpr + (j >> 5)] >> (j & 31)) & 1u;
}

// The SPEC's neighbour rule at a cell: the lowest k minimising d[a + k] + w_k over neighbours with
// d < 65535, diagonals only between two non-hard orthogonal cells.  c points at the cell in the cost
// plane, whose halo of 65535 stands for the cells outside the grid (so a neighbour outside never
// qualifies, whatever the h_* bit passed for it).  Returns the minimum (0x7fffffff: no neighbour
// qualifies) and k through *kbest.  All nine loads are independent: one LDS round trip.
__device__ __forceinline__ int32_t best_of(const uint16_t* c, int S, uint32_t h_up, uint32_t h_dn, uint32_t h_rt,
                                           uint32_t h_lf, int* kbest) {
  const uint32_t d0 = c[S], d1 = c[-S], d2 = c[1], d3 = c[-1], d4 = c[S + 1], d5 = c[S - 1], d6 = c[-S + 1], d7 = c[-S - 1];
  int32_t best = 0x7fffffff;
  int kb = -1;
  auto take = [&](uint32_t d, int32_t w, int k, bool allowed) {
    const int32_t v = (int32_t)d + w;
    if (allowed && d < kInf && v < best) {
      best = v;
      kb = k;
    }
  };
  take(d0, 5, 0, true);
  take(d1, 5, 1, true);
  take(d2, 5, 2, true);
  take(d3, 5, 3, true);
  take(d4, 7, 4, !(h_up | h_rt));
  take(d5, 7, 5, !(h_up | h_lf));
  take(d6, 7, 6, !(h_dn | h_rt));
  take(d7, 7, 7, !(h_dn | h_lf));
  *kbest = kb;
  return best;
}

// the same at cell (i, j), the hard bits read from the mask (rows / columns outside the grid: any value)
__device__ __forceinline__ int32_t best_neighbour(const uint16_t* cost, const uint32_t* hard, int G, int S, int wpr,
                                                  int i, int j, int* kbest) {
  const uint32_t h_up = i + 1 < G ? mask_bit(hard, wpr, i + 1, j) : 1u, h_dn = i > 0 ? mask_bit(hard, wpr, i - 1, j) : 1u;
  const uint32_t h_rt = j + 1 < G ? mask_bit(hard, wpr, i, j + 1) : 1u, h_lf = j > 0 ? mask_bit(hard, wpr, i, j - 1) : 1u;
  return best_of(cost + (i + 1) * S + (j + 1), S, h_up, h_dn, h_rt, h_lf, kbest);
}

// One relaxation of a non-hard, non-goal cell; 1 if its cost went down.  Only the minimum is needed
// here, not its k: a neighbour at 65535 gives a candidate >= 65540, which the cap rejects, so the
// "d < 65535" test of the rule is implied.  x4..x7: the diagonal k is forbidden (a hard orthogonal cell).
__device__ __forceinline__ int relax(uint16_t* c, int S, uint32_t x4, uint32_t x5, uint32_t x6, uint32_t x7,
                                     uint32_t is_soft, int32_t soft_pen) {
  const uint32_t d0 = c[S], d1 = c[-S], d2 = c[1], d3 = c[-1], d4 = c[S + 1], d5 = c[S - 1], d6 = c[-S + 1], d7 = c[-S - 1];
  const uint32_t cur = c[0];
  const uint32_t orth = min(min(d0, d1), min(d2, d3));
  const uint32_t diag = min(min(x4 ? kInf : d4, x5 ? kInf : d5), min(x6 ? kInf : d6, x7 ? kInf : d7));
  const uint32_t v = min(orth + 5u, diag + 7u) + (is_soft ? (uint32_t)soft_pen : 0u);
  if (v > 65534u || v >= cur) return 0;
  c[0] = (uint16_t)v;
  return 1;
}

__device__ __forceinline__ uint32_t occupied4(const float4 v) {
  return (v.x > 0.0f ? 1u : 0u) | (v.y > 0.0f ? 2u : 0u) | (v.z > 0.0f ? 4u : 0u) | (v.w > 0.0f ? 8u : 0u);
}
__device__ __forceinline__ uint32_t occupied4(const uint32_t v) {
  return ((v & 0xffu) ? 1u : 0u) | ((v & 0xff00u) ? 2u : 0u) | ((v & 0xff0000u) ? 4u : 0u) | ((v & 0xff000000u) ? 8u : 0u);
}

template <typename T, bool VEC>
__global__ __launch_bounds__(kNavThreads) void nav_field_kernel(NavArgs a, NavFoot foot, const T* __restrict__ newest,
                                                                const float* __restrict__ goal_ego) {
  extern __shared__ __attribute__((aligned(16))) unsigned char nav_lds[];
  const int G = a.G, S = G + 2, wpr = (G + 31) >> 5, G2 = G * G, words = G * wpr;
  const int tid = threadIdx.x;
  const int64_t e = blockIdx.x;
  uint16_t* cost = reinterpret_cast<uint16_t*>(nav_lds);
  uint32_t* A = reinterpret_cast<uint32_t*>(nav_lds + (((size_t)(G + 2) * S * 2 + 15) & ~(size_t)15));
  uint32_t* B = A + words;  // hard
  uint32_t* Cm = B + words;
  const int ci = G / 2, cj = G / 2;

  // the goal cell, float64, rint half-to-even
  const double gx = (double)goal_ego[e * a.goal_stride + 0], gy = (double)goal_ego[e * a.goal_stride + 1];
  const bool finite = (gx - gx == 0.0) && (gy - gy == 0.0);
  uint16_t* gcost = a.cost ? a.cost + e * G2 : nullptr;
  uint8_t* gdir = a.dir ? a.dir + e * G2 : nullptr;
  if (!finite) {  // unreachable by definition: nothing is read, every output says so
    for (int c4 = tid; c4 < G2 / 4; c4 += kNavThreads) {
      if (gcost) reinterpret_cast<uint2*>(gcost)[c4] = make_uint2(0xffffffffu, 0xffffffffu);
      if (gdir) reinterpret_cast<uint32_t*>(gdir)[c4] = 0xffffffffu;
    }
    if (tid == 0) {
      if (a.geo_cost) a.geo_cost[e] = -1;
      if (a.target) { a.target[e * 2] = 0; a.target[e * 2 + 1] = 0; }
      if (a.cmd) reinterpret_cast<double2*>(a.cmd)[e] = make_double2(0.0, 0.0);
    }
    return;
  }
  double qx = rint((gx + a.half) / a.res), qy = rint((gy + a.half) / a.res);
  qx = qx < 0.0 ? 0.0 : (qx > (double)(G - 1) ? (double)(G - 1) : qx);
  qy = qy < 0.0 ? 0.0 : (qy > (double)(G - 1) ? (double)(G - 1) : qy);
  const int qi = (int)qx, qj = (int)qy;

  // 0. clear the occupancy mask, cost := 65535 everywhere (the halo too)
  for (int w = tid; w < words; w += kNavThreads) A[w] = 0u;
  for (int w = tid; w < (G + 2) * S / 2; w += kNavThreads) reinterpret_cast<uint32_t*>(cost)[w] = 0xffffffffu;
  __syncthreads();

  // 1. the newest frame, once: 4 cells (one row, one mask word: G % 4 == 0) per OR into the mask
  const T* f = newest + e * a.env_stride;
  constexpr int CH = VEC ? 16 / (int)sizeof(T) : 4;  // cells per load
  for (int c = tid; c < G2 / CH; c += kNavThreads) {
    uint32_t nib[CH / 4];
    if constexpr (std::is_same<T, float>::value) {
      if constexpr (VEC) {
        nib[0] = occupied4(reinterpret_cast<const float4*>(f)[c]);
      } else {
        nib[0] = occupied4(make_float4(f[c * 4], f[c * 4 + 1], f[c * 4 + 2], f[c * 4 + 3]));
      }
    } else {
      if constexpr (VEC) {
        const uint4 v = reinterpret_cast<const uint4*>(f)[c];
        nib[0] = occupied4(v.x); nib[1] = occupied4(v.y); nib[2] = occupied4(v.z); nib[3] = occupied4(v.w);
      } else {
        nib[0] = (f[c * 4] ? 1u : 0u) | (f[c * 4 + 1] ? 2u : 0u) | (f[c * 4 + 2] ? 4u : 0u) | (f[c * 4 + 3] ? 8u : 0u);
      }
    }
#pragma unroll
    for (int q4 = 0; q4 < CH / 4; ++q4) {
      if (nib[q4]) {
        const int idx = c * CH + q4 * 4, i = idx / G, j = idx - i * G;
        atomicOr(&A[i * wpr + (j >> 5)], nib[q4] << (j & 31));
      }
    }
  }
  __syncthreads();

  // 2. hard = occupancy gathered over the footprint offsets, a word (32 cells of a row) at a time
  for (int w = tid; w < words; w += kNavThreads) {
    const int i = w / wpr, wj = w - i * wpr;
    const int left = G - wj * 32;  // cells of the row from this word on
    const uint32_t valid = left >= 32 ? 0xffffffffu : ((1u << left) - 1u);
    uint32_t h = 0u;
    for (int k = 0; k < a.n_foot; ++k) {
      const int ii = i + foot.di[k];
      if (ii >= 0 && ii < G) h |= row_bits(A + ii * wpr, wpr, wj * 32 + foot.dj[k]);
    }
    B[w] = h & valid;
  }
  __syncthreads();
  // 3. zone = hard dilated `margin` times by the 3 x 3 neighbourhood (A and Cm ping-pong)
  for (int w = tid; w < words; w += kNavThreads) A[w] = B[w];
  __syncthreads();
  uint32_t* zone = A;
  for (int m = 0; m < a.margin; ++m) {
    uint32_t* dst = zone == A ? Cm : A;
    for (int w = tid; w < words; w += kNavThreads) {
      const int i = w / wpr, wj = w - i * wpr;
      const int left = G - wj * 32;
      const uint32_t valid = left >= 32 ? 0xffffffffu : ((1u << left) - 1u);
      uint32_t z = 0u;
      for (int ii = (i > 0 ? i - 1 : 0); ii <= (i + 1 < G ? i + 1 : G - 1); ++ii) {
        const uint32_t* row = zone + ii * wpr;
        z |= row_bits(row, wpr, wj * 32 - 1) | row[wj] | row_bits(row, wpr, wj * 32 + 1);
      }
      dst[w] = z & valid;
    }
    __syncthreads();
    zone = dst;
  }
  // 4. the robot cell and the goal cell are traversable; soft = zone & ~hard (a cleared cell is soft)
  if (tid == 0) {
    B[ci * wpr + (cj >> 5)] &= ~(1u << (cj & 31));
    B[qi * wpr + (qj >> 5)] &= ~(1u << (qj & 31));
    cost[(qi + 1) * S + (qj + 1)] = 0;
  }
  __syncthreads();
  uint32_t* soft = zone;
  for (int w = tid; w < words; w += kNavThreads) soft[w] &= ~B[w];
  __syncthreads();

  // 5. relax to the fixed point: row sweeps, then column sweeps, until a pass changes nothing.
  // Lane t owns row t, then column t.  Per mask word: H0 / Hp / Hm = the hard bits of the row and of
  // the rows above and below, Hrt / Hlf = H0 moved by one cell; a diagonal is forbidden where either
  // of its two orthogonal cells is hard (bits for cells outside the grid: any value, the halo decides).
  const int max_pass = 2 * G2;
  const int32_t pen = a.soft_pen;
  for (int pass = 0; pass < max_pass; ++pass) {
    int changed = 0;
    if (tid < G) {
      const int i = tid;
      const uint32_t* Bi = B + i * wpr;
      uint16_t* crow = cost + (i + 1) * S + 1;
      for (int dirn = 0; dirn < 2; ++dirn) {
        for (int ww = 0; ww < wpr; ++ww) {
          const int w = dirn ? wpr - 1 - ww : ww;
          const uint32_t H0 = Bi[w], S0 = soft[i * wpr + w];
          const uint32_t Hp = i + 1 < G ? Bi[w + wpr] : 0xffffffffu, Hm = i > 0 ? Bi[w - wpr] : 0xffffffffu;
          const uint32_t Hrt = (H0 >> 1) | ((w + 1 < wpr ? Bi[w + 1] : 1u) << 31), Hlf = (H0 << 1) | (w > 0 ? Bi[w - 1] >> 31 : 1u);
          const uint32_t X4 = Hp | Hrt, X5 = Hp | Hlf, X6 = Hm | Hrt, X7 = Hm | Hlf;
          uint32_t todo = ~H0;  // the non-hard cells of this word
          const int nb = G - w * 32 < 32 ? G - w * 32 : 32;
          if (nb < 32) todo &= (1u << nb) - 1u;
          if (i == qi && (qj >> 5) == w) todo &= ~(1u << (qj & 31));
          for (int bb = 0; bb < nb; ++bb) {
            const int b = dirn ? nb - 1 - bb : bb;
            if (!((todo >> b) & 1u)) continue;
            changed |= relax(crow + w * 32 + b, S, (X4 >> b) & 1u, (X5 >> b) & 1u, (X6 >> b) & 1u, (X7 >> b) & 1u, (S0 >> b) & 1u, pen);
          }
        }
      }
    }
    __syncthreads();
    if (tid < G) {
      const int j = tid, w = j >> 5, b = j & 31;
      for (int dirn = 0; dirn < 2; ++dirn) {
        for (int ii = 0; ii < G; ++ii) {
          const int i = dirn ? G - 1 - ii : ii;
          const uint32_t* Bi = B + i * wpr;
          const uint32_t H0 = Bi[w], S0 = soft[i * wpr + w];
          if (((H0 >> b) & 1u) || (i == qi && j == qj)) continue;
          const uint32_t h_up = i + 1 < G ? (Bi[w + wpr] >> b) & 1u : 1u, h_dn = i > 0 ? (Bi[w - wpr] >> b) & 1u : 1u;
          const uint32_t h_rt = b < 31 ? (H0 >> (b + 1)) & 1u : (w + 1 < wpr ? Bi[w + 1] & 1u : 1u);
          const uint32_t h_lf = b > 0 ? (H0 >> (b - 1)) & 1u : (w > 0 ? Bi[w - 1] >> 31 : 1u);
          changed |= relax(cost + (i + 1) * S + (j + 1), S, h_up | h_rt, h_up | h_lf, h_dn | h_rt, h_dn | h_lf, (S0 >> b) & 1u, pen);
        }
      }
    }
    if (!__syncthreads_or(changed)) break;
  }

  // 6. the planes: 4 cells per store
  if (gcost || gdir) {
    for (int c4 = tid; c4 < G2 / 4; c4 += kNavThreads) {
      const int idx = c4 * 4, i = idx / G, j0 = idx - i * G;
      uint32_t d[4], k8[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int j = j0 + u;
        d[u] = cost[(i + 1) * S + (j + 1)];
        int k = -1;
        if (d[u] < kInf && !(i == qi && j == qj)) best_neighbour(cost, B, G, S, wpr, i, j, &k);
        k8[u] = d[u] == kInf ? 255u : ((i == qi && j == qj) ? 8u : (uint32_t)(k & 0xff));
      }
      if (gcost) reinterpret_cast<uint2*>(gcost)[c4] = make_uint2(d[0] | (d[1] << 16), d[2] | (d[3] << 16));
      if (gdir) reinterpret_cast<uint32_t*>(gdir)[c4] = k8[0] | (k8[1] << 8) | (k8[2] << 16) | (k8[3] << 24);
    }
  }

  // 7. one lane: the descent from the robot cell and the follower
  if (tid == 0) {
    const uint32_t dc = cost[(ci + 1) * S + (cj + 1)];
    int ti = ci, tj = cj;
    if (dc < kInf) {
      for (int s = 0; s < a.lookahead; ++s) {
        if (ti == qi && tj == qj) break;
        int k;
        best_neighbour(cost, B, G, S, wpr, ti, tj, &k);
        if (k < 0) break;
        ti += (k == 0 || k == 4 || k == 5) ? 1 : ((k == 2 || k == 3) ? 0 : -1);
        tj += (k == 2 || k == 4 || k == 6) ? 1 : ((k == 0 || k == 1) ? 0 : -1);
      }
    }
    const int tx = ti - ci, ty = tj - cj;
    if (a.geo_cost) a.geo_cost[e] = dc < kInf ? (int32_t)dc : -1;
    if (a.target) { a.target[e * 2] = tx; a.target[e * 2 + 1] = ty; }
    if (a.cmd) {
      const double dx = (double)tx, dy = (double)ty;
      const double m2 = dx * dx + dy * dy;
      double v = 0.0, w = 0.0;
      if (m2 != 0.0) {
        const double m = sqrt(m2);
        const double ux = dx / m, uy = dy / m;
        w = uy / a.dt;
        w = w < -0.6 ? -0.6 : (w > 0.6 ? 0.6 : w);
        if (ux < 0.0) w = uy >= 0.0 ? 0.6 : -0.6;
        v = 0.6 * (ux > 0.0 ? ux : 0.0);
        if (fabs(uy) > a.turn_sin) v = 0.0;
      }
      reinterpret_cast<double2*>(a.cmd)[e] = make_double2(v, w);
    }
  }
}

// every check that needs no pointer: the shape, the knobs and the LDS budget
int nav_check(const ffmp_cfg_t* cfg, int32_t format, int32_t margin, int32_t soft_pen, int32_t lookahead) {
  if (!cfg) return fail(FFMP_E_ARG, "cfg is NULL");
  if (cfg->grid < 8 || cfg->grid > kNavMaxGrid || (cfg->grid % 4) != 0)
    return fail(FFMP_E_ARG, "ffmp_nav_field: grid must be a multiple of 4 in [8,%d] (one workgroup holds the whole "
                "plane in LDS), got %d", kNavMaxGrid, cfg->grid);
  if (cfg->n_foot < 0 || cfg->n_foot > FFMP_MAX_FOOT) return fail(FFMP_E_ARG, "ffmp_nav_field: n_foot out of range: %d", cfg->n_foot);
  for (int f = 0; f < cfg->n_foot; ++f)
    if (cfg->foot_di[f] < -cfg->grid || cfg->foot_di[f] > cfg->grid || cfg->foot_dj[f] < -cfg->grid || cfg->foot_dj[f] > cfg->grid)
      return fail(FFMP_E_ARG, "ffmp_nav_field: footprint offset %d outside the grid", f);
  if (format != FFMP_OBS_F32 && format != FFMP_OBS_U8F16) return fail(FFMP_E_ARG, "ffmp_nav_field: unknown obs format %d", format);
  if (margin < 0 || margin > 8) return fail(FFMP_E_ARG, "ffmp_nav_field: margin must be in 0..8, got %d", margin);
  if (soft_pen < 0 || soft_pen > 16384) return fail(FFMP_E_ARG, "ffmp_nav_field: soft_pen must be in 0..16384, got %d", soft_pen);
  if (lookahead < 1 || lookahead > 64) return fail(FFMP_E_ARG, "ffmp_nav_field: lookahead must be in 1..64, got %d", lookahead);
  if (nav_lds_bytes(cfg->grid) > kNavLdsLimit)
    return fail(FFMP_E_ARG, "ffmp_nav_field: grid %d needs %zu bytes of LDS", cfg->grid, nav_lds_bytes(cfg->grid));
  return FFMP_OK;
}

template <typename T>
int nav_launch(const NavArgs& a, const NavFoot& foot, int64_t n, const T* newest, const float* goal, bool vec, size_t lds,
               hipStream_t s) {
  auto k = vec ? nav_field_kernel<T, true> : nav_field_kernel<T, false>;
  if (lds > 64 * 1024) {
    // more than the default cap of dynamic LDS: ask for it, once per device and kernel (an attribute
    // of the function, no stream work)
    static std::atomic<uint64_t> asked[2];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return fail(FFMP_E_HIP, "ffmp_nav_field: hipGetDevice failed");
    const uint64_t bit = 1ull << (dev & 63);
    if (!(asked[vec].load() & bit)) {
      hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      if (err != hipSuccess)
        return fail(FFMP_E_HIP, "ffmp_nav_field: hipFuncSetAttribute(%zu bytes of LDS): %s", lds, hipGetErrorString(err));
      asked[vec].fetch_or(bit);
    }
  }
  hipLaunchKernelGGL(k, dim3((unsigned)n), dim3(kNavThreads), lds, s, a, foot, newest, goal);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return fail(FFMP_E_HIP, "ffmp_nav_field: HIP launch failed: %s", hipGetErrorString(err));
  return FFMP_OK;
}

}  // namespace

extern "C" {

int ffmp_nav_field_check(const ffmp_cfg_t* cfg, int32_t format, int32_t margin, int32_t soft_pen, int32_t lookahead) {
  return nav_check(cfg, format, margin, soft_pen, lookahead);
}

int ffmp_nav_field(const ffmp_cfg_t* cfg, int64_t n, const ffmp_obs_t* obs, const float* goal_ego, int64_t goal_stride,
                   int32_t margin, int32_t soft_pen, int32_t lookahead, double turn_sin, uint16_t* cost, uint8_t* dir,
                   int32_t* target, int32_t* geo_cost, double* cmd, void* stream) {
  if (!obs) return fail(FFMP_E_ARG, "ffmp_nav_field: obs is NULL");
  int rc = nav_check(cfg, obs->format, margin, soft_pen, lookahead);
  if (rc) return rc;
  if (!(turn_sin >= 0.0)) return fail(FFMP_E_ARG, "ffmp_nav_field: turn_sin must be >= 0 and not NaN");
  if (n < 0) return fail(FFMP_E_ARG, "ffmp_nav_field: negative n");
  if (!obs->state_m) return fail(FFMP_E_ARG, "ffmp_nav_field: obs.state_m is NULL");
  if (!goal_ego) return fail(FFMP_E_ARG, "ffmp_nav_field: goal_ego is NULL");
  if (goal_stride < 2) return fail(FFMP_E_ARG, "ffmp_nav_field: goal_stride must be >= 2, got %lld", (long long)goal_stride);
  if (((uintptr_t)cmd & 15u) != 0) return fail(FFMP_E_ARG, "ffmp_nav_field: cmd must be 16-byte aligned");
  if (((uintptr_t)cost & 7u) != 0) return fail(FFMP_E_ARG, "ffmp_nav_field: cost must be 8-byte aligned");
  if (((uintptr_t)dir & 3u) != 0) return fail(FFMP_E_ARG, "ffmp_nav_field: dir must be 4-byte aligned");
  if (n == 0) return FFMP_OK;
  if (n > 0x7fffffffLL) return fail(FFMP_E_ARG, "ffmp_nav_field: n too large for one launch: %lld", (long long)n);
  const int G = cfg->grid;
  const int64_t G2 = (int64_t)G * G;
  NavArgs a;
  a.G = G;
  a.n_foot = cfg->n_foot;
  a.margin = margin;
  a.soft_pen = soft_pen;
  a.lookahead = lookahead;
  a.env_stride = obs->state_m_stride ? obs->state_m_stride : 2 * G2;
  a.goal_stride = goal_stride;
  a.half = (double)cfg->half_f;
  a.res = (double)cfg->res_f;
  a.dt = cfg->dt;
  a.turn_sin = turn_sin;
  a.cost = cost;
  a.dir = dir;
  a.target = target;
  a.geo_cost = geo_cost;
  a.cmd = cmd;
  NavFoot foot;
  for (int f = 0; f < FFMP_MAX_FOOT; ++f) {
    foot.di[f] = f < cfg->n_foot ? (int16_t)cfg->foot_di[f] : 0;
    foot.dj[f] = f < cfg->n_foot ? (int16_t)cfg->foot_dj[f] : 0;
  }
  const int64_t frame = obs->state_m_frame_stride ? obs->state_m_frame_stride : G2;
  const size_t lds = nav_lds_bytes(G);
  hipStream_t s = (hipStream_t)stream;
  if (obs->format == FFMP_OBS_F32) {
    const float* newest = obs->state_m + frame;
    const bool vec = ((uintptr_t)newest & 15u) == 0 && ((a.env_stride * 4) & 15) == 0;
    return nav_launch<float>(a, foot, n, newest, goal_ego, vec, lds, s);
  }
  const uint8_t* newest = reinterpret_cast<const uint8_t*>(obs->state_m) + frame;
  const bool vec = ((uintptr_t)newest & 15u) == 0 && (a.env_stride & 15) == 0;
  return nav_launch<uint8_t>(a, foot, n, newest, goal_ego, vec, lds, s);
}

}  // extern "C"
