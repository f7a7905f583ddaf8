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
//
// nav_field_tiled_kernel (ffmp_nav_field_tiled, grids up to 512 x 512): the same field with the cost
// plane in global memory and T x T tiles of it taken through LDS, one workgroup per env at a time on
// a persistent grid of `slots` workgroups (workgroup b plans envs b, b + slots, ...), each with a
// workspace slot of its own; no workgroup ever waits on another.
//   phase A  the cell classes of the whole grid in LDS (the same three masks, the same steps), then
//            hard and soft to the slot, the plane := 65535, d[q] := 0
//   phase B  a dirty bit per tile in LDS, at first only q's tile.  A dirty tile is loaded with a
//            one-cell halo (cost [T + 2][T + 2], the same odd dword row stride; hard / soft
//            [T + 2][T / 32 + 2] words: the mask words left and right of the tile carry the halo
//            columns; outside the grid: 65535 and hard), swept as above over its interior until a
//            pass changes nothing, and, if anything changed, written back; the neighbours that see a
//            changed border cell (edge rows / columns, corner cells) become dirty.  Halo cells are
//            read, never relaxed.  T = 256: 130 KiB + 2 x 10 KiB.  At exit every tile is at its
//            fixed point against final halos and every value is the cost of a real path: the plane
//            is the SPEC's fixed point.  Hard bounds: 2 G^2 tile visits, 4 G^2 passes in all.
//   phase C  dir from one more pass over the tiles; one lane descends on the global plane.
// The workgroup's own global stores are made visible to its later loads by a workgroup-scope fence
// with the barrier (one CU, one vector L1); the plane is never read through const / restrict.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <atomic>
#include <mutex>
#include <type_traits>
#include <vector>

#include "ffmp_host.h"

#pragma clang fp contract(off)

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
__device__ __forceinline__ int32_t best_pick(uint32_t d0, uint32_t d1, uint32_t d2, uint32_t d3, uint32_t d4, uint32_t d5,
                                             uint32_t d6, uint32_t d7, uint32_t h_up, uint32_t h_dn, uint32_t h_rt,
                                             uint32_t h_lf, int* kbest) {
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

__device__ __forceinline__ int32_t best_of(const uint16_t* c, int S, uint32_t h_up, uint32_t h_dn, uint32_t h_rt,
                                           uint32_t h_lf, int* kbest) {
  const uint32_t d0 = c[S], d1 = c[-S], d2 = c[1], d3 = c[-1], d4 = c[S + 1], d5 = c[S - 1], d6 = c[-S + 1], d7 = c[-S - 1];
  return best_pick(d0, d1, d2, d3, d4, d5, d6, d7, h_up, h_dn, h_rt, h_lf, kbest);
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

// The goal cell of env e (float64, rint half-to-even, clamped per axis); false for a non-finite goal.
__device__ __forceinline__ bool goal_cell(const NavArgs& a, const float* goal_ego, int64_t e, int* qi, int* qj) {
  const int G = a.G;
  const double gx = (double)goal_ego[e * a.goal_stride + 0], gy = (double)goal_ego[e * a.goal_stride + 1];
  if (!((gx - gx == 0.0) && (gy - gy == 0.0))) return false;
  double qx = rint((gx + a.half) / a.res), qy = rint((gy + a.half) / a.res);
  qx = qx < 0.0 ? 0.0 : (qx > (double)(G - 1) ? (double)(G - 1) : qx);
  qy = qy < 0.0 ? 0.0 : (qy > (double)(G - 1) ? (double)(G - 1) : qy);
  *qi = (int)qx;
  *qj = (int)qy;
  return true;
}

// A non-finite goal: unreachable by definition, nothing is read, every output says so.
__device__ __forceinline__ void unreachable_outputs(const NavArgs& a, int64_t e, uint16_t* gcost, uint8_t* gdir, int tid) {
  const int G2 = a.G * a.G;
  for (int c4 = tid; c4 < G2 / 4; c4 += kNavThreads) {
    if (gcost) reinterpret_cast<uint2*>(gcost)[c4] = make_uint2(0xffffffffu, 0xffffffffu);
    if (gdir) reinterpret_cast<uint32_t*>(gdir)[c4] = 0xffffffffu;
  }
  if (tid == 0) {
    if (a.geo_cost) a.geo_cost[e] = -1;
    if (a.target) { a.target[e * 2] = 0; a.target[e * 2 + 1] = 0; }
    if (a.cmd) reinterpret_cast<double2*>(a.cmd)[e] = make_double2(0.0, 0.0);
  }
}

// One lane: geo_cost, target and the follower from the cost at the robot cell and the cell reached.
__device__ __forceinline__ void robot_outputs(const NavArgs& a, int64_t e, uint32_t dc, int tx, int ty) {
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

__device__ __forceinline__ void descent_move(int k, int* ti, int* tj) {
  *ti += (k == 0 || k == 4 || k == 5) ? 1 : ((k == 2 || k == 3) ? 0 : -1);
  *tj += (k == 2 || k == 4 || k == 6) ? 1 : ((k == 0 || k == 1) ? 0 : -1);
}

// Steps 0-4 of the field, the cell classes of the whole grid in the three LDS masks A, B, Cm of
// G x wpr words: B = hard (robot and goal cell cleared), the returned mask (A or Cm) = soft.  The
// caller's own LDS initialisation before the call is covered by the first barrier in here; cost_q,
// if given, is the goal's cell of an LDS cost plane, set to 0 with the clearing of step 4.
template <typename T, bool VEC>
__device__ __forceinline__ uint32_t* build_classes(const NavArgs& a, const NavFoot& foot, const T* f, uint32_t* A, uint32_t* B,
                                                   uint32_t* Cm, int qi, int qj, uint16_t* cost_q) {
  const int G = a.G, wpr = (G + 31) >> 5, G2 = G * G, words = G * wpr;
  const int tid = threadIdx.x;
  const int ci = G / 2, cj = G / 2;
  // 0. clear the occupancy mask
  for (int w = tid; w < words; w += kNavThreads) A[w] = 0u;
  __syncthreads();

  // 1. the newest frame, once: 4 cells (one row, one mask word: G % 4 == 0) per OR into the mask
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
    if (cost_q) *cost_q = 0;
  }
  __syncthreads();
  uint32_t* soft = zone;
  for (int w = tid; w < words; w += kNavThreads) soft[w] &= ~B[w];
  __syncthreads();
  return soft;
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

  uint16_t* gcost = a.cost ? a.cost + e * G2 : nullptr;
  uint8_t* gdir = a.dir ? a.dir + e * G2 : nullptr;
  int qi, qj;
  if (!goal_cell(a, goal_ego, e, &qi, &qj)) {
    unreachable_outputs(a, e, gcost, gdir, tid);
    return;
  }

  // cost := 65535 everywhere (the halo too), then steps 0-4: the cell classes, cost[q] := 0
  for (int w = tid; w < (G + 2) * S / 2; w += kNavThreads) reinterpret_cast<uint32_t*>(cost)[w] = 0xffffffffu;
  uint32_t* soft = build_classes<T, VEC>(a, foot, newest + e * a.env_stride, A, B, Cm, qi, qj, cost + (qi + 1) * S + (qj + 1));

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
        descent_move(k, &ti, &tj);
      }
    }
    robot_outputs(a, e, dc, ti - ci, tj - cj);
  }
}

// ------------------------------------------------------------------ the tiled kernel
constexpr int kNavTiledMaxGrid = 512;
constexpr int kNavTileDefault = 256;
constexpr int kNavMaxTiles = 256;  // (512 / 32)^2: one dirty bit each, 8 words
constexpr int kNavSlotCap = 2048;  // 256 CUs x 8 workgroups of 4 waves
enum : uint32_t {  // what a write-back changed, as its neighbours see it: edge rows / columns and corner cells
  kChgIm = 1u, kChgIp = 2u, kChgJm = 4u, kChgJp = 8u, kChgMM = 16u, kChgMP = 32u, kChgPM = 64u, kChgPP = 128u
};

struct NavTiledArgs {
  int32_t T;             // tile edge, a multiple of 32
  int64_t n;             // envs
  unsigned char* ws;     // workspace: gridDim.x slots
  size_t slot_bytes;     // per slot: hard mask, soft mask, then the plane unless the caller gives cost
  size_t plane_off;      // offset of the slot's plane
};

size_t nav_tiled_mask_bytes(int G) { return (((size_t)G * ((G + 31) / 32) * 4 * 2) + 255) & ~(size_t)255; }
size_t nav_tiled_slot_bytes(int G, bool with_cost) {
  return nav_tiled_mask_bytes(G) + (with_cost ? 0 : ((size_t)G * G * 2 + 255) & ~(size_t)255);
}
// the tile edge in use: no larger than the grid rounded up to mask words
int nav_tile_edge(int G, int tile) {
  const int T = tile ? tile : kNavTileDefault, cover = (G + 31) & ~31;
  return T < cover ? T : cover;
}
size_t nav_tiled_lds_bytes(int G, int T) {
  const size_t phase_a = (size_t)3 * G * ((G + 31) / 32) * 4;
  const size_t cost = (((size_t)(T + 2) * (T + 2) * 2) + 15) & ~(size_t)15;
  const size_t phase_b = cost + (size_t)2 * (T + 2) * (T / 32 + 2) * 4;
  return phase_a > phase_b ? phase_a : phase_b;
}

struct NavTile {
  int i0, j0, R, Cn;  // origin, rows, columns (the last row / column of tiles may be ragged; Cn % 4 == 0)
};

__device__ __forceinline__ NavTile nav_tile(int t, int ntj, int T, int G) {
  NavTile tl;
  const int ti = t / ntj, tj = t - ti * ntj;
  tl.i0 = ti * T;
  tl.j0 = tj * T;
  tl.R = G - tl.i0 < T ? G - tl.i0 : T;
  tl.Cn = G - tl.j0 < T ? G - tl.j0 : T;
  return tl;
}

// A tile of the global plane into LDS with its one-cell halo: lc points at the halo's corner (cell
// (r, c) of the tile at lc[(r + 1) * S + c + 1]), Ht / St at word (row 0, word 0) of the tile's
// hard / soft masks (row stride wprT; rows -1 .. R, words -1 .. ceil(Cn / 32): the halo columns are
// bit 31 of word -1 and bit 0 of the word past the tile).  Outside the grid: 65535 and hard.
__device__ __forceinline__ void tile_load(uint16_t* plane, uint32_t* ghard, uint32_t* gsoft, int G, int wpr, const NavTile& tl,
                                          uint16_t* lc, int S, uint32_t* Ht, uint32_t* St, int wprT) {
  const int tid = threadIdx.x;
  const int c4n = tl.Cn >> 2;
  for (int idx = tid; idx < tl.R * c4n; idx += kNavThreads) {
    const int r = idx / c4n, c = (idx - r * c4n) * 4;
    const uint2 v = *reinterpret_cast<uint2*>(plane + (size_t)(tl.i0 + r) * G + tl.j0 + c);
    uint16_t* l = lc + (r + 1) * S + c + 1;
    l[0] = (uint16_t)(v.x & 0xffffu);
    l[1] = (uint16_t)(v.x >> 16);
    l[2] = (uint16_t)(v.y & 0xffffu);
    l[3] = (uint16_t)(v.y >> 16);
  }
  const int across = tl.Cn + 2;  // rows -1 and R with their corners, then columns -1 and Cn
  for (int idx = tid; idx < 2 * across + 2 * tl.R; idx += kNavThreads) {
    int r, c;
    if (idx < 2 * across) {
      r = idx < across ? -1 : tl.R;
      c = (idx < across ? idx : idx - across) - 1;
    } else {
      const int k = idx - 2 * across;
      r = k >> 1;
      c = (k & 1) ? tl.Cn : -1;
    }
    const int gi = tl.i0 + r, gj = tl.j0 + c;
    const bool in = gi >= 0 && gi < G && gj >= 0 && gj < G;
    lc[(r + 1) * S + c + 1] = in ? plane[(size_t)gi * G + gj] : (uint16_t)kInf;
  }
  const int wn = (tl.Cn + 31) >> 5, wacross = wn + 2, gw0 = tl.j0 >> 5;
  for (int idx = tid; idx < (tl.R + 2) * wacross; idx += kNavThreads) {
    const int rr = idx / wacross, r = rr - 1, w = idx - rr * wacross - 1;
    const int gi = tl.i0 + r, gw = gw0 + w;
    const bool in = gi >= 0 && gi < G && gw >= 0 && gw < wpr;
    Ht[r * wprT + w] = in ? ghard[gi * wpr + gw] : 0xffffffffu;
    if (St) St[r * wprT + w] = in ? gsoft[gi * wpr + gw] : 0u;
  }
}

// The sweeps of nav_field_kernel's step 5 over the interior of the tile in LDS, until a pass changes
// nothing or the pass budget runs out: lane t owns row t, then column t; the halo supplies the
// neighbours past the tile's edge, so no row or column needs a bounds test.  (lqi, lqj): the goal
// cell in the tile's coordinates (never relaxed; anywhere else if it is not in this tile).  Returns
// (uniformly) whether any cost went down.
__device__ __forceinline__ int tile_relax(uint16_t* lc, int S, const uint32_t* Ht, const uint32_t* St, int wprT, int R, int Cn,
                                          int lqi, int lqj, int32_t pen, int max_pass, int* budget) {
  const int tid = threadIdx.x;
  const int wn = (Cn + 31) >> 5;
  int any = 0;
  for (int pass = 0; pass < max_pass && *budget > 0; ++pass, --*budget) {
    int changed = 0;
    if (tid < R) {
      const int i = tid;
      const uint32_t* Hi = Ht + i * wprT;
      uint16_t* crow = lc + (i + 1) * S + 1;
      for (int dirn = 0; dirn < 2; ++dirn) {
        for (int ww = 0; ww < wn; ++ww) {
          const int w = dirn ? wn - 1 - ww : ww;
          const uint32_t H0 = Hi[w], S0 = St[i * wprT + w];
          const uint32_t Hp = Hi[w + wprT], Hm = Hi[w - wprT];
          const uint32_t Hrt = (H0 >> 1) | (Hi[w + 1] << 31), Hlf = (H0 << 1) | (Hi[w - 1] >> 31);
          const uint32_t X4 = Hp | Hrt, X5 = Hp | Hlf, X6 = Hm | Hrt, X7 = Hm | Hlf;
          uint32_t todo = ~H0;  // the non-hard cells of this word
          const int nb = Cn - w * 32 < 32 ? Cn - w * 32 : 32;
          if (nb < 32) todo &= (1u << nb) - 1u;
          if (i == lqi && lqj >= 0 && (lqj >> 5) == w) todo &= ~(1u << (lqj & 31));
          for (int bb = 0; bb < nb; ++bb) {
            const int b = dirn ? nb - 1 - bb : bb;
            if (!((todo >> b) & 1u)) continue;
            changed |= relax(crow + w * 32 + b, S, (X4 >> b) & 1u, (X5 >> b) & 1u, (X6 >> b) & 1u, (X7 >> b) & 1u, (S0 >> b) & 1u, pen);
          }
        }
      }
    }
    __syncthreads();
    if (tid < Cn) {
      const int j = tid, w = j >> 5, b = j & 31;
      for (int dirn = 0; dirn < 2; ++dirn) {
        for (int ii = 0; ii < R; ++ii) {
          const int i = dirn ? R - 1 - ii : ii;
          const uint32_t* Hi = Ht + i * wprT;
          const uint32_t H0 = Hi[w], S0 = St[i * wprT + w];
          if (((H0 >> b) & 1u) || (i == lqi && j == lqj)) continue;
          const uint32_t h_up = (Hi[w + wprT] >> b) & 1u, h_dn = (Hi[w - wprT] >> b) & 1u;
          const uint32_t h_rt = b < 31 ? (H0 >> (b + 1)) & 1u : Hi[w + 1] & 1u;
          const uint32_t h_lf = b > 0 ? (H0 >> (b - 1)) & 1u : Hi[w - 1] >> 31;
          changed |= relax(lc + (i + 1) * S + (j + 1), S, h_up | h_rt, h_up | h_lf, h_dn | h_rt, h_dn | h_lf, (S0 >> b) & 1u, pen);
        }
      }
    }
    if (!__syncthreads_or(changed)) break;
    any = 1;
  }
  return any;
}

// The cells of the tile that differ from the global plane go back to it, 4 cells per store; returns
// this lane's kChg* bits.
__device__ __forceinline__ uint32_t tile_store(uint16_t* plane, int G, const NavTile& tl, const uint16_t* lc, int S) {
  const int c4n = tl.Cn >> 2;
  uint32_t chg = 0u;
  for (int idx = threadIdx.x; idx < tl.R * c4n; idx += kNavThreads) {
    const int r = idx / c4n, c = (idx - r * c4n) * 4;
    uint2* g = reinterpret_cast<uint2*>(plane + (size_t)(tl.i0 + r) * G + tl.j0 + c);
    const uint16_t* l = lc + (r + 1) * S + c + 1;
    const uint32_t n0 = l[0], n1 = l[1], n2 = l[2], n3 = l[3];
    const uint2 now = make_uint2(n0 | (n1 << 16), n2 | (n3 << 16)), old = *g;
    if (now.x == old.x && now.y == old.y) continue;
    *g = now;
    const bool first = r == 0, last = r == tl.R - 1;
    if (first) chg |= kChgIm;
    if (last) chg |= kChgIp;
    if (c == 0 && n0 != (old.x & 0xffffu)) chg |= kChgJm | (first ? kChgMM : 0u) | (last ? kChgPM : 0u);
    if (c + 4 == tl.Cn && n3 != (old.y >> 16)) chg |= kChgJp | (first ? kChgMP : 0u) | (last ? kChgPP : 0u);
  }
  return chg;
}

// the SPEC's neighbour rule at cell (i, j) of the global plane (the descent of one lane): bounds tested here
__device__ __forceinline__ int32_t best_global(uint16_t* plane, uint32_t* hard, int G, int wpr, int i, int j, int* kbest) {
  auto d = [&](int ii, int jj) -> uint32_t {
    return (ii >= 0 && ii < G && jj >= 0 && jj < G) ? (uint32_t)plane[(size_t)ii * G + jj] : kInf;
  };
  const uint32_t h_up = i + 1 < G ? mask_bit(hard, wpr, i + 1, j) : 1u, h_dn = i > 0 ? mask_bit(hard, wpr, i - 1, j) : 1u;
  const uint32_t h_rt = j + 1 < G ? mask_bit(hard, wpr, i, j + 1) : 1u, h_lf = j > 0 ? mask_bit(hard, wpr, i, j - 1) : 1u;
  return best_pick(d(i + 1, j), d(i - 1, j), d(i, j + 1), d(i, j - 1), d(i + 1, j + 1), d(i + 1, j - 1), d(i - 1, j + 1),
                   d(i - 1, j - 1), h_up, h_dn, h_rt, h_lf, kbest);
}

// the first dirty tile at or after `from`, cyclically; -1 if none
__device__ __forceinline__ int next_dirty(const uint32_t* dirty, int ntiles, int from) {
  const int nw = (ntiles + 31) >> 5;
  for (int s = 0; s <= nw; ++s) {
    int w = (from >> 5) + s;
    if (w >= nw) w -= nw;
    uint32_t bits = dirty[w];
    if (s == 0) bits &= ~0u << (from & 31);
    if (s == nw) bits &= ~(~0u << (from & 31));
    if (bits) return w * 32 + __ffs(bits) - 1;
  }
  return -1;
}

template <typename T, bool VEC>
__global__ __launch_bounds__(kNavThreads) void nav_field_tiled_kernel(NavArgs a, NavTiledArgs ta, NavFoot foot,
                                                                      const T* __restrict__ newest,
                                                                      const float* __restrict__ goal_ego) {
  extern __shared__ __attribute__((aligned(16))) unsigned char nav_lds[];
  __shared__ uint32_t dirty[kNavMaxTiles / 32];
  __shared__ uint32_t seen;  // the kChg* bits of the tile in hand
  const int G = a.G, wpr = (G + 31) >> 5, G2 = G * G, words = G * wpr;
  const int Te = ta.T, S = Te + 2, wprT = Te / 32 + 2;  // the tile edge
  const int nti = (G + Te - 1) / Te, ntj = nti, ntiles = nti * ntj;
  const int tid = threadIdx.x;
  const int ci = G / 2, cj = G / 2;
  // phase A's view of the LDS
  uint32_t* A = reinterpret_cast<uint32_t*>(nav_lds);
  uint32_t* B = A + words;  // hard
  uint32_t* Cm = B + words;
  // phase B's view
  uint16_t* lc = reinterpret_cast<uint16_t*>(nav_lds);
  uint32_t* Hbase = reinterpret_cast<uint32_t*>(nav_lds + (((size_t)(Te + 2) * S * 2 + 15) & ~(size_t)15));
  uint32_t* Ht = Hbase + wprT + 1;
  uint32_t* St = Ht + (Te + 2) * wprT;
  // this workgroup's slot
  unsigned char* slot = ta.ws + (size_t)blockIdx.x * ta.slot_bytes;
  uint32_t* ghard = reinterpret_cast<uint32_t*>(slot);
  uint32_t* gsoft = ghard + words;

  for (int64_t e = blockIdx.x; e < ta.n; e += gridDim.x) {
    uint16_t* plane = a.cost ? a.cost + e * G2 : reinterpret_cast<uint16_t*>(slot + ta.plane_off);
    uint8_t* gdir = a.dir ? a.dir + e * G2 : nullptr;
    int qi, qj;
    if (!goal_cell(a, goal_ego, e, &qi, &qj)) {
      unreachable_outputs(a, e, a.cost ? plane : nullptr, gdir, tid);
      continue;
    }

    // phase A: the cell classes in LDS, then to the slot; the plane := 65535, d[q] := 0
    __syncthreads();  // the LDS of the env before is done with
    uint32_t* soft = build_classes<T, VEC>(a, foot, newest + e * a.env_stride, A, B, Cm, qi, qj, nullptr);
    for (int w = tid; w < words; w += kNavThreads) {
      ghard[w] = B[w];
      gsoft[w] = soft[w];
    }
    for (int c4 = tid; c4 < G2 / 4; c4 += kNavThreads) {
      uint2 v = make_uint2(0xffffffffu, 0xffffffffu);
      const int at = qi * G + qj - c4 * 4;
      if (at >= 0 && at < 4) (at < 2 ? v.x : v.y) &= (at & 1) ? 0x0000ffffu : 0xffff0000u;
      reinterpret_cast<uint2*>(plane)[c4] = v;
    }
    if (tid < kNavMaxTiles / 32) dirty[tid] = 0u;
    __threadfence_block();
    __syncthreads();
    if (tid == 0) {
      const int qt = (qi / Te) * ntj + qj / Te;
      dirty[qt >> 5] = 1u << (qt & 31);
    }
    __syncthreads();

    // phase B: dirty tiles through LDS until none is left
    const int max_visits = 2 * G2;
    int budget = 4 * G2, from = 0;
    for (int visit = 0; visit < max_visits; ++visit) {
      const int t = next_dirty(dirty, ntiles, from);
      if (t < 0) break;
      from = t + 1 < ntiles ? t + 1 : 0;
      const NavTile tl = nav_tile(t, ntj, Te, G);
      __syncthreads();  // every lane has read the work-list
      if (tid == 0) {
        dirty[t >> 5] &= ~(1u << (t & 31));
        seen = 0u;
      }
      tile_load(plane, ghard, gsoft, G, wpr, tl, lc, S, Ht, St, wprT);
      __syncthreads();
      const bool q_here = qi >= tl.i0 && qi < tl.i0 + tl.R && qj >= tl.j0 && qj < tl.j0 + tl.Cn;
      const int any = tile_relax(lc, S, Ht, St, wprT, tl.R, tl.Cn, q_here ? qi - tl.i0 : -1, q_here ? qj - tl.j0 : -1,
                                 a.soft_pen, 2 * Te * Te, &budget);
      if (any) {
        const uint32_t chg = tile_store(plane, G, tl, lc, S);
        if (chg) atomicOr(&seen, chg);
        __threadfence_block();
        __syncthreads();
        if (tid == 0) {
          const uint32_t sb = seen;
          const int ti = t / ntj, tj = t - ti * ntj;
          auto mark = [&](int di, int dj, uint32_t bit) {
            const int ni = ti + di, nj = tj + dj;
            if ((sb & bit) && ni >= 0 && ni < nti && nj >= 0 && nj < ntj) {
              const int nt = ni * ntj + nj;
              dirty[nt >> 5] |= 1u << (nt & 31);
            }
          };
          mark(-1, 0, kChgIm); mark(1, 0, kChgIp); mark(0, -1, kChgJm); mark(0, 1, kChgJp);
          mark(-1, -1, kChgMM); mark(-1, 1, kChgMP); mark(1, -1, kChgPM); mark(1, 1, kChgPP);
        }
      }
      __syncthreads();
    }

    // phase C: dir from one more pass over the tiles, 4 cells per store
    if (gdir) {
      for (int t = 0; t < ntiles; ++t) {
        const NavTile tl = nav_tile(t, ntj, Te, G);
        __syncthreads();
        tile_load(plane, ghard, nullptr, G, wpr, tl, lc, S, Ht, nullptr, wprT);
        __syncthreads();
        const int c4n = tl.Cn >> 2;
        for (int idx = tid; idx < tl.R * c4n; idx += kNavThreads) {
          const int r = idx / c4n, c0 = (idx - r * c4n) * 4;
          uint32_t k8[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int c = c0 + u, w = c >> 5, b = c & 31;
            const uint16_t* cell = lc + (r + 1) * S + c + 1;
            const uint32_t d = cell[0];
            const bool at_q = tl.i0 + r == qi && tl.j0 + c == qj;
            int k = -1;
            if (d < kInf && !at_q) {
              const uint32_t* Hi = Ht + r * wprT;
              const uint32_t h_rt = b < 31 ? (Hi[w] >> (b + 1)) & 1u : Hi[w + 1] & 1u;
              const uint32_t h_lf = b > 0 ? (Hi[w] >> (b - 1)) & 1u : Hi[w - 1] >> 31;
              best_of(cell, S, (Hi[w + wprT] >> b) & 1u, (Hi[w - wprT] >> b) & 1u, h_rt, h_lf, &k);
            }
            k8[u] = d == kInf ? 255u : (at_q ? 8u : (uint32_t)(k & 0xff));
          }
          *reinterpret_cast<uint32_t*>(gdir + (size_t)(tl.i0 + r) * G + tl.j0 + c0) = k8[0] | (k8[1] << 8) | (k8[2] << 16) | (k8[3] << 24);
        }
      }
    }

    // one lane: the descent from the robot cell on the global plane, and the follower
    if (tid == 0) {
      const uint32_t dc = plane[(size_t)ci * G + cj];
      int ti = ci, tj = cj;
      if (dc < kInf) {
        for (int s = 0; s < a.lookahead; ++s) {
          if (ti == qi && tj == qj) break;
          int k;
          best_global(plane, ghard, G, wpr, ti, tj, &k);
          if (k < 0) break;
          descent_move(k, &ti, &tj);
        }
      }
      robot_outputs(a, e, dc, ti - ci, tj - cj);
    }
  }
}

// the checks of the footprint, the format and the knobs, shared by both entries (`who` names the entry)
int nav_check_knobs(const char* who, const ffmp_cfg_t* cfg, int32_t format, int32_t margin, int32_t soft_pen, int32_t lookahead) {
  if (cfg->n_foot < 0 || cfg->n_foot > FFMP_MAX_FOOT) return fail(FFMP_E_ARG, "%s: n_foot out of range: %d", who, cfg->n_foot);
  for (int f = 0; f < cfg->n_foot; ++f)
    if (cfg->foot_di[f] < -cfg->grid || cfg->foot_di[f] > cfg->grid || cfg->foot_dj[f] < -cfg->grid || cfg->foot_dj[f] > cfg->grid)
      return fail(FFMP_E_ARG, "%s: footprint offset %d outside the grid", who, f);
  if (format != FFMP_OBS_F32 && format != FFMP_OBS_U8F16) return fail(FFMP_E_ARG, "%s: unknown obs format %d", who, format);
  if (margin < 0 || margin > 8) return fail(FFMP_E_ARG, "%s: margin must be in 0..8, got %d", who, margin);
  if (soft_pen < 0 || soft_pen > 16384) return fail(FFMP_E_ARG, "%s: soft_pen must be in 0..16384, got %d", who, soft_pen);
  if (lookahead < 1 || lookahead > 64) return fail(FFMP_E_ARG, "%s: lookahead must be in 1..64, got %d", who, lookahead);
  return FFMP_OK;
}

// every check that needs no pointer: the shape, the knobs and the LDS budget
int nav_check(const ffmp_cfg_t* cfg, int32_t format, int32_t margin, int32_t soft_pen, int32_t lookahead) {
  if (!cfg) return fail(FFMP_E_ARG, "cfg is NULL");
  if (cfg->grid < 8 || cfg->grid > kNavMaxGrid || (cfg->grid % 4) != 0)
    return fail(FFMP_E_ARG, "ffmp_nav_field: grid must be a multiple of 4 in [8,%d] (one workgroup holds the whole "
                "plane in LDS), got %d", kNavMaxGrid, cfg->grid);
  int rc = nav_check_knobs("ffmp_nav_field", cfg, format, margin, soft_pen, lookahead);
  if (rc) return rc;
  if (nav_lds_bytes(cfg->grid) > kNavLdsLimit)
    return fail(FFMP_E_ARG, "ffmp_nav_field: grid %d needs %zu bytes of LDS", cfg->grid, nav_lds_bytes(cfg->grid));
  return FFMP_OK;
}

// the same for the tiled entry: the grid up to 512, the tile
int nav_tiled_check(const ffmp_cfg_t* cfg, int32_t format, int32_t margin, int32_t soft_pen, int32_t lookahead, int32_t tile) {
  if (!cfg) return fail(FFMP_E_ARG, "cfg is NULL");
  if (cfg->grid < 8 || cfg->grid > kNavTiledMaxGrid || (cfg->grid % 4) != 0)
    return fail(FFMP_E_ARG, "ffmp_nav_field_tiled: grid must be a multiple of 4 in [8,%d], got %d", kNavTiledMaxGrid, cfg->grid);
  if (tile != 0 && (tile < 32 || tile > kNavTileDefault || (tile % 32) != 0))
    return fail(FFMP_E_ARG, "ffmp_nav_field_tiled: tile must be 0 (the default, %d) or a multiple of 32 in [32,%d], got %d",
                kNavTileDefault, kNavTileDefault, tile);
  int rc = nav_check_knobs("ffmp_nav_field_tiled", cfg, format, margin, soft_pen, lookahead);
  if (rc) return rc;
  const size_t lds = nav_tiled_lds_bytes(cfg->grid, nav_tile_edge(cfg->grid, tile));
  if (lds > kNavLdsLimit) return fail(FFMP_E_ARG, "ffmp_nav_field_tiled: grid %d, tile %d need %zu bytes of LDS", cfg->grid, tile, lds);
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
  return launch_ok("ffmp_nav_field");
}

const void* nav_tiled_fn(bool u8, bool vec) {
  if (u8) return vec ? reinterpret_cast<const void*>(nav_field_tiled_kernel<uint8_t, true>)
                     : reinterpret_cast<const void*>(nav_field_tiled_kernel<uint8_t, false>);
  return vec ? reinterpret_cast<const void*>(nav_field_tiled_kernel<float, true>)
             : reinterpret_cast<const void*>(nav_field_tiled_kernel<float, false>);
}

// The slots of the persistent grid on the current device for `lds` bytes of dynamic LDS: CUs x the
// workgroups of the kernel resident per CU (the fewest over its four instances), at most
// kNavSlotCap.  Remembered per (device, lds): the workspace query and the launch get one answer, and
// a launch inside a stream capture repeats no query.  *have_device = false (no HIP device to ask):
// the cap itself, an upper bound, which only the workspace query accepts.
int nav_tiled_device_slots(size_t lds, bool* have_device, int* slots) {
  struct Known { int dev; size_t lds; int slots; };
  static std::mutex mu;
  static std::vector<Known> known;
  static uint64_t lds_raised = 0;
  int dev = 0, ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1 || hipGetDevice(&dev) != hipSuccess) {
    (void)hipGetLastError();
    *have_device = false;
    *slots = kNavSlotCap;
    return FFMP_OK;
  }
  *have_device = true;
  std::lock_guard<std::mutex> lock(mu);
  for (const Known& k : known)
    if (k.dev == dev && k.lds == lds) {
      *slots = k.slots;
      return FFMP_OK;
    }
  if (!(lds_raised & (1ull << (dev & 63)))) {
    // more than the default cap of dynamic LDS: ask for it, once per device (an attribute of the
    // functions, no stream work)
    for (int v = 0; v < 4; ++v) {
      hipError_t err = hipFuncSetAttribute(nav_tiled_fn(v & 1, v & 2), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kNavLdsLimit);
      if (err != hipSuccess)
        return fail(FFMP_E_HIP, "ffmp_nav_field_tiled: hipFuncSetAttribute(%zu bytes of LDS): %s", kNavLdsLimit, hipGetErrorString(err));
    }
    lds_raised |= 1ull << (dev & 63);
  }
  int cus = 0;
  hipError_t err = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  if (err != hipSuccess || cus < 1) return fail(FFMP_E_HIP, "ffmp_nav_field_tiled: no CU count for device %d", dev);
  int per_cu = 1 << 30;
  for (int v = 0; v < 4; ++v) {
    int occ = 0;
    err = hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, nav_tiled_fn(v & 1, v & 2), kNavThreads, lds);
    if (err != hipSuccess || occ < 1)
      return fail(FFMP_E_HIP, "ffmp_nav_field_tiled: no workgroup with %zu bytes of LDS fits a CU (%s)", lds, hipGetErrorString(err));
    per_cu = occ < per_cu ? occ : per_cu;
  }
  const int64_t s = (int64_t)cus * per_cu;
  *slots = s > kNavSlotCap ? kNavSlotCap : (int)s;
  known.push_back({dev, lds, *slots});
  return FFMP_OK;
}

}  // namespace

extern "C" {

int ffmp_nav_field_tiled_check(const ffmp_cfg_t* cfg, int32_t format, int32_t margin, int32_t soft_pen, int32_t lookahead,
                               int32_t tile) {
  return nav_tiled_check(cfg, format, margin, soft_pen, lookahead, tile);
}

int ffmp_nav_field_tiled_workspace(const ffmp_cfg_t* cfg, int64_t n, int32_t tile, int with_cost, size_t* bytes) {
  if (!bytes) return fail(FFMP_E_ARG, "ffmp_nav_field_tiled_workspace: bytes is NULL");
  int rc = nav_tiled_check(cfg, FFMP_OBS_F32, 0, 0, 1, tile);
  if (rc) return rc;
  if (n < 0) return fail(FFMP_E_ARG, "ffmp_nav_field_tiled_workspace: negative n");
  bool have_device;
  int slots = 0;
  rc = nav_tiled_device_slots(nav_tiled_lds_bytes(cfg->grid, nav_tile_edge(cfg->grid, tile)), &have_device, &slots);
  if (rc) return rc;
  const int64_t used = n < slots ? n : slots;
  *bytes = (size_t)used * nav_tiled_slot_bytes(cfg->grid, with_cost != 0);
  return FFMP_OK;
}

int ffmp_nav_field_tiled(const ffmp_cfg_t* cfg, int64_t n, const ffmp_obs_t* obs, const float* goal_ego, int64_t goal_stride,
                         int32_t margin, int32_t soft_pen, int32_t lookahead, double turn_sin, uint16_t* cost, uint8_t* dir,
                         int32_t* target, int32_t* geo_cost, double* cmd, int32_t tile, void* workspace, size_t workspace_bytes,
                         void* stream) {
  const char* who = "ffmp_nav_field_tiled";
  if (!obs) return fail(FFMP_E_ARG, "%s: obs is NULL", who);
  int rc = nav_tiled_check(cfg, obs->format, margin, soft_pen, lookahead, tile);
  if (rc) return rc;
  if (!(turn_sin >= 0.0)) return fail(FFMP_E_ARG, "%s: turn_sin must be >= 0 and not NaN", who);
  if (n < 0) return fail(FFMP_E_ARG, "%s: negative n", who);
  if (!obs->state_m) return fail(FFMP_E_ARG, "%s: obs.state_m is NULL", who);
  if (!goal_ego) return fail(FFMP_E_ARG, "%s: goal_ego is NULL", who);
  if (goal_stride < 2) return fail(FFMP_E_ARG, "%s: goal_stride must be >= 2, got %lld", who, (long long)goal_stride);
  if (((uintptr_t)cmd & 15u) != 0) return fail(FFMP_E_ARG, "%s: cmd must be 16-byte aligned", who);
  if (cmd && !(cfg->dt > 0.0)) return fail(FFMP_E_CFG, "%s: dt must be > 0 with cmd (the follower's turn rate divides by it), got %g", who, cfg->dt);
  if (((uintptr_t)cost & 7u) != 0) return fail(FFMP_E_ARG, "%s: cost must be 8-byte aligned", who);
  if (((uintptr_t)dir & 3u) != 0) return fail(FFMP_E_ARG, "%s: dir must be 4-byte aligned", who);
  if (!workspace) return fail(FFMP_E_ARG, "%s: workspace is NULL", who);
  if (((uintptr_t)workspace & 255u) != 0) return fail(FFMP_E_ARG, "%s: workspace must be 256-byte aligned", who);
  const int G = cfg->grid, T = nav_tile_edge(G, tile);
  const size_t slot_bytes = nav_tiled_slot_bytes(G, cost != nullptr);
  if (n > 0 && workspace_bytes < slot_bytes)
    return fail(FFMP_E_ARG, "%s: workspace too small: %zu bytes, one slot takes %zu", who, workspace_bytes, slot_bytes);
  if (n == 0) return FFMP_OK;
  if (n > 0x7fffffffLL) return fail(FFMP_E_ARG, "%s: n too large for one launch: %lld", who, (long long)n);
  const size_t lds = nav_tiled_lds_bytes(G, T);
  bool have_device;
  int slots = 0;
  rc = nav_tiled_device_slots(lds, &have_device, &slots);
  if (rc) return rc;
  if (!have_device) return fail(FFMP_E_HIP, "%s: no HIP device", who);
  if (n < slots) slots = (int)n;
  if (workspace_bytes < (size_t)slots * slot_bytes)
    return fail(FFMP_E_ARG, "%s: workspace too small: %zu bytes, %d slots take %zu (ffmp_nav_field_tiled_workspace)", who,
                workspace_bytes, slots, (size_t)slots * slot_bytes);
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
  NavTiledArgs ta;
  ta.T = T;
  ta.n = n;
  ta.ws = static_cast<unsigned char*>(workspace);
  ta.slot_bytes = slot_bytes;
  ta.plane_off = nav_tiled_mask_bytes(G);
  NavFoot foot;
  for (int f = 0; f < FFMP_MAX_FOOT; ++f) {
    foot.di[f] = f < cfg->n_foot ? (int16_t)cfg->foot_di[f] : 0;
    foot.dj[f] = f < cfg->n_foot ? (int16_t)cfg->foot_dj[f] : 0;
  }
  const int64_t frame = obs->state_m_frame_stride ? obs->state_m_frame_stride : G2;
  hipStream_t s = (hipStream_t)stream;
  if (obs->format == FFMP_OBS_F32) {
    const float* newest = obs->state_m + frame;
    const bool vec = ((uintptr_t)newest & 15u) == 0 && ((a.env_stride * 4) & 15) == 0;
    if (vec) hipLaunchKernelGGL((nav_field_tiled_kernel<float, true>), dim3((unsigned)slots), dim3(kNavThreads), lds, s, a, ta, foot, newest, goal_ego);
    else hipLaunchKernelGGL((nav_field_tiled_kernel<float, false>), dim3((unsigned)slots), dim3(kNavThreads), lds, s, a, ta, foot, newest, goal_ego);
  } else {
    const uint8_t* newest = reinterpret_cast<const uint8_t*>(obs->state_m) + frame;
    const bool vec = ((uintptr_t)newest & 15u) == 0 && (a.env_stride & 15) == 0;
    if (vec) hipLaunchKernelGGL((nav_field_tiled_kernel<uint8_t, true>), dim3((unsigned)slots), dim3(kNavThreads), lds, s, a, ta, foot, newest, goal_ego);
    else hipLaunchKernelGGL((nav_field_tiled_kernel<uint8_t, false>), dim3((unsigned)slots), dim3(kNavThreads), lds, s, a, ta, foot, newest, goal_ego);
  }
  return launch_ok(who);
}

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
  if (cmd && !(cfg->dt > 0.0))
    return fail(FFMP_E_CFG, "ffmp_nav_field: dt must be > 0 with cmd (the follower's turn rate divides by it), got %g", cfg->dt);
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
