// ffmp_potential.hip — clearance, potential plane and robot-cell gradient of any occupancy frame
// (include/ffmp.h ffmp_frame_potential carries the SPEC).  A source of its own: the
// code objects of the step, the raster and the other opt-in passes stay what they are.
//
// One workgroup per env: 256 threads, 512 or 1,024 where the LDS of an env leaves room for fewer workgroups on a
// compute unit (pot_plan).  LDS, per env (dynamic, pot_plan() lays it out):
//   bits  G rows of ceil(G/32) words: bit j of row i is obst[i][j].  Zeroed, then ORed in nibble by nibble
//         while the frame is read once, 16 bytes per lane; an empty nibble costs nothing, and almost every nibble is empty.
//         Bits of a row's last word past column G are never set, so a row's windows see no neighbour row.
//   g     one byte per cell of `grows` rows: the distance along j to the nearest set bit of the row within
//         reach, 255 if there is none — from 64-bit windows of the bit row with ctz / clz.
//   cmask two buffers of ceil(grows/32) words per group of 4 columns: bit r of a group's column says that row r of g
//         holds a byte other than 255 for the group.  Most cells have no obstacle in their window (2 to 9 % had
//         one in the measured scenes): a lane reads the one or two mask words of its window and visits only the
//         rows whose bit is set, instead of 2 reach + 1 words of g.  The bands alternate between the buffers, so
//         the next band's is zeroed while this band's is read and no barrier is added.
//   tab   2 reach^2 + 1 floats: the repulsive addend half_kr_f * (q*q) of every value d2 can take, filled by
//         the SPEC's arithmetic (sqrt_rn, rcp_rn); inr: one byte each, the SPEC's `d < rho0_f`.
// The plane is worked in bands of `band` rows: g for the band and `reach` halo rows on each side (rebuilt
// from the bits, which cost no memory traffic), a barrier, then a lane owns 4 consecutive cells of a row —
// per row of its window that holds something one 4-byte read of g, d2 = min(di^2 + g^2) — looks the addend up, adds it to the attractive term
// and stores its 4 cells at once.  Up to G = 128 the band is the plane; at 512 with reach 32 the LDS is
// 93 KiB (above the default cap of dynamic LDS: asked for once per device).
// The four U of the gradient and d2 at the robot cell: the lanes that own those cells leave their d2 in LDS,
// thread 0 evaluates the SPEC's expressions from them after the last band.  With neither plane asked for,
// only rows c-1..c+1 are worked on, and only the frame rows within reach of them are read.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <atomic>
#include <type_traits>

#include "ffmp_device.h"
#include "ffmp_host.h"

#pragma clang fp contract(off)

namespace {

constexpr int kPotMaxThreads = 1024;
constexpr size_t kPotLdsCu = 160 * 1024;  // LDS of a compute unit
constexpr int kPotMaxReach = 32;
constexpr int kPotNone = 65535;
constexpr size_t kPotLdsDefault = 64 * 1024;
#ifndef FFMP_POT_GBYTES
#define FFMP_POT_GBYTES 24576
#endif
constexpr int kPotGBytes = FFMP_POT_GBYTES;  // g holds about this many bytes, and never fewer than 2 reach + 32 rows

struct PotPlan {
  int32_t row_words;  // words of a bit row
  int32_t grows;      // rows of g
  int32_t band;       // rows of a band
  int32_t tab_n;      // entries of tab / inr
  int32_t mask_words; // words of a column of cmask
  int32_t threads;    // of a block
  size_t lds;         // bytes
};

__host__ __device__ inline int pot_row_words(int G) { return (G + 31) >> 5; }

PotPlan pot_plan(int G, int reach) {
  PotPlan p;
  p.row_words = pot_row_words(G);
  int rows = kPotGBytes / G;
  if (rows < 2 * reach + 32) rows = 2 * reach + 32;
  if (rows >= G) {
    p.grows = G;
    p.band = G;
  } else {
    p.grows = rows;
    p.band = rows - 2 * reach;
  }
  p.tab_n = 2 * reach * reach + 1;
  p.mask_words = (p.grows + 31) >> 5;
  p.lds = (size_t)G * p.row_words * 4 + (size_t)p.grows * G + 2 * (size_t)p.mask_words * G + (size_t)p.tab_n * 4 +
          (size_t)((p.tab_n + 3) & ~3);
  // the LDS decides how many blocks share a compute unit: fewer blocks, more threads each, so that the unit
  // keeps about 2,048 threads to hide the LDS and memory latency of the phases between the barriers
  const size_t blocks = kPotLdsCu / p.lds;
  p.threads = blocks >= 8 ? 256 : blocks >= 4 ? 512 : kPotMaxThreads;
  return p;
}

struct PotArgs {
  const void* frame;
  int64_t frame_stride;  // elements
  const float* goal;
  int64_t goal_stride;
  const uint8_t* mask;
  uint16_t* dist2;       // or NULL
  int64_t dist2_stride;  // elements
  void* pot;             // or NULL
  int64_t pot_stride;    // elements
  float* grad;           // or NULL
  int32_t* robot_d2;     // or NULL
  float res_f, half_f, half_ka_f, half_kr_f, rho0_f, inv_rho0_f, rho_min_f, inv_2res_f;
  int32_t G, occ_min, reach, row_words, grows, band, tab_n, mask_words;
  int32_t frame_vec, dist2_vec, pot_vec;  // the wide accesses allowed
};

// bit u: cell u of the 4 is an obstacle
FFMP_DEV uint32_t pot_obst4(float4 v, float thr) {
  return (v.x >= thr ? 1u : 0u) | (v.y >= thr ? 2u : 0u) | (v.z >= thr ? 4u : 0u) | (v.w >= thr ? 8u : 0u);
}
FFMP_DEV uint32_t pot_obst4(uint32_t w, uint32_t thr) {
  uint32_t m = 0;
#pragma unroll
  for (int u = 0; u < 4; ++u) m |= (((w >> (8 * u)) & 255u) >= thr ? 1u : 0u) << u;
  return m;
}

// A lane's load is 16 bytes, consecutive lanes consecutive addresses: 4 cells of a float32 frame, 16 of a uint8 one.
template <typename FT>
struct PotChunk {
  static constexpr int kCells = 16 / (int)sizeof(FT);
};

// the obstacle bits of the kCells consecutive cells at f
template <typename FT>
FFMP_DEV uint32_t pot_load_chunk(const FT* f, bool vec, int occ_min) {
  if constexpr (std::is_same<FT, float>::value) {
    const float4 v = vec ? *reinterpret_cast<const float4*>(f) : make_float4(f[0], f[1], f[2], f[3]);
    return pot_obst4(v, (float)occ_min);
  } else {
    const uint32_t thr = (uint32_t)occ_min;
    const uint32_t* p = reinterpret_cast<const uint32_t*>(f);
    const uint4 v = vec ? *reinterpret_cast<const uint4*>(f) : make_uint4(p[0], p[1], p[2], p[3]);
    return pot_obst4(v.x, thr) | (pot_obst4(v.y, thr) << 4) | (pot_obst4(v.z, thr) << 8) | (pot_obst4(v.w, thr) << 12);
  }
}

// The g bytes of cells j0..j0+3 (j0 % 4 == 0) of the bit row `row`.
FFMP_DEV uint32_t pot_g4(const uint32_t* row, int row_words, int j0, int reach) {
  const int w = j0 >> 5;
  // 128 bits around the cell: words w-1 .. w+2 of the row, zero outside it; cell j sits at bit 32 + (j & 31)
  const uint32_t w0 = w >= 1 ? row[w - 1] : 0u, w1 = row[w];
  const uint32_t w2 = w + 1 < row_words ? row[w + 1] : 0u, w3 = w + 2 < row_words ? row[w + 2] : 0u;
  const uint64_t lo = (uint64_t)w0 | ((uint64_t)w1 << 32), hi = (uint64_t)w2 | ((uint64_t)w3 << 32);
  if ((lo | hi) == 0ull) return 0xFFFFFFFFu;
  uint32_t out = 0;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int p = 32 + (j0 & 31) + u;  // 32..67
    // the cell and the 63 after it; the cell and the 32 before it, the cell at bit 32
    const uint64_t right = p < 64 ? (lo >> p) | (hi << (64 - p)) : hi >> (p - 64);
    const int s = p - 32;  // 0..35
    const uint64_t left = (s == 0 ? lo : (lo >> s) | (hi << (64 - s))) & 0x1FFFFFFFFull;
    const int dr = right ? __builtin_ctzll(right) : 64;
    const int dl = left ? __builtin_clzll(left << 31) : 64;
    const int d = min(dr, dl);
    out |= (d <= reach ? (uint32_t)d : 255u) << (8 * u);
  }
  return out;
}

struct PotTab {
  const float* tab;
  const uint8_t* inr;
};

// the SPEC's U of cell (i, j) with clearance d2, the attractive term from the goal (gx, gy)
FFMP_DEV float pot_u(const PotArgs& a, const PotTab& t, int i, int j, float gx, float gy, int d2) {
  const float ex = (float)i * a.res_f - a.half_f, ey = (float)j * a.res_f - a.half_f;
  const float dx = ex - gx, dy = ey - gy;
  float U = a.half_ka_f * (dx * dx + dy * dy);
  if (d2 != kPotNone && t.inr[d2]) U = U + t.tab[d2];
  return U;
}

template <typename FT, typename PT>
__global__ __launch_bounds__(kPotMaxThreads) void frame_potential_kernel(PotArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t pot_lds[];
  __shared__ int s_d2[5];  // (c+1,c) (c-1,c) (c,c+1) (c,c-1) (c,c)
  const int G = a.G, G4 = G >> 2, c = G >> 1, reach = a.reach, rw = a.row_words;
  const int tid = threadIdx.x, nt = blockDim.x;
  const int64_t e = blockIdx.x;
  if (a.mask && a.mask[e] == 0) return;  // block-uniform

  uint32_t* bits = pot_lds;
  uint32_t* g32 = bits + G * rw;                                 // grows * G4 words
  uint32_t* cmask = g32 + a.grows * G4;                          // 2 buffers of mask_words * G4 words
  const int n_cm = a.mask_words * G4;
  float* tab = reinterpret_cast<float*>(cmask + 2 * n_cm);       // tab_n floats
  uint8_t* inr = reinterpret_cast<uint8_t*>(tab + a.tab_n);      // tab_n bytes
  const PotTab pt{tab, inr};

  // the rows whose cells are worked on, and the frame rows within reach of them
  const bool planes = a.dist2 != nullptr || a.pot != nullptr;  // block-uniform
  const int r0 = planes ? 0 : c - 1, r1 = planes ? G : c + 2;
  const int f0 = max(r0 - reach, 0), f1 = min(r1 + reach, G);

  for (int w = tid; w < G * rw; w += nt) bits[w] = 0u;
  for (int w = tid; w < n_cm; w += nt) cmask[w] = 0u;
  for (int t = tid; t < a.tab_n; t += nt) {
    float d = ffmp::sqrt_rn((float)t) * a.res_f;
    d = fmaxf(d, a.rho_min_f);
    const float q = ffmp::rcp_rn(d) - a.inv_rho0_f;
    tab[t] = a.half_kr_f * (q * q);
    inr[t] = d < a.rho0_f ? 1 : 0;
  }
  __syncthreads();

  // the frame, once: the 16-byte chunks that hold a cell of rows f0..f1-1 (G*G % 16 == 0: the last chunk ends in the plane)
  const FT* frame = reinterpret_cast<const FT*>(a.frame) + e * a.frame_stride;
  const bool fvec = a.frame_vec != 0;
  constexpr int kCells = PotChunk<FT>::kCells;
  const int ch0 = (f0 * G) / kCells, ch1 = (f1 * G + kCells - 1) / kCells;
  for (int ch = ch0 + tid; ch < ch1; ch += nt) {
    const int q0 = ch * kCells;
    const uint32_t m = pot_load_chunk<FT>(frame + q0, fvec, a.occ_min);
    if (m == 0u) continue;
#pragma unroll
    for (int r = 0; r < kCells / 4; ++r) {
      const uint32_t nib = (m >> (4 * r)) & 15u;
      if (nib == 0u) continue;
      const int q = q0 + 4 * r;  // G % 4 == 0: the 4 cells are in one row, and j & 31 <= 28
      const int i = q / G, j = q - i * G;
      atomicOr(&bits[i * rw + (j >> 5)], nib << (j & 31));
    }
  }
  __syncthreads();

  const float gx = a.goal[e * a.goal_stride], gy = a.goal[e * a.goal_stride + 1];
  uint16_t* dist2 = a.dist2 ? a.dist2 + e * a.dist2_stride : nullptr;
  PT* pot = a.pot ? reinterpret_cast<PT*>(a.pot) + e * a.pot_stride : nullptr;

  int buf = 0;
  for (int b0 = r0; b0 < r1; b0 += a.band, buf ^= 1) {
    const int b1 = min(b0 + a.band, r1);
    const int h0 = max(b0 - reach, 0), h1 = min(b1 + reach, G);  // h1 - h0 <= grows
    uint32_t* cm = cmask + buf * n_cm;
    // g of rows h0..h1-1: only the words that hold something are stored, and marked in the column mask
    for (int t = tid; t < (h1 - h0) * G4; t += nt) {
      const int ri = t / G4, j4 = t - ri * G4;
      const uint32_t gw = pot_g4(bits + (h0 + ri) * rw, rw, j4 << 2, reach);
      if (gw != 0xFFFFFFFFu) {
        g32[t] = gw;
        atomicOr(&cm[(ri >> 5) * G4 + j4], 1u << (ri & 31));
      }
    }
    __syncthreads();
    // the next band's mask: its last readers were the band before this one
    if (b1 < r1)
      for (int w = tid; w < n_cm; w += nt) cmask[(buf ^ 1) * n_cm + w] = 0u;
    // the cells of rows b0..b1-1, 4 per lane
    for (int t = tid; t < (b1 - b0) * G4; t += nt) {
      const int ri = t / G4, j4 = t - ri * G4;
      const int i = b0 + ri, j0 = j4 << 2;
      int d2[4] = {kPotNone, kPotNone, kPotNone, kPotNone};
      const int lo = max(i - reach, h0) - h0, hi = min(i + reach, h1 - 1) - h0;  // the window, in rows of g
      for (int w = lo >> 5; w <= hi >> 5; ++w) {
        uint32_t m = cm[w * G4 + j4];
        const int w0 = w << 5;
        if (lo > w0) m &= 0xFFFFFFFFu << (lo - w0);
        if (hi < w0 + 31) m &= 0xFFFFFFFFu >> (w0 + 31 - hi);
        for (; m; m &= m - 1u) {
          const int rr = w0 + __builtin_ctz(m);
          const uint32_t gw = g32[rr * G4 + j4];
          const int di = rr + h0 - i, di2 = di * di;
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int gb = (int)((gw >> (8 * u)) & 255u);
            const int cand = gb == 255 ? kPotNone : di2 + gb * gb;
            d2[u] = min(d2[u], cand);
          }
        }
      }
      // the gradient's cells
      if (i >= c - 1 && i <= c + 1 && j0 <= c + 1 && j0 + 3 >= c - 1) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int j = j0 + u;
          if (i == c + 1 && j == c) s_d2[0] = d2[u];
          if (i == c - 1 && j == c) s_d2[1] = d2[u];
          if (i == c && j == c + 1) s_d2[2] = d2[u];
          if (i == c && j == c - 1) s_d2[3] = d2[u];
          if (i == c && j == c) s_d2[4] = d2[u];
        }
      }
      const int64_t off = (int64_t)i * G + j0;
      if (dist2) {
        const uint32_t x = (uint32_t)d2[0] | ((uint32_t)d2[1] << 16), y = (uint32_t)d2[2] | ((uint32_t)d2[3] << 16);
        if (a.dist2_vec) {
          *reinterpret_cast<uint2*>(dist2 + off) = make_uint2(x, y);
        } else {
          uint32_t* o = reinterpret_cast<uint32_t*>(dist2 + off);
          o[0] = x; o[1] = y;
        }
      }
      if (pot) {
        float U[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) U[u] = pot_u(a, pt, i, j0 + u, gx, gy, d2[u]);
        if constexpr (std::is_same<PT, float>::value) {
          if (a.pot_vec) {
            *reinterpret_cast<float4*>(pot + off) = make_float4(U[0], U[1], U[2], U[3]);
          } else {
            pot[off] = U[0]; pot[off + 1] = U[1]; pot[off + 2] = U[2]; pot[off + 3] = U[3];
          }
        } else {
          union { _Float16 h[4]; uint32_t w[2]; } v;
#pragma unroll
          for (int u = 0; u < 4; ++u) v.h[u] = (_Float16)U[u];  // round to nearest even
          if (a.pot_vec) {
            *reinterpret_cast<uint2*>(pot + off) = make_uint2(v.w[0], v.w[1]);
          } else {
            uint32_t* o = reinterpret_cast<uint32_t*>(pot + off);
            o[0] = v.w[0]; o[1] = v.w[1];
          }
        }
      }
    }
    __syncthreads();  // the next band rewrites g and fills the other mask; after the last one s_d2 is complete
  }

  if (tid == 0) {
    if (a.grad) {
      const float uxp = pot_u(a, pt, c + 1, c, gx, gy, s_d2[0]), uxm = pot_u(a, pt, c - 1, c, gx, gy, s_d2[1]);
      const float uyp = pot_u(a, pt, c, c + 1, gx, gy, s_d2[2]), uym = pot_u(a, pt, c, c - 1, gx, gy, s_d2[3]);
      a.grad[e * 2 + 0] = (uxp - uxm) * a.inv_2res_f;
      a.grad[e * 2 + 1] = (uyp - uym) * a.inv_2res_f;
    }
    if (a.robot_d2) a.robot_d2[e] = s_d2[4] == kPotNone ? -1 : s_d2[4];
  }
}

int pot_check(const char* who, const ffmp_cfg_t* cfg, int32_t frame_format, int32_t potential_format, int32_t occ_min,
              int32_t reach) {
  if (!cfg) return fail(FFMP_E_ARG, "%s: cfg is NULL", who);
  if (cfg->grid < 8 || cfg->grid > 512 || (cfg->grid % 4) != 0)
    return fail(FFMP_E_ARG, "%s: grid must be a multiple of 4 in [8,512], got %d", who, cfg->grid);
  if (frame_format != FFMP_OBS_F32 && frame_format != FFMP_OBS_U8F16)
    return fail(FFMP_E_ARG, "%s: unknown frame_format %d", who, frame_format);
  if (potential_format != FFMP_OBS_F32 && potential_format != FFMP_OBS_U8F16)
    return fail(FFMP_E_ARG, "%s: unknown potential_format %d", who, potential_format);
  if (occ_min < 1 || occ_min > 255) return fail(FFMP_E_ARG, "%s: occ_min must be in [1,255], got %d", who, occ_min);
  if (reach < 1 || reach > kPotMaxReach) return fail(FFMP_E_ARG, "%s: reach must be in [1,%d], got %d", who, kPotMaxReach, reach);
  return FFMP_OK;
}

// do the byte ranges [a, a + na) and [b, b + nb) meet
bool pot_ranges_meet(const void* a, uint64_t na, const void* b, uint64_t nb) {
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return pa < pb ? pb - pa < na : pa - pb < nb;
}

}  // namespace

extern "C" {

int ffmp_frame_potential_check(const ffmp_cfg_t* cfg, int32_t frame_format, int32_t potential_format, int32_t occ_min,
                               int32_t reach) {
  return pot_check("ffmp_frame_potential", cfg, frame_format, potential_format, occ_min, reach);
}

int ffmp_frame_potential(const ffmp_cfg_t* cfg, int64_t n, const void* frame, int64_t frame_env_stride, int32_t frame_format,
                         const float* goal_ego, int64_t goal_stride, const uint8_t* mask, int32_t occ_min, int32_t reach,
                         uint16_t* dist2, int64_t dist2_env_stride, void* potential, int64_t potential_env_stride,
                         int32_t potential_format, float* grad, int32_t* robot_d2, void* stream) {
  const char* who = "ffmp_frame_potential";
  if (int rc = pot_check(who, cfg, frame_format, potential_format, occ_min, reach)) return rc;
  if (n < 0) return fail(FFMP_E_ARG, "%s: negative n", who);
  if (n > 0x7fffffffLL) return fail(FFMP_E_ARG, "%s: n too large for one launch: %lld", who, (long long)n);
  if (!frame) return fail(FFMP_E_ARG, "%s: frame is NULL", who);
  if (!goal_ego) return fail(FFMP_E_ARG, "%s: goal_ego is NULL", who);
  if (goal_stride < 2) return fail(FFMP_E_ARG, "%s: goal_stride must be >= 2, got %lld", who, (long long)goal_stride);
  if (!dist2 && !potential && !grad && !robot_d2) return fail(FFMP_E_ARG, "%s: every output is NULL", who);
  const int64_t G2 = (int64_t)cfg->grid * cfg->grid;
  if (frame_env_stride < G2)
    return fail(FFMP_E_ARG, "%s: frame_env_stride %lld < G*G = %lld", who, (long long)frame_env_stride, (long long)G2);
  if (dist2 && dist2_env_stride < G2)
    return fail(FFMP_E_ARG, "%s: dist2_env_stride %lld < G*G = %lld", who, (long long)dist2_env_stride, (long long)G2);
  if (potential && potential_env_stride < G2)
    return fail(FFMP_E_ARG, "%s: potential_env_stride %lld < G*G = %lld", who, (long long)potential_env_stride, (long long)G2);
  if (((uintptr_t)frame & 3u) != 0 || (frame_env_stride % 4) != 0)
    return fail(FFMP_E_ARG, "%s: frame must be 4-byte aligned with frame_env_stride a multiple of 4 elements (frame alignment)", who);
  if (dist2 && (((uintptr_t)dist2 & 3u) != 0 || (dist2_env_stride % 4) != 0))
    return fail(FFMP_E_ARG, "%s: dist2 must be 4-byte aligned with dist2_env_stride a multiple of 4 elements (dist2 alignment)", who);
  if (potential && (((uintptr_t)potential & 3u) != 0 || (potential_env_stride % 4) != 0))
    return fail(FFMP_E_ARG, "%s: potential must be 4-byte aligned with potential_env_stride a multiple of 4 elements (potential alignment)", who);
  if (((uintptr_t)goal_ego & 3u) != 0) return fail(FFMP_E_ARG, "%s: goal_ego must be 4-byte aligned", who);
  if (grad && ((uintptr_t)grad & 3u) != 0) return fail(FFMP_E_ARG, "%s: grad must be 4-byte aligned", who);
  if (robot_d2 && ((uintptr_t)robot_d2 & 3u) != 0) return fail(FFMP_E_ARG, "%s: robot_d2 must be 4-byte aligned", who);
  const uint64_t fes = frame_format == FFMP_OBS_F32 ? 4u : 1u, pes = potential_format == FFMP_OBS_F32 ? 4u : 2u;
  if (n > 0) {
    const uint64_t last = (uint64_t)(n - 1);
    // the outputs given, as byte ranges; the frame last
    const void* ptr[5] = {dist2, potential, grad, robot_d2, frame};
    const uint64_t len[5] = {(last * (uint64_t)dist2_env_stride + (uint64_t)G2) * 2u,
                             (last * (uint64_t)potential_env_stride + (uint64_t)G2) * pes, 8u * (uint64_t)n, 4u * (uint64_t)n,
                             (last * (uint64_t)frame_env_stride + (uint64_t)G2) * fes};
    const char* name[5] = {"dist2", "potential", "grad", "robot_d2", "the frame"};
    for (int x = 0; x < 4; ++x)
      for (int y = x + 1; y < 5; ++y)
        if (ptr[x] && ptr[y] && pot_ranges_meet(ptr[x], len[x], ptr[y], len[y]))
          return fail(FFMP_E_ARG, "%s: %s overlaps %s", who, name[x], name[y]);
  }
  if (n == 0) return FFMP_OK;

  const PotPlan plan = pot_plan(cfg->grid, reach);
  PotArgs a;
  a.frame = frame;
  a.frame_stride = frame_env_stride;
  a.goal = goal_ego;
  a.goal_stride = goal_stride;
  a.mask = mask;
  a.dist2 = dist2;
  a.dist2_stride = dist2_env_stride;
  a.pot = potential;
  a.pot_stride = potential_env_stride;
  a.grad = grad;
  a.robot_d2 = robot_d2;
  a.res_f = cfg->res_f;
  a.half_f = cfg->half_f;
  a.half_ka_f = cfg->half_ka_f;
  a.half_kr_f = cfg->half_kr_f;
  a.rho0_f = cfg->rho0_f;
  a.inv_rho0_f = cfg->inv_rho0_f;
  a.rho_min_f = cfg->rho_min_f;
  a.inv_2res_f = cfg->inv_2res_f;
  a.G = cfg->grid;
  a.occ_min = occ_min;
  a.reach = reach;
  a.row_words = plan.row_words;
  a.grows = plan.grows;
  a.band = plan.band;
  a.tab_n = plan.tab_n;
  a.mask_words = plan.mask_words;
  // env strides are multiples of 4 elements: a float32 plane's stride is a multiple of 16 bytes, a 2-byte plane's of 8
  a.frame_vec = ((uintptr_t)frame & 15u) == 0 && (((uint64_t)frame_env_stride * fes) & 15u) == 0;
  a.dist2_vec = ((uintptr_t)dist2 & 7u) == 0;
  a.pot_vec = ((uintptr_t)potential & (potential_format == FFMP_OBS_F32 ? 15u : 7u)) == 0;
  const bool f32 = frame_format == FFMP_OBS_F32, p32 = potential_format == FFMP_OBS_F32;
  void (*k)(PotArgs) = f32 ? (p32 ? frame_potential_kernel<float, float> : frame_potential_kernel<float, _Float16>)
                           : (p32 ? frame_potential_kernel<uint8_t, float> : frame_potential_kernel<uint8_t, _Float16>);
  if (plan.lds > kPotLdsDefault) {
    // more than the default cap of dynamic LDS: ask for it, once per device and kernel (an attribute of the
    // function, no stream work)
    static std::atomic<uint64_t> asked[4];
    const int which = (f32 ? 2 : 0) + (p32 ? 1 : 0);
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return fail(FFMP_E_HIP, "%s: hipGetDevice failed", who);
    const uint64_t bit = 1ull << (dev & 63);
    if (!(asked[which].load() & bit)) {
      const size_t most = pot_plan(512, kPotMaxReach).lds;
      hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)most);
      if (err != hipSuccess)
        return fail(FFMP_E_HIP, "%s: hipFuncSetAttribute(%zu bytes of LDS): %s", who, most, hipGetErrorString(err));
      asked[which].fetch_or(bit);
    }
  }
  hipLaunchKernelGGL(k, dim3((unsigned)n), dim3((unsigned)plan.threads), plan.lds, (hipStream_t)stream, a);
  return launch_ok(who);
}

}  // extern "C"
