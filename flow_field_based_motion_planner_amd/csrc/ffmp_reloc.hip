// ffmp_reloc.hip — wide-prior and global relocalisation: ffmp_scan_match's winner over a window of up to 1024 cells
// and 512 rotation steps, found by a pruned two-level correlative search (include/ffmp.h ffmp_scan_relocalize carries
// the SPEC).  The scores are integer sums, so the upper bound is exact and the pruned search
// returns the exhaustive winner bit for bit.
//
// Six launches on the caller's stream, every intermediate in the caller's workspace (RelocPlan below):
//   1. reloc_xmax_kernel    X, the B x B sliding maximum of the zero-padded plane: separable, a row pass and a column
//                           pass through LDS per 16 x 128 tile; stored phase-major, X[p mod B][q mod B][p div B][q div B]
//                           (p, q counted from -(B - 1)), so lanes that own consecutive blocks read consecutive bytes.
//   2. reloc_coarse_kernel  one workgroup per (env, rotation): the rotation's `on` cell pairs are staged in LDS once (and
//                           kept in the workspace for 3 and 5), a lane owns whole blocks (A, Cc), Cc fastest, walks the
//                           list, stores U and keeps the largest (U, smallest index); one partial per rotation.
//   3. reloc_seed_kernel    per env: the seed block, S1 over its shifts, S(0,0,0) and the valid count.
//   4. reloc_compact_kernel the blocks with U >= S1 appended to the refined list (not launched with FFMP_RELOC_EXHAUSTIVE).
//   5. reloc_refine_kernel  `groups` workgroups per env stride over (refined block, shift) items with §5.18's inner
//                           loop on the map's bytes; the winner's order is a two-word compare (S, then 57 bits of tie
//                           fields), a total order, so neither the list's order nor the reduction's shows.  An env with
//                           no beam on in any rotation has every S = 0: its winner, (0, 0, 0), is written unvisited.
//   6. reloc_final_kernel   per env: the partial winners reduced, the gate, pose_out and info.
// Every X load's index is clamped before the load and the value dropped where the window misses the stored plane;
// every map load is behind its own bounds test; the list, the cell pairs and U are indexed below counts that the
// kernels wrote themselves.
#include <hip/hip_runtime.h>
#include <float.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "ffmp_host.h"

#pragma clang fp contract(off)

namespace {

constexpr int kRlThreads = 256;
constexpr int kRlMaxRadius = 1024, kRlMaxTurns = 512;
constexpr int kRlMaxGroups = 64;         // refinement workgroups per env
constexpr int kRlItemsPerGroup = 4096;   // (block, shift) items of the full set that earn one more workgroup
constexpr int kRlTileP = 16, kRlTileQ = 128;
constexpr int kRlMaxBlock = 16;
constexpr int kRlCompactGroups = 256;    // compaction workgroups per env, at most
constexpr int64_t kRlHeader = 64;        // int32 {refined, S1, S(0,0,0), valid, seed index, ...}

// The per-env workspace, byte offsets, every section a multiple of 16 bytes.
struct RelocPlan {
  int32_t K, nb, lb, B, Nq, NX, groups;
  int64_t nblocks;
  int64_t off_part;   // K uint64: per rotation the largest (U, smallest index)
  int64_t off_win;    // groups x {int32 S, pad, uint64 tie}: partial winners
  int64_t off_cnt;    // K int32: `on` beams per rotation
  int64_t off_cells;  // K x FFMP_MAX_BEAMS uint32 reserved, rows L apart: (fp + R) << 16 | (fq + R)
  int64_t off_U;      // K*nb*nb int32
  int64_t off_list;   // K*nb*nb int32: the refined blocks
  int64_t off_X;      // NX*NX int8
  int64_t bytes;
};

inline int64_t up16(int64_t v) { return (v + 15) & ~(int64_t)15; }

RelocPlan reloc_plan(int32_t cells, int32_t R, int32_t T, int32_t B) {
  RelocPlan p;
  p.B = B;
  p.lb = B == 2 ? 1 : B == 4 ? 2 : B == 8 ? 3 : 4;
  p.K = 2 * T + 1;
  p.nb = (2 * R + B) / B;
  p.nblocks = (int64_t)p.K * p.nb * p.nb;  // <= 1025^3 < 2^31
  p.Nq = (cells + B - 1 + B - 1) / B;
  p.NX = p.Nq * B;
  const int64_t items = p.nblocks * B * B;
  const int64_t g = (items + kRlItemsPerGroup - 1) / kRlItemsPerGroup;
  p.groups = (int32_t)(g < 1 ? 1 : g > kRlMaxGroups ? kRlMaxGroups : g);
  p.off_part = kRlHeader;
  p.off_win = p.off_part + up16((int64_t)p.K * 8);
  p.off_cnt = p.off_win + (int64_t)p.groups * 16;
  p.off_cells = p.off_cnt + up16((int64_t)p.K * 4);
  p.off_U = p.off_cells + (int64_t)p.K * FFMP_MAX_BEAMS * 4;
  p.off_list = p.off_U + up16(p.nblocks * 4);
  p.off_X = p.off_list + up16(p.nblocks * 4);
  p.bytes = p.off_X + up16((int64_t)p.NX * p.NX);
  return p;
}

struct RelocArgs {
  const float* ranges;
  int64_t ranges_stride;
  const float* beams;
  const float* pose;
  int64_t pose_stride;
  const uint8_t* mask;
  const int8_t* map;
  int64_t map_stride;
  const float* turns;
  float* pose_out;
  int32_t* info;
  int32_t* bounds;
  uint8_t* work;
  int32_t L, Wc, R, T, min_valid, min_gain, min_score, exhaustive;
  float rm, wh, res;
  RelocPlan p;
};

typedef int rl_i32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t rl_u32x4 __attribute__((ext_vector_type(4)));

struct RlWin {
  int32_t S;
  int32_t pad;
  uint64_t tie;
};

__device__ __forceinline__ bool rl_finite(float v) { return v - v == 0.0f; }

// X's byte at (pp, qq), both in 0..NX-1, counted from plane index -(B - 1)
__device__ __forceinline__ int rl_xi(int pp, int qq, const RelocPlan& p) {
#ifdef FFMP_RELOC_INTERLEAVED  // the plain plane, for the layout's measurement; not the build's
  return pp * p.NX + qq;
#else
  const int m = p.B - 1;
  return (((pp & m) << p.lb) | (qq & m)) * (p.Nq * p.Nq) + (pp >> p.lb) * p.Nq + (qq >> p.lb);
#endif
}

// ffmp_scan_match's order below the score, larger is better: the smaller a^2 + b^2, |k|, k, a, b.  57 bits.
__device__ __forceinline__ uint64_t rl_tie(int k, int a, int b, int R) {
  const uint32_t d2 = (uint32_t)(a * a + b * b), ak = (uint32_t)(k < 0 ? -k : k);
  return ((uint64_t)(0x3fffffu - d2) << 35) | ((uint64_t)(1023u - ak) << 25) | ((uint64_t)(k < 0 ? 1u : 0u) << 24) |
         ((uint64_t)(4095u - (uint32_t)(a + R)) << 12) | (uint64_t)(4095u - (uint32_t)(b + R));
}

__device__ __forceinline__ bool rl_better(int S, uint64_t tie, int S0, uint64_t tie0) {
  return S > S0 || (S == S0 && tie > tie0);
}

// §5.18's inner loop: the pairs hold (fp + R, fq + R); the candidate's cell is (fp + a, fq + b)
__device__ __forceinline__ int rl_score(const uint32_t* cells, int cnt, int dp, int dq, int Wc, const int8_t* mp) {
  int S = 0;
#pragma unroll 4
  for (int j = 0; j < cnt; ++j) {
    const uint32_t v = cells[j];
    const int p = (int)(v >> 16) + dp, q = (int)(v & 0xffffu) + dq;
    if ((unsigned)p < (unsigned)Wc && (unsigned)q < (unsigned)Wc) S += (int)mp[p * Wc + q];
  }
  return S;
}

__device__ __forceinline__ bool rl_skip(const RelocArgs& a, int64_t e) { return a.mask && a.mask[e] == 0; }

// ---------------------------------------------------------------- 1. the sliding maximum
__global__ __launch_bounds__(kRlThreads) void reloc_xmax_kernel(RelocArgs a) {
  constexpr int kInH = kRlTileP + kRlMaxBlock - 1, kInW = kRlTileQ + kRlMaxBlock - 1;
  __shared__ int8_t s_in[kInH * kInW];
  __shared__ int8_t s_row[kInH * kRlTileQ];
  const int64_t e = blockIdx.x;
  if (rl_skip(a, e)) return;
  const int tid = threadIdx.x, B = a.p.B, Wc = a.Wc, NX = a.p.NX;
  const int tilesQ = (NX + kRlTileQ - 1) / kRlTileQ;
  const int tp = (int)blockIdx.y / tilesQ, tq = (int)blockIdx.y - tp * tilesQ;
  const int p0 = tp * kRlTileP, q0 = tq * kRlTileQ;  // in X's coordinates: plane index + (B - 1)
  const int inH = kRlTileP + B - 1, inW = kRlTileQ + B - 1;
  const int8_t* mp = a.map + e * a.map_stride;
  for (int idx = tid; idx < inH * inW; idx += kRlThreads) {
    const int i = idx / inW, j = idx - i * inW;
    const int p = p0 - (B - 1) + i, q = q0 - (B - 1) + j;
    int8_t v = 0;
    if ((unsigned)p < (unsigned)Wc && (unsigned)q < (unsigned)Wc) v = mp[p * Wc + q];
    s_in[i * kInW + j] = v;
  }
  __syncthreads();
  for (int idx = tid; idx < inH * kRlTileQ; idx += kRlThreads) {
    const int i = idx / kRlTileQ, j = idx - i * kRlTileQ;
    int v = -128;
    for (int t = 0; t < B; ++t) v = max(v, (int)s_in[i * kInW + j + t]);
    s_row[i * kRlTileQ + j] = (int8_t)v;
  }
  __syncthreads();
  int8_t* X = reinterpret_cast<int8_t*>(a.work + e * a.p.bytes + a.p.off_X);
  const int per = kRlTileQ >> a.p.lb;  // blocks of columns per tile row
  for (int idx = tid; idx < kRlTileP * kRlTileQ; idx += kRlThreads) {
    const int i = idx / kRlTileQ, r = idx - i * kRlTileQ;
    const int ph = r / per, qd = r - ph * per;  // the column's phase, then its block: consecutive lanes, consecutive bytes
    const int j = (qd << a.p.lb) | ph;
    const int pp = p0 + i, qq = q0 + j;
    if (pp < NX && qq < NX) {
      int v = -128;
      for (int t = 0; t < B; ++t) v = max(v, (int)s_row[(i + t) * kRlTileQ + j]);
      X[rl_xi(pp, qq, a.p)] = (int8_t)v;
    }
  }
}

// ---------------------------------------------------------------- 2. the bounds
__global__ __launch_bounds__(kRlThreads) void reloc_coarse_kernel(RelocArgs a) {
  __shared__ uint32_t s_cell[FFMP_MAX_BEAMS];
  __shared__ uint64_t s_red[kRlThreads];
  __shared__ int s_cnt;
  const int64_t e = blockIdx.x;
  if (rl_skip(a, e)) return;
  const int tid = threadIdx.x, kk = blockIdx.y;
  const int L = a.L, Wc = a.Wc, R = a.R, B = a.p.B, nb = a.p.nb, NX = a.p.NX;
  const float* ps = a.pose + e * a.pose_stride;
  const float px = ps[0], py = ps[1], c = ps[2], s = ps[3];
  const bool finite = rl_finite(px) && rl_finite(py) && rl_finite(c) && rl_finite(s);
  uint8_t* ws = a.work + e * a.p.bytes;
  if (tid == 0) s_cnt = 0;
  __syncthreads();
  const float* rg = a.ranges + e * a.ranges_stride;
  const float rc = a.turns[2 * kk], rs = a.turns[2 * kk + 1];
  const float ck = c * rc - s * rs, sk = s * rc + c * rs;
  const float lo_f = (float)(-R), hi_f = (float)(Wc - 1 + R);
  for (int l = tid; l < L; l += kRlThreads) {
    const float r = rg[l];
    if ((r > 0.0f) && (r <= a.rm) && (r <= FLT_MAX)) {
      const float bx = r * a.beams[2 * l], by = r * a.beams[2 * l + 1];
      const float wx = (ck * bx - sk * by) + px;
      const float wy = (sk * bx + ck * by) + py;
      const float fp = rintf((wx + a.wh) / a.res);
      const float fq = rintf((wy + a.wh) / a.res);
      const bool on = finite && (fp >= lo_f) && (fp <= hi_f) && (fq >= lo_f) && (fq <= hi_f);
      if (on) {
        const int slot = atomicAdd(&s_cnt, 1);  // < L <= FFMP_MAX_BEAMS
        s_cell[slot] = ((uint32_t)((int)fp + R) << 16) | (uint32_t)((int)fq + R);
      }
    }
  }
  __syncthreads();
  const int cnt = s_cnt;
  uint32_t* wcells = reinterpret_cast<uint32_t*>(ws + a.p.off_cells) + (int64_t)kk * L;
  for (int j = tid; j < cnt; j += kRlThreads) wcells[j] = s_cell[j];
  if (tid == 0) reinterpret_cast<int32_t*>(ws + a.p.off_cnt)[kk] = cnt;

  const int8_t* X = reinterpret_cast<const int8_t*>(ws + a.p.off_X);
  int32_t* wU = reinterpret_cast<int32_t*>(ws + a.p.off_U) + (int64_t)kk * nb * nb;
  int32_t* bo = a.bounds ? a.bounds + (e * a.p.K + kk) * (int64_t)nb * nb : nullptr;
  uint64_t best = 0;
  for (int w = tid; w < nb * nb; w += kRlThreads) {
    const int A = w / nb, Cc = w - A * nb;
    // the pair holds (fp + R, fq + R); X's coordinate of fp + a0(A) is fp - R + A*B + (B - 1)
    const int dp = A * B + (B - 1) - 2 * R, dq = Cc * B + (B - 1) - 2 * R;
    int U = 0;
#pragma unroll 4
    for (int j = 0; j < cnt; ++j) {
      const uint32_t v = s_cell[j];
      const int pp = (int)(v >> 16) + dp, qq = (int)(v & 0xffffu) + dq;
      const bool in = (unsigned)pp < (unsigned)NX && (unsigned)qq < (unsigned)NX;
      const int val = (int)X[in ? rl_xi(pp, qq, a.p) : 0];
      U += in ? val : 0;
    }
    wU[w] = U;
    if (bo) bo[w] = U;
    const uint32_t lin = (uint32_t)(kk * nb * nb + w);
    const uint64_t key = ((uint64_t)(uint32_t)(U + (1 << 20)) << 32) | (uint64_t)(0xffffffffu - lin);  // |U| <= 1024 * 128
    best = key > best ? key : best;
  }
  s_red[tid] = best;
  __syncthreads();
  for (int h = kRlThreads / 2; h > 0; h >>= 1) {
    if (tid < h) {
      const uint64_t o = s_red[tid + h];
      if (o > s_red[tid]) s_red[tid] = o;
    }
    __syncthreads();
  }
  if (tid == 0) reinterpret_cast<uint64_t*>(ws + a.p.off_part)[kk] = s_red[0];
}

// ---------------------------------------------------------------- 3. the seed
__global__ __launch_bounds__(kRlThreads) void reloc_seed_kernel(RelocArgs a) {
  __shared__ uint64_t s_red[kRlThreads];
  __shared__ int s_int[kRlThreads];
  const int64_t e = blockIdx.x;
  if (rl_skip(a, e)) return;
  const int tid = threadIdx.x;
  const int L = a.L, Wc = a.Wc, R = a.R, T = a.T, B = a.p.B, nb = a.p.nb, K = a.p.K;
  uint8_t* ws = a.work + e * a.p.bytes;
  const int8_t* mp = a.map + e * a.map_stride;
  const uint64_t* part = reinterpret_cast<const uint64_t*>(ws + a.p.off_part);
  const int32_t* wcnt = reinterpret_cast<const int32_t*>(ws + a.p.off_cnt);
  const uint32_t* wcells = reinterpret_cast<const uint32_t*>(ws + a.p.off_cells);
  uint64_t best = 0;
  for (int k = tid; k < K; k += kRlThreads) best = part[k] > best ? part[k] : best;
  s_red[tid] = best;
  __syncthreads();
  for (int h = kRlThreads / 2; h > 0; h >>= 1) {
    if (tid < h) {
      const uint64_t o = s_red[tid + h];
      if (o > s_red[tid]) s_red[tid] = o;
    }
    __syncthreads();
  }
  const uint32_t lin = 0xffffffffu - (uint32_t)(s_red[0] & 0xffffffffu);  // < K*nb*nb
  const int kk = (int)(lin / (uint32_t)(nb * nb));
  const int rem = (int)lin - kk * nb * nb;
  const int A = rem / nb, Cc = rem - A * nb;
  // S1: the largest S over the seed's shifts
  int S1 = INT_MIN;
  if (tid < B * B) {
    const int ai = -R + A * B + (tid >> a.p.lb), bi = -R + Cc * B + (tid & (B - 1));
    if (ai <= R && bi <= R) S1 = rl_score(wcells + (int64_t)kk * L, wcnt[kk], ai - R, bi - R, Wc, mp);
  }
  s_int[tid] = S1;
  __syncthreads();
  for (int h = kRlThreads / 2; h > 0; h >>= 1) {
    if (tid < h) s_int[tid] = max(s_int[tid], s_int[tid + h]);
    __syncthreads();
  }
  S1 = s_int[0];
  __syncthreads();
  // S(0,0,0), the beams split over the threads
  int Sz = 0;
  {
    const uint32_t* cells = wcells + (int64_t)T * L;
    const int cnt = wcnt[T];
    for (int j = tid; j < cnt; j += kRlThreads) {
      const uint32_t v = cells[j];
      const int p = (int)(v >> 16) - R, q = (int)(v & 0xffffu) - R;
      if ((unsigned)p < (unsigned)Wc && (unsigned)q < (unsigned)Wc) Sz += (int)mp[p * Wc + q];
    }
  }
  s_int[tid] = Sz;
  __syncthreads();
  for (int h = kRlThreads / 2; h > 0; h >>= 1) {
    if (tid < h) s_int[tid] += s_int[tid + h];
    __syncthreads();
  }
  Sz = s_int[0];
  __syncthreads();
  int nv = 0;
  const float* rg = a.ranges + e * a.ranges_stride;
  for (int l = tid; l < L; l += kRlThreads) {
    const float r = rg[l];
    nv += ((r > 0.0f) && (r <= a.rm) && (r <= FLT_MAX)) ? 1 : 0;
  }
  s_int[tid] = nv;
  __syncthreads();
  for (int h = kRlThreads / 2; h > 0; h >>= 1) {
    if (tid < h) s_int[tid] += s_int[tid + h];
    __syncthreads();
  }
  nv = s_int[0];
  __syncthreads();
  int on = 0;  // beams on over all rotations: 0 leaves every score 0, which the refinement need not visit
  for (int k = tid; k < K; k += kRlThreads) on += wcnt[k];
  s_int[tid] = on;
  __syncthreads();
  for (int h = kRlThreads / 2; h > 0; h >>= 1) {
    if (tid < h) s_int[tid] += s_int[tid + h];
    __syncthreads();
  }
  if (tid == 0) {
    rl_i32x4 h;
    h[0] = a.exhaustive ? (int32_t)a.p.nblocks : 0;  // the refined count: the compaction adds to it
    h[1] = S1;
    h[2] = Sz;
    h[3] = nv;
    *reinterpret_cast<rl_i32x4*>(ws) = h;
    reinterpret_cast<int32_t*>(ws)[4] = (int32_t)lin;
    reinterpret_cast<int32_t*>(ws)[5] = s_int[0];
  }
}

// ---------------------------------------------------------------- 4. the refined list
__global__ __launch_bounds__(kRlThreads) void reloc_compact_kernel(RelocArgs a) {
  __shared__ int s_n, s_base;
  const int64_t e = blockIdx.x;
  if (rl_skip(a, e)) return;
  const int tid = threadIdx.x;
  uint8_t* ws = a.work + e * a.p.bytes;
  int32_t* hdr = reinterpret_cast<int32_t*>(ws);
  const int32_t* wU = reinterpret_cast<const int32_t*>(ws + a.p.off_U);
  int32_t* list = reinterpret_cast<int32_t*>(ws + a.p.off_list);
  const int S1 = hdr[1];
  const int64_t nblocks = a.p.nblocks;
  for (int64_t i0 = (int64_t)blockIdx.y * kRlThreads; i0 < nblocks; i0 += (int64_t)gridDim.y * kRlThreads) {  // uniform
    if (tid == 0) s_n = 0;
    __syncthreads();
    const int64_t i = i0 + tid;
    const bool keep = i < nblocks && wU[i] >= S1;
    int slot = 0;
    if (keep) slot = atomicAdd(&s_n, 1);
    __syncthreads();
    if (tid == 0) s_base = s_n ? atomicAdd(&hdr[0], s_n) : 0;  // the total stays <= nblocks: every block is counted once
    __syncthreads();
    if (keep && (int64_t)s_base + slot < nblocks) list[s_base + slot] = (int32_t)i;
    __syncthreads();
  }
}

// ---------------------------------------------------------------- 5. the refinement
__global__ __launch_bounds__(kRlThreads) void reloc_refine_kernel(RelocArgs a) {
  __shared__ int s_S[kRlThreads];
  __shared__ uint64_t s_t[kRlThreads];
  const int64_t e = blockIdx.x;
  if (rl_skip(a, e)) return;
  const int tid = threadIdx.x;
  const int L = a.L, Wc = a.Wc, R = a.R, T = a.T, B = a.p.B, nb = a.p.nb, lb = a.p.lb;
  uint8_t* ws = a.work + e * a.p.bytes;
  const int8_t* mp = a.map + e * a.map_stride;
  const int32_t* hdr = reinterpret_cast<const int32_t*>(ws);
  const int32_t* wcnt = reinterpret_cast<const int32_t*>(ws + a.p.off_cnt);
  const uint32_t* wcells = reinterpret_cast<const uint32_t*>(ws + a.p.off_cells);
  const int32_t* list = reinterpret_cast<const int32_t*>(ws + a.p.off_list);
  if (hdr[5] == 0 && !a.exhaustive) {
    // no beam is on in any rotation (an empty scan, a non-finite pose): every S is 0 and every block is refined; the
    // winner of that set is (0, 0, 0) by the tie order, without a visit to its (2T+1)(2R+1)^2 shifts
    if (tid == 0) {
      RlWin w;
      w.S = blockIdx.y == 0 ? 0 : INT_MIN;
      w.pad = 0;
      w.tie = blockIdx.y == 0 ? rl_tie(0, 0, 0, R) : 0;
      reinterpret_cast<RlWin*>(ws + a.p.off_win)[blockIdx.y] = w;
    }
    return;
  }
  int64_t refined = hdr[0];
  if (refined > a.p.nblocks) refined = a.p.nblocks;  // never past the list
  const int64_t items = refined << (2 * lb);
  const uint32_t nb2 = (uint32_t)(nb * nb);
  int bS = INT_MIN;
  uint64_t bt = 0;
  for (int64_t it = (int64_t)blockIdx.y * kRlThreads + tid; it < items; it += (int64_t)gridDim.y * kRlThreads) {
    const int64_t bi = it >> (2 * lb);
    const int sh = (int)(it & (int64_t)(B * B - 1));
    const uint32_t blk = a.exhaustive ? (uint32_t)bi : (uint32_t)list[bi];
    if (blk >= (uint32_t)a.p.nblocks) continue;
    const int kk = (int)(blk / nb2);
    const int rem = (int)(blk - (uint32_t)kk * nb2);
    const int A = rem / nb, Cc = rem - A * nb;
    const int ai = -R + A * B + (sh >> lb), bi2 = -R + Cc * B + (sh & (B - 1));  // b fastest: consecutive bytes
    if (ai > R || bi2 > R) continue;
    const int S = rl_score(wcells + (int64_t)kk * L, wcnt[kk], ai - R, bi2 - R, Wc, mp);
    const uint64_t tie = rl_tie(kk - T, ai, bi2, R);
    if (rl_better(S, tie, bS, bt)) {
      bS = S;
      bt = tie;
    }
  }
  s_S[tid] = bS;
  s_t[tid] = bt;
  __syncthreads();
  for (int h = kRlThreads / 2; h > 0; h >>= 1) {
    if (tid < h && rl_better(s_S[tid + h], s_t[tid + h], s_S[tid], s_t[tid])) {
      s_S[tid] = s_S[tid + h];
      s_t[tid] = s_t[tid + h];
    }
    __syncthreads();
  }
  if (tid == 0) {
    RlWin w;
    w.S = s_S[0];
    w.pad = 0;
    w.tie = s_t[0];
    reinterpret_cast<RlWin*>(ws + a.p.off_win)[blockIdx.y] = w;
  }
}

// ---------------------------------------------------------------- 6. the winner, the gate, the outputs
__global__ __launch_bounds__(64) void reloc_final_kernel(RelocArgs a) {
  __shared__ int s_S[64];
  __shared__ uint64_t s_t[64];
  const int64_t e = blockIdx.x;
  if (rl_skip(a, e)) return;
  const int tid = threadIdx.x;
  const int R = a.R, T = a.T;
  const uint8_t* ws = a.work + e * a.p.bytes;
  const RlWin* win = reinterpret_cast<const RlWin*>(ws + a.p.off_win);
  int bS = INT_MIN;
  uint64_t bt = 0;
  for (int g = tid; g < a.p.groups; g += 64) {
    const RlWin w = win[g];
    if (rl_better(w.S, w.tie, bS, bt)) {
      bS = w.S;
      bt = w.tie;
    }
  }
  s_S[tid] = bS;
  s_t[tid] = bt;
  __syncthreads();
  for (int h = 32; h > 0; h >>= 1) {
    if (tid < h && rl_better(s_S[tid + h], s_t[tid + h], s_S[tid], s_t[tid])) {
      s_S[tid] = s_S[tid + h];
      s_t[tid] = s_t[tid + h];
    }
    __syncthreads();
  }
  if (tid != 0) return;
  const int32_t* hdr = reinterpret_cast<const int32_t*>(ws);
  const int S_best = s_S[0];
  const uint64_t tie = s_t[0];
  const int b_w = (4095 - (int)(tie & 4095u)) - R;
  const int a_w = (4095 - (int)((tie >> 12) & 4095u)) - R;
  const int ak = 1023 - (int)((tie >> 25) & 1023u);
  int k_w = ((tie >> 24) & 1u) ? -ak : ak;
  k_w = max(-T, min(T, k_w));  // the table's index below stays inside it whatever the words hold
  const int S_zero = hdr[2], nv = hdr[3];
  const float* ps = a.pose + e * a.pose_stride;
  const float px = ps[0], py = ps[1], c = ps[2], s = ps[3];
  const bool finite = rl_finite(px) && rl_finite(py) && rl_finite(c) && rl_finite(s);
  const bool moved = k_w != 0 || a_w != 0 || b_w != 0;
  const bool ok = finite && nv >= a.min_valid && ((int64_t)S_best - (int64_t)S_zero >= (int64_t)a.min_gain) && moved && S_best >= a.min_score;
  if (a.pose_out) {
    rl_u32x4 out;
    if (ok) {
      const float rc = a.turns[2 * (k_w + T)], rs = a.turns[2 * (k_w + T) + 1];
      const float ck = c * rc - s * rs, sk = s * rc + c * rs;
      const float da = (float)a_w * a.res, db = (float)b_w * a.res;
      out[0] = __float_as_uint(px + da);
      out[1] = __float_as_uint(py + db);
      out[2] = __float_as_uint(ck);
      out[3] = __float_as_uint(sk);
    } else {
      const uint32_t* raw = reinterpret_cast<const uint32_t*>(ps);
      out[0] = raw[0];
      out[1] = raw[1];
      out[2] = raw[2];
      out[3] = raw[3];
    }
    *reinterpret_cast<rl_u32x4*>(a.pose_out + 4 * e) = out;
  }
  if (a.info) {
    rl_i32x4 i0, i1;
    i0[0] = ok ? 1 : 0;
    i0[1] = ok ? k_w : 0;
    i0[2] = ok ? a_w : 0;
    i0[3] = ok ? b_w : 0;
    i1[0] = S_best;
    i1[1] = S_zero;
    i1[2] = nv;
    i1[3] = hdr[0];
    rl_i32x4* dst = reinterpret_cast<rl_i32x4*>(a.info + 8 * e);
    dst[0] = i0;
    dst[1] = i1;
  }
}

int reloc_check(const char* who, const ffmp_cfg_t* cfg, int32_t n_beams, int32_t cells, int32_t radius, int32_t n_turns,
                int32_t block, float range_max, int32_t min_valid, int32_t min_gain, int32_t flags) {
  if (!cfg) return fail(FFMP_E_ARG, "%s: cfg is NULL", who);
  if (cells < 8 || cells > 2048 || (cells % 4) != 0)
    return fail(FFMP_E_ARG, "%s: cells must be a multiple of 4 in [8,2048], got %d", who, cells);
  if (!(cfg->res_f > 0.0f) || isinf(cfg->res_f)) return fail(FFMP_E_ARG, "%s: cfg.res_f must be > 0 and finite", who);
  if (n_beams < 1 || n_beams > FFMP_MAX_BEAMS)
    return fail(FFMP_E_ARG, "%s: n_beams must be in [1,%d], got %d", who, FFMP_MAX_BEAMS, n_beams);
  if (!(range_max > 0.0f)) return fail(FFMP_E_ARG, "%s: range_max must be > 0 (or +inf) and not NaN", who);
  if (radius < 0 || radius > kRlMaxRadius) return fail(FFMP_E_ARG, "%s: radius must be in [0,%d], got %d", who, kRlMaxRadius, radius);
  if (n_turns < 0 || n_turns > kRlMaxTurns) return fail(FFMP_E_ARG, "%s: n_turns must be in [0,%d], got %d", who, kRlMaxTurns, n_turns);
  if (block != 2 && block != 4 && block != 8 && block != 16) return fail(FFMP_E_ARG, "%s: block must be 2, 4, 8 or 16, got %d", who, block);
  if (min_valid < 0) return fail(FFMP_E_ARG, "%s: min_valid must be >= 0, got %d", who, min_valid);
  if (min_gain < 0) return fail(FFMP_E_ARG, "%s: min_gain must be >= 0, got %d", who, min_gain);
  if (flags & ~FFMP_RELOC_EXHAUSTIVE) return fail(FFMP_E_ARG, "%s: unknown flags 0x%x", who, flags);
  return FFMP_OK;
}

// [p, p + bytes) against [q, q + qbytes)
bool rl_overlaps(const void* p, uint64_t bytes, const void* q, uint64_t qbytes) {
  const uintptr_t a0 = (uintptr_t)p, a1 = a0 + bytes, m0 = (uintptr_t)q, m1 = m0 + qbytes;
  return a0 < m1 && m0 < a1;
}

}  // namespace

extern "C" {

int ffmp_scan_relocalize_check(const ffmp_cfg_t* cfg, int32_t n_beams, int32_t cells, int32_t radius, int32_t n_turns,
                               int32_t block, float range_max, int32_t min_valid, int32_t min_gain, int32_t flags) {
  return reloc_check("ffmp_scan_relocalize", cfg, n_beams, cells, radius, n_turns, block, range_max, min_valid, min_gain, flags);
}

int64_t ffmp_scan_relocalize_work(int32_t cells, int32_t radius, int32_t n_turns, int32_t block) {
  const char* who = "ffmp_scan_relocalize_work";
  if (cells < 8 || cells > 2048 || (cells % 4) != 0) return fail(FFMP_E_ARG, "%s: cells must be a multiple of 4 in [8,2048], got %d", who, cells);
  if (radius < 0 || radius > kRlMaxRadius) return fail(FFMP_E_ARG, "%s: radius must be in [0,%d], got %d", who, kRlMaxRadius, radius);
  if (n_turns < 0 || n_turns > kRlMaxTurns) return fail(FFMP_E_ARG, "%s: n_turns must be in [0,%d], got %d", who, kRlMaxTurns, n_turns);
  if (block != 2 && block != 4 && block != 8 && block != 16) return fail(FFMP_E_ARG, "%s: block must be 2, 4, 8 or 16, got %d", who, block);
  return reloc_plan(cells, radius, n_turns, block).bytes;
}

int ffmp_scan_relocalize(const ffmp_cfg_t* cfg, int64_t n, const float* ranges, int64_t ranges_stride, int32_t n_beams,
                         const float* beams, const float* pose, int64_t pose_stride, const uint8_t* mask, const int8_t* map,
                         int64_t map_env_stride, int32_t cells, const float* turns, int32_t n_turns, int32_t radius,
                         int32_t block, float range_max, int32_t min_valid, int32_t min_gain, int32_t min_score,
                         float* pose_out, int32_t* info, int32_t* bounds, void* work, int64_t work_bytes, int32_t flags,
                         void* stream) {
  const char* who = "ffmp_scan_relocalize";
  if (int rc = reloc_check(who, cfg, n_beams, cells, radius, n_turns, block, range_max, min_valid, min_gain, flags)) return rc;
  if (n < 0) return fail(FFMP_E_ARG, "%s: negative n", who);
  if (!ranges) return fail(FFMP_E_ARG, "%s: ranges is NULL", who);
  if (!beams) return fail(FFMP_E_ARG, "%s: beams is NULL", who);
  if (!pose) return fail(FFMP_E_ARG, "%s: pose is NULL", who);
  if (!map) return fail(FFMP_E_ARG, "%s: map is NULL", who);
  if (!turns) return fail(FFMP_E_ARG, "%s: turns is NULL", who);
  if (!pose_out && !info && !bounds) return fail(FFMP_E_ARG, "%s: pose_out, info and bounds are all NULL", who);
  if (!work) return fail(FFMP_E_ARG, "%s: work is NULL", who);
  if (ranges_stride < n_beams)
    return fail(FFMP_E_ARG, "%s: ranges_stride %lld < n_beams = %d", who, (long long)ranges_stride, n_beams);
  if (pose_stride < 4) return fail(FFMP_E_ARG, "%s: pose_stride %lld < 4", who, (long long)pose_stride);
  const int64_t W2 = (int64_t)cells * cells;
  if (map_env_stride < W2)
    return fail(FFMP_E_ARG, "%s: map_env_stride %lld < cells*cells = %lld", who, (long long)map_env_stride, (long long)W2);
  if (((uintptr_t)map & 3u) != 0 || (map_env_stride % 4) != 0)
    return fail(FFMP_E_ARG, "%s: the map must be 4-byte aligned with map_env_stride a multiple of 4 (map alignment)", who);
  if (((uintptr_t)pose_out & 15u) != 0) return fail(FFMP_E_ARG, "%s: pose_out must be 16-byte aligned (output alignment)", who);
  if (((uintptr_t)info & 15u) != 0) return fail(FFMP_E_ARG, "%s: info must be 16-byte aligned (output alignment)", who);
  if (((uintptr_t)bounds & 3u) != 0) return fail(FFMP_E_ARG, "%s: bounds must be 4-byte aligned (output alignment)", who);
  if (((uintptr_t)work & 15u) != 0) return fail(FFMP_E_ARG, "%s: work must be 16-byte aligned (workspace alignment)", who);
  if (n > 0x7fffffffLL) return fail(FFMP_E_ARG, "%s: n too large for one launch: %lld", who, (long long)n);
  const RelocPlan plan = reloc_plan(cells, radius, n_turns, block);
  if (work_bytes < 0 || (n > 0 && work_bytes / n < plan.bytes))
    return fail(FFMP_E_ARG, "%s: work_bytes %lld < n * %lld bytes per env (ffmp_scan_relocalize_work)", who, (long long)work_bytes,
                (long long)plan.bytes);
  if (n == 0) return FFMP_OK;
  const uint64_t map_bytes = (uint64_t)(n - 1) * (uint64_t)map_env_stride + (uint64_t)W2;
  const uint64_t ws_bytes = (uint64_t)n * (uint64_t)plan.bytes;
  const uint64_t bounds_bytes = (uint64_t)n * (uint64_t)plan.nblocks * 4u;
  if (pose_out && rl_overlaps(pose_out, (uint64_t)n * 16u, map, map_bytes)) return fail(FFMP_E_ARG, "%s: pose_out overlaps the map", who);
  if (info && rl_overlaps(info, (uint64_t)n * 32u, map, map_bytes)) return fail(FFMP_E_ARG, "%s: info overlaps the map", who);
  if (bounds && rl_overlaps(bounds, bounds_bytes, map, map_bytes)) return fail(FFMP_E_ARG, "%s: bounds overlaps the map", who);
  if (rl_overlaps(work, ws_bytes, map, map_bytes)) return fail(FFMP_E_ARG, "%s: work overlaps the map", who);
  if (pose_out && rl_overlaps(pose_out, (uint64_t)n * 16u, work, ws_bytes)) return fail(FFMP_E_ARG, "%s: pose_out overlaps the workspace", who);
  if (info && rl_overlaps(info, (uint64_t)n * 32u, work, ws_bytes)) return fail(FFMP_E_ARG, "%s: info overlaps the workspace", who);
  if (bounds && rl_overlaps(bounds, bounds_bytes, work, ws_bytes)) return fail(FFMP_E_ARG, "%s: bounds overlaps the workspace", who);

  RelocArgs a;
  a.ranges = ranges;
  a.ranges_stride = ranges_stride;
  a.beams = beams;
  a.pose = pose;
  a.pose_stride = pose_stride;
  a.mask = mask;
  a.map = map;
  a.map_stride = map_env_stride;
  a.turns = turns;
  a.pose_out = pose_out;
  a.info = info;
  a.bounds = bounds;
  a.work = static_cast<uint8_t*>(work);
  a.L = n_beams;
  a.Wc = cells;
  a.R = radius;
  a.T = n_turns;
  a.min_valid = min_valid;
  a.min_gain = min_gain;
  a.min_score = min_score;
  a.exhaustive = (flags & FFMP_RELOC_EXHAUSTIVE) ? 1 : 0;
  a.rm = range_max;
  a.wh = (float)((double)cells * cfg->res / 2.0);  // wh_f of ffmp_world_map
  a.res = cfg->res_f;
  a.p = plan;
  hipStream_t st = (hipStream_t)stream;
  const unsigned ne = (unsigned)n;
  const int tilesP = (plan.NX + kRlTileP - 1) / kRlTileP, tilesQ = (plan.NX + kRlTileQ - 1) / kRlTileQ;
  hipLaunchKernelGGL(reloc_xmax_kernel, dim3(ne, (unsigned)(tilesP * tilesQ)), dim3(kRlThreads), 0, st, a);
  hipLaunchKernelGGL(reloc_coarse_kernel, dim3(ne, (unsigned)plan.K), dim3(kRlThreads), 0, st, a);
  hipLaunchKernelGGL(reloc_seed_kernel, dim3(ne), dim3(kRlThreads), 0, st, a);
  if (!a.exhaustive) {
    const int64_t cg = (plan.nblocks + kRlThreads - 1) / kRlThreads;
    hipLaunchKernelGGL(reloc_compact_kernel, dim3(ne, (unsigned)(cg > kRlCompactGroups ? kRlCompactGroups : cg)), dim3(kRlThreads), 0, st, a);
  }
  hipLaunchKernelGGL(reloc_refine_kernel, dim3(ne, (unsigned)plan.groups), dim3(kRlThreads), 0, st, a);
  hipLaunchKernelGGL(reloc_final_kernel, dim3(ne), dim3(64), 0, st, a);
  return launch_ok(who);
}

}  // extern "C"
