// ffmp_flowest.hip — motion flow estimated from two scan frames (include/ffmp.h ffmp_scan_flow carries the
// SPEC).  A source of its own: the code objects of the scan kernels stay what they are.
//
// One workgroup of 256 threads per env.  The SPEC is bit arithmetic, so the planes are kept as bits in LDS:
//   Hc  the hits of the current frame,
//   Hp  the hits of the earlier frame, gathered through the warp (scan_map_kernel's index arithmetic),
//   S   (Hc & !D(Hp)) | (Hp & !D(Hc)): the two terms of the static-gate cost are disjoint (the first lies
//       in !Hp, the second in Hp), so c0 is the population of S over the block and the two dilated planes
//       never have to be kept.
// A row is ceil(G/32) words plus one zero word at either end, and there are 8 zero rows above and below
// (radius + block <= 8): a read up to 8 cells past an edge needs no branch.  3 * (G + 16) * (ceil(G/32) + 2)
// words: 3.8 KiB at G = 64, 114,048 bytes at G = 512 (one workgroup per CU there).
//
// Phase 1: 4-byte loads of `cur`, four 1-byte loads of `prev` at the warped cells (an index is formed only
// for an inside cell), the 4 bits of a lane OR-ed into the LDS word (ds_or: hits are sparse, most lanes add
// nothing).  Then S, one word per thread from three rows of either plane.
// Phase 2: a wave task is 256 consecutive cells, 4 per lane.  A task without a hit (one ballot) stores its
// zeros and is done: that is the common case and those stores are the kernel's HBM traffic.  Otherwise the
// hit cells of the task are compacted into a per-wave list in LDS (popcount + prefix over the lanes), every
// lane takes whole cells off the list — the search is up to 121 displacements and the hits are a few per
// cent of the cells, so a per-lane loop would leave most lanes idle — and writes a 10-bit code per cell
// back into LDS; the lanes then read the codes of their own 4 cells and store them: 16-byte stores of
// float32 flow (8-byte of binary16), 4-byte stores of the kinds.  (Storing the zeros of a lane without a hit
// in phase 1 already, under the loads, was measured and is slower: DESIGN §10.7.)
//
// The block of a cell is a signature of (2B+1) rows x (2B+1) bits, rows packed at a stride of 21 bits, three
// to a uint64 (the 17-bit search window of a row fits the stride, so one shift moves three rows at once):
// every cost is a population count of an XOR.  The visiting order of the SPEC is "the smallest
// (cost, du² + dv², du, dv)": the key is one integer and the displacements are visited row by row of the
// earlier plane, each row read from LDS once.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <atomic>

#include "ffmp_device.h"
#include "ffmp_host.h"

#pragma clang fp contract(off)

namespace {

using namespace ffmp;

#ifndef FFMP_FLOW_THREADS
#define FFMP_FLOW_THREADS 256
#endif
constexpr int kFlowThreads = FFMP_FLOW_THREADS;
constexpr int kFlowWaves = kFlowThreads / 64;
constexpr int kFlowTask = 256;   // cells of a wave task: 4 per lane
constexpr int kFlowGuard = 8;    // zero rows above and below: radius + block <= 8
constexpr int kFlowMaxR = 5, kFlowMaxB = 3;
constexpr int kFlowPack = 21;    // bits between two packed rows of a signature
constexpr size_t kFlowWaveLds = kFlowTask + 2 * kFlowTask;  // bytes per wave: the list (uint8), the codes (uint16)
constexpr size_t kFlowLdsDefault = 64 * 1024;

struct FlowArgs {
  const uint8_t* cur;
  const uint8_t* prev;
  int64_t frame_stride;  // bytes
  const float* pose_now;
  int64_t pose_now_stride;
  const float* pose_prev;
  int64_t pose_prev_stride;
  const uint8_t* mask;
  const uint8_t* first;
  void* flow;
  int64_t flow_stride;   // elements
  uint8_t* kind;         // or NULL
  int64_t kind_stride;   // bytes
  float scale;
  int32_t R, B, gate, min_hits;
};

typedef float flow_f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 flow_f16x4 __attribute__((ext_vector_type(4)));

__host__ __device__ constexpr int flow_wpr(int G) { return (G + 31) >> 5; }
__host__ __device__ constexpr int flow_row_words(int G) { return flow_wpr(G) + 2; }
__host__ __device__ constexpr int flow_plane_words(int G) { return (G + 2 * kFlowGuard) * flow_row_words(G); }
__host__ __device__ constexpr int flow_planes_words(int G) { return (3 * flow_plane_words(G) + 3) & ~3; }  // 16-byte aligned end
size_t flow_lds_bytes(int G) { return (size_t)flow_planes_words(G) * 4 + kFlowWaves * kFlowWaveLds; }

// q / G for 0 <= q < 2^24: the float quotient is within one of it
FFMP_DEV int flow_div(int q, int G, float invG) {
  int i = (int)((float)q * invG);
  if (i * G > q) --i;
  if ((i + 1) * G <= q) ++i;
  return i;
}

// 32 bits of row `row` (-8 .. G+7) of a plane starting at column c (-32 <= c): the caller masks what it wants
FFMP_DEV uint32_t flow_bits(const uint32_t* plane, int RS, int row, int c) {
  const int p = c + 32, w = p >> 5, sh = p & 31;
  const uint32_t* r = plane + (row + kFlowGuard) * RS + w;
  const uint64_t pair = (uint64_t)r[0] | ((uint64_t)r[1] << 32);
  return (uint32_t)(pair >> sh);
}

FFMP_DEV void flow_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the code of hit cell (i, j): kind | (du + 5) << 2 | (dv + 5) << 6
FFMP_DEV uint32_t flow_cell(const uint32_t* Hc, const uint32_t* Hp, const uint32_t* S, int RS, int i, int j, int R, int B,
                            int gate, int min_hits) {
  const uint32_t m = (1u << (2 * B + 1)) - 1u;
  const uint64_t m3 = (uint64_t)m | ((uint64_t)m << kFlowPack) | ((uint64_t)m << (2 * kFlowPack));
  // the block of the current frame as a signature, and the static-gate cost
  uint64_t hs[3] = {0, 0, 0};
  int c0 = 0;
#pragma unroll
  for (int s = 0; s < 2 * kFlowMaxB + 1; ++s) {
    const int a = s - kFlowMaxB;
    const bool on = a >= -B && a <= B;  // uniform
    const uint32_t x = on ? flow_bits(Hc, RS, i + a, j - B) & m : 0u;
    const uint32_t y = on ? flow_bits(S, RS, i + a, j - B) & m : 0u;
    hs[s / 3] |= (uint64_t)x << (kFlowPack * (s % 3));
    c0 += __popc(y);
  }
  const int nc = __popcll(hs[0]) + __popcll(hs[1]) + __popc((uint32_t)hs[2]);
  if (nc < min_hits) return 0u;
  if (c0 <= gate) return 1u | (5u << 2) | (5u << 6);

  // the search: slot s holds the 17-bit window (columns j-8 .. j+8) of row i + (s - 3) - du of the earlier
  // plane; from one du to the next every slot takes its neighbour's row and slot 0 reads one new row
  uint32_t r[2 * kFlowMaxB + 1];
  uint32_t on[2 * kFlowMaxB + 1];
#pragma unroll
  for (int s = 0; s < 2 * kFlowMaxB + 1; ++s) {
    const int a = s - kFlowMaxB;
    on[s] = (a >= -B && a <= B) ? 0x1FFFFu : 0u;
    r[s] = flow_bits(Hp, RS, i + a + R, j - kFlowGuard);
  }
  uint32_t best = 0xFFFFFFFFu;
  for (int du = -R; du <= R; ++du) {
    const uint64_t pa = (uint64_t)(r[0] & on[0]) | ((uint64_t)(r[1] & on[1]) << kFlowPack) | ((uint64_t)(r[2] & on[2]) << (2 * kFlowPack));
    const uint64_t pb = (uint64_t)(r[3] & on[3]) | ((uint64_t)(r[4] & on[4]) << kFlowPack) | ((uint64_t)(r[5] & on[5]) << (2 * kFlowPack));
    const uint32_t pc = r[6] & on[6];
    const uint32_t kdu = (uint32_t)(du * du) << 8 | (uint32_t)(du + 5) << 4;
    for (int dv = -R; dv <= R; ++dv) {
      const int sh = kFlowGuard - B - dv;  // 0 .. 12: bit 0 of the result is column j - B - dv
      const uint64_t a1 = (pa >> sh) & m3, b1 = (pb >> sh) & m3;
      const uint32_t c1 = (pc >> sh) & m;
      const int npd = __popcll(a1) + __popcll(b1) + __popc(c1);
      const int cost = __popcll(a1 ^ hs[0]) + __popcll(b1 ^ hs[1]) + __popc(c1 ^ (uint32_t)hs[2]);
      const uint32_t key = ((uint32_t)cost << 16) + kdu + ((uint32_t)(dv * dv) << 8) + (uint32_t)(dv + 5);
      if (npd >= min_hits) best = min(best, key);
    }
    if (du < R) {
#pragma unroll
      for (int s = 2 * kFlowMaxB; s > 0; --s) r[s] = r[s - 1];
      r[0] = flow_bits(Hp, RS, i - kFlowMaxB - (du + 1), j - kFlowGuard);
    }
  }
  if (best == 0xFFFFFFFFu) return 0u;
  return 2u | (((best >> 4) & 15u) << 2) | ((best & 15u) << 6);
}

template <int FMT>
FFMP_DEV void flow_store(const FlowArgs& a, int64_t e, int G2, int q, const uint32_t code[4]) {
  float vx[4], vy[4];
  uint32_t kinds = 0;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const uint32_t k = code[u] & 3u;
    const int du = (int)((code[u] >> 2) & 15u) - 5, dv = (int)((code[u] >> 6) & 15u) - 5;
    vx[u] = k == 2u ? (float)du * a.scale : 0.0f;
    vy[u] = k == 2u ? (float)dv * a.scale : 0.0f;
    kinds |= k << (8 * u);
  }
  if (FMT == FFMP_OBS_F32) {
    float* f = reinterpret_cast<float*>(a.flow) + e * a.flow_stride + q;
    flow_f32x4 x, y;
#pragma unroll
    for (int u = 0; u < 4; ++u) { x[u] = vx[u]; y[u] = vy[u]; }
    *reinterpret_cast<flow_f32x4*>(f) = x;
    *reinterpret_cast<flow_f32x4*>(f + G2) = y;
  } else {
    _Float16* f = reinterpret_cast<_Float16*>(a.flow) + e * a.flow_stride + q;
    flow_f16x4 x, y;
#pragma unroll
    for (int u = 0; u < 4; ++u) { x[u] = (_Float16)vx[u]; y[u] = (_Float16)vy[u]; }  // round to nearest even
    *reinterpret_cast<flow_f16x4*>(f) = x;
    *reinterpret_cast<flow_f16x4*>(f + G2) = y;
  }
  if (a.kind) *reinterpret_cast<uint32_t*>(a.kind + e * a.kind_stride + q) = kinds;
}

template <int FMT>
__global__ __launch_bounds__(kFlowThreads) void scan_flow_kernel(ffmp_cfg_t cfg, FlowArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t flow_lds[];
  const int G = cfg.grid, G2 = G * G, hg = G >> 1;
  const int RS = flow_row_words(G), PW = flow_plane_words(G), wpr = flow_wpr(G);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t e = blockIdx.x;
  if (a.mask && a.mask[e] == 0) return;  // block-uniform

  uint32_t* Hc = flow_lds;
  uint32_t* Hp = flow_lds + PW;
  uint32_t* S = flow_lds + 2 * PW;
  uint8_t* list = reinterpret_cast<uint8_t*>(flow_lds + flow_planes_words(G)) + wave * kFlowWaveLds;
  uint16_t* codes = reinterpret_cast<uint16_t*>(list + kFlowTask);

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

  const uint32_t zero[4] = {0u, 0u, 0u, 0u};
  if (restart) {  // block-uniform: kind 0 and flow 0 everywhere
    for (int q = 4 * tid; q < G2; q += 4 * kFlowThreads) flow_store<FMT>(a, e, G2, q, zero);
    return;
  }

  for (int w = tid; w < 3 * PW; w += kFlowThreads) flow_lds[w] = 0u;
  __syncthreads();

  // phase 1: the two hit planes
  const float invG = 1.0f / (float)G;
  const float lo_f = (float)(-hg), hi_f = (float)(hg - 1);
  const uint8_t* cur = a.cur + e * a.frame_stride;
  const uint8_t* prev = a.prev + e * a.frame_stride;
  for (int q = 4 * tid; q < G2; q += 4 * kFlowThreads) {
    const int i = flow_div(q, G, invG), j = q - i * G;  // G % 4 == 0: the 4 cells share row i and an LDS word
    const uint32_t cw = *reinterpret_cast<const uint32_t*>(cur + q);
    const float fa = (float)(i - hg);
    uint32_t bc = 0, bp = 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      bc |= (((cw >> (8 * u)) & 255u) == 255u ? 1u : 0u) << u;
      const float fb = (float)(j + u - hg);
      const float wu = (cr * fa - sr * fb) + tx;
      const float wv = (sr * fa + cr * fb) + ty;
      const float ru = rintf(wu), rv = rintf(wv);
      const bool inside = (ru >= lo_f) && (ru <= hi_f) && (rv >= lo_f) && (rv <= hi_f);
      const int gi = inside ? (int)ru + hg : 0, gj = inside ? (int)rv + hg : 0;  // in 0..G-1 either way
      const uint32_t b = prev[gi * G + gj];
      bp |= ((inside && b == 255u) ? 1u : 0u) << u;
    }
    const int word = (i + kFlowGuard) * RS + 1 + (j >> 5), sh = j & 31;
    if (bc) atomicOr(&Hc[word], bc << sh);
    if (bp) atomicOr(&Hp[word], bp << sh);
  }
  __syncthreads();

  // S = (Hc & !D(Hp)) | (Hp & !D(Hc)): one word per thread, D from three rows (the guard row and words are 0)
  for (int t = tid; t < G * wpr; t += kFlowThreads) {
    const int i = flow_div(t, wpr, 1.0f / (float)wpr), w = t - i * wpr;
    const int at = (i + kFlowGuard) * RS + 1 + w;
    uint32_t dc = 0, dp = 0;
#pragma unroll
    for (int k = -1; k <= 1; ++k) {
      const uint32_t* rc = Hc + at + k * RS;
      const uint32_t* rp = Hp + at + k * RS;
      dc |= rc[0] | (rc[0] << 1) | (rc[0] >> 1) | (rc[-1] >> 31) | (rc[1] << 31);
      dp |= rp[0] | (rp[0] << 1) | (rp[0] >> 1) | (rp[-1] >> 31) | (rp[1] << 31);
    }
    S[at] = (Hc[at] & ~dp) | (Hp[at] & ~dc);
  }
  __syncthreads();

  // phase 2: wave tasks of 256 cells
  for (int q0 = wave * kFlowTask; q0 < G2; q0 += kFlowWaves * kFlowTask) {  // wave-uniform
    const int q = q0 + 4 * lane;
    const bool valid = q < G2;  // G2 % 16 == 0: a lane's 4 cells are all in the plane or all outside it
    int i = 0, j = 0;
    uint32_t h4 = 0;
    if (valid) {
      i = flow_div(q, G, invG);
      j = q - i * G;
      h4 = (Hc[(i + kFlowGuard) * RS + 1 + (j >> 5)] >> (j & 31)) & 15u;
    }
    if (__ballot(h4 != 0u) == 0ull) {  // wave-uniform: nothing to look at
      if (valid) flow_store<FMT>(a, e, G2, q, zero);
      continue;
    }
    // the hit cells of the task, compacted: an inclusive prefix of the lanes' counts
    const int cnt = __popc(h4);
    int incl = cnt;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int v = __shfl_up(incl, o, 64);
      if (lane >= o) incl += v;
    }
    const int total = __shfl(incl, 63, 64);
    *reinterpret_cast<uint2*>(codes + 4 * lane) = make_uint2(0u, 0u);
    int pos = incl - cnt;
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (h4 & (1u << u)) list[pos++] = (uint8_t)(4 * lane + u);
    flow_wave_sync();
    for (int k = lane; k < total; k += 64) {
      const int c = list[k], qc = q0 + c;
      const int ci = flow_div(qc, G, invG), cj = qc - ci * G;
      codes[c] = (uint16_t)flow_cell(Hc, Hp, S, RS, ci, cj, a.R, a.B, a.gate, a.min_hits);
    }
    flow_wave_sync();
    if (valid) {
      const uint2 cc = *reinterpret_cast<const uint2*>(codes + 4 * lane);
      const uint32_t code[4] = {cc.x & 0xFFFFu, cc.x >> 16, cc.y & 0xFFFFu, cc.y >> 16};
      flow_store<FMT>(a, e, G2, q, code);
    }
    flow_wave_sync();  // the next task's list and codes overwrite these
  }
}

int flow_check(const char* who, const ffmp_cfg_t* cfg, int32_t format, float scale, int32_t radius, int32_t block, int32_t gate,
               int32_t min_hits) {
  if (!cfg) return fail(FFMP_E_ARG, "%s: cfg is NULL", who);
  if (cfg->grid < 8 || cfg->grid > 512 || (cfg->grid % 4) != 0)
    return fail(FFMP_E_ARG, "%s: grid must be a multiple of 4 in [8,512], got %d", who, cfg->grid);
  if (format != FFMP_OBS_F32 && format != FFMP_OBS_U8F16) return fail(FFMP_E_ARG, "%s: unknown format %d", who, format);
  if (!(scale - scale == 0.0f)) return fail(FFMP_E_ARG, "%s: scale must be finite", who);
  if (radius < 1 || radius > kFlowMaxR) return fail(FFMP_E_ARG, "%s: radius must be in [1,%d], got %d", who, kFlowMaxR, radius);
  if (block < 1 || block > kFlowMaxB) return fail(FFMP_E_ARG, "%s: block must be in [1,%d], got %d", who, kFlowMaxB, block);
  if (gate < 0 || gate > 98) return fail(FFMP_E_ARG, "%s: gate must be in [0,98], got %d", who, gate);
  if (min_hits < 1 || min_hits > 49) return fail(FFMP_E_ARG, "%s: min_hits must be in [1,49], got %d", who, min_hits);
  return FFMP_OK;
}

// do the byte ranges [a, a + na) and [b, b + nb) meet
bool flow_ranges_meet(const void* a, uint64_t na, const void* b, uint64_t nb) {
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return pa < pb ? pb - pa < na : pa - pb < nb;
}

}  // namespace

extern "C" {

int ffmp_scan_flow_check(const ffmp_cfg_t* cfg, int32_t format, float scale, int32_t radius, int32_t block, int32_t gate,
                         int32_t min_hits) {
  return flow_check("ffmp_scan_flow", cfg, format, scale, radius, block, gate, min_hits);
}

int ffmp_scan_flow(const ffmp_cfg_t* cfg, int64_t n, const uint8_t* cur, const uint8_t* prev, int64_t frame_env_stride,
                   const float* pose_now, int64_t pose_now_stride, const float* pose_prev, int64_t pose_prev_stride,
                   const uint8_t* mask, const uint8_t* first, void* flow_out, int64_t flow_env_stride, uint8_t* kind_out,
                   int64_t kind_env_stride, int32_t format, float scale, int32_t radius, int32_t block, int32_t gate,
                   int32_t min_hits, void* stream) {
  const char* who = "ffmp_scan_flow";
  if (int rc = flow_check(who, cfg, format, scale, radius, block, gate, min_hits)) return rc;
  if (n < 0) return fail(FFMP_E_ARG, "%s: negative n", who);
  if (n > 0x7fffffffLL) return fail(FFMP_E_ARG, "%s: n too large for one launch: %lld", who, (long long)n);
  if (!cur) return fail(FFMP_E_ARG, "%s: cur is NULL", who);
  if (!prev) return fail(FFMP_E_ARG, "%s: prev is NULL", who);
  if (!pose_now) return fail(FFMP_E_ARG, "%s: pose_now is NULL", who);
  if (!pose_prev) return fail(FFMP_E_ARG, "%s: pose_prev is NULL", who);
  if (!flow_out) return fail(FFMP_E_ARG, "%s: flow_out is NULL", who);
  if (pose_now_stride < 4) return fail(FFMP_E_ARG, "%s: pose_now_stride %lld < 4", who, (long long)pose_now_stride);
  if (pose_prev_stride < 4) return fail(FFMP_E_ARG, "%s: pose_prev_stride %lld < 4", who, (long long)pose_prev_stride);
  const int64_t G2 = (int64_t)cfg->grid * cfg->grid;
  if (frame_env_stride < G2)
    return fail(FFMP_E_ARG, "%s: frame_env_stride %lld < G*G = %lld", who, (long long)frame_env_stride, (long long)G2);
  if (flow_env_stride < 2 * G2)
    return fail(FFMP_E_ARG, "%s: flow_env_stride %lld < 2*G*G = %lld", who, (long long)flow_env_stride, (long long)(2 * G2));
  if (kind_out && kind_env_stride < G2)
    return fail(FFMP_E_ARG, "%s: kind_env_stride %lld < G*G = %lld", who, (long long)kind_env_stride, (long long)G2);
  if ((((uintptr_t)cur | (uintptr_t)prev) & 3u) != 0 || (frame_env_stride % 4) != 0)
    return fail(FFMP_E_ARG, "%s: cur and prev must be 4-byte aligned with frame_env_stride a multiple of 4 (frame alignment)", who);
  const uintptr_t am = format == FFMP_OBS_F32 ? 15u : 7u;
  if (((uintptr_t)flow_out & am) != 0 || (flow_env_stride % 4) != 0)
    return fail(FFMP_E_ARG, "%s: flow_out must be %d-byte aligned with flow_env_stride a multiple of 4 elements (flow alignment)", who,
                (int)am + 1);
  if (kind_out && ((((uintptr_t)kind_out) & 3u) != 0 || (kind_env_stride % 4) != 0))
    return fail(FFMP_E_ARG, "%s: kind_out must be 4-byte aligned with kind_env_stride a multiple of 4 (kind alignment)", who);
  if (n > 0) {
    const uint64_t es = format == FFMP_OBS_F32 ? 4u : 2u, last = (uint64_t)(n - 1);
    const uint64_t fbytes = (last * (uint64_t)flow_env_stride + 2u * (uint64_t)G2) * es;
    const uint64_t kbytes = last * (uint64_t)kind_env_stride + (uint64_t)G2;
    const uint64_t ibytes = last * (uint64_t)frame_env_stride + (uint64_t)G2;
    if (kind_out && flow_ranges_meet(flow_out, fbytes, kind_out, kbytes))
      return fail(FFMP_E_ARG, "%s: the flow_out and kind_out planes overlap", who);
    if (flow_ranges_meet(flow_out, fbytes, cur, ibytes) || flow_ranges_meet(flow_out, fbytes, prev, ibytes) ||
        (kind_out && (flow_ranges_meet(kind_out, kbytes, cur, ibytes) || flow_ranges_meet(kind_out, kbytes, prev, ibytes))))
      return fail(FFMP_E_ARG, "%s: an output overlaps the frames it is computed from", who);
  }
  if (n == 0) return FFMP_OK;

  FlowArgs a;
  a.cur = cur;
  a.prev = prev;
  a.frame_stride = frame_env_stride;
  a.pose_now = pose_now;
  a.pose_now_stride = pose_now_stride;
  a.pose_prev = pose_prev;
  a.pose_prev_stride = pose_prev_stride;
  a.mask = mask;
  a.first = first;
  a.flow = flow_out;
  a.flow_stride = flow_env_stride;
  a.kind = kind_out;
  a.kind_stride = kind_env_stride;
  a.scale = scale;
  a.R = radius;
  a.B = block;
  a.gate = gate;
  a.min_hits = min_hits;
  const bool f32 = format == FFMP_OBS_F32;
  void (*k)(ffmp_cfg_t, FlowArgs) = f32 ? scan_flow_kernel<FFMP_OBS_F32> : scan_flow_kernel<FFMP_OBS_U8F16>;
  const size_t lds = flow_lds_bytes(cfg->grid);
  if (lds > kFlowLdsDefault) {
    // more than the default cap of dynamic LDS: ask for it, once per device and kernel (an attribute of the
    // function, no stream work)
    static std::atomic<uint64_t> asked[2];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return fail(FFMP_E_HIP, "%s: hipGetDevice failed", who);
    const uint64_t bit = 1ull << (dev & 63);
    if (!(asked[f32].load() & bit)) {
      hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)flow_lds_bytes(512));
      if (err != hipSuccess)
        return fail(FFMP_E_HIP, "%s: hipFuncSetAttribute(%zu bytes of LDS): %s", who, flow_lds_bytes(512), hipGetErrorString(err));
      asked[f32].fetch_or(bit);
    }
  }
  hipLaunchKernelGGL(k, dim3((unsigned)n), dim3(kFlowThreads), lds, (hipStream_t)stream, *cfg, a);
  return launch_ok(who);
}

}  // extern "C"
