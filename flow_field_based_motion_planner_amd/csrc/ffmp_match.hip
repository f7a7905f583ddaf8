// ffmp_match.hip — scan-to-map matching: the scan's endpoints scored against the world-fixed map over every
// whole-cell shift and every rotation step of a small window round the prior pose, and the best candidate's
// pose (include/ffmp.h ffmp_scan_match carries the SPEC).
//
// scan_match_kernel: one workgroup of 256 threads per env.
//   1. The valid beams' (bx, by) = r * beam are staged once, compacted (an LDS counter hands out the slots: the
//      scores are integer sums, so the order of the beams does not show).
//   2. The rotations go in chunks of as many as fit kMtChunk cell pairs.  Per chunk every (rotation, valid beam)
//      is turned into its cell pair (fp, fq) once and, if it is on the padded plane, appended to its rotation's
//      list in LDS as (fp + R) << 16 | (fq + R).
//   3. A lane owns whole candidates (rotation, a, b), b fastest: it walks its rotation's list — the pair is a
//      broadcast read, lanes with consecutive b read consecutive bytes of the plane — sums the bytes, stores the
//      sum to the volume and keeps the best packed key.  One tree reduction over the workgroup at the end; thread
//      0 gates and writes pose_out and info.
// The bytes come from global memory: an env's candidates read a few cells round at most L endpoints, which L2
// holds.  A copy of the box round the robot that holds every endpoint (about 75 KiB at 6.4 m and 5 cm) in LDS,
// gathered from there, was built and measured first and is not kept: the copy costs more than the gathers save
// (C3, 32,768 envs: 3.57 against 0.50 ms on the presets' own scans, 9.69 against 5.78 ms with a return on every
// beam — one workgroup per CU at that much LDS).  FFMP_MATCH_GLOBAL, which forced this path while
// there were two, is still accepted and changes nothing.
// LDS: 8 KiB beams + 16 KiB pairs + 2 KiB keys, static.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>

#include "ffmp_host.h"

#pragma clang fp contract(off)

namespace {

constexpr int kMtThreads = 256;
constexpr int kMtChunk = 4096;                  // cell pairs per chunk of rotations: >= 4 rotations at L = 1024
constexpr size_t kMtStaticLds = FFMP_MAX_BEAMS * 8 + kMtChunk * 4 + kMtThreads * 8 + 65 * 4 + 64;
constexpr size_t kMtLdsLimit = 64 * 1024;       // static LDS a kernel may declare
constexpr int kMtMaxRadius = 16, kMtMaxTurns = 32;
static_assert(kMtStaticLds <= kMtLdsLimit, "the match kernel's LDS");

struct MatchArgs {
  const float* ranges;
  int64_t ranges_stride;
  const float* beams;  // (L, 2)
  const float* pose;
  int64_t pose_stride;
  const uint8_t* mask;
  const int8_t* map;
  int64_t map_stride;  // bytes
  const float* turns;  // (2T + 1, 2)
  float* pose_out;
  int32_t* info;
  int32_t* volume;
  int32_t L, Wc, R, T, min_valid, min_gain;
  float rm, wh, res;
};

typedef int mt_i32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t mt_u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ bool mt_finite(float v) { return v - v == 0.0f; }

// q / d for 0 <= q < 2^24, 1 <= d: the float quotient is within one of it
__device__ __forceinline__ int mt_div(int q, int d, float invd) {
  int i = (int)((float)q * invd);
  if (i * d > q) --i;
  if ((i + 1) * d <= q) ++i;
  return i;
}

// The winner's order as one integer under max: S, then the smaller a^2 + b^2, |k|, k, a, b.
__device__ __forceinline__ uint64_t mt_key(int S, int k, int a, int b, int R, int T) {
  const uint32_t d2 = (uint32_t)(a * a + b * b), ak = (uint32_t)(k < 0 ? -k : k);
  const uint64_t low = ((uint64_t)(1023u - d2) << 25) | ((uint64_t)(63u - ak) << 19) | ((uint64_t)(127u - (uint32_t)(k + T)) << 12) |
                       ((uint64_t)(63u - (uint32_t)(a + R)) << 6) | (uint64_t)(63u - (uint32_t)(b + R));
  return ((uint64_t)(uint32_t)(S + (1 << 18)) << 35) | low;  // |S| <= 1024 * 128 = 2^17
}

__device__ __forceinline__ int mt_score(const uint32_t* cells, int cnt, int dp, int dq, int Wc, const int8_t* mp) {
  int S = 0;
#pragma unroll 4
  for (int j = 0; j < cnt; ++j) {
    const uint32_t v = cells[j];
    const int p = (int)(v >> 16) + dp, q = (int)(v & 0xffffu) + dq;
    if ((unsigned)p < (unsigned)Wc && (unsigned)q < (unsigned)Wc) S += (int)mp[p * Wc + q];
  }
  return S;
}

__global__ __launch_bounds__(kMtThreads) void scan_match_kernel(MatchArgs a) {
  __shared__ float2 s_b[FFMP_MAX_BEAMS];
  __shared__ uint32_t s_cell[kMtChunk];
  __shared__ uint64_t s_red[kMtThreads];
  __shared__ int s_cnt[2 * kMtMaxTurns + 1];
  __shared__ int s_nv, s_zero;

  const int tid = threadIdx.x;
  const int64_t e = blockIdx.x;
  if (a.mask && a.mask[e] == 0) return;  // block-uniform
  const int L = a.L, Wc = a.Wc, R = a.R, T = a.T;
  const float* ps = a.pose + e * a.pose_stride;
  const float px = ps[0], py = ps[1], c = ps[2], s = ps[3];
  const bool finite = mt_finite(px) && mt_finite(py) && mt_finite(c) && mt_finite(s);
  const int8_t* mp = a.map + e * a.map_stride;

  if (tid == 0) {
    s_nv = 0;
    s_zero = 0;
  }
  __syncthreads();
  const float* rg = a.ranges + e * a.ranges_stride;
  for (int l = tid; l < L; l += kMtThreads) {
    const float r = rg[l];
    if ((r > 0.0f) && (r <= a.rm) && (r <= FLT_MAX)) {
      const int slot = atomicAdd(&s_nv, 1);  // < L <= FFMP_MAX_BEAMS
      s_b[slot] = make_float2(r * a.beams[2 * l], r * a.beams[2 * l + 1]);
    }
  }

  __syncthreads();

  const int nv = s_nv;
  const int stride = nv > 0 ? nv : 1;
  const int K = 2 * T + 1, A = 2 * R + 1, A2 = A * A;
  const int KR = min(K, kMtChunk / stride);  // >= 4 or K
  const float lo_f = (float)(-R), hi_f = (float)(Wc - 1 + R);
  const float inv_stride = 1.0f / (float)stride, inv_A2 = 1.0f / (float)A2, inv_A = 1.0f / (float)A;
  uint64_t best = 0;

  for (int k0 = 0; k0 < K; k0 += KR) {
    const int kn = min(KR, K - k0);
    if (tid < kn) s_cnt[tid] = 0;
    __syncthreads();
    for (int i = tid; i < kn * nv; i += kMtThreads) {  // kn * nv <= kMtChunk
      const int kr = mt_div(i, stride, inv_stride);
      const float2 b = s_b[i - kr * stride];
      const float rc = a.turns[2 * (k0 + kr)], rs = a.turns[2 * (k0 + kr) + 1];
      const float ck = c * rc - s * rs, sk = s * rc + c * rs;
      const float wx = (ck * b.x - sk * b.y) + px;
      const float wy = (sk * b.x + ck * b.y) + py;
      const float fp = rintf((wx + a.wh) / a.res);
      const float fq = rintf((wy + a.wh) / a.res);
      const bool on = finite && (fp >= lo_f) && (fp <= hi_f) && (fq >= lo_f) && (fq <= hi_f);
      if (on) {
        const int gp = (int)fp, gq = (int)fq;
        const int slot = atomicAdd(&s_cnt[kr], 1);  // < nv
        s_cell[kr * stride + slot] = ((uint32_t)(gp + R) << 16) | (uint32_t)(gq + R);
      }
    }
    __syncthreads();
    for (int w = tid; w < kn * A2; w += kMtThreads) {
      const int kr = mt_div(w, A2, inv_A2);
      const int rem = w - kr * A2;
      const int ai = mt_div(rem, A, inv_A), bi = rem - ai * A;
      const uint32_t* cells = s_cell + kr * stride;
      const int cnt = s_cnt[kr];
      // the pair holds (fp + R, fq + R); the candidate's cell is (fp + ai - R, fq + bi - R)
      const int S = mt_score(cells, cnt, ai - 2 * R, bi - 2 * R, Wc, mp);
      const int k = k0 + kr - T;
      if (a.volume) a.volume[(e * K + (k0 + kr)) * A2 + rem] = S;
      if (k == 0 && ai == R && bi == R) s_zero = S;
      const uint64_t key = mt_key(S, k, ai - R, bi - R, R, T);
      best = key > best ? key : best;
    }
    __syncthreads();
  }

  s_red[tid] = best;
  __syncthreads();
  for (int h = kMtThreads / 2; h > 0; h >>= 1) {
    if (tid < h) {
      const uint64_t o = s_red[tid + h];
      if (o > s_red[tid]) s_red[tid] = o;
    }
    __syncthreads();
  }
  if (tid != 0) return;
  const uint64_t key = s_red[0];
  const int S_best = (int)(uint32_t)(key >> 35) - (1 << 18);
  const int b_w = (63 - (int)(key & 63u)) - R;
  const int a_w = (63 - (int)((key >> 6) & 63u)) - R;
  const int k_w = (127 - (int)((key >> 12) & 127u)) - T;
  const int S_zero = s_zero;
  const bool moved = k_w != 0 || a_w != 0 || b_w != 0;
  const bool ok = finite && nv >= a.min_valid && (S_best - S_zero >= a.min_gain) && moved;
  if (a.pose_out) {
    mt_u32x4 out;
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
    *reinterpret_cast<mt_u32x4*>(a.pose_out + 4 * e) = out;
  }
  if (a.info) {
    mt_i32x4 i0, i1;
    i0[0] = ok ? 1 : 0;
    i0[1] = ok ? k_w : 0;
    i0[2] = ok ? a_w : 0;
    i0[3] = ok ? b_w : 0;
    i1[0] = S_best;
    i1[1] = S_zero;
    i1[2] = nv;
    i1[3] = 0;
    mt_i32x4* dst = reinterpret_cast<mt_i32x4*>(a.info + 8 * e);
    dst[0] = i0;
    dst[1] = i1;
  }
}

int match_check(const char* who, const ffmp_cfg_t* cfg, int32_t n_beams, int32_t cells, int32_t radius, int32_t n_turns,
                float range_max, int32_t min_valid, int32_t min_gain, int32_t flags) {
  if (!cfg) return fail(FFMP_E_ARG, "%s: cfg is NULL", who);
  if (cells < 8 || cells > 2048 || (cells % 4) != 0)
    return fail(FFMP_E_ARG, "%s: cells must be a multiple of 4 in [8,2048], got %d", who, cells);
  if (!(cfg->res_f > 0.0f) || isinf(cfg->res_f)) return fail(FFMP_E_ARG, "%s: cfg.res_f must be > 0 and finite", who);
  if (n_beams < 1 || n_beams > FFMP_MAX_BEAMS)
    return fail(FFMP_E_ARG, "%s: n_beams must be in [1,%d], got %d", who, FFMP_MAX_BEAMS, n_beams);
  if (!(range_max > 0.0f)) return fail(FFMP_E_ARG, "%s: range_max must be > 0 (or +inf) and not NaN", who);
  if (radius < 0 || radius > kMtMaxRadius) return fail(FFMP_E_ARG, "%s: radius must be in [0,%d], got %d", who, kMtMaxRadius, radius);
  if (n_turns < 0 || n_turns > kMtMaxTurns) return fail(FFMP_E_ARG, "%s: n_turns must be in [0,%d], got %d", who, kMtMaxTurns, n_turns);
  if (min_valid < 0) return fail(FFMP_E_ARG, "%s: min_valid must be >= 0, got %d", who, min_valid);
  if (min_gain < 0) return fail(FFMP_E_ARG, "%s: min_gain must be >= 0, got %d", who, min_gain);
  if (flags & ~FFMP_MATCH_GLOBAL) return fail(FFMP_E_ARG, "%s: unknown flags 0x%x", who, flags);
  return FFMP_OK;  // the LDS is static and the same for every shape: the budget is the static_assert above
}

// [p, p + bytes) against the map's bytes
bool mt_overlaps(const void* p, uint64_t bytes, const int8_t* map, uint64_t map_bytes) {
  const uintptr_t a0 = (uintptr_t)p, a1 = a0 + bytes, m0 = (uintptr_t)map, m1 = m0 + map_bytes;
  return a0 < m1 && m0 < a1;
}

}  // namespace

extern "C" {

int ffmp_scan_match_check(const ffmp_cfg_t* cfg, int32_t n_beams, int32_t cells, int32_t radius, int32_t n_turns, float range_max,
                          int32_t min_valid, int32_t min_gain, int32_t flags) {
  return match_check("ffmp_scan_match", cfg, n_beams, cells, radius, n_turns, range_max, min_valid, min_gain, flags);
}

int ffmp_scan_match(const ffmp_cfg_t* cfg, int64_t n, const float* ranges, int64_t ranges_stride, int32_t n_beams,
                    const float* beams, const float* pose, int64_t pose_stride, const uint8_t* mask, const int8_t* map,
                    int64_t map_env_stride, int32_t cells, const float* turns, int32_t n_turns, int32_t radius, float range_max,
                    int32_t min_valid, int32_t min_gain, float* pose_out, int32_t* info, int32_t* volume, int32_t flags,
                    void* stream) {
  const char* who = "ffmp_scan_match";
  if (int rc = match_check(who, cfg, n_beams, cells, radius, n_turns, range_max, min_valid, min_gain, flags)) return rc;
  if (n < 0) return fail(FFMP_E_ARG, "%s: negative n", who);
  if (!ranges) return fail(FFMP_E_ARG, "%s: ranges is NULL", who);
  if (!beams) return fail(FFMP_E_ARG, "%s: beams is NULL", who);
  if (!pose) return fail(FFMP_E_ARG, "%s: pose is NULL", who);
  if (!map) return fail(FFMP_E_ARG, "%s: map is NULL", who);
  if (!turns) return fail(FFMP_E_ARG, "%s: turns is NULL", who);
  if (!pose_out && !info && !volume) return fail(FFMP_E_ARG, "%s: pose_out, info and volume are all NULL", who);
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
  if (((uintptr_t)volume & 3u) != 0) return fail(FFMP_E_ARG, "%s: volume must be 4-byte aligned (output alignment)", who);
  if (n > 0x7fffffffLL) return fail(FFMP_E_ARG, "%s: n too large for one launch: %lld", who, (long long)n);
  if (n == 0) return FFMP_OK;
  const uint64_t map_bytes = (uint64_t)(n - 1) * (uint64_t)map_env_stride + (uint64_t)W2;
  const uint64_t vol_env = (uint64_t)(2 * n_turns + 1) * (uint64_t)(2 * radius + 1) * (uint64_t)(2 * radius + 1);
  if (pose_out && mt_overlaps(pose_out, (uint64_t)n * 16u, map, map_bytes)) return fail(FFMP_E_ARG, "%s: pose_out overlaps the map", who);
  if (info && mt_overlaps(info, (uint64_t)n * 32u, map, map_bytes)) return fail(FFMP_E_ARG, "%s: info overlaps the map", who);
  if (volume && mt_overlaps(volume, (uint64_t)n * vol_env * 4u, map, map_bytes))
    return fail(FFMP_E_ARG, "%s: volume overlaps the map", who);

  MatchArgs a;
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
  a.volume = volume;
  a.L = n_beams;
  a.Wc = cells;
  a.R = radius;
  a.T = n_turns;
  a.min_valid = min_valid;
  a.min_gain = min_gain;
  a.rm = range_max;
  a.wh = (float)((double)cells * cfg->res / 2.0);  // wh_f of ffmp_world_map
  a.res = cfg->res_f;
  hipLaunchKernelGGL(scan_match_kernel, dim3((unsigned)n), dim3(kMtThreads), 0, (hipStream_t)stream, a);
  return launch_ok(who);
}

}  // extern "C"
