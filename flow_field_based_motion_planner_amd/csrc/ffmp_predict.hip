// ffmp_predict.hip — predicted-occupancy frames from a frame and its flow (include/ffmp.h ffmp_flow_predict
// carries the SPEC).  A source of its own: the code objects of the step, the scan and
// the navigation kernels stay what they are.
//
// One workgroup of 256 threads per env.  A lane's unit of work is a group of 16 consecutive cells of the flat
// plane (G % 4 == 0, so G*G % 16 == 0): one 16-byte store of `out`.  LDS, per env:
//   bits  ceil(G*G/32) words: the predicted plane, bit q of the flat cell number q — set with atomicOr, many
//         sources of one disc land on the same word at once;
//   cls   G*G/16 words: occ (low half) and src (high half) of a group, written and read back by the lane
//         that owns the group, so the frame is read from memory once and phase 3 needs no load.
//   list  1,024 words: the flat cell numbers of the env's sources (FFMP_PRED_LIST).
// 3 G*G/8 bytes + 4 KiB: 5.5 KiB at G = 64, 28 KiB at 256, 100 KiB at 512 (above the default cap of dynamic
// LDS: asked for once per device).
//
// Phase 1: zero the bits.
// Phase 2a: a lane loads the 16 frame values of its group — 16-byte loads where the base and the env stride
// allow, 4-byte loads otherwise — and keeps occ / src.  The flow is loaded only for the cells with src set:
// almost every group has none, and the two flow planes are 8 of the 13 bytes per cell in float32.  A cell
// whose flow makes it a source goes onto the list (an LDS atomic add takes the slot; the order cannot matter).
// Phase 2b, after a barrier: the listed sources are dealt out one per thread; a source walks its k = 1..H
// targets and ORs the gated ones into the bits.  The sources of a disc sit in a few groups — up to 16 in
// one lane's — so walked where they are found they leave a wave waiting for one lane through 16 H steps; from
// the list the block's 256 threads share them.  A source that finds the list full is walked by the lane that
// found it (a plane of nothing but sources still gives the same bits).
// Phase 3, after a barrier: out from cls and the bits, one 16-byte store per group (4-byte stores where out's
// base or stride do not allow), and the block's sum of popcount(bit & !occ) into n_swept.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <atomic>
#include <type_traits>

#include "ffmp_device.h"
#include "ffmp_host.h"

#pragma clang fp contract(off)

namespace {

constexpr int kPredThreads = 256;
constexpr int kPredWaves = kPredThreads / 64;
constexpr int kPredMaxSteps = 64, kPredMaxPace = 1024, kPredMaxSlack = 255;
constexpr size_t kPredLdsDefault = 64 * 1024;
#ifndef FFMP_PRED_LIST
#define FFMP_PRED_LIST 1024
#endif
constexpr int kPredList = FFMP_PRED_LIST;  // sources of an env walked by the whole block; 0: every source by its own lane

struct PredArgs {
  const void* frame;
  int64_t frame_stride;  // elements
  const void* flow;
  int64_t flow_stride;   // elements
  const uint8_t* mask;
  uint8_t* out;
  int64_t out_stride;    // bytes
  int32_t* n_swept;      // or NULL
  float cps;
  int32_t G, steps, pace, slack, swept, other;
  int32_t frame_vec, out_vec;  // 16-byte accesses allowed
};

// G*G is a multiple of 16, not always of 32 (G = 100): the last word of the bits may be half used
__host__ __device__ constexpr int pred_bit_words(int G2) { return (G2 + 31) >> 5; }
size_t pred_lds_bytes(int G) { return ((size_t)pred_bit_words(G * G) + (size_t)(G * G >> 4) + (size_t)kPredList) * 4; }

// occ | src << 16 of 4 cells at bit u0
FFMP_DEV uint32_t pred_class4(float4 v, int u0) {
  const uint32_t occ = (v.x > 0.0f ? 1u : 0u) | (v.y > 0.0f ? 2u : 0u) | (v.z > 0.0f ? 4u : 0u) | (v.w > 0.0f ? 8u : 0u);
  const uint32_t src = (v.x == 255.0f ? 1u : 0u) | (v.y == 255.0f ? 2u : 0u) | (v.z == 255.0f ? 4u : 0u) | (v.w == 255.0f ? 8u : 0u);
  return (occ | (src << 16)) << u0;
}
FFMP_DEV uint32_t pred_class4(uint32_t w, int u0) {
  uint32_t occ = 0, src = 0;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const uint32_t b = (w >> (8 * u)) & 255u;
    occ |= (b != 0u ? 1u : 0u) << u;
    src |= (b == 255u ? 1u : 0u) << u;
  }
  return (occ | (src << 16)) << u0;
}

template <typename FT>
FFMP_DEV uint32_t pred_load_group(const FT* f, bool vec) {
  uint32_t c = 0;
  if constexpr (std::is_same<FT, float>::value) {
    if (vec) {
      const float4* p = reinterpret_cast<const float4*>(f);
#pragma unroll
      for (int r = 0; r < 4; ++r) c |= pred_class4(p[r], 4 * r);
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) c |= pred_class4(make_float4(f[4 * r], f[4 * r + 1], f[4 * r + 2], f[4 * r + 3]), 4 * r);
    }
  } else {
    if (vec) {
      const uint4 v = *reinterpret_cast<const uint4*>(f);
      c = pred_class4(v.x, 0) | pred_class4(v.y, 4) | pred_class4(v.z, 8) | pred_class4(v.w, 12);
    } else {
      const uint32_t* p = reinterpret_cast<const uint32_t*>(f);
#pragma unroll
      for (int r = 0; r < 4; ++r) c |= pred_class4(p[r], 4 * r);
    }
  }
  return c;
}

// the 4 bytes of `out` for cells with (occ, src, bit) nibbles
FFMP_DEV uint32_t pred_bytes4(uint32_t occ, uint32_t src, uint32_t bit, uint32_t swept, uint32_t other) {
  uint32_t w = 0;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const uint32_t m = 1u << u;
    const uint32_t b = (src & m) ? 255u : (occ & m) ? other : (bit & m) ? swept : 0u;
    w |= b << (8 * u);
  }
  return w;
}

// the k = 1..H targets of the source at flat cell q, the gated ones ORed into the bits
FFMP_DEV void pred_walk(const PredArgs& a, uint32_t* bits, int q, float su, float sv, float invG) {
  const int G = a.G, c = G >> 1;
  const float Gf = (float)G;
  int i = (int)((float)q * invG);  // q / G for q < 2^24: the float quotient is within one of it
  if (i * G > q) --i;
  if ((i + 1) * G <= q) ++i;
  const int j = q - i * G;
  for (int k = 1; k <= a.steps; ++k) {
    const float ru = rintf((float)k * su), rv = rintf((float)k * sv);
    // |r| >= G leaves the grid from any cell (an overflow to inf included): no integer is formed for it
    if (!(fabsf(ru) < Gf) || !(fabsf(rv) < Gf)) continue;
    const int ti = i + (int)ru, tj = j + (int)rv;
    if ((unsigned)ti >= (unsigned)G || (unsigned)tj >= (unsigned)G) continue;
    const int di = abs(ti - c), dj = abs(tj - c);
    const int ka = (5 * max(di, dj) + 2 * min(di, dj)) / a.pace;
    if (a.slack < 0 || abs(k - ka) <= a.slack) {
      const int t = ti * G + tj;
      atomicOr(&bits[t >> 5], 1u << (t & 31));
    }
  }
}

// is (su, sv) a source's displacement: both finite, not both 0
FFMP_DEV bool pred_moves(float su, float sv) { return (su - su == 0.0f) && (sv - sv == 0.0f) && !(su == 0.0f && sv == 0.0f); }

template <typename FT, typename VT>
__global__ __launch_bounds__(kPredThreads) void flow_predict_kernel(PredArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t pred_lds[];
  __shared__ int wave_sum[kPredWaves];
  __shared__ int n_list;
  const int G = a.G, G2 = G * G;
  const int n_bits = pred_bit_words(G2), n_groups = G2 >> 4;
  const int tid = threadIdx.x;
  const int64_t e = blockIdx.x;
  if (a.mask && a.mask[e] == 0) return;  // block-uniform

  uint32_t* bits = pred_lds;
  uint32_t* cls = pred_lds + n_bits;
  uint32_t* list = cls + n_groups;

  // phase 1
  for (int w = tid; w < n_bits; w += kPredThreads) bits[w] = 0u;
  if (tid == 0) n_list = 0;
  __syncthreads();

  // phase 2a: the frame, once; the sources into the list
  const FT* frame = reinterpret_cast<const FT*>(a.frame) + e * a.frame_stride;
  const VT* vxp = reinterpret_cast<const VT*>(a.flow) + e * a.flow_stride;
  const VT* vyp = vxp + G2;
  const float invG = 1.0f / (float)G;
  const bool fvec = a.frame_vec != 0;
  for (int g = tid; g < n_groups; g += kPredThreads) {
    const int q0 = g << 4;
    const uint32_t cw = pred_load_group<FT>(frame + q0, fvec);
    cls[g] = cw;
    for (uint32_t s = cw >> 16; s; s &= s - 1u) {  // the source candidates of the group: rare
      const int q = q0 + __builtin_ctz(s);
      const float su = (float)vxp[q] * a.cps;
      const float sv = (float)vyp[q] * a.cps;
      if (!pred_moves(su, sv)) continue;
      const int pos = kPredList > 0 ? atomicAdd(&n_list, 1) : kPredList;
      if (pos < kPredList) list[pos] = (uint32_t)q;
      else pred_walk(a, bits, q, su, sv, invG);  // the list is full: walked by the lane that found it
    }
  }
  __syncthreads();

  // phase 2b: the listed sources, one per thread at a time
  const int listed = min(n_list, kPredList);
  for (int s = tid; s < listed; s += kPredThreads) {
    const int q = (int)list[s];
    pred_walk(a, bits, q, (float)vxp[q] * a.cps, (float)vyp[q] * a.cps, invG);
  }
  __syncthreads();

  // phase 3
  uint8_t* out = a.out + e * a.out_stride;
  const uint32_t swept = (uint32_t)a.swept, other = (uint32_t)a.other;
  const bool ovec = a.out_vec != 0;
  int count = 0;
  for (int g = tid; g < n_groups; g += kPredThreads) {
    const uint32_t cw = cls[g];
    const uint32_t occ = cw & 0xFFFFu, src = cw >> 16;
    const uint32_t bit = (bits[g >> 1] >> ((g & 1) << 4)) & 0xFFFFu;
    count += __popc(bit & ~occ);
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if ((cw | bit) != 0u) {
      v.x = pred_bytes4(occ, src, bit, swept, other);
      v.y = pred_bytes4(occ >> 4, src >> 4, bit >> 4, swept, other);
      v.z = pred_bytes4(occ >> 8, src >> 8, bit >> 8, swept, other);
      v.w = pred_bytes4(occ >> 12, src >> 12, bit >> 12, swept, other);
    }
    uint8_t* o = out + (g << 4);
    if (ovec) {
      *reinterpret_cast<uint4*>(o) = v;
    } else {
      uint32_t* o4 = reinterpret_cast<uint32_t*>(o);
      o4[0] = v.x; o4[1] = v.y; o4[2] = v.z; o4[3] = v.w;
    }
  }
  if (a.n_swept) {  // block-uniform
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) count += __shfl_down(count, o, 64);
    if ((tid & 63) == 0) wave_sum[tid >> 6] = count;
    __syncthreads();
    if (tid == 0) {
      int total = 0;
#pragma unroll
      for (int w = 0; w < kPredWaves; ++w) total += wave_sum[w];
      a.n_swept[e] = total;
    }
  }
}

int pred_check(const char* who, const ffmp_cfg_t* cfg, int32_t frame_format, int32_t flow_format, int32_t steps, float cps,
               int32_t pace, int32_t slack, int32_t swept, int32_t other) {
  if (!cfg) return fail(FFMP_E_ARG, "%s: cfg is NULL", who);
  if (cfg->grid < 8 || cfg->grid > 512 || (cfg->grid % 4) != 0)
    return fail(FFMP_E_ARG, "%s: grid must be a multiple of 4 in [8,512], got %d", who, cfg->grid);
  if (frame_format != FFMP_OBS_F32 && frame_format != FFMP_OBS_U8F16)
    return fail(FFMP_E_ARG, "%s: unknown frame_format %d", who, frame_format);
  if (flow_format != FFMP_OBS_F32 && flow_format != FFMP_OBS_U8F16)
    return fail(FFMP_E_ARG, "%s: unknown flow_format %d", who, flow_format);
  if (steps < 1 || steps > kPredMaxSteps) return fail(FFMP_E_ARG, "%s: steps must be in [1,%d], got %d", who, kPredMaxSteps, steps);
  if (!(cps - cps == 0.0f) || cps < 0.0f) return fail(FFMP_E_ARG, "%s: cps must be finite and >= 0", who);
  if (pace < 1 || pace > kPredMaxPace) return fail(FFMP_E_ARG, "%s: pace must be in [1,%d], got %d", who, kPredMaxPace, pace);
  if (slack < -1 || slack > kPredMaxSlack) return fail(FFMP_E_ARG, "%s: slack must be in [-1,%d], got %d", who, kPredMaxSlack, slack);
  if (swept < 0 || swept > 255) return fail(FFMP_E_ARG, "%s: swept must be in [0,255], got %d", who, swept);
  if (other < 0 || other > 255) return fail(FFMP_E_ARG, "%s: other must be in [0,255], got %d", who, other);
  return FFMP_OK;
}

// do the byte ranges [a, a + na) and [b, b + nb) meet
bool pred_ranges_meet(const void* a, uint64_t na, const void* b, uint64_t nb) {
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return pa < pb ? pb - pa < na : pa - pb < nb;
}

}  // namespace

extern "C" {

int ffmp_flow_predict_check(const ffmp_cfg_t* cfg, int32_t frame_format, int32_t flow_format, int32_t steps, float cps,
                            int32_t pace, int32_t slack, int32_t swept, int32_t other) {
  return pred_check("ffmp_flow_predict", cfg, frame_format, flow_format, steps, cps, pace, slack, swept, other);
}

int ffmp_flow_predict(const ffmp_cfg_t* cfg, int64_t n, const void* frame, int64_t frame_env_stride, int32_t frame_format,
                      const void* flow, int64_t flow_env_stride, int32_t flow_format, const uint8_t* mask, uint8_t* out,
                      int64_t out_env_stride, int32_t* n_swept, int32_t steps, float cps, int32_t pace, int32_t slack,
                      int32_t swept, int32_t other, void* stream) {
  const char* who = "ffmp_flow_predict";
  if (int rc = pred_check(who, cfg, frame_format, flow_format, steps, cps, pace, slack, swept, other)) return rc;
  if (n < 0) return fail(FFMP_E_ARG, "%s: negative n", who);
  if (n > 0x7fffffffLL) return fail(FFMP_E_ARG, "%s: n too large for one launch: %lld", who, (long long)n);
  if (!frame) return fail(FFMP_E_ARG, "%s: frame is NULL", who);
  if (!flow) return fail(FFMP_E_ARG, "%s: flow is NULL", who);
  if (!out) return fail(FFMP_E_ARG, "%s: out is NULL", who);
  const int64_t G2 = (int64_t)cfg->grid * cfg->grid;
  if (frame_env_stride < G2)
    return fail(FFMP_E_ARG, "%s: frame_env_stride %lld < G*G = %lld", who, (long long)frame_env_stride, (long long)G2);
  if (flow_env_stride < 2 * G2)
    return fail(FFMP_E_ARG, "%s: flow_env_stride %lld < 2*G*G = %lld", who, (long long)flow_env_stride, (long long)(2 * G2));
  if (out_env_stride < G2)
    return fail(FFMP_E_ARG, "%s: out_env_stride %lld < G*G = %lld", who, (long long)out_env_stride, (long long)G2);
  if (((uintptr_t)frame & 3u) != 0 || (frame_env_stride % 4) != 0)
    return fail(FFMP_E_ARG, "%s: frame must be 4-byte aligned with frame_env_stride a multiple of 4 elements (frame alignment)", who);
  if (((uintptr_t)flow & 3u) != 0 || (flow_env_stride % 4) != 0)
    return fail(FFMP_E_ARG, "%s: flow must be 4-byte aligned with flow_env_stride a multiple of 4 elements (flow alignment)", who);
  if (((uintptr_t)out & 3u) != 0 || (out_env_stride % 4) != 0)
    return fail(FFMP_E_ARG, "%s: out must be 4-byte aligned with out_env_stride a multiple of 4 (out alignment)", who);
  if (n_swept && ((uintptr_t)n_swept & 3u) != 0) return fail(FFMP_E_ARG, "%s: n_swept must be 4-byte aligned", who);
  const uint64_t fes = frame_format == FFMP_OBS_F32 ? 4u : 1u, ves = flow_format == FFMP_OBS_F32 ? 4u : 2u;
  if (n > 0) {
    const uint64_t last = (uint64_t)(n - 1);
    const uint64_t ibytes = (last * (uint64_t)frame_env_stride + (uint64_t)G2) * fes;
    const uint64_t vbytes = (last * (uint64_t)flow_env_stride + 2u * (uint64_t)G2) * ves;
    const uint64_t obytes = last * (uint64_t)out_env_stride + (uint64_t)G2;
    if (pred_ranges_meet(out, obytes, frame, ibytes) || pred_ranges_meet(out, obytes, flow, vbytes))
      return fail(FFMP_E_ARG, "%s: out overlaps the planes it is computed from", who);
    if (n_swept && (pred_ranges_meet(n_swept, 4u * (uint64_t)n, out, obytes) || pred_ranges_meet(n_swept, 4u * (uint64_t)n, frame, ibytes) ||
                    pred_ranges_meet(n_swept, 4u * (uint64_t)n, flow, vbytes)))
      return fail(FFMP_E_ARG, "%s: n_swept overlaps a plane", who);
  }
  if (n == 0) return FFMP_OK;

  PredArgs a;
  a.frame = frame;
  a.frame_stride = frame_env_stride;
  a.flow = flow;
  a.flow_stride = flow_env_stride;
  a.mask = mask;
  a.out = out;
  a.out_stride = out_env_stride;
  a.n_swept = n_swept;
  a.cps = cps;
  a.G = cfg->grid;
  a.steps = steps;
  a.pace = pace;
  a.slack = slack;
  a.swept = swept;
  a.other = other;
  a.frame_vec = ((uintptr_t)frame & 15u) == 0 && (((uint64_t)frame_env_stride * fes) & 15u) == 0;
  a.out_vec = ((uintptr_t)out & 15u) == 0 && (out_env_stride & 15) == 0;
  const bool f32 = frame_format == FFMP_OBS_F32, v32 = flow_format == FFMP_OBS_F32;
  void (*k)(PredArgs) = f32 ? (v32 ? flow_predict_kernel<float, float> : flow_predict_kernel<float, _Float16>)
                            : (v32 ? flow_predict_kernel<uint8_t, float> : flow_predict_kernel<uint8_t, _Float16>);
  const size_t lds = pred_lds_bytes(cfg->grid);
  if (lds > kPredLdsDefault) {
    // more than the default cap of dynamic LDS: ask for it, once per device and kernel (an attribute of the
    // function, no stream work)
    static std::atomic<uint64_t> asked[4];
    const int which = (f32 ? 2 : 0) + (v32 ? 1 : 0);
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return fail(FFMP_E_HIP, "%s: hipGetDevice failed", who);
    const uint64_t bit = 1ull << (dev & 63);
    if (!(asked[which].load() & bit)) {
      hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)pred_lds_bytes(512));
      if (err != hipSuccess)
        return fail(FFMP_E_HIP, "%s: hipFuncSetAttribute(%zu bytes of LDS): %s", who, pred_lds_bytes(512), hipGetErrorString(err));
      asked[which].fetch_or(bit);
    }
  }
  hipLaunchKernelGGL(k, dim3((unsigned)n), dim3(kPredThreads), lds, (hipStream_t)stream, a);
  return launch_ok(who);
}

}  // extern "C"
