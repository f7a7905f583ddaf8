// ffmp_dwa.hip — the rollout (dynamic-window) planner over the navigation field (include/ffmp.h ffmp_dwa carries
// the SPEC).  A source of its own: the code objects of the step, the scan, the navigation
// and the prediction kernels stay what they are.
//
// One workgroup of 256 threads per env.  A rollout table holds cell offsets of at most 28 and a footprint offset
// is at most 3, so every cell a rollout can ask about lies within 31 cells of the robot cell: a 64 x 64 window,
// rows and columns c - 32 .. c + 31.  One window row is one 64-bit word (bit = column), one prediction step one
// window of 64 words, the H <= 32 steps a volume of 16 KiB of LDS — the cells the moving sources cover at step k,
// for every k at once, instead of one plane gated by a guess of the robot's arrival time.  LDS, per env:
//   vol   32 x 64 words of 64 bits: bit (k - 1, row, column) set where a source lands at step k (atomicOr on the
//         32-bit halves: the sources of one disc land on the same words at once);
//   list  1,024 x (cell, su, sv): the moving sources of the env (FFMP_DWA_LIST), 12 KiB;
//   kb    64 ints: the first blocked step per candidate (atomicMin).
// Phase 1: zero the H windows in use, kb = H + 1.
// Phase 2a: the (2R + 1)^2 region of the frame round the robot cell (clipped to the grid), 4 cells per lane and
// trip — 16 lanes along a row, 16 rows per block trip; one 16-byte load for a float32 frame where its base and
// env stride allow, 4-byte loads otherwise.  The flow is loaded only where the frame holds 255, as
// flow_predict_kernel does; a cell whose flow makes it a source goes onto the list with its displacement.
// Phase 2b, after a barrier: the (source, k) pairs are dealt out one per thread; a pair is two multiplies, two
// rintf and one LDS atomic.  A source that finds the list full is walked through its H steps by the lane that
// found it (a region of nothing but sources still gives the same bits).
// Phase 3, after a barrier: the (candidate, k) pairs are dealt out one per thread: the table entry, one uint16
// gather from the cost plane, and — the footprint test — 7 window rows, each shifted to the candidate's column
// and ANDed with the footprint's columns of that row (no dilated copy of the volume is made: A H 7 LDS reads are
// fewer than the H 64 (5 + 1) a dilation would make).  A blocked pair lowers kb[m].
// Phase 4, after a barrier, wave 0 with lane = candidate: the window test of the command, the score of an
// admissible candidate as (J << 6) | m, a wave min over the 64 lanes (J < 2^17, so the lowest m wins ties), the
// ballot's population count as n_adm, and the stores.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <type_traits>

#include "ffmp_device.h"
#include "ffmp_host.h"

#pragma clang fp contract(off)

namespace {

constexpr int kDwaThreads = 256;
constexpr int kDwaMaxCand = 64, kDwaMaxSteps = 32;
constexpr int kDwaTable = 28;              // |cell offset| of a table entry: the caller's contract
constexpr int kDwaFoot = 3;                // |footprint offset|: 28 + 3 = 31, the window's reach
constexpr int kDwaWin = 64, kDwaHalf = 32;  // the window: offsets -32 .. 31 from the robot cell
#ifndef FFMP_DWA_LIST
#define FFMP_DWA_LIST 1024
#endif
constexpr int kDwaList = FFMP_DWA_LIST;    // moving sources of an env dealt out over the block; the rest are walked where found
constexpr uint32_t kDwaInf = 65535u;

struct DwaArgs {
  const uint16_t* cost;
  int64_t cost_stride;   // elements
  const void* frame;     // or NULL (with flow): no moving sources
  int64_t frame_stride;  // elements
  const void* flow;
  int64_t flow_stride;   // elements
  const int16_t* traj;
  const double* cmds;
  const double* vel;     // or NULL
  const uint8_t* mask;   // or NULL
  int32_t* choice;
  double* cmd;
  uint32_t* score;
  int32_t* n_adm;
  uint8_t* blocked_at;
  double dv_max, dw_max;
  float cps;
  int32_t G, R, A, H;
  int32_t frame_vec;               // 16-byte loads of a float32 frame allowed
  uint8_t foot[2 * kDwaFoot + 1];  // foot[di + 3]: bit dj + 3 set where (di, dj) is a footprint offset
};

// the bits of the 4 cells at `f` that hold 255
template <typename FT>
FFMP_DEV uint32_t dwa_src4(const FT* f, bool vec) {
  if constexpr (std::is_same<FT, float>::value) {
    float4 v;
    if (vec) v = *reinterpret_cast<const float4*>(f);
    else v = make_float4(f[0], f[1], f[2], f[3]);
    return (v.x == 255.0f ? 1u : 0u) | (v.y == 255.0f ? 2u : 0u) | (v.z == 255.0f ? 4u : 0u) | (v.w == 255.0f ? 8u : 0u);
  } else {
    const uint32_t w = *reinterpret_cast<const uint32_t*>(f);
    return ((w & 255u) == 255u ? 1u : 0u) | (((w >> 8) & 255u) == 255u ? 2u : 0u) | (((w >> 16) & 255u) == 255u ? 4u : 0u) |
           ((w >> 24) == 255u ? 8u : 0u);
  }
}

// is (su, sv) a source's displacement: both finite, not both 0
FFMP_DEV bool dwa_moves(float su, float sv) { return (su - su == 0.0f) && (sv - sv == 0.0f) && !(su == 0.0f && sv == 0.0f); }

// the cell the source at (i, j) lands on at step k, into window k - 1 of the volume if it lies in the grid and the window
FFMP_DEV void dwa_land(uint32_t* vol32, int G, int i, int j, float su, float sv, int k) {
  const float Gf = (float)G;
  const float ru = rintf((float)k * su), rv = rintf((float)k * sv);
  // |r| >= G leaves the grid from any cell (an overflow to inf included): no integer is formed for it
  if (!(fabsf(ru) < Gf) || !(fabsf(rv) < Gf)) return;
  const int ti = i + (int)ru, tj = j + (int)rv;
  if ((unsigned)ti >= (unsigned)G || (unsigned)tj >= (unsigned)G) return;
  const int wi = ti - (G >> 1) + kDwaHalf, wj = tj - (G >> 1) + kDwaHalf;
  if ((unsigned)wi >= (unsigned)kDwaWin || (unsigned)wj >= (unsigned)kDwaWin) return;
  atomicOr(&vol32[(((k - 1) * kDwaWin + wi) << 1) + (wj >> 5)], 1u << (wj & 31));
}

template <typename FT, typename VT>
__global__ __launch_bounds__(kDwaThreads) void dwa_kernel(DwaArgs a) {
  __shared__ __attribute__((aligned(16))) uint64_t vol[kDwaMaxSteps * kDwaWin];
  __shared__ uint32_t list_ij[kDwaList > 0 ? kDwaList : 1];
  __shared__ float list_su[kDwaList > 0 ? kDwaList : 1], list_sv[kDwaList > 0 ? kDwaList : 1];
  __shared__ int kb[kDwaMaxCand];
  __shared__ int n_list;
  const int G = a.G, c = G >> 1, A = a.A, H = a.H;
  const int tid = threadIdx.x;
  const int64_t e = blockIdx.x;
  if (a.mask && a.mask[e] == 0) return;  // block-uniform
  const bool moving = a.frame != nullptr;  // block-uniform
  uint32_t* vol32 = reinterpret_cast<uint32_t*>(vol);

  // phase 1
  if (moving)
    for (int w = tid; w < H * kDwaWin; w += kDwaThreads) vol[w] = 0ull;
  if (tid < kDwaMaxCand) kb[tid] = H + 1;
  if (tid == 0) n_list = 0;
  __syncthreads();

  if (moving) {
    // phase 2a: the region of the frame within R cells of the robot cell; the sources onto the list
    const FT* frame = reinterpret_cast<const FT*>(a.frame) + e * a.frame_stride;
    const VT* vxp = reinterpret_cast<const VT*>(a.flow) + e * a.flow_stride;
    const VT* vyp = vxp + G * G;
    const int lo = max(c - a.R, 0), hi = min(c + a.R, G - 1);
    const int q_lo = lo >> 2, q_hi = hi >> 2;
    const bool fvec = a.frame_vec != 0;
    for (int i = lo + (tid >> 4); i <= hi; i += kDwaThreads >> 4) {
      for (int qd = q_lo + (tid & 15); qd <= q_hi; qd += 16) {
        const int j0 = qd << 2;
        uint32_t s = dwa_src4<FT>(frame + i * G + j0, fvec);
        for (; s; s &= s - 1u) {  // rare
          const int j = j0 + __builtin_ctz(s);
          if (j < lo || j > hi) continue;
          const int q = i * G + j;
          const float su = (float)vxp[q] * a.cps;
          const float sv = (float)vyp[q] * a.cps;
          if (!dwa_moves(su, sv)) continue;
          const int pos = kDwaList > 0 ? atomicAdd(&n_list, 1) : kDwaList;
          if (pos < kDwaList) {
            list_ij[pos] = ((uint32_t)i << 16) | (uint32_t)j;
            list_su[pos] = su;
            list_sv[pos] = sv;
          } else {  // the list is full: walked by the lane that found it
            for (int k = 1; k <= H; ++k) dwa_land(vol32, G, i, j, su, sv, k);
          }
        }
      }
    }
    __syncthreads();

    // phase 2b: the listed (source, k) pairs, one per thread at a time
    const unsigned pairs = (unsigned)min(n_list, kDwaList) * (unsigned)H;
    for (unsigned p = tid; p < pairs; p += kDwaThreads) {
      const unsigned s = p / (unsigned)H;
      const int k = (int)(p - s * (unsigned)H) + 1;
      const uint32_t ij = list_ij[s];
      dwa_land(vol32, G, (int)(ij >> 16), (int)(ij & 0xFFFFu), list_su[s], list_sv[s], k);
    }
    __syncthreads();
  }

  // phase 3: the (candidate, k) pairs
  const uint16_t* cost = a.cost + e * a.cost_stride;
  const unsigned tests = (unsigned)A * (unsigned)H;
  for (unsigned p = tid; p < tests; p += kDwaThreads) {
    const unsigned m = p / (unsigned)H;
    const int k = (int)(p - m * (unsigned)H) + 1;
    const int16_t* t = a.traj + ((size_t)m * (size_t)(H + 1) + (size_t)(k - 1)) * 2;
    const int oi = t[0], oj = t[1];
    const int pi = c + oi, pj = c + oj;
    bool blocked = (unsigned)pi >= (unsigned)G || (unsigned)pj >= (unsigned)G;
    if (!blocked) blocked = cost[pi * G + pj] == kDwaInf;
    // beyond the table's bound the window does not hold the footprint: no row is read
    if (!blocked && moving && abs(oi) <= kDwaTable && abs(oj) <= kDwaTable) {
      const uint64_t* win = vol + (k - 1) * kDwaWin + (oi + kDwaHalf - kDwaFoot);
      const int sh = oj + kDwaHalf - kDwaFoot;  // 1 .. 57
      uint32_t any = 0;
#pragma unroll
      for (int d = 0; d <= 2 * kDwaFoot; ++d) any |= (uint32_t)(win[d] >> sh) & (uint32_t)a.foot[d];
      blocked = any != 0u;
    }
    if (blocked) atomicMin(&kb[m], k);
  }
  __syncthreads();

  // phase 4: wave 0, lane = candidate
  if (tid >= 64) return;
  const int m = tid;
  const bool valid = m < A;
  double vm = 0.0, wm = 0.0;
  if (valid) {
    vm = a.cmds[2 * m];
    wm = a.cmds[2 * m + 1];
  }
  bool win = valid;
  if (a.vel) {  // block-uniform; a NaN fails
    const double v0 = a.vel[2 * e], w0 = a.vel[2 * e + 1];
    win = valid && fabs(vm - v0) <= a.dv_max && fabs(wm - w0) <= a.dw_max;
  }
  const int kbm = valid ? kb[m] : 0;
  const bool adm = win && kbm == H + 1;
  uint32_t key = 0xFFFFFFFFu;
  if (adm) {  // every p_k lies in the grid on a cost below 65535
    const int16_t* t = a.traj + ((size_t)m * (size_t)(H + 1) + (size_t)(H - 1)) * 2;
    const uint32_t g = cost[(c + t[0]) * G + (c + t[1])];
    const int qi = c + t[2], qj = c + t[3];  // the probe
    uint32_t h = kDwaInf - 1u;
    if ((unsigned)qi < (unsigned)G && (unsigned)qj < (unsigned)G) {
      const uint32_t hc = cost[qi * G + qj];
      if (hc < kDwaInf) h = hc;
    }
    key = ((g + h) << 6) | (uint32_t)m;  // g + h < 2^17
  }
  const int count = __popcll(__ballot(adm));
  uint32_t best = key;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) best = min(best, (uint32_t)__shfl_xor((int)best, o, 64));
  if (a.blocked_at && valid) a.blocked_at[e * A + m] = (uint8_t)(win ? kbm : 0);
  if (tid == 0) {
    const bool none = best == 0xFFFFFFFFu;
    const int ch = none ? -1 : (int)(best & 63u);
    if (a.choice) a.choice[e] = ch;
    if (a.score) a.score[e] = none ? 0xFFFFFFFFu : best >> 6;
    if (a.n_adm) a.n_adm[e] = count;
    if (a.cmd) {
      double2 out = make_double2(0.0, 0.0);
      if (!none) out = make_double2(a.cmds[2 * ch], a.cmds[2 * ch + 1]);
      *reinterpret_cast<double2*>(a.cmd + 2 * e) = out;
    }
  }
}

int dwa_check(const char* who, const ffmp_cfg_t* cfg, int32_t frame_format, int32_t flow_format, float cps, int32_t src_reach,
              int32_t A, int32_t H, double dv_max, double dw_max) {
  if (!cfg) return fail(FFMP_E_ARG, "%s: cfg is NULL", who);
  if (cfg->grid < 8 || cfg->grid > 512 || (cfg->grid % 4) != 0)
    return fail(FFMP_E_ARG, "%s: grid must be a multiple of 4 in [8,512], got %d", who, cfg->grid);
  if (frame_format != FFMP_OBS_F32 && frame_format != FFMP_OBS_U8F16)
    return fail(FFMP_E_ARG, "%s: unknown frame_format %d", who, frame_format);
  if (flow_format != FFMP_OBS_F32 && flow_format != FFMP_OBS_U8F16)
    return fail(FFMP_E_ARG, "%s: unknown flow_format %d", who, flow_format);
  if (!(cps - cps == 0.0f) || cps < 0.0f) return fail(FFMP_E_ARG, "%s: cps must be finite and >= 0", who);
  if (src_reach < 0 || src_reach > cfg->grid)
    return fail(FFMP_E_ARG, "%s: src_reach must be in [0,%d], got %d", who, cfg->grid, src_reach);
  if (A < 1 || A > kDwaMaxCand) return fail(FFMP_E_ARG, "%s: A must be in [1,%d], got %d", who, kDwaMaxCand, A);
  if (H < 1 || H > kDwaMaxSteps) return fail(FFMP_E_ARG, "%s: H must be in [1,%d], got %d", who, kDwaMaxSteps, H);
  if (!(dv_max >= 0.0)) return fail(FFMP_E_ARG, "%s: dv_max must be >= 0", who);
  if (!(dw_max >= 0.0)) return fail(FFMP_E_ARG, "%s: dw_max must be >= 0", who);
  if (cfg->n_foot < 0 || cfg->n_foot > FFMP_MAX_FOOT)
    return fail(FFMP_E_ARG, "%s: n_foot must be in [0,%d], got %d", who, FFMP_MAX_FOOT, cfg->n_foot);
  for (int f = 0; f < cfg->n_foot; ++f) {
    const int32_t di = cfg->foot_di[f], dj = cfg->foot_dj[f];
    if (di < -kDwaFoot || di > kDwaFoot || dj < -kDwaFoot || dj > kDwaFoot)
      return fail(FFMP_E_ARG, "%s: footprint offset (%d, %d) + a table offset of %d leaves the window of 31 cells (footprint)", who,
                  di, dj, kDwaTable);
  }
  return FFMP_OK;
}

// do the byte ranges [a, a + na) and [b, b + nb) meet
bool dwa_ranges_meet(const void* a, uint64_t na, const void* b, uint64_t nb) {
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return pa < pb ? pb - pa < na : pa - pb < nb;
}

// bytes of n envs of `tail` elements at `stride` elements each, `esize` bytes per element; false if they do not fit 64 bits
bool dwa_span(uint64_t last, int64_t stride, uint64_t tail, uint64_t esize, uint64_t* bytes) {
  uint64_t v;
  if (__builtin_mul_overflow(last, (uint64_t)stride, &v) || __builtin_add_overflow(v, tail, &v) ||
      __builtin_mul_overflow(v, esize, &v))
    return false;
  *bytes = v;
  return true;
}

struct DwaRange {
  const void* p;
  uint64_t bytes;
  const char* name;
};

}  // namespace

extern "C" {

int ffmp_dwa_check(const ffmp_cfg_t* cfg, int32_t frame_format, int32_t flow_format, float cps, int32_t src_reach, int32_t A,
                   int32_t H, double dv_max, double dw_max) {
  return dwa_check("ffmp_dwa", cfg, frame_format, flow_format, cps, src_reach, A, H, dv_max, dw_max);
}

int ffmp_dwa(const ffmp_cfg_t* cfg, int64_t n, const uint16_t* cost, int64_t cost_env_stride, const void* frame,
             int64_t frame_env_stride, int32_t frame_format, const void* flow, int64_t flow_env_stride, int32_t flow_format,
             float cps, int32_t src_reach, const int16_t* traj, const double* cmds, int32_t A, int32_t H, const double* vel,
             double dv_max, double dw_max, const uint8_t* mask, int32_t* choice, double* cmd, uint32_t* score, int32_t* n_adm,
             uint8_t* blocked_at, void* stream) {
  const char* who = "ffmp_dwa";
  if (int rc = dwa_check(who, cfg, frame_format, flow_format, cps, src_reach, A, H, dv_max, dw_max)) return rc;
  if (n < 0) return fail(FFMP_E_ARG, "%s: negative n", who);
  if (n > 0x7fffffffLL) return fail(FFMP_E_ARG, "%s: n too large for one launch: %lld", who, (long long)n);
  if (!cost) return fail(FFMP_E_ARG, "%s: cost is NULL", who);
  if (!traj) return fail(FFMP_E_ARG, "%s: traj is NULL", who);
  if (!cmds) return fail(FFMP_E_ARG, "%s: cmds is NULL", who);
  if ((frame == nullptr) != (flow == nullptr))
    return fail(FFMP_E_ARG, "%s: frame and flow go together: both given, or both NULL for no moving sources", who);
  if (!choice && !cmd && !score && !n_adm && !blocked_at) return fail(FFMP_E_ARG, "%s: every output is NULL", who);
  const int64_t G2 = (int64_t)cfg->grid * cfg->grid;
  if (cost_env_stride < G2)
    return fail(FFMP_E_ARG, "%s: cost_env_stride %lld < G*G = %lld", who, (long long)cost_env_stride, (long long)G2);
  if (((uintptr_t)cost & 1u) != 0) return fail(FFMP_E_ARG, "%s: cost must be 2-byte aligned (cost alignment)", who);
  if (frame) {
    if (frame_env_stride < G2)
      return fail(FFMP_E_ARG, "%s: frame_env_stride %lld < G*G = %lld", who, (long long)frame_env_stride, (long long)G2);
    if (flow_env_stride < 2 * G2)
      return fail(FFMP_E_ARG, "%s: flow_env_stride %lld < 2*G*G = %lld", who, (long long)flow_env_stride, (long long)(2 * G2));
    if (((uintptr_t)frame & 3u) != 0 || (frame_env_stride % 4) != 0)
      return fail(FFMP_E_ARG, "%s: frame must be 4-byte aligned with frame_env_stride a multiple of 4 elements (frame alignment)", who);
    if (((uintptr_t)flow & 3u) != 0 || (flow_env_stride % 4) != 0)
      return fail(FFMP_E_ARG, "%s: flow must be 4-byte aligned with flow_env_stride a multiple of 4 elements (flow alignment)", who);
  }
  if (((uintptr_t)traj & 3u) != 0) return fail(FFMP_E_ARG, "%s: traj must be 4-byte aligned (traj alignment)", who);
  if (((uintptr_t)cmds & 7u) != 0) return fail(FFMP_E_ARG, "%s: cmds must be 8-byte aligned (cmds alignment)", who);
  if (vel && ((uintptr_t)vel & 7u) != 0) return fail(FFMP_E_ARG, "%s: vel must be 8-byte aligned (vel alignment)", who);
  if (choice && ((uintptr_t)choice & 3u) != 0) return fail(FFMP_E_ARG, "%s: choice must be 4-byte aligned (choice alignment)", who);
  if (cmd && ((uintptr_t)cmd & 15u) != 0) return fail(FFMP_E_ARG, "%s: cmd must be 16-byte aligned (cmd alignment)", who);
  if (score && ((uintptr_t)score & 3u) != 0) return fail(FFMP_E_ARG, "%s: score must be 4-byte aligned (score alignment)", who);
  if (n_adm && ((uintptr_t)n_adm & 3u) != 0) return fail(FFMP_E_ARG, "%s: n_adm must be 4-byte aligned (n_adm alignment)", who);
  const uint64_t fes = frame_format == FFMP_OBS_F32 ? 4u : 1u, ves = flow_format == FFMP_OBS_F32 ? 4u : 2u;
  if (n > 0) {
    const uint64_t last = (uint64_t)(n - 1), un = (uint64_t)n;
    uint64_t cbytes = 0, ibytes = 0, vbytes = 0;
    if (!dwa_span(last, cost_env_stride, (uint64_t)G2, 2u, &cbytes) ||
        (frame && (!dwa_span(last, frame_env_stride, (uint64_t)G2, fes, &ibytes) ||
                   !dwa_span(last, flow_env_stride, 2u * (uint64_t)G2, ves, &vbytes))))
      return fail(FFMP_E_ARG, "%s: n envs at these env strides do not fit the address space (stride too large)", who);
    const DwaRange in[] = {
        {cost, cbytes, "cost"},
        {frame, ibytes, "frame"},
        {flow, vbytes, "flow"},
        {traj, (uint64_t)A * (uint64_t)(H + 1) * 4u, "traj"},
        {cmds, (uint64_t)A * 16u, "cmds"},
        {vel, vel ? un * 16u : 0u, "vel"},
        {mask, mask ? un : 0u, "mask"}};
    const DwaRange out[] = {{choice, 4u * un, "choice"}, {cmd, 16u * un, "cmd"}, {score, 4u * un, "score"},
                            {n_adm, 4u * un, "n_adm"}, {blocked_at, un * (uint64_t)A, "blocked_at"}};
    for (const DwaRange& o : out)
      for (const DwaRange& i : in)
        if (o.p && i.p && dwa_ranges_meet(o.p, o.bytes, i.p, i.bytes))
          return fail(FFMP_E_ARG, "%s: %s overlaps %s", who, o.name, i.name);
  }
  if (n == 0) return FFMP_OK;

  DwaArgs a;
  a.cost = cost;
  a.cost_stride = cost_env_stride;
  a.frame = frame;
  a.frame_stride = frame_env_stride;
  a.flow = flow;
  a.flow_stride = flow_env_stride;
  a.traj = traj;
  a.cmds = cmds;
  a.vel = vel;
  a.mask = mask;
  a.choice = choice;
  a.cmd = cmd;
  a.score = score;
  a.n_adm = n_adm;
  a.blocked_at = blocked_at;
  a.dv_max = dv_max;
  a.dw_max = dw_max;
  a.cps = cps;
  a.G = cfg->grid;
  a.R = src_reach;
  a.A = A;
  a.H = H;
  a.frame_vec = frame && ((uintptr_t)frame & 15u) == 0 && (((uint64_t)frame_env_stride * fes) & 15u) == 0;
  for (int d = 0; d <= 2 * kDwaFoot; ++d) a.foot[d] = 0;
  for (int f = 0; f < cfg->n_foot; ++f)
    a.foot[cfg->foot_di[f] + kDwaFoot] |= (uint8_t)(1u << (cfg->foot_dj[f] + kDwaFoot));
  const bool f32 = frame_format == FFMP_OBS_F32, v32 = flow_format == FFMP_OBS_F32;
  void (*k)(DwaArgs) = f32 ? (v32 ? dwa_kernel<float, float> : dwa_kernel<float, _Float16>)
                           : (v32 ? dwa_kernel<uint8_t, float> : dwa_kernel<uint8_t, _Float16>);
  hipLaunchKernelGGL(k, dim3((unsigned)n), dim3(kDwaThreads), 0, (hipStream_t)stream, a);
  return launch_ok(who);
}

}  // extern "C"
