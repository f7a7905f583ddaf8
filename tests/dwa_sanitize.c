/* Host-side exercise of ffmp_dwa / ffmp_dwa_check for the sanitizer build (tests/test_dwa_sanitize.py): the
 * argument checks on the paths that need no GPU — refusals, the n == 0 no-op, the corners of the footprint and of
 * the byte-range arithmetic — run against a libffmp whose host code is built with AddressSanitizer +
 * UndefinedBehaviorSanitizer.  No pointer given here is ever dereferenced by the library.  Exit 0 = every
 * expectation held (the sanitizers abort on their own findings). */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "ffmp.h"

static int failures = 0;
#define EXPECT(cond)                                                        \
  do {                                                                      \
    if (!(cond)) {                                                          \
      fprintf(stderr, "%s:%d: expectation failed: %s (last error: %s)\n", \
              __FILE__, __LINE__, #cond, ffmp_last_error());                \
      ++failures;                                                           \
    }                                                                       \
  } while (0)

#define P(x) ((void*)(uintptr_t)(x))

static int call(const ffmp_cfg_t* c, int64_t n, uintptr_t cost, int64_t cost_stride, uintptr_t frame, uintptr_t flow,
                int64_t stride, int32_t A, int32_t H, uintptr_t out) {
  const int64_t flow_stride = stride > INT64_MAX / 2 || stride < INT64_MIN / 2 ? stride : 2 * stride;
  return ffmp_dwa(c, n, (const uint16_t*)P(cost), cost_stride, P(frame), stride, FFMP_OBS_F32, P(flow), flow_stride,
                  FFMP_OBS_U8F16, 2.0f, 32, (const int16_t*)P(0x300000), (const double*)P(0x310000), A, H,
                  (const double*)P(0x320000), 0.1, 0.2, (const uint8_t*)P(0x330000), (int32_t*)P(out),
                  (double*)P(out + 0x1000), (uint32_t*)P(out + 0x2000), (int32_t*)P(out + 0x3000), (uint8_t*)P(out + 0x4000),
                  NULL);
}

int main(void) {
  static ffmp_cfg_t c;
  memset(&c, 0, sizeof(c));
  c.grid = 64;
  int k = 0;
  for (int di = -2; di <= 2; ++di)
    for (int dj = -2; dj <= 2; ++dj, ++k) {
      c.foot_di[k] = di;
      c.foot_dj[k] = dj;
    }
  c.n_foot = k;
  const int64_t G2 = 64 * 64;

  EXPECT(ffmp_dwa_check(&c, 0, 1, 2.0f, 32, 28, 18, 0.0, INFINITY) == FFMP_OK);
  EXPECT(ffmp_dwa_check(NULL, 0, 0, 2.0f, 32, 28, 18, 0.0, 0.0) == FFMP_E_ARG);
  EXPECT(ffmp_dwa_check(&c, 0, 0, NAN, 32, 28, 18, 0.0, 0.0) == FFMP_E_ARG);
  EXPECT(ffmp_dwa_check(&c, 0, 0, 2.0f, 32, 28, 18, NAN, 0.0) == FFMP_E_ARG);
  EXPECT(ffmp_dwa_check(&c, 0, 0, 2.0f, INT32_MAX, 28, 18, 0.0, 0.0) == FFMP_E_ARG);
  EXPECT(ffmp_dwa_check(&c, 0, 0, 2.0f, INT32_MIN, 28, 18, 0.0, 0.0) == FFMP_E_ARG);
  EXPECT(ffmp_dwa_check(&c, INT32_MAX, INT32_MIN, 2.0f, 32, 28, 18, 0.0, 0.0) == FFMP_E_ARG);
  EXPECT(ffmp_dwa_check(&c, 0, 0, 2.0f, 32, INT32_MAX, 18, 0.0, 0.0) == FFMP_E_ARG);
  EXPECT(ffmp_dwa_check(&c, 0, 0, 2.0f, 32, 28, INT32_MIN, 0.0, 0.0) == FFMP_E_ARG);

  /* the footprint: every offset of the table's 128 is looked at, none beyond n_foot; the extremes of int32 */
  ffmp_cfg_t f = c;
  f.n_foot = FFMP_MAX_FOOT;
  EXPECT(ffmp_dwa_check(&f, 0, 0, 2.0f, 32, 28, 18, 0.0, 0.0) == FFMP_OK);
  f.foot_di[FFMP_MAX_FOOT - 1] = 4;
  EXPECT(ffmp_dwa_check(&f, 0, 0, 2.0f, 32, 28, 18, 0.0, 0.0) == FFMP_E_ARG && strstr(ffmp_last_error(), "footprint"));
  f.n_foot = FFMP_MAX_FOOT - 1;
  EXPECT(ffmp_dwa_check(&f, 0, 0, 2.0f, 32, 28, 18, 0.0, 0.0) == FFMP_OK);
  f.n_foot = FFMP_MAX_FOOT + 1;
  EXPECT(ffmp_dwa_check(&f, 0, 0, 2.0f, 32, 28, 18, 0.0, 0.0) == FFMP_E_ARG);
  f.n_foot = -1;
  EXPECT(ffmp_dwa_check(&f, 0, 0, 2.0f, 32, 28, 18, 0.0, 0.0) == FFMP_E_ARG);
  f = c;
  f.foot_dj[0] = INT32_MIN;
  EXPECT(ffmp_dwa_check(&f, 0, 0, 2.0f, 32, 28, 18, 0.0, 0.0) == FFMP_E_ARG);
  f.foot_dj[0] = INT32_MAX;
  EXPECT(ffmp_dwa_check(&f, 0, 0, 2.0f, 32, 28, 18, 0.0, 0.0) == FFMP_E_ARG);
  f.foot_dj[0] = 3;
  f.foot_di[0] = -3;
  EXPECT(ffmp_dwa_check(&f, 0, 0, 2.0f, 32, 28, 18, 0.0, 0.0) == FFMP_OK);

  /* the launch entry: n == 0 passes every check and launches nothing; refusals come before any HIP call */
  EXPECT(call(&c, 0, 0x100000, G2, 0x1000000, 0x2000000, G2, 28, 18, 0x400000) == FFMP_OK);
  EXPECT(call(&f, 0, 0x100000, G2, 0x1000000, 0x2000000, G2, 64, 32, 0x400000) == FFMP_OK);
  EXPECT(call(&c, -1, 0x100000, G2, 0x1000000, 0x2000000, G2, 28, 18, 0x400000) == FFMP_E_ARG);
  EXPECT(call(&c, INT64_MAX, 0x100000, G2, 0x1000000, 0x2000000, G2, 28, 18, 0x400000) == FFMP_E_ARG);
  EXPECT(call(&c, INT64_MIN, 0x100000, G2, 0x1000000, 0x2000000, G2, 28, 18, 0x400000) == FFMP_E_ARG);
  EXPECT(call(&c, 4, 0, G2, 0x1000000, 0x2000000, G2, 28, 18, 0x400000) == FFMP_E_ARG && strstr(ffmp_last_error(), "cost is NULL"));
  EXPECT(call(&c, 4, 0x100000, G2, 0, 0x2000000, G2, 28, 18, 0x400000) == FFMP_E_ARG && strstr(ffmp_last_error(), "go together"));
  EXPECT(call(&c, 4, 0x100000, G2 - 1, 0x1000000, 0x2000000, G2, 28, 18, 0x400000) == FFMP_E_ARG);
  EXPECT(call(&c, 4, 0x100000, INT64_MIN, 0x1000000, 0x2000000, G2, 28, 18, 0x400000) == FFMP_E_ARG);
  EXPECT(call(&c, 4, 0x100000, G2, 0x1000000, 0x2000000, INT64_MIN, 28, 18, 0x400000) == FFMP_E_ARG);
  /* overlaps: an output on the first and on the last byte of the cost plane, and strides whose ranges wrap */
  EXPECT(call(&c, 4, 0x100000, G2, 0x1000000, 0x2000000, G2, 28, 18, 0x100000) == FFMP_E_ARG && strstr(ffmp_last_error(), "overlaps cost"));
  EXPECT(call(&c, 4, 0x100000, G2, 0x1000000, 0x2000000, G2, 28, 18, 0x100000 + 8 * G2 - 4) == FFMP_E_ARG);
  EXPECT(call(&c, 0x7fffffff, 0x100000, INT64_MAX, 0x1000000, 0x2000000, G2, 64, 32, 0x400000) == FFMP_E_ARG && strstr(ffmp_last_error(), "stride too large"));
  EXPECT(call(&c, 0x7fffffff, 0x100000, G2, 0x1000000, 0x2000000, INT64_MAX / 2 - 3, 64, 32, 0x400000) == FFMP_E_ARG && strstr(ffmp_last_error(), "stride too large"));
  EXPECT(call(&c, 3, 0x100000, G2, 0x1000000, 0x2000000, (INT64_MAX / 16) * 4, 64, 32, 0x400000) == FFMP_E_ARG && strstr(ffmp_last_error(), "stride too large"));

  if (failures) {
    fprintf(stderr, "%d expectation(s) failed\n", failures);
    return 1;
  }
  printf("all host-side checks passed\n");
  return 0;
}
