// What ffmp_dwa.hip's host code takes from ffmp_kernels.hip (csrc/ffmp_host.h), restated for the sanitizer build of
// tests/test_dwa_sanitize.py so that it need not compile the step's kernels: the error text behind
// ffmp_last_error() and the check after a launch (never reached there: the program launches nothing).
#include <stdarg.h>
#include <stdio.h>

#include "ffmp.h"

namespace ffmp_detail {
static thread_local char g_err[512];
__attribute__((format(printf, 2, 3))) int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}
int launch_ok(const char* who) { return fail(FFMP_E_HIP, "%s: launched from the sanitizer program", who); }
}  // namespace ffmp_detail

extern "C" const char* ffmp_last_error(void) { return ffmp_detail::g_err; }
