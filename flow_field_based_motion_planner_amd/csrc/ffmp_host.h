// ffmp_host.h — what the host side of every libffmp source shares: the error message behind
// ffmp_last_error(), the check after a kernel launch, and the tuning hooks ffmp_set_tuning() reaches
// in the other sources.  Definitions: ffmp_kernels.hip unless noted.
#pragma once
#include "ffmp.h"

namespace ffmp_detail {
// Sets the thread's ffmp_last_error() text and returns `code`.
__attribute__((format(printf, 2, 3))) int fail(int code, const char* fmt, ...);
// After a kernel launch: FFMP_OK, or FFMP_E_HIP with "<who>: HIP launch failed: <HIP's text>".
int launch_ok(const char* who);

int32_t ring_extra_swap(int32_t v);  // ffmp_ring.hip (FFMP_TUNE_RING_EXTRA)
int conv_mfma_swap(int v);           // ffmp_conv.hip (FFMP_TUNE_CONV_MFMA)
int conv_kys_swap(int v);            // ffmp_conv.hip (FFMP_TUNE_CONV_KYS)
int conv_lb_swap(int v);             // ffmp_conv.hip (FFMP_TUNE_CONV_LB)
int conv_wgpf_swap(int v);           // ffmp_conv.hip (FFMP_TUNE_CONV_WGPF)
int conv_ba2_swap(int v);            // ffmp_conv.hip (FFMP_TUNE_CONV_BA2)
int conv_mbw_swap(int v);            // ffmp_conv.hip (FFMP_TUNE_CONV_MBW)
int conv_planar_swap(int v);         // ffmp_conv.hip (FFMP_TUNE_CONV_PLANAR)
int conv_pin_swap(int v);            // ffmp_conv.hip (FFMP_TUNE_CONV_PIN)
int conv_wgdma_swap(int v);          // ffmp_conv.hip (FFMP_TUNE_CONV_WGDMA)
}  // namespace ffmp_detail
using ffmp_detail::fail;
using ffmp_detail::launch_ok;
