// What every unit of the library shares and none of the kernels own: the calling thread's error text, the code of its last
// conv kernel, the ABI version and the reload of the planning switches.
#include "conv_common.h"

#include <stdarg.h>
#include <stdio.h>

namespace pseg {

static thread_local char g_err[512] = "";
thread_local int g_last_conv_kernel = 0;      // pseg_debug_last_conv_kernel (conv_common.h)
thread_local int g_last_wgrad[kWgradRecord] = {};      // pseg_debug_last_wgrad (conv_common.h)
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
const char* last_error() { return g_err; }

}  // namespace pseg

extern "C" {

int pseg_abi_version(void) { return PSEG_ABI_VERSION; }
int pseg_debug_last_conv_kernel(void) { return pseg::g_last_conv_kernel; }
int pseg_debug_last_wgrad(int* out11) {
  PSEG_REQUIRE(out11 != nullptr, "debug_last_wgrad: null pointer");
  for (int i = 0; i < pseg::kWgradRecord; ++i) out11[i] = pseg::g_last_wgrad[i];
  return PSEG_OK;
}
int pseg_config_reload(void) {
  pseg::cfg_load();
  return PSEG_OK;
}
const char* pseg_last_error(void) { return pseg::last_error(); }

}  // extern "C"
