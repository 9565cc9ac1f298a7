// Library plumbing of libdgmr_hip.so: the last-error text, the ABI version and the deterministic-mode switch.
#include <stdarg.h>

#include "common.h"

// ------------------------------------------------------------------------------------------------
// error plumbing
// ------------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";
void dgmr_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
extern "C" const char* dgmr_last_error(void) { return g_err; }
extern "C" int dgmr_abi_version(void) { return DGMR_ABI_VERSION; }
int g_deterministic = 0;
extern "C" int dgmr_set_deterministic(int on) {
    g_deterministic = on ? 1 : 0;
    return 0;
}
extern "C" int dgmr_get_deterministic(void) { return g_deterministic; }
