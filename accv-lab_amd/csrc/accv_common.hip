// Error reporting, version and the last-dispatch string of libaccv_hip.so.
#include "accv_common.h"

#include <cstring>

namespace accv {

char* error_buffer()
{
    static thread_local char buf[512] = {0};
    return buf;
}

int fail(int code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(error_buffer(), 512, fmt, ap);
    va_end(ap);
    return code;
}

char* dispatch_buffer()
{
    static thread_local char buf[256] = {0};
    return buf;
}

}  // namespace accv

extern "C" {

const char* accv_last_error(void) { return accv::error_buffer(); }

int accv_version(void) { return 100; }

const char* accv_draw_heatmap_last_dispatch(void) { return accv::dispatch_buffer(); }
}
