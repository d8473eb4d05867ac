// Shared host-side helpers for libaccv_hip.so (error reporting, launch checks). gfx950 only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>

#include "accv_hip.h"

namespace accv {

char* error_buffer();  // thread-local, 512 bytes
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

// Checks the sticky launch error after a kernel launch / async enqueue.
inline int check_launch(const char* what)
{
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(ACCV_ELAUNCH, "%s: %s", what, hipGetErrorString(e));
    return ACCV_OK;
}

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// the caller's workspace: present, 16-byte aligned and of at least `need` bytes
inline int check_workspace(const char* who, const void* workspace, size_t given, size_t need)
{
    if (!workspace || given < need || (reinterpret_cast<uintptr_t>(workspace) & 15u))
        return fail(ACCV_EWORKSPACE, "%s: workspace of %zu bytes (16-byte aligned) needed, %zu given", who, need, given);
    return ACCV_OK;
}

constexpr long long kGridLimit = 0x7fffffffll;   // workgroups along x of one launch

char* dispatch_buffer();  // thread-local, 256 bytes: description of the last draw_heatmap dispatch

}  // namespace accv
