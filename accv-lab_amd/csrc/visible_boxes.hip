// Visible-box selection for a ragged batch of 2D boxes: the occlusion test and the minimum-size test of the reference's
// VisibleBboxSelector step (dali_pipeline_framework operators_impl/numba_operators/numba_operators.py:240-403) without the
// H x W canvas.  Per-box arithmetic: visible_boxes_arith.h.
//
// One workgroup of kThreads = kMaxBoxes lanes per frame, a lane per box slot: the lane clips its box to the painted rectangle
// and takes its depth key, the workgroup walks the frame (visible_boxes_block.h: why the points (x edge, y edge) are enough,
// steps 1 to 5 and what they cost; camera_boxes.hip calls the same walk), and the flag AND the size test go out, padding
// slots as 0: every output byte is written, nothing is cleared beforehand.
// No atomics on global memory, no global scratch, no host synchronisation.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "accv_common.h"
#include "accv_numeric.h"
#include "visible_boxes_arith.h"
#include "visible_boxes_block.h"

namespace {

using namespace accv_vb;
using accv::clamp_count;
using accv::load_index;

constexpr unsigned kKnownFlags = ACCV_VB_COUNTS_I64 | ACCV_VB_HW_I64;

static_assert(kMaxBoxes == ACCV_VB_MAX_BOXES, "visible_boxes_arith.h and accv_hip.h disagree");

struct Args {
    const float* boxes;        // [B, G, 4]
    const float* depths;       // [B, G] or null
    const void* counts;        // [B]
    const void* image_hw;      // [B, 2] or null
    unsigned char* out;        // [B, G]
    long long B, G, H, W;
    float min_size;
    int counts64, hw64, occlusion, size, shrink;
};

// (H, W) of frame b as floats, exact: both are clamped to [0, 2^24]
__host__ __device__ inline void frame_extent(const Args& a, long long b, float& Hf, float& Wf)
{
    long long H = a.H, W = a.W;
    if (a.image_hw) H = load_index(a.image_hw, 2 * b, a.hw64), W = load_index(a.image_hw, 2 * b + 1, a.hw64);
    Hf = (float)clamp_extent(H), Wf = (float)clamp_extent(W);
}

// ------------------------------------------------------------------------------------------------------------- device
__global__ __launch_bounds__(kThreads) void visible_boxes_kernel(const Args a)
{
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const long long b = blockIdx.x;
    const int n = (int)clamp_count(a.counts, b, a.G, a.counts64);
    float Hf, Wf;
    frame_extent(a, b, Hf, Wf);
    const bool real = tid < n;
    float box[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (real) {
        const float* p = a.boxes + (b * a.G + tid) * 4;
        box[0] = p[0], box[1] = p[1], box[2] = p[2], box[3] = p[3];
    }
    const bool big = !a.size || (real && size_ok(box, Wf, Hf, a.min_size));
    if (!a.occlusion) {   // the same in every lane
        if (tid < a.G) a.out[b * a.G + tid] = real && big;
        return;
    }
    const Rect r = real ? painted_rect(box, Wf, Hf, a.shrink) : no_rect();
    const uint32_t key = real ? depth_key(a.depths[b * a.G + tid]) : 0u;
    const bool top = block_visible(n, real, r, key, tid, lane, wave);
    if (tid < a.G) a.out[b * a.G + tid] = real && big && top;
}

// --------------------------------------------------------------------------------------------------------------- host
// the same algorithm, one frame after the other
void host_run(const Args& a)
{
    for (long long b = 0; b < a.B; ++b) {
        const int n = (int)clamp_count(a.counts, b, a.G, a.counts64);
        float Hf, Wf;
        frame_extent(a, b, Hf, Wf);
        unsigned char* out = a.out + b * a.G;
        host_frame_visible(a.boxes + b * a.G * 4, a.depths ? a.depths + b * a.G : nullptr, n, Hf, Wf, a.occlusion, a.size,
                           a.min_size, a.shrink, out);
        for (long long i = n; i < a.G; ++i) out[i] = 0;
    }
}

// ------------------------------------------------------------------------------------------------------------- checks
// ACCV_OK with *empty = 1 when there is nothing to write; every check runs before anything else reads the arguments
int check_args(const char* who, const float* boxes, const float* depths, const void* counts, const void* image_hw,
               unsigned flags, long long B, long long G, const accv_visible_boxes_params* p, unsigned char* out, Args& a,
               int* empty)
{
    *empty = 0;
    if (!p) return accv::fail(ACCV_EINVAL, "%s: null params", who);
    if (B < 0 || G < 0) return accv::fail(ACCV_EINVAL, "%s: negative size", who);
    if (flags & ~kKnownFlags) return accv::fail(ACCV_EINVAL, "%s: unknown flags 0x%x", who, flags);
    if (!p->check_occlusion && !p->check_size)
        return accv::fail(ACCV_EINVAL, "%s: at least one of the occlusion and the minimum-size check must be requested", who);
    if (G > kMaxBoxes) return accv::fail(ACCV_EINVAL, "%s: %lld box slots per frame, at most %d supported", who, G, kMaxBoxes);
    if (B == 0 || G == 0) {
        *empty = 1;
        return ACCV_OK;
    }
    if (!boxes || !counts || !out) return accv::fail(ACCV_EINVAL, "%s: null boxes / counts / output pointer", who);
    if (p->check_occlusion && !depths) return accv::fail(ACCV_EINVAL, "%s: the occlusion check needs depths", who);
    if ((reinterpret_cast<uintptr_t>(boxes) | reinterpret_cast<uintptr_t>(depths)) & 3u)
        return accv::fail(ACCV_EINVAL, "%s: boxes / depths are not aligned to their element size", who);
    if ((reinterpret_cast<uintptr_t>(counts) & ((flags & ACCV_VB_COUNTS_I64) ? 7u : 3u)) ||
        (reinterpret_cast<uintptr_t>(image_hw) & ((flags & ACCV_VB_HW_I64) ? 7u : 3u)))
        return accv::fail(ACCV_EINVAL, "%s: counts / image_hw are not aligned to their element size", who);
    if (B > accv::kGridLimit) return accv::fail(ACCV_EINVAL, "%s: %lld workgroups exceed the grid limit", who, B);
    a.boxes = boxes, a.depths = depths, a.counts = counts, a.image_hw = image_hw, a.out = out;
    a.B = B, a.G = G, a.H = p->image_h, a.W = p->image_w;
    a.min_size = (float)p->minimum_size;
    a.counts64 = (flags & ACCV_VB_COUNTS_I64) ? 1 : 0, a.hw64 = (flags & ACCV_VB_HW_I64) ? 1 : 0;
    a.occlusion = p->check_occlusion ? 1 : 0, a.size = p->check_size ? 1 : 0, a.shrink = p->shrink_to_int ? 1 : 0;
    return ACCV_OK;
}

}  // namespace

extern "C" {

int accv_visible_boxes(const float* boxes, const float* depths, const void* counts, const void* image_hw, unsigned flags,
                       long long B, long long G, const accv_visible_boxes_params* params, unsigned char* out, void* stream)
{
    const char* who = "visible_bbox_mask";
    Args a;
    int empty;
    if (int rc = check_args(who, boxes, depths, counts, image_hw, flags, B, G, params, out, a, &empty)) return rc;
    if (empty) return ACCV_OK;
    hipLaunchKernelGGL(visible_boxes_kernel, dim3((unsigned)a.B), dim3(kThreads), 0, static_cast<hipStream_t>(stream), a);
    return accv::check_launch(who);
}

int accv_visible_boxes_host(const float* boxes, const float* depths, const void* counts, const void* image_hw, unsigned flags,
                            long long B, long long G, const accv_visible_boxes_params* params, unsigned char* out)
{
    const char* who = "visible_bbox_mask (host)";
    Args a;
    int empty;
    if (int rc = check_args(who, boxes, depths, counts, image_hw, flags, B, G, params, out, a, &empty)) return rc;
    if (empty) return ACCV_OK;
    host_run(a);
    return ACCV_OK;
}

}  // extern "C"
