// Camera-box augmentation for a ragged batch of 2D annotations in one launch: the annotation side of the reference's
// AffineTransformer (the 2 x 3 image matrix applied to box corners, centres and projection matrices), its
// VisibleBboxSelector on the warped boxes, the condition "categories >= 0 and is_visible", the ConditionalElementRemover
// over boxes, centres, depths and categories, and the two CoordinateCroppers.  Per frame (one camera image) the kept slots
// are compacted in ascending slot order with their source slots; the rest of each row is filled (0, source -1), the keep
// and visible flags of every input slot and the kept count are written, so every output element is written exactly once.
// Per-frame arithmetic: camera_boxes_arith.h; the visibility decision: visible_boxes_arith.h and the walk of
// visible_boxes_block.h, the same one visible_boxes.hip runs.
//
// One workgroup of kThreads = kMaxBoxes lanes per frame, a lane per box slot:
//   1. the lane loads its box, centre, depth, category and flag and warps the points in registers;
//   2. it clips the warped box to its painted rectangle and joins the block-wide visibility walk (block_visible);
//   3. keep = visible && category >= 0 && valid; accv::block_rank gives the output slot (one more barrier, its own LDS row);
//   4. kept lanes store their cropped row, the lanes from the kept count on store the filler, every lane its two flags;
//   5. the same lanes write the projection matrices, an element per lane, striding over all elements of the frame.  The
//      views are 4-byte aligned only, so elements move one by one; rows 2 and 3 move as 32-bit words.
// The matrix of the frame, the extent and the count are the same in every lane.  No atomics on global memory, no workspace,
// no host synchronisation: the order is defined by the slot number, so the result is bitwise reproducible.  The walk is
// nearly all of the time (visible_boxes_block.h); launch and latency bound work, no MFMA.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>
#include <cstring>

#include "accv_common.h"
#include "accv_numeric.h"
#include "camera_boxes_arith.h"
#include "visible_boxes_arith.h"
#include "visible_boxes_block.h"

#pragma clang fp contract(off)

namespace {

using namespace accv_vb;
using namespace accv_cb;
using accv::clamp_count;
using accv::load_index;

constexpr int kMaxMat = ACCV_CB_MAX_MATRICES;
constexpr unsigned kKnownFlags = ACCV_CB_COUNTS_I64 | ACCV_CB_HW_I64 | ACCV_CB_CATEGORIES_I64;

static_assert(kMaxBoxes == ACCV_CB_MAX_BOXES, "visible_boxes_arith.h and accv_hip.h disagree");

struct Args {
    const float* boxes;             // [F, G, 4]
    const float* transforms;        // [F, 2, 3]
    const float* centers;           // [F, G, 2] or null
    const float* depths;            // [F, G] or null
    const void* categories;         // [F, G] or null
    const unsigned char* valid;     // [F, G] or null
    const void* counts;             // [F]
    const void* image_hw;           // [F, 2] or null
    float* out_boxes;               // [F, G, 4]
    float* out_centers;             // [F, G, 2] or null
    float* out_depths;              // [F, G] or null
    void* out_categories;           // [F, G] of the categories' type, or null
    int* source;                    // [F, G]
    unsigned char* keep;            // [F, G]
    unsigned char* visible;         // [F, G]
    long long* sizes;               // [F]
    const float* mat_in[kMaxMat];
    float* mat_out[kMaxMat];
    long long mat_items[kMaxMat];   // elements per frame, K * R * C
    int mat_rows[kMaxMat], mat_cols[kMaxMat];
    long long F, G, H, W;
    float min_size;
    int counts64, hw64, cat64, occlusion, size, shrink, crop, order, num_mat;
};

// (H, W) of frame f as floats, exact: both are clamped to [0, 2^24]
__host__ __device__ inline void frame_extent(const Args& a, long long f, float& Hf, float& Wf)
{
    long long H = a.H, W = a.W;
    if (a.image_hw) H = load_index(a.image_hw, 2 * f, a.hw64), W = load_index(a.image_hw, 2 * f + 1, a.hw64);
    Hf = (float)clamp_extent(H), Wf = (float)clamp_extent(W);
}

// what a slot brings along
struct Slot {
    float box[4], center[2], depth;
    long long category;
    bool wanted;                    // category >= 0 && valid
};

// slot o = f * G + g read and warped; depths, categories and flags are read only where they are given
__host__ __device__ inline Slot load_slot(const Args& a, const Affine& t, long long o)
{
    Slot s;
    const float* p = a.boxes + o * 4;
    warp_point(t, p[0], p[1], s.box[0], s.box[1]);
    warp_point(t, p[2], p[3], s.box[2], s.box[3]);
    if (a.order) order_pair(s.box[0], s.box[2]), order_pair(s.box[1], s.box[3]);
    s.center[0] = s.center[1] = 0.0f;
    if (a.centers) warp_point(t, a.centers[o * 2], a.centers[o * 2 + 1], s.center[0], s.center[1]);
    s.depth = a.depths ? a.depths[o] : 0.0f;
    s.category = a.categories ? load_index(a.categories, o, a.cat64) : 0;
    s.wanted = s.category >= 0 && (!a.valid || a.valid[o] != 0);
    return s;
}

// everything a kept slot writes: output slot o_out (the frame included) from input slot g of the frame
__host__ __device__ inline void write_slot(const Args& a, const Slot& s, long long o_out, int g, float Hf, float Wf)
{
    float* ob = a.out_boxes + o_out * 4;
    if (a.crop) {
        ob[0] = crop_coordinate(s.box[0], Wf), ob[1] = crop_coordinate(s.box[1], Hf);
        ob[2] = crop_coordinate(s.box[2], Wf), ob[3] = crop_coordinate(s.box[3], Hf);
    } else {
        ob[0] = s.box[0], ob[1] = s.box[1], ob[2] = s.box[2], ob[3] = s.box[3];
    }
    if (a.out_centers) {
        a.out_centers[o_out * 2] = a.crop ? crop_coordinate(s.center[0], Wf) : s.center[0];
        a.out_centers[o_out * 2 + 1] = a.crop ? crop_coordinate(s.center[1], Hf) : s.center[1];
    }
    if (a.out_depths) a.out_depths[o_out] = s.depth;
    if (a.out_categories) {
        if (a.cat64) static_cast<long long*>(a.out_categories)[o_out] = s.category;
        else static_cast<int*>(a.out_categories)[o_out] = (int)s.category;
    }
    a.source[o_out] = g;
}

// the filler of output slot o
__host__ __device__ inline void write_padding(const Args& a, long long o)
{
    float* ob = a.out_boxes + o * 4;
    ob[0] = ob[1] = ob[2] = ob[3] = 0.0f;
    if (a.out_centers) a.out_centers[o * 2] = a.out_centers[o * 2 + 1] = 0.0f;
    if (a.out_depths) a.out_depths[o] = 0.0f;
    if (a.out_categories) {
        if (a.cat64) static_cast<long long*>(a.out_categories)[o] = 0;
        else static_cast<int*>(a.out_categories)[o] = 0;
    }
    a.source[o] = -1;
}

// element e of the `items` matrix elements of a frame (in, out: the frame's first element)
__host__ __device__ inline void write_matrix_element(const Affine& t, const float* in, float* out, long long e, int R, int C)
{
    const int rc = R * C;
    const int within = (int)(e % rc), row = within / C, col = within - row * C;
    if (row < 2) {
        out[e] = matrix_element(t, in + (e - within), row, col, C);
    } else {   // bit for bit, a signalling NaN included
        uint32_t bits;
        memcpy(&bits, in + e, 4);
        memcpy(out + e, &bits, 4);
    }
}

// ------------------------------------------------------------------------------------------------------------- device
__global__ __launch_bounds__(kThreads) void camera_boxes_kernel(const Args a)
{
    __shared__ int s_rank[kWaves];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const long long f = blockIdx.x;
    const int n = (int)clamp_count(a.counts, f, a.G, a.counts64);
    float Hf, Wf;
    frame_extent(a, f, Hf, Wf);
    const Affine t = load_affine(a.transforms + f * 6);
    const long long row0 = f * a.G;
    const bool real = tid < n;
    Slot s;
    s.box[0] = s.box[1] = s.box[2] = s.box[3] = s.center[0] = s.center[1] = s.depth = 0.0f;
    s.category = 0, s.wanted = false;
    if (real) s = load_slot(a, t, row0 + tid);
    bool vis = real && (!a.size || size_ok(s.box, Wf, Hf, a.min_size));
    if (a.occlusion) {   // the same in every lane
        const Rect r = real ? painted_rect(s.box, Wf, Hf, a.shrink) : no_rect();
        const uint32_t key = real ? depth_key(s.depth) : 0u;
        const bool top = block_visible(n, real, r, key, tid, lane, wave);
        vis = vis && top;
    }
    const bool on = vis && s.wanted;
    int before, total;
    accv::block_rank<kWaves>(on, s_rank, lane, wave, before, total);
    if (on) write_slot(a, s, row0 + before, tid, Hf, Wf);
    if (tid < a.G) {
        if (tid >= total) write_padding(a, row0 + tid);
        a.keep[row0 + tid] = on ? 1 : 0;
        a.visible[row0 + tid] = vis ? 1 : 0;
    }
    if (tid == 0) a.sizes[f] = total;

#pragma unroll
    for (int i = 0; i < kMaxMat; ++i) {
        if (i >= a.num_mat) break;
        const long long items = a.mat_items[i];
        const float* in = a.mat_in[i] + f * items;
        float* out = a.mat_out[i] + f * items;
        for (long long e = tid; e < items; e += kThreads) write_matrix_element(t, in, out, e, a.mat_rows[i], a.mat_cols[i]);
    }
}

// --------------------------------------------------------------------------------------------------------------- host
void host_run(const Args& a)
{
    static thread_local Slot slots[kMaxBoxes];
    static thread_local float warped[kMaxBoxes * 4], depth[kMaxBoxes];
    static thread_local unsigned char vis[kMaxBoxes];
    for (long long f = 0; f < a.F; ++f) {
        const int n = (int)clamp_count(a.counts, f, a.G, a.counts64);
        float Hf, Wf;
        frame_extent(a, f, Hf, Wf);
        const Affine t = load_affine(a.transforms + f * 6);
        const long long row0 = f * a.G;
        for (int g = 0; g < n; ++g) {
            slots[g] = load_slot(a, t, row0 + g);
            for (int c = 0; c < 4; ++c) warped[g * 4 + c] = slots[g].box[c];
            depth[g] = slots[g].depth;
        }
        if (a.occlusion || a.size) host_frame_visible(warped, depth, n, Hf, Wf, a.occlusion, a.size, a.min_size, a.shrink, vis);
        else for (int g = 0; g < n; ++g) vis[g] = 1;
        long long kept = 0;
        for (int g = 0; g < n; ++g) {
            const bool on = vis[g] && slots[g].wanted;
            a.keep[row0 + g] = on ? 1 : 0;
            a.visible[row0 + g] = vis[g] ? 1 : 0;
            if (on) write_slot(a, slots[g], row0 + kept++, g, Hf, Wf);
        }
        for (long long g = n; g < a.G; ++g) a.keep[row0 + g] = 0, a.visible[row0 + g] = 0;
        for (long long g = kept; g < a.G; ++g) write_padding(a, row0 + g);
        a.sizes[f] = kept;
        for (int i = 0; i < a.num_mat; ++i) {
            const long long items = a.mat_items[i];
            for (long long e = 0; e < items; ++e)
                write_matrix_element(t, a.mat_in[i] + f * items, a.mat_out[i] + f * items, e, a.mat_rows[i], a.mat_cols[i]);
        }
    }
}

// ------------------------------------------------------------------------------------------------------------- checks
inline uintptr_t addr(const void* p) { return reinterpret_cast<uintptr_t>(p); }

// ACCV_OK with *empty = 1 when there is nothing to write; every check runs before anything else reads the arguments
int check_args(const char* who, const float* boxes, const float* transforms, const float* centers, const float* depths,
               const void* categories, const unsigned char* valid, const void* counts, unsigned flags, long long F, long long G,
               const accv_camera_boxes_params* p, float* out_boxes, float* out_centers, float* out_depths, void* out_categories,
               int* source, unsigned char* keep, unsigned char* visible, long long* out_sizes, Args& a, int* empty)
{
    *empty = 0;
    if (!p) return accv::fail(ACCV_EINVAL, "%s: null params", who);
    if (F < 0 || G < 0) return accv::fail(ACCV_EINVAL, "%s: negative size", who);
    if (flags & ~kKnownFlags) return accv::fail(ACCV_EINVAL, "%s: unknown flags 0x%x", who, flags);
    if (G > kMaxBoxes) return accv::fail(ACCV_EINVAL, "%s: %lld box slots per frame, at most %d supported", who, G, kMaxBoxes);
    if (p->num_matrices < 0 || p->num_matrices > kMaxMat)
        return accv::fail(ACCV_EINVAL, "%s: 0..%d matrix tensors supported, got %d", who, kMaxMat, p->num_matrices);
    bool any_matrix = false;
    for (int i = 0; i < p->num_matrices; ++i) {
        if (p->mat_count[i] < 0 || (p->mat_rows[i] != 3 && p->mat_rows[i] != 4) || (p->mat_cols[i] != 3 && p->mat_cols[i] != 4))
            return accv::fail(ACCV_EINVAL, "%s: matrix tensor %d needs K >= 0 matrices of 3 or 4 rows and columns, got %lld of %d x %d",
                              who, i, p->mat_count[i], p->mat_rows[i], p->mat_cols[i]);
        any_matrix = any_matrix || p->mat_count[i] > 0;
    }
    if (F == 0 || (G == 0 && !any_matrix)) {
        *empty = 1;
        return ACCV_OK;
    }
    if (!transforms || !counts || !out_sizes) return accv::fail(ACCV_EINVAL, "%s: null transforms / counts / sizes pointer", who);
    if (G > 0 && (!boxes || !out_boxes || !source || !keep || !visible))
        return accv::fail(ACCV_EINVAL, "%s: null boxes / output pointer", who);
    if (G > 0 && p->check_occlusion && !depths) return accv::fail(ACCV_EINVAL, "%s: the occlusion check needs depths", who);
    if (G > 0 && (flags & ACCV_CB_CATEGORIES_I64) && !categories)
        return accv::fail(ACCV_EINVAL, "%s: int64 categories flagged but not given", who);
    if ((flags & ACCV_CB_HW_I64) && !p->image_hw) return accv::fail(ACCV_EINVAL, "%s: int64 image_hw flagged but not given", who);
    if (G > 0 && ((centers != nullptr) != (out_centers != nullptr) || (depths != nullptr) != (out_depths != nullptr) ||
                  (categories != nullptr) != (out_categories != nullptr)))
        return accv::fail(ACCV_EINVAL, "%s: centers / depths / categories and their outputs come together or not at all", who);
    if ((addr(boxes) | addr(transforms) | addr(centers) | addr(depths) | addr(out_boxes) | addr(out_centers) | addr(out_depths) |
         addr(source)) & 3u)
        return accv::fail(ACCV_EINVAL, "%s: a 4-byte tensor is not aligned to its element size", who);
    if (addr(out_sizes) & 7u) return accv::fail(ACCV_EINVAL, "%s: sizes must be 8-byte aligned", who);
    if (((addr(categories) | addr(out_categories)) & ((flags & ACCV_CB_CATEGORIES_I64) ? 7u : 3u)) ||
        (addr(counts) & ((flags & ACCV_CB_COUNTS_I64) ? 7u : 3u)) || (addr(p->image_hw) & ((flags & ACCV_CB_HW_I64) ? 7u : 3u)))
        return accv::fail(ACCV_EINVAL, "%s: categories / counts / image_hw are not aligned to their element size", who);
    if (F > accv::kGridLimit) return accv::fail(ACCV_EINVAL, "%s: %lld workgroups exceed the grid limit", who, F);
    const long long cap = LLONG_MAX / 64;   // elements of any tensor, in bytes with room to spare
    for (int i = 0; i < kMaxMat; ++i) a.mat_in[i] = nullptr, a.mat_out[i] = nullptr, a.mat_items[i] = 0, a.mat_rows[i] = 3, a.mat_cols[i] = 3;
    for (int i = 0; i < p->num_matrices; ++i) {
        if (p->mat_count[i] > cap / 16 / F) return accv::fail(ACCV_EINVAL, "%s: sizes overflow", who);
        a.mat_rows[i] = p->mat_rows[i], a.mat_cols[i] = p->mat_cols[i];
        a.mat_items[i] = p->mat_count[i] * p->mat_rows[i] * p->mat_cols[i];
        if (a.mat_items[i] == 0) continue;
        if (!p->mat_in[i] || !p->mat_out[i]) return accv::fail(ACCV_EINVAL, "%s: matrix tensor %d has a null pointer", who, i);
        if ((addr(p->mat_in[i]) | addr(p->mat_out[i])) & 3u)
            return accv::fail(ACCV_EINVAL, "%s: matrix tensor %d is not aligned to its element size", who, i);
        a.mat_in[i] = p->mat_in[i], a.mat_out[i] = p->mat_out[i];
    }
    const bool slots = G > 0;
    a.boxes = boxes, a.transforms = transforms, a.centers = slots ? centers : nullptr, a.depths = slots ? depths : nullptr;
    a.categories = slots ? categories : nullptr, a.valid = slots ? valid : nullptr, a.counts = counts, a.image_hw = p->image_hw;
    a.out_boxes = out_boxes, a.out_centers = slots ? out_centers : nullptr, a.out_depths = slots ? out_depths : nullptr;
    a.out_categories = slots ? out_categories : nullptr, a.source = source, a.keep = keep, a.visible = visible, a.sizes = out_sizes;
    a.F = F, a.G = G, a.H = p->image_h, a.W = p->image_w;
    a.min_size = (float)p->minimum_size;
    a.counts64 = (flags & ACCV_CB_COUNTS_I64) ? 1 : 0, a.hw64 = (flags & ACCV_CB_HW_I64) ? 1 : 0;
    a.cat64 = (flags & ACCV_CB_CATEGORIES_I64) ? 1 : 0;
    a.occlusion = p->check_occlusion ? 1 : 0, a.size = p->check_size ? 1 : 0, a.shrink = p->shrink_to_int ? 1 : 0;
    a.crop = p->crop ? 1 : 0, a.order = p->order_corners ? 1 : 0, a.num_mat = p->num_matrices;
    return ACCV_OK;
}

}  // namespace

extern "C" {

int accv_camera_boxes(const float* boxes, const float* transforms, const float* centers, const float* depths,
                      const void* categories, const unsigned char* valid, const void* counts, unsigned flags, long long F,
                      long long G, const accv_camera_boxes_params* params, float* out_boxes, float* out_centers,
                      float* out_depths, void* out_categories, int* source, unsigned char* keep, unsigned char* visible,
                      long long* out_sizes, void* stream)
{
    const char* who = "camera_augment_boxes";
    Args a;
    int empty;
    if (int rc = check_args(who, boxes, transforms, centers, depths, categories, valid, counts, flags, F, G, params, out_boxes,
                            out_centers, out_depths, out_categories, source, keep, visible, out_sizes, a, &empty))
        return rc;
    if (empty) return ACCV_OK;
    hipLaunchKernelGGL(camera_boxes_kernel, dim3((unsigned)a.F), dim3(kThreads), 0, static_cast<hipStream_t>(stream), a);
    return accv::check_launch(who);
}

int accv_camera_boxes_host(const float* boxes, const float* transforms, const float* centers, const float* depths,
                           const void* categories, const unsigned char* valid, const void* counts, unsigned flags,
                           long long F, long long G, const accv_camera_boxes_params* params, float* out_boxes,
                           float* out_centers, float* out_depths, void* out_categories, int* source, unsigned char* keep,
                           unsigned char* visible, long long* out_sizes)
{
    const char* who = "camera_augment_boxes (host)";
    Args a;
    int empty;
    if (int rc = check_args(who, boxes, transforms, centers, depths, categories, valid, counts, flags, F, G, params, out_boxes,
                            out_centers, out_depths, out_categories, source, keep, visible, out_sizes, a, &empty))
        return rc;
    if (empty) return ACCV_OK;
    host_run(a);
    return ACCV_OK;
}

}  // extern "C"
