// Per-box arithmetic of the visible-box selection (visible_boxes.hip): the occlusion and minimum-size tests of the
// reference's VisibleBboxSelector step (check_bbox_visibiity / check_minimum_bbox_size, dali_pipeline_framework
// operators_impl/numba_operators/numba_operators.py:240-403) for one box.  The GPU kernel and the host entry
// accv_visible_boxes_host evaluate the same functions.  Everything is float32 until the conversion to integers; decisions
// are comparisons only.
//
//   corners    min_x = b0 < b2 ? b0 : b2, max_x the other one; y likewise.  A NaN coordinate excludes the box.
//   rounding   expand: lo = floor(min), hi = ceil(max); shrink: lo = ceil(min), hi = floor(max); each rounded edge is
//              clamped in float to [-1, W + 1] ([-1, H + 1] for y) and then converted.  W, H <= 2^24, so the conversion is
//              exact and +-inf / 1e30 are defined; no decision below changes for a finite value.
//   outside    lo_x > W || hi_x < 0 || lo_y > H || hi_y < 0 excludes the box
//   clip       x0 = max(lo_x, 0), x1 = min(hi_x, W), y likewise: the painted rectangle is [x0, x1) x [y0, y1); empty when
//              x0 >= x1 or y0 >= y1
//   order      box j lies above box i iff key(depth_j) < key(depth_i), or the keys are equal and j > i.  key maps a float
//              to an unsigned that ascends with the value, -0.0 == 0.0, every NaN to 0 (below -inf): a NaN depth lies on
//              top, two NaNs tie.  That is np.argsort(-depth, kind="stable"), last painted on top.
//   size       each raw coordinate clipped in float to [0, W] ([0, H] for y) by comparisons (a NaN stays NaN);
//              |x2 - x1| >= min_size && |y2 - y1| >= min_size, NaN fails
//
// A box that paints nothing is stored as the rectangle (-1, -1, -1, -1): it spans no point and its edges equal no real edge.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>

namespace accv_vb {

constexpr int kMaxBoxes = 256;            // ACCV_VB_MAX_BOXES
constexpr int kWords = kMaxBoxes / 64;    // 64-bit words of a bit set over the boxes of a frame
constexpr long long kMaxExtent = 1ll << 24;

struct Rect {
    int x0, y0, x1, y1;
};

__host__ __device__ inline Rect no_rect() { return Rect{-1, -1, -1, -1}; }

__host__ __device__ inline long long clamp_extent(long long v) { return v < 0 ? 0 : (v > kMaxExtent ? kMaxExtent : v); }

// one axis: the clipped integer interval [lo, hi) of the corner pair (a, b) on an image of extent E, false when the box is
// outside on this axis.  Neither a nor b is NaN.
__host__ __device__ inline bool axis_interval(float a, float b, float E, int shrink, int& lo, int& hi)
{
    const float mn = a < b ? a : b, mx = a < b ? b : a;
    float l = shrink ? ceilf(mn) : floorf(mn);
    float h = shrink ? floorf(mx) : ceilf(mx);
    const float top = E + 1.0f;
    l = l < -1.0f ? -1.0f : (l > top ? top : l);
    h = h < -1.0f ? -1.0f : (h > top ? top : h);
    if (l > E || h < 0.0f) return false;
    lo = (int)(l < 0.0f ? 0.0f : l);
    hi = (int)(h > E ? E : h);
    return true;
}

// the rectangle a box paints, no_rect() when it paints nothing
__host__ __device__ inline Rect painted_rect(const float* b, float Wf, float Hf, int shrink)
{
    if (b[0] != b[0] || b[1] != b[1] || b[2] != b[2] || b[3] != b[3]) return no_rect();
    Rect r;
    const bool in_x = axis_interval(b[0], b[2], Wf, shrink, r.x0, r.x1);
    const bool in_y = axis_interval(b[1], b[3], Hf, shrink, r.y0, r.y1);
    if (!in_x || !in_y || r.x0 >= r.x1 || r.y0 >= r.y1) return no_rect();
    return r;
}

__host__ __device__ inline bool paints(const Rect& r) { return r.x0 >= 0; }

__host__ __device__ inline uint32_t depth_key(float d)
{
    if (d != d) return 0u;
    if (d == 0.0f) return 0x80000000u;
    uint32_t u;
    memcpy(&u, &d, 4);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// box j (key kj) lies above box i (key ki)
__host__ __device__ inline bool above(uint32_t kj, int j, uint32_t ki, int i) { return kj < ki || (kj == ki && j > i); }

__host__ __device__ inline float clip_raw(float v, float E) { return v < 0.0f ? 0.0f : (v > E ? E : v); }

__host__ __device__ inline bool size_ok(const float* b, float Wf, float Hf, float min_size)
{
    const float dx = fabsf(clip_raw(b[2], Wf) - clip_raw(b[0], Wf));
    const float dy = fabsf(clip_raw(b[3], Hf) - clip_raw(b[1], Hf));
    return dx >= min_size && dy >= min_size;
}

// Bit k of a bit set is the box with k boxes above it (its layer).  The layer of the top-most box at a point: the lowest set
// bit of X & Y over `words` words, -1 when none; word w of Y is Y[w * stride]
__host__ __device__ inline int top_layer(const unsigned long long* X, const unsigned long long* Y, int stride, int words)
{
    for (int w = 0; w < words; ++w) {
        const unsigned long long m = X[w] & Y[w * stride];
        if (m) return 64 * w + __builtin_ctzll(m);
    }
    return -1;
}

}  // namespace accv_vb
