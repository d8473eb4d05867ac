// Per-object arithmetic of the fused box-to-heat-map targets (box_heatmap.hip): the reference's
// BoundingBoxToHeatmapConverter step (dali_pipeline_framework processing_steps/bounding_box_to_heatmap_converter.py) for one
// object: apply_clipping_and_get_with_clipping_info and get_is_active (operators_impl/python_operator_functions/
// python_operator_functions.py:103-252) and get_center_from_bboxes / get_radii_from_bboxes (operators_impl/numba_operators/
// numba_operators.py:788-905).  The GPU kernel and the host entry accv_box_heatmap_host evaluate the same operation sequence
// from these functions.  Everything is float32; contraction into fma is off for everything that includes this header; every
// `/` below is ONE correctly rounded division (__fdiv_rn on the device, `/` on the host), every other operator one IEEE
// operation, evaluated exactly as parenthesised here.  Decisions are comparisons only, so a NaN fails all of them.
//
// Constants of a frame: sx = (float)Wm / (float)Wi, sy = (float)Hm / (float)Hi (map over image extent; a zero image extent
// gives inf), xm = (float)(Wm - 1), ym = (float)(Hm - 1).  Constants of a call, rounded once to float32 from the caller's
// numbers: thr = min_fraction_area_clipping, rs = radius_scaling_factor, rlo = max(0.5, min_radius), rhi = max_radius.
//
//   centre     given, or ((b0 + b2) * 0.5, (b1 + b3) * 0.5)
//   scaling    X1 = sx * b0, Y1 = sy * b1, X2 = sx * b2, Y2 = sy * b3, CX = sx * c0, CY = sy * c1
//   finite     all six are finite; otherwise the object is inactive and every output of it is 0
//   clip       clip(v, m) = v < 0 ? 0 : (v > m ? m : v);  x1 = clip(X1, xm), y1 = clip(Y1, ym), x2, y2 likewise: the clipped
//              box, in input corner order
//   size       h = |y2 - y1|, w = |x2 - x1|
//   fraction   (h * w) / (|Y2 - Y1| * |X2 - X1|); 0 / 0 is NaN
//   centre     cx = clip(CX, xm), cy = clip(CY, ym); ix = (int)floor(cx), iy = (int)floor(cy); offsets cx - floor(cx),
//              cy - floor(cy)
//   radius     l = x1 <= x2 ? x1 : x2, r the other one, t = y1 <= y2 ? y1 : y2, b the other one;
//              d = min(cx - l, cy - t, r - cx, b - cy) by comparisons; d = d < 0 ? 0 : d; q = d * rs;
//              q = q < rlo ? rlo : q; radius = q > rhi ? rhi : q
//   active     finite && fraction >= thr && (h >= min_h && w >= min_w) && 0 <= category < num_categories && is_valid, each
//              test only where the call requests it; min_h, min_w global or of the object's category
//   drawing    R = (int)ceil(radius); sigma = radius * rsf; the exponent of a pixel at integer distance (dx, dy) is
//              -(float)(dx * dx + dy * dy) * (1 / ((2 * sigma) * sigma)), the factor capped at FLT_MAX
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>

#pragma clang fp contract(off)

namespace accv_bh {

constexpr int kMaxBoxes = 256;         // ACCV_BH_MAX_BOXES
constexpr int kMaxCategories = 128;    // ACCV_BH_MAX_CATEGORIES
constexpr long long kMaxExtent = 1ll << 24;   // of an image and of a map: every extent is exact in float32

// the scalar constants of a call, rounded to float32 once on the host
struct Consts {
    float thr, rs, rlo, rhi, rsf;
    float min_h, min_w;   // the global minimum size
};

// the constants of a frame
struct Frame {
    float sx, sy, xm, ym;
};

// everything the operator knows about one object
struct Record {
    float box[4];     // clipped, input corner order
    float h, w;       // clipped size
    int ix, iy;       // integer centre
    float ox, oy;     // sub-pixel offset
    float radius;
    float fraction;
    bool finite;
};

__host__ __device__ inline float div_rn(float a, float b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __fdiv_rn(a, b);
#else
    return a / b;
#endif
}

__host__ __device__ inline long long clamp_extent(long long v) { return v < 0 ? 0 : (v > kMaxExtent ? kMaxExtent : v); }

// Wm, Hm in [1, 2^24]; Wi, Hi in [0, 2^24]
__host__ __device__ inline Frame frame_consts(long long Wm, long long Hm, long long Wi, long long Hi)
{
    Frame f;
    f.sx = div_rn((float)Wm, (float)Wi);
    f.sy = div_rn((float)Hm, (float)Hi);
    f.xm = (float)(Wm - 1);
    f.ym = (float)(Hm - 1);
    return f;
}

__host__ __device__ inline bool is_finite(float v) { return fabsf(v) <= FLT_MAX; }   // false for NaN

__host__ __device__ inline float clip(float v, float m) { return v < 0.0f ? 0.0f : (v > m ? m : v); }

__host__ __device__ inline Record zero_record()
{
    Record r;
    r.box[0] = r.box[1] = r.box[2] = r.box[3] = 0.0f;
    r.h = r.w = r.ox = r.oy = r.radius = r.fraction = 0.0f;
    r.ix = r.iy = 0;
    r.finite = false;
    return r;
}

// (b0, b1, b2, b3): the raw box; (g0, g1): the raw centre when `given`, else the centre of the box is taken
__host__ __device__ inline Record object_record(float b0, float b1, float b2, float b3, bool given, float g0, float g1,
                                                const Frame& f, const Consts& k)
{
    const float c0 = given ? g0 : (b0 + b2) * 0.5f;
    const float c1 = given ? g1 : (b1 + b3) * 0.5f;
    const float X1 = f.sx * b0, Y1 = f.sy * b1, X2 = f.sx * b2, Y2 = f.sy * b3;
    const float CX = f.sx * c0, CY = f.sy * c1;
    if (!(is_finite(X1) && is_finite(Y1) && is_finite(X2) && is_finite(Y2) && is_finite(CX) && is_finite(CY)))
        return zero_record();
    Record r;
    r.finite = true;
    const float x1 = clip(X1, f.xm), y1 = clip(Y1, f.ym), x2 = clip(X2, f.xm), y2 = clip(Y2, f.ym);
    r.box[0] = x1, r.box[1] = y1, r.box[2] = x2, r.box[3] = y2;
    r.h = fabsf(y2 - y1);
    r.w = fabsf(x2 - x1);
    const float ho = fabsf(Y2 - Y1), wo = fabsf(X2 - X1);
    r.fraction = div_rn(r.h * r.w, ho * wo);
    const float cx = clip(CX, f.xm), cy = clip(CY, f.ym);
    const float fx = floorf(cx), fy = floorf(cy);
    r.ix = (int)fx, r.iy = (int)fy;     // in [0, 2^24): exact
    r.ox = cx - fx, r.oy = cy - fy;
    const float l = x1 <= x2 ? x1 : x2, rr = x1 <= x2 ? x2 : x1;
    const float t = y1 <= y2 ? y1 : y2, bb = y1 <= y2 ? y2 : y1;
    float d = cx - l;
    const float d1 = cy - t, d2 = rr - cx, d3 = bb - cy;
    d = d1 < d ? d1 : d;
    d = d2 < d ? d2 : d;
    d = d3 < d ? d3 : d;
    d = d < 0.0f ? 0.0f : d;
    float q = d * k.rs;
    q = q < k.rlo ? k.rlo : q;
    r.radius = q > k.rhi ? k.rhi : q;
    return r;
}

// the tests of `active` that need no class: finite, area fraction, and the size test against (min_h, min_w) when check_size
__host__ __device__ inline bool passes(const Record& r, const Consts& k, bool check_size, float min_h, float min_w)
{
    return r.finite && r.fraction >= k.thr && (!check_size || (r.h >= min_h && r.w >= min_w));
}

// the patch radius in pixels; radius is in [0.5, rhi] with rhi <= 2^14, or 0 for a record that is not drawn
__host__ __device__ inline int patch_radius(float radius) { return (int)ceilf(radius); }

// the factor of the squared pixel distance in the exponent, positive and at most FLT_MAX (a sigma whose square underflows
// leaves the centre pixel at k and every other one at 0, which is the limit)
__host__ __device__ inline float exponent_factor(float radius, float rsf)
{
    const float sigma = radius * rsf;
    const float inv = div_rn(1.0f, (2.0f * sigma) * sigma);
    return inv > FLT_MAX ? FLT_MAX : inv;
}

}  // namespace accv_bh
