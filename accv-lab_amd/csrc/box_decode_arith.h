// Per-peak and per-pair arithmetic of the 2D box decoder and the axis-aligned NMS (box_decode.hip): the inverse of
// box_heatmap_arith.h for one peak of a CenterNet / FCOS-style camera head, and the greedy IoU rule of mmdet's batched_nms
// (without its coordinate-offset trick: classes are compared, not moved apart) for one pair.  The GPU kernels and the host
// entries accv_box_decode_cpu / accv_box_nms_cpu evaluate the same operation sequence from these functions.  Everything is
// float32; contraction into fma is off for everything that includes this header; every div_rn is ONE correctly rounded
// division (__fdiv_rn on the device, `/` on the host), every other operator one IEEE operation, evaluated exactly as
// parenthesised here.  Decisions are comparisons only, so a NaN fails all of them.
//
// Constants of a frame: ux = div_rn((float)Wi, (float)Wm), uy = div_rn((float)Hi, (float)Hm) (image over map extent, the
// reciprocal direction of box_heatmap_arith.h's frame_consts); EW = (float)Wi, EH = (float)Hi.  Every extent is at most 2^24
// and so exact.  Constants of a call, rounded once to float32 from the caller's numbers: thr = score_threshold; min_h,
// min_w = min_size; iou_thr = iou_threshold.
// Gathered channels (f16 / bf16 widened exactly): (off_x, off_y, h, w) at the peak's cell, xs = index % Wm, ys = index / Wm.
//
//   centre     cx = (float)xs + off_x                  cy = (float)ys + off_y
//   half       hw = 0.5 * w                            hh = 0.5 * h
//   map box    mx1 = cx - hw, my1 = cy - hh, mx2 = cx + hw, my2 = cy + hh
//   image box  x1 = mx1 * ux, y1 = my1 * uy, x2 = mx2 * ux, y2 = my2 * uy
//   clip       (optional) v < 0 ? 0 : (v > E ? E : v) with E = EW for x and EH for y, camera_boxes_arith.h's crop_coordinate:
//              NaN stays NaN, +-inf go to the borders
//   size       bh = y2 - y1, bw = x2 - x1 of the (clipped) box
//   score      s, or with scores_are_logits  div_rn(1, 1 + exp(-s))
//   validity   (no threshold or score > thr) && (no min_size or (bh >= min_h && bw >= min_w)) && x1, y1, x2, y2 all finite
//   area       bw * bh
//   iou        lx = max(ax1, bx1), rx = min(ax2, bx2), ty = max(ay1, by1), by = min(ay2, by2) by comparisons;
//              iw = rx - lx, iw = iw > 0 ? iw : 0; ih likewise; inter = iw * ih;
//              iou = div_rn(inter, (area_a + area_b) - inter); 0 / 0 is NaN
//   suppress   a kept box suppresses a later one iff both take part && (class_agnostic || their classes are equal) &&
//              iou > iou_thr; a NaN iou suppresses nothing
//   inverse    (optional, on written boxes only) with image_prep_arith.h's load_warp of the frame's forward matrix
//              [[a, b, tx], [c, d, ty]] (det = a * d - b * c): u = x - tx, v = y - ty;
//              x' = div_rn(d * u - b * v, det), y' = div_rn(a * v - c * u, det) for each of the two corners; with
//              order_corners the pairs (x1', x2') and (y1', y2') go through camera_boxes_arith.h's order_pair.  A matrix that
//              load_warp does not accept (not finite, det == 0, 1 / det not finite) gives the box (0, 0, 0, 0).
//
// Roundings that feed one written coordinate, which the round-trip tests' bars count (each adds at most 2^-24 times the
// magnitude of what it rounds): centre (1), half (1, exact for a power-of-two factor but counted), map box (1), image box,
// ux included (2): kDecodeRoundings = 5; the inverse adds u / v (1), two products (2), their difference (1), det's own three
// and the division (4): kInverseRoundings = 8.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>

#include "box_heatmap_arith.h"
#include "camera_boxes_arith.h"
#include "image_prep_arith.h"

#pragma clang fp contract(off)

namespace accv_bd {

using accv_bh::div_rn;
using accv_bh::is_finite;

constexpr int kMaxMaps = 8;        // ACCV_BD_MAX_MAPS
constexpr int kMaxExtras = 4;      // ACCV_BD_MAX_EXTRAS
constexpr int kMaxChannels = 4 + kMaxExtras;
constexpr int kMaxK = 1024;        // ACCV_BD_MAX_K: peaks of a frame, and slots of a frame for the NMS alone
constexpr long long kMaxExtent = accv_bh::kMaxExtent;
constexpr int kDecodeRoundings = 5;
constexpr int kInverseRoundings = 8;

// the scalar constants of a call, rounded to float32 once on the host
struct Consts {
    float thr, min_h, min_w, iou_thr;
    int has_thr, has_min, has_iou, logits, clip, order, agnostic;
};

// the constants of a frame
struct Frame {
    float ux, uy, EW, EH;
};

// Wm, Hm in [1, 2^24]; Wi, Hi in [0, 2^24]
__host__ __device__ inline Frame frame_consts(long long Wm, long long Hm, long long Wi, long long Hi)
{
    Frame f;
    f.EW = (float)Wi, f.EH = (float)Hi;
    f.ux = div_rn(f.EW, (float)Wm);
    f.uy = div_rn(f.EH, (float)Hm);
    return f;
}

// an axis-aligned box as the NMS sees it
struct Box {
    float x1, y1, x2, y2, area;
    long long cls;
    bool ok;      // takes part in the IoU test: all four coordinates finite
};

__host__ __device__ inline Box no_box()
{
    Box b;
    b.x1 = b.y1 = b.x2 = b.y2 = b.area = 0.0f;
    b.cls = 0;
    b.ok = false;
    return b;
}

__host__ __device__ inline Box make_box(float x1, float y1, float x2, float y2, long long cls)
{
    Box b;
    b.x1 = x1, b.y1 = y1, b.x2 = x2, b.y2 = y2;
    b.area = (x2 - x1) * (y2 - y1);
    b.cls = cls;
    b.ok = is_finite(x1) && is_finite(y1) && is_finite(x2) && is_finite(y2);
    return b;
}

// steps 2 to 4: the image-space box of a peak from its cell and the four gathered channels
__host__ __device__ inline void corners(const Consts& k, const Frame& f, long long xs, long long ys, float off_x, float off_y, float h,
                                        float w, float& x1, float& y1, float& x2, float& y2)
{
    const float cx = (float)xs + off_x, cy = (float)ys + off_y;
    const float hw = 0.5f * w, hh = 0.5f * h;
    const float mx1 = cx - hw, my1 = cy - hh, mx2 = cx + hw, my2 = cy + hh;
    x1 = mx1 * f.ux, y1 = my1 * f.uy, x2 = mx2 * f.ux, y2 = my2 * f.uy;
    if (k.clip) {
        x1 = accv_cb::crop_coordinate(x1, f.EW), y1 = accv_cb::crop_coordinate(y1, f.EH);
        x2 = accv_cb::crop_coordinate(x2, f.EW), y2 = accv_cb::crop_coordinate(y2, f.EH);
    }
}

// step 5
__host__ __device__ inline float score_of(const Consts& k, float s) { return k.logits ? div_rn(1.0f, 1.0f + expf(-s)) : s; }

__host__ __device__ inline bool passes(const Consts& k, float score, float x1, float y1, float x2, float y2)
{
    if (k.has_thr && !(score > k.thr)) return false;
    if (k.has_min && !((y2 - y1) >= k.min_h && (x2 - x1) >= k.min_w)) return false;
    return is_finite(x1) && is_finite(y1) && is_finite(x2) && is_finite(y2);
}

// step 6
__host__ __device__ inline float iou(const Box& a, const Box& b)
{
    const float lx = a.x1 > b.x1 ? a.x1 : b.x1, rx = a.x2 < b.x2 ? a.x2 : b.x2;
    const float ty = a.y1 > b.y1 ? a.y1 : b.y1, by = a.y2 < b.y2 ? a.y2 : b.y2;
    float iw = rx - lx, ih = by - ty;
    iw = iw > 0.0f ? iw : 0.0f;
    ih = ih > 0.0f ? ih : 0.0f;
    const float inter = iw * ih;
    return div_rn(inter, (a.area + b.area) - inter);
}

// does the kept box `kept` suppress the later box `later`
__host__ __device__ inline bool suppresses(const Box& kept, const Box& later, float thr, bool agnostic)
{
    return kept.ok && later.ok && (agnostic || kept.cls == later.cls) && iou(kept, later) > thr;
}

// step 8: the box back in the source image, in place
__host__ __device__ inline void to_source(const accv_ip::Warp& w, bool order, float& x1, float& y1, float& x2, float& y2)
{
    if (w.copy) return;
    if (!w.ok) {
        x1 = y1 = x2 = y2 = 0.0f;
        return;
    }
    const float u1 = x1 - w.tx, v1 = y1 - w.ty, u2 = x2 - w.tx, v2 = y2 - w.ty;
    x1 = div_rn(w.d * u1 - w.b * v1, w.det), y1 = div_rn(w.a * v1 - w.c * u1, w.det);
    x2 = div_rn(w.d * u2 - w.b * v2, w.det), y2 = div_rn(w.a * v2 - w.c * u2, w.det);
    if (order) accv_cb::order_pair(x1, x2), accv_cb::order_pair(y1, y2);
}

}  // namespace accv_bd
