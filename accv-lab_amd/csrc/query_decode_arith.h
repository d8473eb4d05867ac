// Per-rank arithmetic of the set-prediction box decoders (query_decode.hip): mmdet3d's NMSFreeCoder.decode with
// denormalize_bbox, and mmdet's DETRHead._predict_by_feat_single, for one selected (query, class) pair.  The GPU kernel and
// the host entries accv_query_decode_3d_cpu / accv_query_decode_2d_cpu evaluate the same operation sequence from these
// functions.  Everything is float32; contraction into fma is off for everything that includes this header; every operator is
// ONE IEEE operation, evaluated exactly as parenthesised here; div_rn is ONE correctly rounded division.  Decisions are
// comparisons only, so a NaN fails all of them.  Nothing of the two headers below is restated: the 3D row is
// center_decode_arith.h's score_of, passes and box_row on a re-ordered row, the 2D row box_decode_arith.h's score_of,
// crop_coordinate, passes and to_source.
//
// Selection (topk_select.h): the Q * C raw values of a frame ranked by descending value, equal values (-0.0 == +0.0) by
// ascending flat index q * C + c, every NaN above +inf.  For rank r: q = index / C, label = index % C, x = the raw value.
//
//   score      x, or with scores_are_logits  div_rn(1, 1 + exp(-x))
//
// 3D, from the row p = bbox_preds[b, q] = (cx, cy, log w, log l, cz, log h, sin, cos[, vx, vy]) (f16 / bf16 widened exactly):
//   validity   (no threshold or score > thr) && (no range or lo[0] <= cx && cx <= hi[0] && lo[1] <= cy && cy <= hi[1] &&
//              lo[2] <= cz && cz <= hi[2])
//   row        (cx, cy, cz, exp(log w), exp(log l), exp(log h), atan2(sin, cos)[, vx, vy]); with bottom_center the third value
//              is cz - exp(log h) * 0.5 (after the range test); cx, cy, cz and the velocity are bit copies; exp / atan2 are
//              expf / atan2f of the platform (device and host agree to a few ulp, not bit for bit)
//
// 2D, from the row p = bbox_preds[b, q] and the frame's image extent EW = (float)Wi, EH = (float)Hi:
//   corners    cxcywh: hw = 0.5 * p[2], hh = 0.5 * p[3]; x1 = p[0] - hw, y1 = p[1] - hh, x2 = p[0] + hw, y2 = p[1] + hh
//              xyxy:   (x1, y1, x2, y2) = p
//   scale      (normalized) x1 = x1 * EW, y1 = y1 * EH, x2 = x2 * EW, y2 = y2 * EH
//   clip       (optional) crop_coordinate(v, E): v < 0 ? 0 : (v > E ? E : v)
//   validity   (no threshold or score > thr) && x1, y1, x2, y2 all finite
//   inverse    (optional, on written boxes only) box_decode_arith.h's to_source: the two corners through the inverse of the
//              frame's matrix, ordered per axis with order_corners; (0, 0, 0, 0) for a matrix load_warp does not accept
#pragma once
#include <hip/hip_runtime.h>

#include "box_decode_arith.h"
#include "center_decode_arith.h"

#pragma clang fp contract(off)

namespace accv_qd {

constexpr int kMaxK = 1024;     // ACCV_QD_MAX_K
constexpr int kMaxWidth = 9;    // values of the widest written row: the 10-value 3D code loses one (sin, cos -> yaw)

// ---------------------------------------------------------------------------------------------------------------- 3D
// p: the D (8 or 10) widened values of the row; out: D - 1 values.  Returns the row's validity.
__host__ __device__ inline bool row_3d(const accv_cd::Consts& k, int D, const float* p, float x, float& score, float* out)
{
    // the row in the channel order of center_decode_arith.h: (., ., z, d0, d1, d2, sin, cos[, vx, vy])
    float g[accv_cd::kMaxChannels];
    g[0] = p[0], g[1] = p[1], g[2] = p[4], g[3] = p[2], g[4] = p[3], g[5] = p[5], g[6] = p[6], g[7] = p[7];
    g[8] = D == 10 ? p[8] : 0.0f, g[9] = D == 10 ? p[9] : 0.0f;
    score = accv_cd::score_of(k, x);
    accv_cd::box_row(k, g, D, p[0], p[1], out);
    return accv_cd::passes(k, score, p[0], p[1], p[4]);
}

// ---------------------------------------------------------------------------------------------------------------- 2D
struct Consts2 {
    accv_bd::Consts k;      // thr, has_thr, logits, clip, order; no size test, no NMS
    int cxcywh, normalized;
};

// p: the 4 widened values of the row; out: (x1, y1, x2, y2) in the frame's image (or source-image) pixels
__host__ __device__ inline bool row_2d(const Consts2& c, const accv_bd::Frame& fr, const accv_ip::Warp& w, const float* p, float x,
                                       float& score, float* out)
{
    float x1 = p[0], y1 = p[1], x2 = p[2], y2 = p[3];
    if (c.cxcywh) {
        const float hw = 0.5f * p[2], hh = 0.5f * p[3];
        x1 = p[0] - hw, y1 = p[1] - hh, x2 = p[0] + hw, y2 = p[1] + hh;
    }
    if (c.normalized) x1 = x1 * fr.EW, y1 = y1 * fr.EH, x2 = x2 * fr.EW, y2 = y2 * fr.EH;
    if (c.k.clip) {
        x1 = accv_cb::crop_coordinate(x1, fr.EW), y1 = accv_cb::crop_coordinate(y1, fr.EH);
        x2 = accv_cb::crop_coordinate(x2, fr.EW), y2 = accv_cb::crop_coordinate(y2, fr.EH);
    }
    score = accv_bd::score_of(c.k, x);
    const bool valid = accv_bd::passes(c.k, score, x1, y1, x2, y2);
    accv_bd::to_source(w, c.k.order != 0, x1, y1, x2, y2);
    out[0] = x1, out[1] = y1, out[2] = x2, out[3] = y2;
    return valid;
}

}  // namespace accv_qd
