// Per-pair arithmetic of the matching-cost op (matching_cost.hip): the GPU kernel and accv_matching_cost_host evaluate
// the same operation sequence from these functions, so every term but the focal one (expf / logf / powf of the device
// library against the host's) gives the same bits on both sides.  hipcc contracts a * b + c into an fma where it likes
// (-ffp-contract=fast is the HIP default); contraction is off for everything that includes this header.
//
// Semantics (the float64 definition is the oracle; F is float, or double for f64 inputs):
//   cls  one_minus_prob  1 - p[q, l]                    neg_prob  -p[q, l]
//        focal (mmdet FocalLossCost), s = sigmoid(x[q, l]), 1 - s from exp(-|x|), never as an f32 subtraction:
//              (-log(s + eps)) * alpha * (1 - s)^gamma - (-log(1 - s + eps)) * (1 - alpha) * s^gamma
//        a label outside [0, C) gives NaN
//   l1   sum_d |bp_d - bg_d|, d = 0 .. D-1 in order
//   iou  1 - inter / max(union, eps): intersection sides clamped at 0, areas not clamped, union = area_g + area_p - inter
//   giou -(iou - (enclose - union) / enclose), union and enclose floored at eps (mmdet bbox_overlaps, mode "giou")
// Maxima, minima, clamps and floors keep a NaN operand (no fmaxf / fminf), so NaN in an evaluated input reaches the pair.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "accv_numeric.h"

#pragma clang fp contract(off)

namespace accv_mc {

using namespace accv;   // dtype codes, Compute<DT>, load<DT> (software f16: the host twin runs the same code), m_*

enum Kind { kOneMinusProb = 0, kNegProb = 1, kFocal = 2 };
constexpr int kMaxD = 16;

// NaN-keeping max / min / floor (torch.maximum / torch.minimum / clamp semantics for NaN)
template <class F> __host__ __device__ inline F max_nan(F a, F b) { return a < b ? b : (b != b ? b : a); }
template <class F> __host__ __device__ inline F min_nan(F a, F b) { return b < a ? b : (b != b ? b : a); }
template <class F> __host__ __device__ inline F floor_at(F x, F lo) { return x < lo ? lo : x; }

template <class F>
struct Params {
    F class_weight, l1_weight, iou_weight, giou_weight;
    F alpha, gamma, focal_eps, iou_eps, filler;
    int kind, cxcywh, D;
    bool cls, l1, iou, giou;   // evaluated terms (weight != 0)
};

template <class F>
__host__ __device__ inline F class_term(const Params<F>& p, F v)
{
    if (p.kind == kOneMinusProb) return F(1) - v;
    if (p.kind == kNegProb) return -v;
    const F e = m_exp(-m_abs(v));          // exp(-|x|) in (0, 1]
    const F r = F(1) / (F(1) + e);
    const bool nonneg = v >= F(0);         // false for NaN: s and 1 - s are NaN through e
    const F s = nonneg ? r : e * r;        // sigmoid(x)
    const F t = nonneg ? e * r : r;        // 1 - sigmoid(x)
    const F pos = -m_log(s + p.focal_eps) * p.alpha * m_pow(t, p.gamma);
    const F neg = -m_log(t + p.focal_eps) * (F(1) - p.alpha) * m_pow(s, p.gamma);
    return pos - neg;
}

// b[0..3] as xyxy (cxcywh converted as mmdet's bbox_cxcywh_to_xyxy)
template <class F>
__host__ __device__ inline void to_xyxy(const F* b, int cxcywh, F* o)
{
    if (cxcywh) {
        const F hw = F(0.5) * b[2], hh = F(0.5) * b[3];
        o[0] = b[0] - hw, o[1] = b[1] - hh, o[2] = b[0] + hw, o[3] = b[1] + hh;
    } else {
        o[0] = b[0], o[1] = b[1], o[2] = b[2], o[3] = b[3];
    }
}

template <class F>
__host__ __device__ inline F l1_term(const F* bp, const F* bg, int D)
{
    F acc = F(0);
#pragma unroll
    for (int d = 0; d < kMaxD; ++d)
        if (d < D) acc = acc + m_abs(bp[d] - bg[d]);
    return acc;
}

// xyxy boxes: intersection area and union (not floored) of prediction p and ground truth g
template <class F>
__host__ __device__ inline void overlap(const F* p, const F* g, F& inter, F& uni)
{
    const F area_p = (p[2] - p[0]) * (p[3] - p[1]);
    const F area_g = (g[2] - g[0]) * (g[3] - g[1]);
    const F iw = floor_at(min_nan(p[2], g[2]) - max_nan(p[0], g[0]), F(0));
    const F ih = floor_at(min_nan(p[3], g[3]) - max_nan(p[1], g[1]), F(0));
    inter = iw * ih;
    uni = area_g + area_p - inter;
}

template <class F>
__host__ __device__ inline F iou_term(const F* p, const F* g, F eps)
{
    F inter, uni;
    overlap(p, g, inter, uni);
    return F(1) - inter / floor_at(uni, eps);
}

template <class F>
__host__ __device__ inline F giou_term(const F* p, const F* g, F eps)
{
    F inter, uni;
    overlap(p, g, inter, uni);
    uni = floor_at(uni, eps);
    const F iou = inter / uni;
    const F ew = floor_at(max_nan(p[2], g[2]) - min_nan(p[0], g[0]), F(0));
    const F eh = floor_at(max_nan(p[3], g[3]) - min_nan(p[1], g[1]), F(0));
    const F enclose = floor_at(ew * eh, eps);
    return -(iou - (enclose - uni) / enclose);
}

// the weighted cost of one pair, terms summed in the order cls, l1, iou, giou.  score: p[q, l_g] (NaN for a label outside
// [0, C)); bp / bg: the raw boxes (D coordinates); xp / xg: the boxes as xyxy (IoU / GIoU only)
template <class F>
__host__ __device__ inline F pair_cost(const Params<F>& p, F score, const F* bp, const F* bg, const F* xp, const F* xg)
{
    F acc = F(0);
    if (p.cls) acc = acc + class_term(p, score) * p.class_weight;
    if (p.l1) acc = acc + l1_term(bp, bg, p.D) * p.l1_weight;
    if (p.iou) acc = acc + iou_term(xp, xg, p.iou_eps) * p.iou_weight;
    if (p.giou) acc = acc + giou_term(xp, xg, p.iou_eps) * p.giou_weight;
    return acc;
}

}  // namespace accv_mc
