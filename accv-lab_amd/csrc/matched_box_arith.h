// Per-pair arithmetic of the matched box loss (matched_box.hip) on top of matching_cost_arith.h: the value of a pair and
// its derivative with respect to the raw prediction coordinates.  The GPU kernels and the host entry points
// accv_matched_box_loss_host / _bwd_host evaluate the same operation sequence from these functions; contraction into fma
// is off for everything that includes this header.
//
//   l1    sum_d cw_d |p_d - g_d|, d = 0 .. D-1 in order; derivative cw_d sgn(p_d - g_d), 0 at 0, NaN for NaN
//   iou   1 - iou  = accv_mc::iou_term            giou   1 - giou = accv_mc::giou_term + 1
//
// The derivative of the IoU kinds is the chain rule over the definition, written out in reverse order, with the rules of
// float64 torch autograd where the definition is not smooth:
//   maximum / minimum   the larger / smaller operand takes the gradient, an exact tie splits it evenly; a NaN operand
//                       lets it through (the factor multiplies a NaN anyway)
//   clamp(x, min=0)     (intersection and enclosure sides) passes the gradient where x >= 0, the edge included
//   where(x < eps, eps, x)   (union and enclosure floors) passes no gradient where it fires
// cxcywh predictions: x0 = cx - w / 2, x1 = cx + w / 2 (mmdet's bbox_cxcywh_to_xyxy), so d/dcx = d/dx0 + d/dx1 and
// d/dw = (d/dx1 - d/dx0) / 2, applied here.  A NaN coordinate reaches the union and through it all four components.
#pragma once
#include "matching_cost_arith.h"

#pragma clang fp contract(off)

namespace accv_mb {

using namespace accv_mc;   // and through it accv: dtype codes, Compute<DT>, load / store<DT>, m_*

enum IouKind { kIouNone = 0, kIou = 1, kGiou = 2 };

// d max(a, b) / da and d min(a, b) / da
template <class F> __host__ __device__ inline F max_share(F a, F b) { return a < b ? F(0) : (a == b ? F(0.5) : F(1)); }
template <class F> __host__ __device__ inline F min_share(F a, F b) { return a > b ? F(0) : (a == b ? F(0.5) : F(1)); }

// sgn(x) as torch's abs backward has it
template <class F> __host__ __device__ inline F sign_of(F x) { return x > F(0) ? F(1) : (x < F(0) ? F(-1) : (x == F(0) ? F(0) : x)); }

// one coordinate of the L1 term and its derivative with respect to the prediction
template <class F> __host__ __device__ inline F l1_value(F p, F g, F cw) { return cw * m_abs(p - g); }
template <class F> __host__ __device__ inline F l1_grad(F p, F g, F cw) { return cw * sign_of(p - g); }

// 1 - iou (kIou) or 1 - giou (kGiou) of the raw prediction bp[0..3] against the ground truth as xyxy
template <class F>
__host__ __device__ inline F iou_value(const F* bp, const F* xg, int cxcywh, int kind, F eps)
{
    F xp[4];
    to_xyxy(bp, cxcywh, xp);
    return kind == kGiou ? giou_term(xp, xg, eps) + F(1) : iou_term(xp, xg, eps);
}

// its derivative with respect to bp[0..3]
template <class F>
__host__ __device__ inline void iou_grad(const F* bp, const F* g, int cxcywh, int kind, F eps, F* d)
{
    F p[4];
    to_xyxy(bp, cxcywh, p);
    // forward, the sequence of accv_mc::overlap / giou_term
    const F w = p[2] - p[0], h = p[3] - p[1];
    const F area_p = w * h;
    const F area_g = (g[2] - g[0]) * (g[3] - g[1]);
    const F iw_raw = min_nan(p[2], g[2]) - max_nan(p[0], g[0]);
    const F ih_raw = min_nan(p[3], g[3]) - max_nan(p[1], g[1]);
    const F iw = floor_at(iw_raw, F(0)), ih = floor_at(ih_raw, F(0));
    const F inter = iw * ih;
    const F uni_raw = area_g + area_p - inter;
    const F uni = floor_at(uni_raw, eps);
    const F iou = inter / uni;
    // reverse: loss = 1 - iou [+ (enclose - uni) / enclose]
    F d_uni = iou / uni;          // -d iou / d uni
    F d_inter = F(-1) / uni;      // the direct path
    F d_ew = F(0), d_eh = F(0);
    if (kind == kGiou) {
        const F ew_raw = max_nan(p[2], g[2]) - min_nan(p[0], g[0]);
        const F eh_raw = max_nan(p[3], g[3]) - min_nan(p[1], g[1]);
        const F ew = floor_at(ew_raw, F(0)), eh = floor_at(eh_raw, F(0));
        const F enc_raw = ew * eh;
        const F enclose = floor_at(enc_raw, eps);
        d_uni = d_uni - F(1) / enclose;
        const F d_enc = enc_raw < eps ? F(0) : uni / (enclose * enclose);
        d_ew = ew_raw >= F(0) ? d_enc * eh : F(0);
        d_eh = eh_raw >= F(0) ? d_enc * ew : F(0);
    }
    const F d_area = uni_raw < eps ? F(0) : d_uni;   // d / d uni_raw = d / d area_p = -d / d inter through the union
    d_inter = d_inter - d_area;
    const F d_iw = iw_raw >= F(0) ? d_inter * ih : F(0);
    const F d_ih = ih_raw >= F(0) ? d_inter * iw : F(0);
    F x[4];
    x[0] = -(d_area * h) - d_iw * max_share(p[0], g[0]) - d_ew * min_share(p[0], g[0]);
    x[1] = -(d_area * w) - d_ih * max_share(p[1], g[1]) - d_eh * min_share(p[1], g[1]);
    x[2] = d_area * h + d_iw * min_share(p[2], g[2]) + d_ew * max_share(p[2], g[2]);
    x[3] = d_area * w + d_ih * min_share(p[3], g[3]) + d_eh * max_share(p[3], g[3]);
    if (cxcywh) {
        d[0] = x[0] + x[2], d[1] = x[1] + x[3];
        d[2] = F(0.5) * (x[2] - x[0]), d[3] = F(0.5) * (x[3] - x[1]);
    } else {
        d[0] = x[0], d[1] = x[1], d[2] = x[2], d[3] = x[3];
    }
}

}  // namespace accv_mb
