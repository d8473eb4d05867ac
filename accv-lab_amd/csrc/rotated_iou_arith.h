// Per-pair arithmetic of the rotated BEV IoU (rotated_nms.hip): the intersection over union of two rotated rectangles
// (x, y, dx, dy, yaw) on the ground plane, what mmcv's box_iou_rotated / nms_rotated compute for mmdet3d's nms_bev.  The GPU
// kernels and the host entries accv_rotated_iou_bev_host / accv_rotated_nms_bev_host evaluate the same operation sequence
// from these functions.  Everything is float32; contraction into fma is off for everything that includes this header;
// every operator below is ONE IEEE operation, evaluated exactly as parenthesised here; divisions are __fdiv_rn on the
// device and `/` on the host.  cosf / sinf are the platform's (device and host agree to a few ulp, not bit for bit);
// everything else is bit-equal between the two.
//
// Per box, once (prepare):
//   ok    all five values finite && dx > 0 && dy > 0             a box that is not ok has IoU +0 with every box
//   hx = dx * 0.5   hy = dy * 0.5   area = dx * dy   r = sqrt(hx * hx + hy * hy)   c = cos(yaw)   s = sin(yaw)
// IoU of A against B (iou):
//   0. +0 unless both are ok
//   1. reject   tx = xA - xB, ty = yA - yB, R = rA + rB:  +0 if tx * tx + ty * ty > (R * R) * kRejectSlack.  Exact: boxes
//      whose circumscribed circles are apart do not meet.  kRejectSlack = 1 + 2^-20 is above the rounding of both sides (a
//      dozen operations of 2^-24 each), so the test can only under-reject; what it lets through is clipped to nothing below.
//   2. A in B's frame: centre  cx = tx * cB + ty * sB,  cy = ty * cB - tx * sB;  angle  w = yawA - yawB  with the rounding
//      error of that subtraction recovered exactly (a two-sum) and applied to first order:
//        bv = w - yawA,  av = w - bv,  e = (yawA - av) + ((0 - yawB) - bv)          yawA - yawB == w + e, exactly
//        c0 = cos w,  s0 = sin w;   c = c0 - s0 * e,   s = s0 + c0 * e
//      e is up to half an ulp of |w|: 2.4e-7 rad two turns apart, 3e-5 rad a hundred turns apart, and an error of the
//      angle acts over the box's half length against its width: without e a car a hundred turns ahead of its
//      neighbour is off by 4e-5, a 50 x 0.02 strip one turn ahead by 1e-4.  The correction's own error is e * e / 2.
//      DOMAIN: |yaw| <= 4096 rad (about 650 turns), where |w| <= 8192, |e| <= 4.9e-4 and that term is 1.2e-7; beyond it
//      the value is still a finite number in [0, 1] but no longer within the bar (8e-4 at 100 000 turns).  Equal yaws give
//      w = +0, e = 0, c = 1, s = 0 exactly.
//      ax = hxA * c, ay = hxA * s, bx = hyA * s, by = hyA * c;  corners, counter-clockwise:
//        P0 = ((cx + ax) - bx, (cy + ay) + by)   P1 = ((cx - ax) - bx, (cy - ay) + by)
//        P2 = ((cx - ax) + bx, (cy - ay) - by)   P3 = ((cx + ax) + bx, (cy + ay) - by)
//      In B's frame every coordinate is of the size of the boxes, not of the scene, and B is axis-aligned.
//   3. Sutherland-Hodgman against  x <= hxB,  -x <= hxB,  y <= hyB,  -y <= hyB  in this order.  With p the clipped and o the
//      other coordinate, sp = p or -p:  a vertex is inside iff sp <= h;  walking the edges S -> E in order, an edge whose
//      ends differ gives the vertex  (p, o) = (h or -h exactly,  oS + ((h - spS) / (spE - spS)) * (oE - oS)),  then E
//      follows if it is inside.  At most one vertex is gained per plane: 8 at the end.
//   4. shoelace relative to the first vertex V0, for k = 1 .. m - 2 in order:
//        sum += (xk - x0) * (y(k+1) - y0) - (x(k+1) - x0) * (yk - y0);     inter = 0.5 * sum  (0 when m < 3)
//   5. iou = inter / ((areaA + areaB) - inter);  +0 unless iou > 0 (NaN too);  at most 1.
// Identical boxes: w = 0 and e = 0, the corners are B's own, nothing is cut, inter = areaB = areaA bit for bit: iou = 1.  Boxes that
// share only an edge: every vertex that survives the plane of that edge has the plane's coordinate exactly: inter = 0.
//
// The polygon lives in eight named slots per coordinate.  Every index below is a compile-time constant after unrolling
// (an append to slot m is a select over all slots), so the slots are registers: nothing is indexed at run time, nothing
// goes to scratch.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#pragma clang fp contract(off)

namespace accv_ri {

constexpr int kMaxVertices = 8;
constexpr float kRejectSlack = 1.00000095367431640625f;   // 1 + 2^-20

#define ACCV_RI_INLINE __host__ __device__ __forceinline__

ACCV_RI_INLINE float div_rn(float a, float b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __fdiv_rn(a, b);
#else
    return a / b;
#endif
}

ACCV_RI_INLINE bool finite(float v) { return fabsf(v) <= 3.402823466e+38f; }   // false for NaN and the infinities

// what is computed once per box
struct Box {
    float x, y, hx, hy, yaw, c, s, area, r;
    bool ok;
};

ACCV_RI_INLINE Box prepare(float x, float y, float dx, float dy, float yaw)
{
    Box b;
    b.ok = finite(x) && finite(y) && finite(dx) && finite(dy) && finite(yaw) && dx > 0.0f && dy > 0.0f;
    b.x = x, b.y = y, b.yaw = yaw;
    b.hx = dx * 0.5f, b.hy = dy * 0.5f;
    b.area = dx * dy;
    b.r = sqrtf(b.hx * b.hx + b.hy * b.hy);
    b.c = b.ok ? cosf(yaw) : 1.0f;
    b.s = b.ok ? sinf(yaw) : 0.0f;
    return b;
}

// step 1 for two ok boxes
ACCV_RI_INLINE bool apart(const Box& a, const Box& b)
{
    const float tx = a.x - b.x, ty = a.y - b.y, R = a.r + b.r;
    return tx * tx + ty * ty > (R * R) * kRejectSlack;
}

struct Poly {
    float p[kMaxVertices], o[kMaxVertices];
};

template <int MAXOUT>
ACCV_RI_INLINE void append(float (&qp)[kMaxVertices], float (&qo)[kMaxVertices], int& m, float vp, float vo)
{
#pragma unroll
    for (int k = 0; k < MAXOUT; ++k)
        if (k == m) qp[k] = vp, qo[k] = vo;
    ++m;
}

// step 3 for one plane: the polygon (p, o) of n <= MAXIN vertices against sp <= h into (qp, qo); returns its vertex count
template <int MAXIN, bool NEG>
ACCV_RI_INLINE int clip(const float (&p)[kMaxVertices], const float (&o)[kMaxVertices], int n, float h, float (&qp)[kMaxVertices],
                        float (&qo)[kMaxVertices])
{
    constexpr int MAXOUT = MAXIN + 1;
    int m = 0;
#pragma unroll
    for (int k = 0; k < kMaxVertices; ++k) qp[k] = 0.0f, qo[k] = 0.0f;
#pragma unroll
    for (int i = 0; i < MAXIN; ++i) {
        if (i < n) {
            const bool last = i + 1 == n;
            const float pS = p[i], oS = o[i];
            const float pE = last ? p[0] : p[(i + 1) % kMaxVertices], oE = last ? o[0] : o[(i + 1) % kMaxVertices];
            const float sS = NEG ? -pS : pS, sE = NEG ? -pE : pE;
            const bool inS = sS <= h, inE = sE <= h;
            if (inS != inE) append<MAXOUT>(qp, qo, m, NEG ? -h : h, oS + div_rn(h - sS, sE - sS) * (oE - oS));
            if (inE) append<MAXOUT>(qp, qo, m, pE, oE);
        }
    }
    return m < MAXOUT ? m : MAXOUT;   // a convex polygon gains at most one vertex; what rounding could add is dropped
}

// steps 0 to 5
ACCV_RI_INLINE float iou(const Box& a, const Box& b)
{
    if (!(a.ok && b.ok) || apart(a, b)) return 0.0f;
    const float tx = a.x - b.x, ty = a.y - b.y;
    const float cx = tx * b.c + ty * b.s, cy = ty * b.c - tx * b.s;
    const float w = a.yaw - b.yaw, bv = w - a.yaw, av = w - bv, e = (a.yaw - av) + ((0.0f - b.yaw) - bv);
    const float c0 = cosf(w), s0 = sinf(w), c = c0 - s0 * e, s = s0 + c0 * e;
    const float ax = a.hx * c, ay = a.hx * s, bx = a.hy * s, by = a.hy * c;
    float x0[kMaxVertices], y0[kMaxVertices], x1[kMaxVertices], y1[kMaxVertices];
#pragma unroll
    for (int k = 4; k < kMaxVertices; ++k) x0[k] = 0.0f, y0[k] = 0.0f;
    x0[0] = (cx + ax) - bx, y0[0] = (cy + ay) + by;
    x0[1] = (cx - ax) - bx, y0[1] = (cy - ay) + by;
    x0[2] = (cx - ax) + bx, y0[2] = (cy - ay) - by;
    x0[3] = (cx + ax) + bx, y0[3] = (cy + ay) - by;
    int m = clip<4, false>(x0, y0, 4, b.hx, x1, y1);
    m = clip<5, true>(x1, y1, m, b.hx, x0, y0);
    m = clip<6, false>(y0, x0, m, b.hy, y1, x1);
    m = clip<7, true>(y1, x1, m, b.hy, y0, x0);
    float sum = 0.0f;
#pragma unroll
    for (int k = 1; k + 1 < kMaxVertices; ++k)
        if (k + 1 < m) sum += (x0[k] - x0[0]) * (y0[k + 1] - y0[0]) - (x0[k + 1] - x0[0]) * (y0[k] - y0[0]);
    const float inter = 0.5f * sum;
    const float v = div_rn(inter, (a.area + b.area) - inter);
    return v > 0.0f ? (v < 1.0f ? v : 1.0f) : 0.0f;
}

}  // namespace accv_ri
