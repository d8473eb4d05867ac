// Per-frame arithmetic of the BEV box augmentation (bev_augment.hip): the reference's BEVBBoxesTransformer3D (a global
// rotation about z, then a uniform scaling, then a translation; processing_steps/bev_bboxes_transformer_3d.py) applied to
// box centres, sizes, yaws and velocities and to every matrix that maps to or from the augmented frame, and the centre
// test of PointsInRangeCheck (processing_steps/points_in_range_check.py).  The GPU kernel and the host entry
// accv_bev_augment_host evaluate the same operation sequence from these functions.  Everything is float32; contraction into
// fma is off for everything that includes this header; every operator below is ONE IEEE operation, evaluated exactly as
// parenthesised here; every `/` is one correctly rounded division (div_rn: __fdiv_rn on the device, `/` on the host, as in
// center_targets_arith.h); ceil is exact.  Decisions are comparisons only, so NaN fails all of them.
//
// The parameter row of a frame is (θ, c, s, k, tx, ty, tz): the angle, ITS COSINE AND SINE AS GIVEN (they are read, never
// computed, which is what makes every output bit-equal between the device, the host entry and any float32 restatement),
// the scale and the translation.  A = T . S . R is the augmentation of a point.  P = float32(π), T2 = float32(2π).
//
//   centre      x' = ((c*x - s*y) * k) + tx        y' = ((s*x + c*y) * k) + ty        z' = (z*k) + tz
//   sizes       d' = d * k
//   velocity    ((c*vx - s*vy) * k, (s*vx + c*vy) * k)                                 no translation
//   yaw         v = yaw + θ                                                            the reference's ensure_range
//               if (v < -P)      v = v + ceil((-P - v) / T2) * T2
//               else if (v > P)  v = v - ceil((v - P) / T2) * T2
//               NaN stays NaN, ±inf gives NaN (inf - inf)
//   range       lo_x <= x && x <= hi_x, likewise y and z: both borders inclusive, NaN fails (check_points_in_box); the
//               test reads the raw or the augmented centre.  The borders are the caller's float64 numbers rounded to
//               float32 TOWARD THE INSIDE of the range (lo up, hi down: inward_border below), so the float32 comparison
//               decides exactly what the reference's comparison of the float32 centre with the float64 border decides
//   a row m of a matrix applied to points of the augmented frame (lidar2img, extrinsics, ego_to_world): M . A^-1
//               ik = 1 / k
//               r0 = m0*c - m1*s                   r1 = m0*s + m1*c
//               q0 = r0*ik     q1 = r1*ik          q2 = m2*ik
//               u3 = m3 - ((q0*tx + q1*ty) + q2*tz)
//               the new row is (q0, q1, q2, u3)
//   a column a of a matrix whose results are points of that frame (world_to_ego): A . M
//               (((c*a0 - s*a1) * k) + tx*a3, ((s*a0 + c*a1) * k) + ty*a3, (a2*k) + tz*a3, a3)
//
// These are the reference's three sequential apply_matrix steps written out, with the cosine taken directly where the
// reference has 1 - (1 - cos) from Rodrigues' formula.  k = 0 and non-finite rows are computed as written.
//
// Roundings on the longest chain of each output tensor, the rounded constants c, s and 1/k counted: this is the n of the
// tests' bar n * 2^-24 * (largest magnitude among the tensor's intermediates) against a float64 evaluation.
//   boxes             5   c -> c*x -> (c*x - s*y) -> (..)*k -> (..) + tx          (kBoxRoundings)
//                         (yaw: yaw + θ -> T2 -> ceil(..)*T2 -> v ± (..), 4; what is rounded inside the ceil moves the
//                         result by a whole turn or not at all)
//   point transforms  9   c -> m0*c -> r0 -> [1/k] -> q0 -> q0*tx -> (.. + q1*ty) -> (.. + q2*tz) -> m3 - (..)
//                         (kPointRoundings; 1/k is a rounding of its own on the way to q0)
//   frame transforms  5   c -> c*a0 -> (c*a0 - s*a1) -> (..)*k -> (..) + tx*a3   (kFrameRoundings)
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#pragma clang fp contract(off)

namespace accv_ba {

constexpr int kBoxRoundings = 5;
constexpr int kPointRoundings = 9;
constexpr int kFrameRoundings = 5;

constexpr float kPi = 3.14159274101257324f;      // float32(π)
constexpr float kTwoPi = 6.28318548202514648f;   // float32(2π)

// the parameter row of a frame
struct Row {
    float angle, c, s, k, tx, ty, tz;
};

// the range of a call, rounded to float32 once on the host
struct Range {
    float lo[3], hi[3];
};

// the float32 border that admits the same float32 values as the float64 border v: the nearest float32 on the inside
// (`upper`: at or below v, else at or above).  NaN stays NaN and admits nothing.
inline float inward_border(double v, bool upper)
{
    const float f = (float)v;
    if (upper) return (double)f > v ? nextafterf(f, -INFINITY) : f;
    return (double)f < v ? nextafterf(f, INFINITY) : f;
}

__host__ __device__ inline float div_rn(float a, float b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __fdiv_rn(a, b);
#else
    return a / b;
#endif
}

__host__ __device__ inline Row load_row(const float* p)
{
    return Row{p[0], p[1], p[2], p[3], p[4], p[5], p[6]};
}

__host__ __device__ inline bool in_range(const Range& r, float x, float y, float z)
{
    return r.lo[0] <= x && x <= r.hi[0] && r.lo[1] <= y && y <= r.hi[1] && r.lo[2] <= z && z <= r.hi[2];
}

__host__ __device__ inline void augment_center(const Row& p, float x, float y, float z, float& ox, float& oy, float& oz)
{
    ox = ((p.c * x - p.s * y) * p.k) + p.tx;
    oy = ((p.s * x + p.c * y) * p.k) + p.ty;
    oz = (z * p.k) + p.tz;
}

__host__ __device__ inline float wrap_yaw(float v)
{
    if (v < -kPi) return v + ceilf(div_rn(-kPi - v, kTwoPi)) * kTwoPi;
    if (v > kPi) return v - ceilf(div_rn(v - kPi, kTwoPi)) * kTwoPi;
    return v;
}

// sizes, yaw and velocity of a box (D = 7 or 9) whose augmented centre is (ox, oy, oz): the whole output row
__host__ __device__ inline void augment_box(const Row& p, const float* box, int D, float ox, float oy, float oz, float* out)
{
    out[0] = ox, out[1] = oy, out[2] = oz;
    out[3] = box[3] * p.k, out[4] = box[4] * p.k, out[5] = box[5] * p.k;
    out[6] = wrap_yaw(box[6] + p.angle);
    if (D == 9) {
        const float vx = box[7], vy = box[8];
        out[7] = (p.c * vx - p.s * vy) * p.k;
        out[8] = (p.s * vx + p.c * vy) * p.k;
    }
}

// row m of a matrix applied to points of the augmented frame -> the row of M . A^-1
__host__ __device__ inline void point_transform_row(const Row& p, float ik, float m0, float m1, float m2, float m3, float* out)
{
    const float r0 = m0 * p.c - m1 * p.s;
    const float r1 = m0 * p.s + m1 * p.c;
    const float q0 = r0 * ik, q1 = r1 * ik, q2 = m2 * ik;
    out[0] = q0, out[1] = q1, out[2] = q2;
    out[3] = m3 - ((q0 * p.tx + q1 * p.ty) + q2 * p.tz);
}

// column a of a matrix whose results are points of the augmented frame -> the column of A . M
__host__ __device__ inline void frame_transform_column(const Row& p, float a0, float a1, float a2, float a3, float* out)
{
    out[0] = ((p.c * a0 - p.s * a1) * p.k) + p.tx * a3;
    out[1] = ((p.s * a0 + p.c * a1) * p.k) + p.ty * a3;
    out[2] = (a2 * p.k) + p.tz * a3;
    out[3] = a3;
}

}  // namespace accv_ba
