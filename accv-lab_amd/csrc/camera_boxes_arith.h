// Per-frame arithmetic of the camera-box augmentation (camera_boxes.hip): what the reference's AffineTransformer does to
// its point fields ("centers", "bboxes") and to its projection matrices ("lidar2img", "intr_lidar2img") with the 2 x 3
// matrix that warps the image (processing_steps/affine_transformer.py), and the clamp of its CoordinateCropper
// (crop_coordinates of operators_impl/numba_operators).  The visibility decision in between is visible_boxes_arith.h on the
// warped box.  The GPU kernel and the host entry accv_camera_boxes_host evaluate the same operation sequence from these
// functions.  Everything is float32; contraction into fma is off for everything that includes this header; every operator
// below is ONE IEEE operation, evaluated exactly as parenthesised here.  Decisions are comparisons only.
//
// The matrix of a frame is [[a, b, tx], [c, d, ty]], the forward map from source to output pixels that prepare_images
// takes; its entries are read, never computed, and non-finite ones are computed as written.
//
//   point       x' = ((a*x + b*y) + tx)            y' = ((c*x + d*y) + ty)
//               a box is its two corners (x1, y1) and (x2, y2), each warped as a point: the reference does the same, so a
//               flip leaves x1' > x2' and a rotation gives the box spanned by the two warped corners
//   ordering    (optional) lo = p < q ? p : q, hi = p < q ? q : p per axis, the selection of visible_boxes_arith.h: with a
//               NaN the pair stays as it is
//   matrix      M' = [[a, b, tx], [c, d, ty], [0, 0, 1]] . M for M of 3 or 4 rows; column j:
//               row 0   (a*m0j + b*m1j) + tx*m2j
//               row 1   (c*m0j + d*m1j) + ty*m2j
//               rows 2 and 3 are copied bit for bit
//   crop        v < 0 ? 0 : (v > E ? E : v) with E = W for x and H for y: NaN stays NaN, -0.0 stays -0.0, +-inf go to the
//               borders.  E is exact in float32 (the extents are clamped to [0, 2^24]).
//
// Roundings that feed one output value: this is the n of the tests' bar n * 2^-24 * (largest magnitude among the value's
// float64 intermediates) against a float64 evaluation.  Each rounding adds at most 2^-24 times the magnitude of what it
// rounds, and the errors of the two products add up, so the bound counts every rounding, not only those on the longest
// path (which would be 3 for both).
//   point        4   a*x, b*y, (a*x + b*y), (..) + tx                        (kPointRoundings)
//   matrix row   5   a*m0j, b*m1j, (a*m0j + b*m1j), tx*m2j, (..) + (..)      (kMatrixRoundings)
// The ordering and the crop select among values and round nothing.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#pragma clang fp contract(off)

namespace accv_cb {

constexpr int kPointRoundings = 4;
constexpr int kMatrixRoundings = 5;

// the matrix of a frame
struct Affine {
    float a, b, tx, c, d, ty;
};

__host__ __device__ inline Affine load_affine(const float* p) { return Affine{p[0], p[1], p[2], p[3], p[4], p[5]}; }

__host__ __device__ inline void warp_point(const Affine& t, float x, float y, float& ox, float& oy)
{
    ox = (t.a * x + t.b * y) + t.tx;
    oy = (t.c * x + t.d * y) + t.ty;
}

// (p, q) -> (smaller, larger) by the `<` of visible_boxes_arith.h
__host__ __device__ inline void order_pair(float& p, float& q)
{
    const float lo = p < q ? p : q, hi = p < q ? q : p;
    p = lo, q = hi;
}

__host__ __device__ inline float crop_coordinate(float v, float E) { return v < 0.0f ? 0.0f : (v > E ? E : v); }

// element (row, col) of the new matrix; m points at the matrix, C is its column count
__host__ __device__ inline float matrix_element(const Affine& t, const float* m, int row, int col, int C)
{
    const float m0 = m[col], m1 = m[C + col], m2 = m[2 * C + col];
    if (row == 0) return (t.a * m0 + t.b * m1) + t.tx * m2;
    return (t.c * m0 + t.d * m1) + t.ty * m2;
}

}  // namespace accv_cb
