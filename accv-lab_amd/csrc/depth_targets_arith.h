// Per-point arithmetic of the lidar depth targets (depth_targets.hip): what BEVDepth's loader does per camera
// (map_pointcloud_to_image / depth_transform: project, mask, scatter into a full-resolution map) and what its head does
// per batch (get_downsampled_gt_depth: minimum over stride x stride blocks, bin index), for one point and one cell.  The GPU
// kernel and the host entry accv_depth_targets_cpu evaluate the same operation sequence from these functions.  Everything is
// float32; contraction into fma is off for everything that includes this header; every operator below is ONE IEEE
// operation, evaluated exactly as parenthesised here.  Decisions are comparisons only.
//
//   matrix      rows 0..2 of the camera's R x 4 projection (R = 3 or 4; row 3 is never read).  With an image matrix
//               [[a, b, tx], [c, d, ty]] rows 0 and 1 are first replaced by matrix_element of camera_boxes_arith.h, the
//               arithmetic camera_augment_boxes writes its projection matrices with; row 2 is taken as it is
//   point       p_k = ((m_k0*x + m_k1*y) + m_k2*z) + m_k3 for k = 0, 1, 2;  d = p_2, u = p_0 / d, v = p_1 / d
//   counts      d >= d_min && d < d_max && u >= 0 && u < W && v >= 0 && v < H: NaN fails, d <= 0 fails (d_min > 0)
//   cell        (int(v) / downsample, int(u) / downsample), integer division; u < W and v < H with W, H <= 2^24 exact in
//               float32 keep int(u) <= W - 1 and int(v) <= H - 1, so the cell lies inside the ceil(H / s) x ceil(W / s) map
//   key         the bit pattern of d: d >= d_min > 0, and positive floats order as their unsigned bit patterns, so the
//               smallest key of a cell is its nearest depth.  kEmpty (all ones, a NaN pattern no counted d has) marks a cell
//               without a point
//   depth       the float of the smallest key, +0 for kEmpty
//   bin         t = (depth - lo) / step;  int(t) if the cell has a point, t >= 0 and t < count, else -1.  count <= 2^15 is
//               exact, and for t >= 0, int(t) < count is t < count: the float compare keeps inf and NaN away from the cast
//
// Roundings that feed d: m_20*x, m_21*y, their sum, m_22*z, the sum, + m_23: six (kDepthRoundings), the n of the tests' bar
// n * 2^-24 * (largest float64 intermediate).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "accv_hip.h"
#include "camera_boxes_arith.h"

#pragma clang fp contract(off)

namespace accv_dt {

constexpr int kMaxCameras = ACCV_DT_MAX_CAMERAS;
constexpr int kBandCells = ACCV_DT_BAND_CELLS;
constexpr int kMaxBins = ACCV_DT_MAX_BINS;
constexpr int kDepthRoundings = 6;
constexpr uint32_t kEmpty = 0xffffffffu;

// what every point of a call is tested against; W, H and count are exact in float32
struct Consts {
    float d_min, d_max, Wf, Hf;
    float lo, step, count_f;
    int downsample;
};

// element (row, col), row < 3, of the matrix the points of a camera go through: proj is the camera's R x 4 matrix, affine
// its 2 x 3 image matrix or null
__host__ __device__ inline float projection_element(const float* proj, const float* affine, int row, int col)
{
    if (affine && row < 2) return accv_cb::matrix_element(accv_cb::load_affine(affine), proj, row, col, 4);
    return proj[row * 4 + col];
}

// the point (x, y, z) through the 3 x 4 matrix m (row-major): true iff it counts, then (cy, cx) is its cell and d its depth
__host__ __device__ inline bool project_point(const float* m, const Consts& k, float x, float y, float z, int& cy, int& cx, float& d)
{
    const float p0 = ((m[0] * x + m[1] * y) + m[2] * z) + m[3];
    const float p1 = ((m[4] * x + m[5] * y) + m[6] * z) + m[7];
    const float p2 = ((m[8] * x + m[9] * y) + m[10] * z) + m[11];
    d = p2;
    const float u = p0 / d, v = p1 / d;
    if (!(d >= k.d_min && d < k.d_max && u >= 0.0f && u < k.Wf && v >= 0.0f && v < k.Hf)) return false;
    cx = (int)u / k.downsample;
    cy = (int)v / k.downsample;
    return true;
}

__host__ __device__ inline uint32_t depth_key(float d)
{
    uint32_t bits;
    memcpy(&bits, &d, 4);
    return bits;
}

__host__ __device__ inline float key_depth(uint32_t key)
{
    float d = 0.0f;
    if (key != kEmpty) memcpy(&d, &key, 4);
    return d;
}

__host__ __device__ inline int depth_bin(uint32_t key, const Consts& k)
{
    const float t = (key_depth(key) - k.lo) / k.step;
    return (key != kEmpty && t >= 0.0f && t < k.count_f) ? (int)t : -1;
}

}  // namespace accv_dt
