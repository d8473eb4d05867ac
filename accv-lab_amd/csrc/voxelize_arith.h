// Per-point arithmetic of hard voxelization (voxelize.hip): mmcv's hard_voxelize_forward_cpu, the sequential loop of its
// Voxelization layer (spconv's points_to_voxel is the same rule), restated in float32 so that the GPU kernels and the host
// entry accv_voxelize_cpu evaluate one operation sequence.  Contraction into fma is off for everything that includes this
// header; every operator below is ONE IEEE operation; `/` is one correctly rounded division (accv_ba::div_rn: __fdiv_rn on
// the device, `/` on the host); floor is exact.
//
//   grid        g_k = rint((hi_k - lo_k) / v_k), k = x, y, z, in float32, ties to even: what mmcv's Python wrapper computes with
//               torch.round on float32 tensors.  lo, hi and v are the caller's numbers rounded to float32 once.
//   a point     with an augmentation row (θ, c, s, k, tx, ty, tz) of bev_augment_boxes:
//               (x, y, z) = accv_ba::augment_center(row, x, y, z)                    (bev_augment_arith.h, not restated)
//               t_k = floor((p_k - lo_k) / v_k)
//               in range iff t_k >= 0 && t_k < (float)g_k for all three k: FLOAT compares, so NaN and ±inf fail (mmcv casts
//               to int first, which is undefined for them)
//               c_k = (int)t_k,  key = (c_z * g_y + c_y) * g_x + c_x  < 2^31
//   the loop    per frame, points in slot order: a key without a voxel opens voxel number `count` unless count == max_voxels,
//               in which case the point is SKIPPED AND THE LOOP GOES ON (mmcv's `continue`; older versions stop); a point
//               whose voxel holds fewer than max_points points is stored in the voxel's next row: x, y, z as augmented, the
//               other channels bit for bit.
// The table helpers below are shared by the host loop and the insert kernel: an open-addressing table of a power-of-two
// number of slots, linear probing from mix(key).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "bev_augment_arith.h"

#pragma clang fp contract(off)

namespace accv_vx {

constexpr int kMaxD = 16;
constexpr int kMinD = 3;
constexpr int kMaxT = 128;
constexpr long long kMaxV = 1ll << 20;
constexpr int kNone = -1;   // no key (point out of range), no voxel (refused), an empty slot

// the grid of a call, rounded to float32 once on the host
struct Grid {
    float lo[3], v[3], gf[3];   // x, y, z
    int g[3];
};

// g_k of the grid as a float: rint((hi - lo) / v), ties to even
inline float grid_extent(float lo, float hi, float v) { return nearbyintf((hi - lo) / v); }

// the key of a point, kNone when it is out of range
__host__ __device__ inline int point_key(const Grid& gr, float x, float y, float z)
{
    const float tx = floorf(accv_ba::div_rn(x - gr.lo[0], gr.v[0]));
    const float ty = floorf(accv_ba::div_rn(y - gr.lo[1], gr.v[1]));
    const float tz = floorf(accv_ba::div_rn(z - gr.lo[2], gr.v[2]));
    if (!(tx >= 0.0f && tx < gr.gf[0] && ty >= 0.0f && ty < gr.gf[1] && tz >= 0.0f && tz < gr.gf[2])) return kNone;
    return ((int)tz * gr.g[1] + (int)ty) * gr.g[0] + (int)tx;
}

// x, y, z of a point as the voxels see them: through the frame's row, if there is one
__host__ __device__ inline void place_point(const float* row, float& x, float& y, float& z)
{
    if (!row) return;
    float ox, oy, oz;
    accv_ba::augment_center(accv_ba::load_row(row), x, y, z, ox, oy, oz);
    x = ox, y = oy, z = oz;
}

// (c_z, c_y, c_x) of a key: mmcv's order
__host__ __device__ inline void key_coors(const Grid& gr, int key, int* out)
{
    const int plane = gr.g[0] * gr.g[1];
    const int cz = key / plane, rest = key - cz * plane;
    const int cy = rest / gr.g[0];
    out[0] = cz, out[1] = cy, out[2] = rest - cy * gr.g[0];
}

// where the probe of a key starts in a table of mask + 1 slots (murmur3's finaliser)
__host__ __device__ inline uint32_t first_slot(int key, uint32_t mask)
{
    uint32_t h = (uint32_t)key;
    h ^= h >> 16, h *= 0x85ebca6bu, h ^= h >> 13, h *= 0xc2b2ae35u, h ^= h >> 16;
    return h & mask;
}

}  // namespace accv_vx
