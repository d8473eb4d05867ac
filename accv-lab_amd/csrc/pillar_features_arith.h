// Per-voxel arithmetic of pillar decoration and the voxel mean (pillar_features.hip): mmdet3d's non-legacy
// PillarFeatureNet.forward up to its first linear layer and HardSimpleVFE, restated in float32 so that the GPU kernel and the
// host entries accv_pillar_features_cpu / accv_voxel_mean_cpu evaluate one operation sequence.  Contraction into fma is off
// for everything that includes this header; every operator below is ONE IEEE operation; `/` and sqrt are correctly rounded
// (__fdiv_rn on the device and `/` on the host; sqrtf on both).
//
//   n           clamp(num_points, 0, T)
//   s_k         ((p_0k + p_1k) + p_2k) + ... over the rows j < n IN ROW ORDER, k = x, y, z (torch's sum has no defined order;
//               this one is the library's)
//   mean_k      s_k / float(n);  +0.0 and no division for n == 0
//   centre_k    float(c_k) * v_k + (v_k * 0.5f + lo_k), c = (x, y, z) from coors columns (-1, -2, -3); the bracket is
//               evaluated once per call on the host (centre_offset)
//   a row j < n [the D input channels bit for bit | p_jk - mean_k | p_jk - centre_k | sqrt((x * x + y * y) + z * z)]
//   a row j >= n  +0.0 in every channel, whatever the input holds there
// Rows j < n with a NaN or an infinity in x, y or z give NaN in the computed channels; which NaN is the processor's choice.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#pragma clang fp contract(off)

namespace accv_pf {

constexpr int kMinD = 3;
constexpr int kMaxD = 16;
constexpr int kMaxT = 128;
constexpr unsigned kCluster = 1u, kCentre = 2u, kDistance = 4u;

__host__ __device__ inline float div_rn(float a, float b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __fdiv_rn(a, b);
#else
    return a / b;
#endif
}

// sqrtf is the correctly rounded root on both sides (on the device the compiler's default, -fhip-fp32-correctly-rounded-divide-sqrt)
__host__ __device__ inline float sqrt_rn(float a) { return sqrtf(a); }

__host__ __device__ inline int clamp_points(int n, int T) { return n < 0 ? 0 : (n > T ? T : n); }

// channels a decorated row has
__host__ __device__ inline int feature_count(int D, unsigned flags)
{
    return D + ((flags & kCluster) ? 3 : 0) + ((flags & kCentre) ? 3 : 0) + ((flags & kDistance) ? 1 : 0);
}

// the mean over the first n rows of one channel; p points at the channel in row 0, rows are `stride` floats apart
__host__ __device__ inline float mean_of(const float* p, int stride, int n)
{
    if (n <= 0) return 0.0f;
    float s = p[0];
    for (int j = 1; j < n; ++j) s = s + p[j * stride];
    return div_rn(s, (float)n);
}

// v_k * 0.5f + lo_k
inline float centre_offset(float v, float lo) { return v * 0.5f + lo; }

__host__ __device__ inline float centre_of(int c, float v, float offset) { return (float)c * v + offset; }

// channel ch of a decorated row: p is the input row (D channels), mean and centre the voxel's three values each
__host__ __device__ inline float element(const float* p, const float* mean, const float* centre, bool live, int ch, int D, unsigned flags)
{
    if (!live) return 0.0f;
    if (ch < D) return p[ch];
    ch -= D;
    if (flags & kCluster) {
        if (ch < 3) return p[ch] - mean[ch];
        ch -= 3;
    }
    if (flags & kCentre) {
        if (ch < 3) return p[ch] - centre[ch];
        ch -= 3;
    }
    return sqrt_rn((p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]);
}

}  // namespace accv_pf
