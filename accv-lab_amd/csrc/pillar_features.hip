// Pillar decoration and the voxel mean: from the voxels of voxelize.hip to the rows a pillar feature net's first linear layer
// reads (mmdet3d's non-legacy PillarFeatureNet.forward up to that layer) and to HardSimpleVFE's per-voxel mean.  The torch
// composition is a sum, a divide, three strided slice assignments into a zeros_like, a norm, a cat, a mask build and a
// multiply: about a dozen launches and several passes over the largest tensor of the lidar branch.  Per-voxel arithmetic and
// the definition: pillar_features_arith.h.
//
// One launch.  A workgroup of kThreads lanes takes G consecutive voxels, G = min(kMaxGroup, kLdsFloats / (T * D)), which is
// one contiguous range of `voxels` and one contiguous range of `out`:
//   stage    the G * T * D floats into LDS, 16 bytes a lane where `voxels` is 16-byte aligned and G * T * D is a multiple of
//            4 (then every workgroup's range starts on a 16-byte boundary), else 4 bytes a lane; the clamped point counts
//            next to them; one barrier;
//   sum      a lane per (voxel, channel): the sequential sum over the voxel's rows from LDS, the division; decoration keeps
//            the mean and the voxel centre of x, y, z in LDS (one barrier), the voxel mean writes its output and is done;
//   write    all lanes, an output element (or four consecutive ones, 16 bytes, where `out` and G * T * F allow) each trip:
//            the channel's value from the staged row, +0.0 in rows from the point count on.
// Every output element is stored exactly once; no workspace, no atomics, no global read of anything but the three inputs,
// no scratch.  Store-bound: F / D times the bytes read are written.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>

#include "accv_common.h"
#include "pillar_features_arith.h"

#pragma clang fp contract(off)

namespace {

using namespace accv_pf;

constexpr int kThreads = 256;
constexpr int kMaxGroup = 64;        // voxels a workgroup takes at most
constexpr int kLdsFloats = 8192;     // LDS budget of the staged rows: 32 KiB
static_assert(kMaxGroup * 3 <= kThreads && kMaxGroup <= kThreads, "a lane per (voxel, axis) and per point count");
static_assert(kLdsFloats >= kMaxT * kMaxD, "the largest voxel fits");

struct Args {
    const float* voxels;      // [M, T, D]
    const int* num_points;    // [M]
    const int* coors;         // [M, cw] or null (voxel mean)
    float* out;               // [M, T, F] or [M, nf]
    float vsize[3], offset[3];   // x, y, z; offset_k = v_k * 0.5f + lo_k
    long long M;
    int T, D, F, nf, cw, G;
    unsigned flags;
};

// voxels a workgroup takes
inline int group_of(long long T, long long D)
{
    const long long fit = kLdsFloats / (T * D);
    return (int)(fit < 1 ? 1 : (fit > kMaxGroup ? kMaxGroup : fit));
}

// ------------------------------------------------------------------------------------------------------------- device
template <bool kMean, bool kVecIn, bool kVecOut>
__global__ __launch_bounds__(kThreads) void pillar_features_kernel(const Args a)
{
    __shared__ __attribute__((aligned(16))) float s_rows[kLdsFloats];
    __shared__ float s_mean[kMaxGroup * 3], s_centre[kMaxGroup * 3];
    __shared__ int s_n[kMaxGroup];
    const int tid = threadIdx.x;
    const long long g0 = (long long)blockIdx.x * a.G;
    const int cnt = (int)(a.M - g0 < a.G ? a.M - g0 : a.G);
    const int TD = a.T * a.D;
    const int floats = cnt * TD;
    const float* src = a.voxels + g0 * TD;
    if (kVecIn) {
        const int n4 = floats >> 2;
        const float4* s4 = reinterpret_cast<const float4*>(src);
        float4* d4 = reinterpret_cast<float4*>(s_rows);
        for (int i = tid; i < n4; i += kThreads) d4[i] = s4[i];
        for (int i = (n4 << 2) + tid; i < floats; i += kThreads) s_rows[i] = src[i];
    } else {
        for (int i = tid; i < floats; i += kThreads) s_rows[i] = src[i];
    }
    if (tid < cnt) s_n[tid] = clamp_points(a.num_points[g0 + tid], a.T);
    __syncthreads();

    const int K = kMean ? a.nf : 3;
    for (int i = tid; i < cnt * K; i += kThreads) {
        const int v = i / K, k = i - v * K;
        const float m = mean_of(s_rows + v * TD + k, a.D, s_n[v]);
        if (kMean) {
            a.out[(g0 + v) * a.nf + k] = m;
        } else {
            s_mean[i] = m;
            s_centre[i] = centre_of(a.coors[(g0 + v) * a.cw + (a.cw - 1 - k)], a.vsize[k], a.offset[k]);
        }
    }
    if (kMean) return;
    __syncthreads();

    const int F = a.F, T = a.T;
    const int total = cnt * T * F;
    float* dst = a.out + g0 * T * F;
    if (kVecOut) {
        const int n4 = total >> 2;
        for (int i = tid; i < n4; i += kThreads) {
            const int e = i << 2;
            int row = e / F, ch = e - row * F;
            int v = row / T, j = row - v * T;
            float o[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                o[u] = element(s_rows + v * TD + j * a.D, s_mean + 3 * v, s_centre + 3 * v, j < s_n[v], ch, a.D, a.flags);
                if (++ch == F) {
                    ch = 0;
                    if (++j == T) j = 0, ++v;
                }
            }
            reinterpret_cast<float4*>(dst)[i] = float4{o[0], o[1], o[2], o[3]};
        }
        for (int e = (n4 << 2) + tid; e < total; e += kThreads) {     // the last workgroup's tail; its v stays below cnt
            const int row = e / F, ch = e - row * F;
            const int v = row / T, j = row - v * T;
            dst[e] = element(s_rows + v * TD + j * a.D, s_mean + 3 * v, s_centre + 3 * v, j < s_n[v], ch, a.D, a.flags);
        }
    } else {
        for (int e = tid; e < total; e += kThreads) {
            const int row = e / F, ch = e - row * F;
            const int v = row / T, j = row - v * T;
            dst[e] = element(s_rows + v * TD + j * a.D, s_mean + 3 * v, s_centre + 3 * v, j < s_n[v], ch, a.D, a.flags);
        }
    }
}

// --------------------------------------------------------------------------------------------------------------- host
void host_features(const Args& a)
{
    const int TD = a.T * a.D;
    for (long long m = 0; m < a.M; ++m) {
        const float* rows = a.voxels + m * TD;
        const int n = clamp_points(a.num_points[m], a.T);
        float mean[3], centre[3];
        for (int k = 0; k < 3; ++k) {
            mean[k] = mean_of(rows + k, a.D, n);
            centre[k] = centre_of(a.coors[m * a.cw + (a.cw - 1 - k)], a.vsize[k], a.offset[k]);
        }
        float* out = a.out + m * a.T * a.F;
        for (int j = 0; j < a.T; ++j) {
            const float* p = rows + j * a.D;
            if (j < n) std::memcpy(out + j * a.F, p, (size_t)a.D * sizeof(float));      // bit for bit, NaN payloads included
            for (int ch = j < n ? a.D : 0; ch < a.F; ++ch) out[j * a.F + ch] = element(p, mean, centre, j < n, ch, a.D, a.flags);
        }
    }
}

void host_mean(const Args& a)
{
    const int TD = a.T * a.D;
    for (long long m = 0; m < a.M; ++m) {
        const int n = clamp_points(a.num_points[m], a.T);
        for (int k = 0; k < a.nf; ++k) a.out[m * a.nf + k] = mean_of(a.voxels + m * TD + k, a.D, n);
    }
}

// ------------------------------------------------------------------------------------------------------------- checks
inline uintptr_t addr(const void* p) { return reinterpret_cast<uintptr_t>(p); }

// ACCV_OK with *empty = 1 when there is nothing to write
int check_sizes(const char* who, long long M, long long T, long long D, int* empty)
{
    *empty = 0;
    if (M < 0) return accv::fail(ACCV_EINVAL, "%s: negative size (M %lld)", who, M);
    if (D < kMinD || D > kMaxD) return accv::fail(ACCV_EINVAL, "%s: voxels need %d <= D <= %d channels (x, y, z first), got %lld", who, kMinD, kMaxD, D);
    if (T < 1 || T > kMaxT) return accv::fail(ACCV_EINVAL, "%s: voxels need 1 <= T <= %d rows, got %lld", who, kMaxT, T);
    if ((M + group_of(T, D) - 1) / group_of(T, D) > accv::kGridLimit)
        return accv::fail(ACCV_EINVAL, "%s: M = %lld voxels exceed the grid limit", who, M);
    if (M == 0) *empty = 1;
    return ACCV_OK;
}

int check_features(const char* who, const accv_pillar_features_params* p, long long M, long long T, long long D, float* out, Args& a, int* empty)
{
    if (!p) return accv::fail(ACCV_EINVAL, "%s: null params", who);
    if (int rc = check_sizes(who, M, T, D, empty)) return rc;
    if (p->coor_width != 3 && p->coor_width != 4) return accv::fail(ACCV_EINVAL, "%s: coor_width must be 3 or 4, got %d", who, p->coor_width);
    if (p->flags & ~(ACCV_PF_CLUSTER | ACCV_PF_CENTER | ACCV_PF_DISTANCE)) return accv::fail(ACCV_EINVAL, "%s: unknown flags %u", who, p->flags);
    for (int k = 0; k < 3; ++k) {
        const float v = (float)p->voxel_size[k], lo = (float)p->range_min[k];
        if (!(v > 0.0f && std::isfinite(v)))
            return accv::fail(ACCV_EINVAL, "%s: voxel_size[%d] must be positive and finite in float32, got %g", who, k, p->voxel_size[k]);
        if (!std::isfinite(lo))
            return accv::fail(ACCV_EINVAL, "%s: point_cloud_range[%d] must be finite in float32, got %g", who, k, p->range_min[k]);
        a.vsize[k] = v, a.offset[k] = centre_offset(v, lo);
    }
    if (*empty) return ACCV_OK;
    if (!p->voxels || !p->num_points || !p->coors || !out) return accv::fail(ACCV_EINVAL, "%s: null pointer", who);
    if ((addr(p->voxels) | addr(p->num_points) | addr(p->coors) | addr(out)) & 3u)
        return accv::fail(ACCV_EINVAL, "%s: a 4-byte tensor is not aligned to its element size", who);
    a.voxels = p->voxels, a.num_points = p->num_points, a.coors = p->coors, a.out = out;
    a.M = M, a.T = (int)T, a.D = (int)D, a.flags = p->flags, a.cw = p->coor_width;
    a.F = feature_count(a.D, a.flags), a.nf = 0, a.G = group_of(T, D);
    return ACCV_OK;
}

int check_mean(const char* who, const float* voxels, const int* num_points, long long M, long long T, long long D, long long nf, float* out,
               Args& a, int* empty)
{
    if (int rc = check_sizes(who, M, T, D, empty)) return rc;
    if (nf < 1 || nf > D) return accv::fail(ACCV_EINVAL, "%s: num_features must be in 1..D = %lld, got %lld", who, D, nf);
    if (*empty) return ACCV_OK;
    if (!voxels || !num_points || !out) return accv::fail(ACCV_EINVAL, "%s: null pointer", who);
    if ((addr(voxels) | addr(num_points) | addr(out)) & 3u) return accv::fail(ACCV_EINVAL, "%s: a 4-byte tensor is not aligned to its element size", who);
    a.voxels = voxels, a.num_points = num_points, a.coors = nullptr, a.out = out;
    a.M = M, a.T = (int)T, a.D = (int)D, a.flags = 0, a.cw = 0, a.F = 0, a.nf = (int)nf, a.G = group_of(T, D);
    for (int k = 0; k < 3; ++k) a.vsize[k] = a.offset[k] = 0.0f;
    return ACCV_OK;
}

}  // namespace

extern "C" {

int accv_pillar_features(const accv_pillar_features_params* params, long long M, long long T, long long D, float* out, void* stream_)
{
    const char* who = "pillar_features";
    Args a;
    int empty;
    if (int rc = check_features(who, params, M, T, D, out, a, &empty)) return rc;
    if (empty) return ACCV_OK;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const dim3 grid((unsigned)((a.M + a.G - 1) / a.G)), block(kThreads);
    const bool vec_in = (addr(a.voxels) & 15u) == 0 && ((long long)a.G * a.T * a.D) % 4 == 0;
    const bool vec_out = (addr(a.out) & 15u) == 0 && ((long long)a.G * a.T * a.F) % 4 == 0;
    if (vec_in && vec_out) hipLaunchKernelGGL((pillar_features_kernel<false, true, true>), grid, block, 0, stream, a);
    else if (vec_in) hipLaunchKernelGGL((pillar_features_kernel<false, true, false>), grid, block, 0, stream, a);
    else if (vec_out) hipLaunchKernelGGL((pillar_features_kernel<false, false, true>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((pillar_features_kernel<false, false, false>), grid, block, 0, stream, a);
    return accv::check_launch(who);
}

int accv_pillar_features_cpu(const accv_pillar_features_params* params, long long M, long long T, long long D, float* out)
{
    const char* who = "pillar_features (host)";
    Args a;
    int empty;
    if (int rc = check_features(who, params, M, T, D, out, a, &empty)) return rc;
    if (!empty) host_features(a);
    return ACCV_OK;
}

int accv_voxel_mean(const float* voxels, const int* num_points, long long M, long long T, long long D, long long num_features, float* out,
                    void* stream_)
{
    const char* who = "voxel_mean";
    Args a;
    int empty;
    if (int rc = check_mean(who, voxels, num_points, M, T, D, num_features, out, a, &empty)) return rc;
    if (empty) return ACCV_OK;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const dim3 grid((unsigned)((a.M + a.G - 1) / a.G)), block(kThreads);
    const bool vec_in = (addr(a.voxels) & 15u) == 0 && ((long long)a.G * a.T * a.D) % 4 == 0;
    if (vec_in) hipLaunchKernelGGL((pillar_features_kernel<true, true, false>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((pillar_features_kernel<true, false, false>), grid, block, 0, stream, a);
    return accv::check_launch(who);
}

int accv_voxel_mean_cpu(const float* voxels, const int* num_points, long long M, long long T, long long D, long long num_features, float* out)
{
    const char* who = "voxel_mean (host)";
    Args a;
    int empty;
    if (int rc = check_mean(who, voxels, num_points, M, T, D, num_features, out, a, &empty)) return rc;
    if (!empty) host_mean(a);
    return ACCV_OK;
}

}  // extern "C"
