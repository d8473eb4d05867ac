// Lidar depth targets for the cameras of a ragged batch of frames in one launch: the points of a frame projected into each
// camera (through the image matrix the image was warped with, if given), the nearest depth per cell of the downsampled
// feature map and its bin index.  Replaces BEVDepth's per-camera loader pass (map_pointcloud_to_image, depth_transform) and
// the head's get_downsampled_gt_depth.  Per-point arithmetic: depth_targets_arith.h.
//
// Output-stationary.  The h x w map of a (frame, camera) is cut into bands of band_rows whole rows, the grid is
// (bands, C, B), and a workgroup of kThreads lanes
//   1. computes the 12 elements of its matrix, a lane per element, into LDS, and fills its band_rows * w words of LDS with
//      kEmpty; one barrier;
//   2. streams all real points of the frame, kUnroll loads in flight per lane (one wide load per point where D == 4 and the
//      frame's first point is 16-byte aligned: the compiler fetches the 12 bytes that are used; else three 4-byte loads at
//      stride D), projects each and, for a point that counts and
//      lands in the band, takes an LDS atomicMin on the bit pattern of its depth; one barrier;
//   3. writes its band of depth and bins, which is one contiguous range of both outputs, in 16-byte stores where both
//      ranges are 16-byte aligned, else word by word.
// Every output element is written exactly once; nothing is cleared, no output is read, no atomics on global memory, no
// workspace.  The minimum over unsigned keys does not depend on the order of the atomics, so the result is bitwise
// reproducible and the same for every band split.  Every band repeats the projection of the frame's points: the host adds
// bands beyond those needed only while the launch is small (choose_band_rows), see DESIGN.  Streaming loads, about fifty VALU
// instructions a point and a few LDS atomics; far from any bandwidth limit, no MFMA.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "accv_common.h"
#include "accv_numeric.h"
#include "depth_targets_arith.h"

#pragma clang fp contract(off)

namespace {

using namespace accv_dt;
using accv::clamp_count;

constexpr int kThreads = 1024;
constexpr int kUnroll = 4;
constexpr long long kMaxExtent = 1ll << 24;
constexpr long long kMaxGridZ = 65535;

static_assert(kBandCells % 4 == 0 && kBandCells * 4 + 64 <= 64 * 1024, "the band stays within the LDS a workgroup gets without opting in");

struct Args {
    const float* points;            // [B, P, D]
    const void* sizes;              // [B]
    const float* projection;        // [B, C, R, 4]
    const float* transforms;        // [B, C, 2, 3] or null
    float* depth;                   // [B, C, h, w]
    int* bins;                      // [B, C, h, w] or null
    long long B, P;
    int D, C, R, sizes64;
    int h, w, band_rows, bands;
    Consts k;
};

// element e of the 12 of camera (b, c)
__host__ __device__ inline float matrix_entry(const Args& a, long long bc, int e)
{
    return projection_element(a.projection + bc * (a.R * 4), a.transforms ? a.transforms + bc * 6 : nullptr, e >> 2, e & 3);
}

// ------------------------------------------------------------------------------------------------------------- device
__device__ __forceinline__ void take_point(const float* m, const Consts& k, float x, float y, float z, int row0, int rows, int w,
                                           uint32_t* cells)
{
    int cy, cx;
    float d;
    if (!project_point(m, k, x, y, z, cy, cx, d)) return;
    cy -= row0;
    if (cy < 0 || cy >= rows) return;
    atomicMin(&cells[cy * w + cx], depth_key(d));
}

__global__ __launch_bounds__(kThreads) void depth_targets_kernel(const Args a)
{
    __shared__ __attribute__((aligned(16))) uint32_t s_cells[kBandCells];
    __shared__ float s_m[12];
    const int tid = threadIdx.x;
    const long long b = blockIdx.z, bc = b * a.C + blockIdx.y;
    const int row0 = (int)blockIdx.x * a.band_rows;
    const int rows = a.h - row0 < a.band_rows ? a.h - row0 : a.band_rows;
    const int cells = rows * a.w;

    if (tid < 12) s_m[tid] = matrix_entry(a, bc, tid);
    for (int i = tid; i < cells; i += kThreads) s_cells[i] = kEmpty;
    __syncthreads();
    float m[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) m[e] = s_m[e];

    const long long n = clamp_count(a.sizes, b, a.P, a.sizes64);
    const float* pts = a.points + b * a.P * a.D;
    const Consts k = a.k;
    if (a.D == 4 && (reinterpret_cast<uintptr_t>(pts) & 15u) == 0) {
        const float4* p4 = reinterpret_cast<const float4*>(pts);
        for (long long i0 = tid; i0 < n; i0 += (long long)kThreads * kUnroll) {
            float4 q[kUnroll];
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) {
                const long long i = i0 + (long long)u * kThreads;
                q[u] = i < n ? p4[i] : float4{0.0f, 0.0f, 0.0f, 0.0f};
            }
#pragma unroll
            for (int u = 0; u < kUnroll; ++u)
                if (i0 + (long long)u * kThreads < n) take_point(m, k, q[u].x, q[u].y, q[u].z, row0, rows, a.w, s_cells);
        }
    } else {
        const long long D = a.D;
        for (long long i0 = tid; i0 < n; i0 += (long long)kThreads * kUnroll) {
            float q[kUnroll][3];
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) {
                const long long i = i0 + (long long)u * kThreads;
                const bool in = i < n;
                q[u][0] = in ? pts[i * D] : 0.0f;
                q[u][1] = in ? pts[i * D + 1] : 0.0f;
                q[u][2] = in ? pts[i * D + 2] : 0.0f;
            }
#pragma unroll
            for (int u = 0; u < kUnroll; ++u)
                if (i0 + (long long)u * kThreads < n) take_point(m, k, q[u][0], q[u][1], q[u][2], row0, rows, a.w, s_cells);
        }
    }
    __syncthreads();

    // the band is rows [row0, row0 + rows) of map bc: one contiguous range of `cells` elements
    const long long first = (bc * a.h + row0) * a.w;
    float* od = a.depth + first;
    int* ob = a.bins ? a.bins + first : nullptr;
    int done = 0;
    if (((reinterpret_cast<uintptr_t>(od) | reinterpret_cast<uintptr_t>(ob)) & 15u) == 0) {
        const int groups = cells >> 2;
        for (int g = tid; g < groups; g += kThreads) {
            const uint4 key = reinterpret_cast<const uint4*>(s_cells)[g];
            reinterpret_cast<float4*>(od)[g] = float4{key_depth(key.x), key_depth(key.y), key_depth(key.z), key_depth(key.w)};
            if (ob) reinterpret_cast<int4*>(ob)[g] = int4{depth_bin(key.x, k), depth_bin(key.y, k), depth_bin(key.z, k), depth_bin(key.w, k)};
        }
        done = groups << 2;
    }
    for (int i = done + tid; i < cells; i += kThreads) {
        const uint32_t key = s_cells[i];
        od[i] = key_depth(key);
        if (ob) ob[i] = depth_bin(key, k);
    }
}

// --------------------------------------------------------------------------------------------------------------- host
// the serial form: one map at a time, the same per-point and per-cell functions
void host_run(const Args& a)
{
    const long long cells = (long long)a.h * a.w;
    std::vector<uint32_t> map((size_t)cells);
    for (long long b = 0; b < a.B; ++b) {
        const long long n = clamp_count(a.sizes, b, a.P, a.sizes64);
        const float* pts = a.points + b * a.P * a.D;
        for (int c = 0; c < a.C; ++c) {
            const long long bc = b * a.C + c;
            float m[12];
            for (int e = 0; e < 12; ++e) m[e] = matrix_entry(a, bc, e);
            for (long long i = 0; i < cells; ++i) map[(size_t)i] = kEmpty;
            for (long long i = 0; i < n; ++i) {
                int cy, cx;
                float d;
                if (!project_point(m, a.k, pts[i * a.D], pts[i * a.D + 1], pts[i * a.D + 2], cy, cx, d)) continue;
                uint32_t& cell = map[(size_t)cy * a.w + cx];
                const uint32_t key = depth_key(d);
                if (key < cell) cell = key;
            }
            for (long long i = 0; i < cells; ++i) {
                a.depth[bc * cells + i] = key_depth(map[(size_t)i]);
                if (a.bins) a.bins[bc * cells + i] = depth_bin(map[(size_t)i], a.k);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------- checks
inline uintptr_t addr(const void* p) { return reinterpret_cast<uintptr_t>(p); }

// rows per band of the h x w maps of a call with `maps` = B * C of them, w <= kBandCells.  A band must fit (at most
// kBandCells / w rows); beyond that, bands are added while the launch stays at or below kTargetWorkgroups workgroups.
// Every band repeats the projection of all points of the frame and takes over only its share of the LDS atomics, the fill
// and the write: measured on the MI355X (DESIGN, "Lidar depth targets"), that gains 5 to 15 % while the launch is small and
// loses past one workgroup per CU; 64 is the target with the smallest worst case among those measured.
constexpr int kTargetWorkgroups = 64;

inline int choose_band_rows(int h, int w, long long maps)
{
    const int most = kBandCells / w, fit = (h + most - 1) / most;
    const long long want = kTargetWorkgroups / maps;
    const int bands = (int)(want < fit ? fit : (want > h ? h : want));
    return (h + bands - 1) / bands;
}

// ACCV_OK with *empty = 1 when there is nothing to write; every check runs before anything else reads the data
int check_args(const char* who, const accv_depth_targets_params* p, long long B, long long P, long long D, long long C, long long R,
               float* depth, int* bins, Args& a, int* empty)
{
    *empty = 0;
    if (!p) return accv::fail(ACCV_EINVAL, "%s: null params", who);
    if (B < 0 || P < 0) return accv::fail(ACCV_EINVAL, "%s: negative size (B %lld, P %lld)", who, B, P);
    if (D < 3 || D > INT_MAX) return accv::fail(ACCV_EINVAL, "%s: points need 3 <= D < 2^31 channels (x, y, z first), got %lld", who, D);
    if (C < 1 || C > kMaxCameras) return accv::fail(ACCV_EINVAL, "%s: 1..%d cameras supported, got %lld", who, kMaxCameras, C);
    if (R != 3 && R != 4) return accv::fail(ACCV_EINVAL, "%s: projection matrices have 3 or 4 rows, got %lld", who, R);
    if (p->image_h < 1 || p->image_h > kMaxExtent || p->image_w < 1 || p->image_w > kMaxExtent)
        return accv::fail(ACCV_EINVAL, "%s: image extent must be in 1..2^24, got (%lld, %lld)", who, p->image_h, p->image_w);
    if (p->downsample < 1) return accv::fail(ACCV_EINVAL, "%s: downsample must be at least 1, got %d", who, p->downsample);
    const float d_min = (float)p->depth_min, d_max = (float)p->depth_max;
    if (!(d_min > 0.0f && d_min < d_max && std::isfinite(d_max)))
        return accv::fail(ACCV_EINVAL, "%s: depth_range needs 0 < d_min < d_max, both finite in float32, got (%g, %g)", who, p->depth_min,
                          p->depth_max);
    if (p->bin_count < 0 || p->bin_count > kMaxBins)
        return accv::fail(ACCV_EINVAL, "%s: depth_bins count must be in 1..%d, got %d", who, kMaxBins, p->bin_count);
    const float lo = (float)p->bin_lo, step = (float)p->bin_step;
    if (p->bin_count > 0 && !(step > 0.0f && std::isfinite(step) && std::isfinite(lo)))
        return accv::fail(ACCV_EINVAL, "%s: depth_bins needs a finite lo and a finite step > 0 in float32, got (%g, %g)", who, p->bin_lo,
                          p->bin_step);
    const long long s = p->downsample;
    const long long h = (p->image_h + s - 1) / s, w = (p->image_w + s - 1) / s;
    if (w > kBandCells) return accv::fail(ACCV_EINVAL, "%s: map rows of %lld cells, at most DT_BAND_CELLS = %d supported", who, w, kBandCells);
    if (p->band_rows < 0 || (long long)p->band_rows * w > kBandCells)
        return accv::fail(ACCV_EINVAL, "%s: band_rows = %d of %lld cells exceed DT_BAND_CELLS = %d", who, p->band_rows, w, kBandCells);
    if (B == 0) {
        *empty = 1;
        return ACCV_OK;
    }
    if (!depth || (p->bin_count > 0 && !bins)) return accv::fail(ACCV_EINVAL, "%s: null output pointer", who);
    if (!p->projection || !p->sample_sizes || (P > 0 && !p->points)) return accv::fail(ACCV_EINVAL, "%s: null input pointer", who);
    if ((addr(depth) | addr(bins) | addr(p->points) | addr(p->projection) | addr(p->image_transforms)) & 3u)
        return accv::fail(ACCV_EINVAL, "%s: a 4-byte tensor is not aligned to its element size", who);
    if (addr(p->sample_sizes) & (p->sizes_i64 ? 7u : 3u)) return accv::fail(ACCV_EINVAL, "%s: sample_sizes is not aligned to its element size", who);
    if (B > kMaxGridZ) return accv::fail(ACCV_EINVAL, "%s: %lld frames exceed the grid limit of %lld", who, B, kMaxGridZ);
    const long long cap = LLONG_MAX / 64;   // elements of any tensor, in bytes with room to spare
    if (D > cap / B || (P > 0 && D > cap / B / P) || h > cap / (B * C) / w) return accv::fail(ACCV_EINVAL, "%s: sizes overflow", who);
    a.points = p->points, a.sizes = p->sample_sizes, a.projection = p->projection, a.transforms = p->image_transforms;
    a.depth = depth, a.bins = p->bin_count > 0 ? bins : nullptr;
    a.B = B, a.P = P, a.D = (int)D, a.C = (int)C, a.R = (int)R, a.sizes64 = p->sizes_i64 ? 1 : 0;
    a.h = (int)h, a.w = (int)w;
    const int rows = p->band_rows ? p->band_rows : choose_band_rows(a.h, a.w, B * C);
    a.band_rows = rows < a.h ? rows : a.h;
    a.bands = (a.h + a.band_rows - 1) / a.band_rows;
    a.k.d_min = d_min, a.k.d_max = d_max, a.k.Wf = (float)p->image_w, a.k.Hf = (float)p->image_h;
    a.k.lo = p->bin_count > 0 ? lo : 0.0f, a.k.step = p->bin_count > 0 ? step : 1.0f, a.k.count_f = (float)p->bin_count;
    a.k.downsample = p->downsample;
    return ACCV_OK;
}

}  // namespace

extern "C" {

int accv_depth_targets(const accv_depth_targets_params* params, long long B, long long P, long long D, long long C, long long R,
                       float* depth, int* bins, void* stream)
{
    const char* who = "lidar_depth_targets";
    Args a;
    int empty;
    if (int rc = check_args(who, params, B, P, D, C, R, depth, bins, a, &empty)) return rc;
    if (empty) return ACCV_OK;
    const dim3 grid((unsigned)a.bands, (unsigned)a.C, (unsigned)a.B);
    hipLaunchKernelGGL(depth_targets_kernel, grid, dim3(kThreads), 0, static_cast<hipStream_t>(stream), a);
    return accv::check_launch(who);
}

int accv_depth_targets_cpu(const accv_depth_targets_params* params, long long B, long long P, long long D, long long C, long long R,
                           float* depth, int* bins)
{
    const char* who = "lidar_depth_targets (host)";
    Args a;
    int empty;
    if (int rc = check_args(who, params, B, P, D, C, R, depth, bins, a, &empty)) return rc;
    if (empty) return ACCV_OK;
    host_run(a);
    return ACCV_OK;
}

}  // extern "C"
