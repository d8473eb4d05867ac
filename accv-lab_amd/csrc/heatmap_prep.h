// Small kernels around the heat-map rasteriser: the target-prep front end (targets_from_boxes_kernel,
// targets_from_points_kernel), the flat API's counting sort of the objects by plane (bin_* kernels) and the fill kernels.
// Included once, from draw_heatmap.hip; needs only the HIP runtime.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace {

// ---------------------------------------------------------------- target-prep front end
// centres/boxes (float, source-image pixels) -> integer centre + radius at an output stride; one fused kernel for
// the ~8 element-wise torch ops of the reference helper (packages/draw_heatmap/tests/_test_helpers.py:20-28):
//   r = max(1, int(ceil(min(cx-x0, cy-y0, x1-cx, y1-cy) / stride))),  c = int(c / stride)   (fp32, IEEE division)
__global__ __launch_bounds__(256) void targets_from_boxes_kernel(const float2* __restrict__ centers,
                                                                 const float4* __restrict__ boxes, long long n,
                                                                 float stride, int2* __restrict__ out_centers,
                                                                 int* __restrict__ out_radii)
{
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const float2 c = centers[i];
        const float4 b = boxes[i];
        const float m = fminf(fminf(c.x - b.x, c.y - b.y), fminf(b.z - c.x, b.w - c.y));
        int r = (int)ceilf(__fdiv_rn(m, stride));
        if (r < 1) r = 1;
        out_radii[i] = r;
        out_centers[i] = make_int2((int)__fdiv_rn(c.x, stride), (int)__fdiv_rn(c.y, stride));
    }
}

// sampled polyline points (float, source pixels) -> splat targets of a constant radius at an output stride:
//   c = int(p / stride) (same rule as above); a NaN point (sample of an empty polyline,
//   packages/lane_helpers/ext_impl/polyline/include/polyline_kernels.cuh:216-245) gets radius -1 = never drawn
__global__ __launch_bounds__(256) void targets_from_points_kernel(const float2* __restrict__ points, long long n,
                                                                  float stride, int radius,
                                                                  int2* __restrict__ out_centers,
                                                                  int* __restrict__ out_radii)
{
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const float2 c = points[i];
        const bool bad = (c.x != c.x) || (c.y != c.y);
        out_radii[i] = bad ? -1 : radius;
        out_centers[i] = bad ? make_int2(0, 0) : make_int2((int)__fdiv_rn(c.x, stride), (int)__fdiv_rn(c.y, stride));
    }
}

// ---------------------------------------------------------------- flat API: group objects by plane
__global__ void bin_count_kernel(const int32_t* __restrict__ idx, int n, int planes, int* __restrict__ cnt)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int pl = idx[i];
        if (pl >= 0 && pl < planes) atomicAdd(&cnt[pl], 1);
    }
}

// single workgroup: exclusive scan of cnt[0..planes) into off[0..planes], cnt reset to 0 (reused as cursor)
__global__ __launch_bounds__(1024) void bin_scan_kernel(int* __restrict__ cnt, int* __restrict__ off, int planes)
{
    __shared__ int s_part[1024];
    const int t = threadIdx.x;
    const int per = (planes + 1023) / 1024;
    const int lo = min(t * per, planes), hi = min(lo + per, planes);
    int sum = 0;
    for (int i = lo; i < hi; ++i) sum += cnt[i];
    s_part[t] = sum;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const int v = (t >= d) ? s_part[t - d] : 0;
        __syncthreads();
        s_part[t] += v;
        __syncthreads();
    }
    int run = s_part[t] - sum;  // exclusive prefix of this thread's chunk
    for (int i = lo; i < hi; ++i) {
        const int c = cnt[i];
        off[i] = run;
        cnt[i] = 0;
        run += c;
    }
    if (t == 1023) off[planes] = s_part[1023];
}

// scatters every object into its plane's segment: the splat kernel then reads plane-sorted COPIES (centres, radii)
// with unit stride instead of chasing an index list
__global__ void bin_fill_kernel(const int32_t* __restrict__ idx, int n, int planes, const int* __restrict__ off,
                                int* __restrict__ cursor, const int2* __restrict__ centers,
                                const int32_t* __restrict__ radii, int2* __restrict__ sorted_centers,
                                int32_t* __restrict__ sorted_radii)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int pl = idx[i];
        if (pl >= 0 && pl < planes) {
            const int dst = off[pl] + atomicAdd(&cursor[pl], 1);
            sorted_centers[dst] = centers[i];
            sorted_radii[dst] = radii[i];
        }
    }
}

// count + scan + fill of the three kernels above in ONE single-workgroup launch, for the common small case (a few
// thousand objects, at most kBinSmallPlanes planes): per-plane counters / cursors live in LDS
constexpr int kBinSmallPlanes = 8192, kBinSmallObjects = 1 << 16;
__global__ __launch_bounds__(1024) void bin_small_kernel(const int32_t* __restrict__ idx, int n, int planes,
                                                         const int2* __restrict__ centers,
                                                         const int32_t* __restrict__ radii, int* __restrict__ off,
                                                         int2* __restrict__ sorted_centers,
                                                         int32_t* __restrict__ sorted_radii)
{
    __shared__ int s_cnt[kBinSmallPlanes];
    __shared__ int s_part[1024];
    const int t = threadIdx.x;
    for (int i = t; i < planes; i += 1024) s_cnt[i] = 0;
    __syncthreads();
    for (int i = t; i < n; i += 1024) {
        const int pl = idx[i];
        if (pl >= 0 && pl < planes) atomicAdd(&s_cnt[pl], 1);
    }
    __syncthreads();
    const int per = (planes + 1023) / 1024;
    const int lo = min(t * per, planes), hi = min(lo + per, planes);
    int sum = 0;
    for (int i = lo; i < hi; ++i) sum += s_cnt[i];
    s_part[t] = sum;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const int v = (t >= d) ? s_part[t - d] : 0;
        __syncthreads();
        s_part[t] += v;
        __syncthreads();
    }
    int run = s_part[t] - sum;  // exclusive prefix of this thread's chunk
    for (int i = lo; i < hi; ++i) {
        const int c = s_cnt[i];
        off[i] = run;
        s_cnt[i] = run;  // becomes the plane's write cursor
        run += c;
    }
    if (t == 1023) off[planes] = s_part[1023];
    __syncthreads();
    for (int i = t; i < n; i += 1024) {
        const int pl = idx[i];
        if (pl >= 0 && pl < planes) {
            const int dst = atomicAdd(&s_cnt[pl], 1);
            sorted_centers[dst] = centers[i];
            sorted_radii[dst] = radii[i];
        }
    }
}

// ONE 16-byte store per thread: waves that issue a single store stream at ~7 TB/s, a grid-stride loop (several stores
// per wave) at 4.3-5.9 TB/s on the same boxes (profiles/r01_fill_patterns*.log)
__global__ __launch_bounds__(256) void fill_kernel(float4* __restrict__ dst, size_t n4, float value)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n4) dst[i] = make_float4(value, value, value, value);
}
__global__ void fill_tail_kernel(float* __restrict__ dst, size_t n, float value)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = value;
}

}  // namespace
