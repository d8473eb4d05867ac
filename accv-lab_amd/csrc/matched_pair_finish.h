// The second launch of a matched-pair loss with two per-frame sums (matched_box.hip, polyline_match.hip): one workgroup,
// a wave per frame, adds the frame's per-workgroup partials in a fixed order, counts the pairs, applies the denominator
// and leaves it on the device for the backward.
#pragma once
#include <hip/hip_runtime.h>

#include "accv_numeric.h"

namespace accv {

constexpr int kFinishThreads = 1024;

// part: [2, B * nqb] f64 (the first sums of every workgroup, then the second ones), nqb workgroups per frame; out is [2, B]
template <class O>
__global__ __launch_bounds__(kFinishThreads) void pair_finish_kernel(const double* __restrict__ part,
                                                                     const long long* __restrict__ counts, long long B,
                                                                     long long nqb, long long K, int avg_mode, double avg_value,
                                                                     const float* __restrict__ avg_dev, O* __restrict__ out,
                                                                     double* __restrict__ out_denom)
{
    __shared__ unsigned long long s_cnt[kFinishThreads / 64];
    __shared__ double s_denom;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long m = 0;
    if (avg_mode == ACCV_FL_AVG_NUM_POS)
        for (long long b = threadIdx.x; b < B; b += kFinishThreads) m += (unsigned long long)clamp_count(counts, b, K, 1);
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) m += __shfl_xor(m, s);
    if (lane == 0) s_cnt[wave] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long total = 0;
        for (int i = 0; i < kFinishThreads / 64; ++i) total += s_cnt[i];
        const double denom = denominator(avg_mode, avg_value, avg_dev, total);
        s_denom = denom;
        *out_denom = denom;
    }
    __syncthreads();
    const double denom = s_denom;
    const long long blocks = B * nqb;
    for (long long b = wave; b < B; b += kFinishThreads / 64) {
        double l1 = 0.0, iou = 0.0;
        for (long long i = lane; i < nqb; i += 64) l1 += part[b * nqb + i], iou += part[blocks + b * nqb + i];
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) l1 += __shfl_xor(l1, s), iou += __shfl_xor(iou, s);
        if (lane == 0) out[b] = (O)(l1 / denom), out[B + b] = (O)(iou / denom);
    }
}

}  // namespace accv
