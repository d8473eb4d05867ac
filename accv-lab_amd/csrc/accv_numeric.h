// Numeric building blocks every loss-side operator shares: dtype codes, exact f16 / bf16 conversions, element and 16-byte
// vector access, index / count loads, the fixed-order workgroup sum and the loss denominator.  Host and device see the same
// definitions, so an operator's host twin evaluates what its kernel evaluates.
//
// This header carries NO file-scope `#pragma clang fp contract`: some of its includers compile with contraction on, others
// switch it off for themselves after their includes.  A helper whose result depends on it has the pragma in its own body.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <type_traits>

#include "accv_hip.h"

namespace accv {

// Dtype codes of the loss-side C entry points (an entry that does not take f64 refuses code 3 itself).  The polyline entry
// points use another order (0 f32, 1 f64, 2 f16, 3 bf16) and accv_ragged_accumulate a third; both are ABI and keep their
// own enums (PolyType in polyline.hip, AccType in ragged_ops.hip).
enum DType { kF32 = 0, kF16 = 1, kBF16 = 2, kF64 = 3 };

// arithmetic / accumulation type: float for f32, f16 and bf16 data, double for f64
template <int DT> struct Compute { using type = float; };
template <> struct Compute<kF64> { using type = double; };

// what an element is stored as: float, double, or the 16 bits of an f16 / bf16
template <int DT>
using Stored = std::conditional_t<DT == kF32, float, std::conditional_t<DT == kF64, double, uint16_t>>;

// bytes of one element; 16 / elem_size(dt) elements make a 16-byte vector
__host__ __device__ constexpr int elem_size(int dt) { return dt == kF32 ? 4 : (dt == kF64 ? 8 : 2); }

// ---------------------------------------------------------------------------------------------------------- conversions
// Widening is exact, narrowing rounds to nearest even (torch's casts), NaN stays NaN.  f16 comes in two flavours under one
// name.  The software one (the default) is the same integer code on host and device: operators with a host twin (matched
// focal, matching cost, linear assignment) use it on both sides.  kHwF16 selects the hardware conversion in device code
// (v_cvt_f32_f16 / v_cvt_f16_f32) for device-only kernels; it can differ from the software one in the payload of a
// narrowed NaN only.  On the host both flavours are the software one.
constexpr bool kHwF16 = true;

template <bool HW = false>
__host__ __device__ inline float half_bits_to_float(uint16_t h)
{
#if defined(__HIP_DEVICE_COMPILE__)
    if constexpr (HW) {
        _Float16 v;
        memcpy(&v, &h, 2);
        return (float)v;
    }
#endif
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16;
    const uint32_t e = (h >> 10) & 0x1fu, f = h & 0x3ffu;
    if (e == 0) {   // zero / subnormal: f * 2^-24 is exact in f32
        const float mag = (float)f * 5.9604644775390625e-8f;
        return sign ? -mag : mag;
    }
    uint32_t bits = e == 31 ? (sign | 0x7f800000u | (f << 13)) : (sign | ((e + 112u) << 23) | (f << 13));
    float out;
    memcpy(&out, &bits, 4);
    return out;
}

template <bool HW = false>
__host__ __device__ inline uint16_t float_to_half_bits(float f)
{
#pragma clang fp contract(off)   // the subnormal path is "product, then sum"
#if defined(__HIP_DEVICE_COMPILE__)
    if constexpr (HW) {
        const _Float16 v = (_Float16)f;
        uint16_t out;
        memcpy(&out, &v, 2);
        return out;
    }
#endif
    uint32_t x;
    memcpy(&x, &f, 4);
    const uint32_t sign = (x >> 16) & 0x8000u;
    x &= 0x7fffffffu;
    if (x > 0x7f800000u) return (uint16_t)(sign | 0x7e00u);
    if (x >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);   // 65520 and above round to infinity
    if (x < 0x38800000u) {   // below 2^-14: a subnormal half (or zero): f * 2^24 rounded to an integer by the 2^23 trick
        float a;
        memcpy(&a, &x, 4);
        a = a * 16777216.0f;
        a = a + 8388608.0f;
        uint32_t r;
        memcpy(&r, &a, 4);
        return (uint16_t)(sign | (r - 0x4b000000u));
    }
    const uint32_t odd = (x >> 13) & 1u;
    x += 0xfffu + odd;
    return (uint16_t)(sign | ((x >> 13) - (112u << 10)));
}

__host__ __device__ inline float bf16_bits_to_float(uint16_t b)
{
    const uint32_t bits = (uint32_t)b << 16;
    float out;
    memcpy(&out, &bits, 4);
    return out;
}

// a NaN keeps its sign and high payload bits and gets the quiet bit (| 0x40), so it cannot round to infinity
__host__ __device__ inline uint16_t float_to_bf16_bits(float f)
{
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40u);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

// ------------------------------------------------------------------------------------------------------- element access
// element `off` of a float tensor of dtype DT, widened exactly to the compute type
template <int DT, bool HW = false>
__host__ __device__ inline typename Compute<DT>::type load(const void* p, long long off)
{
    if constexpr (DT == kF32) return static_cast<const float*>(p)[off];
    else if constexpr (DT == kF64) return static_cast<const double*>(p)[off];
    else if constexpr (DT == kF16) return half_bits_to_float<HW>(static_cast<const uint16_t*>(p)[off]);
    else return bf16_bits_to_float(static_cast<const uint16_t*>(p)[off]);
}

// element `off` of a tensor of dtype code dt (f32, f16 or bf16), widened exactly (the software f16 conversion: the same on
// host and device)
__host__ __device__ inline float load_any(const void* p, long long off, int dt)
{
    if (dt == kF32) return load<kF32>(p, off);
    if (dt == kF16) return load<kF16>(p, off);
    return load<kBF16>(p, off);
}

// v narrowed to dtype DT at element `off`
template <int DT, bool HW = false>
__host__ __device__ inline void store(void* p, long long off, typename Compute<DT>::type v)
{
    if constexpr (DT == kF32) static_cast<float*>(p)[off] = v;
    else if constexpr (DT == kF64) static_cast<double*>(p)[off] = v;
    else if constexpr (DT == kF16) static_cast<uint16_t*>(p)[off] = float_to_half_bits<HW>(v);
    else static_cast<uint16_t*>(p)[off] = float_to_bf16_bits(v);
}

// the 16 / elem_size(DT) elements of a 16-byte vector
template <int DT, bool HW = false>
__device__ __forceinline__ void decode(const uint4& v, typename Compute<DT>::type (&x)[16 / elem_size(DT)])
{
    if constexpr (DT == kF32) {
        x[0] = __uint_as_float(v.x), x[1] = __uint_as_float(v.y), x[2] = __uint_as_float(v.z), x[3] = __uint_as_float(v.w);
    } else if constexpr (DT == kF64) {
        x[0] = __hiloint2double((int)v.y, (int)v.x), x[1] = __hiloint2double((int)v.w, (int)v.z);
    } else {
        const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if constexpr (DT == kF16) {
                x[2 * k] = half_bits_to_float<HW>((uint16_t)(w[k] & 0xffffu));
                x[2 * k + 1] = half_bits_to_float<HW>((uint16_t)(w[k] >> 16));
            } else {
                x[2 * k] = __uint_as_float(w[k] << 16);
                x[2 * k + 1] = __uint_as_float(w[k] & 0xffff0000u);
            }
        }
    }
}

template <int DT, bool HW = false>
__device__ __forceinline__ uint4 encode(const typename Compute<DT>::type (&g)[16 / elem_size(DT)])
{
    if constexpr (DT == kF32) {
        return make_uint4(__float_as_uint(g[0]), __float_as_uint(g[1]), __float_as_uint(g[2]), __float_as_uint(g[3]));
    } else if constexpr (DT == kF64) {
        return make_uint4((unsigned)__double2loint(g[0]), (unsigned)__double2hiint(g[0]), (unsigned)__double2loint(g[1]),
                          (unsigned)__double2hiint(g[1]));
    } else {
        unsigned w[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if constexpr (DT == kF16)
                w[k] = (unsigned)float_to_half_bits<HW>(g[2 * k]) | ((unsigned)float_to_half_bits<HW>(g[2 * k + 1]) << 16);
            else
                w[k] = (unsigned)float_to_bf16_bits(g[2 * k]) | ((unsigned)float_to_bf16_bits(g[2 * k + 1]) << 16);
        }
        return make_uint4(w[0], w[1], w[2], w[3]);
    }
}

// --------------------------------------------------------------------------------------------------- indices and counts
// element i of an int32 / int64 index or count tensor
__host__ __device__ inline long long load_index(const void* p, long long i, int is64)
{
    return is64 ? static_cast<const long long*>(p)[i] : (long long)static_cast<const int*>(p)[i];
}

// counts[b] clamped to [0, cap]
__host__ __device__ inline long long clamp_count(const void* counts, long long b, long long cap, int is64)
{
    const long long v = load_index(counts, b, is64);
    return v < 0 ? 0 : (v > cap ? cap : v);
}
// int64 counts that may be absent: without them every frame holds `cap`
__host__ __device__ inline long long clamp_count(const long long* counts, long long b, long long cap)
{
    return counts ? clamp_count(counts, b, cap, 1) : cap;
}

// ---------------------------------------------------------------------------------------------------------- reductions
// The sum of v over a workgroup of kThreads = 256 threads in a FIXED order, which is what makes the losses bitwise
// reproducible: an xor butterfly over the 64 lanes of each wave (offsets 32, 16, ... 1), one LDS slot per wave, then
// (w0 + w1) + (w2 + w3).  The total is returned to thread 0; every other thread gets T(0).  Contains a workgroup barrier:
// all threads call it, and at most once per kernel and type (the LDS slots are per instantiation).
template <class T, int kThreads>
__device__ __forceinline__ T block_sum(T v)
{
    static_assert(kThreads == 256, "the pairwise order is written out for four waves");
    __shared__ T s_part[kThreads / 64];
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = v;
    __syncthreads();
    return threadIdx.x == 0 ? (s_part[0] + s_part[1]) + (s_part[2] + s_part[3]) : T(0);
}
// the same for a (sum, count) pair behind ONE barrier; both totals replace their arguments in thread 0
template <class T, class U, int kThreads>
__device__ __forceinline__ void block_sum(T& a, U& b)
{
    static_assert(kThreads == 256, "the pairwise order is written out for four waves");
    __shared__ T s_sum[kThreads / 64];
    __shared__ U s_cnt[kThreads / 64];
    T acc = a;
    U cnt = b;
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        acc += __shfl_xor(acc, s);
        cnt += __shfl_xor(cnt, s);
    }
    if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6] = acc, s_cnt[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        a = (s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]);
        b = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
    }
}

// The order-preserving rank of a workgroup of kWaves waves of 64 (center_targets.hip, bev_augment.hip): the number of set
// predicates in lower threads of the workgroup (`before`) and in the whole workgroup (`total`); a __ballot + popcount
// inside the wave, the waves' totals in s_cnt[kWaves] (LDS); one barrier.  s_cnt is read between this barrier and the next
// one of the workgroup, so a caller that alternates two rows never writes a row that a slower wave still reads.
template <int kWaves>
__device__ __forceinline__ void block_rank(bool on, int* s_cnt, int lane, int wave, int& before, int& total)
{
    const unsigned long long bits = __ballot(on);
    if (lane == 0) s_cnt[wave] = __popcll(bits);
    __syncthreads();
    before = __popcll(bits & ((1ull << lane) - 1ull));
    total = 0;
#pragma unroll
    for (int v = 0; v < kWaves; ++v) {
        const int c = s_cnt[v];
        total += c;
        if (v < wave) before += c;
    }
}

// The denominator of a mean-reduced loss, in the type of avg_value: the caller's value, the caller's device scalar, or
// max(count, 1) (count.clamp(min=1)).
template <class F>
__host__ __device__ inline F denominator(int avg_mode, F avg_value, const float* avg_dev, unsigned long long count)
{
    if (avg_mode == ACCV_FL_AVG_VALUE) return avg_value;
    if (avg_mode == ACCV_FL_AVG_DEVICE) return (F)*avg_dev;
    return (F)(count > 0 ? count : 1ull);
}

// ---------------------------------------------------------------------------------------------- libm by compute type
__host__ __device__ inline float m_exp(float x) { return expf(x); }
__host__ __device__ inline double m_exp(double x) { return exp(x); }
__host__ __device__ inline float m_log(float x) { return logf(x); }
__host__ __device__ inline double m_log(double x) { return log(x); }
__host__ __device__ inline float m_log1p(float x) { return log1pf(x); }
__host__ __device__ inline double m_log1p(double x) { return log1p(x); }
__host__ __device__ inline float m_pow(float x, float y) { return powf(x, y); }
__host__ __device__ inline double m_pow(double x, double y) { return pow(x, y); }
__host__ __device__ inline float m_abs(float x) { return fabsf(x); }
__host__ __device__ inline double m_abs(double x) { return fabs(x); }

}  // namespace accv
