// Exact top-k of a group of float scores in a defined order, shared by heatmap_peaks.hip and query_decode.hip.
//
// Every element gets a unique 64-bit key: the high word is the order-preserving bit pattern of its score s (-0.0 folded
// onto +0.0 first, so the two zeros tie; every NaN mapped to 0xFFFFFFFF, above +inf, where torch.sort puts it), the low
// word 0xFFFFFFFF - index in group.  Larger key = earlier in the output, and since no two keys are equal the top-k of the
// keys IS torch.sort(s, descending=True, stable=True)[:k]: there are no ties left to resolve.  Key 0 is never a real key
// (the low word of a real one is > 0 because group sizes stay below 2^32 - 1): it marks an empty candidate slot.
//
// radix_select: an MSB-first radix select over 8-bit digits (256-bin LDS histogram, the lanes of a wave that share the
// leading lane's digit add once) finds the k-th largest key of whatever the caller's for_each visits; Cut::take then says
// which keys are among the k.  bitonic_sort_desc orders the winners in LDS.  The LDS slot counter only places the winners
// before the sort; output order comes from the unique keys alone, so results are bitwise reproducible.
#pragma once
#include <hip/hip_runtime.h>

namespace accv_topk {

constexpr int kMaxK = 1024;
constexpr int kBins = 256;
constexpr long long kMaxGroup = 0xfffffffell;   // 2^32 - 2: the low key word of every real key stays above 0

typedef unsigned long long u64;

__host__ __device__ inline unsigned score_bits(float s)
{
    if (s != s) return 0xffffffffu;   // every NaN: one key above +inf (torch.sort puts NaN first), read back as NaN
    unsigned u = __builtin_bit_cast(unsigned, s);
    if (u == 0x80000000u) u = 0u;   // -0.0 ranks with +0.0
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__host__ __device__ inline float score_of(u64 key)
{
    const unsigned h = (unsigned)(key >> 32);
    return __builtin_bit_cast(float, (h & 0x80000000u) ? (h & 0x7fffffffu) : ~h);
}

// the key of the element at `index` of its group
__host__ __device__ inline u64 make_key(float s, unsigned index) { return ((u64)score_bits(s) << 32) | (u64)(0xffffffffu - index); }

// the index in its group a real key was made from
__host__ __device__ inline unsigned index_of(u64 key) { return 0xffffffffu - (unsigned)key; }

// Whether a key is among the selected: all real keys, or those whose top (64 - shift) bits are >= prefix.
struct Cut {
    u64 prefix;
    int shift;   // 64: take every real key
    __device__ bool take(u64 key) const { return key != 0 && (shift >= 64 || (key >> shift) >= prefix); }
};

struct SelectShared {
    unsigned hist[kBins];
    unsigned bin, above, count;
    unsigned slots;   // next free output slot
};

// histogram add; every lane of the wave must call it (the wave's lanes that share the leading lane's digit add once:
// heat maps are mostly suppressed zeros, which would otherwise all hit one bin)
__device__ __forceinline__ void hist_add(unsigned* hist, bool active, unsigned digit)
{
    const u64 act = __ballot(active);
    if (act == 0) return;
    const int leader = __ffsll((long long)act) - 1;
    const unsigned lead_digit = __shfl(digit, leader);
    const bool same = active && digit == lead_digit;
    const u64 same_mask = __ballot(same);
    if (same) {
        if ((int)__lane_id() == leader) atomicAdd(&hist[lead_digit], (unsigned)__popcll(same_mask));
    } else if (active) {
        atomicAdd(&hist[digit], 1u);
    }
}

// MSB-first radix select of the k-th largest real key among those every lane visits with for_each(f).  Returns the cut
// that keeps exactly k keys.  Needs at least k real keys.  Every thread of the block calls it.
template <class ForEach>
__device__ Cut radix_select(ForEach for_each, unsigned k, SelectShared& sh)
{
    const int tid = threadIdx.x;
    u64 prefix = 0;
    unsigned krem = k;
    for (int shift = 56; shift >= 0; shift -= 8) {
        for (int i = tid; i < kBins; i += blockDim.x) sh.hist[i] = 0;
        __syncthreads();
        for_each([&](u64 key) {
            const bool active = key != 0 && (shift == 56 || (key >> (shift + 8)) == prefix);
            hist_add(sh.hist, active, (unsigned)(key >> shift) & 0xffu);
        });
        __syncthreads();
        if (tid < 64) {
            // lane l holds bins 255 - 4l .. 252 - 4l; an inclusive scan from the top bin down finds the k-th key's bin
            unsigned h[4], sum = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) h[j] = sh.hist[255 - 4 * tid - j], sum += h[j];
            unsigned incl = sum;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const unsigned v = __shfl_up(incl, d);
                if (tid >= d) incl += v;
            }
            unsigned before = incl - sum;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (before < krem && krem <= before + h[j]) sh.bin = 255 - 4 * tid - j, sh.above = before, sh.count = h[j];
                before += h[j];
            }
        }
        __syncthreads();
        const unsigned bin = sh.bin, above = sh.above, count = sh.count;
        prefix = (prefix << 8) | bin;
        krem -= above;
        if (count == krem) return Cut{prefix, shift};
        __syncthreads();   // sh.bin is rewritten by the next pass
    }
    return Cut{prefix, 0};   // not reached: keys are unique, so the last digit's bin holds exactly one key
}

// bitonic sort of s[0 .. P), P a power of two, descending, by a workgroup of kThreads lanes; every thread calls it, and the
// caller's barrier after the last write of s is behind it.  Ends with a barrier.
template <int kThreads>
__device__ __forceinline__ void bitonic_sort_desc(u64* s, int P)
{
    const int tid = threadIdx.x;
    for (int size = 2; size <= P; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < P / 2; t += kThreads) {
                const int i = 2 * t - (t & (stride - 1)), j = i + stride;
                const bool desc = (i & size) == 0;
                const u64 a = s[i], b = s[j];
                if ((a < b) == desc) s[i] = b, s[j] = a;
            }
            __syncthreads();
        }
    }
}

}  // namespace accv_topk
