// The matched-pair rule of the losses over matched queries (matched_focal.hip, matched_box.hip, polyline_match.hip), once:
//
//   slot j < clamp(counts[b], 0, K) of frame b names query q = pred_ind[b, j] when 0 <= q < Q and 0 <= gt_ind[b, j] < G;
//   a query named twice takes the LOWEST slot; slots at or past counts[b] are never read;
//   the denominator is max(sum_b clamp(counts[b], 0, K), 1) unless the caller gives one.
//
// Device: a workgroup owns a range of queries of one frame (range_of), fills its LDS slot table with kNoSlot itself and
// has scan_pairs enter the slots.  The second launch, pair_finish_kernel, adds each frame's per-workgroup partials in a
// fixed order, counts the pairs, applies the denominator and leaves it on the device for the backward.
// Host: host_pair_table and host_denom are the same rule for the host twins.
// Also here, because the entry points of these files share them: the dtype dispatcher and the argument checks with one
// wording.
#pragma once
#include <hip/hip_runtime.h>

#include <climits>
#include <initializer_list>
#include <new>
#include <type_traits>
#include <vector>

#include "accv_common.h"
#include "accv_numeric.h"

namespace accv {

constexpr int kNoSlot = INT_MAX;        // table entry of a query that no slot names
constexpr int kFinishThreads = 1024;    // workgroup of pair_finish_kernel

// ------------------------------------------------------------------------------------------------------------- device
// the range of a workgroup: frame, first query, number of queries
struct Range {
    long long b, q0;
    int nq;
};
// Workgroup blockIdx.x of a launch with nqb workgroups of qpb queries per frame of Q queries.  This and scan_pairs take
// the fields of the kernel's argument struct by reference: each is then loaded where it is used, as when the code stood in
// the kernel's file, and the compiler schedules it the same way (profiles/matched_pairs_asm_identity.log).
__device__ __forceinline__ Range range_of(const long long& nqb, const int& qpb, const long long& Q)
{
    Range r;
    r.b = blockIdx.x / nqb;
    r.q0 = (blockIdx.x - r.b * nqb) * qpb;
    const long long left = Q - r.q0;
    r.nq = (int)(left < qpb ? left : qpb);
    return r;
}

// Enters the pairs of frame b into s_slot, the table of the queries [q0, q0 + nq): s_slot[i] = the lowest slot that names
// query q0 + i.  The caller has filled the table with kNoSlot and passed a barrier; this ends with one.  Called by all
// kThreads threads of the workgroup.
template <int kThreads>
__device__ __forceinline__ void scan_pairs(const void* const& pind, const void* const& gind, const int& idx64,
                                           const long long* const& counts, long long b, const long long& K, const long long& G,
                                           long long q0, int nq, int* s_slot)
{
    const int tid = threadIdx.x;
    const long long n = clamp_count(counts, b, K, 1);
    for (long long j = tid; j < n; j += kThreads) {
        long long q, g;   // both indices in ONE branch on their dtype, so the two loads are in flight together
        if (idx64) {
            q = static_cast<const long long*>(pind)[b * K + j];
            g = static_cast<const long long*>(gind)[b * K + j];
        } else {
            q = static_cast<const int*>(pind)[b * K + j];
            g = static_cast<const int*>(gind)[b * K + j];
        }
        if (q >= q0 && q < q0 + nq && g >= 0 && g < G) atomicMin(&s_slot[(int)(q - q0)], (int)j);
    }
    __syncthreads();
}

// One workgroup, a wave per frame, for N sums per frame.  part: [N, B * nqb] f64 (the first sums of every workgroup, then
// the second ones), nqb workgroups per frame; out is [N, B].
// Not block_sum: 1024 threads whose 16 wave counts are added one after the other (integers, any order gives the same
// count), and per-frame sums that stay inside one wave.  Both butterflies keep their own order.
template <int N, class O>
__global__ __launch_bounds__(kFinishThreads) void pair_finish_kernel(const double* __restrict__ part,
                                                                     const long long* __restrict__ counts, long long B,
                                                                     long long nqb, long long K, int avg_mode, double avg_value,
                                                                     const float* __restrict__ avg_dev, O* __restrict__ out,
                                                                     double* __restrict__ out_denom)
{
    static_assert(N == 1 || N == 2, "one or two sums per frame");
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
        double first = 0.0, second = 0.0;   // at N == 1 the second sum and all that hangs on it is dead code
        for (long long i = lane; i < nqb; i += 64) {
            first += part[b * nqb + i];
            if (N == 2) second += part[blocks + b * nqb + i];
        }
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) {
            first += __shfl_xor(first, s);
            if (N == 2) second += __shfl_xor(second, s);
        }
        if (lane == 0) {
            out[b] = (O)(first / denom);
            if (N == 2) out[B + b] = (O)(second / denom);
        }
    }
}

// --------------------------------------------------------------------------------------------------------------- host
// the table of a whole frame: tab[q] = the slot of the pair of query q, or kNoSlot
inline void host_pair_table(const void* pind, const void* gind, int idx64, const long long* counts, long long b, long long K,
                            long long Q, long long G, std::vector<int>& tab)
{
    tab.assign((size_t)Q, kNoSlot);
    const long long n = clamp_count(counts, b, K, 1);
    for (long long j = 0; j < n; ++j) {
        const long long q = load_index(pind, b * K + j, idx64), g = load_index(gind, b * K + j, idx64);
        if (q >= 0 && q < Q && g >= 0 && g < G && tab[(size_t)q] == kNoSlot) tab[(size_t)q] = (int)j;
    }
}

// the number of pairs of the batch as the denominator, or the caller's
inline double host_denom(const long long* counts, long long B, long long K, int avg_mode, double avg_value,
                         const float* avg_ptr)
{
    unsigned long long m = 0;
    if (avg_mode == ACCV_FL_AVG_NUM_POS)
        for (long long b = 0; b < B; ++b) m += (unsigned long long)clamp_count(counts, b, K, 1);
    return denominator(avg_mode, avg_value, avg_ptr, m);
}

// ----------------------------------------------------------------------------------------------------------- dispatch
// fn(std::integral_constant<int, DT>) for the dtype code, which the caller has checked: `[&](auto dt) { run<dt()>(...); }`
template <class Fn>
inline void dispatch_dtype(int dtype, Fn&& fn)
{
    switch (dtype) {
        case kF32: fn(std::integral_constant<int, kF32>{}); break;
        case kF16: fn(std::integral_constant<int, kF16>{}); break;
        case kBF16: fn(std::integral_constant<int, kBF16>{}); break;
        default: fn(std::integral_constant<int, kF64>{}); break;
    }
}

// the same for a host entry, whose tables come from the heap
template <class Fn>
inline int dispatch_host(const char* who, int dtype, Fn&& fn)
{
    try {
        dispatch_dtype(dtype, fn);
    } catch (const std::bad_alloc&) {
        return fail(ACCV_ERUNTIME, "%s: out of host memory", who);
    }
    return ACCV_OK;
}

// -------------------------------------------------------------------------------------------------------------- checks
// The checks that the three entry-point families share, in the four groups in which every one of them runs them.  What an
// operator checks of its own stands between the groups in its file: which error is reported first for an input that is
// wrong in several ways is behaviour, and one function called first would change it.
// 1. the parameter struct, the sizes, the dtype code and the flags
inline int check_pair_sizes(const char* who, const void* params, std::initializer_list<long long> sizes, int dtype,
                            unsigned flags, unsigned known_flags)
{
    if (!params) return fail(ACCV_EINVAL, "%s: null params", who);
    for (long long v : sizes)
        if (v < 0) return fail(ACCV_EINVAL, "%s: negative size", who);
    if (dtype < kF32 || dtype > kF64) return fail(ACCV_EINVAL, "%s: unknown dtype code %d", who, dtype);
    if (flags & ~known_flags) return fail(ACCV_EINVAL, "%s: unknown flags 0x%x", who, flags);
    return ACCV_OK;
}
// 2. the avg-factor mode of a forward and the slot count; `limited` names what the message says is limited ("K")
inline int check_pair_mode(const char* who, bool forward, int avg_mode, long long K, long long other, const char* limited)
{
    if (forward && (avg_mode < ACCV_FL_AVG_NUM_POS || avg_mode > ACCV_FL_AVG_DEVICE))
        return fail(ACCV_EINVAL, "%s: unknown avg_factor mode %d", who, avg_mode);
    if (K > INT_MAX || other > INT_MAX) return fail(ACCV_EINVAL, "%s: %s limited to 2^31 - 1", who, limited);
    return ACCV_OK;
}
// 3. after the empty case has returned: counts, with the operand that the file reports in the same message (`what` is
// "logits / counts", or "counts" with `operand` true), and the index pointers
inline int check_pair_pointers(const char* who, bool operand, const char* what, const long long* counts, const void* pind,
                               const void* gind, long long K)
{
    if (!operand || !counts) return fail(ACCV_EINVAL, "%s: null %s pointer", who, what);
    if (K > 0 && (!pind || !gind)) return fail(ACCV_EINVAL, "%s: null index pointer", who);
    return ACCV_OK;
}
// 4. the device scalar of a forward and the launch: B x nqb workgroups
inline int check_pair_launch(const char* who, bool forward, int avg_mode, const float* avg_dev, long long B, long long nqb)
{
    if (forward && avg_mode == ACCV_FL_AVG_DEVICE && !avg_dev) return fail(ACCV_EINVAL, "%s: null avg_factor pointer", who);
    if (nqb > kGridLimit / B) return fail(ACCV_EINVAL, "%s: %lld x %lld workgroups exceed the grid limit", who, B, nqb);
    return ACCV_OK;
}

}  // namespace accv
