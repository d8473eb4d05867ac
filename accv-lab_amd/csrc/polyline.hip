// lane_helpers — batched polyline arc-length interpolation and lengths for gfx950.
//
// Replaces packages/lane_helpers/ext_impl/polyline/include/polyline_kernels.cuh:390-455 (four kernels) and the host
// launch logic of src/polyline.cu:59-129; edge semantics follow include/polyline_common.cuh:58-163:
//   * accum[i] = distance from the first point to point i; query d (x total length when `relative`);
//   * d before the first point -> first point, d beyond the last -> last point;
//   * otherwise the segment [i, i+1] with accum[i] <= d is interpolated linearly; a segment shorter than
//     epsilon(accumulation type) returns its lower point;
//   * a polyline with zero points yields NaN for every query; lengths: 0 points -> NaN, 1 point -> 0.
// Design (not a translation): ONE workgroup of 256 threads per polyline; segment lengths are written to LDS by
// contiguous per-thread chunks, the 256 chunk totals are scanned by one 64-lane wave with __shfl_up (the reference
// hard-codes 32-lane shuffles, polyline_kernels.cuh:26-35,58-70), then every thread binary-searches its queries in
// LDS.  Accumulation is fp32 for f32/f16/bf16 storage and fp64 for f64 (the reference GPU path accumulates in the
// storage dtype, polyline_common.cuh:56-58).  Polylines longer than the LDS budget use a caller-provided global
// scratch row instead (same code path, pointer swap).
#include <hip/hip_runtime.h>

#include <climits>

#include <cmath>
#include <limits>
#include <thread>
#include <vector>

#include <algorithm>
#include <cstdint>
#include <limits>

#include "accv_common.h"
#include "accv_numeric.h"
#include "polyline_arith.h"

namespace {

constexpr int kThreads = 256;
constexpr int kLdsBudgetBytes = 48 * 1024;
constexpr int kWidePoints = 2048;     // polylines of at least this many points take 1024-thread workgroups
constexpr int kSpreadGroups = 512;    // launches of at most this many single-pass workgroups give each thread one query

// the dtype codes of the polyline entry points: ABI, and not the order of accv::DType
enum PolyType { kPF32 = 0, kPF64 = 1, kPF16 = 2, kPBF16 = 3 };

template <int TY>
struct Storage;
template <>
struct Storage<kPF32> {
    using T = float;
    using Acc = float;
    static __device__ __forceinline__ Acc load(const T* p) { return *p; }
    static __device__ __forceinline__ void store(T* p, Acc v) { *p = v; }
    static __device__ __forceinline__ void copy(T* d, const T* s) { *d = *s; }
};
template <>
struct Storage<kPF64> {
    using T = double;
    using Acc = double;
    static __device__ __forceinline__ Acc load(const T* p) { return *p; }
    static __device__ __forceinline__ void store(T* p, Acc v) { *p = v; }
    static __device__ __forceinline__ void copy(T* d, const T* s) { *d = *s; }
};
template <>
struct Storage<kPF16> {
    using T = uint16_t;
    using Acc = float;
    static __device__ __forceinline__ Acc load(const T* p) { return (float)(*reinterpret_cast<const _Float16*>(p)); }
    static __device__ __forceinline__ void store(T* p, Acc v)
    {
        _Float16 h = (_Float16)v;
        *p = *reinterpret_cast<uint16_t*>(&h);
    }
    static __device__ __forceinline__ void copy(T* d, const T* s) { *d = *s; }
};
template <>
struct Storage<kPBF16> {
    using T = uint16_t;
    using Acc = float;
    static __device__ __forceinline__ Acc load(const T* p) { return accv::bf16_bits_to_float(*p); }
    static __device__ __forceinline__ void store(T* p, Acc v) { *p = accv::float_to_bf16_bits(v); }
    static __device__ __forceinline__ void copy(T* d, const T* s) { *d = *s; }
};

struct PolyParams {
    const void* points;     // [B, P, D]
    const void* distances;  // [B, Q] or null (lengths only)
    const void* point_counts;  // null = all P valid
    const void* dist_counts;   // null = all Q valid
    void* out_points;       // [B, Q, D] or null
    void* out_lengths;      // [B] or null
    void* scratch;          // [B, P] accumulation-type elements, used when P does not fit LDS
    float* out_boxes;       // optional (f32, D == 2): [B, ceil(Q/64), 4] bounding box of every 64 consecutive samples
    long long batch;
    int P, Q, D;
    int counts_i64, relative, use_scratch;
    int q_chunk;            // queries per workgroup: blockIdx.y walks the chunks of one polyline (multiple of kThreads)
};

// accum[i] = distance from the first point to point i (accum[0] = 0), for the n points of one polyline, by the whole
// workgroup: segment lengths by contiguous per-thread chunks, the THREADS chunk totals scanned by wave 0.  Shared by the
// sampler and its backward, which has to land on the same segment for every query (bit-identical arithmetic).
// s_part: THREADS accumulation-type elements of LDS.  Ends with a workgroup barrier.
template <int TY, int THREADS, int DC>
__device__ __forceinline__ void arc_prefix(const typename Storage<TY>::T* pts, int n, int D, typename Storage<TY>::Acc* accum,
                                           typename Storage<TY>::Acc* s_part, bool use_scratch)
{
    constexpr int kPerLane = THREADS / 64;   // chunk totals per lane in the scan by wave 0
    using S = Storage<TY>;
    using Acc = typename S::Acc;
    // ---- segment lengths, chunked: thread t owns segments [lo, hi), writes the chunk-local inclusive prefix
    const int t = threadIdx.x;
    const int n_seg = n - 1;
    const int per = (n_seg + THREADS - 1) / THREADS;
    const int lo = min(t * per, n_seg), hi = min(lo + per, n_seg);
    // (lengths first, with consecutive threads on consecutive segments — coalesced reads of the points; a thread walking its
    // own chunk of the points made every wave load touch 64 different cache lines: 5000 points took 15 us)
    // four segments per thread and trip, their loads issued together: the loop is a chain of memory round trips otherwise
    // (20 trips of ~0.5 us for 5000 points)
    constexpr int kBatch = 4;
    for (int s0 = t; s0 < n_seg; s0 += kBatch * THREADS) {
        Acc sq[kBatch];
#pragma unroll
        for (int u = 0; u < kBatch; ++u) {
            const int s = min(s0 + u * THREADS, n_seg - 1);      // clamped: loads stay in range, surplus results are dropped
            Acc acc2 = 0;
            for (int d = 0; d < D; ++d) {
                const Acc diff = S::load(pts + (size_t)s * D + d) - S::load(pts + (size_t)(s + 1) * D + d);
                if constexpr (TY == kPF32)
                    acc2 = accv_poly::seg_length2_step(acc2, diff);   // (pinned: the fused lane raster repeats it, polyline_arith.h)
                else
                    acc2 += diff * diff;
            }
            sq[u] = acc2;
        }
#pragma unroll
        for (int u = 0; u < kBatch; ++u) {
            const int s = s0 + u * THREADS;
            if (s < n_seg) accum[s + 1] = sqrt(sq[u]);
        }
    }
    if (use_scratch) __threadfence_block();
    __syncthreads();
    Acc run = 0;
    for (int s = lo; s < hi; ++s) {     // same summation order as before: chunk-local prefix, then the chunk offsets
        run += accum[s + 1];
        accum[s + 1] = run;
    }
    if (t == 0) accum[0] = 0;
    s_part[t] = run;
    __syncthreads();
    // ---- exclusive scan of the THREADS chunk totals by wave 0 (kPerLane per lane + 64-lane shuffle scan)
    if (t < 64) {
        Acc v[kPerLane];
        Acc lane_total = 0;
#pragma unroll
        for (int u = 0; u < kPerLane; ++u) {
            v[u] = s_part[kPerLane * t + u];
            lane_total += v[u];
        }
        Acc incl = lane_total;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const Acc up = __shfl_up(incl, off, 64);
            if (t >= off) incl += up;
        }
        Acc run2 = incl - lane_total;
#pragma unroll
        for (int u = 0; u < kPerLane; ++u) {
            s_part[kPerLane * t + u] = run2;
            run2 += v[u];
        }
    }
    __syncthreads();
    const Acc base = s_part[t];
    if (base != 0)
        for (int s = lo; s < hi; ++s) accum[s + 1] += base;
    if (use_scratch) __threadfence_block();
    __syncthreads();
}

// THREADS = workgroup size: 256, or 1024 for long polylines (the scan over the points is the serial part of a workgroup)
// DC = number of coordinates per point when it is 2 or 3 (compile-time), 0 = p.D at run time.  With a run-time D every loop
// over the coordinates is a real loop with its loads and a wait inside: a segment's length cost D dependent round trips to
// memory, and the four segments a thread takes per trip cost 4 D of them one after the other (5000 2-D points on 1024 threads:
// 16 round trips in front of the scan; ISA of round 2's kernel) — with DC the loops unroll and the loads of a trip are in flight
// together, which is what the four-segments-per-trip layout was written for
template <int TY, int THREADS, int DC>
__global__ __launch_bounds__(THREADS) void polyline_kernel(const PolyParams p)
{
    const int D = DC > 0 ? DC : p.D;
    using S = Storage<TY>;
    using T = typename S::T;
    using Acc = typename S::Acc;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    __shared__ Acc s_part[THREADS];

    const long long b = blockIdx.x;
    const int t = threadIdx.x;
    int n = p.P, q = p.Q;
    if (p.point_counts) n = (int)max(0ll, min((long long)p.P, accv::load_index(p.point_counts, b, p.counts_i64)));
    if (p.dist_counts) q = (int)max(0ll, min((long long)p.Q, accv::load_index(p.dist_counts, b, p.counts_i64)));
    const T* pts = static_cast<const T*>(p.points) + (size_t)b * p.P * D;
    T* out = p.out_points ? static_cast<T*>(p.out_points) + (size_t)b * p.Q * D : nullptr;
    const Acc nan = std::numeric_limits<Acc>::quiet_NaN();

    // this workgroup's share of the queries: many queries of few polylines are spread over several workgroups (each repeats
    // the prefix scan, which is cheap next to thousands of binary searches by one workgroup while most of the chip idles)
    const int q_begin = (int)blockIdx.y * p.q_chunk;
    const int q_stop = min(q, q_begin + p.q_chunk), q_cap = min(p.Q, q_begin + p.q_chunk);
    const bool first_chunk = blockIdx.y == 0;

    if (n == 0) {  // undefined polyline: NaN everywhere (polyline_kernels.cuh:216-225)
        if (out)
            for (int i = q_begin * D + t; i < q_stop * D; i += THREADS) S::store(out + i, nan);
        if (p.out_lengths && t == 0 && first_chunk) S::store(static_cast<T*>(p.out_lengths) + b, nan);
        if (p.out_boxes) {
            const int groups = (p.Q + 63) / 64;
            const float inf = __builtin_inff();
            for (int g = (q_begin >> 6) + t; g < min(groups, (q_cap + 63) >> 6); g += THREADS)
                reinterpret_cast<float4*>(p.out_boxes)[b * groups + g] = make_float4(inf, inf, -inf, -inf);
        }
        return;
    }

    Acc* accum = p.use_scratch ? static_cast<Acc*>(p.scratch) + (size_t)b * p.P : reinterpret_cast<Acc*>(lds_raw);
    // the thread's first query distance does not depend on the scan: requested here, ahead of the four barriers, instead of as a
    // round trip of its own behind them
    const T* dist = static_cast<const T*>(p.distances) + (size_t)b * p.Q;
    Acc first_d = 0;
    if (out && q_begin + t < q_stop) first_d = S::load(dist + q_begin + t);

    arc_prefix<TY, THREADS, DC>(pts, n, D, accum, s_part, p.use_scratch);

    const Acc total = accum[n - 1];
    if (p.out_lengths && t == 0 && first_chunk) S::store(static_cast<T*>(p.out_lengths) + b, total);
    if (!out) return;

    // ---- queries
    const Acc eps = std::numeric_limits<Acc>::epsilon();
    // (whole waves walk the loop together: when group boxes are wanted, the 64 lanes of a wave hold 64 consecutive samples
    // and reduce their bounding box with shuffles)
    const int q_span = p.out_boxes ? q_begin + ((q_cap - q_begin + THREADS - 1) / THREADS) * THREADS : q_stop;
    const int groups = (p.Q + 63) / 64;
    for (int i = q_begin + t; i < q_span; i += THREADS) {
        float bx = __builtin_nanf(""), by = bx;  // sample coordinates for the group box (D == 2, f32 instantiation)
        if (i < q_stop) {
            Acc d = i == q_begin + t ? first_d : S::load(dist + i);
            if (p.relative) {
                if constexpr (TY == kPF32) d = accv_poly::scale_query(d, total);
                else d *= total;
            }
            T* res = out + (size_t)i * D;
            // last index whose accumulated distance is <= d (polyline_common.cuh:89-116)
            int idx;
            if (accum[0] > d) {
                idx = -1;
            } else if (accum[n - 1] < d) {
                idx = n - 1;
            } else {
                int mn = 0, mx = n - 1;
                while (mx - mn > 1) {
                    const int c = (mx + mn) >> 1;
                    const Acc v = accum[c];
                    if (v < d) mn = c;
                    else if (v > d) mx = c;
                    else mn = mx = c;
                }
                idx = mn;
            }
            if constexpr (DC > 0) {
                // every coordinate is READ before the first one is written: as far as the compiler knows the output may alias the
                // points, so a write between two reads made every coordinate a round trip of its own
                const bool inside = idx >= 0 && idx < n - 1;
                const int ia = inside ? idx : (idx == -1 ? 0 : n - 1);
                const T* a = pts + (size_t)ia * D;
                const T* c = inside ? a + D : a;
                T ra[DC], rc[DC];
#pragma unroll
                for (int k = 0; k < DC; ++k) {
                    ra[k] = a[k];
                    rc[k] = c[k];
                }
                Acc d0 = 0, d1 = 0;
                if (inside) {
                    d0 = accum[idx];
                    d1 = accum[idx + 1];
                }
                const Acc len = d1 - d0;
                if (inside && len >= eps) {
                    Acc w0, w1;
                    if constexpr (TY == kPF32) {
                        accv_poly::lerp_weights(d, d0, d1, len, w0, w1);
                    } else {
                        w1 = (d - d0) / len;
                        w0 = (d1 - d) / len;
                    }
#pragma unroll
                    for (int k = 0; k < DC; ++k) {
                        if constexpr (TY == kPF32) {
                            ra[k] = accv_poly::lerp_coord(ra[k], w0, rc[k], w1);
                            res[k] = ra[k];
                        } else {
                            S::store(res + k, S::load(&ra[k]) * w0 + S::load(&rc[k]) * w1);
                        }
                    }
                } else {   // before the first / beyond the last point, or a segment shorter than epsilon: its lower point
#pragma unroll
                    for (int k = 0; k < DC; ++k) S::copy(res + k, &ra[k]);
                }
                if constexpr (TY == kPF32 && DC == 2) {   // what this thread wrote (group boxes: f32, 2-D only)
                    bx = ra[0];
                    by = ra[1];
                }
            } else {
            if (idx >= 0 && idx < n - 1) {
                const Acc d0 = accum[idx], d1 = accum[idx + 1], len = d1 - d0;
                const T* a = pts + (size_t)idx * D;
                const T* c = a + D;
                if (len >= eps) {
                    if constexpr (TY == kPF32) {
                        float w0, w1;
                        accv_poly::lerp_weights(d, d0, d1, len, w0, w1);
                        for (int k = 0; k < D; ++k) res[k] = accv_poly::lerp_coord(a[k], w0, c[k], w1);
                    } else {
                        const Acc w1 = (d - d0) / len, w0 = (d1 - d) / len;
                        for (int k = 0; k < D; ++k) S::store(res + k, S::load(a + k) * w0 + S::load(c + k) * w1);
                    }
                } else {
                    for (int k = 0; k < D; ++k) S::copy(res + k, a + k);
                }
            } else if (idx == -1) {
                for (int k = 0; k < D; ++k) S::copy(res + k, pts + k);
            } else {
                for (int k = 0; k < D; ++k) S::copy(res + k, pts + (size_t)(n - 1) * D + k);
            }
            }
        }
        if (p.out_boxes) {
            const float inf = __builtin_inff();
            const bool ok = bx == bx && by == by;
            float x0 = ok ? bx : inf, y0 = ok ? by : inf, x1 = ok ? bx : -inf, y1 = ok ? by : -inf;
#pragma unroll
            for (int sft = 32; sft >= 1; sft >>= 1) {
                x0 = fminf(x0, __shfl_xor(x0, sft));
                y0 = fminf(y0, __shfl_xor(y0, sft));
                x1 = fmaxf(x1, __shfl_xor(x1, sft));
                y1 = fmaxf(y1, __shfl_xor(y1, sft));
            }
            const int g = i >> 6;
            if ((t & 63) == 0 && g < groups) reinterpret_cast<float4*>(p.out_boxes)[b * groups + g] = make_float4(x0, y0, x1, y1);
        }
    }
}

inline size_t acc_size(int ty) { return ty == kPF64 ? 8 : 4; }

}  // namespace

extern "C" {

size_t accv_polyline_scratch_bytes(long long batch, int max_points, int dtype)
{
    if (batch <= 0 || max_points <= 0) return 0;
    const size_t need = (size_t)max_points * acc_size(dtype);
    return need <= (size_t)kLdsBudgetBytes ? 0 : need * (size_t)batch;
}

int accv_polyline_sample_boxes(const void* points, const void* distances, const void* point_counts, const void* dist_counts,
                               void* out_points, void* out_lengths, float* out_group_boxes, long long batch, int max_points,
                               int max_distances, int num_dims, int dtype, int counts_i64, int relative, void* scratch,
                               size_t scratch_bytes, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (out_group_boxes && (dtype != kPF32 || num_dims != 2 || !out_points))
        return accv::fail(ACCV_EINVAL, "polyline: group boxes need float32 samples of 2-D points");
    if (out_group_boxes && (reinterpret_cast<uintptr_t>(out_group_boxes) & 15u))
        return accv::fail(ACCV_EINVAL, "polyline: group boxes need 16-byte alignment");
    if (batch < 0 || max_points < 0 || max_distances < 0 || num_dims < 0)
        return accv::fail(ACCV_EINVAL, "polyline: negative extent");
    if (dtype < kPF32 || dtype > kPBF16) return accv::fail(ACCV_EINVAL, "polyline: unsupported dtype code %d", dtype);
    if (batch == 0) return ACCV_OK;
    if (!out_points && !out_lengths) return ACCV_OK;
    if (out_points && (max_distances == 0 || num_dims == 0) && !out_lengths) return ACCV_OK;
    if (max_points > 0 && num_dims > 0 && !points) return accv::fail(ACCV_EINVAL, "polyline: null points");
    if (out_points && max_distances > 0 && !distances) return accv::fail(ACCV_EINVAL, "polyline: null distances");
    PolyParams p{};
    p.points = points;
    p.distances = distances;
    p.point_counts = point_counts;
    p.dist_counts = dist_counts;
    p.out_points = (max_distances > 0 && num_dims > 0) ? out_points : nullptr;
    p.out_lengths = out_lengths;
    p.out_boxes = out_group_boxes;
    p.batch = batch;
    p.P = max_points;
    p.Q = max_distances;
    p.D = num_dims;
    p.counts_i64 = counts_i64;
    p.relative = relative;
    const size_t need = accv_polyline_scratch_bytes(batch, max_points, dtype);
    size_t lds = (size_t)std::max(1, max_points) * acc_size(dtype);
    if (need > 0) {
        if (!scratch || scratch_bytes < need)
            return accv::fail(ACCV_EWORKSPACE, "polyline: %d points per polyline need %zu bytes of scratch", max_points, need);
        p.scratch = scratch;
        p.use_scratch = 1;
        lds = 16;
    }
    if (!p.out_points && !p.out_lengths) return ACCV_OK;
    // queries per workgroup: everything, unless few polylines carry thousands of queries each — then the queries of a polyline
    // are cut into chunks (multiples of the workgroup size, so that groups of 64 samples never straddle a chunk), as many as
    // keep the launch at <= ~4096 workgroups (batch 64, 5000 x 5000: 50 us with one workgroup per polyline; profiles/r02_bench_published.jsonl)
    // long polylines take 1024-thread workgroups: the scan over the points is the serial part of a workgroup (5000 points:
    // 20 segments per thread with 256 threads, 5 with 1024)
    const bool wide = max_points >= kWidePoints;
    const long long threads = wide ? 1024 : kThreads;
    long long chunks = 1;
    // (every chunk repeats the scan over max_points, so a chunk should hold at least ~max_points / 4 queries)
    long long min_chunk = std::max<long long>(threads, ((max_points / 4 + threads - 1) / threads) * threads);
    // few polylines: the chip is idle anyway, so every thread takes ONE query and the queries of a polyline spread over as
    // many workgroups as that needs (each repeats the scan) — a second query per thread is a second serial pass of loads,
    // binary search and interpolation (batch 1, 2000 x 2000: 9.1 -> 7.7 us, 5000 x 5000: 12.3 -> 10.4 us;
    // profiles/r03_tails_probe_sampler_launch_shapes.log)
    if (batch * ((max_distances + threads - 1) / threads) <= kSpreadGroups) min_chunk = threads;
    if (p.out_points && !p.use_scratch && max_distances >= 2 * min_chunk && batch < 2048)
        chunks = std::max<long long>(1, std::min<long long>((max_distances + min_chunk - 1) / min_chunk, 4096 / batch));
    const long long per_chunk = (max_distances + chunks - 1) / chunks;
    p.q_chunk = (int)std::min<long long>(((per_chunk + threads - 1) / threads) * threads, (long long)INT_MAX - threads);
    if (p.q_chunk < threads) p.q_chunk = (int)threads;
    chunks = std::max<long long>(1, ((long long)max_distances + p.q_chunk - 1) / p.q_chunk);
    const dim3 grid((unsigned)batch, (unsigned)chunks), block((unsigned)threads);
#define ACCV_LAUNCH_POLY_D(TYV, DCV)                                                                        \
    do {                                                                                                    \
        if (wide)                                                                                           \
            hipLaunchKernelGGL((polyline_kernel<TYV, 1024, DCV>), grid, block, lds, stream, p);             \
        else                                                                                                \
            hipLaunchKernelGGL((polyline_kernel<TYV, kThreads, DCV>), grid, block, lds, stream, p);         \
    } while (0)
#define ACCV_LAUNCH_POLY(TYV)                                                                               \
    do {                                                                                                    \
        if (num_dims == 2)                                                                                  \
            ACCV_LAUNCH_POLY_D(TYV, 2);                                                                     \
        else if (num_dims == 3)                                                                             \
            ACCV_LAUNCH_POLY_D(TYV, 3);                                                                     \
        else                                                                                                \
            ACCV_LAUNCH_POLY_D(TYV, 0);                                                                     \
    } while (0)
    switch (dtype) {
        case kPF32: ACCV_LAUNCH_POLY(kPF32); break;
        case kPF64: ACCV_LAUNCH_POLY(kPF64); break;
        case kPF16: ACCV_LAUNCH_POLY(kPF16); break;
        default: ACCV_LAUNCH_POLY(kPBF16); break;
    }
#undef ACCV_LAUNCH_POLY
#undef ACCV_LAUNCH_POLY_D
    return accv::check_launch("polyline");
}

int accv_polyline_sample(const void* points, const void* distances, const void* point_counts, const void* dist_counts,
                         void* out_points, void* out_lengths, long long batch, int max_points, int max_distances,
                         int num_dims, int dtype, int counts_i64, int relative, void* scratch, size_t scratch_bytes,
                         void* stream)
{
    return accv_polyline_sample_boxes(points, distances, point_counts, dist_counts, out_points, out_lengths, nullptr, batch,
                                      max_points, max_distances, num_dims, dtype, counts_i64, relative, scratch,
                                      scratch_bytes, stream);
}
}

// ---------------------------------------------------------------- backward (an extension: the reference has none)
// Gradient of polyline_kernel's samples and lengths w.r.t. the points and the distances, for the branch every query took in
// the forward (l_i = |p_{i+1} - p_i|, C_i = sum_{k<i} l_k, T = C_{n-1}, g = incoming gradient of one sample):
//   inside segment i (len >= eps): out = p_i + w1 (p_{i+1} - p_i), w1 = (d - C_i) / l_i; with e_i = (p_{i+1} - p_i) / l_i and
//     s = g . e_i: p_i += (1 - w1) g, p_{i+1} += w1 g, lambda_i -= w1 s, lambda_k -= s for k < i, lambda_k += r s for every
//     k (relative, d = r T), d(distance) = s (absolute) or s T (relative);
//   a copy of one point (before the start, beyond the end, a segment shorter than epsilon, one point): that point += g;
//   lengths: lambda_k += g_b for every segment;
// then every segment with l_k >= eps adds lambda_k e_k to p_{k+1} and -lambda_k e_k to p_k (lambda_k = d loss / d l_k).
// One workgroup per polyline and chunk of its queries (the forward's q_chunk): it repeats the prefix scan (arc_prefix, so the
// binary search lands where the forward's did) and accumulates per-point vectors and per-segment scalars with LDS float
// atomics.  The scalars are ONE array b[] with lambda_k = sum_{j > k} b[j]: a query on segment i adds -(1 - w1) s to b[i]
// and -w1 s to b[i+1], the relative and lengths terms go to b[n-1].  One suffix scan (double) turns b into lambda, and each
// point takes lambda_{k-1} e_{k-1} - lambda_k e_k in double before its one rounding: on straight stretches the two nearly
// cancel, and lambda grows with the number of queries behind a segment.  The workgroup then writes every element of its
// rows of grad_points once (zeros behind the point count) — or, when the queries of a polyline are spread over several
// workgroups, its partial row into a slab that a second launch sums in chunk order.  Accumulators too large for LDS live in
// a private region of the caller's workspace (same code, global atomics).  LDS / global float atomics make the gradients
// depend on arrival order in the last bits.
namespace {

constexpr int kGradLdsBudgetBytes = 64 * 1024;   // dynamic + static LDS of one backward workgroup

struct GradParams {
    const void* points;         // [B, P, D]
    const void* distances;      // [B, Q] or null
    const void* point_counts;   // null = all P valid
    const void* dist_counts;    // null = all Q valid
    const void* grad_out;       // [B, Q, D] or null
    const void* grad_lengths;   // [B] or null
    void* grad_points;          // [B, P, D] or null
    void* grad_distances;       // [B, Q] or null
    void* acc_ws;               // use_ws: [B * chunks] regions of acc_stride accumulation-type elements
    void* slab;                 // chunks > 1: [chunks, B, P, D] partial grad_points, accumulation type
    long long batch;
    long long acc_stride;       // elements per accumulator region: accum[P] | point vectors [P * D] | segment scalars b[P]
    int P, Q, D;
    int counts_i64, relative, use_ws, q_chunk, chunks;
};

// last index whose accumulated distance is <= d, -1 before the start, n - 1 at / beyond the end (polyline_kernel's search)
template <typename Acc>
__device__ __forceinline__ int find_segment(const Acc* accum, int n, Acc d)
{
    if (accum[0] > d) return -1;
    if (accum[n - 1] < d) return n - 1;
    int mn = 0, mx = n - 1;
    while (mx - mn > 1) {
        const int c = (mx + mn) >> 1;
        const Acc v = accum[c];
        if (v < d) mn = c;
        else if (v > d) mx = c;
        else mn = mx = c;
    }
    return mn;
}

// WS: accumulators in the workspace (p.use_ws) instead of LDS
template <int TY, int THREADS, int DC, bool WS>
__global__ __launch_bounds__(THREADS) void polyline_grad_kernel(const GradParams p)
{
    const int D = DC > 0 ? DC : p.D;
    constexpr int kPerLane = THREADS / 64;
    using S = Storage<TY>;
    using T = typename S::T;
    using Acc = typename S::Acc;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    __shared__ double s_sum[THREADS];   // the forward's scan (as Acc), then the suffix scan of the segment scalars

    const long long b = blockIdx.x;
    const int c = (int)blockIdx.y;
    const int t = threadIdx.x;
    int n = p.P, q = p.Q;
    if (p.point_counts) n = (int)max(0ll, min((long long)p.P, accv::load_index(p.point_counts, b, p.counts_i64)));
    if (p.dist_counts) q = (int)max(0ll, min((long long)p.Q, accv::load_index(p.dist_counts, b, p.counts_i64)));
    const T* pts = static_cast<const T*>(p.points) + (size_t)b * p.P * D;
    const size_t row = (size_t)p.P * D;
    T* gpts = p.grad_points && p.chunks == 1 ? static_cast<T*>(p.grad_points) + (size_t)b * row : nullptr;
    Acc* gslab = p.grad_points && p.chunks > 1 ? static_cast<Acc*>(p.slab) + ((size_t)c * p.batch + b) * row : nullptr;
    const bool want_points = p.grad_points != nullptr;
    T* gdist = p.grad_distances ? static_cast<T*>(p.grad_distances) + (size_t)b * p.Q : nullptr;

    const int q_begin = c * p.q_chunk;
    const int q_cap = min(p.Q, q_begin + p.q_chunk);
    // queries that carry a gradient: the valid ones of a non-empty polyline, when there is an incoming gradient
    const int q_live = (p.grad_out && n > 0) ? max(q_begin, min(q, q_begin + p.q_chunk)) : q_begin;
    if (gdist)
        for (int i = q_live + t; i < q_cap; i += THREADS) S::store(gdist + i, Acc(0));
    if (n == 0) {   // undefined polyline (NaN samples): zero gradient
        for (size_t e = t; e < row; e += THREADS) {
            if (gpts) S::store(gpts + e, Acc(0));
            else if (gslab) gslab[e] = 0;
        }
        return;
    }
    if (!want_points && q_live == q_begin) return;

    Acc* const lds = reinterpret_cast<Acc*>(lds_raw);
    Acc* const base = WS ? static_cast<Acc*>(p.acc_ws) + ((size_t)b * p.chunks + c) * p.acc_stride : lds;
    Acc* const accum = base;
    const size_t o_gp = (size_t)p.P, o_b = (size_t)p.P * (D + 1);
    auto add = [&](size_t off, Acc v) { atomicAdd(base + off, v); };   // ds_add / global_atomic_add (WS)
    if (want_points) {
        for (size_t e = t; e < (size_t)n * D; e += THREADS) base[o_gp + e] = 0;
        for (int e = t; e < n; e += THREADS) base[o_b + e] = 0;
    }
    arc_prefix<TY, THREADS, DC>(pts, n, D, accum, reinterpret_cast<Acc*>(s_sum), WS);   // ends with a barrier
    const Acc total = accum[n - 1];
    const Acc eps = std::numeric_limits<Acc>::epsilon();

    // ---- queries: the forward's branch, its exact derivative
    const T* gout = p.grad_out ? static_cast<const T*>(p.grad_out) + (size_t)b * p.Q * D : nullptr;
    const T* dist = static_cast<const T*>(p.distances) + (size_t)b * p.Q;
    double r_sum = 0;   // relative: sum of r s over this thread's queries (-> b[n-1])
    for (int i = q_begin + t; i < q_live; i += THREADS) {
        const T* gq = gout + (size_t)i * D;
        const Acc r = S::load(dist + i);
        Acc d = r;
        if (p.relative) {
            if constexpr (TY == kPF32) d = accv_poly::scale_query(d, total);
            else d *= total;
        }
        const int idx = find_segment(accum, n, d);
        const bool inside = idx >= 0 && idx < n - 1;
        Acc d0 = 0, d1 = 0;
        if (inside) {
            d0 = accum[idx];
            d1 = accum[idx + 1];
        }
        const Acc len = d1 - d0;
        Acc gd = 0;
        if (inside && len >= eps) {
            Acc w0, w1;
            if constexpr (TY == kPF32) {
                accv_poly::lerp_weights(d, d0, d1, len, w0, w1);
            } else {
                w1 = (d - d0) / len;
                w0 = (d1 - d) / len;
            }
            const T* a = pts + (size_t)idx * D;
            Acc l2 = 0;
            for (int k = 0; k < D; ++k) {
                const Acc diff = S::load(a + k) - S::load(a + D + k);
                if constexpr (TY == kPF32) l2 = accv_poly::seg_length2_step(l2, diff);
                else l2 += diff * diff;
            }
            const Acc inv = Acc(1) / sqrt(l2);   // > 0: len >= eps
            Acc sdot = 0;
            for (int k = 0; k < D; ++k) {
                const Acc gk = S::load(gq + k);
                sdot += gk * ((S::load(a + D + k) - S::load(a + k)) * inv);
                if (want_points) {
                    add(o_gp + (size_t)idx * D + k, w0 * gk);   // w0: what the forward weighted p_i with (= 1 - w1)
                    add(o_gp + (size_t)(idx + 1) * D + k, w1 * gk);
                }
            }
            if (want_points) {
                add(o_b + idx, -w0 * sdot);
                add(o_b + idx + 1, -w1 * sdot);
            }
            if (p.relative) {
                r_sum += (double)r * (double)sdot;
                gd = sdot * total;
            } else {
                gd = sdot;
            }
        } else if (want_points) {
            const int j = inside ? idx : (idx < 0 ? 0 : n - 1);
            for (int k = 0; k < D; ++k) add(o_gp + (size_t)j * D + k, S::load(gq + k));
        }
        if (gdist) S::store(gdist + i, gd);
    }
    if (!want_points) return;
    if (n >= 2) {
        if (p.relative && q_live > q_begin) {
            double v = r_sum;
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
            if ((t & 63) == 0 && v != 0) add(o_b + n - 1, (Acc)v);
        }
        if (p.grad_lengths && c == 0 && t == 0) add(o_b + n - 1, S::load(static_cast<const T*>(p.grad_lengths) + b));
    }
    if (WS) __threadfence_block();
    __syncthreads();

    // ---- lambda_k = sum_{j > k} b[j]: thread t owns segments [lo, hi) and the points lo + 1 .. hi (and point 0)
    const int n_seg = n - 1;
    const int per = (n_seg + THREADS - 1) / THREADS;
    const int lo = min(t * per, n_seg), hi = min(lo + per, n_seg);
    double tot = 0;
    for (int j = lo + 1; j <= hi; ++j) tot += (double)base[o_b + j];
    s_sum[t] = tot;
    __syncthreads();
    if (t < 64) {   // exclusive suffix scan of the chunk totals: entry t <- sum over t' > t
        double v[kPerLane];
        double lane_total = 0;
#pragma unroll
        for (int u = 0; u < kPerLane; ++u) {
            v[u] = s_sum[THREADS - 1 - (kPerLane * t + u)];
            lane_total += v[u];
        }
        double incl = lane_total;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const double up = __shfl_up(incl, off, 64);
            if (t >= off) incl += up;
        }
        double run = incl - lane_total;
#pragma unroll
        for (int u = 0; u < kPerLane; ++u) {
            s_sum[THREADS - 1 - (kPerLane * t + u)] = run;
            run += v[u];
        }
    }
    __syncthreads();
    // 1 / l_k in double, 0 for segments shorter than epsilon (they pass no gradient: the zero subgradient of the norm at 0)
    auto inv_len = [&](int k) {
        double l2 = 0;
        for (int e = 0; e < D; ++e) {
            const double diff = (double)S::load(pts + (size_t)(k + 1) * D + e) - (double)S::load(pts + (size_t)k * D + e);
            l2 += diff * diff;
        }
        const double l = sqrt(l2);
        return l >= (double)eps ? 1.0 / l : 0.0;
    };
    auto dir = [&](int k, int e, double inv) {   // (inv == 0 for k >= n - 1: the indices are clamped all the same)
        const int k0 = min(k, n - 2), k1 = k0 + 1;
        return inv == 0.0 ? 0.0 : ((double)S::load(pts + (size_t)k1 * D + e) - (double)S::load(pts + (size_t)k0 * D + e)) * inv;
    };
    double lam_next = s_sum[t];                     // lambda_hi
    double inv_next = hi < n_seg ? inv_len(hi) : 0.0;
    for (int k = hi - 1; k >= lo; --k) {
        const double lam = lam_next + (double)base[o_b + k + 1];
        const double inv = inv_len(k);
        for (int e = 0; e < D; ++e) {
            Acc* g = base + o_gp + (size_t)(k + 1) * D + e;
            *g = (Acc)((double)*g + lam * dir(k, e, inv) - lam_next * dir(k + 1, e, inv_next));
        }
        lam_next = lam;
        inv_next = inv;
    }
    if (t == 0 && n_seg > 0)   // point 0: -lambda_0 e_0
        for (int e = 0; e < D; ++e) {
            Acc* g = base + o_gp + e;
            *g = (Acc)((double)*g - lam_next * dir(0, e, inv_next));
        }
    if (WS) __threadfence_block();
    __syncthreads();
    for (size_t e = t; e < row; e += THREADS) {
        const Acc v = e < (size_t)n * D ? base[o_gp + e] : Acc(0);
        if (gpts) S::store(gpts + e, v);
        else gslab[e] = v;
    }
}

// chunks > 1: grad_points = sum of the chunks' partial rows, in chunk order
template <int TY>
__global__ __launch_bounds__(256) void polyline_grad_sum_kernel(const typename Storage<TY>::Acc* slab, typename Storage<TY>::T* out,
                                                                size_t count, int chunks)
{
    using S = Storage<TY>;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < count; e += (size_t)gridDim.x * 256) {
        typename S::Acc v = slab[e];
        for (int c = 1; c < chunks; ++c) v += slab[(size_t)c * count + e];
        S::store(out + e, v);
    }
}

struct GradPlan {
    long long threads, chunks;
    int q_chunk;
    bool use_ws;
    size_t lds, region_bytes, ws_acc, ws_slab;
};

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// launch shape of the backward: the forward's chunking of the queries (polyline_kernel's launcher), LDS or workspace
// accumulators; the workspace query and the launch both come through here
GradPlan grad_plan(long long batch, int max_points, int max_distances, int num_dims, int dtype)
{
    GradPlan g{};
    const bool wide = max_points >= kWidePoints;
    g.threads = wide ? 1024 : kThreads;
    long long min_chunk = std::max<long long>(g.threads, ((max_points / 4 + g.threads - 1) / g.threads) * g.threads);
    if (batch * ((max_distances + g.threads - 1) / g.threads) <= kSpreadGroups) min_chunk = g.threads;
    long long chunks = 1;
    if (max_distances >= 2 * min_chunk && batch < 2048)
        chunks = std::max<long long>(1, std::min<long long>((max_distances + min_chunk - 1) / min_chunk, 4096 / batch));
    const long long per_chunk = (max_distances + chunks - 1) / chunks;
    g.q_chunk = (int)std::min<long long>(((per_chunk + g.threads - 1) / g.threads) * g.threads, (long long)INT_MAX - g.threads);
    if (g.q_chunk < g.threads) g.q_chunk = (int)g.threads;
    g.chunks = std::max<long long>(1, ((long long)max_distances + g.q_chunk - 1) / g.q_chunk);
    const size_t acc = acc_size(dtype);
    g.region_bytes = (size_t)std::max(1, max_points) * ((size_t)num_dims + 2) * acc;
    g.use_ws = g.region_bytes + (size_t)g.threads * sizeof(double) > (size_t)kGradLdsBudgetBytes;
    g.lds = g.use_ws ? 16 : g.region_bytes;
    g.ws_acc = g.use_ws ? align256(g.region_bytes) * (size_t)batch * (size_t)g.chunks : 0;
    g.ws_slab = g.chunks > 1 ? align256((size_t)g.chunks * (size_t)batch * (size_t)max_points * (size_t)num_dims * acc) : 0;
    return g;
}

}  // namespace

extern "C" {

size_t accv_polyline_grad_workspace_bytes(long long batch, int max_points, int max_distances, int num_dims, int dtype)
{
    if (batch <= 0 || max_points < 0 || max_distances < 0 || num_dims < 0 || dtype < kPF32 || dtype > kPBF16) return 0;
    const GradPlan g = grad_plan(batch, max_points, max_distances, num_dims, dtype);
    return g.ws_acc + g.ws_slab;
}

int accv_polyline_grad(const void* points, const void* distances, const void* point_counts, const void* dist_counts,
                       const void* grad_out, const void* grad_lengths, void* grad_points, void* grad_distances,
                       long long batch, int max_points, int max_distances, int num_dims, int dtype, int counts_i64,
                       int relative, void* workspace, size_t workspace_bytes, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (batch < 0 || max_points < 0 || max_distances < 0 || num_dims < 0)
        return accv::fail(ACCV_EINVAL, "polyline backward: negative extent");
    if (dtype < kPF32 || dtype > kPBF16) return accv::fail(ACCV_EINVAL, "polyline backward: unsupported dtype code %d", dtype);
    if (batch == 0 || (!grad_points && !grad_distances)) return ACCV_OK;
    if (max_points > 0 && num_dims > 0 && !points) return accv::fail(ACCV_EINVAL, "polyline backward: null points");
    if ((grad_out || grad_distances) && max_distances > 0 && !distances)
        return accv::fail(ACCV_EINVAL, "polyline backward: null distances");
    const GradPlan g = grad_plan(batch, max_points, max_distances, num_dims, dtype);
    const size_t need = g.ws_acc + g.ws_slab;
    if (need > 0 && (!workspace || workspace_bytes < need))
        return accv::fail(ACCV_EWORKSPACE, "polyline backward: needs %zu bytes of workspace", need);
    GradParams p{};
    p.points = points;
    p.distances = distances;
    p.point_counts = point_counts;
    p.dist_counts = dist_counts;
    p.grad_out = max_distances > 0 ? grad_out : nullptr;
    p.grad_lengths = grad_lengths;
    p.grad_points = (max_points > 0 && num_dims > 0) ? grad_points : nullptr;
    p.grad_distances = max_distances > 0 ? grad_distances : nullptr;
    if (!p.grad_points && !p.grad_distances) return ACCV_OK;
    p.acc_ws = g.use_ws ? workspace : nullptr;
    p.slab = g.chunks > 1 ? static_cast<unsigned char*>(workspace) + g.ws_acc : nullptr;
    p.batch = batch;
    p.acc_stride = (long long)(align256(g.region_bytes) / acc_size(dtype));
    p.P = max_points;
    p.Q = max_distances;
    p.D = num_dims;
    p.counts_i64 = counts_i64;
    p.relative = relative;
    p.use_ws = g.use_ws ? 1 : 0;
    p.q_chunk = g.q_chunk;
    p.chunks = (int)g.chunks;
    const dim3 grid((unsigned)batch, (unsigned)g.chunks), block((unsigned)g.threads);
    const bool wide = g.threads == 1024;
    const size_t lds = g.lds;
#define ACCV_LAUNCH_GRAD_W(TYV, DCV, WSV)                                                                   \
    do {                                                                                                    \
        if (wide)                                                                                           \
            hipLaunchKernelGGL((polyline_grad_kernel<TYV, 1024, DCV, WSV>), grid, block, lds, stream, p);   \
        else                                                                                                \
            hipLaunchKernelGGL((polyline_grad_kernel<TYV, kThreads, DCV, WSV>), grid, block, lds, stream, p); \
    } while (0)
#define ACCV_LAUNCH_GRAD_D(TYV, DCV)                                                                        \
    do {                                                                                                    \
        if (g.use_ws)                                                                                       \
            ACCV_LAUNCH_GRAD_W(TYV, DCV, true);                                                             \
        else                                                                                                \
            ACCV_LAUNCH_GRAD_W(TYV, DCV, false);                                                            \
    } while (0)
#define ACCV_LAUNCH_GRAD(TYV)                                                                               \
    do {                                                                                                    \
        if (num_dims == 2)                                                                                  \
            ACCV_LAUNCH_GRAD_D(TYV, 2);                                                                     \
        else if (num_dims == 3)                                                                             \
            ACCV_LAUNCH_GRAD_D(TYV, 3);                                                                     \
        else                                                                                                \
            ACCV_LAUNCH_GRAD_D(TYV, 0);                                                                     \
        if (p.grad_points && g.chunks > 1) {                                                                \
            const size_t count = (size_t)batch * max_points * num_dims;                                     \
            const unsigned blocks = (unsigned)std::min<size_t>((count + 255) / 256, 4096);                  \
            hipLaunchKernelGGL((polyline_grad_sum_kernel<TYV>), dim3(blocks), dim3(256), 0, stream,         \
                               static_cast<const Storage<TYV>::Acc*>(p.slab),                               \
                               static_cast<Storage<TYV>::T*>(p.grad_points), count, p.chunks);              \
        }                                                                                                   \
    } while (0)
    switch (dtype) {
        case kPF32: ACCV_LAUNCH_GRAD(kPF32); break;
        case kPF64: ACCV_LAUNCH_GRAD(kPF64); break;
        case kPF16: ACCV_LAUNCH_GRAD(kPF16); break;
        default: ACCV_LAUNCH_GRAD(kPBF16); break;
    }
#undef ACCV_LAUNCH_GRAD
#undef ACCV_LAUNCH_GRAD_D
#undef ACCV_LAUNCH_GRAD_W
    return accv::check_launch("polyline backward");
}
}

// ---------------------------------------------------------------- host path (CPU tensors)
// The reference's CPU implementation (packages/lane_helpers/ext_impl/polyline/src/polyline_cpu.cpp:28-132) accumulates in
// at::acc_type<dtype, false> = double for float and double inputs and runs at::parallel_for over the polylines; this is its
// counterpart for host memory: double accumulation, the same search / clamping / zero-length-segment / empty-polyline
// rules as the kernel above (polyline_common.cuh:58-163), polylines split over std::threads when there is enough work.
namespace {

// acc[i] = distance from the first point to point i, double (the sampler and its backward)
template <typename T>
void host_prefix(const T* pts, int n, int dims, std::vector<double>& acc)
{
    acc.resize((size_t)n);
    acc[0] = 0.0;
    for (int i = 1; i < n; ++i) {
        double s = 0.0;
        for (int k = 0; k < dims; ++k) {
            const double d = (double)pts[(size_t)(i - 1) * dims + k] - (double)pts[(size_t)i * dims + k];
            s += d * d;
        }
        acc[(size_t)i] = acc[(size_t)i - 1] + std::sqrt(s);
    }
}

// index of the last accumulated distance <= d (-1: before the start, n-1: at / beyond the end)
inline int host_find(const std::vector<double>& acc, int n, double d)
{
    if (acc[0] > d) return -1;
    if (acc[(size_t)n - 1] < d) return n - 1;
    int lo = 0, hi = n - 1;
    while (hi - lo > 1) {
        const int c = (lo + hi) >> 1;
        if (acc[(size_t)c] < d)
            lo = c;
        else if (acc[(size_t)c] > d)
            hi = c;
        else
            lo = hi = c;
    }
    return lo;
}

template <typename T>
void sample_one_host(const T* pts, const T* dist, int n, int q, int dims, bool relative, T* out, T* out_len,
                     std::vector<double>& acc)
{
    const double nan = std::numeric_limits<double>::quiet_NaN();
    if (out_len) *out_len = (T)(n == 0 ? nan : 0.0);
    if (n == 0) {
        if (out)
            for (int i = 0; i < q * dims; ++i) out[i] = (T)nan;
        return;
    }
    host_prefix(pts, n, dims, acc);
    const double total = acc[(size_t)n - 1];
    if (out_len) *out_len = (T)total;
    if (!out) return;
    const double eps = std::numeric_limits<double>::epsilon();
    for (int j = 0; j < q; ++j) {
        double d = (double)dist[j];
        if (relative) d *= total;
        const int idx = host_find(acc, n, d);
        T* o = out + (size_t)j * dims;
        if (idx >= 0 && idx < n - 1) {
            const double seg = acc[(size_t)idx + 1] - acc[(size_t)idx];
            if (seg >= eps) {
                const double w0 = (acc[(size_t)idx + 1] - d) / seg, w1 = (d - acc[(size_t)idx]) / seg;
                for (int k = 0; k < dims; ++k)
                    o[k] = (T)((double)pts[(size_t)idx * dims + k] * w0 + (double)pts[(size_t)(idx + 1) * dims + k] * w1);
            } else {
                for (int k = 0; k < dims; ++k) o[k] = pts[(size_t)idx * dims + k];   // zero-length segment: its lower point
            }
        } else {
            const int e = idx < 0 ? 0 : n - 1;                                        // clamped to an end point
            for (int k = 0; k < dims; ++k) o[k] = pts[(size_t)e * dims + k];
        }
    }
}

template <typename T>
void sample_host(const void* points, const void* distances, const void* pc, const void* dc, void* out_points, void* out_lengths,
                 long long batch, int P, int Q, int D, int counts_i64, int relative, int threads)
{
    auto count_of = [&](const void* c, long long i, int cap) {
        return c ? (int)accv::clamp_count(c, i, cap, counts_i64) : cap;
    };
    auto run = [&](long long lo, long long hi) {
        std::vector<double> acc;
        for (long long i = lo; i < hi; ++i)
            sample_one_host<T>(static_cast<const T*>(points) + (size_t)i * P * D,
                               distances ? static_cast<const T*>(distances) + (size_t)i * Q : nullptr, count_of(pc, i, P),
                               out_points ? count_of(dc, i, Q) : 0, D, relative != 0,
                               out_points ? static_cast<T*>(out_points) + (size_t)i * Q * D : nullptr,
                               out_lengths ? static_cast<T*>(out_lengths) + i : nullptr, acc);
    };
    const long long work = batch * ((long long)P + Q) * std::max(1, D);
    int t = (int)std::min<long long>(std::max(1, threads), std::min<long long>(batch, work / 65536 + 1));
    if (t <= 1) {
        run(0, batch);
        return;
    }
    std::vector<std::thread> pool;
    for (int k = 0; k < t; ++k) pool.emplace_back(run, batch * k / t, batch * (k + 1) / t);
    for (auto& th : pool) th.join();
}


// backward of sample_one_host for one polyline (the kernel's backward above, in double): grad rows written whole
template <typename T>
void grad_one_host(const T* pts, const T* dist, const T* gout, const T* glen, int n, int P, int q, int Q, int dims,
                   bool relative, T* gp, T* gd, std::vector<double>& acc, std::vector<double>& gacc, std::vector<double>& bs)
{
    if (gd)
        for (int j = (n > 0 && gout) ? q : 0; j < Q; ++j) gd[j] = (T)0;
    if (n == 0 || (!gp && !gd)) {
        if (gp)
            for (size_t e = 0; e < (size_t)P * dims; ++e) gp[e] = (T)0;
        return;
    }
    host_prefix(pts, n, dims, acc);
    const double total = acc[(size_t)n - 1];
    const double eps = std::numeric_limits<double>::epsilon();
    gacc.assign((size_t)n * dims, 0.0);
    bs.assign((size_t)n, 0.0);   // lambda_k = sum_{j > k} bs[j]
    auto inv_len = [&](int k) {
        double l2 = 0.0;
        for (int e = 0; e < dims; ++e) {
            const double diff = (double)pts[(size_t)(k + 1) * dims + e] - (double)pts[(size_t)k * dims + e];
            l2 += diff * diff;
        }
        const double l = std::sqrt(l2);
        return l >= eps ? 1.0 / l : 0.0;
    };
    if (gout)
        for (int j = 0; j < q; ++j) {
            const T* g = gout + (size_t)j * dims;
            const double r = (double)dist[j];
            const double d = relative ? r * total : r;
            const int idx = host_find(acc, n, d);
            double gdj = 0.0;
            if (idx >= 0 && idx < n - 1 && acc[(size_t)idx + 1] - acc[(size_t)idx] >= eps) {
                const double seg = acc[(size_t)idx + 1] - acc[(size_t)idx];
                const double w0 = (acc[(size_t)idx + 1] - d) / seg, w1 = (d - acc[(size_t)idx]) / seg;
                double l2 = 0.0;
                for (int k = 0; k < dims; ++k) {
                    const double diff = (double)pts[(size_t)idx * dims + k] - (double)pts[(size_t)(idx + 1) * dims + k];
                    l2 += diff * diff;
                }
                const double inv = 1.0 / std::sqrt(l2);
                double s = 0.0;
                for (int k = 0; k < dims; ++k) {
                    const double gk = (double)g[k];
                    s += gk * ((double)pts[(size_t)(idx + 1) * dims + k] - (double)pts[(size_t)idx * dims + k]) * inv;
                    gacc[(size_t)idx * dims + k] += w0 * gk;
                    gacc[(size_t)(idx + 1) * dims + k] += w1 * gk;
                }
                bs[(size_t)idx] -= w0 * s;
                bs[(size_t)idx + 1] -= w1 * s;
                if (relative) bs[(size_t)n - 1] += r * s;
                gdj = relative ? s * total : s;
            } else {
                const int c = idx < 0 ? 0 : idx;   // a copy of one point: the first, the last or a short segment's lower one
                for (int k = 0; k < dims; ++k) gacc[(size_t)c * dims + k] += (double)g[k];
            }
            if (gd) gd[j] = (T)gdj;
        }
    else if (gd)
        for (int j = 0; j < q; ++j) gd[j] = (T)0;
    if (!gp) return;
    if (glen && n >= 2) bs[(size_t)n - 1] += (double)*glen;
    double lam = 0.0;   // lambda_k, from the last segment down
    for (int k = n - 2; k >= 0; --k) {
        lam += bs[(size_t)k + 1];
        const double inv = inv_len(k);
        if (inv == 0.0) continue;
        for (int e = 0; e < dims; ++e) {
            const double v = lam * ((double)pts[(size_t)(k + 1) * dims + e] - (double)pts[(size_t)k * dims + e]) * inv;
            gacc[(size_t)(k + 1) * dims + e] += v;
            gacc[(size_t)k * dims + e] -= v;
        }
    }
    for (size_t e = 0; e < (size_t)P * dims; ++e) gp[e] = (T)(e < (size_t)n * dims ? gacc[e] : 0.0);
}

template <typename T>
void grad_host(const void* points, const void* distances, const void* pc, const void* dc, const void* grad_out,
               const void* grad_lengths, void* grad_points, void* grad_distances, long long batch, int P, int Q, int D,
               int counts_i64, int relative, int threads)
{
    auto count_of = [&](const void* c, long long i, int cap) {
        return c ? (int)accv::clamp_count(c, i, cap, counts_i64) : cap;
    };
    auto run = [&](long long lo, long long hi) {
        std::vector<double> acc, gacc, bs;
        for (long long i = lo; i < hi; ++i)
            grad_one_host<T>(static_cast<const T*>(points) + (size_t)i * P * D,
                             distances ? static_cast<const T*>(distances) + (size_t)i * Q : nullptr,
                             grad_out ? static_cast<const T*>(grad_out) + (size_t)i * Q * D : nullptr,
                             grad_lengths ? static_cast<const T*>(grad_lengths) + i : nullptr, count_of(pc, i, P), P,
                             count_of(dc, i, Q), Q, D, relative != 0,
                             grad_points ? static_cast<T*>(grad_points) + (size_t)i * P * D : nullptr,
                             grad_distances ? static_cast<T*>(grad_distances) + (size_t)i * Q : nullptr, acc, gacc, bs);
    };
    const long long work = batch * ((long long)P + Q) * std::max(1, D);
    int t = (int)std::min<long long>(std::max(1, threads), std::min<long long>(batch, work / 65536 + 1));
    if (t <= 1) {
        run(0, batch);
        return;
    }
    std::vector<std::thread> pool;
    for (int k = 0; k < t; ++k) pool.emplace_back(run, batch * k / t, batch * (k + 1) / t);
    for (auto& th : pool) th.join();
}

}  // namespace

extern "C" int accv_polyline_sample_host(const void* points, const void* distances, const void* point_counts,
                                         const void* dist_counts, void* out_points, void* out_lengths, long long batch,
                                         int max_points, int max_distances, int num_dims, int dtype, int counts_i64,
                                         int relative, int threads)
{
    if (batch < 0 || max_points < 0 || max_distances < 0 || num_dims < 0)
        return accv::fail(ACCV_EINVAL, "polyline (host): negative extent");
    if (dtype != 0 && dtype != 1) return accv::fail(ACCV_EINVAL, "polyline (host): float32 / float64 only, got dtype code %d", dtype);
    if (batch == 0 || (!out_points && !out_lengths)) return ACCV_OK;
    if (max_points > 0 && num_dims > 0 && !points) return accv::fail(ACCV_EINVAL, "polyline (host): null points");
    if (out_points && max_distances > 0 && !distances) return accv::fail(ACCV_EINVAL, "polyline (host): null distances");
    if (threads <= 0) threads = (int)std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
    if (dtype == 0)
        sample_host<float>(points, distances, point_counts, dist_counts, out_points, out_lengths, batch, max_points,
                           max_distances, num_dims, counts_i64, relative, threads);
    else
        sample_host<double>(points, distances, point_counts, dist_counts, out_points, out_lengths, batch, max_points,
                            max_distances, num_dims, counts_i64, relative, threads);
    return ACCV_OK;
}

extern "C" int accv_polyline_grad_host(const void* points, const void* distances, const void* point_counts,
                                       const void* dist_counts, const void* grad_out, const void* grad_lengths,
                                       void* grad_points, void* grad_distances, long long batch, int max_points,
                                       int max_distances, int num_dims, int dtype, int counts_i64, int relative, int threads)
{
    if (batch < 0 || max_points < 0 || max_distances < 0 || num_dims < 0)
        return accv::fail(ACCV_EINVAL, "polyline backward (host): negative extent");
    if (dtype != 0 && dtype != 1)
        return accv::fail(ACCV_EINVAL, "polyline backward (host): float32 / float64 only, got dtype code %d", dtype);
    if (batch == 0 || (!grad_points && !grad_distances)) return ACCV_OK;
    if (max_points > 0 && num_dims > 0 && !points) return accv::fail(ACCV_EINVAL, "polyline backward (host): null points");
    if ((grad_out || grad_distances) && max_distances > 0 && !distances)
        return accv::fail(ACCV_EINVAL, "polyline backward (host): null distances");
    if (max_points == 0 || num_dims == 0) grad_points = nullptr;
    if (max_distances == 0) {
        grad_out = nullptr;
        grad_distances = nullptr;
    }
    if (!grad_points && !grad_distances) return ACCV_OK;
    if (threads <= 0) threads = (int)std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
    if (dtype == 0)
        grad_host<float>(points, distances, point_counts, dist_counts, grad_out, grad_lengths, grad_points, grad_distances,
                         batch, max_points, max_distances, num_dims, counts_i64, relative, threads);
    else
        grad_host<double>(points, distances, point_counts, dist_counts, grad_out, grad_lengths, grad_points, grad_distances,
                          batch, max_points, max_distances, num_dims, counts_i64, relative, threads);
    return ACCV_OK;
}
