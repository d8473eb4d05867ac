// Set prediction over polylines (MapTR-style vectorised map heads, lane-DETR heads): the [B, Q, G_max] matching cost and
// the loss over the matched pairs.  A ground-truth line equals all of its equivalent orders (an open line its reverse, a
// closed polygon its cyclic shifts in both directions), so both take the minimum over the orders of the point-wise L1
// distance; the torch composition materialises a [B, Q, G, V, P, D] tensor for that.  Per-pair arithmetic:
// polyline_match_arith.h; the class term of the cost: matching_cost_arith.h.
//
// Cost: a workgroup of kThreads lanes owns one frame and kQueryTile queries, whose points it stages in LDS in the
// arithmetic type.  It walks the frame's ground-truth lines in chunks of up to kWave lines, staged in LDS with a row
// stride padded to an odd number of elements, so that the lanes of a wave, which read different lines at the same point,
// land on different banks.  Lanes run along g: every store of the contiguous output row is coalesced.  A wave owns
// kQueriesPerWave queries and keeps their sums side by side, so one LDS read of the ground truth serves all of them; the
// query's point is a broadcast read.  No order is ever written anywhere.  One launch.
// Loss forward: a workgroup owns kLossQueries consecutive queries of one frame and builds their query -> slot table in LDS
// (the pair rule of matched_pairs.h).  A wave takes one matched pair at a time: its lanes search the orders side by side
// (lowest v on ties), then take the points of the best order side by side and the wave adds them up in f64 in a fixed
// order.  One (pts, dir) partial per workgroup; the one-block launch of matched_pairs.h adds them per frame.
// Loss backward: the same table and search, then every element of the contiguous [B, Q, P, D] gradient written exactly
// once, +0 for a query without a pair: no zero fill, no atomics.
// Neither direction synchronises; both are bitwise reproducible.  No MFMA: the work is absolute differences and minima.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>
#include <limits>
#include <vector>

#include "accv_common.h"
#include "matched_pairs.h"
#include "polyline_match_arith.h"

#pragma clang fp contract(off)

namespace {

using namespace accv_pm;

constexpr int kThreads = 256;
constexpr int kWave = 64;                                   // ground-truth lines per LDS chunk at most, one per lane
constexpr int kWaves = kThreads / kWave;
constexpr int kQueriesPerWave = 4;
constexpr int kQueryTile = kWaves * kQueriesPerWave;        // queries per workgroup of the cost kernel
constexpr int kLossQueries = 64;                            // queries per workgroup of the loss kernels
constexpr size_t kLdsBudget = 64 * 1024;                    // dynamic LDS of the cost kernel
constexpr unsigned kKnownFlags = ACCV_PM_IDX_I64 | ACCV_PM_REVERSIBLE | ACCV_PM_LABELS_I64 | ACCV_PM_CLOSED_I32 | ACCV_PM_CLOSED_I64;

struct Args {
    const void* x;              // [B, Q, P, D] predictions, element (b, q, i) at b * sb + q * sq + i
    const void* t;              // [B, G, P, D] ground truth, contiguous
    const void* closed;         // [B, G] or null
    const long long* counts;    // [B]
    long long B, Q, G, sb, sq;
    int P, D, PD, reversible, closed_size;
    // cost
    const void* scores;
    const void* labels;
    long long C, ssb, ssq;
    void* out;
    long long nqt;              // query tiles per frame
    int chunk, stride, labels64;   // lines per LDS chunk, LDS row stride (elements)
    // loss
    const void* pind;           // [B, K]
    const void* gind;
    long long K, nqb;           // workgroups per frame
    int idx64, dir;
    double eps;
};

__host__ __device__ inline int is_closed(const Args& a, long long i)
{
    if (!a.closed) return 0;
    if (a.closed_size == 1) return static_cast<const unsigned char*>(a.closed)[i] != 0;
    return load_index(a.closed, i, a.closed_size == 8) != 0;
}

template <class F>
__host__ __device__ inline F pair_cost(const Params<F>& p, F score, F pts)
{
    F acc = F(0);
    if (p.cls) acc = acc + class_term(p, score) * p.class_weight;
    if (p.l1) acc = acc + pts * p.l1_weight;
    return acc;
}

template <int DT>
__host__ __device__ inline typename Compute<DT>::type score_at(const Args& a, long long b, long long q, long long g)
{
    using F = typename Compute<DT>::type;
    const long long label = load_index(a.labels, b * a.G + g, a.labels64);
    if (label < 0 || label >= a.C) return std::numeric_limits<F>::quiet_NaN();
    return load<DT>(a.scores, b * a.ssb + q * a.ssq + label);
}

// ---------------------------------------------------------------------------------------------------------- cost, device
template <int DT, int D>
__global__ __launch_bounds__(kThreads) void pm_cost_kernel(const Args a, const Params<typename Compute<DT>::type> p)
{
    using F = typename Compute<DT>::type;
    extern __shared__ double s_raw[];
    F* s_x = reinterpret_cast<F*>(s_raw);            // [kQueryTile][PD]
    F* s_t = s_x + kQueryTile * a.PD;                // [chunk][stride]
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const long long b = blockIdx.x / a.nqt;
    const long long q0 = (blockIdx.x - b * a.nqt) * kQueryTile;
    const long long left = a.Q - q0;
    const int nq = (int)(left < kQueryTile ? left : kQueryTile);
    const int P = a.P, PD = a.PD;
    const long long Gb = clamp_count(a.counts, b, a.G);
    if (p.l1) {
        for (int e = tid; e < kQueryTile * PD; e += kThreads) {
            const int i = e / PD, r = e - i * PD;
            s_x[e] = i < nq ? load<DT>(a.x, b * a.sb + (q0 + i) * a.sq + r) : F(0);
        }
    }
    F* out = static_cast<F*>(a.out) + (b * a.Q + q0) * a.G;
    const int k0 = wave * kQueriesPerWave;
    for (long long g0 = 0; g0 < a.G; g0 += a.chunk) {
        if (p.l1) {
            if (g0 > 0) __syncthreads();             // the previous chunk is read no more
            const long long rest = Gb - g0;
            const int lines = (int)(rest < 0 ? 0 : (rest < a.chunk ? rest : a.chunk));
            for (int e = tid; e < lines * PD; e += kThreads) {
                const int l = e / PD, r = e - l * PD;
                s_t[l * a.stride + r] = load<DT>(a.t, (b * a.G + g0 + l) * PD + r);
            }
            __syncthreads();
        }
        const long long g = g0 + lane;
        if (lane >= a.chunk || g >= a.G) continue;
        if (g >= Gb) {
#pragma unroll
            for (int k = 0; k < kQueriesPerWave; ++k)
                if (k0 + k < nq) out[(long long)(k0 + k) * a.G + g] = p.filler;
            continue;
        }
        F best[kQueriesPerWave];
#pragma unroll
        for (int k = 0; k < kQueriesPerWave; ++k) best[k] = F(0);
        if (p.l1) {
            const int closed = is_closed(a, b * a.G + g);
            const int V = num_variants(P, closed, a.reversible);
            const F* row = s_t + lane * a.stride;
            const F* xs = s_x + k0 * PD;
            for (int v = 0; v < V; ++v) {
                L1Acc<F> acc[kQueriesPerWave];       // the sequence of variant_sum, kQueriesPerWave queries side by side
                for (int pt = 0; pt < P; ++pt) {
                    const int i = variant_point(v, pt, P, closed);
#pragma unroll
                    for (int d = 0; d < D; ++d) {
                        const F tv = row[i * D + d];
#pragma unroll
                        for (int k = 0; k < kQueriesPerWave; ++k) acc[k].add(m_abs(xs[k * PD + pt * D + d] - tv));
                    }
#pragma unroll
                    for (int k = 0; k < kQueriesPerWave; ++k) acc[k].end_point(pt);
                }
#pragma unroll
                for (int k = 0; k < kQueriesPerWave; ++k) {
                    const F s = acc[k].value();
                    if (v == 0 || s < best[k]) best[k] = s;
                }
            }
        }
#pragma unroll
        for (int k = 0; k < kQueriesPerWave; ++k) {
            if (k0 + k >= nq) continue;
            const F score = p.cls ? score_at<DT>(a, b, q0 + k0 + k, g) : F(0);
            out[(long long)(k0 + k) * a.G + g] = pair_cost(p, score, best[k]);
        }
    }
}

// ------------------------------------------------------------------------------------------------------------ cost, host
template <int DT>
void cost_host(const Args& a, const Params<typename Compute<DT>::type>& p)
{
    using F = typename Compute<DT>::type;
    F* out = static_cast<F*>(a.out);
    for (long long b = 0; b < a.B; ++b) {
        const long long Gb = clamp_count(a.counts, b, a.G);
        for (long long q = 0; q < a.Q; ++q)
            for (long long g = 0; g < a.G; ++g) {
                F& o = out[(b * a.Q + q) * a.G + g];
                if (g >= Gb) {
                    o = p.filler;
                    continue;
                }
                F best = F(0);
                if (p.l1) {
                    const int closed = is_closed(a, b * a.G + g);
                    const Row<DT> x{a.x, b * a.sb + q * a.sq}, t{a.t, (b * a.G + g) * a.PD};
                    best_variant<F>(x, t, num_variants(a.P, closed, a.reversible), a.P, a.D, closed, best);
                }
                o = pair_cost(p, p.cls ? score_at<DT>(a, b, q, g) : F(0), best);
            }
    }
}

// ---------------------------------------------------------------------------------------------------------- loss, device
// s_slot[i] = the slot of the pair of query q0 + i, or kNoSlot
__device__ __forceinline__ void build_table(const Args& a, long long b, long long q0, int nq, int* s_slot)
{
    const int tid = threadIdx.x;
    if (tid < kLossQueries) s_slot[tid] = kNoSlot;
    __syncthreads();
    scan_pairs<kThreads>(a.pind, a.gind, a.idx64, a.counts, b, a.K, a.G, q0, nq, s_slot);
}

// best_variant by a whole wave: lane l takes the orders l, l + 64, ...; the same v in every lane
template <class F, class X, class T>
__device__ __forceinline__ int wave_best_variant(const X& x, const T& t, int V, int P, int D, int closed, int lane)
{
    if (V == 1) return 0;
    F bs = F(0);
    int bv = INT_MAX;
    for (int v = lane; v < V; v += kWave) {
        const F s = variant_sum<F>(x, t, v, P, D, closed);
        if (bv == INT_MAX || s < bs) bs = s, bv = v;
    }
#pragma unroll
    for (int m = kWave / 2; m >= 1; m >>= 1) {
        const F os = __shfl_xor(bs, m);
        const int ov = __shfl_xor(bv, m);
        if (ov != INT_MAX && (bv == INT_MAX || os < bs || (os == bs && ov < bv))) bs = os, bv = ov;
    }
    return __shfl(bv, 0);   // lane 0 starts at v = 0, which NaN sums leave in place
}

template <int DT>
__global__ __launch_bounds__(kThreads) void pm_fwd_kernel(const Args a, double* __restrict__ part)
{
    using F = typename Compute<DT>::type;
    __shared__ int s_slot[kLossQueries];
    const Range r = range_of(a.nqb, kLossQueries, a.Q);
    build_table(a, r.b, r.q0, r.nq, s_slot);
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    double pts = 0.0, dir = 0.0;
    for (int i = wave; i < r.nq; i += kWaves) {
        const int j = s_slot[i];
        if (j == kNoSlot) continue;
        const long long g = load_index(a.gind, r.b * a.K + j, a.idx64);   // in range: checked when the slot was entered
        const Row<DT> x{a.x, r.b * a.sb + (r.q0 + i) * a.sq}, t{a.t, (r.b * a.G + g) * a.PD};
        const int closed = is_closed(a, r.b * a.G + g);
        const int v = wave_best_variant<F>(x, t, num_variants(a.P, closed, a.reversible), a.P, a.D, closed, lane);
        const int segs = num_segments(a.P, closed);
        double sp = 0.0, sd = 0.0;
        for (int pt = lane; pt < a.P; pt += kWave) {
            sp += (double)point_l1<F>(x, t, v, pt, a.P, a.D, closed);
            if (a.dir && pt < segs) {
                double sa[3], sb[3];
                segment(x, t, v, pt, a.P, a.D, closed, sa, sb);
                sd += dir_value(sa, sb, a.eps);
            }
        }
#pragma unroll
        for (int m = kWave / 2; m >= 1; m >>= 1) sp += __shfl_xor(sp, m), sd += __shfl_xor(sd, m);
        if (lane == 0) pts += sp, dir += sd;
    }
    block_sum<double, double, kThreads>(pts, dir);
    if (threadIdx.x == 0) {
        part[blockIdx.x] = pts;
        part[(size_t)gridDim.x + blockIdx.x] = dir;
    }
}

template <int DT, class O>
__global__ __launch_bounds__(kThreads) void pm_bwd_kernel(const Args a, const O* __restrict__ grad_pts,
                                                          const O* __restrict__ grad_dir, const double* __restrict__ denom,
                                                          void* __restrict__ grad)
{
    using F = typename Compute<DT>::type;
    __shared__ int s_slot[kLossQueries];
    const Range r = range_of(a.nqb, kLossQueries, a.Q);
    build_table(a, r.b, r.q0, r.nq, s_slot);
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const double dn = *denom;
    const bool use_pts = grad_pts != nullptr, use_dir = a.dir && grad_dir != nullptr;
    const F s1 = use_pts ? (F)((double)grad_pts[r.b] / dn) : F(0);
    const double s2 = use_dir ? (double)grad_dir[r.b] / dn : 0.0;
    for (int i = wave; i < r.nq; i += kWaves) {
        const long long first = (r.b * a.Q + r.q0 + i) * a.PD;
        const int j = s_slot[i];
        if (j == kNoSlot) {
            for (int e = lane; e < a.PD; e += kWave) store<DT>(grad, first + e, F(0));
            continue;
        }
        const long long g = load_index(a.gind, r.b * a.K + j, a.idx64);
        const Row<DT> x{a.x, r.b * a.sb + (r.q0 + i) * a.sq}, t{a.t, (r.b * a.G + g) * a.PD};
        const int closed = is_closed(a, r.b * a.G + g);
        const int v = wave_best_variant<F>(x, t, num_variants(a.P, closed, a.reversible), a.P, a.D, closed, lane);
        for (int pt = lane; pt < a.P; pt += kWave) {
            F o[3];
            point_grad<F>(x, t, v, pt, a.P, a.D, closed, use_pts, s1, use_dir, s2, a.eps, o);
            store<DT>(grad, first + pt * a.D, o[0]);
            store<DT>(grad, first + pt * a.D + 1, o[1]);
            if (a.D == 3) store<DT>(grad, first + pt * a.D + 2, o[2]);
        }
    }
}

// ------------------------------------------------------------------------------------------------------------ loss, host
void host_table(const Args& a, long long b, std::vector<int>& tab)
{
    host_pair_table(a.pind, a.gind, a.idx64, a.counts, b, a.K, a.Q, a.G, tab);
}

template <int DT>
void host_fwd(const Args& a, const accv_polyline_match_params* p, void* out_v, double* out_denom)
{
    using F = typename Compute<DT>::type;
    F* out = static_cast<F*>(out_v);
    const double denom = host_denom(a.counts, a.B, a.K, p->avg_mode, p->avg_factor, p->avg_factor_dev);
    std::vector<int> tab;
    for (long long b = 0; b < a.B; ++b) {
        host_table(a, b, tab);
        double pts = 0.0, dir = 0.0;
        for (long long q = 0; q < a.Q; ++q) {
            const int j = tab[(size_t)q];
            if (j == kNoSlot) continue;
            const long long g = load_index(a.gind, b * a.K + j, a.idx64);
            const Row<DT> x{a.x, b * a.sb + q * a.sq}, t{a.t, (b * a.G + g) * a.PD};
            const int closed = is_closed(a, b * a.G + g);
            F best;
            const int v = best_variant<F>(x, t, num_variants(a.P, closed, a.reversible), a.P, a.D, closed, best);
            const int segs = num_segments(a.P, closed);
            for (int pt = 0; pt < a.P; ++pt) {
                pts += (double)point_l1<F>(x, t, v, pt, a.P, a.D, closed);
                if (a.dir && pt < segs) {
                    double sa[3], sb[3];
                    segment(x, t, v, pt, a.P, a.D, closed, sa, sb);
                    dir += dir_value(sa, sb, a.eps);
                }
            }
        }
        out[b] = (F)(pts / denom), out[a.B + b] = (F)(dir / denom);
    }
    *out_denom = denom;
}

template <int DT>
void host_bwd(const Args& a, const void* grad_pts_v, const void* grad_dir_v, const double* denom, void* grad)
{
    using F = typename Compute<DT>::type;
    const F* grad_pts = static_cast<const F*>(grad_pts_v);
    const F* grad_dir = static_cast<const F*>(grad_dir_v);
    const bool use_pts = grad_pts != nullptr, use_dir = a.dir && grad_dir != nullptr;
    std::vector<int> tab;
    for (long long b = 0; b < a.B; ++b) {
        host_table(a, b, tab);
        const F s1 = use_pts ? (F)((double)grad_pts[b] / *denom) : F(0);
        const double s2 = use_dir ? (double)grad_dir[b] / *denom : 0.0;
        for (long long q = 0; q < a.Q; ++q) {
            const int j = tab[(size_t)q];
            const long long first = (b * a.Q + q) * a.PD;
            if (j == kNoSlot) {
                for (int e = 0; e < a.PD; ++e) store<DT>(grad, first + e, F(0));
                continue;
            }
            const long long g = load_index(a.gind, b * a.K + j, a.idx64);
            const Row<DT> x{a.x, b * a.sb + q * a.sq}, t{a.t, (b * a.G + g) * a.PD};
            const int closed = is_closed(a, b * a.G + g);
            F best;
            const int v = best_variant<F>(x, t, num_variants(a.P, closed, a.reversible), a.P, a.D, closed, best);
            for (int pt = 0; pt < a.P; ++pt) {
                F o[3];
                point_grad<F>(x, t, v, pt, a.P, a.D, closed, use_pts, s1, use_dir, s2, a.eps, o);
                for (int d = 0; d < a.D; ++d) store<DT>(grad, first + pt * a.D + d, o[d]);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------- checks
// what the cost and the loss share; ACCV_OK with *empty = 1 when an extent in `extents` is 0.  Every check runs before
// anything else reads the arguments.
int check_common(const char* who, const void* pred, const void* gt, int dtype, unsigned flags, unsigned allowed, long long B,
                 long long Q, long long G, long long P, long long D, long long other, const accv_polyline_match_params* p,
                 bool need_lines, long long zero_extent, Args& a, int* empty)
{
    *empty = 0;
    if (int rc = check_pair_sizes(who, p, {B, Q, G, P, D, other}, dtype, flags, allowed)) return rc;
    if ((flags & ACCV_PM_CLOSED_I32) && (flags & ACCV_PM_CLOSED_I64))
        return accv::fail(ACCV_EINVAL, "%s: gt_closed cannot be both int32 and int64", who);
    if (zero_extent == 0) {
        *empty = 1;
        return ACCV_OK;
    }
    if (P < kMinP || P > kMaxP) return accv::fail(ACCV_EINVAL, "%s: needs %d <= P <= %d (got %lld)", who, kMinP, kMaxP, P);
    if (D != 2 && D != 3) return accv::fail(ACCV_EINVAL, "%s: needs D of 2 or 3 (got %lld)", who, D);
    if (need_lines) {
        if (p->pred_stride_q < P * D || p->pred_stride_b < 0)
            return accv::fail(ACCV_EINVAL, "%s: query stride %lld below P * D = %lld, or negative batch stride", who,
                              p->pred_stride_q, P * D);
        if (!pred) return accv::fail(ACCV_EINVAL, "%s: null lines pointer", who);
        if (G > 0 && !gt) return accv::fail(ACCV_EINVAL, "%s: null ground-truth pointer", who);
        if (reinterpret_cast<uintptr_t>(pred) % (uintptr_t)elem_size(dtype) || reinterpret_cast<uintptr_t>(gt) % (uintptr_t)elem_size(dtype))
            return accv::fail(ACCV_EINVAL, "%s: lines are not aligned to their element size", who);
    }
    if (Q > LLONG_MAX / (P * D) / B) return accv::fail(ACCV_EINVAL, "%s: B x Q x P x D overflows", who);
    a = Args{};
    a.x = pred, a.t = gt, a.closed = p->gt_closed;
    a.B = B, a.Q = Q, a.G = G, a.sb = p->pred_stride_b, a.sq = p->pred_stride_q;
    a.P = (int)P, a.D = (int)D, a.PD = (int)(P * D);
    a.reversible = (flags & ACCV_PM_REVERSIBLE) ? 1 : 0;
    a.closed_size = (flags & ACCV_PM_CLOSED_I64) ? 8 : ((flags & ACCV_PM_CLOSED_I32) ? 4 : 1);
    return ACCV_OK;
}

int check_cost(const char* who, const void* pred, const void* gt, const void* scores, const void* labels,
               const long long* counts, int dtype, unsigned flags, long long B, long long Q, long long G, long long P,
               long long D, long long C, long long ssb, long long ssq, const accv_polyline_match_params* p, const void* out,
               Args& a, int* empty)
{
    const bool pts = p && p->pts_weight != 0.0, cls = p && p->class_weight != 0.0;
    if (p && (p->class_kind < kOneMinusProb || p->class_kind > kFocal))
        return accv::fail(ACCV_EINVAL, "%s: unknown class cost kind %d", who, p->class_kind);
    const unsigned allowed = kKnownFlags & ~ACCV_PM_IDX_I64;
    if (int rc = check_common(who, pred, gt, dtype, flags, allowed, B, Q, G, P, D, C, p, pts, B * Q * G, a, empty)) return rc;
    if (*empty) return ACCV_OK;
    if (!out) return accv::fail(ACCV_EINVAL, "%s: null output", who);
    if (cls && (!scores || !labels)) return accv::fail(ACCV_EINVAL, "%s: null scores / labels for the class cost", who);
    a.counts = counts, a.scores = scores, a.labels = labels, a.C = C, a.ssb = ssb, a.ssq = ssq;
    a.labels64 = (flags & ACCV_PM_LABELS_I64) ? 1 : 0;
    a.out = const_cast<void*>(out);
    a.nqt = (Q + kQueryTile - 1) / kQueryTile;
    if (a.nqt > accv::kGridLimit / B) return accv::fail(ACCV_EINVAL, "%s: %lld x %lld workgroups exceed the grid limit", who, B, a.nqt);
    return ACCV_OK;
}

int check_loss(const char* who, const void* pred, const void* gt, const void* pind, const void* gind, const long long* counts,
               int dtype, unsigned flags, long long B, long long Q, long long G, long long P, long long D, long long K,
               const accv_polyline_match_params* p, bool forward, Args& a, int* empty)
{
    if (int rc = check_pair_mode(who, forward && p, p ? p->avg_mode : 0, K, 0, "K is")) return rc;
    const unsigned allowed = kKnownFlags & ~ACCV_PM_LABELS_I64;
    if (int rc = check_common(who, pred, gt, dtype, flags, allowed, B, Q, G, P, D, K, p, true, B * Q, a, empty)) return rc;
    if (*empty) return ACCV_OK;
    if (int rc = check_pair_pointers(who, true, "counts", counts, pind, gind, K)) return rc;
    a.counts = counts, a.pind = pind, a.gind = gind, a.K = K;
    a.idx64 = (flags & ACCV_PM_IDX_I64) ? 1 : 0, a.dir = p->dir_loss ? 1 : 0, a.eps = p->dir_eps;
    a.nqb = (Q + kLossQueries - 1) / kLossQueries;
    return check_pair_launch(who, forward, p->avg_mode, p->avg_factor_dev, B, a.nqb);
}

template <class F>
Params<F> make_params(const accv_polyline_match_params* in)
{
    Params<F> p{};
    p.class_weight = (F)in->class_weight, p.l1_weight = (F)in->pts_weight;
    p.alpha = (F)in->focal_alpha, p.gamma = (F)in->focal_gamma, p.focal_eps = (F)in->focal_eps, p.filler = (F)in->filler;
    p.kind = in->class_kind;
    // a term is evaluated when its weight (as given, before any narrowing) is not zero; a NaN weight counts
    p.cls = in->class_weight != 0.0, p.l1 = in->pts_weight != 0.0;
    return p;
}

// lines per LDS chunk and the padded row stride: an odd number of elements, so that the rows of consecutive lanes start
// on different banks in both the 4-byte and the 8-byte arithmetic type
template <class F>
size_t plan_lds(Args& a)
{
    a.stride = a.PD | 1;
    const size_t x_bytes = (size_t)kQueryTile * a.PD * sizeof(F), row = (size_t)a.stride * sizeof(F);
    const size_t fit = (kLdsBudget - x_bytes) / row;   // >= 5 at P = 128, D = 3 in f64
    const long long want = a.G < kWave ? a.G : kWave;
    a.chunk = (int)((long long)fit < want ? (long long)fit : want);
    return x_bytes + (size_t)a.chunk * row;
}

template <int DT>
int launch_cost(Args a, const accv_polyline_match_params* in, hipStream_t s)
{
    using F = typename Compute<DT>::type;
    const Params<F> p = make_params<F>(in);
    const size_t lds = p.l1 ? plan_lds<F>(a) : 0;
    if (!p.l1) a.chunk = kWave, a.stride = 0;
    const dim3 grid((unsigned)(a.B * a.nqt)), block(kThreads);
    if (a.D == 2) hipLaunchKernelGGL((pm_cost_kernel<DT, 2>), grid, block, lds, s, a, p);
    else hipLaunchKernelGGL((pm_cost_kernel<DT, 3>), grid, block, lds, s, a, p);
    return accv::check_launch("polyline_matching_cost");
}

template <int DT>
void launch_fwd(const Args& a, const accv_polyline_match_params* p, double* part, void* out, double* out_denom, hipStream_t s)
{
    using O = typename Compute<DT>::type;
    hipLaunchKernelGGL(pm_fwd_kernel<DT>, dim3((unsigned)(a.B * a.nqb)), dim3(kThreads), 0, s, a, part);
    hipLaunchKernelGGL((pair_finish_kernel<2, O>), dim3(1), dim3(kFinishThreads), 0, s, part, a.counts, a.B, a.nqb, a.K, p->avg_mode,
                       p->avg_factor, p->avg_factor_dev, static_cast<O*>(out), out_denom);
}

template <int DT>
void launch_bwd(const Args& a, const void* grad_pts, const void* grad_dir, const double* denom, void* grad, hipStream_t s)
{
    using O = typename Compute<DT>::type;
    hipLaunchKernelGGL((pm_bwd_kernel<DT, O>), dim3((unsigned)(a.B * a.nqb)), dim3(kThreads), 0, s, a,
                       static_cast<const O*>(grad_pts), static_cast<const O*>(grad_dir), denom, grad);
}

}  // namespace

extern "C" {

int accv_polyline_matching_cost(const void* pred_lines, const void* gt_lines, const void* scores, const void* gt_labels,
                                const long long* counts, int dtype, unsigned flags, long long B, long long Q, long long G,
                                long long P, long long D, long long C, long long scores_stride_b, long long scores_stride_q,
                                const accv_polyline_match_params* params, void* out, void* stream)
{
    Args a;
    int empty;
    if (int rc = check_cost("polyline_matching_cost", pred_lines, gt_lines, scores, gt_labels, counts, dtype, flags, B, Q, G, P,
                            D, C, scores_stride_b, scores_stride_q, params, out, a, &empty))
        return rc;
    if (empty) return ACCV_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    int rc = ACCV_OK;
    dispatch_dtype(dtype, [&](auto dt) { rc = launch_cost<dt()>(a, params, s); });
    return rc;
}

int accv_polyline_matching_cost_host(const void* pred_lines, const void* gt_lines, const void* scores, const void* gt_labels,
                                     const long long* counts, int dtype, unsigned flags, long long B, long long Q,
                                     long long G, long long P, long long D, long long C, long long scores_stride_b,
                                     long long scores_stride_q, const accv_polyline_match_params* params, void* out)
{
    Args a;
    int empty;
    if (int rc = check_cost("polyline_matching_cost (host)", pred_lines, gt_lines, scores, gt_labels, counts, dtype, flags, B, Q,
                            G, P, D, C, scores_stride_b, scores_stride_q, params, out, a, &empty))
        return rc;
    if (empty) return ACCV_OK;
    dispatch_dtype(dtype, [&](auto dt) { cost_host<dt()>(a, make_params<typename Compute<dt()>::type>(params)); });
    return ACCV_OK;
}

size_t accv_matched_polyline_loss_workspace_bytes(long long B, long long Q)
{
    if (B <= 0 || Q <= 0) return 0;
    const long long nqb = (Q + kLossQueries - 1) / kLossQueries;
    if (nqb > accv::kGridLimit / B) return 0;
    return accv::align_up((size_t)(2 * B * nqb) * sizeof(double), 16);
}

int accv_matched_polyline_loss(const void* pred_lines, const void* gt_lines, const void* pred_ind, const void* gt_ind,
                               const long long* counts, int dtype, unsigned flags, long long B, long long Q, long long G,
                               long long P, long long D, long long K, const accv_polyline_match_params* params, void* out,
                               double* out_denom, void* workspace, size_t workspace_bytes, void* stream)
{
    const char* who = "matched_polyline_loss";
    Args a;
    int empty;
    if (int rc = check_loss(who, pred_lines, gt_lines, pred_ind, gt_ind, counts, dtype, flags, B, Q, G, P, D, K, params, true, a,
                            &empty))
        return rc;
    if (empty) return ACCV_OK;
    if (!out || !out_denom) return accv::fail(ACCV_EINVAL, "%s: null output pointer", who);
    const size_t need = accv_matched_polyline_loss_workspace_bytes(B, Q);
    if (int rc = accv::check_workspace(who, workspace, workspace_bytes, need)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    double* part = static_cast<double*>(workspace);
    dispatch_dtype(dtype, [&](auto dt) { launch_fwd<dt()>(a, params, part, out, out_denom, s); });
    return accv::check_launch(who);
}

int accv_matched_polyline_loss_bwd(const void* pred_lines, const void* gt_lines, const void* pred_ind, const void* gt_ind,
                                   const long long* counts, const void* grad_pts, const void* grad_dir, const double* denom,
                                   int dtype, unsigned flags, long long B, long long Q, long long G, long long P,
                                   long long D, long long K, const accv_polyline_match_params* params, void* grad_lines,
                                   void* stream)
{
    const char* who = "matched_polyline_loss_bwd";
    Args a;
    int empty;
    if (int rc = check_loss(who, pred_lines, gt_lines, pred_ind, gt_ind, counts, dtype, flags, B, Q, G, P, D, K, params, false, a,
                            &empty))
        return rc;
    if (empty) return ACCV_OK;
    if (!denom || !grad_lines) return accv::fail(ACCV_EINVAL, "%s: null denom / gradient pointer", who);
    if (reinterpret_cast<uintptr_t>(grad_lines) % (uintptr_t)elem_size(dtype))
        return accv::fail(ACCV_EINVAL, "%s: the gradient is not aligned to its element size", who);
    hipStream_t s = static_cast<hipStream_t>(stream);
    dispatch_dtype(dtype, [&](auto dt) { launch_bwd<dt()>(a, grad_pts, grad_dir, denom, grad_lines, s); });
    return accv::check_launch(who);
}

int accv_matched_polyline_loss_host(const void* pred_lines, const void* gt_lines, const void* pred_ind, const void* gt_ind,
                                    const long long* counts, int dtype, unsigned flags, long long B, long long Q,
                                    long long G, long long P, long long D, long long K,
                                    const accv_polyline_match_params* params, void* out, double* out_denom)
{
    const char* who = "matched_polyline_loss (host)";
    Args a;
    int empty;
    if (int rc = check_loss(who, pred_lines, gt_lines, pred_ind, gt_ind, counts, dtype, flags, B, Q, G, P, D, K, params, true, a,
                            &empty))
        return rc;
    if (empty) return ACCV_OK;
    if (!out || !out_denom) return accv::fail(ACCV_EINVAL, "%s: null output pointer", who);
    return dispatch_host(who, dtype, [&](auto dt) { host_fwd<dt()>(a, params, out, out_denom); });
}

int accv_matched_polyline_loss_bwd_host(const void* pred_lines, const void* gt_lines, const void* pred_ind,
                                        const void* gt_ind, const long long* counts, const void* grad_pts,
                                        const void* grad_dir, const double* denom, int dtype, unsigned flags, long long B,
                                        long long Q, long long G, long long P, long long D, long long K,
                                        const accv_polyline_match_params* params, void* grad_lines)
{
    const char* who = "matched_polyline_loss_bwd (host)";
    Args a;
    int empty;
    if (int rc = check_loss(who, pred_lines, gt_lines, pred_ind, gt_ind, counts, dtype, flags, B, Q, G, P, D, K, params, false, a,
                            &empty))
        return rc;
    if (empty) return ACCV_OK;
    if (!denom || !grad_lines) return accv::fail(ACCV_EINVAL, "%s: null denom / gradient pointer", who);
    return dispatch_host(who, dtype, [&](auto dt) { host_bwd<dt()>(a, grad_pts, grad_dir, denom, grad_lines); });
}

}  // extern "C"
