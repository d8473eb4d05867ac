// Sigmoid focal classification loss of a set-prediction head (DETR / StreamPETR / Focal head) over ALL queries against the
// labels of the matched ground truth, per frame:
//
//   out[b] = sum_{q, c} w[b, q] * focal(x[b, q, c], c == label_b(q)) / denom
//
// label_b(q) is the label gt_labels[b, gt_ind[b, j]] of the LOWEST slot j < clamp(counts[b], 0, K) whose pair
// (pred_ind[b, j], gt_ind[b, j]) names q with both indices in range; no such slot, or a label outside [0, C): background.
// The [B, Q, C] one-hot target of the torch composition is never built.  Per-element arithmetic: matched_focal_arith.h.
//
// Forward: a workgroup owns a range of queries of one frame.  It builds the range's query -> label table in LDS
// (the pair rule of matched_pairs.h, then the label look-up of the winning slot; no global atomics), then streams the
// range's logits — one 16-byte load per lane and step where the rows of the range are contiguous (element loads up to the
// first 16-byte boundary and after the last one), element loads for strided queries — and accumulates in a double per
// lane.  A lane finds (query, class) of its first vector with ONE 32-bit division and walks on by additions.  Wave
// shuffle + LDS give one partial per workgroup in the caller's workspace; the one-block launch of matched_pairs.h adds
// each frame's partials in a fixed order, counts the pairs, applies the denominator and leaves it on the device for the
// backward.
// Backward: the same table, then every element of the contiguous [B, Q, C] gradient written exactly once in the logits
// dtype: no zero fill, no atomics.  Neither direction synchronises; both are bitwise reproducible.
// Bandwidth / launch bound work: no MFMA.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>
#include <vector>

#include "accv_common.h"
#include "matched_focal_arith.h"
#include "matched_pairs.h"

#pragma clang fp contract(off)

namespace {

using namespace accv_mf;

constexpr int kThreads = 256;
constexpr int kMaxQ = 1024;                 // queries per workgroup the LDS tables hold
constexpr long long kTargetElems = 8192;    // elements per workgroup aimed at
constexpr unsigned kKnownFlags = ACCV_MF_IDX_I64 | ACCV_MF_LABELS_I64;

struct Args {
    const void* x;              // [B, Q, C] logits, element (b, q, c) at b * sb + q * sq + c
    const void* labels;         // [B, G]
    const void* pind;           // [B, K]
    const void* gind;           // [B, K]
    const long long* counts;    // [B]
    const void* w;              // [B, Q] or null
    long long B, Q, C, G, K, sb, sq;
    int idx64, lab64;
    int qpb;                    // queries per workgroup
    long long nqb;              // workgroups per frame
};

// label of the pair in slot j of frame b as a table entry: the class, or -1 for background
__host__ __device__ inline int label_of_slot(const Args& a, long long b, int j)
{
    const long long g = load_index(a.gind, b * a.K + j, a.idx64);   // in range: checked when the slot was entered
    const long long l = load_index(a.labels, b * a.G + g, a.lab64);
    return (l >= 0 && l < a.C) ? (int)l : -1;
}

void geometry(long long Q, long long C, int& qpb, long long& nqb)
{
    long long q = C > 0 ? kTargetElems / C : kMaxQ;
    q = q < 1 ? 1 : (q > kMaxQ ? kMaxQ : q);
    q = q > Q ? (Q > 0 ? Q : 1) : q;
    qpb = (int)q;
    nqb = (Q + q - 1) / q;
}

// ------------------------------------------------------------------------------------------------------------- device
// s_lab[i] = class of query q0 + i or -1, s_w[i] = its weight
template <int DT>
__device__ __forceinline__ void build_table(const Args& a, long long b, long long q0, int nq, int* s_lab,
                                            typename Compute<DT>::type* s_w)
{
    using F = typename Compute<DT>::type;
    const int tid = threadIdx.x;
    for (int i = tid; i < nq; i += kThreads) s_lab[i] = kNoSlot;
    __syncthreads();
    scan_pairs<kThreads>(a.pind, a.gind, a.idx64, a.counts, b, a.K, a.G, q0, nq, s_lab);
    for (int i = tid; i < nq; i += kThreads) {
        const int j = s_lab[i];
        s_lab[i] = j == kNoSlot ? -1 : label_of_slot(a, b, j);
        s_w[i] = a.w ? load<DT>(a.w, b * a.Q + q0 + i) : F(1);
    }
    __syncthreads();
}

// items i = tid, tid + kThreads, ... < n; item i starts at element e0 + i * V of the workgroup's range.  fn(i, q, c) gets
// the range-local query and the class of that element: one 32-bit division per lane, additions afterwards
template <int V, class Fn>
__device__ __forceinline__ void walk(unsigned e0, unsigned n, unsigned C, Fn&& fn)
{
    unsigned i = threadIdx.x;
    if (i >= n) return;
    const unsigned e = e0 + i * V;
    unsigned q = e / C, c = e - q * C;
    const unsigned dq = (unsigned)(kThreads * V) / C, dc = (unsigned)(kThreads * V) - dq * C;
    for (; i < n; i += kThreads) {
        fn(i, q, c);
        q += dq, c += dc;
        if (c >= C) c -= C, ++q;
    }
}

// elements before the first 16-byte boundary of a range that starts at address `addr`
template <int DT>
__device__ __forceinline__ unsigned head_of(uintptr_t addr, unsigned total)
{
    const unsigned h = (unsigned)((16u - (unsigned)(addr & 15u)) & 15u) / elem_size(DT);
    return h < total ? h : total;
}

template <int DT, bool G2>
__global__ __launch_bounds__(kThreads) void mf_fwd_kernel(const Args a, const Coef<typename Compute<DT>::type> k,
                                                          double* __restrict__ part)
{
    using F = typename Compute<DT>::type;
    constexpr int V = 16 / elem_size(DT);   // elements of a 16-byte access
    __shared__ int s_lab[kMaxQ];
    __shared__ F s_w[kMaxQ];
    const Range r = range_of(a.nqb, a.qpb, a.Q);
    const unsigned total = (unsigned)r.nq * (unsigned)a.C;   // elements of the range
    build_table<DT>(a, r.b, r.q0, r.nq, s_lab, s_w);
    const unsigned C = (unsigned)a.C;
    const long long first = r.b * a.sb + r.q0 * a.sq;   // element offset of the range's first logit
    double acc = 0.0;
    auto one = [&](F x, unsigned q, unsigned c) { acc += (double)(s_w[q] * focal_value<F, G2>(x, (int)c == s_lab[q], k)); };
    if (a.sq == a.C) {
        const char* base = static_cast<const char*>(a.x) + first * elem_size(DT);
        const unsigned head = head_of<DT>(reinterpret_cast<uintptr_t>(base), total);
        const unsigned nvec = (total - head) / V, tail0 = head + nvec * V;
        walk<V>(head, nvec, C, [&](unsigned i, unsigned q, unsigned c) {
            const uint4 v = *reinterpret_cast<const uint4*>(base + ((size_t)head + (size_t)i * V) * elem_size(DT));
            F x[V];
            decode<DT>(v, x);
#pragma unroll
            for (int e = 0; e < V; ++e) {
                one(x[e], q, c);
                if (++c == C) c = 0, ++q;
            }
        });
        // at most V - 1 elements on either side of the vectors
        const unsigned t = threadIdx.x;
        if (t < head) one(load<DT>(a.x, first + t), t / C, t % C);
        if (t < total - tail0) one(load<DT>(a.x, first + tail0 + t), (tail0 + t) / C, (tail0 + t) % C);
    } else {
        walk<1>(0u, total, C, [&](unsigned, unsigned q, unsigned c) { one(load<DT>(a.x, first + (long long)q * a.sq + c), q, c); });
    }
    acc = block_sum<double, kThreads>(acc);
    if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

template <int DT, bool G2, class O>
__global__ __launch_bounds__(kThreads) void mf_bwd_kernel(const Args a, const Coef<typename Compute<DT>::type> k,
                                                          const O* __restrict__ grad_out, const double* __restrict__ denom,
                                                          void* __restrict__ grad)
{
    using F = typename Compute<DT>::type;
    constexpr int V = 16 / elem_size(DT);   // elements of a 16-byte access
    __shared__ int s_lab[kMaxQ];
    __shared__ F s_w[kMaxQ];
    const Range r = range_of(a.nqb, a.qpb, a.Q);
    const unsigned total = (unsigned)r.nq * (unsigned)a.C;   // elements of the range
    build_table<DT>(a, r.b, r.q0, r.nq, s_lab, s_w);
    const unsigned C = (unsigned)a.C;
    const long long first = r.b * a.sb + r.q0 * a.sq;
    const long long gfirst = (r.b * a.Q + r.q0) * a.C;   // the gradient is contiguous
    const F scale = (F)((double)grad_out[r.b] / *denom);
    auto one = [&](F x, unsigned q, unsigned c) -> F { return (s_w[q] * focal_grad<F, G2>(x, (int)c == s_lab[q], k)) * scale; };
    const char* base = static_cast<const char*>(a.x) + first * elem_size(DT);
    char* gbase = static_cast<char*>(grad) + gfirst * elem_size(DT);
    const bool same = ((reinterpret_cast<uintptr_t>(base) ^ reinterpret_cast<uintptr_t>(gbase)) & 15u) == 0;
    if (a.sq == a.C && same) {
        const unsigned head = head_of<DT>(reinterpret_cast<uintptr_t>(base), total);
        const unsigned nvec = (total - head) / V, tail0 = head + nvec * V;
        walk<V>(head, nvec, C, [&](unsigned i, unsigned q, unsigned c) {
            const size_t at = ((size_t)head + (size_t)i * V) * elem_size(DT);
            const uint4 v = *reinterpret_cast<const uint4*>(base + at);
            F x[V], g[V];
            decode<DT>(v, x);
#pragma unroll
            for (int e = 0; e < V; ++e) {
                g[e] = one(x[e], q, c);
                if (++c == C) c = 0, ++q;
            }
            *reinterpret_cast<uint4*>(gbase + at) = encode<DT>(g);
        });
        const unsigned t = threadIdx.x;
        if (t < head) store<DT>(grad, gfirst + t, one(load<DT>(a.x, first + t), t / C, t % C));
        if (t < total - tail0)
            store<DT>(grad, gfirst + tail0 + t, one(load<DT>(a.x, first + tail0 + t), (tail0 + t) / C, (tail0 + t) % C));
    } else {
        walk<1>(0u, total, C, [&](unsigned i, unsigned q, unsigned c) {
            store<DT>(grad, gfirst + i, one(load<DT>(a.x, first + (long long)q * a.sq + c), q, c));
        });
    }
}

// --------------------------------------------------------------------------------------------------------------- host
// the table of a whole frame: tab[q] = class or -1
void host_table(const Args& a, long long b, std::vector<int>& tab)
{
    host_pair_table(a.pind, a.gind, a.idx64, a.counts, b, a.K, a.Q, a.G, tab);
    for (int& t : tab) t = t == kNoSlot ? -1 : label_of_slot(a, b, t);
}

template <int DT, bool G2, class O>
void host_fwd(const Args& a, const accv_matched_focal_params* p, O* out, double* out_denom)
{
    using F = typename Compute<DT>::type;
    const Coef<F> k = make_coef<F>(p->alpha, p->gamma);
    const double denom = host_denom(a.counts, a.B, a.K, p->avg_mode, p->avg_factor, p->avg_factor_dev);
    std::vector<int> tab;
    for (long long b = 0; b < a.B; ++b) {
        host_table(a, b, tab);
        double acc = 0.0;
        for (long long q = 0; q < a.Q; ++q) {
            const F w = a.w ? load<DT>(a.w, b * a.Q + q) : F(1);
            const int lab = tab[(size_t)q];
            for (long long c = 0; c < a.C; ++c)
                acc += (double)(w * focal_value<F, G2>(load<DT>(a.x, b * a.sb + q * a.sq + c), c == lab, k));
        }
        out[b] = (O)(acc / denom);
    }
    *out_denom = denom;
}

template <int DT, bool G2, class O>
void host_bwd(const Args& a, const accv_matched_focal_params* p, const O* grad_out, const double* denom, void* grad)
{
    using F = typename Compute<DT>::type;
    const Coef<F> k = make_coef<F>(p->alpha, p->gamma);
    std::vector<int> tab;
    for (long long b = 0; b < a.B; ++b) {
        host_table(a, b, tab);
        const F scale = (F)((double)grad_out[b] / *denom);
        for (long long q = 0; q < a.Q; ++q) {
            const F w = a.w ? load<DT>(a.w, b * a.Q + q) : F(1);
            const int lab = tab[(size_t)q];
            for (long long c = 0; c < a.C; ++c)
                store<DT>(grad, (b * a.Q + q) * a.C + c,
                          (w * focal_grad<F, G2>(load<DT>(a.x, b * a.sb + q * a.sq + c), c == lab, k)) * scale);
        }
    }
}

// ------------------------------------------------------------------------------------------------------------- checks
// ACCV_OK with *empty = 1 when there is no logit; every check runs before anything else reads the arguments
int check_args(const char* who, const void* logits, const void* labels, const void* pind, const void* gind,
               const long long* counts, int dtype, unsigned flags, long long B, long long Q, long long C, long long G,
               long long K, long long sb, long long sq, const accv_matched_focal_params* p, bool forward, Args& a, int* empty)
{
    *empty = 0;
    if (int rc = check_pair_sizes(who, p, {B, Q, C, G, K}, dtype, flags, kKnownFlags)) return rc;
    if (!(p->gamma >= 0.0)) return accv::fail(ACCV_EINVAL, "%s: needs gamma >= 0 (got %g)", who, p->gamma);
    if (p->alpha != p->alpha) return accv::fail(ACCV_EINVAL, "%s: alpha is NaN", who);
    if (int rc = check_pair_mode(who, forward, p->avg_mode, K, C, "C and K are")) return rc;
    if (B == 0 || Q == 0 || C == 0) {
        *empty = 1;
        return ACCV_OK;
    }
    if (sq < C || sb < 0) return accv::fail(ACCV_EINVAL, "%s: query stride %lld below C = %lld, or negative batch stride", who, sq, C);
    if (int rc = check_pair_pointers(who, logits != nullptr, "logits / counts", counts, pind, gind, K)) return rc;
    if (K > 0 && G > 0 && !labels) return accv::fail(ACCV_EINVAL, "%s: null labels pointer", who);
    if (reinterpret_cast<uintptr_t>(logits) % (uintptr_t)elem_size(dtype)) return accv::fail(ACCV_EINVAL, "%s: logits are not aligned to their element size", who);
    a.x = logits, a.labels = labels, a.pind = pind, a.gind = gind, a.counts = counts, a.w = nullptr;
    a.B = B, a.Q = Q, a.C = C, a.G = G, a.K = K, a.sb = sb, a.sq = sq;
    a.idx64 = (flags & ACCV_MF_IDX_I64) ? 1 : 0, a.lab64 = (flags & ACCV_MF_LABELS_I64) ? 1 : 0;
    geometry(Q, C, a.qpb, a.nqb);
    return check_pair_launch(who, forward, p->avg_mode, p->avg_factor_dev, B, a.nqb);
}

template <int DT>
void launch_fwd(const Args& a, const accv_matched_focal_params* p, double* part, void* out, double* out_denom, hipStream_t s)
{
    using F = typename Compute<DT>::type;
    using O = typename Compute<DT>::type;
    const Coef<F> k = make_coef<F>(p->alpha, p->gamma);
    const dim3 grid((unsigned)(a.B * a.nqb)), block(kThreads);
    if (p->gamma == 2.0) hipLaunchKernelGGL((mf_fwd_kernel<DT, true>), grid, block, 0, s, a, k, part);
    else hipLaunchKernelGGL((mf_fwd_kernel<DT, false>), grid, block, 0, s, a, k, part);
    hipLaunchKernelGGL((pair_finish_kernel<1, O>), dim3(1), dim3(kFinishThreads), 0, s, part, a.counts, a.B, a.nqb, a.K, p->avg_mode,
                       p->avg_factor, p->avg_factor_dev, static_cast<O*>(out), out_denom);
}

template <int DT>
void launch_bwd(const Args& a, const accv_matched_focal_params* p, const void* grad_out, const double* denom, void* grad,
                hipStream_t s)
{
    using F = typename Compute<DT>::type;
    using O = typename Compute<DT>::type;
    const Coef<F> k = make_coef<F>(p->alpha, p->gamma);
    const dim3 grid((unsigned)(a.B * a.nqb)), block(kThreads);
    const O* go = static_cast<const O*>(grad_out);
    if (p->gamma == 2.0) hipLaunchKernelGGL((mf_bwd_kernel<DT, true, O>), grid, block, 0, s, a, k, go, denom, grad);
    else hipLaunchKernelGGL((mf_bwd_kernel<DT, false, O>), grid, block, 0, s, a, k, go, denom, grad);
}

template <int DT>
void run_host_fwd(const Args& a, const accv_matched_focal_params* p, void* out, double* out_denom)
{
    using O = typename Compute<DT>::type;
    if (p->gamma == 2.0) host_fwd<DT, true, O>(a, p, static_cast<O*>(out), out_denom);
    else host_fwd<DT, false, O>(a, p, static_cast<O*>(out), out_denom);
}
template <int DT>
void run_host_bwd(const Args& a, const accv_matched_focal_params* p, const void* grad_out, const double* denom, void* grad)
{
    using O = typename Compute<DT>::type;
    if (p->gamma == 2.0) host_bwd<DT, true, O>(a, p, static_cast<const O*>(grad_out), denom, grad);
    else host_bwd<DT, false, O>(a, p, static_cast<const O*>(grad_out), denom, grad);
}

}  // namespace

extern "C" {

size_t accv_matched_focal_loss_workspace_bytes(long long B, long long Q, long long C)
{
    if (B <= 0 || Q <= 0 || C <= 0) return 0;
    int qpb;
    long long nqb;
    geometry(Q, C, qpb, nqb);
    if (nqb > accv::kGridLimit / B) return 0;
    return accv::align_up((size_t)(B * nqb) * sizeof(double), 16);
}

int accv_matched_focal_loss(const void* logits, const void* gt_labels, const void* pred_ind, const void* gt_ind,
                            const long long* counts, const void* query_weights_or_null, int dtype, unsigned flags,
                            long long B, long long Q, long long C, long long G, long long K, long long stride_b,
                            long long stride_q, const accv_matched_focal_params* params, void* out, double* out_denom,
                            void* workspace, size_t workspace_bytes, void* stream)
{
    const char* who = "matched_focal_loss";
    Args a;
    int empty;
    if (int rc = check_args(who, logits, gt_labels, pred_ind, gt_ind, counts, dtype, flags, B, Q, C, G, K, stride_b, stride_q,
                            params, true, a, &empty))
        return rc;
    if (empty) return ACCV_OK;
    a.w = query_weights_or_null;
    if (!out || !out_denom) return accv::fail(ACCV_EINVAL, "%s: null output pointer", who);
    const size_t need = accv_matched_focal_loss_workspace_bytes(B, Q, C);
    if (int rc = accv::check_workspace(who, workspace, workspace_bytes, need)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    double* part = static_cast<double*>(workspace);
    dispatch_dtype(dtype, [&](auto dt) { launch_fwd<dt()>(a, params, part, out, out_denom, s); });
    return accv::check_launch(who);
}

int accv_matched_focal_loss_bwd(const void* logits, const void* gt_labels, const void* pred_ind, const void* gt_ind,
                                const long long* counts, const void* query_weights_or_null, const void* grad_out,
                                const double* denom, int dtype, unsigned flags, long long B, long long Q, long long C,
                                long long G, long long K, long long stride_b, long long stride_q,
                                const accv_matched_focal_params* params, void* grad_logits, void* stream)
{
    const char* who = "matched_focal_loss_bwd";
    Args a;
    int empty;
    if (int rc = check_args(who, logits, gt_labels, pred_ind, gt_ind, counts, dtype, flags, B, Q, C, G, K, stride_b, stride_q,
                            params, false, a, &empty))
        return rc;
    if (empty) return ACCV_OK;
    a.w = query_weights_or_null;
    if (!grad_out || !denom || !grad_logits) return accv::fail(ACCV_EINVAL, "%s: null grad_out / denom / gradient pointer", who);
    if (reinterpret_cast<uintptr_t>(grad_logits) % (uintptr_t)elem_size(dtype))
        return accv::fail(ACCV_EINVAL, "%s: the gradient is not aligned to its element size", who);
    hipStream_t s = static_cast<hipStream_t>(stream);
    dispatch_dtype(dtype, [&](auto dt) { launch_bwd<dt()>(a, params, grad_out, denom, grad_logits, s); });
    return accv::check_launch(who);
}

int accv_matched_focal_loss_host(const void* logits, const void* gt_labels, const void* pred_ind, const void* gt_ind,
                                 const long long* counts, const void* query_weights_or_null, int dtype, unsigned flags,
                                 long long B, long long Q, long long C, long long G, long long K, long long stride_b,
                                 long long stride_q, const accv_matched_focal_params* params, void* out, double* out_denom)
{
    const char* who = "matched_focal_loss (host)";
    Args a;
    int empty;
    if (int rc = check_args(who, logits, gt_labels, pred_ind, gt_ind, counts, dtype, flags, B, Q, C, G, K, stride_b, stride_q,
                            params, true, a, &empty))
        return rc;
    if (empty) return ACCV_OK;
    a.w = query_weights_or_null;
    if (!out || !out_denom) return accv::fail(ACCV_EINVAL, "%s: null output pointer", who);
    return dispatch_host(who, dtype, [&](auto dt) { run_host_fwd<dt()>(a, params, out, out_denom); });
}

int accv_matched_focal_loss_bwd_host(const void* logits, const void* gt_labels, const void* pred_ind, const void* gt_ind,
                                     const long long* counts, const void* query_weights_or_null, const void* grad_out,
                                     const double* denom, int dtype, unsigned flags, long long B, long long Q, long long C,
                                     long long G, long long K, long long stride_b, long long stride_q,
                                     const accv_matched_focal_params* params, void* grad_logits)
{
    const char* who = "matched_focal_loss_bwd (host)";
    Args a;
    int empty;
    if (int rc = check_args(who, logits, gt_labels, pred_ind, gt_ind, counts, dtype, flags, B, Q, C, G, K, stride_b, stride_q,
                            params, false, a, &empty))
        return rc;
    if (empty) return ACCV_OK;
    a.w = query_weights_or_null;
    if (!grad_out || !denom || !grad_logits) return accv::fail(ACCV_EINVAL, "%s: null grad_out / denom / gradient pointer", who);
    return dispatch_host(who, dtype, [&](auto dt) { run_host_bwd<dt()>(a, params, grad_out, denom, grad_logits); });
}

}  // extern "C"
