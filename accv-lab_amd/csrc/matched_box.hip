// Box regression loss of a set-prediction head (DETR / Deformable-DETR / StreamPETR) over the matched pairs, per frame:
//
//   out[0][b] = sum_pairs w[b, q] * sum_d cw[d] |p[b, q, d] - g[b, gi, d]| / denom
//   out[1][b] = sum_pairs w[b, q] * (1 - giou(p, g))  or  (1 - iou(p, g)) / denom          (D == 4; zeros without an IoU kind)
//
// The pair of query q in frame b is the LOWEST slot j < clamp(counts[b], 0, K) whose (pred_ind[b, j], gt_ind[b, j]) names q
// with both indices in range — the rule of matched_pairs.h, which matched_focal.hip reads too, so the two losses see the
// same pairs.  Per-pair arithmetic: matched_box_arith.h.
//
// Forward: a workgroup owns kThreads consecutive queries of one frame.  It builds their query -> slot table in LDS
// (scan_pairs of matched_pairs.h; no global atomics); a lane per query looks its pair up, evaluates both terms and
// the workgroup sums them in f64 in a fixed order: one (l1, iou) partial per workgroup in the caller's workspace.  A
// one-block launch (matched_pairs.h) adds each frame's partials in a fixed order, counts the pairs, applies the
// denominator and leaves it on the device for the backward.
// Backward: the same table, then every element of the contiguous [B, Q, D] gradient written exactly once in the boxes'
// dtype, +0 for a query without a pair: no zero fill, no atomics, no read of the gradient.  D == 4: a lane per query and
// one store per row (16 bytes f32, 8 bytes f16 / bf16, 2 x 16 bytes f64) where the gradient's base allows it; other D: a
// lane per element, consecutive lanes on consecutive addresses.
// Neither direction synchronises; both are bitwise reproducible.  Launch bound work: no MFMA.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>
#include <vector>

#include "accv_common.h"
#include "matched_box_arith.h"
#include "matched_pairs.h"

#pragma clang fp contract(off)

namespace {

using namespace accv_mb;

constexpr int kThreads = 256;               // and queries per workgroup
constexpr unsigned kKnownFlags = ACCV_MB_IDX_I64 | ACCV_MB_CXCYWH;

struct Args {
    const void* p;              // [B, Q, D] predictions, element (b, q, d) at b * sb + q * sq + d
    const void* g;              // [B, G, D] ground truth, contiguous
    const void* pind;           // [B, K]
    const void* gind;           // [B, K]
    const long long* counts;    // [B]
    const void* w;              // [B, Q] or null
    const void* cw_dev;         // [D] or null: then cw
    double cw[kMaxD];
    double eps;
    long long B, Q, D, G, K, sb, sq;
    long long nqb;              // workgroups per frame
    int idx64, cxcywh, kind;
};

template <int DT>
__host__ __device__ inline typename Compute<DT>::type code_weight(const Args& a, int d)
{
    using F = typename Compute<DT>::type;
    return a.cw_dev ? load<DT>(a.cw_dev, d) : (F)a.cw[d];
}

// the two terms of the pair (query q, object g) of frame b, without the query weight
template <int DT>
__host__ __device__ inline void pair_value(const Args& a, long long b, long long q, long long g, const typename Compute<DT>::type* cw,
                                           typename Compute<DT>::type& l1, typename Compute<DT>::type& iou)
{
    using F = typename Compute<DT>::type;
    const long long po = b * a.sb + q * a.sq, go = (b * a.G + g) * a.D;
    l1 = F(0), iou = F(0);
    if (a.kind != kIouNone) {   // D == 4
        F bp[4], bg[4], xg[4];
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            bp[d] = load<DT>(a.p, po + d), bg[d] = load<DT>(a.g, go + d);
            l1 = l1 + l1_value(bp[d], bg[d], cw[d]);
        }
        to_xyxy(bg, a.cxcywh, xg);
        iou = iou_value(bp, xg, a.cxcywh, a.kind, (F)a.eps);
    } else {
        for (int d = 0; d < (int)a.D; ++d) l1 = l1 + l1_value(load<DT>(a.p, po + d), load<DT>(a.g, go + d), cw[d]);
    }
}

// the four gradient components of a D == 4 pair: (s1 * dL1 + s2 * dIoU) * w
template <int DT>
__host__ __device__ inline void pair_grad4(const Args& a, long long b, long long q, long long g, const typename Compute<DT>::type* cw,
                                           typename Compute<DT>::type s1, typename Compute<DT>::type s2,
                                           typename Compute<DT>::type w, typename Compute<DT>::type* out)
{
    using F = typename Compute<DT>::type;
    const long long po = b * a.sb + q * a.sq, go = (b * a.G + g) * a.D;
    F bp[4], bg[4], di[4] = {F(0), F(0), F(0), F(0)};
#pragma unroll
    for (int d = 0; d < 4; ++d) bp[d] = load<DT>(a.p, po + d), bg[d] = load<DT>(a.g, go + d);
    if (a.kind != kIouNone) {
        F xg[4];
        to_xyxy(bg, a.cxcywh, xg);
        iou_grad(bp, xg, a.cxcywh, a.kind, (F)a.eps, di);
    }
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const F t = s1 * l1_grad(bp[d], bg[d], cw[d]);
        out[d] = (a.kind != kIouNone ? t + s2 * di[d] : t) * w;
    }
}

// one gradient element of an L1-only pair
template <int DT>
__host__ __device__ inline typename Compute<DT>::type elem_grad(const Args& a, long long b, long long q, long long g, int d,
                                                                 typename Compute<DT>::type cw, typename Compute<DT>::type s1,
                                                                 typename Compute<DT>::type w)
{
    return (s1 * l1_grad(load<DT>(a.p, b * a.sb + q * a.sq + d), load<DT>(a.g, (b * a.G + g) * a.D + d), cw)) * w;
}

// ------------------------------------------------------------------------------------------------------------- device
// s_slot[i] = the slot of the pair of query q0 + i, or kNoSlot; s_cw[d] = the code weight of coordinate d
template <int DT>
__device__ __forceinline__ void build_table(const Args& a, long long b, long long q0, int nq, int* s_slot,
                                            typename Compute<DT>::type* s_cw)
{
    const int tid = threadIdx.x;
    s_slot[tid] = kNoSlot;
    if (tid < kMaxD) s_cw[tid] = tid < a.D ? code_weight<DT>(a, tid) : typename Compute<DT>::type(0);
    __syncthreads();
    scan_pairs<kThreads>(a.pind, a.gind, a.idx64, a.counts, b, a.K, a.G, q0, nq, s_slot);
}

template <int DT>
__global__ __launch_bounds__(kThreads) void mb_fwd_kernel(const Args a, double* __restrict__ part)
{
    using F = typename Compute<DT>::type;
    __shared__ int s_slot[kThreads];
    __shared__ F s_cw[kMaxD];
    const Range r = range_of(a.nqb, kThreads, a.Q);
    build_table<DT>(a, r.b, r.q0, r.nq, s_slot, s_cw);
    double l1 = 0.0, iou = 0.0;
    const int j = s_slot[threadIdx.x];   // kNoSlot at and past nq
    if (j != kNoSlot) {
        const long long q = r.q0 + threadIdx.x;
        const long long g = load_index(a.gind, r.b * a.K + j, a.idx64);   // in range: checked when the slot was entered
        const F w = a.w ? load<DT>(a.w, r.b * a.Q + q) : F(1);
        F v1, v2;
        pair_value<DT>(a, r.b, q, g, s_cw, v1, v2);
        l1 = (double)(w * v1), iou = (double)(w * v2);
    }
    block_sum<double, double, kThreads>(l1, iou);
    if (threadIdx.x == 0) {
        part[blockIdx.x] = l1;
        part[(size_t)gridDim.x + blockIdx.x] = iou;
    }
}

// a D == 4 gradient row in one store where `aligned` (the base of the gradient allows it) says so
template <int DT>
__device__ __forceinline__ void store_row4(void* grad, long long row, const typename Compute<DT>::type (&v)[4], bool aligned)
{
    if (!aligned) {
#pragma unroll
        for (int d = 0; d < 4; ++d) store<DT>(grad, row * 4 + d, v[d]);
        return;
    }
    if constexpr (DT == kF32) {
        reinterpret_cast<uint4*>(grad)[row] = encode<DT>(v);
    } else if constexpr (DT == kF64) {
        const double lo[2] = {v[0], v[1]}, hi[2] = {v[2], v[3]};
        reinterpret_cast<uint4*>(grad)[row * 2] = encode<DT>(lo);
        reinterpret_cast<uint4*>(grad)[row * 2 + 1] = encode<DT>(hi);
    } else {
        uint16_t h[4];
#pragma unroll
        for (int d = 0; d < 4; ++d) h[d] = DT == kF16 ? float_to_half_bits(v[d]) : float_to_bf16_bits(v[d]);
        reinterpret_cast<uint2*>(grad)[row] = make_uint2((unsigned)h[0] | ((unsigned)h[1] << 16), (unsigned)h[2] | ((unsigned)h[3] << 16));
    }
}

template <int DT, class O>
__global__ __launch_bounds__(kThreads) void mb_bwd_kernel(const Args a, const O* __restrict__ grad_l1,
                                                          const O* __restrict__ grad_iou, const double* __restrict__ denom,
                                                          void* __restrict__ grad)
{
    using F = typename Compute<DT>::type;
    __shared__ int s_slot[kThreads];
    __shared__ F s_cw[kMaxD];
    const Range r = range_of(a.nqb, kThreads, a.Q);
    build_table<DT>(a, r.b, r.q0, r.nq, s_slot, s_cw);
    const double dn = *denom;
    const F s1 = grad_l1 ? (F)((double)grad_l1[r.b] / dn) : F(0), s2 = grad_iou ? (F)((double)grad_iou[r.b] / dn) : F(0);
    if (a.D == 4) {
        const int i = threadIdx.x;
        if (i >= r.nq) return;
        const long long q = r.q0 + i;
        const int j = s_slot[i];
        F v[4] = {F(0), F(0), F(0), F(0)};
        if (j != kNoSlot) {
            const long long g = load_index(a.gind, r.b * a.K + j, a.idx64);
            const F w = a.w ? load<DT>(a.w, r.b * a.Q + q) : F(1);
            pair_grad4<DT>(a, r.b, q, g, s_cw, s1, s2, w, v);
        }
        const bool aligned = (reinterpret_cast<uintptr_t>(grad) & (DT == kF16 || DT == kBF16 ? 7u : 15u)) == 0;
        store_row4<DT>(grad, r.b * a.Q + q, v, aligned);
        return;
    }
    // L1 only: a lane per element of the workgroup's nq x D block of the gradient
    const unsigned D = (unsigned)a.D, total = (unsigned)r.nq * D;
    const long long first = (r.b * a.Q + r.q0) * a.D;
    for (unsigned e = threadIdx.x; e < total; e += kThreads) {
        const unsigned i = e / D, d = e - i * D;
        const int j = s_slot[i];
        F v = F(0);
        if (j != kNoSlot) {
            const long long q = r.q0 + i;
            const long long g = load_index(a.gind, r.b * a.K + j, a.idx64);
            const F w = a.w ? load<DT>(a.w, r.b * a.Q + q) : F(1);
            v = elem_grad<DT>(a, r.b, q, g, (int)d, s_cw[d], s1, w);
        }
        store<DT>(grad, first + e, v);
    }
}

// --------------------------------------------------------------------------------------------------------------- host
// the table of a whole frame: tab[q] = slot or kNoSlot
void host_table(const Args& a, long long b, std::vector<int>& tab)
{
    host_pair_table(a.pind, a.gind, a.idx64, a.counts, b, a.K, a.Q, a.G, tab);
}

template <int DT>
void host_fwd(const Args& a, const accv_matched_box_params* p, void* out_v, double* out_denom)
{
    using F = typename Compute<DT>::type;
    F* out = static_cast<F*>(out_v);
    const double denom = host_denom(a.counts, a.B, a.K, p->avg_mode, p->avg_factor, p->avg_factor_dev);
    F cw[kMaxD];
    for (int d = 0; d < kMaxD; ++d) cw[d] = d < a.D ? code_weight<DT>(a, d) : F(0);
    std::vector<int> tab;
    for (long long b = 0; b < a.B; ++b) {
        host_table(a, b, tab);
        double l1 = 0.0, iou = 0.0;
        for (long long q = 0; q < a.Q; ++q) {
            const int j = tab[(size_t)q];
            if (j == kNoSlot) continue;
            const long long g = load_index(a.gind, b * a.K + j, a.idx64);
            const F w = a.w ? load<DT>(a.w, b * a.Q + q) : F(1);
            F v1, v2;
            pair_value<DT>(a, b, q, g, cw, v1, v2);
            l1 += (double)(w * v1), iou += (double)(w * v2);
        }
        out[b] = (F)(l1 / denom), out[a.B + b] = (F)(iou / denom);
    }
    *out_denom = denom;
}

template <int DT>
void host_bwd(const Args& a, const void* grad_l1_v, const void* grad_iou_v, const double* denom, void* grad)
{
    using F = typename Compute<DT>::type;
    const F* grad_l1 = static_cast<const F*>(grad_l1_v);
    const F* grad_iou = static_cast<const F*>(grad_iou_v);
    F cw[kMaxD];
    for (int d = 0; d < kMaxD; ++d) cw[d] = d < a.D ? code_weight<DT>(a, d) : F(0);
    std::vector<int> tab;
    for (long long b = 0; b < a.B; ++b) {
        host_table(a, b, tab);
        const F s1 = grad_l1 ? (F)((double)grad_l1[b] / *denom) : F(0), s2 = grad_iou ? (F)((double)grad_iou[b] / *denom) : F(0);
        for (long long q = 0; q < a.Q; ++q) {
            const int j = tab[(size_t)q];
            const long long row = (b * a.Q + q) * a.D;
            if (j == kNoSlot) {
                for (int d = 0; d < (int)a.D; ++d) store<DT>(grad, row + d, F(0));
                continue;
            }
            const long long g = load_index(a.gind, b * a.K + j, a.idx64);
            const F w = a.w ? load<DT>(a.w, b * a.Q + q) : F(1);
            if (a.D == 4) {
                F v[4];
                pair_grad4<DT>(a, b, q, g, cw, s1, s2, w, v);
                for (int d = 0; d < 4; ++d) store<DT>(grad, row + d, v[d]);
            } else {
                for (int d = 0; d < (int)a.D; ++d) store<DT>(grad, row + d, elem_grad<DT>(a, b, q, g, d, cw[d], s1, w));
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------- checks
// ACCV_OK with *empty = 1 when there is no prediction; every check runs before anything else reads the arguments
int check_args(const char* who, const void* pred, const void* gt, const void* pind, const void* gind, const long long* counts,
               int dtype, unsigned flags, long long B, long long Q, long long D, long long G, long long K, long long sb,
               long long sq, const accv_matched_box_params* p, bool forward, Args& a, int* empty)
{
    *empty = 0;
    if (int rc = check_pair_sizes(who, p, {B, Q, D, G, K}, dtype, flags, kKnownFlags)) return rc;
    if (p->iou_kind < ACCV_MB_IOU_NONE || p->iou_kind > ACCV_MB_GIOU)
        return accv::fail(ACCV_EINVAL, "%s: unknown IoU kind %d", who, p->iou_kind);
    if (int rc = check_pair_mode(who, forward, p->avg_mode, K, 0, "K is")) return rc;
    if (B == 0 || Q == 0) {
        *empty = 1;
        return ACCV_OK;
    }
    if (D < 1 || D > kMaxD) return accv::fail(ACCV_EINVAL, "%s: needs 1 <= D <= %d (got %lld)", who, kMaxD, D);
    if (p->iou_kind != ACCV_MB_IOU_NONE && D != 4) return accv::fail(ACCV_EINVAL, "%s: an IoU kind needs D == 4 (got %lld)", who, D);
    if (sq < D || sb < 0) return accv::fail(ACCV_EINVAL, "%s: query stride %lld below D = %lld, or negative batch stride", who, sq, D);
    if (int rc = check_pair_pointers(who, pred != nullptr, "boxes / counts", counts, pind, gind, K)) return rc;
    if (K > 0 && G > 0 && !gt) return accv::fail(ACCV_EINVAL, "%s: null ground-truth pointer", who);
    if (reinterpret_cast<uintptr_t>(pred) % (uintptr_t)elem_size(dtype) || reinterpret_cast<uintptr_t>(gt) % (uintptr_t)elem_size(dtype))
        return accv::fail(ACCV_EINVAL, "%s: boxes are not aligned to their element size", who);
    a.p = pred, a.g = gt, a.pind = pind, a.gind = gind, a.counts = counts;
    a.w = p->query_weights, a.cw_dev = p->code_weights_dev;
    for (int d = 0; d < kMaxD; ++d) a.cw[d] = p->code_weights[d];
    a.eps = p->iou_eps;
    a.B = B, a.Q = Q, a.D = D, a.G = G, a.K = K, a.sb = sb, a.sq = sq;
    a.nqb = (Q + kThreads - 1) / kThreads;
    a.idx64 = (flags & ACCV_MB_IDX_I64) ? 1 : 0, a.cxcywh = (flags & ACCV_MB_CXCYWH) ? 1 : 0, a.kind = p->iou_kind;
    if (int rc = check_pair_launch(who, forward, p->avg_mode, p->avg_factor_dev, B, a.nqb)) return rc;
    if (Q > LLONG_MAX / D / B) return accv::fail(ACCV_EINVAL, "%s: B x Q x D overflows", who);
    return ACCV_OK;
}

template <int DT>
void launch_fwd(const Args& a, const accv_matched_box_params* p, double* part, void* out, double* out_denom, hipStream_t s)
{
    using O = typename Compute<DT>::type;
    hipLaunchKernelGGL(mb_fwd_kernel<DT>, dim3((unsigned)(a.B * a.nqb)), dim3(kThreads), 0, s, a, part);
    hipLaunchKernelGGL((pair_finish_kernel<2, O>), dim3(1), dim3(kFinishThreads), 0, s, part, a.counts, a.B, a.nqb, a.K, p->avg_mode,
                       p->avg_factor, p->avg_factor_dev, static_cast<O*>(out), out_denom);
}

template <int DT>
void launch_bwd(const Args& a, const void* grad_l1, const void* grad_iou, const double* denom, void* grad, hipStream_t s)
{
    using O = typename Compute<DT>::type;
    hipLaunchKernelGGL((mb_bwd_kernel<DT, O>), dim3((unsigned)(a.B * a.nqb)), dim3(kThreads), 0, s, a,
                       static_cast<const O*>(grad_l1), static_cast<const O*>(grad_iou), denom, grad);
}

}  // namespace

extern "C" {

size_t accv_matched_box_loss_workspace_bytes(long long B, long long Q, long long D)
{
    if (B <= 0 || Q <= 0 || D <= 0) return 0;
    const long long nqb = (Q + kThreads - 1) / kThreads;
    if (nqb > accv::kGridLimit / B) return 0;
    return accv::align_up((size_t)(2 * B * nqb) * sizeof(double), 16);
}

int accv_matched_box_loss(const void* pred_boxes, const void* gt_boxes, const void* pred_ind, const void* gt_ind,
                          const long long* counts, int dtype, unsigned flags, long long B, long long Q, long long D, long long G,
                          long long K, long long stride_b, long long stride_q, const accv_matched_box_params* params, void* out,
                          double* out_denom, void* workspace, size_t workspace_bytes, void* stream)
{
    const char* who = "matched_box_loss";
    Args a;
    int empty;
    if (int rc = check_args(who, pred_boxes, gt_boxes, pred_ind, gt_ind, counts, dtype, flags, B, Q, D, G, K, stride_b, stride_q,
                            params, true, a, &empty))
        return rc;
    if (empty) return ACCV_OK;
    if (!out || !out_denom) return accv::fail(ACCV_EINVAL, "%s: null output pointer", who);
    const size_t need = accv_matched_box_loss_workspace_bytes(B, Q, D);
    if (int rc = accv::check_workspace(who, workspace, workspace_bytes, need)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    double* part = static_cast<double*>(workspace);
    dispatch_dtype(dtype, [&](auto dt) { launch_fwd<dt()>(a, params, part, out, out_denom, s); });
    return accv::check_launch(who);
}

int accv_matched_box_loss_bwd(const void* pred_boxes, const void* gt_boxes, const void* pred_ind, const void* gt_ind,
                              const long long* counts, const void* grad_l1, const void* grad_iou, const double* denom, int dtype,
                              unsigned flags, long long B, long long Q, long long D, long long G, long long K, long long stride_b,
                              long long stride_q, const accv_matched_box_params* params, void* grad_boxes, void* stream)
{
    const char* who = "matched_box_loss_bwd";
    Args a;
    int empty;
    if (int rc = check_args(who, pred_boxes, gt_boxes, pred_ind, gt_ind, counts, dtype, flags, B, Q, D, G, K, stride_b, stride_q,
                            params, false, a, &empty))
        return rc;
    if (empty) return ACCV_OK;
    if (!denom || !grad_boxes) return accv::fail(ACCV_EINVAL, "%s: null denom / gradient pointer", who);
    if (reinterpret_cast<uintptr_t>(grad_boxes) % (uintptr_t)elem_size(dtype))
        return accv::fail(ACCV_EINVAL, "%s: the gradient is not aligned to its element size", who);
    hipStream_t s = static_cast<hipStream_t>(stream);
    dispatch_dtype(dtype, [&](auto dt) { launch_bwd<dt()>(a, grad_l1, grad_iou, denom, grad_boxes, s); });
    return accv::check_launch(who);
}

int accv_matched_box_loss_host(const void* pred_boxes, const void* gt_boxes, const void* pred_ind, const void* gt_ind,
                               const long long* counts, int dtype, unsigned flags, long long B, long long Q, long long D,
                               long long G, long long K, long long stride_b, long long stride_q,
                               const accv_matched_box_params* params, void* out, double* out_denom)
{
    const char* who = "matched_box_loss (host)";
    Args a;
    int empty;
    if (int rc = check_args(who, pred_boxes, gt_boxes, pred_ind, gt_ind, counts, dtype, flags, B, Q, D, G, K, stride_b, stride_q,
                            params, true, a, &empty))
        return rc;
    if (empty) return ACCV_OK;
    if (!out || !out_denom) return accv::fail(ACCV_EINVAL, "%s: null output pointer", who);
    return dispatch_host(who, dtype, [&](auto dt) { host_fwd<dt()>(a, params, out, out_denom); });
}

int accv_matched_box_loss_bwd_host(const void* pred_boxes, const void* gt_boxes, const void* pred_ind, const void* gt_ind,
                                   const long long* counts, const void* grad_l1, const void* grad_iou, const double* denom,
                                   int dtype, unsigned flags, long long B, long long Q, long long D, long long G, long long K,
                                   long long stride_b, long long stride_q, const accv_matched_box_params* params,
                                   void* grad_boxes)
{
    const char* who = "matched_box_loss_bwd (host)";
    Args a;
    int empty;
    if (int rc = check_args(who, pred_boxes, gt_boxes, pred_ind, gt_ind, counts, dtype, flags, B, Q, D, G, K, stride_b, stride_q,
                            params, false, a, &empty))
        return rc;
    if (empty) return ACCV_OK;
    if (!denom || !grad_boxes) return accv::fail(ACCV_EINVAL, "%s: null denom / gradient pointer", who);
    return dispatch_host(who, dtype, [&](auto dt) { host_bwd<dt()>(a, grad_l1, grad_iou, denom, grad_boxes); });
}

}  // extern "C"
