// Fused matching-cost matrices for ragged Hungarian matching: the [B, Q, G_max] cost that batched_linear_sum_assignment
// reads, built in one launch instead of the broadcast chains of a DETR-style matcher
// (packages/batching_helpers/example/matcher.py:22-31, 78-132: IoU through ~ten element-wise ops, one-hot labels in a
// per-sample, per-object loop, an einsum).  Per-pair arithmetic: matching_cost_arith.h.
//
// Device layout: a workgroup of GT x NY lanes (GT = 64, 128 or 256 ground-truth columns, the smallest tile that covers
// G_max up to 256; NY = 256 / GT query rows side by side) owns one (frame, block of kRowsPerLane * NY queries, tile of GT
// columns).  Lanes run along g, so every store of the contiguous output row is coalesced.  A lane keeps its column's
// label and box in registers and walks its queries: the query's box is the same address for the whole wave (a
// broadcast load), the class score p[q, l_g] is a gather within row q (one or two cache lines).  Columns in
// [G_b, G_max) only store the filler.  No LDS, no atomics, no inter-workgroup communication.  The byte floor is the
// output write; at the sizes of real heads the launch is launch-bound.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <limits>

#include "accv_common.h"
#include "matching_cost_arith.h"

namespace {

using namespace accv_mc;

constexpr int kThreads = 256;
constexpr int kRowsPerLane = 8;   // queries per lane and workgroup
constexpr unsigned kKnownFlags = ACCV_MC_LABELS_I64 | ACCV_MC_CXCYWH;

struct Args {
    const void* scores;
    const void* pboxes;
    const void* labels;
    const void* gboxes;
    const long long* counts;
    long long B, Q, C, G, D;
    long long ssb, ssq, spb, spq;   // strides (elements) of scores / pred_boxes: batch, query
    void* out;
    long long nq, ng;               // query blocks per frame, column tiles per frame
    int qpb;                        // queries per workgroup
};

// what a column holds for the whole walk over the queries
template <class F>
struct Column {
    long long label;
    bool label_ok;
    F box[kMaxD];
    F xyxy[4];
};

template <int DT, bool L64>
__host__ __device__ inline void load_column(const Args& a, const Params<typename Compute<DT>::type>& p, long long b,
                                            long long g, Column<typename Compute<DT>::type>& c)
{
    c.label = 0, c.label_ok = false;
    if (p.cls) {
        const long long off = b * a.G + g;
        c.label = load_index(a.labels, off, L64);
        c.label_ok = c.label >= 0 && c.label < a.C;
    }
#pragma unroll
    for (int d = 0; d < kMaxD; ++d) c.box[d] = 0;
    if (p.l1 || p.iou || p.giou) {
        const long long base = (b * a.G + g) * a.D;
#pragma unroll
        for (int d = 0; d < kMaxD; ++d)
            if (d < a.D) c.box[d] = load<DT>(a.gboxes, base + d);
    }
    if (p.iou || p.giou) to_xyxy(c.box, p.cxcywh, c.xyxy);
}

template <int DT>
__host__ __device__ inline typename Compute<DT>::type pair_at(const Args& a, const Params<typename Compute<DT>::type>& p,
                                                              long long b, long long q,
                                                              const Column<typename Compute<DT>::type>& c)
{
    using F = typename Compute<DT>::type;
    F score = std::numeric_limits<F>::quiet_NaN();
    if (p.cls && c.label_ok) score = load<DT>(a.scores, b * a.ssb + q * a.ssq + c.label);
    F bp[kMaxD], xp[4];
#pragma unroll
    for (int d = 0; d < kMaxD; ++d) bp[d] = 0;
    if (p.l1 || p.iou || p.giou) {
        const long long base = b * a.spb + q * a.spq;
#pragma unroll
        for (int d = 0; d < kMaxD; ++d)
            if (d < a.D) bp[d] = load<DT>(a.pboxes, base + d);
    }
    if (p.iou || p.giou) to_xyxy(bp, p.cxcywh, xp);
    return pair_cost(p, score, bp, c.box, xp, c.xyxy);
}

template <int DT, bool L64>
__global__ __launch_bounds__(kThreads) void matching_cost_kernel(Args a, Params<typename Compute<DT>::type> p)
{
    using F = typename Compute<DT>::type;
    long long blk = blockIdx.x;
    const long long tile = blk % a.ng;
    blk /= a.ng;
    const long long qblk = blk % a.nq, b = blk / a.nq;
    const long long g = tile * blockDim.x + threadIdx.x;
    if (g >= a.G) return;
    const long long q_end = (qblk + 1) * a.qpb < a.Q ? (qblk + 1) * a.qpb : a.Q;
    const long long q0 = qblk * a.qpb + threadIdx.y;
    const int step = blockDim.y;
    F* out = static_cast<F*>(a.out) + b * a.Q * a.G + g;
    if (g >= clamp_count(a.counts, b, a.G)) {
        for (long long q = q0; q < q_end; q += step) out[q * a.G] = p.filler;
        return;
    }
    Column<F> c;
    load_column<DT, L64>(a, p, b, g, c);
    for (long long q = q0; q < q_end; q += step) out[q * a.G] = pair_at<DT>(a, p, b, q, c);
}

template <int DT, bool L64>
void run_host(const Args& a, const Params<typename Compute<DT>::type>& p)
{
    using F = typename Compute<DT>::type;
    F* out = static_cast<F*>(a.out);
    for (long long b = 0; b < a.B; ++b) {
        const long long Gb = clamp_count(a.counts, b, a.G);
        for (long long g = 0; g < a.G; ++g) {
            F* col = out + b * a.Q * a.G + g;
            if (g >= Gb) {
                for (long long q = 0; q < a.Q; ++q) col[q * a.G] = p.filler;
                continue;
            }
            Column<F> c;
            load_column<DT, L64>(a, p, b, g, c);
            for (long long q = 0; q < a.Q; ++q) col[q * a.G] = pair_at<DT>(a, p, b, q, c);
        }
    }
}

template <class F>
Params<F> make_params(const accv_matching_cost_params* in, int kind, unsigned flags, long long D)
{
    Params<F> p;
    p.class_weight = (F)in->class_weight, p.l1_weight = (F)in->l1_weight;
    p.iou_weight = (F)in->iou_weight, p.giou_weight = (F)in->giou_weight;
    p.alpha = (F)in->focal_alpha, p.gamma = (F)in->focal_gamma, p.focal_eps = (F)in->focal_eps;
    p.iou_eps = (F)in->iou_eps, p.filler = (F)in->filler;
    p.kind = kind, p.cxcywh = (flags & ACCV_MC_CXCYWH) ? 1 : 0, p.D = (int)D;
    // a term is evaluated when its weight (as given, before any narrowing) is not zero; a NaN weight counts
    p.cls = in->class_weight != 0.0, p.l1 = in->l1_weight != 0.0;
    p.iou = in->iou_weight != 0.0, p.giou = in->giou_weight != 0.0;
    return p;
}

// ACCV_OK with *empty = 1 when there is nothing to write; every check runs before anything else reads the arguments
int check_args(const char* who, const void* scores, const void* pboxes, const void* labels, const void* gboxes,
               int dtype, int kind, unsigned flags, long long B, long long Q, long long C, long long G, long long D,
               const accv_matching_cost_params* params, const void* out, int* empty)
{
    *empty = 0;
    if (!params) return accv::fail(ACCV_EINVAL, "%s: null params", who);
    if (B < 0 || Q < 0 || C < 0 || G < 0 || D < 0) return accv::fail(ACCV_EINVAL, "%s: negative size", who);
    if (dtype < kF32 || dtype > kF64) return accv::fail(ACCV_EINVAL, "%s: unknown dtype code %d", who, dtype);
    if (kind < kOneMinusProb || kind > kFocal) return accv::fail(ACCV_EINVAL, "%s: unknown class cost kind %d", who, kind);
    if (flags & ~kKnownFlags) return accv::fail(ACCV_EINVAL, "%s: unknown flags 0x%x", who, flags);
    if (D > kMaxD) return accv::fail(ACCV_EINVAL, "%s: box dimension %lld above %d", who, D, kMaxD);
    const bool cls = params->class_weight != 0.0, l1 = params->l1_weight != 0.0;
    const bool iou = params->iou_weight != 0.0 || params->giou_weight != 0.0;
    if (iou && D != 4) return accv::fail(ACCV_EINVAL, "%s: IoU / GIoU costs need 4 box coordinates, got %lld", who, D);
    if (B == 0 || Q == 0 || G == 0) {
        *empty = 1;
        return ACCV_OK;
    }
    if (!out) return accv::fail(ACCV_EINVAL, "%s: null output", who);
    if (cls && (!scores || !labels)) return accv::fail(ACCV_EINVAL, "%s: null scores / labels for the class cost", who);
    if ((l1 || iou) && (!pboxes || !gboxes)) return accv::fail(ACCV_EINVAL, "%s: null boxes for a box cost", who);
    return ACCV_OK;
}

Args make_args(const void* scores, const void* pboxes, const void* labels, const void* gboxes, const long long* counts,
               long long B, long long Q, long long C, long long G, long long D, long long ssb, long long ssq,
               long long spb, long long spq, void* out)
{
    Args a;
    a.scores = scores, a.pboxes = pboxes, a.labels = labels, a.gboxes = gboxes, a.counts = counts;
    a.B = B, a.Q = Q, a.C = C, a.G = G, a.D = D;
    a.ssb = ssb, a.ssq = ssq, a.spb = spb, a.spq = spq;
    a.out = out;
    a.nq = a.ng = 0, a.qpb = 0;
    return a;
}

template <int DT>
int launch(Args a, const accv_matching_cost_params* in, int kind, unsigned flags, hipStream_t stream)
{
    using F = typename Compute<DT>::type;
    const int gt = a.G <= 64 ? 64 : (a.G <= 128 ? 128 : 256);
    const int ny = kThreads / gt;
    a.qpb = ny * kRowsPerLane;
    a.ng = (a.G + gt - 1) / gt, a.nq = (a.Q + a.qpb - 1) / a.qpb;
    const long long blocks = a.B * a.nq * a.ng;
    if (a.B > (long long)std::numeric_limits<int>::max() / a.nq / a.ng || blocks > std::numeric_limits<int>::max())
        return accv::fail(ACCV_EINVAL, "matching_cost: %lld x %lld x %lld exceeds the launch grid", a.B, a.Q, a.G);
    const Params<F> p = make_params<F>(in, kind, flags, a.D);
    if (flags & ACCV_MC_LABELS_I64)
        hipLaunchKernelGGL((matching_cost_kernel<DT, true>), dim3((unsigned)blocks), dim3(gt, ny), 0, stream, a, p);
    else
        hipLaunchKernelGGL((matching_cost_kernel<DT, false>), dim3((unsigned)blocks), dim3(gt, ny), 0, stream, a, p);
    return accv::check_launch("matching_cost");
}

template <int DT>
void host(const Args& a, const accv_matching_cost_params* in, int kind, unsigned flags)
{
    const auto p = make_params<typename Compute<DT>::type>(in, kind, flags, a.D);
    if (flags & ACCV_MC_LABELS_I64) run_host<DT, true>(a, p);
    else run_host<DT, false>(a, p);
}

}  // namespace

extern "C" {

int accv_matching_cost(const void* scores, const void* pred_boxes, const void* gt_labels, const void* gt_boxes,
                       const long long* counts, int dtype, int kind, unsigned flags, long long B, long long Q,
                       long long C, long long G, long long D, long long scores_stride_b, long long scores_stride_q,
                       long long boxes_stride_b, long long boxes_stride_q, const accv_matching_cost_params* params,
                       void* out, void* stream)
{
    int empty;
    if (int rc = check_args("matching_cost", scores, pred_boxes, gt_labels, gt_boxes, dtype, kind, flags, B, Q, C, G, D,
                            params, out, &empty))
        return rc;
    if (empty) return ACCV_OK;
    const Args a = make_args(scores, pred_boxes, gt_labels, gt_boxes, counts, B, Q, C, G, D, scores_stride_b,
                             scores_stride_q, boxes_stride_b, boxes_stride_q, out);
    hipStream_t s = static_cast<hipStream_t>(stream);
    switch (dtype) {
        case kF32: return launch<kF32>(a, params, kind, flags, s);
        case kF16: return launch<kF16>(a, params, kind, flags, s);
        case kBF16: return launch<kBF16>(a, params, kind, flags, s);
        default: return launch<kF64>(a, params, kind, flags, s);
    }
}

int accv_matching_cost_host(const void* scores, const void* pred_boxes, const void* gt_labels, const void* gt_boxes,
                            const long long* counts, int dtype, int kind, unsigned flags, long long B, long long Q,
                            long long C, long long G, long long D, long long scores_stride_b, long long scores_stride_q,
                            long long boxes_stride_b, long long boxes_stride_q, const accv_matching_cost_params* params,
                            void* out)
{
    int empty;
    if (int rc = check_args("matching_cost (host)", scores, pred_boxes, gt_labels, gt_boxes, dtype, kind, flags, B, Q, C,
                            G, D, params, out, &empty))
        return rc;
    if (empty) return ACCV_OK;
    const Args a = make_args(scores, pred_boxes, gt_labels, gt_boxes, counts, B, Q, C, G, D, scores_stride_b,
                             scores_stride_q, boxes_stride_b, boxes_stride_q, out);
    switch (dtype) {
        case kF32: host<kF32>(a, params, kind, flags); break;
        case kF16: host<kF16>(a, params, kind, flags); break;
        case kBF16: host<kBF16>(a, params, kind, flags); break;
        default: host<kF64>(a, params, kind, flags); break;
    }
    return ACCV_OK;
}

}  // extern "C"
