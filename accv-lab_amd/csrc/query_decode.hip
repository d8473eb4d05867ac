// Prediction side of a set-prediction head (DETR, Deformable DETR, DINO, PETR / StreamPETR, BEVFormer, DETR3D): from the raw
// class logits [B, Q, C] and box rows [B, Q, D] of the last decoder layer to the top max_num (query, class) pairs of every
// frame, decoded, filtered and compacted — mmdet3d's NMSFreeCoder.decode with denormalize_bbox (3D) and mmdet's
// DETRHead._predict_by_feat_single (2D) — in ONE launch, in a defined order and without a host round trip.  Per-rank
// arithmetic: query_decode_arith.h; the selection: topk_select.h, shared with heatmap_peaks.hip.
//
// query_decode_kernel, one workgroup of kThreads lanes per frame, templated over the score dtype and the row decoder:
//   1. select: an MSB-first radix select over the 64-bit keys (order-preserving bits of the RAW logit, 0xFFFFFFFF - flat
//      index q * C + c).  Sigmoid is monotone, so no sigmoid pass runs over the Q * C logits.  Every pass reads the logits
//      from global memory (kUnroll loads in flight per lane; L2 hits after the first pass) and builds the keys on the fly:
//      no per-lane key array bounds Q * C.  Equal logits descend into the index bits: at most 8 passes.
//   2. the max_num winners go to LDS (an LDS slot counter places them; the order comes from the unique keys alone) and through
//      a bitonic sort.
//   3. lane r decodes rank r: q = index / C, label = index % C, one row gather, the row decoder's arithmetic and validity.
//      accv::block_rank gives every valid lane its slot; valid lanes write their row, lanes total .. max_num - 1 the
//      padding of their own slot, lane 0 the count: every output element is written exactly once.
// LDS: 8 KiB of keys, the 256-bin histogram and 16 wave counts — about 9 KiB of the CU's 160 KiB.  No atomics on global
// memory, no workspace, bitwise reproducible.  Latency-bound selection work: no MFMA.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <functional>
#include <vector>

#include "accv_common.h"
#include "accv_numeric.h"
#include "detect_common.h"
#include "query_decode_arith.h"
#include "topk_select.h"

#pragma clang fp contract(off)

namespace {

using accv::load_any;
using accv_topk::u64;

constexpr int kWave = 64;
constexpr int kThreads = 1024;   // lanes of a frame's workgroup, and the most ranks it decodes: a lane per rank
constexpr int kWaves = kThreads / kWave;
constexpr int kUnroll = 8;       // scores per lane and step of the select loop
constexpr int kMaxD = 10;        // values of the widest input row

static_assert(accv_qd::kMaxK == ACCV_QD_MAX_K && accv_qd::kMaxK == kThreads && accv_qd::kMaxK <= accv_topk::kMaxK,
              "a lane per rank; query_decode_arith.h and accv_hip.h must agree");
static_assert(accv_qd::kMaxWidth == kMaxD - 1, "the widest written row");

// ======================================================================================================== row decoders
// A row decoder: D values in, width() values out, the constants of a frame, and decode() = score, row and validity.
struct Row3 {
    accv_cd::Consts k;
    int D;   // 8 or 10
    struct Frame {};
    __host__ __device__ int width() const { return D - 1; }
    __host__ __device__ Frame frame(long long) const { return Frame{}; }
    __host__ __device__ bool decode(const Frame&, const float* p, float x, float& score, float* out) const
    {
        return accv_qd::row_3d(k, D, p, x, score, out);
    }
};

struct Row2 {
    accv_qd::Consts2 c;
    const void* image_hw;      // [B, 2] rows (H, W), or null
    const float* matrices;     // [B, 2, 3] or null
    long long Hi, Wi;
    int hw64;
    static constexpr int D = 4;
    struct Frame {
        accv_bd::Frame fr;
        accv_ip::Warp w;
    };
    __host__ __device__ int width() const { return 4; }
    __host__ __device__ Frame frame(long long b) const
    {
        long long H = Hi, W = Wi;
        if (image_hw) {
            if (hw64) H = static_cast<const long long*>(image_hw)[2 * b], W = static_cast<const long long*>(image_hw)[2 * b + 1];
            else H = static_cast<const int*>(image_hw)[2 * b], W = static_cast<const int*>(image_hw)[2 * b + 1];
        }
        Frame f;
        f.fr = accv_bd::frame_consts(1, 1, accv_bh::clamp_extent(W), accv_bh::clamp_extent(H));   // only EW and EH are used
        f.w = accv_ip::load_warp(matrices ? matrices + b * 6 : nullptr);
        return f;
    }
    __host__ __device__ bool decode(const Frame& f, const float* p, float x, float& score, float* out) const
    {
        return accv_qd::row_2d(c, f.fr, f.w, p, x, score, out);
    }
};

template <class Row>
struct Args {
    const void* cls;       // [B, Q, C]
    const void* rows;      // [B, Q, D]
    Row row;
    float* boxes;          // [B, M, width]
    float* scores;         // [B, M]
    long long* labels;     // [B, M]
    int* source;           // [B, M]
    long long* sizes;      // [B]
    long long B, Q, C, N;  // N = Q * C
    int M, cls_dt, row_dt;
};

// rank with flat index `idx` of frame b: its query, label, score, row and validity
template <class Row>
__host__ __device__ inline bool decode_rank(const Args<Row>& a, const typename Row::Frame& fr, long long b, unsigned idx, long long& q,
                                            long long& label, float& score, float (&out)[accv_qd::kMaxWidth])
{
    q = (long long)idx / a.C;
    label = (long long)idx - q * a.C;
    const float x = load_any(a.cls, b * a.N + (long long)idx, a.cls_dt);
    const int D = a.row.D;
    const long long at = (b * a.Q + q) * D;
    float p[kMaxD];
#pragma unroll
    for (int j = 0; j < kMaxD; ++j) p[j] = j < D ? load_any(a.rows, at + j, a.row_dt) : 0.0f;
    return a.row.decode(fr, p, x, score, out);
}

template <class Row>
__host__ __device__ inline void write_row(const Args<Row>& a, long long o, long long q, long long label, float score,
                                          const float (&out)[accv_qd::kMaxWidth])
{
    const int W = a.row.width();
    float* dst = a.boxes + o * W;
#pragma unroll
    for (int j = 0; j < accv_qd::kMaxWidth; ++j)
        if (j < W) dst[j] = out[j];
    a.scores[o] = score;
    a.labels[o] = label;
    a.source[o] = (int)q;
}

template <class Row>
__host__ __device__ inline void write_padding(const Args<Row>& a, long long o)
{
    const int W = a.row.width();
    float* dst = a.boxes + o * W;
    for (int j = 0; j < W; ++j) dst[j] = 0.0f;
    a.scores[o] = 0.0f;
    a.labels[o] = 0;
    a.source[o] = -1;
}

// ============================================================================================================== kernel
template <int DT, class Row>
__global__ __launch_bounds__(kThreads) void query_decode_kernel(const Args<Row> a)
{
    __shared__ u64 s_sel[accv_topk::kMaxK];
    __shared__ accv_topk::SelectShared sh;
    __shared__ int s_cnt[kWaves];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const long long b = blockIdx.x;
    const long long N = a.N, frame_off = b * N;
    const unsigned k = (unsigned)a.M;

    // 1. select.  The same trip count on every lane (f ballots); kUnroll independent loads in flight per lane.
    auto each = [&](auto&& f) {
        for (long long base = 0; base < N; base += (long long)kThreads * kUnroll) {
            float v[kUnroll];
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) {
                const long long i = base + (long long)u * kThreads + tid;
                v[u] = i < N ? accv::load<DT, accv::kHwF16>(a.cls, frame_off + i) : 0.0f;
            }
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) {
                const long long i = base + (long long)u * kThreads + tid;
                f(i < N ? accv_topk::make_key(v[u], (unsigned)i) : 0ull);
            }
        }
    };
    accv_topk::Cut cut{0, 64};
    if (N > (long long)k) cut = accv_topk::radix_select(each, k, sh);   // N == k: every key is taken

    // 2. the k winners into LDS, sorted
    int P = 1;
    while (P < (int)k) P <<= 1;
    for (int i = tid; i < P; i += kThreads) s_sel[i] = 0;
    if (tid == 0) sh.slots = 0;
    __syncthreads();
    each([&](u64 key) {
        if (cut.take(key)) s_sel[atomicAdd(&sh.slots, 1u)] = key;
    });
    __syncthreads();
    accv_topk::bitonic_sort_desc<kThreads>(s_sel, P);

    // 3. a lane per rank: decode, rank the valid ones in order, write
    const typename Row::Frame fr = a.row.frame(b);
    bool valid = false;
    long long q = 0, label = 0;
    float score = 0.0f, out[accv_qd::kMaxWidth];
    if (tid < (int)k) valid = decode_rank(a, fr, b, accv_topk::index_of(s_sel[tid]), q, label, score, out);
    int before, total;
    accv::block_rank<kWaves>(valid, s_cnt, lane, wave, before, total);
    const long long first = b * (long long)k;
    if (valid) write_row(a, first + before, q, label, score, out);
    if (tid >= total && tid < (int)k) write_padding(a, first + tid);
    if (tid == 0) a.sizes[b] = total;
}

// the serial form: a stable sort on the same keys, then the same per-rank functions
template <class Row>
void host_run(const Args<Row>& a)
{
    std::vector<u64> keys((size_t)a.N);
    for (long long b = 0; b < a.B; ++b) {
        for (long long i = 0; i < a.N; ++i) keys[(size_t)i] = accv_topk::make_key(load_any(a.cls, b * a.N + i, a.cls_dt), (unsigned)i);
        std::stable_sort(keys.begin(), keys.end(), std::greater<u64>());
        const typename Row::Frame fr = a.row.frame(b);
        long long kept = 0;
        for (int r = 0; r < a.M; ++r) {
            long long q, label;
            float score, out[accv_qd::kMaxWidth];
            if (decode_rank(a, fr, b, accv_topk::index_of(keys[(size_t)r]), q, label, score, out))
                write_row(a, b * a.M + kept++, q, label, score, out);
        }
        for (long long j = kept; j < a.M; ++j) write_padding(a, b * a.M + j);
        a.sizes[b] = kept;
    }
}

// ========================================================================================================= host checks
// What both decoders check and set.  ACCV_OK with *empty = 1 when there is nothing to write; every check runs before anything
// reads the data.
template <class Row>
int check_common(const char* who, const void* cls, const void* rows, int cls_dt, int row_dt, long long B, long long Q, long long C, long long M,
                 float* boxes, float* scores, long long* labels, int* source, long long* out_sizes, Args<Row>& a, int* empty)
{
    *empty = 0;
    if (B < 0 || Q < 0 || C < 0 || M < 0) return accv::fail(ACCV_EINVAL, "%s: negative size (B %lld, Q %lld, C %lld, max_num %lld)", who, B, Q, C, M);
    if (cls_dt < accv::kF32 || cls_dt > accv::kBF16 || row_dt < accv::kF32 || row_dt > accv::kBF16)
        return accv::fail(ACCV_EINVAL, "%s: unknown dtype code %d / %d (0 f32, 1 f16, 2 bf16)", who, cls_dt, row_dt);
    if (Q < 1 || C < 1) return accv::fail(ACCV_EINVAL, "%s: Q and C must be at least 1, got %lld and %lld", who, Q, C);
    if (Q > accv_topk::kMaxGroup / C) return accv::fail(ACCV_EINVAL, "%s: Q * C = %lld * %lld must stay below 2^32 - 1", who, Q, C);
    if (M < 1 || M > accv_qd::kMaxK) return accv::fail(ACCV_EINVAL, "%s: max_num must be in 1..%d, got %lld", who, accv_qd::kMaxK, M);
    if (M > Q * C) return accv::fail(ACCV_EINVAL, "%s: max_num = %lld exceeds Q * C = %lld", who, M, Q * C);
    if (B == 0) {
        *empty = 1;
        return ACCV_OK;
    }
    if (int rc = accv_det::outputs_present(who, boxes, scores, labels, source, out_sizes)) return rc;
    if (!cls || !rows) return accv::fail(ACCV_EINVAL, "%s: null input pointer", who);
    if (int rc = accv_det::outputs_aligned(who, boxes, scores, labels, source, out_sizes)) return rc;
    if ((reinterpret_cast<uintptr_t>(cls) & ((uintptr_t)accv::elem_size(cls_dt) - 1u)) ||
        (reinterpret_cast<uintptr_t>(rows) & ((uintptr_t)accv::elem_size(row_dt) - 1u)))
        return accv::fail(ACCV_EINVAL, "%s: an input is not aligned to its element size", who);
    if (int rc = accv_det::grid_fits(who, B)) return rc;
    if (B > LLONG_MAX / 64 / kMaxD / (Q * C)) return accv::fail(ACCV_EINVAL, "%s: sizes overflow", who);
    a.cls = cls, a.rows = rows;
    a.boxes = boxes, a.scores = scores, a.labels = labels, a.source = source, a.sizes = out_sizes;
    a.B = B, a.Q = Q, a.C = C, a.N = Q * C;
    a.M = (int)M, a.cls_dt = cls_dt, a.row_dt = row_dt;
    return ACCV_OK;
}

int check_3d(const char* who, const accv_query_decode_3d_params* p, long long B, long long Q, long long C, long long D, long long M, float* boxes,
             float* scores, long long* labels, int* source, long long* out_sizes, Args<Row3>& a, int* empty)
{
    *empty = 0;
    if (!p) return accv::fail(ACCV_EINVAL, "%s: null params", who);
    if (D != 8 && D != 10) return accv::fail(ACCV_EINVAL, "%s: D must be 8 or 10 (cx, cy, log w, log l, cz, log h, sin, cos[, vx, vy]), got %lld", who, D);
    if (p->has_score_threshold && !(p->score_threshold == p->score_threshold)) return accv::fail(ACCV_EINVAL, "%s: score_threshold is NaN", who);
    if (p->has_post_center_range)
        for (int i = 0; i < 6; ++i)
            if (!(p->post_center_range[i] == p->post_center_range[i])) return accv::fail(ACCV_EINVAL, "%s: post_center_range holds NaN", who);
    if (int rc = check_common(who, p->cls_scores, p->bbox_preds, p->score_dtype, p->box_dtype, B, Q, C, M, boxes, scores, labels, source,
                              out_sizes, a, empty))
        return rc;
    accv_cd::Consts& k = a.row.k;
    k.pc0 = k.pc1 = 0.0f, k.vs0 = k.vs1 = k.f = 1.0f;   // not used: the centre is the row's own
    k.thr = (float)p->score_threshold;
    for (int i = 0; i < 3; ++i) k.lo[i] = (float)p->post_center_range[i], k.hi[i] = (float)p->post_center_range[3 + i];
    k.has_thr = p->has_score_threshold ? 1 : 0, k.has_range = p->has_post_center_range ? 1 : 0;
    k.logits = p->scores_are_logits ? 1 : 0, k.norm_bbox = 1, k.bottom = p->bottom_center ? 1 : 0;
    a.row.D = (int)D;
    return ACCV_OK;
}

int check_2d(const char* who, const accv_query_decode_2d_params* p, long long B, long long Q, long long C, long long M, float* boxes, float* scores,
             long long* labels, int* source, long long* out_sizes, Args<Row2>& a, int* empty)
{
    *empty = 0;
    if (!p) return accv::fail(ACCV_EINVAL, "%s: null params", who);
    if (p->has_score_threshold && !(p->score_threshold == p->score_threshold)) return accv::fail(ACCV_EINVAL, "%s: score_threshold is NaN", who);
    if (int rc = check_common(who, p->cls_scores, p->bbox_preds, p->score_dtype, p->box_dtype, B, Q, C, M, boxes, scores, labels, source,
                              out_sizes, a, empty))
        return rc;
    if (*empty) return ACCV_OK;
    if (reinterpret_cast<uintptr_t>(p->image_hw) & (p->image_hw_i64 ? 7u : 3u))
        return accv::fail(ACCV_EINVAL, "%s: image_hw is not aligned to its element size", who);
    if (reinterpret_cast<uintptr_t>(p->image_matrices) & 3u) return accv::fail(ACCV_EINVAL, "%s: image_matrices is not aligned to its element size", who);
    accv_bd::Consts& k = a.row.c.k;
    k.thr = (float)p->score_threshold, k.min_h = k.min_w = k.iou_thr = 0.0f;
    k.has_thr = p->has_score_threshold ? 1 : 0, k.has_min = 0, k.has_iou = 0;
    k.logits = p->scores_are_logits ? 1 : 0, k.clip = p->clip ? 1 : 0, k.order = p->order_corners ? 1 : 0, k.agnostic = 0;
    a.row.c.cxcywh = p->cxcywh ? 1 : 0, a.row.c.normalized = p->normalized ? 1 : 0;
    a.row.image_hw = p->image_hw, a.row.matrices = p->image_matrices;
    a.row.Hi = accv_bh::clamp_extent(p->image_h), a.row.Wi = accv_bh::clamp_extent(p->image_w);
    a.row.hw64 = p->image_hw_i64 ? 1 : 0;
    return ACCV_OK;
}

template <class Row>
int launch(const char* who, const Args<Row>& a, void* stream)
{
    const dim3 grid((unsigned)a.B), block(kThreads);
    hipStream_t s = static_cast<hipStream_t>(stream);
    switch (a.cls_dt) {
        case accv::kF32: hipLaunchKernelGGL((query_decode_kernel<accv::kF32, Row>), grid, block, 0, s, a); break;
        case accv::kF16: hipLaunchKernelGGL((query_decode_kernel<accv::kF16, Row>), grid, block, 0, s, a); break;
        default: hipLaunchKernelGGL((query_decode_kernel<accv::kBF16, Row>), grid, block, 0, s, a); break;
    }
    return accv::check_launch(who);
}

}  // namespace

extern "C" {

int accv_query_decode_3d(const accv_query_decode_3d_params* params, long long B, long long Q, long long C, long long D, long long M,
                         float* boxes, float* scores, long long* labels, int* source, long long* out_sizes, void* stream)
{
    const char* who = "query_box_decode_3d";
    Args<Row3> a;
    int empty;
    if (int rc = check_3d(who, params, B, Q, C, D, M, boxes, scores, labels, source, out_sizes, a, &empty)) return rc;
    if (empty) return ACCV_OK;
    return launch(who, a, stream);
}

int accv_query_decode_3d_cpu(const accv_query_decode_3d_params* params, long long B, long long Q, long long C, long long D, long long M,
                             float* boxes, float* scores, long long* labels, int* source, long long* out_sizes)
{
    const char* who = "query_box_decode_3d (host)";
    Args<Row3> a;
    int empty;
    if (int rc = check_3d(who, params, B, Q, C, D, M, boxes, scores, labels, source, out_sizes, a, &empty)) return rc;
    if (empty) return ACCV_OK;
    host_run(a);
    return ACCV_OK;
}

int accv_query_decode_2d(const accv_query_decode_2d_params* params, long long B, long long Q, long long C, long long M, float* boxes,
                         float* scores, long long* labels, int* source, long long* out_sizes, void* stream)
{
    const char* who = "query_box_decode_2d";
    Args<Row2> a;
    int empty;
    if (int rc = check_2d(who, params, B, Q, C, M, boxes, scores, labels, source, out_sizes, a, &empty)) return rc;
    if (empty) return ACCV_OK;
    return launch(who, a, stream);
}

int accv_query_decode_2d_cpu(const accv_query_decode_2d_params* params, long long B, long long Q, long long C, long long M, float* boxes,
                             float* scores, long long* labels, int* source, long long* out_sizes)
{
    const char* who = "query_box_decode_2d (host)";
    Args<Row2> a;
    int empty;
    if (int rc = check_2d(who, params, B, Q, C, M, boxes, scores, labels, source, out_sizes, a, &empty)) return rc;
    if (empty) return ACCV_OK;
    host_run(a);
    return ACCV_OK;
}

}  // extern "C"
