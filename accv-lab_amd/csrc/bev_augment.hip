// BEV box augmentation with range filter for a ragged batch of 3D boxes in one launch: the reference's
// BEVBBoxesTransformer3D (rotation about z, uniform scaling, translation of centres, sizes, yaws and velocities, and the
// update of every matrix that maps to or from the augmented frame), PointsInRangeCheck on the centres and the
// ConditionalElementRemover over the resulting flag.  Per frame the kept boxes are augmented and compacted in ascending
// slot order with their labels and source slots; the rest of each row is filled (0, source -1), the keep flag of every
// input slot and the kept count are written, so every output element is written exactly once.  Per-frame arithmetic:
// bev_augment_arith.h.
//
// One workgroup of kThreads lanes per frame.
//   boxes     the frame's slots are walked in chunks of kThreads, a lane per slot: the lane reads its centre, `valid` and
//             the range decide, and the order-preserving rank (accv::block_rank: __ballot + popcount inside the wave, the
//             waves' totals in LDS behind one barrier) gives the output slot, with a running base across chunks.  The LDS
//             row alternates with the chunk, so the barrier of chunk i + 1 separates the reads of chunk i from the writes
//             of chunk i + 2.  Kept lanes then compute and store their row; the tail is filled.
//   matrices  a lane per matrix row (point transforms) or column (frame transforms), the lanes striding over all matrices
//             of the frame.  A row moves as one 16-byte load and store when the base pointers of its tensor are 16-byte
//             aligned (checked on the host, passed as a bit), else as four floats.
// Tensor pointers and the range travel by value in the kernel arguments.  No atomics, no workspace: the order is defined
// by the slot number, so the result is bitwise reproducible.  Launch and latency bound work: no MFMA.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>

#include "accv_common.h"
#include "accv_numeric.h"
#include "bev_augment_arith.h"

#pragma clang fp contract(off)

namespace {

using namespace accv_ba;
using accv::clamp_count;
using accv::load_index;

constexpr int kWave = 64;
constexpr int kThreads = 256;               // and slots per chunk
constexpr int kWaves = kThreads / kWave;
constexpr int kMaxPoint = ACCV_BA_MAX_POINT_TRANSFORMS;
constexpr int kMaxFrame = ACCV_BA_MAX_FRAME_TRANSFORMS;
constexpr int kRow = 7;                     // floats of a parameter row
constexpr unsigned kKnownFlags = ACCV_BA_COUNTS_I64 | ACCV_BA_LABELS_I64 | ACCV_BA_RANGE_ON_OUTPUT;

struct Args {
    const float* boxes;             // [B, N, D]
    const float* rows;              // [B, 7]
    const void* labels;             // [B, N] or null
    const unsigned char* valid;     // [B, N] or null
    const void* counts;             // [B]
    float* out_boxes;               // [B, N, D]
    void* out_labels;               // [B, N] of the labels' type, or null
    int* source;                    // [B, N]
    unsigned char* keep;            // [B, N]
    long long* sizes;               // [B]
    const float* point_in[kMaxPoint];
    float* point_out[kMaxPoint];
    long long point_rows[kMaxPoint];    // matrix rows per frame, K * R
    const float* frame_in[kMaxFrame];
    float* frame_out[kMaxFrame];
    long long frame_cols[kMaxFrame];    // matrix columns per frame, K * 4
    Range range;
    long long B, N;
    int D, labels64, counts64, has_range, range_on_output, num_point, num_frame;
    unsigned vec16;                 // bit i: point transform i moves its rows as 16-byte vectors
};

// valid && in range of slot o = b * N + n, whose raw centre is the first three floats of `box`; the augmented centre comes
// back either way
__host__ __device__ inline bool decide(const Args& a, const Row& p, long long o, const float* box, float& ox, float& oy, float& oz)
{
    const float x = box[0], y = box[1], z = box[2];
    augment_center(p, x, y, z, ox, oy, oz);
    bool on = !a.valid || a.valid[o] != 0;
    if (a.has_range) on = on && (a.range_on_output ? in_range(a.range, ox, oy, oz) : in_range(a.range, x, y, z));
    return on;
}

// everything a kept box writes: output slot o_out from input slot n (both offsets include the frame)
__host__ __device__ inline void write_box(const Args& a, const Row& p, long long o_out, long long o_in, long long n, const float* box,
                                          float ox, float oy, float oz)
{
    float row[9];
    augment_box(p, box, a.D, ox, oy, oz, row);
    float* out = a.out_boxes + o_out * a.D;
#pragma unroll
    for (int c = 0; c < 7; ++c) out[c] = row[c];
    if (a.D == 9) out[7] = row[7], out[8] = row[8];
    a.source[o_out] = (int)n;
    if (a.labels) {
        if (a.labels64) static_cast<long long*>(a.out_labels)[o_out] = static_cast<const long long*>(a.labels)[o_in];
        else static_cast<int*>(a.out_labels)[o_out] = static_cast<const int*>(a.labels)[o_in];
    }
}

// the filler of output slot o, all outputs but the boxes
__host__ __device__ inline void write_padding(const Args& a, long long o)
{
    a.source[o] = -1;
    if (a.labels) {
        if (a.labels64) static_cast<long long*>(a.out_labels)[o] = 0;
        else static_cast<int*>(a.out_labels)[o] = 0;
    }
}

__host__ __device__ inline void point_row_scalar(const Row& p, float ik, const float* in, float* out)
{
    float r[4];
    point_transform_row(p, ik, in[0], in[1], in[2], in[3], r);
    out[0] = r[0], out[1] = r[1], out[2] = r[2], out[3] = r[3];
}

// column `col` of the 4 x 4 matrix at `in`
__host__ __device__ inline void frame_column(const Row& p, const float* in, float* out, int col)
{
    float r[4];
    frame_transform_column(p, in[col], in[4 + col], in[8 + col], in[12 + col], r);
    out[col] = r[0], out[4 + col] = r[1], out[8 + col] = r[2], out[12 + col] = r[3];
}

// ------------------------------------------------------------------------------------------------------------- device
__global__ __launch_bounds__(kThreads) void bev_augment_kernel(const Args a)
{
    __shared__ int s_cnt[2][kWaves];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const long long b = blockIdx.x;
    const Row p = load_row(a.rows + b * kRow);
    const long long size = clamp_count(a.counts, b, a.N, a.counts64);
    const long long row0 = b * a.N;
    long long kept = 0;   // running base, the same in every lane
    int parity = 0;
    for (long long base = 0; base < size; base += kThreads, parity ^= 1) {
        const long long n = base + tid;
        const float* box = a.boxes + (row0 + n) * a.D;
        float ox = 0.0f, oy = 0.0f, oz = 0.0f;
        bool on = false;
        if (n < size) {
            on = decide(a, p, row0 + n, box, ox, oy, oz);
            a.keep[row0 + n] = on ? 1 : 0;
        }
        int before, total;
        accv::block_rank<kWaves>(on, s_cnt[parity], lane, wave, before, total);
        if (on) write_box(a, p, row0 + kept + before, row0 + n, n, box, ox, oy, oz);
        kept += total;
    }
    for (long long j = size + tid; j < a.N; j += kThreads) a.keep[row0 + j] = 0;
    for (long long j = kept + tid; j < a.N; j += kThreads) write_padding(a, row0 + j);
    float* brow = a.out_boxes + row0 * a.D;
    for (long long e = kept * a.D + tid; e < a.N * a.D; e += kThreads) brow[e] = 0.0f;
    if (tid == 0) a.sizes[b] = kept;

    if (a.num_point > 0) {
        const float ik = div_rn(1.0f, p.k);
#pragma unroll
        for (int i = 0; i < kMaxPoint; ++i) {
            if (i >= a.num_point) break;
            const long long items = a.point_rows[i];
            const float* in = a.point_in[i] + b * items * 4;
            float* out = a.point_out[i] + b * items * 4;
            if ((a.vec16 >> i) & 1u) {
                for (long long it = tid; it < items; it += kThreads) {
                    const float4 m = reinterpret_cast<const float4*>(in)[it];
                    float r[4];
                    point_transform_row(p, ik, m.x, m.y, m.z, m.w, r);
                    reinterpret_cast<float4*>(out)[it] = make_float4(r[0], r[1], r[2], r[3]);
                }
            } else {
                for (long long it = tid; it < items; it += kThreads) point_row_scalar(p, ik, in + it * 4, out + it * 4);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < kMaxFrame; ++i) {
        if (i >= a.num_frame) break;
        const long long items = a.frame_cols[i];
        const float* in = a.frame_in[i] + b * items * 4;
        float* out = a.frame_out[i] + b * items * 4;
        for (long long it = tid; it < items; it += kThreads) frame_column(p, in + (it >> 2) * 16, out + (it >> 2) * 16, (int)(it & 3));
    }
}

// --------------------------------------------------------------------------------------------------------------- host
void host_run(const Args& a)
{
    for (long long b = 0; b < a.B; ++b) {
        const Row p = load_row(a.rows + b * kRow);
        const long long size = clamp_count(a.counts, b, a.N, a.counts64);
        const long long row0 = b * a.N;
        long long kept = 0;
        for (long long n = 0; n < size; ++n) {
            const float* box = a.boxes + (row0 + n) * a.D;
            float ox, oy, oz;
            const bool on = decide(a, p, row0 + n, box, ox, oy, oz);
            a.keep[row0 + n] = on ? 1 : 0;
            if (on) write_box(a, p, row0 + kept++, row0 + n, n, box, ox, oy, oz);
        }
        for (long long j = size; j < a.N; ++j) a.keep[row0 + j] = 0;
        for (long long j = kept; j < a.N; ++j) write_padding(a, row0 + j);
        for (long long e = kept * a.D; e < a.N * a.D; ++e) a.out_boxes[row0 * a.D + e] = 0.0f;
        a.sizes[b] = kept;
        const float ik = div_rn(1.0f, p.k);
        for (int i = 0; i < a.num_point; ++i) {
            const long long items = a.point_rows[i];
            for (long long it = 0; it < items; ++it)
                point_row_scalar(p, ik, a.point_in[i] + (b * items + it) * 4, a.point_out[i] + (b * items + it) * 4);
        }
        for (int i = 0; i < a.num_frame; ++i) {
            const long long items = a.frame_cols[i];
            for (long long it = 0; it < items; ++it)
                frame_column(p, a.frame_in[i] + b * items * 4 + (it >> 2) * 16, a.frame_out[i] + b * items * 4 + (it >> 2) * 16,
                             (int)(it & 3));
        }
    }
}

// ------------------------------------------------------------------------------------------------------------- checks
inline uintptr_t addr(const void* p) { return reinterpret_cast<uintptr_t>(p); }

// ACCV_OK with *empty = 1 when there is nothing to write; every check runs before anything else reads the arguments
int check_args(const char* who, const float* boxes, const float* rows, const void* labels, const unsigned char* valid,
               const void* counts, unsigned flags, long long B, long long N, long long D, const accv_bev_augment_params* p,
               float* out_boxes, void* out_labels, int* source, unsigned char* keep, long long* out_sizes, Args& a, int* empty)
{
    *empty = 0;
    if (!p) return accv::fail(ACCV_EINVAL, "%s: null params", who);
    if (B < 0 || N < 0 || D < 0) return accv::fail(ACCV_EINVAL, "%s: negative size", who);
    if (D != 7 && D != 9) return accv::fail(ACCV_EINVAL, "%s: boxes need D = 7 or 9 (got %lld)", who, D);
    if (flags & ~kKnownFlags) return accv::fail(ACCV_EINVAL, "%s: unknown flags 0x%x", who, flags);
    if (p->num_point_transforms < 0 || p->num_point_transforms > kMaxPoint || p->num_frame_transforms < 0 ||
        p->num_frame_transforms > kMaxFrame)
        return accv::fail(ACCV_EINVAL, "%s: 0..%d point transforms and 0..%d frame transforms supported, got %d and %d", who,
                          kMaxPoint, kMaxFrame, p->num_point_transforms, p->num_frame_transforms);
    for (int i = 0; i < p->num_point_transforms; ++i)
        if (p->point_count[i] < 0 || (p->point_rows[i] != 3 && p->point_rows[i] != 4))
            return accv::fail(ACCV_EINVAL, "%s: point transform %d needs K >= 0 matrices of 3 or 4 rows, got %lld of %d", who, i,
                              p->point_count[i], p->point_rows[i]);
    for (int i = 0; i < p->num_frame_transforms; ++i)
        if (p->frame_count[i] < 0) return accv::fail(ACCV_EINVAL, "%s: frame transform %d has a negative matrix count", who, i);
    if (N > INT_MAX) return accv::fail(ACCV_EINVAL, "%s: N is limited to 2^31 - 1", who);
    if (B == 0) {
        *empty = 1;
        return ACCV_OK;
    }
    if (!rows || !counts || !out_sizes) return accv::fail(ACCV_EINVAL, "%s: null params rows / counts / sizes pointer", who);
    if (N > 0 && (!boxes || !out_boxes || !source || !keep)) return accv::fail(ACCV_EINVAL, "%s: null boxes / output pointer", who);
    if (N > 0 && (flags & ACCV_BA_LABELS_I64) && !labels) return accv::fail(ACCV_EINVAL, "%s: int64 labels flagged but not given", who);
    if (N > 0 && ((labels != nullptr) != (out_labels != nullptr)))
        return accv::fail(ACCV_EINVAL, "%s: labels and out_labels come together or not at all", who);
    if ((addr(boxes) | addr(rows) | addr(out_boxes) | addr(source)) & 3u)
        return accv::fail(ACCV_EINVAL, "%s: a 4-byte tensor is not aligned to its element size", who);
    if (addr(out_sizes) & 7u) return accv::fail(ACCV_EINVAL, "%s: sizes must be 8-byte aligned", who);
    if (((addr(labels) | addr(out_labels)) & ((flags & ACCV_BA_LABELS_I64) ? 7u : 3u)) ||
        (addr(counts) & ((flags & ACCV_BA_COUNTS_I64) ? 7u : 3u)))
        return accv::fail(ACCV_EINVAL, "%s: labels / counts are not aligned to their element size", who);
    if (B > accv::kGridLimit) return accv::fail(ACCV_EINVAL, "%s: %lld workgroups exceed the grid limit", who, B);
    const long long cap = LLONG_MAX / 64;   // elements of any tensor, in bytes with room to spare
    if (N > cap / 9 / B) return accv::fail(ACCV_EINVAL, "%s: sizes overflow", who);
    a.vec16 = 0;
    for (int i = 0; i < kMaxPoint; ++i) a.point_in[i] = nullptr, a.point_out[i] = nullptr, a.point_rows[i] = 0;
    for (int i = 0; i < kMaxFrame; ++i) a.frame_in[i] = nullptr, a.frame_out[i] = nullptr, a.frame_cols[i] = 0;
    for (int i = 0; i < p->num_point_transforms; ++i) {
        if (p->point_count[i] > cap / 16 / B) return accv::fail(ACCV_EINVAL, "%s: sizes overflow", who);
        a.point_rows[i] = p->point_count[i] * p->point_rows[i];
        if (a.point_rows[i] == 0) continue;
        if (!p->point_in[i] || !p->point_out[i]) return accv::fail(ACCV_EINVAL, "%s: point transform %d has a null pointer", who, i);
        if ((addr(p->point_in[i]) | addr(p->point_out[i])) & 3u)
            return accv::fail(ACCV_EINVAL, "%s: point transform %d is not aligned to its element size", who, i);
        a.point_in[i] = p->point_in[i], a.point_out[i] = p->point_out[i];
        if (!((addr(p->point_in[i]) | addr(p->point_out[i])) & 15u)) a.vec16 |= 1u << i;
    }
    for (int i = 0; i < p->num_frame_transforms; ++i) {
        if (p->frame_count[i] > cap / 16 / B) return accv::fail(ACCV_EINVAL, "%s: sizes overflow", who);
        a.frame_cols[i] = p->frame_count[i] * 4;
        if (a.frame_cols[i] == 0) continue;
        if (!p->frame_in[i] || !p->frame_out[i]) return accv::fail(ACCV_EINVAL, "%s: frame transform %d has a null pointer", who, i);
        if ((addr(p->frame_in[i]) | addr(p->frame_out[i])) & 3u)
            return accv::fail(ACCV_EINVAL, "%s: frame transform %d is not aligned to its element size", who, i);
        a.frame_in[i] = p->frame_in[i], a.frame_out[i] = p->frame_out[i];
    }
    a.boxes = boxes, a.rows = rows, a.labels = N > 0 ? labels : nullptr, a.valid = valid, a.counts = counts;
    a.out_boxes = out_boxes, a.out_labels = out_labels, a.source = source, a.keep = keep, a.sizes = out_sizes;
    for (int c = 0; c < 3; ++c) a.range.lo[c] = inward_border(p->range_min[c], false), a.range.hi[c] = inward_border(p->range_max[c], true);
    a.B = B, a.N = N, a.D = (int)D;
    a.labels64 = (flags & ACCV_BA_LABELS_I64) ? 1 : 0, a.counts64 = (flags & ACCV_BA_COUNTS_I64) ? 1 : 0;
    a.has_range = p->has_range ? 1 : 0, a.range_on_output = (flags & ACCV_BA_RANGE_ON_OUTPUT) ? 1 : 0;
    a.num_point = p->num_point_transforms, a.num_frame = p->num_frame_transforms;
    return ACCV_OK;
}

}  // namespace

extern "C" {

int accv_bev_augment(const float* boxes, const float* rows, const void* labels, const unsigned char* valid, const void* counts,
                     unsigned flags, long long B, long long N, long long D, const accv_bev_augment_params* params,
                     float* out_boxes, void* out_labels, int* source, unsigned char* keep, long long* out_sizes, void* stream)
{
    const char* who = "bev_augment_boxes";
    Args a;
    int empty;
    if (int rc = check_args(who, boxes, rows, labels, valid, counts, flags, B, N, D, params, out_boxes, out_labels, source, keep,
                            out_sizes, a, &empty))
        return rc;
    if (empty) return ACCV_OK;
    hipLaunchKernelGGL(bev_augment_kernel, dim3((unsigned)a.B), dim3(kThreads), 0, static_cast<hipStream_t>(stream), a);
    return accv::check_launch(who);
}

int accv_bev_augment_host(const float* boxes, const float* rows, const void* labels, const unsigned char* valid,
                          const void* counts, unsigned flags, long long B, long long N, long long D,
                          const accv_bev_augment_params* params, float* out_boxes, void* out_labels, int* source,
                          unsigned char* keep, long long* out_sizes)
{
    const char* who = "bev_augment_boxes (host)";
    Args a;
    int empty;
    if (int rc = check_args(who, boxes, rows, labels, valid, counts, flags, B, N, D, params, out_boxes, out_labels, source, keep,
                            out_sizes, a, &empty))
        return rc;
    if (empty) return ACCV_OK;
    host_run(a);
    return ACCV_OK;
}

}  // extern "C"
