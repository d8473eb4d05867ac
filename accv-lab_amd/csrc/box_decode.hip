// Prediction side of a CenterNet / FCOS-style camera head, the inverse of box_heatmap.hip, and the axis-aligned NMS it
// needs as an operator of its own (torchvision.ops.nms / mmdet's batched_nms rule, ragged, per frame).  Per-peak and per-pair
// arithmetic: box_decode_arith.h.
//
// box_decode_kernel: from the top-K peaks of a heat map and the regression maps (off_x, off_y, h, w, extras) to the
// filtered, NMS'd, compacted xyxy boxes in image (or, with the frame's matrix, source-image) pixels.
// box_nms_kernel: the same NMS on an existing ragged set of xyxy boxes, kept rows copied bit for bit.
//
// Both run one workgroup of kThreads lanes per frame and share every phase but the first and the row they write:
//   1. a lane per slot, kThreads slots a chunk, so a lane owns up to kChunks slots and keeps one `alive` bit for each.  The
//      decoder gathers offset and size at its peak's cell, computes the clipped image-space box and tests validity (alive =
//      valid); the NMS reads its row (alive = the slot exists: k < min(sample_sizes[f], pre_max_size)).  Corners, area, class
//      and the `ok` flag (all four coordinates finite) go to LDS as a structure of arrays: a lane per box is conflict-free,
//      one box for all lanes a broadcast.
//   2. greedy_walk, by blocks of kWave slots in slot order.  The wave that owns block j resolves it among its own lanes:
//      the lowest alive slot is kept, the alive lanes behind it test themselves against it, a __ballot gives the next — no
//      workgroup barrier inside the block.  It publishes the kept mask in s_keep[j]; after ONE barrier every lane tests its
//      alive slots of later blocks against the block's kept boxes (LDS broadcast reads).  That is n / kWave barriers, not
//      n.  A box that is not ok is kept and suppresses nothing.  The walk stops once M boxes are kept.  Without a threshold
//      s_keep is the ballot of alive.
//   3. the output slot of a kept box is the popcount of the kept masks of the blocks before it plus that of the lower lanes
//      of its own.  Kept lanes below the cut write their row; the rest of the M slots is filled (+0, source -1); the count
//      goes to sizes.
// No atomics, no workspace, no host synchronisation: the order is the slot order, so the result is bitwise reproducible.
// Latency-bound work on at most 1024 boxes a frame: no MFMA.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>

#include "accv_common.h"
#include "accv_numeric.h"
#include "box_decode_arith.h"
#include "detect_common.h"

#pragma clang fp contract(off)

namespace {

using namespace accv_bd;

using accv::load_any;
using accv_det::clamp_size;

constexpr int kWave = 64;
constexpr int kThreads = 256;               // and slots per chunk
using Geo = accv_det::Geometry<kMaxK, kThreads, kWave>;
constexpr int kWaves = Geo::kWaves, kChunks = Geo::kChunks, kBlocks = Geo::kBlocks;

static_assert(kMaxMaps == ACCV_BD_MAX_MAPS && kMaxExtras == ACCV_BD_MAX_EXTRAS && kMaxK == ACCV_BD_MAX_K,
              "box_decode_arith.h and accv_hip.h disagree");

// the prepared boxes of a workgroup, structure of arrays
struct Staged {
    float x1[kMaxK], y1[kMaxK], x2[kMaxK], y2[kMaxK], area[kMaxK];
    long long cls[kMaxK];
    unsigned char ok[kMaxK];

    __device__ void put(int i, const Box& b)
    {
        x1[i] = b.x1, y1[i] = b.y1, x2[i] = b.x2, y2[i] = b.y2, area[i] = b.area, cls[i] = b.cls;
        ok[i] = b.ok ? 1 : 0;
    }
    __device__ Box get(int i) const
    {
        Box b;
        b.x1 = x1[i], b.y1 = y1[i], b.x2 = x2[i], b.y2 = y2[i], b.area = area[i], b.cls = cls[i];
        b.ok = ok[i] != 0;
        return b;
    }
};

// ======================================================================================================= shared phases
// Phase 2.  n: slots of the frame (every chunk below ceil(n / kThreads) is staged in full); alive: bit c = my slot of chunk
// c is a candidate; s_keep[j] holds 0 for every block on entry and the kept mask of every block on return (the caller's
// barrier after phase 1 is behind us; the last iteration's barrier or the one below makes s_keep visible).
__device__ inline void greedy_walk(const Staged& sb, unsigned long long* s_keep, unsigned alive, int n, int M, float thr, bool agnostic)
{
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const int nblocks = (n + kWave - 1) / kWave;
    int kept = 0;   // the same in every lane
    for (int j = 0; j < nblocks && kept < M; ++j) {
        const int first = j * kWave;
        if (wave == j % kWaves) {
            const int c = j / kWaves;
            bool live = (alive >> c) & 1u;
            const Box mine = sb.get(first + lane);
            unsigned long long todo = __ballot(live), keep = 0;
            while (todo) {
                const int i = __ffsll((long long)todo) - 1;   // the lowest alive slot: kept
                keep |= 1ull << i;
                if (live && lane > i && suppresses(sb.get(first + i), mine, thr, agnostic)) live = false;
                todo = __ballot(live) & ~((2ull << i) - 1ull);
            }
            if (lane == 0) s_keep[j] = keep;
        }
        __syncthreads();
        unsigned long long rest = s_keep[j];
        kept += __popcll(rest);
        if (kept >= M) break;
        while (rest) {
            const int i = __ffsll((long long)rest) - 1;
            rest &= rest - 1ull;
            const Box kj = sb.get(first + i);
            if (!kj.ok) continue;   // the same in every lane
#pragma unroll 1
            for (int c = 0; c < kChunks; ++c)
                if (c * kWaves + wave > j && ((alive >> c) & 1u) && suppresses(kj, sb.get(c * kThreads + tid), thr, agnostic))
                    alive &= ~(1u << c);
        }
    }
}

// ============================================================================================================== decode
struct DecodeArgs {
    const void* scores;                  // [F, K]
    const long long* indices;            // [F, K]
    const long long* classes;            // [F, K]
    const void* chan[kMaxChannels];      // concatenated channel c: its plane in frame 0 of its map
    unsigned char chan_count[kMaxChannels];   // the channel count of that map
    const void* image_hw;                // [F, 2] rows (H, W), or null
    const float* matrices;               // [F, 2, 3] or null
    float* boxes;                        // [F, M, 4]
    float* out_scores;                   // [F, M]
    long long* labels;                   // [F, M]
    int* source;                         // [F, M]
    float* extras;                       // [F, M, E]
    long long* sizes;                    // [F]
    Consts k;
    long long F, K, M, Wm, Hm, plane, Wi, Hi;
    int E, score_dt, map_dt, hw64;
};

// concatenated channel c at `cell` of frame f
__host__ __device__ inline float channel_at(const DecodeArgs& a, int c, long long f, long long cell)
{
    return load_any(a.chan[c], f * (long long)a.chan_count[c] * a.plane + cell, a.map_dt);
}

__host__ __device__ inline Frame frame_of(const DecodeArgs& a, long long f)
{
    long long H = a.Hi, W = a.Wi;
    if (a.image_hw) {
        if (a.hw64) H = static_cast<const long long*>(a.image_hw)[2 * f], W = static_cast<const long long*>(a.image_hw)[2 * f + 1];
        else H = static_cast<const int*>(a.image_hw)[2 * f], W = static_cast<const int*>(a.image_hw)[2 * f + 1];
    }
    return frame_consts(a.Wm, a.Hm, accv_bh::clamp_extent(W), accv_bh::clamp_extent(H));
}

// steps 1 to 5 for peak k of frame f: whether it is valid, its box (clipped, image space), score and cell.  An illegal index
// or a negative class reads nothing from the maps.
__host__ __device__ inline bool decode_peak(const DecodeArgs& a, const Frame& fr, long long f, long long k, Box& box, float& score,
                                            long long& cell)
{
    const long long at = f * a.K + k;
    cell = a.indices[at];
    const long long cls = a.classes[at];
    box = no_box();
    if (cell < 0 || cell >= a.plane || cls < 0) return false;
    const long long ys = cell / a.Wm, xs = cell - ys * a.Wm;
    float x1, y1, x2, y2;
    corners(a.k, fr, xs, ys, channel_at(a, 0, f, cell), channel_at(a, 1, f, cell), channel_at(a, 2, f, cell), channel_at(a, 3, f, cell),
            x1, y1, x2, y2);
    score = score_of(a.k, load_any(a.scores, at, a.score_dt));
    if (!passes(a.k, score, x1, y1, x2, y2)) return false;
    box = make_box(x1, y1, x2, y2, cls);
    return true;
}

// everything a kept peak writes: slot `slot` of frame f, from peak rank k (a valid one)
__host__ __device__ inline void write_peak(const DecodeArgs& a, const Frame& fr, const accv_ip::Warp& w, long long f, long long slot,
                                           long long k)
{
    Box box;
    float score;
    long long cell;
    decode_peak(a, fr, f, k, box, score, cell);
    to_source(w, a.k.order != 0, box.x1, box.y1, box.x2, box.y2);
    const long long o = f * a.M + slot;
    float* out = a.boxes + o * 4;
    out[0] = box.x1, out[1] = box.y1, out[2] = box.x2, out[3] = box.y2;
    a.out_scores[o] = score;
    a.labels[o] = box.cls;
    a.source[o] = (int)k;
    for (int e = 0; e < a.E; ++e) a.extras[o * a.E + e] = channel_at(a, 4 + e, f, cell);
}

// the filler of padding slot j of frame f (E: extras per slot)
__host__ __device__ inline void write_padding(float* boxes, float* scores, long long* labels, int* source, float* extras, int E,
                                              long long o)
{
    float* out = boxes + o * 4;
    out[0] = out[1] = out[2] = out[3] = 0.0f;
    scores[o] = 0.0f;
    labels[o] = 0;
    source[o] = -1;
    for (int e = 0; e < E; ++e) extras[o * E + e] = 0.0f;
}

__host__ __device__ inline accv_ip::Warp warp_of(const float* matrices, long long f)
{
    return accv_ip::load_warp(matrices ? matrices + f * 6 : nullptr);
}

__global__ __launch_bounds__(kThreads) void box_decode_kernel(const DecodeArgs a)
{
    __shared__ Staged sb;
    __shared__ unsigned long long s_keep[kBlocks];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const long long f = blockIdx.x;
    const int K = (int)a.K, M = (int)a.M;
    const bool nms_on = a.k.has_iou != 0;
    const Frame fr = frame_of(a, f);

    // 1. boxes and validity, a lane per peak
    unsigned alive = 0;   // bit c: my peak of chunk c is valid and not suppressed so far
    const int nchunks = (K + kThreads - 1) / kThreads;   // the same in every lane
#pragma unroll 1
    for (int c = 0; c < kChunks; ++c) {
        if (c >= nchunks) {   // no peak of this chunk exists: only its kept masks are needed, by phase 3
            if (lane == 0) s_keep[c * kWaves + wave] = 0ull;
            continue;
        }
        const int k = c * kThreads + tid;
        Box box = no_box();
        bool valid = false;
        if (k < K) {
            float score;
            long long cell;
            valid = decode_peak(a, fr, f, k, box, score, cell);
        }
        if (nms_on) sb.put(k, box);   // phase 2 reads whole blocks of the chunks that exist
        const unsigned long long vote = __ballot(valid);
        if (lane == 0) s_keep[c * kWaves + wave] = nms_on ? 0ull : vote;
        alive |= (valid ? 1u : 0u) << c;
    }
    __syncthreads();

    // 2. greedy IoU NMS by blocks of one wave in rank order
    if (nms_on) greedy_walk(sb, s_keep, alive, K, M, a.k.iou_thr, a.k.agnostic != 0);

    // 3. output slots from the kept masks, rows, padding, count
    int base[kChunks];
    const int total = Geo::slot_bases(s_keep, base);
    const accv_ip::Warp w = warp_of(a.matrices, f);
#pragma unroll
    for (int c = 0; c < kChunks; ++c) {   // unrolled: base[] stays in registers
        const int k = c * kThreads + tid;
        if (k >= K) continue;
        const unsigned long long keep = s_keep[c * kWaves + wave];
        if (!((keep >> lane) & 1ull)) continue;
        const int slot = base[c] + __popcll(keep & ((1ull << lane) - 1ull));
        if (slot < M) write_peak(a, fr, w, f, slot, k);
    }
    const int count = total < M ? total : M;
    for (int j = count + tid; j < M; j += kThreads) write_padding(a.boxes, a.out_scores, a.labels, a.source, a.extras, a.E, f * a.M + j);
    if (tid == 0) a.sizes[f] = count;
}

void decode_host_run(const DecodeArgs& a)
{
    static thread_local Box kept_box[kMaxK];
    for (long long f = 0; f < a.F; ++f) {
        const Frame fr = frame_of(a, f);
        const accv_ip::Warp w = warp_of(a.matrices, f);
        long long kept = 0;
        for (long long k = 0; k < a.K && kept < a.M; ++k) {
            Box me;
            float score;
            long long cell;
            if (!decode_peak(a, fr, f, k, me, score, cell)) continue;
            bool dead = false;
            if (a.k.has_iou)
                for (long long j = 0; j < kept && !dead; ++j) dead = suppresses(kept_box[j], me, a.k.iou_thr, a.k.agnostic != 0);
            if (dead) continue;
            kept_box[kept] = me;
            write_peak(a, fr, w, f, kept++, k);
        }
        for (long long j = kept; j < a.M; ++j) write_padding(a.boxes, a.out_scores, a.labels, a.source, a.extras, a.E, f * a.M + j);
        a.sizes[f] = kept;
    }
}

// ACCV_OK with *empty = 1 when there is nothing to write; every check runs before anything else reads the arguments
int decode_check_args(const char* who, const accv_box_decode_params* p, long long F, long long K, long long Hm, long long Wm, long long M,
                      float* boxes, float* out_scores, long long* labels, int* source, float* extras, long long* out_sizes,
                      DecodeArgs& a, int* empty)
{
    *empty = 0;
    if (!p) return accv::fail(ACCV_EINVAL, "%s: null params", who);
    if (F < 0 || K < 0 || Hm < 0 || Wm < 0 || M < 0) return accv::fail(ACCV_EINVAL, "%s: negative size", who);
    if (K < 1 || K > kMaxK) return accv::fail(ACCV_EINVAL, "%s: K must be in 1..%d, got %lld", who, kMaxK, K);
    if (M < 1 || M > K) return accv::fail(ACCV_EINVAL, "%s: M must be in 1..K = %lld, got %lld", who, K, M);
    if (Wm < 1 || Hm < 1 || Wm > kMaxExtent || Hm > kMaxExtent || Wm > INT_MAX / Hm)
        return accv::fail(ACCV_EINVAL, "%s: a map of %lld x %lld cells is empty, exceeds 2^24 a side or 2^31 - 1 cells", who, Wm, Hm);
    if (p->score_dtype < accv::kF32 || p->score_dtype > accv::kBF16 || p->map_dtype < accv::kF32 || p->map_dtype > accv::kBF16)
        return accv::fail(ACCV_EINVAL, "%s: unknown dtype code %d / %d (0 f32, 1 f16, 2 bf16)", who, p->score_dtype, p->map_dtype);
    if (p->num_maps < 1 || p->num_maps > kMaxMaps) return accv::fail(ACCV_EINVAL, "%s: 1..%d maps supported, got %d", who, kMaxMaps, p->num_maps);
    long long C = 0;
    for (int i = 0; i < p->num_maps; ++i) {
        if (p->channels[i] < 0) return accv::fail(ACCV_EINVAL, "%s: map %d has a negative channel count", who, i);
        C += p->channels[i];
    }
    if (C < 4 || C > kMaxChannels)
        return accv::fail(ACCV_EINVAL, "%s: the maps hold %lld channels, 4..%d are needed (off_x, off_y, h, w and up to %d extras)", who, C,
                          kMaxChannels, kMaxExtras);
    if (p->has_score_threshold && !(p->score_threshold == p->score_threshold)) return accv::fail(ACCV_EINVAL, "%s: score_threshold is NaN", who);
    if (p->has_iou_threshold && !(p->iou_threshold == p->iou_threshold)) return accv::fail(ACCV_EINVAL, "%s: iou_threshold is NaN", who);
    if (p->has_min_size && (!(p->min_size[0] == p->min_size[0]) || !(p->min_size[1] == p->min_size[1])))
        return accv::fail(ACCV_EINVAL, "%s: min_size holds NaN", who);
    if (F == 0) {
        *empty = 1;
        return ACCV_OK;
    }
    const int E = (int)C - 4;
    if (int rc = accv_det::check_outputs(who, F, boxes, out_scores, labels, source, out_sizes, E > 0, extras)) return rc;
    const long long plane = Hm * Wm;
    if (F > LLONG_MAX / 64 / kMaxChannels / plane || F > LLONG_MAX / 64 / kMaxChannels / K) return accv::fail(ACCV_EINVAL, "%s: sizes overflow", who);
    const uintptr_t score_mask = (uintptr_t)accv::elem_size(p->score_dtype) - 1u, map_size = (uintptr_t)accv::elem_size(p->map_dtype);
    if (!p->scores || !p->indices || !p->classes) return accv::fail(ACCV_EINVAL, "%s: null peaks pointer", who);
    if ((reinterpret_cast<uintptr_t>(p->scores) & score_mask) ||
        ((reinterpret_cast<uintptr_t>(p->indices) | reinterpret_cast<uintptr_t>(p->classes)) & 7u))
        return accv::fail(ACCV_EINVAL, "%s: the peaks are not aligned to their element size", who);
    if (reinterpret_cast<uintptr_t>(p->image_hw) & (p->image_hw_i64 ? 7u : 3u))
        return accv::fail(ACCV_EINVAL, "%s: image_hw is not aligned to its element size", who);
    if (reinterpret_cast<uintptr_t>(p->image_matrices) & 3u) return accv::fail(ACCV_EINVAL, "%s: image_matrices is not aligned to its element size", who);
    if (int rc = accv_det::fill_planes(who, "", p->maps, p->channels, p->num_maps, plane, map_size, kMaxChannels, a.chan, a.chan_count)) return rc;
    a.scores = p->scores, a.indices = p->indices, a.classes = p->classes;
    a.image_hw = p->image_hw, a.matrices = p->image_matrices;
    a.boxes = boxes, a.out_scores = out_scores, a.labels = labels, a.source = source, a.extras = extras, a.sizes = out_sizes;
    Consts& k = a.k;
    k.thr = (float)p->score_threshold, k.min_h = (float)p->min_size[0], k.min_w = (float)p->min_size[1], k.iou_thr = (float)p->iou_threshold;
    k.has_thr = p->has_score_threshold ? 1 : 0, k.has_min = p->has_min_size ? 1 : 0, k.has_iou = p->has_iou_threshold ? 1 : 0;
    k.logits = p->scores_are_logits ? 1 : 0, k.clip = p->clip ? 1 : 0, k.order = p->order_corners ? 1 : 0;
    k.agnostic = p->class_agnostic ? 1 : 0;
    a.F = F, a.K = K, a.M = M, a.Wm = Wm, a.Hm = Hm, a.plane = plane;
    a.Wi = accv_bh::clamp_extent(p->image_w), a.Hi = accv_bh::clamp_extent(p->image_h);
    a.E = E, a.score_dt = p->score_dtype, a.map_dt = p->map_dtype, a.hw64 = p->image_hw_i64 ? 1 : 0;
    return ACCV_OK;
}

// ================================================================================================================= NMS
struct NmsArgs {
    const float* boxes;          // [F, N, 4]
    const float* scores;         // [F, N]
    const long long* labels;     // [F, N]
    const int* source;           // [F, N]
    const float* extras;         // [F, N, E]
    const long long* in_sizes;   // [F]
    float* out_boxes;            // [F, M, 4]
    float* out_scores;           // [F, M]
    long long* out_labels;       // [F, M]
    int* out_source;             // [F, M]
    float* out_extras;           // [F, M, E]
    long long* sizes;            // [F]
    long long F, N, M, pre;
    float thr;
    int E, has_thr, agnostic;
};

__host__ __device__ inline Box box_of(const NmsArgs& a, long long f, long long k)
{
    const float* p = a.boxes + (f * a.N + k) * 4;
    return make_box(p[0], p[1], p[2], p[3], a.labels[f * a.N + k]);
}

// how many slots of frame f exist
__host__ __device__ inline long long slots_of(const NmsArgs& a, long long f)
{
    const long long n = clamp_size(a.in_sizes[f], a.N);
    return n < a.pre ? n : a.pre;
}

// input slot k of frame f to output slot `slot`, bit for bit
__host__ __device__ inline void write_kept(const NmsArgs& a, long long f, long long slot, long long k)
{
    const long long in = f * a.N + k, o = f * a.M + slot;
    const float* src = a.boxes + in * 4;
    float* dst = a.out_boxes + o * 4;
    dst[0] = src[0], dst[1] = src[1], dst[2] = src[2], dst[3] = src[3];
    a.out_scores[o] = a.scores[in];
    a.out_labels[o] = a.labels[in];
    a.out_source[o] = a.source[in];
    for (int e = 0; e < a.E; ++e) a.out_extras[o * a.E + e] = a.extras[in * a.E + e];
}

__global__ __launch_bounds__(kThreads) void box_nms_kernel(const NmsArgs a)
{
    __shared__ Staged sb;
    __shared__ unsigned long long s_keep[kBlocks];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const long long f = blockIdx.x;
    const int M = (int)a.M;
    const int n = (int)slots_of(a, f);   // the same in every lane
    const bool nms_on = a.has_thr != 0;

    // 1. the boxes, a lane per slot
    unsigned alive = 0;   // bit c: my slot of chunk c exists and is not suppressed so far
    const int nchunks = (n + kThreads - 1) / kThreads;   // the same in every lane
#pragma unroll 1
    for (int c = 0; c < kChunks; ++c) {
        if (c >= nchunks) {   // no slot of this chunk exists: only its kept masks are needed, by phase 3
            if (lane == 0) s_keep[c * kWaves + wave] = 0ull;
            continue;
        }
        const int k = c * kThreads + tid;
        const bool in = k < n;
        if (nms_on) sb.put(k, in ? box_of(a, f, k) : no_box());   // phase 2 reads whole blocks of the chunks that exist
        const unsigned long long vote = __ballot(in);
        if (lane == 0) s_keep[c * kWaves + wave] = nms_on ? 0ull : vote;
        alive |= (in ? 1u : 0u) << c;
    }
    __syncthreads();

    // 2. greedy IoU NMS by blocks of one wave in slot order
    if (nms_on) greedy_walk(sb, s_keep, alive, n, M, a.thr, a.agnostic != 0);

    // 3. output slots from the kept masks, rows, padding, count
    int base[kChunks];
    const int total = Geo::slot_bases(s_keep, base);
#pragma unroll
    for (int c = 0; c < kChunks; ++c) {   // unrolled: base[] stays in registers
        const int k = c * kThreads + tid;
        if (k >= n) continue;
        const unsigned long long keep = s_keep[c * kWaves + wave];
        if (!((keep >> lane) & 1ull)) continue;
        const int slot = base[c] + __popcll(keep & ((1ull << lane) - 1ull));
        if (slot < M) write_kept(a, f, slot, k);
    }
    const int count = total < M ? total : M;
    for (int j = count + tid; j < M; j += kThreads)
        write_padding(a.out_boxes, a.out_scores, a.out_labels, a.out_source, a.out_extras, a.E, f * a.M + j);
    if (tid == 0) a.sizes[f] = count;
}

void nms_host_run(const NmsArgs& a)
{
    static thread_local Box kept_box[kMaxK];
    for (long long f = 0; f < a.F; ++f) {
        const long long n = slots_of(a, f);
        long long kept = 0;
        for (long long k = 0; k < n && kept < a.M; ++k) {
            Box me = no_box();
            if (a.has_thr) {
                me = box_of(a, f, k);
                bool dead = false;
                for (long long j = 0; j < kept && !dead; ++j) dead = suppresses(kept_box[j], me, a.thr, a.agnostic != 0);
                if (dead) continue;
            }
            kept_box[kept] = me;
            write_kept(a, f, kept++, k);
        }
        for (long long j = kept; j < a.M; ++j)
            write_padding(a.out_boxes, a.out_scores, a.out_labels, a.out_source, a.out_extras, a.E, f * a.M + j);
        a.sizes[f] = kept;
    }
}

// ACCV_OK with *empty = 1 when there is nothing to write; every check runs before anything reads the data
int nms_check_args(const char* who, const accv_box_nms_params* p, long long F, long long N, long long E, long long pre_max_size, long long M,
                   float* boxes, float* scores, long long* labels, int* source, float* extras, long long* out_sizes, NmsArgs& a, int* empty)
{
    *empty = 0;
    if (!p) return accv::fail(ACCV_EINVAL, "%s: null params", who);
    if (F < 0 || N < 0 || E < 0 || M < 0) return accv::fail(ACCV_EINVAL, "%s: negative size", who);
    if (N < 1 || N > kMaxK) return accv::fail(ACCV_EINVAL, "%s: N must be in 1..%d, got %lld", who, kMaxK, N);
    if (E > kMaxExtras) return accv::fail(ACCV_EINVAL, "%s: E must be in 0..%d, got %lld", who, kMaxExtras, E);
    if (pre_max_size < 1) return accv::fail(ACCV_EINVAL, "%s: pre_max_size must be at least 1, got %lld", who, pre_max_size);
    if (M < 1 || M > N || M > pre_max_size)
        return accv::fail(ACCV_EINVAL, "%s: M must be in 1..min(N, pre_max_size) = %lld, got %lld", who, N < pre_max_size ? N : pre_max_size, M);
    if (p->has_threshold && !(p->iou_threshold == p->iou_threshold)) return accv::fail(ACCV_EINVAL, "%s: iou_threshold is NaN", who);
    if (F == 0) {
        *empty = 1;
        return ACCV_OK;
    }
    if (!boxes || !scores || !labels || !source || !out_sizes || (E > 0 && !extras)) return accv::fail(ACCV_EINVAL, "%s: null output pointer", who);
    if (!p->boxes || !p->scores || !p->labels || !p->source || !p->sizes || (E > 0 && !p->extras))
        return accv::fail(ACCV_EINVAL, "%s: null input pointer", who);
    if ((reinterpret_cast<uintptr_t>(boxes) | reinterpret_cast<uintptr_t>(scores) | reinterpret_cast<uintptr_t>(source) |
         reinterpret_cast<uintptr_t>(p->boxes) | reinterpret_cast<uintptr_t>(p->scores) | reinterpret_cast<uintptr_t>(p->source) |
         (E > 0 ? reinterpret_cast<uintptr_t>(extras) | reinterpret_cast<uintptr_t>(p->extras) : 0)) & 3u)
        return accv::fail(ACCV_EINVAL, "%s: a 4-byte tensor is not aligned to its element size", who);
    if ((reinterpret_cast<uintptr_t>(labels) | reinterpret_cast<uintptr_t>(out_sizes) | reinterpret_cast<uintptr_t>(p->labels) |
         reinterpret_cast<uintptr_t>(p->sizes)) & 7u)
        return accv::fail(ACCV_EINVAL, "%s: labels and sizes must be 8-byte aligned", who);
    if (F > accv::kGridLimit) return accv::fail(ACCV_EINVAL, "%s: %lld workgroups exceed the grid limit", who, F);
    if (F > LLONG_MAX / 64 / kMaxChannels / N) return accv::fail(ACCV_EINVAL, "%s: sizes overflow", who);
    a.boxes = p->boxes, a.scores = p->scores, a.labels = p->labels, a.source = p->source, a.extras = p->extras, a.in_sizes = p->sizes;
    a.out_boxes = boxes, a.out_scores = scores, a.out_labels = labels, a.out_source = source, a.out_extras = extras, a.sizes = out_sizes;
    a.F = F, a.N = N, a.M = M, a.pre = pre_max_size;
    a.thr = (float)p->iou_threshold;
    a.E = (int)E, a.has_thr = p->has_threshold ? 1 : 0, a.agnostic = p->class_agnostic ? 1 : 0;
    return ACCV_OK;
}

}  // namespace

extern "C" {

int accv_box_decode(const accv_box_decode_params* params, long long F, long long K, long long Hm, long long Wm, long long M, float* boxes,
                    float* scores, long long* labels, int* source, float* extras, long long* out_sizes, void* stream)
{
    const char* who = "box_heatmap_decode";
    DecodeArgs a;
    int empty;
    if (int rc = decode_check_args(who, params, F, K, Hm, Wm, M, boxes, scores, labels, source, extras, out_sizes, a, &empty)) return rc;
    if (empty) return ACCV_OK;
    hipLaunchKernelGGL(box_decode_kernel, dim3((unsigned)a.F), dim3(kThreads), 0, static_cast<hipStream_t>(stream), a);
    return accv::check_launch(who);
}

int accv_box_decode_cpu(const accv_box_decode_params* params, long long F, long long K, long long Hm, long long Wm, long long M,
                        float* boxes, float* scores, long long* labels, int* source, float* extras, long long* out_sizes)
{
    const char* who = "box_heatmap_decode (host)";
    DecodeArgs a;
    int empty;
    if (int rc = decode_check_args(who, params, F, K, Hm, Wm, M, boxes, scores, labels, source, extras, out_sizes, a, &empty)) return rc;
    if (empty) return ACCV_OK;
    decode_host_run(a);
    return ACCV_OK;
}

int accv_box_nms(const accv_box_nms_params* params, long long F, long long N, long long E, long long pre_max_size, long long M,
                 float* boxes, float* scores, long long* labels, int* source, float* extras, long long* out_sizes, void* stream)
{
    const char* who = "nms_boxes";
    NmsArgs a;
    int empty;
    if (int rc = nms_check_args(who, params, F, N, E, pre_max_size, M, boxes, scores, labels, source, extras, out_sizes, a, &empty)) return rc;
    if (empty) return ACCV_OK;
    hipLaunchKernelGGL(box_nms_kernel, dim3((unsigned)a.F), dim3(kThreads), 0, static_cast<hipStream_t>(stream), a);
    return accv::check_launch(who);
}

int accv_box_nms_cpu(const accv_box_nms_params* params, long long F, long long N, long long E, long long pre_max_size, long long M,
                     float* boxes, float* scores, long long* labels, int* source, float* extras, long long* out_sizes)
{
    const char* who = "nms_boxes (host)";
    NmsArgs a;
    int empty;
    if (int rc = nms_check_args(who, params, F, N, E, pre_max_size, M, boxes, scores, labels, source, extras, out_sizes, a, &empty)) return rc;
    if (empty) return ACCV_OK;
    nms_host_run(a);
    return ACCV_OK;
}

}  // extern "C"
