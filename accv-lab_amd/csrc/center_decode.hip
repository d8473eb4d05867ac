// Prediction side of a centre-point head, the inverse of center_targets.hip: mmdet3d's CenterPointBBoxCoder.decode and the
// `circle` branch of CenterHead.get_bboxes for every task of the head in one launch — from the top-K peaks of each task's
// heat map and its regression maps to the filtered, circle-NMS'd, compacted detections, every output element written
// exactly once (padding: +0, source -1) and the kept count next to them.  Per-peak arithmetic: center_decode_arith.h.
//
// One workgroup of kThreads lanes per (frame, task); the K <= kMaxK peaks are walked in chunks of kThreads, a lane per
// peak, so a lane owns up to kChunks peaks and keeps their centres and an `alive` bit each in registers.
//   1. A lane gathers offset and height at its peak's cell, maps the centre to metres and tests validity; centres go to
//      LDS, the wave's __ballot of `valid` to s_valid[block].  A block is kWave consecutive ranks = one wave of one chunk.
//   2. Circle NMS, by blocks in rank order.  The wave that owns block j resolves it among its own lanes: the lowest alive
//      rank is kept, the alive lanes behind it test themselves against it, a __ballot gives the next — no workgroup
//      barrier inside the block.  It publishes the kept mask in s_keep[j]; after ONE barrier every lane tests its alive
//      peaks of later blocks against the block's kept centres (LDS broadcast reads).  That is K / kWave barriers, not K.
//      A block without a valid peak is passed over without a barrier; one whose peaks have all been suppressed costs its
//      barrier and nothing else.  The walk stops once post_max_size peaks are kept.  Without NMS s_keep = s_valid.
//   3. The output slot of a kept peak is the popcount of the kept masks of the blocks before it plus that of the lower
//      lanes of its own (ballot + popcount through LDS, as center_targets.hip ranks).  Kept lanes below the cut gather the
//      remaining channels and store their row; the rest of each row of M slots is filled.
// No atomics and no workspace: the order is the rank order, so the result is bitwise reproducible.  Launch and latency
// bound work (a few hundred peaks per frame and task): no MFMA.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>

#include "accv_common.h"
#include "accv_numeric.h"
#include "center_decode_arith.h"
#include "detect_common.h"

#pragma clang fp contract(off)

namespace {

using namespace accv_cd;

using accv::load_any;

constexpr int kWave = 64;
constexpr int kThreads = 256;               // and peaks per chunk
using Geo = accv_det::Geometry<kMaxK, kThreads, kWave>;
constexpr int kWaves = Geo::kWaves, kChunks = Geo::kChunks, kBlocks = Geo::kBlocks;

static_assert(kMaxTasks == ACCV_CD_MAX_TASKS && kMaxMaps == ACCV_CD_MAX_MAPS && kMaxClasses == ACCV_CD_MAX_CLASSES &&
                  kMaxK == ACCV_CD_MAX_K,
              "center_decode_arith.h and accv_hip.h disagree");

struct Args {
    const void* scores[kMaxTasks];                  // [B, K]
    const long long* indices[kMaxTasks];            // [B, K]
    const long long* classes[kMaxTasks];            // [B, K]
    const void* chan[kMaxTasks][kMaxChannels];      // concatenated channel c of task t: its plane in frame 0 of its map
    unsigned char chan_count[kMaxTasks][kMaxChannels];   // the channel count of that map
    float nms[kMaxTasks];
    unsigned char has_nms[kMaxTasks];
    unsigned char task_first[kMaxTasks + 1], class_ids[kMaxClasses];
    float* boxes;                                   // [T, B, M, C - 1]
    float* out_scores;                              // [T, B, M]
    long long* labels;                              // [T, B, M]
    int* source;                                    // [T, B, M]
    long long* sizes;                               // [T, B]
    Consts k;
    long long B, K, M, W, plane;
    int C, T, score_dt, map_dt;
};

// concatenated channel c of task t at `cell` of frame b
__host__ __device__ inline float channel_at(const Args& a, int t, int c, long long b, long long cell)
{
    return accv_det::channel_at(a.chan[t], a.chan_count[t], a.plane, a.map_dt, c, b, cell);
}

// steps 1 to 4 for peak k of (b, t): whether it is valid, and its centre, height, score, cell and global class id.  An
// illegal index or class position reads nothing from the maps.
__host__ __device__ inline bool centre_of(const Args& a, int t, long long b, long long k, float& x, float& y, float& z, float& score,
                                          long long& cell, int& label)
{
    const long long at = b * a.K + k;
    cell = a.indices[t][at];
    const long long pos = a.classes[t][at];
    const int first = a.task_first[t], count = a.task_first[t + 1] - first;
    if (cell < 0 || cell >= a.plane || pos < 0 || pos >= count) return false;
    label = a.class_ids[first + pos];
    const long long ys = cell / a.W, xs = cell - ys * a.W;
    x = coordinate(xs, channel_at(a, t, 0, b, cell), a.k.f, a.k.vs0, a.k.pc0);
    y = coordinate(ys, channel_at(a, t, 1, b, cell), a.k.f, a.k.vs1, a.k.pc1);
    z = channel_at(a, t, 2, b, cell);
    score = score_of(a.k, load_any(a.scores[t], at, a.score_dt));
    return passes(a.k, score, x, y, z);
}

// everything a kept peak writes: slot `slot` of row (t, b), from peak rank k (a valid one)
__host__ __device__ inline void write_peak(const Args& a, int t, long long b, long long row0, long long slot, long long k)
{
    float x, y, score, g[kMaxChannels], row[kMaxChannels - 1];
    long long cell;
    int label;
    centre_of(a, t, b, k, x, y, g[2], score, cell, label);
#pragma unroll
    for (int c = 3; c < 8; ++c) g[c] = channel_at(a, t, c, b, cell);
    if (a.C == 10) g[8] = channel_at(a, t, 8, b, cell), g[9] = channel_at(a, t, 9, b, cell);
    box_row(a.k, g, a.C, x, y, row);
    const long long o = row0 + slot;
    float* out = a.boxes + o * (a.C - 1);
#pragma unroll
    for (int c = 0; c < 7; ++c) out[c] = row[c];
    if (a.C == 10) out[7] = row[7], out[8] = row[8];
    a.out_scores[o] = score;
    a.labels[o] = label;
    a.source[o] = (int)k;
}

// the filler of padding slot j of row (t, b)
__host__ __device__ inline void write_padding(const Args& a, long long row0, long long j)
{
    const long long o = row0 + j;
    float* out = a.boxes + o * (a.C - 1);
    for (int c = 0; c < a.C - 1; ++c) out[c] = 0.0f;
    a.out_scores[o] = 0.0f;
    a.labels[o] = 0;
    a.source[o] = -1;
}

// ------------------------------------------------------------------------------------------------------------- device
__global__ __launch_bounds__(kThreads) void center_point_decode_kernel(const Args a)
{
    __shared__ float s_x[kMaxK], s_y[kMaxK];
    __shared__ unsigned long long s_valid[kBlocks], s_keep[kBlocks];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const long long b = blockIdx.x;
    const int t = blockIdx.y;
    const int K = (int)a.K, M = (int)a.M;
    const bool nms_on = a.has_nms[t] != 0;
    const long long row0 = ((long long)t * a.B + b) * a.M;

    // 1. centres and validity, a lane per peak
    float x[kChunks], y[kChunks];
    unsigned alive = 0;   // bit c: my peak of chunk c is valid and not suppressed so far
#pragma unroll
    for (int c = 0; c < kChunks; ++c) {
        const int k = c * kThreads + tid;
        x[c] = y[c] = 0.0f;
        bool valid = false;
        if (k < K) {
            float z, score;
            long long cell;
            int label;
            valid = centre_of(a, t, b, k, x[c], y[c], z, score, cell, label);
        }
        s_x[k] = x[c], s_y[k] = y[c];
        const unsigned long long vote = __ballot(valid);
        if (lane == 0) s_valid[c * kWaves + wave] = vote, s_keep[c * kWaves + wave] = nms_on ? 0ull : vote;
        alive |= (valid ? 1u : 0u) << c;
    }
    __syncthreads();

    // 2. circle NMS by blocks of one wave in rank order
    if (nms_on) {
        const float thr = a.nms[t];
        const int nblocks = (K + kWave - 1) / kWave;
        int kept = 0;   // the same in every lane
        for (int j = 0; j < nblocks && kept < M; ++j) {
            if (s_valid[j] == 0) continue;   // the same in every lane: no barrier is skipped by some
            const int first = j * kWave;
            if (wave == j % kWaves) {
                const int c = j / kWaves;
                bool live = (alive >> c) & 1u;
                const float mx = s_x[first + lane], my = s_y[first + lane];
                unsigned long long todo = __ballot(live), keep = 0;
                while (todo) {
                    const int i = __ffsll((long long)todo) - 1;   // the lowest alive rank: kept
                    keep |= 1ull << i;
                    if (live && lane > i && suppresses(s_x[first + i], s_y[first + i], mx, my, thr)) live = false;
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
                const float xj = s_x[first + i], yj = s_y[first + i];
#pragma unroll
                for (int c = 0; c < kChunks; ++c)
                    if (c * kWaves + wave > j && ((alive >> c) & 1u) && suppresses(xj, yj, x[c], y[c], thr)) alive &= ~(1u << c);
            }
        }
    }

    // 3. output slots from the kept masks, rows, padding, count
    int total = 0, base[kChunks];
#pragma unroll
    for (int j = 0; j < kBlocks; ++j) {
        if (j % kWaves == wave) base[j / kWaves] = total;
        total += __popcll(s_keep[j]);
    }
#pragma unroll
    for (int c = 0; c < kChunks; ++c) {
        const int k = c * kThreads + tid;
        if (k >= K) continue;
        const unsigned long long keep = s_keep[c * kWaves + wave];
        if (!((keep >> lane) & 1ull)) continue;
        const int slot = base[c] + __popcll(keep & ((1ull << lane) - 1ull));
        if (slot < M) write_peak(a, t, b, row0, slot, k);
    }
    const int n = total < M ? total : M;
    for (int j = n + tid; j < M; j += kThreads) write_padding(a, row0, j);
    if (tid == 0) a.sizes[(long long)t * a.B + b] = n;
}

// --------------------------------------------------------------------------------------------------------------- host
void host_run(const Args& a)
{
    float kx[kMaxK], ky[kMaxK];
    for (int t = 0; t < a.T; ++t) {
        for (long long b = 0; b < a.B; ++b) {
            const long long row0 = ((long long)t * a.B + b) * a.M;
            long long kept = 0;
            for (long long k = 0; k < a.K && kept < a.M; ++k) {
                float x, y, z, score;
                long long cell;
                int label;
                if (!centre_of(a, t, b, k, x, y, z, score, cell, label)) continue;
                bool dead = false;
                if (a.has_nms[t])
                    for (long long j = 0; j < kept && !dead; ++j) dead = suppresses(kx[j], ky[j], x, y, a.nms[t]);
                if (dead) continue;
                kx[kept] = x, ky[kept] = y;
                write_peak(a, t, b, row0, kept++, k);
            }
            for (long long j = kept; j < a.M; ++j) write_padding(a, row0, j);
            a.sizes[(long long)t * a.B + b] = kept;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------- checks
// ACCV_OK with *empty = 1 when there is nothing to write; every check runs before anything else reads the arguments
int check_args(const char* who, const accv_center_point_decode_params* p, long long B, long long K, long long H, long long W,
               long long M, float* boxes, float* out_scores, long long* labels, int* source, long long* out_sizes, Args& a,
               int* empty)
{
    *empty = 0;
    if (!p) return accv::fail(ACCV_EINVAL, "%s: null params", who);
    if (B < 0 || K < 0 || H < 0 || W < 0 || M < 0) return accv::fail(ACCV_EINVAL, "%s: negative size", who);
    if (p->num_tasks < 1 || p->num_tasks > kMaxTasks)
        return accv::fail(ACCV_EINVAL, "%s: 1..%d tasks supported, got %d", who, kMaxTasks, p->num_tasks);
    if (K < 1 || K > kMaxK) return accv::fail(ACCV_EINVAL, "%s: K must be in 1..%d, got %lld", who, kMaxK, K);
    if (M < 1 || M > K) return accv::fail(ACCV_EINVAL, "%s: M must be in 1..K = %lld, got %lld", who, K, M);
    if (W < 1 || H < 1 || W > INT_MAX / H) return accv::fail(ACCV_EINVAL, "%s: a grid of %lld x %lld cells is empty or exceeds 2^31 - 1", who, W, H);
    if (p->score_dtype < accv::kF32 || p->score_dtype > accv::kBF16 || p->map_dtype < accv::kF32 || p->map_dtype > accv::kBF16)
        return accv::fail(ACCV_EINVAL, "%s: unknown dtype code %d / %d (0 f32, 1 f16, 2 bf16)", who, p->score_dtype, p->map_dtype);
    const int T = p->num_tasks;
    if (p->task_first[0] != 0) return accv::fail(ACCV_EINVAL, "%s: task_first[0] must be 0", who);
    for (int t = 0; t < T; ++t)
        if (p->task_first[t + 1] < p->task_first[t] || p->task_first[t + 1] > kMaxClasses)
            return accv::fail(ACCV_EINVAL, "%s: task_first must ascend and stay within %d classes", who, kMaxClasses);
    for (int c = 0; c < p->task_first[T]; ++c)
        if (p->class_ids[c] >= kMaxClasses) return accv::fail(ACCV_EINVAL, "%s: class id %d is outside [0, %d)", who, (int)p->class_ids[c], kMaxClasses);
    int C = 0;
    for (int t = 0; t < T; ++t) {
        if (p->num_maps[t] < 1 || p->num_maps[t] > kMaxMaps)
            return accv::fail(ACCV_EINVAL, "%s: 1..%d maps per task supported, task %d has %d", who, kMaxMaps, t, p->num_maps[t]);
        long long sum = 0;
        for (int i = 0; i < p->num_maps[t]; ++i) {
            if (p->channels[t][i] < 0) return accv::fail(ACCV_EINVAL, "%s: map %d of task %d has a negative channel count", who, i, t);
            sum += p->channels[t][i];
        }
        if (sum != 8 && sum != 10) return accv::fail(ACCV_EINVAL, "%s: the maps of task %d hold %lld channels, 8 or 10 are needed", who, t, sum);
        if (t > 0 && sum != C) return accv::fail(ACCV_EINVAL, "%s: task %d holds %lld channels, task 0 %d", who, t, sum, C);
        C = (int)sum;
        if (p->has_nms[t] && !(p->nms_threshold[t] == p->nms_threshold[t])) return accv::fail(ACCV_EINVAL, "%s: nms_threshold[%d] is NaN", who, t);
    }
    if (!(p->voxel_size[0] > 0.0) || !(p->voxel_size[1] > 0.0) || !(p->out_size_factor > 0.0))
        return accv::fail(ACCV_EINVAL, "%s: voxel_size and out_size_factor must be positive", who);
    if (p->has_score_threshold && !(p->score_threshold == p->score_threshold)) return accv::fail(ACCV_EINVAL, "%s: score_threshold is NaN", who);
    if (p->has_post_center_range)
        for (int i = 0; i < 6; ++i)
            if (!(p->post_center_range[i] == p->post_center_range[i])) return accv::fail(ACCV_EINVAL, "%s: post_center_range[%d] is NaN", who, i);
    if (B == 0) {
        *empty = 1;
        return ACCV_OK;
    }
    if (int rc = accv_det::check_outputs(who, B, boxes, out_scores, labels, source, out_sizes)) return rc;
    const long long plane = H * W;
    if (B > LLONG_MAX / 64 / kMaxChannels / plane || B > LLONG_MAX / 64 / kMaxChannels / kMaxTasks / K)
        return accv::fail(ACCV_EINVAL, "%s: sizes overflow", who);
    const uintptr_t score_mask = (uintptr_t)accv::elem_size(p->score_dtype) - 1u, map_size = (uintptr_t)accv::elem_size(p->map_dtype);
    for (int t = 0; t < T; ++t) {
        if (!p->scores[t] || !p->indices[t] || !p->classes[t]) return accv::fail(ACCV_EINVAL, "%s: null peaks pointer of task %d", who, t);
        if ((reinterpret_cast<uintptr_t>(p->scores[t]) & score_mask) ||
            ((reinterpret_cast<uintptr_t>(p->indices[t]) | reinterpret_cast<uintptr_t>(p->classes[t])) & 7u))
            return accv::fail(ACCV_EINVAL, "%s: the peaks of task %d are not aligned to their element size", who, t);
        a.scores[t] = p->scores[t], a.indices[t] = p->indices[t], a.classes[t] = p->classes[t];
        char of[32];
        snprintf(of, sizeof of, " of task %d", t);
        if (int rc = accv_det::fill_planes(who, of, p->maps[t], p->channels[t], p->num_maps[t], plane, map_size, kMaxChannels, a.chan[t],
                                           a.chan_count[t]))
            return rc;
        a.nms[t] = (float)p->nms_threshold[t];
        a.has_nms[t] = p->has_nms[t] ? 1 : 0;
    }
    for (int t = T; t < kMaxTasks; ++t) {
        a.scores[t] = nullptr, a.indices[t] = nullptr, a.classes[t] = nullptr, a.nms[t] = 0.0f, a.has_nms[t] = 0;
        for (int c = 0; c < kMaxChannels; ++c) a.chan[t][c] = nullptr, a.chan_count[t][c] = 0;
    }
    for (int t = 0; t <= kMaxTasks; ++t) a.task_first[t] = p->task_first[t <= T ? t : T];
    for (int c = 0; c < kMaxClasses; ++c) a.class_ids[c] = p->class_ids[c];
    a.boxes = boxes, a.out_scores = out_scores, a.labels = labels, a.source = source, a.sizes = out_sizes;
    Consts& k = a.k;
    k.pc0 = (float)p->pc_range[0], k.pc1 = (float)p->pc_range[1];
    k.vs0 = (float)p->voxel_size[0], k.vs1 = (float)p->voxel_size[1];
    k.f = (float)p->out_size_factor;
    k.thr = (float)p->score_threshold;
    for (int i = 0; i < 3; ++i) k.lo[i] = (float)p->post_center_range[i], k.hi[i] = (float)p->post_center_range[3 + i];
    k.has_thr = p->has_score_threshold ? 1 : 0, k.has_range = p->has_post_center_range ? 1 : 0;
    k.logits = p->scores_are_logits ? 1 : 0, k.norm_bbox = p->norm_bbox ? 1 : 0, k.bottom = p->bottom_center ? 1 : 0;
    if (!(k.vs0 > 0.0f) || !(k.vs1 > 0.0f) || !(k.f > 0.0f))
        return accv::fail(ACCV_EINVAL, "%s: voxel_size and out_size_factor must be positive in float32", who);
    a.B = B, a.K = K, a.M = M, a.W = W, a.plane = plane;
    a.C = C, a.T = T, a.score_dt = p->score_dtype, a.map_dt = p->map_dtype;
    return ACCV_OK;
}

}  // namespace

extern "C" {

int accv_center_point_decode(const accv_center_point_decode_params* params, long long B, long long K, long long H,
                             long long W, long long M, float* boxes, float* out_scores, long long* labels, int* source,
                             long long* out_sizes, void* stream)
{
    const char* who = "center_point_decode";
    Args a;
    int empty;
    if (int rc = check_args(who, params, B, K, H, W, M, boxes, out_scores, labels, source, out_sizes, a, &empty)) return rc;
    if (empty) return ACCV_OK;
    hipLaunchKernelGGL(center_point_decode_kernel, dim3((unsigned)a.B, (unsigned)a.T), dim3(kThreads), 0, static_cast<hipStream_t>(stream), a);
    return accv::check_launch(who);
}

int accv_center_point_decode_host(const accv_center_point_decode_params* params, long long B, long long K, long long H,
                                  long long W, long long M, float* boxes, float* out_scores, long long* labels, int* source,
                                  long long* out_sizes)
{
    const char* who = "center_point_decode (host)";
    Args a;
    int empty;
    if (int rc = check_args(who, params, B, K, H, W, M, boxes, out_scores, labels, source, out_sizes, a, &empty)) return rc;
    if (empty) return ACCV_OK;
    host_run(a);
    return ACCV_OK;
}

}  // extern "C"
