// Rotated BEV IoU and rotated NMS for centre-point detections: the `rotate` branch of mmdet3d's CenterHead.get_bboxes
// (nms_bev over mmcv's nms_rotated), on what center_decode.hip writes with its circle NMS switched off.  Per-pair arithmetic:
// rotated_iou_arith.h.
//
// rotated_iou_bev_kernel: the [B, Na, Nb] IoU matrix of two ragged box sets.  One workgroup per kTile x kTile tile of one
// frame; the tile's B-side boxes with cos / sin of their yaw and its A-side boxes are prepared once into LDS, a lane owns
// one column and walks the rows.  Every output element is written exactly once; pairs beyond either size are +0.
//
// rotated_nms_bev_kernel: one workgroup of kThreads lanes per (frame, task), all tasks in one launch, laid out as
// center_decode.hip and with its wave-block walk:
//   1. a lane per input slot, kThreads slots a chunk: the BEV columns (0, 1, 3, 4, 6) of the slot are prepared into LDS
//      (centre, half extents, yaw, cos / sin, circumscribed radius: once per box, not per pair).  Only the first
//      n = min(sample_sizes[b], pre_max_size) slots exist; `alive` holds a bit per chunk.
//   2. by blocks of kWave slots in slot order: the wave that owns block j resolves it among its own lanes (the lowest alive
//      slot is kept, the alive lanes behind it test themselves against it, a __ballot gives the next) and publishes the kept
//      mask; after ONE barrier every lane tests its alive boxes of later blocks against the block's kept boxes (LDS
//      broadcast reads).  The predicate is the circumscribed-circle reject and then iou > threshold[t], strictly.  A box that
//      is not ok is kept and suppresses nothing.  The walk stops once M boxes are kept.  Without a threshold kept = alive.
//   3. output slots from the popcounts of the kept masks; kept rows are copied bit for bit (all D box columns, score, label,
//      source), the rest of the M slots is filled (+0, source -1), the count goes to sizes.
// No atomics, no workspace, no host synchronisation: the order is the slot order, so the result is bitwise reproducible.
// Latency-bound geometry on a few hundred boxes: no MFMA.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>

#include "accv_common.h"
#include "detect_common.h"
#include "rotated_iou_arith.h"

#pragma clang fp contract(off)

namespace {

using namespace accv_ri;

constexpr int kMaxTasks = ACCV_RN_MAX_TASKS;
constexpr int kMaxN = ACCV_RN_MAX_N;
using accv_det::clamp_size;
constexpr int kWave = 64;
constexpr int kThreads = 256;               // and slots per chunk
using Geo = accv_det::Geometry<kMaxN, kThreads, kWave>;
constexpr int kWaves = Geo::kWaves, kChunks = Geo::kChunks, kBlocks = Geo::kBlocks;
constexpr int kTile = 64;                   // IoU matrix: rows and columns per workgroup
constexpr int kCols[5] = {0, 1, 3, 4, 6};   // (x, y, dx, dy, yaw) inside a box row

static_assert(kTile == kWave && kThreads % kTile == 0, "a wave covers a row of a tile");

// the prepared boxes of a workgroup, structure of arrays (a lane per box: conflict-free; one box for all: broadcast)
template <int N>
struct Staged {
    float x[N], y[N], hx[N], hy[N], yaw[N], c[N], s[N], area[N], r[N];
    unsigned char ok[N];

    __device__ void put(int i, const Box& b)
    {
        x[i] = b.x, y[i] = b.y, hx[i] = b.hx, hy[i] = b.hy, yaw[i] = b.yaw, c[i] = b.c, s[i] = b.s, area[i] = b.area, r[i] = b.r;
        ok[i] = b.ok ? 1 : 0;
    }
    __device__ Box get(int i) const
    {
        Box b;
        b.x = x[i], b.y = y[i], b.hx = hx[i], b.hy = hy[i], b.yaw = yaw[i], b.c = c[i], b.s = s[i], b.area = area[i], b.r = r[i];
        b.ok = ok[i] != 0;
        return b;
    }
};

__host__ __device__ inline Box no_box()
{
    Box b;
    b.x = b.y = b.hx = b.hy = b.yaw = b.s = b.area = b.r = 0.0f;
    b.c = 1.0f;
    b.ok = false;
    return b;
}

// ================================================================================================================ IoU
struct IouArgs {
    const float *a, *b;                 // [B, Na, 5], [B, Nb, 5]
    const long long *a_sizes, *b_sizes; // [B]
    float* out;                         // [B, Na, Nb]
    long long B, Na, Nb, tiles_a, tiles_b;
};

__host__ __device__ inline Box box5(const float* p) { return prepare(p[0], p[1], p[2], p[3], p[4]); }

__global__ __launch_bounds__(kThreads) void rotated_iou_bev_kernel(const IouArgs g)
{
    __shared__ Staged<kTile> sa, sb;
    const int tid = threadIdx.x, col = tid % kTile, row0 = tid / kTile;
    const long long tile = blockIdx.x;
    const long long tb = tile % g.tiles_b, ta = (tile / g.tiles_b) % g.tiles_a, f = tile / (g.tiles_b * g.tiles_a);
    const long long na = clamp_size(g.a_sizes[f], g.Na), nb = clamp_size(g.b_sizes[f], g.Nb);
    const long long i0 = ta * kTile, j0 = tb * kTile;
    const bool any = i0 < na && j0 < nb;   // the same in every lane
    if (any) {
        if (tid < kTile) {
            const long long j = j0 + tid;
            sb.put(tid, j < nb ? box5(g.b + (f * g.Nb + j) * 5) : no_box());
        } else if (tid < 2 * kTile) {
            const long long i = i0 + (tid - kTile);
            sa.put(tid - kTile, i < na ? box5(g.a + (f * g.Na + i) * 5) : no_box());
        }
        __syncthreads();
    }
    const long long j = j0 + col;
    if (j >= g.Nb) return;
    const Box mine = any ? sb.get(col) : no_box();
#pragma unroll 1
    for (int r = row0; r < kTile; r += kThreads / kTile) {
        const long long i = i0 + r;
        if (i >= g.Na) break;
        float v = 0.0f;
        if (any) v = iou(sa.get(r), mine);
        g.out[(f * g.Na + i) * g.Nb + j] = v;
    }
}

void iou_host_run(const IouArgs& g)
{
    for (long long f = 0; f < g.B; ++f) {
        const long long na = clamp_size(g.a_sizes[f], g.Na), nb = clamp_size(g.b_sizes[f], g.Nb);
        for (long long i = 0; i < g.Na; ++i) {
            float* row = g.out + (f * g.Na + i) * g.Nb;
            const Box a = i < na ? box5(g.a + (f * g.Na + i) * 5) : no_box();
            for (long long j = 0; j < g.Nb; ++j) row[j] = (i < na && j < nb) ? iou(a, box5(g.b + (f * g.Nb + j) * 5)) : 0.0f;
        }
    }
}

// ACCV_OK with *empty = 1 when there is nothing to write; every check runs before anything reads the data
int iou_check_args(const char* who, const float* a, const long long* a_sizes, const float* b, const long long* b_sizes, long long B,
                   long long Na, long long Nb, float* out, IouArgs& g, int* empty)
{
    *empty = 0;
    if (B < 0 || Na < 0 || Nb < 0) return accv::fail(ACCV_EINVAL, "%s: negative size", who);
    if (B == 0 || Na == 0 || Nb == 0) {
        *empty = 1;
        return ACCV_OK;
    }
    if (!a || !b || !a_sizes || !b_sizes || !out) return accv::fail(ACCV_EINVAL, "%s: null pointer", who);
    if ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(out)) & 3u)
        return accv::fail(ACCV_EINVAL, "%s: a float32 tensor is not aligned to its element size", who);
    if ((reinterpret_cast<uintptr_t>(a_sizes) | reinterpret_cast<uintptr_t>(b_sizes)) & 7u)
        return accv::fail(ACCV_EINVAL, "%s: the sizes must be 8-byte aligned", who);
    if (Na > LLONG_MAX / 64 / Nb || B > LLONG_MAX / 64 / (Na * Nb)) return accv::fail(ACCV_EINVAL, "%s: sizes overflow", who);
    const long long tiles_a = (Na + kTile - 1) / kTile, tiles_b = (Nb + kTile - 1) / kTile;
    if (tiles_a > accv::kGridLimit / tiles_b || B > accv::kGridLimit / (tiles_a * tiles_b))
        return accv::fail(ACCV_EINVAL, "%s: %lld x %lld x %lld tiles exceed the grid limit", who, B, tiles_a, tiles_b);
    g.a = a, g.b = b, g.a_sizes = a_sizes, g.b_sizes = b_sizes, g.out = out;
    g.B = B, g.Na = Na, g.Nb = Nb, g.tiles_a = tiles_a, g.tiles_b = tiles_b;
    return ACCV_OK;
}

// ================================================================================================================ NMS
struct Args {
    const float* boxes[kMaxTasks];        // [B, N, D]
    const float* scores[kMaxTasks];       // [B, N]
    const long long* labels[kMaxTasks];   // [B, N]
    const int* source[kMaxTasks];         // [B, N]
    const long long* in_sizes[kMaxTasks]; // [B]
    float thr[kMaxTasks];
    unsigned char has_thr[kMaxTasks];
    float* out_boxes;                     // [T, B, M, D]
    float* out_scores;                    // [T, B, M]
    long long* out_labels;                // [T, B, M]
    int* out_source;                      // [T, B, M]
    long long* sizes;                     // [T, B]
    long long B, N, M, pre;
    int D, T;
};

// the BEV box of slot k of row (b, t)
__host__ __device__ inline Box box_of(const Args& a, int t, long long b, long long k)
{
    const float* p = a.boxes[t] + (b * a.N + k) * a.D;
    return prepare(p[kCols[0]], p[kCols[1]], p[kCols[2]], p[kCols[3]], p[kCols[4]]);
}

// how many slots of row (b, t) exist
__host__ __device__ inline long long slots_of(const Args& a, int t, long long b)
{
    const long long n = clamp_size(a.in_sizes[t][b], a.N);
    return n < a.pre ? n : a.pre;
}

// does the kept box `kept` suppress the later box `later`: never when either is not ok, whatever the threshold's sign
__host__ __device__ inline bool suppresses(const Box& kept, const Box& later, float thr)
{
    return kept.ok && later.ok && iou(later, kept) > thr;
}

// input slot k of row (b, t) to output slot `slot`, bit for bit
__host__ __device__ inline void write_kept(const Args& a, int t, long long b, long long row0, long long slot, long long k)
{
    const long long in = b * a.N + k, o = row0 + slot;
    const float* src = a.boxes[t] + in * a.D;
    float* dst = a.out_boxes + o * a.D;
    for (int c = 0; c < a.D; ++c) dst[c] = src[c];
    a.out_scores[o] = a.scores[t][in];
    a.out_labels[o] = a.labels[t][in];
    a.out_source[o] = a.source[t][in];
}

__host__ __device__ inline void write_padding(const Args& a, long long row0, long long j)
{
    const long long o = row0 + j;
    float* dst = a.out_boxes + o * a.D;
    for (int c = 0; c < a.D; ++c) dst[c] = 0.0f;
    a.out_scores[o] = 0.0f;
    a.out_labels[o] = 0;
    a.out_source[o] = -1;
}

__global__ __launch_bounds__(kThreads) void rotated_nms_bev_kernel(const Args a)
{
    __shared__ Staged<kMaxN> sb;
    __shared__ unsigned long long s_keep[kBlocks];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const long long b = blockIdx.x;
    const int t = blockIdx.y;
    const int M = (int)a.M;
    const int n = (int)slots_of(a, t, b);   // the same in every lane
    const bool nms_on = a.has_thr[t] != 0;
    const long long row0 = ((long long)t * a.B + b) * a.M;

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
        if (nms_on) sb.put(k, in ? box_of(a, t, b, k) : no_box());   // phase 2 reads whole blocks of the chunks that exist
        const unsigned long long vote = __ballot(in);
        if (lane == 0) s_keep[c * kWaves + wave] = nms_on ? 0ull : vote;
        alive |= (in ? 1u : 0u) << c;
    }
    __syncthreads();

    // 2. rotated NMS by blocks of one wave in slot order
    if (nms_on) {
        const float thr = a.thr[t];
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
                    if (live && lane > i && suppresses(sb.get(first + i), mine, thr)) live = false;
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
                    if (c * kWaves + wave > j && ((alive >> c) & 1u) && suppresses(kj, sb.get(c * kThreads + tid), thr)) alive &= ~(1u << c);
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
        if (k >= n) continue;
        const unsigned long long keep = s_keep[c * kWaves + wave];
        if (!((keep >> lane) & 1ull)) continue;
        const int slot = base[c] + __popcll(keep & ((1ull << lane) - 1ull));
        if (slot < M) write_kept(a, t, b, row0, slot, k);
    }
    const int count = total < M ? total : M;
    for (int j = count + tid; j < M; j += kThreads) write_padding(a, row0, j);
    if (tid == 0) a.sizes[(long long)t * a.B + b] = count;
}

void nms_host_run(const Args& a)
{
    static thread_local Box kept_box[kMaxN];
    for (int t = 0; t < a.T; ++t) {
        for (long long b = 0; b < a.B; ++b) {
            const long long row0 = ((long long)t * a.B + b) * a.M, n = slots_of(a, t, b);
            long long kept = 0;
            for (long long k = 0; k < n && kept < a.M; ++k) {
                Box me = no_box();
                if (a.has_thr[t]) {
                    me = box_of(a, t, b, k);
                    bool dead = false;
                    for (long long j = 0; j < kept && !dead; ++j) dead = suppresses(kept_box[j], me, a.thr[t]);
                    if (dead) continue;
                }
                kept_box[kept] = me;
                write_kept(a, t, b, row0, kept++, k);
            }
            for (long long j = kept; j < a.M; ++j) write_padding(a, row0, j);
            a.sizes[(long long)t * a.B + b] = kept;
        }
    }
}

// ACCV_OK with *empty = 1 when there is nothing to write; every check runs before anything reads the data
int nms_check_args(const char* who, const accv_rotated_nms_params* p, long long B, long long N, long long D, long long pre_max_size,
                   long long M, float* boxes, float* scores, long long* labels, int* source, long long* out_sizes, Args& a, int* empty)
{
    *empty = 0;
    if (!p) return accv::fail(ACCV_EINVAL, "%s: null params", who);
    if (B < 0 || N < 0 || D < 0 || M < 0) return accv::fail(ACCV_EINVAL, "%s: negative size", who);
    if (p->num_tasks < 1 || p->num_tasks > kMaxTasks)
        return accv::fail(ACCV_EINVAL, "%s: 1..%d tasks supported, got %d", who, kMaxTasks, p->num_tasks);
    if (N < 1 || N > kMaxN) return accv::fail(ACCV_EINVAL, "%s: N must be in 1..%d, got %lld", who, kMaxN, N);
    if (D < ACCV_RN_MIN_D || D > ACCV_RN_MAX_D)
        return accv::fail(ACCV_EINVAL, "%s: D must be in %d..%d, got %lld", who, ACCV_RN_MIN_D, ACCV_RN_MAX_D, D);
    if (pre_max_size < 1) return accv::fail(ACCV_EINVAL, "%s: pre_max_size must be at least 1, got %lld", who, pre_max_size);
    if (M < 1 || M > N || M > pre_max_size)
        return accv::fail(ACCV_EINVAL, "%s: M must be in 1..min(N, pre_max_size) = %lld, got %lld", who, N < pre_max_size ? N : pre_max_size, M);
    const int T = p->num_tasks;
    for (int t = 0; t < T; ++t)
        if (p->has_threshold[t] && !(p->iou_threshold[t] == p->iou_threshold[t]))
            return accv::fail(ACCV_EINVAL, "%s: iou_threshold[%d] is NaN", who, t);
    if (B == 0) {
        *empty = 1;
        return ACCV_OK;
    }
    if (int rc = accv_det::check_outputs(who, B, boxes, scores, labels, source, out_sizes)) return rc;
    if (B > LLONG_MAX / 64 / kMaxTasks / ACCV_RN_MAX_D / N) return accv::fail(ACCV_EINVAL, "%s: sizes overflow", who);
    for (int t = 0; t < T; ++t) {
        if (!p->boxes[t] || !p->scores[t] || !p->labels[t] || !p->source[t] || !p->sizes[t])
            return accv::fail(ACCV_EINVAL, "%s: null input pointer of task %d", who, t);
        if ((reinterpret_cast<uintptr_t>(p->boxes[t]) | reinterpret_cast<uintptr_t>(p->scores[t]) | reinterpret_cast<uintptr_t>(p->source[t])) & 3u)
            return accv::fail(ACCV_EINVAL, "%s: a 4-byte input of task %d is not aligned to its element size", who, t);
        if ((reinterpret_cast<uintptr_t>(p->labels[t]) | reinterpret_cast<uintptr_t>(p->sizes[t])) & 7u)
            return accv::fail(ACCV_EINVAL, "%s: labels and sizes of task %d must be 8-byte aligned", who, t);
        a.boxes[t] = p->boxes[t], a.scores[t] = p->scores[t], a.labels[t] = p->labels[t], a.source[t] = p->source[t];
        a.in_sizes[t] = p->sizes[t];
        a.thr[t] = (float)p->iou_threshold[t];
        a.has_thr[t] = p->has_threshold[t] ? 1 : 0;
    }
    for (int t = T; t < kMaxTasks; ++t) {
        a.boxes[t] = nullptr, a.scores[t] = nullptr, a.labels[t] = nullptr, a.source[t] = nullptr, a.in_sizes[t] = nullptr;
        a.thr[t] = 0.0f, a.has_thr[t] = 0;
    }
    a.out_boxes = boxes, a.out_scores = scores, a.out_labels = labels, a.out_source = source, a.sizes = out_sizes;
    a.B = B, a.N = N, a.M = M, a.pre = pre_max_size;
    a.D = (int)D, a.T = T;
    return ACCV_OK;
}

}  // namespace

extern "C" {

int accv_rotated_iou_bev(const float* a, const long long* a_sizes, const float* b, const long long* b_sizes, long long B, long long Na,
                         long long Nb, float* out, void* stream)
{
    const char* who = "rotated_iou_bev";
    IouArgs g;
    int empty;
    if (int rc = iou_check_args(who, a, a_sizes, b, b_sizes, B, Na, Nb, out, g, &empty)) return rc;
    if (empty) return ACCV_OK;
    hipLaunchKernelGGL(rotated_iou_bev_kernel, dim3((unsigned)(g.B * g.tiles_a * g.tiles_b)), dim3(kThreads), 0,
                       static_cast<hipStream_t>(stream), g);
    return accv::check_launch(who);
}

int accv_rotated_iou_bev_host(const float* a, const long long* a_sizes, const float* b, const long long* b_sizes, long long B,
                              long long Na, long long Nb, float* out)
{
    const char* who = "rotated_iou_bev (host)";
    IouArgs g;
    int empty;
    if (int rc = iou_check_args(who, a, a_sizes, b, b_sizes, B, Na, Nb, out, g, &empty)) return rc;
    if (empty) return ACCV_OK;
    iou_host_run(g);
    return ACCV_OK;
}

int accv_rotated_nms_bev(const accv_rotated_nms_params* params, long long B, long long N, long long D, long long pre_max_size,
                         long long M, float* boxes, float* scores, long long* labels, int* source, long long* out_sizes, void* stream)
{
    const char* who = "rotated_nms_bev";
    Args a;
    int empty;
    if (int rc = nms_check_args(who, params, B, N, D, pre_max_size, M, boxes, scores, labels, source, out_sizes, a, &empty)) return rc;
    if (empty) return ACCV_OK;
    hipLaunchKernelGGL(rotated_nms_bev_kernel, dim3((unsigned)a.B, (unsigned)a.T), dim3(kThreads), 0, static_cast<hipStream_t>(stream), a);
    return accv::check_launch(who);
}

int accv_rotated_nms_bev_host(const accv_rotated_nms_params* params, long long B, long long N, long long D, long long pre_max_size,
                              long long M, float* boxes, float* scores, long long* labels, int* source, long long* out_sizes)
{
    const char* who = "rotated_nms_bev (host)";
    Args a;
    int empty;
    if (int rc = nms_check_args(who, params, B, N, D, pre_max_size, M, boxes, scores, labels, source, out_sizes, a, &empty)) return rc;
    if (empty) return ACCV_OK;
    nms_host_run(a);
    return ACCV_OK;
}

}  // extern "C"
