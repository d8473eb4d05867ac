// Target side of a centre-point head (mmdet3d's CenterHead.get_targets_single) for a ragged batch of 3D boxes and every
// task of the head in one launch: per (task, frame) the kept objects' integer centres, Gaussian radii, in-task labels,
// regression targets, in-plane indices and source slots, compacted in ascending slot order; the rest of each [M] row is
// filled (0, source -1) and the kept count written, so every output element is written exactly once.  Per-object
// arithmetic: center_targets_arith.h.
//
// One workgroup of kThreads lanes per (frame, task).  The frame's slots are walked in chunks of kThreads, a lane per slot:
// the lane looks its label up in the class table (by value in the kernel arguments), and a candidate evaluates the validity
// test.  Two order-preserving ranks follow, each a __ballot + popcount inside the wave, the waves' totals meeting in LDS
// behind one barrier per rank (the barrier of the other rank separates a row's reads from its next writes), with a running
// base across chunks:
//   1. the rank among the candidates, which applies the max_objs cut (mmdet3d cuts before it tests validity);
//   2. the rank among the kept candidates = the output slot.
// Kept lanes then compute radius and row and store them.  No atomics: the order is defined by the slot number, so the
// result is bitwise reproducible.  Launch and latency bound work (a few hundred objects per frame): no MFMA.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>

#include "accv_common.h"
#include "accv_numeric.h"
#include "center_targets_arith.h"

#pragma clang fp contract(off)

namespace {

using namespace accv_ct;
using accv::clamp_count;
using accv::load_index;

constexpr int kWave = 64;
constexpr int kThreads = 256;               // and slots per chunk
constexpr int kWaves = kThreads / kWave;
constexpr unsigned kKnownFlags = ACCV_CT_LABELS_I64 | ACCV_CT_COUNTS_I64;

static_assert(kMaxTasks == ACCV_CT_MAX_TASKS && kMaxClasses == ACCV_CT_MAX_CLASSES && kNoTask == ACCV_CT_NO_TASK,
              "center_targets_arith.h and accv_hip.h disagree");

struct Args {
    const float* boxes;         // [B, N, D]
    const void* labels;         // [B, N]
    const void* counts;         // [B]
    int* centers;               // [T, B, M, 2]
    int* radii;                 // [T, B, M]
    int* out_labels;            // [T, B, M]
    float* targets;             // [T, B, M, D + 1]
    long long* indices;         // [T, B, M]
    int* source;                // [T, B, M]
    long long* sizes;           // [T, B]
    Consts k;
    long long B, N, M, W;
    int D, T, max_objs, labels64, counts64;
    unsigned char cls_task[kMaxClasses], cls_pos[kMaxClasses];
};

// the position of label `lab` inside task t, or -1 when it is not one of the task's classes
__host__ __device__ inline int position_in_task(const Args& a, long long lab, int t)
{
    if (lab < 0 || lab >= kMaxClasses) return -1;
    return a.cls_task[lab] == t ? (int)a.cls_pos[lab] : -1;
}

// everything a kept object writes: slot `slot` of row (t, b), from input slot n
__host__ __device__ inline void write_object(const Args& a, long long row0, long long slot, long long n, const float* box, int pos,
                                             float cx, float cy, float w, float l)
{
    const int ix = (int)cx, iy = (int)cy;   // cx in (-1, W), cy in (-1, H)
    const long long o = row0 + slot;
    reinterpret_cast<int2*>(a.centers)[o] = make_int2(ix, iy);
    a.radii[o] = radius_of(a.k, w, l);
    a.out_labels[o] = pos;
    a.indices[o] = (long long)iy * a.W + ix;
    a.source[o] = (int)n;
    float row[10];
    target_row(a.k, box, a.D, cx, cy, ix, iy, row);
    float2* out = reinterpret_cast<float2*>(a.targets + o * (a.D + 1));   // D + 1 is even and the base 8-byte aligned
#pragma unroll
    for (int c = 0; c < 4; ++c) out[c] = make_float2(row[2 * c], row[2 * c + 1]);
    if (a.D == 9) out[4] = make_float2(row[8], row[9]);
}

// the filler of padding slot j of row (t, b), all outputs but the targets
__host__ __device__ inline void write_padding(const Args& a, long long row0, long long j)
{
    const long long o = row0 + j;
    reinterpret_cast<int2*>(a.centers)[o] = make_int2(0, 0);
    a.radii[o] = 0;
    a.out_labels[o] = 0;
    a.indices[o] = 0;
    a.source[o] = -1;
}

// ------------------------------------------------------------------------------------------------------------- device
// accv::block_rank (accv_numeric.h) is called on two alternating rows (candidates, kept), so neither is written while a
// slower wave still reads it
__global__ __launch_bounds__(kThreads) void center_point_targets_kernel(const Args a)
{
    __shared__ int s_cand[kWaves], s_keep[kWaves];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const long long b = blockIdx.x / a.T;
    const int t = (int)(blockIdx.x - b * a.T);
    const long long size = clamp_count(a.counts, b, a.N, a.counts64);
    const long long row0 = ((long long)t * a.B + b) * a.M;
    int cands = 0, kept = 0;   // running bases, the same in every lane
    for (long long base = 0; base < size && cands < a.max_objs; base += kThreads) {
        const long long n = base + tid;
        const float* box = a.boxes + (b * a.N + n) * a.D;
        int pos = -1;
        if (n < size) pos = position_in_task(a, load_index(a.labels, b * a.N + n, a.labels64), t);
        float cx = 0.0f, cy = 0.0f, w = 0.0f, l = 0.0f;
        const bool valid = pos >= 0 && scale_and_test(a.k, box[0], box[1], box[3], box[4], cx, cy, w, l);
        int before, total;
        accv::block_rank<kWaves>(pos >= 0, s_cand, lane, wave, before, total);
        const bool keep = valid && cands + before < a.max_objs;
        cands += total;
        accv::block_rank<kWaves>(keep, s_keep, lane, wave, before, total);
        const long long slot = kept + before;
        kept += total;
        if (keep && slot < a.M) write_object(a, row0, slot, n, box, pos, cx, cy, w, l);
    }
    for (long long j = kept + tid; j < a.M; j += kThreads) write_padding(a, row0, j);
    const long long C = a.D + 1;
    float* trow = a.targets + row0 * C;
    for (long long e = kept * C + tid; e < a.M * C; e += kThreads) trow[e] = 0.0f;
    if (tid == 0) a.sizes[(long long)t * a.B + b] = kept;
}

// --------------------------------------------------------------------------------------------------------------- host
void host_run(const Args& a)
{
    const long long C = a.D + 1;
    for (int t = 0; t < a.T; ++t) {
        for (long long b = 0; b < a.B; ++b) {
            const long long size = clamp_count(a.counts, b, a.N, a.counts64);
            const long long row0 = ((long long)t * a.B + b) * a.M;
            long long cands = 0, kept = 0;
            for (long long n = 0; n < size && cands < a.max_objs; ++n) {
                const int pos = position_in_task(a, load_index(a.labels, b * a.N + n, a.labels64), t);
                if (pos < 0) continue;
                ++cands;
                const float* box = a.boxes + (b * a.N + n) * a.D;
                float cx, cy, w, l;
                if (!scale_and_test(a.k, box[0], box[1], box[3], box[4], cx, cy, w, l) || kept >= a.M) continue;
                write_object(a, row0, kept++, n, box, pos, cx, cy, w, l);
            }
            for (long long j = kept; j < a.M; ++j) write_padding(a, row0, j);
            for (long long e = kept * C; e < a.M * C; ++e) a.targets[row0 * C + e] = 0.0f;
            a.sizes[(long long)t * a.B + b] = kept;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------- checks
// ACCV_OK with *empty = 1 when there is nothing to write; every check runs before anything else reads the arguments
int check_args(const char* who, const float* boxes, const void* labels, const void* counts, unsigned flags, long long B,
               long long N, long long D, long long W, long long H, long long M, const accv_center_point_targets_params* p,
               int* centers, int* radii, int* out_labels, float* targets, long long* indices, int* source, long long* out_sizes,
               Args& a, int* empty)
{
    *empty = 0;
    if (!p) return accv::fail(ACCV_EINVAL, "%s: null params", who);
    if (B < 0 || N < 0 || M < 0 || W < 0 || H < 0 || D < 0 || p->max_objs < 0) return accv::fail(ACCV_EINVAL, "%s: negative size", who);
    if (p->num_tasks < 1 || p->num_tasks > kMaxTasks)
        return accv::fail(ACCV_EINVAL, "%s: 1..%d tasks supported, got %d", who, kMaxTasks, p->num_tasks);
    if (D != 7 && D != 9) return accv::fail(ACCV_EINVAL, "%s: boxes need D = 7 or 9 (got %lld)", who, D);
    if (flags & ~kKnownFlags) return accv::fail(ACCV_EINVAL, "%s: unknown flags 0x%x", who, flags);
    for (int c = 0; c < kMaxClasses; ++c)
        if (p->class_task[c] != kNoTask && p->class_task[c] >= p->num_tasks)
            return accv::fail(ACCV_EINVAL, "%s: class %d is in task %d of %d", who, c, (int)p->class_task[c], p->num_tasks);
    if (!(p->voxel_size[0] > 0.0) || !(p->voxel_size[1] > 0.0) || !(p->out_size_factor > 0.0))
        return accv::fail(ACCV_EINVAL, "%s: voxel_size and out_size_factor must be positive", who);
    if (W < 1 || H < 1 || W > INT_MAX / H) return accv::fail(ACCV_EINVAL, "%s: a grid of %lld x %lld cells is empty or exceeds 2^31 - 1", who, W, H);
    if (N > INT_MAX) return accv::fail(ACCV_EINVAL, "%s: N is limited to 2^31 - 1", who);
    if (M < (N < p->max_objs ? N : (long long)p->max_objs))
        return accv::fail(ACCV_EINVAL, "%s: M = %lld is below min(max_objs, N) = %lld", who, M, N < p->max_objs ? N : (long long)p->max_objs);
    if (B == 0 || M == 0) {
        *empty = 1;
        return ACCV_OK;
    }
    if (!counts || !out_sizes) return accv::fail(ACCV_EINVAL, "%s: null counts / sizes pointer", who);
    if (N > 0 && (!boxes || !labels)) return accv::fail(ACCV_EINVAL, "%s: null boxes / labels pointer", who);
    if (!centers || !radii || !out_labels || !targets || !indices || !source) return accv::fail(ACCV_EINVAL, "%s: null output pointer", who);
    if ((reinterpret_cast<uintptr_t>(boxes) | reinterpret_cast<uintptr_t>(radii) | reinterpret_cast<uintptr_t>(out_labels) |
         reinterpret_cast<uintptr_t>(source)) & 3u)
        return accv::fail(ACCV_EINVAL, "%s: a 4-byte tensor is not aligned to its element size", who);
    if ((reinterpret_cast<uintptr_t>(centers) | reinterpret_cast<uintptr_t>(targets) | reinterpret_cast<uintptr_t>(indices) |
         reinterpret_cast<uintptr_t>(out_sizes)) & 7u)
        return accv::fail(ACCV_EINVAL, "%s: centers, targets, indices and sizes must be 8-byte aligned", who);
    if ((reinterpret_cast<uintptr_t>(labels) & ((flags & ACCV_CT_LABELS_I64) ? 7u : 3u)) ||
        (reinterpret_cast<uintptr_t>(counts) & ((flags & ACCV_CT_COUNTS_I64) ? 7u : 3u)))
        return accv::fail(ACCV_EINVAL, "%s: labels / counts are not aligned to their element size", who);
    if (B > accv::kGridLimit / p->num_tasks) return accv::fail(ACCV_EINVAL, "%s: %lld x %d workgroups exceed the grid limit", who, B, p->num_tasks);
    if (M > LLONG_MAX / 16 / (D + 1) / p->num_tasks / B || N > LLONG_MAX / 16 / D / B) return accv::fail(ACCV_EINVAL, "%s: sizes overflow", who);
    a.boxes = boxes, a.labels = labels, a.counts = counts;
    a.centers = centers, a.radii = radii, a.out_labels = out_labels, a.targets = targets, a.indices = indices, a.source = source;
    a.sizes = out_sizes;
    const float m = (float)p->gaussian_overlap;
    a.k.pc0 = (float)p->pc_range[0], a.k.pc1 = (float)p->pc_range[1];
    a.k.vs0 = (float)p->voxel_size[0], a.k.vs1 = (float)p->voxel_size[1];
    a.k.f = (float)p->out_size_factor;
    a.k.m = m, a.k.omm = 1.0f - m, a.k.opm = 1.0f + m;
    a.k.Wf = (float)W, a.k.Hf = (float)H;
    a.k.min_radius = p->min_radius, a.k.norm_bbox = p->norm_bbox ? 1 : 0;
    if (!(a.k.vs0 > 0.0f) || !(a.k.vs1 > 0.0f) || !(a.k.f > 0.0f))
        return accv::fail(ACCV_EINVAL, "%s: voxel_size and out_size_factor must be positive in float32", who);
    a.B = B, a.N = N, a.M = M, a.W = W;
    a.D = (int)D, a.T = p->num_tasks, a.max_objs = p->max_objs;
    a.labels64 = (flags & ACCV_CT_LABELS_I64) ? 1 : 0, a.counts64 = (flags & ACCV_CT_COUNTS_I64) ? 1 : 0;
    for (int c = 0; c < kMaxClasses; ++c) a.cls_task[c] = p->class_task[c], a.cls_pos[c] = p->class_pos[c];
    return ACCV_OK;
}

}  // namespace

extern "C" {

int accv_center_point_targets(const float* boxes, const void* labels, const void* counts, unsigned flags, long long B,
                              long long N, long long D, long long W, long long H, long long M,
                              const accv_center_point_targets_params* params, int* centers, int* radii, int* out_labels,
                              float* targets, long long* indices, int* source, long long* out_sizes, void* stream)
{
    const char* who = "center_point_targets";
    Args a;
    int empty;
    if (int rc = check_args(who, boxes, labels, counts, flags, B, N, D, W, H, M, params, centers, radii, out_labels, targets,
                            indices, source, out_sizes, a, &empty))
        return rc;
    if (empty) return ACCV_OK;
    hipLaunchKernelGGL(center_point_targets_kernel, dim3((unsigned)(a.B * a.T)), dim3(kThreads), 0, static_cast<hipStream_t>(stream), a);
    return accv::check_launch(who);
}

int accv_center_point_targets_host(const float* boxes, const void* labels, const void* counts, unsigned flags, long long B,
                                   long long N, long long D, long long W, long long H, long long M,
                                   const accv_center_point_targets_params* params, int* centers, int* radii,
                                   int* out_labels, float* targets, long long* indices, int* source, long long* out_sizes)
{
    const char* who = "center_point_targets (host)";
    Args a;
    int empty;
    if (int rc = check_args(who, boxes, labels, counts, flags, B, N, D, W, H, M, params, centers, radii, out_labels, targets,
                            indices, source, out_sizes, a, &empty))
        return rc;
    if (empty) return ACCV_OK;
    host_run(a);
    return ACCV_OK;
}

}  // extern "C"
