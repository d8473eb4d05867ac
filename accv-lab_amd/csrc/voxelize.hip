// Hard voxelization of a ragged batch of lidar frames: mmcv's Voxelization (hard_voxelize_forward, one call per frame in
// Base3DDetector.voxelize) for the whole batch, with the voxel order, the voxels that survive max_voxels and the points that
// survive max_points of the SEQUENTIAL loop (hard_voxelize_forward_cpu) whatever the order in which the lanes run.  Per-point
// arithmetic and the definition: voxelize_arith.h.
//
// No atomic counter decides an order.  Per frame, in a caller-provided workspace: an open-addressing table of S slots
// (key word, first-index word, number word), the slot of every point [P] and an index list [V, T] per voxel.
//   clear    hipMemsetAsync of the key and first-index words to 0xFF bytes (empty, UINT_MAX).
//   insert   a lane per point: the key of the point; linear probing from first_slot(key) with a compare-and-swap on the key
//            word until the slot holds the key (at most S steps; S > P, so an empty slot exists); atomicMin of the point's
//            index into the slot's first-index word; the slot is kept.  Slot positions vary from run to run, the set of
//            (key, first index) does not.
//   count    a point opens its voxel iff first[slot[p]] == p.  A workgroup of kScanThreads lanes per chunk of kScanThreads *
//            kUnroll consecutive points (kUnroll a lane) counts the chunk's opening points.  Further workgroups of the same
//            launch fill the index lists with INT_MAX.
//   number   the same workgroups again: the sum of the counts of the chunks before its own, then the exclusive prefix sum of
//            the flag inside the chunk (wave scan by shuffles, the wave totals through LDS, one barrier) is the voxel's
//            number.  Numbers >= V are refused.  The lane of the opening point writes the number (or kNone) into the slot
//            and coors[number]; the last chunk's workgroup writes voxel_counts.  A workgroup reads the counts of all chunks
//            before it: a lane reads one count per 4 M points of the frame before its chunk.
//   rank     a lane per point of an accepted voxel walks the voxel's list: old = atomicMin(&list[j], v), v = max(old, v),
//            ++j, until v == INT_MAX or j == T.  Position j sees every value that left position j - 1 and keeps the
//            smallest, so the list ends sorted and holds the T smallest indices whatever the interleaving.  point_voxel is
//            written here.
//   gather   a lane per 16 bytes (D a multiple of 4, points and voxels 16-byte aligned) or per element of voxels: the
//            point list[j] names, x, y, z through the frame's row again, +0 where the list holds INT_MAX; the lane of a
//            row's first element writes num_points where the row is the voxel's last, and coors = -1 for a voxel without
//            points (a voxel that exists holds its opening point, so these are the voxels from voxel_counts on).
// Every output element is written exactly once, no output is read, no input is written.  Every loop is bounded (S probe
// steps, T rank steps); nothing waits for another lane or workgroup.  All atomics are 32-bit vector atomics on global
// memory.  Latency-bound in insert, count and number (dependent loads), store-bound in gather; LDS only for the wave totals of
// count and number; no MFMA.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "accv_common.h"
#include "accv_numeric.h"
#include "voxelize_arith.h"

#pragma clang fp contract(off)

namespace {

using namespace accv_vx;
using accv::clamp_count;

constexpr int kThreads = 256;        // insert, rank, gather: a lane per point / per store
constexpr int kScanThreads = 1024;   // count, number: a workgroup per chunk of kScanThreads * kUnroll points
constexpr int kUnroll = 4;           // count, number: consecutive points per lane
constexpr int kFillBlocks = 64;      // count: at most this many list-filling workgroups per frame
constexpr long long kMaxFrames = 65535;
constexpr long long kMaxSlots = 1ll << 31;

struct Args {
    const float* points;   // [B, P, D]
    const void* sizes;     // [B]
    const float* aug;      // [B, 7] or null
    float* voxels;         // [B, V, T, D]
    int* coors;            // [B, V, 3]
    int* num_points;       // [B, V]
    int* counts;           // [B]
    int* point_voxel;      // [B, P] or null
    int* keys;             // workspace [B, S]: the key of a slot, kNone while empty
    unsigned* first;       // workspace [B, S]: the lowest point index of the slot's key
    int* number;           // workspace [B, S]: the voxel number of the slot's key, kNone when refused
    int* slot;             // workspace [B, P]: the slot of a point, kNone without a key
    int* lists;            // workspace [B, V, T]: the point indices of a voxel, ascending, INT_MAX behind them
    int* chunk_counts;     // workspace [B, chunks]: the points of a chunk that open a voxel
    long long B, P, S, chunks;
    int D, V, T, sizes64;
    int fill_blocks;
    Grid g;
};

__host__ __device__ inline const float* frame_row(const Args& a, long long b) { return a.aug ? a.aug + b * 7 : nullptr; }

// ------------------------------------------------------------------------------------------------------------- device
__global__ __launch_bounds__(kThreads) void voxelize_insert_kernel(const Args a)
{
    const long long b = blockIdx.y, p = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (p >= a.P) return;
    int s = kNone;
    if (p < clamp_count(a.sizes, b, a.P, a.sizes64)) {
        const float* q = a.points + (b * a.P + p) * a.D;
        float x = q[0], y = q[1], z = q[2];
        place_point(frame_row(a, b), x, y, z);
        const int key = point_key(a.g, x, y, z);
        if (key != kNone) {
            int* keys = a.keys + b * a.S;
            const uint32_t mask = (uint32_t)(a.S - 1);
            uint32_t h = first_slot(key, mask);
            for (long long step = 0; step < a.S; ++step) {
                const int old = atomicCAS(&keys[h], kNone, key);
                if (old == kNone || old == key) {
                    s = (int)h;
                    break;
                }
                h = (h + 1) & mask;
            }
            if (s != kNone) atomicMin(&a.first[b * a.S + s], (unsigned)p);
        }
    }
    a.slot[b * a.P + p] = s;
}

// the kUnroll consecutive points from p0 on of a frame with n points: the slot of each and whether it opens its voxel (it is
// the lowest index of its key); returns how many do
__device__ __forceinline__ int load_opens(const Args& a, long long b, long long n, long long p0, int* s, bool* opens)
{
    const int* slot = a.slot + b * a.P;
    const unsigned* first = a.first + b * a.S;
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) s[u] = p0 + u < n ? slot[p0 + u] : kNone;
    int mine = 0;
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
        opens[u] = s[u] != kNone && first[s[u]] == (unsigned)(p0 + u);
        mine += opens[u] ? 1 : 0;
    }
    return mine;
}

// the sum of v over the lanes of a wave up to and including this one
__device__ __forceinline__ int wave_inclusive(int v, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl_up(v, d, 64);
        if (lane >= d) v += up;
    }
    return v;
}

// workgroup x < chunks of frame y: how many points of its chunk of kScanThreads * kUnroll points open a voxel.  The further
// workgroups fill the index lists of all frames, as one range dealt over the filling workgroups of all frames.
__global__ __launch_bounds__(kScanThreads) void voxelize_count_kernel(const Args a)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (blockIdx.x >= a.chunks) {
        const long long total = a.B * a.V * a.T, groups = total >> 2;
        const long long lanes = (long long)a.fill_blocks * a.B * kScanThreads;
        const long long me = ((long long)blockIdx.y * a.fill_blocks + (blockIdx.x - a.chunks)) * kScanThreads + tid;
        int4* l4 = reinterpret_cast<int4*>(a.lists);
        for (long long i = me; i < groups; i += lanes) l4[i] = int4{INT_MAX, INT_MAX, INT_MAX, INT_MAX};
        for (long long i = (groups << 2) + me; i < total; i += lanes) a.lists[i] = INT_MAX;
        return;
    }
    __shared__ int s_wave[kScanThreads / 64];
    const long long b = blockIdx.y;
    int s[kUnroll];
    bool opens[kUnroll];
    const int mine = load_opens(a, b, clamp_count(a.sizes, b, a.P, a.sizes64), ((long long)blockIdx.x * kScanThreads + tid) * kUnroll, s, opens);
    const int incl = wave_inclusive(mine, lane);
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    if (tid == 0) {
        int total = 0;
#pragma unroll
        for (int w = 0; w < kScanThreads / 64; ++w) total += s_wave[w];
        a.chunk_counts[b * a.chunks + blockIdx.x] = total;
    }
}

// workgroup x of frame y numbers the voxels its chunk opens: the counts of the chunks before it, then the exclusive prefix sum
// of the flags inside the chunk (wave scan by shuffles, the wave totals through LDS)
__global__ __launch_bounds__(kScanThreads) void voxelize_number_kernel(const Args a)
{
    __shared__ int s_wave[kScanThreads / 64];
    __shared__ long long s_before[kScanThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long b = blockIdx.y, chunk = blockIdx.x;
    const int* keys = a.keys + b * a.S;
    int* number = a.number + b * a.S;
    long long part = 0;
    for (long long i = tid; i < chunk; i += kScanThreads) part += a.chunk_counts[b * a.chunks + i];
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) part += __shfl_xor(part, d, 64);
    int s[kUnroll];
    bool opens[kUnroll];
    const int mine = load_opens(a, b, clamp_count(a.sizes, b, a.P, a.sizes64), (chunk * kScanThreads + tid) * kUnroll, s, opens);
    const int incl = wave_inclusive(mine, lane);
    if (lane == 63) s_wave[wave] = incl, s_before[wave] = part;
    __syncthreads();
    long long base = 0;
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kScanThreads / 64; ++w) {
        const int t = s_wave[w];
        base += s_before[w];
        before += w < wave ? t : 0;
        total += t;
    }
    long long v = base + before + (incl - mine);
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
        if (!opens[u]) continue;
        const bool accepted = v < a.V;
        number[s[u]] = accepted ? (int)v : kNone;
        if (accepted) key_coors(a.g, keys[s[u]], a.coors + (b * a.V + v) * 3);
        ++v;
    }
    if (chunk == a.chunks - 1 && tid == 0) a.counts[b] = (int)(base + total < a.V ? base + total : a.V);
}

__global__ __launch_bounds__(kThreads) void voxelize_rank_kernel(const Args a)
{
    const long long b = blockIdx.y, p = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (p >= a.P) return;
    const int s = a.slot[b * a.P + p];
    const int v = s == kNone ? kNone : a.number[b * a.S + s];
    if (a.point_voxel) a.point_voxel[b * a.P + p] = v;
    if (v == kNone) return;
    int* list = a.lists + (b * a.V + v) * a.T;
    int val = (int)p;
    for (int j = 0; j < a.T && val != INT_MAX; ++j) {
        const int old = atomicMin(&list[j], val);
        val = old > val ? old : val;
    }
}

// what the lane of a row's first element writes besides: num_points where the row is the last of its voxel, and the coors
// of a voxel without points
__device__ __forceinline__ void finish_row(const Args& a, long long b, long long r, const int* list, int idx)
{
    const long long v = r / a.T;
    const int j = (int)(r - v * a.T);
    if (idx == INT_MAX) {
        if (j == 0) {
            a.num_points[b * a.V + v] = 0;
            int* c = a.coors + (b * a.V + v) * 3;
            c[0] = kNone, c[1] = kNone, c[2] = kNone;
        }
    } else if (j == a.T - 1 || list[r + 1] == INT_MAX) {
        a.num_points[b * a.V + v] = j + 1;
    }
}

template <bool kVec>
__global__ __launch_bounds__(kThreads) void voxelize_gather_kernel(const Args a)
{
    const long long b = blockIdx.y, e = (long long)blockIdx.x * kThreads + threadIdx.x;
    const int per_row = kVec ? a.D >> 2 : a.D;
    const long long rows = (long long)a.V * a.T;
    if (e >= rows * per_row) return;
    const long long r = e / per_row;
    const int part = (int)(e - r * per_row);
    const int* list = a.lists + b * rows;
    const int idx = list[r];
    if (part == 0) finish_row(a, b, r, list, idx);
    const float* q = idx == INT_MAX ? nullptr : a.points + (b * a.P + idx) * a.D;
    const float* row = frame_row(a, b);
    if (kVec) {
        float4 out{0.0f, 0.0f, 0.0f, 0.0f};
        if (idx != INT_MAX) {
            out = reinterpret_cast<const float4*>(q)[part];
            if (part == 0) place_point(row, out.x, out.y, out.z);
        }
        reinterpret_cast<float4*>(a.voxels)[(b * rows + r) * per_row + part] = out;
    } else {
        float out = 0.0f;
        if (idx != INT_MAX) {
            if (part < 3 && row) {
                float xyz[3] = {q[0], q[1], q[2]};
                place_point(row, xyz[0], xyz[1], xyz[2]);
                out = part == 0 ? xyz[0] : (part == 1 ? xyz[1] : xyz[2]);
            } else {
                out = q[part];
            }
        }
        a.voxels[(b * rows + r) * per_row + part] = out;
    }
}

// --------------------------------------------------------------------------------------------------------------- host
// the sequential loop itself, with a table of its own: the same probe sequence, one point at a time
void host_run(const Args& a)
{
    const long long rows = (long long)a.V * a.T;
    std::memset(a.voxels, 0, (size_t)(a.B * rows * a.D) * sizeof(float));
    for (long long i = 0; i < a.B * a.V * 3; ++i) a.coors[i] = kNone;
    for (long long i = 0; i < a.B * a.V; ++i) a.num_points[i] = 0;
    std::vector<int> keys((size_t)a.S), number((size_t)a.S);
    const uint32_t mask = (uint32_t)(a.S - 1);
    for (long long b = 0; b < a.B; ++b) {
        const long long n = clamp_count(a.sizes, b, a.P, a.sizes64);
        for (long long i = 0; i < a.S; ++i) keys[(size_t)i] = kNone;
        int count = 0;
        for (long long p = 0; p < a.P; ++p) {
            if (a.point_voxel) a.point_voxel[b * a.P + p] = kNone;
            if (p >= n) continue;
            const float* q = a.points + (b * a.P + p) * a.D;
            float x = q[0], y = q[1], z = q[2];
            place_point(frame_row(a, b), x, y, z);
            const int key = point_key(a.g, x, y, z);
            if (key == kNone) continue;
            uint32_t h = first_slot(key, mask);
            for (long long step = 0; step < a.S && keys[h] != kNone && keys[h] != key; ++step) h = (h + 1) & mask;
            if (keys[h] == kNone) {
                if (count == a.V) continue;     // mmcv's `continue`: the point is skipped, the loop goes on
                keys[h] = key, number[h] = count;
                key_coors(a.g, key, a.coors + (b * a.V + count) * 3);
                ++count;
            }
            const int v = number[h];
            if (a.point_voxel) a.point_voxel[b * a.P + p] = v;
            int& held = a.num_points[b * a.V + v];
            if (held < a.T) {
                float* out = a.voxels + ((b * a.V + v) * a.T + held) * a.D;
                std::memcpy(out, q, (size_t)a.D * sizeof(float));      // bit for bit, NaN payloads included
                if (a.aug) out[0] = x, out[1] = y, out[2] = z;
                ++held;
            }
        }
        a.counts[b] = count;
    }
}

// ------------------------------------------------------------------------------------------------------------- checks
inline uintptr_t addr(const void* p) { return reinterpret_cast<uintptr_t>(p); }

// the table of a frame: the power of two that is at least 2 * P (so at most half of it is ever used), capped at 2^31, which
// is still more than P
inline long long default_slots(long long P)
{
    long long s = 1;
    while (s < 2 * P && s < kMaxSlots) s <<= 1;
    return s;
}

// the chunks of kScanThreads * kUnroll points of a frame; one where there are no points, for voxel_counts
inline long long chunks_of(long long P)
{
    const long long per = (long long)kScanThreads * kUnroll;
    return P > 0 ? (P + per - 1) / per : 1;
}

inline bool legal_slots(long long slots, long long P) { return slots > P && slots <= kMaxSlots && (slots & (slots - 1)) == 0; }

struct Layout {
    size_t table, number, slot, lists, chunks, total;   // table: keys then first, cleared as one range
};

// false for sizes the call refuses
inline bool workspace_layout(long long B, long long P, long long V, long long T, long long table_slots, Layout& l)
{
    if (B < 0 || B > kMaxFrames || P < 0 || P >= INT_MAX || V < 1 || V > kMaxV || T < 1 || T > kMaxT) return false;
    const long long S = table_slots ? table_slots : default_slots(P);
    if (!legal_slots(S, P)) return false;
    l.table = accv::align_up((size_t)(B * S) * 8, 16);
    l.number = accv::align_up((size_t)(B * S) * 4, 16);
    l.slot = accv::align_up((size_t)(B * P) * 4, 16);
    l.lists = accv::align_up((size_t)(B * V * T) * 4, 16);
    l.chunks = accv::align_up((size_t)(B * chunks_of(P)) * 4, 16);
    l.total = l.table + l.number + l.slot + l.lists + l.chunks;
    return true;
}

// ACCV_OK with *empty = 1 when there is nothing to write; every check runs before anything else reads the data
int check_args(const char* who, const accv_voxelize_params* p, long long B, long long P, long long D, float* voxels, int* coors,
               int* num_points, int* voxel_counts, int* point_voxel, Args& a, int* empty)
{
    *empty = 0;
    if (!p) return accv::fail(ACCV_EINVAL, "%s: null params", who);
    if (B < 0 || P < 0) return accv::fail(ACCV_EINVAL, "%s: negative size (B %lld, P %lld)", who, B, P);
    if (B > kMaxFrames) return accv::fail(ACCV_EINVAL, "%s: %lld frames exceed the grid limit of %lld", who, B, kMaxFrames);
    if (P >= INT_MAX) return accv::fail(ACCV_EINVAL, "%s: P = %lld point slots, fewer than 2^31 - 1 supported", who, P);
    if (D < kMinD || D > kMaxD) return accv::fail(ACCV_EINVAL, "%s: points need %d <= D <= %d channels (x, y, z first), got %lld", who, kMinD, kMaxD, D);
    if (p->max_points < 1 || p->max_points > kMaxT)
        return accv::fail(ACCV_EINVAL, "%s: max_points must be in 1..%d, got %d", who, kMaxT, p->max_points);
    if (p->max_voxels < 1 || p->max_voxels > kMaxV)
        return accv::fail(ACCV_EINVAL, "%s: max_voxels must be in 1..%lld, got %d", who, kMaxV, p->max_voxels);
    double cells = 1.0;
    for (int k = 0; k < 3; ++k) {
        const float v = (float)p->voxel_size[k], lo = (float)p->range_min[k], hi = (float)p->range_max[k];
        if (!(v > 0.0f && std::isfinite(v)))
            return accv::fail(ACCV_EINVAL, "%s: voxel_size[%d] must be positive and finite in float32, got %g", who, k, p->voxel_size[k]);
        if (!(std::isfinite(lo) && std::isfinite(hi) && hi > lo))
            return accv::fail(ACCV_EINVAL, "%s: point_cloud_range needs finite lo < hi in float32 along axis %d, got (%g, %g)", who, k,
                              p->range_min[k], p->range_max[k]);
        const float g = grid_extent(lo, hi, v);
        if (!(g >= 1.0f && g < 2147483648.0f))
            return accv::fail(ACCV_EINVAL, "%s: the grid has %g cells along axis %d, 1 .. 2^31 - 1 supported", who, (double)g, k);
        a.g.lo[k] = lo, a.g.v[k] = v, a.g.gf[k] = g, a.g.g[k] = (int)g;
        cells *= (double)g;
    }
    if (cells >= 2147483648.0) return accv::fail(ACCV_EINVAL, "%s: the grid has %.0f cells, fewer than 2^31 supported", who, cells);
    const long long S = p->table_slots ? p->table_slots : default_slots(P);
    if (!legal_slots(S, P))
        return accv::fail(ACCV_EINVAL, "%s: table_slots must be 0 or a power of two above P = %lld and at most 2^31, got %lld", who, P,
                          p->table_slots);
    if (B == 0) {
        *empty = 1;
        return ACCV_OK;
    }
    if (!voxels || !coors || !num_points || !voxel_counts) return accv::fail(ACCV_EINVAL, "%s: null output pointer", who);
    if (!p->sample_sizes || (P > 0 && !p->points)) return accv::fail(ACCV_EINVAL, "%s: null input pointer", who);
    if ((addr(voxels) | addr(coors) | addr(num_points) | addr(voxel_counts) | addr(point_voxel) | addr(p->points) | addr(p->augmentation)) & 3u)
        return accv::fail(ACCV_EINVAL, "%s: a 4-byte tensor is not aligned to its element size", who);
    if (addr(p->sample_sizes) & (p->sizes_i64 ? 7u : 3u)) return accv::fail(ACCV_EINVAL, "%s: sample_sizes is not aligned to its element size", who);
    a.points = p->points, a.sizes = p->sample_sizes, a.aug = p->augmentation;
    a.voxels = voxels, a.coors = coors, a.num_points = num_points, a.counts = voxel_counts, a.point_voxel = point_voxel;
    a.keys = nullptr, a.first = nullptr, a.number = nullptr, a.slot = nullptr, a.lists = nullptr, a.chunk_counts = nullptr;
    a.B = B, a.P = P, a.S = S, a.chunks = chunks_of(P);
    a.D = (int)D, a.V = p->max_voxels, a.T = p->max_points, a.sizes64 = p->sizes_i64 ? 1 : 0;
    const long long list_words = (long long)a.V * a.T;
    const long long want = (list_words + (long long)kScanThreads * 64 - 1) / ((long long)kScanThreads * 64);
    a.fill_blocks = (int)(want < 1 ? 1 : (want > kFillBlocks ? kFillBlocks : want));
    return ACCV_OK;
}

}  // namespace

extern "C" {

size_t accv_voxelize_workspace_bytes(long long B, long long P, long long V, long long T, long long table_slots)
{
    Layout l;
    return workspace_layout(B, P, V, T, table_slots, l) ? (l.total ? l.total : 16) : 0;
}

int accv_voxelize(const accv_voxelize_params* params, long long B, long long P, long long D, float* voxels, int* coors, int* num_points,
                  int* voxel_counts, int* point_voxel, void* workspace, size_t workspace_bytes, void* stream_)
{
    const char* who = "voxelize_points";
    Args a;
    int empty;
    if (int rc = check_args(who, params, B, P, D, voxels, coors, num_points, voxel_counts, point_voxel, a, &empty)) return rc;
    if (empty) return ACCV_OK;
    Layout l;
    if (!workspace_layout(B, P, a.V, a.T, params->table_slots, l)) return accv::fail(ACCV_EINVAL, "%s: sizes overflow", who);
    if (int rc = accv::check_workspace(who, workspace, workspace_bytes, l.total)) return rc;
    char* ws = static_cast<char*>(workspace);
    a.keys = reinterpret_cast<int*>(ws);
    a.first = reinterpret_cast<unsigned*>(ws) + B * a.S;
    a.number = reinterpret_cast<int*>(ws + l.table);
    a.slot = reinterpret_cast<int*>(ws + l.table + l.number);
    a.lists = reinterpret_cast<int*>(ws + l.table + l.number + l.slot);
    a.chunk_counts = reinterpret_cast<int*>(ws + l.table + l.number + l.slot + l.lists);

    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const hipError_t e = hipMemsetAsync(ws, 0xFF, (size_t)(B * a.S) * 8, stream);
    if (e != hipSuccess) return accv::fail(ACCV_ELAUNCH, "%s: %s", who, hipGetErrorString(e));
    const dim3 per_point((unsigned)((P + kThreads - 1) / kThreads), (unsigned)B);
    if (P > 0) hipLaunchKernelGGL(voxelize_insert_kernel, per_point, dim3(kThreads), 0, stream, a);
    hipLaunchKernelGGL(voxelize_count_kernel, dim3((unsigned)(a.chunks + a.fill_blocks), (unsigned)B), dim3(kScanThreads), 0, stream, a);
    hipLaunchKernelGGL(voxelize_number_kernel, dim3((unsigned)a.chunks, (unsigned)B), dim3(kScanThreads), 0, stream, a);
    if (P > 0) hipLaunchKernelGGL(voxelize_rank_kernel, per_point, dim3(kThreads), 0, stream, a);
    const bool vec = a.D % 4 == 0 && ((addr(a.points) | addr(a.voxels)) & 15u) == 0;
    const long long units = (long long)a.V * a.T * (vec ? a.D / 4 : a.D);
    const dim3 per_store((unsigned)((units + kThreads - 1) / kThreads), (unsigned)B);
    if (vec)
        hipLaunchKernelGGL(voxelize_gather_kernel<true>, per_store, dim3(kThreads), 0, stream, a);
    else
        hipLaunchKernelGGL(voxelize_gather_kernel<false>, per_store, dim3(kThreads), 0, stream, a);
    return accv::check_launch(who);
}

int accv_voxelize_cpu(const accv_voxelize_params* params, long long B, long long P, long long D, float* voxels, int* coors,
                      int* num_points, int* voxel_counts, int* point_voxel)
{
    const char* who = "voxelize_points (host)";
    Args a;
    int empty;
    if (int rc = check_args(who, params, B, P, D, voxels, coors, num_points, voxel_counts, point_voxel, a, &empty)) return rc;
    if (empty) return ACCV_OK;
    host_run(a);
    return ACCV_OK;
}

}  // extern "C"
