// Visible-box selection for a ragged batch of 2D boxes: the occlusion test and the minimum-size test of the reference's
// VisibleBboxSelector step (dali_pipeline_framework operators_impl/numba_operators/numba_operators.py:240-403) without the
// H x W canvas.  Per-box arithmetic: visible_boxes_arith.h.
//
// After clipping all edges are integers, so the top-most box is constant on every cell between consecutive x edges and
// consecutive y edges, and a box is visible iff it is the top-most box of some cell.  It is enough to look at the pixel
// (ex, ey) for every x edge ex and y edge ey: of the visible pixels of a box take the one with the smallest x and then the
// smallest y; its left neighbour is outside the box (x = x0 of the box) or covered by a box above that ends there (x = x1 of
// that box), and the same holds for its upper neighbour.  So no edge sort is needed, only the distinct edge values.
//
// One workgroup of kThreads = kMaxBoxes lanes per frame, a lane per box slot:
//   1. the painted rectangle and depth key of the slot go to LDS in slot order;
//   2. one loop over the frame's boxes counts the box's layer (the number of boxes above it: layer 0 is on top) and marks
//      each of the lane's four edges that an earlier slot already holds;
//   3. rectangles are scattered to LDS in layer order, and the distinct edges of each axis are compacted (__ballot +
//      popcount, the waves' totals behind one barrier);
//   4. for every distinct edge e a lane per layer tests x0 <= e < x1: the __ballot is one 64-box word of the bit set of the
//      boxes that span e, bit k = layer k;
//   5. lanes take x edges, waves take y edges: the top-most box at (ex, ey) is the LOWEST set bit of M = X & Y, which is
//      M & -M: one and, one subtract-with-borrow and one and-or per 32 bits.  Each lane collects the layers it saw on top
//      in registers and ORs them into LDS once at the end;
//   6. flag AND size test go out, padding slots as 0: every output byte is written, nothing is cleared beforehand.
// Steps 4 and 5 are nearly all of the time (measured with both compiled out: 6 of 49 us remain at 64 frames of up to 128
// boxes), so their inner loops hold no LDS round trip per edge, no store and no branch.
// No atomics on global memory, no global scratch, no host synchronisation; the OR of step 5 does not depend on its order.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "accv_common.h"
#include "accv_numeric.h"
#include "visible_boxes_arith.h"

namespace {

using namespace accv_vb;
using accv::clamp_count;
using accv::load_index;

constexpr int kWave = 64;
constexpr int kThreads = kMaxBoxes;          // a lane per box slot
constexpr int kWaves = kThreads / kWave;
constexpr int kEdges = 2 * kMaxBoxes;        // per axis
constexpr unsigned kKnownFlags = ACCV_VB_COUNTS_I64 | ACCV_VB_HW_I64;

static_assert(kMaxBoxes == ACCV_VB_MAX_BOXES, "visible_boxes_arith.h and accv_hip.h disagree");
static_assert(kWaves == kWords, "a wave per 64-box word");

struct Args {
    const float* boxes;        // [B, G, 4]
    const float* depths;       // [B, G] or null
    const void* counts;        // [B]
    const void* image_hw;      // [B, 2] or null
    unsigned char* out;        // [B, G]
    long long B, G, H, W;
    float min_size;
    int counts64, hw64, occlusion, size, shrink;
};

// (H, W) of frame b as floats, exact: both are clamped to [0, 2^24]
__host__ __device__ inline void frame_extent(const Args& a, long long b, float& Hf, float& Wf)
{
    long long H = a.H, W = a.W;
    if (a.image_hw) H = load_index(a.image_hw, 2 * b, a.hw64), W = load_index(a.image_hw, 2 * b + 1, a.hw64);
    Hf = (float)clamp_extent(H), Wf = (float)clamp_extent(W);
}

// ------------------------------------------------------------------------------------------------------------- device
// One 64-box word of the bit sets of all `count` edges of an axis: this wave's lanes hold the boxes of 64 consecutive
// layers, [lo, hi) is the lane's interval on the axis; the word of edge q goes to words[q * stride].  The edges are taken 64 at a time, a lane per edge; each is broadcast
// from its lane's register, the __ballot of lo <= e < hi is the word, and the lane of the edge keeps it: one LDS read and
// one LDS write per lane and 64 edges.  A lane beyond `count` holds -1, which no interval spans.
__device__ __forceinline__ void span_words(const int* edges, int count, int lo, int hi, int lane, unsigned long long* words,
                                           int stride)
{
    for (int base = 0; base < count; base += kWave) {
        const int mine = base + lane < count ? edges[base + lane] : -1;
        const int live = count - base < kWave ? count - base : kWave;
        unsigned long long word = 0;
        for (int k0 = 0; k0 < live; k0 += 8) {   // eight at a time: a lane beyond `live` holds -1 and gets the word 0
#pragma unroll
            for (int k = k0; k < k0 + 8; ++k) {
                const int e = __builtin_amdgcn_readlane(mine, k);
                const unsigned long long m = __ballot(lo <= e && e < hi);
                if (lane == k) word = m;
            }
        }
        words[(base + lane) * stride] = word;   // base + lane < kEdges
    }
}

// Lanes take x edges, waves take y edges; the top-most box at (ex, ey) is the lowest set bit of M = X & Y over NW words:
// M & -M, the negation carried through the words by the subtraction's borrow.  Each lane collects the layers it saw on top
// in registers; the lanes' sets meet in LDS at the end.  bx is [word][edge] (consecutive lanes read consecutive edges), by
// is [edge][word] (every lane of the wave reads the same 8 * NW bytes).
template <int NW>
__device__ __forceinline__ void mark_tops(const unsigned long long (*bx)[kEdges], const unsigned long long (*by)[kWords], int cx,
                                          int cy, int lane, int wave, unsigned long long* vis)
{
    unsigned long long seen[NW];
#pragma unroll
    for (int w = 0; w < NW; ++w) seen[w] = 0;
    for (int ex = lane; ex < cx; ex += kWave) {
        unsigned long long X[NW], any = 0;
#pragma unroll
        for (int w = 0; w < NW; ++w) any |= X[w] = bx[w][ex];
        if (!any) continue;   // the right edge of a box with nothing beside it
#pragma unroll 4
        for (int ey = wave; ey < cy; ey += kWaves) {
            unsigned long long borrow = 0;
#pragma unroll
            for (int w = 0; w < NW; ++w) {
                const unsigned long long m = X[w] & by[ey][w];
                const unsigned long long neg = __builtin_subcll(0ull, m, borrow, &borrow);
                seen[w] |= m & neg;
            }
        }
    }
#pragma unroll
    for (int w = 0; w < NW; ++w)
        if (seen[w]) atomicOr(&vis[w], seen[w]);   // LDS; the result does not depend on the order
}

__global__ __launch_bounds__(kThreads) void visible_boxes_kernel(const Args a)
{
    __shared__ Rect s_slot[kMaxBoxes];                          // slot order
    __shared__ Rect s_layer[kMaxBoxes];                         // layer order
    __shared__ uint32_t s_key[kMaxBoxes];
    __shared__ int s_edge[2][kEdges];                           // the distinct edges of x and of y
    __shared__ unsigned long long s_bx[kWords][kEdges];         // per x edge: the layers that span it, word-major
    __shared__ unsigned long long s_by[kEdges][kWords];         // per y edge, edge-major
    __shared__ int s_cnt[4][kWaves];
    __shared__ unsigned long long s_vis[kWords];                // bit k: the box of layer k is on top somewhere

    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const long long b = blockIdx.x;
    const int n = (int)clamp_count(a.counts, b, a.G, a.counts64);
    float Hf, Wf;
    frame_extent(a, b, Hf, Wf);
    const bool real = tid < n;
    float box[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (real) {
        const float* p = a.boxes + (b * a.G + tid) * 4;
        box[0] = p[0], box[1] = p[1], box[2] = p[2], box[3] = p[3];
    }
    const bool big = !a.size || (real && size_ok(box, Wf, Hf, a.min_size));
    if (!a.occlusion) {   // the same in every lane
        if (tid < a.G) a.out[b * a.G + tid] = real && big;
        return;
    }
    const Rect r = real ? painted_rect(box, Wf, Hf, a.shrink) : no_rect();
    const uint32_t key = real ? depth_key(a.depths[b * a.G + tid]) : 0u;
    s_slot[tid] = r;
    s_key[tid] = key;
    if (tid < kWords) s_vis[tid] = 0;
    __syncthreads();

    int layer = 0;
    bool dup_x0 = false, dup_x1 = false, dup_y0 = false, dup_y1 = false;
#pragma unroll 4
    for (int j = 0; j < n; ++j) {
        const Rect q = s_slot[j];
        layer += above(s_key[j], j, key, tid) ? 1 : 0;
        const bool earlier = j < tid;
        dup_x0 |= earlier && (q.x0 == r.x0 || q.x1 == r.x0);
        dup_x1 |= earlier && (q.x0 == r.x1 || q.x1 == r.x1);
        dup_y0 |= earlier && (q.y0 == r.y0 || q.y1 == r.y0);
        dup_y1 |= earlier && (q.y0 == r.y1 || q.y1 == r.y1);
    }
    s_layer[real ? layer : tid] = r;   // the layers are a permutation of 0 .. n - 1; slots from n on hold no_rect()

    const bool on = paints(r);
    const bool act[4] = {on && !dup_x0, on && !dup_x1, on && !dup_y0, on && !dup_y1};
    unsigned long long bal[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        bal[k] = __ballot(act[k]);
        if (lane == 0) s_cnt[k][wave] = __popcll(bal[k]);
    }
    __syncthreads();
    int pos[4], tot[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        pos[k] = __popcll(bal[k] & ((1ull << lane) - 1ull));
        tot[k] = 0;
#pragma unroll
        for (int v = 0; v < kWaves; ++v) {
            const int c = s_cnt[k][v];
            tot[k] += c;
            if (v < wave) pos[k] += c;
        }
    }
    const int cx = tot[0] + tot[1], cy = tot[2] + tot[3];   // <= 2 n
    if (act[0]) s_edge[0][pos[0]] = r.x0;
    if (act[1]) s_edge[0][tot[0] + pos[1]] = r.x1;
    if (act[2]) s_edge[1][pos[2]] = r.y0;
    if (act[3]) s_edge[1][tot[2] + pos[3]] = r.y1;
    __syncthreads();

    const int words = (n + kWave - 1) / kWave;
    if (wave < words) {   // the other waves hold no box
        const Rect me = s_layer[tid];
        span_words(s_edge[0], cx, me.x0, me.x1, lane, s_bx[wave], 1);
        span_words(s_edge[1], cy, me.y0, me.y1, lane, &s_by[0][wave], kWords);
    }
    __syncthreads();

    switch (words) {   // the same in every lane
    case 1: mark_tops<1>(s_bx, s_by, cx, cy, lane, wave, s_vis); break;
    case 2: mark_tops<2>(s_bx, s_by, cx, cy, lane, wave, s_vis); break;
    case 3: mark_tops<3>(s_bx, s_by, cx, cy, lane, wave, s_vis); break;
    case 4: mark_tops<4>(s_bx, s_by, cx, cy, lane, wave, s_vis); break;
    default: break;    // no box
    }
    __syncthreads();
    if (tid < a.G) a.out[b * a.G + tid] = real && big && ((s_vis[layer >> 6] >> (layer & 63)) & 1ull) != 0;
}

// --------------------------------------------------------------------------------------------------------------- host
// the same algorithm, one frame after the other
void host_run(const Args& a)
{
    static thread_local Rect slot[kMaxBoxes];
    static thread_local uint32_t key[kMaxBoxes];
    static thread_local int layer[kMaxBoxes], edge[2][kEdges];
    static thread_local unsigned long long bits[2][kWords][kEdges];
    static thread_local unsigned char vis[kMaxBoxes], big[kMaxBoxes];
    for (long long b = 0; b < a.B; ++b) {
        const int n = (int)clamp_count(a.counts, b, a.G, a.counts64);
        float Hf, Wf;
        frame_extent(a, b, Hf, Wf);
        unsigned char* out = a.out + b * a.G;
        for (int i = 0; i < n; ++i) {
            const float* box = a.boxes + (b * a.G + i) * 4;
            big[i] = !a.size || size_ok(box, Wf, Hf, a.min_size);
            vis[i] = 0;
            if (!a.occlusion) continue;
            slot[i] = painted_rect(box, Wf, Hf, a.shrink);
            key[i] = depth_key(a.depths[b * a.G + i]);
        }
        for (long long i = n; i < a.G; ++i) out[i] = 0;
        if (!a.occlusion) {
            for (int i = 0; i < n; ++i) out[i] = big[i];
            continue;
        }
        const int words = (n + 63) / 64;
        int cnt[2] = {0, 0};
        for (int i = 0; i < n; ++i) {
            int rk = 0;
            for (int j = 0; j < n; ++j) rk += above(key[j], j, key[i], i) ? 1 : 0;
            layer[i] = rk;
            if (!paints(slot[i])) continue;
            const int mine[2][2] = {{slot[i].x0, slot[i].x1}, {slot[i].y0, slot[i].y1}};
            for (int axis = 0; axis < 2; ++axis) {
                for (int s = 0; s < 2; ++s) {
                    bool dup = false;
                    for (int q = 0; q < cnt[axis] && !dup; ++q) dup = edge[axis][q] == mine[axis][s];
                    if (!dup) edge[axis][cnt[axis]++] = mine[axis][s];
                }
            }
        }
        for (int axis = 0; axis < 2; ++axis) {
            for (int q = 0; q < cnt[axis]; ++q) {
                const int e = edge[axis][q];
                for (int w = 0; w < words; ++w) bits[axis][w][q] = 0;
                for (int i = 0; i < n; ++i) {
                    const int lo = axis ? slot[i].y0 : slot[i].x0, hi = axis ? slot[i].y1 : slot[i].x1;
                    if (lo <= e && e < hi) bits[axis][layer[i] >> 6][q] |= 1ull << (layer[i] & 63);
                }
            }
        }
        for (int ex = 0; ex < cnt[0]; ++ex) {
            unsigned long long X[kWords] = {0, 0, 0, 0};
            for (int w = 0; w < words; ++w) X[w] = bits[0][w][ex];
            for (int ey = 0; ey < cnt[1]; ++ey) {
                const int top = top_layer(X, &bits[1][0][ey], kEdges, words);
                if (top >= 0) vis[top] = 1;
            }
        }
        for (int i = 0; i < n; ++i) out[i] = big[i] && vis[layer[i]];
    }
}

// ------------------------------------------------------------------------------------------------------------- checks
// ACCV_OK with *empty = 1 when there is nothing to write; every check runs before anything else reads the arguments
int check_args(const char* who, const float* boxes, const float* depths, const void* counts, const void* image_hw,
               unsigned flags, long long B, long long G, const accv_visible_boxes_params* p, unsigned char* out, Args& a,
               int* empty)
{
    *empty = 0;
    if (!p) return accv::fail(ACCV_EINVAL, "%s: null params", who);
    if (B < 0 || G < 0) return accv::fail(ACCV_EINVAL, "%s: negative size", who);
    if (flags & ~kKnownFlags) return accv::fail(ACCV_EINVAL, "%s: unknown flags 0x%x", who, flags);
    if (!p->check_occlusion && !p->check_size)
        return accv::fail(ACCV_EINVAL, "%s: at least one of the occlusion and the minimum-size check must be requested", who);
    if (G > kMaxBoxes) return accv::fail(ACCV_EINVAL, "%s: %lld box slots per frame, at most %d supported", who, G, kMaxBoxes);
    if (B == 0 || G == 0) {
        *empty = 1;
        return ACCV_OK;
    }
    if (!boxes || !counts || !out) return accv::fail(ACCV_EINVAL, "%s: null boxes / counts / output pointer", who);
    if (p->check_occlusion && !depths) return accv::fail(ACCV_EINVAL, "%s: the occlusion check needs depths", who);
    if ((reinterpret_cast<uintptr_t>(boxes) | reinterpret_cast<uintptr_t>(depths)) & 3u)
        return accv::fail(ACCV_EINVAL, "%s: boxes / depths are not aligned to their element size", who);
    if ((reinterpret_cast<uintptr_t>(counts) & ((flags & ACCV_VB_COUNTS_I64) ? 7u : 3u)) ||
        (reinterpret_cast<uintptr_t>(image_hw) & ((flags & ACCV_VB_HW_I64) ? 7u : 3u)))
        return accv::fail(ACCV_EINVAL, "%s: counts / image_hw are not aligned to their element size", who);
    if (B > accv::kGridLimit) return accv::fail(ACCV_EINVAL, "%s: %lld workgroups exceed the grid limit", who, B);
    a.boxes = boxes, a.depths = depths, a.counts = counts, a.image_hw = image_hw, a.out = out;
    a.B = B, a.G = G, a.H = p->image_h, a.W = p->image_w;
    a.min_size = (float)p->minimum_size;
    a.counts64 = (flags & ACCV_VB_COUNTS_I64) ? 1 : 0, a.hw64 = (flags & ACCV_VB_HW_I64) ? 1 : 0;
    a.occlusion = p->check_occlusion ? 1 : 0, a.size = p->check_size ? 1 : 0, a.shrink = p->shrink_to_int ? 1 : 0;
    return ACCV_OK;
}

}  // namespace

extern "C" {

int accv_visible_boxes(const float* boxes, const float* depths, const void* counts, const void* image_hw, unsigned flags,
                       long long B, long long G, const accv_visible_boxes_params* params, unsigned char* out, void* stream)
{
    const char* who = "visible_bbox_mask";
    Args a;
    int empty;
    if (int rc = check_args(who, boxes, depths, counts, image_hw, flags, B, G, params, out, a, &empty)) return rc;
    if (empty) return ACCV_OK;
    hipLaunchKernelGGL(visible_boxes_kernel, dim3((unsigned)a.B), dim3(kThreads), 0, static_cast<hipStream_t>(stream), a);
    return accv::check_launch(who);
}

int accv_visible_boxes_host(const float* boxes, const float* depths, const void* counts, const void* image_hw, unsigned flags,
                            long long B, long long G, const accv_visible_boxes_params* params, unsigned char* out)
{
    const char* who = "visible_bbox_mask (host)";
    Args a;
    int empty;
    if (int rc = check_args(who, boxes, depths, counts, image_hw, flags, B, G, params, out, a, &empty)) return rc;
    if (empty) return ACCV_OK;
    host_run(a);
    return ACCV_OK;
}

}  // extern "C"
