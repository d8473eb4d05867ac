// The visibility walk of one frame, shared by visible_boxes.hip and camera_boxes.hip: from the painted rectangle and depth
// key of every box slot to the bit "this box is the top-most box somewhere".  Per-box arithmetic: visible_boxes_arith.h.
//
// After clipping all edges are integers, so the top-most box is constant on every cell between consecutive x edges and
// consecutive y edges, and a box is visible iff it is the top-most box of some cell.  It is enough to look at the pixel
// (ex, ey) for every x edge ex and y edge ey: of the visible pixels of a box take the one with the smallest x and then the
// smallest y; its left neighbour is outside the box (x = x0 of the box) or covered by a box above that ends there (x = x1 of
// that box), and the same holds for its upper neighbour.  So no edge sort is needed, only the distinct edge values.
//
// Device (block_visible): one workgroup of kThreads = kMaxBoxes lanes per frame, a lane per box slot:
//   1. the painted rectangle and depth key of the slot go to LDS in slot order;
//   2. one loop over the frame's boxes counts the box's layer (the number of boxes above it: layer 0 is on top) and marks
//      each of the lane's four edges that an earlier slot already holds;
//   3. rectangles are scattered to LDS in layer order, and the distinct edges of each axis are compacted (__ballot +
//      popcount, the waves' totals behind one barrier);
//   4. for every distinct edge e a lane per layer tests x0 <= e < x1: the __ballot is one 64-box word of the bit set of the
//      boxes that span e, bit k = layer k;
//   5. lanes take x edges, waves take y edges: the top-most box at (ex, ey) is the LOWEST set bit of M = X & Y, which is
//      M & -M: one and, one subtract-with-borrow and one and-or per 32 bits.  Each lane collects the layers it saw on top
//      in registers and ORs them into LDS once at the end.
// Steps 4 and 5 are nearly all of the time (measured with both compiled out: 6 of 49 us remain at 64 frames of up to 128
// boxes), so their inner loops hold no LDS round trip per edge, no store and no branch.
// No atomics on global memory, no global scratch; the OR of step 5 does not depend on its order.  The LDS (about 45 KB)
// belongs to the function: each kernel that calls it gets one copy, and calls it at most once.
//
// Host (host_frame_visible): the same algorithm for one frame, serially.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "visible_boxes_arith.h"

namespace accv_vb {

constexpr int kWave = 64;
constexpr int kThreads = kMaxBoxes;          // a lane per box slot
constexpr int kWaves = kThreads / kWave;
constexpr int kEdges = 2 * kMaxBoxes;        // per axis

static_assert(kWaves == kWords, "a wave per 64-box word");

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

// Steps 1 to 5 for the frame of this workgroup: lane `tid` brings the painted rectangle `r` and depth key `key` of its slot
// (no_rect() and 0 when the slot is none of the frame's `n` boxes, `real` false) and gets back whether its box is on top
// somewhere.  Every lane of the workgroup calls it (it holds barriers); the last one is behind the last LDS access.
__device__ __forceinline__ bool block_visible(int n, bool real, const Rect& r, uint32_t key, int tid, int lane, int wave)
{
    __shared__ Rect s_slot[kMaxBoxes];                          // slot order
    __shared__ Rect s_layer[kMaxBoxes];                         // layer order
    __shared__ uint32_t s_key[kMaxBoxes];
    __shared__ int s_edge[2][kEdges];                           // the distinct edges of x and of y
    __shared__ unsigned long long s_bx[kWords][kEdges];         // per x edge: the layers that span it, word-major
    __shared__ unsigned long long s_by[kEdges][kWords];         // per y edge, edge-major
    __shared__ int s_cnt[4][kWaves];
    __shared__ unsigned long long s_vis[kWords];                // bit k: the box of layer k is on top somewhere

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
    return ((s_vis[layer >> 6] >> (layer & 63)) & 1ull) != 0;
}

// --------------------------------------------------------------------------------------------------------------- host
// out[i] (i < n) = the AND of the requested checks for the n boxes at `boxes` ([n, 4]) with depths `depths` ([n], read
// with `occlusion` only) on an image of Hf x Wf
inline void host_frame_visible(const float* boxes, const float* depths, int n, float Hf, float Wf, int occlusion, int size,
                               float min_size, int shrink, unsigned char* out)
{
    static thread_local Rect slot[kMaxBoxes];
    static thread_local uint32_t key[kMaxBoxes];
    static thread_local int layer[kMaxBoxes], edge[2][kEdges];
    static thread_local unsigned long long bits[2][kWords][kEdges];
    static thread_local unsigned char vis[kMaxBoxes], big[kMaxBoxes];
    for (int i = 0; i < n; ++i) {
        const float* box = boxes + i * 4;
        big[i] = !size || size_ok(box, Wf, Hf, min_size);
        vis[i] = 0;
        if (!occlusion) continue;
        slot[i] = painted_rect(box, Wf, Hf, shrink);
        key[i] = depth_key(depths[i]);
    }
    if (!occlusion) {
        for (int i = 0; i < n; ++i) out[i] = big[i];
        return;
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

}  // namespace accv_vb
