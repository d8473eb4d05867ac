// Shared pieces of the heat-map rasteriser (draw_heatmap.hip): the kernel parameter blocks (SplatParams, MultiParams), the
// names of the SRC / SM template values, the hit record, the NaN-skipping max, tile location and the per-plane object range,
// the cull (Cand / cull_load / cull_test / cull_round), make_hit, the prologue of the multi-scale kernels (scale_of_group,
// preload_params) and the DPP moves.  Included once, from draw_heatmap.hip, first of the splat_*.h headers; needs accv_common.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "accv_common.h"

namespace {

constexpr int kWavesPerGroup = 1;  // 1 wave per workgroup measured 6.5 % faster than 4 (profiles/r01_h1_variants_wpg.log)
constexpr int kBoxTileR = 8;  // rows per half-wave of a box-map tile (multi-scale launches): 128 x 16 pixel tiles.  4 = 128 x 8 tiles
                              // (54 VGPRs, 8 waves per SIMD, twice the waves): box maps of config 3 17.1 -> 18.4 us, measured
constexpr int kCand = 64;  // candidates per cull round = one per lane
constexpr float kLog2e = 1.4426950408889634f;

// what the candidates of a tile kernel are (template parameter SRC; an int, so that the mangled kernel names stay what the
// profiles of this repository call them)
constexpr int kSrcObjects = 0;     // integer centres + radii (flat and batched API)
constexpr int kSrcFloatBoxes = 1;  // float centres / boxes in source pixels, converted per scale inside the cull (multi-scale front end)
constexpr int kSrcPoints = 2;      // float sample points of one common radius, culled in two levels (lane rasters)
// how a tile is stored (template parameter SM, and the host's store mode)
constexpr int kStorePlain = 0;
constexpr int kStoreWriteThrough = 4;  // write-through non-temporal (sc1 nt) buffer stores
constexpr int kStoreAdaptive = 5;      // in-place tile kernel: plain or write-through per plane, by the density of its objects

struct SplatParams {
    float* hm;
    const int32_t* centers;
    const int32_t* radii;
    const int32_t* labels;     // class-wise batched: labels; otherwise any readable int32 array shaped like radii
    const void* counts;        // batched: i32[B] or i64[B]
    const int32_t* plane_off;  // flat: [P+1] offsets into centers/radii (which are then the plane-sorted copies)
    int H, W;
    int n_max;      // batched: padded objects per sample
    int n_classes;  // class-wise: C, else 0
    int tiles_x, tiles_y;
    long long n_tiles;
    float factor, k;
    int counts_i64;
    int grid3d;           // tile index comes from a 3-D grid instead of a linear block index
    float dense_area;     // SM == 5: a plane whose objects cover at least this many pixels (sum (2r+1)^2) stores write-through
    // multi-scale front end (SRC == 1): objects are float centres / boxes in source pixels, converted per scale
    const float* centers_f;  // [B, n_max, 2] (x, y)
    const float* boxes_f;    // [B, n_max, 4] (x0, y0, x1, y1)
    float stride;
    // point splats (SRC == 2): centers_f = sampled points [B, n_max, 2]; boxes_f = bounding boxes of every 64 consecutive
    // points [B, n_groups, 4] (xmin, ymin, xmax, ymax; source pixels); every point gets the same radius
    int radius, n_groups;
#ifdef ACCV_SPLAT_STAMPS
    // diagnostic build only (scripts/splat_phase_stamps.py): one 64-byte record of phase time stamps per tile wave
    unsigned long long* stamps;
    long long stamp_records;
#endif
};

constexpr int kMaxScales = 4;
struct MultiParams {
    SplatParams scale[kMaxScales];
    long long tile_begin[kMaxScales + 1];  // linear workgroup index where each scale's tiles start
    int n_scales;
};

// one culled hit, read back as a single ds_read_b128 broadcast.  The clipped box is stored relative to the tile and
// clamped to it (each bound fits a byte: tiles are at most 128 x 32), so a wave needs 1 KB for the list instead of 2
// and 5 KB of LDS in total -> 32 single-wave workgroups (8 waves per SIMD) fit a CU's 160 KB
struct __attribute__((aligned(16))) Hit {
    int x, y;
    float c2;      // log2(e) / var
    unsigned box;  // xlo | xhi << 8 | ylo << 16 | yhi << 24 : columns [xlo,xhi), rows [ylo,yhi) of the tile
};

template <int PX>
struct Vec;
typedef float vfloat4 __attribute__((ext_vector_type(4)));
template <>
struct Vec<4> {
    using type = vfloat4;
};
template <>
struct Vec<1> {
    using type = float;
};

__device__ __forceinline__ float raw_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

// max that treats a quiet NaN as "no data" in ONE instruction.  fmaxf() has the same meaning, but hipcc puts a
// canonicalising v_max_f32 x, x, x in front of every call whose operand it cannot prove to be a quiet value (the
// loop-carried accumulator), i.e. 3 VALU ops per pixel instead of 2.  All masks in this file are the quiet NaN
// 0x7fc00000 and products of a quiet NaN stay quiet, so the raw instruction is exact here.
__device__ __forceinline__ float max_skip_nan(float acc, float v)
{
    float r;
    asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(acc), "v"(v));
    return r;
}

// ---------------------------------------------------------------- pieces shared by the tile kernels
struct TileCtx {
    int tx0, ty0, tx1, ty1;  // pixel bounds of the tile, clipped to the frame
    long long plane;
    const int2* centers2;    // objects of this plane: [0, n)
    const int32_t* radii;
    const int32_t* labels;
    const float2* centers_f;  // SRC == 1: float objects of this plane
    const float4* boxes_f;
    float4 box0;             // SRC == 2 (SCALAR_COUNT): group box min(lane, n_groups - 1) of the plane, requested ahead of the count
    float stride;
    int radius;              // SRC == 2: the radius of every point
    int n, cls;              // cls < 0: no class filter
};

template <bool SCALAR_COUNT = false>
__device__ __forceinline__ void plane_objects(const SplatParams& p, TileCtx& t);

// tile coordinates from the launch geometry + the object range that feeds this plane; false = wave has no tile
template <int TW, int TH, int WPG, bool SCALAR_COUNT = false>
__device__ __forceinline__ bool locate_tile(const SplatParams& p, int wave, TileCtx& t, long long linear_group)
{
    int tx, ty;
    if (p.grid3d) {
        // 3-D grid (x = group of WPG column tiles, y = row tile, z = plane): no divisions in the prologue
        tx = blockIdx.x * WPG + wave;
        ty = blockIdx.y;
        t.plane = blockIdx.z;
        if (tx >= p.tiles_x) return false;
    } else {  // linear block index (more than 65535 planes or tile rows)
        const long long tile = linear_group * WPG + wave;
        if (tile >= p.n_tiles) return false;  // whole wave exits; waves never synchronise with each other
        if (p.n_tiles <= 0x7fffffffll) {      // 32-bit divisions (a 64-bit one costs ~60 instructions, and there are three)
            const unsigned t32 = (unsigned)tile, t2 = t32 / (unsigned)p.tiles_x;
            tx = (int)(t32 - t2 * (unsigned)p.tiles_x);
            const unsigned pl = t2 / (unsigned)p.tiles_y;
            ty = (int)(t2 - pl * (unsigned)p.tiles_y);
            t.plane = pl;
        } else {
            tx = (int)(tile % p.tiles_x);
            const long long t2 = tile / p.tiles_x;
            ty = (int)(t2 % p.tiles_y);
            t.plane = t2 / p.tiles_y;
        }
    }
    t.tx0 = tx * TW;
    t.ty0 = ty * TH;
    t.tx1 = min(t.tx0 + TW, p.W);
    t.ty1 = min(t.ty0 + TH, p.H);
    plane_objects<SCALAR_COUNT>(p, t);
    return true;
}

// which objects feed plane t.plane: objects [obj_base, obj_base + n) of centers/radii(/labels)
// SCALAR_COUNT: the plane's count is read through the scalar cache (constant address space: the array is not written by this
// launch, and the scalar cache is invalidated between launches).  hipcc chooses that by itself while the parameters are read
// straight from the kernel arguments, but falls back to a vector-memory load — ten times the latency, in front of everything a
// short-lived tile wave does — once they are a preloaded copy (preload_params)
template <bool SCALAR_COUNT>
__device__ __forceinline__ void plane_objects(const SplatParams& p, TileCtx& t)
{
    long long obj_base;
    t.cls = -1;
    if (p.plane_off) {  // flat API: the binning pre-pass left plane-sorted copies of the objects
        const int o0 = p.plane_off[t.plane];
        obj_base = o0;
        t.n = p.plane_off[t.plane + 1] - o0;
    } else {
        long long s = t.plane;
        if (p.n_classes > 0) {
            s = t.plane / p.n_classes;
            t.cls = (int)(t.plane - s * p.n_classes);
        }
        long long cnt;
        if constexpr (SCALAR_COUNT) {
            // the first round of group boxes does not depend on the count: requested first, so that both are in flight together
            if (p.n_groups > 0)
                t.box0 = reinterpret_cast<const float4*>(p.boxes_f)[t.plane * p.n_groups + min((int)(threadIdx.x & 63), p.n_groups - 1)];
            using ConstI32 = const __attribute__((address_space(4))) int;
            using ConstI64 = const __attribute__((address_space(4))) long long;
            const uintptr_t base = reinterpret_cast<uintptr_t>(p.counts);
            cnt = p.counts_i64 ? reinterpret_cast<ConstI64*>(base)[s] : (long long)reinterpret_cast<ConstI32*>(base)[s];
        } else {
            cnt = p.counts_i64 ? ((const long long*)p.counts)[s] : (long long)((const int*)p.counts)[s];
        }
        t.n = (int)max(0ll, min(cnt, (long long)p.n_max));
        obj_base = s * p.n_max;
    }
    t.centers2 = reinterpret_cast<const int2*>(p.centers) + obj_base;
    t.radii = p.radii + obj_base;
    t.labels = p.labels + obj_base;
    t.centers_f = reinterpret_cast<const float2*>(p.centers_f) + obj_base;
    t.boxes_f = reinterpret_cast<const float4*>(p.boxes_f) + (p.n_groups > 0 ? (t.plane * p.n_groups) : obj_base);
    t.stride = p.stride;
    t.radius = p.radius;
}

// One candidate per lane and round, fetched with branch-free loads (index clamped to the last object, result masked).
// The cull is VALU-bound for long object lists (lane rasters walk 10^3 candidates per tile), so the test every lane
// runs is a cheap CONSERVATIVE one in 32-bit: coordinates clamped to +-2^29 and the radius to 2^30 cannot overflow and
// never miss a real hit while H, W <= 2^29 (host-checked).  Returns the ballot of hitting lanes.
struct Cand {
    int x, y, r, label;
};
template <int SRC = kSrcObjects>
__device__ __forceinline__ Cand cull_load(const TileCtx& t, int base, int lane)
{
    const int cc = min(base + lane, t.n - 1);  // n >= 1 inside the candidate loop
    if constexpr (SRC == kSrcFloatBoxes) {
        // float centre + box in source pixels -> integer target at this scale, exactly targets_from_boxes_kernel below
        // (packages/draw_heatmap/tests/_test_helpers.py:20-28): r = max(1, ceil(min edge distance / stride)),
        // c = int(c / stride); IEEE division
        const float2 c = t.centers_f[cc];
        const float4 b = t.boxes_f[cc];
        const float m = fminf(fminf(c.x - b.x, c.y - b.y), fminf(b.z - c.x, b.w - c.y));
        // (a stride that is a power of two: the product with its reciprocal is the same correctly rounded value as the IEEE
        // division — both round x * 2^-k once — for a third of the instructions of this cull)
        const bool pow2 = (__float_as_uint(t.stride) & 0x007fffffu) == 0u && t.stride > 1.0e-30f && t.stride < 1.0e30f;   // uniform
        if (pow2) {
            const float inv = 1.0f / t.stride;
            int r = (int)ceilf(m * inv);
            if (r < 1) r = 1;
            return Cand{(int)(c.x * inv), (int)(c.y * inv), r, 0};
        }
        int r = (int)ceilf(__fdiv_rn(m, t.stride));
        if (r < 1) r = 1;
        return Cand{(int)__fdiv_rn(c.x, t.stride), (int)__fdiv_rn(c.y, t.stride), r, 0};
    } else if constexpr (SRC == kSrcPoints) {
        // sampled polyline point -> target of the common radius, exactly targets_from_points_kernel below
        const float2 c = t.centers_f[cc];
        const bool bad = (c.x != c.x) || (c.y != c.y);
        if (bad) return Cand{0, 0, -1, 0};
        return Cand{(int)__fdiv_rn(c.x, t.stride), (int)__fdiv_rn(c.y, t.stride), t.radius, 0};
    } else {
        const int2 cxy = t.centers2[cc];
        return Cand{cxy.x, cxy.y, t.radii[cc], t.labels[cc]};
    }
}
__device__ __forceinline__ unsigned long long cull_test(const TileCtx& t, int base, int lane, const Cand& c)
{
    constexpr int kClampXY = 1 << 29, kClampR = 1 << 30;
    const int xc = min(max(c.x, -kClampXY), kClampXY), yc = min(max(c.y, -kClampXY), kClampXY);
    const int rc = min(c.r, kClampR);
    const bool hit = (base + lane < t.n) && (t.cls < 0 || c.label == t.cls) && c.r >= 0 && xc - rc < t.tx1 &&
                     xc + rc >= t.tx0 && yc - rc < t.ty1 && yc + rc >= t.ty0;
    return __ballot(hit);
}
template <int SRC = kSrcObjects>
__device__ __forceinline__ unsigned long long cull_round(const TileCtx& t, int base, int lane, int& x, int& y, int& r)
{
    const Cand c = cull_load<SRC>(t, base, lane);
    x = c.x;
    y = c.y;
    r = c.r;
    return cull_test(t, base, lane, c);
}

// hit record of a lane that passed the cull: the exact clipped box of the reference (left/right/top/bottom,
// cuh:64-67, 92-95; 64-bit), relative to the tile and clamped to it; an empty exact box masks every pixel
__device__ __forceinline__ float hit_exponent_scale(const SplatParams& p, int r)   // log2(e) / (2 sigma^2), sigma = diameter / factor
{
    const float sigma = (float)(2 * r + 1) / p.factor;
    return kLog2e / (2.0f * sigma * sigma);
}
__device__ __forceinline__ Hit make_hit(const SplatParams& p, const TileCtx& t, int x, int y, int r, float c2);
__device__ __forceinline__ Hit make_hit(const SplatParams& p, const TileCtx& t, int x, int y, int r)
{
    return make_hit(p, t, x, y, r, hit_exponent_scale(p, r));
}
// (c2 given: point splats share one radius, and the two IEEE divisions behind it were repeated per lane and fetched group)
__device__ __forceinline__ Hit make_hit(const SplatParams& p, const TileCtx& t, int x, int y, int r, float c2)
{
    const long long x0 = (long long)x - min(x, r), x1 = (long long)x + min((long long)p.W - x, (long long)r + 1);
    const long long y0 = (long long)y - min(y, r), y1 = (long long)y + min((long long)p.H - y, (long long)r + 1);
    const long long xlo = max(x0, (long long)t.tx0) - t.tx0, xhi = min(x1, (long long)t.tx1) - t.tx0;
    const long long ylo = max(y0, (long long)t.ty0) - t.ty0, yhi = min(y1, (long long)t.ty1) - t.ty0;
    unsigned box = 0;  // empty: only possible for coordinates beyond the clamps of the cull
    if (xhi > xlo && yhi > ylo) box = (unsigned)xlo | ((unsigned)xhi << 8) | ((unsigned)ylo << 16) | ((unsigned)yhi << 24);
    return Hit{x, y, c2, box};
}

// the same for two candidates at once (v_max3_f32 follows the same NaN rule: NaN operands are skipped)
__device__ __forceinline__ float max3_skip_nan(float acc, float a, float b)
{
    float r;
    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(acc), "v"(a), "v"(b));
    return r;
}

// Prologue of the multi-scale kernels.  Their tiles are short-lived waves (most of a lane raster's tiles store zeros and leave),
// and what such a wave did first was a CHAIN of dependent scalar loads: number of scales -> prefix entry after prefix entry ->
// one field of the scale's parameters, a branch, the next field ... (~20 load / wait pairs in the ISA of round 3's point splat).
// Here the scale comes from the whole prefix at once, without a branch (entries past the last scale hold the total: never
// matched), and the scale's parameters are copied in one batch of loads, held there by empty asm statements.
__device__ __forceinline__ int scale_of_group(const MultiParams& mp, long long group, long long& first)
{
    int s = 0;
    first = 0;   // tile_begin[0]
#pragma unroll
    for (int i = 1; i < kMaxScales; ++i) {
        const long long begin = mp.tile_begin[i];
        if (group >= begin) {
            s = i;
            first = begin;
        }
    }
    return s;
}
template <typename T>
__device__ __forceinline__ void pin_scalar(T& v)
{
    asm volatile("" : "+s"(v));
}
__device__ __forceinline__ SplatParams preload_params(const SplatParams& src)
{
    SplatParams p = src;
    // (the pointers are left alone: behind an asm statement hipcc no longer knows them to be global memory and turns every load
    // through them — the frame's count, a scalar load before — into a flat VMEM load)
    asm volatile("" ::"s"(p.hm), "s"(p.counts), "s"(p.centers_f), "s"(p.boxes_f));   // (requested with the rest, value untouched)
    pin_scalar(p.H);
    pin_scalar(p.W);
    pin_scalar(p.n_max);
    pin_scalar(p.n_classes);
    pin_scalar(p.tiles_x);
    pin_scalar(p.tiles_y);
    pin_scalar(p.n_tiles);
    pin_scalar(p.factor);
    pin_scalar(p.k);
    pin_scalar(p.counts_i64);
    pin_scalar(p.grid3d);
    pin_scalar(p.dense_area);
    pin_scalar(p.stride);
    pin_scalar(p.radius);
    pin_scalar(p.n_groups);
    return p;
}

// data-parallel-primitive moves (gfx9 DPP controls); lanes without a source lane keep `old`
constexpr int kDppQuad0 = 0x00, kDppQuad1 = 0x55, kDppQuad2 = 0xAA, kDppQuad3 = 0xFF;   // broadcast lane 0..3 of every quad
constexpr int kDppRowShr = 0x110;                                                      // + n: lane i <- lane i - n inside rows of 16
constexpr int kDppWaveShl1 = 0x130, kDppWaveShr1 = 0x138;                              // lane i <- lane i + 1 / i - 1, whole wave
template <int CTRL>
__device__ __forceinline__ float dpp_f(float old, float src)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(old), __float_as_int(src), CTRL, 0xf, 0xf, false));
}
template <int CTRL>
__device__ __forceinline__ int dpp_i(int old, int src)
{
    return __builtin_amdgcn_update_dpp(old, src, CTRL, 0xf, 0xf, false);
}

}  // namespace
