// The LDS small-splat family of the heat-map rasteriser: the tile lives in LDS and the lanes walk each hit's box (walk_hits,
// splat_round), the two-level cull over sample-group boxes, the write-back of the LDS tile, small_body and its kernels
// splat_small_kernel (ACCV_HM_SMALL_RADII) and splat_points_multi_kernel (lane raster from sampled points).
// Included once, from draw_heatmap.hip; needs splat_common.h.
#pragma once

namespace {

// ---------------------------------------------------------------- small splats (lane rasters, point-like targets)
// The tile kernel above pays a full 128x16-pixel register update per hit, whatever the size of the object's box.  For
// boxes of a few pixels (a lane sample of radius 2 covers 5x5) that is 2048 pixel updates for 25 useful ones, and
// tiles that a lane crosses hold 10^2 such hits.  This variant keeps the tile in LDS instead (8 KB per wave) and, per
// hit, lets 16 lanes walk the pixels of the hit's clipped box only: v = k * exp2(-(dx^2 + dy^2) c), one LDS float-max
// atomic (ds_max_f32) per box pixel, four hits in flight per wave.  Correct for any radius, but only faster below
// ~15x15 boxes; the host selects it on the caller's ACCV_HM_SMALL_RADII hint.  Same culling, same store path, same
// clear / in-place semantics.  SRC = 2 (splat_points_multi_kernel) reads float sample points and culls in two levels.
// NW waves share one tile (NW = 4 for the lane raster): a tile crossed by several lanes at a coarse scale has 6-8 sample
// groups to walk, a serial chain of ~2.5 us per group for ONE wave (24 us for the 576 tiles of a stride-16 map, as long
// as the 8704 tiles of the stride-4 map take) — with four waves the groups of a tile are dealt round-robin over the waves
// (the LDS float-max atomics commute, also across waves), and an empty tile is stored by four waves with two store
// instructions each instead of one wave with eight.
// ---- pieces of the per-tile body (small_body)
constexpr int kSmallTW = 128, kSmallTH = 16;
// LDS row stride of the tile: 128 + 4 floats.  The row walk below puts consecutive ROWS of a splat on consecutive lanes; with a
// stride of 128 floats they would all land on one LDS bank, with 132 they are 4 banks apart (16-byte row reads stay aligned)
constexpr int kSmallLdsW = kSmallTW + 4;
using SmallTile = float (*)[kSmallLdsW];

// the hits of a cull round (or of several, merged) are walked box by box.  Pixel updates are LDS float-max atomics
// (ds_max_f32, no return value): they commute, so neither overlapping boxes of concurrent hits nor successive hits need
// any ordering — the wave just streams them.
// rows_hint > 0: no clipped box of the list is taller than that (point splats: 2 r + 1) — then a lane takes ONE ROW of one hit
// and runs along its columns (radius 2: 12 hits per pass, 5 updates per lane) instead of 16 lanes sharing a hit's box in
// row-major order (4 hits per pass, 2 trips of ~15 dependent instructions for 25 pixels).  With one wave per tile the walk
// is part of the tile's serial chain, and the tiles of a coarse scale carry dozens of hits (round 3)
template <bool WG_SCOPE>
__device__ __forceinline__ void walk_hits(const SplatParams& p, const TileCtx& t, int lane, int nh, const Hit* __restrict__ hits,
                                          SmallTile tile, int rows_hint)
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // the hit list is complete
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (rows_hint > 0 && rows_hint <= 7) {   // (taller boxes: the 16-lane walk below needs fewer trips per hit — measured at r = 5)
        const int per_pass = 64 / rows_hint;
        const int hl = (int)((float)lane * (1.0f / (float)rows_hint) + 1e-3f);   // lane / rows_hint for lane < 64, rows <= 7
        const int rl = lane - hl * rows_hint;
        for (int h0 = 0; h0 < nh; h0 += per_pass) {
            const int h = h0 + hl;
            if (h >= nh || hl >= per_pass) continue;
            const Hit hh = hits[h];
            const int xlo = hh.box & 255u, xhi = (hh.box >> 8) & 255u, ylo = (hh.box >> 16) & 255u, yhi = hh.box >> 24;
            const int py = ylo + rl;
            if (py >= yhi) continue;
            const float dy = (float)(t.ty0 + py - hh.y);
            const float dy2 = dy * dy;
            float* row = &tile[py][0];
            for (int px = xlo; px < xhi; ++px) {
                const float dx = (float)(t.tx0 + px - hh.x);
                const float v = p.k * raw_exp2(-(dx * dx + dy2) * hh.c2);
                __hip_atomic_fetch_max(row + px, v, __ATOMIC_RELAXED,
                                       WG_SCOPE ? __HIP_MEMORY_SCOPE_WORKGROUP : __HIP_MEMORY_SCOPE_WAVEFRONT);
            }
        }
    } else {   // four hits at a time, 16 lanes per hit over its box in row-major order
        const int grp = lane >> 4, l16 = lane & 15;
        for (int h0 = 0; h0 < nh; h0 += 4) {
            const int h = h0 + grp;
            if (h >= nh) continue;
            const Hit hh = hits[h];
            const int xlo = hh.box & 255u, xhi = (hh.box >> 8) & 255u, ylo = (hh.box >> 16) & 255u, yhi = hh.box >> 24;
            const int w = xhi - xlo, area = w * (yhi - ylo);  // 0 for an empty box
            const float inv_w = 1.0f / (float)max(w, 1);
            for (int q = l16; q < area; q += 16) {
                // q / w for q < 2048, w <= 128: (q + 0.5) / w is at least 1/256 away from an integer, far more
                // than the error of the reciprocal
                const int py = (int)(((float)q + 0.5f) * inv_w);
                const int px = q - py * w;
                const float dx = (float)(t.tx0 + xlo + px - hh.x), dy = (float)(t.ty0 + ylo + py - hh.y);
                const float v = p.k * raw_exp2(-(dx * dx + dy * dy) * hh.c2);
                __hip_atomic_fetch_max(&tile[ylo + py][xlo + px], v, __ATOMIC_RELAXED,
                                       WG_SCOPE ? __HIP_MEMORY_SCOPE_WORKGROUP : __HIP_MEMORY_SCOPE_WAVEFRONT);
            }
        }
    }
    // the next round overwrites the hit list: order it behind this round's reads
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
template <bool WG_SCOPE>
__device__ __forceinline__ int splat_round(const SplatParams& p, const TileCtx& t, int lane, unsigned long long m, const Cand& cand,
                                           Hit* __restrict__ hits, SmallTile tile, int rows_hint = 0)
{
    const int nh = __popcll(m);
    int rows = 0;
    if ((m >> lane) & 1ull) {
        const Hit mine = make_hit(p, t, cand.x, cand.y, cand.r);
        hits[__popcll(m & ((1ull << lane) - 1ull))] = mine;
        rows = (int)(mine.box >> 24) - (int)((mine.box >> 16) & 255u);
    }
    if (rows_hint == 0) {   // objects of any radius (splat_small_kernel): the tallest clipped box of this round, wave-uniform
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) rows = max(rows, __shfl_xor(rows, d));
        rows_hint = max(1, __builtin_amdgcn_readfirstlane(rows));
    }
    walk_hits<WG_SCOPE>(p, t, lane, nh, hits, tile, rows_hint);
    return nh;
}

// sample-group bounding box (float, source pixels) of group g; valid = false for an empty group (a group of NaN points keeps
// xmin = +inf) or a group past the plane's sample count
struct GroupBox {
    float x0, y0, x1, y1;
    bool valid;
};
template <bool FIRST = false>   // FIRST: g = lane, the box plane_objects<true> requested (t.box0)
__device__ __forceinline__ GroupBox load_group_box(const SplatParams& p, const TileCtx& t, int g)
{
    // the load is UNCONDITIONAL (index clamped; callers run only with n_groups >= 1): its address does not depend on the
    // plane's sample count, so it is in flight together with the count's load instead of behind it — one dependent round
    // trip less in front of every tile's first store
    float4 v = FIRST ? t.box0 : t.boxes_f[min(g, p.n_groups - 1)];
    // (all four components at once: left alone, hipcc splits the load and sinks three of the pieces into the short-circuit
    // evaluation of group_reaches() — up to three dependent round trips to memory where one does)
    asm volatile("" : "+v"(v.x), "+v"(v.y), "+v"(v.z), "+v"(v.w));
    return GroupBox{v.x, v.y, v.z, v.w, g < p.n_groups && g * kCand < t.n && v.x <= v.z};
}
// can a sample of the group reach pixel columns [cx0, cx1) x rows [cy0, cy1) of this scale?  CONSERVATIVE and division-free
// (the exact integer test runs per candidate afterwards): a sample at source x lands on pixel int(x / stride), which lies in
// (x / stride - 1, x / stride], and is drawn over [pixel - r, pixel + r]; the comparisons below are done in source pixels
// with one extra pixel of slack on either side for the rounding of the products.
struct ReachBounds {
    float xlo, xhi, ylo, yhi;   // the group can reach the region iff box.x1 >= xlo && box.x0 < xhi && (same in y)
};
__device__ __forceinline__ ReachBounds reach_bounds(const TileCtx& t, int rc, int cx0, int cx1, int cy0, int cy1)
{
    const float r1 = (float)min(rc, 1 << 24) + 2.0f;
    return ReachBounds{((float)cx0 - r1) * t.stride, ((float)cx1 + r1) * t.stride, ((float)cy0 - r1) * t.stride,
                       ((float)cy1 + r1) * t.stride};
}
__device__ __forceinline__ bool group_reaches(const GroupBox& b, const ReachBounds& rb)
{
    return b.valid && b.x1 >= rb.xlo && b.x0 < rb.xhi && b.y1 >= rb.ylo && b.y0 < rb.yhi;
}

// candidates of sample group `g` (one per lane), in two steps so that the requests of several groups are in flight together
// (fetch + use in one function made every group its own round trip to memory: the use waits for the data): the raw sample ...
__device__ __forceinline__ float2 request_group_samples(const TileCtx& t, int sub_base, int lane)
{
    return t.centers_f[min(sub_base + lane, t.n - 1)];  // n >= 1 inside the candidate loop
}
// ... and its target at this scale, exactly cull_load<2>; consecutive samples that land on the same pixel are one and the same
// splat (coarse scales see several samples per pixel): the first of a run is kept, results are unchanged
// x / stride, exactly: for a stride that is a power of two the product with its reciprocal is the same correctly rounded
// value as the IEEE division (both round x * 2^-k once) and costs one instruction instead of a dozen
struct PixelScale {
    float stride, inv;
    bool pow2;   // wave-uniform
};
__device__ __forceinline__ PixelScale pixel_scale(float stride)
{
    const bool pow2 = (__float_as_uint(stride) & 0x007fffffu) == 0u && stride > 1.0e-30f && stride < 1.0e30f;
    return PixelScale{stride, pow2 ? 1.0f / stride : 0.0f, pow2};
}
__device__ __forceinline__ float to_pixels(float x, const PixelScale& ps) { return ps.pow2 ? x * ps.inv : __fdiv_rn(x, ps.stride); }
__device__ __forceinline__ Cand group_candidates(const TileCtx& t, const PixelScale& ps, const float2 c, int lane)
{
    Cand out{(int)to_pixels(c.x, ps), (int)to_pixels(c.y, ps), t.radius, 0};
    if ((c.x != c.x) || (c.y != c.y)) out = Cand{0, 0, -1, 0};
    const int nx = dpp_i<kDppWaveShr1>(0, out.x), ny = dpp_i<kDppWaveShr1>(0, out.y), nr = dpp_i<kDppWaveShr1>(-2, out.r);
    if (lane > 0 && nx == out.x && ny == out.y && nr == out.r) out.r = -1;
    return out;
}

template <int SM>
__device__ __forceinline__ void store_segment(const SplatParams& p, float* plane_ptr, int row, int col0, const vfloat4& v)
{
    if constexpr (SM == kStoreWriteThrough) {
        const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(plane_ptr, 0, (int)((size_t)p.H * p.W * 4), 0x00020000);
        __builtin_amdgcn_raw_buffer_store_b128(v, rsrc, (int)(((size_t)row * p.W + col0) * 4), 0, 18);
    } else {
        *reinterpret_cast<vfloat4*>(plane_ptr + (size_t)row * p.W + col0) = v;
    }
}

// rows [row0, row0 + RPW) of the finished LDS tile -> the map.  Fused clear: every segment is written (once).  In place: a
// segment still at its initial value (-inf) received nothing and is neither read nor written.
template <bool CLEAR, int SM, int RPW>
__device__ __forceinline__ void write_back_rows(const SplatParams& p, const TileCtx& t, float* plane_ptr, SmallTile tile, int row0,
                                                int lane, int col0)
{
    const float init = CLEAR ? 0.0f : -__builtin_inff();
    // the rows are read from LDS in batches of up to four (all reads of a batch in flight together — one row at a time was a chain
    // of RPW LDS round trips at the end of every touched tile), in place the old segments of a batch are requested together too
    constexpr int kBatch = RPW > 4 ? 4 : RPW;
    static_assert(RPW % kBatch == 0, "rows per half-wave come in whole batches");
#pragma unroll
    for (int i0 = 0; i0 < RPW; i0 += kBatch) {
        vfloat4 out[kBatch];
#pragma unroll
        for (int i = 0; i < kBatch; ++i) out[i] = *reinterpret_cast<const vfloat4*>(&tile[row0 + i0 + i][(lane & 31) * 4]);
        if constexpr (CLEAR) {
#pragma unroll
            for (int i = 0; i < kBatch; ++i) {
                const int row = t.ty0 + row0 + i0 + i;
                if (row < p.H) store_segment<SM>(p, plane_ptr, row, col0, out[i]);
            }
        } else {
            bool dirty[kBatch];
            vfloat4 old[kBatch];
#pragma unroll
            for (int i = 0; i < kBatch; ++i) {
                const int row = t.ty0 + row0 + i0 + i;
                dirty[i] = row < p.H && !(out[i].x == init && out[i].y == init && out[i].z == init && out[i].w == init);
                old[i] = vfloat4{0.0f, 0.0f, 0.0f, 0.0f};
                if (dirty[i]) old[i] = *reinterpret_cast<const vfloat4*>(plane_ptr + (size_t)row * p.W + col0);
            }
            const float nanv = __builtin_nanf("");
#pragma unroll
            for (int i = 0; i < kBatch; ++i) {
                if (!dirty[i]) continue;
                vfloat4 o = out[i];
                o.x = max_skip_nan(old[i].x, o.x == init ? nanv : o.x);
                o.y = max_skip_nan(old[i].y, o.y == init ? nanv : o.y);
                o.z = max_skip_nan(old[i].z, o.z == init ? nanv : o.z);
                o.w = max_skip_nan(old[i].w, o.w == init ? nanv : o.w);
                store_segment<SM>(p, plane_ptr, t.ty0 + row0 + i0 + i, col0, o);
            }
        }
    }
}

template <bool CLEAR, int SM, int SRC, int NW = 1, int TH = kSmallTH>
__device__ __forceinline__ void small_body(const SplatParams& p, long long linear_group, Hit (*s_hit)[kCand], SmallTile s_tile)
{
    constexpr int TW = kSmallTW;
    constexpr int RPW = TH / NW / 2;  // rows per half-wave in the init / read-back passes
    static_assert(TH % (2 * NW) == 0, "rows must split evenly over the half-waves of the workgroup");

    const int lane = threadIdx.x & 63;
    const int wave = NW > 1 ? __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6) : 0;
    TileCtx t;
    if (!locate_tile<TW, TH, 1, SRC == kSrcPoints>(p, 0, t, linear_group)) return;  // uniform over the workgroup
    const int sub = lane >> 5, col0 = t.tx0 + (lane & 31) * 4;
    const int row0 = wave * (TH / NW) + sub * RPW;               // first of this half-wave's rows
    float* plane_ptr = p.hm + (size_t)t.plane * (size_t)p.H * (size_t)p.W;

    // "untouched" is -inf in the LDS tile (fused-clear mode starts from 0 = the cleared map).  Round 3: the tile is set up
    // LAZILY, at the first sample (group) that can reach it — a tile nothing reaches (most tiles of a lane raster) costs
    // no LDS traffic and no barrier: fused clear stores its zeros, in place does nothing.  The condition is uniform over
    // the workgroup.
    const float init = CLEAR ? 0.0f : -__builtin_inff();
    // ONE register quad for the initial value: prepare_tile is inlined into every unrolled cull round, and hipcc otherwise
    // materialises a fresh copy of the constant per store (8 rows x 4 rounds x 4 registers: 188 VGPRs, 2 waves per SIMD)
    vfloat4 vinit = vfloat4{init, init, init, init};
    asm volatile("" : "+v"(vinit));
    bool tile_ready = false;
    auto prepare_tile = [&]() {
        if (tile_ready) return;
        tile_ready = true;
#pragma unroll
        for (int i = 0; i < RPW; ++i) *reinterpret_cast<vfloat4*>(&s_tile[row0 + i][(lane & 31) * 4]) = vinit;
        if constexpr (NW > 1) {
            __syncthreads();  // tile initialised by all waves before the first atomic of any
        } else {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // tile initialised before the first atomic
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
    };
    // one cull round over the 64 candidates [sub_base, sub_base + 64)
    auto process_round = [&](int sub_base, const Cand& cand) {
        const unsigned long long m = cull_test(t, sub_base, lane, cand);
        if (m == 0) return;
        if constexpr (NW == 1) prepare_tile();   // (NW > 1: the caller prepared it — a barrier must not sit in per-wave flow)
        splat_round<(NW > 1)>(p, t, lane, m, cand, s_hit[wave], s_tile);
    };

    if constexpr (SRC == kSrcPoints) {
        // two-level cull: consecutive polyline samples are neighbours in space, so each group of 64 carries a
        // bounding box (group_boxes_kernel); a lane tests one GROUP, and only groups that can reach the tile are
        // walked candidate by candidate — a tile crossed by a lane visits 1-3 rounds instead of all of them
        const int rc = min(max(t.radius, 0), 1 << 30);
        const int rows_hint = 2 * min(rc, 64) + 1;   // every sample has the same radius: no clipped box is taller
        const float c2_tile = hit_exponent_scale(p, t.radius);   // ... and the same exponent scale
        const PixelScale ps = pixel_scale(t.stride);
        const ReachBounds rb = reach_bounds(t, rc, t.tx0, t.tx1, t.ty0, t.ty1);
        for (int g0 = 0; g0 < p.n_groups; g0 += kCand) {
            unsigned long long mg = __ballot(group_reaches(g0 == 0 ? load_group_box<true>(p, t, lane) : load_group_box(p, t, g0 + lane), rb));
            if (mg == 0) continue;
            if constexpr (NW > 1) {  // every wave found the same groups; this one walks the (k * NW + wave)-th of them
                unsigned long long mine = 0;
                int k = 0;
                for (unsigned long long rest = mg; rest; rest &= rest - 1, ++k)
                    if (k % NW == wave) mine |= rest & (~rest + 1ull);
                mg = mine;
            }
            do {  // wave-uniform; the candidates of up to four groups are fetched together (one round trip)
                constexpr int kFetch = 4;
                int sub_base[kFetch];
                float2 raw[kFetch];
                Cand cand[kFetch];
#pragma unroll
                for (int u = 0; u < kFetch; ++u) {
                    sub_base[u] = -1;
                    raw[u] = float2{0.0f, 0.0f};
                    if (mg) {
                        sub_base[u] = (g0 + __builtin_ctzll(mg)) * kCand;
                        mg &= mg - 1;
                        raw[u] = request_group_samples(t, sub_base[u], lane);
                    }
                }
                // NW > 1: the tile is set up (LDS writes + a barrier, uniform over the workgroup: every wave saw the same
                // groups and comes through here even when none of them is its own) BEHIND the candidate requests, so that
                // the barrier overlaps their flight
                if constexpr (NW > 1) prepare_tile();
#pragma unroll
                for (int u = 0; u < kFetch; ++u)
                    if (sub_base[u] >= 0) cand[u] = group_candidates(t, ps, raw[u], lane);
                // Round 3: the hits of the (up to four) fetched groups go into ONE list and are walked together when they fit
                // it — a tile of a coarse scale is crossed by several lanes, each contributing a handful of samples per
                // group, and one compaction + one walk replaces four dependent ballot / LDS / fence / walk rounds
                unsigned long long mm[kFetch];
                int total = 0;
#pragma unroll
                for (int u = 0; u < kFetch; ++u) {
                    mm[u] = sub_base[u] >= 0 ? cull_test(t, sub_base[u], lane, cand[u]) : 0ull;
                    total += __popcll(mm[u]);
                }
                if (total == 0) continue;
                if (total <= kCand) {
                    if constexpr (NW == 1) prepare_tile();
                    int at = 0;
#pragma unroll
                    for (int u = 0; u < kFetch; ++u) {
                        if ((mm[u] >> lane) & 1ull)
                            s_hit[wave][at + __popcll(mm[u] & ((1ull << lane) - 1ull))] =
                                make_hit(p, t, cand[u].x, cand[u].y, cand[u].r, c2_tile);
                        at += __popcll(mm[u]);
                    }
                    walk_hits<(NW > 1)>(p, t, lane, total, s_hit[wave], s_tile, rows_hint);
                } else {
#pragma unroll
                    for (int u = 0; u < kFetch; ++u)
                        if (mm[u]) {
                            if constexpr (NW == 1) prepare_tile();
                            splat_round<(NW > 1)>(p, t, lane, mm[u], cand[u], s_hit[wave], s_tile, rows_hint);
                        }
                }
            } while (mg);
        }
    } else {
        static_assert(SRC == kSrcPoints || NW == 1, "the candidate-level cull prepares the tile per wave");
        // long object lists are the normal case here (10^3 lane samples per plane) and the wave needs few registers,
        // so the candidate loads of kFetch rounds are issued together: one memory round trip per kFetch * 64 candidates
        constexpr int kFetch = 4;
        for (int base = 0; base < t.n; base += kFetch * kCand) {
            Cand cand[kFetch];
#pragma unroll
            for (int u = 0; u < kFetch; ++u) cand[u] = cull_load<SRC>(t, base + u * kCand, lane);
#pragma unroll
            for (int u = 0; u < kFetch; ++u) {
                const int sub_base = base + u * kCand;
                if (sub_base >= t.n) break;
                process_round(sub_base, cand[u]);
            }
        }
    }

    if (!tile_ready) {   // nothing reached the tile: fused clear = zeros, in place = no HBM traffic at all
        if constexpr (CLEAR) {
            if (col0 < p.W) {
#pragma unroll
                for (int i = 0; i < RPW; ++i) {
                    const int row = t.ty0 + row0 + i;
                    if (row < p.H) store_segment<SM>(p, plane_ptr, row, col0, vfloat4{0.0f, 0.0f, 0.0f, 0.0f});
                }
            }
        }
        return;
    }
    if constexpr (NW > 1) {
        __syncthreads();  // all atomics of all waves landed before the tile is read back
    } else {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // all atomics landed before the tile is read back
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    if (col0 >= p.W) return;
    write_back_rows<CLEAR, SM, RPW>(p, t, plane_ptr, s_tile, row0, lane, col0);
}

template <bool CLEAR, int SM>
__global__ __launch_bounds__(64) void splat_small_kernel(const SplatParams p)
{
    __shared__ Hit s_hit[1][kCand];
    __shared__ __attribute__((aligned(16))) float s_tile[kSmallTH][kSmallLdsW];
    // (preload_params: +-1 % here — the one-level cull over 10^3 candidates is not bound by its prologue,
    // profiles/r03_prologue_preload_elsewhere.log)
    small_body<CLEAR, SM, kSrcObjects>(p, blockIdx.x, s_hit, s_tile);
}

// lane rasters of all scales in one launch: float sample points, two-level cull (SRC = 2), scale from the tile prefix.
// NW = 4 (four waves share a tile) when coarse scales — many sample groups per tile — make up at least half of the tiles,
// else one wave per tile (decided on the host).  What bounds the launch is the chain of dependent round trips of each
// touched tile (kernel arguments -> count / group boxes -> candidates -> LDS -> store) times the tiles a CU holds at once,
// not an instruction count (PMC: a wave waits 70-77 % of its life).  Round 3 on config 3, in the order it was found
// (profiles/r03_lane_splat_*.log, every variant bit-identical): the tile set-up on first use, zeros ahead of the cull, a
// division-free group test, candidate requests ahead of the set-up barrier, count and box loads in parallel: +-2 % with four
// waves per tile (33.5 us); strips of 2 / 4 tiles per wave 43-77 us; a per-scale choice inside one 256-thread launch 36-37 us;
// coarse tiles dealt out every 2nd / 4th workgroup 36 / 43 us; 128 x 8 tiles 28-30 us.  What paid: ONE wave per tile for the
// whole launch (9 KB of LDS: 17 tiles per CU instead of 8; the coarse tiles' long chains run underneath the fine scale's
// stream) 28.5 us, the hits of up to four sample groups compacted and walked together 27.7 us, and a row of a splat per
// lane in that walk (12 hits per pass instead of 4 — with one wave per tile the walk IS part of the chain) 24.0 us.
template <bool CLEAR, int SM, int NW, int TH = kSmallTH>
__global__ __launch_bounds__(NW * 64) void splat_points_multi_kernel(const MultiParams mp)
{
    __shared__ Hit s_hit[NW][kCand];
    __shared__ __attribute__((aligned(16))) float s_tile[TH][kSmallLdsW];
    long long first;
    const int s = scale_of_group(mp, blockIdx.x, first);
    const SplatParams p = preload_params(mp.scale[s]);
    small_body<CLEAR, SM, kSrcPoints, NW, TH>(p, (long long)blockIdx.x - first, s_hit, s_tile);
}

}  // namespace
