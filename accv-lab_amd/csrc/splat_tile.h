// The headline tile kernel of the heat-map rasteriser: splat_body (one wave per 128 x 2R pixel tile, accumulators in registers)
// and its two kernels, splat_kernel (flat / batched API) and splat_multi_kernel (box maps of up to four scales in one launch).
// Included once, from draw_heatmap.hip; needs splat_common.h and splat_stamps.h.
#pragma once

namespace {

template <int PX, int R, bool CLEAR, int SM, int WPG, int SRC>
__device__ __forceinline__ void splat_body(const SplatParams& p, long long linear_group)
{
    constexpr int kWavesPerGroup = WPG;  // shadows the namespace constant inside the body
    constexpr int TW = 32 * PX;  // 32 lanes side by side cover one row segment of the tile
    constexpr int TH = 2 * R;    // the two half-waves take R rows each
    static_assert(R % 4 == 0, "row registers are fetched four at a time");

    __shared__ Hit s_hit[kWavesPerGroup][kCand];
    __shared__ __attribute__((aligned(16))) float s_ey[kWavesPerGroup][kCand][TH];

    // fused-clear tile kernel: the half-waves share a hit's column factors (see the accumulate loop).  Not the in-place
    // instantiations (register bound) and not the multi-scale launches
    constexpr bool kSharedColumns = CLEAR && SRC == kSrcObjects && PX == 4;
    PhaseStamps<kSplatStampsBuilt && CLEAR && SRC == kSrcObjects && PX == 4> stamps;   // diagnostic build only (splat_stamps.h)
    stamps.start();
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    TileCtx t;
    if (!locate_tile<TW, TH, kWavesPerGroup>(p, wave, t, linear_group)) return;
    const int tx0 = t.tx0, ty0 = t.ty0, n = t.n;
    const long long plane = t.plane;

    const int sub = lane >> 5;  // which half-wave: rows [sub*R, sub*R + R) of the tile
    const int col0 = tx0 + (lane & 31) * PX;

    float acc[R][PX];
    const float init = CLEAR ? 0.0f : __builtin_nanf("");
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
        for (int c = 0; c < PX; ++c) acc[i][c] = init;

    int total_hits = 0;
    float cover = 0.0f;  // SM == 5: this lane's share of sum (2r+1)^2 over the plane's objects (density estimate)

    for (int base = 0; base < n; base += kCand) {
        // ---- cull: conservative 32-bit test, ballot, popcount-prefix compaction into LDS
        int x, y, r;
        const unsigned long long m = cull_round<SRC>(t, base, lane, x, y, r);
        if constexpr (SM == kStoreAdaptive) {
            const float dia = (float)(2 * min(max(r, 0), 1 << 20) + 1);
            cover += (base + lane < n) ? dia * dia : 0.0f;
        }
        const bool hit = (m >> lane) & 1ull;
        const int nh = __popcll(m);
        stamps.cull();
        if (nh == 0) continue;
        if constexpr (!CLEAR) {
            // in-place: the tile is touched -> fetch its current content into the accumulators NOW, so the load
            // latency hides behind the table and accumulate phases (max is order independent)
            if (total_hits == 0 && col0 < p.W) {
                const float* plane_rd = p.hm + (size_t)plane * (size_t)p.H * (size_t)p.W;
#pragma unroll
                for (int i = 0; i < R; ++i) {
                    const int row = ty0 + sub * R + i;
                    if (row < p.H) {
                        if constexpr (PX == 4) {
                            const vfloat4 o = *reinterpret_cast<const vfloat4*>(plane_rd + (size_t)row * p.W + col0);
                            acc[i][0] = o.x;
                            acc[i][1] = o.y;
                            acc[i][2] = o.z;
                            acc[i][3] = o.w;
                        } else {
                            acc[i][0] = plane_rd[(size_t)row * p.W + col0];
                        }
                    }
                }
            }
        }
        if (hit) s_hit[wave][__popcll(m & ((1ull << lane) - 1ull))] = make_hit(p, t, x, y, r);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

        // ---- row-factor table: ey[h][row] = k * exp(-dy^2/var), NaN outside the clipped rows
        for (int t = lane; t < nh * TH; t += 64) {
            const int h = t / TH, rr = t % TH;
            const Hit hy = s_hit[wave][h];
            const float d = (float)(ty0 + rr - hy.y);
            const float v = p.k * raw_exp2(-(d * d) * hy.c2);
            const unsigned ylo = (hy.box >> 16) & 255u, yhi = hy.box >> 24;
            s_ey[wave][h][rr] = ((unsigned)rr >= ylo && (unsigned)rr < yhi) ? v : __builtin_nanf("");
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        stamps.table();

        // ---- accumulate: per hit PX column factors in registers, row factors from LDS.  Hits are taken two at a time:
        // acc = max3(acc, ex_a * ey_a, ex_b * ey_b) is 3 VALU ops per pixel for two hits instead of 4
        const unsigned colr0 = (unsigned)(lane & 31) * PX;  // first column of this lane, tile relative
        auto column_factors = [&](const Hit& hx, float (&ex)[PX]) {
            const unsigned xlo = hx.box & 255u, xhi = (hx.box >> 8) & 255u;
#pragma unroll
            for (int c = 0; c < PX; ++c) {
                const float d = (float)(col0 + c - hx.x);
                const float e = raw_exp2(-(d * d) * hx.c2);
                ex[c] = (colr0 + c >= xlo && colr0 + c < xhi) ? e : __builtin_nanf("");
            }
        };
        // Both half-waves hold the same columns (different rows), so each half evaluates two of the four factors and the
        // halves exchange them: v_permlane32_swap of a register with a copy of itself leaves the lower half's value in every
        // lane of one result and the upper half's in the other.  Same argument and same mask per column: the same factor.
        // A one-round launch ends with the SIMD whose four waves have the most arithmetic between them (phase stamps,
        // DESIGN §3), so what counts is instructions per hit: 2 exp + 2 masks + 2 swaps instead of 4 exp + 4 masks
        [[maybe_unused]] auto column_factors_shared = [&](const Hit& hx, float (&ex)[PX]) {
            if constexpr (PX == 4) {
                const unsigned xlo = hx.box & 255u, xhi = (hx.box >> 8) & 255u;
                unsigned f[2];
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int c = 2 * sub + j;
                    const float d = (float)(col0 + c - hx.x);
                    const float e = raw_exp2(-(d * d) * hx.c2);
                    f[j] = __float_as_uint((colr0 + c >= xlo && colr0 + c < xhi) ? e : __builtin_nanf(""));
                }
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const auto sw = __builtin_amdgcn_permlane32_swap(f[j], f[j], false, false);
                    ex[j] = __uint_as_float(sw[0]);       // from lanes 0-31: column j
                    ex[2 + j] = __uint_as_float(sw[1]);   // from lanes 32-63: column 2 + j
                }
            }
        };
        int h = 0;
        // (fused-clear instantiations only: the in-place ones are register bound, and the second set of factors costs
        // them a wave of occupancy — sparse in-place launches lost 5 %)
        for (; CLEAR && h + 1 < nh; h += 2) {
            float exa[PX], exb[PX];
            if constexpr (kSharedColumns) {
                column_factors_shared(s_hit[wave][h], exa);
                column_factors_shared(s_hit[wave][h + 1], exb);
            } else {
                column_factors(s_hit[wave][h], exa);
                column_factors(s_hit[wave][h + 1], exb);
            }
#pragma unroll
            for (int q = 0; q < R / 4; ++q) {
                const float4 a4 = *reinterpret_cast<const float4*>(&s_ey[wave][h][sub * R + 4 * q]);
                const float4 b4 = *reinterpret_cast<const float4*>(&s_ey[wave][h + 1][sub * R + 4 * q]);
                const float eya[4] = {a4.x, a4.y, a4.z, a4.w}, eyb[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int c = 0; c < PX; ++c)
                        acc[4 * q + i][c] = max3_skip_nan(acc[4 * q + i][c], exa[c] * eya[i], exb[c] * eyb[i]);
            }
        }
        for (; h < nh; ++h) {
            float ex[PX];
            if constexpr (kSharedColumns)
                column_factors_shared(s_hit[wave][h], ex);
            else
                column_factors(s_hit[wave][h], ex);
#pragma unroll
            for (int q = 0; q < R / 4; ++q) {
                const float4 e4 = *reinterpret_cast<const float4*>(&s_ey[wave][h][sub * R + 4 * q]);
                const float ey[4] = {e4.x, e4.y, e4.z, e4.w};
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int c = 0; c < PX; ++c) acc[4 * q + i][c] = max_skip_nan(acc[4 * q + i][c], ex[c] * ey[i]);
            }
        }
        total_hits += nh;
        stamps.accumulate();
        // the next round overwrites the LDS lists: order it behind this round's reads
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }

    if (!CLEAR && total_hits == 0) return;  // in-place: untouched tile costs no HBM traffic
    if (col0 >= p.W) return;                 // PX == 4 requires W % 4 == 0, so a lane is all-in or all-out

    using V = typename Vec<PX>::type;
    float* plane_ptr = p.hm + (size_t)plane * (size_t)p.H * (size_t)p.W;
    // SM == 5 (in-place launches): the store policy is chosen PER PLANE from the density of its objects, known to the
    // wave for free after its cull loop: sum (2r+1)^2 over the plane's objects relative to the plane's area.  Planes that
    // are covered about once or more rewrite most of their tiles -> write-through non-temporal stores (sc1 nt: -6 % on
    // the dense rule-A batch); sparse planes touch a few tiles that the next consumer finds in L2 / Infinity Cache ->
    // plain stores (write-through costs them 27 %, profiles/r01_h1_ab_rows_store_policy.log).  Same values either way.
    bool write_through = SM == kStoreWriteThrough;
    if constexpr (SM == kStoreAdaptive && PX == 4) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) cover += __shfl_xor(cover, d);
        write_through = cover >= p.dense_area;   // wave-uniform
    }
#pragma unroll
    for (int i = 0; i < R; ++i) {
        const int row = ty0 + sub * R + i;
        if (row >= p.H) break;
        V* dst = reinterpret_cast<V*>(plane_ptr + (size_t)row * p.W + col0);
        V out;
        if constexpr (PX == 4)
            out = V{acc[i][0], acc[i][1], acc[i][2], acc[i][3]};  // in-place mode: acc already holds max(old, splats)
        else
            out = acc[i][0];
        if constexpr (SM != kStorePlain && PX == 4) {
            // write-through non-temporal (sc1 nt) 16-byte buffer store
            if (write_through) {
                const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(plane_ptr, 0, (int)((size_t)p.H * p.W * 4), 0x00020000);
                __builtin_amdgcn_raw_buffer_store_b128(out, rsrc, (int)(((size_t)row * p.W + col0) * 4), 0, 18);   // sc1 | nt
            } else {
                *dst = out;
            }
        } else {
            *dst = out;
        }
    }
    stamps.record(p, (plane * p.tiles_y + ty0 / TH) * p.tiles_x + tx0 / TW, lane, n, total_hits);
}

template <int PX, int R, bool CLEAR, int SM, int WPG = kWavesPerGroup>
__global__ __launch_bounds__(WPG * 64) void splat_kernel(const SplatParams p)
{
    splat_body<PX, R, CLEAR, SM, WPG, kSrcObjects>(p, blockIdx.x);
}

// ---------------------------------------------------------------- multi-scale: all strides of one batch in ONE launch
// A detection head wants the same objects rasterised at several strides (config 3: 4 / 8 / 16).  Per scale that is a
// target-prep launch plus a splat launch of a map of a few MB — launch bound.  Here one grid covers the tiles of every
// scale; a workgroup finds its scale from the tile prefix (wave-uniform), and the candidates are the FLOAT centres and
// boxes in source pixels, converted to that scale's integer centre / radius inside the cull (same arithmetic as
// targets_from_boxes_kernel), so the front end needs no launch and no intermediate tensors at all.
template <bool CLEAR, int SM>
__global__ __launch_bounds__(64) void splat_multi_kernel(const MultiParams mp)
{
    long long first;
    const int s = scale_of_group(mp, blockIdx.x, first);
    // (the scale's parameters are NOT requested up front here, neither as copies (preload_params) nor as asm inputs: either way
    // the register-bound tile body goes from 79 to 85-124 VGPRs and loses one or two waves per SIMD)
    splat_body<4, kBoxTileR, CLEAR, SM, 1, kSrcFloatBoxes>(mp.scale[s], (long long)blockIdx.x - first);
}

}  // namespace
