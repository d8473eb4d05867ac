// H1 — Gaussian heat-map rasteriser for gfx950 (MI355X), written as a GATHER-BY-TILE:
//
//   * the frame is cut into wave tiles of (32*PX) columns x (2*R) rows; one 64-lane wavefront owns one
//     tile, lane l holds PX consecutive pixels of rows {i, i+R} (half-wave each) in registers;
//   * the wave culls the plane's objects against its tile with one __ballot per 64 candidates, compacts the
//     hits into LDS with a popcount prefix (no atomics, no pre-pass, no workspace for the batched API);
//   * exp(-(dx^2+dy^2)/var) is evaluated separably: a per-tile LDS table of k*exp(-dy^2/var) per (hit,row)
//     and PX in-register column factors per hit, so the inner loop is one multiply + one max per pixel;
//     "outside the object's clipped box" is encoded as NaN in either factor — fmaxf(acc, NaN) == acc —
//     which reproduces the reference's write extent exactly for any sign of k and any base value;
//   * max is order independent, so the result is deterministic and equals the reference's atomicMax result;
//   * each pixel is written exactly once with 16-byte stores (fused-clear mode) or read-max-written once
//     (in-place mode, only tiles that are touched).
//
// This file is the only translation unit of the rasteriser: the host dispatch and every extern "C" entry point.  The kernels
// live in headers beside it, each included once, below (all share locate_tile / cull_round / make_hit of splat_common.h):
//   splat_tile.h    splat_kernel        the tile kernel above = splat_body<PX,R,CLEAR,SM,WPG,SRC=0> (headline: <4,8,true,0,1>, in place <4,8,false,5,1>)
//                   splat_multi_kernel  the same body over the tiles of up to four scales in one launch, objects given as float
//                                       centres / boxes and converted per scale inside the cull (SRC=1)
//   splat_small.h   splat_small_kernel  point-like objects (ACCV_HM_SMALL_RADII): tile in LDS, lanes walk each hit's box, ds_max_f32
//                   splat_points_multi_kernel   lane raster: sampled polyline points of all scales, two-level cull (group boxes), same LDS tile
//   splat_lanes.h   lane_raster_multi_kernel    lane raster of sparse lane sets in ONE launch: the tile waves sample the polylines themselves
//                   splat_multi_sampler_kernel  splat_multi_kernel with the polyline sampler riding in the launch (draw_targets_multiscale)
//                   group_boxes_kernel  bounding box of every 64 sampled points, for the two-level cull
//   heatmap_prep.h  bin_* kernels       flat API: counting sort of the objects by plane into plane-sorted copies
//                   targets_from_*      float boxes / sampled polyline points -> integer centre + radius
//                   fill_kernel, fill_tail_kernel   accv_fill_f32
//   splat_stamps.h  no kernel: the phase stamps of the diagnostic build -DACCV_SPLAT_STAMPS
//
// Replaces: packages/draw_heatmap/accvlab/draw_heatmap/include/draw_heatmap_cuda_kernel.cuh:26-108 and
// csrc/draw_heatmap_cuda.cu:29-165 of the reference (one thread per object, serial atomicMax splat).
// Plane offsets are 64-bit (the reference's are int and overflow for class-wise full-HD batches).
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <atomic>
#include <climits>
#include <cstdint>
#include <cstring>
#include <type_traits>

#include "accv_common.h"
#include "splat_common.h"
#include "splat_stamps.h"
#include "splat_tile.h"
#include "splat_small.h"
#include "splat_lanes.h"
#include "heatmap_prep.h"

namespace {

void note_dispatch(const char* kernel, int px, int r, bool clear, int sm, const dim3& grid, const dim3& block)
{
    snprintf(accv::dispatch_buffer(), 256, "%s<PX=%d,R=%d,CLEAR=%d,SM=%d> grid(%u,%u,%u) block(%u)", kernel, px, r, clear ? 1 : 0,
             sm, grid.x, grid.y, grid.z, block.x);
}

// one-shot, per thread: events for the splat launch of the next flat / batched call (accv_draw_heatmap_time_next_launch)
struct LaunchEvents {
    hipEvent_t start = nullptr, stop = nullptr;
};
LaunchEvents& launch_events()
{
    static thread_local LaunchEvents ev;
    return ev;
}
LaunchEvents take_launch_events()
{
    const LaunchEvents ev = launch_events();
    launch_events() = LaunchEvents{};
    return ev;
}
// same kernel, same launch parameters; with events the kernel's own start / stop time stamps are recorded (hip_ext.h)
template <class K>
inline void launch_maybe_timed(K kernel, const dim3& grid, const dim3& block, hipStream_t stream, const LaunchEvents& ev,
                               const SplatParams& p)
{
    if (ev.start || ev.stop)
        hipExtLaunchKernelGGL(kernel, grid, block, 0, stream, ev.start, ev.stop, 0, p);
    else
        hipLaunchKernelGGL(kernel, grid, block, 0, stream, p);
}
// the run-time (clear, write-through) pair as compile-time constants: f(std::bool_constant<CLEAR>{}, std::integral_constant<int,
// SM>{}) with SM = kStoreWriteThrough (write-through non-temporal stores) or kStorePlain (plain stores)
template <class F>
void with_variant(bool clear, bool write_through, F&& f)
{
    using Plain = std::integral_constant<int, kStorePlain>;
    using WriteThrough = std::integral_constant<int, kStoreWriteThrough>;
    if (clear && write_through)
        f(std::true_type{}, WriteThrough{});
    else if (clear)
        f(std::true_type{}, Plain{});
    else if (write_through)
        f(std::false_type{}, WriteThrough{});
    else
        f(std::false_type{}, Plain{});
}

int launch_splat_small(SplatParams p, long long planes, bool clear, bool write_through, hipStream_t stream, const LaunchEvents& ev)
{
    p.tiles_x = (p.W + 127) / 128;
    p.tiles_y = (p.H + 15) / 16;
    p.n_tiles = planes * p.tiles_x * p.tiles_y;
    if (p.n_tiles == 0) return ACCV_OK;
    dim3 grid;
    p.grid3d = (planes <= 65535 && p.tiles_y <= 65535) ? 1 : 0;
    if (p.grid3d) {
        grid = dim3((unsigned)p.tiles_x, (unsigned)p.tiles_y, (unsigned)planes);
    } else {
        if (p.n_tiles > INT_MAX) return accv::fail(ACCV_EINVAL, "draw_heatmap: %lld tiles exceed the grid limit", p.n_tiles);
        grid = dim3((unsigned)p.n_tiles);
    }
    with_variant(clear, write_through, [&](auto CL, auto SM) {
        launch_maybe_timed(splat_small_kernel<CL, SM>, grid, dim3(64), stream, ev, p);
    });
    note_dispatch("splat_small_kernel", 4, 8, clear, write_through ? kStoreWriteThrough : kStorePlain, grid, dim3(64));
    return accv::check_launch("draw_heatmap small-splat kernel");
}

// store mode sm: kStorePlain, kStoreWriteThrough (non-temporal, sc1 nt) or kStoreAdaptive (by density; in-place launches only: a
// fused-clear launch asking for it gets plain stores).  PX == 1 has plain stores only.
template <int PX, int R>
int launch_splat(SplatParams p, long long planes, bool clear, int sm, hipStream_t stream, const LaunchEvents& ev)
{
    p.tiles_x = (p.W + 32 * PX - 1) / (32 * PX);
    p.tiles_y = (p.H + 2 * R - 1) / (2 * R);
    p.n_tiles = planes * p.tiles_x * p.tiles_y;
    if (p.n_tiles == 0) return ACCV_OK;
    const int groups_x = (p.tiles_x + kWavesPerGroup - 1) / kWavesPerGroup;
    dim3 grid, block(kWavesPerGroup * 64);
    p.grid3d = (planes <= 65535 && p.tiles_y <= 65535) ? 1 : 0;
    if (p.grid3d) {
        grid = dim3((unsigned)groups_x, (unsigned)p.tiles_y, (unsigned)planes);
    } else {
        const long long groups = (p.n_tiles + kWavesPerGroup - 1) / kWavesPerGroup;
        if (groups > INT_MAX) return accv::fail(ACCV_EINVAL, "draw_heatmap: %lld tiles exceed the grid limit", p.n_tiles);
        grid = dim3((unsigned)groups);
    }
    attach_splat_stamps(p);   // diagnostic build only (splat_stamps.h)
    if (PX == 1 || (sm == kStoreAdaptive && clear)) sm = kStorePlain;
    if (sm == kStoreAdaptive) {
        if constexpr (PX == 4) launch_maybe_timed(splat_kernel<PX, R, false, kStoreAdaptive>, grid, block, stream, ev, p);
    } else {
        with_variant(clear, sm == kStoreWriteThrough, [&](auto CL, auto SM) {
            if constexpr (PX == 4 || SM == kStorePlain) launch_maybe_timed(splat_kernel<PX, R, CL, SM>, grid, block, stream, ev, p);
        });
    }
    note_dispatch("splat_kernel", PX, R, clear, sm, grid, block);
    return accv::check_launch("draw_heatmap splat kernel");
}

// compute units of the current device (cached per device ordinal; 0 when the query fails)
long long compute_units()
{
    static std::atomic<int> cached[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 0;
    int v = cached[dev].load(std::memory_order_relaxed);
    if (v == 0) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) return 0;
        cached[dev].store(n, std::memory_order_relaxed);
        v = n;
    }
    return v;
}

int dispatch_splat(SplatParams p, long long planes, bool clear, unsigned flags, hipStream_t stream, const LaunchEvents& ev)
{
    const bool small_hint = (flags & ACCV_HM_SMALL_RADII) != 0;
    const bool vec4 = (p.W % 4 == 0) && ((reinterpret_cast<uintptr_t>(p.hm) & 15u) == 0);
    // Tile height: 128 x 16 pixel tiles (R = 8) for every launch.  Round 1 shipped 128 x 32 for fused-clear launches above
    // 128 MB after an A/B on nine boxes (profiles/r01_h1_ab_rows_store_policy.log: -4..-7 % there); with this round's
    // build the same A/B on four boxes of the slow class puts R = 8 ahead by 1.1-2.8 % on the headline batch and 6 % on
    // small-object batches (profiles/r02_h1_flags_ab_*.log), and in-place launches always preferred it.  R = 16 stays
    // available as a hint (ACCV_HM_TILE_ROWS_16).  Store policy: plain stores for fused-clear launches; in-place launches
    // decide per plane inside the kernel (SM = 5); ACCV_HM_WRITE_THROUGH / ACCV_HM_PLAIN_STORES override.
    const bool plane_fits_rsrc = (size_t)p.H * p.W * sizeof(float) < ((size_t)1 << 31);
    int nt;
    if (flags & ACCV_HM_WRITE_THROUGH)
        nt = kStoreWriteThrough;
    else if (flags & ACCV_HM_PLAIN_STORES)
        nt = kStorePlain;
    else
        nt = clear ? kStorePlain : kStoreAdaptive;   // in-place: per-plane choice by object density (see the store loop of splat_body)
    if (nt != kStorePlain && !plane_fits_rsrc) nt = kStorePlain;
    p.dense_area = 0.75f * (float)p.H * (float)p.W;
    int rows = (flags & ACCV_HM_TILE_ROWS_16) ? 16 : 8;
    // ... with one exception (round 3): a fused-clear launch whose 128 x 16 tiles are MORE than the chip holds at once (24
    // one-wave workgroups per CU) while its 128 x 32 tiles all fit (16 per CU) runs as a single round of resident tiles
    // instead of one full round plus a short second one — the 8-frame shards of the strong-scaling split (8160 tiles on
    // 256 CUs): 18.1 / 13.8 -> 17.3 / 13.2 us slowest / fastest shard (profiles/r03_small_launch_tile_rows.log); 16 frames
    // and more, which need several rounds either way, keep R = 8 (+0.5..1.5 % with 128 x 32 there)
    if (!(flags & (ACCV_HM_TILE_ROWS_8 | ACCV_HM_TILE_ROWS_16)) && clear && vec4 && !small_hint) {
        const long long cus = compute_units();
        const long long tx = (p.W + 127) / 128;
        const long long tiles8 = planes * tx * ((p.H + 15) / 16), tiles16 = planes * tx * ((p.H + 31) / 32);
        if (cus > 0 && tiles8 > 24 * cus && tiles16 <= 16 * cus) rows = 16;
    }
    if (!p.labels) p.labels = p.radii;  // branch-free candidate loads: always a readable array (ignored when cls < 0)
    if (!vec4) return launch_splat<1, 8>(p, planes, clear, kStorePlain, stream, ev);
    // point-like objects (the caller's ACCV_HM_SMALL_RADII hint): the small-splat kernel has no per-plane density choice.
    // Point-like objects are the sparse case, where write-through costs up to 27 %, so the adaptive default
    // (kStoreAdaptive) means PLAIN stores there; only an explicit ACCV_HM_WRITE_THROUGH selects kStoreWriteThrough
    if (small_hint) return launch_splat_small(p, planes, clear, nt == kStoreWriteThrough, stream, ev);
    if (rows == 16) return launch_splat<4, 16>(p, planes, clear, nt, stream, ev);
    return launch_splat<4, 8>(p, planes, clear, nt, stream, ev);
}

int check_common(int h, int w, const char* who)
{
    if (h < 0 || w < 0) return accv::fail(ACCV_EINVAL, "%s: negative heatmap extent %dx%d", who, h, w);
    if (h > (1 << 29) || w > (1 << 29))
        return accv::fail(ACCV_EINVAL, "%s: heatmap extent %dx%d exceeds 2^29 per dimension", who, h, w);
    return ACCV_OK;
}

// Workgroups are dispatched in linear order: put the COARSE scales first.  Their tiles see the same objects / lane samples on
// fewer pixels, i.e. the longest per-tile chains, and started last they are the tail of the launch; the many short tiles of
// the fine scales fill in behind them (config 3: box maps 19.4 -> 17.4 us, in-place 24.9 -> 22.0, lane raster 40.8 -> 38.7;
// profiles/r02_scale_order_ab.log).
inline void coarse_scales_first(MultiParams& mp)
{
    std::stable_sort(mp.scale, mp.scale + mp.n_scales,
                     [](const SplatParams& a, const SplatParams& b) { return a.n_tiles < b.n_tiles; });
    long long tiles = 0;
    for (int i = 0; i < mp.n_scales; ++i) {
        mp.tile_begin[i] = tiles;
        tiles += mp.scale[i].n_tiles;
    }
    mp.tile_begin[mp.n_scales] = tiles;
}
// entries of the tile prefix past the last scale = the total, so that the kernels find a workgroup's scale with plain
// comparisons (scale_of_group)
inline void seal_tile_prefix(MultiParams& mp)
{
    for (int i = mp.n_scales + 1; i <= kMaxScales; ++i) mp.tile_begin[i] = mp.tile_begin[mp.n_scales];
}

// store mode of the multi-scale launches: plain stores unless the caller asks for write-through.  (dispatch_splat has the
// single-scale policy, with its per-plane choice for in-place launches.)
inline int multiscale_store_mode(unsigned flags) { return (flags & ACCV_HM_WRITE_THROUGH) ? kStoreWriteThrough : kStorePlain; }

// end of the map-rule message of the box and point entry points (the polyline entry point's message has none)
constexpr const char* kPerScaleNote = " (use the per-scale calls otherwise)";
// The per-scale set-up of the multi-scale entry points: checks each map (`who` names the entry point, `map_note` ends the
// message of the map rule), fills mp.scale[0..used) from `proto` plus the scale's map, extent, stride and 128 x tile_h tile
// counts (maps of zero extent are skipped), and builds the tile prefix.  Returns the tile total, or a negative status.
long long setup_scales(MultiParams& mp, const SplatParams& proto, float* const* heatmaps, const int* heights, const int* widths,
                       const float* strides, int num_scales, int batch, int tile_h, unsigned flags, const char* who,
                       const char* map_note)
{
    long long tiles = 0;
    int used = 0;
    for (int i = 0; i < num_scales; ++i) {
        if (int rc = check_common(heights[i], widths[i], who)) return rc;
        if (!(strides[i] > 0.0f)) return accv::fail(ACCV_EINVAL, "%s: stride %d is not positive", who, i);
        if (heights[i] == 0 || widths[i] == 0) continue;
        if (!heatmaps[i]) return accv::fail(ACCV_EINVAL, "%s: heatmap %d is null", who, i);
        if (widths[i] % 4 != 0 || (reinterpret_cast<uintptr_t>(heatmaps[i]) & 15u) ||
            (size_t)heights[i] * widths[i] * sizeof(float) >= ((size_t)1 << 31))
            return accv::fail(ACCV_EINVAL, "%s: map %d needs a width that is a multiple of 4, a 16-byte aligned base and planes "
                                           "below 2 GiB%s", who, i, map_note);
        SplatParams& p = mp.scale[used];
        p = proto;
        p.hm = heatmaps[i];
        p.H = heights[i];
        p.W = widths[i];
        p.stride = strides[i];
        p.tiles_x = (p.W + 127) / 128;
        p.tiles_y = (p.H + tile_h - 1) / tile_h;
        p.n_tiles = (long long)batch * p.tiles_x * p.tiles_y;
        p.grid3d = 0;
        mp.tile_begin[used] = tiles;
        tiles += p.n_tiles;
        ++used;
    }
    mp.n_scales = used;
    mp.tile_begin[used] = tiles;
    if (!(flags & ACCV_HM_CALLER_SCALE_ORDER)) coarse_scales_first(mp);
    seal_tile_prefix(mp);
    return tiles;
}

// What the multi-scale entry points (`who`) check first, in this order: the scale count and the per-scale arrays ...
int check_scale_arrays(const char* who, float* const* heatmaps, const int* heights, const int* widths, const float* strides,
                       int num_scales)
{
    if (num_scales < 1 || num_scales > kMaxScales)
        return accv::fail(ACCV_EINVAL, "%s: 1..%d scales supported, got %d", who, kMaxScales, num_scales);
    if (!heatmaps || !heights || !widths || !strides) return accv::fail(ACCV_EINVAL, "%s: null array", who);
    return ACCV_OK;
}
// ... then the batch and the padded number of `what` ("objects", "points") per sample
int check_scale_counts(const char* who, int batch, int per_sample, const char* what)
{
    if (batch < 0 || per_sample < 0) return accv::fail(ACCV_EINVAL, "%s: negative count", who);
    if (per_sample > (1 << 30)) return accv::fail(ACCV_EINVAL, "%s: more than 2^30 %s per sample", who, what);
    return ACCV_OK;
}
// the fields every scale of a multi-scale launch shares (setup_scales adds the scale's own); the caller adds its object arrays
SplatParams multiscale_proto(const void* counts, int n_max, float diameter_to_sigma_factor, float k_scale, unsigned flags)
{
    SplatParams proto{};
    proto.counts = counts;
    proto.n_max = n_max;
    proto.factor = diameter_to_sigma_factor;
    proto.k = k_scale;
    proto.counts_i64 = (flags & ACCV_HM_COUNTS_I64) ? 1 : 0;
    return proto;
}

}  // namespace

extern "C" {

int accv_draw_heatmap_time_next_launch(void* start_event, void* stop_event)
{
    launch_events() = LaunchEvents{static_cast<hipEvent_t>(start_event), static_cast<hipEvent_t>(stop_event)};
    return ACCV_OK;
}

size_t accv_draw_heatmap_flat_workspace_bytes(int num_planes, int num_objects)
{
    if (num_planes < 0 || num_objects < 0) return 0;
    // bin counters [P] | plane offsets [P+1] | plane-sorted centres int2[N] | plane-sorted radii [N]
    return accv::align_up((size_t)num_planes * 4, 16) + accv::align_up(((size_t)num_planes + 1) * 4, 16) +
           accv::align_up((size_t)num_objects * 8, 16) + accv::align_up((size_t)num_objects * 4, 16) + 16;
}

int accv_draw_heatmap_flat_f32(float* heatmaps, int num_planes, int height, int width, const int32_t* centers,
                               const int32_t* radii, const int32_t* heatmap_idxes, int num_objects,
                               float diameter_to_sigma_factor, float k_scale, unsigned flags, void* workspace,
                               size_t workspace_bytes, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const LaunchEvents ev = take_launch_events();   // consumed by this call whether or not it launches
    if (int rc = check_common(height, width, "draw_heatmap")) return rc;
    if (num_planes < 0 || num_objects < 0) return accv::fail(ACCV_EINVAL, "draw_heatmap: negative count");
    if (num_objects > (1 << 30)) return accv::fail(ACCV_EINVAL, "draw_heatmap: more than 2^30 objects");
    const bool clear = (flags & ACCV_HM_CLEAR) != 0;
    if (num_planes == 0 || height == 0 || width == 0) return ACCV_OK;
    if (!heatmaps) return accv::fail(ACCV_EINVAL, "draw_heatmap: heatmap pointer is null");
    if (num_objects > 0 && (!centers || !radii || !heatmap_idxes))
        return accv::fail(ACCV_EINVAL, "draw_heatmap: null object array");
    if (num_objects == 0 && !clear) return ACCV_OK;
    const size_t need = accv_draw_heatmap_flat_workspace_bytes(num_planes, num_objects);
    if (!workspace || workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 15u))
        return accv::fail(ACCV_EWORKSPACE, "draw_heatmap: workspace needs %zu aligned bytes, got %zu", need,
                          workspace_bytes);

    char* ws = static_cast<char*>(workspace);
    int* cnt = reinterpret_cast<int*>(ws);
    int* off = reinterpret_cast<int*>(ws + accv::align_up((size_t)num_planes * 4, 16));
    char* sc_raw = reinterpret_cast<char*>(off) + accv::align_up(((size_t)num_planes + 1) * 4, 16);
    int2* sorted_centers = reinterpret_cast<int2*>(sc_raw);
    int32_t* sorted_radii = reinterpret_cast<int32_t*>(sc_raw + accv::align_up((size_t)num_objects * 8, 16));

    if (num_planes <= kBinSmallPlanes && num_objects <= kBinSmallObjects) {
        hipLaunchKernelGGL(bin_small_kernel, dim3(1), dim3(1024), 0, stream, heatmap_idxes, num_objects, num_planes,
                           reinterpret_cast<const int2*>(centers), radii, off, sorted_centers, sorted_radii);
    } else {
        if (hipMemsetAsync(cnt, 0, (size_t)num_planes * 4, stream) != hipSuccess)
            return accv::fail(ACCV_ELAUNCH, "draw_heatmap: memset of the bin counters failed");
        const int nb = num_objects > 0 ? min((num_objects + 255) / 256, 1024) : 1;
        if (num_objects > 0)
            hipLaunchKernelGGL(bin_count_kernel, dim3(nb), dim3(256), 0, stream, heatmap_idxes, num_objects, num_planes, cnt);
        hipLaunchKernelGGL(bin_scan_kernel, dim3(1), dim3(1024), 0, stream, cnt, off, num_planes);
        if (num_objects > 0)
            hipLaunchKernelGGL(bin_fill_kernel, dim3(nb), dim3(256), 0, stream, heatmap_idxes, num_objects, num_planes, off,
                               cnt, reinterpret_cast<const int2*>(centers), radii, sorted_centers, sorted_radii);
    }
    if (int rc = accv::check_launch("draw_heatmap binning")) return rc;

    SplatParams p{};
    p.hm = heatmaps;
    p.centers = reinterpret_cast<const int32_t*>(sorted_centers);
    p.radii = sorted_radii;
    p.plane_off = off;
    p.H = height;
    p.W = width;
    p.factor = diameter_to_sigma_factor;
    p.k = k_scale;
    return dispatch_splat(p, num_planes, clear, flags, stream, ev);
}

int accv_draw_heatmap_batched_f32(float* heatmap, int batch, int num_classes, int height, int width,
                                  const int32_t* centers, const int32_t* radii, const void* counts,
                                  const int32_t* labels, int max_num_targets, float diameter_to_sigma_factor,
                                  float k_scale, unsigned flags, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const LaunchEvents ev = take_launch_events();   // consumed by this call whether or not it launches
    if (int rc = check_common(height, width, "draw_heatmap_batched")) return rc;
    if (batch < 0 || max_num_targets < 0 || num_classes < 0)
        return accv::fail(ACCV_EINVAL, "draw_heatmap_batched: negative count");
    if (max_num_targets > (1 << 30))
        return accv::fail(ACCV_EINVAL, "draw_heatmap_batched: more than 2^30 objects per sample");
    if (batch == 0 || height == 0 || width == 0) return ACCV_OK;
    // (an empty [B, 0] or [0, N] label tensor has no storage: without object slots the pointer is not looked at)
    if (max_num_targets > 0 && (num_classes > 0) != (labels != nullptr))
        return accv::fail(ACCV_EINVAL, "draw_heatmap_batched: labels and num_classes must be given together");
    if (!heatmap) return accv::fail(ACCV_EINVAL, "draw_heatmap_batched: heatmap pointer is null");
    if (!counts) return accv::fail(ACCV_EINVAL, "draw_heatmap_batched: counts pointer is null");
    if (max_num_targets > 0 && (!centers || !radii))
        return accv::fail(ACCV_EINVAL, "draw_heatmap_batched: null object array");
    const bool clear = (flags & ACCV_HM_CLEAR) != 0;
    if (max_num_targets == 0 && !clear) return ACCV_OK;

    SplatParams p{};
    p.hm = heatmap;
    p.centers = centers;
    p.radii = radii;
    p.labels = labels;
    p.counts = counts;
    p.H = height;
    p.W = width;
    p.n_max = max_num_targets;
    p.n_classes = num_classes;
    p.factor = diameter_to_sigma_factor;
    p.k = k_scale;
    p.counts_i64 = (flags & ACCV_HM_COUNTS_I64) ? 1 : 0;
    const long long planes = (long long)batch * (num_classes > 0 ? num_classes : 1);
    return dispatch_splat(p, planes, clear, flags, stream, ev);
}

}  // extern "C"

namespace {

// shape rule of the fused lane raster (one place: the entry point below and accv_draw_polylines_fused_applicable)
struct FusedLaneShape {
    bool ok;
    int p2_shift;
};
FusedLaneShape fused_lane_shape(const int* heights, const int* widths, int num_scales, int batch, int lanes, int points,
                                int num_samples)
{
    FusedLaneShape out{false, 0};
    if (lanes < 1 || points < 1 || points > 64 || num_samples < 1 || num_samples > (1 << 20) || batch < 1) return out;
    int sh = 2;   // at least four slots per polyline: the polylines in reach are a 64-bit mask
    while ((1 << sh) < points) ++sh;
    if (((long long)lanes << sh) > kLaneRounds * 64) return out;
    // a pass evaluates 2^sh samples per polyline: more than a pass or two per segment in reach (few, long segments carrying many
    // samples: 8 polylines x 8 points x 256 samples 42 us against 30 us) and the sampler launch is the cheaper way
    if ((long long)num_samples * 2 > (long long)std::max(points - 1, 1) << sh) return out;
    // one wave per tile only: launches that the point splat would run with four waves per tile (coarse scales are at least
    // half of the tiles) stay on the two-launch path
    long long tiles = 0, coarse = 0;
    for (int i = 0; i < num_scales; ++i) {
        if (heights[i] <= 0 || widths[i] <= 0) continue;
        const long long nt = (long long)batch * ((widths[i] + 127) / 128) * ((heights[i] + 15) / 16);
        tiles += nt;
        if ((double)batch * lanes * num_samples >= 24.0 * (double)nt) coarse += nt;
    }
    if (tiles == 0 || 2 * coarse >= tiles) return out;
    out.ok = true;
    out.p2_shift = sh;
    return out;
}

// box maps of all scales in one launch; with `sampler` the polyline sampler rides in the same launch (splat_multi_sampler_kernel)
int draw_multiscale_impl(float* const* heatmaps, const int* heights, const int* widths, const float* strides, int num_scales,
                         int batch, const float* centers_xy, const float* boxes_xyxy, const void* counts, int max_num_targets,
                         float diameter_to_sigma_factor, float k_scale, unsigned flags, const WaveSamplerParams* sampler,
                         hipStream_t stream)
{
    (void)take_launch_events();   // a pending accv_draw_heatmap_time_next_launch pair is dropped, not kept for a later call
    // the sampler's workgroups alone: whenever the box maps have nothing to launch
    auto sampler_only = [&]() -> int {
        if (!sampler) return ACCV_OK;
        TargetsParams tp{};
        tp.sp = *sampler;
        seal_tile_prefix(tp.mp);
        hipLaunchKernelGGL((splat_multi_sampler_kernel<true, kStorePlain>), dim3((unsigned)sampler->n_polylines), dim3(64), 0, stream, tp);
        note_dispatch("splat_multi_sampler_kernel", 4, 8, true, kStorePlain, dim3((unsigned)sampler->n_polylines), dim3(64));
        return accv::check_launch("draw_heatmap multi-scale splat + sampler kernel");
    };
    constexpr const char* who = "draw_heatmap_multiscale";
    if (int rc = check_scale_arrays(who, heatmaps, heights, widths, strides, num_scales)) return rc;
    if (int rc = check_scale_counts(who, batch, max_num_targets, "objects")) return rc;
    if (batch == 0) return sampler_only();
    if (!counts) return accv::fail(ACCV_EINVAL, "draw_heatmap_multiscale: counts pointer is null");
    if (max_num_targets > 0 && (!centers_xy || !boxes_xyxy))
        return accv::fail(ACCV_EINVAL, "draw_heatmap_multiscale: null object array");
    if ((reinterpret_cast<uintptr_t>(boxes_xyxy) & 15u) || (reinterpret_cast<uintptr_t>(centers_xy) & 7u))
        return accv::fail(ACCV_EINVAL, "draw_heatmap_multiscale: centres need 8-byte and boxes 16-byte alignment");
    const bool clear = (flags & ACCV_HM_CLEAR) != 0;
    if (max_num_targets == 0 && !clear) return sampler_only();

    SplatParams proto = multiscale_proto(counts, max_num_targets, diameter_to_sigma_factor, k_scale, flags);
    proto.centers_f = centers_xy;
    proto.boxes_f = boxes_xyxy;
    MultiParams mp{};
    const long long tiles = setup_scales(mp, proto, heatmaps, heights, widths, strides, num_scales, batch, 2 * kBoxTileR,
                                         flags, who, kPerScaleNote);
    if (tiles < 0) return (int)tiles;
    if (tiles == 0) return sampler_only();
    if (tiles + (sampler ? sampler->n_polylines : 0) > INT_MAX)
        return accv::fail(ACCV_EINVAL, "draw_heatmap_multiscale: %lld tiles exceed the grid limit", tiles);
    const int sm = multiscale_store_mode(flags);
    if (sampler) {
        TargetsParams tp{};
        tp.mp = mp;
        tp.sp = *sampler;
        const dim3 grid((unsigned)(tiles + sampler->n_polylines)), block(64);
        with_variant(clear, sm == kStoreWriteThrough, [&](auto CL, auto SM) {
            hipLaunchKernelGGL((splat_multi_sampler_kernel<CL, SM>), grid, block, 0, stream, tp);
        });
        note_dispatch("splat_multi_sampler_kernel", 4, 8, clear, sm, grid, block);
        return accv::check_launch("draw_heatmap multi-scale splat + sampler kernel");
    }
    const dim3 grid((unsigned)tiles), block(64);
    with_variant(clear, sm == kStoreWriteThrough, [&](auto CL, auto SM) {
        hipLaunchKernelGGL((splat_multi_kernel<CL, SM>), grid, block, 0, stream, mp);
    });
    note_dispatch("splat_multi_kernel", 4, 8, clear, sm, grid, block);
    return accv::check_launch("draw_heatmap multi-scale splat kernel");
}

}  // namespace

extern "C" {

int accv_draw_heatmap_multiscale_f32(float* const* heatmaps, const int* heights, const int* widths, const float* strides,
                                     int num_scales, int batch, const float* centers_xy, const float* boxes_xyxy,
                                     const void* counts, int max_num_targets, float diameter_to_sigma_factor,
                                     float k_scale, unsigned flags, void* stream_)
{
    return draw_multiscale_impl(heatmaps, heights, widths, strides, num_scales, batch, centers_xy, boxes_xyxy, counts,
                                max_num_targets, diameter_to_sigma_factor, k_scale, flags, nullptr, static_cast<hipStream_t>(stream_));
}

int accv_draw_heatmap_multiscale_sample_f32(float* const* heatmaps, const int* heights, const int* widths, const float* strides,
                                            int num_scales, int batch, const float* centers_xy, const float* boxes_xyxy,
                                            const void* counts, int max_num_targets, float diameter_to_sigma_factor,
                                            float k_scale, unsigned flags, const float* polylines_xy, int num_polylines,
                                            int points, const void* point_counts, int num_samples, float* samples,
                                            float* group_boxes, void* stream_)
{
    if (num_polylines < 0) return accv::fail(ACCV_EINVAL, "draw_heatmap_multiscale_sample: negative polyline count");
    if (points < 1 || points > 64)
        return accv::fail(ACCV_EINVAL, "draw_heatmap_multiscale_sample: 1..64 points per polyline (wave-level sampler), got %d",
                          points);
    if (num_samples < 64 || num_samples % 64 != 0 || num_samples > (1 << 20))
        return accv::fail(ACCV_EINVAL, "draw_heatmap_multiscale_sample: the number of samples must be a multiple of 64 up to 2^20 "
                                       "(one group box per 64 samples), got %d", num_samples);
    if (num_polylines > 0 && (!polylines_xy || !samples || !group_boxes))
        return accv::fail(ACCV_EINVAL, "draw_heatmap_multiscale_sample: null polylines / samples / group_boxes");
    if ((reinterpret_cast<uintptr_t>(polylines_xy) & 7u) || (reinterpret_cast<uintptr_t>(samples) & 7u) ||
        (reinterpret_cast<uintptr_t>(group_boxes) & 15u))
        return accv::fail(ACCV_EINVAL, "draw_heatmap_multiscale_sample: polylines / samples need 8-byte, group boxes 16-byte alignment");
    WaveSamplerParams sp{};
    sp.points = reinterpret_cast<const float2*>(polylines_xy);
    sp.point_counts = point_counts;
    sp.samples = reinterpret_cast<float2*>(samples);
    sp.boxes = reinterpret_cast<float4*>(group_boxes);
    sp.n_polylines = num_polylines;
    sp.P = points;
    sp.S = num_samples;
    sp.counts_i64 = (flags & ACCV_HM_POINT_COUNTS_I64) ? 1 : 0;
    return draw_multiscale_impl(heatmaps, heights, widths, strides, num_scales, batch, centers_xy, boxes_xyxy, counts,
                                max_num_targets, diameter_to_sigma_factor, k_scale, flags, num_polylines > 0 ? &sp : nullptr,
                                static_cast<hipStream_t>(stream_));
}

size_t accv_draw_points_workspace_bytes(int batch, int num_points)
{
    if (batch < 0 || num_points < 0) return 0;
    return (size_t)batch * (size_t)((num_points + 63) / 64) * sizeof(float4) + 16;
}

int accv_draw_points_multiscale_f32(float* const* heatmaps, const int* heights, const int* widths, const float* strides,
                                    int num_scales, int batch, const float* points_xy, const void* counts, int num_points,
                                    int radius, float diameter_to_sigma_factor, float k_scale, unsigned flags,
                                    void* workspace, size_t workspace_bytes, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    (void)take_launch_events();   // a pending accv_draw_heatmap_time_next_launch pair is dropped, not kept for a later call
    constexpr const char* who = "draw_points_multiscale";
    if (int rc = check_scale_arrays(who, heatmaps, heights, widths, strides, num_scales)) return rc;
    if (int rc = check_scale_counts(who, batch, num_points, "points")) return rc;
    if (batch == 0) return ACCV_OK;
    if (!counts) return accv::fail(ACCV_EINVAL, "draw_points_multiscale: counts pointer is null");
    if (num_points > 0 && !points_xy) return accv::fail(ACCV_EINVAL, "draw_points_multiscale: null point array");
    if (reinterpret_cast<uintptr_t>(points_xy) & 7u)
        return accv::fail(ACCV_EINVAL, "draw_points_multiscale: points need 8-byte alignment");
    const bool clear = (flags & ACCV_HM_CLEAR) != 0;
    if (num_points == 0 && !clear) return ACCV_OK;
    const size_t need = accv_draw_points_workspace_bytes(batch, num_points);
    if (!workspace || workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 15u))
        return accv::fail(ACCV_EWORKSPACE, "draw_points_multiscale: workspace needs %zu aligned bytes, got %zu", need,
                          workspace_bytes);
    const int n_groups = (num_points + 63) / 64;

    SplatParams proto = multiscale_proto(counts, num_points, diameter_to_sigma_factor, k_scale, flags);
    proto.centers_f = points_xy;
    proto.boxes_f = static_cast<const float*>(workspace);
    proto.radius = radius;
    proto.n_groups = n_groups;
    MultiParams mp{};
    const long long tiles = setup_scales(mp, proto, heatmaps, heights, widths, strides, num_scales, batch, kSmallTH,
                                         flags, who, kPerScaleNote);
    if (tiles <= 0) return (int)tiles;   // an error, or no map to draw
    if (tiles > INT_MAX) return accv::fail(ACCV_EINVAL, "draw_points_multiscale: %lld tiles exceed the grid limit", tiles);
    const long long total_groups = (long long)batch * n_groups;
    if (total_groups > INT_MAX) return accv::fail(ACCV_EINVAL, "draw_points_multiscale: too many point groups");
    if (total_groups > 0 && !(flags & ACCV_HM_GROUP_BOXES_GIVEN))
        hipLaunchKernelGGL(group_boxes_kernel, dim3((unsigned)total_groups), dim3(64), 0, stream,
                           reinterpret_cast<const float2*>(points_xy), num_points, n_groups, total_groups,
                           static_cast<float4*>(workspace));
    // a tile of a coarse scale is crossed by several lanes and has many sample groups to walk: share it among four waves
    // when some scale averages >= 24 samples per tile (config 3: 7.5 / 30 / 113 at strides 4 / 8 / 16); fine scales alone
    // keep one wave per tile (mostly empty tiles would only pay the barriers: 21.7 -> 23.8 us at stride 4)
    // Round 3: ... and only when those coarse tiles are at least half of the launch.  Next to a fine scale with several times
    // their tile count the coarse tiles' long chains run underneath the fine scale's stream either way, and one wave per tile
    // (9 KB of LDS, 17-20 tiles resident per CU instead of 8) is what the fine scale wants: config 3 (strides 4 / 8 / 16)
    // 32.9 -> 28.7 us, its empty-tile floor 21 -> 15 us (profiles/r03_lane_splat_modes_sweep4_tile_height.log)
    long long coarse_tiles = 0;
    for (int i = 0; i < mp.n_scales; ++i)
        if ((double)batch * num_points >= 24.0 * (double)mp.scale[i].n_tiles) coarse_tiles += mp.scale[i].n_tiles;
    const bool heavy = 2 * coarse_tiles >= tiles;
    const int sm = multiscale_store_mode(flags);
    const dim3 grid((unsigned)tiles), block(heavy ? 256 : 64);
    with_variant(clear, sm == kStoreWriteThrough, [&](auto CL, auto SM) {
        if (heavy)
            hipLaunchKernelGGL((splat_points_multi_kernel<CL, SM, 4>), grid, block, 0, stream, mp);
        else
            hipLaunchKernelGGL((splat_points_multi_kernel<CL, SM, 1>), grid, block, 0, stream, mp);
    });
    note_dispatch("splat_points_multi_kernel", 4, 8, clear, sm, grid, block);
    return accv::check_launch("draw_heatmap multi-scale point splat kernel");
}

int accv_draw_polylines_fused_applicable(const int* heights, const int* widths, int num_scales, int batch, int lanes,
                                         int points, int num_samples)
{
    if (!heights || !widths || num_scales < 1 || num_scales > kMaxScales) return 0;
    return fused_lane_shape(heights, widths, num_scales, batch, lanes, points, num_samples).ok ? 1 : 0;
}

int accv_draw_polylines_multiscale_f32(float* const* heatmaps, const int* heights, const int* widths, const float* strides,
                                       int num_scales, int batch, const float* polylines_xy, int lanes, int points,
                                       const void* point_counts, const void* lane_counts, int num_samples, int radius,
                                       float diameter_to_sigma_factor, float k_scale, unsigned flags, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    constexpr const char* who = "draw_polylines_multiscale";
    if (int rc = check_scale_arrays(who, heatmaps, heights, widths, strides, num_scales)) return rc;
    if (batch < 0) return accv::fail(ACCV_EINVAL, "draw_polylines_multiscale: negative batch");
    if (batch == 0) return ACCV_OK;
    if (radius < 0) return accv::fail(ACCV_EINVAL, "draw_polylines_multiscale: negative radius");
    const FusedLaneShape shape = fused_lane_shape(heights, widths, num_scales, batch, lanes, points, num_samples);
    if (!shape.ok)
        return accv::fail(ACCV_EINVAL, "draw_polylines_multiscale: shape outside the fused kernel (1..64 points per polyline, "
                                       "lanes x points rounded up to a power of two <= %d, samples <= (points - 1) x that power "
                                       "of two / 2, fine scales in the majority: accv_draw_polylines_fused_applicable); use "
                                       "accv_polyline_sample_boxes + accv_draw_points_multiscale_f32", kLaneRounds * 64);
    if (!polylines_xy || !lane_counts)
        return accv::fail(ACCV_EINVAL, "draw_polylines_multiscale: null polylines / lane_counts");
    if (reinterpret_cast<uintptr_t>(polylines_xy) & 7u)
        return accv::fail(ACCV_EINVAL, "draw_polylines_multiscale: polylines need 8-byte alignment");
    const bool clear = (flags & ACCV_HM_CLEAR) != 0;

    SplatParams proto = multiscale_proto(lane_counts, lanes, diameter_to_sigma_factor, k_scale, flags);
    proto.radius = radius;
    FusedLaneParams fp{};
    const long long tiles = setup_scales(fp.mp, proto, heatmaps, heights, widths, strides, num_scales, batch, kSmallTH,
                                         flags, who, "");
    if (tiles <= 0) return (int)tiles;   // an error, or no map to draw
    if (tiles > INT_MAX) return accv::fail(ACCV_EINVAL, "draw_polylines_multiscale: %lld tiles exceed the grid limit", tiles);
    fp.lp.points = reinterpret_cast<const float2*>(polylines_xy);
    fp.lp.point_counts = point_counts;
    fp.lp.L = lanes;
    fp.lp.P = points;
    fp.lp.S = num_samples;
    fp.lp.p2_shift = shape.p2_shift;
    fp.lp.counts_i64 = (flags & ACCV_HM_POINT_COUNTS_I64) ? 1 : 0;
    const int sm = multiscale_store_mode(flags);
    const dim3 grid((unsigned)tiles), block(64);
    with_variant(clear, sm == kStoreWriteThrough, [&](auto CL, auto SM) {
        hipLaunchKernelGGL((lane_raster_multi_kernel<CL, SM>), grid, block, 0, stream, fp);
    });
    note_dispatch("lane_raster_multi_kernel", 4, 8, clear, sm, grid, block);
    return accv::check_launch("draw_heatmap fused lane raster kernel");
}

int accv_heatmap_targets_from_boxes_f32(const float* centers_xy, const float* boxes_xyxy, long long num_objects,
                                        float stride, int32_t* out_centers, int32_t* out_radii, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (num_objects < 0) return accv::fail(ACCV_EINVAL, "targets_from_boxes: negative count");
    if (num_objects == 0) return ACCV_OK;
    if (!centers_xy || !boxes_xyxy || !out_centers || !out_radii)
        return accv::fail(ACCV_EINVAL, "targets_from_boxes: null pointer");
    if ((reinterpret_cast<uintptr_t>(boxes_xyxy) & 15u) || (reinterpret_cast<uintptr_t>(centers_xy) & 7u) ||
        (reinterpret_cast<uintptr_t>(out_centers) & 7u))
        return accv::fail(ACCV_EINVAL, "targets_from_boxes: centres need 8-byte and boxes 16-byte alignment");
    const unsigned grid = (unsigned)std::min<long long>((num_objects + 255) / 256, 4096);
    hipLaunchKernelGGL(targets_from_boxes_kernel, dim3(grid), dim3(256), 0, stream,
                       reinterpret_cast<const float2*>(centers_xy), reinterpret_cast<const float4*>(boxes_xyxy),
                       num_objects, stride, reinterpret_cast<int2*>(out_centers), out_radii);
    return accv::check_launch("targets_from_boxes");
}

int accv_heatmap_targets_from_points_f32(const float* points_xy, long long num_points, float stride, int radius,
                                         int32_t* out_centers, int32_t* out_radii, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (num_points < 0) return accv::fail(ACCV_EINVAL, "targets_from_points: negative count");
    if (num_points == 0) return ACCV_OK;
    if (!points_xy || !out_centers || !out_radii) return accv::fail(ACCV_EINVAL, "targets_from_points: null pointer");
    if ((reinterpret_cast<uintptr_t>(points_xy) & 7u) || (reinterpret_cast<uintptr_t>(out_centers) & 7u))
        return accv::fail(ACCV_EINVAL, "targets_from_points: points and centres need 8-byte alignment");
    const unsigned grid = (unsigned)std::min<long long>((num_points + 255) / 256, 4096);
    hipLaunchKernelGGL(targets_from_points_kernel, dim3(grid), dim3(256), 0, stream,
                       reinterpret_cast<const float2*>(points_xy), num_points, stride, radius,
                       reinterpret_cast<int2*>(out_centers), out_radii);
    return accv::check_launch("targets_from_points");
}

int accv_fill_f32(float* dst, size_t count, float value, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (count == 0) return ACCV_OK;
    if (!dst) return accv::fail(ACCV_EINVAL, "fill: null pointer");
    size_t head = 0;
    while (((reinterpret_cast<uintptr_t>(dst + head)) & 15u) && head < count) ++head;
    if (head) hipLaunchKernelGGL(fill_tail_kernel, dim3(1), dim3(64), 0, stream, dst, head, value);
    const size_t n4 = (count - head) / 4;
    for (size_t done = 0; done < n4;) {  // one launch unless the buffer has more than 2^31 * 256 vectors
        const size_t part = std::min(n4 - done, (size_t)0x7fffffff * 256);
        hipLaunchKernelGGL(fill_kernel, dim3((unsigned)((part + 255) / 256)), dim3(256), 0, stream,
                           reinterpret_cast<float4*>(dst + head) + done, part, value);
        done += part;
    }
    const size_t tail = count - head - n4 * 4;
    if (tail) hipLaunchKernelGGL(fill_tail_kernel, dim3(1), dim3(64), 0, stream, dst + head + n4 * 4, tail, value);
    return accv::check_launch("fill");
}

}  // extern "C"
