// Fused box-to-heat-map targets for a ragged batch of 2D boxes: the reference's BoundingBoxToHeatmapConverter step
// (dali_pipeline_framework processing_steps/bounding_box_to_heatmap_converter.py; rasteriser ext_impl/DrawGaussians.cc:32-76)
// in ONE launch: scaling to the map, clipping, the active decision, the per-object side outputs and the Gaussian maps.
// Per-object arithmetic: box_heatmap_arith.h.
//
// One workgroup of kThreads = kMaxBoxes lanes per (frame, plane, tile of kTileW x kTileH pixels), a lane per box slot:
//   1. every lane computes the record of its slot from the raw inputs.  The arithmetic is deterministic float32, so every
//      workgroup of a frame derives the same records: no pre-pass, no global scratch, no second launch;
//   2. the workgroup of tile 0 of plane 0 stores the per-object outputs of its frame, padding slots as 0;
//   3. a lane whose object is active, belongs to the plane and whose patch [c - R, c + R] meets the tile is a hit; the hits
//      are compacted into LDS (__ballot + popcount, the waves' totals behind one barrier) as (cx, cy, R, exponent factor);
//   4. every lane owns 4 consecutive pixels of one tile row and takes the maximum over the hits in registers, starting
//      from 0; a hit whose rows do not reach the lane's row costs one LDS read and one compare;
//   5. one 16-byte store per lane when the map's width is a multiple of 4 and its base is 16-byte aligned, else up to four
//      4-byte stores with a bound check each.  Every pixel of the map is stored exactly once; nothing is read or cleared.
// No atomics on global memory, no memset, no host synchronisation; the maximum does not depend on the order of the hits, so
// the map is bitwise reproducible.  All global indices are 64-bit.
//
// The exponent is taken per pixel: k * __expf(-(dx^2 + dy^2) * factor), one v_exp_f32 per pixel and hit inside the patch.
// The separable form (a row factor times a column factor from LDS tables, as the headline rasteriser has it) was NOT built,
// because the exponent is not where the time goes.  Measured at 64 frames x 10 planes x 270 x 480 with 3159 active objects
// (332 MB of map; two alternated runs each): 0.112 ms per call as it stands (profiles/box_heatmap_bench.log), 0.111 ms with
// the __expf replaced by a multiply, 0.111 ms with every object invalid (nothing drawn), and 0.046 ms for torch's zero_() of
// the same map.  So the drawing costs about 1 % and the call takes 2.4 fill times: what bounds it is the start of each
// workgroup (counts, inputs, records, two barriers) in front of 4 KiB of stores.  Several tiles per workgroup is the open
// lever; it is not done here.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "accv_common.h"
#include "accv_numeric.h"
#include "box_heatmap_arith.h"

namespace {

using namespace accv_bh;
using accv::clamp_count;
using accv::load_index;

constexpr int kWave = 64;
constexpr int kThreads = kMaxBoxes;                 // a lane per box slot
constexpr int kWaves = kThreads / kWave;
constexpr int kTileW = ACCV_BH_TILE_W, kTileH = ACCV_BH_TILE_H;
constexpr int kLanePixels = 4;                      // consecutive pixels of a row per lane: one 16-byte store
constexpr int kLanesPerRow = kTileW / kLanePixels;
constexpr unsigned kKnownFlags = ACCV_BH_COUNTS_I64 | ACCV_BH_HW_I64 | ACCV_BH_CATEGORIES_I64;
constexpr double kMaxRadius = 16384.0;              // dx^2 + dy^2 of a patch pixel stays below 2^31

static_assert(kMaxBoxes == ACCV_BH_MAX_BOXES && kMaxCategories == ACCV_BH_MAX_CATEGORIES,
              "box_heatmap_arith.h and accv_hip.h disagree");
static_assert(kLanesPerRow * kTileH == kThreads, "a lane per 4 pixels of the tile");

struct Args {
    const float* boxes;             // [B, G, 4]
    const float* centers;           // [B, G, 2] or null
    const void* categories;         // [B, G] or null
    const unsigned char* valid;     // [B, G] or null
    const void* counts;             // [B]
    const void* image_hw;           // [B, 2] or null
    float* map;                     // [B, planes, Hm, Wm]
    unsigned char* active;          // [B, G]
    int* center;                    // [B, G, 2]
    float* offset;                  // [B, G, 2]
    float* hw;                      // [B, G, 2]
    float* boxes_out;               // [B, G, 4]
    float* radii;                   // [B, G]
    long long B, G, Hi, Wi;
    int Hm, Wm, planes, tiles_x, tiles_y;
    int counts64, hw64, cats64;
    int num_categories;             // 0: categories are not used
    int plane_by_category, size_mode /* 0 none, 1 global, 2 per category */, vec4;
    Consts k;
    float min_sizes[kMaxCategories][2];   // (h, w) per category, size_mode 2
    float k_for_planes[kMaxCategories];
};

struct __attribute__((aligned(16))) Hit {
    int cx, cy, R;
    float factor;
};

__host__ __device__ inline Frame frame_of(const Args& a, long long b)
{
    long long H = a.Hi, W = a.Wi;
    if (a.image_hw) H = load_index(a.image_hw, 2 * b, a.hw64), W = load_index(a.image_hw, 2 * b + 1, a.hw64);
    return frame_consts(a.Wm, a.Hm, clamp_extent(W), clamp_extent(H));
}

// the record of slot s = b * G + i (a real one), whether it is active, and its category (0 without categories)
__host__ __device__ inline Record slot_record(const Args& a, const Frame& f, long long s, bool& active, long long& category)
{
    const float* p = a.boxes + s * 4;
    float g0 = 0.0f, g1 = 0.0f;
    if (a.centers) g0 = a.centers[s * 2], g1 = a.centers[s * 2 + 1];
    const Record r = object_record(p[0], p[1], p[2], p[3], a.centers != nullptr, g0, g1, f, a.k);
    bool in_class = true;
    category = 0;
    if (a.num_categories > 0) {
        category = load_index(a.categories, s, a.cats64);
        in_class = category >= 0 && category < a.num_categories;
    }
    float min_h = a.k.min_h, min_w = a.k.min_w;
    if (a.size_mode == 2 && in_class) min_h = a.min_sizes[category][0], min_w = a.min_sizes[category][1];
    active = passes(r, a.k, a.size_mode != 0, min_h, min_w) && in_class && (!a.valid || a.valid[s] != 0);
    return r;
}

// the per-object outputs of slot s; a padding slot passes zero_record() and false
__host__ __device__ inline void store_record(const Args& a, long long s, const Record& r, bool active)
{
    a.active[s] = active ? 1 : 0;
    a.center[s * 2] = r.ix, a.center[s * 2 + 1] = r.iy;
    a.offset[s * 2] = r.ox, a.offset[s * 2 + 1] = r.oy;
    a.hw[s * 2] = r.h, a.hw[s * 2 + 1] = r.w;
    a.boxes_out[s * 4] = r.box[0], a.boxes_out[s * 4 + 1] = r.box[1];
    a.boxes_out[s * 4 + 2] = r.box[2], a.boxes_out[s * 4 + 3] = r.box[3];
    a.radii[s] = r.radius;
}

// ------------------------------------------------------------------------------------------------------------- device
__global__ __launch_bounds__(kThreads) void box_heatmap_kernel(const Args a)
{
    __shared__ Hit s_hit[kMaxBoxes];
    __shared__ int s_cnt[kWaves];

    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    unsigned wg = blockIdx.x;                     // ((b * planes + plane) * tiles_y + ty) * tiles_x + tx
    const int tx = (int)(wg % (unsigned)a.tiles_x);
    wg /= (unsigned)a.tiles_x;
    const int ty = (int)(wg % (unsigned)a.tiles_y);
    wg /= (unsigned)a.tiles_y;
    const int plane = (int)(wg % (unsigned)a.planes);
    const long long b = wg / (unsigned)a.planes;

    const int n = (int)clamp_count(a.counts, b, a.G, a.counts64);
    const Frame f = frame_of(a, b);
    const long long s = b * a.G + tid;
    Record r = zero_record();
    bool active = false;
    long long category = 0;
    if (tid < n) r = slot_record(a, f, s, active, category);
    if (tx == 0 && ty == 0 && plane == 0 && tid < a.G) store_record(a, s, r, active);

    const int x0 = tx * kTileW, y0 = ty * kTileH;
    const int R = patch_radius(r.radius);
    const bool hit = active && (!a.plane_by_category || category == plane) && r.ix + R >= x0 && r.ix - R < x0 + kTileW &&
                     r.iy + R >= y0 && r.iy - R < y0 + kTileH;
    const unsigned long long bal = __ballot(hit);
    if (lane == 0) s_cnt[wave] = __popcll(bal);
    __syncthreads();
    int pos = __popcll(bal & ((1ull << lane) - 1ull)), total = 0;
#pragma unroll
    for (int v = 0; v < kWaves; ++v) {
        const int c = s_cnt[v];
        total += c;
        if (v < wave) pos += c;
    }
    if (hit) s_hit[pos] = Hit{r.ix, r.iy, R, exponent_factor(r.radius, a.k.rsf)};   // pos < kMaxBoxes
    __syncthreads();

    const int y = y0 + tid / kLanesPerRow, x = x0 + (tid % kLanesPerRow) * kLanePixels;
    const float kc = a.k_for_planes[plane];
    float acc[kLanePixels] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int h = 0; h < total; ++h) {
        const Hit q = s_hit[h];
        const int dy = y - q.cy;
        if (dy < -q.R || dy > q.R) continue;
        const int dy2 = dy * dy;
#pragma unroll
        for (int j = 0; j < kLanePixels; ++j) {
            const int dx = x + j - q.cx;
            if (dx >= -q.R && dx <= q.R) acc[j] = fmaxf(acc[j], kc * __expf(-(float)(dx * dx + dy2) * q.factor));
        }
    }
    if (y >= a.Hm || x >= a.Wm) return;
    float* p = a.map + (((b * a.planes + plane) * a.Hm + y) * (long long)a.Wm + x);
    if (a.vec4) {   // Wm % 4 == 0: x + 3 < Wm, and p is 16-byte aligned
        *reinterpret_cast<float4*>(p) = make_float4(acc[0], acc[1], acc[2], acc[3]);
    } else {
#pragma unroll
        for (int j = 0; j < kLanePixels; ++j)
            if (x + j < a.Wm) p[j] = acc[j];
    }
}

// --------------------------------------------------------------------------------------------------------------- host
// the same records, one frame after the other; the map is cleared and painted object by object
void host_run(const Args& a)
{
    const long long plane_px = (long long)a.Hm * a.Wm;
    for (long long b = 0; b < a.B; ++b) {
        const int n = (int)clamp_count(a.counts, b, a.G, a.counts64);
        const Frame f = frame_of(a, b);
        float* maps = a.map + b * a.planes * plane_px;
        for (long long i = 0; i < a.planes * plane_px; ++i) maps[i] = 0.0f;
        for (long long i = 0; i < a.G; ++i) {
            const long long s = b * a.G + i;
            Record r = zero_record();
            bool active = false;
            long long category = 0;
            if (i < n) r = slot_record(a, f, s, active, category);
            store_record(a, s, r, active);
            if (!active) continue;
            const int plane = a.plane_by_category ? (int)category : 0;
            const int R = patch_radius(r.radius);
            const float factor = exponent_factor(r.radius, a.k.rsf), kc = a.k_for_planes[plane];
            float* m = maps + plane * plane_px;
            const int ya = r.iy - R < 0 ? 0 : r.iy - R, yb = r.iy + R > a.Hm - 1 ? a.Hm - 1 : r.iy + R;
            const int xa = r.ix - R < 0 ? 0 : r.ix - R, xb = r.ix + R > a.Wm - 1 ? a.Wm - 1 : r.ix + R;
            for (int y = ya; y <= yb; ++y) {
                const int dy2 = (y - r.iy) * (y - r.iy);
                for (int x = xa; x <= xb; ++x) {
                    const int dx = x - r.ix;
                    const float v = kc * std::exp(-(float)(dx * dx + dy2) * factor);
                    float& px = m[(long long)y * a.Wm + x];
                    if (v > px) px = v;
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------- checks
// ACCV_OK with *empty = 1 when there is nothing to write; every check runs before anything else reads the arguments
int check_args(const char* who, const float* boxes, const float* centers, const void* categories, const unsigned char* is_valid,
               const void* counts, const void* image_hw, unsigned flags, long long B, long long G,
               const accv_box_heatmap_params* p, float* heatmap, unsigned char* is_active, int* center, float* center_offset,
               float* height_width, float* bboxes_heatmap, float* radii, Args& a, int* empty)
{
    *empty = 0;
    if (!p) return accv::fail(ACCV_EINVAL, "%s: null params", who);
    if (B < 0 || G < 0) return accv::fail(ACCV_EINVAL, "%s: negative size", who);
    if (flags & ~kKnownFlags) return accv::fail(ACCV_EINVAL, "%s: unknown flags 0x%x", who, flags);
    if (G > kMaxBoxes) return accv::fail(ACCV_EINVAL, "%s: %lld box slots per frame, at most %d supported", who, G, kMaxBoxes);
    if (p->num_categories < 0 || p->num_categories > kMaxCategories)
        return accv::fail(ACCV_EINVAL, "%s: %d categories, 0 (not used) to %d supported", who, p->num_categories, kMaxCategories);
    if (p->has_min_object_size && p->has_per_category_min_object_sizes)
        return accv::fail(ACCV_EINVAL, "%s: min_object_size and per_category_min_object_sizes exclude each other", who);
    if ((p->per_category_heatmap || p->has_per_category_min_object_sizes) && p->num_categories < 1)
        return accv::fail(ACCV_EINVAL, "%s: per-category maps and per-category minimum sizes need num_categories >= 1", who);
    if (p->map_h < 1 || p->map_w < 1 || p->map_h > kMaxExtent || p->map_w > kMaxExtent)
        return accv::fail(ACCV_EINVAL, "%s: map of %lld x %lld, each extent must be in [1, 2^24]", who, p->map_h, p->map_w);
    const double scalars[5] = {p->min_fraction_area_clipping, p->min_radius, p->max_radius, p->radius_scaling_factor,
                               p->radius_to_sigma_factor};
    for (double v : scalars)
        if (!std::isfinite(v)) return accv::fail(ACCV_EINVAL, "%s: a scalar parameter is not finite", who);
    if (!(p->max_radius > 0.0 && p->max_radius <= kMaxRadius))
        return accv::fail(ACCV_EINVAL, "%s: max_radius %g outside (0, %g]", who, p->max_radius, kMaxRadius);
    if (!((float)p->radius_to_sigma_factor > 0.0f))
        return accv::fail(ACCV_EINVAL, "%s: radius_to_sigma_factor %g is not positive", who, p->radius_to_sigma_factor);
    const int planes = p->per_category_heatmap ? p->num_categories : 1;
    for (int c = 0; c < planes; ++c)
        if (!std::isfinite(p->k_for_classes[c])) return accv::fail(ACCV_EINVAL, "%s: k_for_classes[%d] is not finite", who, c);
    if (B == 0) {
        *empty = 1;
        return ACCV_OK;
    }
    if (!heatmap || !counts) return accv::fail(ACCV_EINVAL, "%s: null heatmap / counts pointer", who);
    if (G > 0 && (!boxes || !is_active || !center || !center_offset || !height_width || !bboxes_heatmap || !radii))
        return accv::fail(ACCV_EINVAL, "%s: null boxes / per-object output pointer", who);
    if (G > 0 && p->num_categories > 0 && !categories)
        return accv::fail(ACCV_EINVAL, "%s: num_categories is set but categories is null", who);
    if ((reinterpret_cast<uintptr_t>(boxes) | reinterpret_cast<uintptr_t>(centers) | reinterpret_cast<uintptr_t>(heatmap) |
         reinterpret_cast<uintptr_t>(center) | reinterpret_cast<uintptr_t>(center_offset) |
         reinterpret_cast<uintptr_t>(height_width) | reinterpret_cast<uintptr_t>(bboxes_heatmap) |
         reinterpret_cast<uintptr_t>(radii)) & 3u)
        return accv::fail(ACCV_EINVAL, "%s: a float / int32 pointer is not aligned to its element size", who);
    if ((reinterpret_cast<uintptr_t>(counts) & ((flags & ACCV_BH_COUNTS_I64) ? 7u : 3u)) ||
        (reinterpret_cast<uintptr_t>(image_hw) & ((flags & ACCV_BH_HW_I64) ? 7u : 3u)) ||
        (reinterpret_cast<uintptr_t>(categories) & ((flags & ACCV_BH_CATEGORIES_I64) ? 7u : 3u)))
        return accv::fail(ACCV_EINVAL, "%s: counts / image_hw / categories are not aligned to their element size", who);
    const long long tiles_x = (p->map_w + kTileW - 1) / kTileW, tiles_y = (p->map_h + kTileH - 1) / kTileH;
    if (tiles_x * tiles_y > accv::kGridLimit || tiles_x * tiles_y * planes > accv::kGridLimit ||
        B > accv::kGridLimit / (tiles_x * tiles_y * planes))
        return accv::fail(ACCV_EINVAL, "%s: %lld frames x %d planes x %lld tiles exceed the grid limit", who, B, planes,
                          tiles_x * tiles_y);
    a.boxes = boxes, a.centers = centers, a.categories = categories, a.valid = is_valid, a.counts = counts, a.image_hw = image_hw;
    a.map = heatmap, a.active = is_active, a.center = center, a.offset = center_offset, a.hw = height_width;
    a.boxes_out = bboxes_heatmap, a.radii = radii;
    a.B = B, a.G = G, a.Hi = p->image_h, a.Wi = p->image_w;
    a.Hm = (int)p->map_h, a.Wm = (int)p->map_w, a.planes = planes, a.tiles_x = (int)tiles_x, a.tiles_y = (int)tiles_y;
    a.counts64 = (flags & ACCV_BH_COUNTS_I64) ? 1 : 0, a.hw64 = (flags & ACCV_BH_HW_I64) ? 1 : 0;
    a.cats64 = (flags & ACCV_BH_CATEGORIES_I64) ? 1 : 0;
    a.num_categories = p->num_categories;
    a.plane_by_category = p->per_category_heatmap ? 1 : 0;
    a.size_mode = p->has_per_category_min_object_sizes ? 2 : (p->has_min_object_size ? 1 : 0);
    a.vec4 = (p->map_w % 4 == 0 && (reinterpret_cast<uintptr_t>(heatmap) & 15u) == 0) ? 1 : 0;
    const float min_radius = (float)p->min_radius;
    a.k.thr = (float)p->min_fraction_area_clipping;
    a.k.rs = (float)p->radius_scaling_factor;
    a.k.rlo = min_radius > 0.5f ? min_radius : 0.5f;
    a.k.rhi = (float)p->max_radius;
    a.k.rsf = (float)p->radius_to_sigma_factor;
    a.k.min_h = (float)p->min_object_size[0], a.k.min_w = (float)p->min_object_size[1];
    for (int c = 0; c < kMaxCategories; ++c) {
        a.min_sizes[c][0] = p->per_category_min_object_sizes[c][0], a.min_sizes[c][1] = p->per_category_min_object_sizes[c][1];
        a.k_for_planes[c] = p->k_for_classes[c];
    }
    return ACCV_OK;
}

}  // namespace

extern "C" {

int accv_box_heatmap(const float* boxes, const float* centers, const void* categories, const unsigned char* is_valid,
                     const void* counts, const void* image_hw, unsigned flags, long long B, long long G,
                     const accv_box_heatmap_params* params, float* heatmap, unsigned char* is_active, int* center,
                     float* center_offset, float* height_width, float* bboxes_heatmap, float* radii, void* stream)
{
    const char* who = "boxes_to_heatmap";
    Args a;
    int empty;
    if (int rc = check_args(who, boxes, centers, categories, is_valid, counts, image_hw, flags, B, G, params, heatmap, is_active,
                            center, center_offset, height_width, bboxes_heatmap, radii, a, &empty))
        return rc;
    if (empty) return ACCV_OK;
    const long long groups = a.B * a.planes * a.tiles_y * a.tiles_x;
    hipLaunchKernelGGL(box_heatmap_kernel, dim3((unsigned)groups), dim3(kThreads), 0, static_cast<hipStream_t>(stream), a);
    return accv::check_launch(who);
}

int accv_box_heatmap_host(const float* boxes, const float* centers, const void* categories, const unsigned char* is_valid,
                          const void* counts, const void* image_hw, unsigned flags, long long B, long long G,
                          const accv_box_heatmap_params* params, float* heatmap, unsigned char* is_active, int* center,
                          float* center_offset, float* height_width, float* bboxes_heatmap, float* radii)
{
    const char* who = "boxes_to_heatmap (host)";
    Args a;
    int empty;
    if (int rc = check_args(who, boxes, centers, categories, is_valid, counts, image_hw, flags, B, G, params, heatmap, is_active,
                            center, center_offset, height_width, bboxes_heatmap, radii, a, &empty))
        return rc;
    if (empty) return ACCV_OK;
    host_run(a);
    return ACCV_OK;
}

}  // extern "C"
