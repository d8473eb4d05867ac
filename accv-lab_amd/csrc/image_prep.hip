// Fused camera-image preparation: the image side of the reference's camera pipeline (dali_pipeline_framework
// processing_steps/affine_transformer.py -> fn.warp_affine, photo_metric_distorter.py, image_to_tile_size_padder.py,
// image_mean_std_dev_normalizer.py / image_range_0_1_normalizer.py; wired up in examples/pipeline_setup/
// stream_petr_pipeline.py) in ONE launch: uint8 HWC source -> warped, colour-augmented, normalised, tile-padded float tensor.
// Per-pixel arithmetic: image_prep_arith.h.
//
// One workgroup of kThreads lanes per (image, tile of kTileW x kTileH output pixels), padding included; a lane owns 4
// consecutive output x of one row:
//   1. the image's matrix, colour row and valid extent are read once per workgroup (the addresses depend on the workgroup
//      alone) and the matrix is inverted in place of a pre-pass;
//   2. per pixel: the sample position, up to four neighbours straight from global memory (the gather path: any matrix; the
//      two neighbours of a source row are six contiguous bytes, read as 4 + 2), the blend, the colour chain, scale and bias;
//      a pixel of the padding takes the pad value; without a matrix a lane reads its four pixels as 12 contiguous bytes;
//   3. stores: CHW three row stores of 4 values, HWC 12 contiguous values; 16 bytes each for float32, 8 bytes for f16 / bf16,
//      when the padded width is a multiple of 4 and the base is aligned to the store; else one store per element with a
//      bound check each.
// Every output element is stored exactly once and nothing is read from the output; no clear, no workspace, no atomics, no
// host synchronisation; bitwise reproducible.  All global indices are 64-bit.
//
// The kernel and the host loop are templated on the source kind: Args, the interleaved RGB batch above, or Nv12Args, the two
// planes of NV12 decoder surfaces addressed by byte strides (accv_prepare_images_nv12).  The NV12 kind converts every source
// tap to the uint8 triple accv_nv12_to_rgb would have written (nv12_arith.h) and is the same code from there on, so it equals
// conversion + accv_prepare_images bit for bit; the two taps of a source row share one chroma pair when x0 is even (two
// adjacent pairs, 4 contiguous bytes, when it is odd), the two rows of a footprint share a chroma row when y0 is even, and
// without a matrix a lane reads 4 luma bytes and the 4 bytes of its two chroma pairs.  DESIGN.md §9z.
//
// One kernel path.  A staged variant for axis-aligned matrices (source rows through LDS) was not built: DESIGN.md §9w has the
// measurements of what bounds this one.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <type_traits>

#include "accv_common.h"
#include "accv_numeric.h"
#include "image_prep_arith.h"

namespace {

using namespace accv_ip;
using accv::kBF16;
using accv::kF16;
using accv::kF32;
using accv::load_index;

constexpr int kTileW = ACCV_IP_TILE_W, kTileH = ACCV_IP_TILE_H;
constexpr int kLanePixels = 4;                      // consecutive pixels of a row per lane
constexpr int kLanesPerRow = kTileW / kLanePixels;
constexpr int kThreads = kLanesPerRow * kTileH;

static_assert(kMaxExtent == ACCV_IP_MAX_EXTENT, "image_prep_arith.h and accv_hip.h disagree");
static_assert(kThreads == 256, "four waves per workgroup");

struct Args {
    const unsigned char* images;    // [B, Hs, Ws, 3]
    const void* source_hw;          // [B, 2] or null
    const float* transforms;        // [B, 2, 3] or null
    const float* photometric;       // [B, 6] or null
    void* out;                      // [B, 3, Hp, Wp] or [B, Hp, Wp, 3]
    float* coords;                  // host entry only: [B, Ho, Wo, 4] or null
    long long B;
    int Hs, Ws, Ho, Wo, Hp, Wp, tiles_x, tiles_y;
    int hw64, vec;
    Norm n;
};

// the NV12 source kind: `images` is the Y plane, the planes are addressed by byte strides
struct Nv12Args : Args {
    const unsigned char* uv;
    long long y_batch, y_row, uv_batch, uv_row;
    accv_nv12::Format f;
};

// everything a pixel of image b needs
struct Image {
    const unsigned char* px;
    int Wv, Hv;
    Warp w;
    Colour k;
};

struct Nv12Image : Image {
    Nv12Source src;
};

__host__ __device__ inline Image image_of(const Args& a, long long b)
{
    Image im;
    im.px = a.images + b * a.Hs * (long long)a.Ws * 3;
    long long H = a.Hs, W = a.Ws;
    if (a.source_hw) H = load_index(a.source_hw, 2 * b, a.hw64), W = load_index(a.source_hw, 2 * b + 1, a.hw64);
    im.Hv = (int)(H < 0 ? 0 : (H > a.Hs ? a.Hs : H));
    im.Wv = (int)(W < 0 ? 0 : (W > a.Ws ? a.Ws : W));
    im.w = load_warp(a.transforms ? a.transforms + b * 6 : nullptr);
    im.k = load_colour(a.photometric ? a.photometric + b * 6 : nullptr);
    return im;
}

// the same per-image parameters; the planes of image b in place of its pixels
__host__ __device__ inline Nv12Image image_of(const Nv12Args& a, long long b)
{
    Nv12Image im;
    static_cast<Image&>(im) = image_of(static_cast<const Args&>(a), b);
    im.px = nullptr;
    im.src.y = a.images + b * a.y_batch, im.src.uv = a.uv + b * a.uv_batch;
    im.src.y_pitch = a.y_row, im.src.uv_pitch = a.uv_row;
    im.src.f = a.f;
    return im;
}

// the sampled value of either source kind
__host__ __device__ inline void sample_source(const Args& a, const Image& im, const Position& p, float (&val)[3])
{
    sample(im.px, a.Ws, im.w, p, im.Wv, im.Hv, val);
}

__host__ __device__ inline void sample_source(const Nv12Args&, const Nv12Image& im, const Position& p, float (&val)[3])
{
    sample(im.src, im.w, p, im.Wv, im.Hv, val);
}

// the three output channels of pixel (X, Y) of the padded output
template <class A, class I>
__host__ __device__ inline void output_pixel(const A& a, const I& im, int X, int Y, float (&o)[3], Position* where)
{
    if (X >= a.Wo || Y >= a.Ho) {
        o[0] = a.n.pad[0], o[1] = a.n.pad[1], o[2] = a.n.pad[2];
        return;
    }
    const Position p = sample_position(im.w, X, Y, im.Wv, im.Hv);
    if (where) *where = p;
    float val[3];
    sample_source(a, im, p, val);
    colour_chain(im.k, a.n, val, o);
}

template <int DT>
__host__ __device__ inline void store_one(void* out, long long off, float v)
{
    if constexpr (DT == kF32) static_cast<float*>(out)[off] = v;
    else if constexpr (DT == kF16) static_cast<uint16_t*>(out)[off] = accv::float_to_half_bits(v);
    else static_cast<uint16_t*>(out)[off] = accv::float_to_bf16_bits(v);
}

// four consecutive elements from `off` on in one store; the address is aligned to the store
template <int DT>
__device__ __forceinline__ void store_four(void* out, long long off, float v0, float v1, float v2, float v3)
{
    if constexpr (DT == kF32) {
        *reinterpret_cast<float4*>(static_cast<float*>(out) + off) = make_float4(v0, v1, v2, v3);
    } else if constexpr (DT == kF16) {
        const unsigned lo = (unsigned)accv::float_to_half_bits(v0) | ((unsigned)accv::float_to_half_bits(v1) << 16);
        const unsigned hi = (unsigned)accv::float_to_half_bits(v2) | ((unsigned)accv::float_to_half_bits(v3) << 16);
        *reinterpret_cast<uint2*>(static_cast<uint16_t*>(out) + off) = make_uint2(lo, hi);
    } else {
        const unsigned lo = (unsigned)accv::float_to_bf16_bits(v0) | ((unsigned)accv::float_to_bf16_bits(v1) << 16);
        const unsigned hi = (unsigned)accv::float_to_bf16_bits(v2) | ((unsigned)accv::float_to_bf16_bits(v3) << 16);
        *reinterpret_cast<uint2*>(static_cast<uint16_t*>(out) + off) = make_uint2(lo, hi);
    }
}

// ------------------------------------------------------------------------------------------------------------- device
// A: the source kind, Args (the interleaved RGB batch) or Nv12Args (the two planes)
template <int DT, bool HWC, class A>
__global__ __launch_bounds__(kThreads) void image_prep_gather_kernel(const A a)
{
    const int tid = threadIdx.x;
    unsigned wg = blockIdx.x;                     // (b * tiles_y + ty) * tiles_x + tx
    const int tx = (int)(wg % (unsigned)a.tiles_x);
    wg /= (unsigned)a.tiles_x;
    const int ty = (int)(wg % (unsigned)a.tiles_y);
    const long long b = wg / (unsigned)a.tiles_y;
    const int Y = ty * kTileH + tid / kLanesPerRow, X = tx * kTileW + (tid % kLanesPerRow) * kLanePixels;
    if (Y >= a.Hp || X >= a.Wp) return;

    const auto im = image_of(a, b);
    float o[kLanePixels][3];
    if (im.w.copy && Y < im.Hv && X + kLanePixels <= im.Wv) {
        if constexpr (std::is_same<A, Nv12Args>::value) {
            // without a matrix the lane's four pixels are 4 luma bytes and the 4 bytes of their two chroma pairs
            float val[kLanePixels][3];
            load_four(im.src, X, Y, val);
#pragma unroll
            for (int j = 0; j < kLanePixels; ++j) colour_chain(im.k, a.n, val[j], o[j]);
        } else {
            // without a matrix the lane's four pixels are 12 contiguous source bytes: three 4-byte reads (not aligned)
            uint32_t w[3];
            memcpy(w, im.px + ((long long)Y * a.Ws + X) * 3, 12);
#pragma unroll
            for (int j = 0; j < kLanePixels; ++j) {
                float val[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) val[c] = (float)((w[(j * 3 + c) / 4] >> (8 * ((j * 3 + c) % 4))) & 0xffu);
                colour_chain(im.k, a.n, val, o[j]);
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < kLanePixels; ++j) output_pixel(a, im, X + j, Y, o[j], nullptr);
    }

    if constexpr (HWC) {
        const long long off = ((b * a.Hp + Y) * (long long)a.Wp + X) * 3;
        if (a.vec) {   // Wp % 4 == 0: X + 3 < Wp, and 12 elements from an aligned address
            store_four<DT>(a.out, off, o[0][0], o[0][1], o[0][2], o[1][0]);
            store_four<DT>(a.out, off + 4, o[1][1], o[1][2], o[2][0], o[2][1]);
            store_four<DT>(a.out, off + 8, o[2][2], o[3][0], o[3][1], o[3][2]);
        } else {
#pragma unroll
            for (int j = 0; j < kLanePixels; ++j)
                if (X + j < a.Wp) {
                    store_one<DT>(a.out, off + j * 3, o[j][0]);
                    store_one<DT>(a.out, off + j * 3 + 1, o[j][1]);
                    store_one<DT>(a.out, off + j * 3 + 2, o[j][2]);
                }
        }
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const long long off = (((b * 3 + c) * a.Hp + Y) * (long long)a.Wp + X);
            if (a.vec) {
                store_four<DT>(a.out, off, o[0][c], o[1][c], o[2][c], o[3][c]);
            } else {
#pragma unroll
                for (int j = 0; j < kLanePixels; ++j)
                    if (X + j < a.Wp) store_one<DT>(a.out, off + j, o[j][c]);
            }
        }
    }
}

template <int DT, bool HWC, class A>
int launch(const A& a, hipStream_t stream)
{
    const long long groups = a.B * a.tiles_y * a.tiles_x;
    hipLaunchKernelGGL((image_prep_gather_kernel<DT, HWC, A>), dim3((unsigned)groups), dim3(kThreads), 0, stream, a);
    return accv::check_launch(std::is_same<A, Nv12Args>::value ? "prepare_images_nv12" : "prepare_images");
}

template <class A>
int launch_for(const A& a, int dtype, bool hwc, hipStream_t s)
{
    switch (dtype) {
    case kF32: return hwc ? launch<kF32, true>(a, s) : launch<kF32, false>(a, s);
    case kF16: return hwc ? launch<kF16, true>(a, s) : launch<kF16, false>(a, s);
    default: return hwc ? launch<kBF16, true>(a, s) : launch<kBF16, false>(a, s);
    }
}

// --------------------------------------------------------------------------------------------------------------- host
template <int DT, class A>
void host_run(const A& a, bool hwc)
{
    for (long long b = 0; b < a.B; ++b) {
        const auto im = image_of(a, b);
        for (int Y = 0; Y < a.Hp; ++Y)
            for (int X = 0; X < a.Wp; ++X) {
                float o[3];
                Position p;
                p.x0 = p.y0 = -2, p.wx = p.wy = 0.0f, p.inside = false;
                output_pixel(a, im, X, Y, o, &p);
                if (a.coords && X < a.Wo && Y < a.Ho) {
                    float* q = a.coords + ((b * a.Ho + Y) * (long long)a.Wo + X) * 4;
                    q[0] = (float)p.x0, q[1] = (float)p.y0, q[2] = p.wx, q[3] = p.wy;
                }
                for (int c = 0; c < 3; ++c) {
                    const long long off = hwc ? ((b * a.Hp + Y) * (long long)a.Wp + X) * 3 + c
                                              : ((b * 3 + c) * a.Hp + Y) * (long long)a.Wp + X;
                    store_one<DT>(a.out, off, o[c]);
                }
            }
    }
}

// ------------------------------------------------------------------------------------------------------------- checks
// ACCV_OK with *empty = 1 when there is nothing to write; every check runs before anything else reads the arguments
int check_args(const char* who, const unsigned char* images, const void* source_hw, const float* transforms,
               const float* photometric, const accv_prepare_images_params* p, void* out, Args& a, int* empty)
{
    *empty = 0;
    if (!p) return accv::fail(ACCV_EINVAL, "%s: null params", who);
    if (p->batch < 0) return accv::fail(ACCV_EINVAL, "%s: negative batch size", who);
    const long long extents[6] = {p->source_h, p->source_w, p->output_h, p->output_w, p->tile_h, p->tile_w};
    for (long long v : extents)
        if (v < 1 || v > kMaxExtent)
            return accv::fail(ACCV_EINVAL, "%s: source %lld x %lld, output %lld x %lld, tile %lld x %lld: each must be in [1, %d]",
                              who, p->source_h, p->source_w, p->output_h, p->output_w, p->tile_h, p->tile_w, kMaxExtent);
    if (!transforms && (p->output_h != p->source_h || p->output_w != p->source_w))
        return accv::fail(ACCV_EINVAL, "%s: an output of %lld x %lld from a source of %lld x %lld needs transforms", who,
                          p->output_h, p->output_w, p->source_h, p->source_w);
    if (p->layout != ACCV_IP_LAYOUT_CHW && p->layout != ACCV_IP_LAYOUT_HWC)
        return accv::fail(ACCV_EINVAL, "%s: unknown layout %d", who, p->layout);
    if (p->dtype != kF32 && p->dtype != kF16 && p->dtype != kBF16)
        return accv::fail(ACCV_EINVAL, "%s: unknown output dtype %d (0 f32, 1 f16, 2 bf16)", who, p->dtype);
    for (int c = 0; c < 3; ++c)
        if (!std::isfinite(p->mean[c]) || !std::isfinite(p->std[c]) || !(p->std[c] > 0.0))
            return accv::fail(ACCV_EINVAL, "%s: mean %g / std %g of channel %d: both finite and std > 0", who, p->mean[c],
                              p->std[c], c);
    if (p->batch == 0) {
        *empty = 1;
        return ACCV_OK;
    }
    if (!images || !out) return accv::fail(ACCV_EINVAL, "%s: null images / out pointer", who);
    const int esize = accv::elem_size(p->dtype);
    if ((reinterpret_cast<uintptr_t>(transforms) | reinterpret_cast<uintptr_t>(photometric)) & 3u)
        return accv::fail(ACCV_EINVAL, "%s: transforms / photometric are not aligned to their element size", who);
    if (reinterpret_cast<uintptr_t>(source_hw) & (p->source_hw_i64 ? 7u : 3u))
        return accv::fail(ACCV_EINVAL, "%s: source_hw is not aligned to its element size", who);
    if (reinterpret_cast<uintptr_t>(out) & (uintptr_t)(esize - 1))
        return accv::fail(ACCV_EINVAL, "%s: out is not aligned to its element size", who);
    const long long Hp = (p->output_h + p->tile_h - 1) / p->tile_h * p->tile_h;
    const long long Wp = (p->output_w + p->tile_w - 1) / p->tile_w * p->tile_w;
    const long long tiles_x = (Wp + kTileW - 1) / kTileW, tiles_y = (Hp + kTileH - 1) / kTileH;
    if (p->batch > accv::kGridLimit / (tiles_x * tiles_y))
        return accv::fail(ACCV_EINVAL, "%s: %lld images x %lld tiles exceed the grid limit", who, p->batch, tiles_x * tiles_y);
    a.images = images, a.source_hw = source_hw, a.transforms = transforms, a.photometric = photometric, a.out = out;
    a.coords = nullptr;
    a.B = p->batch;
    a.Hs = (int)p->source_h, a.Ws = (int)p->source_w, a.Ho = (int)p->output_h, a.Wo = (int)p->output_w;
    a.Hp = (int)Hp, a.Wp = (int)Wp, a.tiles_x = (int)tiles_x, a.tiles_y = (int)tiles_y;
    a.hw64 = p->source_hw_i64 ? 1 : 0;
    a.vec = (Wp % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & (uintptr_t)(4 * esize - 1)) == 0) ? 1 : 0;
    for (int c = 0; c < 3; ++c) {
        a.n.scale[c] = (float)(255.0 / p->std[c]);
        a.n.bias[c] = (float)(-p->mean[c] / p->std[c]);
        a.n.pad[c] = p->pad_before_normalize ? a.n.bias[c] : 0.0f;
    }
    a.n.is_bgr = p->is_bgr ? 1 : 0;
    return ACCV_OK;
}

// the NV12 entries: everything the two source kinds share is check_args; the planes' strides and format on top of it
int check_nv12_args(const char* who, const unsigned char* y, const unsigned char* uv, const void* source_hw,
                    const float* transforms, const float* photometric, const accv_prepare_images_nv12_params* p, void* out,
                    Nv12Args& a, int* empty)
{
    *empty = 0;
    if (!p) return accv::fail(ACCV_EINVAL, "%s: null params", who);
    const accv_nv12_params& pl = p->planes;
    if (pl.y_stride_batch < 0 || pl.y_stride_row < 0 || pl.uv_stride_batch < 0 || pl.uv_stride_row < 0)
        return accv::fail(ACCV_EINVAL, "%s: negative stride (y %lld, %lld; uv %lld, %lld)", who, pl.y_stride_batch, pl.y_stride_row,
                          pl.uv_stride_batch, pl.uv_stride_row);
    accv_prepare_images_params prepare = p->prepare;
    prepare.is_bgr = pl.as_bgr;
    if (int rc = check_args(who, y, source_hw, transforms, photometric, &prepare, out, a, empty)) return rc;
    if (*empty) return ACCV_OK;
    if (!uv) return accv::fail(ACCV_EINVAL, "%s: null uv pointer", who);
    a.uv = uv;
    a.y_batch = pl.y_stride_batch, a.y_row = pl.y_stride_row, a.uv_batch = pl.uv_stride_batch, a.uv_row = pl.uv_stride_row;
    a.f.full_range = pl.full_range ? 1 : 0, a.f.as_bgr = pl.as_bgr ? 1 : 0, a.f.vu = pl.chroma_vu ? 1 : 0;
    return ACCV_OK;
}

template <class A>
void host_for(const A& a, int dtype, bool hwc)
{
    switch (dtype) {
    case kF32: host_run<kF32>(a, hwc); break;
    case kF16: host_run<kF16>(a, hwc); break;
    default: host_run<kBF16>(a, hwc); break;
    }
}

}  // namespace

extern "C" {

int accv_prepare_images(const unsigned char* images, const void* source_hw, const float* transforms, const float* photometric,
                        const accv_prepare_images_params* params, void* out, void* stream)
{
    const char* who = "prepare_images";
    Args a;
    int empty;
    if (int rc = check_args(who, images, source_hw, transforms, photometric, params, out, a, &empty)) return rc;
    if (empty) return ACCV_OK;
    return launch_for(a, params->dtype, params->layout == ACCV_IP_LAYOUT_HWC, static_cast<hipStream_t>(stream));
}

int accv_prepare_images_host(const unsigned char* images, const void* source_hw, const float* transforms,
                             const float* photometric, const accv_prepare_images_params* params, void* out, float* coords)
{
    const char* who = "prepare_images (host)";
    Args a;
    int empty;
    if (int rc = check_args(who, images, source_hw, transforms, photometric, params, out, a, &empty)) return rc;
    if (empty) return ACCV_OK;
    if (reinterpret_cast<uintptr_t>(coords) & 3u) return accv::fail(ACCV_EINVAL, "%s: coords is not aligned to its element size", who);
    a.coords = coords;
    host_for(a, params->dtype, params->layout == ACCV_IP_LAYOUT_HWC);
    return ACCV_OK;
}

int accv_prepare_images_nv12(const unsigned char* y, const unsigned char* uv, const void* source_hw, const float* transforms,
                             const float* photometric, const accv_prepare_images_nv12_params* params, void* out, void* stream)
{
    const char* who = "prepare_images_nv12";
    Nv12Args a;
    int empty;
    if (int rc = check_nv12_args(who, y, uv, source_hw, transforms, photometric, params, out, a, &empty)) return rc;
    if (empty) return ACCV_OK;
    return launch_for(a, params->prepare.dtype, params->prepare.layout == ACCV_IP_LAYOUT_HWC, static_cast<hipStream_t>(stream));
}

int accv_prepare_images_nv12_host(const unsigned char* y, const unsigned char* uv, const void* source_hw,
                                  const float* transforms, const float* photometric,
                                  const accv_prepare_images_nv12_params* params, void* out)
{
    const char* who = "prepare_images_nv12 (host)";
    Nv12Args a;
    int empty;
    if (int rc = check_nv12_args(who, y, uv, source_hw, transforms, photometric, params, out, a, &empty)) return rc;
    if (empty) return ACCV_OK;
    host_for(a, params->prepare.dtype, params->prepare.layout == ACCV_IP_LAYOUT_HWC);
    return ACCV_OK;
}

}  // extern "C"
