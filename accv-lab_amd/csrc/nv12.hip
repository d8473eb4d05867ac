// NV12 decoder surfaces -> interleaved uint8 RGB: the reference's convert_nv12_to_rgb (on_demand_video_decoder,
// ColorConvertKernels.cu) as an operator of its own.  Per-pixel arithmetic: nv12_arith.h.
//
// One workgroup of kThreads lanes per (image, tile of kTileW x kTileH pixels); a lane owns 4 consecutive x of one row.  A
// lane whose 4 pixels lie inside the image reads its 4 Y bytes and the 4 chroma bytes of its two UV pairs as two 4-byte
// loads (not aligned), else byte by byte up to the image's width; it writes its 12 output bytes as three 4-byte stores when
// the address is aligned, per byte otherwise.  Every output byte is written once; nothing beyond W bytes of a Y row and
// 2 * ceil(W / 2) bytes of a UV row is read; no workspace, no atomics, no host synchronisation.  All global indices are 64-bit.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "accv_common.h"
#include "nv12_arith.h"

namespace {

using accv_nv12::Format;

constexpr int kTileW = ACCV_IP_TILE_W, kTileH = ACCV_IP_TILE_H;
constexpr int kLanePixels = 4;
constexpr int kLanesPerRow = kTileW / kLanePixels;
constexpr int kThreads = kLanesPerRow * kTileH;
constexpr int kMaxExtent = ACCV_IP_MAX_EXTENT;

static_assert(kThreads == 256, "four waves per workgroup");

struct Args {
    const unsigned char* y;
    const unsigned char* uv;
    unsigned char* out;             // [B, H, W, 3]
    long long B;
    long long y_batch, y_row, uv_batch, uv_row;
    int H, W, tiles_x, tiles_y;
    Format f;
};

// pixel (x, y) of image b, byte by byte
__host__ __device__ inline void convert_one(const Args& a, long long b, int x, int y, int (&c)[3])
{
    const int Y = a.y[b * a.y_batch + y * a.y_row + x];
    const unsigned char* q = a.uv + b * a.uv_batch + (y / 2) * a.uv_row + (x / 2) * 2;
    accv_nv12::convert(a.f, Y, q[0], q[1], c[0], c[1], c[2]);
}

__global__ __launch_bounds__(kThreads) void nv12_to_rgb_kernel(const Args a)
{
    const int tid = threadIdx.x;
    unsigned wg = blockIdx.x;                     // (b * tiles_y + ty) * tiles_x + tx
    const int tx = (int)(wg % (unsigned)a.tiles_x);
    wg /= (unsigned)a.tiles_x;
    const int ty = (int)(wg % (unsigned)a.tiles_y);
    const long long b = wg / (unsigned)a.tiles_y;
    const int Y = ty * kTileH + tid / kLanesPerRow, X = tx * kTileW + (tid % kLanesPerRow) * kLanePixels;
    if (Y >= a.H || X >= a.W) return;

    unsigned char* o = a.out + ((b * a.H + Y) * (long long)a.W + X) * 3;
    if (X + kLanePixels <= a.W) {
        // X is a multiple of 4: the two chroma pairs of the four pixels are the 4 bytes from byte X of the UV row on
        uint32_t luma, chroma;
        memcpy(&luma, a.y + b * a.y_batch + Y * a.y_row + X, 4);
        memcpy(&chroma, a.uv + b * a.uv_batch + (Y / 2) * a.uv_row + X, 4);
        int c[kLanePixels][3];
#pragma unroll
        for (int j = 0; j < kLanePixels; ++j) {
            const uint32_t pair = chroma >> (16 * (j / 2));
            accv_nv12::convert(a.f, (int)((luma >> (8 * j)) & 0xffu), (int)(pair & 0xffu), (int)((pair >> 8) & 0xffu), c[j][0],
                               c[j][1], c[j][2]);
        }
        if ((reinterpret_cast<uintptr_t>(o) & 3u) == 0) {
            uint32_t w[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                w[k] = 0;
#pragma unroll
                for (int i = 0; i < 4; ++i) w[k] |= (uint32_t)c[(k * 4 + i) / 3][(k * 4 + i) % 3] << (8 * i);
            }
            uint32_t* o4 = reinterpret_cast<uint32_t*>(o);
            o4[0] = w[0], o4[1] = w[1], o4[2] = w[2];
        } else {
#pragma unroll
            for (int j = 0; j < kLanePixels; ++j)
#pragma unroll
                for (int k = 0; k < 3; ++k) o[j * 3 + k] = (unsigned char)c[j][k];
        }
    } else {
        for (int j = 0; X + j < a.W; ++j) {
            int c[3];
            convert_one(a, b, X + j, Y, c);
            o[j * 3] = (unsigned char)c[0], o[j * 3 + 1] = (unsigned char)c[1], o[j * 3 + 2] = (unsigned char)c[2];
        }
    }
}

void host_run(const Args& a)
{
    for (long long b = 0; b < a.B; ++b)
        for (int y = 0; y < a.H; ++y)
            for (int x = 0; x < a.W; ++x) {
                int c[3];
                convert_one(a, b, x, y, c);
                unsigned char* o = a.out + ((b * a.H + y) * (long long)a.W + x) * 3;
                o[0] = (unsigned char)c[0], o[1] = (unsigned char)c[1], o[2] = (unsigned char)c[2];
            }
}

// ACCV_OK with *empty = 1 when there is nothing to write; every check runs before anything else reads the arguments
int check_args(const char* who, const unsigned char* y, const unsigned char* uv, const accv_nv12_params* p, unsigned char* out,
               Args& a, int* empty)
{
    *empty = 0;
    if (!p) return accv::fail(ACCV_EINVAL, "%s: null params", who);
    if (p->batch < 0) return accv::fail(ACCV_EINVAL, "%s: negative batch size", who);
    if (p->height < 1 || p->height > kMaxExtent || p->width < 1 || p->width > kMaxExtent)
        return accv::fail(ACCV_EINVAL, "%s: planes of %lld x %lld: each extent must be in [1, %d]", who, p->height, p->width,
                          kMaxExtent);
    if (p->y_stride_batch < 0 || p->y_stride_row < 0 || p->uv_stride_batch < 0 || p->uv_stride_row < 0)
        return accv::fail(ACCV_EINVAL, "%s: negative stride (y %lld, %lld; uv %lld, %lld)", who, p->y_stride_batch, p->y_stride_row,
                          p->uv_stride_batch, p->uv_stride_row);
    if (p->batch == 0) {
        *empty = 1;
        return ACCV_OK;
    }
    if (!y || !uv || !out) return accv::fail(ACCV_EINVAL, "%s: null y / uv / out pointer", who);
    const long long tiles_x = (p->width + kTileW - 1) / kTileW, tiles_y = (p->height + kTileH - 1) / kTileH;
    if (p->batch > accv::kGridLimit / (tiles_x * tiles_y))
        return accv::fail(ACCV_EINVAL, "%s: %lld images x %lld tiles exceed the grid limit", who, p->batch, tiles_x * tiles_y);
    a.y = y, a.uv = uv, a.out = out;
    a.B = p->batch;
    a.y_batch = p->y_stride_batch, a.y_row = p->y_stride_row, a.uv_batch = p->uv_stride_batch, a.uv_row = p->uv_stride_row;
    a.H = (int)p->height, a.W = (int)p->width, a.tiles_x = (int)tiles_x, a.tiles_y = (int)tiles_y;
    a.f.full_range = p->full_range ? 1 : 0, a.f.as_bgr = p->as_bgr ? 1 : 0, a.f.vu = p->chroma_vu ? 1 : 0;
    return ACCV_OK;
}

}  // namespace

extern "C" {

int accv_nv12_to_rgb(const unsigned char* y, const unsigned char* uv, const accv_nv12_params* params, unsigned char* out,
                     void* stream)
{
    const char* who = "nv12_to_rgb";
    Args a;
    int empty;
    if (int rc = check_args(who, y, uv, params, out, a, &empty)) return rc;
    if (empty) return ACCV_OK;
    const long long groups = a.B * a.tiles_y * a.tiles_x;
    hipLaunchKernelGGL(nv12_to_rgb_kernel, dim3((unsigned)groups), dim3(kThreads), 0, static_cast<hipStream_t>(stream), a);
    return accv::check_launch(who);
}

int accv_nv12_to_rgb_host(const unsigned char* y, const unsigned char* uv, const accv_nv12_params* params, unsigned char* out)
{
    const char* who = "nv12_to_rgb (host)";
    Args a;
    int empty;
    if (int rc = check_args(who, y, uv, params, out, a, &empty)) return rc;
    if (empty) return ACCV_OK;
    host_run(a);
    return ACCV_OK;
}

}  // extern "C"
