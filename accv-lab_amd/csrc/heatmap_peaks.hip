// Heat-map peak extraction — the read-back half of mmdet's models/utils/gaussian_target.py that the drawn maps feed
// (get_local_maximum + get_topk_from_heatmap), fused:
//
//   s   = x * (x == max_pool2d(x, kernel, stride 1, padding kernel / 2))    window clipped at the border
//   out = the k largest s of each group in descending order, equal scores by ascending flat index in the group
//         (= torch.sort(s, descending=True, stable=True)[:k]);  a group is a frame (C*H*W) or one (b, c) plane (H*W)
//
// NaN: the window maximum carries NaN through as max_pool2d does, so a NaN scores NaN, its finite neighbours are
// suppressed to ±0 and a suppressed ±inf scores NaN (inf * 0).  torch.sort ranks NaN above +inf.
//
// Every element gets a unique 64-bit key (score bits, 0xFFFFFFFF - index in group; topk_select.h, which also holds the
// radix select and the bitonic sort both launches use): suppressed negatives tie with real zeros, larger key = earlier in
// the output, and the top-k of the keys IS the definition.
//
// Launch 1 (peaks_chunk_kernel): one workgroup per chunk of at most kChunk elements of one plane (R whole rows, or column
// tiles of kMaxCols columns with their halo for wider maps).  Phase A takes the vertical window maximum of every column
// of the chunk (plus the column halo) straight from global memory — the halo rows are L2 hits — into LDS together with
// the centre values; phase B takes the horizontal maximum from LDS and builds kPerThread keys per lane in registers.  An
// MSB-first radix select over 8-bit digits (256-bin LDS histogram, the lanes of a wave that share the leading lane's digit
// add once) finds the chunk's k-th largest key; the chunk's top min(k, size) keys go to its k workspace slots, the rest of
// the slots are zeroed.  Launch 2 (peaks_group_kernel): one workgroup per group runs the same radix select over the
// group's chunks * k workspace keys (L2 / Infinity Cache resident), gathers the k winners into LDS, sorts them with a
// bitonic network and writes scores, indices, classes, ys and xs.  The LDS slot counters only place the winners before the
// sort; output order comes from the unique keys alone, so results are bitwise reproducible.  Bandwidth work: no MFMA.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "accv_common.h"
#include "accv_numeric.h"
#include "topk_select.h"

namespace {

using namespace accv;   // dtype codes (f64 is not taken here), load / store<DT> with the hardware f16 conversion
using namespace accv_topk;   // keys, Cut, SelectShared, radix_select, bitonic_sort_desc, kMaxK, kBins, kMaxGroup

constexpr int kThreads = 256;
constexpr int kPerThread = 16;
constexpr int kChunk = kThreads * kPerThread;   // interior elements of one chunk: 4096
constexpr int kMaxCols = 2048;                  // widest chunk; wider maps are cut into column tiles
constexpr int kMaxHalf = 3;                     // kernel <= 7
constexpr int kTileElems = kChunk + 2 * (2 * kMaxHalf);   // R * (chunk columns + halo): 2 rows * (2048 + 6) at most
constexpr int kUnroll = 8;                      // candidate keys per lane and step of the group kernel
constexpr int kGroupThreads = 1024;            // the group kernel: one workgroup per group, 16 waves of candidate loads
constexpr int kBatch = 4;                       // phase A elements per lane and step

struct Geometry {
    long long cw;          // columns of a chunk
    long long col_tiles;   // chunks across a row
    long long rows;        // rows of a chunk
    long long row_tiles;   // chunks down a plane
    long long per_plane() const { return col_tiles * row_tiles; }
};

Geometry geometry(long long H, long long W)
{
    Geometry g;
    g.cw = W < kMaxCols ? W : kMaxCols;
    g.col_tiles = (W + g.cw - 1) / g.cw;
    const long long r = kChunk / g.cw;
    g.rows = r < H ? r : H;
    g.row_tiles = (H + g.rows - 1) / g.rows;
    return g;
}

struct Params {
    long long H, W, C;
    long long cw, col_tiles, rows, row_tiles;
    int half;        // kernel / 2
    int k;
    int per_class;
    long long chunks_per_group;
};

// max_pool2d's window maximum: a NaN anywhere in the window makes it NaN (fmaxf would skip it).  One v_maximum3_f32
// per two elements on gfx950, as v_max3_f32 for fmaxf.
__device__ __forceinline__ float nan_max(float a, float b) { return __builtin_elementwise_maximum(a, b); }

template <int DT, int HALF>
__global__ __launch_bounds__(kThreads) void peaks_chunk_kernel(const void* __restrict__ x, Params p, u64* __restrict__ ws)
{
    __shared__ float s_vmax[kTileElems];
    __shared__ float s_centre[kTileElems];
    __shared__ SelectShared sh;
    const int tid = threadIdx.x;
    const long long chunks_per_plane = p.col_tiles * p.row_tiles;
    const long long plane = (long long)blockIdx.x / chunks_per_plane;
    const long long chunk = (long long)blockIdx.x - plane * chunks_per_plane;
    const long long r0 = (chunk / p.col_tiles) * p.rows, c0 = (chunk % p.col_tiles) * p.cw;
    const int R = (int)(p.rows < p.H - r0 ? p.rows : p.H - r0);
    const int CW = (int)(p.cw < p.W - c0 ? p.cw : p.W - c0);
    constexpr int h = HALF;
    const long long ca = c0 - h > 0 ? c0 - h : 0, cb = c0 + CW + h < p.W ? c0 + CW + h : p.W;
    const int AW = (int)(cb - ca);   // columns of the vertical-max tile: the chunk plus its clipped column halo
    const long long plane_off = plane * p.H * p.W;

    // phase A: vertical window maximum (rows clipped at the border) and the centre value of each tile column.  The
    // window is a compile-time height and kBatch elements go per step, so all their loads are in flight together.
    const int na = R * AW;
    for (int e0 = tid; e0 < na; e0 += kBatch * kThreads) {
        float v[kBatch][2 * HALF + 1];
#pragma unroll
        for (int u = 0; u < kBatch; ++u) {
            const int e = e0 + u * kThreads;
            const int r = e / AW;
            const long long row = r0 + r, col = ca + (e - r * AW);
            const long long base = plane_off + row * p.W + col;
#pragma unroll
            for (int d = -HALF; d <= HALF; ++d) {
                const bool ok = e < na && row + d >= 0 && row + d < p.H;
                v[u][d + HALF] = ok ? load<DT, kHwF16>(x, base + d * p.W) : -INFINITY;
            }
        }
#pragma unroll
        for (int u = 0; u < kBatch; ++u) {
            const int e = e0 + u * kThreads;
            float m = v[u][0];
#pragma unroll
            for (int d = 1; d <= 2 * HALF; ++d) m = nan_max(m, v[u][d]);
            if (e < na) s_vmax[e] = m, s_centre[e] = v[u][HALF];
        }
    }
    __syncthreads();

    // phase B: horizontal maximum, suppression, keys (kPerThread per lane, element tid + kThreads * j)
    const long long group_base = p.per_class ? 0 : (plane % p.C) * p.H * p.W;
    const int n = R * CW;
    const int off = (int)(c0 - ca);
    u64 keys[kPerThread];
#pragma unroll
    for (int j = 0; j < kPerThread; ++j) {
        const int e = tid + kThreads * j;
        keys[j] = 0;
        if (e < n) {
            const int r = e / CW, c = e - r * CW;
            const int a = r * AW + off + c;
            const int lo = (off + c - h > 0 ? -h : -(off + c)), hi = (off + c + h < AW ? h : AW - 1 - off - c);
            float m = -INFINITY;
            for (int d = lo; d <= hi; ++d) m = nan_max(m, s_vmax[a + d]);
            const float v = s_centre[a];
            // x * (x == max): a local maximum keeps its exact value, a suppressed element becomes v * 0 — ±0 for a
            // finite one, NaN for ±inf and for NaN (whose window maximum is NaN, never equal)
            const float s = v == m ? v : v * 0.0f;
            const long long idx = group_base + (r0 + r) * p.W + c0 + c;
            keys[j] = ((u64)score_bits(s) << 32) | (u64)(0xffffffffu - (unsigned)idx);
        }
    }

    const unsigned k = (unsigned)p.k;
    Cut cut{0, 64};
    if ((unsigned)n > k) {
        cut = radix_select(
            [&](auto&& f) {
#pragma unroll
                for (int j = 0; j < kPerThread; ++j) f(keys[j]);
            },
            k, sh);
    }
    if (tid == 0) sh.slots = 0;
    __syncthreads();
    u64* out = ws + (long long)blockIdx.x * k;
#pragma unroll
    for (int j = 0; j < kPerThread; ++j)
        if (cut.take(keys[j])) out[atomicAdd(&sh.slots, 1u)] = keys[j];
    __syncthreads();
    const unsigned taken = sh.slots;   // min(k, n)
    for (unsigned i = taken + tid; i < k; i += kThreads) out[i] = 0;
}

__global__ __launch_bounds__(kGroupThreads) void peaks_group_kernel(const u64* __restrict__ ws, Params p, int dtype,
                                                               void* __restrict__ scores, long long* __restrict__ indices,
                                                               long long* __restrict__ classes, long long* __restrict__ ys,
                                                               long long* __restrict__ xs)
{
    __shared__ u64 s_sel[kMaxK];
    __shared__ SelectShared sh;
    const int tid = threadIdx.x;
    const long long g = blockIdx.x;
    const unsigned k = (unsigned)p.k;
    const long long m = p.chunks_per_group * k;
    const u64* cand = ws + g * m;
    auto each = [&](auto&& f) {
        // kUnroll independent loads in flight per lane; the same trip count on every lane (f ballots)
        for (long long base = 0; base < m; base += (long long)kGroupThreads * kUnroll) {
            u64 key[kUnroll];
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) {
                const long long i = base + (long long)u * kGroupThreads + tid;
                key[u] = i < m ? cand[i] : 0ull;
            }
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) f(key[u]);
        }
    };
    const Cut cut = radix_select(each, k, sh);

    int P = 1;
    while (P < (int)k) P <<= 1;
    for (int i = tid; i < P; i += kGroupThreads) s_sel[i] = 0;
    if (tid == 0) sh.slots = 0;
    __syncthreads();
    each([&](u64 key) {
        if (cut.take(key)) s_sel[atomicAdd(&sh.slots, 1u)] = key;
    });
    __syncthreads();

    bitonic_sort_desc<kGroupThreads>(s_sel, P);

    const long long hw = p.H * p.W;
    for (int i = tid; i < (int)k; i += kGroupThreads) {
        const u64 key = s_sel[i];
        const long long idx = (long long)(0xffffffffu - (unsigned)key);
        const long long cls = p.per_class ? g % p.C : idx / hw;
        const long long in_plane = p.per_class ? idx : idx - cls * hw;
        const long long o = g * k + i;
        const float s = score_of(key);
        if (dtype == kF32) store<kF32>(scores, o, s);
        else if (dtype == kF16) store<kF16, kHwF16>(scores, o, s);   // exact: s came from an f16
        else static_cast<uint16_t*>(scores)[o] = (uint16_t)(__float_as_uint(s) >> 16);   // exact, as above: truncation is enough
        indices[o] = in_plane;
        classes[o] = cls;
        ys[o] = in_plane / p.W;
        xs[o] = in_plane % p.W;
    }
}

int check_args(const char* who, long long B, long long C, long long H, long long W, int kernel, int k, int dtype)
{
    if (B < 0 || C < 0 || H < 0 || W < 0)
        return accv::fail(ACCV_EINVAL, "%s: negative size (B %lld, C %lld, H %lld, W %lld)", who, B, C, H, W);
    if (dtype < kF32 || dtype > kBF16)
        return accv::fail(ACCV_EINVAL, "%s: unknown dtype code %d (0 f32, 1 f16, 2 bf16)", who, dtype);
    if (kernel < 1 || kernel > 2 * kMaxHalf + 1 || kernel % 2 == 0)
        return accv::fail(ACCV_EINVAL, "%s: kernel must be odd and in 1..7, got %d", who, kernel);
    if (k < 1 || k > kMaxK) return accv::fail(ACCV_EINVAL, "%s: k must be in 1..%d, got %d", who, kMaxK, k);
    return ACCV_OK;
}

// sizes the kernels index with: H * W and the group below 2^32 - 1 (the low key word), B * C and the chunk count within
// the launch grid.  Returns the chunk geometry's block count, or -1.
long long chunk_blocks(long long B, long long C, long long H, long long W)
{
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return -1;
    if (H > kMaxGroup / W || B > accv::kGridLimit || C > accv::kGridLimit / B) return -1;
    const long long pp = geometry(H, W).per_plane();
    if (pp > accv::kGridLimit / (B * C)) return -1;
    return B * C * pp;
}

int check_group(const char* who, long long B, long long C, long long H, long long W, int k, int per_class)
{
    if (chunk_blocks(B, C, H, W) < 0 || (!per_class && C > kMaxGroup / (H * W)))
        return accv::fail(ACCV_EINVAL, "%s: map %lld x %lld x %lld x %lld too large (groups below 2^32 - 1 elements, "
                          "fewer than 2^31 chunks)", who, B, C, H, W);
    const long long group = per_class ? H * W : C * H * W;
    if (group < k) return accv::fail(ACCV_EINVAL, "%s: k = %d exceeds the group size %lld", who, k, group);
    return ACCV_OK;
}

template <int DT>
void launch_chunks(long long blocks, hipStream_t stream, const void* x, const Params& p, u64* ws)
{
    const dim3 grid((unsigned)blocks), block(kThreads);
    switch (p.half) {
        case 0: hipLaunchKernelGGL((peaks_chunk_kernel<DT, 0>), grid, block, 0, stream, x, p, ws); break;
        case 1: hipLaunchKernelGGL((peaks_chunk_kernel<DT, 1>), grid, block, 0, stream, x, p, ws); break;
        case 2: hipLaunchKernelGGL((peaks_chunk_kernel<DT, 2>), grid, block, 0, stream, x, p, ws); break;
        default: hipLaunchKernelGGL((peaks_chunk_kernel<DT, 3>), grid, block, 0, stream, x, p, ws); break;
    }
}

}  // namespace

extern "C" {

size_t accv_heatmap_peaks_workspace_bytes(long long B, long long C, long long H, long long W, int k)
{
    const long long blocks = chunk_blocks(B, C, H, W);
    if (blocks < 0 || k < 1 || k > kMaxK) return 0;
    return accv::align_up((size_t)blocks * (size_t)k * sizeof(u64), 16);
}

int accv_heatmap_peaks(const void* x, int dtype, long long B, long long C, long long H, long long W, int kernel, int k,
                       int per_class, void* scores, long long* indices, long long* classes, long long* ys, long long* xs,
                       void* workspace, size_t workspace_bytes, void* stream_)
{
    const char* who = "heatmap_peaks";
    if (int rc = check_args(who, B, C, H, W, kernel, k, dtype)) return rc;
    if (B == 0 || (per_class && C == 0)) return ACCV_OK;   // no group: nothing to write
    if (int rc = check_group(who, B, C, H, W, k, per_class)) return rc;
    if (!x) return accv::fail(ACCV_EINVAL, "%s: null heat-map pointer", who);
    if (!scores || !indices || !classes || !ys || !xs) return accv::fail(ACCV_EINVAL, "%s: null output pointer", who);
    const size_t need = accv_heatmap_peaks_workspace_bytes(B, C, H, W, k);
    if (int rc = accv::check_workspace(who, workspace, workspace_bytes, need)) return rc;
    const Geometry g = geometry(H, W);
    Params p;
    p.H = H, p.W = W, p.C = C;
    p.cw = g.cw, p.col_tiles = g.col_tiles, p.rows = g.rows, p.row_tiles = g.row_tiles;
    p.half = kernel / 2;
    p.k = k;
    p.per_class = per_class ? 1 : 0;
    p.chunks_per_group = per_class ? g.per_plane() : C * g.per_plane();
    const long long blocks = chunk_blocks(B, C, H, W);
    const long long groups = per_class ? B * C : B;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    u64* ws = static_cast<u64*>(workspace);
    switch (dtype) {
        case kF32: launch_chunks<kF32>(blocks, stream, x, p, ws); break;
        case kF16: launch_chunks<kF16>(blocks, stream, x, p, ws); break;
        default: launch_chunks<kBF16>(blocks, stream, x, p, ws); break;
    }
    if (int rc = accv::check_launch(who)) return rc;
    hipLaunchKernelGGL(peaks_group_kernel, dim3((unsigned)groups), dim3(kGroupThreads), 0, stream, ws, p, dtype, scores, indices,
                       classes, ys, xs);
    return accv::check_launch(who);
}
}
