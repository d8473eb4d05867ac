// Centre-point regression — the second branch of a CenterNet / CenterPoint head next to the heat map: the values of the
// regression maps (offset, size, height, rot, vel ...) at the object centres, their L1 / smooth-L1 loss against a
// [B, N, C] table of targets, and the backward of both.  It replaces mmdet's transpose_and_gather_feat pattern
// (models/utils/gaussian_target.py: cat of the heads, permute(0, 2, 3, 1).contiguous() of the whole [B, C, H, W] tensor, a
// gather of a few hundred rows, and in the backward a scatter into a zero-filled tensor, a permute back and the split of
// the cat) by N * C scattered reads forward and ONE write-only pass over the gradient maps backward.
//
//   gather   out[b, n, c] = maps[b, c, y_bn, x_bn] at a valid slot, +0 elsewhere              (one launch)
//   loss     sum over valid (b, n), c of  w * l(maps[b, c, y, x] - targets[b, n, c]) / denom
//            one workgroup per frame -> an f64 partial and a valid count per frame, then a one-block launch that adds
//            the partials in a fixed order and writes loss and denominator                     (two launches)
//   scatter  the backward of either: every gradient map written completely, exactly once       (one launch)
//
// The scatter kernel has the "fused clear + a few hits" shape of the splat.  A workgroup owns a band of rows of one frame
// across all channels of all maps.  It (1) culls the frame's centres to its band (ballot per wave, as the splat does) into
// an LDS list that keeps the slot order, (2) streams +0 over its band with 16-byte stores per lane (element stores for the
// at most 15 bytes before and after the aligned body of a channel's span), (3) passes a workgroup barrier and (4) patches
// the cells of its band that a valid slot names.  Every cell lies in exactly one band, so no two workgroups ever write
// the same address: there is no ordering between workgroups to rely on, no atomics and no read-modify-write.  Zero and
// patch stores are both plain global stores from the same workgroup separated by __syncthreads(), which is a
// workgroup-scope release / acquire: the zero stores have completed at the CU's cache before any patch store issues, and
// that cache keeps stores to one address in order.  (No non-temporal policy on either store: a streaming zero store
// followed by a plain patch store would not have that guarantee.)
//
// Several valid slots of a frame on one cell: the LOWEST slot is the cell's leader (a slot is a leader when no earlier
// valid slot names its cell); the leader's lanes add the contributions of all slots on the cell in ascending slot order
// in f32, round once and store.  The others store nothing.  The summation order is therefore fixed by the slot order
// alone.  A band named by more than kList slots (thousands of objects on a few rows) applies the same rule with the
// centres re-read from global memory instead of the list.  Contraction into fma is switched off for this file so that
// "product, then sum" means exactly that.
// Bandwidth / launch bound work: no MFMA.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "accv_common.h"
#include "accv_numeric.h"
#include "pointwise_loss_arith.h"

#pragma clang fp contract(off)

namespace {

using accv_loss::dloss_of;
using accv_loss::kL1;
using accv_loss::kSmoothL1;
using accv_loss::loss_of;

using namespace accv;   // dtype codes (f64 is not taken here), Stored<DT>, load / store<DT>, block_sum, denominator

constexpr int kThreads = 256;
constexpr int kMaxMaps = ACCV_CR_MAX_MAPS;
constexpr int kMaxChannels = ACCV_CR_MAX_CHANNELS;
constexpr int kList = 2048;                     // slots of one band the LDS list holds; a band with more takes the slow path

// Elements are widened and narrowed with the hardware f16 conversion (load / store<DT, kHwF16>): device-only kernels.

// the maps of a call: base pointers and the first concatenated channel of each (first[n] = C)
struct MapSet {
    void* p[kMaxMaps];
    int first[kMaxMaps + 1];
    int n;
};
struct Centers {
    const void* where;    // int32 [B, N, 2] (x, y) or, index_form, int64 [B, N] of y * W + x
    const void* counts;   // [B] int32 / int64; not read in index form
    long long N;
    int index_form, counts_i64;
};
struct Plane {
    long long B, H, W;
    int C;
};
struct LossArgs {
    const float* targets;    // [B, N, C]
    const float* weights;    // null, [B, N] or [B, N, C]
    int per_channel;
    float beta;
    const float* grad_out;   // backward: device scalars
    const float* denom;
};

// map and channel inside it of concatenated channel c — constant indices only, so the by-value struct stays in registers
struct Chan {
    void* p;
    int local, count;
};
__device__ __forceinline__ Chan channel_of(const MapSet& ms, int c)
{
    Chan o{ms.p[0], c, ms.first[1]};
#pragma unroll
    for (int i = 1; i < kMaxMaps; ++i)
        if (i < ms.n && c >= ms.first[i]) o = Chan{ms.p[i], c - ms.first[i], ms.first[i + 1] - ms.first[i]};
    return o;
}
// element offset of (b, local channel, cell) in a [B, count, H * W] map
__device__ __forceinline__ long long element_of(const Chan& ch, long long b, long long plane, long long cell)
{
    return (b * ch.count + ch.local) * plane + cell;
}

__device__ __forceinline__ long long slots_of(const Centers& ce, long long b)
{
    return ce.index_form ? ce.N : clamp_count(ce.counts, b, ce.N, ce.counts_i64);
}
// in-plane cell of slot n (below the frame's slot count), -1 when it lies outside the map
__device__ __forceinline__ long long cell_of(const Centers& ce, const Plane& g, long long b, long long n)
{
    const long long s = b * ce.N + n;
    if (ce.index_form) {
        const long long v = static_cast<const long long*>(ce.where)[s];
        return (v >= 0 && v < g.H * g.W) ? v : -1;
    }
    const int* xy = static_cast<const int*>(ce.where) + 2 * s;
    const long long x = xy[0], y = xy[1];
    return (x >= 0 && x < g.W && y >= 0 && y < g.H) ? y * g.W + x : -1;
}

// ---------------------------------------------------------------------------------------------------------------- gather
template <int DT>
__global__ __launch_bounds__(kThreads) void gather_kernel(const MapSet maps, const Centers ce, const Plane g,
                                                          Stored<DT>* __restrict__ out)
{
    using raw = Stored<DT>;
    const long long total = g.B * ce.N * g.C, stride = (long long)gridDim.x * kThreads;
    const long long plane = g.H * g.W;
    for (long long e = (long long)blockIdx.x * kThreads + threadIdx.x; e < total; e += stride) {
        const long long r = e / g.C, b = r / ce.N, n = r - b * ce.N;
        const int c = (int)(e - r * g.C);
        const long long cell = n < slots_of(ce, b) ? cell_of(ce, g, b, n) : -1;
        raw v = raw(0);
        if (cell >= 0) {
            const Chan ch = channel_of(maps, c);
            v = static_cast<const raw*>(ch.p)[element_of(ch, b, plane, cell)];
        }
        out[e] = v;
    }
}

// ------------------------------------------------------------------------------------------------------------------ loss
template <int DT, int KIND>
__global__ __launch_bounds__(kThreads) void loss_fwd_kernel(const MapSet maps, const Centers ce, const Plane g, const LossArgs la,
                                                            double* __restrict__ part_sum,
                                                            unsigned long long* __restrict__ part_cnt)
{
    const long long b = blockIdx.x, plane = g.H * g.W;
    const long long total = slots_of(ce, b) * g.C;
    double acc = 0.0;
    unsigned long long cnt = 0;
    for (long long t = threadIdx.x; t < total; t += kThreads) {
        const long long n = t / g.C;
        const int c = (int)(t - n * g.C);
        const long long cell = cell_of(ce, g, b, n);
        if (cell < 0) continue;
        cnt += c == 0;
        const Chan ch = channel_of(maps, c);
        const float x = load<DT, kHwF16>(ch.p, element_of(ch, b, plane, cell));
        const long long row = b * ce.N + n;
        const float w = la.weights ? la.weights[la.per_channel ? row * g.C + c : row] : 1.0f;
        acc += (double)(loss_of<KIND, float>(x - la.targets[row * g.C + c], la.beta) * w);
    }
    block_sum<double, unsigned long long, kThreads>(acc, cnt);
    if (threadIdx.x == 0) part_sum[b] = acc, part_cnt[b] = cnt;
}

// one workgroup: the frames' partials in a fixed order -> loss, denominator
__global__ __launch_bounds__(kThreads) void loss_finish_kernel(const double* __restrict__ part_sum,
                                                               const unsigned long long* __restrict__ part_cnt, long long nparts,
                                                               int avg_mode, float avg_value, const float* __restrict__ avg_dev,
                                                               float* __restrict__ out_loss, float* __restrict__ out_denom)
{
    double acc = 0.0;
    unsigned long long cnt = 0;
    for (long long i = threadIdx.x; i < nparts; i += kThreads) acc += part_sum[i], cnt += part_cnt[i];
    block_sum<double, unsigned long long, kThreads>(acc, cnt);
    if (threadIdx.x == 0) {
        const float denom = denominator(avg_mode, avg_value, avg_dev, cnt);   // valid.sum().clamp(min=1), as float32
        *out_loss = (float)(acc / (double)denom);
        *out_denom = denom;
    }
}

// --------------------------------------------------------------------------------------------------------------- scatter
// +0 over n elements from p (element-aligned): element stores up to the first 16-byte boundary and after the last one,
// 16-byte stores per lane between them
template <class raw>
__device__ __forceinline__ void zero_span(raw* p, long long n)
{
    constexpr long long VEC = 16 / sizeof(raw);
    long long head = (long long)((16u - (unsigned)(reinterpret_cast<uintptr_t>(p) & 15u)) & 15u) / (long long)sizeof(raw);
    head = head > n ? n : head;
    const long long nvec = (n - head) / VEC, tail = n - head - nvec * VEC;
    if (threadIdx.x < head) p[threadIdx.x] = raw(0);
    uint4* v = reinterpret_cast<uint4*>(p + head);
    const uint4 z = make_uint4(0u, 0u, 0u, 0u);
    long long i = threadIdx.x;
    for (; i + 3 * kThreads < nvec; i += 4 * kThreads) {
        v[i] = z;
        v[i + kThreads] = z;
        v[i + 2 * kThreads] = z;
        v[i + 3 * kThreads] = z;
    }
    for (; i < nvec; i += kThreads) v[i] = z;
    if (threadIdx.x < tail) p[head + nvec * VEC + threadIdx.x] = raw(0);
}

// SRC: -1 the gradient rows of gather_at_centers, otherwise the loss kind
constexpr int kRows = -1;

template <int DT, int SRC>
__global__ __launch_bounds__(kThreads) void scatter_kernel(const MapSet grads, const MapSet feats, const Centers ce, const Plane g,
                                                           const long long band_rows, const long long bands, const LossArgs la,
                                                           const Stored<DT>* __restrict__ rows)
{
    using raw = Stored<DT>;
    __shared__ int s_slot[kList], s_hit[kList];   // the frame's valid slots on cells of this band, in slot order
    __shared__ int s_wave[kThreads / 64];
    __shared__ int s_lead[kThreads];
    const long long b = blockIdx.x / bands, band = blockIdx.x - b * bands;
    const long long r0 = band * band_rows, r1 = r0 + band_rows < g.H ? r0 + band_rows : g.H;
    const long long plane = g.H * g.W, lo = r0 * g.W, hi = r1 * g.W;
    const long long ns = slots_of(ce, b);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    // cull the frame's centres to the band: ballot per wave, wave totals through LDS, so the list keeps the slot order
    long long count = 0;
    for (long long base = 0; base < ns; base += kThreads) {
        const long long n = base + tid;
        const long long cell = n < ns ? cell_of(ce, g, b, n) : -1;
        const bool hit = cell >= lo && cell < hi;
        const unsigned long long vote = __ballot(hit);
        if (lane == 0) s_wave[wave] = __popcll(vote);
        __syncthreads();
        long long pos = count + __popcll(vote & ((1ull << lane) - 1ull));
#pragma unroll
        for (int w = 0; w < kThreads / 64; ++w) {
            pos += w < wave ? s_wave[w] : 0;
            count += s_wave[w];
        }
        if (hit && pos < kList) s_slot[pos] = (int)n, s_hit[pos] = (int)cell;
        __syncthreads();
    }

    for (int c = 0; c < g.C; ++c) {
        const Chan ch = channel_of(grads, c);
        zero_span<raw>(static_cast<raw*>(ch.p) + element_of(ch, b, plane, lo), hi - lo);
    }
    __syncthreads();   // the band's zero stores are ordered before the patch stores below
    if (count == 0) return;

    float scale = 1.0f;
    if constexpr (SRC != kRows) scale = *la.grad_out / *la.denom;
    // the contribution of slot j to channel c of its cell (x: the map's value there)
    auto contribution = [&](long long j, int c, float x) -> float {
        const long long row = b * ce.N + j;
        if constexpr (SRC == kRows) {
            return load<DT, kHwF16>(rows, row * g.C + c);
        } else {
            const float w = la.weights ? la.weights[la.per_channel ? row * g.C + c : row] : 1.0f;
            return (w * dloss_of<SRC, float>(x - la.targets[row * g.C + c], la.beta)) * scale;
        }
    };

    if (count <= kList) {
        // one lane per (listed slot, channel): the first listed slot of a cell leads it and adds the later ones in order
        for (long long t = tid; t < count * g.C; t += kThreads) {
            const int i = (int)(t / g.C), c = (int)(t - (long long)i * g.C);
            const int cell = s_hit[i];
            bool leader = true;
            for (int k = 0; k < i; ++k) leader = leader && s_hit[k] != cell;
            if (!leader) continue;
            const Chan gc = channel_of(grads, c);
            const long long at = element_of(gc, b, plane, cell);
            float x = 0.0f;
            if constexpr (SRC != kRows) x = load<DT, kHwF16>(channel_of(feats, c).p, at);
            float acc = 0.0f;
            for (int k = i; k < (int)count; ++k)
                if (s_hit[k] == cell) acc += contribution(s_slot[k], c, x);
            store<DT, kHwF16>(gc.p, at, acc);
        }
        return;
    }

    // more hits in one band than the list holds: the same rule straight from the centres in global memory
    for (long long base = 0; base < ns; base += kThreads) {
        const long long n = base + tid;
        const long long mine = n < ns ? cell_of(ce, g, b, n) : -1;
        bool leader = mine >= lo && mine < hi;
        if (leader)
            for (long long j = 0; j < n; ++j)
                if (cell_of(ce, g, b, j) == mine) {
                    leader = false;
                    break;
                }
        if (!__syncthreads_or(leader)) continue;   // also keeps s_lead of the previous step until every lane is done with it
        s_lead[tid] = leader ? (int)mine : -1;
        __syncthreads();
        for (int t = tid; t < kThreads * g.C; t += kThreads) {
            const int i = t / g.C, c = t - i * g.C;
            const long long cell = s_lead[i];
            if (cell < 0) continue;
            const Chan gc = channel_of(grads, c);
            const long long at = element_of(gc, b, plane, cell);
            float x = 0.0f;
            if constexpr (SRC != kRows) x = load<DT, kHwF16>(channel_of(feats, c).p, at);
            float acc = 0.0f;
            for (long long j = base + i; j < ns; ++j)
                if (cell_of(ce, g, b, j) == cell) acc += contribution(j, c, x);
            store<DT, kHwF16>(gc.p, at, acc);
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------ host
struct Problem {
    MapSet maps;
    Centers ce;
    Plane g;
    size_t esize;
};

// the checks every entry shares; fills `pr`.  `second` is an optional second pointer array of the same maps (the gradient
// maps of the loss backward).
int prepare(const char* who, const void* const* maps, const void* const* second, const int* channels, int num_maps, int dtype,
            long long B, long long H, long long W, const void* centers, const void* counts, long long N, unsigned flags,
            unsigned allowed_flags, Problem& pr, MapSet* second_set)
{
    if (B < 0 || H < 0 || W < 0 || N < 0) return accv::fail(ACCV_EINVAL, "%s: negative size (B %lld, H %lld, W %lld, N %lld)", who, B, H, W, N);
    if (dtype < kF32 || dtype > kBF16) return accv::fail(ACCV_EINVAL, "%s: unknown dtype code %d (0 f32, 1 f16, 2 bf16)", who, dtype);
    if (flags & ~allowed_flags) return accv::fail(ACCV_EINVAL, "%s: unknown flag bits 0x%x", who, flags & ~allowed_flags);
    if (num_maps < 1 || num_maps > kMaxMaps)
        return accv::fail(ACCV_EINVAL, "%s: 1..%d maps supported, got %d", who, kMaxMaps, num_maps);
    if (!maps || !channels || (second_set && !second)) return accv::fail(ACCV_EINVAL, "%s: null array", who);
    if (H > 0 && W > 0 && H > 0x7fffffffll / W) return accv::fail(ACCV_EINVAL, "%s: a plane of %lld x %lld exceeds 2^31 - 1 cells", who, H, W);
    pr.esize = (size_t)elem_size(dtype);
    pr.maps.n = num_maps;
    long long C = 0;
    for (int i = 0; i < kMaxMaps + 1; ++i) pr.maps.first[i] = 0;
    for (int i = 0; i < kMaxMaps; ++i) pr.maps.p[i] = nullptr;
    for (int i = 0; i < num_maps; ++i) {
        if (channels[i] < 0) return accv::fail(ACCV_EINVAL, "%s: map %d has a negative channel count %d", who, i, channels[i]);
        pr.maps.first[i] = (int)C;
        C += channels[i];
        if (C > kMaxChannels)
            return accv::fail(ACCV_EINVAL, "%s: more than %d channels in total", who, kMaxChannels);
    }
    for (int i = num_maps; i < kMaxMaps + 1; ++i) pr.maps.first[i] = (int)C;
    if (second_set) *second_set = pr.maps;
    const bool has_elems = B > 0 && H > 0 && W > 0;
    for (int i = 0; i < num_maps; ++i) {
        const void* both[2] = {maps[i], second_set ? second[i] : maps[i]};
        for (const void* p : both) {
            if (has_elems && channels[i] > 0 && !p) return accv::fail(ACCV_EINVAL, "%s: map %d is null", who, i);
            if (reinterpret_cast<uintptr_t>(p) % pr.esize)
                return accv::fail(ACCV_EINVAL, "%s: map %d is not aligned to its element size", who, i);
        }
        pr.maps.p[i] = const_cast<void*>(maps[i]);
        if (second_set) second_set->p[i] = const_cast<void*>(second[i]);
    }
    pr.ce = Centers{centers, counts, N, (flags & ACCV_CR_INDEX_FORM) ? 1 : 0, (flags & ACCV_CR_COUNTS_I64) ? 1 : 0};
    pr.g = Plane{B, H, W, (int)C};
    if (B > 0 && N > 0 && !centers) return accv::fail(ACCV_EINVAL, "%s: null centers pointer", who);
    if (B > 0 && !pr.ce.index_form && !counts) return accv::fail(ACCV_EINVAL, "%s: null counts pointer", who);
    return ACCV_OK;
}

int check_loss(const char* who, const accv_center_regression_params* params, bool forward)
{
    if (!params) return accv::fail(ACCV_EINVAL, "%s: null params", who);
    if (params->kind != ACCV_CR_L1 && params->kind != ACCV_CR_SMOOTH_L1)
        return accv::fail(ACCV_EINVAL, "%s: unknown loss kind %d (0 l1, 2 smooth_l1)", who, params->kind);
    if (params->kind == ACCV_CR_SMOOTH_L1 && !(params->beta > 0.0f))
        return accv::fail(ACCV_EINVAL, "%s: smooth_l1 needs beta > 0 (got %g)", who, params->beta);
    if (forward && (params->avg_mode < ACCV_FL_AVG_NUM_POS || params->avg_mode > ACCV_FL_AVG_DEVICE))
        return accv::fail(ACCV_EINVAL, "%s: unknown avg_factor mode %d", who, params->avg_mode);
    return ACCV_OK;
}

// rows of a band: workgroups of 16..64 KB, and about 2048 of them when the maps are large enough for that
void band_geometry(const Problem& pr, long long& band_rows, long long& bands)
{
    const long long row_bytes = pr.g.W * (long long)pr.esize * (pr.g.C > 0 ? pr.g.C : 1);
    const long long lo = (16384 + row_bytes - 1) / row_bytes;
    const long long hi = 65536 / row_bytes > lo ? 65536 / row_bytes : lo;
    long long rows = pr.g.H * pr.g.B / 2048;
    rows = rows < lo ? lo : (rows > hi ? hi : rows);
    band_rows = rows > pr.g.H ? pr.g.H : rows;
    bands = (pr.g.H + band_rows - 1) / band_rows;
}

template <int DT>
void launch_scatter(int src, dim3 grid, hipStream_t stream, const MapSet& grads, const MapSet& feats, const Problem& pr,
                    long long band_rows, long long bands, const LossArgs& la, const void* rows_)
{
    const auto* rows = static_cast<const Stored<DT>*>(rows_);
    const dim3 block(kThreads);
#define SCATTER(S) hipLaunchKernelGGL((scatter_kernel<DT, S>), grid, block, 0, stream, grads, feats, pr.ce, pr.g, band_rows, bands, la, rows)
    if (src == kRows) SCATTER(kRows);
    else if (src == kL1) SCATTER(kL1);
    else SCATTER(kSmoothL1);
#undef SCATTER
}

// the complete write of the gradient maps: `pr.maps` are read (loss) or unused (rows), `grads` written
int scatter(const char* who, int src, int dtype, const Problem& pr, const MapSet& grads, const LossArgs& la, const void* rows,
            hipStream_t stream)
{
    if (pr.g.B == 0 || pr.g.C == 0 || pr.g.H == 0 || pr.g.W == 0) return ACCV_OK;   // the gradient maps have no elements
    long long band_rows, bands;
    band_geometry(pr, band_rows, bands);
    if (bands > accv::kGridLimit / pr.g.B) return accv::fail(ACCV_EINVAL, "%s: %lld x %lld bands exceed the grid limit", who, pr.g.B, bands);
    const dim3 grid((unsigned)(pr.g.B * bands));
    switch (dtype) {
        case kF32: launch_scatter<kF32>(src, grid, stream, grads, pr.maps, pr, band_rows, bands, la, rows); break;
        case kF16: launch_scatter<kF16>(src, grid, stream, grads, pr.maps, pr, band_rows, bands, la, rows); break;
        default: launch_scatter<kBF16>(src, grid, stream, grads, pr.maps, pr, band_rows, bands, la, rows); break;
    }
    return accv::check_launch(who);
}

template <int DT>
void launch_loss(int kind, dim3 grid, hipStream_t stream, const Problem& pr, const LossArgs& la, double* ps, unsigned long long* pc)
{
    if (kind == kL1)
        hipLaunchKernelGGL((loss_fwd_kernel<DT, kL1>), grid, dim3(kThreads), 0, stream, pr.maps, pr.ce, pr.g, la, ps, pc);
    else
        hipLaunchKernelGGL((loss_fwd_kernel<DT, kSmoothL1>), grid, dim3(kThreads), 0, stream, pr.maps, pr.ce, pr.g, la, ps, pc);
}

}  // namespace

extern "C" {

int accv_gather_at_centers(const void* const* maps, const int* channels, int num_maps, int dtype, long long B, long long H,
                           long long W, const void* centers, const void* counts, long long N, unsigned flags, void* out,
                           void* stream_)
{
    const char* who = "gather_at_centers";
    Problem pr;
    if (int rc = prepare(who, maps, nullptr, channels, num_maps, dtype, B, H, W, centers, counts, N, flags,
                         ACCV_CR_COUNTS_I64 | ACCV_CR_INDEX_FORM, pr, nullptr))
        return rc;
    if (B == 0 || N == 0 || pr.g.C == 0) return ACCV_OK;
    if (!out) return accv::fail(ACCV_EINVAL, "%s: null output pointer", who);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const long long total = B * N * pr.g.C;
    long long blocks = (total + kThreads - 1) / kThreads;
    blocks = blocks > 8192 ? 8192 : blocks;
    const dim3 grid((unsigned)blocks), block(kThreads);
    switch (dtype) {
        case kF32: hipLaunchKernelGGL(gather_kernel<kF32>, grid, block, 0, stream, pr.maps, pr.ce, pr.g, static_cast<float*>(out)); break;
        case kF16: hipLaunchKernelGGL(gather_kernel<kF16>, grid, block, 0, stream, pr.maps, pr.ce, pr.g, static_cast<uint16_t*>(out)); break;
        default: hipLaunchKernelGGL(gather_kernel<kBF16>, grid, block, 0, stream, pr.maps, pr.ce, pr.g, static_cast<uint16_t*>(out)); break;
    }
    return accv::check_launch(who);
}

int accv_scatter_at_centers(void* const* grad_maps, const int* channels, int num_maps, int dtype, long long B, long long H,
                            long long W, const void* centers, const void* counts, long long N, unsigned flags,
                            const void* grad_rows, void* stream_)
{
    const char* who = "scatter_at_centers";
    Problem pr;
    if (int rc = prepare(who, grad_maps, nullptr, channels, num_maps, dtype, B, H, W, centers, counts, N, flags,
                         ACCV_CR_COUNTS_I64 | ACCV_CR_INDEX_FORM, pr, nullptr))
        return rc;
    if (B > 0 && N > 0 && pr.g.C > 0 && !grad_rows) return accv::fail(ACCV_EINVAL, "%s: null gradient rows pointer", who);
    return scatter(who, kRows, dtype, pr, pr.maps, LossArgs{}, grad_rows, static_cast<hipStream_t>(stream_));
}

size_t accv_center_regression_loss_workspace_bytes(long long B)
{
    if (B <= 0) return 0;
    return accv::align_up((size_t)B * (sizeof(double) + sizeof(unsigned long long)), 16);
}

int accv_center_regression_loss(const void* const* maps, const int* channels, int num_maps, int dtype, long long B,
                                long long H, long long W, const void* centers, const void* counts, long long N,
                                unsigned flags, const float* targets, const float* weights_or_null,
                                const accv_center_regression_params* params, const float* avg_factor_dev, float* out_loss,
                                float* out_denom, void* workspace, size_t workspace_bytes, void* stream_)
{
    const char* who = "center_regression_loss";
    Problem pr;
    if (int rc = prepare(who, maps, nullptr, channels, num_maps, dtype, B, H, W, centers, counts, N, flags,
                         ACCV_CR_COUNTS_I64 | ACCV_CR_WEIGHTS_PER_CHANNEL, pr, nullptr))
        return rc;
    if (int rc = check_loss(who, params, true)) return rc;
    if (B == 0) return ACCV_OK;
    if (B > accv::kGridLimit) return accv::fail(ACCV_EINVAL, "%s: batch exceeds the grid limit", who);
    if (N > 0 && pr.g.C > 0 && !targets) return accv::fail(ACCV_EINVAL, "%s: null targets pointer", who);
    if (!out_loss || !out_denom) return accv::fail(ACCV_EINVAL, "%s: null output pointer", who);
    if (params->avg_mode == ACCV_FL_AVG_DEVICE && !avg_factor_dev) return accv::fail(ACCV_EINVAL, "%s: null avg_factor pointer", who);
    const size_t need = accv_center_regression_loss_workspace_bytes(B);
    if (int rc = accv::check_workspace(who, workspace, workspace_bytes, need)) return rc;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    double* ps = static_cast<double*>(workspace);
    unsigned long long* pc = reinterpret_cast<unsigned long long*>(ps + B);
    const LossArgs la{targets, weights_or_null, (flags & ACCV_CR_WEIGHTS_PER_CHANNEL) ? 1 : 0, params->beta, nullptr, nullptr};
    const dim3 grid((unsigned)B);
    switch (dtype) {
        case kF32: launch_loss<kF32>(params->kind, grid, stream, pr, la, ps, pc); break;
        case kF16: launch_loss<kF16>(params->kind, grid, stream, pr, la, ps, pc); break;
        default: launch_loss<kBF16>(params->kind, grid, stream, pr, la, ps, pc); break;
    }
    if (int rc = accv::check_launch(who)) return rc;
    hipLaunchKernelGGL(loss_finish_kernel, dim3(1), dim3(kThreads), 0, stream, ps, pc, B, params->avg_mode, params->avg_factor,
                       avg_factor_dev, out_loss, out_denom);
    return accv::check_launch(who);
}

int accv_center_regression_loss_bwd(const void* const* maps, void* const* grad_maps, const int* channels, int num_maps,
                                    int dtype, long long B, long long H, long long W, const void* centers,
                                    const void* counts, long long N, unsigned flags, const float* targets,
                                    const float* weights_or_null, const accv_center_regression_params* params,
                                    const float* grad_out, const float* denom, void* stream_)
{
    const char* who = "center_regression_loss_bwd";
    Problem pr;
    MapSet grads;
    if (int rc = prepare(who, maps, grad_maps, channels, num_maps, dtype, B, H, W, centers, counts, N, flags,
                         ACCV_CR_COUNTS_I64 | ACCV_CR_WEIGHTS_PER_CHANNEL, pr, &grads))
        return rc;
    if (int rc = check_loss(who, params, false)) return rc;
    if (B == 0) return ACCV_OK;
    if (N > 0 && pr.g.C > 0 && !targets) return accv::fail(ACCV_EINVAL, "%s: null targets pointer", who);
    if (!grad_out || !denom) return accv::fail(ACCV_EINVAL, "%s: null grad_out / denom pointer", who);
    const LossArgs la{targets, weights_or_null, (flags & ACCV_CR_WEIGHTS_PER_CHANNEL) ? 1 : 0, params->beta, grad_out, denom};
    return scatter(who, params->kind, dtype, pr, grads, la, nullptr, static_cast<hipStream_t>(stream_));
}
}
