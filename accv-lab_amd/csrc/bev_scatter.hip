// BEV scatter: from the per-pillar features [rows, C] and their coors to the dense map [B, C, ny, nx] that a 2D backbone
// convolves (mmdet3d's PointPillarsScatter, a Python loop over frames: a zeros canvas, a mask, an index assignment of a
// transposed tensor, a stack), for the whole batch, with the zeros written by the same stores, and its backward.
//
// A row r is placed iff 0 <= b < B, 0 <= y < ny, 0 <= x < nx (b from its coors, or r / V in the padded form); z is ignored.
// index[b, y, x] is the highest placed r of the cell or -1: the last write of the sequential loop, made order-independent.
//   clear    hipMemsetAsync of index to 0xFF bytes.
//   mark     a lane per row: atomicMax(&index[cell], r), a 32-bit vector atomic on global memory.  Max does not depend on
//            the order, so index is a pure function of the inputs.
//   write    a workgroup of kThreads lanes per (frame, map row, kTileW cells along x, kChunk channels), x tiles fastest so
//            that neighbouring workgroups continue each other's channel rows.  Every wave reads the tile's index words (a
//            lane per cell) and ballots: a tile without rows stores zeros and is done.  Otherwise the occupied cells' feature
//            rows are read in 16-byte pieces (the lanes of a piece run along the row: 256 contiguous bytes per 16 lanes in
//            f32), transposed through an LDS tile [channel][cell] whose channel stride is odd in words (kTileW + 1 words in
//            f32: the four 4-byte writes of a piece then spread over all banks, two lanes a bank, which costs a
//            ds_write_b32 nothing), and stored channel-major: kTileW cells = 256 B (f32) per channel row, 16 bytes a lane.
//            Where features, canvas, C * esize or nx * esize is not 16-byte aligned the same is done element by element.
//   backward a lane per 16 bytes (or per element) of grad_features: coors[r] and index[cell] decide between the C values of
//            grad_canvas at the cell (stride ny * nx) and zeros.
// Every element of canvas, index and grad_features is stored exactly once per pass over it (index: the clear, then atomics);
// the canvas is never read, never cleared and sees no atomic; features is not read by the backward.  The copy moves bits:
// f16 and bf16 travel as 16-bit words.  Store-bound in write (the canvas is written once, which is all the bytes that
// count), latency-bound in backward (a sector per 4 bytes gathered).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "accv_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kTileW = 64;      // cells along x a workgroup writes
constexpr int kChunk = 64;      // channels a workgroup writes
constexpr long long kMaxC = ACCV_BS_MAX_C;

struct Args {
    const void* features;     // [rows, C]; backward: null
    const int* coors;         // [rows, cw]
    void* canvas;             // [B, C, ny, nx]; backward: grad_canvas (read)
    int* index;               // [B, ny, nx]
    void* grad_features;      // [rows, C], backward only
    long long rows, V, B, C, ny, nx;
    long long tiles_x, chunks;
    int cw;
};

// the cell of a row, -1 when it is not placed; b is its frame
__host__ __device__ inline long long cell_of(const Args& a, long long r, long long& b)
{
    const int* c = a.coors + r * a.cw;
    b = a.cw == 4 ? (long long)c[0] : r / a.V;
    const long long y = c[a.cw - 2], x = c[a.cw - 1];
    if (b < 0 || b >= a.B || y < 0 || y >= a.ny || x < 0 || x >= a.nx) return -1;
    return (b * a.ny + y) * a.nx + x;
}

// ------------------------------------------------------------------------------------------------------------- device
__global__ __launch_bounds__(kThreads) void bev_mark_kernel(const Args a)
{
    const long long r = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (r >= a.rows) return;
    long long b;
    const long long cell = cell_of(a, r, b);
    if (cell >= 0) atomicMax(&a.index[cell], (int)r);
}

template <class E> struct Piece {       // the elements of 16 bytes
    static constexpr int kPer = 16 / (int)sizeof(E);
    union {
        uint4 v;
        E e[kPer];
    };
};

template <class E, bool kVec>
__global__ __launch_bounds__(kThreads) void bev_write_kernel(const Args a)
{
    constexpr int kPer = Piece<E>::kPer;
    constexpr int kStride = kTileW + 4 / (int)sizeof(E);      // an odd number of 4-byte words
    __shared__ __attribute__((aligned(16))) E s_tile[kChunk * kStride];
    __shared__ int s_idx[kTileW];
    const int tid = threadIdx.x, lane = tid & 63;
    long long id = blockIdx.x;
    const int tx = (int)(id % a.tiles_x);
    id /= a.tiles_x;
    const int chunk = (int)(id % a.chunks);
    id /= a.chunks;
    const long long y = id % a.ny, b = id / a.ny;
    const long long x0 = (long long)tx * kTileW;
    const int c0 = chunk * kChunk;
    const int cells = (int)(a.nx - x0 < kTileW ? a.nx - x0 : kTileW);
    const int chans = (int)(a.C - c0 < kChunk ? a.C - c0 : kChunk);
    const long long plane = a.ny * a.nx;
    const int idx = lane < cells ? a.index[(b * a.ny + y) * a.nx + x0 + lane] : -1;
    const bool any = __ballot(idx >= 0) != 0ull;       // the same in every wave of the workgroup
    E* out = static_cast<E*>(a.canvas) + ((b * a.C + c0) * a.ny + y) * a.nx + x0;
    const E* feat = static_cast<const E*>(a.features);

    if (!any) {
        if (kVec) {
            const int q = cells / kPer;
            for (int u = tid; u < chans * q; u += kThreads) {
                const int ch = u / q, p = u - ch * q;
                *reinterpret_cast<uint4*>(out + ch * plane + p * kPer) = uint4{0u, 0u, 0u, 0u};
            }
        } else {
            for (int u = tid; u < chans * cells; u += kThreads) {
                const int ch = u / cells, cell = u - ch * cells;
                out[ch * plane + cell] = E(0);
            }
        }
        return;
    }
    if (tid < kTileW) s_idx[tid] = idx;
    __syncthreads();
    if (kVec) {
        const int pieces = chans / kPer;
        for (int u = tid; u < cells * pieces; u += kThreads) {
            const int cell = u / pieces, p = u - cell * pieces;
            const int r = s_idx[cell];
            Piece<E> w;
            w.v = uint4{0u, 0u, 0u, 0u};
            if (r >= 0) w.v = *reinterpret_cast<const uint4*>(feat + (long long)r * a.C + c0 + p * kPer);
#pragma unroll
            for (int i = 0; i < kPer; ++i) s_tile[(p * kPer + i) * kStride + cell] = w.e[i];
        }
        __syncthreads();
        const int q = cells / kPer;
        for (int u = tid; u < chans * q; u += kThreads) {
            const int ch = u / q, p = u - ch * q;
            Piece<E> w;
#pragma unroll
            for (int i = 0; i < kPer; ++i) w.e[i] = s_tile[ch * kStride + p * kPer + i];
            *reinterpret_cast<uint4*>(out + ch * plane + p * kPer) = w.v;
        }
    } else {
        for (int u = tid; u < cells * chans; u += kThreads) {
            const int cell = u / chans, ch = u - cell * chans;
            const int r = s_idx[cell];
            s_tile[ch * kStride + cell] = r >= 0 ? feat[(long long)r * a.C + c0 + ch] : E(0);
        }
        __syncthreads();
        for (int u = tid; u < chans * cells; u += kThreads) {
            const int ch = u / cells, cell = u - ch * cells;
            out[ch * plane + cell] = s_tile[ch * kStride + cell];
        }
    }
}

template <class E, bool kVec>
__global__ __launch_bounds__(kThreads) void bev_gather_kernel(const Args a)
{
    constexpr int kPer = kVec ? Piece<E>::kPer : 1;
    const long long per_row = a.C / kPer;
    const long long u = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (u >= a.rows * per_row) return;
    const long long r = u / per_row;
    const int c = (int)(u - r * per_row) * kPer;
    long long b;
    const long long cell = cell_of(a, r, b);
    const bool won = cell >= 0 && a.index[cell] == (int)r;
    const long long plane = a.ny * a.nx;
    const E* g = won ? static_cast<const E*>(a.canvas) + (b * a.C + c) * plane + (cell - b * plane) : nullptr;
    E* out = static_cast<E*>(a.grad_features) + r * a.C + c;
    if (kVec) {
        Piece<E> w;
        w.v = uint4{0u, 0u, 0u, 0u};
        if (won) {
#pragma unroll
            for (int i = 0; i < Piece<E>::kPer; ++i) w.e[i] = g[i * plane];
        }
        *reinterpret_cast<uint4*>(out) = w.v;
    } else {
        *out = won ? *g : E(0);
    }
}

// --------------------------------------------------------------------------------------------------------------- host
// the sequential loop: rows in order, the last one of a cell stays
template <class E>
void host_forward(const Args& a)
{
    const long long plane = a.ny * a.nx;
    for (long long i = 0; i < a.B * plane; ++i) a.index[i] = -1;
    for (long long r = 0; r < a.rows; ++r) {
        long long b;
        const long long cell = cell_of(a, r, b);
        if (cell >= 0) a.index[cell] = (int)r;
    }
    const E* feat = static_cast<const E*>(a.features);
    E* out = static_cast<E*>(a.canvas);
    for (long long b = 0; b < a.B; ++b)
        for (long long c = 0; c < a.C; ++c)
            for (long long i = 0; i < plane; ++i) {
                const int r = a.index[b * plane + i];
                out[(b * a.C + c) * plane + i] = r >= 0 ? feat[(long long)r * a.C + c] : E(0);
            }
}

template <class E>
void host_backward(const Args& a)
{
    const long long plane = a.ny * a.nx;
    const E* g = static_cast<const E*>(a.canvas);
    E* out = static_cast<E*>(a.grad_features);
    for (long long r = 0; r < a.rows; ++r) {
        long long b;
        const long long cell = cell_of(a, r, b);
        const bool won = cell >= 0 && a.index[cell] == (int)r;
        for (long long c = 0; c < a.C; ++c) out[r * a.C + c] = won ? g[(b * a.C + c) * plane + (cell - b * plane)] : E(0);
    }
}

// ------------------------------------------------------------------------------------------------------------- checks
inline uintptr_t addr(const void* p) { return reinterpret_cast<uintptr_t>(p); }

// ACCV_OK with *empty = 1 when there is nothing to write
int check_args(const char* who, const void* dense, const int* coors, const int* index, const void* sparse, bool backward, long long rows,
               long long V, long long B, long long C, long long ny, long long nx, int cw, int esize, Args& a, int* empty)
{
    *empty = 0;
    if (rows < 0 || B < 0 || ny < 0 || nx < 0 || V < 0)
        return accv::fail(ACCV_EINVAL, "%s: negative size (rows %lld, V %lld, B %lld, ny %lld, nx %lld)", who, rows, V, B, ny, nx);
    if (C < 1 || C > kMaxC) return accv::fail(ACCV_EINVAL, "%s: features need 1 <= C <= %lld channels, got %lld", who, kMaxC, C);
    if (esize != 2 && esize != 4) return accv::fail(ACCV_EINVAL, "%s: elem_size must be 2 or 4, got %d", who, esize);
    if (cw != 3 && cw != 4) return accv::fail(ACCV_EINVAL, "%s: coor_width must be 3 or 4, got %d", who, cw);
    if (cw == 3 && rows != B * V) return accv::fail(ACCV_EINVAL, "%s: the padded form needs rows == B * V, got %lld rows for %lld x %lld", who, rows, B, V);
    if (rows > 0x7fffffffll) return accv::fail(ACCV_EINVAL, "%s: %lld rows, fewer than 2^31 supported", who, rows);
    if (ny > 0x7fffffffll || nx > 0x7fffffffll || (double)B * (double)ny * (double)nx >= 2147483648.0)
        return accv::fail(ACCV_EINVAL, "%s: the map has B * ny * nx = %lld * %lld * %lld cells, fewer than 2^31 supported", who, B, ny, nx);
    a.rows = rows, a.V = V, a.B = B, a.C = C, a.ny = ny, a.nx = nx, a.cw = cw;
    a.tiles_x = (nx + kTileW - 1) / kTileW, a.chunks = (C + kChunk - 1) / kChunk;
    const long long cells = B * ny * nx;
    const bool nothing = backward ? rows == 0 : cells == 0;
    if (nothing) {
        *empty = 1;
        return ACCV_OK;
    }
    // a backward over a map without cells reads neither grad_canvas nor index: no row is placed
    if ((cells > 0 && (!dense || !index)) || (rows > 0 && (!coors || !sparse))) return accv::fail(ACCV_EINVAL, "%s: null pointer", who);
    if (!backward && (double)B * (double)ny * (double)a.tiles_x * (double)a.chunks > (double)accv::kGridLimit)
        return accv::fail(ACCV_EINVAL, "%s: %lld x %lld map rows of %lld tiles and %lld channel chunks exceed the grid limit", who, B, ny,
                          a.tiles_x, a.chunks);
    if (((addr(dense) | addr(sparse)) & (uintptr_t)(esize - 1)) || ((addr(coors) | addr(index)) & 3u))
        return accv::fail(ACCV_EINVAL, "%s: a tensor is not aligned to its element size", who);
    if (backward && (rows * C + kThreads - 1) / kThreads > accv::kGridLimit)
        return accv::fail(ACCV_EINVAL, "%s: rows * C = %lld elements exceed the grid limit", who, rows * C);
    a.features = backward ? nullptr : sparse, a.grad_features = backward ? const_cast<void*>(sparse) : nullptr;
    a.coors = coors, a.canvas = const_cast<void*>(dense), a.index = const_cast<int*>(index);
    return ACCV_OK;
}

// 16-byte pieces of the rows and of the map rows line up
inline bool vector_path(const Args& a, const void* sparse, int esize)
{
    return ((addr(a.canvas) | addr(sparse)) & 15u) == 0 && (a.C * esize) % 16 == 0 && (a.nx * esize) % 16 == 0;
}

}  // namespace

extern "C" {

int accv_bev_scatter(const void* features, const int* coors, long long rows, long long V, long long B, long long C, long long ny,
                     long long nx, int coor_width, int elem_size, void* canvas, int* index, void* stream_)
{
    const char* who = "scatter_to_bev";
    Args a;
    int empty;
    if (int rc = check_args(who, canvas, coors, index, features, false, rows, V, B, C, ny, nx, coor_width, elem_size, a, &empty)) return rc;
    if (empty) return ACCV_OK;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const hipError_t e = hipMemsetAsync(index, 0xFF, (size_t)(B * ny * nx) * 4, stream);
    if (e != hipSuccess) return accv::fail(ACCV_ELAUNCH, "%s: %s", who, hipGetErrorString(e));
    if (rows > 0) hipLaunchKernelGGL(bev_mark_kernel, dim3((unsigned)((rows + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, a);
    const dim3 grid((unsigned)(B * ny * a.tiles_x * a.chunks)), block(kThreads);
    const bool vec = vector_path(a, features, elem_size);
    if (elem_size == 4) {
        if (vec) hipLaunchKernelGGL((bev_write_kernel<uint32_t, true>), grid, block, 0, stream, a);
        else hipLaunchKernelGGL((bev_write_kernel<uint32_t, false>), grid, block, 0, stream, a);
    } else {
        if (vec) hipLaunchKernelGGL((bev_write_kernel<uint16_t, true>), grid, block, 0, stream, a);
        else hipLaunchKernelGGL((bev_write_kernel<uint16_t, false>), grid, block, 0, stream, a);
    }
    return accv::check_launch(who);
}

int accv_bev_scatter_cpu(const void* features, const int* coors, long long rows, long long V, long long B, long long C, long long ny,
                         long long nx, int coor_width, int elem_size, void* canvas, int* index)
{
    const char* who = "scatter_to_bev (host)";
    Args a;
    int empty;
    if (int rc = check_args(who, canvas, coors, index, features, false, rows, V, B, C, ny, nx, coor_width, elem_size, a, &empty)) return rc;
    if (empty) return ACCV_OK;
    if (elem_size == 4) host_forward<uint32_t>(a);
    else host_forward<uint16_t>(a);
    return ACCV_OK;
}

int accv_bev_scatter_bwd(const void* grad_canvas, const int* coors, const int* index, long long rows, long long V, long long B,
                         long long C, long long ny, long long nx, int coor_width, int elem_size, void* grad_features, void* stream_)
{
    const char* who = "scatter_to_bev backward";
    Args a;
    int empty;
    if (int rc = check_args(who, grad_canvas, coors, index, grad_features, true, rows, V, B, C, ny, nx, coor_width, elem_size, a, &empty)) return rc;
    if (empty) return ACCV_OK;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const bool vec = (addr(grad_features) & 15u) == 0 && (C * elem_size) % 16 == 0;
    const long long units = rows * (vec ? C / (16 / elem_size) : C);
    const dim3 grid((unsigned)((units + kThreads - 1) / kThreads)), block(kThreads);
    if (elem_size == 4) {
        if (vec) hipLaunchKernelGGL((bev_gather_kernel<uint32_t, true>), grid, block, 0, stream, a);
        else hipLaunchKernelGGL((bev_gather_kernel<uint32_t, false>), grid, block, 0, stream, a);
    } else {
        if (vec) hipLaunchKernelGGL((bev_gather_kernel<uint16_t, true>), grid, block, 0, stream, a);
        else hipLaunchKernelGGL((bev_gather_kernel<uint16_t, false>), grid, block, 0, stream, a);
    }
    return accv::check_launch(who);
}

int accv_bev_scatter_bwd_cpu(const void* grad_canvas, const int* coors, const int* index, long long rows, long long V, long long B,
                             long long C, long long ny, long long nx, int coor_width, int elem_size, void* grad_features)
{
    const char* who = "scatter_to_bev backward (host)";
    Args a;
    int empty;
    if (int rc = check_args(who, grad_canvas, coors, index, grad_features, true, rows, V, B, C, ny, nx, coor_width, elem_size, a, &empty)) return rc;
    if (empty) return ACCV_OK;
    if (elem_size == 4) host_backward<uint32_t>(a);
    else host_backward<uint16_t>(a);
    return ACCV_OK;
}

}  // extern "C"
