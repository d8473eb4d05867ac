// Batched linear sum assignment (the Hungarian matching of DETR-style heads) for ragged cost matrices — the per-frame
// scipy.optimize.linear_sum_assignment loop of packages/batching_helpers/example/matcher.py:52-74, on the device.
//
// Algorithm: scipy's (rectangular_lsap.cpp, Crouse 2016): successive shortest augmenting paths, Dijkstra with dual
// potentials u (rows) / v (columns).  A frame of R_b x C_b is solved with n = min(R_b, C_b) solver rows and
// m = max(R_b, C_b) solver columns, transposed when R_b > C_b.  Each of the n augmentations runs Dijkstra steps; a step
// relaxes one solver row against every unvisited column
//
//     r = ((minVal + c[i, j]) - u[i]) - v[j];   if (r < spc[j]) { spc[j] = r; path[j] = i; }
//
// and takes the unvisited column of least (spc[j], tag[j]), tag = (column assigned ? 4096 : 0) + j: among equal costs an
// unassigned column (a sink) first, then the lowest index.  The tag makes the key a total order, so the parallel argmin
// and the serial scan of the host solver pick the same column.  Every value is f64; the reduced cost and the dual
// updates are the same sequence of rounded additions on both sides (contraction off below), so the device and the host
// solver agree bitwise.
//
// Device layout: one workgroup per frame, all solver state in LDS (dynamic, sized by the padded M = max(R, C),
// N = min(R, C)): v, spc (f64), path, row4col (i32), visited SC (u8) per column; u (f64), col4row (i32), visited SR (u8)
// per row — 115 KB at 4096 x 1024.  The workgroup first copies its frame, widened to f64, negated under maximize and in
// solver orientation, into the caller's workspace while it scans for NaN / -inf; after that every Dijkstra step reads one
// contiguous row of m doubles (L2-resident).  Column j belongs to lane j % THREADS for the whole solve, so a step has a
// single barrier: lanes relax and reduce their own columns, wave minima go to a double-buffered LDS slot, and every lane
// reduces the slots itself.  Loops are bounded by construction: n augmentations, at most n steps each (a step that does
// not end in a sink visits a column assigned to one of the < n assigned rows), and a step whose minimum is +inf ends the
// frame as infeasible.  No atomics, no inter-workgroup communication.  The assigned pairs are compacted in ascending row
// order with a ballot scan and written with ordinary stores.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <limits>
#include <mutex>
#include <vector>

#include "accv_common.h"
#include "accv_numeric.h"

#pragma clang fp contract(off)

namespace {

using namespace accv;   // dtype codes, load<DT>, clamp_count

constexpr long long kMaxLarge = 4096;   // max(R, C)
constexpr long long kMaxSmall = 1024;   // min(R, C)
constexpr int kAssignedTag = 4096;      // tag bit of an assigned column (> every column index)
constexpr int kMaxWaves = 16;
constexpr double kInf = std::numeric_limits<double>::infinity();

enum Status { kOk = 0, kInfeasible = 1, kInvalid = 2 };

struct Args {
    const void* cost;
    long long R, C, sb, sr, sc;
    const long long* rows;   // nullable per-frame row counts
    const long long* cols;   // nullable per-frame column counts
    int maximize;
    long long* row_ind;
    long long* col_ind;
    long long* sizes;
    int* status;
    double* ws;
    long long W;   // output width min(R, C)
    int M, N;      // LDS capacity: max(R, C), min(R, C)
};

__host__ __device__ inline double load_cost(const void* p, int dtype, long long off)
{
    switch (dtype) {
        case kF32: return (double)load<kF32>(p, off);
        case kF64: return load<kF64>(p, off);
        case kF16: return (double)load<kF16>(p, off);   // software f16, as the host solver
        default: return (double)load<kBF16>(p, off);
    }
}

// (d, t) < (d2, t2) lexicographically: the argmin order of both solvers
__host__ __device__ inline bool key_less(double d, int t, double d2, int t2)
{
    return d < d2 || (d == d2 && t < t2);
}

size_t lds_bytes(int M, int N)
{
    return (size_t)2 * kMaxWaves * 8 + (size_t)M * 16 + (size_t)N * 8            // reduction d, v, spc, u
           + (size_t)2 * kMaxWaves * 4 + (size_t)kMaxWaves * 4 + (size_t)M * 8 + (size_t)N * 4   // tags, scan, path, row4col, col4row
           + (size_t)M + (size_t)N;                                                // SC, SR
}

template <int THREADS>
__global__ __launch_bounds__(THREADS) void lsa_kernel(Args a, int dtype)
{
    constexpr int NW = THREADS / 64;
    extern __shared__ double lds[];
    double* red_d = lds;                      // [2][kMaxWaves]
    double* v = red_d + 2 * kMaxWaves;        // [M]
    double* spc = v + a.M;                    // [M]
    double* u = spc + a.M;                    // [N]
    int* red_t = reinterpret_cast<int*>(u + a.N);   // [2][kMaxWaves]
    int* scan = red_t + 2 * kMaxWaves;        // [kMaxWaves]
    int* path = scan + kMaxWaves;             // [M]
    int* row4col = path + a.M;                // [M]
    int* col4row = row4col + a.M;             // [N]
    uint8_t* SC = reinterpret_cast<uint8_t*>(col4row + a.N);   // [M]
    uint8_t* SR = SC + a.M;                   // [N]

    const long long b = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int Rb = (int)clamp_count(a.rows, b, a.R);
    const int Cb = (int)clamp_count(a.cols, b, a.C);
    const bool tr = Rb > Cb;
    const int n = tr ? Cb : Rb, m = tr ? Rb : Cb;
    long long* row_out = a.row_ind + b * a.W;
    long long* col_out = a.col_ind + b * a.W;
    double* c = a.ws + b * a.R * a.C;

    // ---- copy the frame into the workspace (f64, solver orientation, negated under maximize) and scan it
    int bad = 0;
    const char* src = static_cast<const char*>(a.cost);
    const int total = Rb * Cb;
    for (int idx = tid; idx < total; idx += THREADS) {
        const int r = idx / Cb, cc = idx - r * Cb;
        double x = load_cost(src, dtype, b * a.sb + (long long)r * a.sr + (long long)cc * a.sc);
        if (a.maximize) x = -x;
        bad |= (x != x) | (x == -kInf);
        c[tr ? (long long)cc * m + r : (long long)r * m + cc] = x;
    }
    __syncthreads();               // the workspace writes are visible to the whole workgroup
    bad = __syncthreads_or(bad);

    int status = bad ? kInvalid : kOk;
    if (status == kOk && n > 0) {
        for (int j = tid; j < m; j += THREADS) v[j] = 0.0, row4col[j] = -1;
        for (int i = tid; i < n; i += THREADS) u[i] = 0.0, col4row[i] = -1;
        int parity = 0;
        for (int cur = 0; cur < n; ++cur) {
            for (int j = tid; j < m; j += THREADS) spc[j] = kInf, SC[j] = 0, path[j] = -1;
            for (int i = tid; i < n; i += THREADS) SR[i] = i == cur;
            __syncthreads();
            double minVal = 0.0;
            int i = cur, sink = -1;
            for (int step = 0; step < n && sink < 0; ++step) {   // <= cur + 1 steps reach a sink
                const double* row = c + (long long)i * m;
                const double ui = u[i];
                double bd = kInf;
                int bt = 0x7fffffff;
                for (int j = tid; j < m; j += THREADS) {
                    if (SC[j]) continue;
                    const double r = minVal + row[j] - ui - v[j];
                    double s = spc[j];
                    if (r < s) spc[j] = s = r, path[j] = i;
                    const int t = (row4col[j] >= 0 ? kAssignedTag : 0) + j;
                    if (key_less(s, t, bd, bt)) bd = s, bt = t;
                }
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) {
                    const double d2 = __shfl_xor(bd, off);
                    const int t2 = __shfl_xor(bt, off);
                    if (key_less(d2, t2, bd, bt)) bd = d2, bt = t2;
                }
                if (lane == 0) red_d[parity * kMaxWaves + wave] = bd, red_t[parity * kMaxWaves + wave] = bt;
                __syncthreads();
                bd = red_d[parity * kMaxWaves], bt = red_t[parity * kMaxWaves];
#pragma unroll
                for (int w = 1; w < NW; ++w) {
                    const double d2 = red_d[parity * kMaxWaves + w];
                    const int t2 = red_t[parity * kMaxWaves + w];
                    if (key_less(d2, t2, bd, bt)) bd = d2, bt = t2;
                }
                parity ^= 1;
                if (bd == kInf) break;   // no finite path: infeasible (uniform across the workgroup)
                const int j = bt & (kAssignedTag - 1);
                minVal = bd;
                if (j % THREADS == tid) SC[j] = 1;   // column j's owner: no other lane touches SC[j]
                const int owner = row4col[j];
                if (owner < 0) {
                    sink = j;
                } else {
                    i = owner;
                    if (tid == 0) SR[i] = 1;
                }
            }
            if (sink < 0) {
                status = kInfeasible;
                break;
            }
            __syncthreads();   // spc / SC / SR of the search are visible to every lane
            for (int r = tid; r < n; r += THREADS) {
                if (r == cur) u[r] += minVal;
                else if (SR[r]) u[r] += minVal - spc[col4row[r]];
            }
            for (int j = tid; j < m; j += THREADS)
                if (SC[j]) v[j] -= minVal - spc[j];
            __syncthreads();   // col4row is read above before the augmentation rewrites it
            if (tid == 0) {
                int j = sink;
                for (int k = 0; k <= n; ++k) {   // the path has at most cur + 1 edges
                    const int r = path[j];
                    row4col[j] = r;
                    const int prev = col4row[r];
                    col4row[r] = j;
                    j = prev;
                    if (r == cur) break;
                }
            }
            __syncthreads();
        }
    }

    // ---- compact the pairs in ascending row order, zero the rest of the output row
    const int size = status == kOk ? n : 0;
    if (size > 0) {
        if (!tr) {
            for (int k = tid; k < n; k += THREADS) row_out[k] = k, col_out[k] = col4row[k];
        } else {
            int base = 0;
            for (int j0 = 0; j0 < m; j0 += THREADS) {
                const int j = j0 + tid;
                const bool f = j < m && row4col[j] >= 0;
                const unsigned long long bits = __ballot(f);
                if (lane == 0) scan[wave] = __popcll(bits);
                __syncthreads();
                int off = base, chunk = 0;
                for (int w = 0; w < NW; ++w) {
                    const int cnt = scan[w];
                    off += w < wave ? cnt : 0;
                    chunk += cnt;
                }
                if (f) {
                    const int pos = off + __popcll(bits & ((1ull << lane) - 1ull));
                    row_out[pos] = j, col_out[pos] = row4col[j];
                }
                base += chunk;
                __syncthreads();   // scan[] is rewritten by the next chunk
            }
        }
    }
    for (long long k = size + tid; k < a.W; k += THREADS) row_out[k] = 0, col_out[k] = 0;
    if (tid == 0) a.sizes[b] = size, a.status[b] = status;
}

// ------------------------------------------------------------------------------------------------ host solver
// The same algorithm, orientation, tie rule and f64 operation sequence as lsa_kernel, one frame at a time.
int solve_host_frame(const double* c, int n, int m, std::vector<double>& v, std::vector<double>& spc,
                     std::vector<double>& u, std::vector<int>& path, std::vector<int>& row4col, std::vector<int>& col4row,
                     std::vector<uint8_t>& SC, std::vector<uint8_t>& SR)
{
    v.assign(m, 0.0), spc.assign(m, kInf), path.assign(m, -1), row4col.assign(m, -1), SC.assign(m, 0);
    u.assign(n, 0.0), col4row.assign(n, -1), SR.assign(n, 0);
    for (int cur = 0; cur < n; ++cur) {
        std::fill(spc.begin(), spc.end(), kInf);
        std::fill(SC.begin(), SC.end(), 0);
        std::fill(path.begin(), path.end(), -1);
        std::fill(SR.begin(), SR.end(), 0);
        SR[cur] = 1;
        double minVal = 0.0;
        int i = cur, sink = -1;
        for (int step = 0; step < n && sink < 0; ++step) {
            const double* row = c + (long long)i * m;
            const double ui = u[i];
            double bd = kInf;
            int bt = 0x7fffffff;
            for (int j = 0; j < m; ++j) {
                if (SC[j]) continue;
                const double r = minVal + row[j] - ui - v[j];
                double s = spc[j];
                if (r < s) spc[j] = s = r, path[j] = i;
                const int t = (row4col[j] >= 0 ? kAssignedTag : 0) + j;
                if (key_less(s, t, bd, bt)) bd = s, bt = t;
            }
            if (bd == kInf) break;
            const int j = bt & (kAssignedTag - 1);
            minVal = bd;
            SC[j] = 1;
            if (row4col[j] < 0) sink = j;
            else i = row4col[j], SR[i] = 1;
        }
        if (sink < 0) return kInfeasible;
        for (int r = 0; r < n; ++r) {
            if (r == cur) u[r] += minVal;
            else if (SR[r]) u[r] += minVal - spc[col4row[r]];
        }
        for (int j = 0; j < m; ++j)
            if (SC[j]) v[j] -= minVal - spc[j];
        int j = sink;
        for (int k = 0; k <= n; ++k) {
            const int r = path[j];
            row4col[j] = r;
            const int prev = col4row[r];
            col4row[r] = j;
            j = prev;
            if (r == cur) break;
        }
    }
    return kOk;
}

int check_args(const char* who, const void* cost, int dtype, long long B, long long R, long long C, unsigned flags,
               const void* row_ind, const void* col_ind, const void* sizes, const void* status)
{
    if (B < 0 || R < 0 || C < 0) return accv::fail(ACCV_EINVAL, "%s: negative extent", who);
    if (dtype < kF32 || dtype > kF64) return accv::fail(ACCV_EINVAL, "%s: unknown dtype code %d", who, dtype);
    if (flags & ~(unsigned)(ACCV_LSA_MAXIMIZE | ACCV_LSA_THREADS_64 | ACCV_LSA_THREADS_1024))
        return accv::fail(ACCV_EINVAL, "%s: unknown flags 0x%x", who, flags);
    const long long lo = R < C ? R : C, hi = R < C ? C : R;
    if (hi > kMaxLarge || lo > kMaxSmall)
        return accv::fail(ACCV_EINVAL, "%s: %lld x %lld frames exceed the limit (max(R, C) <= %lld, min(R, C) <= %lld)",
                          who, R, C, kMaxLarge, kMaxSmall);
    if (B == 0) return ACCV_OK;
    if (!sizes || !status) return accv::fail(ACCV_EINVAL, "%s: null sizes / status pointer", who);
    if (lo > 0 && (!cost || !row_ind || !col_ind)) return accv::fail(ACCV_EINVAL, "%s: null cost / index pointer", who);
    return ACCV_OK;
}

template <int THREADS>
int launch(const Args& a, long long B, int dtype, hipStream_t stream)
{
    static std::once_flag once;
    std::call_once(once, [] {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&lsa_kernel<THREADS>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes(kMaxLarge, kMaxSmall));
    });
    hipLaunchKernelGGL(lsa_kernel<THREADS>, dim3((unsigned)B), dim3(THREADS), lds_bytes(a.M, a.N), stream, a, dtype);
    return accv::check_launch("linear_assignment");
}

}  // namespace

extern "C" {

size_t accv_linear_assignment_workspace_bytes(long long B, long long R, long long C, int dtype)
{
    if (B < 0 || R < 0 || C < 0 || dtype < kF32 || dtype > kF64) return 0;
    if ((R > C ? R : C) > kMaxLarge || (R < C ? R : C) > kMaxSmall) return 0;
    return accv::align_up((size_t)B * (size_t)R * (size_t)C * sizeof(double), 16);
}

int accv_linear_assignment(const void* cost, int dtype, long long B, long long R, long long C, long long stride_b,
                           long long stride_r, long long stride_c, const long long* row_counts,
                           const long long* col_counts, unsigned flags, long long* row_ind, long long* col_ind,
                           long long* sizes, int* status, void* workspace, size_t workspace_bytes, void* stream)
{
    const char* who = "linear_assignment";
    if (int rc = check_args(who, cost, dtype, B, R, C, flags, row_ind, col_ind, sizes, status)) return rc;
    if (B == 0) return ACCV_OK;
    const size_t need = accv_linear_assignment_workspace_bytes(B, R, C, dtype);
    if (need > 0)
        if (int rc = accv::check_workspace(who, workspace, workspace_bytes, need)) return rc;
    Args a;
    a.cost = cost, a.R = R, a.C = C, a.sb = stride_b, a.sr = stride_r, a.sc = stride_c;
    a.rows = row_counts, a.cols = col_counts, a.maximize = (flags & ACCV_LSA_MAXIMIZE) ? 1 : 0;
    a.row_ind = row_ind, a.col_ind = col_ind, a.sizes = sizes, a.status = status;
    a.ws = static_cast<double*>(workspace);
    a.W = R < C ? R : C;
    a.M = (int)(R > C ? R : C), a.N = (int)a.W;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (flags & ACCV_LSA_THREADS_64) return launch<64>(a, B, dtype, s);
    if (flags & ACCV_LSA_THREADS_1024) return launch<1024>(a, B, dtype, s);
    return launch<256>(a, B, dtype, s);
}

int accv_linear_assignment_host(const void* cost, int dtype, long long B, long long R, long long C, long long stride_b,
                                long long stride_r, long long stride_c, const long long* row_counts,
                                const long long* col_counts, unsigned flags, long long* row_ind, long long* col_ind,
                                long long* sizes, int* status)
{
    const char* who = "linear_assignment (host)";
    if (int rc = check_args(who, cost, dtype, B, R, C, flags, row_ind, col_ind, sizes, status)) return rc;
    const long long W = R < C ? R : C;
    const bool maximize = (flags & ACCV_LSA_MAXIMIZE) != 0;
    std::vector<double> c, v, spc, u;
    std::vector<int> path, row4col, col4row;
    std::vector<uint8_t> SC, SR;
    for (long long b = 0; b < B; ++b) {
        const int Rb = (int)clamp_count(row_counts, b, R), Cb = (int)clamp_count(col_counts, b, C);
        const bool tr = Rb > Cb;
        const int n = tr ? Cb : Rb, m = tr ? Rb : Cb;
        c.resize((size_t)Rb * Cb);
        bool bad = false;
        for (int r = 0; r < Rb; ++r)
            for (int cc = 0; cc < Cb; ++cc) {
                double x = load_cost(cost, dtype, b * stride_b + (long long)r * stride_r + (long long)cc * stride_c);
                if (maximize) x = -x;
                bad |= (x != x) || (x == -kInf);
                c[tr ? (size_t)cc * m + r : (size_t)r * m + cc] = x;
            }
        int st = bad ? kInvalid : kOk;
        if (st == kOk && n > 0) st = solve_host_frame(c.data(), n, m, v, spc, u, path, row4col, col4row, SC, SR);
        const int size = st == kOk ? n : 0;
        long long* ro = row_ind + b * W;
        long long* co = col_ind + b * W;
        long long k = 0;
        if (size > 0) {
            if (!tr) {
                for (; k < n; ++k) ro[k] = k, co[k] = col4row[k];
            } else {
                for (int j = 0; j < m; ++j)
                    if (row4col[j] >= 0) ro[k] = j, co[k] = row4col[j], ++k;
            }
        }
        for (; k < W; ++k) ro[k] = 0, co[k] = 0;
        sizes[b] = size;
        status[b] = st;
    }
    return ACCV_OK;
}

}  // extern "C"
