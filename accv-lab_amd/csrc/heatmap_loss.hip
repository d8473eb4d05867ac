// Gaussian focal loss on a drawn heat-map target — the consumer the draw_heatmap maps are made for
// (packages/draw_heatmap/docs/intro.rst:7-25, the GaussianFocalLoss centerness term of CenterPoint-style heads):
//
//   p   = clamp(sigmoid(x), eps, 1 - eps)                    (eps = 0: no clamp)
//   l   = pos_weight * [t == 1] * -log(p + 1e-12) * (1 - p)^alpha
//       + neg_weight *            -log(1 - p + 1e-12) * p^alpha * (1 - t)^gamma
//   out = sum(l) / denom,  denom = max(#{t == 1}, 1) or a caller-given factor (host value or device scalar)
//
// Forward: a grid-stride streaming reduction, 16-byte loads per lane (float4 of f32 logits; 8 f16 / bf16 logits as one
// 16-byte load with their targets as two float4), f32 arithmetic per element, a double accumulator per thread, wave shuffle
// + LDS tree per block into a per-block slot of the caller's workspace (partial sum, integer positive count), then a second
// one-block launch that sums the slots in a FIXED order and writes loss and denominator.  No atomics: the grid depends on
// numel alone, so the result is bitwise reproducible from run to run.  Backward: element-wise, reads logits, target and the
// two device scalars (grad_out, denom), writes the gradient once in the logits dtype.  Bandwidth work: no MFMA.
//
// 1 - sigmoid(x) is computed from exp(-|x|) directly (not as 1 - p in f32), so log(1 - p) and the sigmoid derivative keep
// their relative precision where the sigmoid saturates; the clamp tests compare that accurate value against eps.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "accv_common.h"
#include "accv_numeric.h"

namespace {

using namespace accv;   // dtype codes (f64 is not taken here), decode / encode, block_sum, denominator

constexpr int kThreads = 256;
constexpr long long kMaxBlocks = 2048;          // 8 workgroups per CU: the forward grid and the workspace slots
constexpr float kLogEps = 1e-12f;

struct FocalParams {
    float alpha, gamma, pos_weight, neg_weight, clamp_eps;
};

template <int VEC>
__device__ __forceinline__ void load_target(const float* __restrict__ t, long long c, float (&y)[VEC])
{
    const float4* v = reinterpret_cast<const float4*>(t) + c * (VEC / 4);
#pragma unroll
    for (int k = 0; k < VEC / 4; ++k) {
        const float4 q = v[k];
        y[4 * k] = q.x, y[4 * k + 1] = q.y, y[4 * k + 2] = q.z, y[4 * k + 3] = q.w;
    }
}

// natural log / exp on the hardware's log2 / exp2 (v_log_f32 / v_exp_f32, about 1 ulp)
__device__ __forceinline__ float fast_log(float v) { return __builtin_amdgcn_logf(v) * 0.69314718055994531f; }
__device__ __forceinline__ float fast_exp(float v) { return __builtin_amdgcn_exp2f(v * 1.44269504088896341f); }

// Powers: alpha = 2, gamma = 4 (INT_POW) are spelled out as multiplications; any other exponent goes through powf, which
// has torch.pow's semantics for them (x^0 = 1 also for x = 0, integer exponents of negative bases) — and then both terms
// are evaluated, since gamma = 0 leaves the negative term alive at a positive.

// One element: p and q = 1 - p after the clamp, whether the clamp lets the gradient through, and
// s (1 - s) of the unclamped sigmoid.
struct Sig {
    float p, q, dsig;
    bool pass;
};
__device__ __forceinline__ Sig sigmoid_clamped(float x, float eps)
{
    const float e = fast_exp(-fabsf(x));           // exp(-|x|) in (0, 1]
    const float r = __builtin_amdgcn_rcpf(1.0f + e);
    const float big = r, small = e * r;            // sigmoid(|x|), sigmoid(-|x|)
    const float s = x >= 0.0f ? big : small, q = x >= 0.0f ? small : big;
    Sig o;
    o.dsig = big * small;
    o.pass = s >= eps && q >= eps;                 // torch.clamp passes gradient on eps <= s <= 1 - eps (inclusive)
    o.p = s < eps ? eps : (q < eps ? 1.0f - eps : s);
    o.q = s < eps ? 1.0f - eps : (q < eps ? eps : q);
    return o;
}

// alpha = 2, gamma = 4.  gamma > 0 makes (1 - t)^gamma = 0 at a positive, so exactly one of the two terms is non-zero per
// element and one log (one reciprocal for the gradient) serves it:  with a = 1 - p, c = pos_weight at a positive and
// a = p, c = neg_weight (1 - t)^4 elsewhere,  l = -c log(a' + 1e-12) a^2  where a' is the other one of p, 1 - p.
struct IntPowTerm {
    float a, arg, c, sign;   // sign of dl/dp: -1 at a positive, +1 elsewhere
};
__device__ __forceinline__ IntPowTerm int_pow_term(const Sig& z, float t, const FocalParams& f)
{
    const bool pos = t == 1.0f;
    const float w = 1.0f - t, w2 = w * w;
    IntPowTerm o;
    o.a = pos ? z.q : z.p;
    o.arg = (pos ? z.p : z.q) + kLogEps;
    o.c = pos ? f.pos_weight : f.neg_weight * (w2 * w2);
    o.sign = pos ? -1.0f : 1.0f;
    return o;
}

template <bool INT_POW>
__device__ __forceinline__ float focal_value(float x, float t, const FocalParams& f)
{
    const Sig z = sigmoid_clamped(x, f.clamp_eps);
    if constexpr (INT_POW) {
        const IntPowTerm m = int_pow_term(z, t, f);
        return -fast_log(m.arg) * (m.c * (m.a * m.a));
    } else {
        const float lp = fast_log(z.p + kLogEps), lq = fast_log(z.q + kLogEps);
        const float pos = t == 1.0f ? -lp * powf(z.q, f.alpha) : 0.0f;
        const float neg = -lq * powf(z.p, f.alpha) * powf(1.0f - t, f.gamma);
        return f.pos_weight * pos + f.neg_weight * neg;
    }
}

// d loss_element / d x (before the 1 / denom and grad_out scale)
template <bool INT_POW>
__device__ __forceinline__ float focal_grad(float x, float t, const FocalParams& f)
{
    const Sig z = sigmoid_clamped(x, f.clamp_eps);
    // the clamp passes no gradient outside [eps, 1 - eps], but a NaN logit fails both comparisons: autograd multiplies
    // that zero by the NaN sigmoid derivative, so the element's gradient is NaN (and AMP's inf / NaN check sees it)
    if (!z.pass) return x != x ? x : 0.0f;
    if constexpr (INT_POW) {
        // at a positive (a = 1 - p):  d/dp [-log(p + 1e-12) (1 - p)^2] = -[(1 - p)^2 / (p + 1e-12) - 2 (1 - p) log(p + 1e-12)]
        // elsewhere (a = p):          d/dp [-log(1 - p + 1e-12) p^2] = +[p^2 / (1 - p + 1e-12) - 2 p log(1 - p + 1e-12)]
        const IntPowTerm m = int_pow_term(z, t, f);
        const float l = fast_log(m.arg), r = __builtin_amdgcn_rcpf(m.arg);
        return m.sign * m.c * (m.a * (m.a * r - 2.0f * l)) * z.dsig;
    } else {
        const float pc = z.p + kLogEps, qc = z.q + kLogEps;
        const float lp = fast_log(pc), lq = fast_log(qc);
        const float qa = powf(z.q, f.alpha), qa1 = f.alpha * powf(z.q, f.alpha - 1.0f);
        const float pa = powf(z.p, f.alpha), pa1 = f.alpha * powf(z.p, f.alpha - 1.0f);
        // d/dp [-log(p + c) (1 - p)^a] = -(1 - p)^a / (p + c) + a (1 - p)^(a-1) log(p + c)
        const float dpos = t == 1.0f ? -qa / pc + qa1 * lp : 0.0f;
        // d/dp [-log(1 - p + c) p^a] = p^a / (1 - p + c) - a p^(a-1) log(1 - p + c)
        const float dneg = (pa / qc - pa1 * lq) * powf(1.0f - t, f.gamma);
        return (f.pos_weight * dpos + f.neg_weight * dneg) * z.dsig;
    }
}

long long fwd_blocks(long long numel)
{
    const long long b = (numel + 2047) / 2048;
    return b < 1 ? 1 : (b > kMaxBlocks ? kMaxBlocks : b);
}

template <int DT, bool INT_POW>
__global__ __launch_bounds__(kThreads) void focal_fwd_kernel(const void* __restrict__ logits, const float* __restrict__ target,
                                                             long long numel, int vec_ok, FocalParams f,
                                                             double* __restrict__ part_sum,
                                                             unsigned long long* __restrict__ part_pos)
{
    constexpr int VEC = 16 / elem_size(DT);   // 16 bytes of logits per lane, widened to f32 (hardware f16 conversion)
    double acc = 0.0;
    unsigned npos = 0;
    const long long tid = (long long)blockIdx.x * kThreads + threadIdx.x, stride = (long long)gridDim.x * kThreads;
    const long long nchunks = vec_ok ? numel / VEC : 0;
    auto chunk = [&](const float (&x)[VEC], const float (&y)[VEC]) {
        float s = 0.0f;
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            s += focal_value<INT_POW>(x[k], y[k], f);
            npos += y[k] == 1.0f;
        }
        acc += (double)s;
    };
    long long c = tid;
    for (; c + stride < nchunks; c += 2 * stride) {   // two chunks in flight per lane
        float x0[VEC], y0[VEC], x1[VEC], y1[VEC];
        decode<DT, kHwF16>(static_cast<const uint4*>(logits)[c], x0);
        load_target<VEC>(target, c, y0);
        decode<DT, kHwF16>(static_cast<const uint4*>(logits)[c + stride], x1);
        load_target<VEC>(target, c + stride, y1);
        chunk(x0, y0);
        chunk(x1, y1);
    }
    if (c < nchunks) {
        float x0[VEC], y0[VEC];
        decode<DT, kHwF16>(static_cast<const uint4*>(logits)[c], x0);
        load_target<VEC>(target, c, y0);
        chunk(x0, y0);
    }
    // the tail (and every element when the pointers are not 16-byte aligned), one element per lane
    for (long long i = nchunks * VEC + tid; i < numel; i += stride) {
        const float y = target[i];
        acc += (double)focal_value<INT_POW>(load<DT, kHwF16>(logits, i), y, f);
        npos += y == 1.0f;
    }

    unsigned long long cnt = npos;
    block_sum<double, unsigned long long, kThreads>(acc, cnt);
    if (threadIdx.x == 0) part_sum[blockIdx.x] = acc, part_pos[blockIdx.x] = cnt;
}

// one workgroup: the block slots in a fixed order -> loss, denominator
__global__ __launch_bounds__(kThreads) void focal_finish_kernel(const double* __restrict__ part_sum,
                                                                const unsigned long long* __restrict__ part_pos, int nparts,
                                                                int avg_mode, float avg_value, const float* __restrict__ avg_dev,
                                                                float* __restrict__ out_loss, float* __restrict__ out_denom)
{
    double acc = 0.0;
    unsigned long long cnt = 0;
    for (int i = threadIdx.x; i < nparts; i += kThreads) acc += part_sum[i], cnt += part_pos[i];
    block_sum<double, unsigned long long, kThreads>(acc, cnt);
    if (threadIdx.x == 0) {
        const float denom = denominator(avg_mode, avg_value, avg_dev, cnt);   // pos.sum().clamp(min=1), as float32
        *out_loss = (float)(acc / (double)denom);
        *out_denom = denom;
    }
}

template <int DT, bool INT_POW>
__global__ __launch_bounds__(kThreads) void focal_bwd_kernel(const void* __restrict__ logits, const float* __restrict__ target,
                                                             long long numel, int vec_ok, FocalParams f,
                                                             const float* __restrict__ grad_out,
                                                             const float* __restrict__ denom, void* __restrict__ grad)
{
    constexpr int VEC = 16 / elem_size(DT);   // 16 bytes of logits per lane, widened to f32 (hardware f16 conversion)
    const float scale = *grad_out / *denom;
    const long long tid = (long long)blockIdx.x * kThreads + threadIdx.x, stride = (long long)gridDim.x * kThreads;
    const long long nchunks = vec_ok ? numel / VEC : 0;
    auto chunk = [&](long long cc, const float (&x)[VEC], const float (&y)[VEC]) {
        float g[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) g[k] = scale * focal_grad<INT_POW>(x[k], y[k], f);
        static_cast<uint4*>(grad)[cc] = encode<DT, kHwF16>(g);
    };
    long long c = tid;
    for (; c + stride < nchunks; c += 2 * stride) {
        float x0[VEC], y0[VEC], x1[VEC], y1[VEC];
        decode<DT, kHwF16>(static_cast<const uint4*>(logits)[c], x0);
        load_target<VEC>(target, c, y0);
        decode<DT, kHwF16>(static_cast<const uint4*>(logits)[c + stride], x1);
        load_target<VEC>(target, c + stride, y1);
        chunk(c, x0, y0);
        chunk(c + stride, x1, y1);
    }
    if (c < nchunks) {
        float x0[VEC], y0[VEC];
        decode<DT, kHwF16>(static_cast<const uint4*>(logits)[c], x0);
        load_target<VEC>(target, c, y0);
        chunk(c, x0, y0);
    }
    for (long long i = nchunks * VEC + tid; i < numel; i += stride)
        store<DT, kHwF16>(grad, i, scale * focal_grad<INT_POW>(load<DT, kHwF16>(logits, i), target[i], f));
}

int check_args(const char* who, const void* logits, const void* target, long long numel, int dtype, const FocalParams& f)
{
    if (numel < 0) return accv::fail(ACCV_EINVAL, "%s: negative numel %lld", who, numel);
    if (dtype < kF32 || dtype > kBF16)
        return accv::fail(ACCV_EINVAL, "%s: unknown logits dtype code %d (0 f32, 1 f16, 2 bf16)", who, dtype);
    if (!(f.alpha >= 1.0f) || !(f.gamma >= 0.0f))
        return accv::fail(ACCV_EINVAL, "%s: needs alpha >= 1 and gamma >= 0 (got %g, %g)", who, f.alpha, f.gamma);
    if (!(f.clamp_eps >= 0.0f && f.clamp_eps < 0.5f))
        return accv::fail(ACCV_EINVAL, "%s: needs 0 <= clamp_eps < 0.5 (got %g)", who, f.clamp_eps);
    if (numel > 0 && (!logits || !target)) return accv::fail(ACCV_EINVAL, "%s: null logits / target pointer", who);
    return ACCV_OK;
}

// 16-byte vectors need 16-byte aligned logits and target; otherwise every element goes through the scalar loop
int vectors_ok(const void* logits, const void* target, const void* grad = nullptr)
{
    const uintptr_t bits = reinterpret_cast<uintptr_t>(logits) | reinterpret_cast<uintptr_t>(target) |
                           reinterpret_cast<uintptr_t>(grad);
    return (bits & 15u) == 0;
}

bool int_pow(const FocalParams& f) { return f.alpha == 2.0f && f.gamma == 4.0f; }

template <int DT>
void launch_fwd(bool ip, dim3 grid, hipStream_t stream, const void* x, const float* t, long long n, int vec, const FocalParams& f,
                double* ps, unsigned long long* pp)
{
    if (ip) hipLaunchKernelGGL((focal_fwd_kernel<DT, true>), grid, dim3(kThreads), 0, stream, x, t, n, vec, f, ps, pp);
    else hipLaunchKernelGGL((focal_fwd_kernel<DT, false>), grid, dim3(kThreads), 0, stream, x, t, n, vec, f, ps, pp);
}

template <int DT>
void launch_bwd(bool ip, dim3 grid, hipStream_t stream, const void* x, const float* t, long long n, int vec, const FocalParams& f,
                const float* go, const float* den, void* g)
{
    if (ip) hipLaunchKernelGGL((focal_bwd_kernel<DT, true>), grid, dim3(kThreads), 0, stream, x, t, n, vec, f, go, den, g);
    else hipLaunchKernelGGL((focal_bwd_kernel<DT, false>), grid, dim3(kThreads), 0, stream, x, t, n, vec, f, go, den, g);
}

}  // namespace

extern "C" {

size_t accv_gaussian_focal_loss_workspace_bytes(long long numel)
{
    if (numel <= 0) return 0;
    return accv::align_up((size_t)fwd_blocks(numel) * (sizeof(double) + sizeof(unsigned long long)), 16);
}

int accv_gaussian_focal_loss(const void* logits, const float* target, long long numel, int dtype, float alpha, float gamma,
                             float pos_weight, float neg_weight, float clamp_eps, int avg_mode, float avg_factor,
                             const float* avg_factor_dev, float* out_loss, float* out_denom, void* workspace,
                             size_t workspace_bytes, void* stream_)
{
    const char* who = "gaussian_focal_loss";
    const FocalParams f{alpha, gamma, pos_weight, neg_weight, clamp_eps};
    if (int rc = check_args(who, logits, target, numel, dtype, f)) return rc;
    if (avg_mode < ACCV_FL_AVG_NUM_POS || avg_mode > ACCV_FL_AVG_DEVICE)
        return accv::fail(ACCV_EINVAL, "%s: unknown avg_factor mode %d", who, avg_mode);
    if (numel == 0) return ACCV_OK;
    if (!out_loss || !out_denom) return accv::fail(ACCV_EINVAL, "%s: null output pointer", who);
    if (avg_mode == ACCV_FL_AVG_DEVICE && !avg_factor_dev) return accv::fail(ACCV_EINVAL, "%s: null avg_factor pointer", who);
    const size_t need = accv_gaussian_focal_loss_workspace_bytes(numel);
    if (int rc = accv::check_workspace(who, workspace, workspace_bytes, need)) return rc;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const long long blocks = fwd_blocks(numel);
    double* ps = static_cast<double*>(workspace);
    unsigned long long* pp = reinterpret_cast<unsigned long long*>(ps + blocks);
    const int vec = vectors_ok(logits, target);
    const dim3 grid((unsigned)blocks);
    const bool ip = int_pow(f);
    switch (dtype) {
        case kF32: launch_fwd<kF32>(ip, grid, stream, logits, target, numel, vec, f, ps, pp); break;
        case kF16: launch_fwd<kF16>(ip, grid, stream, logits, target, numel, vec, f, ps, pp); break;
        default: launch_fwd<kBF16>(ip, grid, stream, logits, target, numel, vec, f, ps, pp); break;
    }
    if (int rc = accv::check_launch(who)) return rc;
    hipLaunchKernelGGL(focal_finish_kernel, dim3(1), dim3(kThreads), 0, stream, ps, pp, (int)blocks, avg_mode, avg_factor,
                       avg_factor_dev, out_loss, out_denom);
    return accv::check_launch(who);
}

int accv_gaussian_focal_loss_bwd(const void* logits, const float* target, long long numel, int dtype, float alpha, float gamma,
                                 float pos_weight, float neg_weight, float clamp_eps, const float* grad_out,
                                 const float* denom, void* grad_logits, void* stream_)
{
    const char* who = "gaussian_focal_loss_bwd";
    const FocalParams f{alpha, gamma, pos_weight, neg_weight, clamp_eps};
    if (int rc = check_args(who, logits, target, numel, dtype, f)) return rc;
    if (numel == 0) return ACCV_OK;
    if (!grad_out || !denom || !grad_logits) return accv::fail(ACCV_EINVAL, "%s: null grad_out / denom / gradient pointer", who);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const int vec = vectors_ok(logits, target, grad_logits);
    const long long per_block = (long long)kThreads * (16 / elem_size(dtype)) * 2;   // two vectors per lane per pass
    long long blocks = (numel + per_block - 1) / per_block;
    blocks = blocks > 4 * kMaxBlocks ? 4 * kMaxBlocks : blocks;
    const dim3 grid((unsigned)blocks);
    const bool ip = int_pow(f);
    switch (dtype) {
        case kF32: launch_bwd<kF32>(ip, grid, stream, logits, target, numel, vec, f, grad_out, denom, grad_logits); break;
        case kF16: launch_bwd<kF16>(ip, grid, stream, logits, target, numel, vec, f, grad_out, denom, grad_logits); break;
        default: launch_bwd<kBF16>(ip, grid, stream, logits, target, numel, vec, f, grad_out, denom, grad_logits); break;
    }
    return accv::check_launch(who);
}
}
