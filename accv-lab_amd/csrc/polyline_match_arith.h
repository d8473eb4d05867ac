// Per-pair arithmetic of the polyline matching cost and the matched polyline loss (polyline_match.hip): the equivalent
// orders of a ground-truth line, the point-wise L1 sum over one order, the search for the best order, the direction
// (cosine) term of a segment and its derivative.  The GPU kernels and the host entry points evaluate the same operation
// sequence from these functions; contraction into fma is off for everything that includes this header.
//
// Orders of a ground-truth line t of P points (variant v, point p -> index into t):
//   open     v = 0: p                      v = 1 (reversible): P - 1 - p
//   closed   v = s < P: (s + p) mod P      v = P + s (reversible): (s - p) mod P, the mathematical modulus
// so V is 1, 2, P or 2 P.  The best order is the LOWEST v that minimises the L1 sum in the arithmetic type (strict <
// in ascending v); a NaN sum is NaN in every order and leaves v = 0.
//
// L1 sum: |x[p, d] - t^v[p, d]| over p, d in order, in partial sums of kBlockPts points that are then added up: a chain of
// at most kBlockPts * D + P / kBlockPts additions instead of P * D, which keeps a float32 sum of 384 terms well inside
// 1e-5 relative.
//
// Direction term of segment s (a = x[s+1] - x[s], b = t*[s+1] - t*[s]; s + 1 taken mod P for a closed line), in double:
//   1 - <a, b> / sqrt((|a|^2 + eps) (|b|^2 + eps)),  its derivative w.r.t. a:  -(b / den - <a, b> (|b|^2 + eps) a / den^3)
#pragma once
#include "matched_box_arith.h"

#pragma clang fp contract(off)

namespace accv_pm {

using namespace accv_mb;   // sign_of; through accv_mc the class term; through accv dtype codes, Compute<DT>, load / store<DT>, m_*

constexpr int kMinP = 2, kMaxP = 128;
constexpr int kBlockPts = 8;

__host__ __device__ inline int num_variants(int P, int closed, int reversible)
{
    return closed ? (reversible ? 2 * P : P) : (reversible ? 2 : 1);
}

// index into the ground-truth line of point p in order v
__host__ __device__ inline int variant_point(int v, int p, int P, int closed)
{
    if (!closed) return v ? P - 1 - p : p;
    if (v < P) {
        const int i = v + p;
        return i >= P ? i - P : i;
    }
    const int i = v - P - p;
    return i < 0 ? i + P : i;
}

__host__ __device__ inline int num_segments(int P, int closed) { return closed ? P : P - 1; }

// a row of P * D numbers in memory of dtype DT, widened on access
template <int DT>
struct Row {
    const void* base;
    long long off;
    __host__ __device__ typename Compute<DT>::type operator()(int i) const { return load<DT>(base, off + i); }
};
// the same, already in the arithmetic type (LDS, host copies)
template <class F>
struct Plain {
    const F* base;
    __host__ __device__ F operator()(int i) const { return base[i]; }
};

// the blocked sum: add() every term in order, end_point() after the last coordinate of point p, value() at the end
template <class F>
struct L1Acc {
    F total = F(0), part = F(0);
    __host__ __device__ void add(F v) { part = part + v; }
    __host__ __device__ void end_point(int p)
    {
        if ((p & (kBlockPts - 1)) == kBlockPts - 1) total = total + part, part = F(0);
    }
    __host__ __device__ F value() const { return total + part; }
};

// sum_{p, d} |x[p, d] - t^v[p, d]|
template <class F, class X, class T>
__host__ __device__ inline F variant_sum(const X& x, const T& t, int v, int P, int D, int closed)
{
    L1Acc<F> acc;
    for (int p = 0; p < P; ++p) {
        const int i = variant_point(v, p, P, closed);
        for (int d = 0; d < D; ++d) acc.add(m_abs(x(p * D + d) - t(i * D + d)));
        acc.end_point(p);
    }
    return acc.value();
}

// the best order and its sum, one order after the other
template <class F, class X, class T>
__host__ __device__ inline int best_variant(const X& x, const T& t, int V, int P, int D, int closed, F& best)
{
    int bv = 0;
    best = variant_sum<F>(x, t, 0, P, D, closed);
    for (int v = 1; v < V; ++v) {
        const F s = variant_sum<F>(x, t, v, P, D, closed);
        if (s < best) best = s, bv = v;
    }
    return bv;
}

// sum_d |x[p, d] - t^v[p, d]| of one point
template <class F, class X, class T>
__host__ __device__ inline F point_l1(const X& x, const T& t, int v, int p, int P, int D, int closed)
{
    const int i = variant_point(v, p, P, closed);
    F acc = F(0);
    for (int d = 0; d < D; ++d) acc = acc + m_abs(x(p * D + d) - t(i * D + d));
    return acc;
}

// The direction term is evaluated in double for every dtype: for nearly parallel segments, which is what a matched pair
// has, 1 - cos cancels to a few 1e-5 and a float evaluation keeps two digits of it.  The inputs widen exactly.
// a = x[s+1] - x[s], b = t^v[s+1] - t^v[s] of segment s (D <= 3)
template <class X, class T>
__host__ __device__ inline void segment(const X& x, const T& t, int v, int s, int P, int D, int closed, double* a, double* b)
{
    const int s1 = s + 1 == P ? 0 : s + 1;   // only a closed line has segment P - 1
    const int i0 = variant_point(v, s, P, closed), i1 = variant_point(v, s1, P, closed);
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        a[d] = d < D ? (double)x(s1 * D + d) - (double)x(s * D + d) : 0.0;
        b[d] = d < D ? (double)t(i1 * D + d) - (double)t(i0 * D + d) : 0.0;
    }
}

__host__ __device__ inline void dir_parts(const double* a, const double* b, double eps, double& dot, double& nb, double& den)
{
    dot = (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
    const double na = ((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]) + eps;
    nb = ((b[0] * b[0] + b[1] * b[1]) + b[2] * b[2]) + eps;
    den = sqrt(na * nb);
}

// 1 - cos(a, b) with the floor eps under both squared lengths
__host__ __device__ inline double dir_value(const double* a, const double* b, double eps)
{
    double dot, nb, den;
    dir_parts(a, b, eps, dot, nb, den);
    return 1.0 - dot / den;
}

// its derivative with respect to a
__host__ __device__ inline void dir_grad(const double* a, const double* b, double eps, double* g)
{
    double dot, nb, den;
    dir_parts(a, b, eps, dot, nb, den);
    const double k = dot * nb / (den * den * den);
#pragma unroll
    for (int d = 0; d < 3; ++d) g[d] = k * a[d] - b[d] / den;
}

// the gradient of one point of a matched prediction: s1 * d pts / d x[p, d] + s2 * d dir / d x[p, d], d < D, the sum formed
// in double and rounded to the arithmetic type.  A term whose switch is off is not evaluated.
template <class F, class X, class T>
__host__ __device__ inline void point_grad(const X& x, const T& t, int v, int p, int P, int D, int closed, bool pts, F s1,
                                           bool dir, double s2, double eps, F* out)
{
    out[0] = out[1] = out[2] = F(0);
    if (pts) {
        const int i = variant_point(v, p, P, closed);
#pragma unroll
        for (int d = 0; d < 3; ++d)
            if (d < D) out[d] = s1 * sign_of(x(p * D + d) - t(i * D + d));
    }
    if (dir) {
        double dd[3] = {0.0, 0.0, 0.0}, a[3], b[3], g[3];
        if (closed || p >= 1) {           // the segment that ends at p
            segment(x, t, v, p >= 1 ? p - 1 : P - 1, P, D, closed, a, b);
            dir_grad(a, b, eps, g);
#pragma unroll
            for (int d = 0; d < 3; ++d) dd[d] = dd[d] + g[d];
        }
        if (closed || p <= P - 2) {       // the segment that starts at p
            segment(x, t, v, p, P, D, closed, a, b);
            dir_grad(a, b, eps, g);
#pragma unroll
            for (int d = 0; d < 3; ++d) dd[d] = dd[d] - g[d];
        }
#pragma unroll
        for (int d = 0; d < 3; ++d)
            if (d < D) out[d] = (F)((double)out[d] + s2 * dd[d]);
    }
}

}  // namespace accv_pm
