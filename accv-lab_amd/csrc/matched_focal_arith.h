// Per-element arithmetic of the matched sigmoid focal loss (matched_focal.hip): the GPU kernels and the host entry points
// accv_matched_focal_loss_host / _bwd_host evaluate the same operation sequence from these functions.  Contraction into
// fma is off for everything that includes this header, so "product, then sum" means that on both sides; what differs is
// the exp / log1p / pow of the device library against the host's.
//
// With e = exp(-|x|) and r = 1 / (1 + e):  sigmoid(|x|) = r,  sigmoid(-|x|) = e r,  log1p(e) = softplus(-|x|), so
//     s = sigmoid(x), 1 - s, softplus(x) = -log(1 - s) and softplus(-x) = -log(s)
// come without a subtraction of nearly equal numbers (the approach of heatmap_loss.hip and of the focal matching cost).
//   positive element (class == the query's matched label)   alpha       (1 - s)^gamma  softplus(-x)
//   negative element                                        (1 - alpha)  s^gamma       softplus(x)
// alpha < 0: no alpha blend (both coefficients 1).  gamma == 2 runs as a multiplication, other values through pow with
// torch.pow's semantics (x^0 = 1).  The derivative w.r.t. x, with a the base of the power, b = 1 - a, sp the softplus:
//   positive  -alpha       a^gamma (gamma b sp + a)          (a = 1 - s, b = s,     sp = softplus(-x))
//   negative  (1 - alpha)  a^gamma (gamma b sp + a)          (a = s,     b = 1 - s, sp = softplus(x))
// b sp is taken as 0 where b is 0 (its limit; without that an infinite logit would give 0 * inf).  Infinite logits hence
// give: x = +inf negative: loss +inf, gradient 1 - alpha; positive: 0 and -0.  x = -inf positive: loss +inf, gradient
// -alpha; negative: 0 (gamma = 0 included) and 0.  NaN reaches value and gradient of its own element only.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "accv_numeric.h"

#pragma clang fp contract(off)

namespace accv_mf {

using namespace accv;   // dtype codes, Compute<DT>, load / store<DT> (software f16: the host twin runs the same code), m_*

template <class F>
struct Coef {
    F pos, neg;   // alpha and 1 - alpha, or 1 and 1 without the blend
    F gamma;
};

template <class F>
__host__ __device__ inline Coef<F> make_coef(double alpha, double gamma)
{
    Coef<F> k;
    k.pos = alpha >= 0.0 ? (F)alpha : F(1);
    k.neg = alpha >= 0.0 ? (F)(1.0 - alpha) : F(1);
    k.gamma = (F)gamma;
    return k;
}

// what one element needs: the base a of the power, b = 1 - a, the softplus and the coefficient of its side
template <class F>
struct Side {
    F a, b, sp, c;
};

template <class F>
__host__ __device__ inline Side<F> side_of(F x, bool positive, const Coef<F>& k)
{
    const F e = m_exp(-m_abs(x));    // exp(-|x|) in [0, 1]; NaN for NaN
    const F r = F(1) / (F(1) + e);
    const F big = r, small = e * r;  // sigmoid(|x|), sigmoid(-|x|)
    const F l = m_log1p(e);          // softplus(-|x|)
    const bool nonneg = x >= F(0);   // false for NaN, which reaches everything through e
    const F s = nonneg ? big : small, t = nonneg ? small : big;
    const F sp_x = (nonneg ? x : F(0)) + l;     // softplus(x)
    const F sp_mx = (nonneg ? F(0) : -x) + l;   // softplus(-x)
    Side<F> o;
    o.a = positive ? t : s;
    o.b = positive ? s : t;
    o.sp = positive ? sp_mx : sp_x;
    o.c = positive ? k.pos : k.neg;
    return o;
}

template <class F, bool G2>
__host__ __device__ inline F power(F a, F gamma)
{
    if constexpr (G2) return a * a;
    else return m_pow(a, gamma);
}

template <class F, bool G2>
__host__ __device__ inline F focal_value(F x, bool positive, const Coef<F>& k)
{
    const Side<F> o = side_of(x, positive, k);
    return o.c * (power<F, G2>(o.a, k.gamma) * o.sp);
}

template <class F, bool G2>
__host__ __device__ inline F focal_grad(F x, bool positive, const Coef<F>& k)
{
    const Side<F> o = side_of(x, positive, k);
    const F bsp = o.b == F(0) ? F(0) : o.b * o.sp;
    const F g = o.c * (power<F, G2>(o.a, k.gamma) * (k.gamma * bsp + o.a));
    return positive ? -g : g;
}

}  // namespace accv_mf
