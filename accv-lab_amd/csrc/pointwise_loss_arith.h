// The element-wise regression losses shared by matched_loss.hip (matched-pair reduction) and center_regression.hip
// (regression at object centres): l(d) and dl/dd on the difference d = prediction - target, with torch's definitions and
// NaN behaviour (torch.nn.functional.l1_loss / mse_loss / smooth_l1_loss and their autograd).
#pragma once
#include <hip/hip_runtime.h>

namespace accv_loss {

// kinds 0-2: element-wise on d, summed over the row.  3 and 4 are the per-object losses of matched_loss.hip (their
// arithmetic lives there); kOneHotL1 takes the L1 branch here.
enum Kind { kL1 = 0, kL2 = 1, kSmoothL1 = 2, kIoUxyxy = 3, kOneHotL1 = 4 };

template <int KIND, class A>
__device__ __forceinline__ A loss_of(A d, A beta)
{
    const A ad = d < A(0) ? -d : d;
    if (KIND == kL1 || KIND == kOneHotL1) return ad;
    if (KIND == kL2) return d * d;
    return ad < beta ? A(0.5) * d * d / beta : ad - A(0.5) * beta;   // torch.nn.functional.smooth_l1_loss
}
template <int KIND, class A>
__device__ __forceinline__ A dloss_of(A d, A beta)
{
    if (KIND == kL1 || KIND == kOneHotL1) return d > A(0) ? A(1) : (d < A(0) ? A(-1) : A(0));
    if (KIND == kL2) return A(2) * d;
    const A ad = d < A(0) ? -d : d;
    if (d != d) return d;   // NaN, as autograd of smooth_l1_loss gives (L1's sign() gives 0 there, L2's 2 d NaN)
    return ad < beta ? d / beta : (d > A(0) ? A(1) : A(-1));
}

}  // namespace accv_loss
