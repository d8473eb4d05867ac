// Per-object arithmetic of the centre-point target encoder (center_targets.hip): mmdet3d's CenterHead.get_targets_single
// for one ground-truth box.  The GPU kernel and the host entry accv_center_point_targets_host evaluate the same operation
// sequence from these functions.  Everything is float32; contraction into fma is off for everything that includes this
// header; every `/` below is ONE correctly rounded division and every sqrt ONE correctly rounded square root, every other
// operator one IEEE operation, evaluated exactly as parenthesised here.  Division: __fdiv_rn on the device, `/` on the
// host.  Square root: sqrtf on both sides; hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt expands it on the device
// to v_sqrt_f32 plus the two-candidate fma fix-up (the library must not be built with that option off).  __fsqrt_rn is NOT
// used: in this ROCm it is the native 1-ulp root unless OCML_BASIC_ROUNDED_OPERATIONS is defined.  Decisions are comparisons
// only, so NaN fails all of them.
//
// Constants (rounded once to float32 from the caller's numbers): pc0, pc1 = pc_range[0], [1]; vs0, vs1 = voxel_size[0],
// [1]; f = out_size_factor; m = gaussian_overlap; omm = 1 - m; opm = 1 + m; Wf, Hf = (float)W, (float)H.
//
//   scaling    w  = (dx / vs0) / f            l  = (dy / vs1) / f
//              cx = ((x - pc0) / vs0) / f     cy = ((y - pc1) / vs1) / f
//   validity   w > 0 && l > 0 && cx > -1 && cx < Wf && cy > -1 && cy < Hf
//   cell       ix = (int)cx, iy = (int)cy     truncated toward zero: a centre in (-1, 0) lands in cell 0
//   radius     CenterPoint's / CornerNet's gaussian_radius((l, w), m):
//              s   = l + w
//              c1  = ((w * l) * omm) / opm        sq1 = sqrt(s * s - 4 * c1)                  r1 = (s + sq1) / 2
//              b2  = 2 * s     c2 = (omm * w) * l sq2 = sqrt(b2 * b2 - 16 * c2)               r2 = (b2 + sq2) / 2
//              a3  = 4 * m     b3 = (-2 * m) * s  c3 = ((m - 1) * w) * l
//                                                 sq3 = sqrt(b3 * b3 - (4 * a3) * c3)         r3 = (b3 + sq3) / 2
//              rm  = r1; if (r2 < rm) rm = r2; if (r3 < rm) rm = r3
//              radius = max(min_radius, to_int(rm))
//              to_int truncates toward zero and is total: NaN -> 0, rm >= 2^31 -> INT_MAX, rm <= -2^31 -> INT_MIN (a box
//              of infinite extent has rm = NaN and gets min_radius)
//   target     (cx - (float)ix, cy - (float)iy, z, dims, sin(yaw), cos(yaw)[, vx, vy]) with dims = (dx, dy, dz), or
//              (log dx, log dy, log dz) under norm_bbox; z, the raw dims and the velocity are bit copies; log / sin / cos are
//              logf / sinf / cosf of the platform (device and host agree to a few ulp, not bit for bit)
#pragma once
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>

#pragma clang fp contract(off)

namespace accv_ct {

constexpr int kMaxTasks = 8;      // ACCV_CT_MAX_TASKS
constexpr int kMaxClasses = 64;   // ACCV_CT_MAX_CLASSES
constexpr int kNoTask = 255;

// the constants of a call, rounded to float32 once on the host
struct Consts {
    float pc0, pc1, vs0, vs1, f, m, omm, opm, Wf, Hf;
    int min_radius, norm_bbox;
};

__host__ __device__ inline float div_rn(float a, float b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __fdiv_rn(a, b);
#else
    return a / b;
#endif
}

// correctly rounded on the host (libm) and on the device (see the header comment)
__host__ __device__ inline float sqrt_rn(float a) { return sqrtf(a); }

__host__ __device__ inline int to_int(float v)
{
    if (v >= 2147483648.0f) return INT_MAX;
    if (v <= -2147483648.0f) return INT_MIN;
    return v == v ? (int)v : 0;
}

// steps 2 and 3: the box in cells, and whether it is kept
__host__ __device__ inline bool scale_and_test(const Consts& k, float x, float y, float dx, float dy, float& cx, float& cy,
                                               float& w, float& l)
{
    w = div_rn(div_rn(dx, k.vs0), k.f);
    l = div_rn(div_rn(dy, k.vs1), k.f);
    cx = div_rn(div_rn(x - k.pc0, k.vs0), k.f);
    cy = div_rn(div_rn(y - k.pc1, k.vs1), k.f);
    return w > 0.0f && l > 0.0f && cx > -1.0f && cx < k.Wf && cy > -1.0f && cy < k.Hf;
}

// step 4
__host__ __device__ inline int radius_of(const Consts& k, float w, float l)
{
    const float s = l + w;
    const float c1 = div_rn((w * l) * k.omm, k.opm);
    const float sq1 = sqrt_rn(s * s - 4.0f * c1);
    const float r1 = div_rn(s + sq1, 2.0f);
    const float b2 = 2.0f * s;
    const float c2 = (k.omm * w) * l;
    const float sq2 = sqrt_rn(b2 * b2 - 16.0f * c2);
    const float r2 = div_rn(b2 + sq2, 2.0f);
    const float a3 = 4.0f * k.m;
    const float b3 = (-2.0f * k.m) * s;
    const float c3 = ((k.m - 1.0f) * w) * l;
    const float sq3 = sqrt_rn(b3 * b3 - (4.0f * a3) * c3);
    const float r3 = div_rn(b3 + sq3, 2.0f);
    float rm = r1;
    if (r2 < rm) rm = r2;
    if (r3 < rm) rm = r3;
    const int r = to_int(rm);
    return r > k.min_radius ? r : k.min_radius;
}

// step 5: the D + 1 channels of a kept box (D = 7 or 9)
__host__ __device__ inline void target_row(const Consts& k, const float* box, int D, float cx, float cy, int ix, int iy, float* out)
{
    out[0] = cx - (float)ix;
    out[1] = cy - (float)iy;
    out[2] = box[2];
    if (k.norm_bbox) {
        out[3] = logf(box[3]), out[4] = logf(box[4]), out[5] = logf(box[5]);
    } else {
        out[3] = box[3], out[4] = box[4], out[5] = box[5];
    }
    out[6] = sinf(box[6]);
    out[7] = cosf(box[6]);
    if (D == 9) out[8] = box[7], out[9] = box[8];
}

}  // namespace accv_ct
