// Per-peak arithmetic of the centre-point box decoder (center_decode.hip): mmdet3d's CenterPointBBoxCoder.decode and the
// `circle` branch of CenterHead.get_bboxes for one peak.  The GPU kernel and the host entry accv_center_point_decode_host
// evaluate the same operation sequence from these functions.  Everything is float32; contraction into fma is off for
// everything that includes this header; every operator below is ONE IEEE operation, evaluated exactly as parenthesised
// here; the one division (in the sigmoid) is __fdiv_rn on the device and `/` on the host.  Decisions are comparisons only,
// so NaN fails all of them.
//
// Constants (rounded once to float32 from the caller's numbers): pc0, pc1 = pc_range[0], [1]; vs0, vs1 = voxel_size[0],
// [1]; f = out_size_factor; thr = score_threshold; lo[i], hi[i] = post_center_range[i], [3 + i]; nms = nms_threshold[t].
// Gathered channels (f16 / bf16 widened exactly): g = (off_x, off_y, z, d0, d1, d2, sin, cos[, vx, vy]) at the peak's cell,
// xs = index % W, ys = index / W.
//
//   centre     x = (((float)xs + off_x) * f) * vs0 + pc0          y = (((float)ys + off_y) * f) * vs1 + pc1
//   score      s, or with scores_are_logits  1 / (1 + exp(-s))
//   validity   (no threshold or score > thr) && (no range or lo[0] <= x && x <= hi[0] && lo[1] <= y && y <= hi[1] &&
//              lo[2] <= z && z <= hi[2])
//   circle     peak j suppresses a later peak iff  (x - xj) * (x - xj) + (y - yj) * (y - yj) <= nms
//   row        (x, y, z, dims, atan2(sin, cos)[, vx, vy]) with dims = (d0, d1, d2), or (exp d0, exp d1, exp d2) under
//              norm_bbox; with bottom_center z becomes z - dims[2] * 0.5 (after the range test); z, the raw dims and the
//              velocity are bit copies; exp / atan2 are expf / atan2f of the platform (device and host agree to a few ulp,
//              not bit for bit)
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#pragma clang fp contract(off)

namespace accv_cd {

constexpr int kMaxTasks = 8;      // ACCV_CD_MAX_TASKS
constexpr int kMaxMaps = 8;       // ACCV_CD_MAX_MAPS
constexpr int kMaxClasses = 64;   // ACCV_CD_MAX_CLASSES
constexpr int kMaxChannels = 10;
constexpr int kMaxK = 1024;       // ACCV_CD_MAX_K

// the constants of a call, rounded to float32 once on the host
struct Consts {
    float pc0, pc1, vs0, vs1, f, thr;
    float lo[3], hi[3];
    int has_thr, has_range, logits, norm_bbox, bottom;
};

__host__ __device__ inline float div_rn(float a, float b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __fdiv_rn(a, b);
#else
    return a / b;
#endif
}

// step 2: a centre coordinate in metres from its cell and the regressed offset
__host__ __device__ inline float coordinate(long long cell, float off, float f, float vs, float pc)
{
    return (((float)cell + off) * f) * vs + pc;
}

// step 3
__host__ __device__ inline float score_of(const Consts& k, float s)
{
    return k.logits ? div_rn(1.0f, 1.0f + expf(-s)) : s;
}

// step 4, for a peak whose index and class position are legal
__host__ __device__ inline bool passes(const Consts& k, float score, float x, float y, float z)
{
    if (k.has_thr && !(score > k.thr)) return false;
    if (k.has_range && !(k.lo[0] <= x && x <= k.hi[0] && k.lo[1] <= y && y <= k.hi[1] && k.lo[2] <= z && z <= k.hi[2])) return false;
    return true;
}

// step 5: does the kept centre (xj, yj) suppress the later centre (x, y)
__host__ __device__ inline bool suppresses(float xj, float yj, float x, float y, float nms)
{
    const float dx = x - xj, dy = y - yj;
    return dx * dx + dy * dy <= nms;
}

// steps 2 and 7: the C - 1 values of a written box from the C gathered channels g and the centre
__host__ __device__ inline void box_row(const Consts& k, const float* g, int C, float x, float y, float* row)
{
    row[0] = x, row[1] = y;
    if (k.norm_bbox) {
        row[3] = expf(g[3]), row[4] = expf(g[4]), row[5] = expf(g[5]);
    } else {
        row[3] = g[3], row[4] = g[4], row[5] = g[5];
    }
    row[2] = k.bottom ? g[2] - row[5] * 0.5f : g[2];
    row[6] = atan2f(g[6], g[7]);
    if (C == 10) row[7] = g[8], row[8] = g[9];
}

}  // namespace accv_cd
