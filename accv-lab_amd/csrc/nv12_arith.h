// Arithmetic of the NV12 -> RGB conversion (nv12.hip, and the NV12 source of image_prep.hip): the reference's
// convert_nv12_to_rgb (on_demand_video_decoder, ColorConvertKernels.cu: yuv42xxp_to_rgb_kernel and its full-range form) for
// ONE pixel.  The GPU kernels and the host entries evaluate the same operation sequence from these functions.
//
// Inputs: the pixel's Y and the U, V of chroma sample (y / 2, x / 2), integer division: chroma is taken nearest, not
// interpolated.  In a UV plane row the pair of chroma sample i is bytes 2 i and 2 i + 1; U is the even byte ("uv", NV12) or
// the odd one ("vu", NV21).
//   limited range  all int32; >> 20 is an arithmetic shift (floor):
//                  yy = max(0, Y - 16) * 1220542; uu = U - 128; vv = V - 128;
//                  R = clamp((yy + 1673527 * vv + 2^19) >> 20, 0, 255)
//                  G = clamp((yy - 852492 * vv - 409993 * uu + 2^19) >> 20, 0, 255)
//                  B = clamp((yy + 2116026 * uu + 2^19) >> 20, 0, 255)
//                  No intermediate leaves int32: over all 2^24 triples the extremes are -270 851 328 and 560 444 840.
//   full range     float32, every operator ONE IEEE operation in the order written (contraction into fma is off for
//                  everything that includes this header):
//                  yy = max(0, (float)Y) * C0; uu = (float)U - 127.5f; vv = (float)V - 127.5f;
//                  r = (int32)((yy + C1 * vv) + 0.5f); g = (int32)(((yy + C2 * vv) + C3 * uu) + 0.5f);
//                  b = (int32)((yy + C4 * uu) + 0.5f), the conversion truncating toward zero;
//                  then clamp((t + 2^19) >> 20, 0, 255) as above.  C0..C4 are the float32 nearest the reference's constants.
//                  DIVERGENCE: the reference builds with fast math, so its compiler may contract these products and sums
//                  into fma; this library's definition is the uncontracted sequence, the same on the device and the host.
//   as_bgr         the triple is stored, or handed on, as B, G, R.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#pragma clang fp contract(off)

namespace accv_nv12 {

// how a surface is read and the triple ordered
struct Format {
    int full_range;
    int as_bgr;
    int vu;          // V at the even byte of a chroma pair (NV21)
};

__host__ __device__ inline int descale_clamp(int t)
{
    const int v = (t + (1 << 19)) >> 20;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

__host__ __device__ inline void limited_range(int Y, int U, int V, int& r, int& g, int& b)
{
    const int y16 = Y - 16;
    const int yy = (y16 < 0 ? 0 : y16) * 1220542;
    const int uu = U - 128, vv = V - 128;
    r = descale_clamp(yy + 1673527 * vv);
    g = descale_clamp(yy - 852492 * vv - 409993 * uu);
    b = descale_clamp(yy + 2116026 * uu);
}

__host__ __device__ inline void full_range(int Y, int U, int V, int& r, int& g, int& b)
{
    constexpr float C0 = 1048230.1882352941f, C1 = 1470078.6196078432f, C2 = -748855.7176470588f, C3 = -360150.7137254902f,
                    C4 = 1858783.6235294119f;
    const float fy = (float)Y;
    const float yy = (fy < 0.0f ? 0.0f : fy) * C0;
    const float uu = (float)U - 127.5f, vv = (float)V - 127.5f;
    r = descale_clamp((int32_t)((yy + C1 * vv) + 0.5f));
    g = descale_clamp((int32_t)(((yy + C2 * vv) + C3 * uu) + 0.5f));
    b = descale_clamp((int32_t)((yy + C4 * uu) + 0.5f));
}

// the stored triple of one pixel: c0, c1, c2 in 0..255; e and o are the even and the odd byte of its chroma pair
__host__ __device__ inline void convert(const Format& f, int Y, int e, int o, int& c0, int& c1, int& c2)
{
    const int U = f.vu ? o : e, V = f.vu ? e : o;
    int r, g, b;
    if (f.full_range) full_range(Y, U, V, r, g, b);
    else limited_range(Y, U, V, r, g, b);
    c0 = f.as_bgr ? b : r, c1 = g, c2 = f.as_bgr ? r : b;
}

}  // namespace accv_nv12
