// Arithmetic of the fused camera-image preparation (image_prep.hip): the reference's AffineTransformer (fn.warp_affine,
// bilinear, fill 0), PhotoMetricDistorter._process_images, ImageToTileSizePadder and ImageMeanStdDevNormalizer /
// ImageRange01Normalizer (dali_pipeline_framework processing_steps/) for ONE output pixel.  The GPU kernel and the host
// entry accv_prepare_images_host evaluate the same operation sequence from these functions.  Everything is float32;
// contraction into fma is off for everything that includes this header; every div_rn is ONE correctly rounded division
// (__fdiv_rn on the device, `/` on the host), every other operator one IEEE operation, evaluated exactly as parenthesised.
//
// Per image (Warp, Colour):
//   matrix     [[a, b, tx], [c, d, ty]] maps source to output coordinates; det = a * d - b * c.  The image is "outside"
//              (every sample is 0) unless the six entries, det and div_rn(1, det) are finite and det != 0.
//   colour     (delta, alpha_pre, saturation, hue_degrees, alpha_post, permutation_index); a stage runs unless its value is
//              the identity: delta == 0, alpha == 1, saturation == 1 && hue_degrees == 0.  The hue shift in sectors of 60
//              degrees: sh = div_rn(hue_degrees, 60); shift = sh - 6 * floor(div_rn(sh, 6)), in [0, 6].  A permutation
//              index that is not one of 0..5 is 0.
// Per output pixel (X, Y), the pixel centre at +0.5:
//   position   u = (X + 0.5) - tx, v = (Y + 0.5) - ty;
//              sx = div_rn(d * u - b * v, det) - 0.5, sy = div_rn(a * v - c * u, det) - 0.5;
//              outside unless -1 < sx < Wv and -1 < sy < Hv (the valid extent; decided BEFORE any float -> int conversion,
//              a NaN fails); x0 = (int)floor(sx), wx = sx - floor(sx), likewise y0, wy
//   sample     p00 = (x0, y0), p01 = (x0 + 1, y0), p10 = (x0, y0 + 1), p11 the fourth; a neighbour outside
//              [0, Wv) x [0, Hv) is 0 and is not read (two neighbours of a row that are both inside are read as their six
//              contiguous bytes); ax = 1 - wx, ay = 1 - wy;
//              top = p00 * ax + p01 * wx, bot = p10 * ax + p11 * wx, value = top * ay + bot * wy, per channel.
//              Without a matrix the byte at (X, Y) is taken as is, which is what the identity matrix gives bit for bit.
//   unit       v = value * kInv255 (the float32 nearest 1 / 255)
//   chain      1 v = clamp(v + delta)   2 v = clamp(v * alpha_pre)
//              3 mx, mn = max, min of (r, g, b); dc = mx - mn; s = div_rn(dc, mx) * saturation and
//                h = div_rn(g - b, dc) | 2 + div_rn(b - r, dc) | 4 + div_rn(r - g, dc) for mx == r | g | b (first match),
//                both 0 when dc == 0; h = h + shift; h += 6 if h < 0; h -= 6 if h >= 6; i = floor(h), f = h - i;
//                p = mx * (1 - s), q = mx * (1 - s * f), t = mx * (1 - s * (1 - f)); (r, g, b) = (mx, t, p), (q, mx, p),
//                (p, mx, t), (p, q, mx), (t, p, mx), (mx, p, q) for i = 0..5.  Not clamped.
//              4 v = clamp(v * alpha_post)   5 channel k takes channel perm[k]   6 v = clamp(v)
//              clamp(v) = v < 0 ? 0 : (v > 1 ? 1 : v)
//   normalise  out[k] = v[k] * scale[k] + bias[k]; scale = 255 / std, bias = -mean / std, float64 rounded once to float32
//
// An NV12 source (Nv12Source: the two planes of a decoder surface) has its own load_pixel / load_pair / sample / load_four
// below: each tap is converted by nv12_arith.h to the uint8 triple the stand-alone conversion writes and handed on as three
// floats in 0..255, exact, so `sample` and everything after it see what they would see from the converted RGB batch.
//
// The longest chain of ROUNDED operations from the four source bytes to an output (every stage active), which the tests'
// tolerance is built from: ax (1), p00 * ax (1), + p01 * wx (1), top * ay (1), + bot * wy (1), kInv255 and its product (2),
// delta (1), alpha_pre (1), the hue path sh, div_rn(sh, 6), shift, h + shift, the wrap, 1 - f, s * (1 - f), 1 - (.), mx * (.)
// (9; floor, f, max and min are exact; the path dc, div_rn(g - b, dc), 2 + (.) to h is as long), alpha_post (1), scale and
// its product (2), bias and its sum (2): K = 23.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "nv12_arith.h"

#pragma clang fp contract(off)

namespace accv_ip {

constexpr int kMaxExtent = 16384;          // of a source image, an output image and a tile: ACCV_IP_MAX_EXTENT
constexpr float kInv255 = 1.0f / 255.0f;

__host__ __device__ inline float div_rn(float a, float b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __fdiv_rn(a, b);
#else
    return a / b;
#endif
}

__host__ __device__ inline bool is_finite(float v) { return fabsf(v) <= FLT_MAX; }   // false for NaN

__host__ __device__ inline float clamp01(float v) { return v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v); }

// the matrix of one image
struct Warp {
    float a, b, tx, c, d, ty, det;
    bool copy;      // no matrix: the source pixel as is
    bool ok;        // invertible and finite; meaningless with copy
};

// m: the six floats of the image's matrix, or null
__host__ __device__ inline Warp load_warp(const float* m)
{
    Warp w;
    w.copy = m == nullptr;
    w.a = w.d = w.det = 1.0f;
    w.b = w.c = w.tx = w.ty = 0.0f;
    w.ok = true;
    if (w.copy) return w;
    w.a = m[0], w.b = m[1], w.tx = m[2], w.c = m[3], w.d = m[4], w.ty = m[5];
    w.det = w.a * w.d - w.b * w.c;
    w.ok = is_finite(w.a) && is_finite(w.b) && is_finite(w.tx) && is_finite(w.c) && is_finite(w.d) && is_finite(w.ty) &&
           is_finite(w.det) && w.det != 0.0f && is_finite(div_rn(1.0f, w.det));
    return w;
}

// where output pixel (X, Y) samples; (-2, -2, 0, 0) and !inside when no neighbour can lie inside the valid extent
struct Position {
    int x0, y0;
    float wx, wy;
    bool inside;
};

__host__ __device__ inline Position sample_position(const Warp& w, int X, int Y, int Wv, int Hv)
{
    Position p;
    p.x0 = p.y0 = -2;
    p.wx = p.wy = 0.0f;
    p.inside = false;
    if (w.copy) {
        if (X < Wv && Y < Hv) p.x0 = X, p.y0 = Y, p.inside = true;
        return p;
    }
    if (!w.ok) return p;
    const float u = ((float)X + 0.5f) - w.tx;
    const float v = ((float)Y + 0.5f) - w.ty;
    const float sx = div_rn(w.d * u - w.b * v, w.det) - 0.5f;
    const float sy = div_rn(w.a * v - w.c * u, w.det) - 0.5f;
    if (!(sx > -1.0f && sx < (float)Wv && sy > -1.0f && sy < (float)Hv)) return p;
    const float fx = floorf(sx), fy = floorf(sy);     // in [-1, 16383]
    p.x0 = (int)fx, p.y0 = (int)fy;
    p.wx = sx - fx, p.wy = sy - fy;
    p.inside = true;
    return p;
}

// the three channels of source pixel (x, y) of an image whose rows are `pitch` pixels apart; 0 outside the valid extent
__host__ __device__ inline void load_pixel(const unsigned char* img, long long pitch, int x, int y, int Wv, int Hv, float (&o)[3])
{
    o[0] = o[1] = o[2] = 0.0f;
    if (x < 0 || y < 0 || x >= Wv || y >= Hv) return;
    const unsigned char* q = img + ((long long)y * pitch + x) * 3;
    o[0] = (float)q[0], o[1] = (float)q[1], o[2] = (float)q[2];
}

// the two horizontally adjacent source pixels (x, y) and (x + 1, y): when both lie inside, their six contiguous bytes come
// as one 4-byte and one 2-byte read (not aligned; no byte beyond the six is touched), else pixel by pixel.  Same values.
__host__ __device__ inline void load_pair(const unsigned char* img, long long pitch, int x, int y, int Wv, int Hv,
                                          float (&l)[3], float (&r)[3])
{
    if (y >= 0 && y < Hv && x >= 0 && x + 1 < Wv) {
        const unsigned char* q = img + ((long long)y * pitch + x) * 3;
        uint32_t lo;
        uint16_t hi;
        memcpy(&lo, q, 4);
        memcpy(&hi, q + 4, 2);
        l[0] = (float)(lo & 0xffu), l[1] = (float)((lo >> 8) & 0xffu), l[2] = (float)((lo >> 16) & 0xffu);
        r[0] = (float)(lo >> 24), r[1] = (float)(hi & 0xffu), r[2] = (float)(hi >> 8);
        return;
    }
    load_pixel(img, pitch, x, y, Wv, Hv, l);
    load_pixel(img, pitch, x + 1, y, Wv, Hv, r);
}

// the bilinear blend of the four taps, per channel
__host__ __device__ inline void blend(const float (&p00)[3], const float (&p01)[3], const float (&p10)[3], const float (&p11)[3],
                                      const Position& p, float (&val)[3])
{
    const float ax = 1.0f - p.wx, ay = 1.0f - p.wy;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float top = p00[c] * ax + p01[c] * p.wx;
        const float bot = p10[c] * ax + p11[c] * p.wx;
        val[c] = top * ay + bot * p.wy;
    }
}

// the sampled value in 0..255 per channel
__host__ __device__ inline void sample(const unsigned char* img, long long pitch, const Warp& w, const Position& p, int Wv,
                                       int Hv, float (&val)[3])
{
    val[0] = val[1] = val[2] = 0.0f;
    if (!p.inside) return;
    if (w.copy) {
        load_pixel(img, pitch, p.x0, p.y0, Wv, Hv, val);
        return;
    }
    float p00[3], p01[3], p10[3], p11[3];
    load_pair(img, pitch, p.x0, p.y0, Wv, Hv, p00, p01);
    load_pair(img, pitch, p.x0, p.y0 + 1, Wv, Hv, p10, p11);
    blend(p00, p01, p10, p11, p, val);
}

// ---- the same three functions for a source of NV12 planes: every tap is converted to the uint8 triple nv12_to_rgb would
// have written (nv12_arith.h) and handed on as floats, so everything after the load is the code above
struct Nv12Source {
    const unsigned char* y;      // luma of the image: pixel (x, y) at y * y_pitch + x
    const unsigned char* uv;     // chroma of the image: the pair of sample (i, r) at r * uv_pitch + 2 * i
    long long y_pitch, uv_pitch; // bytes
    accv_nv12::Format f;
};

__host__ __device__ inline void nv12_tap(const accv_nv12::Format& f, int Y, int e, int o, float (&out)[3])
{
    int c0, c1, c2;
    accv_nv12::convert(f, Y, e, o, c0, c1, c2);
    out[0] = (float)c0, out[1] = (float)c1, out[2] = (float)c2;
}

// 0 outside the valid extent.  The chroma sample (x / 2, y / 2) of a valid pixel always lies in the plane.
__host__ __device__ inline void load_pixel(const Nv12Source& s, int x, int y, int Wv, int Hv, float (&o)[3])
{
    o[0] = o[1] = o[2] = 0.0f;
    if (x < 0 || y < 0 || x >= Wv || y >= Hv) return;
    const unsigned char* q = s.uv + (y / 2) * s.uv_pitch + (x / 2) * 2;
    nv12_tap(s.f, s.y[y * s.y_pitch + x], q[0], q[1], o);
}

// the chroma pairs of pixels x and x + 1 (both inside the plane's width) of chroma row cy, as (e0, o0, e1, o1) in one word:
// one UV pair (2 bytes) when x is even, two adjacent ones (4 contiguous bytes) when it is odd.  Not aligned.
__host__ __device__ inline uint32_t load_chroma_pair(const Nv12Source& s, int x, int cy)
{
    const unsigned char* q = s.uv + cy * s.uv_pitch + (x / 2) * 2;
    if (x & 1) {
        uint32_t w;
        memcpy(&w, q, 4);
        return w;
    }
    uint16_t h;
    memcpy(&h, q, 2);
    return (uint32_t)h | ((uint32_t)h << 16);
}

// the two taps (x, y), (x + 1, y), both inside, from their chroma word
__host__ __device__ inline void nv12_pair(const Nv12Source& s, int x, int y, uint32_t chroma, float (&l)[3], float (&r)[3])
{
    uint16_t luma;
    memcpy(&luma, s.y + y * s.y_pitch + x, 2);
    nv12_tap(s.f, (int)(luma & 0xffu), (int)(chroma & 0xffu), (int)((chroma >> 8) & 0xffu), l);
    nv12_tap(s.f, (int)(luma >> 8), (int)((chroma >> 16) & 0xffu), (int)(chroma >> 24), r);
}

// the two horizontally adjacent taps (x, y) and (x + 1, y): when both lie inside, two luma bytes and their chroma word,
// else pixel by pixel.  Same values.
__host__ __device__ inline void load_pair(const Nv12Source& s, int x, int y, int Wv, int Hv, float (&l)[3], float (&r)[3])
{
    if (y >= 0 && y < Hv && x >= 0 && x + 1 < Wv) {
        nv12_pair(s, x, y, load_chroma_pair(s, x, y / 2), l, r);
        return;
    }
    load_pixel(s, x, y, Wv, Hv, l);
    load_pixel(s, x + 1, y, Wv, Hv, r);
}

// a footprint that lies inside reads the chroma of its two rows once when y0 is even: they share the chroma row
__host__ __device__ inline void sample(const Nv12Source& s, const Warp& w, const Position& p, int Wv, int Hv, float (&val)[3])
{
    val[0] = val[1] = val[2] = 0.0f;
    if (!p.inside) return;
    if (w.copy) {
        load_pixel(s, p.x0, p.y0, Wv, Hv, val);
        return;
    }
    float p00[3], p01[3], p10[3], p11[3];
    if (p.y0 >= 0 && p.y0 + 1 < Hv && p.x0 >= 0 && p.x0 + 1 < Wv) {
        const uint32_t top = load_chroma_pair(s, p.x0, p.y0 / 2);
        const uint32_t bot = (p.y0 & 1) ? load_chroma_pair(s, p.x0, p.y0 / 2 + 1) : top;
        nv12_pair(s, p.x0, p.y0, top, p00, p01);
        nv12_pair(s, p.x0, p.y0 + 1, bot, p10, p11);
    } else {
        load_pair(s, p.x0, p.y0, Wv, Hv, p00, p01);
        load_pair(s, p.x0, p.y0 + 1, Wv, Hv, p10, p11);
    }
    blend(p00, p01, p10, p11, p, val);
}

// without a matrix: the four pixels (X .. X + 3, Y), X a multiple of 4 and all inside, from 4 luma bytes and the 4 chroma
// bytes of their two pairs (two 4-byte reads, not aligned)
__host__ __device__ inline void load_four(const Nv12Source& s, int X, int Y, float (&val)[4][3])
{
    uint32_t luma, chroma;
    memcpy(&luma, s.y + Y * s.y_pitch + X, 4);
    memcpy(&chroma, s.uv + (Y / 2) * s.uv_pitch + X, 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t pair = chroma >> (16 * (j / 2));
        nv12_tap(s.f, (int)((luma >> (8 * j)) & 0xffu), (int)(pair & 0xffu), (int)((pair >> 8) & 0xffu), val[j]);
    }
}

// the colour row of one image
struct Colour {
    float delta, alpha_pre, saturation, shift, alpha_post;
    int perm;
    bool do_delta, do_pre, do_hsv, do_post;
};

// row: the six floats of the image's photometric row, or null
__host__ __device__ inline Colour load_colour(const float* row)
{
    Colour k;
    k.delta = 0.0f, k.alpha_pre = k.saturation = k.alpha_post = 1.0f, k.shift = 0.0f;
    k.perm = 0;
    k.do_delta = k.do_pre = k.do_hsv = k.do_post = false;
    if (!row) return k;
    k.delta = row[0], k.alpha_pre = row[1], k.saturation = row[2], k.alpha_post = row[4];
    const float hue = row[3], pi = row[5];
    k.do_delta = !(k.delta == 0.0f);
    k.do_pre = !(k.alpha_pre == 1.0f);
    k.do_hsv = !(k.saturation == 1.0f && hue == 0.0f);
    k.do_post = !(k.alpha_post == 1.0f);
    const float sh = div_rn(hue, 60.0f);
    k.shift = sh - 6.0f * floorf(div_rn(sh, 6.0f));
    if (pi >= 0.0f && pi <= 5.0f && pi == floorf(pi)) k.perm = (int)pi;
    return k;
}

// which input channel output channel k takes: get_color_channel_permutation of the reference
__host__ __device__ inline int perm_source(int perm, int k)
{
    switch (perm) {
    case 1: return k == 0 ? 0 : (k == 1 ? 2 : 1);   // 0 2 1
    case 2: return k == 0 ? 1 : (k == 1 ? 0 : 2);   // 1 0 2
    case 3: return 2 - k;                           // 2 1 0
    case 4: return k == 0 ? 2 : k - 1;              // 2 0 1
    case 5: return k == 2 ? 0 : k + 1;              // 1 2 0
    default: return k;
    }
}

// saturation and hue in HSV space, in place on (r, g, b)
__host__ __device__ inline void hsv_stage(const Colour& k, float& r, float& g, float& b)
{
    const float mx = fmaxf(r, fmaxf(g, b)), mn = fminf(r, fminf(g, b));
    const float dc = mx - mn;
    float s = 0.0f, h = 0.0f;
    if (dc > 0.0f) {     // then mx > mn >= 0
        s = div_rn(dc, mx) * k.saturation;
        if (mx == r) h = div_rn(g - b, dc);
        else if (mx == g) h = 2.0f + div_rn(b - r, dc);
        else h = 4.0f + div_rn(r - g, dc);
    }
    h = h + k.shift;
    if (h < 0.0f) h = h + 6.0f;
    if (h >= 6.0f) h = h - 6.0f;
    if (!(h >= 0.0f && h < 6.0f)) h = 0.0f;      // a hue that is not finite
    const float fi = floorf(h), f = h - fi;
    const int i = (int)fi;
    const float p = mx * (1.0f - s), q = mx * (1.0f - s * f), t = mx * (1.0f - s * (1.0f - f));
    switch (i) {
    case 0: r = mx, g = t, b = p; break;
    case 1: r = q, g = mx, b = p; break;
    case 2: r = p, g = mx, b = t; break;
    case 3: r = p, g = q, b = mx; break;
    case 4: r = t, g = p, b = mx; break;
    default: r = mx, g = p, b = q; break;
    }
}

// scale and bias per output channel, the value of a padding pixel, the source's channel order
struct Norm {
    float scale[3], bias[3], pad[3];
    int is_bgr;
};

// val: the sampled 0..255 value per source channel; out: the normalised value per output channel
__host__ __device__ inline void colour_chain(const Colour& k, const Norm& n, const float (&val)[3], float (&out)[3])
{
    float v[3] = {val[0] * kInv255, val[1] * kInv255, val[2] * kInv255};
    if (k.do_delta) {
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = clamp01(v[c] + k.delta);
    }
    if (k.do_pre) {
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = clamp01(v[c] * k.alpha_pre);
    }
    if (k.do_hsv) {
        if (n.is_bgr) hsv_stage(k, v[2], v[1], v[0]);
        else hsv_stage(k, v[0], v[1], v[2]);
    }
    if (k.do_post) {
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = clamp01(v[c] * k.alpha_post);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int src = perm_source(k.perm, c);
        const float x = src == 0 ? v[0] : (src == 1 ? v[1] : v[2]);
        out[c] = clamp01(x) * n.scale[c] + n.bias[c];
    }
}

}  // namespace accv_ip
