// augment_pixel.h -- one output pixel of the training augmentation chain (include/sisic.h, sisic_augment) in PIL's own
// arithmetic: integer 8-bit resampling with 22-bit coefficients, float32 blends truncated to uint8, a 16.16 fixed-point
// nearest rotation.  Plain integer / IEEE code with no fused multiply-add (the including file is built with
// -ffp-contract=off), so the host and the device give the same bits.
#pragma once

#include <cstdint>

#include "../../include/sisic.h"

#define AUG_HD __host__ __device__ __forceinline__

namespace sisic {
namespace aug {

constexpr int PRECISION_BITS = 22;           // PIL Resample.c: 32 - 8 - 2

AUG_HD int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
AUG_HD int clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// the taps of output index o of a bilinear resize n_in -> n_out, n_in <= n_out (support 1, at most 3 taps): PIL's
// precompute_coeffs + normalize_coeffs_8bpc.  n_in == n_out is the copy PIL makes of that axis.
struct Taps {
    int lo, n;
    int k[3];
};

AUG_HD Taps resize_taps(int o, int n_in, int n_out) {
#pragma clang fp contract(off)
    Taps t;
    t.k[0] = 1 << PRECISION_BITS;
    t.k[1] = t.k[2] = 0;
    if (n_in == n_out) {
        t.lo = o;
        t.n = 1;
        return t;
    }
    const double scale = (double)n_in / (double)n_out;
    const double c = ((double)o + 0.5) * scale;
    int lo = (int)(c - 1.0 + 0.5);
    if (lo < 0) lo = 0;
    int hi = (int)(c + 1.0 + 0.5);
    if (hi > n_in) hi = n_in;
    const int n = clampi(hi - lo, 1, 3);
    double w[3] = {0.0, 0.0, 0.0};
    double ww = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        if (i < n) {
            double v = (double)(i + lo) - c + 0.5;
            if (v < 0.0) v = -v;
            w[i] = v < 1.0 ? 1.0 - v : 0.0;
            ww += w[i];
        }
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        double kk = w[i];
        if (ww != 0.0) kk /= ww;
        t.k[i] = i < n ? (int)(0.5 + kk * (double)(1 << PRECISION_BITS)) : 0;
    }
    t.lo = lo;
    t.n = n;
    return t;
}

// the record's box with every value forced inside the image: a bad record can never make a pixel read out of bounds
struct Box {
    int x, y, w, h;
};
AUG_HD Box clamped_box(const sisic_augment_params& p, int H, int W) {
    Box b;
    b.w = clampi(p.crop_w, 1, W);
    b.h = clampi(p.crop_h, 1, H);
    b.x = clampi(p.crop_x, 0, W - b.w);
    b.y = clampi(p.crop_y, 0, H - b.h);
    return b;
}

// stages 1 and 2 at output (x, y): img.crop(box).resize((W, H), BILINEAR), horizontal pass rounded to uint8 before the
// vertical one, then the flips as index reversal.  img: this record's source image, uint8 [H, W, 3].
AUG_HD void resized_pixel(const uint8_t* __restrict__ img, const sisic_augment_params& p, const Box& box, int H, int W,
                          int x, int y, int rgb[3]) {
    const int rx = p.hflip ? W - 1 - x : x;
    const int ry = p.vflip ? H - 1 - y : y;
    const Taps tx = resize_taps(rx, box.w, W);
    const Taps ty = resize_taps(ry, box.h, H);
    int acc[3] = {1 << (PRECISION_BITS - 1), 1 << (PRECISION_BITS - 1), 1 << (PRECISION_BITS - 1)};
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        if (j >= ty.n) break;
        const int row = clampi(box.y + ty.lo + j, 0, H - 1);
        int h[3] = {1 << (PRECISION_BITS - 1), 1 << (PRECISION_BITS - 1), 1 << (PRECISION_BITS - 1)};
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            if (i >= tx.n) break;
            const int col = clampi(box.x + tx.lo + i, 0, W - 1);
            const uint8_t* px = img + ((int64_t)row * W + col) * 3;
            h[0] += (int)px[0] * tx.k[i];
            h[1] += (int)px[1] * tx.k[i];
            h[2] += (int)px[2] * tx.k[i];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] += clip8(h[c] >> PRECISION_BITS) * ty.k[j];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) rgb[c] = clip8(acc[c] >> PRECISION_BITS);
}

// PIL's Image.blend(degenerate, image, f) on one band: one float32 multiply, one float32 add, truncation
AUG_HD int blend(int d, int i, float f) {
#pragma clang fp contract(off)
    const float t = (float)d + f * (float)(i - d);
    return t <= 0.0f ? 0 : (t >= 255.0f ? 255 : (int)t);
}

AUG_HD int gray(const int rgb[3]) { return (rgb[0] * 19595 + rgb[1] * 38470 + rgb[2] * 7471 + 0x8000) >> 16; }

// stage 3: the record's colour operations in its order.  until_contrast: stop in front of the contrast operation (what the
// grey mean is taken of); an order without contrast then runs to its end.
AUG_HD void colour_ops(const sisic_augment_params& p, int mean_gray, bool until_contrast, int rgb[3]) {
#pragma unroll
    for (int s = 0; s < 3; ++s) {
        const int op = p.order[s];
        if (op == 0) {
#pragma unroll
            for (int c = 0; c < 3; ++c) rgb[c] = blend(0, rgb[c], p.factor[0]);
        } else if (op == 1) {
            if (until_contrast) return;
#pragma unroll
            for (int c = 0; c < 3; ++c) rgb[c] = blend(mean_gray, rgb[c], p.factor[1]);
        } else if (op == 2) {
            const int g = gray(rgb);
#pragma unroll
            for (int c = 0; c < 3; ++c) rgb[c] = blend(g, rgb[c], p.factor[2]);
        }
    }
}

// stages 1-4 at output (x, y): the rotation's source pixel first (nearest, fill 0), the rest of the chain there
AUG_HD void chain_pixel(const uint8_t* __restrict__ img, const sisic_augment_params& p, const Box& box, int H, int W, int x,
                        int y, int mean_gray, int rgb[3]) {
    int sx = x, sy = y;
    if (p.rotate) {
        // int32 accumulation as PIL's affine_fixed runs it (wrapping, hence unsigned here)
        const uint32_t xx = (uint32_t)p.rot[2] + (uint32_t)y * (uint32_t)p.rot[1] + (uint32_t)x * (uint32_t)p.rot[0];
        const uint32_t yy = (uint32_t)p.rot[5] + (uint32_t)y * (uint32_t)p.rot[4] + (uint32_t)x * (uint32_t)p.rot[3];
        sx = (int32_t)xx >> 16;
        sy = (int32_t)yy >> 16;
        if (sx < 0 || sx >= W || sy < 0 || sy >= H) {
            rgb[0] = rgb[1] = rgb[2] = 0;
            return;
        }
    }
    resized_pixel(img, p, box, H, W, sx, sy, rgb);
    colour_ops(p, mean_gray, false, rgb);
}

// stage 5: ToTensor + Normalize(0.5, 0.5) in float32, correctly rounded divisions
AUG_HD float to_normalized(int v) {
#pragma clang fp contract(off)
    return ((float)v / 255.0f - 0.5f) / 0.5f;
}

}  // namespace aug
}  // namespace sisic
