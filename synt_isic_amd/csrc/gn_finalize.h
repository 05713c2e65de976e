// gn_finalize.h -- ONE (image, group) job of the GroupNorm finalisation from per-workgroup partials, as a device function: the
// body of gn_finalize_kernel (groupnorm.hip), and of the RIDER workgroups that the bf16x3 1x1 kernels (conv_pointwise_bf3.hip)
// run ahead of their own items when a finalisation is independent of the convolution (a ResNet block's norm1 beside its
// shortcut).  One definition, so that both compile to the same operations in the same order and give the same bits.
#pragma once

#include <hip/hip_runtime.h>

#include "gn_merge.h"

namespace sisic {

constexpr int GNF_WAVES = 4;             // jobs (= waves) per workgroup, in gn_finalize_kernel and in a rider workgroup

// today's arguments of the finalisation: partials [b][c][slot] of one or two producers (the channel concatenation), the module's
// gamma / beta, the (scale, shift) [B, c0 + c1] it leaves, optionally (mean, rstd) [B, groups, 2].  n_jobs = B * groups.
struct GnFinJob {
    const float4* st0;
    const float4* st1;
    int c0, slots0, c1, slots1;
    int groups, n_jobs;
    float eps;
    const float* gamma;
    const float* beta;
    float* scale;
    float* shift;
    float* mean_rstd;
};

// Sum of a double over the 64 lanes in a fixed order: DPP butterflies on the two 32-bit halves inside each row of 16
// lanes (a few cycles each; ds_bpermute shuffles cost an LDS round trip per step), then the four row totals by readlane.
__device__ __forceinline__ double dpp_f64(double v, const int ctrl_sel) {
    const long long b = __double_as_longlong(v);
    int lo = (int)(b & 0xffffffffll), hi = (int)(b >> 32);
    switch (ctrl_sel) {
        case 0: lo = __builtin_amdgcn_update_dpp(0, lo, 0xB1, 0xf, 0xf, true); hi = __builtin_amdgcn_update_dpp(0, hi, 0xB1, 0xf, 0xf, true); break;
        case 1: lo = __builtin_amdgcn_update_dpp(0, lo, 0x4E, 0xf, 0xf, true); hi = __builtin_amdgcn_update_dpp(0, hi, 0x4E, 0xf, 0xf, true); break;
        case 2: lo = __builtin_amdgcn_update_dpp(0, lo, 0x141, 0xf, 0xf, true); hi = __builtin_amdgcn_update_dpp(0, hi, 0x141, 0xf, 0xf, true); break;
        default: lo = __builtin_amdgcn_update_dpp(0, lo, 0x140, 0xf, 0xf, true); hi = __builtin_amdgcn_update_dpp(0, hi, 0x140, 0xf, 0xf, true); break;
    }
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
__device__ __forceinline__ double wave64_sum_f64(double v) {
    v += dpp_f64(v, 0);      // quad_perm [1,0,3,2]
    v += dpp_f64(v, 1);      // quad_perm [2,3,0,1]
    v += dpp_f64(v, 2);      // row_half_mirror
    v += dpp_f64(v, 3);      // row_mirror
    const long long b = __double_as_longlong(v);
    const int lo = (int)(b & 0xffffffffll), hi = (int)(b >> 32);
    double r[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
        r[i] = __longlong_as_double(((long long)__builtin_amdgcn_readlane(hi, 16 * i) << 32) |
                                    (unsigned int)__builtin_amdgcn_readlane(lo, 16 * i));
    return (r[0] + r[1]) + (r[2] + r[3]);
}

// Finalize from per-workgroup partials (count, sum, M2 about the partial's own mean): one wave per (image, group).
// Lanes stride over the (channel, slot) pairs of the group; the pairwise-merge identity
//     M2 = sum_i M2_i + sum_i n_i (mean_i - mean)^2
// is evaluated in float64 with fixed-order butterflies, so the result is independent of timing and as robust against
// |mean| >> std as the shifted single pass of gn_stats_kernel.
// The whole wave calls this with its job index (wave-uniform); a wave past the last job returns at once.  No LDS, no barrier.
__device__ __forceinline__ void gn_finalize_job(const GnFinJob& q, const int job, const int lane) {
    const int c0 = q.c0, c1 = q.c1, slots0 = q.slots0, slots1 = q.slots1, groups = q.groups;
    const float4* __restrict__ st0 = q.st0;
    const float4* __restrict__ st1 = q.st1;
    const float* __restrict__ gamma = q.gamma;
    const float* __restrict__ beta = q.beta;
    float* __restrict__ scale = q.scale;
    float* __restrict__ shift = q.shift;
    float* __restrict__ mean_rstd = q.mean_rstd;
    const float eps = q.eps;
    const int C = c0 + c1, gs = C / groups;
    if (job >= q.n_jobs) return;             // whole waves leave: no barrier below
    const int b = job / groups, g = job % groups;
    // the group's channels are one contiguous run of partials in each producer's buffer ([b][c][slot])
    const int ca = g * gs, cb = ca + gs;
    const int a0 = min(ca, c0), b0 = min(cb, c0);                 // channels [a0, b0) of the first producer
    const int a1 = max(ca, c0) - c0, b1 = max(cb, c0) - c0;       // channels [a1, b1) of the second
    const float4* run0 = st0 + ((size_t)b * c0 + a0) * slots0;
    const int len0 = (b0 - a0) * slots0;
    const float4* run1 = st1 ? st1 + ((size_t)b * c1 + a1) * slots1 : nullptr;
    const int len1 = st1 ? (b1 - a1) * slots1 : 0;
    // this lane's output channel (gs <= 64 in every network here; the tail loop below covers larger groups)
    const float my_gamma = lane < gs ? gamma[ca + lane] : 0.0f, my_beta = lane < gs ? beta[ca + lane] : 0.0f;
    constexpr int KEEP = 4;                                        // partials per lane and producer held in registers
    float4 k0[KEEP], k1[KEEP];
    double n = 0.0, s1 = 0.0, m2 = 0.0;
#pragma unroll
    for (int j = 0; j < KEEP; ++j) {
        const int i = lane + 64 * j;
        k0[j] = i < len0 ? run0[i] : make_float4(0.f, 0.f, 0.f, 0.f);
        k1[j] = i < len1 ? run1[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int j = 0; j < KEEP; ++j) {
        n += (double)k0[j].x + (double)k1[j].x;
        s1 += (double)k0[j].y + (double)k1[j].y;
        m2 += (double)k0[j].z + (double)k1[j].z;
    }
    for (int i = lane + 64 * KEEP; i < len0; i += 64) { const float4 v = run0[i]; n += v.x; s1 += v.y; m2 += v.z; }
    for (int i = lane + 64 * KEEP; i < len1; i += 64) { const float4 v = run1[i]; n += v.x; s1 += v.y; m2 += v.z; }
    n = wave64_sum_f64(n);
    s1 = wave64_sum_f64(s1);
    m2 = wave64_sum_f64(m2);
    const double mean = s1 / n;
    double between = 0.0;
    auto dev = [&](const float4 v) { between += gn_between_term(v.x, v.y, mean); };       // (gn_merge.h)
#pragma unroll
    for (int j = 0; j < KEEP; ++j) { dev(k0[j]); dev(k1[j]); }
    for (int i = lane + 64 * KEEP; i < len0; i += 64) dev(run0[i]);
    for (int i = lane + 64 * KEEP; i < len1; i += 64) dev(run1[i]);
    between = wave64_sum_f64(between);
    float meanf, rstd;
    gn_mean_rstd(n, s1, m2, between, eps, meanf, rstd, mean);
    if (mean_rstd && lane == 0) {
        mean_rstd[2 * (size_t)job] = meanf;
        mean_rstd[2 * (size_t)job + 1] = rstd;
    }
    if (lane < gs) {
        float sc, sh;
        gn_affine(my_gamma, my_beta, meanf, rstd, sc, sh);
        scale[(size_t)b * C + ca + lane] = sc;
        shift[(size_t)b * C + ca + lane] = sh;
    }
    for (int cc = lane + 64; cc < gs; cc += 64) {
        const int c = ca + cc;
        float sc, sh;
        gn_affine(gamma[c], beta[c], meanf, rstd, sc, sh);
        scale[(size_t)b * C + c] = sc;
        shift[(size_t)b * C + c] = sh;
    }
}

}  // namespace sisic
