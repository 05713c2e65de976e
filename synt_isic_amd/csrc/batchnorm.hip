// batchnorm.hip -- BatchNorm2d in batch-statistics (training) mode over y [B, C, HW] (NCHW, a convolution output without bias):
//   * bn_moments_kernel          : per-channel (count, mean, M2) of one SLICE of a channel per workgroup, Welford in fp32 per lane,
//                                  lanes and waves merged with Chan's formula in double, in a fixed order
//   * bn_moments_finalize_kernel : the slices of a channel merged the same way (the arithmetic of gn_finalize.h), one wave per
//                                  channel: mean, invstd = 1/sqrt(var + eps), the biased var, and nn.BatchNorm2d's running update
//                                  rm <- (1-m) rm + m mean,  rv <- (1-m) rv + m var n/(n-1)
//   * bn_apply_kernel            : a = [relu](gamma (y - mean) invstd + beta [+ residual]) in one pass
//   * bn_bwd_reduce_kernel       : per slice, sum g' and sum g' xhat (g' = g, or g [act > 0] with the mask read from the kept
//                                  activation), the same slices and merges
//   * bn_bwd_finalize_kernel     : dbeta[c], dgamma[c]
//   * bn_bwd_apply_kernel        : dy = gamma invstd (g' - dbeta/n - xhat dgamma/n) in one pass, into a buffer of its own
//   * bn_fold_kernel             : the inference fold of a trained BatchNorm, sc = gamma / sqrt(rv + eps) and
//                                  bias = (float)(beta - rm sc) in double, the load path's arithmetic (resnet.cpp: fold)
// Never E[x^2] - E[x]^2.  No atomics: every summation order is a function of (B, C, HW) alone, two calls give equal bits.
//
// Memory bound, so the shape of the work is the shape of the loads.  A plane (b, c) is HW contiguous floats; it is cut into
// segments of BN_SEG floats (the reductions) or BN_APPLY_RUN floats (the apply passes) and a (plane, segment) RUN is read by one wave: up to three scalar head elements to the next 16-byte
// boundary, float4 loads, up to three scalar tail elements (HW is 1, 2, 4, 16, 49, 196, ... in ResNet18: head and tail are the
// whole run there).  The 16-byte path needs every tensor of a launch at the same offset from a 16-byte boundary; otherwise
// the run is read by scalars.
// Slices: a channel's runs (image-major) are dealt to S workgroups, S = clamp(B*HW / 8192, 1, 2048 / C) (never more than there
// are runs), so that the stem's 64 channels fill the chip (B = 32 at 112x112: 32 slices per channel, 2048 workgroups) while a
// small plane stays one workgroup per channel.
#include <cmath>

#include "common.h"
#include "gn_finalize.h"
#include "poison_switch.h"
#include "train.h"

namespace sisic {

constexpr int BN_SEG = 4096;              // floats of a run
constexpr int BN_THREADS = 256, BN_WAVES = 4;
constexpr int BN_MAX_WG = 2048;           // workgroups of a launch (guideline: 256 CUs x 8)
constexpr int BN_SLICE_MIN = 8192;        // elements a slice is worth
// the two apply passes cut a plane into runs of 256 floats -- one float4 per lane -- and launch up to 16384 workgroups
// (launch_add_relu's cap): at the stem's shape 47.7 us against 60.5 for 4096-float runs on 2048 workgroups (forward), 71.6
// against 77 - 82 (backward); 1024-float runs on 8192 workgroups were in between (60.6 / 74.2)
constexpr int BN_APPLY_RUN = 256;
constexpr int BN_APPLY_MAX_WG = 16384;

struct BnSplit { int segs, units, ups, S; };

// a function of the shape alone
static BnSplit bn_split(int B, int C, int HW) {
    BnSplit p;
    p.segs = cdiv(HW, BN_SEG);
    p.units = B * p.segs;
    const int64_t n = (int64_t)B * HW;
    int want = (int)std::min<int64_t>(std::max<int64_t>(n / BN_SLICE_MIN, 1), std::max(1, BN_MAX_WG / C));
    want = std::min(want, p.units);
    p.ups = cdiv(p.units, want);
    p.S = cdiv(p.units, p.ups);           // no empty slice
    return p;
}

int bn_slices(int B, int C, int HW) { return (B > 0 && C > 0 && HW > 0) ? bn_split(B, C, HW).S : 0; }

// One run [e0, e0 + L) walked by a wave.  mis: floats the tensors' common base lies past a 16-byte boundary (0..3), or -1: no
// common alignment, scalars only.  f1(e): one element, f4(e): four elements from a 16-byte aligned e.
template <class F1, class F4>
__device__ __forceinline__ void bn_run(const int64_t e0, const int L, const int mis, const int lane, F1&& f1, F4&& f4) {
    int head = L;
    if (mis >= 0) head = min(L, (4 - (int)(((int64_t)mis + e0) & 3)) & 3);
    const int body = (L - head) >> 2, tail = L - head - 4 * body;
    for (int i = lane; i < head; i += 64) f1(e0 + i);
    const int64_t v0 = e0 + head;
    for (int i = lane; i < body; i += 64) f4(v0 + 4 * (int64_t)i);
    if (lane < tail) f1(v0 + 4 * (int64_t)body + lane);
}

// the run of unit u (image-major, then segment) of channel c
__device__ __forceinline__ void bn_unit(const int u, const int c, const int C, const int HW, const int segs, int64_t& e0, int& L) {
    const int b = u / segs, seg = u - b * segs;
    e0 = ((int64_t)b * C + c) * HW + (int64_t)seg * BN_SEG;
    L = min(BN_SEG, HW - seg * BN_SEG);
}

// ================================================================ moments ==========================================
struct Welford {
    float cnt = 0.0f, mean = 0.0f, m2 = 0.0f;
    __device__ __forceinline__ void add(const float x) {
        cnt += 1.0f;
        const float d = x - mean;
        mean += d * __frcp_rn(cnt);
        m2 += d * (x - mean);
    }
    // four values at once: their own (mean, M2), then Chan's merge
    __device__ __forceinline__ void add4(const float4 v) {
        const float gm = ((v.x + v.y) + (v.z + v.w)) * 0.25f;
        const float a = v.x - gm, b = v.y - gm, c = v.z - gm, d = v.w - gm;
        const float g2 = (a * a + b * b) + (c * c + d * d);
        const float delta = gm - mean, tot = cnt + 4.0f, r = 4.0f * __frcp_rn(tot);
        mean += delta * r;
        m2 += g2 + delta * delta * cnt * r;
        cnt = tot;
    }
};

// (count, mean, M2) of the 64 lanes' records, in double, fixed order; every lane of the wave calls
__device__ __forceinline__ void bn_merge_lanes(const double cnt, const double mean, const double m2, double& n, double& mu, double& q) {
    n = wave64_sum_f64(cnt);
    const double s1 = wave64_sum_f64(cnt * mean);
    mu = n > 0.0 ? s1 / n : 0.0;
    const double d = mean - mu;
    q = wave64_sum_f64(m2 + cnt * d * d);
}

__global__ void __launch_bounds__(BN_THREADS)
bn_moments_kernel(const float* __restrict__ y, double* __restrict__ part, int C, int HW, int segs, int units, int ups, int S, int mis) {
    __shared__ double red[BN_WAVES][3];
    const int c = blockIdx.x / S, s = blockIdx.x - c * S;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int u0 = s * ups, u1 = min(units, u0 + ups);
    Welford w;
    for (int u = u0 + wave; u < u1; u += BN_WAVES) {
        int64_t e0; int L;
        bn_unit(u, c, C, HW, segs, e0, L);
        bn_run(e0, L, mis, lane, [&](int64_t e) { w.add(y[e]); },
               [&](int64_t e) { w.add4(*reinterpret_cast<const float4*>(y + e)); });
    }
    double n, mu, q;
    bn_merge_lanes(w.cnt, w.mean, w.m2, n, mu, q);
    if (lane == 0) { red[wave][0] = n; red[wave][1] = mu; red[wave][2] = q; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double N = 0.0, s1 = 0.0;
        for (int i = 0; i < BN_WAVES; ++i) { N += red[i][0]; s1 += red[i][0] * red[i][1]; }
        const double M = N > 0.0 ? s1 / N : 0.0;
        double Q = 0.0;
        for (int i = 0; i < BN_WAVES; ++i) { const double d = red[i][1] - M; Q += red[i][2] + red[i][0] * d * d; }
        double* dst = part + (size_t)blockIdx.x * 3;
        dst[0] = N; dst[1] = M; dst[2] = Q;
    }
}

__global__ void __launch_bounds__(BN_THREADS)
bn_moments_finalize_kernel(const double* __restrict__ part, int C, int S, float eps, float* __restrict__ mean,
                           float* __restrict__ invstd, float* __restrict__ var, float* __restrict__ rm, float* __restrict__ rv,
                           double momentum) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int c = blockIdx.x * BN_WAVES + wave;
    if (c >= C) return;                       // whole waves leave: no barrier below
    const double* p = part + (size_t)c * S * 3;
    double n = 0.0, s1 = 0.0;
    for (int i = lane; i < S; i += 64) { n += p[3 * i]; s1 += p[3 * i] * p[3 * i + 1]; }
    n = wave64_sum_f64(n);
    s1 = wave64_sum_f64(s1);
    const double mu = s1 / n;
    double q = 0.0;
    for (int i = lane; i < S; i += 64) { const double d = p[3 * i + 1] - mu; q += p[3 * i + 2] + p[3 * i] * d * d; }
    q = wave64_sum_f64(q);
    if (lane == 0) {
        const double v = fmax(q / n, 0.0);
        mean[c] = (float)mu;
        invstd[c] = (float)(1.0 / sqrt(v + (double)eps));
        if (var) var[c] = (float)v;
        if (rm) rm[c] = (float)((1.0 - momentum) * (double)rm[c] + momentum * mu);
        if (rv) rv[c] = (float)((1.0 - momentum) * (double)rv[c] + momentum * (v * n / (n - 1.0)));
    }
}

// ================================================================ apply ============================================
template <bool RES, bool RELU>
__global__ void __launch_bounds__(BN_THREADS)
bn_apply_kernel(const float* __restrict__ y, const float* __restrict__ gamma, const float* __restrict__ beta,
                const float* __restrict__ mean, const float* __restrict__ invstd, const float* __restrict__ residual,
                float* __restrict__ out, int C, int HW, int segs, int run, int64_t total_units, int mis) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int64_t u = (int64_t)blockIdx.x * BN_WAVES + wave; u < total_units; u += (int64_t)gridDim.x * BN_WAVES) {
        const int64_t plane = u / segs;
        const int seg = (int)(u - plane * segs), c = (int)(plane % C);
        const int64_t e0 = plane * HW + (int64_t)seg * run;
        const int L = min(run, HW - seg * run);
        const float m = mean[c], is = invstd[c], ga = gamma[c], be = beta[c];
        auto f = [&](float v, float r) {
            float a = (v - m) * is * ga + be;
            if (RES) a += r;
            return RELU ? fmaxf(a, 0.0f) : a;
        };
        bn_run(e0, L, mis, lane, [&](int64_t e) { out[e] = f(y[e], RES ? residual[e] : 0.0f); },
               [&](int64_t e) {
                   const float4 v = *reinterpret_cast<const float4*>(y + e);
                   float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
                   if (RES) r = *reinterpret_cast<const float4*>(residual + e);
                   *reinterpret_cast<float4*>(out + e) = make_float4(f(v.x, r.x), f(v.y, r.y), f(v.z, r.z), f(v.w, r.w));
               });
    }
}

// ================================================================ backward =========================================
template <bool MASK>
__global__ void __launch_bounds__(BN_THREADS)
bn_bwd_reduce_kernel(const float* __restrict__ g, const float* __restrict__ y, const float* __restrict__ act,
                     const float* __restrict__ mean, const float* __restrict__ invstd, double* __restrict__ part, int C, int HW,
                     int segs, int units, int ups, int S, int mis) {
    __shared__ double red[BN_WAVES][2];
    const int c = blockIdx.x / S, s = blockIdx.x - c * S;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int u0 = s * ups, u1 = min(units, u0 + ups);
    const float m = mean[c], is = invstd[c];
    double sb = 0.0, sg = 0.0;                // per lane: fp32 inside a run, double across runs
    for (int u = u0 + wave; u < u1; u += BN_WAVES) {
        int64_t e0; int L;
        bn_unit(u, c, C, HW, segs, e0, L);
        float rb = 0.0f, rg = 0.0f;
        auto f = [&](float gv, float yv, float av) {
            const float gp = (!MASK || av > 0.0f) ? gv : 0.0f;
            rb += gp;
            rg += gp * ((yv - m) * is);
        };
        bn_run(e0, L, mis, lane, [&](int64_t e) { f(g[e], y[e], MASK ? act[e] : 1.0f); },
               [&](int64_t e) {
                   const float4 gv = *reinterpret_cast<const float4*>(g + e);
                   const float4 yv = *reinterpret_cast<const float4*>(y + e);
                   float4 av = make_float4(1.f, 1.f, 1.f, 1.f);
                   if (MASK) av = *reinterpret_cast<const float4*>(act + e);
                   f(gv.x, yv.x, av.x); f(gv.y, yv.y, av.y); f(gv.z, yv.z, av.z); f(gv.w, yv.w, av.w);
               });
        sb += (double)rb;
        sg += (double)rg;
    }
    sb = wave64_sum_f64(sb);
    sg = wave64_sum_f64(sg);
    if (lane == 0) { red[wave][0] = sb; red[wave][1] = sg; }
    __syncthreads();
    if (threadIdx.x == 0) {
        part[(size_t)blockIdx.x * 2] = (red[0][0] + red[1][0]) + (red[2][0] + red[3][0]);
        part[(size_t)blockIdx.x * 2 + 1] = (red[0][1] + red[1][1]) + (red[2][1] + red[3][1]);
    }
}

__global__ void __launch_bounds__(BN_THREADS)
bn_bwd_finalize_kernel(const double* __restrict__ part, int C, int S, float* __restrict__ dgamma, float* __restrict__ dbeta) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int c = blockIdx.x * BN_WAVES + wave;
    if (c >= C) return;
    const double* p = part + (size_t)c * S * 2;
    double sb = 0.0, sg = 0.0;
    for (int i = lane; i < S; i += 64) { sb += p[2 * i]; sg += p[2 * i + 1]; }
    sb = wave64_sum_f64(sb);
    sg = wave64_sum_f64(sg);
    if (lane == 0) { dbeta[c] = (float)sb; dgamma[c] = (float)sg; }
}

template <bool MASK>
__global__ void __launch_bounds__(BN_THREADS)
bn_bwd_apply_kernel(const float* __restrict__ g, const float* __restrict__ y, const float* __restrict__ act,
                    const float* __restrict__ mean, const float* __restrict__ invstd, const float* __restrict__ gamma,
                    const float* __restrict__ dgamma, const float* __restrict__ dbeta, float* __restrict__ dy, int C, int HW,
                    int segs, int run, int64_t total_units, float inv_n, int mis) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int64_t u = (int64_t)blockIdx.x * BN_WAVES + wave; u < total_units; u += (int64_t)gridDim.x * BN_WAVES) {
        const int64_t plane = u / segs;
        const int seg = (int)(u - plane * segs), c = (int)(plane % C);
        const int64_t e0 = plane * HW + (int64_t)seg * run;
        const int L = min(run, HW - seg * run);
        const float m = mean[c], is = invstd[c], k = gamma[c] * is, mb = dbeta[c] * inv_n, mg = dgamma[c] * inv_n;
        auto f = [&](float gv, float yv, float av) {
            const float gp = (!MASK || av > 0.0f) ? gv : 0.0f;
            return k * (gp - mb - (yv - m) * is * mg);
        };
        bn_run(e0, L, mis, lane, [&](int64_t e) { dy[e] = f(g[e], y[e], MASK ? act[e] : 1.0f); },
               [&](int64_t e) {
                   const float4 gv = *reinterpret_cast<const float4*>(g + e);
                   const float4 yv = *reinterpret_cast<const float4*>(y + e);
                   float4 av = make_float4(1.f, 1.f, 1.f, 1.f);
                   if (MASK) av = *reinterpret_cast<const float4*>(act + e);
                   *reinterpret_cast<float4*>(dy + e) = make_float4(f(gv.x, yv.x, av.x), f(gv.y, yv.y, av.y), f(gv.z, yv.z, av.z), f(gv.w, yv.w, av.w));
               });
    }
}

// ================================================================ inference fold ===================================
// resnet.cpp fold(): sc = (double)gamma / sqrt((double)rv + (double)eps), bias = (float)((double)beta - (double)rm * sc); the
// product and the difference are rounded separately, as the host rounds them (no fused multiply-add)
__global__ void __launch_bounds__(BN_THREADS)
bn_fold_kernel(const float* __restrict__ gamma, const float* __restrict__ beta, const float* __restrict__ rm,
               const float* __restrict__ rv, float eps, double* __restrict__ sc, float* __restrict__ bias, int C) {
    const int c = blockIdx.x * BN_THREADS + threadIdx.x;
    if (c >= C) return;
    const double s = (double)gamma[c] / sqrt((double)rv[c] + (double)eps);
    sc[c] = s;
    bias[c] = (float)__dsub_rn((double)beta[c], __dmul_rn((double)rm[c], s));
}

// ================================================================ host side ========================================
// floats the tensors' common base lies past a 16-byte boundary, -1 without one; *ok = false: a pointer is no float address
static int bn_misalign(std::initializer_list<const void*> ptrs, bool* ok) {
    int mis = -2;
    *ok = true;
    for (const void* p : ptrs) {
        if (!p) continue;
        const uintptr_t a = reinterpret_cast<uintptr_t>(p);
        if (a & 3) { *ok = false; return -1; }
        const int m = (int)((a & 15) >> 2);
        if (mis == -2) mis = m;
        else if (mis != m) mis = -1;
    }
    return mis == -2 ? -1 : mis;
}

// The stream's partials (doubles), grown on demand as the attention backward's row statistics are (attention_wide.hip): a
// growth waits for the stream once, later calls neither allocate nor wait.
static int bn_scratch(sisic_ctx* ctx, hipStream_t s, size_t doubles, double** ptr) {
    std::lock_guard<std::mutex> lock(ctx->bn_part_mutex);
    auto& buf = ctx->bn_part[s];
    const size_t floats = 2 * doubles;
    if (buf.floats < floats) {
        SISIC_HIP(hipStreamSynchronize(s));          // earlier launches on this stream may still read the old buffer
        if (buf.p) SISIC_HIP(hipFree(buf.p));
        buf.p = nullptr; buf.floats = 0;
        SISIC_HIP(hipMalloc(reinterpret_cast<void**>(&buf.p), floats * sizeof(float)));
        if (poison_alloc()) {                        // SISIC_POISON_ALLOC=1: a partial no workgroup writes is NaN
            SISIC_HIP(hipMemset(buf.p, 0xFF, floats * sizeof(float)));
            SISIC_HIP(hipDeviceSynchronize());
        }
        buf.floats = floats;
        ctx->scratch_generation.fetch_add(1);
    }
    *ptr = reinterpret_cast<double*>(buf.p);
    return SISIC_OK;
}

static int bn_check_shape(const char* who, int B, int C, int HW) {
    SISIC_REQUIRE(B > 0 && C > 0 && HW > 0, "%s: B = %d, C = %d, HW = %d", who, B, C, HW);
    SISIC_REQUIRE((int64_t)B * HW >= 2, "%s: expected more than 1 value per channel when training (B * HW = 1)", who);
    SISIC_REQUIRE((int64_t)B * HW < (int64_t(1) << 31) && (int64_t)B * C < (int64_t(1) << 31), "%s: B = %d, C = %d, HW = %d is too large", who, B, C, HW);
    return SISIC_OK;
}

static unsigned bn_apply_grid(int64_t total_units) {
    return (unsigned)std::min<int64_t>(cdiv64(total_units, BN_WAVES), BN_APPLY_MAX_WG);
}

int launch_bn_moments(sisic_ctx* ctx, const float* y, int B, int C, int HW, float eps, float* mean, float* invstd, float* var,
                      float* running_mean, float* running_var, double momentum, hipStream_t s) {
    SISIC_REQUIRE(y && mean && invstd, "batchnorm moments: null tensor");
    SISIC_TRY(bn_check_shape("batchnorm moments", B, C, HW));
    SISIC_REQUIRE(eps >= 0.0f && (!!running_mean == !!running_var), "batchnorm moments: eps %g, running statistics both or neither", eps);
    SISIC_REQUIRE(!running_mean || (momentum > 0.0 && momentum <= 1.0), "batchnorm moments: momentum %g is outside (0, 1]", momentum);
    bool ok;
    const int mis = bn_misalign({y}, &ok);
    SISIC_REQUIRE(ok, "batchnorm moments: a tensor is not 4-byte aligned");
    const BnSplit p = bn_split(B, C, HW);
    double* part = nullptr;
    SISIC_TRY(bn_scratch(ctx, s, (size_t)C * p.S * 3, &part));
    {
        ProfileScope prof(ctx, s, PK_OTHER, 4.0 * B * C * HW, 0.0);
        hipLaunchKernelGGL(bn_moments_kernel, dim3((unsigned)(C * p.S)), dim3(BN_THREADS), 0, s, y, part, C, HW, p.segs, p.units, p.ups, p.S, mis);
        SISIC_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(bn_moments_finalize_kernel, dim3((unsigned)cdiv(C, BN_WAVES)), dim3(BN_THREADS), 0, s, part, C, p.S, eps, mean, invstd,
                       var, running_mean, running_var, momentum);
    SISIC_HIP(hipGetLastError());
    return SISIC_OK;
}

int launch_bn_apply(sisic_ctx* ctx, const float* y, const float* gamma, const float* beta, const float* mean, const float* invstd,
                    const float* residual, bool relu, float* out, int B, int C, int HW, hipStream_t s) {
    SISIC_REQUIRE(y && gamma && beta && mean && invstd && out, "batchnorm apply: null tensor");
    SISIC_TRY(bn_check_shape("batchnorm apply", B, C, HW));
    bool ok;
    const int mis = bn_misalign({y, residual, out}, &ok);
    SISIC_REQUIRE(ok, "batchnorm apply: a tensor is not 4-byte aligned");
    const int run = BN_APPLY_RUN;
    const int segs = cdiv(HW, run);
    const int64_t total = (int64_t)B * C * segs;
    ProfileScope prof(ctx, s, PK_OTHER, (residual ? 12.0 : 8.0) * B * C * HW, 0.0);
    const dim3 grid(bn_apply_grid(total)), block(BN_THREADS);
#define SISIC_BN_APPLY(RES, RELU) hipLaunchKernelGGL((bn_apply_kernel<RES, RELU>), grid, block, 0, s, y, gamma, beta, mean, invstd, residual, out, C, HW, segs, run, total, mis)
    if (residual) { if (relu) SISIC_BN_APPLY(true, true); else SISIC_BN_APPLY(true, false); }
    else { if (relu) SISIC_BN_APPLY(false, true); else SISIC_BN_APPLY(false, false); }
#undef SISIC_BN_APPLY
    SISIC_HIP(hipGetLastError());
    return SISIC_OK;
}

int launch_bn_bwd(sisic_ctx* ctx, const float* g, const float* y, const float* act, const float* mean, const float* invstd,
                  const float* gamma, float* dy, float* dgamma, float* dbeta, int B, int C, int HW, hipStream_t s) {
    SISIC_REQUIRE(g && y && mean && invstd && gamma && dgamma && dbeta, "batchnorm backward: null tensor");
    SISIC_TRY(bn_check_shape("batchnorm backward", B, C, HW));
    bool ok;
    const int mis = bn_misalign({g, y, act, dy}, &ok);
    SISIC_REQUIRE(ok, "batchnorm backward: a tensor is not 4-byte aligned");
    const BnSplit p = bn_split(B, C, HW);
    double* part = nullptr;
    SISIC_TRY(bn_scratch(ctx, s, (size_t)C * p.S * 3, &part));
    const double bytes = (act ? 12.0 : 8.0) * B * C * HW;
    {
        ProfileScope prof(ctx, s, PK_OTHER, bytes, 0.0);
        const dim3 grid((unsigned)(C * p.S)), block(BN_THREADS);
        if (act) hipLaunchKernelGGL(bn_bwd_reduce_kernel<true>, grid, block, 0, s, g, y, act, mean, invstd, part, C, HW, p.segs, p.units, p.ups, p.S, mis);
        else hipLaunchKernelGGL(bn_bwd_reduce_kernel<false>, grid, block, 0, s, g, y, act, mean, invstd, part, C, HW, p.segs, p.units, p.ups, p.S, mis);
        SISIC_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3((unsigned)cdiv(C, BN_WAVES)), dim3(BN_THREADS), 0, s, part, C, p.S, dgamma, dbeta);
    SISIC_HIP(hipGetLastError());
    if (dy) {                                        // (NULL: dgamma and dbeta alone)
        ProfileScope prof(ctx, s, PK_OTHER, bytes + 4.0 * B * C * HW, 0.0);
        const int run = BN_APPLY_RUN;
        const int asegs = cdiv(HW, run);
        const int64_t total = (int64_t)B * C * asegs;
        const dim3 grid(bn_apply_grid(total)), block(BN_THREADS);
        const float inv_n = (float)(1.0 / ((double)B * HW));
        if (act) hipLaunchKernelGGL(bn_bwd_apply_kernel<true>, grid, block, 0, s, g, y, act, mean, invstd, gamma, dgamma, dbeta, dy, C, HW, asegs, run, total, inv_n, mis);
        else hipLaunchKernelGGL(bn_bwd_apply_kernel<false>, grid, block, 0, s, g, y, act, mean, invstd, gamma, dgamma, dbeta, dy, C, HW, asegs, run, total, inv_n, mis);
        SISIC_HIP(hipGetLastError());
    }
    return SISIC_OK;
}

int launch_bn_fold(sisic_ctx* ctx, const float* gamma, const float* beta, const float* rm, const float* rv, float eps, double* sc,
                   float* bias, int C, hipStream_t s) {
    SISIC_REQUIRE(gamma && beta && rm && rv && sc && bias && C > 0, "batchnorm fold: bad arguments");
    hipLaunchKernelGGL(bn_fold_kernel, dim3((unsigned)cdiv(C, BN_THREADS)), dim3(BN_THREADS), 0, s, gamma, beta, rm, rv, eps, sc, bias, C);
    SISIC_HIP(hipGetLastError());
    return SISIC_OK;
}

}  // namespace sisic
