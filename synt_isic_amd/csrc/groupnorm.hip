// groupnorm.hip -- GroupNorm statistics, folded with the affine parameters.
//
// Replaces the reduction half of torch.nn.GroupNorm(32, C, eps=1e-5) in ResnetBlock2D
// (norm1/norm2), Attention.group_norm and conv_norm_out.
// The normalise+affine(+SiLU) half is fused into the consuming convolution's load path
// (conv_mfma.hip), so the activation tensor is read once here and once by the conv.
//
// One workgroup per (sample, group): one pass over the group's cpg*HW elements accumulating
// shifted first and second moments, wavefront-shuffle + LDS reductions, then
//   scale[b,c] = gamma[c]*rstd,  shift[b,c] = beta[c] - mean*scale[b,c].
// The input may be the channel concatenation of two tensors (up-path skip connections);
// a group may straddle the seam.
//
// HBM-bound.  Algorithmic bytes per launch: 4*B*C*HW (read once) + 8*B*C (written).
#include "common.h"
#include "gn_finalize.h"
#include "gn_merge.h"

namespace sisic {

constexpr int GN_THREADS = 256;

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ float block_sum(float v, float* red) {
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();   // protect red[] from the previous use
    if (lane == 0) red[wave] = v;
    __syncthreads();
    float t = 0.0f;
#pragma unroll
    for (int w = 0; w < GN_THREADS / 64; ++w) t += red[w];
    return t;
}

__global__ void __launch_bounds__(GN_THREADS)
gn_stats_kernel(const float* __restrict__ in0, int c0, const float* __restrict__ in1, int c1, int HW, int groups,
                float eps, const float* __restrict__ gamma, const float* __restrict__ beta,
                float* __restrict__ scale, float* __restrict__ shift, int aligned16, float* __restrict__ mean_rstd) {
    __shared__ float red[GN_THREADS / 64];
    const int C = c0 + c1;
    const int cpg = C / groups;
    const int b = blockIdx.x / groups, g = blockIdx.x % groups;
    const int tid = threadIdx.x;
    const bool vec = aligned16 && (HW & 3) == 0;

    auto plane = [&](int c) -> const float* {
        return (c < c0) ? in0 + ((size_t)b * c0 + c) * HW : in1 + ((size_t)b * c1 + (c - c0)) * HW;
    };

    // ONE pass over the data with shifted sums: K = the group's first element, s1 = sum(x-K),
    // s2 = sum((x-K)^2); mean = K + s1/n, var = s2/n - (s1/n)^2.  Shifting by a sample of the data keeps the
    // cancellation in the variance benign (|mean-K| is O(std)), at half the memory traffic of two passes.
    const float K = plane(g * cpg)[0];
    float s1 = 0.0f, s2 = 0.0f;
    for (int j = 0; j < cpg; ++j) {
        const float* src = plane(g * cpg + j);
        if (vec) {
            const float4* s4 = reinterpret_cast<const float4*>(src);
            const int n4 = HW / 4;
            int i = tid;
            // four independent 16-byte loads in flight per thread: the kernel is latency/bandwidth-bound
            for (; i + 3 * GN_THREADS < n4; i += 4 * GN_THREADS) {
                const float4 v0 = s4[i], v1 = s4[i + GN_THREADS], v2 = s4[i + 2 * GN_THREADS], v3 = s4[i + 3 * GN_THREADS];
                const float4 vv[4] = {v0, v1, v2, v3};
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const float a = vv[u].x - K, bq = vv[u].y - K, c = vv[u].z - K, d = vv[u].w - K;
                    s1 += (a + bq) + (c + d);
                    s2 += (a * a + bq * bq) + (c * c + d * d);
                }
            }
            for (; i < n4; i += GN_THREADS) {
                const float4 v = s4[i];
                const float a = v.x - K, bq = v.y - K, c = v.z - K, d = v.w - K;
                s1 += (a + bq) + (c + d);
                s2 += (a * a + bq * bq) + (c * c + d * d);
            }
        } else {
            for (int i = tid; i < HW; i += GN_THREADS) {
                const float a = src[i] - K;
                s1 += a;
                s2 += a * a;
            }
        }
    }
    const float n = (float)cpg * (float)HW;
    const float m1 = block_sum(s1, red) / n;
    const float m2 = block_sum(s2, red) / n;
    const float mean = K + m1;
    const float var = fmaxf(m2 - m1 * m1, 0.0f);
    const float rstd = 1.0f / sqrtf(var + eps);
    if (mean_rstd && tid == 0) {
        mean_rstd[2 * (size_t)blockIdx.x] = mean;
        mean_rstd[2 * (size_t)blockIdx.x + 1] = rstd;
    }
    if (tid < cpg) {
        const int c = g * cpg + tid;
        const float sc = gamma[c] * rstd;
        scale[(size_t)b * C + c] = sc;
        shift[(size_t)b * C + c] = beta[c] - mean * sc;
    }
}

int launch_gn_stats(sisic_ctx* ctx, const float* in0, int c0, const float* in1, int c1, int B, int HW, int groups,
                    float eps, const float* gamma, const float* beta, float* scale, float* shift, hipStream_t s,
                    float* mean_rstd) {
    SISIC_REQUIRE(in0 && gamma && beta && scale && shift, "groupnorm_stats: null tensor");
    SISIC_REQUIRE((c1 == 0) == (in1 == nullptr), "groupnorm_stats: in1/c1 mismatch");
    const int C = c0 + c1;
    SISIC_REQUIRE(B > 0 && HW > 0 && groups > 0 && C % groups == 0, "groupnorm_stats: C=%d not divisible by groups=%d", C, groups);
    SISIC_REQUIRE(C / groups <= GN_THREADS, "groupnorm_stats: %d channels per group unsupported", C / groups);
    ProfileScope prof(ctx, s, PK_GN, 4.0 * B * C * HW + 8.0 * B * C, 0.0);
    const int aligned16 = ((reinterpret_cast<uintptr_t>(in0) | reinterpret_cast<uintptr_t>(in1)) & 15) == 0;
    hipLaunchKernelGGL(gn_stats_kernel, dim3(B * groups), dim3(GN_THREADS), 0, s, in0, c0, in1, c1, HW, groups, eps,
                       gamma, beta, scale, shift, aligned16, mean_rstd);
    SISIC_HIP(hipGetLastError());
    return SISIC_OK;
}

// Finalize from per-workgroup partials: gn_finalize_job (gn_finalize.h), one wave per (image, group).
// (four (image, group) pairs per workgroup, one per wave: a quarter of the workgroups to dispatch -- the launch is 2048
//  one-wave jobs of a microsecond each at batch 64, and most of its 5 us was getting them onto the chip)
__global__ void __launch_bounds__(64 * GNF_WAVES) gn_finalize_kernel(const GnFinJob q) {
    gn_finalize_job(q, blockIdx.x * GNF_WAVES + (threadIdx.x >> 6), threadIdx.x & 63);
}

// The checked arguments of a finalisation as the job the kernels take (a launch of its own below, or riding on a 1x1 convolution:
// conv_pointwise_bf3.hip)
int make_gn_fin_job(GnFinJob* q, const float* st0, int c0, int slots0, const float* st1, int c1, int slots1, int B, int groups,
                    float eps, const float* gamma, const float* beta, float* scale, float* shift, float* mean_rstd) {
    SISIC_REQUIRE(st0 && gamma && beta && scale && shift, "groupnorm_finalize: null tensor");
    SISIC_REQUIRE((c1 == 0) == (st1 == nullptr), "groupnorm_finalize: stats1/c1 mismatch");
    const int C = c0 + c1;
    SISIC_REQUIRE(B > 0 && groups > 0 && c0 > 0 && C % groups == 0 && slots0 > 0 && (c1 == 0 || slots1 > 0),
                  "groupnorm_finalize: C=%d groups=%d slots=%d/%d", C, groups, slots0, slots1);
    SISIC_REQUIRE((int64_t)B * groups < (int64_t(1) << 31), "groupnorm_finalize: B=%d groups=%d: too many jobs", B, groups);
    q->st0 = reinterpret_cast<const float4*>(st0); q->st1 = reinterpret_cast<const float4*>(st1);
    q->c0 = c0; q->slots0 = slots0; q->c1 = c1; q->slots1 = slots1;
    q->groups = groups; q->n_jobs = B * groups; q->eps = eps;
    q->gamma = gamma; q->beta = beta; q->scale = scale; q->shift = shift; q->mean_rstd = mean_rstd;
    return SISIC_OK;
}

int launch_gn_finalize_job(sisic_ctx* ctx, const GnFinJob& q, hipStream_t s) {
    const int B = q.n_jobs / q.groups, C = q.c0 + q.c1;
    ProfileScope prof(ctx, s, PK_GN, 16.0 * B * (q.c0 * (double)q.slots0 + q.c1 * (double)q.slots1) + 8.0 * B * C, 0.0);
    hipLaunchKernelGGL(gn_finalize_kernel, dim3(cdiv(q.n_jobs, GNF_WAVES)), dim3(64 * GNF_WAVES), 0, s, q);
    SISIC_HIP(hipGetLastError());
    return SISIC_OK;
}

int launch_gn_finalize(sisic_ctx* ctx, const float* st0, int c0, int slots0, const float* st1, int c1, int slots1, int B,
                       int HW, int groups, float eps, const float* gamma, const float* beta, float* scale, float* shift,
                       hipStream_t s, float* mean_rstd) {
    SISIC_REQUIRE(HW > 0, "groupnorm_finalize: HW=%d", HW);        // (the element count travels with the partials)
    GnFinJob q{};
    SISIC_TRY(make_gn_fin_job(&q, st0, c0, slots0, st1, c1, slots1, B, groups, eps, gamma, beta, scale, shift, mean_rstd));
    return launch_gn_finalize_job(ctx, q, s);
}

}  // namespace sisic
