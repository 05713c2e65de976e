// augment.hip -- the training loader's augmentation chain (diffusion/train_diffusion.py:72-81) on a device-resident dataset,
// two launches per batch:
//   * augment_gray_mean : one workgroup per output image; the rounded mean grey value the contrast operation blends towards
//   * augment_apply     : one thread per output pixel; crop-resize, flips, colour operations, rotation, normalisation
// Every stage is PIL's arithmetic (augment_pixel.h), so the result equals what torchvision's PIL backend returns for the
// same parameters bit for bit.  The work per batch is tens of microseconds of integer code: launch- and latency-bound, no
// intermediate image, no tiling.  Built with -ffp-contract=off: the blends are one multiply and one add.
#include "common.h"
#include "augment_pixel.h"

namespace sisic {

constexpr int AUG_MEAN_THREADS = 1024;
constexpr int AUG_MEAN_WAVES = AUG_MEAN_THREADS / 64;
constexpr int AUG_APPLY_THREADS = 256;

static_assert(sizeof(sisic_augment_params) == 96, "sisic_augment_params is 96 bytes without padding (include/sisic.h)");

// dataset uint8 [N,H,W,3]; params [B]; gray_mean int32 [B].  The sum is an integer (<= 255 * H * W < 2^31, checked by the
// launcher), so the reduction order does not matter.
__global__ void __launch_bounds__(AUG_MEAN_THREADS)
augment_gray_mean_kernel(const uint8_t* __restrict__ dataset, int N, int H, int W,
                         const sisic_augment_params* __restrict__ params, int32_t* __restrict__ gray_mean) {
    __shared__ int red[AUG_MEAN_WAVES];
    const int b = blockIdx.x;
    const sisic_augment_params p = params[b];
    const aug::Box box = aug::clamped_box(p, H, W);
    const uint8_t* img = dataset + (int64_t)aug::clampi(p.src, 0, N - 1) * H * W * 3;
    const int n = H * W;
    int sum = 0;
    for (int idx = threadIdx.x; idx < n; idx += AUG_MEAN_THREADS) {
        int rgb[3];
        aug::resized_pixel(img, p, box, H, W, idx % W, idx / W, rgb);
        aug::colour_ops(p, 0, true, rgb);
        sum += aug::gray(rgb);
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) sum += __shfl_xor(sum, d, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t total = 0;
#pragma unroll
        for (int w = 0; w < AUG_MEAN_WAVES; ++w) total += red[w];
        // floor(total / n + 0.5): int(ImageStat.Stat(grey).mean[0] + 0.5)
        gray_mean[b] = (int32_t)((2 * total + n) / (2 * (int64_t)n));
    }
}

// out: float32 [B,3,H,W] in [-1,1] (U8 = false) or uint8 [B,H,W,3], the image PIL returns (U8 = true)
template <bool U8>
__global__ void __launch_bounds__(AUG_APPLY_THREADS)
augment_apply_kernel(const uint8_t* __restrict__ dataset, int N, int H, int W, const sisic_augment_params* __restrict__ params,
                     const int32_t* __restrict__ gray_mean, void* __restrict__ out) {
    const int b = blockIdx.y;
    const int n = H * W;
    const int idx = blockIdx.x * AUG_APPLY_THREADS + threadIdx.x;
    if (idx >= n) return;
    const sisic_augment_params p = params[b];
    const aug::Box box = aug::clamped_box(p, H, W);
    const uint8_t* img = dataset + (int64_t)aug::clampi(p.src, 0, N - 1) * n * 3;
    int rgb[3];
    aug::chain_pixel(img, p, box, H, W, idx % W, idx / W, gray_mean[b], rgb);
    if (U8) {
        uint8_t* o = static_cast<uint8_t*>(out) + ((int64_t)b * n + idx) * 3;
        o[0] = (uint8_t)rgb[0];
        o[1] = (uint8_t)rgb[1];
        o[2] = (uint8_t)rgb[2];
    } else {
        float* o = static_cast<float*>(out) + (int64_t)b * 3 * n + idx;
        o[0] = aug::to_normalized(rgb[0]);
        o[n] = aug::to_normalized(rgb[1]);
        o[2 * (int64_t)n] = aug::to_normalized(rgb[2]);
    }
}

int launch_augment(sisic_ctx* ctx, const uint8_t* dataset, int N, int H, int W, const sisic_augment_params* params_dev, int B,
                   int32_t* gray_mean_scratch, void* out, bool u8, hipStream_t s) {
    SISIC_REQUIRE(dataset && params_dev && gray_mean_scratch && out, "augment: null argument");
    SISIC_REQUIRE(N > 0 && B > 0, "augment: empty dataset (%d images) or batch (%d records)", N, B);
    SISIC_REQUIRE(H > 0 && W > 0 && H % 8 == 0 && W % 8 == 0, "augment: %d x %d: height and width must be positive multiples of 8",
                  H, W);
    SISIC_REQUIRE((int64_t)H * W * 255 < ((int64_t)1 << 31), "augment: an image of %d x %d pixels is too large", H, W);
    SISIC_REQUIRE(B <= 65535, "augment: %d records in one call (at most 65535)", B);
    const int n = H * W;
    ProfileScope prof(ctx, s, PK_OTHER, (double)B * n * (u8 ? 3.0 + 3.0 : 3.0 + 12.0), 0.0);
    hipLaunchKernelGGL(augment_gray_mean_kernel, dim3(B), dim3(AUG_MEAN_THREADS), 0, s, dataset, N, H, W, params_dev,
                       gray_mean_scratch);
    SISIC_HIP(hipGetLastError());
    const dim3 grid(cdiv(n, AUG_APPLY_THREADS), B);
    if (u8)
        hipLaunchKernelGGL(augment_apply_kernel<true>, grid, dim3(AUG_APPLY_THREADS), 0, s, dataset, N, H, W, params_dev,
                           gray_mean_scratch, out);
    else
        hipLaunchKernelGGL(augment_apply_kernel<false>, grid, dim3(AUG_APPLY_THREADS), 0, s, dataset, N, H, W, params_dev,
                           gray_mean_scratch, out);
    SISIC_HIP(hipGetLastError());
    return SISIC_OK;
}

}  // namespace sisic
