// classifier_train.hip -- what turns the classifier's data-gradient walk (classifier_bwd.hip, resnet.cpp) into a training
// step with BatchNorm frozen (torchvision.ops.FrozenBatchNorm2d semantics: the function the folded forward computes).
// The weight gradients of the 3x3 and 1x1 convolutions are launch_conv_wgrad's (train_kernels.hip); this file holds the rest:
//   * stem_wgrad_kernel     : dW of the 7x7 stride-2 stem, K-split over pixel tiles, slabs summed in a fixed order
//   * gather_even_kernel    : the even pixels of a plane (inverse of scatter_add_even): a 1x1 stride-2 convolution's weight
//                             gradient is the 1x1 stride-1 form on the gathered input
//   * ce_head_kernel        : cross-entropy (per-class weights, reduction "mean") and d loss / d logits in one launch
//   * fc_head_bwd_kernel    : d loss / d (layer4 output) through Linear, average pool and ReLU mask; d fc.weight, d fc.bias
//   * unfold_grad_kernel    : d w_raw[co] = sc[co] * d w_folded[co]        (the chain differentiates the FOLDED filter)
//   * refold_kernel         : raw = (float)((double)w * sc[co]) and its transposed, tap-flipped twin, the load path's arithmetic
// No atomics anywhere: two calls give equal bits, and the summation order of every element is a function of (B, H, W) alone.
#include "common.h"
#include "train.h"

namespace sisic {

// ================================================================ stem weight gradient ==============================
// dW[co,ci,ky,kx] = sum_{b,y,x} dy[b,co,y,x] * in[b,ci,2y+ky-3,2x+kx-3]: a 64 x 147 output reduced over B*OH*OW pixels.
// Vector ALU, not the matrix pipe: the 147-wide side is 4.6 MFMA tiles of 32 (five, one mostly padding), a k-step of
// v_mfma_f32_32x32x2_f32 wants two pixels per operand row from a stride-2, 49-tap gather, and the whole gradient is
// 2 * 64 * 147 flops per pixel -- 0.24 GFLOP per 224x224 image, one per cent of the step's arithmetic -- while dy (3.2 MB
// per image) has to be read either way.  fp32 fused multiply-adds: products exact, one rounding per accumulation.
// Measured at batch 32, 224x224: 250 us, 4 % of the step's kernel time (30 TFLOP/s: fourteen LDS reads feed forty
// multiply-adds, so the LDS pipe and not the ALU sets the pace; dy alone is 103 MB, 20 us at memory rate).
// Workgroup = one K-split slice: it walks its share of the 4 x 16 output-pixel tiles (in tile order: image, row, column),
// stages a tile's dy [64 px][64 co] and the 13 x 37 input patch of the three channels in LDS, and thread (cg, tg) keeps
// 4 output channels x 10 taps in registers (taps tg, tg + 16, ...: 160 >= 147, the last thirteen are padding).
constexpr int SW_TR = 4, SW_TC = 16, SW_P = SW_TR * SW_TC;
constexpr int SW_IH = 2 * SW_TR + 5, SW_IW = 2 * SW_TC + 5, SW_PLANE = SW_IH * SW_IW;
constexpr int SW_DYS = 65;                       // dy row (64 channels of a pixel) + 1: conflict-free staging
constexpr int SW_TAPS = 147, SW_TPT = 10;        // taps, taps per thread
constexpr int SW_MAX_SLICES = 1024;             // four workgroups per CU at a full batch (256, one wave per SIMD: 422 us against 250)

__global__ void __launch_bounds__(256)
stem_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ part, int H, int W, int OH,
                  int OW, int tiles_x, int tiles_y, int nblocks, int blocks_per_slice) {
    __shared__ float xL[3 * SW_PLANE];
    __shared__ float dL[SW_P * SW_DYS];
    const int tid = threadIdx.x, cg = tid >> 4, tg = tid & 15;
    int off[SW_TPT];
#pragma unroll
    for (int i = 0; i < SW_TPT; ++i) {
        const int j = tg + 16 * i;
        const int jj = j < SW_TAPS ? j : 0;
        off[i] = (jj / 49) * SW_PLANE + ((jj % 49) / 7) * SW_IW + jj % 7;
    }
    float acc[SW_TPT][4];
#pragma unroll
    for (int i = 0; i < SW_TPT; ++i)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[i][c] = 0.0f;

    const int blk_lo = blockIdx.x * blocks_per_slice, blk_hi = min(nblocks, blk_lo + blocks_per_slice);
    for (int blk = blk_lo; blk < blk_hi; ++blk) {
        int t = blk;
        const int tx = t % tiles_x; t /= tiles_x;
        const int ty = t % tiles_y;
        const int b = t / tiles_y;
        const int oy0 = ty * SW_TR, ox0 = tx * SW_TC;
        const int iy0 = 2 * oy0 - 3, ix0 = 2 * ox0 - 3;
        __syncthreads();                          // the previous tile has been read
        for (int i = tid; i < 3 * SW_PLANE; i += 256) {
            const int ci = i / SW_PLANE, r = i % SW_PLANE;
            const int y = iy0 + r / SW_IW, xx = ix0 + r % SW_IW;
            const bool ok = y >= 0 && y < H && xx >= 0 && xx < W;
            xL[i] = ok ? x[(((size_t)b * 3 + ci) * H + y) * W + xx] : 0.0f;
        }
        for (int i = tid; i < 64 * SW_P; i += 256) {
            const int p = i & (SW_P - 1), co = i >> 6;
            const int oy = oy0 + p / SW_TC, ox = ox0 + p % SW_TC;
            const bool ok = oy < OH && ox < OW;
            dL[p * SW_DYS + co] = ok ? dy[(((size_t)b * 64 + co) * OH + oy) * OW + ox] : 0.0f;
        }
        __syncthreads();
#pragma unroll 2
        for (int p = 0; p < SW_P; ++p) {
            const float* xp = xL + 2 * (p / SW_TC) * SW_IW + 2 * (p % SW_TC);
            const float* dp = dL + p * SW_DYS + 4 * cg;
            const float d0 = dp[0], d1 = dp[1], d2 = dp[2], d3 = dp[3];
#pragma unroll
            for (int i = 0; i < SW_TPT; ++i) {
                const float xv = xp[off[i]];
                acc[i][0] += d0 * xv;
                acc[i][1] += d1 * xv;
                acc[i][2] += d2 * xv;
                acc[i][3] += d3 * xv;
            }
        }
    }
    float* dst = part + (size_t)blockIdx.x * 64 * SW_TAPS;
#pragma unroll
    for (int i = 0; i < SW_TPT; ++i) {
        const int j = tg + 16 * i;
        if (j < SW_TAPS) {
#pragma unroll
            for (int c = 0; c < 4; ++c) dst[(4 * cg + c) * SW_TAPS + j] = acc[i][c];
        }
    }
}

static void stem_wgrad_split(int B, int OH, int OW, int* tiles_x, int* tiles_y, int* nblocks, int* bps, int* ksplit) {
    *tiles_x = cdiv(OW, SW_TC);
    *tiles_y = cdiv(OH, SW_TR);
    *nblocks = B * *tiles_x * *tiles_y;
    *bps = cdiv(*nblocks, std::min(*nblocks, SW_MAX_SLICES));
    *ksplit = cdiv(*nblocks, *bps);               // no empty slices
}

size_t stem_wgrad_scratch_floats() { return (size_t)SW_MAX_SLICES * 64 * SW_TAPS; }

int launch_stem_wgrad(sisic_ctx* ctx, const float* x, const float* dy, float* dw, int B, int H, int W, float* part,
                      size_t part_floats, hipStream_t s) {
    SISIC_REQUIRE(x && dy && dw && part && B > 0, "stem_wgrad: bad arguments");
    SISIC_REQUIRE(H >= 8 && W >= 8 && H % 2 == 0 && W % 2 == 0, "stem_wgrad: input %dx%d (even sizes from 8)", H, W);
    const int OH = H / 2, OW = W / 2;
    int tiles_x, tiles_y, nblocks, bps, ksplit;
    SISIC_REQUIRE((int64_t)B * cdiv(OH, SW_TR) * cdiv(OW, SW_TC) < (int64_t(1) << 31), "stem_wgrad: too many tiles");
    stem_wgrad_split(B, OH, OW, &tiles_x, &tiles_y, &nblocks, &bps, &ksplit);
    const size_t n = (size_t)64 * SW_TAPS;
    SISIC_REQUIRE((size_t)ksplit * n <= part_floats, "stem_wgrad: scratch too small");
    {
        ProfileScope prof(ctx, s, PK_OTHER, 4.0 * B * (3.0 * H * W + 64.0 * OH * OW), 2.0 * B * 64.0 * SW_TAPS * OH * OW);
        hipLaunchKernelGGL(stem_wgrad_kernel, dim3(ksplit), dim3(256), 0, s, x, dy, part, H, W, OH, OW, tiles_x, tiles_y, nblocks, bps);
        SISIC_HIP(hipGetLastError());
    }
    return launch_wgrad_reduce(ctx, part, ksplit, n, dw, s);
}

// ================================================================ even pixels of a plane ============================
// out[plane,i,j] = in[plane,2i,2j]   (in [planes,H,W], out [planes,OH,OW] with OH = (H-1)/2+1)
__global__ void __launch_bounds__(256)
gather_even_kernel(const float* __restrict__ in, float* __restrict__ out, int H, int W, int OH, int OW, int64_t total) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int j = (int)(i % OW);
        const int64_t r = i / OW;
        const int ii = (int)(r % OH);
        const int64_t plane = r / OH;
        out[i] = in[(plane * H + 2 * ii) * W + 2 * j];
    }
}

int launch_gather_even(sisic_ctx* ctx, const float* in, float* out, int planes, int H, int W, hipStream_t s) {
    SISIC_REQUIRE(in && out && planes > 0 && H > 0 && W > 0, "gather_even: bad arguments");
    const int OH = (H - 1) / 2 + 1, OW = (W - 1) / 2 + 1;
    const int64_t total = (int64_t)planes * OH * OW;
    ProfileScope prof(ctx, s, PK_OTHER, 8.0 * total, 0.0);
    hipLaunchKernelGGL(gather_even_kernel, dim3((unsigned)std::min<int64_t>((total + 255) / 256, 16384)), dim3(256), 0, s, in, out,
                       H, W, OH, OW, total);
    SISIC_HIP(hipGetLastError());
    return SISIC_OK;
}

// ================================================================ cross-entropy head =================================
// torch.nn.functional.cross_entropy(logits, labels, weight = w, reduction = "mean"):
//   loss = sum_b w[y_b] * (lse_b - logits[b,y_b]) / sum_b w[y_b],   dlogits[b,k] = w[y_b] / sum_b' w[y_b'] * (softmax_b[k] - [k == y_b])
// One workgroup: thread t owns samples t, t + 256, ... (ascending), the 256 partial sums meet in a fixed tree, in double.
__global__ void __launch_bounds__(256)
ce_head_kernel(const float* __restrict__ logits, const int* __restrict__ labels, const float* __restrict__ w, int B, int n,
               float* __restrict__ loss, float* __restrict__ dlogits) {
    __shared__ double num[256], den[256];
    const int tid = threadIdx.x;
    double a = 0.0, d = 0.0;
    for (int b = tid; b < B; b += 256) {
        const float* lg = logits + (size_t)b * n;
        float m = lg[0];
        for (int k = 1; k < n; ++k) m = fmaxf(m, lg[k]);
        float sum = 0.0f;
        for (int k = 0; k < n; ++k) sum += expf(lg[k] - m);
        const int y = labels[b];
        const float wb = w ? w[y] : 1.0f;
        a += (double)wb * (double)((m + logf(sum)) - lg[y]);
        d += (double)wb;
    }
    num[tid] = a;
    den[tid] = d;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) {
            num[tid] += num[tid + o];
            den[tid] += den[tid + o];
        }
        __syncthreads();
    }
    const double total_w = den[0];
    if (tid == 0) loss[0] = (float)(num[0] / total_w);
    for (int b = tid; b < B; b += 256) {
        const float* lg = logits + (size_t)b * n;
        float m = lg[0];
        for (int k = 1; k < n; ++k) m = fmaxf(m, lg[k]);
        float sum = 0.0f;
        for (int k = 0; k < n; ++k) sum += expf(lg[k] - m);
        const int y = labels[b];
        const float coef = (float)((double)(w ? w[y] : 1.0f) / total_w);
        for (int k = 0; k < n; ++k) dlogits[(size_t)b * n + k] = coef * (expf(lg[k] - m) / sum - (k == y ? 1.0f : 0.0f));
    }
}

int launch_ce_head(sisic_ctx* ctx, const float* logits, const int* labels, const float* w, int B, int n, float* loss,
                   float* dlogits, hipStream_t s) {
    SISIC_REQUIRE(logits && labels && loss && dlogits && B > 0 && n > 0, "ce_head: bad arguments");
    ProfileScope prof(ctx, s, PK_OTHER, 8.0 * B * n, 0.0);
    hipLaunchKernelGGL(ce_head_kernel, dim3(1), dim3(256), 0, s, logits, labels, w, B, n, loss, dlogits);
    SISIC_HIP(hipGetLastError());
    return SISIC_OK;
}

// ================================================================ head backward =====================================
// logits = fc(mean_p act):  g[b,c,p] = [act > 0] / HW * sum_k W[k,c] dlogits[b,k]
//                           dW[k,c] = sum_b dlogits[b,k] * mean_p act[b,c,p]      db[k] = sum_b dlogits[b,k]
// One workgroup per channel c; the sums over b run in ascending b, those over p in ascending p.
__global__ void __launch_bounds__(256)
fc_head_bwd_kernel(const float* __restrict__ dlogits, const float* __restrict__ fc_w, const float* __restrict__ act,
                   float* __restrict__ g, float* __restrict__ dfc_w, float* __restrict__ dfc_b, int B, int C, int HW, int n) {
    extern __shared__ float sm[];
    float* pooled = sm;            // [B]
    float* dpool = sm + B;         // [B]
    const int c = blockIdx.x, tid = threadIdx.x;
    const float inv = 1.0f / (float)HW;
    for (int b = tid; b < B; b += 256) {
        const float* a = act + ((size_t)b * C + c) * HW;
        float sum = 0.0f;
        for (int p = 0; p < HW; ++p) sum += a[p];
        pooled[b] = sum * inv;
        float d = 0.0f;
        for (int k = 0; k < n; ++k) d += fc_w[(size_t)k * C + c] * dlogits[(size_t)b * n + k];
        dpool[b] = d * inv;
    }
    __syncthreads();
    for (int k = tid; k < n; k += 256) {
        float sw = 0.0f, sb = 0.0f;
        for (int b = 0; b < B; ++b) {
            const float dl = dlogits[(size_t)b * n + k];
            sw += dl * pooled[b];
            sb += dl;
        }
        dfc_w[(size_t)k * C + c] = sw;
        if (c == 0) dfc_b[k] = sb;
    }
    const int total = B * HW;
    for (int i = tid; i < total; i += 256) {
        const int b = i / HW, p = i % HW;
        const size_t e = ((size_t)b * C + c) * HW + p;
        g[e] = act[e] > 0.0f ? dpool[b] : 0.0f;
    }
}

int launch_fc_head_bwd(sisic_ctx* ctx, const float* dlogits, const float* fc_w, const float* act, float* g, float* dfc_w,
                       float* dfc_b, int B, int C, int HW, int n, hipStream_t s) {
    SISIC_REQUIRE(dlogits && fc_w && act && g && dfc_w && dfc_b && B > 0 && C > 0 && HW > 0 && n > 0, "fc_head_bwd: bad arguments");
    SISIC_REQUIRE(B <= 4096 && (int64_t)B * HW < (int64_t(1) << 31), "fc_head_bwd: batch %d", B);
    ProfileScope prof(ctx, s, PK_OTHER, 8.0 * B * C * HW, 0.0);
    hipLaunchKernelGGL(fc_head_bwd_kernel, dim3(C), dim3(256), 2 * (size_t)B * sizeof(float), s, dlogits, fc_w, act, g, dfc_w,
                       dfc_b, B, C, HW, n);
    SISIC_HIP(hipGetLastError());
    return SISIC_OK;
}

// ================================================================ fold / unfold =====================================
// the forward convolves with w' = w * sc[co], so d loss / d w = sc[co] * d loss / d w'   (sc in double, as at load time)
__global__ void __launch_bounds__(256)
unfold_grad_kernel(float* __restrict__ g, const double* __restrict__ sc, int64_t per, int64_t numel) {
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < numel; e += (int64_t)gridDim.x * blockDim.x)
        g[e] = (float)((double)g[e] * sc[e / per]);
}

int launch_unfold_grad(sisic_ctx* ctx, float* g, const double* sc, int cout, int cin, int k, hipStream_t s) {
    SISIC_REQUIRE(g && sc && cout > 0 && cin > 0 && k > 0, "unfold_grad: bad arguments");
    const int64_t per = (int64_t)cin * k * k, numel = per * cout;
    hipLaunchKernelGGL(unfold_grad_kernel, dim3((unsigned)std::min<int64_t>((numel + 255) / 256, 2048)), dim3(256), 0, s, g, sc,
                       per, numel);
    SISIC_HIP(hipGetLastError());
    return SISIC_OK;
}

// raw[co][ci][t] = (float)((double)w[co][ci][t] * sc[co]),  raw_t[ci][co][kk-1-t] = the same value (raw_t may be NULL)
__global__ void __launch_bounds__(256)
refold_kernel(const float* __restrict__ w, const double* __restrict__ sc, float* __restrict__ raw, float* __restrict__ raw_t,
              int cout, int cin, int kk, int64_t numel) {
    const int64_t per = (int64_t)cin * kk;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < numel; e += (int64_t)gridDim.x * blockDim.x) {
        const int co = (int)(e / per);
        const int64_t rem = e - (int64_t)co * per;
        const int ci = (int)(rem / kk), t = (int)(rem - (int64_t)ci * kk);
        const float f = (float)((double)w[e] * sc[co]);
        raw[e] = f;
        if (raw_t) raw_t[((int64_t)ci * cout + co) * kk + (kk - 1 - t)] = f;
    }
}

int launch_refold(sisic_ctx* ctx, const float* w, const double* sc, float* raw, float* raw_t, int cout, int cin, int k,
                  hipStream_t s) {
    SISIC_REQUIRE(w && sc && raw && cout > 0 && cin > 0 && k > 0, "refold: bad arguments");
    const int64_t numel = (int64_t)cout * cin * k * k;
    hipLaunchKernelGGL(refold_kernel, dim3((unsigned)std::min<int64_t>((numel + 255) / 256, 2048)), dim3(256), 0, s, w, sc, raw,
                       raw_t, cout, cin, k * k, numel);
    SISIC_HIP(hipGetLastError());
    return SISIC_OK;
}

}  // namespace sisic
