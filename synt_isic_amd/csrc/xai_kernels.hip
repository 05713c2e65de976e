// xai_kernels.hip -- stage 2 of the explainability pipeline (xai/XAI.py:1454-1700, :2822-2896) as two launches:
//   * intervene_kernel   : every counterfactual image of a run -- (frame, region mask, intervention type) jobs -- in one launch
//   * cfi_metrics_kernel : the classifier's logits of the originals and of the modified images -> every causal-shift number
// and the device work of stages 5 and 6 (:1845-1904, :2056-2059):
//   * resample_diffs_kernel   : the bootstrap and permutation resamples of the mean difference, one thread per resample
//   * randomize_weight_kernel : a classifier weight replaced by seeded normals, written in its BatchNorm-folded forms
// The reference builds one image at a time with a Python loop over channels and spends 18 batch-1 classifier forwards per
// image on the metrics.  This is latency work (tens of jobs of 12k-150k floats): one workgroup per job, and every reduction
// (channel mean, standard deviation, the four statistics) runs in a fixed order, so that a job's bits depend on nothing but
// the job.  Built with -ffp-contract=off like elementwise.hip: the noise blocks of noise_device.h keep their bits.
#include "common.h"
#include "noise_device.h"

namespace sisic {

constexpr int IV_THREADS = 1024;
constexpr int IV_WAVES = IV_THREADS / 64;
constexpr int IV_JOB_PACK = 64;              // jobs per launch: the table travels as a launch argument (no device buffer to own)
constexpr int IV_MAX_BLUR = 31;
constexpr int IV_TILE = 64;                  // box filter: output tile edge; the row sums of a tile and its halo live in LDS
constexpr int IV_TILE_ROWS = IV_TILE + IV_MAX_BLUR - 1;
constexpr uint32_t IV_NOISE_TAG = 2u;        // noise_device.h tag of the intervention noise (0: sampling loop, 1: x_T)

struct IvJob {
    uint64_t seed;
    int frame, mask, type, k;                // k: the odd box edge (blur / inpaint), 0 otherwise
    float noise_std;
    int pad;
};
struct IvJobPack { IvJob j[IV_JOB_PACK]; };

// ---- fixed-order workgroup reductions: butterfly inside a wave, then the waves' values summed in index order ----------------
__device__ __forceinline__ double block_sum(double v, double* red) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    __syncthreads();                          // red may still be read from the previous reduction
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < IV_WAVES; ++w) s += red[w];
    return s;
}

__device__ __forceinline__ float block_max(float v, double* red) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v = fmaxf(v, __shfl_xor(v, d, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = (double)v;
    __syncthreads();
    float m = 0.0f;
#pragma unroll
    for (int w = 0; w < IV_WAVES; ++w) m = fmaxf(m, (float)red[w]);
    return m;
}

struct IvAcc {
    double cover = 0.0, diff = 0.0, strength = 0.0;
    float dmax = 0.0f;
};

// one element: blend, clamp, store, statistics.  m is 0 or 1, so both products are exact and the blend is the image or the
// intervention bit for bit; the clamp covers the whole image (XAI.py:1572-1575)
__device__ __forceinline__ void iv_emit(float img, float iv, float m, int64_t e, float* __restrict__ out,
                                        float* __restrict__ iv_out, IvAcc& acc) {
#pragma clang fp contract(off)
    float mod = img * (1.0f - m) + iv * m;
    mod = fminf(fmaxf(mod, -1.0f), 1.0f);
    out[e] = mod;
    if (iv_out) iv_out[e] = iv;
    const float d = fabsf(img - mod);
    acc.cover += (double)m;
    acc.diff += (double)d;
    acc.strength += (double)fabsf(iv);
    acc.dmax = fmaxf(acc.dmax, d);
}

enum { IV_NOISE = 0, IV_GAUSSIAN_NOISE = 1, IV_ZERO = 2, IV_MEAN = 3, IV_BLUR = 4, IV_INPAINT = 5, IV_SHUFFLE = 6, IV_TYPES = 7 };

// frames [F,C,H,W]; masks uint8 [M,H,W]; src_index int32 [jobs,C,HW] or NULL; out / iv_out [jobs,C,H,W]; stats [jobs,4]
// (the pointers are already offset to the first job of this launch)
__global__ void __launch_bounds__(IV_THREADS)
intervene_kernel(const float* __restrict__ frames, const uint8_t* __restrict__ masks, const int* __restrict__ src_index,
                 float* __restrict__ out_all, float* __restrict__ iv_all, float* __restrict__ stats, IvJobPack jobs, int C,
                 int H, int W) {
    __shared__ float rows[IV_TILE_ROWS * IV_TILE];
    __shared__ double red[IV_WAVES];
    __shared__ float chan_mean[64];

    const IvJob job = jobs.j[blockIdx.x];
    const int tid = threadIdx.x;
    const int HW = H * W;
    const int64_t n = (int64_t)C * HW;
    const float* __restrict__ img = frames + (int64_t)job.frame * n;
    const uint8_t* __restrict__ msk = masks + (int64_t)job.mask * HW;
    float* __restrict__ out = out_all + (int64_t)blockIdx.x * n;
    float* __restrict__ iv_out = iv_all ? iv_all + (int64_t)blockIdx.x * n : nullptr;
    IvAcc acc;

    if (job.type == IV_BLUR || job.type == IV_INPAINT) {
        // k x k box average, stride 1, zero padding k/2, divisor k*k (avg_pool2d with count_include_pad): row sums of a tile and
        // its k-1 halo rows into LDS, then column sums over them -- 2k additions per pixel instead of k*k
        const int k = job.k, r = k >> 1;
        const float div = (float)(k * k);
        const int tiles_x = (W + IV_TILE - 1) / IV_TILE, tiles_y = (H + IV_TILE - 1) / IV_TILE;
        const int nrows = IV_TILE + 2 * r;
        for (int c = 0; c < C; ++c) {
            const float* __restrict__ plane = img + (int64_t)c * HW;
            for (int t = 0; t < tiles_x * tiles_y; ++t) {
                const int y0 = (t / tiles_x) * IV_TILE, x0 = (t % tiles_x) * IV_TILE;
                for (int i = tid; i < nrows * IV_TILE; i += IV_THREADS) {
                    const int gy = y0 - r + i / IV_TILE, gx = x0 + (i % IV_TILE);
                    float s = 0.0f;
                    if (gy >= 0 && gy < H && gx < W) {
                        const int lo = max(gx - r, 0), hi = min(gx + r, W - 1);
                        const float* __restrict__ row = plane + (int64_t)gy * W;
                        for (int x = lo; x <= hi; ++x) s += row[x];
                    }
                    rows[i] = s;
                }
                __syncthreads();
                for (int i = tid; i < IV_TILE * IV_TILE; i += IV_THREADS) {
                    const int ly = i / IV_TILE, lx = i % IV_TILE;
                    const int y = y0 + ly, x = x0 + lx;
                    if (y < H && x < W) {
                        float s = 0.0f;
                        for (int d = 0; d < k; ++d) s += rows[(ly + d) * IV_TILE + lx];
                        const int p = y * W + x;
                        iv_emit(plane[p], s / div, msk[p] ? 1.0f : 0.0f, (int64_t)c * HW + p, out, iv_out, acc);
                    }
                }
                __syncthreads();
            }
        }
    } else {
        float scale = job.noise_std;               // the factor of z (noise types)
        if (job.type == IV_GAUSSIAN_NOISE) {
            // max(noise_std, 0.5 * std(image)): unbiased standard deviation over the image's C*H*W values, two passes in double
            double s = 0.0;
            for (int64_t e = tid; e < n; e += IV_THREADS) s += (double)img[e];
            const double mean = block_sum(s, red) / (double)n;
            double q = 0.0;
            for (int64_t e = tid; e < n; e += IV_THREADS) {
                const double d = (double)img[e] - mean;
                q += d * d;
            }
            const double var = n > 1 ? block_sum(q, red) / (double)(n - 1) : 0.0;
            scale = fmaxf(job.noise_std, (float)(0.5 * sqrt(var)));
        } else if (job.type == IV_MEAN) {
            for (int c0 = 0; c0 < C; c0 += 64) {   // channel means in groups of 64 (the LDS row)
                const int cn = min(64, C - c0);
                for (int c = 0; c < cn; ++c) {
                    const float* __restrict__ plane = img + (int64_t)(c0 + c) * HW;
                    double s = 0.0;
                    for (int p = tid; p < HW; p += IV_THREADS) s += (double)plane[p];
                    const double tot = block_sum(s, red);
                    if (tid == 0) chan_mean[c] = (float)(tot / (double)HW);
                }
                __syncthreads();
                for (int64_t e = (int64_t)c0 * HW + tid; e < (int64_t)(c0 + cn) * HW; e += IV_THREADS) {
                    const int c = (int)(e / HW), p = (int)(e - (int64_t)c * HW);
                    iv_emit(img[e], chan_mean[c - c0], msk[p] ? 1.0f : 0.0f, e, out, iv_out, acc);
                }
                __syncthreads();
            }
        }
        if (job.type == IV_NOISE || job.type == IV_GAUSSIAN_NOISE) {
            // one Philox block per four consecutive elements of the job's image: the values of sisic_noise_fill(seed, step 0, tag 2)
            const int64_t nq = (n + 3) >> 2;
            for (int64_t q = tid; q < nq; q += IV_THREADS) {
                const float4 z4 = noise_normal4(job.seed, (uint32_t)q, 0u, IV_NOISE_TAG);
                const float z[4] = {z4.x, z4.y, z4.z, z4.w};
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int64_t e = 4 * q + i;
                    if (e < n) {
                        const int p = (int)(e % HW);
                        iv_emit(img[e], z[i] * scale, msk[p] ? 1.0f : 0.0f, e, out, iv_out, acc);
                    }
                }
            }
        } else if (job.type == IV_ZERO) {
            for (int64_t e = tid; e < n; e += IV_THREADS)
                iv_emit(img[e], 0.0f, msk[(int)(e % HW)] ? 1.0f : 0.0f, e, out, iv_out, acc);
        } else if (job.type == IV_SHUFFLE) {
            // intervention[c, p] = image[c, src_index[c, p]]; an index outside the plane reads the pixel itself
            const int* __restrict__ src = src_index + (int64_t)blockIdx.x * n;
            for (int64_t e = tid; e < n; e += IV_THREADS) {
                const int c = (int)(e / HW), p = (int)(e - (int64_t)c * HW);
                const int sp = src[e];
                const float iv = img[(int64_t)c * HW + ((unsigned)sp < (unsigned)HW ? sp : p)];
                iv_emit(img[e], iv, msk[p] ? 1.0f : 0.0f, e, out, iv_out, acc);
            }
        }
    }

    const double cover = block_sum(acc.cover, red), diff = block_sum(acc.diff, red), strength = block_sum(acc.strength, red);
    const float dmax = block_max(acc.dmax, red);
    if (tid == 0) {
        float* st = stats + (int64_t)blockIdx.x * 4;
        st[0] = (float)(cover / (double)n);
        st[1] = (float)(diff / (double)n);
        st[2] = dmax;
        st[3] = (float)(strength / (double)n);
    }
}

int launch_intervene(sisic_ctx* ctx, const float* frames, int F, const uint8_t* masks, int M, int C, int H, int W, int J,
                     const sisic_intervention_job* jobs, const uint64_t* seeds, const int32_t* src_index, float* out,
                     float* intervention_out, float* stats, hipStream_t s) {
    SISIC_REQUIRE(frames && masks && out && stats && jobs && seeds, "intervene: null argument");
    SISIC_REQUIRE(F > 0 && M > 0 && J > 0 && C > 0 && H > 0 && W > 0, "intervene: empty frames, masks, jobs or image");
    SISIC_REQUIRE((int64_t)C * H * W < ((int64_t)1 << 31), "intervene: an image of %d x %d x %d floats is too large", C, H, W);
    // everything the kernel indexes with is checked here: no job table makes it read outside frames / masks / src_index
    for (int j = 0; j < J; ++j) {
        const sisic_intervention_job& jb = jobs[j];
        SISIC_REQUIRE(jb.frame >= 0 && jb.frame < F, "intervene: job %d uses frame %d of %d", j, jb.frame, F);
        SISIC_REQUIRE(jb.mask >= 0 && jb.mask < M, "intervene: job %d uses mask %d of %d", j, jb.mask, M);
        SISIC_REQUIRE(jb.type >= 0 && jb.type < IV_TYPES,
                      "intervene: job %d has unknown intervention type %d (0 noise, 1 gaussian_noise, 2 zero, 3 mean, 4 blur, "
                      "5 inpaint, 6 shuffle)", j, jb.type);
        if (jb.type == IV_BLUR)
            SISIC_REQUIRE(jb.blur_kernel >= 1 && (jb.blur_kernel | 1) <= IV_MAX_BLUR, "intervene: job %d blur kernel %d (1 .. %d)",
                          j, jb.blur_kernel, IV_MAX_BLUR);
        if (jb.type == IV_SHUFFLE) SISIC_REQUIRE(src_index != nullptr, "intervene: job %d is a shuffle but src_index is NULL", j);
    }
    const int64_t n = (int64_t)C * H * W;
    ProfileScope prof(ctx, s, PK_OTHER, 4.0 * (double)n * J * (intervention_out ? 3.0 : 2.0), 0.0);
    for (int j0 = 0; j0 < J; j0 += IV_JOB_PACK) {
        const int nj = std::min(IV_JOB_PACK, J - j0);
        IvJobPack pack = {};
        for (int i = 0; i < nj; ++i) {
            const sisic_intervention_job& src = jobs[j0 + i];
            IvJob& jb = pack.j[i];
            jb.seed = seeds[j0 + i];
            jb.frame = src.frame;
            jb.mask = src.mask;
            jb.type = src.type;
            jb.k = src.type == IV_BLUR ? (src.blur_kernel | 1) : src.type == IV_INPAINT ? 5 : 0;    // an even edge becomes k + 1
            jb.noise_std = src.noise_std;
        }
        hipLaunchKernelGGL(intervene_kernel, dim3(nj), dim3(IV_THREADS), 0, s, frames, masks,
                           src_index ? src_index + (int64_t)j0 * n : nullptr, out + (int64_t)j0 * n,
                           intervention_out ? intervention_out + (int64_t)j0 * n : nullptr, stats + (int64_t)j0 * 4, pack, C, H, W);
        SISIC_HIP(hipGetLastError());
    }
    return SISIC_OK;
}

// ---- causal-shift metrics -------------------------------------------------------------------------------------------------
// softmax of one logit row in fp32 with the maximum subtracted; score(c) = log(p_c + 1e-8).  Where p_c > 1/2 the score is
// formed from the OTHER classes' mass, log1p(1e-8 - sum_{i != c} p_i): the same number without the cancellation in p_c near
// 1, where delta = |cfi| / (|score| + 1e-8) divides by it.
struct SoftmaxRow {
    const float* l;
    int n;
    float mx, sum;
    __device__ __forceinline__ void init(const float* logits, int n_) {
        l = logits;
        n = n_;
        mx = l[0];
        for (int i = 1; i < n; ++i) mx = fmaxf(mx, l[i]);
        sum = 0.0f;
        for (int i = 0; i < n; ++i) sum += expf(l[i] - mx);
    }
    __device__ __forceinline__ float prob(int c) const { return expf(l[c] - mx) / sum; }
    __device__ __forceinline__ float score(int c, float p) const {
        if (p <= 0.5f) return logf(p + 1e-8f);
        float rest = 0.0f;
        for (int i = 0; i < n; ++i)
            if (i != c) rest += expf(l[i] - mx);
        return log1pf(1e-8f - rest / sum);
    }
};

constexpr int CFI_JOB_PACK = 512;            // jobs per launch: the job -> frame map travels as a launch argument
struct CfiFramePack { int f[CFI_JOB_PACK]; };

// logits_mod / rows are already offset to the first job of this launch
__global__ void __launch_bounds__(64)
cfi_metrics_kernel(const float* __restrict__ logits_orig, const float* __restrict__ logits_mod, CfiFramePack job_frame, int J,
                   int n, float* __restrict__ rows) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= J) return;
    SoftmaxRow o, m;
    o.init(logits_orig + (int64_t)job_frame.f[j] * n, n);
    m.init(logits_mod + (int64_t)j * n, n);
    float* row = rows + (int64_t)j * (6 * n + 7);
    int arg_o = 0, arg_m = 0;
    float max_o = -1.0f, max_m = -1.0f, kl = 0.0f, js = 0.0f, tv = 0.0f;
    for (int c = 0; c < n; ++c) {
        const float po = o.prob(c), pm = m.prob(c);
        const float so = o.score(c, po), sm = m.score(c, pm);
        const float cfi = so - sm;
        row[6 * c + 0] = so;
        row[6 * c + 1] = sm;
        row[6 * c + 2] = cfi;
        row[6 * c + 3] = fabsf(cfi) / (fabsf(so) + 1e-8f);
        row[6 * c + 4] = po;
        row[6 * c + 5] = pm;
        if (po > max_o) { max_o = po; arg_o = c; }          // first maximum, like torch.argmax
        if (pm > max_m) { max_m = pm; arg_m = c; }
        // F.kl_div(log q, p, 'sum') = sum p (log p - log q), a term with p = 0 is 0
        const float lmid = logf((po + pm) * 0.5f + 1e-8f);
        const float lpo = po > 0.0f ? logf(po) : 0.0f, lpm = pm > 0.0f ? logf(pm) : 0.0f;
        if (po > 0.0f) {
            kl += po * (lpo - logf(pm + 1e-8f));
            js += 0.5f * po * (lpo - lmid);
        }
        if (pm > 0.0f) js += 0.5f * pm * (lpm - lmid);
        tv += 0.5f * fabsf(po - pm);
    }
    float* tail = row + 6 * n;
    tail[0] = (float)arg_o;
    tail[1] = (float)arg_m;
    tail[2] = max_o;
    tail[3] = max_m;
    tail[4] = kl;
    tail[5] = js;
    tail[6] = tv;
}

int launch_cfi_metrics(sisic_ctx* ctx, const float* logits_orig, int F, const float* logits_mod, int J, int n,
                       const int* job_frame, float* rows, hipStream_t s) {
    SISIC_REQUIRE(logits_orig && logits_mod && job_frame && rows, "cfi_metrics: null argument");
    SISIC_REQUIRE(F > 0 && J > 0 && n > 0, "cfi_metrics: empty frames, jobs or classes");
    for (int j = 0; j < J; ++j)
        SISIC_REQUIRE(job_frame[j] >= 0 && job_frame[j] < F, "cfi_metrics: job %d uses frame %d of %d", j, job_frame[j], F);
    const int64_t row = 6 * (int64_t)n + 7;
    for (int j0 = 0; j0 < J; j0 += CFI_JOB_PACK) {
        const int nj = std::min(CFI_JOB_PACK, J - j0);
        CfiFramePack pack = {};
        for (int i = 0; i < nj; ++i) pack.f[i] = job_frame[j0 + i];
        hipLaunchKernelGGL(cfi_metrics_kernel, dim3(cdiv(nj, 64)), dim3(64), 0, s, logits_orig, logits_mod + (int64_t)j0 * n, pack,
                           nj, n, rows + (int64_t)j0 * row);
        SISIC_HIP(hipGetLastError());
    }
    return SISIC_OK;
}

// ---- bootstrap and permutation resamples of the statistics stage (xai/XAI.py:1845-1904) -------------------------------------
// One thread per resample; the N <= 4096 values (top followed by bottom) are staged once per workgroup in LDS as doubles.
// Resample r reads the words w[0..N-1] of the block stream (seed, step = r, tag): word j is word j & 3 of block j >> 2.  Every
// sum runs sequentially in index order in double and this file is built without FMA contraction, so a resample's bits are a
// function of (values, seed, r) alone (include/sisic.h states the two draws).
constexpr int RS_THREADS = 256;
constexpr int RS_MAX_VALUES = 4096;
constexpr uint32_t RS_TAG_BOOTSTRAP = 3u, RS_TAG_PERMUTATION = 4u;

__device__ __forceinline__ uint32_t word_of(const uint4& b, int k) { return k == 0 ? b.x : k == 1 ? b.y : k == 2 ? b.z : b.w; }

// comb: dev double [n_top + n_bottom]; the first boot_blocks workgroups draw bootstrap resamples, the others permutations
__global__ void __launch_bounds__(RS_THREADS)
resample_diffs_kernel(const double* __restrict__ comb, int n_top, int n_bottom, uint64_t seed, int n_bootstrap,
                      int n_permutations, int boot_blocks, double* __restrict__ boot_out, double* __restrict__ perm_out) {
    __shared__ double vals[RS_MAX_VALUES];
    const int N = n_top + n_bottom;
    for (int i = threadIdx.x; i < N; i += RS_THREADS) vals[i] = comb[i];
    __syncthreads();
    const bool boot = (int)blockIdx.x < boot_blocks;
    const int r = ((int)blockIdx.x - (boot ? 0 : boot_blocks)) * RS_THREADS + (int)threadIdx.x;
    if (r >= (boot ? n_bootstrap : n_permutations)) return;
    double s1 = 0.0, s2 = 0.0;
    uint4 blk = make_uint4(0u, 0u, 0u, 0u);
    if (boot) {
        for (int j = 0; j < N; ++j) {
            if ((j & 3) == 0) blk = noise_bits4(seed, (uint32_t)(j >> 2), (uint32_t)r, RS_TAG_BOOTSTRAP);
            const uint32_t w = word_of(blk, j & 3);
            if (j < n_top) s1 += vals[__umulhi(w, (uint32_t)n_top)];
            else s2 += vals[n_top + (int)__umulhi(w, (uint32_t)n_bottom)];
        }
        boot_out[r] = s1 / (double)n_top - s2 / (double)n_bottom;
    } else {
        // selection sampling (Knuth, TAOCP vol. 2, 3.4.2, Algorithm S): element i joins the n_top-subset with probability
        // need / (N - i); need reaches 0 exactly when n_top elements have been taken (the last candidates are taken for sure)
        int need = n_top;
        for (int i = 0; i < N; ++i) {
            if ((i & 3) == 0) blk = noise_bits4(seed, (uint32_t)(i >> 2), (uint32_t)r, RS_TAG_PERMUTATION);
            const uint32_t w = word_of(blk, i & 3);
            if ((int)__umulhi(w, (uint32_t)(N - i)) < need) {
                s1 += vals[i];
                --need;
            } else {
                s2 += vals[i];
            }
        }
        perm_out[r] = s1 / (double)n_top - s2 / (double)n_bottom;
    }
}

int launch_resample_diffs(sisic_ctx* ctx, const double* top, int n_top, const double* bottom, int n_bottom, uint64_t seed,
                          int n_bootstrap, int n_permutations, double* boot_out, double* perm_out, hipStream_t s) {
    SISIC_REQUIRE(top && bottom, "resample_diffs: null top or bottom");
    SISIC_REQUIRE(n_top >= 1 && n_bottom >= 1 && (int64_t)n_top + n_bottom <= RS_MAX_VALUES,
                  "resample_diffs: n_top = %d, n_bottom = %d (each at least 1, at most %d together)", n_top, n_bottom, RS_MAX_VALUES);
    SISIC_REQUIRE(n_bootstrap >= 0 && n_permutations >= 0, "resample_diffs: negative resample count");
    SISIC_REQUIRE((n_bootstrap == 0) == (boot_out == nullptr), "resample_diffs: boot_out must be NULL exactly when n_bootstrap is 0");
    SISIC_REQUIRE((n_permutations == 0) == (perm_out == nullptr), "resample_diffs: perm_out must be NULL exactly when n_permutations is 0");
    if (n_bootstrap == 0 && n_permutations == 0) return SISIC_OK;
    const int N = n_top + n_bottom;
    std::vector<double> comb((size_t)N);
    for (int i = 0; i < n_top; ++i) comb[i] = top[i];
    for (int i = 0; i < n_bottom; ++i) comb[n_top + i] = bottom[i];
    // the values travel through a buffer of this call (at most 32 KB): the blocking copy reads the host arrays before the call
    // returns, and hipFree waits for the kernel.  A once-per-report call whose results the caller reads back at once.
    void* dev = nullptr;
    SISIC_HIP(hipSetDevice(ctx->device));
    SISIC_HIP(hipMalloc(&dev, (size_t)N * sizeof(double)));
    hipError_t e = hipMemcpy(dev, comb.data(), (size_t)N * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        const int boot_blocks = cdiv(n_bootstrap, RS_THREADS), perm_blocks = cdiv(n_permutations, RS_THREADS);
        hipLaunchKernelGGL(resample_diffs_kernel, dim3(boot_blocks + perm_blocks), dim3(RS_THREADS), 0, s,
                           static_cast<const double*>(dev), n_top, n_bottom, seed, n_bootstrap, n_permutations, boot_blocks,
                           boot_out, perm_out);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(s);
    }
    (void)hipFree(dev);
    SISIC_HIP(e);
    return SISIC_OK;
}

// ---- weight randomisation of the sanity check (xai/XAI.py:2056-2059) ---------------------------------------------------------
// w[e] = noise_normal1(seed, e, step = trial, tag) * strength replaces an OIHW convolution weight; the kernel writes what
// resnet.cpp's fold() would upload for it: raw[e] = (float)((double)w[e] * sc[co]) and, where raw_t is given, the tap-flipped
// transposed copy raw_t[ci][co][kk-1-t].  sc NULL (fc.weight): the values themselves.  One Philox block per four elements.
__global__ void __launch_bounds__(256)
randomize_weight_kernel(float* __restrict__ raw, float* __restrict__ raw_t, const double* __restrict__ sc, int64_t numel,
                        int cout, int cin, int kk, uint64_t seed, uint32_t trial, uint32_t tag, float strength) {
    const int64_t nq = (numel + 3) >> 2;
    const int64_t per = (int64_t)cin * kk;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += (int64_t)gridDim.x * blockDim.x) {
        const float4 z4 = noise_normal4(seed, (uint32_t)q, trial, tag);
        const float z[4] = {z4.x, z4.y, z4.z, z4.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t e = 4 * q + i;
            if (e >= numel) break;
            const float w = z[i] * strength;
            if (!sc) {
                raw[e] = w;
                continue;
            }
            const int co = (int)(e / per);
            const int64_t rem = e - (int64_t)co * per;
            const int ci = (int)(rem / kk), t = (int)(rem - (int64_t)ci * kk);
            const float f = (float)((double)w * sc[co]);
            raw[e] = f;
            if (raw_t) raw_t[((int64_t)ci * cout + co) * kk + (kk - 1 - t)] = f;
        }
    }
}

int launch_randomize_weight(sisic_ctx* ctx, float* raw, float* raw_t, const double* sc, int cout, int cin, int k, uint64_t seed,
                            uint32_t trial, uint32_t tag, float strength, hipStream_t s) {
    SISIC_REQUIRE(raw && cout > 0 && cin > 0 && k > 0, "randomize_weight: bad arguments");
    const int64_t numel = (int64_t)cout * cin * k * k;
    const int64_t nq = (numel + 3) >> 2;
    const int blocks = (int)std::min<int64_t>((nq + 255) / 256, 2048);
    hipLaunchKernelGGL(randomize_weight_kernel, dim3(blocks), dim3(256), 0, s, raw, raw_t, sc, numel, cout, cin, k * k, seed,
                       trial, tag, strength);
    SISIC_HIP(hipGetLastError());
    return SISIC_OK;
}

}  // namespace sisic
