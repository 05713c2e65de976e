/*
 * sisic.h -- C ABI of libsisic_hip.so, the MI355X (gfx950) implementation of the
 * SYNT_ISIC DDPM sampling hot path.
 *
 * The reference (fims9000/SYNT_ISIC) is pure Python: it has no FFI, the boundary
 * of its hot path is duck-typing on two third-party objects
 *     noise_pred = model(latents, t).sample                         core/generator/image_generator.py:400
 *     latents    = scheduler.step(noise_pred, t, latents).prev_sample               image_generator.py:403
 * built at core/generator/model_manager.py:173-194 (UNet2DModel) and :196-212
 * (DDPMScheduler).  A maintainer of the reference binds this library with
 * ctypes; synt_isic_amd/_lib.py is that binding.
 *
 * Conventions
 *   - every function returns 0 (SISIC_OK) or a negative SISIC_E* code; the message
 *     of the last failure on the calling thread is sisic_last_error();
 *   - "dev" pointers are device (HBM) addresses of contiguous fp32 NCHW tensors
 *     owned by the caller (torch); the library never frees or reallocates them;
 *   - weights are copied into a library-owned arena at load time; workspace is
 *     library-owned per handle and grows on demand (never inside the sampling loop);
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream);
 *     all work is enqueued asynchronously on it unless stated otherwise: a call returns while the stream may still be
 *     busy with earlier work, and its results are ordered behind that work.  The calls that wait for the stream say so
 *     below ("synchronis..."); besides those, a call that has to allocate or grow library memory -- the first call of a
 *     handle at a shape, a table that grows -- may wait for the device once;
 *   - handles are not thread-safe; use one handle per (device, stream): a handle serves one stream at a time, and the
 *     caller synchronises that stream before it passes the handle another one.  Threads that each own a handle and a
 *     stream may share a context ("Streams").
 */
#ifndef SISIC_H
#define SISIC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2 (round 4): sisic_sample_frames added; the packed-filter buffers grew in round 3 (1x1: three layouts = 3.5 x the
 * [Cin_pad][1][Cout_pad] floats; Winograd: the f32 U plus the bf16x3 split of it) -- ALWAYS size them with the *_numel
 * functions below, never from the layout comment. */
#define SISIC_ABI_VERSION 3

#define SISIC_OK 0
#define SISIC_EINVAL (-1)   /* bad argument / unsupported shape */
#define SISIC_EHIP (-2)     /* a HIP runtime call failed        */
#define SISIC_ESTATE (-3)   /* call order violated (e.g. forward before load) */
#define SISIC_ECANCEL (-4)  /* sampling loop stopped by the cancel flag */

typedef struct sisic_ctx sisic_ctx;     /* device context: weights-independent scratch */
typedef struct sisic_unet sisic_unet;   /* one UNet2DModel instance (weights + workspace) */
typedef struct sisic_resnet sisic_resnet; /* one ResNet18 classifier instance */

int sisic_abi_version(void);
const char* sisic_last_error(void);

/* ---- context ------------------------------------------------------------------ */
int sisic_create(int device_id, sisic_ctx** out);
int sisic_destroy(sisic_ctx* ctx);

/* ---- single operators (parity-test surface; also what the model executor calls) -- */

/* Generic NCHW fp32 convolution on the f32 MFMA pipe, replaces the F.conv2d /
 * GroupNorm / SiLU / cat / interpolate instances inside diffusers' ResnetBlock2D,
 * Downsample2D, Upsample2D and Attention projections.
 *   out[b,co,y,x] = bias[co] + chan_bias[b,co] + residual[b,co,y,x]
 *                 + sum_{ci,ky,kx} W[co,ci,ky,kx] * act(in[b,ci,...])
 * where `in` is the channel concatenation of in0 (c0 channels) and in1 (c1 channels,
 * may be NULL), optionally nearest-upsampled 2x, and act(v) is the optional
 * GroupNorm-apply prologue v*gn_scale[b,ci]+gn_shift[b,ci] followed by SiLU when
 * gn_silu != 0.  Zero padding ksize/2 is applied AFTER the prologue.            */
typedef struct sisic_conv_args {
    const float* in0;       /* dev [B,c0,Hin,Win]                        */
    const float* in1;       /* dev [B,c1,Hin,Win] or NULL                */
    int c0, c1;
    int B, Hin, Win;
    int upsample;           /* 1: nearest 2x before the conv; 2: zero insertion (source at the even
                               coordinates of the 2x grid, zeros elsewhere) = the input side of a
                               transposed stride-2 convolution (classifier backward-to-input)        */
    int ksize;              /* 1, 3 or 7                                  */
    int stride;             /* 1 or 2                                     */
    const float* w_packed;  /* dev, layout of sisic_conv_pack_weights     */
    const float* bias;      /* dev [Cout] or NULL                         */
    int Cout;
    const float* gn_scale;  /* dev [B,c0+c1] or NULL (no prologue)        */
    const float* gn_shift;  /* dev [B,c0+c1] or NULL                      */
    int gn_silu;
    const float* chan_bias; /* dev [B,Cout] or NULL                       */
    int chan_bias_stride;   /* floats between samples of chan_bias; 0 = one row shared by all samples */
    const float* residual;  /* dev [B,Cout,Hout,Wout] or NULL; MAY BE `out` itself (in-place accumulate, out += conv(...)):
                             * every kernel reads a residual element in the thread that stores that element, before the
                             * store (tests/test_gpu_kernels.py::test_conv_residual_may_alias_out).  No other argument
                             * may overlap `out`.                         */
    int relu;               /* 1: max(0, .) after everything (classifier) */
    float* out;             /* dev [B,Cout,Hout,Wout]                     */
    int tile_cfg;           /* 0 = auto; >0 forces a tile configuration (tests/tuning) */
    const float* w_winograd; /* dev, layout of sisic_conv_winograd_pack, or NULL: when given, 3x3 stride-1
                                convolutions may run as Winograd F(2x2,3x3) (tile_cfg 60..74 force a form; 74 = the
                                fp32-equivalent bf16x3 form, the automatic choice for whole 64-channel x 16x16-pixel
                                tiles; 1x1: tile_cfg 28 = the bf16x3 pointwise kernel, 20 = the f32 one).
                                For ksize 3, stride 2 the field carries the layout of sisic_conv_s2_pack instead, or NULL:
                                when given, the convolution may run with fp32-equivalent products on the bf16 matrix pipe
                                (tile_cfg 36 forces it; needs no upsample, no GroupNorm prologue, c1 == 0, c0 % 8 == 0 and
                                Cout % 64 == 0 -- everything else runs the f32 kernel as with NULL)                  */
    float* stats_out;        /* dev [B,Cout,slots,4] or NULL: each workgroup also writes (count, sum, sum of squared
                                deviations from its own mean, 0) of the values it stored, per image and channel, so that the GroupNorm
                                that follows needs sisic_groupnorm_finalize only (no second pass over `out`).
                                slots = sisic_conv_stats_slots(args); 0 there means "not available for this
                                launch" and stats_out must stay NULL                                          */
    /* Optional (ABI 3): the launch also FINALIZES the GroupNorm that reads its output alone -- groups over Cout, the module's
     * gamma / beta -- and leaves that layer's (scale, shift) [B,Cout] (what sisic_groupnorm_finalize would compute from
     * stats_out, bit for bit), so that no finalisation launch follows.  Only where sisic_conv_finalizes(args) says so
     * (today: the K-split 8x8-level forms with 8 channels per group); elsewhere the fields are ignored.                */
    const float* fin_gamma;  /* dev [Cout] or NULL (NULL: none of this)   */
    const float* fin_beta;   /* dev [Cout]                                */
    int fin_groups;
    float fin_eps;
    float* fin_scale;        /* dev [B,Cout] out                          */
    float* fin_shift;        /* dev [B,Cout] out                          */
    float* fin_mean_rstd;    /* dev [B,groups,2] out or NULL              */
} sisic_conv_args;

/* 1 when sisic_conv2d(args) with fin_gamma set will write fin_scale / fin_shift, 0 when the kernel selected for these
 * arguments does not (the caller then runs sisic_groupnorm_finalize on stats_out as before).                          */
int sisic_conv_finalizes(const sisic_conv_args* args);

/* Number of partial-statistics slots per (image, output channel) that sisic_conv2d(args) writes to
 * args->stats_out, or 0 when the kernel selected for these arguments does not produce them.      */
int sisic_conv_stats_slots(const sisic_conv_args* args);

/* What sisic_conv2d(args) would run, for tests and tools.  Host only: no device, no stream, nothing is launched.
 * Returns 0 when the launch would be made, 1 when args->tile_cfg forces a kernel form that does not take these arguments (the
 * launch's message goes to `refusal`, at most refusal_len bytes, NUL terminated), a negative error code for arguments no kernel
 * takes.  kernel / cfg / form (each may be NULL): the kernel family, the resolved tile configuration and the family's sub-form
 * as csrc/conv_plan.h numbers them (1x1 bf16x3 forms: 0 K-split, 1 staged, 2 / 3 64- / 32-pixel items, 4 staged K-split).      */
int sisic_conv_plan_info(const sisic_conv_args* args, int* kernel, int* cfg, int* form, char* refusal, int refusal_len);

/* Winograd-domain filters U = G g G^T of an OIHW 3x3 weight, computed in float64:
 * number of floats, and dev OIHW -> dev packed [Cin_pad][16][Cout_pad], FOLLOWED by the same filters split into three bf16
 * terms in the operand order of the bf16x3 kernels (pack_device.h).  The buffer must hold sisic_conv_winograd_numel floats:
 * more than the f32 layout alone.                                                             */
int64_t sisic_conv_winograd_numel(int Cout, int Cin);
int sisic_conv_winograd_pack(sisic_ctx*, const float* w_oihw, int Cout, int Cin, float* u_packed, void* stream);

/* The split filter of the stride-2 3x3 kernel: an OIHW 3x3 weight as three bf16 terms per element in the operand order of
 * the bf16x3 kernel, [8-channel chunk][tap][64-channel tile][768 dwords], zero padded: number of floats (-1: bad shape), and
 * dev OIHW -> dev buffer of that many floats.  Passed as sisic_conv_args.w_winograd of a ksize 3, stride 2 convolution.  */
int64_t sisic_conv_s2_numel(int Cout, int Cin);
int sisic_conv_s2_pack(sisic_ctx*, const float* w_oihw, int Cout, int Cin, float* out, void* stream);

/* number of floats of the packed form of an OIHW weight [Cout,Cin,k,k] (-1: unsupported ksize).  For ksize 1 this is 3.5 x
 * the [Cin_pad][1][Cout_pad] layout: the direct kernel's, the pointwise kernel's and the bf16x3 split are all written. */
int64_t sisic_conv_packed_numel(int Cout, int Cin, int ksize);
/* dev OIHW -> dev packed [Cin_pad][k*k][Cout_pad] (+ the further layouts above), zero padded; w_packed must hold
 * sisic_conv_packed_numel floats */
int sisic_conv_pack_weights(sisic_ctx*, const float* w_oihw, int Cout, int Cin, int ksize,
                            float* w_packed, void* stream);
int sisic_conv2d(sisic_ctx*, const sisic_conv_args* args, void* stream);

/* GroupNorm statistics folded with the affine parameters (replaces the reduction
 * half of torch.nn.GroupNorm inside ResnetBlock2D.norm1/norm2, Attention.group_norm
 * and conv_norm_out):  for c in group g of sample b
 *     scale[b,c] = gamma[c]*rstd[b,g],  shift[b,c] = beta[c] - mean[b,g]*scale[b,c].
 * The input is the concatenation of in0/in1 as in sisic_conv_args; HW = H*W.      */
int sisic_groupnorm_stats(sisic_ctx*, const float* in0, int c0, const float* in1, int c1,
                          int B, int HW, int groups, float eps,
                          const float* gamma, const float* beta,
                          float* scale, float* shift, void* stream);

/* GroupNorm statistics from convolution-epilogue partials (sisic_conv_args.stats_out) instead of a pass
 * over the tensor: same outputs as sisic_groupnorm_stats for the concatenation of two producers'
 * outputs (stats1 NULL / c1 = 0 for one).  The partials are merged in float64 (sum of M2_i + n_i (mean_i - mean)^2) in a fixed order.
 * HW is accepted for symmetry with sisic_groupnorm_stats; the element counts travel with the partials.   */
int sisic_groupnorm_finalize(sisic_ctx*, const float* stats0, int c0, int slots0,
                             const float* stats1, int c1, int slots1,
                             int B, int HW, int groups, float eps,
                             const float* gamma, const float* beta,
                             float* scale, float* shift, void* stream);

/* sisic_conv2d(args) whose launch also CARRIES the finalisation sisic_groupnorm_finalize(stats0 .. shift) would run, as extra
 * workgroups ahead of the convolution's own: for a GroupNorm that neither reads this convolution's output nor feeds its
 * prologue (a ResNet block's norm1 beside its 1x1 shortcut), so that it costs no launch.  Same bits as the two calls.
 * *carried = 1 when the kernel chosen for `args` ran the jobs -- the bf16x3 1x1 kernels (their 32-pixel, 64-pixel and K-split
 * forms) without a GroupNorm prologue; 0 when it did not: the convolution has run as sisic_conv2d would have, scale / shift are
 * untouched and the caller runs sisic_groupnorm_finalize itself.  The partials' B need not be the convolution's.             */
int sisic_conv2d_gn_rider(sisic_ctx*, const sisic_conv_args* args,
                          const float* stats0, int c0, int slots0,
                          const float* stats1, int c1, int slots1,
                          int B, int HW, int groups, float eps,
                          const float* gamma, const float* beta,
                          float* scale, float* shift, int* carried, void* stream);

/* Multi-head self-attention core (replaces scaled_dot_product_attention inside
 * diffusers' Attention, heads = C/head_dim, softmax in fp32, scale head_dim^-0.5).
 * qkv: dev [B,3*C,N] (q channels, then k, then v; channel = head*head_dim + d),
 * out: dev [B,C,N].  head_dim: 8 (the reference's attention_head_dim), 32 or 64; C a
 * multiple of it; any N >= 1.  8 runs attention.hip, 32 and 64 attention_wide.hip
 * (exact fp32 products on the matrix pipe); anything else is SISIC_EINVAL ("head_dim").
 * A sample's bits do not depend on the batch.  No allocation, no synchronisation.  */
int sisic_attention(sisic_ctx*, const float* qkv, float* out, int B, int C, int N, int head_dim,
                    void* stream);

/* Fused DDPMScheduler.step, elementwise over n floats:
 *   x0 = clamp((x - sqrt_beta_prod*eps)/sqrt_alpha_prod, -clip, clip)   (clip<=0: no clamp)
 *   out = (c0*x0 + c1*x) + sigma*z                                      (z==NULL or sigma==0: no noise)
 * evaluated in exactly that fp32 operation order (no FMA contraction).            */
int sisic_ddpm_step(sisic_ctx*, const float* eps, const float* x, const float* z, float* out,
                    int64_t n, float sqrt_beta_prod, float sqrt_alpha_prod, float c0, float c1,
                    float sigma, float clip, void* stream);

/* The scheduler-step rules of the sampling loop and what the floats of a step's table row mean under each:
 *   SISIC_RULE_DDPM   {sqrt_beta_prod, sqrt_alpha_prod, c0, c1, sigma}          sisic_ddpm_step above (ancestral sampling)
 *   SISIC_RULE_DDIM   {sqrt_beta_prod, sqrt_alpha_prod, c_prev, c_dir, sigma}   sisic_ddim_step below
 *   SISIC_RULE_DPMPP  {sqrt_beta_prod, sqrt_alpha_prod, cx, k0, sigma, k1}      sisic_dpmpp_step below (DPM-Solver++(2M))
 * A row is SISIC_RULE_ROW_WIDTH(rule) floats: 5, 5, 6.  sigma is column 4 under every rule.
 * rule_flags: SISIC_RULE_FLAG_CLIPPED_OUTPUT (DDIM only: use_clipped_model_output); 0 under DDPM and DPM-Solver++.        */
#define SISIC_RULE_DDPM 0
#define SISIC_RULE_DDIM 1
#define SISIC_RULE_DPMPP 2
#define SISIC_RULE_ROW_WIDTH(rule) ((rule) == SISIC_RULE_DPMPP ? 6 : 5)
#define SISIC_RULE_FLAG_CLIPPED_OUTPUT 1

/* ---- prediction type: what a model's output means ("the step contract per type") ---------------------
 * Every step rule starts from the model's estimate of x0.  Let o be the model's output (under guidance o_u + w * (o_c - o_u),
 * formed as ever), sb = sqrt_beta_prod, sa = sqrt_alpha_prod.  x0 before the clamp, one fp32 rounding per operation, no FMA:
 *   SISIC_PRED_EPSILON   x0 = (x - sb*o)/sa      the model predicts the noise (the default; the bits the library always gave)
 *   SISIC_PRED_SAMPLE    x0 = o                  the model predicts x0
 *   SISIC_PRED_V         x0 = sa*x - sb*o        the model predicts v = sa*eps - sb*x0 (Salimans & Ho 2022); no division, so
 *                                                nothing is amplified where sa is small (the first steps of a cosine schedule)
 * The clamp follows as documented at each rule.  DDPM and DPM-Solver++ change in this line only (hist stays the clamped x0).
 * DDIM's direction term pe: EPSILON o; SAMPLE (x - sa*x0)/sb with the UNCLAMPED x0 (needs sb != 0); V sa*o + sb*x; and with
 * use_clipped_model_output pe = (x - sa*x0_clamped)/sb under every type.  Noise, the edit epilogue and the guided write to
 * both halves are untouched.  sa == 0 (a zero-terminal-SNR table) stays refused under every type.
 *
 * Two owners, both set through stream-less setters (the kernels run on the stream the existing entry points receive):
 *   the CONTEXT's type says what the `eps` argument of the nine single-step entries means -- sisic_{ddpm,ddim,dpmpp}_step, their
 *     _rng and their _edit forms -- read when the entry is called.  UNet handles never read it.
 *   the HANDLE's type says what the UNet's output means: read by every sisic_sample* loop of the handle (plain, _rule, _rng,
 *     _cond, _edit; eager and graph-replayed) and by sisic_unet_train_step, _ext and _cond (the regression target below).  In
 *     graph mode the type is part of what a captured step is, like the rule and its flags: alternating types on one handle
 *     re-captures (sisic_unet_graph_builds), and a call under a type returns the bits it returned before the alternation.
 *     sisic_unet_forward* is unaffected: the network does not know what its output means.  A caller's rule_flags still accepts
 *     SISIC_RULE_FLAG_CLIPPED_OUTPUT only.
 * A type outside 0..2 is SISIC_EINVAL and leaves the setting as it was.                                                   */
#define SISIC_PRED_EPSILON 0
#define SISIC_PRED_SAMPLE  1      /* the model predicts x0 */
#define SISIC_PRED_V       2      /* v = sqrt(abar) * eps - sqrt(1 - abar) * x0 */
int sisic_set_step_prediction_type(sisic_ctx*, int type);      /* default EPSILON */
int sisic_step_prediction_type(const sisic_ctx*);

/* Fused DDIMScheduler.step (the published rule for epsilon prediction), elementwise over n floats.
 * With abar_t = alphas_cumprod[t], abar_prev = alphas_cumprod[prev_t] (or the final alpha when prev_t < 0),
 * variance = ((1 - abar_prev) / (1 - abar_t)) * (1 - abar_t / abar_prev) and sigma = eta * variance^0.5, the row is
 *   sqrt_beta_prod = (1 - abar_t)^0.5, sqrt_alpha_prod = abar_t^0.5, c_prev = abar_prev^0.5,
 *   c_dir = (1 - abar_prev - sigma^2)^0.5, sigma
 * and the step
 *   x0  = clamp((x - sqrt_beta_prod*eps)/sqrt_alpha_prod, -clip, clip)   (clip<=0: no clamp)
 *   pe  = eps, or (x - sqrt_alpha_prod*x0)/sqrt_beta_prod when use_clipped_model_output != 0
 *   out = (c_prev*x0 + c_dir*pe) + sigma*z                               (z==NULL or sigma==0: no noise)
 * evaluated in exactly that fp32 operation order (no FMA contraction).  out may be x.  sqrt_alpha_prod != 0, and
 * sqrt_beta_prod != 0 when use_clipped_model_output is set.                                                             */
int sisic_ddim_step(sisic_ctx*, const float* eps, const float* x, const float* z, float* out,
                    int64_t n, float sqrt_beta_prod, float sqrt_alpha_prod, float c_prev, float c_dir,
                    float sigma, float clip, int use_clipped_model_output, void* stream);

/* Fused DPM-Solver++(2M) step (Lu et al. 2022, the second-order multistep data-prediction solver with the midpoint rule, for
 * epsilon prediction), elementwise over n floats.  With alpha = abar^0.5, sigma_ = (1 - abar)^0.5,
 * lambda = ln alpha - ln sigma_ at this step's t, the next step's t' (abar = 1 after the last step) and the previous step's
 * t", h = lambda' - lambda and r = (lambda - lambda")/h, the host folds the published update into
 *   ODE ("dpmsolver++"):      cx = sigma_'/sigma_,            A = -alpha' * expm1(-h),   sigma = 0
 *   SDE ("sde-dpmsolver++"):  cx = (sigma_'/sigma_) * exp(-h), A = -alpha' * expm1(-2h),  sigma = sigma_' * (-expm1(-2h))^0.5
 *   first order:  k0 = A, k1 = 0          second order:  k0 = A * (1 + 1/(2r)), k1 = -A/(2r)
 * in float64, rounded to fp32 once.  The row is {sqrt_beta_prod = sigma_, sqrt_alpha_prod = alpha, cx, k0, sigma, k1}, the step
 *   x0   = clamp((x - sqrt_beta_prod*eps)/sqrt_alpha_prod, -clip, clip)  (clip<=0: no clamp)
 *   out  = ((cx*x + k0*x0) + k1*hist) + sigma*z                          (k1==0: hist is not read; z==NULL or sigma==0: no noise)
 *   hist = x0
 * evaluated in exactly that fp32 operation order (no FMA contraction).  hist: dev float [n], the previous step's x0, written
 * on every step and read only when k1 != 0: the first step of a run (k1 == 0) may be handed uninitialised memory.  out may be
 * x; hist is a buffer of its own.  sqrt_alpha_prod != 0.                                                                  */
int sisic_dpmpp_step(sisic_ctx*, const float* eps, const float* x, const float* z, float* hist, float* out,
                     int64_t n, float sqrt_beta_prod, float sqrt_alpha_prod, float cx, float k0, float sigma, float k1,
                     float clip, void* stream);

/* De-normalise image_generator.py:441-447: [B,3,H,W] fp32 -> uint8 [B,H,W,3],
 * trunc(clamp((x+1)/2,0,1)*255).                                                   */
int sisic_denorm_u8(sisic_ctx*, const float* x, uint8_t* out, int B, int C, int H, int W, void* stream);
/* The reference's three spellings of the same conversion, each in its own fp32 operation order:
 *   form 0  image_generator.py:441-447       trunc(clamp((x+1)/2, 0, 1) * 255)            (= sisic_denorm_u8)
 *   form 1  generate_test.py:94-97           trunc((clamp(x,-1,1) + 1) * 0.5 * 255)       (bit-equal to form 0)
 *   form 2  diffusion_generator.py:231-232   trunc(clip((x+1) * 127.5, 0, 255))           (bit-equal to form 0 as well:
 *           halving is exact in binary floating point, so (x+1)/2*255 and (x+1)*127.5 round the same real number once;
 *           tests/test_gpu_kernels.py::test_denorm_u8_three_reference_forms_bit_exact asserts it on every boundary)    */
int sisic_denorm_u8_form(sisic_ctx*, const float* x, uint8_t* out, int B, int C, int H, int W, int form, void* stream);

/* ---- UNet2DModel ---------------------------------------------------------------- */
typedef struct sisic_unet_config {
    int in_channels, out_channels;
    int layers_per_block;
    int n_blocks;                    /* <= 8 */
    int block_out_channels[8];
    int down_attn[8];                /* 1 = AttnDownBlock2D */
    int up_attn[8];                  /* 1 = AttnUpBlock2D   */
    int norm_groups;
    float norm_eps;
    int head_dim;                    /* 8, 32 or 64; every width that carries attention (down block i, up block
                                        n_blocks-1-i, the mid block) a multiple of it; at 8: every width */
    int n_freqs;                     /* block_out_channels[0] / 2 */
    const float* freqs;              /* host [n_freqs]: sinusoid frequencies (fp32, copied) */
} sisic_unet_config;

/* Host work only: the configuration is checked, the tensor list (sisic_unet_num_tensors / sisic_unet_tensor_name: diffusers
 * key names in state-dict order) is built, and the context pointer is KEPT, not read -- no device call is made before
 * sisic_unet_load.  The description of an architecture can therefore be queried where there is no GPU
 * (tests/test_arch_ref_cpu.py does, with a stand-in context).                                                           */
int sisic_unet_create(sisic_ctx*, const sisic_unet_config* cfg, sisic_unet** out);
/* The class-conditional UNet2DModel(num_class_embeds = N): one more tensor, class_embedding.weight [N, 4 *
 * block_out_channels[0]], directly after time_embedding.linear_2.bias in the state dict (diffusers registers class_embedding
 * between time_embedding and down_blocks), in the parameter, gradient, Adam and EMA arenas like every other.  Row
 * class_labels[b] is added to the time embedding of sample b before its SiLU.  num_class_embeds == 0 is sisic_unet_create.
 * A conditional handle is driven through the *_cond entry points; on it sisic_unet_forward, sisic_unet_train_forward,
 * sisic_unet_train_step[_ext] and the sisic_sample* loops return SISIC_EINVAL, as the *_cond entry points do on an
 * unconditional handle.  Classifier-free guidance keeps its "null" class as one more row: build the model with
 * n_classes + 1 rows.                                                                                                    */
int sisic_unet_create_cond(sisic_ctx*, const sisic_unet_config* cfg, int num_class_embeds, sisic_unet** out);
int sisic_unet_destroy(sisic_unet*);
/* number / names of the tensors load expects (diffusers state_dict key order) */
int sisic_unet_num_tensors(const sisic_unet*);
const char* sisic_unet_tensor_name(const sisic_unet*, int index);
/* Strict load of a flat state dict: n host pointers to contiguous fp32 tensors with
 * the given element counts; every expected tensor must be present exactly once.    */
int sisic_unet_load(sisic_unet*, int n, const char* const* names, const float* const* host_ptrs,
                    const int64_t* numels);
/* Latency mode (off by default): kernel choices that let ONE image fill the chip -- the reference generates its images one
 * at a time (image_generator.py:379, batch 1) -- at the price of extra partial-sum traffic that costs throughput at large
 * batches.  The choice depends on the layer shapes only, so results stay independent of the batch WITHIN a mode; between
 * the two modes results differ in the last bits (different summation order over the input channels).                  */
int sisic_unet_set_latency_mode(sisic_unet*, int on);
/* sisic_sample as one captured step (hipGraph) replayed T-1 times instead of ~190 launches per step from the host:
 * mode 1 on, 0 off, -1 (default) on exactly when latency mode is on.  Same kernels, same arithmetic, same bits; the
 * loop then runs on a library-owned copy of x (written back at the end) so that every address in the graph is stable.
 * The step is captured on the caller's stream.  The NULL stream cannot be captured: there the graph runs on a blocking stream
 * the handle owns (ordered with the NULL stream like any blocking stream), and the call synchronises it before it returns.  */
int sisic_unet_set_graph_mode(sisic_unet*, int mode);
/* How many times this handle has captured + instantiated the sampling step (a second sisic_sample at the same shape,
 * stream and mode replays the cached graph: the count does not move).                                                  */
int64_t sisic_unet_graph_builds(const sisic_unet*);
/* eps = model(sample, timestep).sample.  timesteps: host int64 [B] (one per sample). */
int sisic_unet_forward(sisic_unet*, const float* sample, const int64_t* timesteps,
                       float* out, int B, int H, int W, void* stream);
/* eps = model(sample, timestep, class_labels).sample of a conditional handle.  class_labels: host int64 [B]; a label outside
 * [0, num_class_embeds) is SISIC_EINVAL before anything is launched.  A sample's output bits depend on its own
 * (timestep, label) alone, never on the rest of the batch.                                                               */
int sisic_unet_forward_cond(sisic_unet*, const float* sample, const int64_t* timesteps, const int64_t* class_labels,
                            float* out, int B, int H, int W, void* stream);

/* The whole reverse-diffusion loop (image_generator.py:395-403) on one stream:
 *   for i in 0..T-1:  eps = unet(x, t[i]);  x = ddpm_step(eps, x, z[i], coef[i])
 * x: dev [B,C,H,W], updated in place (x_T in, x_0 out).
 * timesteps: host int64 [T].  coef: host float [T*5] = per step
 *   {sqrt_beta_prod, sqrt_alpha_prod, c0, c1, sigma}.
 * noise: dev [n_noise,B,C,H,W] consumed in order by the steps with sigma != 0, or NULL.
 * traj: dev [T,B,C,H,W] receiving x after every step, or NULL.
 * out_u8: dev uint8 [B,H,W,C] final de-normalised image, or NULL.
 * cancel: host int* polled between steps (non-zero stops the loop with SISIC_ECANCEL), or NULL.
 *   A non-NULL cancel makes the call synchronise the stream before step 0 and before every eighth step after it (the
 *   poll is worth something only while the host runs a bounded number of steps ahead); with NULL the loop is enqueued
 *   without waiting.  This holds for every sisic_sample* entry.
 * steps_done: host int* receiving the number of completed steps, or NULL.           */
int sisic_sample(sisic_unet*, float* x, int B, int H, int W, int T, const int64_t* timesteps,
                 const float* coef, float clip, const float* noise, float* traj, uint8_t* out_u8,
                 const volatile int* cancel, int* steps_done, void* stream);
/* The same loop keeping only SOME frames of the trajectory (xai/XAI.py:751-757 `save_indices`, :815-826: every N-th step and
 * the last one, or the steps whose t is a multiple of N): traj_row is a host int [T], traj_row[i] = the row of traj that
 * receives x after step i, or -1 for a step that is not kept (traj must hold max(traj_row)+1 rows of B*C*H*W floats).
 * traj_row NULL keeps every step in row i (= sisic_sample).                                                              */
int sisic_sample_frames(sisic_unet*, float* x, int B, int H, int W, int T, const int64_t* timesteps,
                        const float* coef, float clip, const float* noise, float* traj, const int* traj_row,
                        uint8_t* out_u8, const volatile int* cancel, int* steps_done, void* stream);

/* ---- device noise ("device noise contract") ------------------------------------------------------
 * z for image b (64-bit seed s_b), step index i of a run and element e of the image's n_per_image floats comes from one
 * Philox4x32-10 block per four consecutive elements: counter (e >> 2, i, tag, 0), key (s_b & 0xffffffff, s_b >> 32), words
 * (r0, r1) -> elements 4q, 4q+1 and (r2, r3) -> 4q+2, 4q+3 by Box-Muller (cos, sin) with u1 = ((r >> 8) + 1) * 2^-24,
 * u2 = (r >> 8) * 2^-24.  tag 0: the per-step noise of the sampling loop; tag 1: reserved for an x_T; tag 2: the noise
 * interventions of sisic_intervene; tag 3: the bootstrap resamples and tag 4: the permutation resamples of
 * sisic_resample_diffs (raw words, step = the resample); tag 5: the known-region noise and tag 6: the jump noise of the
 * edit epilogue (sisic_*_step_edit below); tag 7: the z of a noised classifier-training batch (the Python package's
 * train_classifier(noise_timesteps=...): step 0, one 64-bit seed per image); tag 16 + k: tensor k of a classifier randomised by
 * sisic_resnet_randomize (step = the trial).  A pure function of
 * (seed, step, tag, element): independent of the batch, the GPU count, graph or eager mode.  1 <= n_per_image <= 2^34.
 * seeds: HOST uint64 [B], read before the call returns.
 * sisic_noise_fill: out dev float [B, n_per_image];
 * sisic_noise_bits: the same blocks as raw words, out dev uint32 [B, 4 * ceil(n_per_image / 4)].                         */
int sisic_noise_fill(sisic_ctx*, float* out, int B, int64_t n_per_image, const uint64_t* seeds, uint32_t step,
                     uint32_t tag, void* stream);
int sisic_noise_bits(sisic_ctx*, uint32_t* out, int B, int64_t n_per_image, const uint64_t* seeds, uint32_t step,
                     uint32_t tag, void* stream);
/* sisic_ddpm_step over n = B * n_per_image floats with z generated in the kernel (tag 0) for step index `step`; unlike the
 * entries above, seeds is a DEVICE uint64 [B] (the caller's buffer: the sampling loop below keeps its own).  out may be x.
 * Any alignment and any n_per_image: tensors off a 16-byte line, or images that are not whole blocks, take an
 * element-by-element path with the same values.                                                                        */
int sisic_ddpm_step_rng(sisic_ctx*, const float* eps, const float* x, float* out, int B, int64_t n_per_image,
                        const uint64_t* seeds_dev, uint32_t step, float sqrt_beta_prod, float sqrt_alpha_prod, float c0,
                        float c1, float sigma, float clip, void* stream);
/* sisic_sample_frames with the per-step noise generated inside the scheduler-step kernel (tag 0) instead of read from a
 * buffer: bit-identical to sisic_sample_frames given rows filled by sisic_noise_fill(step = step0 + i) for the steps i with
 * sigma != 0.  seeds: HOST uint64 [B], read before the call returns.  step i of this call draws with step index step0 + i
 * (a run cut into several calls passes its offset; step0 >= 0).  Steps with sigma == 0 draw nothing.  In graph mode the
 * captured step of a shape serves every seed list and step0; buffer-noise and generated-noise calls capture different
 * steps, so alternating between the two at one shape re-captures (sisic_unet_graph_builds).                              */
int sisic_sample_frames_rng(sisic_unet*, float* x, int B, int H, int W, int T, const int64_t* timesteps,
                            const float* coef, float clip, const uint64_t* seeds, int step0, float* traj,
                            const int* traj_row, uint8_t* out_u8, const volatile int* cancel, int* steps_done,
                            void* stream);
/* sisic_ddim_step with z generated in the kernel: sisic_ddpm_step_rng's arguments and alignment rules, the DDIM row.     */
int sisic_ddim_step_rng(sisic_ctx*, const float* eps, const float* x, float* out, int B, int64_t n_per_image,
                        const uint64_t* seeds_dev, uint32_t step, float sqrt_beta_prod, float sqrt_alpha_prod, float c_prev,
                        float c_dir, float sigma, float clip, int use_clipped_model_output, void* stream);
/* sisic_dpmpp_step with z generated in the kernel: sisic_ddpm_step_rng's arguments and alignment rules, the DPM-Solver++
 * row and its history buffer.                                                                                            */
int sisic_dpmpp_step_rng(sisic_ctx*, const float* eps, const float* x, float* hist, float* out, int B, int64_t n_per_image,
                         const uint64_t* seeds_dev, uint32_t step, float sqrt_beta_prod, float sqrt_alpha_prod, float cx,
                         float k0, float sigma, float k1, float clip, void* stream);
/* sisic_sample_frames and sisic_sample_frames_rng under a chosen step rule:
 *   for i in 0..T-1:  eps = unet(x, t[i]);  x = step_rule(eps, x, z[i], coef[i])
 * rule: SISIC_RULE_DDPM (what the entries above run), SISIC_RULE_DDIM or SISIC_RULE_DPMPP; rule_flags: SISIC_RULE_FLAG_* of
 * that rule.  coef: host float, T rows of the rule's width (SISIC_RULE_ROW_WIDTH; see SISIC_RULE_* above).  Under every rule the steps with sigma != 0, and
 * only those, consume a noise row (buffer) or draw (generated noise): a DDIM run at eta = 0 has none, and takes noise NULL
 * or a buffer of no rows.  In graph mode the rule and its flags are part of what a captured step is, like the noise source:
 * a DDPM step is never replayed for a DDIM call or the other way round, and alternating re-captures
 * (sisic_unet_graph_builds).  Everything else as documented at sisic_sample_frames / sisic_sample_frames_rng.
 * SISIC_RULE_DPMPP: the handle owns the history buffer of the run.  A call starts with no history, so row 0 of a call must
 * be a first-order row (k1 == 0; SISIC_EINVAL otherwise), and a run cut into two calls is NOT bit-equal to the uncut run:
 * the second call's first step has to be first order where the uncut run's is second order.  Run it in one call.         */
int sisic_sample_frames_rule(sisic_unet*, float* x, int B, int H, int W, int T, const int64_t* timesteps,
                             const float* coef, float clip, int rule, int rule_flags, const float* noise, float* traj,
                             const int* traj_row, uint8_t* out_u8, const volatile int* cancel, int* steps_done,
                             void* stream);
int sisic_sample_frames_rule_rng(sisic_unet*, float* x, int B, int H, int W, int T, const int64_t* timesteps,
                                 const float* coef, float clip, int rule, int rule_flags, const uint64_t* seeds, int step0,
                                 float* traj, const int* traj_row, uint8_t* out_u8, const volatile int* cancel,
                                 int* steps_done, void* stream);

/* ---- class-conditional sampling and classifier-free guidance (Ho & Salimans 2022) ---------------------------------------
 * sisic_sample_frames_rule / _rule_rng for a conditional handle (sisic_unet_create_cond).  seeds == NULL: host-noise mode
 * (noise: a buffer or NULL, as in sisic_sample_frames_rule); otherwise device noise (noise must be NULL; seeds, step0 as in
 * sisic_sample_frames_rule_rng).  class_labels: host int64 [B], one label per image, each in [0, num_class_embeds).
 *   guidance_scale == 1:  one UNet pass per step at batch B under the given labels; null_label is not read.  This is plain
 *                         conditional sampling, and bit-identical to a guided run whose unconditional half is ignored.
 *   any other scale w:    each step runs the UNet ONCE at batch 2B, the B images under their labels first, the same B images
 *                         under null_label second, and the step rule is applied to
 *                             eps = eps_u + w * (eps_c - eps_u)
 *                         formed inside the step kernel in fp32 in exactly that order (subtract, multiply, add; no FMA
 *                         contraction).  The kernel writes the new x to both halves of a [2B] buffer the handle owns, so the
 *                         next pass needs no copy.  x, the noise rows, the Philox indexing, the DPM-Solver++ history, traj and
 *                         out_u8 stay B images wide.  w == 0 is the unconditional model at the cost of a guided step: pass
 *                         null labels at scale 1 instead.
 * Before the loop the projected embeddings of every (step, distinct label of the call) are computed in one batch; each row on
 * its own, so an image's result depends on its own (x, seed, label) alone and not on the batch it is in.  In graph mode a
 * captured step serves every label list and every w (they live in device tables); what changes its launches is part of its
 * key: conditional or not, guided or not (a call at w == 1 after one at w != 1 re-captures, and the other way round), and the
 * buffers -- the embedding table grows with T x distinct labels beyond 1000 rows and never shrinks.  As in the unconditional
 * loops, x holds the latent after the steps that ran under every exit, a cancelled run (SISIC_ECANCEL) included.         */
int sisic_sample_frames_cond(sisic_unet*, float* x, int B, int H, int W, int T, const int64_t* timesteps, const float* coef,
                             float clip, int rule, int rule_flags, const float* noise, const uint64_t* seeds, int step0,
                             const int64_t* class_labels, int null_label, float guidance_scale, float* traj,
                             const int* traj_row, uint8_t* out_u8, const volatile int* cancel, int* steps_done, void* stream);
/* out = eps_u + w * (eps_c - eps_u) over n floats with the device function the guided step kernels call (parity-test
 * surface: a caller's own loop over two sisic_unet_forward_cond passes, this and a sisic_*_step reproduces the guided loop
 * bit for bit).  Any alignment, any n >= 1; out may be either input.                                                      */
int sisic_guide_eps(sisic_ctx*, const float* eps_c, const float* eps_u, float w, float* out, int64_t n, void* stream);

/* ---- classifier guidance (Dhariwal & Nichol 2021, Alg. 2) ---------------------------------------------
 * An UNCONDITIONAL epsilon-prediction model is pushed towards a class by the input gradient of the ResNet18 classifier:
 *     k = scale * sb;   eps_hat = eps - k * g          (sb = sqrt(1 - abar_t), entry 0 of the step's row)
 * in fp32, k * g then the subtraction, one rounding per operation and no FMA contraction; the step rule is applied to eps_hat
 * as it is applied to classifier-free guidance's combined eps.  g = d log(softmax(clf(x_t))[c_b] + 1e-8) / d x_t is
 * sisic_resnet_input_gradient_targets at the step's latent, pre-processing included, with image b's own target c_b.  The
 * classifier is not time-conditioned, and its pre-processing clamps: g is zero wherever x_t lies outside [-1, 1].  A non-finite
 * g propagates into x; nothing guards it.
 *
 * sisic_clf_guide_eps: out = eps - (scale * sb) * g over n floats with the device function the guided step kernels call
 * (parity-test surface, as sisic_guide_eps is).  Any alignment, any n >= 1; out may be eps (not g).
 *
 * sisic_sample_frames_clf: sisic_sample_frames_rule_rng's loop with the classifier in it.  Per step, on ONE stream and in this
 * order: the UNet pass, the gradient walk on the loop's latent, the guided step kernel.  The fields that
 * sisic_sample_frames_rule_rng has mean what they mean there (x, B, H, W, T, timesteps, coef, clip, rule, rule_flags, seeds,
 * step0, traj, traj_row, out_u8, cancel); steps_done is an out field.  classifier: a loaded handle of the UNet's context;
 * targets: HOST int64 [B], image b's class, each in [0, num_classes); scale: finite, 0 gives the bits of the unguided loop.
 * noise must be NULL: the loop draws its noise on the device (host-noise mode is refused, as is seeds == NULL).
 * SISIC_EINVAL before anything is launched (steps_done = 0): a conditional handle, a handle whose prediction_type is not
 * epsilon, a noise buffer or no seeds, a classifier of another context or device, a classifier that is not loaded, H or W
 * above 224, a target outside [0, num_classes), a scale that is not finite.
 * In graph mode targets and scale live in a device table the UNet handle owns, so a captured step serves every target list
 * and every scale.  The classifier's activation blocks are sized by the eager step 0, as the UNet's are; the key of a captured
 * step holds "classifier-guided", the classifier handle and the generation of its workspace (a value no other state of any
 * handle in the process has, so a handle destroyed and created again at the same address does not match), which moves whenever the
 * classifier releases or derives its buffers again (a call at another input shape, sisic_resnet_load, train_begin /
 * train_end): the next guided call then re-captures (sisic_unet_graph_builds) and never replays onto freed blocks.  Weights
 * that change in place (sisic_resnet_optimizer_step, sisic_resnet_randomize / _restore) keep their buffers and need no
 * re-capture.                                                                                                                */
typedef struct sisic_clf_guide_args {
    const float* eps;
    const float* g;
    float*       out;
    void*        stream;
    int64_t      n;
    float        sb, scale;
} sisic_clf_guide_args;                    /* 48 bytes, no padding */
int sisic_clf_guide_eps(sisic_ctx*, sisic_clf_guide_args* args);
typedef struct sisic_sample_clf_args {
    float*              x;
    const int64_t*      timesteps;
    const float*        coef;
    const float*        noise;             /* must be NULL */
    const uint64_t*     seeds;
    sisic_resnet*       classifier;
    const int64_t*      targets;
    float*              traj;
    const int*          traj_row;
    uint8_t*            out_u8;
    const volatile int* cancel;
    void*               stream;
    int                 B, H, W, T;
    int                 rule, rule_flags, step0;
    int                 steps_done;        /* out */
    float               clip, scale;
} sisic_sample_clf_args;                   /* 136 bytes, no padding */
int sisic_sample_frames_clf(sisic_unet*, sisic_sample_clf_args* args);

/* ---- dynamic thresholding of x0 (Saharia et al. 2022, Imagen section 2.3) ------------------------------
 * The published schedulers' `thresholding`: per image, a high percentile s of |x0| replaces the static clamp range, and x0 is
 * divided by it.  For image b, with x0 the rule's estimate BEFORE any clamp (from the step's eps as the rule sees it: after
 * the guidance combine, under the prediction type), n = n_per_image and a_0 <= ... <= a_{n-1} the image's |x0| in order:
 *     r = fl32(fl32(ratio) * fl32(n - 1));   lo = floor(r);   hi = ceil(r);   w = fl32(r - lo);   d = fl32(a_hi - a_lo)
 *     q = w < 0.5 ? fma(w, d, a_lo) : fma(fl32(w - 1), d, a_hi)            ONE rounding: a fused multiply-add
 *     s = min(max(q, 1), sample_max_value);      x0' = min(max(x0, -s), s) / s
 * which is _threshold_sample with torch.quantile(abs, ratio, dim=1) spelled out, bit for bit.  A NaN anywhere in an image
 * gives s = NaN and a NaN image; infinities follow the formula.  Thresholding takes precedence over `clip` (the published
 * `if thresholding ... elif clip_sample`): the clip argument of a thresholded step is not read.  sample_max_value = 1 makes
 * s exactly 1: the bits of clip = 1.  DDIM's use_clipped_model_output re-derives its epsilon from x0'; DPM-Solver++ stores x0'
 * in its history.  s is exact selection by integer counting (radix select on the bit patterns of |x0|, one workgroup per
 * image), so two calls give equal bits; it is one more launch ahead of the step kernel on the step's stream.
 *
 * Two owners, as the prediction type has, both set through stream-less setters:
 *   the CONTEXT's setting is read by the nine single-step entries.  The _rng and _edit entries know their images; the three
 *     buffer-noise entries take n_per_image from sisic_set_step_image_elems (0, the default: refused while thresholding is on).
 *     s lies in a buffer the context owns per stream, grown (freed and allocated again, behind a synchronise of that stream) when a
 *     call brings more images than any before it on the stream: a caller who captures a thresholded single step into a graph of
 *     their own holds that address, and must capture again after a call with a larger batch on the same stream.
 *   the HANDLE's setting is read by every sisic_sample* loop of the handle, eager and graph-replayed, latency mode included.
 *     s [B] (B, not 2B, in a guided call) is owned by the handle.  The setting is part of what a captured step is: on -> off ->
 *     on re-captures, and never replays the other chain.
 * ratio = 0 switches thresholding off (the default).  SISIC_EINVAL, with the previous setting left in force: ratio outside
 * [0, 1] or not finite; sample_max_value below 1 or not finite.  A thresholded launch with n_per_image above 2^24 is
 * SISIC_EINVAL (n - 1 must be exact in fp32).
 *
 * sisic_x0_threshold: the selection alone, s [B] for images of n_per_image elements, under the context's prediction type.
 * source 0: eps as it stands; 1: classifier-free guidance, eps2 the null-label half and w the scale (eps2 + w * (eps - eps2));
 * 2: classifier guidance, eps2 the gradient g and w the scale (eps - (w * sb) * g; epsilon prediction only).  ratio may be 0
 * here (the image's smallest |x0|).  Any alignment.  s may alias none of eps, eps2 and x (SISIC_EINVAL), and in a thresholded step
 * none of the step's outputs.  A refused call has launched nothing.                                                                         */
int sisic_set_step_thresholding(sisic_ctx*, float ratio, float sample_max_value);
int sisic_set_step_image_elems(sisic_ctx*, int64_t n_per_image);
int sisic_unet_set_thresholding(sisic_unet*, float ratio, float sample_max_value);
typedef struct sisic_x0_threshold_args {
    const float* eps;
    const float* eps2;                     /* source 1, 2; else NULL */
    const float* x;
    float*       s;                        /* out: [B] */
    void*        stream;
    int64_t      n_per_image;
    int          B, source;
    float        sb, sa, w;
    float        ratio, sample_max_value;
    float        reserved;                 /* 0 */
} sisic_x0_threshold_args;                 /* 80 bytes, no padding */
int sisic_x0_threshold(sisic_ctx*, sisic_x0_threshold_args* args);

/* ---- image editing: the inpainting epilogue of the step kernels (RePaint, Lugmayr et al. 2022) -------
 * sisic_{ddpm,ddim,dpmpp}_step_rng with an epilogue applied to the rule's result u in the register that holds it, before the
 * store (no second pass over the latent).  Per element, one fp32 rounding per operation, no FMA contraction, in this order:
 *     k   = ck * x0k + sk * e1              (sk == 0: k = ck * x0k, e1 is not drawn)
 *     y   = m * k + (1 - m) * u             (m * k, 1 - m, (1 - m) * u, then the sum)
 *     out = ja * y + jb * e2                (jb == 0: out = y exactly, ja is not applied, e2 is not drawn)
 * x0k:  the known image, dev float [B, C, HW] in [-1, 1].  It must be FINITE everywhere, also where the mask is 0: the blend
 *       multiplies it by (a rounding of) 0, and 0 * NaN is NaN.
 * mask: dev float [B, 1, HW], broadcast over the C channels; 1 keeps the known pixel, 0 synthesises, values in between blend
 *       (soft seams).  n_per_image must equal C * HW.
 * e1, e2: the device-noise contract above with the image's seed at step index `step`, tag 5 (e1, the known region noised to
 *       the level the step arrives at) and tag 6 (e2, the jump back up the schedule).  z is drawn under tag 0 as in the _rng
 *       entries, or not at all when sigma == 0.
 * {ck, sk, ja, jb}: the edit row of the step.  For a step arriving at abar_prev: ck = abar_prev^.5, sk = (1 - abar_prev)^.5
 *       (the last step: 1, 0).  For a RePaint jump from there up to abar_target: ja = (abar_target / abar_prev)^.5,
 *       jb = (1 - abar_target / abar_prev)^.5, the j forward steps composed into one Gaussian draw; no jump: 1, 0.
 * sisic_dpmpp_step_edit: hist stays the model's predicted x0; the epilogue does not touch it.
 * Alignment: the vector path needs n_per_image % 4 == 0, HW % 4 == 0 (a float4 of the latent then maps to one float4 of the
 * mask row) and every tensor on a 16-byte line; anything else takes an element-by-element path with the same values.
 * out may be x; x0k and mask alias no output.  seeds_dev: DEVICE uint64 [B], as in the _rng entries.                      */
int sisic_ddpm_step_edit(sisic_ctx*, const float* eps, const float* x, float* out, int B, int64_t n_per_image,
                         const uint64_t* seeds_dev, uint32_t step, float sqrt_beta_prod, float sqrt_alpha_prod, float c0,
                         float c1, float sigma, float clip, const float* x0k, const float* mask, int C, int64_t HW, float ck,
                         float sk, float ja, float jb, void* stream);
int sisic_ddim_step_edit(sisic_ctx*, const float* eps, const float* x, float* out, int B, int64_t n_per_image,
                         const uint64_t* seeds_dev, uint32_t step, float sqrt_beta_prod, float sqrt_alpha_prod, float c_prev,
                         float c_dir, float sigma, float clip, int use_clipped_model_output, const float* x0k,
                         const float* mask, int C, int64_t HW, float ck, float sk, float ja, float jb, void* stream);
int sisic_dpmpp_step_edit(sisic_ctx*, const float* eps, const float* x, float* hist, float* out, int B, int64_t n_per_image,
                          const uint64_t* seeds_dev, uint32_t step, float sqrt_beta_prod, float sqrt_alpha_prod, float cx,
                          float k0, float sigma, float k1, float clip, const float* x0k, const float* mask, int C, int64_t HW,
                          float ck, float sk, float ja, float jb, void* stream);
/* The sampling loop with the epilogue in every step: sisic_sample_frames_cond's arguments in device-noise mode (seeds: HOST
 * uint64 [B], REQUIRED; there is no noise buffer), with class_labels == NULL meaning an unconditional handle (null_label and
 * guidance_scale are then not read), plus
 *   x0k:       dev float [B, C, H, W], mask: dev float [B, 1, H, W] (as above; neither is x),
 *   edit_rows: host float [T * 4], row i = {ck, sk, ja, jb} of step i, all finite.
 * timesteps may go up as well as down: after a jump (jb != 0) the next entry is a noisier level again (the expanded RePaint
 * schedule; the rule's row of an entry is that of its own timestep on the run's grid).  Step i draws z, e1 and e2 at step
 * index step0 + i, so a run cut into several calls (T <= 1000 per call) with their offsets is bit-equal to the uncut run
 * under DDPM and DDIM.  SISIC_RULE_DPMPP: every edit row must have jb == 0 (SISIC_EINVAL otherwise): a jump invalidates the
 * history.  traj frames are the values after the epilogue.  Eager and graph-replayed: in graph mode the handle keeps its
 * own copies of x0k, mask and edit_rows, so a captured step serves every image, mask and edit table at a shape; edited or not
 * is part of the key of a captured step, like the rule and guidance (alternating re-captures: sisic_unet_graph_builds).  A
 * call of another entry after this one returns the bits it returned before.                                               */
int sisic_sample_frames_edit(sisic_unet*, float* x, int B, int H, int W, int T, const int64_t* timesteps, const float* coef,
                             float clip, int rule, int rule_flags, const uint64_t* seeds, int step0,
                             const int64_t* class_labels, int null_label, float guidance_scale, const float* x0k,
                             const float* mask, const float* edit_rows, float* traj, const int* traj_row, uint8_t* out_u8,
                             const volatile int* cancel, int* steps_done, void* stream);

/* ---- training step (diffusion/train_diffusion.py:201-266) -----------------------------------
 * fp32 throughout.  The reference wraps the forward in torch.cuda.amp.autocast() (fp16 matmuls/convolutions) and scales the
 * loss with a GradScaler; here the GradScaler PROTOCOL is implemented (loss_scale multiplies d loss, the optimizer step
 * unscales, checks for inf/nan and skips), the arithmetic stays fp32.
 *
 * train_begin allocates the gradient and Adam (m, v) arenas (zeroed, step count 0) and the filters of the backward-data
 * convolutions; train_end frees them.  One tape at a time: train_forward records it, backward consumes it.           */
int sisic_unet_train_begin(sisic_unet*);
int sisic_unet_train_end(sisic_unet*);
/* DDPMScheduler.add_noise (train_diffusion.py:217): out[b] = sqrt_alpha_prod[b] * x0[b] + sqrt_one_minus_alpha_prod[b] *
 * noise[b]; the two coefficient rows are DEVICE arrays [B] (alphas_cumprod[t]**0.5 and (1 - alphas_cumprod[t])**0.5 as
 * fp32, built by the caller), per_sample = C*H*W.  Two products and one sum in fp32, no FMA: bit-equal to torch.        */
int sisic_add_noise(sisic_ctx*, const float* x0, const float* noise, const float* sqrt_alpha_prod,
                    const float* sqrt_one_minus_alpha_prod, float* out, int B, int64_t per_sample, void* stream);
/* noise_pred = model(noisy, timesteps).sample in training mode (train_diffusion.py:218): the inference kernels, every
 * activation and GroupNorm statistic kept for the backward pass.  timesteps: host int64 [B], one per sample.
 * `sample` is read again by sisic_unet_backward (conv_in's weight gradient): it must stay valid until then.
 * SISIC_EINVAL, before anything is recorded, when an attention level would hold more tokens than the attention backward
 * pass takes (136x136 trains, 144x144 does not; inference has no such limit).                                         */
int sisic_unet_train_forward(sisic_unet*, const float* sample, const int64_t* timesteps, float* out, int B, int H, int W,
                             void* stream);
/* The same for a conditional handle; the labels (host int64 [B]) are kept with the tape.  sisic_unet_backward then also fills
 * the gradient of class_embedding.weight: row k is the sum, in ascending sample order and without atomics, of the embedding
 * gradients of the samples labelled k; the row of a label absent from the batch is written as zero.                     */
int sisic_unet_train_forward_cond(sisic_unet*, const float* sample, const int64_t* timesteps, const int64_t* class_labels,
                                  float* out, int B, int H, int W, void* stream);
/* ---- ResnetBlock2D dropout ("dropout mask contract") ----------------------------------------------
 * UNet2DModel's `dropout` argument: in every ResnetBlock2D (down, mid and up: 22 in the default architecture)
 *   h = conv2(dropout(silu(norm2(h))))
 * and nothing else drops.  It applies exactly where a tape is recorded -- sisic_unet_train_forward[_cond] and the
 * sisic_unet_train_step* entries; sisic_unet_forward*, every sisic_sample* loop and so every evaluation never drop.  The new
 * kernels run on the stream those entry points receive.
 *
 * The handle holds (p, seed, call).  call starts at first_call and advances by one per tape-recording forward while p > 0.
 * For sample b, resnet block r (0-based, in execution order) and element e of that sample's [C,H,W] activation: word e & 3 of
 * the device-noise contract's Philox block with seed seed + b, block e >> 2, step = call, tag = 256 + r (the words
 * sisic_noise_bits returns for those arguments) gives u = (word >> 8) * 2^-24; the element is kept iff u >= p (an fp32
 * compare).  A kept value is a * inv_keep, inv_keep = fp32(1.0 / (1.0 - (double)p)): one rounding; a dropped value is +0.  The
 * backward pass regenerates the mask from (seed, call, r, b, e) -- nothing is stored -- with the values the forward that
 * recorded the tape used, whatever has been set since.  C*H*W is a multiple of 4 at every level of every model the library
 * builds; the kernels require it.
 * set_dropout: 0 <= p < 1 and finite, else SISIC_EINVAL with the previous setting left in force; p == 0 turns dropout off
 * (the launches of a handle that never had it).  dropout_next_call: the counter value the next tape-recording forward uses. */
int sisic_unet_set_dropout(sisic_unet*, float p, uint64_t seed, uint32_t first_call);
uint32_t sisic_unet_dropout_next_call(const sisic_unet*);
/* ---- training objective ------------------------------------------------------------------------------
 * sisic_unet_set_prediction_type (default SISIC_PRED_EPSILON): besides the sampling loops (above), the regression target of
 * sisic_unet_train_step, _ext and _cond: EPSILON the noise; SAMPLE the images; V  t = sa_b*noise - sb_b*x0 (two products, one
 * difference, fp32, no FMA) formed in the loss kernel's registers from the two coefficient rows the step already takes -- no
 * target tensor is written.  sisic_add_noise(x0 := noise, noise := x0, a = sa, c = -sb) gives the same bits as a tensor
 * (DDPMScheduler.get_velocity), so a step spelled out of the single entry points equals the fused one bit for bit.
 * sisic_unet_set_loss_weights: B per-sample weights (HOST fp32, finite; copied and kept until replaced or cleared by NULL or
 * B == 0), e.g. Min-SNR-gamma.  While set, with c = grad_scale * 2 / n:
 *     dpred = (c * w_b) * d,     loss = (sum of w_b * d^2) / n,     d = pred - target
 * in sisic_mse_loss (n % B must be 0, else SISIC_EINVAL) and in the train_step entries (their B must equal the weights' B, else
 * SISIC_EINVAL before anything is launched: a stale table is an error, never a silent loss).  Same fixed-order reduction; the
 * weights reach the device through the handle's upload ring on the consuming call's stream.  Weights of all ones give the
 * loss and dpred bits of no weights.                                                                                     */
int sisic_unet_set_prediction_type(sisic_unet*, int type);     /* default EPSILON; anything else SISIC_EINVAL, setting unchanged */
int sisic_unet_prediction_type(const sisic_unet*);
int sisic_unet_set_loss_weights(sisic_unet*, const float* weights_host, int B);   /* NULL / 0 clears */
/* F.mse_loss(pred, target) (train_diffusion.py:219): loss_dev[0] = mean((pred - target)^2) (NULL: kept internally),
 * dpred = grad_scale * 2 (pred - target) / n (NULL: loss only).  Fixed-order reduction.                               */
int sisic_mse_loss(sisic_unet*, const float* pred, const float* target, int64_t n, float grad_scale, float* loss_dev,
                   float* dpred, void* stream);
/* loss.backward() (train_diffusion.py:231): dout = d loss / d model output [B,C,H,W]; fills the gradient arena
 * (overwrites: one backward per step, like zero_grad(set_to_none=True) + backward) and releases the tape.              */
int sisic_unet_backward(sisic_unet*, const float* dout, void* stream);
int sisic_unet_zero_grad(sisic_unet*, void* stream);
/* scaler.step(optimizer) (train_diffusion.py:232-233) with torch.optim.Adam's update: gradients are multiplied by inv_scale,
 * m/v/step advance, parameters move, and every packed form of the weights is rebuilt.  lr, betas and eps are doubles, as
 * torch.optim.Adam holds them (1 - beta and lr / bias_correction are formed in double and rounded to fp32 once).  found_inf != NULL: the gradients are
 * first checked for inf/nan (one synchronisation); *found_inf = 1 skips the update like GradScaler.step does.           */
int sisic_unet_optimizer_step(sisic_unet*, double lr, double beta1, double beta2, double eps, float inv_scale, int* found_inf,
                              void* stream);
/* The whole loop body (train_diffusion.py:215-233) on one stream: add_noise, forward, MSE, backward, optimizer step.
 * images / noise: dev [B,C,H,W]; timesteps and the two add_noise coefficient rows: HOST arrays [B].
 * loss_out (host, may be NULL) receives the unscaled loss (one synchronisation).
 * The target has the input's shape, so the three fused steps need in_channels == out_channels, as the sisic_sample* loops
 * do: SISIC_EINVAL naming both counts otherwise, before anything is allocated or launched.                              */
int sisic_unet_train_step(sisic_unet*, const float* images, const float* noise, const int64_t* timesteps,
                          const float* sqrt_alpha_prod, const float* sqrt_one_minus_alpha_prod, int B, int H, int W, double lr,
                          double beta1, double beta2, double eps, float loss_scale, float* loss_out, int* found_inf, void* stream);
/* ---- global-norm gradient clipping and an exponential moving average of the weights -----------------------------------
 * What diffusers' unconditional training example wraps round the same UNet2DModel: torch.nn.utils.clip_grad_norm_ before
 * the optimizer step and EMAModel.step after it.  One path: every optimizer step of the library, the entry points above
 * included, is the same two passes -- a statistics pass over the gradient (run if and only if ext != NULL or found_inf !=
 * NULL; its 12-byte read-back is the one synchronisation) and one fused Adam + EMA pass, which reads the clip coefficient
 * from the statistics record when the first pass ran and takes it as 1 otherwise.  A plain step with found_inf == NULL is
 * the second pass alone: one launch, nothing waits.  The training kernels have no atomics at all.
 *
 * sisic_optim_ext (16 bytes; the double comes first so that the struct has no padding):
 *   ema_decay      at 0, double: the decay of THIS step (EMAModel.get_decay; the caller computes it per step)
 *   max_grad_norm  at 8, float:  clip_grad_norm_'s max_norm; <= 0 or +inf: the norm is reported, nothing is clipped
 *   ema_update     at 12, int:   1: ema = ema - (1 - ema_decay) * (ema - p_new) rides in the update pass (needs
 *                                sisic_unet_ema_begin); on a step that found_inf skips, the EMA moves towards the unchanged
 *                                weights, as EMAModel.step after a skipped scaler.step does
 * A NULL pointer means {0, 0, 0}.                                                                                        */
typedef struct sisic_optim_ext {           /* 16 bytes, no padding */
    double ema_decay;
    float  max_grad_norm;
    int    ema_update;
} sisic_optim_ext;
/* sisic_unet_optimizer_step / sisic_unet_train_step with the options above: one statistics pass over the gradient arena
 * (squares of fp32(g * inv_scale) summed in double in a fixed order; found_inf as before), one 12-byte read-back (one
 * synchronisation, also when found_inf is NULL), the skip decision on the host, one fused Adam + EMA pass, the same
 * rebuild of the packed weights.  Adam's arithmetic is that of sisic_unet_optimizer_step on (g * inv_scale) * clip_coef,
 * clip_coef = min(1, max_grad_norm / (norm + 1e-6)) in fp32 (a NaN norm gives a NaN coefficient, as torch's clamp does).
 * grad_norm_out (host, may be NULL): the norm of the unscaled gradient before clipping, what clip_grad_norm_ returns.   */
int sisic_unet_optimizer_step_ext(sisic_unet*, double lr, double beta1, double beta2, double eps, float inv_scale,
                                  const sisic_optim_ext* ext, int* found_inf, float* grad_norm_out, void* stream);
int sisic_unet_train_step_ext(sisic_unet*, const float* images, const float* noise, const int64_t* timesteps,
                              const float* sqrt_alpha_prod, const float* sqrt_one_minus_alpha_prod, int B, int H, int W, double lr,
                              double beta1, double beta2, double eps, float loss_scale, const sisic_optim_ext* ext,
                              float* loss_out, int* found_inf, float* grad_norm_out, void* stream);
/* sisic_unet_train_step_ext for a conditional handle: its arguments plus class_labels (host int64 [B]).  ext == NULL is the
 * plain step of sisic_unet_train_step (no statistics pass; grad_norm_out is not written).                              */
int sisic_unet_train_step_cond(sisic_unet*, const float* images, const float* noise, const int64_t* timesteps,
                               const int64_t* class_labels, const float* sqrt_alpha_prod,
                               const float* sqrt_one_minus_alpha_prod, int B, int H, int W, double lr, double beta1, double beta2,
                               double eps, float loss_scale, const sisic_optim_ext* ext, float* loss_out, int* found_inf,
                               float* grad_norm_out, void* stream);
/* The EMA arena.  ema_begin (after train_begin) allocates it and copies the current weights into it (EMAModel.__init__;
 * called again: copies again); train_end frees it.  ema_step is EMAModel.step on its own, for an EMA kept beside
 * sisic_unet_optimizer_step.  ema_swap exchanges the EMA with the trained weights and rebuilds every packed form, so that
 * every entry point that reads weights (forward, sample, read what = 0) sees the averaged ones; a second call swaps back.
 * While swapped, the optimizer_step / train_step entry points, ema_step, ema_begin and a reload return SISIC_ESTATE:
 * training on the averaged weights is always a bug.  ema_active: 0 no arena, 1 arena, 2 arena and currently swapped.     */
int sisic_unet_ema_begin(sisic_unet*);
int sisic_unet_ema_step(sisic_unet*, double ema_decay, void* stream);
int sisic_unet_ema_swap(sisic_unet*, void* stream);
int sisic_unet_ema_active(const sisic_unet*);
/* The two kernels on the caller's device vectors (parity-test surface; any n >= 1, pointers aligned to a float; scratch is
 * allocated per call).  grad_stats writes the record {float total_norm; float clip_coef; int found_inf} (3 x 4 bytes) to
 * stats_dev.  adam_ema: one Adam step number `step` (>= 1) on p, m, v from g, reading clip_coef from stats_dev (NULL: 1)
 * and updating ema (NULL: none) with ema_decay; with both NULL it is the update sisic_unet_optimizer_step launches (the
 * same kernel: there is one).
 * sisic_grad_stats: Synchronises the stream: the scratch is freed before the call returns.  sisic_adam_ema allocates
 * nothing and does not wait.                                                                                           */
int sisic_grad_stats(sisic_ctx*, const float* g, int64_t n, float inv_scale, float max_norm, void* stats_dev, void* stream);
int sisic_adam_ema(sisic_ctx*, float* p, const float* g, float* m, float* v, float* ema_or_null, int64_t n, double lr,
                   double beta1, double beta2, double eps, int64_t step, float inv_scale, const void* stats_dev_or_null,
                   double ema_decay, void* stream);
/* Copy one tensor of the state dict (index as in sisic_unet_tensor_name) to the host: what = 0 parameter, 1 gradient,
 * 2 Adam first moment, 3 Adam second moment, 4 EMA (after sisic_unet_ema_begin).  Synchronises the device.               */
int sisic_unet_read(sisic_unet*, int what, int index, float* host_out, int64_t numel);
/* The counterpart of sisic_unet_read (parity-test surface: optimizer tests choose their own gradients): copy one tensor
 * from the host into the gradient (what = 1), Adam first-moment (2), second-moment (3) or EMA (4, after
 * sisic_unet_ema_begin: EMAModel.load_state_dict) arena.  what = 0 is refused:
 * parameters have packed forms that must follow them, sisic_unet_load sets them.  Synchronises the device.              */
int sisic_unet_write(sisic_unet*, int what, int index, const float* host_in, int64_t numel);
int64_t sisic_unet_train_steps(const sisic_unet*);

/* Single-operator entry points of the backward pass (parity-test surface).
 * dW of a convolution: arguments as sisic_conv_args (prologue and index maps of the FORWARD convolution), dy = gradient of
 * its output, dw = OIHW [Cout, c0+c1, k, k].  Its K-split scratch is allocated per call.
 * Synchronises the stream: the scratch is freed before the call returns.                                               */
int sisic_conv2d_wgrad(sisic_ctx*, const sisic_conv_args* fwd_args, const float* dy, float* dw, void* stream);
/* attention backward: dqkv [B,3C,N] from qkv, the forward output o [B,C,N] and its gradient dO.  (o must be a valid
 * pointer but is not read: D_i = dO_i . o_i is formed from the recomputed probabilities)
 * head_dim 8: one workgroup per head with the head's rows in LDS, at most 1170 tokens.  head_dim 32 and 64: tiled over
 * keys and queries (two launches), at most 65536 tokens; the row statistics between the two launches live in a scratch
 * buffer of the context, one per stream: the first call on a stream at a larger B * heads * N allocates it and waits for
 * the stream once, later calls neither allocate nor wait.  More tokens, another head_dim or a C that is no multiple of
 * it: SISIC_EINVAL before any launch.  No atomics: two calls give equal bits.                                           */
int sisic_attention_bwd(sisic_ctx*, const float* qkv, const float* o, const float* dO, float* dqkv, int B, int C, int N,
                        int head_dim, void* stream);
/* GroupNorm(+SiLU) backward: a = act(GroupNorm(x)); given da, ADDS dx to dx_accum and writes dgamma, dbeta.
 * scale/shift: outputs of sisic_groupnorm_stats for x (recomputed here, into scratch allocated per call).
 * Synchronises the stream: the scratch is freed before the call returns.                                               */
int sisic_groupnorm_bwd(sisic_ctx*, const float* da, const float* x, int B, int C, int HW, int groups, float eps,
                        const float* gamma, const float* beta, int silu, float* dx_accum, float* dgamma, float* dbeta,
                        void* stream);

/* BatchNorm2d in training mode (batch statistics) over y dev [B,C,HW] (NCHW, a convolution output without bias), forward and
 * backward, on the caller's tensors.  One argument struct for both; the stream travels in it.
 *   forward  (sisic_batchnorm_train):     reads y, gamma, beta [C], residual (dev [B,C,HW] or NULL), relu, eps, momentum;
 *            writes mean, invstd = 1/sqrt(var + eps) [C] (var the biased variance over n = B*HW) and
 *            out = [relu](gamma (y - mean) invstd + beta [+ residual]); running_mean / running_var ([C], both or neither; NULL: no
 *            update) receive nn.BatchNorm2d's update rm <- (1-m) rm + m mean, rv <- (1-m) rv + m var n/(n-1), momentum m in (0, 1]
 *   backward (sisic_batchnorm_train_bwd): reads g = dL/d(out), y, mean, invstd, gamma and act (dev [B,C,HW] or NULL: the
 *            activation behind the BatchNorm's ReLU; g' = g where act > 0, else 0.  NULL: g' = g); writes dbeta = sum g',
 *            dgamma = sum g' xhat [C] and dy = gamma invstd (g' - dbeta/n - xhat dgamma/n), xhat = (y - mean) invstd.  dy is a
 *            buffer of its own (not g).
 * Moments: each workgroup reduces a slice of a channel to (count, mean, M2) by Welford's update, the slices are merged with
 * Chan's formula in double (never E[x^2] - E[x]^2).  No atomics: every summation order is a function of (B, C, HW) alone, two
 * calls give equal bits.  The slice partials live in a scratch buffer of the context, one per stream: the first call on a stream
 * at a larger C * slices allocates it and waits for the stream once, later calls neither allocate nor wait.
 * B * HW = 1 ("expected more than 1 value per channel when training"): SISIC_EINVAL before any launch.
 * out = NULL: the moments (and the running update) alone; dy = NULL: dgamma and dbeta alone -- how tools time each launch.
 * sisic_add_relu: out = relu(y + residual) over the B * C * HW elements, the elementwise pass the classifier's Grad-CAM path
 * already runs, here on the caller's tensors: the yardstick the BatchNorm passes are measured against.                      */
typedef struct sisic_bn_args {
    const float* y;
    const float* gamma;
    const float* beta;
    const float* residual;
    float*       running_mean;
    float*       running_var;
    float*       out;
    float*       mean;
    float*       invstd;
    const float* g;
    const float* act;
    float*       dy;
    float*       dgamma;
    float*       dbeta;
    void*        stream;
    double       momentum;
    float        eps;
    int          relu;
    int          B, C, HW;
    int          reserved;                 /* 0 */
} sisic_bn_args;                           /* 152 bytes, no padding */
int sisic_batchnorm_train(sisic_ctx*, sisic_bn_args* args);
int sisic_batchnorm_train_bwd(sisic_ctx*, sisic_bn_args* args);
int sisic_add_relu(sisic_ctx*, sisic_bn_args* args);

/* ---- ResNet18 classifier (xai/XAI.py:357-471): forward, explanations, training with frozen or batch-statistics BatchNorm ---- */
/* torchvision resnet18 with fc -> num_classes, eval mode (BatchNorm folded at load).  The state dict
 * uses the reference's key names, prefixed "model." (XAI.py:389), float tensors only: conv/fc weights
 * and biases, BatchNorm weight/bias/running_mean/running_var (num_batches_tracked is not a float tensor
 * and is not passed).                                                                         */
int sisic_resnet_create(sisic_ctx*, int num_classes, sisic_resnet** out);
int sisic_resnet_destroy(sisic_resnet*);
int sisic_resnet_num_tensors(const sisic_resnet*);
const char* sisic_resnet_tensor_name(const sisic_resnet*, int index);
int sisic_resnet_load(sisic_resnet*, int n, const char* const* names, const float* const* host_ptrs,
                      const int64_t* numels);
/* The weight randomisation of the sanity check (xai/XAI.py:2056-2059: param.data = randn_like(param) * strength for every
 * parameter with more than one dimension): the 20 convolution weights and fc.weight are REPLACED, element e of tensor k
 * (index as in sisic_resnet_tensor_name) by noise_normal(seed, element e, step = trial, tag = 16 + k) * strength, one fp32
 * multiply -- the values of sisic_noise_fill(out, 1, numel, &seed, trial, 16 + k) times strength.  BatchNorm vectors, running
 * statistics and fc.bias stay, so the folded biases stay.  The filters are generated on the device in their BatchNorm-folded
 * form (float)((double)w * gamma / sqrt(var + eps)), the scale in double as at load time, and every packed form is rebuilt in
 * the buffers the handle owns: nothing is uploaded or allocated.  The device then holds what sisic_resnet_load of that state
 * dict would leave, bit for bit.  Forward, input gradient and Grad-CAM use the new filters.
 * sisic_resnet_restore derives the filters of the loaded state dict again (the load path, blocking uploads);
 * sisic_resnet_load always leaves the handle un-randomised.                                                              */
int sisic_resnet_randomize(sisic_resnet*, uint64_t seed, uint32_t trial, float strength, void* stream);
int sisic_resnet_restore(sisic_resnet*, void* stream);
/* logits[B,num_classes] = classifier.forward(x).  preprocess=1: x is dev [B,3,H,W] in [-1,1] (the
 * sampler's latents) and goes through preprocess_for_classifier (XAI.py:399-431): clamp((x+1)/2,0,1),
 * bilinear resize to 224x224 (H,W <= 224), ImageNet normalisation.  preprocess=0: x is already the
 * normalised network input [B,3,H,W].                                                         */
int sisic_resnet_forward(sisic_resnet*, const float* x, float* logits, int B, int H, int W, int preprocess,
                         void* stream);
/* relu(bn1(conv1(preprocess(x)))): the stem activation [B,64,(S+1)/2,(S+1)/2] (S = 224 with preprocess=1) the max-pool
 * routes are chosen from -- introspection for parity tests of the backward pass.                              */
int sisic_resnet_stem(sisic_resnet*, const float* x, float* c1_out, int B, int H, int W, int preprocess, void* stream);
/* d score / d x of the classifier for score = log(softmax(logits)[target] + 1e-8) (xai/XAI.py:443-459), x = the raw
 * input in [-1,1] with the pre-processing differentiated through (clamp, bilinear 224x224, normalise): the gradient
 * captum's IntegratedGradients(forward_func = get_per_class_score) and the plain-gradient fallback of
 * xai/XAI.py:1039-1109 take.  grad_x: dev [B,3,H,W]; logits_out: dev [B,n_classes] or NULL.              */
int sisic_resnet_input_gradient(sisic_resnet*, const float* x, int B, int H, int W, int target,
                                float* grad_x, float* logits_out, void* stream);
/* The same gradient with one target per image: row b of grad_x is d log(softmax(logits_b)[targets[b]] + 1e-8) / d x_b.  The
 * walk is sisic_resnet_input_gradient's, launch for launch; only the head reads its class from a device table, so row b has
 * the bits of a single-target call with target = targets[b], and the logits are the forward's.  One argument struct that
 * carries the stream as a field:
 *   x           dev [B,3,H,W] in [-1,1], H, W <= 224
 *   targets     HOST int64 [B], each in [0, num_classes): every one is checked before anything is launched (SISIC_EINVAL)
 *   grad_x      dev [B,3,H,W];  logits_out: dev [B,num_classes] or NULL
 * The targets travel through a pinned ring of the handle: the call does not wait for its stream.                            */
typedef struct sisic_resnet_targets_args {
    const float*   x;
    const int64_t* targets;
    float*         grad_x;
    float*         logits_out;
    void*          stream;
    int            B, H, W, reserved;
} sisic_resnet_targets_args;               /* 56 bytes, no padding */
int sisic_resnet_input_gradient_targets(sisic_resnet*, sisic_resnet_targets_args* args);

/* Grad-CAM of the class logit on model.layer4[-1].conv2 as pytorch_grad_cam's GradCAM(target_layers=[...conv2]) with
 * ClassifierOutputTarget(target) computes it in xai/XAI.py:2945-3035 (pre-processing included): cam = relu(sum_k
 * mean(dlogit/dA_k) A_k), min-max scaled, bilinearly resized to 224x224, min-max scaled again.
 * cam: dev [B,224,224]; logits_out: dev [B,n_classes] or NULL.                                            */
int sisic_resnet_gradcam(sisic_resnet*, const float* x, int B, int H, int W, int target,
                         float* cam, float* logits_out, void* stream);

/* ---- training the classifier with BatchNorm frozen ("classifier training") --------------------------
 * torchvision.ops.FrozenBatchNorm2d semantics: running statistics, gamma and beta stay the constants they were loaded as, so
 * the training forward IS the folded forward above, bit for bit, and a trained model needs no other inference path.
 * Trainable tensors (22): the 20 convolution weights, fc.weight and fc.bias.  BatchNorm with batch statistics
 * (nn.BatchNorm2d in training mode, 62 trainable tensors) is the second mode, entered by sisic_resnet_train_begin_bn and
 * described behind the entries below; everything in this paragraph and the next ones speaks of the frozen mode.
 *
 * train_begin (after sisic_resnet_load) allocates arenas for the un-folded parameters, their gradients and the two Adam
 * moments, and the scratch of the K-split weight gradients; train_end frees them and leaves the handle as
 * sisic_resnet_load of the current state dict would leave it.  A reload (sisic_resnet_load) ends training as well.
 *
 * Both launching entries take one argument struct that carries the stream as a field:
 *   x              dev [B,3,H,W]: preprocess = 1 the sampler's latents in [-1,1] (H, W <= 224), 0 the normalised network input;
 *                  the stem's input (224x224, or HxW) must have even sizes from 8, and so must every plane a stride-2 layer reads
 *   labels         HOST int64 [B], each in [0, num_classes): checked before anything is launched
 *   class_weights  HOST float [num_classes] or NULL: torch.nn.functional.cross_entropy(weight = w, reduction = "mean"),
 *                  i.e. the weighted sum divided by the sum of the picked weights
 *   logits_out     dev [B,num_classes] or NULL: the forward's logits, the bits of sisic_resnet_forward
 *   loss           out (loss_backward): the loss; found_inf, grad_norm: out (optimizer_step)
 *   lr .. eps      torch.optim.Adam's constants, doubles as there; max_grad_norm: clip_grad_norm_'s max_norm, <= 0 or +inf: the
 *                  norm is reported, nothing is clipped
 * loss_backward: forward with the activations kept, cross-entropy head, the data-gradient walk of
 * sisic_resnet_input_gradient down to the stem's output, and at every convolution its weight gradient.  It OVERWRITES the
 * gradient arena and waits for the stream once (the loss is returned to the host).  No atomics: two calls from one state
 * give equal bits in every gradient, and an element's summation order is a function of (B, H, W) alone.
 * optimizer_step: the statistics pass of sisic_grad_stats over the gradient arena, one 12-byte read-back (one
 * synchronisation), then -- unless a gradient is not finite: found_inf = 1, nothing moves -- the Adam pass of sisic_adam_ema
 * on g * clip_coef, and every folded, transposed, packed and Winograd form rebuilt on the device in the buffers the handle
 * owns (the arithmetic of the load path: (float)((double)w * gamma / sqrt(var + eps))).  Nothing is uploaded or allocated.
 * Without train_begin both return SISIC_ESTATE.                                                                          */
typedef struct sisic_resnet_train_args {
    const float*   x;
    const int64_t* labels;
    const float*   class_weights;
    float*         logits_out;
    void*          stream;
    double         lr, beta1, beta2, eps;
    int            B, H, W, preprocess;
    float          max_grad_norm;
    float          loss;
    float          grad_norm;
    int            found_inf;
} sisic_resnet_train_args;                 /* 104 bytes, no padding */
int sisic_resnet_train_begin(sisic_resnet*);
int sisic_resnet_train_end(sisic_resnet*);
int sisic_resnet_loss_backward(sisic_resnet*, sisic_resnet_train_args* args);
int sisic_resnet_optimizer_step(sisic_resnet*, sisic_resnet_train_args* args);
int sisic_resnet_zero_grad(sisic_resnet*);                    /* zero-fills the gradient arena; synchronises the device */
int64_t sisic_resnet_train_steps(const sisic_resnet*);        /* optimizer steps that moved the weights; 0 outside training */
/* Copy one tensor (index as in sisic_resnet_tensor_name) to / from the host: what = 0 parameter, 1 gradient, 2 Adam first
 * moment, 3 Adam second moment.  Parameters can be read at any time after a load (during training: the trained values);
 * what = 1..3 need train_begin and one of the 22 trainable tensors (a BatchNorm tensor has no gradient: SISIC_EINVAL).
 * Writing parameters is refused: their folded and packed forms must follow them, sisic_resnet_load sets them.
 * Both synchronise the device.                                                                                            */
int sisic_resnet_read(sisic_resnet*, int what, int index, float* host_out, int64_t numel);
int sisic_resnet_write(sisic_resnet*, int what, int index, const float* host_in, int64_t numel);

/* ---- training the classifier with batch-statistics BatchNorm (nn.BatchNorm2d in training mode) ----------------------------
 * train_begin_bn: mode 0 (frozen) is exactly sisic_resnet_train_begin.  mode 1 (batch statistics) takes momentum in (0, 1]
 * (torch's momentum = None cumulative average is not offered); any other mode or momentum: SISIC_EINVAL.
 * In mode 1 the trainable tensors are 62 -- the 20 convolution weights, their 20 gamma and 20 beta, fc.weight and fc.bias -- side
 * by side in the four arenas in state-dict order; the 40 running statistics live in a buffer arena beside them.  A second set of
 * filter forms (transposed, packed, Winograd, and the transposes' forms) is allocated for the UNFOLDED weights.
 *   loss_backward   forward: every convolution with its unfolded filters and no bias, then the moments of its output, then the
 *                   apply pass (sisic_batchnorm_train's kernels); the pre-BatchNorm outputs and (mean, invstd) are kept beside the
 *                   activations.  The running statistics are updated here, once per call, as torch updates them in the forward.
 *                   logits_out are the training-mode logits.  backward: the walk of the frozen mode with a BatchNorm backward in
 *                   front of every weight gradient and transposed convolution (the stem and the downsample branch included), on
 *                   the unfolded transposed filters.  The geometry checks of the frozen mode, and B * h * w >= 2 at the last
 *                   plane.  Same determinism: two calls from one state give equal bits in every gradient.
 *   optimizer_step  the same statistics and Adam passes over the larger arena; then the unfolded forms the training forward
 *                   reads, and the folded inference forms from (w, gamma, beta, running_mean, running_var): sc = gamma /
 *                   sqrt(running_var + eps) and bias = (float)(beta - running_mean * sc) formed on the device in double, the load
 *                   path's arithmetic.  Both rebuilds run on EVERY call, also when found_inf skipped the update: the running
 *                   statistics moved.  After every optimizer_step the inference side of the handle (sisic_resnet_forward,
 *                   _input_gradient, _gradcam, _randomize) equals a fresh sisic_resnet_load of the current state dict bit for bit.
 *                   Between a loss_backward and the next optimizer_step the inference side lags by that one running-statistics
 *                   update.
 *   read / write    what = 0 returns the current value of any tensor; what = 1..3 work for the 62 trainable tensors, for a
 *                   running statistic they return SISIC_EINVAL.
 *   train_end       copies parameters and buffers back to the host copies (refreshing the inference side first if a
 *                   loss_backward moved the running statistics since the last optimizer_step) and frees the second set.
 * train_bn_mode: 0 frozen, 1 batch statistics, -1 outside training.                                                          */
typedef struct { int mode; double momentum; } sisic_resnet_bn_config;
int sisic_resnet_train_begin_bn(sisic_resnet*, const sisic_resnet_bn_config* config);
int sisic_resnet_train_bn_mode(const sisic_resnet*);

/* Bytes of activation workspace the handle currently keeps resident (its pool).  The pool is sized for the last
 * (B,H,W) seen and released when the shape changes, so this does not grow with the history of batch sizes
 * (the GUI's memory poll, main.py:230-253, would otherwise watch it climb).                                  */
int64_t sisic_resnet_workspace_bytes(const sisic_resnet*);
int64_t sisic_unet_workspace_bytes(const sisic_unet*);

/* get_confidence / get_per_class_score (XAI.py:443-471): prob[b] = softmax(logits[b])[target],
 * logscore[b] = log(prob[b] + 1e-8); either output may be NULL.                               */
int sisic_class_scores(sisic_ctx*, const float* logits, int B, int n_classes, int target, float* prob,
                       float* logscore, void* stream);
/* The masked copies of compute_shap_approximation (XAI.py:1147-1161): out[s,c,y,x] = image[c,y,x] where
 * masks[s, y/patch, x/patch] != 0, else 0.  image: dev [C,H,W]; masks: dev uint8 [S,H/patch,W/patch].  */
int sisic_mask_patches(sisic_ctx*, const float* image, const uint8_t* masks, float* out, int S, int C, int H, int W,
                       int patch, void* stream);

/* ---- counterfactual interventions and causal-shift metrics (xai/XAI.py:1454-1700, stage 2 of :2822-2896) ---------------
 * sisic_intervene builds J modified images in one launch (64 jobs per launch beyond that).  Job j takes frame
 * jobs[j].frame of frames (dev [F,C,H,W]) and mask jobs[j].mask of masks (dev uint8 [M,H,W], non-zero = inside the region,
 * shared by the channels) and writes
 *     out[j] = clamp(image * (1 - m) + intervention * m, -1, 1)
 * The clamp covers the WHOLE image as in the reference (XAI.py:1575): values of an early-trajectory latent outside [-1, 1]
 * change outside the mask too.  m is 0 or 1, so inside [-1, 1] the blend is the image or the intervention bit for bit.
 * intervention, by jobs[j].type:
 *   0 noise           z * noise_std
 *   1 gaussian_noise  z * max(noise_std, 0.5 * std(image)), std = the unbiased standard deviation of the image's C*H*W values
 *   2 zero            0
 *   3 mean            the channel's mean over H x W
 *   4 blur            blur_kernel x blur_kernel box average, stride 1, zero padding k/2, divisor k*k (F.avg_pool2d); an even
 *                     blur_kernel becomes k + 1 (XAI.py:1513); 1 <= k <= 31
 *   5 inpaint         the 5 x 5 box average with zero padding (XAI.py:1530-1538)
 *   6 shuffle         intervention[c, p] = image[c, src_index[j, c, p]]: the caller's permutation of the masked pixels of
 *                     every channel (identity elsewhere); an index outside 0 .. H*W-1 reads pixel p itself
 * z: the device-noise contract above with seeds[j] (HOST uint64 [J]), step 0 and tag 2 -- element e of job j is element e of
 * sisic_noise_fill(out, J, C*H*W, seeds, 0, 2), a pure function of (seed, element).
 * src_index: dev int32 [J,C,H*W], read by shuffle jobs only; may be NULL when no job is a shuffle.
 * intervention_out: dev [J,C,H,W] receiving the intervention itself, or NULL.
 * stats: dev [J,4] = mask coverage (mean of m), mean |image - out|, max |image - out|, mean |intervention|
 * (the 'statistics' of XAI.py:1587-1593).
 * Every reduction runs in a fixed order inside the job's own workgroup: a job's output depends on the job alone, not on its
 * position in the table or on the other jobs, and two runs are bit-equal.  Any C, H, W.  The job table is validated before
 * anything is launched: a frame or mask index out of range, an unknown type, a blur kernel out of range or a shuffle
 * without src_index return SISIC_EINVAL.                                                                              */
typedef struct sisic_intervention_job {
    int frame;          /* row of frames, 0 .. F-1 */
    int mask;           /* row of masks, 0 .. M-1  */
    int type;           /* 0 .. 6, see above        */
    int blur_kernel;    /* type 4 only              */
    float noise_std;    /* types 0 and 1            */
} sisic_intervention_job;
int sisic_intervene(sisic_ctx*, const float* frames, int F, const uint8_t* masks, int M, int C, int H, int W, int J,
                    const sisic_intervention_job* jobs, const uint64_t* seeds, const int32_t* src_index, float* out,
                    float* intervention_out, float* stats, void* stream);

/* compute_causal_shift_comprehensive (XAI.py:1600-1700) for J modified images at once, from logits the caller obtained with
 * ONE sisic_resnet_forward over originals and modified images: logits_orig dev [F,n], logits_mod dev [J,n], job_frame HOST
 * int [J] (the original of job j).  Softmax in fp32 with the maximum subtracted; score(c) = log(p_c + 1e-8).
 * rows: dev [J, 6*n + 7] fp32.  Row j holds, for every class c, the six floats at 6*c:
 *     orig_score, mod_score, cfi = orig_score - mod_score, delta = |cfi| / (|orig_score| + 1e-8), p_orig, p_mod
 * and then, at 6*n:
 *     argmax p_orig, argmax p_mod (class ids as floats, the first maximum), max p_orig, max p_mod,
 *     KL = sum_c p_orig (log p_orig - log(p_mod + 1e-8))            (a term with p_orig = 0 is 0, as F.kl_div defines it),
 *     JS = 0.5 * sum_c [ p_orig (log p_orig - l_c) + p_mod (log p_mod - l_c) ],  l_c = log((p_orig + p_mod)/2 + 1e-8),
 *     TV = 0.5 * sum_c |p_orig - p_mod|.
 * A frame index out of range returns SISIC_EINVAL.                                                                   */
int sisic_cfi_metrics(sisic_ctx*, const float* logits_orig, int F, const float* logits_mod, int J, int n_classes,
                      const int* job_frame, float* rows, void* stream);

/* ---- bootstrap and permutation resamples of the statistics stage (xai/XAI.py:1845-1904) ------------------------------------
 * The difference of means of n_bootstrap bootstrap resamples and n_permutations random relabellings of two samples, one GPU
 * thread per resample.  top / bottom: HOST doubles [n_top] / [n_bottom], read before the call returns; boot_out: DEVICE double
 * [n_bootstrap], perm_out: DEVICE double [n_permutations]; a count of 0 goes with a NULL pointer (that output is not touched).
 * 1 <= n_top, n_bottom and n_top + n_bottom <= 4096, anything else is SISIC_EINVAL.  Synchronises the stream.
 * N = n_top + n_bottom, comb = top followed by bottom.  Resample r reads the words w[0..N-1] of the device-noise block stream:
 * word j is word j & 3 of philox4x32_10(counter (j >> 2, r, tag, 0), key seed) = sisic_noise_bits(n_per_image = N, step = r, tag).
 *   bootstrap (tag 3):    s1 = sum_{j < n_top} top[(w[j] * n_top) >> 32],  s2 = sum_{j < n_bottom} bottom[(w[n_top + j] * n_bottom) >> 32]
 *   permutation (tag 4):  selection sampling (Knuth, Algorithm S), a uniform n_top-subset without a stored permutation:
 *                         need = n_top; for i = 0 .. N-1: if ((w[i] * (N - i)) >> 32 < need) { s1 += comb[i]; need -= 1 } else s2 += comb[i]
 * (64-bit products; the sums sequential in index order, in double) and the result is s1 / n_top - s2 / n_bottom.  The mean
 * difference depends only on which subset is chosen, so the permutation draw has the distribution of the reference's
 * shuffle-and-split.  A function of (values, seed, r) alone: bit-reproducible.                                              */
int sisic_resample_diffs(sisic_ctx*, const double* top, int n_top, const double* bottom, int n_bottom, uint64_t seed,
                         int n_bootstrap, int n_permutations, double* boot_out, double* perm_out, void* stream);

/* ---- training loader: the reference's augmentation chain on a device-resident dataset (diffusion/train_diffusion.py:72-114)
 * dataset: dev uint8 [N,H,W,3] (HWC, as PIL lays an RGB image out), H and W positive multiples of 8, not necessarily equal.
 * params_dev: dev array of B records, one per output image.  gray_mean_scratch: dev int32 [B], written by the first launch.
 * out: dev float32 [B,3,H,W] in [-1,1] (the output has the dataset's image size, as in the reference).
 * Two launches on `stream`, no host synchronisation: the rounded mean grey value of each image as it stands in front of its
 * contrast operation (integer sums: no dependence on reduction order; defined but unused for a record without contrast),
 * then one thread per output pixel.  For given parameters every stage is PIL's arithmetic, so the uint8 image equals what
 * torchvision's PIL backend returns bit for bit, in chain order:
 *   1. crop(box) + resize((W,H), BILINEAR): per axis, 22-bit integer coefficients of at most three taps (an axis whose box
 *      length equals the output length is copied), the horizontal pass rounded to uint8 before the vertical pass;
 *   2. horizontal / vertical flip: index reversal;
 *   3. order[0..2]: 0 brightness, 1 contrast, 2 saturation, -1 skips the slot.  Each is Image.blend(degenerate, image, f):
 *      t = (float)d + f * (float)(i - d) in float32 without fusing, 0 if t <= 0, 255 if t >= 255, else truncated;
 *      d = 0, the rounded mean grey, the pixel's grey value; grey = (R*19595 + G*38470 + B*7471 + 0x8000) >> 16;
 *   4. rotation (nearest, fill 0) when `rotate`: source pixel (xx >> 16, yy >> 16), xx = a2 + y*a1 + x*a0,
 *      yy = a5 + y*a4 + x*a3 in int32, rot = {a0 .. a5} PIL's 16.16 fixed-point inverse affine map; outside the image: 0;
 *   5. ToTensor + Normalize(0.5, 0.5): ((float)v / 255 - 0.5) / 0.5 in float32.
 * An image's output depends on its record alone, never on the batch it is in.
 * SISIC_EINVAL: a null pointer, N or B < 1, B > 65535, H or W not a positive multiple of 8.  The records live in device
 * memory and are not read back: their owner validates them before upload (synt_isic_amd.ops.augment does: src out of
 * range, a box outside the image or larger than the output -- down-scaling needs PIL's widened support and is refused).
 * The kernels clamp src and the box into range all the same, so that no record makes them read out of bounds.      */
typedef struct sisic_augment_params {      /* 96 bytes, no padding */
    int32_t src;                           /* index into the dataset, 0 .. N-1 */
    int32_t crop_x, crop_y, crop_w, crop_h;/* box in source pixels; 0 < crop_w <= W, 0 < crop_h <= H */
    int32_t hflip, vflip;
    int32_t order[3];                      /* permutation of 0 brightness, 1 contrast, 2 saturation; -1 = skip that slot */
    float   factor[3];                     /* brightness, contrast, saturation factors (indexed by operation, not by slot) */
    int32_t rotate;                        /* 0: none */
    int32_t rot[6];                        /* a0 a1 a2 a3 a4 a5 */
    int32_t reserved[4];                   /* 0 */
} sisic_augment_params;
int sisic_augment(sisic_ctx*, const uint8_t* dataset, int N, int H, int W, const sisic_augment_params* params_dev, int B,
                  int32_t* gray_mean_scratch, float* out, void* stream);
/* The same chain up to and including the rotation: out_hwc dev uint8 [B,H,W,3], the image PIL returns (tests, debugging). */
int sisic_augment_u8(sisic_ctx*, const uint8_t* dataset, int N, int H, int W, const sisic_augment_params* params_dev, int B,
                     int32_t* gray_mean_scratch, uint8_t* out_hwc, void* stream);

/* ---- evaluation of generated sets (synt_isic_amd/evaluate.py) ---------------------------------------------------------------
 * The pairwise arithmetic of the Frechet and kernel distances, improved precision / recall and the nearest-neighbour audit.
 * Every entry takes one argument struct that carries the stream as a field, launches on that stream without waiting for it,
 * allocates nothing, and writes only the outputs named below.  Matrices are row-major fp32 with a leading dimension in
 * floats (ld >= the row length).  Sums in double run in a fixed order without atomics: two calls give equal bits.       */

/* out[B,512] = the classifier's forward up to and including AdaptiveAvgPool2d(1): what sisic_resnet_forward feeds its Linear.
 * x, preprocess and the workspace rules are sisic_resnet_forward's; row b does not depend on the batch.                  */
typedef struct sisic_resnet_features_args {
    const float* x;                        /* dev [B,3,H,W] */
    float*       out;                      /* dev [B,512] */
    void*        stream;
    int          B, H, W, preprocess;
} sisic_resnet_features_args;              /* 40 bytes, no padding */
int sisic_resnet_features(sisic_resnet*, sisic_resnet_features_args* args);

/* mean_out[c] = (1/n) sum_r x[r,c] in double: rows r = g, g + 16, ... summed in order for g = 0 .. 15, the 16 partial sums
 * added in order of g.                                                                                                  */
typedef struct sisic_col_means_args {
    const float* x;                        /* dev [n,d], leading dimension ld */
    double*      mean_out;                 /* dev double [d] */
    void*        stream;
    int64_t      ld;
    int          n, d;
} sisic_col_means_args;                    /* 40 bytes, no padding */
int sisic_col_means(sisic_ctx*, sisic_col_means_args* args);

/* out[n,m] = f(A' B'^T), A' = A - shift_a and B' = B - shift_b (row vectors of length d, each optional), s = a'_i . b'_j formed
 * on the f32 matrix pipe: exact fp32 products, fp32 accumulation in a fixed order.  The shifts are subtracted
 * while the operands are staged; no centred copy exists.  b NULL: B = A (ldb and shift_b are still B's own).
 *   SISIC_GRAM_DOT     f = s
 *   SISIC_GRAM_SQDIST  f = max(0, |a'_i|^2 + |b'_j|^2 - 2 s), the norms of the shifted rows summed in fp32 by the same launch
 *   SISIC_GRAM_POLY3   f = (s / d + 1)^3, the kernel of the kernel inception distance
 * contract_rows = 1 contracts over the row index instead: out[d,d] = A'^T A' from the same [n,d] layout (the covariance
 * numerator when shift_a is the mean); b and shift_b must be NULL, m is not read, the mode must be SISIC_GRAM_DOT.
 * Any n, m, d >= 1: edges are handled in the kernel.  SISIC_EINVAL: a null a or out, a size below 1, a leading dimension
 * below its row length, an unknown mode, contract_rows with b, shift_b or another mode.                                  */
#define SISIC_GRAM_DOT 0
#define SISIC_GRAM_SQDIST 1
#define SISIC_GRAM_POLY3 2
typedef struct sisic_gram_args {
    const float* a;                        /* dev [n,d], leading dimension lda */
    const float* b;                        /* dev [m,d], leading dimension ldb; NULL: a */
    const float* shift_a;                  /* dev [d] or NULL */
    const float* shift_b;                  /* dev [d] or NULL */
    float*       out;                      /* dev [n,m] ([d,d] with contract_rows), leading dimension ldo */
    void*        stream;
    int64_t      lda, ldb, ldo;
    int          n, m, d, mode, contract_rows, reserved;
} sisic_gram_args;                         /* 96 bytes, no padding */
int sisic_gram(sisic_ctx*, const sisic_gram_args* args);

/* The k smallest of dist[i,j] - col_offset[j] (one fp32 subtraction; col_offset optional) of every row i, ascending, ties to
 * the lower column; skip_diagonal = 1 leaves j == i out.  Exact and deterministic; the values must be finite.
 * SISIC_EINVAL unless 1 <= k <= 8 and k <= m - skip_diagonal (the message names k and m).                                */
typedef struct sisic_rows_topk_args {
    const float* dist;                     /* dev [n,m], leading dimension ld */
    const float* col_offset;               /* dev [m] or NULL */
    float*       val_out;                  /* dev [n,k] */
    int32_t*     idx_out;                  /* dev int32 [n,k] */
    void*        stream;
    int64_t      ld;
    int          n, m, k, skip_diagonal;
} sisic_rows_topk_args;                    /* 64 bytes, no padding */
int sisic_rows_topk(sisic_ctx*, sisic_rows_topk_args* args);

/* out[i,j] = sum_c (a[i,c] - b[idx[i,j],c])^2: both converted to double before the subtraction, summed in double in a fixed
 * order (coordinates t, t + 256, ... per lane, then a binary tree), stored as fp32.  An index outside [0, nb) gives NaN.  */
typedef struct sisic_pair_sqdist_args {
    const float*   a;                      /* dev [n,d], leading dimension lda */
    const float*   b;                      /* dev [nb,d], leading dimension ldb */
    const int32_t* idx;                    /* dev int32 [n,k] */
    float*         out;                    /* dev [n,k] */
    void*          stream;
    int64_t        lda, ldb;
    int            n, nb, d, k;
} sisic_pair_sqdist_args;                  /* 72 bytes, no padding */
int sisic_pair_sqdist(sisic_ctx*, sisic_pair_sqdist_args* args);

/* out[0] = sum of x[n,m] in double (exclude_diagonal = 1: without the entries i == j, on any shape): lane t of one workgroup
 * sums the columns t, t + 1024, ... of every row in row order, then a binary tree.                                        */
typedef struct sisic_matrix_sum_args {
    const float* x;                        /* dev [n,m], leading dimension ld */
    double*      out;                      /* dev double [1] */
    void*        stream;
    int64_t      ld;
    int          n, m, exclude_diagonal, reserved;
} sisic_matrix_sum_args;                   /* 48 bytes, no padding */
int sisic_matrix_sum(sisic_ctx*, sisic_matrix_sum_args* args);

/* ---- instrumentation (bench.py roofline leg) -------------------------------------- */
/* When enabled, every conv launch is bracketed by HIP events on its own stream and
 * accumulated per class; reading synchronises the stream.                           */
int sisic_profile_enable(sisic_ctx*, int on);
/* kind: 0 = conv3x3, 1 = conv1x1, 2 = groupnorm stats, 3 = attention, 4 = ddpm step,
 *       5 = other, 6 = the f32-MFMA Winograd kernels alone (tile_cfg 66 / 68-73 / 78 / 79), 7 = the bf16x3 Winograd kernel
 *       alone (tile_cfg 74, the dominant kernel; 6 and 7 are subsets of kind 0).  Returns accumulated milliseconds, launches,
 *       algorithmic bytes, algorithmic flops (2*MAC of the direct form) and the fp32 multiply-adds x 2 of the algorithm that
 *       ran (16/36 of the direct form for Winograd launches; kind 7 issues six bf16 products for each of them).          */
int sisic_profile_read(sisic_ctx*, int kind, double* ms, int64_t* launches, double* bytes, double* flops,
                       double* flops_executed);
int sisic_profile_reset(sisic_ctx*);

#ifdef __cplusplus
}
#endif
#endif /* SISIC_H */
