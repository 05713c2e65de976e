// train.h -- launchers of train_kernels.hip (used by train.cpp and by the single-operator C entry points).
#pragma once

#include <vector>

#include "common.h"

namespace sisic {

// dW[co][ci][ky][kx] = sum_{b,oy,ox} dy[b,co,oy,ox] * act(cat(in0,in1))[b,ci,oy*stride+ky-pad, ox*stride+kx-pad]
// with the forward convolution's prologue act (GroupNorm apply + optional SiLU, zero padding after it) and index maps.
struct WgradArgs {
    const float* in0 = nullptr; const float* in1 = nullptr;
    int c0 = 0, c1 = 0, B = 0, Hin = 0, Win = 0;
    int ups = 0;                 // nearest 2x before the convolution
    int ksize = 3, stride = 1;
    const float* gn_scale = nullptr; const float* gn_shift = nullptr; int gn_silu = 0;
    const float* dy = nullptr;   // [B, Cout, Hout, Wout]
    int Cout = 0;
    float* dw = nullptr;         // [Cout, c0+c1, k, k] (OIHW, the state-dict layout)
    float* dw1 = nullptr;        // 1x1 only, with dw2: the gradient leaves as three [Cout/3, Cin] tensors (fused q/k/v projection)
    float* dw2 = nullptr;
};
size_t conv_wgrad_scratch_floats(const WgradArgs& a);
int launch_conv_wgrad(sisic_ctx*, const WgradArgs& a, float* part, size_t part_floats, hipStream_t s);
int launch_transpose_flip(sisic_ctx*, const float* w, int Cout, int Cin, int KK, float* wt, hipStream_t s);
// out[i] = sum over k of part[k][i] in launch_conv_wgrad's fixed order (its reduction kernels, for slabs of another kernel)
int launch_wgrad_reduce(sisic_ctx*, const float* part, int ksplit, size_t n, float* out, hipStream_t s);

// classifier_train.hip: the classifier's training step with BatchNorm frozen (resnet.cpp)
// dW [64,3,7,7] of the 7x7 stride-2 padding-3 stem from its input x [B,3,H,W] (H, W even, >= 8) and dy [B,64,H/2,W/2]
size_t stem_wgrad_scratch_floats();
int launch_stem_wgrad(sisic_ctx*, const float* x, const float* dy, float* dw, int B, int H, int W, float* part, size_t part_floats,
                      hipStream_t s);
int launch_gather_even(sisic_ctx*, const float* in, float* out, int planes, int H, int W, hipStream_t s);
// labels: device int [B], each in [0, n) (the caller checks); w: device [n] or NULL; loss: device float; dlogits [B, n]
int launch_ce_head(sisic_ctx*, const float* logits, const int* labels, const float* w, int B, int n, float* loss, float* dlogits,
                   hipStream_t s);
int launch_fc_head_bwd(sisic_ctx*, const float* dlogits, const float* fc_w, const float* act, float* g, float* dfc_w, float* dfc_b,
                       int B, int C, int HW, int n, hipStream_t s);
int launch_unfold_grad(sisic_ctx*, float* g, const double* sc, int cout, int cin, int k, hipStream_t s);
int launch_refold(sisic_ctx*, const float* w, const double* sc, float* raw, float* raw_t, int cout, int cin, int k, hipStream_t s);

// batchnorm.hip: BatchNorm2d with batch statistics over y [B, C, HW].  B * HW = 1 is SISIC_EINVAL before any launch.
// moments: mean, invstd = 1/sqrt(var + eps) and (var may be NULL) the biased variance, [C] each; running_mean / running_var
// (both or neither) receive nn.BatchNorm2d's update with the unbiased variance, momentum in (0, 1].  The slice partials live in
// the context's per-stream scratch (a larger shape grows it and waits for the stream once).
int launch_bn_moments(sisic_ctx*, const float* y, int B, int C, int HW, float eps, float* mean, float* invstd, float* var,
                      float* running_mean, float* running_var, double momentum, hipStream_t s);
// out = [relu](gamma (y - mean) invstd + beta [+ residual])
int launch_bn_apply(sisic_ctx*, const float* y, const float* gamma, const float* beta, const float* mean, const float* invstd,
                    const float* residual, bool relu, float* out, int B, int C, int HW, hipStream_t s);
// g' = g, or g [act > 0] (act: the kept activation behind the BatchNorm's ReLU, or NULL); dbeta = sum g', dgamma = sum g' xhat,
// dy = gamma invstd (g' - dbeta/n - xhat dgamma/n); dy is a buffer of its own (NULL: the two sums alone)
int launch_bn_bwd(sisic_ctx*, const float* g, const float* y, const float* act, const float* mean, const float* invstd,
                  const float* gamma, float* dy, float* dgamma, float* dbeta, int B, int C, int HW, hipStream_t s);
// sc = gamma / sqrt(rv + eps) and bias = (float)(beta - rm sc), in double: the fold of sisic_resnet_load
int launch_bn_fold(sisic_ctx*, const float* gamma, const float* beta, const float* rm, const float* rv, float eps, double* sc,
                   float* bias, int C, hipStream_t s);
int bn_slices(int B, int C, int HW);      // slices a channel's moments are split into (a function of the shape alone)

// repack.hip: one re-layout of one tensor inside a batched launch (pack_batch_kernel)
struct PackJob {
    enum Kind : int { COPY = 0, TRANSPOSE2D, FLIP, CONV_PACK, WINO_FIRST, WINO_WIDE, WINO_BF3, CONV_S2_BF3 };
    int kind;
    int a, b, c, d, e;          // shape arguments of the kind's per-element function (see the constructors in repack.hip)
    const float* src;
    float* dst;
    size_t total;               // elements of the job's index space
    int first_block;            // first workgroup of the launch that works on this job
};
int pack_job_blocks(const PackJob& j);
int launch_pack_batch(sisic_ctx*, const PackJob* dev_jobs, int njobs, int nblocks, hipStream_t s);
// a job table onto the device: assigns every job's first_block, frees the table *dev held, allocates at least one slot, poisons
// the fresh block and copies.  Blocking; a table a running launch still reads must not be replaced (the caller waits first).
int upload_pack_table(std::vector<PackJob>& jobs, void** dev, int* njobs, int* nblocks);
PackJob pack_job_copy(const float* src, float* dst, size_t n);
PackJob pack_job_transpose2d(const float* in, int rows, int cols, float* out, int out_ld, int out_col0);
PackJob pack_job_flip(const float* w, int Cout, int Cin, int KK, float* wt);
PackJob pack_job_conv(const float* w, int Cout, int Cin, int k, float* packed);
PackJob pack_job_wino_first(const float* w, int Cout, int Cin, float* packed);
PackJob pack_job_wino_wide(int Cout, int Cin, float* packed);
PackJob pack_job_wino_bf3(int Cout, int Cin, float* packed);
PackJob pack_job_conv_s2(const float* w, int Cout, int Cin, float* out);
int launch_plane_sums(sisic_ctx*, const float* x, int planes, int HW, float* out, hipStream_t s);
// bias gradient of a convolution in one launch: db[c] = sum over (b, pixels) of dy; split > 0: channels [0, split) -> db0,
// [split, 2 split) -> db1, the rest -> db2; tproj (optional): the per-(image, channel) sums into column c of [B, tproj_ld]
int launch_bias_grad(sisic_ctx*, const float* dy, int B, int C, int HW, float* db0, float* db1, float* db2, int split, float* tproj,
                     int tproj_ld, hipStream_t s);
int launch_col_sums(sisic_ctx*, const float* m, int rows, int cols, int ld, float* out, int accumulate, hipStream_t s);
int launch_copy_cols(sisic_ctx*, const float* src, int rows, int cols, float* dst, int ld_dst, hipStream_t s);
// sums: scratch [2][B][c0+c1]
int launch_gn_bwd(sisic_ctx*, const float* da, const float* in0, int c0, const float* in1, int c1, int B, int HW, int groups,
                  const float* scale, const float* shift, const float* mean_rstd, const float* gamma, int silu,
                  float* sums, float* g0, float* g1, float* dgamma, float* dbeta, hipStream_t s);
// ResnetBlock2D dropout (the mask contract of include/sisic.h; tag = 256 + the block's index, call = the forward's counter value):
// out = dropout(silu(h * scale[b,c] + shift[b,c])) over [B, C, HW], and the same mask times inv_keep applied to a gradient in
// place.  C*HW % 4 == 0 and 16-byte aligned tensors, or SISIC_EINVAL.
int launch_gn_silu_dropout(sisic_ctx*, const float* h, const float* scale, const float* shift, float* out, int B, int C, int HW,
                           uint64_t seed, uint32_t call, uint32_t tag, float p, float inv_keep, hipStream_t s);
int launch_dropout_bwd(sisic_ctx*, float* d, int B, int C, int HW, uint64_t seed, uint32_t call, uint32_t tag, float p, float inv_keep,
                       hipStream_t s);
int launch_accum_split(sisic_ctx*, const float* da, int B, int C, int HW, float* g0, int c0, float* g1, int c1, hipStream_t s);
int launch_accum_pool2(sisic_ctx*, const float* da, int planes, int H, int W, float* g, hipStream_t s);
int launch_add_inplace(sisic_ctx*, float* dst, const float* src, size_t n, hipStream_t s);
// head_dim 8: attention_bwd keeps a head's whole key/value rows in LDS, 32 + 3 floats per token within 160 KB: the most tokens
// it accepts.  launch_attention_bwd refuses more, and sisic_unet_train_forward refuses a resolution whose attention levels have more.
constexpr int ATTN_BWD_LDS_BYTES = 160 * 1024;
constexpr int ATTN_BWD_MAX_TOKENS = 1170;
static_assert(ATTN_BWD_MAX_TOKENS * 35 * 4 <= ATTN_BWD_LDS_BYTES && (ATTN_BWD_MAX_TOKENS + 1) * 35 * 4 > ATTN_BWD_LDS_BYTES,
              "ATTN_BWD_MAX_TOKENS is the most tokens whose key/value rows fit the LDS");
// head_dim 32 and 64: the backward pass is tiled over keys and queries (attention_wide.hip) and holds 64 tokens of a head in
// LDS at a time, so the LDS sets no limit.  What remains is the kernels' 32-bit token arithmetic and the row-statistics scratch
// (3 floats per sample, head and token): 65536 tokens, a 256 x 256 attention plane, is the most launch_attention_bwd accepts at
// these widths.  (The pass is quadratic in the tokens: at the bound one head is 2 * 10^12 multiply-adds.)
constexpr int ATTN_BWD_TILED_MAX_TOKENS = 65536;
// the bound of a model's head dimension (check_trainable_resolution)
inline int attn_bwd_max_tokens(int head_dim) { return head_dim == 8 ? ATTN_BWD_MAX_TOKENS : ATTN_BWD_TILED_MAX_TOKENS; }
int launch_attention_bwd(sisic_ctx*, const float* qkv, const float* o, const float* dO, float* dqkv, int B, int C, int N,
                         int head_dim, hipStream_t s);
int launch_linear_wgrad(sisic_ctx*, const float* dy, int ld, const float* x, int B, int R, int K, float* dW, hipStream_t s);
int launch_linear_dgrad(sisic_ctx*, const float* dy, int ld, const float* W, int B, int R, int K, float* dx, hipStream_t s,
                        int w_is_transposed);
// class embedding gradient: dE[k][j] = sum over the samples b with labels[b] == k, in ascending b, of dt[b][j] (no atomics: the
// same bits every time); every one of the N rows is written, a label absent from the batch leaves its row zero
int launch_class_embed_grad(sisic_ctx*, const float* dt, const int* labels, int B, int N, int hidden, float* dE, hipStream_t s);
int launch_silu_fwd(sisic_ctx*, const float* pre, size_t n, float* out, hipStream_t s);
int launch_silu_bwd(sisic_ctx*, const float* dy, const float* pre, size_t n, float* out, hipStream_t s);
// loss_dev[0] = mean(w_b (pred - t)^2) and dpred = grad_scale * 2 w_b (pred - t) / n in one launch plus a one-block finish, in a
// fixed order.  t = target, or the v target sa[b]*noise - sb[b]*target formed in the register (noise, sa, sb: all or none;
// `target` is then x0); w: per-sample weights (device [B]) or NULL.  With neither, B only has to divide n.
int launch_mse_objective(sisic_ctx*, const float* pred, const float* target, const float* noise, const float* sa, const float* sb,
                         const float* w, int B, size_t n, float grad_scale, float* loss_dev, float* dpred, float* part, int nparts,
                         hipStream_t s);
// What grad_stats leaves on the device for adam_ema (and the host reads back in one 12-byte copy): the norm of the unscaled
// gradient, clip_grad_norm_'s coefficient, GradScaler's found_inf.
struct GradStats {
    float total_norm;
    float clip_coef;
    int found_inf;
};
static_assert(sizeof(GradStats) == 12, "the C ABI documents the record as 3 x 4 bytes");
constexpr int GRAD_STATS_MAX_BLOCKS = 2048;         // block partials the scratch holds
size_t grad_stats_scratch_bytes();                  // GRAD_STATS_MAX_BLOCKS doubles, then as many ints
int launch_grad_stats(sisic_ctx*, const float* g, size_t n, float inv_scale, float max_norm, GradStats* stats_dev, void* scratch,
                      hipStream_t s);
// ema == nullptr: Adam alone; stats_dev == nullptr: clip coefficient 1
int launch_adam_ema(sisic_ctx*, float* p, const float* g, float* m, float* v, float* ema, size_t n, double lr, double b1, double b2,
                    double eps, int64_t step, float inv_scale, const GradStats* stats_dev, double ema_decay, hipStream_t s);
int launch_ema(sisic_ctx*, float* ema, const float* p, size_t n, double ema_decay, hipStream_t s);
// The one optimizer update of the library (the UNet's plain and extended steps and the classifier's): when want_stats,
// launch_grad_stats, one 12-byte read-back and one stream synchronisation; the skip decision on the host (skip_on_inf and a
// non-finite gradient); then launch_adam_ema -- reading the record when the statistics pass ran, coefficient 1 otherwise -- or,
// on a skipped step, launch_ema alone when there is an EMA.  *step advances only when the update runs.  Without want_stats
// nothing waits for the stream and norm / found_inf come back 0.  The caller re-derives its packed weights afterwards.
struct AdamStepArgs {
    float* p = nullptr; const float* g = nullptr; float* m = nullptr; float* v = nullptr;
    size_t n = 0;
    float* ema = nullptr;               // EMA arena of this step, or nullptr
    double ema_decay = 0.0;
    double lr = 0.0, beta1 = 0.0, beta2 = 0.0, eps = 0.0;
    float inv_scale = 1.0f, max_norm = 0.0f;
    int64_t* step = nullptr;
    GradStats* stats = nullptr;         // the record and grad_stats' scratch (needed with want_stats only)
    void* scratch = nullptr;
    bool want_stats = false, skip_on_inf = false;
};
struct AdamStepResult {
    float norm = 0.0f;
    int found_inf = 0;
    bool skipped = false;
};
int adam_step(sisic_ctx*, const AdamStepArgs& a, AdamStepResult* out, hipStream_t s);
int launch_swap_arenas(sisic_ctx*, float* a, float* b, size_t n, hipStream_t s);
int launch_add_noise(sisic_ctx*, const float* x0, const float* noise, const float* a_dev, const float* c_dev, float* out, int B,
                     size_t per, hipStream_t s);

}  // namespace sisic
