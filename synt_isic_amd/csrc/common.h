// Internal declarations shared by the libsisic_hip.so translation units.
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <map>
#include <mutex>
#include <vector>

#include "../../include/sisic.h"

namespace sisic {

void set_error(const char* fmt, ...);

#define SISIC_HIP(call)                                                                   \
    do {                                                                                  \
        hipError_t _e = (call);                                                           \
        if (_e != hipSuccess) {                                                           \
            ::sisic::set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(_e),     \
                               __FILE__, __LINE__);                                       \
            return SISIC_EHIP;                                                            \
        }                                                                                 \
    } while (0)

#define SISIC_REQUIRE(cond, ...)                 \
    do {                                         \
        if (!(cond)) {                           \
            ::sisic::set_error(__VA_ARGS__);     \
            return SISIC_EINVAL;                 \
        }                                        \
    } while (0)

#define SISIC_TRY(expr)             \
    do {                            \
        int _rc = (expr);           \
        if (_rc != SISIC_OK) return _rc; \
    } while (0)

// PK_WINO_MAIN / PK_WINO_BF3: the Winograd kernel families on their own -- the f32-MFMA forms (tile_cfg 66, 68-73, 78, 79) and
// the bf16x3 form (tile_cfg 74); their launches are credited to PK_CONV3 (the class) AND to their slot (same event pair)
enum ProfileKind { PK_CONV3 = 0, PK_CONV1 = 1, PK_GN = 2, PK_ATTN = 3, PK_DDPM = 4, PK_OTHER = 5, PK_WINO_MAIN = 6, PK_WINO_BF3 = 7, PK_COUNT = 8 };

struct ProfileSlot {
    double ms = 0, bytes = 0, flops = 0, flops_exec = 0;   // flops: algorithmic (2*MAC of the direct form); flops_exec: issued to the matrix pipe
    int64_t launches = 0;
};

struct PendingEvent {
    hipEvent_t start, stop;
    int kind;
    int kind2;      // second slot credited with the same launch, or -1
};

}  // namespace sisic

struct sisic_ctx {
    int device = 0;
    int num_cus = 0;
    int step_pred = 0;              // sisic_set_step_prediction_type: what the single-step entries' eps argument means
    // sisic_set_step_thresholding: the single-step entries clamp x0 dynamically (ratio 0: off); the entries that are not told
    // the image size take it from sisic_set_step_image_elems
    float step_thr_ratio = 0.0f, step_thr_max = 1.0f;
    int64_t step_npi = 0;
    bool profiling = false;
    sisic::ProfileSlot prof[sisic::PK_COUNT];
    std::vector<sisic::PendingEvent> pending;
    std::vector<hipEvent_t> event_pool;
    // partial outputs of K-split convolutions (conv_winograd.hip): one scratch buffer per stream, grown on demand, so
    // that models sampling concurrently on different streams of this context never share it
    struct SplitK { float* p = nullptr; size_t floats = 0; };
    std::map<hipStream_t, SplitK> splitk;
    std::mutex splitk_mutex;
    // row statistics (m_i, 1/l_i, D_i) that the tiled attention backward pass (attention_wide.hip) hands from its query-owned
    // kernel to its key-owned kernel: one buffer per stream, grown on demand, for the same reason
    std::map<hipStream_t, SplitK> attn_rows;
    std::mutex attn_rows_mutex;
    // slice partials of the training-mode BatchNorm launches (batchnorm.hip), handed from the slice kernel to the merge
    // kernel: one buffer per stream, grown on demand, for the same reason
    std::map<hipStream_t, SplitK> bn_part;
    std::mutex bn_part_mutex;
    // every image's s of a thresholded single step (elementwise.hip), handed from the quantile kernel to the step kernel: one
    // buffer per stream, grown on demand, for the same reason
    std::map<hipStream_t, SplitK> thr_s;
    std::mutex thr_s_mutex;
    // item tables of the bf16x3 Winograd kernel (conv_winograd_bf3.inc): one per launch geometry, filled on the device the
    // first time the geometry is met, never moved or freed before the context (captured graphs hold their addresses)
    // (fill_done: recorded behind the fill; until it has passed, only launches on the filling stream use the table)
    struct Bf3Items { int key[9]; unsigned* tab = nullptr; hipStream_t fill_stream = nullptr; hipEvent_t fill_done = nullptr; };
    std::vector<Bf3Items> bf3_items;
    std::mutex bf3_items_mutex;
    std::atomic<uint64_t> scratch_generation{0};    // bumped whenever a scratch buffer is re-allocated: captured graphs that
                                                    // may hold its old address are rebuilt
};

namespace sisic {

// RAII-less helper: brackets one launch with events when profiling is on.
struct ProfileScope {
    sisic_ctx* ctx;
    hipStream_t stream;
    PendingEvent ev{};
    bool active = false;
    ProfileScope(sisic_ctx* c, hipStream_t s, int kind, double bytes, double flops, double flops_exec = -1.0, int kind2 = -1);
    ~ProfileScope();
};

int profile_collect(sisic_ctx* ctx);

// Opt a kernel in to more than 64 KB of dynamic LDS.  The attribute belongs to the (kernel, device) pair, and several
// devices and threads may use one process (sisic_create(device_id)), so every template instance keeps one bit per device
// in an atomic mask; setting the attribute twice from two racing threads is harmless (same value).
inline int ensure_dynamic_lds(sisic_ctx* ctx, const void* kern, int bytes, std::atomic<uint64_t>& done) {
    const uint64_t bit = uint64_t(1) << (ctx->device & 63);
    if (done.load(std::memory_order_acquire) & bit) return SISIC_OK;
    SISIC_HIP(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    done.fetch_or(bit, std::memory_order_release);
    return SISIC_OK;
}

// A process-wide switch in the environment: on unless set to 0.  Callers keep the answer (static const): one read per process.
inline bool env_on(const char* name) { const char* e = std::getenv(name); return !e || std::atoi(e) != 0; }

inline int cdiv(int a, int b) { return (a + b - 1) / b; }
// Latency mode (tile_cfg 78 / 79): ways the input channels of a Winograd convolution are split over workgroups so that ONE
// image already offers ~256 workgroups.  A function of the layer shape only -- never of the batch -- so that an image's
// bits do not depend on the batch it is computed in.
inline int wino_latency_ksplit(int Cout, int Cin, int Hout, int Wout) {
    const int co_t = Cout > 64 ? 128 : 64;
    const int per_image = cdiv(Hout, 8) * cdiv(Wout, 16) * cdiv(Cout, co_t);
    const int nchunks = cdiv(Cin, 8);
    int k = 1;
    while (per_image * k < 256 && k < 8 && nchunks % (2 * k) == 0) k *= 2;
    return k;
}
// segments a plane is cut into by the K-split plane reduction (one workgroup and one statistics slot each): 1024 pixels
inline int wino_latency_segments(int Hout, int Wout) { return cdiv(Hout * Wout, 1024); }
inline int64_t cdiv64(int64_t a, int64_t b) { return (a + b - 1) / b; }
inline int round_up(int a, int b) { return cdiv(a, b) * b; }

// conv weight packing geometry (must match conv_mfma.hip)
constexpr int CONV_CO_TILE = 64;
inline int conv_ci_chunk(int ksize) { return ksize == 1 ? 32 : (ksize == 3 ? 16 : 4); }   // channel padding of the packed weights (1x1: tiles use 16 or 32)
inline int conv_cin_pad(int cin, int ksize) { return round_up(cin, conv_ci_chunk(ksize)); }
inline int conv_cout_pad(int cout) { return round_up(cout, CONV_CO_TILE); }
// floats of a packed filter: 1x1 filters carry three layouts (pack_device.h: generic, conv_pointwise.hip's, the bf16x3 split)
inline int64_t conv_packed_floats(int cout, int cin, int ksize) {
    const int64_t first = (int64_t)conv_cin_pad(cin, ksize) * ksize * ksize * conv_cout_pad(cout);
    return ksize == 1 ? 3 * first + first / 2 : first;
}

// launchers implemented in the .hip files
// launch_conv2d: plans the convolution once (conv_plan.h: kernel, tile configuration, GroupNorm partial slots, finalisation, rider)
// and hands (args, plan) to the chosen kernel's launcher below; the launchers act on the plan and do not test the arguments again.
// rider / carried (optional): a GroupNorm finalisation that is independent of this convolution (gn_finalize.h) runs as extra
// workgroups of its launch where the planned kernel offers that -- the bf16x3 1x1 kernels without a GroupNorm prologue.
// *carried says whether THIS launch ran the jobs; false: nothing of the job was touched and the caller launches it itself.
struct GnFinJob;
struct ConvPlan;
int launch_conv2d(sisic_ctx*, const sisic_conv_args& a, hipStream_t s, const GnFinJob* rider = nullptr, bool* carried = nullptr);
int launch_conv_smallcout(sisic_ctx*, const sisic_conv_args& a, const ConvPlan& plan, hipStream_t s);
int launch_score_head_bwd(sisic_ctx*, const float* logits, const float* fc_w, const float* act, float* g, int B, int C,
                          int HW, int n_classes, int target, hipStream_t s);
// the same head with image b's target read from targets_dev (device int [B], each in [0, n_classes): the caller checks)
int launch_score_head_bwd_targets(sisic_ctx*, const float* logits, const float* fc_w, const float* act, float* g, int B, int C,
                                  int HW, int n_classes, const int* targets_dev, hipStream_t s);
int launch_relu_bwd(sisic_ctx*, const float* dy, const float* y, float* out, int64_t n, hipStream_t s);
int launch_scatter_add_even(sisic_ctx*, float* dst, const float* src, int planes, int H, int W, hipStream_t s);
int launch_maxpool_bwd(sisic_ctx*, const float* dm, const float* xin, float* dx, int planes, int H, int W, hipStream_t s);
int launch_stem_bwd(sisic_ctx*, const float* g, const float* w_oihw, float* dp, int B, int CO, int OH, int OW, int H, int W,
                    hipStream_t s);
int launch_preprocess_bwd(sisic_ctx*, const float* dp, const float* x, float* dx, int B, int H, int W, int OH, int OW,
                          hipStream_t s);
int launch_add_relu(sisic_ctx*, const float* y, const float* identity, float* out, int64_t n, hipStream_t s);
int launch_gradcam(sisic_ctx*, const float* y, const float* outp, const float* fc_w, const float* bias, float* cam, int B, int C,
                   int h, int w, int S, int target, hipStream_t s);
// the plan's answers for sisic_conv_stats_slots / sisic_conv_finalizes (conv_plan.cpp); 0 / false where planning fails
int conv_stats_slots(const sisic_conv_args& a);
bool conv_finalizes(const sisic_conv_args& a);       // the launch leaves the following GroupNorm's (scale, shift) itself (sisic.h)
// conv_pointwise.hip: the lean 1x1 kernel (tile_cfg 20) and the shapes it takes
bool conv_pointwise_applicable(const sisic_conv_args& a);
int launch_conv_pointwise(sisic_ctx*, const sisic_conv_args& a, const ConvPlan& plan, hipStream_t s);
// conv_pointwise_bf3.hip: the same GEMM with fp32-equivalent products on the bf16 matrix pipe (tile_cfg 28); rider: jobs to run, or NULL
bool conv_pointwise_bf3_applicable(const sisic_conv_args& a);
int launch_conv_pointwise_bf3(sisic_ctx*, const sisic_conv_args& a, const ConvPlan& plan, hipStream_t s, const GnFinJob* rider);
// conv_s2_bf3.hip: 3x3 stride-2 convolutions with fp32-equivalent products on the bf16 matrix pipe (tile_cfg 36); the split
// filter (conv_s2_pack_bf3_elem, pack_device.h) travels in sisic_conv_args.w_winograd
bool conv_s2_bf3_applicable(const sisic_conv_args& a);
int conv_s2_bf3_stats_slots(const sisic_conv_args& a);
int launch_conv_s2_bf3(sisic_ctx*, const sisic_conv_args& a, const ConvPlan& plan, hipStream_t s);
int64_t conv_s2_packed_floats(int Cout, int Cin);
int launch_conv_s2_pack(sisic_ctx*, const float* w, int Cout, int Cin, float* out, hipStream_t s);
// mean_rstd (optional, training): [B, groups, 2] = (mean, rstd) of every (sample, group)
int launch_gn_finalize(sisic_ctx*, const float* st0, int c0, int slots0, const float* st1, int c1, int slots1, int B,
                       int HW, int groups, float eps, const float* gamma, const float* beta, float* scale, float* shift,
                       hipStream_t s, float* mean_rstd = nullptr);
// the same finalisation as a checked job (gn_finalize.h), and the stand-alone launch of one
int make_gn_fin_job(GnFinJob* q, const float* st0, int c0, int slots0, const float* st1, int c1, int slots1, int B, int groups,
                    float eps, const float* gamma, const float* beta, float* scale, float* shift, float* mean_rstd = nullptr);
int launch_gn_finalize_job(sisic_ctx*, const GnFinJob& q, hipStream_t s);
// conv_winograd.hip: F(2x2,3x3) for 3x3 stride-1 convolutions, every Winograd kernel of the plan (filters in a.w_winograd)
int launch_conv_winograd(sisic_ctx*, const sisic_conv_args& a, const ConvPlan& plan, hipStream_t s);
int launch_winograd_pack(sisic_ctx*, const float* w, int Cout, int Cin, float* packed, hipStream_t s);
int64_t winograd_packed_numel(int Cout, int Cin);
// floats of the first Winograd layout [Cin_pad][16][cout_pad]; the wide layout follows it in the same buffer
inline int64_t winograd_first_floats(int Cout, int Cin) { return (int64_t)round_up(Cin, 16) * 16 * conv_cout_pad(Cout); }
int launch_conv_pack(sisic_ctx*, const float* w, int Cout, int Cin, int k, float* packed, hipStream_t s);
int launch_gn_stats(sisic_ctx*, const float* in0, int c0, const float* in1, int c1, int B, int HW, int groups,
                    float eps, const float* gamma, const float* beta, float* scale, float* shift, hipStream_t s,
                    float* mean_rstd = nullptr);
int launch_attention(sisic_ctx*, const float* qkv, float* out, int B, int C, int N, int head_dim, hipStream_t s);
// head_dim 32 and 64 (attention_wide.hip); launch_attention and launch_attention_bwd dispatch to these
int launch_attention_wide(sisic_ctx*, const float* qkv, float* out, int B, int C, int N, int head_dim, hipStream_t s);
int launch_attention_bwd_wide(sisic_ctx*, const float* qkv, const float* dO, float* dqkv, int B, int C, int N, int head_dim,
                              hipStream_t s);
// The scheduler-step rules of the sampling loop (elementwise.hip; sisic.h SISIC_RULE_*): the row of a step is
// {sb, sa, c2, c3, sigma} with (c2, c3) = DDPM (c0, c1) or DDIM (c_prev, c_dir).  flags: STEP_FLAG_CLIPPED_OUTPUT (DDIM only),
// and under every rule the prediction type in its private bits (below).
enum StepRule { STEP_RULE_DDPM = SISIC_RULE_DDPM, STEP_RULE_DDIM = SISIC_RULE_DDIM, STEP_RULE_DPMPP = SISIC_RULE_DPMPP };
enum StepFlag { STEP_FLAG_CLIPPED_OUTPUT = SISIC_RULE_FLAG_CLIPPED_OUTPUT };
// What the model's output means (sisic.h SISIC_PRED_*) travels in private bits of `flags`, beside the rule's own: the launchers
// and the captured step's key (LoopKey::rule_flags) carry it without a parameter of their own.  A caller's rule_flags never has
// these bits (the public entry points refuse them and add the handle's or the context's type).
constexpr int STEP_FLAG_PRED_SHIFT = 8;
constexpr int STEP_FLAG_PRED_MASK = 3 << STEP_FLAG_PRED_SHIFT;
inline int step_pred(int flags) { return (flags & STEP_FLAG_PRED_MASK) >> STEP_FLAG_PRED_SHIFT; }
inline int step_pred_flags(int type) { return type << STEP_FLAG_PRED_SHIFT; }
// a known rule, flags it has, sa != 0, and sb != 0 where the rule divides by it
int check_step_row(int rule, int flags, float sb, float sa);
// graph-replayed sampling loop (elementwise.hip): per-step parameters selected on the device by a step index
size_t loop_state_bytes();     // {int step; int step_base; const float* noise_base}
int launch_loop_select_row(sisic_ctx*, const float* table, int R, const void* state, float* out, hipStream_t s);
int launch_loop_advance(sisic_ctx*, void* state, hipStream_t s);
// One step of any kind (elementwise.hip step_kernel), described by name.  What its eps is:
//   STEP_EPS_PLAIN       the model's output as it stands
//   STEP_EPS_GUIDED      classifier-free guidance: eps_u + w * (eps - eps_u), formed in the kernel; the new x goes to both halves of
//                        out [2n]
//   STEP_EPS_CLASSIFIER  classifier guidance: eps - (w * sb) * grad, formed in the kernel, grad the classifier's input gradient at x
//                        (epsilon prediction and device noise only)
enum StepEps { STEP_EPS_PLAIN, STEP_EPS_GUIDED, STEP_EPS_CLASSIFIER };
struct StepLaunch {
    int rule = STEP_RULE_DDPM;
    int flags = 0;
    StepEps source = STEP_EPS_PLAIN;
    bool device_noise = false;          // z is generated in the kernel from seeds_dev; else read from the buffer z (or none)
    bool edit = false;                  // the inpainting epilogue (device noise only)
    const float* eps = nullptr;         // [n]
    const float* eps_u = nullptr;       // STEP_EPS_GUIDED: the null-label half
    const float* grad = nullptr;        // STEP_EPS_CLASSIFIER
    const float* x = nullptr;
    float* out = nullptr;               // may be x
    float* hist = nullptr;              // DPM-Solver++: the previous step's x0 [n], written on every step, read when k1 != 0
    int64_t n = 0;
    float clip = 0.0f;
    // dynamic thresholding (thr_s set): the launcher first writes every image's s = clamp(quantile(|x0|, thr_ratio), 1, thr_max)
    // to thr_s [n / n_per_image] (launch_x0_threshold), then runs the step with clamp(x0, -s, s) / s in place of `clip`
    float* thr_s = nullptr;
    float thr_ratio = 0.0f, thr_max = 1.0f;
    const uint64_t* seeds_dev = nullptr;    // device uint64 [n / n_per_image]
    int64_t n_per_image = 0;                // device noise, an edit, thresholding
    const float* x0k = nullptr;         // edit: the known image [n] and the mask, whose row [B, 1, hw] is broadcast over the
    const float* mask = nullptr;        //       n_per_image / hw channels
    int64_t hw = 0;
    // the eager form: the rule's host row (SISIC_RULE_ROW_WIDTH floats), the host edit row {ck, sk, ja, jb}, this step's noise
    // row, its index in the run, and the guidance or classifier scale
    const float* row = nullptr;
    const float* erow = nullptr;
    const float* z = nullptr;
    uint32_t step = 0;
    float w = 1.0f;
    // the replayed form (state set): all of these are read on the device by the loop's step index instead.  coef_dev, zrow_dev
    // (buffer noise) and erows_dev are the loop's tables; entry 0 of w_tab is w (LoopCond, LoopClf)
    const void* state = nullptr;
    const float* coef_dev = nullptr;
    const int* zrow_dev = nullptr;
    const float* erows_dev = nullptr;
    const float* w_tab = nullptr;
};
int launch_step(sisic_ctx*, const StepLaunch& L, hipStream_t s);
// the quantile launch alone: what launch_step runs first when L.thr_s is set (ratio in [0, 1], max >= 1, images of at most 2^24)
int launch_x0_threshold(sisic_ctx*, const StepLaunch& L, hipStream_t s);
int check_thresholding(const char* what, float ratio, float max_value);
// the s buffer of the context's own thresholded steps on stream s (one per stream, grown on demand): [images] floats
int step_threshold_scratch(sisic_ctx*, hipStream_t s, int64_t images, float** out);
int launch_guide_eps(sisic_ctx*, const float* eps_c, const float* eps_u, float w, float* out, int64_t n, hipStream_t s);
// the loop's device table of a classifier-guided call (LoopClf): {scale, -, -, -, int target[B]}
constexpr size_t LOOP_CLF_HEAD = 4;
int launch_clf_guide_eps(sisic_ctx*, const float* eps, const float* g, float sb, float scale, float* out, int64_t n, hipStream_t s);
// resnet.cpp, for the classifier-guided sampling loop (unet.cpp): what the loop checks before its first launch, and the walk of
// sisic_resnet_input_gradient with image b's target read from targets_dev (device int [B]; NULL: `target` for every image).
// The walk checks nothing but the shape: its callers have.
sisic_ctx* resnet_ctx(const sisic_resnet* r);
bool resnet_loaded(const sisic_resnet* r);
int resnet_num_classes(const sisic_resnet* r);
// renewed whenever the handle's activation blocks or weight buffers are released or derived again (a change of the input shape, a
// load, train_begin / train_end): a captured step that ran the walk holds their addresses.  Unique in the process: no state of
// another handle, or of a later handle at the same address, has the same value
uint64_t resnet_workspace_generation(const sisic_resnet* r);
int resnet_input_gradient_walk(sisic_resnet* r, const float* x, int B, int H, int W, int target, const int* targets_dev,
                               float* grad_x, float* logits_out, hipStream_t s);
// conditional loop: out[b][r] = table[(step * L + slot[b]) * R + r] for the `rows` samples of a pass; cond: LoopCond
// {w, L, -, -, slot[rows]}; state != NULL: the step index is the loop state's (graph-replayed form)
constexpr size_t LOOP_COND_HEAD = 4;
int launch_loop_gather_rows(sisic_ctx*, const float* table, int R, const void* state, int step, const float* cond, int rows,
                            float* out, hipStream_t s);
int launch_noise_fill(sisic_ctx*, void* out, int B, int64_t n_per_image, const uint64_t* seeds_host, uint32_t step,
                      uint32_t tag, bool bits, hipStream_t s);
int launch_denorm_u8(sisic_ctx*, const float* x, uint8_t* out, int B, int C, int H, int W, hipStream_t s, int form = 0);
// time embedding: sinusoid -> linear1 -> SiLU -> linear2 -> SiLU  (weights transposed [in][out])
// save_* (optional, training): the sinusoid [B, 2 n_freqs] and the two linear outputs before their SiLU [B, hidden]
// class_table [N, hidden] with labels (device int [B], each in [0, N): the caller checks), both or neither: the class
// embedding's row is added to linear_2's output before its SiLU (and save_t2 holds the sum)
int launch_temb_mlp(sisic_ctx*, const float* t_vals, int B, const float* freqs, int n_freqs, const float* w1t,
                    const float* b1, const float* w2t, const float* b2, int hidden, float* temb_act, hipStream_t s,
                    float* save_emb = nullptr, float* save_h1 = nullptr, float* save_t2 = nullptr,
                    const float* class_table = nullptr, const int* labels = nullptr);
// out[b, r] = sum_k wt[k][r] * x[b][k] + bias[r]
int launch_linear_t(sisic_ctx*, const float* x, int B, int K, const float* wt, const float* bias, int R,
                    float* out, hipStream_t s);
int launch_transpose2d(sisic_ctx*, const float* in, int rows, int cols, float* out, int out_ld, int out_col0,
                       hipStream_t s);
// classifier.hip
int launch_preprocess(sisic_ctx*, const float* x, float* out, int B, int H, int W, int OH, int OW, hipStream_t s);
int launch_maxpool(sisic_ctx*, const float* x, float* out, int B, int C, int H, int W, hipStream_t s);
int launch_avgpool_fc(sisic_ctx*, const float* x, const float* w, const float* bias, float* out, int B, int C, int HW,
                      int n_out, hipStream_t s);
// AdaptiveAvgPool2d(1) alone: out [B, C], each value the bits avgpool_fc_kernel feeds its Linear
int launch_avgpool(sisic_ctx*, const float* x, float* out, int B, int C, int HW, hipStream_t s);
int launch_class_scores(sisic_ctx*, const float* logits, int B, int n, int target, float* prob, float* logscore,
                        hipStream_t s);
int launch_mask_patches(sisic_ctx*, const float* image, const uint8_t* masks, float* out, int S, int C, int H, int W,
                        int patch, hipStream_t s);

// xai_kernels.hip: counterfactual interventions and causal-shift metrics (include/sisic.h)
int launch_intervene(sisic_ctx*, const float* frames, int F, const uint8_t* masks, int M, int C, int H, int W, int J,
                     const sisic_intervention_job* jobs, const uint64_t* seeds, const int32_t* src_index, float* out,
                     float* intervention_out, float* stats, hipStream_t s);
int launch_cfi_metrics(sisic_ctx*, const float* logits_orig, int F, const float* logits_mod, int J, int n,
                       const int* job_frame, float* rows, hipStream_t s);
// bootstrap / permutation resamples of the mean difference (top, bottom: HOST doubles); synchronises s
int launch_resample_diffs(sisic_ctx*, const double* top, int n_top, const double* bottom, int n_bottom, uint64_t seed,
                          int n_bootstrap, int n_permutations, double* boot_out, double* perm_out, hipStream_t s);
// an OIHW weight replaced by noise_normal1(seed, e, trial, tag) * strength: raw = the BN-folded filter (float)((double)w * sc[co]),
// raw_t (may be NULL) its tap-flipped transposed copy; sc NULL writes the values themselves
int launch_randomize_weight(sisic_ctx*, float* raw, float* raw_t, const double* sc, int cout, int cin, int k, uint64_t seed,
                            uint32_t trial, uint32_t tag, float strength, hipStream_t s);

// eval_kernels.hip: the pairwise arithmetic of the evaluation metrics (include/sisic.h); the entry points check the arguments
int launch_gram(sisic_ctx*, const sisic_gram_args& g, hipStream_t s);
int launch_col_means(sisic_ctx*, const float* x, int64_t ld, int n, int d, double* mean_out, hipStream_t s);
int launch_matrix_sum(sisic_ctx*, const float* x, int64_t ld, int n, int m, int exclude_diagonal, double* out, hipStream_t s);
int launch_rows_topk(sisic_ctx*, const float* dist, int64_t ld, const float* col_offset, int n, int m, int k, int skip_diagonal,
                     float* val_out, int32_t* idx_out, hipStream_t s);
int launch_pair_sqdist(sisic_ctx*, const float* a, int64_t lda, const float* b, int64_t ldb, int n, int nb, int d, int k,
                       const int32_t* idx, float* out, hipStream_t s);

// augment.hip: the training loader's augmentation chain on a device-resident uint8 dataset (include/sisic.h); out is
// float32 [B,3,H,W] or, with u8, uint8 [B,H,W,3]
int launch_augment(sisic_ctx*, const uint8_t* dataset, int N, int H, int W, const sisic_augment_params* params_dev, int B,
                   int32_t* gray_mean_scratch, void* out, bool u8, hipStream_t s);

}  // namespace sisic

#include "tensor_dir.h"
