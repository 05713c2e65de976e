// api.cpp -- context, error reporting, launch timing and the extern "C" operator entry points
// of libsisic_hip.so (include/sisic.h).
#include <cstdio>
#include <cstring>

#include "common.h"
#include "conv_plan.h"
#include "gn_finalize.h"
#include "train.h"

namespace sisic {

static thread_local char g_err[1024] = "";

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// ---- launch timing ----------------------------------------------------------------------
// bench.py's roofline leg: every launch is bracketed by two HIP events recorded on the stream
// the kernel runs on; elapsed times are accumulated per kernel class when the profile is read.
static hipEvent_t take_event(sisic_ctx* ctx) {
    if (!ctx->event_pool.empty()) {
        hipEvent_t e = ctx->event_pool.back();
        ctx->event_pool.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    return e;
}

ProfileScope::ProfileScope(sisic_ctx* c, hipStream_t s, int kind, double bytes, double flops, double flops_exec, int kind2)
    : ctx(c), stream(s) {
    if (!c || !c->profiling) return;
    ev.start = take_event(c);
    ev.stop = take_event(c);
    ev.kind = kind;
    ev.kind2 = kind2;
    if (!ev.start || !ev.stop) return;
    for (int k : {kind, kind2}) {
        if (k < 0) continue;
        c->prof[k].bytes += bytes;
        c->prof[k].flops += flops;
        c->prof[k].flops_exec += (flops_exec < 0.0) ? flops : flops_exec;
        c->prof[k].launches += 1;
    }
    (void)hipEventRecord(ev.start, s);
    active = true;
}

ProfileScope::~ProfileScope() {
    if (!active) return;
    (void)hipEventRecord(ev.stop, stream);
    ctx->pending.push_back(ev);
}

int profile_collect(sisic_ctx* ctx) {
    for (auto& ev : ctx->pending) {
        SISIC_HIP(hipEventSynchronize(ev.stop));
        float ms = 0.f;
        SISIC_HIP(hipEventElapsedTime(&ms, ev.start, ev.stop));
        ctx->prof[ev.kind].ms += ms;
        if (ev.kind2 >= 0) ctx->prof[ev.kind2].ms += ms;
        ctx->event_pool.push_back(ev.start);
        ctx->event_pool.push_back(ev.stop);
    }
    ctx->pending.clear();
    return SISIC_OK;
}

}  // namespace sisic

using namespace sisic;

extern "C" {

int sisic_abi_version(void) { return SISIC_ABI_VERSION; }

const char* sisic_last_error(void) { return sisic::g_err; }

int sisic_create(int device_id, sisic_ctx** out) {
    SISIC_REQUIRE(out != nullptr, "sisic_create: out is NULL");
    *out = nullptr;
    int n = 0;
    SISIC_HIP(hipGetDeviceCount(&n));
    SISIC_REQUIRE(device_id >= 0 && device_id < n, "sisic_create: device %d of %d", device_id, n);
    SISIC_HIP(hipSetDevice(device_id));
    hipDeviceProp_t prop;
    SISIC_HIP(hipGetDeviceProperties(&prop, device_id));
    SISIC_REQUIRE(std::strncmp(prop.gcnArchName, "gfx950", 6) == 0,
                  "sisic_create: device %d is %s; this library is built for gfx950 (MI355X) only", device_id,
                  prop.gcnArchName);
    auto* ctx = new sisic_ctx();
    ctx->device = device_id;
    ctx->num_cus = prop.multiProcessorCount;
    *out = ctx;
    return SISIC_OK;
}

int sisic_destroy(sisic_ctx* ctx) {
    if (!ctx) return SISIC_OK;
    (void)profile_collect(ctx);
    for (auto e : ctx->event_pool) (void)hipEventDestroy(e);
    for (auto& kv : ctx->splitk)
        if (kv.second.p) (void)hipFree(kv.second.p);
    for (auto& kv : ctx->attn_rows)
        if (kv.second.p) (void)hipFree(kv.second.p);
    for (auto& kv : ctx->bn_part)
        if (kv.second.p) (void)hipFree(kv.second.p);
    for (auto& kv : ctx->thr_s)
        if (kv.second.p) (void)hipFree(kv.second.p);
    for (auto& it : ctx->bf3_items) {
        if (it.fill_done) (void)hipEventDestroy(it.fill_done);
        if (it.tab) (void)hipFree(it.tab);
    }
    delete ctx;
    return SISIC_OK;
}

int64_t sisic_conv_packed_numel(int Cout, int Cin, int ksize) {
    if (Cout <= 0 || Cin <= 0 || (ksize != 1 && ksize != 3 && ksize != 7)) return -1;
    return conv_packed_floats(Cout, Cin, ksize);
}

int sisic_conv_pack_weights(sisic_ctx* ctx, const float* w, int Cout, int Cin, int ksize, float* packed, void* stream) {
    SISIC_REQUIRE(ctx && w && packed && Cout > 0 && Cin > 0, "conv_pack_weights: bad arguments");
    return launch_conv_pack(ctx, w, Cout, Cin, ksize, packed, static_cast<hipStream_t>(stream));
}

int64_t sisic_conv_s2_numel(int Cout, int Cin) {
    if (Cout <= 0 || Cin <= 0) return -1;
    return conv_s2_packed_floats(Cout, Cin);
}

int sisic_conv_s2_pack(sisic_ctx* ctx, const float* w, int Cout, int Cin, float* out, void* stream) {
    SISIC_REQUIRE(ctx && w && out && Cout > 0 && Cin > 0, "conv_s2_pack: bad arguments");
    return launch_conv_s2_pack(ctx, w, Cout, Cin, out, static_cast<hipStream_t>(stream));
}

int64_t sisic_conv_winograd_numel(int Cout, int Cin) {
    if (Cout <= 0 || Cin <= 0) return -1;
    return winograd_packed_numel(Cout, Cin);
}

int sisic_conv_winograd_pack(sisic_ctx* ctx, const float* w, int Cout, int Cin, float* packed, void* stream) {
    SISIC_REQUIRE(ctx && w && packed && Cout > 0 && Cin > 0, "conv_winograd_pack: bad arguments");
    return launch_winograd_pack(ctx, w, Cout, Cin, packed, static_cast<hipStream_t>(stream));
}

int sisic_conv2d(sisic_ctx* ctx, const sisic_conv_args* args, void* stream) {
    SISIC_REQUIRE(ctx && args, "conv2d: null argument");
    return launch_conv2d(ctx, *args, static_cast<hipStream_t>(stream));
}

int sisic_conv_stats_slots(const sisic_conv_args* args) { return args ? conv_stats_slots(*args) : 0; }
int sisic_conv_finalizes(const sisic_conv_args* args) { return args && conv_finalizes(*args) ? 1 : 0; }
int sisic_conv_plan_info(const sisic_conv_args* args, int* kernel, int* cfg, int* form, char* refusal, int refusal_len) {
    SISIC_REQUIRE(args && (refusal || refusal_len <= 0), "conv_plan_info: null argument");
    if (refusal && refusal_len > 0) refusal[0] = 0;
    ConvPlan plan;
    SISIC_TRY(conv_plan(*args, &plan));
    if (kernel) *kernel = (int)plan.kernel;
    if (cfg) *cfg = plan.cfg;
    if (form) *form = plan.form;
    if (!plan.refusal[0]) return 0;
    if (refusal && refusal_len > 0) std::snprintf(refusal, (size_t)refusal_len, "%s", plan.refusal);
    return 1;
}

int sisic_groupnorm_finalize(sisic_ctx* ctx, const float* stats0, int c0, int slots0, const float* stats1, int c1,
                             int slots1, int B, int HW, int groups, float eps, const float* gamma, const float* beta,
                             float* scale, float* shift, void* stream) {
    SISIC_REQUIRE(ctx, "groupnorm_finalize: null context");
    return launch_gn_finalize(ctx, stats0, c0, slots0, stats1, c1, slots1, B, HW, groups, eps, gamma, beta, scale,
                              shift, static_cast<hipStream_t>(stream));
}

int sisic_conv2d_gn_rider(sisic_ctx* ctx, const sisic_conv_args* args, const float* stats0, int c0, int slots0,
                          const float* stats1, int c1, int slots1, int B, int HW, int groups, float eps, const float* gamma,
                          const float* beta, float* scale, float* shift, int* carried, void* stream) {
    SISIC_REQUIRE(ctx && args && carried, "conv2d_gn_rider: null argument");
    *carried = 0;
    SISIC_REQUIRE(HW > 0, "conv2d_gn_rider: HW=%d", HW);
    GnFinJob q{};
    SISIC_TRY(make_gn_fin_job(&q, stats0, c0, slots0, stats1, c1, slots1, B, groups, eps, gamma, beta, scale, shift));
    bool rode = false;
    SISIC_TRY(launch_conv2d(ctx, *args, static_cast<hipStream_t>(stream), &q, &rode));
    *carried = rode ? 1 : 0;
    return SISIC_OK;
}

int sisic_groupnorm_stats(sisic_ctx* ctx, const float* in0, int c0, const float* in1, int c1, int B, int HW,
                          int groups, float eps, const float* gamma, const float* beta, float* scale, float* shift,
                          void* stream) {
    SISIC_REQUIRE(ctx, "groupnorm_stats: null context");
    return launch_gn_stats(ctx, in0, c0, in1, c1, B, HW, groups, eps, gamma, beta, scale, shift,
                           static_cast<hipStream_t>(stream));
}

int sisic_attention(sisic_ctx* ctx, const float* qkv, float* out, int B, int C, int N, int head_dim, void* stream) {
    SISIC_REQUIRE(ctx, "attention: null context");
    return launch_attention(ctx, qkv, out, B, C, N, head_dim, static_cast<hipStream_t>(stream));
}

// The single scheduler steps: each entry names its part of one StepLaunch.  What eps means is the context's
// (sisic_set_step_prediction_type), in all nine.
static void step_tensors(StepLaunch& L, const sisic_ctx* ctx, int rule, int use_clipped_model_output, const float* eps,
                         const float* x, float* hist, float* out, int64_t n, const float* row, float clip) {
    L.rule = rule;
    L.flags = (use_clipped_model_output ? STEP_FLAG_CLIPPED_OUTPUT : 0) | step_pred_flags(ctx->step_pred);
    L.eps = eps; L.x = x; L.hist = hist; L.out = out; L.n = n; L.row = row; L.clip = clip;
}

// launch_step under the context's thresholding setting (sisic_set_step_thresholding): off, the launch as it is; on, the images
// are the entry's own (n_per_image) or the context's (sisic_set_step_image_elems), and s lies in the context's buffer of the stream
static int step_launch(sisic_ctx* ctx, const char* what, StepLaunch& L, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (ctx->step_thr_ratio > 0.0f) {
        if (L.n_per_image <= 0) L.n_per_image = ctx->step_npi;
        SISIC_REQUIRE(L.n_per_image > 0 && L.n > 0 && L.n % L.n_per_image == 0,
                      "%s: thresholding is on and %lld elements are not whole images of %lld (sisic_set_step_image_elems)", what,
                      (long long)L.n, (long long)L.n_per_image);
        L.thr_ratio = ctx->step_thr_ratio; L.thr_max = ctx->step_thr_max;
        SISIC_TRY(step_threshold_scratch(ctx, s, L.n / L.n_per_image, &L.thr_s));
    }
    return launch_step(ctx, L, s);
}

// the _rng entries: z generated in the kernel
static int step_rng(sisic_ctx* ctx, const char* what, StepLaunch& L, int rule, int use_clipped_model_output, const float* eps,
                    const float* x, float* hist, float* out, int B, int64_t n_per_image, const uint64_t* seeds_dev, uint32_t step,
                    const float* row, float clip, void* stream) {
    SISIC_REQUIRE(ctx && B > 0 && n_per_image > 0, "%s: null context or empty batch", what);
    step_tensors(L, ctx, rule, use_clipped_model_output, eps, x, hist, out, (int64_t)B * n_per_image, row, clip);
    L.device_noise = true; L.seeds_dev = seeds_dev; L.n_per_image = n_per_image; L.step = step;
    return step_launch(ctx, what, L, stream);
}

// the _edit entries: the _rng entries' arguments, the known image, the mask and the edit row
static int step_edit(sisic_ctx* ctx, const char* what, int rule, int use_clipped_model_output, const float* eps, const float* x,
                     float* hist, float* out, int B, int64_t n_per_image, const uint64_t* seeds_dev, uint32_t step,
                     const float* row, float clip, const float* x0k, const float* mask, int Cn, int64_t HW, float ck, float sk,
                     float ja, float jb, void* stream) {
    SISIC_REQUIRE(ctx && B > 0 && n_per_image > 0, "%s: null context or empty batch", what);
    SISIC_REQUIRE(Cn > 0 && HW > 0 && (int64_t)Cn * HW == n_per_image, "%s: C = %d, HW = %lld for images of %lld elements", what,
                  Cn, (long long)HW, (long long)n_per_image);
    const float erow[4] = {ck, sk, ja, jb};
    StepLaunch L;
    L.edit = true; L.x0k = x0k; L.mask = mask; L.hw = HW; L.erow = erow;
    return step_rng(ctx, what, L, rule, use_clipped_model_output, eps, x, hist, out, B, n_per_image, seeds_dev, step, row, clip, stream);
}

int sisic_ddpm_step(sisic_ctx* ctx, const float* eps, const float* x, const float* z, float* out, int64_t n,
                    float sqrt_beta_prod, float sqrt_alpha_prod, float c0, float c1, float sigma, float clip,
                    void* stream) {
    SISIC_REQUIRE(ctx, "ddpm_step: null context");
    const float row[5] = {sqrt_beta_prod, sqrt_alpha_prod, c0, c1, sigma};
    StepLaunch L;
    step_tensors(L, ctx, STEP_RULE_DDPM, 0, eps, x, nullptr, out, n, row, clip);
    L.z = z;
    return step_launch(ctx, "step", L, stream);
}

int sisic_ddim_step(sisic_ctx* ctx, const float* eps, const float* x, const float* z, float* out, int64_t n,
                    float sqrt_beta_prod, float sqrt_alpha_prod, float c_prev, float c_dir, float sigma, float clip,
                    int use_clipped_model_output, void* stream) {
    SISIC_REQUIRE(ctx, "ddim_step: null context");
    const float row[5] = {sqrt_beta_prod, sqrt_alpha_prod, c_prev, c_dir, sigma};
    StepLaunch L;
    step_tensors(L, ctx, STEP_RULE_DDIM, use_clipped_model_output, eps, x, nullptr, out, n, row, clip);
    L.z = z;
    return step_launch(ctx, "step", L, stream);
}

int sisic_dpmpp_step(sisic_ctx* ctx, const float* eps, const float* x, const float* z, float* hist, float* out, int64_t n,
                     float sqrt_beta_prod, float sqrt_alpha_prod, float cx, float k0, float sigma, float k1, float clip,
                     void* stream) {
    SISIC_REQUIRE(ctx, "dpmpp_step: null context");
    const float row[6] = {sqrt_beta_prod, sqrt_alpha_prod, cx, k0, sigma, k1};
    StepLaunch L;
    step_tensors(L, ctx, STEP_RULE_DPMPP, 0, eps, x, hist, out, n, row, clip);
    L.z = z;
    return step_launch(ctx, "step", L, stream);
}

int sisic_ddpm_step_rng(sisic_ctx* ctx, const float* eps, const float* x, float* out, int B, int64_t n_per_image,
                        const uint64_t* seeds_dev, uint32_t step, float sqrt_beta_prod, float sqrt_alpha_prod, float c0,
                        float c1, float sigma, float clip, void* stream) {
    const float row[5] = {sqrt_beta_prod, sqrt_alpha_prod, c0, c1, sigma};
    StepLaunch L;
    return step_rng(ctx, "ddpm_step_rng", L, STEP_RULE_DDPM, 0, eps, x, nullptr, out, B, n_per_image, seeds_dev, step, row, clip, stream);
}

int sisic_ddim_step_rng(sisic_ctx* ctx, const float* eps, const float* x, float* out, int B, int64_t n_per_image,
                        const uint64_t* seeds_dev, uint32_t step, float sqrt_beta_prod, float sqrt_alpha_prod, float c_prev,
                        float c_dir, float sigma, float clip, int use_clipped_model_output, void* stream) {
    const float row[5] = {sqrt_beta_prod, sqrt_alpha_prod, c_prev, c_dir, sigma};
    StepLaunch L;
    return step_rng(ctx, "ddim_step_rng", L, STEP_RULE_DDIM, use_clipped_model_output, eps, x, nullptr, out, B, n_per_image, seeds_dev,
                    step, row, clip, stream);
}

int sisic_dpmpp_step_rng(sisic_ctx* ctx, const float* eps, const float* x, float* hist, float* out, int B,
                         int64_t n_per_image, const uint64_t* seeds_dev, uint32_t step, float sqrt_beta_prod,
                         float sqrt_alpha_prod, float cx, float k0, float sigma, float k1, float clip, void* stream) {
    const float row[6] = {sqrt_beta_prod, sqrt_alpha_prod, cx, k0, sigma, k1};
    StepLaunch L;
    return step_rng(ctx, "dpmpp_step_rng", L, STEP_RULE_DPMPP, 0, eps, x, hist, out, B, n_per_image, seeds_dev, step, row, clip, stream);
}

int sisic_ddpm_step_edit(sisic_ctx* ctx, const float* eps, const float* x, float* out, int B, int64_t n_per_image,
                         const uint64_t* seeds_dev, uint32_t step, float sqrt_beta_prod, float sqrt_alpha_prod, float c0,
                         float c1, float sigma, float clip, const float* x0k, const float* mask, int C, int64_t HW, float ck,
                         float sk, float ja, float jb, void* stream) {
    const float row[5] = {sqrt_beta_prod, sqrt_alpha_prod, c0, c1, sigma};
    return step_edit(ctx, "ddpm_step_edit", STEP_RULE_DDPM, 0, eps, x, nullptr, out, B, n_per_image, seeds_dev, step, row, clip,
                     x0k, mask, C, HW, ck, sk, ja, jb, stream);
}

int sisic_ddim_step_edit(sisic_ctx* ctx, const float* eps, const float* x, float* out, int B, int64_t n_per_image,
                         const uint64_t* seeds_dev, uint32_t step, float sqrt_beta_prod, float sqrt_alpha_prod, float c_prev,
                         float c_dir, float sigma, float clip, int use_clipped_model_output, const float* x0k,
                         const float* mask, int C, int64_t HW, float ck, float sk, float ja, float jb, void* stream) {
    const float row[5] = {sqrt_beta_prod, sqrt_alpha_prod, c_prev, c_dir, sigma};
    return step_edit(ctx, "ddim_step_edit", STEP_RULE_DDIM, use_clipped_model_output, eps, x, nullptr, out, B, n_per_image, seeds_dev,
                     step, row, clip, x0k, mask, C, HW, ck, sk, ja, jb, stream);
}

int sisic_dpmpp_step_edit(sisic_ctx* ctx, const float* eps, const float* x, float* hist, float* out, int B,
                          int64_t n_per_image, const uint64_t* seeds_dev, uint32_t step, float sqrt_beta_prod,
                          float sqrt_alpha_prod, float cx, float k0, float sigma, float k1, float clip, const float* x0k,
                          const float* mask, int C, int64_t HW, float ck, float sk, float ja, float jb, void* stream) {
    const float row[6] = {sqrt_beta_prod, sqrt_alpha_prod, cx, k0, sigma, k1};
    return step_edit(ctx, "dpmpp_step_edit", STEP_RULE_DPMPP, 0, eps, x, hist, out, B, n_per_image, seeds_dev, step, row, clip,
                     x0k, mask, C, HW, ck, sk, ja, jb, stream);
}

int sisic_noise_fill(sisic_ctx* ctx, float* out, int B, int64_t n_per_image, const uint64_t* seeds, uint32_t step,
                     uint32_t tag, void* stream) {
    SISIC_REQUIRE(ctx, "noise_fill: null context");
    return launch_noise_fill(ctx, out, B, n_per_image, seeds, step, tag, false, static_cast<hipStream_t>(stream));
}

int sisic_noise_bits(sisic_ctx* ctx, uint32_t* out, int B, int64_t n_per_image, const uint64_t* seeds, uint32_t step,
                     uint32_t tag, void* stream) {
    SISIC_REQUIRE(ctx, "noise_bits: null context");
    return launch_noise_fill(ctx, out, B, n_per_image, seeds, step, tag, true, static_cast<hipStream_t>(stream));
}

int sisic_set_step_prediction_type(sisic_ctx* ctx, int type) {
    SISIC_REQUIRE(ctx, "set_step_prediction_type: null context");
    SISIC_REQUIRE(type == SISIC_PRED_EPSILON || type == SISIC_PRED_SAMPLE || type == SISIC_PRED_V,
                  "set_step_prediction_type: type %d (0 = epsilon, 1 = sample, 2 = v)", type);
    ctx->step_pred = type;
    return SISIC_OK;
}

int sisic_step_prediction_type(const sisic_ctx* ctx) { return ctx ? ctx->step_pred : SISIC_PRED_EPSILON; }

int sisic_set_step_thresholding(sisic_ctx* ctx, float ratio, float sample_max_value) {
    SISIC_REQUIRE(ctx, "set_step_thresholding: null context");
    SISIC_TRY(check_thresholding("set_step_thresholding", ratio, sample_max_value));
    ctx->step_thr_ratio = ratio > 0.0f ? ratio : 0.0f;
    ctx->step_thr_max = sample_max_value;
    return SISIC_OK;
}

int sisic_set_step_image_elems(sisic_ctx* ctx, int64_t n_per_image) {
    SISIC_REQUIRE(ctx, "set_step_image_elems: null context");
    SISIC_REQUIRE(n_per_image >= 0 && n_per_image <= ((int64_t)1 << 24), "set_step_image_elems: %lld elements per image (0 .. 2^24)",
                  (long long)n_per_image);
    ctx->step_npi = n_per_image;
    return SISIC_OK;
}

int sisic_x0_threshold(sisic_ctx* ctx, sisic_x0_threshold_args* a) {
    SISIC_REQUIRE(ctx && a, "x0_threshold: null argument");
    SISIC_REQUIRE(a->B > 0 && a->n_per_image > 0, "x0_threshold: empty batch");
    SISIC_REQUIRE(a->source >= 0 && a->source <= 2, "x0_threshold: eps source %d (0 = plain, 1 = guided, 2 = classifier)", a->source);
    const float row[6] = {a->sb, a->sa, 0.0f, 0.0f, 0.0f, 0.0f};
    StepLaunch L;
    L.rule = STEP_RULE_DDPM;
    L.flags = step_pred_flags(ctx->step_pred);
    L.source = a->source == 1 ? STEP_EPS_GUIDED : a->source == 2 ? STEP_EPS_CLASSIFIER : STEP_EPS_PLAIN;
    L.eps = a->eps; L.eps_u = a->eps2; L.grad = a->eps2; L.x = a->x; L.row = row; L.w = a->w;
    L.n_per_image = a->n_per_image; L.n = (int64_t)a->B * a->n_per_image;
    L.thr_s = a->s; L.thr_ratio = a->ratio; L.thr_max = a->sample_max_value;
    return launch_x0_threshold(ctx, L, static_cast<hipStream_t>(a->stream));
}

int sisic_denorm_u8(sisic_ctx* ctx, const float* x, uint8_t* out, int B, int C, int H, int W, void* stream) {
    SISIC_REQUIRE(ctx, "denorm_u8: null context");
    return launch_denorm_u8(ctx, x, out, B, C, H, W, static_cast<hipStream_t>(stream));
}

int sisic_denorm_u8_form(sisic_ctx* ctx, const float* x, uint8_t* out, int B, int C, int H, int W, int form, void* stream) {
    SISIC_REQUIRE(ctx, "denorm_u8_form: null context");
    return launch_denorm_u8(ctx, x, out, B, C, H, W, static_cast<hipStream_t>(stream), form);
}

int sisic_intervene(sisic_ctx* ctx, const float* frames, int F, const uint8_t* masks, int M, int C, int H, int W, int J,
                    const sisic_intervention_job* jobs, const uint64_t* seeds, const int32_t* src_index, float* out,
                    float* intervention_out, float* stats, void* stream) {
    SISIC_REQUIRE(ctx, "intervene: null context");
    return launch_intervene(ctx, frames, F, masks, M, C, H, W, J, jobs, seeds, src_index, out, intervention_out, stats,
                            static_cast<hipStream_t>(stream));
}

int sisic_cfi_metrics(sisic_ctx* ctx, const float* logits_orig, int F, const float* logits_mod, int J, int n_classes,
                      const int* job_frame, float* rows, void* stream) {
    SISIC_REQUIRE(ctx, "cfi_metrics: null context");
    return launch_cfi_metrics(ctx, logits_orig, F, logits_mod, J, n_classes, job_frame, rows, static_cast<hipStream_t>(stream));
}

int sisic_resample_diffs(sisic_ctx* ctx, const double* top, int n_top, const double* bottom, int n_bottom, uint64_t seed,
                         int n_bootstrap, int n_permutations, double* boot_out, double* perm_out, void* stream) {
    SISIC_REQUIRE(ctx, "resample_diffs: null context");
    return launch_resample_diffs(ctx, top, n_top, bottom, n_bottom, seed, n_bootstrap, n_permutations, boot_out, perm_out,
                                 static_cast<hipStream_t>(stream));
}

int sisic_augment(sisic_ctx* ctx, const uint8_t* dataset, int N, int H, int W, const sisic_augment_params* params_dev, int B,
                  int32_t* gray_mean_scratch, float* out, void* stream) {
    SISIC_REQUIRE(ctx, "augment: null context");
    return launch_augment(ctx, dataset, N, H, W, params_dev, B, gray_mean_scratch, out, false, static_cast<hipStream_t>(stream));
}

int sisic_augment_u8(sisic_ctx* ctx, const uint8_t* dataset, int N, int H, int W, const sisic_augment_params* params_dev,
                     int B, int32_t* gray_mean_scratch, uint8_t* out_hwc, void* stream) {
    SISIC_REQUIRE(ctx, "augment_u8: null context");
    return launch_augment(ctx, dataset, N, H, W, params_dev, B, gray_mean_scratch, out_hwc, true, static_cast<hipStream_t>(stream));
}

int sisic_batchnorm_train(sisic_ctx* ctx, sisic_bn_args* a) {
    SISIC_REQUIRE(ctx && a, "batchnorm_train: null argument");
    SISIC_REQUIRE(a->y && a->mean && a->invstd && (!a->out || (a->gamma && a->beta)), "batchnorm_train: y, mean and invstd are required, and gamma and beta with out");
    hipStream_t s = static_cast<hipStream_t>(a->stream);
    SISIC_TRY(launch_bn_moments(ctx, a->y, a->B, a->C, a->HW, a->eps, a->mean, a->invstd, nullptr, a->running_mean, a->running_var,
                                a->momentum, s));
    if (!a->out) return SISIC_OK;              // the moments alone
    return launch_bn_apply(ctx, a->y, a->gamma, a->beta, a->mean, a->invstd, a->residual, a->relu != 0, a->out, a->B, a->C, a->HW, s);
}

int sisic_batchnorm_train_bwd(sisic_ctx* ctx, sisic_bn_args* a) {
    SISIC_REQUIRE(ctx && a, "batchnorm_train_bwd: null argument");
    SISIC_REQUIRE(a->g && a->y && a->gamma && a->mean && a->invstd && a->dgamma && a->dbeta,
                  "batchnorm_train_bwd: g, y, gamma, mean, invstd, dgamma and dbeta are required");
    return launch_bn_bwd(ctx, a->g, a->y, a->act, a->mean, a->invstd, a->gamma, a->dy, a->dgamma, a->dbeta, a->B, a->C, a->HW,
                         static_cast<hipStream_t>(a->stream));
}

int sisic_add_relu(sisic_ctx* ctx, sisic_bn_args* a) {
    SISIC_REQUIRE(ctx && a && a->y && a->residual && a->out && a->B > 0 && a->C > 0 && a->HW > 0, "add_relu: y, residual, out and a shape are required");
    return launch_add_relu(ctx, a->y, a->residual, a->out, (int64_t)a->B * a->C * a->HW, static_cast<hipStream_t>(a->stream));
}

// ---- evaluation of generated sets (eval_kernels.hip) ---------------------------------------------------------------------------
int sisic_col_means(sisic_ctx* ctx, sisic_col_means_args* a) {
    SISIC_REQUIRE(ctx && a && a->x && a->mean_out, "col_means: null argument");
    SISIC_REQUIRE(a->n > 0 && a->d > 0 && a->ld >= a->d, "col_means: n %d, d %d, ld %lld", a->n, a->d, (long long)a->ld);
    return launch_col_means(ctx, a->x, a->ld, a->n, a->d, a->mean_out, static_cast<hipStream_t>(a->stream));
}

int sisic_gram(sisic_ctx* ctx, const sisic_gram_args* a) {
    SISIC_REQUIRE(ctx && a && a->a && a->out, "gram: null argument");
    SISIC_REQUIRE(a->n > 0 && a->d > 0 && a->lda >= a->d, "gram: n %d, d %d, lda %lld", a->n, a->d, (long long)a->lda);
    SISIC_REQUIRE(a->mode == SISIC_GRAM_DOT || a->mode == SISIC_GRAM_SQDIST || a->mode == SISIC_GRAM_POLY3, "gram: unknown mode %d",
                  a->mode);
    if (a->contract_rows) {
        SISIC_REQUIRE(!a->b && !a->shift_b && a->mode == SISIC_GRAM_DOT,
                      "gram: contract_rows computes A'^T A' alone: b and shift_b must be NULL and the mode SISIC_GRAM_DOT (mode %d)", a->mode);
        SISIC_REQUIRE(a->ldo >= a->d, "gram: ldo %lld below the row length %d", (long long)a->ldo, a->d);
    } else {
        SISIC_REQUIRE(a->m > 0 && a->ldo >= a->m, "gram: m %d, ldo %lld", a->m, (long long)a->ldo);
        SISIC_REQUIRE(!a->b || a->ldb >= a->d, "gram: ldb %lld below the row length %d", (long long)a->ldb, a->d);
    }
    return launch_gram(ctx, *a, static_cast<hipStream_t>(a->stream));
}

int sisic_rows_topk(sisic_ctx* ctx, sisic_rows_topk_args* a) {
    SISIC_REQUIRE(ctx && a && a->dist && a->val_out && a->idx_out, "rows_topk: null argument");
    SISIC_REQUIRE(a->n > 0 && a->m > 0 && a->ld >= a->m, "rows_topk: n %d, m %d, ld %lld", a->n, a->m, (long long)a->ld);
    const int skip = a->skip_diagonal ? 1 : 0;
    SISIC_REQUIRE(a->k >= 1 && a->k <= 8 && a->k <= a->m - skip,
                  "rows_topk: k = %d with m = %d columns%s: 1 <= k <= 8 and k <= m - skip_diagonal", a->k, a->m,
                  skip ? " and the diagonal skipped" : "");
    return launch_rows_topk(ctx, a->dist, a->ld, a->col_offset, a->n, a->m, a->k, skip, a->val_out, a->idx_out,
                            static_cast<hipStream_t>(a->stream));
}

int sisic_pair_sqdist(sisic_ctx* ctx, sisic_pair_sqdist_args* a) {
    SISIC_REQUIRE(ctx && a && a->a && a->b && a->idx && a->out, "pair_sqdist: null argument");
    SISIC_REQUIRE(a->n > 0 && a->nb > 0 && a->d > 0 && a->k > 0 && a->lda >= a->d && a->ldb >= a->d,
                  "pair_sqdist: n %d, nb %d, d %d, k %d, lda %lld, ldb %lld", a->n, a->nb, a->d, a->k, (long long)a->lda,
                  (long long)a->ldb);
    SISIC_REQUIRE((int64_t)a->n * a->k <= 0x7fffffff, "pair_sqdist: %lld pairs in one call", (long long)a->n * a->k);
    return launch_pair_sqdist(ctx, a->a, a->lda, a->b, a->ldb, a->n, a->nb, a->d, a->k, a->idx, a->out,
                              static_cast<hipStream_t>(a->stream));
}

int sisic_matrix_sum(sisic_ctx* ctx, sisic_matrix_sum_args* a) {
    SISIC_REQUIRE(ctx && a && a->x && a->out, "matrix_sum: null argument");
    SISIC_REQUIRE(a->n > 0 && a->m > 0 && a->ld >= a->m, "matrix_sum: n %d, m %d, ld %lld", a->n, a->m, (long long)a->ld);
    return launch_matrix_sum(ctx, a->x, a->ld, a->n, a->m, a->exclude_diagonal ? 1 : 0, a->out, static_cast<hipStream_t>(a->stream));
}

int sisic_profile_enable(sisic_ctx* ctx, int on) {
    SISIC_REQUIRE(ctx, "profile_enable: null context");
    ctx->profiling = on != 0;
    return SISIC_OK;
}

int sisic_profile_read(sisic_ctx* ctx, int kind, double* ms, int64_t* launches, double* bytes, double* flops,
                       double* flops_executed) {
    SISIC_REQUIRE(ctx && kind >= 0 && kind < PK_COUNT, "profile_read: bad arguments");
    SISIC_TRY(profile_collect(ctx));
    if (ms) *ms = ctx->prof[kind].ms;
    if (launches) *launches = ctx->prof[kind].launches;
    if (bytes) *bytes = ctx->prof[kind].bytes;
    if (flops) *flops = ctx->prof[kind].flops;
    if (flops_executed) *flops_executed = ctx->prof[kind].flops_exec;
    return SISIC_OK;
}

int sisic_profile_reset(sisic_ctx* ctx) {
    SISIC_REQUIRE(ctx, "profile_reset: null context");
    SISIC_TRY(profile_collect(ctx));
    for (auto& p : ctx->prof) p = ProfileSlot();
    return SISIC_OK;
}

}  // extern "C"
