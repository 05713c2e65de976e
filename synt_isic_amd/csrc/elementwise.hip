// elementwise.hip -- the HBM-bound and tiny kernels of the sampling loop:
//   * ddpm_step_kernel  : fused DDPMScheduler.step, bit-exact vs torch CPU
//   * ddim_step_kernel  : fused DDIMScheduler.step (epsilon prediction), bit-exact vs torch CPU
//   * dpm_step_kernel   : fused DPM-Solver++(2M) step with its one-step history, bit-exact vs torch CPU
//   * step_edit_kernel  : the three steps with the inpainting epilogue (RePaint) applied before the store
//     (every step kernel under each prediction type -- epsilon, sample, v: sisic.h SISIC_PRED_*, a template parameter of the rule)
//   * denorm_u8_kernel  : clamp((x+1)/2,0,1)*255 -> uint8 HWC (image_generator.py:441-447)
//   * temb_mlp_kernel   : sinusoidal timestep embedding -> Linear -> SiLU -> Linear -> SiLU
//   * linear_t_kernel   : every ResnetBlock2D.time_emb_proj in one launch
//   * transpose2d_kernel: weight re-layout at load time
#include "common.h"
#include "noise_device.h"
#include "pack_device.h"

namespace sisic {

// ---- DDPM step -------------------------------------------------------------------------
// One IEEE rounding per operation and NO FMA contraction (this file is built with
// -ffp-contract=off, and the pragma pins it locally): that is what the reference's sequence of
// separate torch ops produces, so the step is bit-exact against torch on the CPU.
//
// P, the prediction type (sisic.h SISIC_PRED_*): what the model's output e means, and so how a rule gets its x0 from it.  A
// template parameter of every rule, like the rule itself: no element branches on it, and P = PRED_EPS is the code these
// kernels always were.
constexpr int PRED_EPS = SISIC_PRED_EPSILON, PRED_SAMPLE = SISIC_PRED_SAMPLE, PRED_V = SISIC_PRED_V;

// x0 before the clamp: epsilon (x - sb*e)/sa; sample e; v (= sa*eps - sb*x0) sa*x - sb*e, with no division
template <int P>
__device__ __forceinline__ float pred_x0(float e, float x, float sb, float sa) {
#pragma clang fp contract(off)
    if constexpr (P == PRED_SAMPLE) return e;
    else if constexpr (P == PRED_V) return sa * x - sb * e;
    else return (x - sb * e) / sa;
}

template <int P>
__device__ __forceinline__ float ddpm_one(float e, float x, float z, float sb, float sa, float c0, float c1,
                                          float sigma, float clip, bool noise) {
#pragma clang fp contract(off)
    float x0 = pred_x0<P>(e, x, sb, sa);
    if (clip > 0.0f) x0 = fminf(fmaxf(x0, -clip), clip);
    float r = c0 * x0 + c1 * x;
    if (noise) r = r + sigma * z;
    return r;
}

// ---- DDIM step -------------------------------------------------------------------------
// The published DDIMScheduler.step for epsilon prediction, under the same rounding rules as ddpm_one.  The row of a step is
// {sb = (1-abar_t)^.5, sa = abar_t^.5, c_prev = abar_prev^.5, c_dir = (1 - abar_prev - sigma^2)^.5, sigma = eta * variance^.5}.
// CLIPPED (use_clipped_model_output): the direction term uses the epsilon re-derived from the clamped x0.
// The direction term's epsilon under the other types: sample (x - sa*x0)/sb with the UNCLAMPED x0; v sa*e + sb*x.
template <bool CLIPPED, int P>
__device__ __forceinline__ float ddim_one(float e, float x, float z, float sb, float sa, float c_prev, float c_dir,
                                          float sigma, float clip, bool noise) {
#pragma clang fp contract(off)
    const float x0u = pred_x0<P>(e, x, sb, sa);
    float x0 = x0u;
    if (clip > 0.0f) x0 = fminf(fmaxf(x0, -clip), clip);
    float pe = e;
    if constexpr (CLIPPED) pe = (x - sa * x0) / sb;
    else if constexpr (P == PRED_SAMPLE) pe = (x - sa * x0u) / sb;
    else if constexpr (P == PRED_V) pe = sa * e + sb * x;
    float r = c_prev * x0 + c_dir * pe;
    if (noise) r = r + sigma * z;
    return r;
}

// The step rule as a functor: the row of five scalars and the clip range, applied to one element.  step_body is instantiated
// once per rule and noise source, so no element pays for a branch on the rule.
template <int P = PRED_EPS>
struct DdpmRule {
    float sb, sa, c0, c1, sigma, clip;
    __device__ __forceinline__ float operator()(float e, float x, float z, bool noise) const {
        return ddpm_one<P>(e, x, z, sb, sa, c0, c1, sigma, clip, noise);
    }
};

template <bool CLIPPED, int P = PRED_EPS>
struct DdimRule {
    float sb, sa, c_prev, c_dir, sigma, clip;
    __device__ __forceinline__ float operator()(float e, float x, float z, bool noise) const {
        return ddim_one<CLIPPED, P>(e, x, z, sb, sa, c_prev, c_dir, sigma, clip, noise);
    }
};

// Where a step's z comes from: a buffer the caller filled, or the counter-based generator of noise_device.h (the device-noise
// contract).  Both feed the same rule, so the step's arithmetic after z does not depend on the source.
struct BufferNoise {
    const float* __restrict__ z;
    __device__ __forceinline__ bool present() const { return z != nullptr; }
    __device__ __forceinline__ bool vec_ok() const { return (reinterpret_cast<uintptr_t>(z) & 15) == 0; }
    __device__ __forceinline__ float4 get4(int64_t i4) const { return reinterpret_cast<const float4*>(z)[i4]; }
    __device__ __forceinline__ float get1(int64_t i) const { return z[i]; }
};

struct PhiloxNoise {
    const uint64_t* seeds;    // [B] device
    int64_t npi;              // floats per image
    uint32_t step;            // step index of the run (position in its timestep list)
    uint32_t tag = 0u;        // the stream of the contract (sisic.h): 0 = a step's z; the edit epilogue draws under 5 and 6
    __device__ __forceinline__ bool present() const { return true; }
    __device__ __forceinline__ bool vec_ok() const { return (npi & 3) == 0; }     // otherwise a block straddles two images
    __device__ __forceinline__ float4 get4(int64_t i4) const {
        const int64_t q_per_image = npi >> 2, b = i4 / q_per_image;
        return noise_normal4(seeds[b], (uint32_t)(i4 - b * q_per_image), step, tag);
    }
    __device__ __forceinline__ float get1(int64_t i) const {
        const int64_t b = i / npi;
        return noise_normal1(seeds[b], i - b * npi, step, tag);
    }
};

// Where a step's eps comes from: the UNet's output as it stands, or (classifier-free guidance) combined from the conditional
// and the unconditional prediction of one pass at twice the batch.  The rule sees one eps either way.
struct PlainEps {
    const float* __restrict__ e;
    static constexpr bool dup = false;
    __device__ __forceinline__ float4 get4(int64_t i4) const { return reinterpret_cast<const float4*>(e)[i4]; }
    __device__ __forceinline__ float get1(int64_t i) const { return e[i]; }
};

// eps = eps_u + w * (eps_c - eps_u): subtract, multiply, add, each rounded to fp32 (what sisic_guide_eps computes)
__device__ __forceinline__ float guide_one(float c, float u, float w) {
#pragma clang fp contract(off)
    const float d = c - u;
    const float t = w * d;
    return u + t;
}

// dup: the step's result goes to out AND out + n, the two halves of the [2B] latent buffer the next pass reads
struct GuidedEps {
    const float* __restrict__ ec;
    const float* __restrict__ eu;
    float w;
    static constexpr bool dup = true;
    __device__ __forceinline__ float4 get4(int64_t i4) const {
        const float4 c = reinterpret_cast<const float4*>(ec)[i4], u = reinterpret_cast<const float4*>(eu)[i4];
        return make_float4(guide_one(c.x, u.x, w), guide_one(c.y, u.y, w), guide_one(c.z, u.z, w), guide_one(c.w, u.w, w));
    }
    __device__ __forceinline__ float get1(int64_t i) const { return guide_one(ec[i], eu[i], w); }
};

// What happens to a step's result before it is stored: nothing, or the inpainting epilogue (RePaint, Lugmayr et al. 2022;
// DESIGN.md section 2).  The epilogue re-imposes the known image x0k at the noise level the step arrives at, under the mask m
// (1 = keep the known pixel), and optionally jumps the result back up the schedule.  One fp32 rounding per operation, in this
// order (sisic.h, sisic_ddpm_step_edit):
//   k = ck * x0k [+ sk * e1];   y = m * k + (1 - m) * u;   out = jb != 0 ? ja * y + jb * e2 : y
// e1, e2: the image's Philox normals at this step's index under tags 5 and 6, drawn only where sk / jb are not zero.  x0k and
// m are two more read streams of the launch (m a third as wide: it is broadcast over the channels), u never leaves its
// register: the known region costs no second pass over the latent.
struct NoEdit {
    static constexpr bool on = false;
};

constexpr uint32_t NOISE_TAG_KNOWN = 5u, NOISE_TAG_JUMP = 6u;

__device__ __forceinline__ float edit_one(float u, float x0k, float m, float e1, float e2, float ck, float sk, float ja,
                                          float jb) {
#pragma clang fp contract(off)
    float k = ck * x0k;
    if (sk != 0.0f) k = k + sk * e1;
    const float a = m * k;
    const float om = 1.0f - m;
    const float b = om * u;
    float y = a + b;
    if (jb != 0.0f) y = ja * y + jb * e2;
    return y;
}

struct InpaintEdit {
    static constexpr bool on = true;
    const float* __restrict__ x0k;      // [B, C, HW], finite
    const float* __restrict__ mask;     // [B, 1, HW]
    const uint64_t* seeds;              // [B] device
    int64_t npi, hw;                    // C * HW and HW
    uint32_t step;
    float ck, sk, ja, jb;
    // (get4: npi and hw are multiples of 4, so float4 i4 of the latent lies in one image, one channel and one float4 of m)
    __device__ __forceinline__ float4 apply4(int64_t i4, float4 u) const {
        const int64_t q_per_image = npi >> 2, b = i4 / q_per_image, q = i4 - b * q_per_image, hw4 = hw >> 2;
        const float4 kv = reinterpret_cast<const float4*>(x0k)[i4];
        const float4 mv = reinterpret_cast<const float4*>(mask)[b * hw4 + q % hw4];
        float4 e1 = make_float4(0.f, 0.f, 0.f, 0.f), e2 = make_float4(0.f, 0.f, 0.f, 0.f);
        if (sk != 0.0f) e1 = noise_normal4(seeds[b], (uint32_t)q, step, NOISE_TAG_KNOWN);
        if (jb != 0.0f) e2 = noise_normal4(seeds[b], (uint32_t)q, step, NOISE_TAG_JUMP);
        return make_float4(edit_one(u.x, kv.x, mv.x, e1.x, e2.x, ck, sk, ja, jb), edit_one(u.y, kv.y, mv.y, e1.y, e2.y, ck, sk, ja, jb),
                           edit_one(u.z, kv.z, mv.z, e1.z, e2.z, ck, sk, ja, jb), edit_one(u.w, kv.w, mv.w, e1.w, e2.w, ck, sk, ja, jb));
    }
    __device__ __forceinline__ float apply1(int64_t i, float u) const {
        const int64_t b = i / npi, r = i - b * npi;
        const float e1 = sk != 0.0f ? noise_normal1(seeds[b], r, step, NOISE_TAG_KNOWN) : 0.f;
        const float e2 = jb != 0.0f ? noise_normal1(seeds[b], r, step, NOISE_TAG_JUMP) : 0.f;
        return edit_one(u, x0k[i], mask[b * hw + r % hw], e1, e2, ck, sk, ja, jb);
    }
};

// out may alias x (the loop steps in place): every element is read before it is written, by the thread that writes it
// (E::dup: vec4 only with n a multiple of 4, so that out + n is aligned like out)
template <class R, class Z, class E, class D = NoEdit>
__device__ __forceinline__ void step_body(const E es, const float* x, float* out, int64_t n, bool vec4,
                                          const R rule, const Z zs, const D ed = D{}) {
    const bool noise = zs.present() && (rule.sigma != 0.0f);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (vec4) {
        const int64_t n4 = n >> 2;
        const float4* x4 = reinterpret_cast<const float4*>(x);
        float4* o4 = reinterpret_cast<float4*>(out);
        for (int64_t i = t0; i < n4; i += stride) {
            const float4 e = es.get4(i), xv = x4[i];
            float4 zv = make_float4(0.f, 0.f, 0.f, 0.f);
            if (noise) zv = zs.get4(i);
            float4 r;
            r.x = rule(e.x, xv.x, zv.x, noise);
            r.y = rule(e.y, xv.y, zv.y, noise);
            r.z = rule(e.z, xv.z, zv.z, noise);
            r.w = rule(e.w, xv.w, zv.w, noise);
            if constexpr (D::on) r = ed.apply4(i, r);
            o4[i] = r;
            if constexpr (E::dup) o4[n4 + i] = r;
        }
        for (int64_t i = (n4 << 2) + t0; i < n; i += stride) {
            float r = rule(es.get1(i), x[i], noise ? zs.get1(i) : 0.f, noise);
            if constexpr (D::on) r = ed.apply1(i, r);
            out[i] = r;
            if constexpr (E::dup) out[n + i] = r;
        }
    } else {
        for (int64_t i = t0; i < n; i += stride) {
            float r = rule(es.get1(i), x[i], noise ? zs.get1(i) : 0.f, noise);
            if constexpr (D::on) r = ed.apply1(i, r);
            out[i] = r;
            if constexpr (E::dup) out[n + i] = r;
        }
    }
}

template <int P>
__global__ void __launch_bounds__(256)
ddpm_step_kernel(const float* __restrict__ eps, const float* x, const float* __restrict__ z,
                 float* out, int64_t n, float sb, float sa, float c0, float c1, float sigma, float clip,
                 int vec4) {
    step_body(PlainEps{eps}, x, out, n, vec4 != 0, DdpmRule<P>{sb, sa, c0, c1, sigma, clip}, BufferNoise{z});
}

// the same step with z generated in the kernel (sisic_sample_frames_rng, eager form)
template <int P>
__global__ void __launch_bounds__(256)
ddpm_step_rng_kernel(const float* __restrict__ eps, const float* x, float* out, int64_t n, int64_t n_per_image,
                     const uint64_t* __restrict__ seeds, uint32_t step, float sb, float sa, float c0, float c1, float sigma,
                     float clip, int vec4) {
    const PhiloxNoise zs{seeds, n_per_image, step};
    step_body(PlainEps{eps}, x, out, n, vec4 != 0 && zs.vec_ok(), DdpmRule<P>{sb, sa, c0, c1, sigma, clip}, zs);
}

// the DDIM rule in the same two forms
template <bool CLIPPED, int P>
__global__ void __launch_bounds__(256)
ddim_step_kernel(const float* __restrict__ eps, const float* x, const float* __restrict__ z, float* out, int64_t n, float sb,
                 float sa, float c_prev, float c_dir, float sigma, float clip, int vec4) {
    step_body(PlainEps{eps}, x, out, n, vec4 != 0, DdimRule<CLIPPED, P>{sb, sa, c_prev, c_dir, sigma, clip}, BufferNoise{z});
}

template <bool CLIPPED, int P>
__global__ void __launch_bounds__(256)
ddim_step_rng_kernel(const float* __restrict__ eps, const float* x, float* out, int64_t n, int64_t n_per_image,
                     const uint64_t* __restrict__ seeds, uint32_t step, float sb, float sa, float c_prev, float c_dir,
                     float sigma, float clip, int vec4) {
    const PhiloxNoise zs{seeds, n_per_image, step};
    step_body(PlainEps{eps}, x, out, n, vec4 != 0 && zs.vec_ok(), DdimRule<CLIPPED, P>{sb, sa, c_prev, c_dir, sigma, clip}, zs);
}

// ---- DPM-Solver++(2M) step -------------------------------------------------------------
// The second-order multistep rule of Lu et al. 2022 for epsilon prediction, with its coefficients folded on the host: the row
// of a step is {sb = sigma_t, sa = alpha_t, cx, k0, sigma, k1} (sisic.h SISIC_RULE_DPMPP) and the step
//   x0 = clamp((x - sb*e)/sa);  out = cx*x + k0*x0 [+ k1*hist] [+ sigma*z];  hist = x0
// under the rounding rules of ddpm_one.  hist is the previous step's x0: one more stream, read (second-order steps only) and
// written in place by the thread that owns the element, so a captured step replays as it is.  A first-order step (k1 == 0,
// uniform over the launch) does not read it: whatever an earlier run left there, NaN included, stays out of the result.
template <int P = PRED_EPS>
struct DpmRule {
    float sb, sa, cx, k0, sigma, k1, clip;
    // h: the history's element (any value when !second); m0: this step's x0, the next step's history
    __device__ __forceinline__ float operator()(float e, float x, float z, float h, bool noise, bool second, float& m0) const {
#pragma clang fp contract(off)
        float x0 = pred_x0<P>(e, x, sb, sa);
        if (clip > 0.0f) x0 = fminf(fmaxf(x0, -clip), clip);
        float r = cx * x + k0 * x0;
        if (second) r = r + k1 * h;
        if (noise) r = r + sigma * z;
        m0 = x0;
        return r;
    }
};

// step_body with the history stream.  out may alias x; hist aliases nothing else (and stays n wide under E::dup).
template <class R, class Z, class E, class D = NoEdit>
__device__ __forceinline__ void dpm_step_body(const E es, const float* x, float* hist, float* out, int64_t n,
                                              bool vec4, const R rule, const Z zs, const D ed = D{}) {
    const bool noise = zs.present() && (rule.sigma != 0.0f);
    const bool second = rule.k1 != 0.0f;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t tail = t0;
    if (vec4) {
        const int64_t n4 = n >> 2;
        const float4* x4 = reinterpret_cast<const float4*>(x);
        float4* h4 = reinterpret_cast<float4*>(hist);
        float4* o4 = reinterpret_cast<float4*>(out);
        for (int64_t i = t0; i < n4; i += stride) {
            const float4 e = es.get4(i), xv = x4[i];
            float4 hv = make_float4(0.f, 0.f, 0.f, 0.f), zv = make_float4(0.f, 0.f, 0.f, 0.f);
            if (second) hv = h4[i];
            if (noise) zv = zs.get4(i);
            float4 r, m;
            r.x = rule(e.x, xv.x, zv.x, hv.x, noise, second, m.x);
            r.y = rule(e.y, xv.y, zv.y, hv.y, noise, second, m.y);
            r.z = rule(e.z, xv.z, zv.z, hv.z, noise, second, m.z);
            r.w = rule(e.w, xv.w, zv.w, hv.w, noise, second, m.w);
            if constexpr (D::on) r = ed.apply4(i, r);      // (the history stays the model's x0)
            h4[i] = m;
            o4[i] = r;
            if constexpr (E::dup) o4[n4 + i] = r;
        }
        tail = (n4 << 2) + t0;
    }
    for (int64_t i = tail; i < n; i += stride) {
        float m;
        float r = rule(es.get1(i), x[i], noise ? zs.get1(i) : 0.f, second ? hist[i] : 0.f, noise, second, m);
        if constexpr (D::on) r = ed.apply1(i, r);
        hist[i] = m;
        out[i] = r;
        if constexpr (E::dup) out[n + i] = r;
    }
}

template <int P>
__global__ void __launch_bounds__(256)
dpm_step_kernel(const float* __restrict__ eps, const float* x, const float* __restrict__ z, float* hist, float* out, int64_t n,
                float sb, float sa, float cx, float k0, float sigma, float k1, float clip, int vec4) {
    dpm_step_body(PlainEps{eps}, x, hist, out, n, vec4 != 0, DpmRule<P>{sb, sa, cx, k0, sigma, k1, clip}, BufferNoise{z});
}

template <int P>
__global__ void __launch_bounds__(256)
dpm_step_rng_kernel(const float* __restrict__ eps, const float* x, float* hist, float* out, int64_t n, int64_t n_per_image,
                    const uint64_t* __restrict__ seeds, uint32_t step, float sb, float sa, float cx, float k0, float sigma,
                    float k1, float clip, int vec4) {
    const PhiloxNoise zs{seeds, n_per_image, step};
    dpm_step_body(PlainEps{eps}, x, hist, out, n, vec4 != 0 && zs.vec_ok(), DpmRule<P>{sb, sa, cx, k0, sigma, k1, clip}, zs);
}

static const char* rule_name(int rule) {
    return rule == STEP_RULE_DPMPP ? "dpmpp_step" : rule == STEP_RULE_DDIM ? "ddim_step" : "ddpm_step";
}

// the rule and its flags as the C ABI passes them; the divisors of the rule's row when they are launch arguments
static int check_rule(int rule, int flags) {
    SISIC_REQUIRE(rule == STEP_RULE_DDPM || rule == STEP_RULE_DDIM || rule == STEP_RULE_DPMPP,
                  "step rule %d (0 = DDPM, 1 = DDIM, 2 = DPM-Solver++)", rule);
    // (the prediction type's private bits ride along: common.h STEP_FLAG_PRED_MASK)
    const int own = flags & ~STEP_FLAG_PRED_MASK;
    SISIC_REQUIRE((own & ~STEP_FLAG_CLIPPED_OUTPUT) == 0 && (rule == STEP_RULE_DDIM || own == 0),
                  "%s: rule flags %d (DDIM: 1 = use_clipped_model_output; DDPM, DPM-Solver++: none)", rule_name(rule), own);
    SISIC_REQUIRE(step_pred(flags) <= PRED_V, "%s: prediction type %d (0 = epsilon, 1 = sample, 2 = v)", rule_name(rule),
                  step_pred(flags));
    return SISIC_OK;
}

// A launch under the prediction type that `flags` carries: the statements see it as the constant P.
#define SISIC_PRED_SWITCH(flags, ...)                                                  \
    switch (step_pred(flags)) {                                                        \
        case PRED_SAMPLE: { constexpr int P = PRED_SAMPLE; __VA_ARGS__; } break;       \
        case PRED_V: { constexpr int P = PRED_V; __VA_ARGS__; } break;                 \
        default: { constexpr int P = PRED_EPS; __VA_ARGS__; } break;                   \
    }

int check_step_row(int rule, int flags, float sb, float sa) {
    SISIC_TRY(check_rule(rule, flags));
    SISIC_REQUIRE(sa != 0.0f, "%s: sqrt_alpha_prod is zero", rule_name(rule));
    SISIC_REQUIRE(!(flags & STEP_FLAG_CLIPPED_OUTPUT) || sb != 0.0f,
                  "%s: sqrt_beta_prod is zero with use_clipped_model_output", rule_name(rule));
    SISIC_REQUIRE(!(rule == STEP_RULE_DDIM && step_pred(flags) == PRED_SAMPLE) || sb != 0.0f,
                  "%s: sqrt_beta_prod is zero under sample prediction (the direction term divides by it)", rule_name(rule));
    return SISIC_OK;
}

int launch_step(sisic_ctx* ctx, int rule, int flags, const float* eps, const float* x, const float* z, float* out, int64_t n,
                float sb, float sa, float c2, float c3, float sigma, float clip, hipStream_t s) {
    SISIC_TRY(check_rule(rule, flags));
    SISIC_REQUIRE(rule != STEP_RULE_DPMPP, "dpmpp_step: the rule takes a history buffer (launch_dpm_step*)");
    SISIC_REQUIRE(eps && x && out && n > 0, "%s: null tensor or empty", rule_name(rule));
    SISIC_TRY(check_step_row(rule, flags, sb, sa));
    const bool noise = z != nullptr && sigma != 0.0f;
    ProfileScope prof(ctx, s, PK_DDPM, (noise ? 16.0 : 12.0) * (double)n, 0.0);
    const uintptr_t al = reinterpret_cast<uintptr_t>(eps) | reinterpret_cast<uintptr_t>(x) |
                         reinterpret_cast<uintptr_t>(z) | reinterpret_cast<uintptr_t>(out);
    const int vec4 = (al & 15) == 0;
    const int64_t work = vec4 ? (n + 3) / 4 : n;
    const int blocks = (int)std::min<int64_t>((work + 255) / 256, 2048);
    SISIC_PRED_SWITCH(flags,
        if (rule == STEP_RULE_DDPM)
            hipLaunchKernelGGL(ddpm_step_kernel<P>, dim3(blocks), dim3(256), 0, s, eps, x, z, out, n, sb, sa, c2, c3, sigma, clip,
                               vec4);
        else if (flags & STEP_FLAG_CLIPPED_OUTPUT)
            hipLaunchKernelGGL((ddim_step_kernel<true, P>), dim3(blocks), dim3(256), 0, s, eps, x, z, out, n, sb, sa, c2, c3, sigma,
                               clip, vec4);
        else
            hipLaunchKernelGGL((ddim_step_kernel<false, P>), dim3(blocks), dim3(256), 0, s, eps, x, z, out, n, sb, sa, c2, c3, sigma,
                               clip, vec4))
    SISIC_HIP(hipGetLastError());
    return SISIC_OK;
}

// counter word 0 of a block is its index in the image: 32 bits
static constexpr int64_t NOISE_MAX_PER_IMAGE = (int64_t)1 << 34;

int launch_step_rng(sisic_ctx* ctx, int rule, int flags, const float* eps, const float* x, float* out, int64_t n,
                    int64_t n_per_image, const uint64_t* seeds_dev, uint32_t step, float sb, float sa, float c2, float c3,
                    float sigma, float clip, hipStream_t s) {
    SISIC_TRY(check_rule(rule, flags));
    SISIC_REQUIRE(rule != STEP_RULE_DPMPP, "dpmpp_step: the rule takes a history buffer (launch_dpm_step*)");
    SISIC_REQUIRE(eps && x && out && seeds_dev && n > 0, "%s_rng: null tensor or empty", rule_name(rule));
    SISIC_REQUIRE(n_per_image > 0 && n_per_image <= NOISE_MAX_PER_IMAGE && n % n_per_image == 0,
                  "%s_rng: %lld elements are not whole images of %lld", rule_name(rule), (long long)n, (long long)n_per_image);
    SISIC_TRY(check_step_row(rule, flags, sb, sa));
    ProfileScope prof(ctx, s, PK_DDPM, 12.0 * (double)n, 0.0);
    const uintptr_t al = reinterpret_cast<uintptr_t>(eps) | reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out);
    const int vec4 = (al & 15) == 0 && (n_per_image & 3) == 0;
    const int64_t work = vec4 ? n / 4 : n;
    const int blocks = (int)std::min<int64_t>((work + 255) / 256, 2048);
    SISIC_PRED_SWITCH(flags,
        if (rule == STEP_RULE_DDPM)
            hipLaunchKernelGGL(ddpm_step_rng_kernel<P>, dim3(blocks), dim3(256), 0, s, eps, x, out, n, n_per_image, seeds_dev, step,
                               sb, sa, c2, c3, sigma, clip, vec4);
        else if (flags & STEP_FLAG_CLIPPED_OUTPUT)
            hipLaunchKernelGGL((ddim_step_rng_kernel<true, P>), dim3(blocks), dim3(256), 0, s, eps, x, out, n, n_per_image,
                               seeds_dev, step, sb, sa, c2, c3, sigma, clip, vec4);
        else
            hipLaunchKernelGGL((ddim_step_rng_kernel<false, P>), dim3(blocks), dim3(256), 0, s, eps, x, out, n, n_per_image,
                               seeds_dev, step, sb, sa, c2, c3, sigma, clip, vec4))
    SISIC_HIP(hipGetLastError());
    return SISIC_OK;
}

// the DPM-Solver++ step: launch_step / launch_step_rng with the history stream and the sixth scalar of its row
int launch_dpm_step(sisic_ctx* ctx, const float* eps, const float* x, const float* z, float* hist, float* out, int64_t n,
                    float sb, float sa, float cx, float k0, float sigma, float k1, float clip, hipStream_t s, int flags) {
    SISIC_REQUIRE(eps && x && hist && out && n > 0, "dpmpp_step: null tensor or empty");
    SISIC_REQUIRE(hist != x && hist != out && hist != eps, "dpmpp_step: the history aliases another tensor");
    SISIC_TRY(check_step_row(STEP_RULE_DPMPP, flags, sb, sa));
    const bool noise = z != nullptr && sigma != 0.0f;
    ProfileScope prof(ctx, s, PK_DDPM, ((noise ? 20.0 : 16.0) + (k1 != 0.0f ? 4.0 : 0.0)) * (double)n, 0.0);
    const uintptr_t al = reinterpret_cast<uintptr_t>(eps) | reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(z) |
                         reinterpret_cast<uintptr_t>(hist) | reinterpret_cast<uintptr_t>(out);
    const int vec4 = (al & 15) == 0;
    const int64_t work = vec4 ? (n + 3) / 4 : n;
    const int blocks = (int)std::min<int64_t>((work + 255) / 256, 2048);
    SISIC_PRED_SWITCH(flags, hipLaunchKernelGGL(dpm_step_kernel<P>, dim3(blocks), dim3(256), 0, s, eps, x, z, hist, out, n, sb, sa,
                                                cx, k0, sigma, k1, clip, vec4))
    SISIC_HIP(hipGetLastError());
    return SISIC_OK;
}

int launch_dpm_step_rng(sisic_ctx* ctx, const float* eps, const float* x, float* hist, float* out, int64_t n,
                        int64_t n_per_image, const uint64_t* seeds_dev, uint32_t step, float sb, float sa, float cx, float k0,
                        float sigma, float k1, float clip, hipStream_t s, int flags) {
    SISIC_REQUIRE(eps && x && hist && out && seeds_dev && n > 0, "dpmpp_step_rng: null tensor or empty");
    SISIC_REQUIRE(hist != x && hist != out && hist != eps, "dpmpp_step_rng: the history aliases another tensor");
    SISIC_REQUIRE(n_per_image > 0 && n_per_image <= NOISE_MAX_PER_IMAGE && n % n_per_image == 0,
                  "dpmpp_step_rng: %lld elements are not whole images of %lld", (long long)n, (long long)n_per_image);
    SISIC_TRY(check_step_row(STEP_RULE_DPMPP, flags, sb, sa));
    ProfileScope prof(ctx, s, PK_DDPM, (16.0 + (k1 != 0.0f ? 4.0 : 0.0)) * (double)n, 0.0);
    const uintptr_t al = reinterpret_cast<uintptr_t>(eps) | reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(hist) |
                         reinterpret_cast<uintptr_t>(out);
    const int vec4 = (al & 15) == 0 && (n_per_image & 3) == 0;
    const int64_t work = vec4 ? n / 4 : n;
    const int blocks = (int)std::min<int64_t>((work + 255) / 256, 2048);
    SISIC_PRED_SWITCH(flags, hipLaunchKernelGGL(dpm_step_rng_kernel<P>, dim3(blocks), dim3(256), 0, s, eps, x, hist, out, n,
                                                n_per_image, seeds_dev, step, sb, sa, cx, k0, sigma, k1, clip, vec4))
    SISIC_HIP(hipGetLastError());
    return SISIC_OK;
}

// ---- the same step with its per-step parameters read from device memory (graph-replayed sampling loop) ----------------
// One captured step is replayed for every step of the loop, so nothing that changes from step to step may be a launch
// argument: the loop keeps {step index, noise base pointer} and its per-step tables (coefficients, noise row of the step
// or -1) in device memory; this kernel selects its row, ddpm_advance_kernel moves the index on.  Nothing that changes from
// call to call either: a generated-noise call's first step index is `step_base`, and its seeds lie in a library-owned
// buffer whose address is part of the captured launch.  The rule and its flag choose the kernel, so they are part of what a
// captured step is (LoopKey).
struct LoopState {
    int step;
    int step_base;            // generated noise: the Philox step index is step_base + step (0 in buffer-noise calls)
    const float* noise;       // base of the [n_noise, n] noise rows of this call
};

// R{sb, sa, c2, c3, sigma, clip}: DdpmRule or DdimRule<>, the row of the current step
template <class R>
__device__ __forceinline__ R loop_rule(const float* __restrict__ coef, int step, float clip) {
    return R{coef[5 * step + 0], coef[5 * step + 1], coef[5 * step + 2], coef[5 * step + 3], coef[5 * step + 4], clip};
}

template <class R>
__device__ __forceinline__ void step_indexed_body(const float* __restrict__ eps, float* x, int64_t n,
                                                  const LoopState* __restrict__ st, const float* __restrict__ coef,
                                                  const int* __restrict__ zrow, float clip, int vec4) {
    const int step = st->step;
    const int zr = zrow[step];
    const BufferNoise zs{zr >= 0 ? st->noise + (int64_t)zr * n : nullptr};
    step_body(PlainEps{eps}, x, x, n, vec4 != 0 && zs.vec_ok(), loop_rule<R>(coef, step, clip), zs);
}

template <class R>
__device__ __forceinline__ void step_indexed_rng_body(const float* __restrict__ eps, float* x, int64_t n, int64_t n_per_image,
                                                      const LoopState* __restrict__ st, const float* __restrict__ coef,
                                                      const uint64_t* __restrict__ seeds, float clip, int vec4) {
    const int step = st->step;
    const PhiloxNoise zs{seeds, n_per_image, (uint32_t)(st->step_base + step)};
    step_body(PlainEps{eps}, x, x, n, vec4 != 0 && zs.vec_ok(), loop_rule<R>(coef, step, clip), zs);
}

template <int P>
__global__ void __launch_bounds__(256)
ddpm_step_indexed_kernel(const float* __restrict__ eps, float* x, int64_t n, const LoopState* __restrict__ st,
                         const float* __restrict__ coef, const int* __restrict__ zrow, float clip, int vec4) {
    step_indexed_body<DdpmRule<P>>(eps, x, n, st, coef, zrow, clip, vec4);
}

template <int P>
__global__ void __launch_bounds__(256)
ddpm_step_indexed_rng_kernel(const float* __restrict__ eps, float* x, int64_t n, int64_t n_per_image,
                             const LoopState* __restrict__ st, const float* __restrict__ coef,
                             const uint64_t* __restrict__ seeds, float clip, int vec4) {
    step_indexed_rng_body<DdpmRule<P>>(eps, x, n, n_per_image, st, coef, seeds, clip, vec4);
}

template <bool CLIPPED, int P>
__global__ void __launch_bounds__(256)
ddim_step_indexed_kernel(const float* __restrict__ eps, float* x, int64_t n, const LoopState* __restrict__ st,
                         const float* __restrict__ coef, const int* __restrict__ zrow, float clip, int vec4) {
    step_indexed_body<DdimRule<CLIPPED, P>>(eps, x, n, st, coef, zrow, clip, vec4);
}

template <bool CLIPPED, int P>
__global__ void __launch_bounds__(256)
ddim_step_indexed_rng_kernel(const float* __restrict__ eps, float* x, int64_t n, int64_t n_per_image,
                             const LoopState* __restrict__ st, const float* __restrict__ coef,
                             const uint64_t* __restrict__ seeds, float clip, int vec4) {
    step_indexed_rng_body<DdimRule<CLIPPED, P>>(eps, x, n, n_per_image, st, coef, seeds, clip, vec4);
}

// the DPM-Solver++ rule: rows of six floats, and the history buffer of the loop
template <int P>
__device__ __forceinline__ DpmRule<P> loop_dpm_rule(const float* __restrict__ coef, int step, float clip) {
    const float* c = coef + 6 * step;
    return DpmRule<P>{c[0], c[1], c[2], c[3], c[4], c[5], clip};
}

template <int P>
__global__ void __launch_bounds__(256)
dpm_step_indexed_kernel(const float* __restrict__ eps, float* x, float* hist, int64_t n, const LoopState* __restrict__ st,
                        const float* __restrict__ coef, const int* __restrict__ zrow, float clip, int vec4) {
    const int step = st->step;
    const int zr = zrow[step];
    const BufferNoise zs{zr >= 0 ? st->noise + (int64_t)zr * n : nullptr};
    dpm_step_body(PlainEps{eps}, x, hist, x, n, vec4 != 0 && zs.vec_ok(), loop_dpm_rule<P>(coef, step, clip), zs);
}

template <int P>
__global__ void __launch_bounds__(256)
dpm_step_indexed_rng_kernel(const float* __restrict__ eps, float* x, float* hist, int64_t n, int64_t n_per_image,
                            const LoopState* __restrict__ st, const float* __restrict__ coef,
                            const uint64_t* __restrict__ seeds, float clip, int vec4) {
    const int step = st->step;
    const PhiloxNoise zs{seeds, n_per_image, (uint32_t)(st->step_base + step)};
    dpm_step_body(PlainEps{eps}, x, hist, x, n, vec4 != 0 && zs.vec_ok(), loop_dpm_rule<P>(coef, step, clip), zs);
}

// tproj_cur[r] = tproj_table[step][r]: the time-embedding projections of the step about to run
__global__ void loop_select_row_kernel(const float* __restrict__ table, int R, const LoopState* __restrict__ st,
                                       float* __restrict__ out) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < R) out[r] = table[(size_t)st->step * R + r];
}

__global__ void loop_advance_kernel(LoopState* st) { st->step += 1; }

int launch_loop_select_row(sisic_ctx*, const float* table, int R, const void* state, float* out, hipStream_t s) {
    hipLaunchKernelGGL(loop_select_row_kernel, dim3(cdiv(R, 256)), dim3(256), 0, s, table, R, static_cast<const LoopState*>(state), out);
    SISIC_HIP(hipGetLastError());
    return SISIC_OK;
}

int launch_loop_advance(sisic_ctx*, void* state, hipStream_t s) {
    hipLaunchKernelGGL(loop_advance_kernel, dim3(1), dim3(1), 0, s, static_cast<LoopState*>(state));
    SISIC_HIP(hipGetLastError());
    return SISIC_OK;
}

int launch_step_indexed(sisic_ctx* ctx, int rule, int flags, const float* eps, float* x, int64_t n, const void* state,
                        const float* coef, const int* zrow, float clip, hipStream_t s) {
    SISIC_TRY(check_rule(rule, flags));
    SISIC_REQUIRE(rule != STEP_RULE_DPMPP, "dpmpp_step: the rule takes a history buffer (launch_dpm_step*)");
    SISIC_REQUIRE(eps && x && state && coef && zrow && n > 0, "%s_indexed: null argument", rule_name(rule));
    ProfileScope prof(ctx, s, PK_DDPM, 16.0 * (double)n, 0.0);
    const uintptr_t al = reinterpret_cast<uintptr_t>(eps) | reinterpret_cast<uintptr_t>(x);
    const int vec4 = (al & 15) == 0 && (n & 3) == 0;
    const int64_t work = vec4 ? (n + 3) / 4 : n;
    const int blocks = (int)std::min<int64_t>((work + 255) / 256, 2048);
    const LoopState* st = static_cast<const LoopState*>(state);
    SISIC_PRED_SWITCH(flags,
        if (rule == STEP_RULE_DDPM)
            hipLaunchKernelGGL(ddpm_step_indexed_kernel<P>, dim3(blocks), dim3(256), 0, s, eps, x, n, st, coef, zrow, clip, vec4);
        else if (flags & STEP_FLAG_CLIPPED_OUTPUT)
            hipLaunchKernelGGL((ddim_step_indexed_kernel<true, P>), dim3(blocks), dim3(256), 0, s, eps, x, n, st, coef, zrow, clip, vec4);
        else
            hipLaunchKernelGGL((ddim_step_indexed_kernel<false, P>), dim3(blocks), dim3(256), 0, s, eps, x, n, st, coef, zrow, clip, vec4))
    SISIC_HIP(hipGetLastError());
    return SISIC_OK;
}

int launch_step_indexed_rng(sisic_ctx* ctx, int rule, int flags, const float* eps, float* x, int64_t n, int64_t n_per_image,
                            const void* state, const float* coef, const uint64_t* seeds_dev, float clip, hipStream_t s) {
    SISIC_TRY(check_rule(rule, flags));
    SISIC_REQUIRE(rule != STEP_RULE_DPMPP, "dpmpp_step: the rule takes a history buffer (launch_dpm_step*)");
    SISIC_REQUIRE(eps && x && state && coef && seeds_dev && n > 0, "%s_indexed_rng: null argument", rule_name(rule));
    SISIC_REQUIRE(n_per_image > 0 && n_per_image <= NOISE_MAX_PER_IMAGE && n % n_per_image == 0,
                  "%s_indexed_rng: %lld elements are not whole images of %lld", rule_name(rule), (long long)n,
                  (long long)n_per_image);
    ProfileScope prof(ctx, s, PK_DDPM, 12.0 * (double)n, 0.0);
    const uintptr_t al = reinterpret_cast<uintptr_t>(eps) | reinterpret_cast<uintptr_t>(x);
    const int vec4 = (al & 15) == 0 && (n_per_image & 3) == 0;
    const int64_t work = vec4 ? n / 4 : n;
    const int blocks = (int)std::min<int64_t>((work + 255) / 256, 2048);
    const LoopState* st = static_cast<const LoopState*>(state);
    SISIC_PRED_SWITCH(flags,
        if (rule == STEP_RULE_DDPM)
            hipLaunchKernelGGL(ddpm_step_indexed_rng_kernel<P>, dim3(blocks), dim3(256), 0, s, eps, x, n, n_per_image, st, coef,
                               seeds_dev, clip, vec4);
        else if (flags & STEP_FLAG_CLIPPED_OUTPUT)
            hipLaunchKernelGGL((ddim_step_indexed_rng_kernel<true, P>), dim3(blocks), dim3(256), 0, s, eps, x, n, n_per_image, st,
                               coef, seeds_dev, clip, vec4);
        else
            hipLaunchKernelGGL((ddim_step_indexed_rng_kernel<false, P>), dim3(blocks), dim3(256), 0, s, eps, x, n, n_per_image, st,
                               coef, seeds_dev, clip, vec4))
    SISIC_HIP(hipGetLastError());
    return SISIC_OK;
}

int launch_dpm_step_indexed(sisic_ctx* ctx, const float* eps, float* x, float* hist, int64_t n, const void* state,
                            const float* coef, const int* zrow, float clip, hipStream_t s, int flags) {
    SISIC_TRY(check_rule(STEP_RULE_DPMPP, flags));
    SISIC_REQUIRE(eps && x && hist && state && coef && zrow && n > 0, "dpmpp_step_indexed: null argument");
    ProfileScope prof(ctx, s, PK_DDPM, 24.0 * (double)n, 0.0);
    const uintptr_t al = reinterpret_cast<uintptr_t>(eps) | reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(hist);
    const int vec4 = (al & 15) == 0 && (n & 3) == 0;
    const int64_t work = vec4 ? (n + 3) / 4 : n;
    const int blocks = (int)std::min<int64_t>((work + 255) / 256, 2048);
    SISIC_PRED_SWITCH(flags, hipLaunchKernelGGL(dpm_step_indexed_kernel<P>, dim3(blocks), dim3(256), 0, s, eps, x, hist, n,
                                                static_cast<const LoopState*>(state), coef, zrow, clip, vec4))
    SISIC_HIP(hipGetLastError());
    return SISIC_OK;
}

int launch_dpm_step_indexed_rng(sisic_ctx* ctx, const float* eps, float* x, float* hist, int64_t n, int64_t n_per_image,
                                const void* state, const float* coef, const uint64_t* seeds_dev, float clip, hipStream_t s,
                                int flags) {
    SISIC_TRY(check_rule(STEP_RULE_DPMPP, flags));
    SISIC_REQUIRE(eps && x && hist && state && coef && seeds_dev && n > 0, "dpmpp_step_indexed_rng: null argument");
    SISIC_REQUIRE(n_per_image > 0 && n_per_image <= NOISE_MAX_PER_IMAGE && n % n_per_image == 0,
                  "dpmpp_step_indexed_rng: %lld elements are not whole images of %lld", (long long)n, (long long)n_per_image);
    ProfileScope prof(ctx, s, PK_DDPM, 20.0 * (double)n, 0.0);
    const uintptr_t al = reinterpret_cast<uintptr_t>(eps) | reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(hist);
    const int vec4 = (al & 15) == 0 && (n_per_image & 3) == 0;
    const int64_t work = vec4 ? n / 4 : n;
    const int blocks = (int)std::min<int64_t>((work + 255) / 256, 2048);
    SISIC_PRED_SWITCH(flags, hipLaunchKernelGGL(dpm_step_indexed_rng_kernel<P>, dim3(blocks), dim3(256), 0, s, eps, x, hist, n,
                                                n_per_image, static_cast<const LoopState*>(state), coef, seeds_dev, clip, vec4))
    SISIC_HIP(hipGetLastError());
    return SISIC_OK;
}

// ---- classifier-free guidance: the same steps reading eps through GuidedEps --------------------------------------------------
// One UNet pass at batch 2B leaves the conditional predictions in the first n floats of eps2 and the null-label ones in the
// second n; the step applies its rule to guide_one() of the two and writes the new x to both halves of x2 [2n].  z, the seeds,
// the history and n are those of the B images.  NZ: 0 a noise buffer, 1 generated noise.  The eager kernels take w and the row
// as launch arguments; the indexed ones read the row by the loop's step index and w from cond[0] (LoopCond, below), so that a
// captured step replays under another scale.
struct StepRow { float v[6]; };     // a rule's row: {sb, sa, c2, c3, sigma} or DPM-Solver++'s six

template <class R>
__device__ __forceinline__ R row_rule(const StepRow& r, float clip) { return R{r.v[0], r.v[1], r.v[2], r.v[3], r.v[4], clip}; }

template <class R, int NZ>
__global__ void __launch_bounds__(256)
step_guided_kernel(const float* __restrict__ ec, const float* __restrict__ eu, float w, const float* x, const float* __restrict__ z,
                   const uint64_t* __restrict__ seeds, int64_t n_per_image, uint32_t step, float* out, int64_t n, StepRow row,
                   float clip, int vec4) {
    const GuidedEps es{ec, eu, w};
    if constexpr (NZ == 0) {
        step_body(es, x, out, n, vec4 != 0, row_rule<R>(row, clip), BufferNoise{z});
    } else {
        const PhiloxNoise zs{seeds, n_per_image, step};
        step_body(es, x, out, n, vec4 != 0 && zs.vec_ok(), row_rule<R>(row, clip), zs);
    }
}

template <int NZ, int P>
__global__ void __launch_bounds__(256)
dpm_step_guided_kernel(const float* __restrict__ ec, const float* __restrict__ eu, float w, const float* x,
                       const float* __restrict__ z, const uint64_t* __restrict__ seeds, int64_t n_per_image, uint32_t step,
                       float* hist, float* out, int64_t n, StepRow row, float clip, int vec4) {
    const GuidedEps es{ec, eu, w};
    const DpmRule<P> rule{row.v[0], row.v[1], row.v[2], row.v[3], row.v[4], row.v[5], clip};
    if constexpr (NZ == 0) {
        dpm_step_body(es, x, hist, out, n, vec4 != 0, rule, BufferNoise{z});
    } else {
        const PhiloxNoise zs{seeds, n_per_image, step};
        dpm_step_body(es, x, hist, out, n, vec4 != 0 && zs.vec_ok(), rule, zs);
    }
}

template <class R, int NZ>
__global__ void __launch_bounds__(256)
step_guided_indexed_kernel(const float* __restrict__ eps2, float* x2, int64_t n, int64_t n_per_image,
                           const LoopState* __restrict__ st, const float* __restrict__ coef, const int* __restrict__ zrow,
                           const uint64_t* __restrict__ seeds, const float* __restrict__ cond, float clip, int vec4) {
    const int step = st->step;
    const GuidedEps es{eps2, eps2 + n, cond[0]};
    if constexpr (NZ == 0) {
        const int zr = zrow[step];
        const BufferNoise zs{zr >= 0 ? st->noise + (int64_t)zr * n : nullptr};
        step_body(es, x2, x2, n, vec4 != 0 && zs.vec_ok(), loop_rule<R>(coef, step, clip), zs);
    } else {
        const PhiloxNoise zs{seeds, n_per_image, (uint32_t)(st->step_base + step)};
        step_body(es, x2, x2, n, vec4 != 0 && zs.vec_ok(), loop_rule<R>(coef, step, clip), zs);
    }
}

template <int NZ, int P>
__global__ void __launch_bounds__(256)
dpm_step_guided_indexed_kernel(const float* __restrict__ eps2, float* x2, float* hist, int64_t n, int64_t n_per_image,
                               const LoopState* __restrict__ st, const float* __restrict__ coef, const int* __restrict__ zrow,
                               const uint64_t* __restrict__ seeds, const float* __restrict__ cond, float clip, int vec4) {
    const int step = st->step;
    const GuidedEps es{eps2, eps2 + n, cond[0]};
    if constexpr (NZ == 0) {
        const int zr = zrow[step];
        const BufferNoise zs{zr >= 0 ? st->noise + (int64_t)zr * n : nullptr};
        dpm_step_body(es, x2, hist, x2, n, vec4 != 0 && zs.vec_ok(), loop_dpm_rule<P>(coef, step, clip), zs);
    } else {
        const PhiloxNoise zs{seeds, n_per_image, (uint32_t)(st->step_base + step)};
        dpm_step_body(es, x2, hist, x2, n, vec4 != 0 && zs.vec_ok(), loop_dpm_rule<P>(coef, step, clip), zs);
    }
}

// z != NULL or seeds_dev == NULL: the noise buffer (or none); seeds_dev: generated noise.  row: the rule's host row.
// out: [2n] (may be x's own buffer: x is its first n floats); hist: DPM-Solver++ only.
int launch_step_guided(sisic_ctx* ctx, int rule, int flags, const float* eps_c, const float* eps_u, float w, const float* x,
                       const float* z, const uint64_t* seeds_dev, int64_t n_per_image, uint32_t step, float* hist, float* out,
                       int64_t n, const float* row, float clip, hipStream_t s) {
    SISIC_TRY(check_rule(rule, flags));
    SISIC_REQUIRE(eps_c && eps_u && x && out && row && n > 0, "%s (guided): null tensor or empty", rule_name(rule));
    SISIC_REQUIRE(rule != STEP_RULE_DPMPP || (hist && hist != x && hist != out && hist != eps_c && hist != eps_u),
                  "dpmpp_step (guided): the history is missing or aliases another tensor");
    SISIC_REQUIRE(!seeds_dev || (n_per_image > 0 && n_per_image <= NOISE_MAX_PER_IMAGE && n % n_per_image == 0),
                  "%s (guided): %lld elements are not whole images of %lld", rule_name(rule), (long long)n, (long long)n_per_image);
    SISIC_TRY(check_step_row(rule, flags, row[0], row[1]));
    ProfileScope prof(ctx, s, PK_DDPM, 24.0 * (double)n, 0.0);
    StepRow r{};
    for (int k = 0; k < (int)SISIC_RULE_ROW_WIDTH(rule); ++k) r.v[k] = row[k];
    const uintptr_t al = reinterpret_cast<uintptr_t>(eps_c) | reinterpret_cast<uintptr_t>(eps_u) | reinterpret_cast<uintptr_t>(x) |
                         reinterpret_cast<uintptr_t>(z) | reinterpret_cast<uintptr_t>(hist) | reinterpret_cast<uintptr_t>(out);
    const int vec4 = (al & 15) == 0 && (n & 3) == 0 && (!seeds_dev || (n_per_image & 3) == 0);
    const int64_t work = vec4 ? n / 4 : n;
    const dim3 grid((unsigned)std::min<int64_t>((work + 255) / 256, 2048)), block(256);
#define SISIC_GUIDED(K) hipLaunchKernelGGL(K, grid, block, 0, s, eps_c, eps_u, w, x, z, seeds_dev, n_per_image, step, out, n, r, clip, vec4)
    SISIC_PRED_SWITCH(flags,
        if (rule == STEP_RULE_DPMPP) {
            if (seeds_dev) hipLaunchKernelGGL((dpm_step_guided_kernel<1, P>), grid, block, 0, s, eps_c, eps_u, w, x, z, seeds_dev, n_per_image, step, hist, out, n, r, clip, vec4);
            else hipLaunchKernelGGL((dpm_step_guided_kernel<0, P>), grid, block, 0, s, eps_c, eps_u, w, x, z, seeds_dev, n_per_image, step, hist, out, n, r, clip, vec4);
        } else if (rule == STEP_RULE_DDPM) {
            if (seeds_dev) SISIC_GUIDED((step_guided_kernel<DdpmRule<P>, 1>)); else SISIC_GUIDED((step_guided_kernel<DdpmRule<P>, 0>));
        } else if (flags & STEP_FLAG_CLIPPED_OUTPUT) {
            if (seeds_dev) SISIC_GUIDED((step_guided_kernel<DdimRule<true, P>, 1>)); else SISIC_GUIDED((step_guided_kernel<DdimRule<true, P>, 0>));
        } else {
            if (seeds_dev) SISIC_GUIDED((step_guided_kernel<DdimRule<false, P>, 1>)); else SISIC_GUIDED((step_guided_kernel<DdimRule<false, P>, 0>));
        })
#undef SISIC_GUIDED
    SISIC_HIP(hipGetLastError());
    return SISIC_OK;
}

// the graph-replayed form: eps2 [2n] and x2 [2n] are the loop's own buffers, zrow the buffer-noise rows (seeds_dev NULL) or
// unused (generated noise), cond the loop's LoopCond table (w at cond[0])
int launch_step_guided_indexed(sisic_ctx* ctx, int rule, int flags, const float* eps2, float* x2, float* hist, int64_t n,
                               int64_t n_per_image, const void* state, const float* coef, const int* zrow,
                               const uint64_t* seeds_dev, const float* cond, float clip, hipStream_t s) {
    SISIC_TRY(check_rule(rule, flags));
    SISIC_REQUIRE(eps2 && x2 && state && coef && cond && (zrow || seeds_dev) && n > 0, "%s_indexed (guided): null argument", rule_name(rule));
    SISIC_REQUIRE(rule != STEP_RULE_DPMPP || hist, "dpmpp_step_indexed (guided): no history buffer");
    SISIC_REQUIRE(n_per_image > 0 && n_per_image <= NOISE_MAX_PER_IMAGE && n % n_per_image == 0,
                  "%s_indexed (guided): %lld elements are not whole images of %lld", rule_name(rule), (long long)n, (long long)n_per_image);
    ProfileScope prof(ctx, s, PK_DDPM, 24.0 * (double)n, 0.0);
    const uintptr_t al = reinterpret_cast<uintptr_t>(eps2) | reinterpret_cast<uintptr_t>(x2) | reinterpret_cast<uintptr_t>(hist);
    const int vec4 = (al & 15) == 0 && (n & 3) == 0 && (!seeds_dev || (n_per_image & 3) == 0);
    const int64_t work = vec4 ? n / 4 : n;
    const dim3 grid((unsigned)std::min<int64_t>((work + 255) / 256, 2048)), block(256);
    const LoopState* st = static_cast<const LoopState*>(state);
#define SISIC_GUIDED(K) hipLaunchKernelGGL(K, grid, block, 0, s, eps2, x2, n, n_per_image, st, coef, zrow, seeds_dev, cond, clip, vec4)
    SISIC_PRED_SWITCH(flags,
        if (rule == STEP_RULE_DPMPP) {
            if (seeds_dev) hipLaunchKernelGGL((dpm_step_guided_indexed_kernel<1, P>), grid, block, 0, s, eps2, x2, hist, n, n_per_image, st, coef, zrow, seeds_dev, cond, clip, vec4);
            else hipLaunchKernelGGL((dpm_step_guided_indexed_kernel<0, P>), grid, block, 0, s, eps2, x2, hist, n, n_per_image, st, coef, zrow, seeds_dev, cond, clip, vec4);
        } else if (rule == STEP_RULE_DDPM) {
            if (seeds_dev) SISIC_GUIDED((step_guided_indexed_kernel<DdpmRule<P>, 1>)); else SISIC_GUIDED((step_guided_indexed_kernel<DdpmRule<P>, 0>));
        } else if (flags & STEP_FLAG_CLIPPED_OUTPUT) {
            if (seeds_dev) SISIC_GUIDED((step_guided_indexed_kernel<DdimRule<true, P>, 1>)); else SISIC_GUIDED((step_guided_indexed_kernel<DdimRule<true, P>, 0>));
        } else {
            if (seeds_dev) SISIC_GUIDED((step_guided_indexed_kernel<DdimRule<false, P>, 1>)); else SISIC_GUIDED((step_guided_indexed_kernel<DdimRule<false, P>, 0>));
        })
#undef SISIC_GUIDED
    SISIC_HIP(hipGetLastError());
    return SISIC_OK;
}

// ---- classifier guidance: the same steps reading eps through ClassifierEps ----------------------------------------------------
// eps_hat = eps - k * g with k = scale * sb (Dhariwal & Nichol 2021, Alg. 2): g is the classifier's input
// gradient at the step's latent, sb entry 0 of the step's row.  k is formed in the kernel, so the eager, the indexed and the
// stand-alone form (sisic_clf_guide_eps) round it the same way.  Epsilon prediction and generated noise only.  The eager kernels
// take scale and the row as launch arguments; the indexed ones read the row by the loop's step index and scale from
// clf_tab[0] (LoopClf: {scale, -, -, -, int target[B]}), so that a captured step replays under another scale.
__device__ __forceinline__ float clf_guide_k(float scale, float sb) {
#pragma clang fp contract(off)
    return scale * sb;
}

__device__ __forceinline__ float clf_guide_one(float e, float g, float k) {
#pragma clang fp contract(off)
    const float t = k * g;
    return e - t;
}

struct ClassifierEps {
    const float* __restrict__ e;
    const float* __restrict__ g;
    float k;
    static constexpr bool dup = false;
    __device__ __forceinline__ float4 get4(int64_t i4) const {
        const float4 ev = reinterpret_cast<const float4*>(e)[i4], gv = reinterpret_cast<const float4*>(g)[i4];
        return make_float4(clf_guide_one(ev.x, gv.x, k), clf_guide_one(ev.y, gv.y, k), clf_guide_one(ev.z, gv.z, k),
                           clf_guide_one(ev.w, gv.w, k));
    }
    __device__ __forceinline__ float get1(int64_t i) const { return clf_guide_one(e[i], g[i], k); }
};

template <class R>
__global__ void __launch_bounds__(256)
step_clf_kernel(const float* __restrict__ eps, const float* __restrict__ g, float scale, const float* x,
                const uint64_t* __restrict__ seeds, int64_t n_per_image, uint32_t step, float* out, int64_t n, StepRow row,
                float clip, int vec4) {
    const PhiloxNoise zs{seeds, n_per_image, step};
    step_body(ClassifierEps{eps, g, clf_guide_k(scale, row.v[0])}, x, out, n, vec4 != 0 && zs.vec_ok(), row_rule<R>(row, clip), zs);
}

__global__ void __launch_bounds__(256)
dpm_step_clf_kernel(const float* __restrict__ eps, const float* __restrict__ g, float scale, const float* x,
                    const uint64_t* __restrict__ seeds, int64_t n_per_image, uint32_t step, float* hist, float* out, int64_t n,
                    StepRow row, float clip, int vec4) {
    const PhiloxNoise zs{seeds, n_per_image, step};
    const DpmRule<PRED_EPS> rule{row.v[0], row.v[1], row.v[2], row.v[3], row.v[4], row.v[5], clip};
    dpm_step_body(ClassifierEps{eps, g, clf_guide_k(scale, row.v[0])}, x, hist, out, n, vec4 != 0 && zs.vec_ok(), rule, zs);
}

template <class R>
__global__ void __launch_bounds__(256)
step_clf_indexed_kernel(const float* __restrict__ eps, const float* __restrict__ g, float* x, int64_t n, int64_t n_per_image,
                        const LoopState* __restrict__ st, const float* __restrict__ coef, const uint64_t* __restrict__ seeds,
                        const float* __restrict__ clf_tab, float clip, int vec4) {
    const int step = st->step;
    const PhiloxNoise zs{seeds, n_per_image, (uint32_t)(st->step_base + step)};
    const R rule = loop_rule<R>(coef, step, clip);
    step_body(ClassifierEps{eps, g, clf_guide_k(clf_tab[0], rule.sb)}, x, x, n, vec4 != 0 && zs.vec_ok(), rule, zs);
}

__global__ void __launch_bounds__(256)
dpm_step_clf_indexed_kernel(const float* __restrict__ eps, const float* __restrict__ g, float* x, float* hist, int64_t n,
                            int64_t n_per_image, const LoopState* __restrict__ st, const float* __restrict__ coef,
                            const uint64_t* __restrict__ seeds, const float* __restrict__ clf_tab, float clip, int vec4) {
    const int step = st->step;
    const PhiloxNoise zs{seeds, n_per_image, (uint32_t)(st->step_base + step)};
    const DpmRule<PRED_EPS> rule = loop_dpm_rule<PRED_EPS>(coef, step, clip);
    dpm_step_body(ClassifierEps{eps, g, clf_guide_k(clf_tab[0], rule.sb)}, x, hist, x, n, vec4 != 0 && zs.vec_ok(), rule, zs);
}

static int check_clf_step(int rule, int flags, const char* form) {
    SISIC_TRY(check_rule(rule, flags));
    SISIC_REQUIRE(step_pred(flags) == PRED_EPS, "%s (%s): prediction_type %d: classifier guidance takes epsilon-prediction models only",
                  rule_name(rule), form, step_pred(flags));
    return SISIC_OK;
}

// the eager form.  row: the rule's host row; out may be x; hist: DPM-Solver++ only
int launch_step_clf(sisic_ctx* ctx, int rule, int flags, const float* eps, const float* g, float scale, const float* x,
                    const uint64_t* seeds_dev, int64_t n_per_image, uint32_t step, float* hist, float* out, int64_t n,
                    const float* row, float clip, hipStream_t s) {
    SISIC_TRY(check_clf_step(rule, flags, "classifier-guided"));
    SISIC_REQUIRE(eps && g && x && out && seeds_dev && row && n > 0, "%s (classifier-guided): null tensor or empty", rule_name(rule));
    SISIC_REQUIRE(g != out && eps != out, "%s (classifier-guided): eps or the gradient aliases the output", rule_name(rule));
    SISIC_REQUIRE(rule != STEP_RULE_DPMPP || (hist && hist != x && hist != out && hist != eps && hist != g),
                  "dpmpp_step (classifier-guided): the history is missing or aliases another tensor");
    SISIC_REQUIRE(n_per_image > 0 && n_per_image <= NOISE_MAX_PER_IMAGE && n % n_per_image == 0,
                  "%s (classifier-guided): %lld elements are not whole images of %lld", rule_name(rule), (long long)n,
                  (long long)n_per_image);
    SISIC_TRY(check_step_row(rule, flags, row[0], row[1]));
    ProfileScope prof(ctx, s, PK_DDPM, 16.0 * (double)n, 0.0);
    StepRow r{};
    for (int k = 0; k < (int)SISIC_RULE_ROW_WIDTH(rule); ++k) r.v[k] = row[k];
    const uintptr_t al = reinterpret_cast<uintptr_t>(eps) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(x) |
                         reinterpret_cast<uintptr_t>(hist) | reinterpret_cast<uintptr_t>(out);
    const int vec4 = (al & 15) == 0 && (n_per_image & 3) == 0;
    const int64_t work = vec4 ? n / 4 : n;
    const dim3 grid((unsigned)std::min<int64_t>((work + 255) / 256, 2048)), block(256);
#define SISIC_CLF(K) hipLaunchKernelGGL(K, grid, block, 0, s, eps, g, scale, x, seeds_dev, n_per_image, step, out, n, r, clip, vec4)
    if (rule == STEP_RULE_DPMPP)
        hipLaunchKernelGGL(dpm_step_clf_kernel, grid, block, 0, s, eps, g, scale, x, seeds_dev, n_per_image, step, hist, out, n, r, clip, vec4);
    else if (rule == STEP_RULE_DDPM) SISIC_CLF((step_clf_kernel<DdpmRule<PRED_EPS>>));
    else if (flags & STEP_FLAG_CLIPPED_OUTPUT) SISIC_CLF((step_clf_kernel<DdimRule<true, PRED_EPS>>));
    else SISIC_CLF((step_clf_kernel<DdimRule<false, PRED_EPS>>));
#undef SISIC_CLF
    SISIC_HIP(hipGetLastError());
    return SISIC_OK;
}

// the graph-replayed form: eps, g and x are the loop's own buffers, clf_tab its LoopClf table (scale at clf_tab[0])
int launch_step_clf_indexed(sisic_ctx* ctx, int rule, int flags, const float* eps, const float* g, float* x, float* hist, int64_t n,
                            int64_t n_per_image, const void* state, const float* coef, const uint64_t* seeds_dev,
                            const float* clf_tab, float clip, hipStream_t s) {
    SISIC_TRY(check_clf_step(rule, flags, "classifier-guided, indexed"));
    SISIC_REQUIRE(eps && g && x && state && coef && seeds_dev && clf_tab && n > 0, "%s_indexed (classifier-guided): null argument", rule_name(rule));
    SISIC_REQUIRE(rule != STEP_RULE_DPMPP || hist, "dpmpp_step_indexed (classifier-guided): no history buffer");
    SISIC_REQUIRE(n_per_image > 0 && n_per_image <= NOISE_MAX_PER_IMAGE && n % n_per_image == 0,
                  "%s_indexed (classifier-guided): %lld elements are not whole images of %lld", rule_name(rule), (long long)n,
                  (long long)n_per_image);
    ProfileScope prof(ctx, s, PK_DDPM, 16.0 * (double)n, 0.0);
    const uintptr_t al = reinterpret_cast<uintptr_t>(eps) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(x) |
                         reinterpret_cast<uintptr_t>(hist);
    const int vec4 = (al & 15) == 0 && (n_per_image & 3) == 0;
    const int64_t work = vec4 ? n / 4 : n;
    const dim3 grid((unsigned)std::min<int64_t>((work + 255) / 256, 2048)), block(256);
    const LoopState* st = static_cast<const LoopState*>(state);
#define SISIC_CLF(K) hipLaunchKernelGGL(K, grid, block, 0, s, eps, g, x, n, n_per_image, st, coef, seeds_dev, clf_tab, clip, vec4)
    if (rule == STEP_RULE_DPMPP)
        hipLaunchKernelGGL(dpm_step_clf_indexed_kernel, grid, block, 0, s, eps, g, x, hist, n, n_per_image, st, coef, seeds_dev, clf_tab, clip, vec4);
    else if (rule == STEP_RULE_DDPM) SISIC_CLF((step_clf_indexed_kernel<DdpmRule<PRED_EPS>>));
    else if (flags & STEP_FLAG_CLIPPED_OUTPUT) SISIC_CLF((step_clf_indexed_kernel<DdimRule<true, PRED_EPS>>));
    else SISIC_CLF((step_clf_indexed_kernel<DdimRule<false, PRED_EPS>>));
#undef SISIC_CLF
    SISIC_HIP(hipGetLastError());
    return SISIC_OK;
}

// the combine alone (sisic_clf_guide_eps): clf_guide_one() on every element, any alignment; out may be eps
__global__ void __launch_bounds__(256)
clf_guide_eps_kernel(const float* eps, const float* g, float sb, float scale, float* out, int64_t n, int vec4) {
    const float k = clf_guide_k(scale, sb);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    // (plain pointers, not the restrict-qualified ClassifierEps: out may be eps; a thread reads its elements first)
    int64_t tail = t0;
    if (vec4) {
        const int64_t n4 = n >> 2;
        for (int64_t i = t0; i < n4; i += stride) {
            const float4 e = reinterpret_cast<const float4*>(eps)[i], gv = reinterpret_cast<const float4*>(g)[i];
            reinterpret_cast<float4*>(out)[i] = make_float4(clf_guide_one(e.x, gv.x, k), clf_guide_one(e.y, gv.y, k),
                                                            clf_guide_one(e.z, gv.z, k), clf_guide_one(e.w, gv.w, k));
        }
        tail = (n4 << 2) + t0;
    }
    for (int64_t i = tail; i < n; i += stride) out[i] = clf_guide_one(eps[i], g[i], k);
}

int launch_clf_guide_eps(sisic_ctx* ctx, const float* eps, const float* g, float sb, float scale, float* out, int64_t n,
                         hipStream_t s) {
    SISIC_REQUIRE(eps && g && out && n > 0, "clf_guide_eps: null tensor or empty");
    SISIC_REQUIRE(g != out, "clf_guide_eps: out aliases the gradient (out may be eps)");
    ProfileScope prof(ctx, s, PK_OTHER, 12.0 * (double)n, 0.0);
    const uintptr_t al = reinterpret_cast<uintptr_t>(eps) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(out);
    const int vec4 = (al & 15) == 0;
    const int64_t work = vec4 ? (n + 3) / 4 : n;
    hipLaunchKernelGGL(clf_guide_eps_kernel, dim3((unsigned)std::min<int64_t>((work + 255) / 256, 2048)), dim3(256), 0, s, eps, g, sb,
                       scale, out, n, vec4);
    SISIC_HIP(hipGetLastError());
    return SISIC_OK;
}

// ---- the edited steps (sisic_*_step_edit, sisic_sample_frames_edit) -------------------------------------------------------
// rule x {plain, guided} with the inpainting epilogue, generated noise only.  One kernel serves the eager and the replayed
// form: with st set, the rule's row, the edit row and the step index are read by the loop's step (and w from cond[0]);
// otherwise they are the launch's own.
struct EditStepArgs {
    const float* ec;                    // eps [n]; guided: the conditional half
    const float* eu;                    // guided: the null-label half
    const float* cond;                  // guided, replayed: LoopCond (w at cond[0])
    const float* x;
    float* out;                         // may be x; guided: [2n]
    float* hist;                        // DPM-Solver++
    const float* x0k;
    const float* mask;
    const uint64_t* seeds;
    const LoopState* st;                // replayed form, or nullptr
    const float* coef;                  // replayed form: the rule's rows ...
    const float* erows;                 // ... and the edit rows {ck, sk, ja, jb}
    int64_t n, npi, hw;
    StepRow row;
    float er[4];
    float w, clip;
    uint32_t step;
    int vec4;
};

template <int WIDTH>
__device__ __forceinline__ void edit_step_rows(const EditStepArgs& a, StepRow& row, float (&er)[4], uint32_t& step, float& w) {
    row = a.row;
    for (int k = 0; k < 4; ++k) er[k] = a.er[k];
    step = a.step;
    w = a.w;
    if (a.st) {
        const int i = a.st->step;
        step = (uint32_t)(a.st->step_base + i);
        for (int k = 0; k < WIDTH; ++k) row.v[k] = a.coef[WIDTH * i + k];
        for (int k = 0; k < 4; ++k) er[k] = a.erows[4 * i + k];
        if (a.cond) w = a.cond[0];
    }
}

template <class R, bool GUIDED>
__global__ void __launch_bounds__(256)
step_edit_kernel(const EditStepArgs a) {
    StepRow row; float er[4], w; uint32_t step;
    edit_step_rows<5>(a, row, er, step, w);
    const PhiloxNoise zs{a.seeds, a.npi, step};
    const InpaintEdit ed{a.x0k, a.mask, a.seeds, a.npi, a.hw, step, er[0], er[1], er[2], er[3]};
    if constexpr (GUIDED) step_body(GuidedEps{a.ec, a.eu, w}, a.x, a.out, a.n, a.vec4 != 0, row_rule<R>(row, a.clip), zs, ed);
    else step_body(PlainEps{a.ec}, a.x, a.out, a.n, a.vec4 != 0, row_rule<R>(row, a.clip), zs, ed);
}

template <bool GUIDED, int P>
__global__ void __launch_bounds__(256)
dpm_step_edit_kernel(const EditStepArgs a) {
    StepRow row; float er[4], w; uint32_t step;
    edit_step_rows<6>(a, row, er, step, w);
    const PhiloxNoise zs{a.seeds, a.npi, step};
    const InpaintEdit ed{a.x0k, a.mask, a.seeds, a.npi, a.hw, step, er[0], er[1], er[2], er[3]};
    const DpmRule<P> rule{row.v[0], row.v[1], row.v[2], row.v[3], row.v[4], row.v[5], a.clip};
    if constexpr (GUIDED) dpm_step_body(GuidedEps{a.ec, a.eu, w}, a.x, a.hist, a.out, a.n, a.vec4 != 0, rule, zs, ed);
    else dpm_step_body(PlainEps{a.ec}, a.x, a.hist, a.out, a.n, a.vec4 != 0, rule, zs, ed);
}

// One launcher for every edited step.  eps_u: a guided step (out is then [2n]).  state/coef_dev/erows_dev: the replayed form
// (row, erow, step and w unused; cond holds w when guided); otherwise row [rule's width] and erow [4] are host rows.
int launch_step_edit(sisic_ctx* ctx, int rule, int flags, const float* eps, const float* eps_u, float w, const float* cond,
                     const float* x, float* hist, float* out, int64_t n, int64_t n_per_image, int64_t hw,
                     const uint64_t* seeds_dev, uint32_t step, const float* row, const float* erow, const void* state,
                     const float* coef_dev, const float* erows_dev, const float* x0k, const float* mask, float clip,
                     hipStream_t s) {
    SISIC_TRY(check_rule(rule, flags));
    const char* name = rule_name(rule);
    SISIC_REQUIRE(eps && x && out && seeds_dev && x0k && mask && n > 0, "%s_edit: null tensor or empty", name);
    SISIC_REQUIRE(rule != STEP_RULE_DPMPP || (hist && hist != x && hist != out && hist != eps && hist != eps_u),
                  "dpmpp_step_edit: the history is missing or aliases another tensor");
    SISIC_REQUIRE(n_per_image > 0 && n_per_image <= NOISE_MAX_PER_IMAGE && n % n_per_image == 0,
                  "%s_edit: %lld elements are not whole images of %lld", name, (long long)n, (long long)n_per_image);
    SISIC_REQUIRE(hw > 0 && n_per_image % hw == 0, "%s_edit: an image of %lld elements is not whole channels of %lld", name,
                  (long long)n_per_image, (long long)hw);
    SISIC_REQUIRE(x0k != out && mask != out && x0k != hist && mask != hist, "%s_edit: the known image or the mask aliases an output", name);
    EditStepArgs a{};
    if (state) {
        SISIC_REQUIRE(coef_dev && erows_dev && (!eps_u || cond), "%s_edit (indexed): null table", name);
    } else {
        SISIC_REQUIRE(row && erow, "%s_edit: null row", name);
        SISIC_TRY(check_step_row(rule, flags, row[0], row[1]));
        for (int k = 0; k < (int)SISIC_RULE_ROW_WIDTH(rule); ++k) a.row.v[k] = row[k];
        for (int k = 0; k < 4; ++k) {
            SISIC_REQUIRE(std::isfinite(erow[k]), "%s_edit: edit row {%g, %g, %g, %g}", name, erow[0], erow[1], erow[2], erow[3]);
            a.er[k] = erow[k];
        }
    }
    ProfileScope prof(ctx, s, PK_DDPM, (eps_u ? 32.0 : 20.0) * (double)n, 0.0);
    const uintptr_t al = reinterpret_cast<uintptr_t>(eps) | reinterpret_cast<uintptr_t>(eps_u) | reinterpret_cast<uintptr_t>(x) |
                         reinterpret_cast<uintptr_t>(hist) | reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(x0k) |
                         reinterpret_cast<uintptr_t>(mask);
    a.ec = eps; a.eu = eps_u; a.cond = state ? cond : nullptr; a.x = x; a.out = out; a.hist = hist; a.x0k = x0k; a.mask = mask;
    a.seeds = seeds_dev; a.st = static_cast<const LoopState*>(state); a.coef = coef_dev; a.erows = erows_dev;
    a.n = n; a.npi = n_per_image; a.hw = hw; a.w = w; a.clip = clip; a.step = step;
    a.vec4 = (al & 15) == 0 && (n_per_image & 3) == 0 && (hw & 3) == 0;
    const int64_t work = a.vec4 ? n / 4 : n;
    const dim3 grid((unsigned)std::min<int64_t>((work + 255) / 256, 2048)), block(256);
#define SISIC_EDIT(K) hipLaunchKernelGGL(K, grid, block, 0, s, a)
    SISIC_PRED_SWITCH(flags,
        if (rule == STEP_RULE_DPMPP) {
            if (eps_u) SISIC_EDIT((dpm_step_edit_kernel<true, P>)); else SISIC_EDIT((dpm_step_edit_kernel<false, P>));
        } else if (rule == STEP_RULE_DDPM) {
            if (eps_u) SISIC_EDIT((step_edit_kernel<DdpmRule<P>, true>)); else SISIC_EDIT((step_edit_kernel<DdpmRule<P>, false>));
        } else if (flags & STEP_FLAG_CLIPPED_OUTPUT) {
            if (eps_u) SISIC_EDIT((step_edit_kernel<DdimRule<true, P>, true>)); else SISIC_EDIT((step_edit_kernel<DdimRule<true, P>, false>));
        } else {
            if (eps_u) SISIC_EDIT((step_edit_kernel<DdimRule<false, P>, true>)); else SISIC_EDIT((step_edit_kernel<DdimRule<false, P>, false>));
        })
#undef SISIC_EDIT
    SISIC_HIP(hipGetLastError());
    return SISIC_OK;
}

#undef SISIC_PRED_SWITCH

// the combine alone (sisic_guide_eps): guide_one() on every element, any alignment; out may be either input
__global__ void __launch_bounds__(256)
guide_eps_kernel(const float* eps_c, const float* eps_u, float w, float* out, int64_t n, int vec4) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    // (plain pointers, not the restrict-qualified GuidedEps: out may be one of the inputs; a thread reads its elements first)
    int64_t tail = t0;
    if (vec4) {
        const int64_t n4 = n >> 2;
        for (int64_t i = t0; i < n4; i += stride) {
            const float4 c = reinterpret_cast<const float4*>(eps_c)[i], u = reinterpret_cast<const float4*>(eps_u)[i];
            reinterpret_cast<float4*>(out)[i] = make_float4(guide_one(c.x, u.x, w), guide_one(c.y, u.y, w), guide_one(c.z, u.z, w),
                                                            guide_one(c.w, u.w, w));
        }
        tail = (n4 << 2) + t0;
    }
    for (int64_t i = tail; i < n; i += stride) out[i] = guide_one(eps_c[i], eps_u[i], w);
}

int launch_guide_eps(sisic_ctx* ctx, const float* eps_c, const float* eps_u, float w, float* out, int64_t n, hipStream_t s) {
    SISIC_REQUIRE(eps_c && eps_u && out && n > 0, "guide_eps: null tensor or empty");
    ProfileScope prof(ctx, s, PK_OTHER, 12.0 * (double)n, 0.0);
    const uintptr_t al = reinterpret_cast<uintptr_t>(eps_c) | reinterpret_cast<uintptr_t>(eps_u) | reinterpret_cast<uintptr_t>(out);
    const int vec4 = (al & 15) == 0;
    const int64_t work = vec4 ? (n + 3) / 4 : n;
    hipLaunchKernelGGL(guide_eps_kernel, dim3((unsigned)std::min<int64_t>((work + 255) / 256, 2048)), dim3(256), 0, s, eps_c, eps_u,
                       w, out, n, vec4);
    SISIC_HIP(hipGetLastError());
    return SISIC_OK;
}

// ---- per-sample embedding rows of a conditional loop ---------------------------------------------------------------------------
// LoopCond, the loop's device table of a conditional call, as floats: [0] w (guidance scale), [1] L (int: distinct labels of the
// call, the null one included), [2], [3] unused, [4 + b] slot of sample b (int, < L) for the B or 2B samples of a pass.
// table holds the projected embedding of (step i, slot j) in row i * L + j; sample b of the pass gets its row:
//     out[b][r] = table[(step * L + slot[b]) * R + r]
// st != NULL: the step index comes from the loop state (graph-replayed form), else from the argument.
__global__ void __launch_bounds__(256)
loop_gather_rows_kernel(const float* __restrict__ table, int R, const LoopState* __restrict__ st, int step,
                        const float* __restrict__ cond, float* __restrict__ out) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    const int b = blockIdx.y;
    if (r >= R) return;
    const int* ci = reinterpret_cast<const int*>(cond);
    const int i = st ? st->step : step;
    out[(size_t)b * R + r] = table[((size_t)i * ci[1] + ci[4 + b]) * R + r];
}

int launch_loop_gather_rows(sisic_ctx*, const float* table, int R, const void* state, int step, const float* cond, int rows,
                            float* out, hipStream_t s) {
    SISIC_REQUIRE(table && cond && out && R > 0 && rows > 0 && rows <= 65535, "loop_gather_rows: bad arguments");
    hipLaunchKernelGGL(loop_gather_rows_kernel, dim3(cdiv(R, 256), rows), dim3(256), 0, s, table, R,
                       static_cast<const LoopState*>(state), step, cond, out);
    SISIC_HIP(hipGetLastError());
    return SISIC_OK;
}

size_t loop_state_bytes() { return sizeof(LoopState); }

// ---- stand-alone noise: the blocks of noise_device.h as a buffer -----------------------------------------------------------
// For tests and for callers that want z_t (or an x_T, tag 1) in memory.  Seeds travel as a launch argument, up to
// NOISE_PACK images per launch (blockIdx.y): no device buffer to own, nothing to order between calls.
constexpr int NOISE_PACK = 64;
struct SeedPack { uint64_t s[NOISE_PACK]; };

// out: [images of this launch, n_per_image] normals
__global__ void __launch_bounds__(256)
noise_fill_kernel(float* out, int64_t n_per_image, SeedPack seeds, uint32_t step, uint32_t tag, int vec4) {
    const uint64_t seed = seeds.s[blockIdx.y];
    float* o = out + (int64_t)blockIdx.y * n_per_image;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (vec4) {
        for (int64_t q = t0; q < (n_per_image >> 2); q += stride)
            reinterpret_cast<float4*>(o)[q] = noise_normal4(seed, (uint32_t)q, step, tag);
    } else {
        for (int64_t e = t0; e < n_per_image; e += stride) o[e] = noise_normal1(seed, e, step, tag);
    }
}

// out: [images of this launch, 4 * ceil(n_per_image / 4)] raw words, whole blocks
__global__ void __launch_bounds__(256)
noise_bits_kernel(uint32_t* out, int64_t blocks_per_image, SeedPack seeds, uint32_t step, uint32_t tag) {
    const uint64_t seed = seeds.s[blockIdx.y];
    uint32_t* o = out + (int64_t)blockIdx.y * blocks_per_image * 4;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < blocks_per_image; q += stride) {
        const uint4 r = noise_bits4(seed, (uint32_t)q, step, tag);
        o[4 * q + 0] = r.x; o[4 * q + 1] = r.y; o[4 * q + 2] = r.z; o[4 * q + 3] = r.w;
    }
}

int launch_noise_fill(sisic_ctx* ctx, void* out, int B, int64_t n_per_image, const uint64_t* seeds_host, uint32_t step,
                      uint32_t tag, bool bits, hipStream_t s) {
    SISIC_REQUIRE(out && seeds_host && B > 0, "noise_fill: null argument or empty batch");
    SISIC_REQUIRE(n_per_image > 0 && n_per_image <= NOISE_MAX_PER_IMAGE, "noise_fill: n_per_image %lld (1 .. 2^34)", (long long)n_per_image);
    const int64_t blocks_per_image = (n_per_image + 3) / 4;
    const int64_t row = bits ? blocks_per_image * 4 : n_per_image;
    ProfileScope prof(ctx, s, PK_OTHER, 4.0 * (double)row * B, 0.0);
    const int vec4 = (reinterpret_cast<uintptr_t>(out) & 15) == 0 && (n_per_image & 3) == 0;
    const int64_t work = (bits || vec4) ? blocks_per_image : n_per_image;
    const int gx = (int)std::min<int64_t>((work + 255) / 256, 2048);
    for (int b0 = 0; b0 < B; b0 += NOISE_PACK) {
        const int nb = std::min(NOISE_PACK, B - b0);
        SeedPack pack = {};
        for (int k = 0; k < nb; ++k) pack.s[k] = seeds_host[b0 + k];
        if (bits)
            hipLaunchKernelGGL(noise_bits_kernel, dim3(gx, nb), dim3(256), 0, s, static_cast<uint32_t*>(out) + (int64_t)b0 * row,
                               blocks_per_image, pack, step, tag);
        else
            hipLaunchKernelGGL(noise_fill_kernel, dim3(gx, nb), dim3(256), 0, s, static_cast<float*>(out) + (int64_t)b0 * row,
                               n_per_image, pack, step, tag, vec4);
        SISIC_HIP(hipGetLastError());
    }
    return SISIC_OK;
}

// ---- de-normalise to uint8 HWC ---------------------------------------------------------------
// FORM 0: image_generator.py:441-447     clamp((x + 1) / 2, 0, 1) * 255, truncated
// FORM 1: generate_test.py:94-97          (clamp(x, -1, 1) + 1) * 0.5 * 255, truncated   (bit-equal to form 0)
// FORM 2: diffusion_generator.py:231-232  clip((x + 1) * 127.5, 0, 255), truncated      (rounds differently: one
//         multiplication by 127.5 instead of a halving and a multiplication by 255)
// fp32 operation order of the respective torch / numpy expressions; this file is compiled without FMA contraction.
template <int FORM>
__global__ void __launch_bounds__(256)
denorm_u8_kernel(const float* __restrict__ x, uint8_t* __restrict__ out, int C, int HW, int64_t total) {
    // one thread per output byte: index = (b*HW + p)*C + c
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        const int64_t bp = i / C;
        const int p = (int)(bp % HW);
        const int64_t b = bp / HW;
        float v = x[(b * C + c) * HW + p];
        if constexpr (FORM == 0) {
            v = (v + 1.0f) / 2.0f;
            v = fminf(fmaxf(v, 0.0f), 1.0f);
            v = v * 255.0f;
        } else if constexpr (FORM == 1) {
            v = fminf(fmaxf(v, -1.0f), 1.0f);
            v = (v + 1.0f) * 0.5f;
            v = v * 255.0f;
        } else {
            v = (v + 1.0f) * 127.5f;
            v = fminf(fmaxf(v, 0.0f), 255.0f);
        }
        out[i] = (uint8_t)(int)v;
    }
}

int launch_denorm_u8(sisic_ctx* ctx, const float* x, uint8_t* out, int B, int C, int H, int W, hipStream_t s, int form) {
    SISIC_REQUIRE(x && out && B > 0 && C > 0 && H > 0 && W > 0, "denorm_u8: bad arguments");
    SISIC_REQUIRE(form >= 0 && form <= 2, "denorm_u8: form %d (0 = image_generator, 1 = generate_test, 2 = diffusion_generator)", form);
    const int64_t total = (int64_t)B * C * H * W;
    ProfileScope prof(ctx, s, PK_OTHER, 5.0 * (double)total, 0.0);
    const int blocks = (int)std::min<int64_t>((total + 255) / 256, 2048);
    if (form == 0) hipLaunchKernelGGL(denorm_u8_kernel<0>, dim3(blocks), dim3(256), 0, s, x, out, C, H * W, total);
    else if (form == 1) hipLaunchKernelGGL(denorm_u8_kernel<1>, dim3(blocks), dim3(256), 0, s, x, out, C, H * W, total);
    else hipLaunchKernelGGL(denorm_u8_kernel<2>, dim3(blocks), dim3(256), 0, s, x, out, C, H * W, total);
    SISIC_HIP(hipGetLastError());
    return SISIC_OK;
}

// ---- time embedding -----------------------------------------------------------------------------
__device__ __forceinline__ float silu_acc(float v) { return v / (1.0f + expf(-v)); }

// one workgroup per sample; hidden <= 1024; weights stored transposed [in][hidden]
// class_table / labels (both or neither): row labels[b] of the class embedding [N, hidden] is added to linear_2's output, one
// fp32 add, before the SiLU (UNet2DModel: emb = time_embedding(t_emb) + class_embedding(class_labels)); save_t2 keeps the sum
__global__ void __launch_bounds__(256)
temb_mlp_kernel(const float* __restrict__ t_vals, const float* __restrict__ freqs, int n_freqs,
                const float* __restrict__ w1t, const float* __restrict__ b1, const float* __restrict__ w2t,
                const float* __restrict__ b2, int hidden, float* __restrict__ temb_act, float* __restrict__ save_emb,
                float* __restrict__ save_h1, float* __restrict__ save_t2, const float* __restrict__ class_table,
                const int* __restrict__ labels) {
    __shared__ float e[256];
    __shared__ float h[1024];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float t = t_vals[b];
    const int nin = 2 * n_freqs;
    const float* crow = class_table ? class_table + (size_t)labels[b] * hidden : nullptr;
    for (int k = tid; k < nin; k += blockDim.x) {
        const float arg = t * freqs[k % n_freqs];
        e[k] = (k < n_freqs) ? cosf(arg) : sinf(arg);   // flip_sin_to_cos=True: cos half first
        if (save_emb) save_emb[(size_t)b * nin + k] = e[k];
    }
    __syncthreads();
    for (int j = tid; j < hidden; j += blockDim.x) {
        float acc = 0.0f;
        for (int k = 0; k < nin; ++k) acc += w1t[(size_t)k * hidden + j] * e[k];
        h[j] = silu_acc(acc + b1[j]);
        if (save_h1) save_h1[(size_t)b * hidden + j] = acc + b1[j];
    }
    __syncthreads();
    for (int j = tid; j < hidden; j += blockDim.x) {
        float acc = 0.0f;
        for (int k = 0; k < hidden; ++k) acc += w2t[(size_t)k * hidden + j] * h[k];
        float t2 = acc + b2[j];
        if (crow) t2 = t2 + crow[j];
        temb_act[(size_t)b * hidden + j] = silu_acc(t2);
        if (save_t2) save_t2[(size_t)b * hidden + j] = t2;
    }
}

int launch_temb_mlp(sisic_ctx* ctx, const float* t_vals, int B, const float* freqs, int n_freqs, const float* w1t,
                    const float* b1, const float* w2t, const float* b2, int hidden, float* temb_act, hipStream_t s,
                    float* save_emb, float* save_h1, float* save_t2, const float* class_table, const int* labels) {
    SISIC_REQUIRE(n_freqs > 0 && 2 * n_freqs <= 256 && hidden > 0 && hidden <= 1024, "temb_mlp: sizes unsupported");
    SISIC_REQUIRE((class_table == nullptr) == (labels == nullptr), "temb_mlp: a class table goes with labels");
    ProfileScope prof(ctx, s, PK_OTHER, 0.0, 0.0);
    hipLaunchKernelGGL(temb_mlp_kernel, dim3(B), dim3(256), 0, s, t_vals, freqs, n_freqs, w1t, b1, w2t, b2, hidden,
                       temb_act, save_emb, save_h1, save_t2, class_table, labels);
    SISIC_HIP(hipGetLastError());
    return SISIC_OK;
}

// out[b, r] = bias[r] + sum_k wt[k][r] * x[b][k]
__global__ void __launch_bounds__(256)
linear_t_kernel(const float* __restrict__ x, int K, const float* __restrict__ wt, const float* __restrict__ bias,
                int R, float* __restrict__ out) {
    __shared__ float xs[1024];
    const int b = blockIdx.y;
    for (int k = threadIdx.x; k < K; k += blockDim.x) xs[k] = x[(size_t)b * K + k];
    __syncthreads();
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < R) {
        float acc = 0.0f;
        for (int k = 0; k < K; ++k) acc += wt[(size_t)k * R + r] * xs[k];
        out[(size_t)b * R + r] = acc + (bias ? bias[r] : 0.0f);
    }
}

int launch_linear_t(sisic_ctx* ctx, const float* x, int B, int K, const float* wt, const float* bias, int R,
                    float* out, hipStream_t s) {
    SISIC_REQUIRE(K > 0 && K <= 1024 && R > 0 && B > 0, "linear_t: sizes unsupported");
    ProfileScope prof(ctx, s, PK_OTHER, 0.0, 0.0);
    hipLaunchKernelGGL(linear_t_kernel, dim3(cdiv(R, 256), B), dim3(256), 0, s, x, K, wt, bias, R, out);
    SISIC_HIP(hipGetLastError());
    return SISIC_OK;
}

// out[c * out_ld + out_col0 + r] = in[r * cols + c]
__global__ void transpose2d_kernel(const float* __restrict__ in, int rows, int cols, float* __restrict__ out,
                                   int out_ld, int out_col0) {
    const int64_t total = (int64_t)rows * cols;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        transpose2d_elem((size_t)i, in, cols, out, out_ld, out_col0);
    }
}

int launch_transpose2d(sisic_ctx*, const float* in, int rows, int cols, float* out, int out_ld, int out_col0,
                       hipStream_t s) {
    const int64_t total = (int64_t)rows * cols;
    const int blocks = (int)std::min<int64_t>((total + 255) / 256, 1024);
    hipLaunchKernelGGL(transpose2d_kernel, dim3(blocks), dim3(256), 0, s, in, rows, cols, out, out_ld, out_col0);
    SISIC_HIP(hipGetLastError());
    return SISIC_OK;
}

}  // namespace sisic
