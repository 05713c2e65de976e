// elementwise.hip -- the HBM-bound and tiny kernels of the sampling loop:
//   * step_kernel<Rule, Eps, Noise, Edit>: every scheduler step, eager and graph-replayed, bit-exact vs torch CPU
//       Rule : DdpmRule      fused DDPMScheduler.step
//              DdimRule      fused DDIMScheduler.step, with or without use_clipped_model_output
//              DpmRule       fused DPM-Solver++(2M) step with its one-step history
//              (each under a prediction type -- epsilon, sample, v: sisic.h SISIC_PRED_*, a template parameter of the rule)
//       Eps  : PlainEps, GuidedEps (classifier-free guidance), ClassifierEps (classifier guidance)
//       Noise: BufferNoise (the caller's z), PhiloxNoise (generated in the kernel)
//       Edit : NoEdit, InpaintEdit (the RePaint epilogue applied before the store)
//     launch_step(StepLaunch) is the one way in: its table holds the 76 instantiations a caller can reach
//   * denorm_u8_kernel  : clamp((x+1)/2,0,1)*255 -> uint8 HWC (image_generator.py:441-447)
//   * temb_mlp_kernel   : sinusoidal timestep embedding -> Linear -> SiLU -> Linear -> SiLU
//   * linear_t_kernel   : every ResnetBlock2D.time_emb_proj in one launch
//   * transpose2d_kernel: weight re-layout at load time
#include "common.h"
#include "noise_device.h"
#include "pack_device.h"
#include "poison_switch.h"
#include <type_traits>

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

// The clamp of x0.  THR = false: the static range `clip` (0: none).  THR = true, dynamic thresholding (Saharia et al. 2022;
// DESIGN.md section 2): clip is the image's s from x0_quantile_kernel below, and x0 becomes clamp(x0, -s, s) / s.  s = 1 divides
// by one: the bits of the static clip = 1.  A NaN s passes the clamp and poisons the quotient, as torch.clamp's NaN does.
template <bool THR>
__device__ __forceinline__ float clamp_x0(float x0, float clip) {
#pragma clang fp contract(off)
    if constexpr (THR) {
        return fminf(fmaxf(x0, -clip), clip) / clip;
    } else {
        if (clip > 0.0f) x0 = fminf(fmaxf(x0, -clip), clip);
        return x0;
    }
}

template <int P, bool THR>
__device__ __forceinline__ float ddpm_one(float e, float x, float z, float sb, float sa, float c0, float c1,
                                          float sigma, float clip, bool noise) {
#pragma clang fp contract(off)
    float x0 = clamp_x0<THR>(pred_x0<P>(e, x, sb, sa), clip);
    float r = c0 * x0 + c1 * x;
    if (noise) r = r + sigma * z;
    return r;
}

// ---- DDIM step -------------------------------------------------------------------------
// The published DDIMScheduler.step for epsilon prediction, under the same rounding rules as ddpm_one.  The row of a step is
// {sb = (1-abar_t)^.5, sa = abar_t^.5, c_prev = abar_prev^.5, c_dir = (1 - abar_prev - sigma^2)^.5, sigma = eta * variance^.5}.
// CLIPPED (use_clipped_model_output): the direction term uses the epsilon re-derived from the clamped x0.
// The direction term's epsilon under the other types: sample (x - sa*x0)/sb with the UNCLAMPED x0; v sa*e + sb*x.
template <bool CLIPPED, int P, bool THR>
__device__ __forceinline__ float ddim_one(float e, float x, float z, float sb, float sa, float c_prev, float c_dir,
                                          float sigma, float clip, bool noise) {
#pragma clang fp contract(off)
    const float x0u = pred_x0<P>(e, x, sb, sa);
    const float x0 = clamp_x0<THR>(x0u, clip);
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
template <int P = PRED_EPS, bool THR = false>
struct DdpmRule {
    float sb, sa, c0, c1, sigma, clip;
    __device__ __forceinline__ float operator()(float e, float x, float z, bool noise) const {
        return ddpm_one<P, THR>(e, x, z, sb, sa, c0, c1, sigma, clip, noise);
    }
};

template <bool CLIPPED, int P = PRED_EPS, bool THR = false>
struct DdimRule {
    float sb, sa, c_prev, c_dir, sigma, clip;
    __device__ __forceinline__ float operator()(float e, float x, float z, bool noise) const {
        return ddim_one<CLIPPED, P, THR>(e, x, z, sb, sa, c_prev, c_dir, sigma, clip, noise);
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

// Where the clamp's range comes from: the rule's own scalar, or (dynamic thresholding) the image's s, which replaces the scalar
// element by element.  (of4: npi is a multiple of 4 on the vector path, so float4 i4 lies in one image)
struct ScalarClip {
    static constexpr bool on = false;
};

struct ImageThreshold {
    static constexpr bool on = true;
    const float* __restrict__ s;        // [n / npi]
    int64_t npi;
    __device__ __forceinline__ float of4(int64_t i4) const { return s[i4 / (npi >> 2)]; }
    __device__ __forceinline__ float of1(int64_t i) const { return s[i / npi]; }
};

// out may alias x (the loop steps in place): every element is read before it is written, by the thread that writes it
// (E::dup: vec4 only with n a multiple of 4, so that out + n is aligned like out)
template <class R, class Z, class E, class D = NoEdit, class C = ScalarClip>
__device__ __forceinline__ void step_body(const E es, const float* x, float* out, int64_t n, bool vec4,
                                          const R rule0, const Z zs, const D ed = D{}, const C cs = C{}) {
    R rule = rule0;
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
            if constexpr (C::on) rule.clip = cs.of4(i);
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
            if constexpr (C::on) rule.clip = cs.of1(i);
            float r = rule(es.get1(i), x[i], noise ? zs.get1(i) : 0.f, noise);
            if constexpr (D::on) r = ed.apply1(i, r);
            out[i] = r;
            if constexpr (E::dup) out[n + i] = r;
        }
    } else {
        for (int64_t i = t0; i < n; i += stride) {
            if constexpr (C::on) rule.clip = cs.of1(i);
            float r = rule(es.get1(i), x[i], noise ? zs.get1(i) : 0.f, noise);
            if constexpr (D::on) r = ed.apply1(i, r);
            out[i] = r;
            if constexpr (E::dup) out[n + i] = r;
        }
    }
}

// ---- DPM-Solver++(2M) step -------------------------------------------------------------
// The second-order multistep rule of Lu et al. 2022 for epsilon prediction, with its coefficients folded on the host: the row
// of a step is {sb = sigma_t, sa = alpha_t, cx, k0, sigma, k1} (sisic.h SISIC_RULE_DPMPP) and the step
//   x0 = clamp((x - sb*e)/sa);  out = cx*x + k0*x0 [+ k1*hist] [+ sigma*z];  hist = x0
// under the rounding rules of ddpm_one.  hist is the previous step's x0: one more stream, read (second-order steps only) and
// written in place by the thread that owns the element, so a captured step replays as it is.  A first-order step (k1 == 0,
// uniform over the launch) does not read it: whatever an earlier run left there, NaN included, stays out of the result.
template <int P = PRED_EPS, bool THR = false>
struct DpmRule {
    float sb, sa, cx, k0, sigma, k1, clip;
    // h: the history's element (any value when !second); m0: this step's x0, the next step's history
    __device__ __forceinline__ float operator()(float e, float x, float z, float h, bool noise, bool second, float& m0) const {
#pragma clang fp contract(off)
        const float x0 = clamp_x0<THR>(pred_x0<P>(e, x, sb, sa), clip);
        float r = cx * x + k0 * x0;
        if (second) r = r + k1 * h;
        if (noise) r = r + sigma * z;
        m0 = x0;
        return r;
    }
};

// step_body with the history stream.  out may alias x; hist aliases nothing else (and stays n wide under E::dup).
template <class R, class Z, class E, class D = NoEdit, class C = ScalarClip>
__device__ __forceinline__ void dpm_step_body(const E es, const float* x, float* hist, float* out, int64_t n,
                                              bool vec4, const R rule0, const Z zs, const D ed = D{}, const C cs = C{}) {
    R rule = rule0;
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
            if constexpr (C::on) rule.clip = cs.of4(i);
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
        if constexpr (C::on) rule.clip = cs.of1(i);
        float r = rule(es.get1(i), x[i], noise ? zs.get1(i) : 0.f, second ? hist[i] : 0.f, noise, second, m);
        if constexpr (D::on) r = ed.apply1(i, r);
        hist[i] = m;
        out[i] = r;
        if constexpr (E::dup) out[n + i] = r;
    }
}

// ---- the state of the graph-replayed sampling loop ---------------------------------------------------------------------
// One captured step is replayed for every step of the loop, so nothing that changes from step to step may be a launch
// argument: the loop keeps {step index, noise base pointer} and its per-step tables (coefficients, noise row of the step
// or -1) in device memory; the step kernel selects its row, loop_advance_kernel moves the index on.  Nothing that changes from
// call to call either: a generated-noise call's first step index is `step_base`, and its seeds lie in a library-owned
// buffer whose address is part of the captured launch.  The rule and its flag choose the kernel, so they are part of what a
// captured step is (LoopKey).
struct LoopState {
    int step;
    int step_base;            // generated noise: the Philox step index is step_base + step (0 in buffer-noise calls)
    const float* noise;       // base of the [n_noise, n] noise rows of this call
};

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

// ---- classifier guidance: the same steps reading eps through ClassifierEps ----------------------------------------------------
// eps_hat = eps - k * g with k = scale * sb (Dhariwal & Nichol 2021, Alg. 2): g is the classifier's input
// gradient at the step's latent, sb entry 0 of the step's row.  k is formed in the kernel, so the eager, the indexed and the
// stand-alone form (sisic_clf_guide_eps) round it the same way.  Epsilon prediction and generated noise only.  An eager step
// takes scale and the row as launch arguments; a replayed one reads the row by the loop's step index and scale from entry 0
// of the loop's table (LoopClf: {scale, -, -, -, int target[B]}), so that a captured step replays under another scale.
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

// ---- the step kernel: one template over {rule, eps source, noise source, edit}, one argument block ---------------------------
// Every step of the library is step_kernel<R, EPS, NZ, EDIT>(StepArgs).  With st set (the replayed form) the rule's row, the
// edit row, the step index, w and the noise row are read by the loop's step, one wave-uniform branch at entry; otherwise they
// are the launch's own.  A feature of the step is a policy struct above and a row of the table below.
struct StepRow { float v[6]; };     // a rule's row: {sb, sa, c2, c3, sigma} or DPM-Solver++'s six

// what the kernel has to know of a rule beside its arithmetic
template <class R> struct RuleTraits { static constexpr int width = 5; static constexpr bool history = false; };
template <int P, bool THR> struct RuleTraits<DpmRule<P, THR>> { static constexpr int width = 6; static constexpr bool history = true; };

struct StepArgs {
    const float* eps;                   // eps [n]; GuidedEps: the conditional half
    const float* eps2;                  // GuidedEps: the null-label half; ClassifierEps: the gradient g
    const float* x;
    float* out;                         // may be x; GuidedEps: [2n]
    float* hist;                        // rules with a history
    const float* z;                     // BufferNoise, eager: this step's row, or nullptr
    const uint64_t* seeds;              // PhiloxNoise, InpaintEdit: [n / npi] device
    const float* x0k;                   // InpaintEdit
    const float* mask;
    const LoopState* st;                // replayed form, or nullptr
    const float* coef;                  // replayed form: the rule's rows ...
    const int* zrow;                    // ... BufferNoise: the noise row of each step, or -1 ...
    const float* erows;                 // ... InpaintEdit: the edit rows {ck, sk, ja, jb} ...
    const float* wtab;                  // ... and the table whose entry 0 is w (LoopCond) or the classifier scale (LoopClf)
    int64_t n, npi, hw;
    StepRow row;
    float er[4];
    float w, clip;
    uint32_t step;
    int vec4;
    const float* thr;                   // ImageThreshold: s [n / npi], written by x0_quantile_kernel ahead of this launch
};

template <class R, class EPS, class NZ, class EDIT, class CLIP = ScalarClip>
__global__ void __launch_bounds__(256)
step_kernel(const StepArgs a) {
    constexpr int WIDTH = RuleTraits<R>::width;
    StepRow row = a.row;
    float er[4] = {a.er[0], a.er[1], a.er[2], a.er[3]};
    uint32_t step = a.step;
    float w = a.w;
    const float* z = a.z;
    if (a.st) {
        const int i = a.st->step;
        step = (uint32_t)(a.st->step_base + i);
        for (int k = 0; k < WIDTH; ++k) row.v[k] = a.coef[WIDTH * i + k];
        if constexpr (EDIT::on)
            for (int k = 0; k < 4; ++k) er[k] = a.erows[4 * i + k];
        if constexpr (!std::is_same_v<EPS, PlainEps>) w = a.wtab[0];
        if constexpr (std::is_same_v<NZ, BufferNoise>) {
            const int zr = a.zrow[i];
            z = zr >= 0 ? a.st->noise + (int64_t)zr * a.n : nullptr;
        }
    }
    const auto es = [&] {
        if constexpr (std::is_same_v<EPS, GuidedEps>) return GuidedEps{a.eps, a.eps2, w};
        else if constexpr (std::is_same_v<EPS, ClassifierEps>) return ClassifierEps{a.eps, a.eps2, clf_guide_k(w, row.v[0])};
        else return PlainEps{a.eps};
    }();
    const auto zs = [&] {
        if constexpr (std::is_same_v<NZ, BufferNoise>) return BufferNoise{z};
        else return PhiloxNoise{a.seeds, a.npi, step};
    }();
    const auto ed = [&] {
        if constexpr (EDIT::on) return InpaintEdit{a.x0k, a.mask, a.seeds, a.npi, a.hw, step, er[0], er[1], er[2], er[3]};
        else return NoEdit{};
    }();
    const auto cs = [&] {
        if constexpr (CLIP::on) return ImageThreshold{a.thr, a.npi};
        else return ScalarClip{};
    }();
    // (a noise row chosen on the device is only known here: the launcher's vec4 covers every pointer it could see)
    const bool vec4 = a.vec4 != 0 && zs.vec_ok();
    if constexpr (RuleTraits<R>::history)
        dpm_step_body(es, a.x, a.hist, a.out, a.n, vec4, R{row.v[0], row.v[1], row.v[2], row.v[3], row.v[4], row.v[5], a.clip}, zs, ed, cs);
    else
        step_body(es, a.x, a.out, a.n, vec4, R{row.v[0], row.v[1], row.v[2], row.v[3], row.v[4], a.clip}, zs, ed, cs);
}

// The instantiations a caller can reach: every rule and prediction type in six forms, and classifier guidance under epsilon
// prediction.  The template arguments are a kernel's name in a trace.
using StepKernel = void (*)(StepArgs);
enum StepForm { FORM_BUFFER, FORM_DEVICE, FORM_GUIDED_BUFFER, FORM_GUIDED_DEVICE, FORM_EDIT, FORM_GUIDED_EDIT, FORM_CLF, STEP_FORMS };

template <class R, int P, class C>
static constexpr StepKernel clf_form() {
    if constexpr (P == PRED_EPS) return step_kernel<R, ClassifierEps, PhiloxNoise, NoEdit, C>;
    else return nullptr;
}

template <class R, int P, class C = ScalarClip>
struct StepFormsOf {
    static constexpr StepKernel k[STEP_FORMS] = {
        step_kernel<R, PlainEps, BufferNoise, NoEdit, C>,      step_kernel<R, PlainEps, PhiloxNoise, NoEdit, C>,
        step_kernel<R, GuidedEps, BufferNoise, NoEdit, C>,     step_kernel<R, GuidedEps, PhiloxNoise, NoEdit, C>,
        step_kernel<R, PlainEps, PhiloxNoise, InpaintEdit, C>, step_kernel<R, GuidedEps, PhiloxNoise, InpaintEdit, C>,
        clf_form<R, P, C>()};
};

// rows: DDPM, DDIM, DDIM with use_clipped_model_output, DPM-Solver++; the same four again under dynamic thresholding
template <int P>
static StepKernel step_kernel_of(int rule, bool clipped, int form, bool thr) {
    using T = ImageThreshold;
    const StepKernel* rows[8] = {StepFormsOf<DdpmRule<P>, P>::k, StepFormsOf<DdimRule<false, P>, P>::k,
                                 StepFormsOf<DdimRule<true, P>, P>::k, StepFormsOf<DpmRule<P>, P>::k,
                                 StepFormsOf<DdpmRule<P, true>, P, T>::k, StepFormsOf<DdimRule<false, P, true>, P, T>::k,
                                 StepFormsOf<DdimRule<true, P, true>, P, T>::k, StepFormsOf<DpmRule<P, true>, P, T>::k};
    return rows[(thr ? 4 : 0) + (rule == STEP_RULE_DPMPP ? 3 : rule == STEP_RULE_DDIM ? 1 + (clipped ? 1 : 0) : 0)][form];
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

int check_step_row(int rule, int flags, float sb, float sa) {
    SISIC_TRY(check_rule(rule, flags));
    SISIC_REQUIRE(sa != 0.0f, "%s: sqrt_alpha_prod is zero", rule_name(rule));
    SISIC_REQUIRE(!(flags & STEP_FLAG_CLIPPED_OUTPUT) || sb != 0.0f,
                  "%s: sqrt_beta_prod is zero with use_clipped_model_output", rule_name(rule));
    SISIC_REQUIRE(!(rule == STEP_RULE_DDIM && step_pred(flags) == PRED_SAMPLE) || sb != 0.0f,
                  "%s: sqrt_beta_prod is zero under sample prediction (the direction term divides by it)", rule_name(rule));
    return SISIC_OK;
}

// counter word 0 of a block is its index in the image: 32 bits
static constexpr int64_t NOISE_MAX_PER_IMAGE = (int64_t)1 << 34;

// ---- dynamic thresholding: the image's s ---------------------------------------------------------------
// s[b] = clamp(quantile(|x0| of image b, ratio), 1, max) with torch.quantile's linear interpolation, spelled out (sisic.h,
// sisic_x0_threshold): with a_0 <= ... <= a_{n-1} the image's |x0|, r = ratio * (n - 1) in fp32, lo = floor(r), hi = ceil(r),
// w = r - lo, d = a_hi - a_lo:  q = w < 0.5 ? fma(w, d, a_lo) : fma(w - 1, d, a_hi) -- ONE rounding, torch's lerp.
// One workgroup owns one image.  The keys are the bit patterns of |x0| (non-negative floats order as their bits do): an image
// of up to 49152 elements on the vector path keeps them in registers, 48 a thread, formed once from loads issued together; any
// other forms them again from (eps, x) on every pass.  Radix select from the top, 8 bits per pass over the 31 key bits, an integer histogram in
// LDS.  The last pass leaves a_lo and the count of keys <= a_lo; a_hi is a_lo where that count reaches lo + 2 (or hi == lo),
// else the smallest key above a_lo, one more pass.  Everything before the float formula is integer counting: two calls give
// equal bits whatever order the waves arrive in.  A key above 0x7f800000 (a NaN) makes s NaN, as torch does.
constexpr int QUANT_THREADS = 1024;
constexpr int QUANT_CACHE = 48;                                    // keys a thread keeps in registers (12 float4)
constexpr int64_t QUANT_CACHE_MAX = (int64_t)QUANT_CACHE * QUANT_THREADS;
constexpr uint32_t QUANT_NO_KEY = 0xffffffffu;                     // a register slot behind the image's end: above every key
constexpr int64_t THRESHOLD_MAX_PER_IMAGE = (int64_t)1 << 24;      // n - 1 is exact in fp32

struct QuantArgs {
    const float* eps;                   // as StepArgs: eps, the second stream of a guided or classifier source, x
    const float* eps2;
    const float* x;
    const LoopState* st;                // replayed form: (sb, sa) from row st->step of coef, w from wtab[0]
    const float* coef;
    const float* wtab;
    float* s;                           // [images]
    int64_t npi;
    float sb, sa, w;
    float wq, maxv;                     // the interpolation weight r - lo; sample_max_value
    uint32_t lo, hi;
    int width;                          // floats per row of coef
    int vec4;
};

// The histogram of a pass: 256 bins in QUANT_COPIES interleaved copies, a lane counting in copy (lane % QUANT_COPIES).  Pass 0 sees
// the exponent byte, a handful of values: the copies lie in different banks and cut the lanes that meet on one address by that
// factor.  (Counting a wave's equal digits with ballots first, one atomic per distinct digit, was measured at 98 us for one
// image of 49152 against this form's time in profiles/r34/threshold.txt: the loop over the distinct digits costs more than
// the conflicts it saves.)
constexpr int QUANT_COPIES = 8;

template <int P, class EPS, bool CACHED>
__global__ void __launch_bounds__(QUANT_THREADS)
x0_quantile_kernel(const QuantArgs a) {
    __shared__ uint32_t hist[256 * QUANT_COPIES];
    __shared__ uint32_t bins[256];      // the copies summed
    __shared__ uint32_t sel[4];         // {prefix, rank inside the prefix, keys in the chosen bin, successor}
    __shared__ int has_nan;
    float sb = a.sb, sa = a.sa, w = a.w;
    if (a.st) {
        const int i = a.st->step;
        sb = a.coef[a.width * i];
        sa = a.coef[a.width * i + 1];
        if constexpr (!std::is_same_v<EPS, PlainEps>) w = a.wtab[0];
    }
    const auto es = [&] {
        if constexpr (std::is_same_v<EPS, GuidedEps>) return GuidedEps{a.eps, a.eps2, w};
        else if constexpr (std::is_same_v<EPS, ClassifierEps>) return ClassifierEps{a.eps, a.eps2, clf_guide_k(w, sb)};
        else return PlainEps{a.eps};
    }();
    const int tid = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * a.npi;
    const bool vec4 = a.vec4 != 0;
    // f(key, valid) on every key of the image, every thread making the same number of trips
    const int64_t items = vec4 ? a.npi >> 2 : a.npi;
    auto key_of = [&](float e, float x) -> uint32_t { return __float_as_uint(pred_x0<P>(e, x, sb, sa)) & 0x7fffffffu; };
    // CACHED: the loads of the image in one basic block (an index behind the end reads the last item and keeps no key), so
    // that they are in flight together; the passes then run on registers
    uint32_t kc[CACHED ? QUANT_CACHE : 1];
    if constexpr (CACHED) {
        // (the launcher chooses CACHED for the vector path only.)  Two batches of six float4 per stream: the loads of a batch
        // first, then its keys, each pinned to a register so that the passes keep 48 keys and not the values they came from
        constexpr int HALF = QUANT_CACHE / 8;
        auto pin = [](uint32_t k) -> uint32_t { asm volatile("" : "+v"(k)); return k; };
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            float4 e[HALF], xv[HALF];
#pragma unroll
            for (int v = 0; v < HALF; ++v) {
                const int64_t j = (int64_t)(h * HALF + v) * QUANT_THREADS + tid, jc = j < items ? j : items - 1;
                e[v] = es.get4((base >> 2) + jc);
                xv[v] = reinterpret_cast<const float4*>(a.x)[(base >> 2) + jc];
            }
#pragma unroll
            for (int v = 0; v < HALF; ++v) {
                const int u = h * HALF + v;
                const bool valid = (int64_t)u * QUANT_THREADS + tid < items;
                kc[4 * u + 0] = pin(valid ? key_of(e[v].x, xv[v].x) : QUANT_NO_KEY);
                kc[4 * u + 1] = pin(valid ? key_of(e[v].y, xv[v].y) : QUANT_NO_KEY);
                kc[4 * u + 2] = pin(valid ? key_of(e[v].z, xv[v].z) : QUANT_NO_KEY);
                kc[4 * u + 3] = pin(valid ? key_of(e[v].w, xv[v].w) : QUANT_NO_KEY);
            }
        }
    }
    // (slot u holds a key of item u / 4; whole rounds behind the image's end are skipped)
    auto for_keys = [&](auto&& f) {
        if constexpr (CACHED) {
#pragma unroll
            for (int u = 0; u < QUANT_CACHE; ++u) {
                if ((int64_t)(u / 4) * QUANT_THREADS >= items) break;
                f(kc[u], kc[u] != QUANT_NO_KEY);
            }
            return;
        }
        for (int64_t j0 = 0; j0 < items; j0 += QUANT_THREADS) {
            const int64_t j = j0 + tid;
            const bool valid = j < items;
            if (vec4) {
                float4 e = make_float4(0.f, 0.f, 0.f, 0.f), xv = e;
                if (valid) {
                    e = es.get4((base >> 2) + j);
                    xv = reinterpret_cast<const float4*>(a.x)[(base >> 2) + j];
                }
                f(key_of(e.x, xv.x), valid);
                f(key_of(e.y, xv.y), valid);
                f(key_of(e.z, xv.z), valid);
                f(key_of(e.w, xv.w), valid);
            } else {
                float e = 0.f, xv = 0.f;
                if (valid) {
                    e = es.get1(base + j);
                    xv = a.x[base + j];
                }
                f(key_of(e, xv), valid);
            }
        }
    };
    for (int k = tid; k < 256 * QUANT_COPIES; k += QUANT_THREADS) hist[k] = 0u;
    if (tid == 0) { sel[0] = 0u; sel[1] = a.lo; sel[2] = 0u; sel[3] = 0xffffffffu; has_nan = 0; }
    __syncthreads();
    uint32_t prefix = 0u;
    for (int pass = 0; pass < 4; ++pass) {
        const int sh = pass == 3 ? 0 : 23 - 8 * pass, top = pass == 3 ? 7 : sh + 8;
        const uint32_t dmask = pass == 3 ? 0x7fu : 0xffu;
        const uint32_t copy = tid & (QUANT_COPIES - 1);
        if (pass == 0) {
            for_keys([&](uint32_t key, bool valid) {
                if (valid && key > 0x7f800000u) has_nan = 1;
                if (valid) atomicAdd(&hist[(key >> 23) * QUANT_COPIES + copy], 1u);
            });
        } else {
            for_keys([&](uint32_t key, bool valid) {
                if (valid && (key >> top) == (prefix >> top)) atomicAdd(&hist[((key >> sh) & dmask) * QUANT_COPIES + copy], 1u);
            });
        }
        __syncthreads();
        if (tid < 256) {
            uint32_t c = 0u;
            for (int r = 0; r < QUANT_COPIES; ++r) {
                c += hist[tid * QUANT_COPIES + r];
                hist[tid * QUANT_COPIES + r] = 0u;      // (for the next pass: counting resumes two barriers on)
            }
            bins[tid] = c;
        }
        __syncthreads();
        if (tid < 64) {
            const uint32_t k = sel[1];
            const uint32_t c0 = bins[4 * tid], c1 = bins[4 * tid + 1], c2 = bins[4 * tid + 2], c3 = bins[4 * tid + 3];
            const uint32_t c = c0 + c1 + c2 + c3;
            uint32_t incl = c;
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t v = (uint32_t)__shfl_up((int)incl, o);
                if (tid >= o) incl += v;
            }
            const uint32_t excl = incl - c;
            if (k >= excl && k < incl) {        // one lane: the four bins that hold rank k
                uint32_t kk = k - excl, d = 4u * tid, cnt = c0;
                if (kk >= c0) { kk -= c0; d += 1; cnt = c1;
                    if (kk >= c1) { kk -= c1; d += 1; cnt = c2;
                        if (kk >= c2) { kk -= c2; d += 1; cnt = c3; } } }
                sel[0] = prefix | (d << sh);
                sel[1] = kk;
                sel[2] = cnt;
            }
        }
        __syncthreads();
        prefix = sel[0];
    }
    const uint32_t a_lo = prefix;
    const uint32_t cnt_le = (a.lo - sel[1]) + sel[2];       // keys below a_lo, and the keys equal to it
    uint32_t a_hi = a_lo;
    if (a.hi != a.lo && cnt_le < a.lo + 2u) {               // (uniform over the workgroup)
        uint32_t m = 0xffffffffu;
        for_keys([&](uint32_t key, bool valid) {
            if (valid && key > a_lo && key < m) m = key;
        });
        atomicMin(&sel[3], m);
        __syncthreads();
        a_hi = sel[3];
    }
    if (tid == 0) {
        const float lo_v = __uint_as_float(a_lo), hi_v = __uint_as_float(a_hi);
        const float d = hi_v - lo_v;
        const float q = a.wq < 0.5f ? __builtin_fmaf(a.wq, d, lo_v) : __builtin_fmaf(a.wq - 1.0f, d, hi_v);
        float sv = fminf(fmaxf(q, 1.0f), a.maxv);
        if (q != q) sv = q;                                 // (fmaxf would drop the NaN that torch.clamp keeps)
        if (has_nan) sv = __uint_as_float(0x7fc00000u);
        a.s[blockIdx.x] = sv;
    }
}

using QuantKernel = void (*)(QuantArgs);
template <int P, bool CACHED>
static QuantKernel quant_kernel_of(StepEps source) {
    if (source == STEP_EPS_GUIDED) return x0_quantile_kernel<P, GuidedEps, CACHED>;
    if constexpr (P == PRED_EPS)
        if (source == STEP_EPS_CLASSIFIER) return x0_quantile_kernel<P, ClassifierEps, CACHED>;
    return source == STEP_EPS_PLAIN ? x0_quantile_kernel<P, PlainEps, CACHED> : nullptr;
}

template <int P>
static QuantKernel quant_kernel_of(StepEps source, bool cached) {
    return cached ? quant_kernel_of<P, true>(source) : quant_kernel_of<P, false>(source);
}

// [a, a + na) and [b, b + nb) floats share an element
static bool ranges_overlap(const float* a, int64_t na, const float* b, int64_t nb) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a && b && a0 < b0 + 4u * (uintptr_t)nb && b0 < a0 + 4u * (uintptr_t)na;
}

int check_thresholding(const char* what, float ratio, float max_value) {
    SISIC_REQUIRE(std::isfinite(ratio) && ratio >= 0.0f && ratio <= 1.0f, "%s: dynamic_thresholding_ratio %g is outside [0, 1]", what,
                  (double)ratio);
    SISIC_REQUIRE(std::isfinite(max_value) && max_value >= 1.0f, "%s: sample_max_value %g is below 1 or not finite", what,
                  (double)max_value);
    return SISIC_OK;
}

// The launch of x0_quantile_kernel for the step L describes: L.thr_s [L.n / L.n_per_image] gets every image's s.  Reads what
// the step reads (eps, x, the row's sb and sa, w) and nothing the step writes: the step follows it on the same stream.
int launch_x0_threshold(sisic_ctx* ctx, const StepLaunch& L, hipStream_t s) {
    SISIC_TRY(check_rule(L.rule, L.flags));
    SISIC_TRY(check_thresholding("x0_threshold", L.thr_ratio, L.thr_max));
    const bool guided = L.source == STEP_EPS_GUIDED, clf = L.source == STEP_EPS_CLASSIFIER, replayed = L.state != nullptr;
    const float* eps2 = guided ? L.eps_u : clf ? L.grad : nullptr;
    SISIC_REQUIRE(L.eps && L.x && L.thr_s && L.n > 0 && (L.source == STEP_EPS_PLAIN || eps2), "x0_threshold: null tensor or empty");
    SISIC_REQUIRE(!clf || step_pred(L.flags) == PRED_EPS, "x0_threshold: prediction_type %d: classifier guidance takes "
                  "epsilon-prediction models only", step_pred(L.flags));
    SISIC_REQUIRE(L.n_per_image > 0 && L.n % L.n_per_image == 0, "x0_threshold: %lld elements are not whole images of %lld",
                  (long long)L.n, (long long)L.n_per_image);
    SISIC_REQUIRE(L.n_per_image <= THRESHOLD_MAX_PER_IMAGE, "x0_threshold: an image of %lld elements (at most 2^24: the rank is "
                  "formed in fp32)", (long long)L.n_per_image);
    SISIC_REQUIRE(L.n / L.n_per_image <= INT32_MAX, "x0_threshold: %lld images", (long long)(L.n / L.n_per_image));
    SISIC_REQUIRE(!ranges_overlap(L.thr_s, L.n / L.n_per_image, L.eps, L.n) && !ranges_overlap(L.thr_s, L.n / L.n_per_image, eps2, L.n) &&
                  !ranges_overlap(L.thr_s, L.n / L.n_per_image, L.x, L.n), "x0_threshold: s aliases eps, its second stream or x");
    QuantArgs a{};
    if (replayed) {
        SISIC_REQUIRE(L.coef_dev && (L.source == STEP_EPS_PLAIN || L.w_tab), "x0_threshold: null table");
    } else {
        SISIC_REQUIRE(L.row, "x0_threshold: null row");
        SISIC_TRY(check_step_row(L.rule, L.flags, L.row[0], L.row[1]));
        a.sb = L.row[0]; a.sa = L.row[1];
    }
    a.eps = L.eps; a.eps2 = eps2; a.x = L.x; a.s = L.thr_s; a.npi = L.n_per_image;
    a.st = static_cast<const LoopState*>(L.state); a.coef = L.coef_dev; a.wtab = L.w_tab; a.w = L.w;
    a.width = (int)SISIC_RULE_ROW_WIDTH(L.rule);
    // the rank in fp32, as torch.quantile forms it from a float32 q
    const float r = L.thr_ratio * (float)(L.n_per_image - 1);
    const float lo = std::floor(r), hi = std::ceil(r);
    a.lo = (uint32_t)lo; a.hi = (uint32_t)hi; a.wq = r - lo; a.maxv = L.thr_max;
    const uintptr_t al = reinterpret_cast<uintptr_t>(a.eps) | reinterpret_cast<uintptr_t>(a.eps2) | reinterpret_cast<uintptr_t>(a.x);
    a.vec4 = (al & 15) == 0 && (L.n_per_image & 3) == 0;
    ProfileScope prof(ctx, s, PK_DDPM, 4.0 * (a.vec4 && L.n_per_image <= QUANT_CACHE_MAX ? 1.0 : 5.0) * (eps2 ? 3.0 : 2.0) * (double)L.n, 0.0);
    const int P = step_pred(L.flags);
    const bool cached = a.vec4 && L.n_per_image <= QUANT_CACHE_MAX;
    const QuantKernel kernel = P == PRED_SAMPLE ? quant_kernel_of<PRED_SAMPLE>(L.source, cached)
                               : P == PRED_V    ? quant_kernel_of<PRED_V>(L.source, cached)
                                                : quant_kernel_of<PRED_EPS>(L.source, cached);
    SISIC_REQUIRE(kernel, "x0_threshold: eps source %d", (int)L.source);
    void* args[] = {&a};
    SISIC_HIP(hipLaunchKernel(reinterpret_cast<const void*>(kernel), dim3((unsigned)(L.n / L.n_per_image)), dim3(QUANT_THREADS), args, 0, s));
    return SISIC_OK;
}

int step_threshold_scratch(sisic_ctx* ctx, hipStream_t s, int64_t images, float** out) {
    std::lock_guard<std::mutex> lock(ctx->thr_s_mutex);
    auto& buf = ctx->thr_s[s];
    const size_t floats = (size_t)std::max<int64_t>(images, 64);
    if (buf.floats < floats) {
        SISIC_HIP(hipStreamSynchronize(s));          // earlier launches on this stream may still read the old buffer
        if (buf.p) SISIC_HIP(hipFree(buf.p));
        buf.p = nullptr; buf.floats = 0;
        SISIC_HIP(hipMalloc(reinterpret_cast<void**>(&buf.p), floats * sizeof(float)));
        if (poison_alloc()) {                        // SISIC_POISON_ALLOC=1: an s no workgroup writes is NaN
            SISIC_HIP(hipMemset(buf.p, 0xFF, floats * sizeof(float)));
            SISIC_HIP(hipDeviceSynchronize());
        }
        buf.floats = floats;
        ctx->scratch_generation.fetch_add(1);
    }
    *out = buf.p;
    return SISIC_OK;
}

// The one launcher (common.h StepLaunch): every check, the alignment rule, the grid and the byte count of a step, once.
int launch_step(sisic_ctx* ctx, const StepLaunch& L, hipStream_t s) {
    SISIC_TRY(check_rule(L.rule, L.flags));
    const bool guided = L.source == STEP_EPS_GUIDED, clf = L.source == STEP_EPS_CLASSIFIER;
    const bool hist = L.rule == STEP_RULE_DPMPP, replayed = L.state != nullptr;
    char name[64];
    std::snprintf(name, sizeof(name), "%s%s%s", rule_name(L.rule), replayed ? "_indexed" : "",
                  clf ? " (classifier-guided)" : L.edit ? "_edit" : guided ? " (guided)" : L.device_noise ? "_rng" : "");
    // what no kernel is built for
    SISIC_REQUIRE(!clf || step_pred(L.flags) == PRED_EPS, "%s: prediction_type %d: classifier guidance takes epsilon-prediction models only",
                  name, step_pred(L.flags));
    SISIC_REQUIRE(!clf || (L.device_noise && !L.edit), "%s: classifier guidance draws its noise on the device and takes no edit", name);
    SISIC_REQUIRE(!L.edit || L.device_noise, "%s: an edited step draws its noise on the device", name);
    SISIC_REQUIRE(!L.device_noise || !L.z, "%s: a noise buffer and seeds", name);
    // null, whole-image and alias checks
    const float* eps2 = guided ? L.eps_u : clf ? L.grad : nullptr;
    SISIC_REQUIRE(L.eps && L.x && L.out && L.n > 0 && (L.source == STEP_EPS_PLAIN || eps2) && (!L.device_noise || L.seeds_dev) &&
                  (!L.edit || (L.x0k && L.mask)), "%s: null tensor or empty", name);
    SISIC_REQUIRE(!clf || (L.grad != L.out && L.eps != L.out), "%s: eps or the gradient aliases the output", name);
    SISIC_REQUIRE(!hist || (L.hist && L.hist != L.x && L.hist != L.out && L.hist != L.eps && L.hist != eps2),
                  "%s: the history is missing or aliases another tensor", name);
    if (L.device_noise)
        SISIC_REQUIRE(L.n_per_image > 0 && L.n_per_image <= NOISE_MAX_PER_IMAGE && L.n % L.n_per_image == 0,
                      "%s: %lld elements are not whole images of %lld", name, (long long)L.n, (long long)L.n_per_image);
    // dynamic thresholding: s must lie apart from everything the step writes (what it reads is launch_x0_threshold's to check)
    const bool thr = L.thr_s != nullptr;
    if (thr) {
        const int64_t images = L.n_per_image > 0 ? (L.n + L.n_per_image - 1) / L.n_per_image : 1;
        SISIC_REQUIRE(!ranges_overlap(L.thr_s, images, L.out, guided ? 2 * L.n : L.n) && (!hist || !ranges_overlap(L.thr_s, images, L.hist, L.n)),
                      "%s: s aliases an output of the step", name);
    }
    if (L.edit) {
        SISIC_REQUIRE(L.hw > 0 && L.n_per_image % L.hw == 0, "%s: an image of %lld elements is not whole channels of %lld", name,
                      (long long)L.n_per_image, (long long)L.hw);
        SISIC_REQUIRE(L.x0k != L.out && L.mask != L.out && L.x0k != L.hist && L.mask != L.hist,
                      "%s: the known image or the mask aliases an output", name);
    }
    StepArgs a{};
    if (replayed) {
        // (the tables were checked row by row before the loop's first launch: the kernel reads its row and cannot refuse it)
        SISIC_REQUIRE(L.coef_dev && (L.device_noise || L.zrow_dev) && (!L.edit || L.erows_dev) && (L.source == STEP_EPS_PLAIN || L.w_tab),
                      "%s: null table", name);
    } else {
        SISIC_REQUIRE(L.row && (!L.edit || L.erow), "%s: null row", name);
        SISIC_TRY(check_step_row(L.rule, L.flags, L.row[0], L.row[1]));
        for (int k = 0; k < (int)SISIC_RULE_ROW_WIDTH(L.rule); ++k) a.row.v[k] = L.row[k];
        for (int k = 0; L.edit && k < 4; ++k) {
            SISIC_REQUIRE(std::isfinite(L.erow[k]), "%s: edit row {%g, %g, %g, %g}", name, L.erow[0], L.erow[1], L.erow[2], L.erow[3]);
            a.er[k] = L.erow[k];
        }
    }
    a.eps = L.eps; a.eps2 = eps2; a.x = L.x; a.out = L.out; a.hist = hist ? L.hist : nullptr;
    a.z = L.z; a.seeds = L.seeds_dev; a.x0k = L.edit ? L.x0k : nullptr; a.mask = L.edit ? L.mask : nullptr;
    a.st = static_cast<const LoopState*>(L.state); a.coef = L.coef_dev; a.zrow = L.zrow_dev; a.erows = L.erows_dev; a.wtab = L.w_tab;
    a.n = L.n; a.npi = L.n_per_image; a.hw = L.hw; a.w = L.w; a.clip = L.clip; a.step = L.step; a.thr = L.thr_s;
    // every refusal of the step lies above: the quantile launch (which checks the images and the setting, and may refuse too)
    // goes directly before the step's own, so that a refused call has launched nothing
    if (thr) SISIC_TRY(launch_x0_threshold(ctx, L, s));
    // 4 bytes per element of every stream read or written (the mask is a channel's worth per image); a row on the device
    // leaves out what only the row decides, and is never profiled (the replayed loop runs without the profiler)
    const bool z_read = !replayed && L.z && L.row[4] != 0.0f, hist_read = !replayed && hist && L.row[5] != 0.0f;
    double streams = (eps2 ? 2.0 : 1.0) + 1.0 + (guided ? 2.0 : 1.0) + (z_read ? 1.0 : 0.0) + (hist ? 1.0 : 0.0) + (hist_read ? 1.0 : 0.0);
    if (L.edit) streams += 1.0 + (double)L.hw / (double)L.n_per_image;
    ProfileScope prof(ctx, s, PK_DDPM, 4.0 * streams * (double)L.n, 0.0);
    // one alignment rule: every pointer of the launch on a 16-byte line; whole float4s per image with generated noise, per
    // channel with an edit, and per half when the result goes to both halves.  The scalar tail of the bodies takes n % 4.
    uintptr_t al = 0;
    for (const void* p : {(const void*)a.eps, (const void*)a.eps2, (const void*)a.x, (const void*)a.out, (const void*)a.hist,
                          (const void*)a.z, (const void*)a.x0k, (const void*)a.mask})
        al |= reinterpret_cast<uintptr_t>(p);
    a.vec4 = (al & 15) == 0 && (!(L.device_noise || thr) || (L.n_per_image & 3) == 0) && (!L.edit || (L.hw & 3) == 0) && (!guided || (L.n & 3) == 0);
    const int64_t work = a.vec4 ? (L.n + 3) / 4 : L.n;
    const dim3 grid((unsigned)std::min<int64_t>((work + 255) / 256, 2048)), block(256);
    const int form = clf ? FORM_CLF : L.edit ? FORM_EDIT + (guided ? 1 : 0) : (guided ? FORM_GUIDED_BUFFER : FORM_BUFFER) + (L.device_noise ? 1 : 0);
    const bool clipped = (L.flags & STEP_FLAG_CLIPPED_OUTPUT) != 0;
    const int P = step_pred(L.flags);
    const StepKernel kernel = P == PRED_SAMPLE ? step_kernel_of<PRED_SAMPLE>(L.rule, clipped, form, thr)
                              : P == PRED_V    ? step_kernel_of<PRED_V>(L.rule, clipped, form, thr)
                                               : step_kernel_of<PRED_EPS>(L.rule, clipped, form, thr);
    void* args[] = {&a};
    SISIC_HIP(hipLaunchKernel(reinterpret_cast<const void*>(kernel), grid, block, args, 0, s));
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
