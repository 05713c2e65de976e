// conv_mfma.hip -- fp32 NCHW convolution as an implicit GEMM on the gfx950 f32 MFMA pipe.
//
// Replaces every F.conv2d instance on the hot path (52 conv3x3 + 14 conv1x1 shortcuts per
// UNet forward, plus the attention q/k/v/out projections which are 1x1 convolutions in
// NCHW) together with the elementwise work diffusers runs around them -- GroupNorm-apply,
// SiLU, torch.cat of the skip tensor, nearest 2x upsampling, the time-embedding add and
// the residual add.
//
// GEMM view:  D[co, pixel] = sum_k W[co, k] * X[k, pixel],  k = (ci, ky, kx).
//   * pixels ride the MFMA lane dimension, so NCHW rows are read and written as
//     contiguous 128-byte segments and no layout change is needed at the boundary;
//   * v_mfma_f32_32x32x2_f32: exact fp32 FMA chain, one VGPR per operand; the two k of an
//     instruction are two consecutive input channels at the same filter tap;
//   * a workgroup owns CO_TILE=64 output channels x PIX pixels (a TH x TW rectangle of
//     one image) and walks the input channels in chunks of CIC, double-buffered in LDS:
//     the input halo tile [CIC][IH][IW] (GroupNorm+SiLU applied on the way in, zero
//     padding after it) and the weight slab [CIC][k*k][64];
//   * operands are read from LDS with ds_read_b32 at compile-time offsets from one
//     per-lane base each; per k-step a wave issues MT+NT reads for MT*NT MFMAs.
//
// Algorithmic bytes per launch: 4*B*(Cin*Hin*Win + Cout*Hout*Wout)
//   + 4*(Cin*Cout*k*k + Cout) (+ 4*B*Cout*Hout*Wout when a residual is read).
#include <cstdlib>
#include <type_traits>

#include "conv_plan.h"
#include "pack_device.h"

namespace sisic {

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct ConvParams {
    const float* in0;
    const float* in1;
    int c0, c1;
    int B, Hin, Win;   // source tensors
    int Hc, Wc;        // conv input extent (after the optional 2x upsample)
    int Hout, Wout;
    int ups;
    int zero_insert;   // with ups: the 2x grid holds the source at even coordinates and zeros elsewhere (transposed stride-2 conv)
    const float* w;    // packed [Cin_pad][KK][cout_pad]
    int cout_pad;
    const float* bias;
    int Cout;
    const float* gn_scale;
    const float* gn_shift;
    int gn_silu;
    const float* chan_bias;
    int chan_bias_stride;
    const float* residual;
    int relu;
    float* out;
    float* stats;      // optional GroupNorm partials [B][Cout][tiles_y*tiles_x*WN][4] = (count, sum, centred M2, 0)
    const void* reserved;   // (unused: holds the place of a former host-only field, so that the kernels' argument layout -- and with it their code -- is unchanged)
    int tiles_x, tiles_y, n_co_tiles, nwg, nchunks;
};

// sum over each aligned run of 32 lanes (the pixels of one accumulator row): DPP butterflies inside the two rows of 16,
// then one cross-row exchange.  Fixed order: the GroupNorm partials are bit-reproducible.
__device__ __forceinline__ float half_wave_sum(float v) {
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xf, 0xf, true));    // quad_perm [1,0,3,2]
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xf, 0xf, true));    // quad_perm [2,3,0,1]
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x141, 0xf, 0xf, true));   // row_half_mirror
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x140, 0xf, 0xf, true));   // row_mirror
    return v + __shfl_xor(v, 16);
}

__device__ __forceinline__ float silu_f(float v) { return v * __builtin_amdgcn_rcpf(1.0f + __expf(-v)); }   // v_rcp_f32, not the IEEE division sequence

template <int KS, int STRIDE, int MT, int NT, int WM, int WN, int TW, int CIC, int KSP = 1>
struct ConvGeom {
    static constexpr int NWAVES = WM * WN * KSP;              // KSP > 1: wave groups split the channel pairs of a chunk
    static constexpr int NTHR = 64 * NWAVES;
    static constexpr int CO_TILE = WM * MT * 32;
    static constexpr int PIX = WN * NT * 32;
    static constexpr int TH = PIX / TW;
    static constexpr int KK = KS * KS;
    static constexpr int PAD = KS / 2;
    static constexpr int IH = (TH - 1) * STRIDE + KS;
    static constexpr int IW = (TW - 1) * STRIDE + KS;
    static constexpr int TPC = NTHR / CIC;                    // threads staging one channel
    static constexpr int EPT = (IH * IW + TPC - 1) / TPC;     // input elements per thread per chunk
    static constexpr int CHS = EPT * TPC;                     // LDS floats per staged channel (>= IH*IW, padded so
                                                              // every thread stores all its EPT elements)
    static constexpr int IN_BUF = ((CIC * CHS + 3) / 4) * 4;  // floats, 16-B multiple
    static constexpr int W_F4 = CIC * KK * CO_TILE / 4;       // float4 per weight slab
    static constexpr int W_F4_PT = (W_F4 + NTHR - 1) / NTHR;
    static constexpr int W_BUF = W_F4_PT * NTHR * 4;          // padded likewise
    static constexpr size_t LDS_BYTES = size_t(2) * (IN_BUF + W_BUF) * sizeof(float);
    static_assert(CO_TILE == CONV_CO_TILE, "weight packing assumes 64-channel tiles");
    static_assert(PIX % TW == 0, "tile must be whole rows");
    static_assert(NTHR % CIC == 0, "staging split");
    static_assert(CIC % (2 * KSP) == 0, "two channels per MFMA, whole pairs per K group");
};

// V4 (1x1 stride 1, H*W a multiple of 4): the pixel tile of a channel is one contiguous run, so a staging thread moves
// four consecutive pixels per instruction (global_load_dwordx4 -> ds_write_b128) instead of single elements strided by
// the staging-thread count: 5x fewer vector instructions per chunk and 256-byte instead of 64-byte global segments.
template <int KS, int STRIDE, int MT, int NT, int WM, int WN, int TW, int CIC, int OCC, int KSP, bool V4 = false>
__global__ void __launch_bounds__(64 * WM * WN * KSP, OCC) conv_mfma_kernel(const ConvParams p) {
    using G = ConvGeom<KS, STRIDE, MT, NT, WM, WN, TW, CIC, KSP>;
    static_assert(!V4 || (KS == 1 && STRIDE == 1 && TW == G::PIX && G::EPT % 4 == 0 && G::CHS % 4 == 0),
                  "the float4 staging path is for flat 1x1 tiles");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* const in_lds = smem;                    // [2][IN_BUF]
    float* const w_lds = smem + 2 * G::IN_BUF;     // [2][W_BUF]

    // ---- which tile: XCD-aware bijective remap (blocks b, b+8 share an XCD's L2) so that the
    // co-tiles of one pixel tile and the neighbouring pixel tiles of one image land on one XCD.
    int work;
    {
        const int L = blockIdx.x, nwg = p.nwg;
        const int xcd = L & 7, slot = L >> 3, q = nwg >> 3, r = nwg & 7;
        work = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + slot;
    }
    const int co_t = work % p.n_co_tiles;
    int tile = work / p.n_co_tiles;
    const int tx = tile % p.tiles_x;
    tile /= p.tiles_x;
    const int ty = tile % p.tiles_y;
    const int b = tile / p.tiles_y;
    const int oy0 = ty * G::TH, ox0 = tx * TW;   // output-space origin of the tile
    const int co0 = co_t * G::CO_TILE;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int kg = wave / (WM * WN), wq = wave % (WM * WN);   // K-split group, position inside the output tile
    const int wm = wq / WN, wn = wq % WN;
    const int half = lane >> 5, l31 = lane & 31;

    // ---- input staging plan (invariant over the channel loop)
    const int sci = tid / G::TPC;   // staged channel within the chunk
    const int sl = tid % G::TPC;
    const int HWin = p.Hin * p.Win;
    const int Cin = p.c0 + p.c1;
    int goff[G::EPT];
    unsigned vmask = 0;
    constexpr int EPT4 = V4 ? G::EPT / 4 : 1;
    int goff4[EPT4];              // V4: first pixel of this thread's i-th float4 (clamped), valid bit i in vmask4
    unsigned vmask4 = 0;
    if constexpr (V4) {
#pragma unroll
        for (int i = 0; i < EPT4; ++i) {
            const int px = ox0 + 4 * sl + i * G::TPC * 4;
            const bool v = px < p.Wc;                         // H*W % 4 == 0: a float4 is inside or outside as a whole
            goff4[i] = v ? px : 0;
            vmask4 |= (v ? 1u : 0u) << i;
        }
    }
#pragma unroll
    for (int i = 0; i < (V4 ? 0 : G::EPT); ++i) {
        const int e = sl + i * G::TPC;
        const int yy = e / G::IW, xx = e % G::IW;
        const int gy = oy0 * STRIDE - G::PAD + yy;
        const int gx = ox0 * STRIDE - G::PAD + xx;
        const bool v = (e < G::IH * G::IW) && gy >= 0 && gy < p.Hc && gx >= 0 && gx < p.Wc &&
                       !(p.zero_insert && ((gy | gx) & 1));
        goff[i] = v ? ((gy >> p.ups) * p.Win + (gx >> p.ups)) : 0;
        vmask |= (v ? 1u : 0u) << i;
    }
    static_assert(G::EPT <= 32, "valid mask is 32 bits");

    // ---- MFMA operand bases
    const int a_base = half * G::KK * G::CO_TILE + wm * MT * 32 + l31;
    int b_base;
    {
        const int pix = wn * NT * 32 + l31;
        const int y = pix / TW, x = pix % TW;
        b_base = half * G::CHS + (y * STRIDE) * G::IW + x * STRIDE;
    }
    // offset of N-tile nt relative to nt=0 (32 pixels further along the tile)
    constexpr int NT_STEP = (TW >= 32) ? ((TW > 32) ? 32 * STRIDE : STRIDE * G::IW) : (32 / TW) * STRIDE * G::IW;
    static_assert(TW >= 32 || 32 % TW == 0, "TW must divide 32");
    static_assert(TW <= 32 || TW % 32 == 0, "TW must be a multiple of 32");

    f32x16 acc[MT][NT];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.0f;

    float rin[G::EPT];
    float rw[G::W_F4_PT * 4];   // scalars, not a float4 array: hipcc keeps a float4[] staging array in scratch
    float gsc = 1.0f, gsh = 0.0f;
    bool cval = false;

    // All staging loads are UNCONDITIONAL at clamped, always-valid addresses and masked afterwards:
    // a per-element "load or zero" select makes hipcc branch around every load and wait vmcnt(0)
    // inside each branch, which serialises the whole prefetch (cdna_hip_programming.md, .s-level trap c).
    const int prologue = (p.gn_scale == nullptr) ? 0 : (p.gn_silu ? 2 : 1);   // wave-uniform

    // (always_inline: called from two instances of `step`, the 7x7 instance's compute_chunk was left as a function of its own --
    //  its accumulators went through memory and config 5 ran four times slower until tools/bench_configs.py was run again)
    auto load_chunk = [&](int chunk) __attribute__((always_inline)) {
        const int c = chunk * CIC + sci;
        cval = c < Cin;
        const int cc = min(c, Cin - 1);
        const float* src = (cc < p.c0) ? p.in0 + ((size_t)b * p.c0 + cc) * HWin
                                       : p.in1 + ((size_t)b * p.c1 + (cc - p.c0)) * HWin;
        if constexpr (V4) {
#pragma unroll
            for (int i = 0; i < EPT4; ++i) {
                const float4 t = *reinterpret_cast<const float4*>(src + goff4[i]);
                rin[4 * i + 0] = t.x; rin[4 * i + 1] = t.y; rin[4 * i + 2] = t.z; rin[4 * i + 3] = t.w;
            }
        } else {
#pragma unroll
            for (int i = 0; i < G::EPT; ++i) rin[i] = src[goff[i]];
        }
        if (prologue) {
            gsc = p.gn_scale[(size_t)b * Cin + cc];
            gsh = p.gn_shift[(size_t)b * Cin + cc];
        }
        const float* wsrc = p.w + (size_t)chunk * CIC * G::KK * p.cout_pad + co0;
#pragma unroll
        for (int i = 0; i < G::W_F4_PT; ++i) {
            const int f = min(tid + i * G::NTHR, G::W_F4 - 1);
            const int rr = f / (G::CO_TILE / 4), c4 = f % (G::CO_TILE / 4);
            const float4 t = *reinterpret_cast<const float4*>(wsrc + (size_t)rr * p.cout_pad + c4 * 4);
            rw[4 * i + 0] = t.x; rw[4 * i + 1] = t.y; rw[4 * i + 2] = t.z; rw[4 * i + 3] = t.w;
        }
    };

    // (buf is a compile-time constant in the channel loop below: no buffer-parity arithmetic in the operand addresses)
    auto store_chunk = [&](const int buf) __attribute__((always_inline)) {
        float* dst = in_lds + buf * G::IN_BUF + sci * G::CHS + sl;
        const unsigned m = cval ? vmask : 0u;       // padding / missing channels stay zero AFTER the prologue
        float v[G::EPT];
        if (prologue == 2) {
#pragma unroll
            for (int i = 0; i < G::EPT; ++i) v[i] = silu_f(rin[i] * gsc + gsh);
        } else if (prologue == 1) {
#pragma unroll
            for (int i = 0; i < G::EPT; ++i) v[i] = rin[i] * gsc + gsh;
        } else {
#pragma unroll
            for (int i = 0; i < G::EPT; ++i) v[i] = rin[i];
        }
        if constexpr (V4) {
            float* dst4 = in_lds + buf * G::IN_BUF + sci * G::CHS + 4 * sl;
            const unsigned m4 = cval ? vmask4 : 0u;
#pragma unroll
            for (int i = 0; i < EPT4; ++i) {
                const bool on = (m4 >> i) & 1u;
                *reinterpret_cast<float4*>(dst4 + i * G::TPC * 4) =
                    make_float4(on ? v[4 * i + 0] : 0.0f, on ? v[4 * i + 1] : 0.0f, on ? v[4 * i + 2] : 0.0f, on ? v[4 * i + 3] : 0.0f);
            }
        } else {
#pragma unroll
            for (int i = 0; i < G::EPT; ++i) dst[i * G::TPC] = ((m >> i) & 1u) ? v[i] : 0.0f;
        }
        float* wdst = w_lds + buf * G::W_BUF + tid * 4;
#pragma unroll
        for (int i = 0; i < G::W_F4_PT; ++i)
            *reinterpret_cast<float4*>(wdst + i * G::NTHR * 4) =
                make_float4(rw[4 * i + 0], rw[4 * i + 1], rw[4 * i + 2], rw[4 * i + 3]);
    };

    auto compute_chunk = [&](const int buf) __attribute__((always_inline)) {
        const float* A = w_lds + buf * G::W_BUF + a_base;
        const float* Bm = in_lds + buf * G::IN_BUF + b_base;
#pragma unroll
        for (int cp = kg * (CIC / 2 / KSP); cp < (kg + 1) * (CIC / 2 / KSP); ++cp) {
#pragma unroll
            for (int ky = 0; ky < KS; ++ky) {
#pragma unroll
                for (int kx = 0; kx < KS; ++kx) {
                    float a[MT], bb[NT];
#pragma unroll
                    for (int m = 0; m < MT; ++m)
                        a[m] = A[(2 * cp * G::KK + ky * KS + kx) * G::CO_TILE + m * 32];
#pragma unroll
                    for (int n = 0; n < NT; ++n)
                        bb[n] = Bm[2 * cp * G::CHS + ky * G::IW + kx + n * NT_STEP];
#pragma unroll
                    for (int m = 0; m < MT; ++m)
#pragma unroll
                        for (int n = 0; n < NT; ++n)
                            acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[m], bb[n], acc[m][n], 0, 0, 0);
                }
            }
        }
    };

    // ---- channel loop: register-staged double buffering, one barrier per chunk
    load_chunk(0);
    store_chunk(0);
    __syncthreads();
    auto step = [&](const int chunk, auto buf_tag) __attribute__((always_inline)) {
        constexpr int BUF = decltype(buf_tag)::value;
        const bool more = chunk + 1 < p.nchunks;
        if (more) load_chunk(chunk + 1);
        compute_chunk(BUF);
        if (more) store_chunk(BUF ^ 1);
        __syncthreads();
    };
    {
        int chunk = 0;
        for (; chunk + 1 < p.nchunks; chunk += 2) {
            step(chunk, std::integral_constant<int, 0>{});
            step(chunk + 1, std::integral_constant<int, 1>{});
        }
        if (chunk < p.nchunks) step(chunk, std::integral_constant<int, 0>{});
    }

    // ---- K-split: the wave groups hold partial sums over disjoint channel pairs of the same output tile; groups
    // 1.. hand their accumulators to group 0 through LDS (the staging buffers are dead after the loop's last barrier).
    if constexpr (KSP > 1) {
        static_assert(KSP == 2, "two K groups");
        static_assert((size_t)WM * WN * MT * NT * 16 * 64 * sizeof(float) <= G::LDS_BYTES, "reduction slab fits the staging LDS");
        float* red = smem + (size_t)wq * MT * NT * 16 * 64 + lane;
        if (kg == 1) {
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int n = 0; n < NT; ++n)
#pragma unroll
                    for (int r = 0; r < 16; ++r) red[((m * NT + n) * 16 + r) * 64] = acc[m][n][r];
        }
        __syncthreads();
        if (kg != 0) return;
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int n = 0; n < NT; ++n)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[m][n][r] += red[((m * NT + n) * 16 + r) * 64];
    }

    // ---- epilogue: bias + per-sample channel bias (time embedding) + residual, NCHW store.
    // Loads use clamped indices and are unconditional; only the stores are predicated.
    const size_t HWout = (size_t)p.Hout * p.Wout;
    float cbias[MT][16];
#pragma unroll
    for (int m = 0; m < MT; ++m) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            cbias[m][r] = 0.0f;
        }
    }
    if (p.bias) {
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                cbias[m][r] += p.bias[min(co0 + wm * MT * 32 + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * half, p.Cout - 1)];
    }
    if (p.chan_bias) {
        const float* cb = p.chan_bias + (size_t)b * p.chan_bias_stride;
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                cbias[m][r] += cb[min(co0 + wm * MT * 32 + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * half, p.Cout - 1)];
    }
    float psum[MT][16];      // per output channel: sum of this lane's stored values (GroupNorm partials)
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) psum[m][r] = 0.0f;
    unsigned pvmask = 0;
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        const int pix = wn * NT * 32 + n * 32 + l31;
        const int oy = oy0 + pix / TW, ox = ox0 + pix % TW;
        const bool pv = oy < p.Hout && ox < p.Wout;
        pvmask |= pv ? (1u << n) : 0u;
        const size_t pix_off = (size_t)min(oy, p.Hout - 1) * p.Wout + min(ox, p.Wout - 1);
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            float res[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) res[r] = 0.0f;
            if (p.residual) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int co = min(co0 + wm * MT * 32 + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * half, p.Cout - 1);
                    res[r] = p.residual[((size_t)b * p.Cout + co) * HWout + pix_off];
                }
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = co0 + wm * MT * 32 + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                float v = acc[m][n][r] + cbias[m][r] + res[r];
                if (p.relu) v = fmaxf(v, 0.0f);
                if (pv && co < p.Cout) p.out[((size_t)b * p.Cout + co) * HWout + pix_off] = v;
                acc[m][n][r] = v;
                psum[m][r] += pv ? v : 0.0f;
            }
        }
    }

    // ---- GroupNorm partials of what was just stored: per output channel and wave, (count, sum, sum of squared
    // deviations from the wave's own mean) over the wave's NT*32 pixels; merged exactly by gn_finalize_kernel.
    if (p.stats) {
        const float cnt = half_wave_sum((float)__builtin_popcount(pvmask));
        const float inv = 1.0f / fmaxf(cnt, 1.0f);
        const int slots = p.tiles_x * p.tiles_y * WN, slot = (ty * p.tiles_x + tx) * WN + wn;
#pragma unroll
        for (int m = 0; m < MT; ++m) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = co0 + wm * MT * 32 + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                const float s1 = half_wave_sum(psum[m][r]);
                const float mean = s1 * inv;
                float q = 0.0f;
#pragma unroll
                for (int n = 0; n < NT; ++n) {
                    const float d = acc[m][n][r] - mean;
                    q += ((pvmask >> n) & 1u) ? d * d : 0.0f;
                }
                q = half_wave_sum(q);
                if (l31 == 0 && co < p.Cout)
                    reinterpret_cast<float4*>(p.stats)[((size_t)b * p.Cout + co) * slots + slot] = make_float4(cnt, s1, q, 0.0f);
            }
        }
    }
}


// OIHW -> [Cin_pad][KK][cout_pad], zero padded
__global__ void conv_pack_kernel(const float* __restrict__ w, int Cout, int Cin, int KK, int cin_pad, int cout_pad,
                                 float* __restrict__ out) {
    const size_t first = (size_t)cin_pad * KK * cout_pad;
    const size_t total = KK == 1 ? 3 * first + first / 2 : first;                   // 1x1: all three layouts (pack_device.h)
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        conv_pack_elem(i, w, Cout, Cin, KK, cin_pad, cout_pad, out);
    }
}

template <int KS, int STRIDE, int MT, int NT, int WM, int WN, int TW, int CIC, int OCC = 2, int KSP = 1>
static int launch_cfg(sisic_ctx* ctx, ConvParams& p, hipStream_t s) {
    using G = ConvGeom<KS, STRIDE, MT, NT, WM, WN, TW, CIC, KSP>;
    p.tiles_x = cdiv(p.Wout, TW);
    p.tiles_y = cdiv(p.Hout, G::TH);
    p.n_co_tiles = p.cout_pad / G::CO_TILE;
    p.nchunks = cdiv(p.c0 + p.c1, CIC);
    p.nwg = p.B * p.tiles_x * p.tiles_y * p.n_co_tiles;       // (conv_plan checked that the grid fits)
    static std::atomic<uint64_t> lds_opt_in{0}, lds_opt_in4{0};     // one bit per device (common.h)
    auto run = [&](auto kern, std::atomic<uint64_t>& opt_in) -> int {
        SISIC_TRY(ensure_dynamic_lds(ctx, reinterpret_cast<const void*>(kern), (int)G::LDS_BYTES, opt_in));
        hipLaunchKernelGGL(kern, dim3(p.nwg), dim3(G::NTHR), G::LDS_BYTES, s, p);
        SISIC_HIP(hipGetLastError());
        return SISIC_OK;
    };
    if constexpr (KS == 1 && STRIDE == 1 && TW == G::PIX && G::EPT % 4 == 0) {
        // flat 1x1 tile: float4 staging when every plane is a whole number of 16-byte aligned float4
        const bool aligned = ((reinterpret_cast<uintptr_t>(p.in0) | reinterpret_cast<uintptr_t>(p.in1)) & 15) == 0;
        if (p.Wc % 4 == 0 && aligned) return run(conv_mfma_kernel<KS, STRIDE, MT, NT, WM, WN, TW, CIC, OCC, KSP, true>, lds_opt_in4);
    }
    return run(conv_mfma_kernel<KS, STRIDE, MT, NT, WM, WN, TW, CIC, OCC, KSP>, lds_opt_in);
}

int launch_conv_pack(sisic_ctx*, const float* w, int Cout, int Cin, int k, float* packed, hipStream_t s) {
    SISIC_REQUIRE(k == 1 || k == 3 || k == 7, "conv_pack: ksize %d unsupported", k);
    const int cin_pad = conv_cin_pad(Cin, k), cout_pad = conv_cout_pad(Cout);
    const size_t total = (size_t)cin_pad * k * k * cout_pad;
    const int blocks = (int)std::min<size_t>((total * (k == 1 ? 4 : 1) + 255) / 256, 4096);
    hipLaunchKernelGGL(conv_pack_kernel, dim3(blocks), dim3(256), 0, s, w, Cout, Cin, k * k, cin_pad, cout_pad, packed);
    SISIC_HIP(hipGetLastError());
    return SISIC_OK;
}

// The direct kernel in the tiling the plan chose (SISIC_DIRECT_TILINGS, conv_plan.h)
static int launch_conv_direct(sisic_ctx* ctx, const sisic_conv_args& a, const ConvPlan& plan, hipStream_t s) {
    ConvParams p{};
    p.in0 = a.in0; p.in1 = a.in1; p.c0 = a.c0; p.c1 = a.c1;
    p.B = a.B; p.Hin = a.Hin; p.Win = a.Win;
    p.ups = a.upsample ? 1 : 0;
    p.zero_insert = a.upsample == 2 ? 1 : 0;
    p.Hc = a.Hin << p.ups; p.Wc = a.Win << p.ups;
    p.Hout = plan.Hout; p.Wout = plan.Wout;
    p.w = a.w_packed; p.cout_pad = conv_cout_pad(a.Cout);
    p.bias = a.bias; p.Cout = a.Cout;
    p.gn_scale = a.gn_scale; p.gn_shift = a.gn_shift; p.gn_silu = a.gn_silu;
    p.chan_bias = a.chan_bias; p.chan_bias_stride = a.chan_bias_stride; p.residual = a.residual; p.relu = a.relu; p.out = a.out;
    p.stats = a.stats_out;
    if (a.ksize == 1 && a.stride == 1) {      // 1x1: the image is a flat row of H*W pixels
        p.Hin = 1; p.Win = a.Hin * a.Win; p.Hc = 1; p.Wc = p.Win; p.Hout = 1; p.Wout = p.Win;
    }
    switch (plan.cfg) {
#define X(id, KS, STRIDE, MT, NT, WM, WN, TW, CIC, OCC, KSP) \
        case id: return launch_cfg<KS, STRIDE, MT, NT, WM, WN, TW, CIC, OCC, KSP>(ctx, p, s);
        SISIC_DIRECT_TILINGS(X)
#undef X
    }
    set_error("conv2d: internal: no direct tiling %d", plan.cfg);
    return SISIC_EINVAL;
}

// Plans once (conv_plan.h), opens the profile scope from the plan and hands (a, plan) to the chosen launcher.
int launch_conv2d(sisic_ctx* ctx, const sisic_conv_args& a, hipStream_t s, const GnFinJob* rider, bool* carried) {
    if (carried) *carried = false;
    ConvPlan plan;
    SISIC_TRY(conv_plan(a, &plan));
    SISIC_REQUIRE(!plan.refusal[0], "%s", plan.refusal);
    ProfileScope prof(ctx, s, plan.profile_kind, plan.bytes, plan.flops, plan.issued_flops, plan.profile_slot);
    const GnFinJob* ride = (plan.carries_rider && carried) ? rider : nullptr;
    int rc;
    switch (plan.kernel) {
        case CK_SMALLCOUT: rc = launch_conv_smallcout(ctx, a, plan, s); break;
        case CK_DIRECT: rc = launch_conv_direct(ctx, a, plan, s); break;
        case CK_POINTWISE: rc = launch_conv_pointwise(ctx, a, plan, s); break;
        case CK_POINTWISE_BF3: rc = launch_conv_pointwise_bf3(ctx, a, plan, s, ride); break;
        case CK_S2_BF3: rc = launch_conv_s2_bf3(ctx, a, plan, s); break;
        default: rc = launch_conv_winograd(ctx, a, plan, s); break;
    }
    if (rc == SISIC_OK && ride) *carried = true;      // the plan's word, once the launch has been made
    return rc;
}

}  // namespace sisic
