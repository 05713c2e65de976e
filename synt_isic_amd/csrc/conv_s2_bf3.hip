// conv_s2_bf3.hip -- 3x3 stride-2 convolutions (the UNet's downsamplers) with fp32-EQUIVALENT products on the bf16 matrix pipe
// (tile_cfg 36).
//
// The arithmetic of conv_pointwise_bf3.hip / conv_winograd_bf3.inc applied to the implicit GEMM over nine taps
//     D[co, (oy, ox)] = sum_ci sum_tap W[co, ci, ky, kx] * x[ci, 2 oy + ky - 1, 2 ox + kx - 1]:
// every fp32 operand is split exactly into three bf16 terms (hi + mid + lo), six of the nine term products are summed by three
// v_mfma_f32_32x32x16_bf16 per 8-channel chunk, tap, 32-channel block and 32-pixel block; the MFMA operand grouping is the
// pointwise kernels' (K = 16 = four channels x two terms per half-wave).
//
// A WAVE owns a tile of 4 x 8 output pixels (its 32 MFMA columns) x 64 output channels of one image.  Per 8-channel chunk it
//   stages the tile's 9 x 17 input patch ONCE: 20 dword loads per lane, zero outside the image (a select on the loaded value,
//          never a product with it), the exact split, and the B operands -- (hi, mid) 16 bytes and lo 8 bytes per position and
//          channel group -- into the wave's PRIVATE piece of LDS.  A stride-2 input element serves 2.25 taps on average: it is
//          split once, not once per tap.  Columns are stored by parity and rows 20 slots apart, so that the 32 lanes of a tap's
//          read (column stride 2, row stride 2) fall on distinct banks;
//   B      per tap one 16-byte and one 8-byte LDS read at a constant offset from the lane's base;
//   A      the split filters straight from global memory (pack_device.h, conv_s2_pack_bf3_elem), two taps ahead in registers
//          (three sets; nine taps, so a tap's set does not change from chunk to chunk);
//   the next chunk's patch is requested before the taps of this one run.  Nothing is shared between waves, so there is no
//   barrier in the loop.
// K-SPLIT: the four waves of a workgroup share ONE tile and take a quarter of the input chunks each (conv_pwbk_kernel); the
// partial accumulators go through LDS and are summed in the fixed order ((k0 + k1) + k2) + k3, every wave finishing a quarter
// of the 64 channels.  For EVERY shape: a grid of (image, tile, channel tile) only, so an image's bits do not depend on its
// batch.  (Measured and removed, profiles/r07/conv_bench_s2_bf16x3.txt: a wave running the whole contraction of a tile of
// its own -- slower on all three downsamplers, 47 vs 43, 63 vs 38 and 115 vs 39 us; two tiles per wave under one filter
// fetch -- 47 vs 42, 38 vs 38, 49 vs 38 us; filters one tap ahead instead of two, three waves per SIMD instead of four -- level.)
#include <cstdlib>

#include "conv_plan.h"
#include "pack_device.h"

namespace sisic {

typedef float s2b_f32x16 __attribute__((ext_vector_type(16)));
typedef short s2b_bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned s2b_u4 __attribute__((ext_vector_type(4)));
typedef unsigned s2b_u2 __attribute__((ext_vector_type(2)));

struct S2bParams {
    const float* in;
    int Cin, B, H, W, Hout, Wout;
    const float* wb;         // [Cin/8][9][Cout/64][768 dwords]
    int n_co64;
    const float* bias;
    int Cout;
    const float* chan_bias;
    int chan_bias_stride;
    const float* residual;
    int relu;
    float* out;
    float* stats;            // optional [B][Cout][tiles][4]
    int tiles_x, tiles_y, n_co_items, nwg, nchunks;
};

constexpr int S2B_WAVES = 4;
constexpr int S2B_TH = 4, S2B_TW = 8;                          // output pixels of a tile
constexpr int S2B_PH = 2 * S2B_TH + 1, S2B_PW = 2 * S2B_TW + 1; // its input patch: 9 x 17
constexpr int S2B_NPOS = S2B_PH * S2B_PW;                      // 153 positions
constexpr int S2B_ROUNDS = (S2B_NPOS + 31) / 32;               // a half-wave stages 32 positions of its channel group per round
constexpr int S2B_ROW = 20;                                    // slots per patch row: even columns at 0 .. 8, odd at 9 .. 16
constexpr int S2B_SLOTS = S2B_PH * S2B_ROW;                    // per channel group
constexpr int S2B_WAVE_DWORDS = 2 * S2B_SLOTS * 6;             // (hi, mid) [2][slots][4] then lo [2][slots][2]

__device__ __forceinline__ float s2b_half_wave_sum(float v) {
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xf, 0xf, true));
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xf, 0xf, true));
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x141, 0xf, 0xf, true));
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x140, 0xf, 0xf, true));
    return v + __shfl_xor(v, 16);
}

__global__ void __launch_bounds__(64 * S2B_WAVES, 4) conv_s2b_kernel(const S2bParams p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    int item;
    {   // XCD-aware bijective remap (conv_mfma.hip)
        const int L = blockIdx.x, nwg = p.nwg;
        const int xcd = L & 7, slot = L >> 3, q = nwg >> 3, r = nwg & 7;
        item = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + slot;
    }
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave_u = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5, l31 = lane & 31;
    const int ntiles = p.tiles_x * p.tiles_y;
    int co_i = item % p.n_co_items;                                 // output channel item fastest: its waves share the patch
    const int t = item / p.n_co_items;
    int tile = t % ntiles, b = t / ntiles;
    asm volatile("" : "+s"(co_i), "+s"(tile), "+s"(b));             // (uniform values in scalar registers, conv_pointwise_bf3.hip)
    const int ty = tile / p.tiles_x, tx = tile - ty * p.tiles_x;
    constexpr int CB = 2;                                           // 32-channel blocks per wave
    const int H = p.H, W = p.W, HW = H * W, Ho = p.Hout, Wo = p.Wout, HWo = Ho * Wo;
    const int oy0 = S2B_TH * ty, ox0 = S2B_TW * tx, co0 = 64 * co_i;
    const int iy0 = 2 * oy0 - 1, ix0 = 2 * ox0 - 1;
    // this wave's chunks (a ragged quarter: the last waves get fewer, or none)
    const int per = (p.nchunks + S2B_WAVES - 1) / S2B_WAVES;
    const int c_begin = min(wave_u * per, p.nchunks), c_end = min(c_begin + per, p.nchunks);

    const __amdgpu_buffer_rsrc_t rsx = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.in + (size_t)b * p.Cin * HW), 0, -1, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsw = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.wb), 0, -1, 0x00020000);
    const unsigned a_lane16 = 16u * (unsigned)lane, a_lane8 = 8u * (unsigned)lane;

    unsigned* const S_hm = reinterpret_cast<unsigned*>(smem) + wave_u * S2B_WAVE_DWORDS;
    unsigned* const S_lo = S_hm + 2 * S2B_SLOTS * 4;

    // staging: in round rd the lane holds position 32 rd + l31 of the patch, channels 4 half .. 4 half + 3 of the chunk
    unsigned x_voff[S2B_ROUNDS], st_slot[S2B_ROUNDS], inside = 0, staged = 0;
#pragma unroll
    for (int rd = 0; rd < S2B_ROUNDS; ++rd) {
        const int pp = 32 * rd + l31;
        const int py = pp / S2B_PW, px = pp - S2B_PW * py;
        const int iy = iy0 + py, ix = ix0 + px;
        const bool in_patch = pp < S2B_NPOS;
        const bool ok = in_patch && iy >= 0 && iy < H && ix >= 0 && ix < W;
        x_voff[rd] = 4u * (unsigned)((4 * half) * HW + (ok ? iy * W + ix : 0));     // (outside: an address inside the plane; the value is discarded)
        st_slot[rd] = (unsigned)(half * S2B_SLOTS + py * S2B_ROW + (px & 1) * 9 + (px >> 1));
        inside |= (ok ? 1u : 0u) << rd;
        staged |= (in_patch ? 1u : 0u) << rd;
    }
    // reading: the lane's pixel (oy_l, ox_l) = (l31 >> 3, l31 & 7); tap (ky, kx) lies ky rows and {0, 9, 1}[kx] slots further
    const unsigned rd_slot = (unsigned)(half * S2B_SLOTS + 2 * (l31 >> 3) * S2B_ROW + (l31 & 7));
    const unsigned* const R_hm = S_hm + 4 * rd_slot;
    const unsigned* const R_lo = S_lo + 2 * rd_slot;

    s2b_f32x16 acc[CB];
#pragma unroll
    for (int x = 0; x < CB; ++x)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[x][r] = 0.0f;

    struct XRegs { float x[S2B_ROUNDS][4]; };
    auto load_x = [&](int c, XRegs& xr) {
        const unsigned soff = 4u * (unsigned)(8 * c * HW);
#pragma unroll
        for (int rd = 0; rd < S2B_ROUNDS; ++rd)
#pragma unroll
            for (int k = 0; k < 4; ++k)
                xr.x[rd][k] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsx, x_voff[rd], soff + 4u * (unsigned)(k * HW), 0));
    };
    auto load_f = [&](int c, int tap, s2b_u4 (&fa)[CB], s2b_u2 (&fl)[CB]) {
        const unsigned s0 = 3072u * (unsigned)((c * 9 + tap) * p.n_co64 + co_i);
#pragma unroll
        for (int x = 0; x < CB; ++x) {
            fa[x] = __builtin_amdgcn_raw_buffer_load_b128(rsw, a_lane16, s0 + 1024u * (unsigned)x, 0);
            fl[x] = __builtin_amdgcn_raw_buffer_load_b64(rsw, a_lane8, s0 + 2048u + 512u * (unsigned)x, 0);
        }
    };
    // the exact split of the staged values (truncations and exact differences, conv_pointwise_bf3.hip) into the wave's LDS
    auto stage = [&](const XRegs& xr) {
#pragma unroll
        for (int rd = 0; rd < S2B_ROUNDS; ++rd) {
            const bool ok = (inside >> rd) & 1u;
            unsigned hi[2], mid[2], lo[2];
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const float v0 = ok ? xr.x[rd][2 * q] : 0.0f, v1 = ok ? xr.x[rd][2 * q + 1] : 0.0f;       // zero padding: a select
                const unsigned h0 = __float_as_uint(v0) & 0xffff0000u, h1 = __float_as_uint(v1) & 0xffff0000u;
                const float r0 = v0 - __uint_as_float(h0), r1 = v1 - __uint_as_float(h1);
                const unsigned m0 = __float_as_uint(r0) & 0xffff0000u, m1 = __float_as_uint(r1) & 0xffff0000u;
                const float l0 = r0 - __uint_as_float(m0), l1 = r1 - __uint_as_float(m1);
                hi[q] = __builtin_amdgcn_perm(h1, h0, 0x07060302u);
                mid[q] = __builtin_amdgcn_perm(m1, m0, 0x07060302u);
                lo[q] = __builtin_amdgcn_perm(__float_as_uint(l1), __float_as_uint(l0), 0x07060302u);
            }
            if ((staged >> rd) & 1u) {
                *reinterpret_cast<s2b_u4*>(S_hm + 4 * st_slot[rd]) = s2b_u4{hi[0], hi[1], mid[0], mid[1]};
                *reinterpret_cast<s2b_u2*>(S_lo + 2 * st_slot[rd]) = s2b_u2{lo[0], lo[1]};
            }
        }
    };
    // the patch is written and read by this wave only: LDS operations of a wave complete in order, the fence keeps the
    // compiler from moving one lane's reads over another lane's writes
    auto wave_fence = [&]() {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_wave_barrier();
    };
    auto mm = [&](int tap, const s2b_u4 (&fa)[CB], const s2b_u2 (&fl)[CB]) {
        const int ky = tap / 3, kx = tap - 3 * ky;
        const int so = ky * S2B_ROW + (kx == 0 ? 0 : (kx == 1 ? 9 : 1));
        const s2b_u4 hm = *reinterpret_cast<const s2b_u4*>(R_hm + 4 * so);
        const s2b_u2 lo = *reinterpret_cast<const s2b_u2*>(R_lo + 2 * so);
        const s2b_u4 mh = {hm.z, hm.w, hm.x, hm.y}, lh = {lo.x, lo.y, hm.x, hm.y};
#pragma unroll
        for (int x = 0; x < CB; ++x) {
            const s2b_u4 a_hl = {fa[x].x, fa[x].y, fl[x].x, fl[x].y};
            acc[x] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(s2b_bf16x8, fa[x]), __builtin_bit_cast(s2b_bf16x8, hm), acc[x], 0, 0, 0);
            acc[x] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(s2b_bf16x8, fa[x]), __builtin_bit_cast(s2b_bf16x8, mh), acc[x], 0, 0, 0);
            acc[x] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(s2b_bf16x8, a_hl), __builtin_bit_cast(s2b_bf16x8, lh), acc[x], 0, 0, 0);
        }
    };

    XRegs xr;
    s2b_u4 fa[3][CB];            // filters of tap t in set t % 3
    s2b_u2 fl[3][CB];
    if (c_begin < c_end) {
        load_x(c_begin, xr);
        load_f(c_begin, 0, fa[0], fl[0]);
        load_f(c_begin, 1, fa[1], fl[1]);
    }
    for (int c = c_begin; c < c_end; ++c) {
        stage(xr);
        wave_fence();
        const bool more = c + 1 < c_end;
        if (more) load_x(c + 1, xr);
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            if (tap + 2 < 9) load_f(c, tap + 2, fa[(tap + 2) % 3], fl[(tap + 2) % 3]);
            else if (more) load_f(c + 1, tap + 2 - 9, fa[(tap + 2) % 3], fl[(tap + 2) % 3]);
            mm(tap, fa[tap % 3], fl[tap % 3]);
        }
        wave_fence();
    }

    // ---- epilogue: bias + per-sample channel bias + residual, NCHW stores; GroupNorm partials (one slot per tile)
    const int oy = oy0 + (l31 >> 3), ox = ox0 + (l31 & 7);
    const bool pv = oy < Ho && ox < Wo;
    const __amdgpu_buffer_rsrc_t rso = __builtin_amdgcn_make_buffer_rsrc(p.out + (size_t)b * p.Cout * HWo, 0, -1, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsr = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(p.residual ? p.residual + (size_t)b * p.Cout * HWo : p.out), 0, -1, 0x00020000);
    const unsigned o_voff = 4u * (unsigned)((4 * half) * HWo + (pv ? oy * Wo + ox : 0));
    const float cnt = (float)(min(S2B_TH, Ho - oy0) * min(S2B_TW, Wo - ox0));      // pixels of the tile inside the image
    const float inv_cnt = 1.0f / cnt;
    // eight accumulator rows rb .. rb + 7 of channel block x; value(rr) is the contraction's result of row rb + rr
    auto finish = [&](int x, int rb, auto value) {
        float add[8], res[8];
#pragma unroll
        for (int rr = 0; rr < 8; ++rr) {                    // (all residual / bias operands are requested before the first is used)
            const int r = rb + rr;
            const int cs = co0 + 32 * x + 8 * (r >> 2) + (r & 3);          // + 4 half: the lane's part
            const int col = cs + 4 * half;
            add[rr] = 0.0f;
            if (p.bias) add[rr] += p.bias[col];
            if (p.chan_bias) add[rr] += p.chan_bias[(size_t)b * p.chan_bias_stride + col];
            res[rr] = 0.0f;
            if (p.residual && pv) res[rr] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsr, o_voff, 4u * (unsigned)(cs * HWo), 0));
        }
#pragma unroll
        for (int rr = 0; rr < 8; ++rr) {
            const int r = rb + rr;
            const int cs = co0 + 32 * x + 8 * (r >> 2) + (r & 3);
            float v = value(rr) + add[rr] + res[rr];
            if (p.relu) v = fmaxf(v, 0.0f);
            if (pv) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), rso, o_voff, 4u * (unsigned)(cs * HWo), 0);
            if (p.stats) {          // (count, sum, sum of squared deviations from the tile's own mean) over the tile's pixels
                const int co = cs + 4 * half;
                const float s1 = s2b_half_wave_sum(pv ? v : 0.0f);
                const float d = pv ? v - s1 * inv_cnt : 0.0f;
                float dd;                  // the ROUNDED square (conv_pointwise_bf3.hip)
                asm volatile("v_mul_f32 %0, %1, %1" : "=v"(dd) : "v"(d));
                const float q = s2b_half_wave_sum(dd);
                if (l31 == 0)
                    reinterpret_cast<float4*>(p.stats)[((size_t)b * p.Cout + co) * ntiles + tile] = make_float4(cnt, s1, q, 0.0f);
            }
        }
    };
    {
        // the four partial tiles through LDS (over the patches: every wave is done with its own first); wave w sums and stores
        // accumulator rows 8 (w & 1) .. + 7 of channel block w >> 1
        float* const P_lds = smem;                                  // [4 waves][32 accumulator registers][64 lanes]
        __syncthreads();
#pragma unroll
        for (int x = 0; x < CB; ++x)
#pragma unroll
            for (int r = 0; r < 16; ++r) P_lds[((wave_u * 2 + x) * 16 + r) * 64 + lane] = acc[x][r];
        __syncthreads();
        const int x = wave_u >> 1, rb = 8 * (wave_u & 1);
        finish(x, rb, [&](int rr) {
            float part[S2B_WAVES];
#pragma unroll
            for (int k = 0; k < S2B_WAVES; ++k) part[k] = P_lds[((k * 2 + x) * 16 + rb + rr) * 64 + lane];
            return ((part[0] + part[1]) + part[2]) + part[3];
        });
    }
}

__global__ void conv_s2_pack_kernel(const float* __restrict__ w, int Cout, int Cin, int cout_pad, size_t total, unsigned* __restrict__ out) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x)
        conv_s2_pack_bf3_elem(i, w, Cout, Cin, cout_pad, out);
}

int64_t conv_s2_packed_floats(int Cout, int Cin) { return (int64_t)(round_up(Cin, 8) / 8) * 9 * (conv_cout_pad(Cout) / 64) * 768; }

int launch_conv_s2_pack(sisic_ctx*, const float* w, int Cout, int Cin, float* out, hipStream_t s) {
    const size_t total = (size_t)conv_s2_packed_floats(Cout, Cin);
    const int blocks = (int)std::min<size_t>((total + 255) / 256, 4096);
    hipLaunchKernelGGL(conv_s2_pack_kernel, dim3(blocks), dim3(256), 0, s, w, Cout, Cin, conv_cout_pad(Cout), total, reinterpret_cast<unsigned*>(out));
    SISIC_HIP(hipGetLastError());
    return SISIC_OK;
}

// The arguments this kernel takes: a plain 3x3 stride-2 convolution of one input with a split filter at hand, whole 8-channel
// chunks and 64-channel tiles, 32-bit byte offsets inside an image of either tensor and inside the filter
bool conv_s2_bf3_applicable(const sisic_conv_args& a) {
    if (a.ksize != 3 || a.stride != 2 || a.upsample || a.gn_scale || a.c1 != 0 || a.in1 || !a.w_winograd) return false;
    if (a.c0 % 8 != 0 || a.Cout % 64 != 0) return false;
    const int Ho = (a.Hin + 1) / 2, Wo = (a.Win + 1) / 2;
    if (4.0 * a.c0 * a.Hin * a.Win >= 2147483648.0 || 4.0 * a.Cout * Ho * Wo >= 2147483648.0 ||
        4.0 * conv_s2_packed_floats(a.Cout, a.c0) >= 2147483648.0) return false;
    return true;
}
int conv_s2_bf3_stats_slots(const sisic_conv_args& a) { return cdiv((a.Hin + 1) / 2, S2B_TH) * cdiv((a.Win + 1) / 2, S2B_TW); }

int launch_conv_s2_bf3(sisic_ctx* ctx, const sisic_conv_args& a, const ConvPlan& plan, hipStream_t s) {
    S2bParams p{};
    p.in = a.in0; p.Cin = a.c0; p.B = a.B; p.H = a.Hin; p.W = a.Win;
    p.Hout = plan.Hout; p.Wout = plan.Wout;
    p.wb = a.w_winograd; p.n_co64 = a.Cout / 64;
    p.bias = a.bias; p.Cout = a.Cout;
    p.chan_bias = a.chan_bias; p.chan_bias_stride = a.chan_bias_stride; p.residual = a.residual; p.relu = a.relu;
    p.out = a.out; p.stats = a.stats_out;
    p.tiles_x = cdiv(p.Wout, S2B_TW); p.tiles_y = cdiv(p.Hout, S2B_TH);
    p.n_co_items = a.Cout / 64; p.nchunks = a.c0 / 8;
    const int64_t nitems = (int64_t)p.B * p.tiles_x * p.tiles_y * p.n_co_items;
    SISIC_REQUIRE(nitems > 0 && nitems < (int64_t(1) << 31), "conv2d(stride-2 bf16x3): grid too large");
    p.nwg = (int)nitems;
    const size_t lds = sizeof(float) * (size_t)(S2B_WAVES * S2B_WAVE_DWORDS);       // (the partials, 32 KB, lie over the patches)
    static_assert(S2B_WAVES * S2B_WAVE_DWORDS >= S2B_WAVES * 32 * 64, "partials must fit over the patches");
    static std::atomic<uint64_t> opt{0};
    SISIC_TRY(ensure_dynamic_lds(ctx, reinterpret_cast<const void*>(conv_s2b_kernel), (int)lds, opt));
    hipLaunchKernelGGL(conv_s2b_kernel, dim3(p.nwg), dim3(64 * S2B_WAVES), lds, s, p);
    SISIC_HIP(hipGetLastError());
    return SISIC_OK;
}

}  // namespace sisic
