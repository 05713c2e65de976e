// attention_wide.hip -- multi-head self-attention at 32 and 64 channels per head: forward, and a backward pass tiled over keys.
//
// Same operands as attention.hip: qkv is [B, 3C, N] with the token index contiguous (q channels, then k, then v; head h owns
// channels h*d .. h*d+d-1 of each), out and dO are [B, C, N].  At these widths every product belongs on the matrix pipe, and
// all of them are exact fp32 products: v_mfma_f32_32x32x2_f32, whose result is bit for bit a k-ordered fmaf chain.
//
// Two building blocks, both over a [dim][token] LDS image of 64 tokens of one head (rows padded by four floats):
//   aw_dot_tile   X^T tile = img^T . R: the image's 32 tokens are the A operand (lane l: token l & 31, dim 2s + (l >> 5) in
//                 k-step s, one conflict-free ds_read_b32), R is a register-held [dim][32 entities] operand (lane l: entity
//                 l & 31, the same dim).  d/2 MFMAs.  The result has the ENTITY on the lane and the image's tokens in the 16
//                 accumulator registers: register r is token (r & 3) + 8 (r >> 2) + 4 (l >> 5).  With K as the image and q as R
//                 this is the "swapped" score tile S^T = K^T Q of attention.hip: a query's softmax row is register-local plus
//                 one exchange between the lane halves.
//   aw_acc_tile   Y^T[dim x entity] += img[dim x 2 tokens] . X^T[2 tokens x entity], for the token pairs {t_r, t_r + 4}: register
//                 r of such a tile IS the B operand of v_mfma_f32_32x32x2_f32 for that pair (B[k = l >> 5][j = l & 31]), so the
//                 probabilities go back into the matrix pipe with no shuffle and no LDS.  A is img[dim l & 31][token t_r + 4 (l >> 5)]:
//                 one ds_read_b128 along the token feeds four consecutive r.  16 MFMAs per 32 tokens and 32 dims.
// The vector-ALU form of P.V that attention.hip uses at d = 8 would cost d/4 broadcast ds_read_b128 per key here -- the traffic
// DESIGN.md section 8 item 4 names as the bound at d = 8, times 4 or 8.
//
// Forward (attention_wide_kernel): a wave owns 32 queries, a workgroup 128; S^T = aw_dot_tile(K, q), online softmax in fp32 with
// d^-1/2 * log2(e) folded into q, O^T += aw_acc_tile(V, P^T), the per-query rescale is per lane.  One launch form: a sample's
// bits depend on nothing but its own operands.  No allocation, no synchronisation: capturable.
//
// Backward (two launches, no atomics, every output row has one owner):
//   attention_wide_bwd_q_kernel   a wave owns 32 queries.  Sweep 1 over the keys: S^T and G^T = V dO^T, m_i, l_i and
//       a_i = sum_j e_ij g_ij online (the per-tile sums in fp32, the running sums across tiles in double: attention_bwd_kernel's
//       reasoning), D_i = a_i / l_i from the pass's own P_ij.  Sweep 2: the same tiles again (same code, same bits),
//       dS^T = P (G - D), dQ^T += aw_acc_tile(K, dS^T).  m_i, 1/l_i, D_i go to the stream's row-statistics scratch.
//   attention_wide_bwd_kv_kernel  a wave owns 32 keys (entity = key); the images are scale*q and dO of 64 queries.  The score
//       tile has the same k-ordered chain over the same (scale q_id) k_jd products as the query-owned pass -- ONE definition of
//       the score: P_ij is normalised by the very scores that produced m_i and l_i.  dV^T += aw_acc_tile(dO, P),
//       dK^T += aw_acc_tile(scale q, dS).
// 64 tokens of a head in LDS at a time: no LDS-derived token limit (train.h: ATTN_BWD_TILED_MAX_TOKENS).
//
// Algorithmic FLOPs: forward 4*B*C*N*N, backward 14*B*C*N*N (S and G twice per pass pair plus dQ, dK, dV).
#include <cmath>

#include "common.h"
#include "poison_switch.h"
#include "train.h"

namespace sisic {

typedef float aw_f32x16 __attribute__((ext_vector_type(16)));

constexpr int AW_KB = 64;               // tokens per LDS image
constexpr int AW_LD = AW_KB + 4;        // floats per image row: 16-byte aligned rows, ds_read_b128 of 16 lanes on 64 banks
constexpr int AW_WAVES = 4;
constexpr int AW_THREADS = 64 * AW_WAVES;
constexpr int AW_WG = 32 * AW_WAVES;    // queries (or keys) a workgroup owns

// tokens t0 .. t0 + 63 of a head's d rows (row stride N) into a [dim][token] image, times mul; zero past the last token.
// Every load is issued, at a clamped address, and the select follows: a load under the condition is a branch and a full
// vmcnt(0) wait per element, D / 4 dependent round trips per image instead of one.
template <int D>
__device__ __forceinline__ void aw_stage(float* __restrict__ img, const float* __restrict__ src, int N, int t0, int tid, float mul) {
    constexpr int PER = D * AW_KB / AW_THREADS;
    const int t = tid % AW_KB, d0 = tid / AW_KB;        // thread: one token, dims d0, d0 + 4, ...
    const int tok = t0 + t;
    const float* p = src + min(tok, N - 1);
    float v[PER];
#pragma unroll
    for (int i = 0; i < PER; ++i) v[i] = p[(size_t)(d0 + i * (AW_THREADS / AW_KB)) * N];
#pragma unroll
    for (int i = 0; i < PER; ++i) img[(d0 + i * (AW_THREADS / AW_KB)) * AW_LD + t] = tok < N ? v[i] * mul : 0.0f;
}

// the register operand of entity e: reg[s] = src[dim 2s + half][e] * mul, zero for e >= N (loads clamped, as above)
template <int D>
__device__ __forceinline__ void aw_load_entity(float (&reg)[D / 2], const float* __restrict__ src, int N, int e, int half, float mul) {
    const float* p = src + min(e, N - 1);
#pragma unroll
    for (int s = 0; s < D / 2; ++s) reg[s] = p[(size_t)(2 * s + half) * N];
#pragma unroll
    for (int s = 0; s < D / 2; ++s) reg[s] = e < N ? reg[s] * mul : 0.0f;
}

template <int D>
__device__ __forceinline__ aw_f32x16 aw_dot_tile(const float* __restrict__ img, int t, int half, const float (&reg)[D / 2]) {
    aw_f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
#pragma unroll
    for (int s = 0; s < D / 2; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(img[(2 * s + half) * AW_LD + t], reg[s], acc, 0, 0, 0);
    return acc;
}

template <int D>
__device__ __forceinline__ void aw_acc_tile(aw_f32x16 (&acc)[D / 32], const float* __restrict__ img, int t0, int half, int l31,
                                            const aw_f32x16& x) {
#pragma unroll
    for (int db = 0; db < D / 32; ++db) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float4 a = *reinterpret_cast<const float4*>(&img[(l31 + 32 * db) * AW_LD + t0 + 8 * g + 4 * half]);
            acc[db] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, x[4 * g + 0], acc[db], 0, 0, 0);
            acc[db] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, x[4 * g + 1], acc[db], 0, 0, 0);
            acc[db] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, x[4 * g + 2], acc[db], 0, 0, 0);
            acc[db] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, x[4 * g + 3], acc[db], 0, 0, 0);
        }
    }
}

// acc^T [dim x entity] times mul to dst rows (row stride N), entity e < N only
template <int D>
__device__ __forceinline__ void aw_store(float* __restrict__ dst, int N, int e, int half, const aw_f32x16 (&acc)[D / 32], float mul) {
    if (e >= N) return;
#pragma unroll
    for (int db = 0; db < D / 32; ++db)
#pragma unroll
        for (int r = 0; r < 16; ++r) dst[(size_t)(32 * db + (r & 3) + 8 * (r >> 2) + 4 * half) * N + e] = acc[db][r] * mul;
}

// own value and the other lane half's (lane l and l ^ 32): v_permlane32_swap; op(own, other) of a commutative op has the same
// bits in both halves
__device__ __forceinline__ float aw_other_max(float x) {
    const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return fmaxf(__uint_as_float(sw[0]), __uint_as_float(sw[1]));
}
__device__ __forceinline__ float aw_other_sum(float x) {
    const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return __uint_as_float(sw[0]) + __uint_as_float(sw[1]);
}

// token (of the image) that accumulator register r of a tile holds in lane half `half`
__device__ __forceinline__ constexpr int aw_row(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

// ================================================================ forward
template <int D>
__global__ void __launch_bounds__(AW_THREADS)
attention_wide_kernel(const float* __restrict__ qkv, float* __restrict__ out, int C, int N, int heads, int q_blocks, float scale) {
    __shared__ __attribute__((aligned(16))) float Ks[D * AW_LD];
    __shared__ __attribute__((aligned(16))) float Vs[D * AW_LD];

    int blk = blockIdx.x;
    const int qb = blk % q_blocks;
    blk /= q_blocks;
    const int head = blk % heads;
    const int b = blk / heads;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int half = lane >> 5, l31 = lane & 31;
    const int q0 = qb * AW_WG + wave * 32;
    const int q = q0 + l31;
    const bool wave_active = q0 < N;      // wave-uniform

    const float* Qp = qkv + ((size_t)b * 3 * C + (size_t)head * D) * N;
    const float* Kp = Qp + (size_t)C * N;
    const float* Vp = Kp + (size_t)C * N;

    float qreg[D / 2];                    // d^-1/2 * log2(e) folded in: p = 2^(s - m) is a bare v_exp_f32
    aw_load_entity<D>(qreg, Qp, N, q, half, scale);

    aw_f32x16 o[D / 32];
#pragma unroll
    for (int db = 0; db < D / 32; ++db)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[db][r] = 0.0f;
    float m_run = -INFINITY, l_part = 0.0f;   // l_part: this lane half's keys

    for (int kb0 = 0; kb0 < N; kb0 += AW_KB) {
        __syncthreads();
        aw_stage<D>(Ks, Kp, N, kb0, tid, 1.0f);
        aw_stage<D>(Vs, Vp, N, kb0, tid, 1.0f);
        __syncthreads();
        if (!wave_active) continue;
        const int nk = min(AW_KB, N - kb0);
#pragma unroll 1
        for (int kt = 0; kt * 32 < nk; ++kt) {
            aw_f32x16 S = aw_dot_tile<D>(Ks, kt * 32 + l31, half, qreg);
            if (kt * 32 + 32 > nk) {      // the tile reaches past the last key
#pragma unroll
                for (int r = 0; r < 16; ++r) S[r] = (kt * 32 + aw_row(r, half) < nk) ? S[r] : -INFINITY;
            }
            float tmax = -INFINITY;
#pragma unroll
            for (int r = 0; r < 16; ++r) tmax = fmaxf(tmax, S[r]);
            tmax = aw_other_max(tmax);
            const float m_new = fmaxf(m_run, tmax);      // finite: every tile holds at least one key
            const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);     // first tile: 2^(-inf) = 0
            l_part *= alpha;
#pragma unroll
            for (int db = 0; db < D / 32; ++db) o[db] *= alpha;
            m_run = m_new;
            float sum = 0.0f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                S[r] = __builtin_amdgcn_exp2f(S[r] - m_new);               // masked keys: 2^(-inf) = 0
                sum += S[r];
            }
            l_part += sum;
            aw_acc_tile<D>(o, Vs, kt * 32, half, l31, S);
        }
    }

    if (wave_active) {
        const float inv = 1.0f / aw_other_sum(l_part);
        aw_store<D>(out + ((size_t)b * C + (size_t)head * D) * N, N, q, half, o, inv);
    }
}

// ================================================================ backward, query-owned: row statistics and dQ
// stats: [B * heads][3][N]: m_i, 1 / l_i, D_i
template <int D>
__global__ void __launch_bounds__(AW_THREADS)
attention_wide_bwd_q_kernel(const float* __restrict__ qkv, const float* __restrict__ dO, float* __restrict__ dqkv,
                            float* __restrict__ stats, int C, int N, int heads, int q_blocks, float scale) {
    __shared__ __attribute__((aligned(16))) float Ks[D * AW_LD];
    __shared__ __attribute__((aligned(16))) float Vs[D * AW_LD];

    int blk = blockIdx.x;
    const int qb = blk % q_blocks;
    blk /= q_blocks;
    const int head = blk % heads;
    const int b = blk / heads;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int half = lane >> 5, l31 = lane & 31;
    const int q0 = qb * AW_WG + wave * 32;
    const int q = q0 + l31;
    const bool wave_active = q0 < N;

    const size_t qoff = ((size_t)b * 3 * C + (size_t)head * D) * N;
    const float* Qp = qkv + qoff;
    const float* Kp = Qp + (size_t)C * N;
    const float* Vp = Kp + (size_t)C * N;
    const float* Gp = dO + ((size_t)b * C + (size_t)head * D) * N;

    float qreg[D / 2], greg[D / 2];
    aw_load_entity<D>(qreg, Qp, N, q, half, scale);      // scale q: the one definition of the score
    aw_load_entity<D>(greg, Gp, N, q, half, 1.0f);

    // ---- sweep 1: m, l = sum_j exp(s_ij - m), a = sum_j exp(s_ij - m) (dO_i . v_j)
    float m = -INFINITY;
    double l = 0.0, a = 0.0;
    for (int kb0 = 0; kb0 < N; kb0 += AW_KB) {
        __syncthreads();
        aw_stage<D>(Ks, Kp, N, kb0, tid, 1.0f);
        aw_stage<D>(Vs, Vp, N, kb0, tid, 1.0f);
        __syncthreads();
        if (!wave_active) continue;
        const int nk = min(AW_KB, N - kb0);
#pragma unroll 1
        for (int kt = 0; kt * 32 < nk; ++kt) {
            aw_f32x16 S = aw_dot_tile<D>(Ks, kt * 32 + l31, half, qreg);
            const aw_f32x16 G = aw_dot_tile<D>(Vs, kt * 32 + l31, half, greg);
            if (kt * 32 + 32 > nk) {
#pragma unroll
                for (int r = 0; r < 16; ++r) S[r] = (kt * 32 + aw_row(r, half) < nk) ? S[r] : -INFINITY;
            }
            float tmax = -INFINITY;
#pragma unroll
            for (int r = 0; r < 16; ++r) tmax = fmaxf(tmax, S[r]);
            tmax = aw_other_max(tmax);
            const float mn = fmaxf(m, tmax);
            const float resc = __expf(m - mn);
            float tl = 0.0f, ta = 0.0f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float e = __expf(S[r] - mn);       // a masked key: exp(-inf) = 0 (its G is 0: V is staged as zero there)
                tl += e;
                ta += e * G[r];
            }
            tl = aw_other_sum(tl);                       // both lane halves carry the whole row's sums, with equal bits
            ta = aw_other_sum(ta);
            l = l * (double)resc + (double)tl;
            a = a * (double)resc + (double)ta;
            m = mn;
        }
    }
    const float il = (float)(1.0 / l);
    const float Dv = (float)(a / l);
    if (wave_active && half == 0 && q < N) {
        float* st = stats + ((size_t)b * heads + head) * 3 * N;
        st[q] = m; st[(size_t)N + q] = il; st[2 * (size_t)N + q] = Dv;
    }

    // ---- sweep 2: dQ_i = scale * sum_j P_ij (dO_i . v_j - D_i) k_j
    aw_f32x16 dq[D / 32];
#pragma unroll
    for (int db = 0; db < D / 32; ++db)
#pragma unroll
        for (int r = 0; r < 16; ++r) dq[db][r] = 0.0f;
    for (int kb0 = 0; kb0 < N; kb0 += AW_KB) {
        __syncthreads();
        aw_stage<D>(Ks, Kp, N, kb0, tid, 1.0f);
        aw_stage<D>(Vs, Vp, N, kb0, tid, 1.0f);
        __syncthreads();
        if (!wave_active) continue;
        const int nk = min(AW_KB, N - kb0);
#pragma unroll 1
        for (int kt = 0; kt * 32 < nk; ++kt) {
            aw_f32x16 S = aw_dot_tile<D>(Ks, kt * 32 + l31, half, qreg);
            const aw_f32x16 G = aw_dot_tile<D>(Vs, kt * 32 + l31, half, greg);
            const bool tail = kt * 32 + 32 > nk;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float p = __expf(S[r] - m) * il;
                const float ds = p * (G[r] - Dv);
                S[r] = (tail && kt * 32 + aw_row(r, half) >= nk) ? 0.0f : ds;
            }
            aw_acc_tile<D>(dq, Ks, kt * 32, half, l31, S);
        }
    }
    if (wave_active) aw_store<D>(dqkv + qoff, N, q, half, dq, scale);
}

// ================================================================ backward, key-owned: dK and dV
template <int D>
__global__ void __launch_bounds__(AW_THREADS)
attention_wide_bwd_kv_kernel(const float* __restrict__ qkv, const float* __restrict__ dO, float* __restrict__ dqkv,
                             const float* __restrict__ stats, int C, int N, int heads, int k_blocks, float scale) {
    __shared__ __attribute__((aligned(16))) float Qs[D * AW_LD];      // scale * q
    __shared__ __attribute__((aligned(16))) float Gs[D * AW_LD];      // dO
    __shared__ float St[3 * AW_KB];                                    // m_i, 1 / l_i, D_i of the image's queries

    int blk = blockIdx.x;
    const int kb = blk % k_blocks;
    blk /= k_blocks;
    const int head = blk % heads;
    const int b = blk / heads;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int half = lane >> 5, l31 = lane & 31;
    const int k0 = kb * AW_WG + wave * 32;
    const int key = k0 + l31;
    const bool wave_active = k0 < N;

    const size_t qoff = ((size_t)b * 3 * C + (size_t)head * D) * N;
    const size_t koff = qoff + (size_t)C * N, voff = koff + (size_t)C * N;
    const float* Qp = qkv + qoff;
    const float* Gp = dO + ((size_t)b * C + (size_t)head * D) * N;
    const float* st = stats + ((size_t)b * heads + head) * 3 * N;

    float kreg[D / 2], vreg[D / 2];
    aw_load_entity<D>(kreg, qkv + koff, N, key, half, 1.0f);
    aw_load_entity<D>(vreg, qkv + voff, N, key, half, 1.0f);

    aw_f32x16 dk[D / 32], dv[D / 32];
#pragma unroll
    for (int db = 0; db < D / 32; ++db)
#pragma unroll
        for (int r = 0; r < 16; ++r) { dk[db][r] = 0.0f; dv[db][r] = 0.0f; }

    for (int qb0 = 0; qb0 < N; qb0 += AW_KB) {
        __syncthreads();
        aw_stage<D>(Qs, Qp, N, qb0, tid, scale);
        aw_stage<D>(Gs, Gp, N, qb0, tid, 1.0f);
        if (tid < 3 * AW_KB) {            // a query past the last: m = 0, 1 / l = 0, D = 0 -- its P and dS are exactly zero
            const int which = tid / AW_KB, t = tid % AW_KB;
            St[tid] = qb0 + t < N ? st[(size_t)which * N + qb0 + t] : 0.0f;
        }
        __syncthreads();
        if (!wave_active) continue;
        const int nq = min(AW_KB, N - qb0);
#pragma unroll 1
        for (int qt = 0; qt * 32 < nq; ++qt) {
            // register r: query qt * 32 + aw_row(r, half); lane: key.  The same fma chain over the same products as the
            // query-owned pass (a b = b a): the same score bits
            aw_f32x16 S = aw_dot_tile<D>(Qs, qt * 32 + l31, half, kreg);
            aw_f32x16 G = aw_dot_tile<D>(Gs, qt * 32 + l31, half, vreg);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int qi = qt * 32 + aw_row(r, half);
                const float p = __expf(S[r] - St[qi]) * St[AW_KB + qi];
                G[r] = p * (G[r] - St[2 * AW_KB + qi]);      // dS
                S[r] = p;
            }
            aw_acc_tile<D>(dv, Gs, qt * 32, half, l31, S);
            aw_acc_tile<D>(dk, Qs, qt * 32, half, l31, G);   // Qs carries the scale
        }
    }
    if (wave_active) {
        aw_store<D>(dqkv + koff, N, key, half, dk, 1.0f);
        aw_store<D>(dqkv + voff, N, key, half, dv, 1.0f);
    }
}

// ================================================================ launchers
static int aw_check(const char* what, int B, int C, int N, int head_dim, int64_t* grid, int* blocks) {
    SISIC_REQUIRE(head_dim == 32 || head_dim == 64, "%s: head_dim %d unsupported (8, 32 and 64 have kernels)", what, head_dim);
    SISIC_REQUIRE(B > 0 && N > 0 && C > 0, "%s: bad shape B=%d C=%d N=%d", what, B, C, N);
    SISIC_REQUIRE(C % head_dim == 0, "%s: C=%d is no multiple of head_dim %d", what, C, head_dim);
    *blocks = cdiv(N, AW_WG);
    *grid = (int64_t)B * (C / head_dim) * *blocks;
    SISIC_REQUIRE(*grid < (int64_t(1) << 31), "%s: grid too large", what);
    return SISIC_OK;
}

int launch_attention_wide(sisic_ctx* ctx, const float* qkv, float* out, int B, int C, int N, int head_dim, hipStream_t s) {
    SISIC_REQUIRE(qkv && out, "attention: null tensor");
    int64_t grid = 0;
    int q_blocks = 0;
    SISIC_TRY(aw_check("attention", B, C, N, head_dim, &grid, &q_blocks));
    const int heads = C / head_dim;
    ProfileScope prof(ctx, s, PK_ATTN, 16.0 * B * C * N, 4.0 * B * C * double(N) * N);
    const float scale = 1.4426950408889634f / sqrtf((float)head_dim);     // head_dim^-1/2 * log2(e)
    if (head_dim == 32)
        hipLaunchKernelGGL(attention_wide_kernel<32>, dim3((unsigned)grid), dim3(AW_THREADS), 0, s, qkv, out, C, N, heads, q_blocks, scale);
    else
        hipLaunchKernelGGL(attention_wide_kernel<64>, dim3((unsigned)grid), dim3(AW_THREADS), 0, s, qkv, out, C, N, heads, q_blocks, scale);
    SISIC_HIP(hipGetLastError());
    return SISIC_OK;
}

// The stream's row-statistics scratch, grown on demand (the K-split scratch of conv_winograd.hip is the model: a growth waits
// for the stream, and captured graphs that might hold the old address are rebuilt).
static int attn_rows_scratch(sisic_ctx* ctx, hipStream_t s, size_t floats, float** ptr) {
    std::lock_guard<std::mutex> lock(ctx->attn_rows_mutex);
    auto& buf = ctx->attn_rows[s];
    if (buf.floats < floats) {
        SISIC_HIP(hipStreamSynchronize(s));          // earlier launches on this stream may still read the old buffer
        if (buf.p) SISIC_HIP(hipFree(buf.p));
        buf.p = nullptr; buf.floats = 0;
        SISIC_HIP(hipMalloc(reinterpret_cast<void**>(&buf.p), floats * sizeof(float)));
        if (poison_alloc()) {                        // SISIC_POISON_ALLOC=1: a row no workgroup writes is NaN
            SISIC_HIP(hipMemset(buf.p, 0xFF, floats * sizeof(float)));
            SISIC_HIP(hipDeviceSynchronize());
        }
        buf.floats = floats;
        ctx->scratch_generation.fetch_add(1);
    }
    *ptr = buf.p;
    return SISIC_OK;
}

int launch_attention_bwd_wide(sisic_ctx* ctx, const float* qkv, const float* dO, float* dqkv, int B, int C, int N, int head_dim,
                              hipStream_t s) {
    SISIC_REQUIRE(qkv && dO && dqkv, "attention_bwd: null tensor");
    int64_t grid = 0;
    int blocks = 0;
    SISIC_TRY(aw_check("attention_bwd", B, C, N, head_dim, &grid, &blocks));
    SISIC_REQUIRE(N <= ATTN_BWD_TILED_MAX_TOKENS, "attention_bwd: %d tokens are more than the tiled backward pass takes (max %d)", N,
                  ATTN_BWD_TILED_MAX_TOKENS);
    const int heads = C / head_dim;
    float* stats = nullptr;
    SISIC_TRY(attn_rows_scratch(ctx, s, (size_t)B * heads * 3 * N, &stats));
    ProfileScope prof(ctx, s, PK_ATTN, 32.0 * B * C * N, 14.0 * B * C * double(N) * N);
    const float scale = 1.0f / sqrtf((float)head_dim);
    if (head_dim == 32) {
        hipLaunchKernelGGL(attention_wide_bwd_q_kernel<32>, dim3((unsigned)grid), dim3(AW_THREADS), 0, s, qkv, dO, dqkv, stats, C, N, heads, blocks, scale);
        hipLaunchKernelGGL(attention_wide_bwd_kv_kernel<32>, dim3((unsigned)grid), dim3(AW_THREADS), 0, s, qkv, dO, dqkv, stats, C, N, heads, blocks, scale);
    } else {
        hipLaunchKernelGGL(attention_wide_bwd_q_kernel<64>, dim3((unsigned)grid), dim3(AW_THREADS), 0, s, qkv, dO, dqkv, stats, C, N, heads, blocks, scale);
        hipLaunchKernelGGL(attention_wide_bwd_kv_kernel<64>, dim3((unsigned)grid), dim3(AW_THREADS), 0, s, qkv, dO, dqkv, stats, C, N, heads, blocks, scale);
    }
    SISIC_HIP(hipGetLastError());
    return SISIC_OK;
}

}  // namespace sisic
