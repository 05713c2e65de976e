// eval_kernels.hip -- the pairwise arithmetic behind synt_isic_amd/evaluate.py (include/sisic.h, "Evaluation of generated sets"):
//   * gram_kernel: out = f(A' B'^T) on v_mfma_f32_32x32x2_f32, A' = A - shift_a and B' = B - shift_b formed while the operand is
//     staged, epilogues DOT / SQDIST / POLY3; the transposed loader gives A'^T A' from the [n, d] layout (contract_rows)
//   * col_means_kernel, matrix_sum_kernel: fixed-order double sums (no atomics: two calls give equal bits)
//   * rows_topk_kernel: the k <= 8 smallest of a row, exact, ties to the lower column
//   * pair_sqdist_kernel: sum_c (A[i, c] - B[idx[i, j], c])^2 in double, stored as fp32
// Every store is a vector store.  Nothing here allocates.
#include "common.h"

namespace sisic {

namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;

// ---- gram --------------------------------------------------------------------------------------------------------------------
// One workgroup of 4 waves owns a 128 x 128 tile of the output; the waves sit 2 x 2, each on 64 x 64 = 2 x 2 MFMA tiles of
// 32 x 32 (64 accumulator registers).  A K step is 32.  Both operand tiles lie in LDS as [128 rows][32 k] with a row stride of 34
// floats: lane l of an MFMA operand read takes the two consecutive k of row l & 31 at k offset 2 (l >> 5) as one 8-byte read, and
// 34 (l & 31) + 2 (l >> 5) runs over all 64 banks once.  (So the k of one 32x32x2 instruction are kk + {0, 2} and kk + {1, 3}
// instead of kk + {0, 1} and kk + {2, 3}: both operands use the same order, and the order is fixed.)  Global loads are 16 bytes
// per lane, 8 lanes along k per row (128 contiguous bytes), issued for the next step before the MFMAs of the current one; an
// operand whose base, leading dimension or shift does not allow 16-byte loads, and the edges, go element by element.
// What bounds the tile: 64 accumulators and 2 * 128 * 34 * 4 = 34 KB of LDS leave room for four workgroups per CU; a K step
// holds 64 MFMAs (4096 cycles) per wave between two barriers against 16 LDS reads and 8 global loads per lane.
constexpr int GT = 128;          // tile edge, both ways
constexpr int GK = 32;           // K step
constexpr int GLD = GK + 2;      // LDS row stride (floats)
constexpr int GP = 4;            // float4 loads per lane, operand and step: 128 * 32 / (256 * 4)

// row-major operand: element [i][k] at p[i * ld + k]; pass q of thread t stages row (t >> 3) + 32 q, k (t & 7) * 4 .. + 4
__device__ __forceinline__ void load_rows(const float* __restrict__ p, int64_t ld, int rows, int K, int row0, int k0,
                                          const float* __restrict__ shift, bool vec, float4 v[GP]) {
    const int k = k0 + (threadIdx.x & 7) * 4;
#pragma unroll
    for (int q = 0; q < GP; ++q) {
        const int r = row0 + (threadIdx.x >> 3) + 32 * q;
        float4 x = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (r < rows) {
            const float* src = p + (int64_t)r * ld;
            if (vec && k + 3 < K) {
                x = *reinterpret_cast<const float4*>(src + k);
                if (shift) {
                    const float4 sh = *reinterpret_cast<const float4*>(shift + k);
                    x.x -= sh.x; x.y -= sh.y; x.z -= sh.z; x.w -= sh.w;
                }
            } else {
                if (k < K) x.x = src[k] - (shift ? shift[k] : 0.0f);
                if (k + 1 < K) x.y = src[k + 1] - (shift ? shift[k + 1] : 0.0f);
                if (k + 2 < K) x.z = src[k + 2] - (shift ? shift[k + 2] : 0.0f);
                if (k + 3 < K) x.w = src[k + 3] - (shift ? shift[k + 3] : 0.0f);
            }
        }
        v[q] = x;
    }
}

__device__ __forceinline__ void store_rows(float (*tile)[GLD], const float4 v[GP]) {
    const int kq = (threadIdx.x & 7) * 4;
#pragma unroll
    for (int q = 0; q < GP; ++q) {
        float* dst = &tile[(threadIdx.x >> 3) + 32 * q][kq];          // 8-byte aligned: 34 r + 4 j is even
        *reinterpret_cast<float2*>(dst) = make_float2(v[q].x, v[q].y);
        *reinterpret_cast<float2*>(dst + 2) = make_float2(v[q].z, v[q].w);
    }
}

// transposed operand (contract_rows): element [i][k] at p[k * ld + i]; pass q of thread t stages k (t >> 5) + 8 q,
// i (t & 31) * 4 .. + 4
__device__ __forceinline__ void load_cols(const float* __restrict__ p, int64_t ld, int cols, int K, int col0, int k0,
                                          const float* __restrict__ shift, bool vec, float4 v[GP]) {
    const int c = col0 + (threadIdx.x & 31) * 4;
    float4 sh = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (shift) {
        if (c < cols) sh.x = shift[c];
        if (c + 1 < cols) sh.y = shift[c + 1];
        if (c + 2 < cols) sh.z = shift[c + 2];
        if (c + 3 < cols) sh.w = shift[c + 3];
    }
#pragma unroll
    for (int q = 0; q < GP; ++q) {
        const int k = k0 + (threadIdx.x >> 5) + 8 * q;
        float4 x = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (k < K) {
            const float* src = p + (int64_t)k * ld;
            if (vec && c + 3 < cols) {
                x = *reinterpret_cast<const float4*>(src + c);
                x.x -= sh.x; x.y -= sh.y; x.z -= sh.z; x.w -= sh.w;
            } else {
                if (c < cols) x.x = src[c] - sh.x;
                if (c + 1 < cols) x.y = src[c + 1] - sh.y;
                if (c + 2 < cols) x.z = src[c + 2] - sh.z;
                if (c + 3 < cols) x.w = src[c + 3] - sh.w;
            }
        }
        v[q] = x;
    }
}

__device__ __forceinline__ void store_cols(float (*tile)[GLD], const float4 v[GP]) {
    const int cb = (threadIdx.x & 31) * 4;
#pragma unroll
    for (int q = 0; q < GP; ++q) {
        const int k = (threadIdx.x >> 5) + 8 * q;
        tile[cb][k] = v[q].x; tile[cb + 1][k] = v[q].y; tile[cb + 2][k] = v[q].z; tile[cb + 3][k] = v[q].w;
    }
}

// M x N output, contraction length K.  TRANS false: a is [M, K], b is [N, K]; true: a is [K, M], b is [K, N].
// MODE: SISIC_GRAM_*; kdiv: what POLY3 divides by (the contraction length); vec_a / vec_b: the operand takes 16-byte loads.
template <int MODE, bool TRANS>
__global__ void __launch_bounds__(256)
gram_kernel(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ shift_a,
            const float* __restrict__ shift_b, float* __restrict__ out, int M, int N, int K, int64_t lda, int64_t ldb,
            int64_t ldo, float kdiv, int vec_a, int vec_b) {
    __shared__ float As[GT][GLD];
    __shared__ float Bs[GT][GLD];
    __shared__ float norm_a[GT];
    __shared__ float norm_b[GT];

    const int m0 = blockIdx.y * GT, n0 = blockIdx.x * GT;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
    const int li = lane & 31, lk = lane >> 5;

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;

    float4 ra[GP], rb[GP];
    float sq_a[GP], sq_b[GP];      // SQDIST: this thread's share of |a'_row|^2 and |b'_row|^2 of its GP rows, in k order
#pragma unroll
    for (int q = 0; q < GP; ++q) sq_a[q] = sq_b[q] = 0.0f;
    if (TRANS) {
        load_cols(a, lda, M, K, m0, 0, shift_a, vec_a != 0, ra);
        load_cols(b, ldb, N, K, n0, 0, shift_b, vec_b != 0, rb);
    } else {
        load_rows(a, lda, M, K, m0, 0, shift_a, vec_a != 0, ra);
        load_rows(b, ldb, N, K, n0, 0, shift_b, vec_b != 0, rb);
    }
    for (int k0 = 0; k0 < K; k0 += GK) {
        if (TRANS) {
            store_cols(As, ra);
            store_cols(Bs, rb);
        } else {
            store_rows(As, ra);
            store_rows(Bs, rb);
            if (MODE == SISIC_GRAM_SQDIST) {
#pragma unroll
                for (int q = 0; q < GP; ++q) {
                    sq_a[q] = fmaf(ra[q].w, ra[q].w, fmaf(ra[q].z, ra[q].z, fmaf(ra[q].y, ra[q].y, fmaf(ra[q].x, ra[q].x, sq_a[q]))));
                    sq_b[q] = fmaf(rb[q].w, rb[q].w, fmaf(rb[q].z, rb[q].z, fmaf(rb[q].y, rb[q].y, fmaf(rb[q].x, rb[q].x, sq_b[q]))));
                }
            }
        }
        __syncthreads();
        if (k0 + GK < K) {
            if (TRANS) {
                load_cols(a, lda, M, K, m0, k0 + GK, shift_a, vec_a != 0, ra);
                load_cols(b, ldb, N, K, n0, k0 + GK, shift_b, vec_b != 0, rb);
            } else {
                load_rows(a, lda, M, K, m0, k0 + GK, shift_a, vec_a != 0, ra);
                load_rows(b, ldb, N, K, n0, k0 + GK, shift_b, vec_b != 0, rb);
            }
        }
#pragma unroll
        for (int kk = 0; kk < GK; kk += 4) {
            const float2 a0 = *reinterpret_cast<const float2*>(&As[wm + li][kk + 2 * lk]);
            const float2 a1 = *reinterpret_cast<const float2*>(&As[wm + 32 + li][kk + 2 * lk]);
            const float2 b0 = *reinterpret_cast<const float2*>(&Bs[wn + li][kk + 2 * lk]);
            const float2 b1 = *reinterpret_cast<const float2*>(&Bs[wn + 32 + li][kk + 2 * lk]);
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.x, b0.x, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.x, b1.x, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.x, b0.x, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.x, b1.x, acc[1][1], 0, 0, 0);
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.y, b0.y, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.y, b1.y, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.y, b0.y, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.y, b1.y, acc[1][1], 0, 0, 0);
        }
        __syncthreads();
    }

    if (MODE == SISIC_GRAM_SQDIST) {
        // the 8 lanes that share a row are neighbours: three exchange steps, the same tree for every row
#pragma unroll
        for (int q = 0; q < GP; ++q) {
#pragma unroll
            for (int sft = 1; sft < 8; sft <<= 1) {
                sq_a[q] += __shfl_xor(sq_a[q], sft, 64);
                sq_b[q] += __shfl_xor(sq_b[q], sft, 64);
            }
            if ((threadIdx.x & 7) == 0) {
                norm_a[(threadIdx.x >> 3) + 32 * q] = sq_a[q];
                norm_b[(threadIdx.x >> 3) + 32 * q] = sq_b[q];
            }
        }
        __syncthreads();
    }

    // C/D map of the 32x32 forms: register e of lane l is row (e & 3) + 8 (e >> 2) + 4 (l >> 5), column l & 31
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int cl = wn + j * 32 + li;
            const int col = n0 + cl;
            float nb = 0.0f;
            if (MODE == SISIC_GRAM_SQDIST) nb = norm_b[cl];
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int rl = wm + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * lk;
                const int row = m0 + rl;
                float s = acc[i][j][e];
                if (MODE == SISIC_GRAM_SQDIST) {
                    s = fmaxf(0.0f, (norm_a[rl] + nb) - 2.0f * s);
                } else if (MODE == SISIC_GRAM_POLY3) {
                    const float t = s / kdiv + 1.0f;
                    s = t * t * t;
                }
                if (row < M && col < N) out[(int64_t)row * ldo + col] = s;
            }
        }
}

// ---- column means ----------------------------------------------------------------------------------------------------------------
// 64 columns x 16 row groups per workgroup: group g sums rows g, g + 16, ... in double, the 16 partials are added in group order
__global__ void __launch_bounds__(1024)
col_means_kernel(const float* __restrict__ x, int64_t ld, int n, int d, double* __restrict__ mean_out) {
    __shared__ double part[16][64];
    const int c = blockIdx.x * 64 + threadIdx.x;
    const int g = threadIdx.y;
    double acc = 0.0;
    if (c < d)
        for (int r = g; r < n; r += 16) acc += (double)x[(int64_t)r * ld + c];
    part[g][threadIdx.x] = acc;
    __syncthreads();
    if (g == 0 && c < d) {
        double s = 0.0;
#pragma unroll
        for (int i = 0; i < 16; ++i) s += part[i][threadIdx.x];
        mean_out[c] = s / (double)n;
    }
}

// ---- matrix sum ------------------------------------------------------------------------------------------------------------------
// one workgroup: thread t sums the elements t, t + 1024, ... (row-major order of the [n, m] matrix) in double, then a tree in LDS
__global__ void __launch_bounds__(1024)
matrix_sum_kernel(const float* __restrict__ x, int64_t ld, int n, int m, int exclude_diagonal, double* __restrict__ out) {
    __shared__ double part[1024];
    double acc = 0.0;
    // a thread walks whole rows' columns t, t + 1024, ...: the same order whatever the leading dimension
    for (int r = 0; r < n; ++r) {
        const float* row = x + (int64_t)r * ld;
        for (int c = threadIdx.x; c < m; c += 1024)
            if (!(exclude_diagonal && c == r)) acc += (double)row[c];
    }
    part[threadIdx.x] = acc;
    __syncthreads();
    for (int w = 512; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = part[0];
}

// ---- k smallest of every row -----------------------------------------------------------------------------------------------------
// one wave per row: every lane keeps the 8 smallest of its columns (lane, lane + 64, ...) sorted in registers, then k rounds pick
// the smallest head of the 64 lists (value first, then column) and pop it
__global__ void __launch_bounds__(256)
rows_topk_kernel(const float* __restrict__ dist, int64_t ld, const float* __restrict__ col_offset, int n, int m, int k,
                 int skip_diagonal, float* __restrict__ val_out, int32_t* __restrict__ idx_out) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    const float INF = __builtin_inff();
    float v[8];
    int id[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) { v[i] = INF; id[i] = 0x7fffffff; }
    const float* src = dist + (int64_t)row * ld;
    for (int j = lane; j < m; j += 64) {
        if (skip_diagonal && j == row) continue;
        float x = src[j];
        if (col_offset) x -= col_offset[j];
        if (x < v[7]) {                      // columns arrive in ascending order: an equal value never displaces an earlier one
            v[7] = x; id[7] = j;
#pragma unroll
            for (int p = 7; p > 0; --p)
                if (v[p] < v[p - 1]) {
                    const float tv = v[p]; v[p] = v[p - 1]; v[p - 1] = tv;
                    const int ti = id[p]; id[p] = id[p - 1]; id[p - 1] = ti;
                }
        }
    }
    for (int round = 0; round < k; ++round) {
        float bv = v[0];
        int bi = id[0];
#pragma unroll
        for (int sft = 32; sft > 0; sft >>= 1) {
            const float ov = __shfl_xor(bv, sft, 64);
            const int oi = __shfl_xor(bi, sft, 64);
            if (ov < bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        }
        if (bi == id[0] && bi != 0x7fffffff) {          // the owner of the winning column pops its head
#pragma unroll
            for (int p = 0; p < 7; ++p) { v[p] = v[p + 1]; id[p] = id[p + 1]; }
            v[7] = INF; id[7] = 0x7fffffff;
        }
        if (lane == 0) {
            val_out[(int64_t)row * k + round] = bv;
            idx_out[(int64_t)row * k + round] = bi == 0x7fffffff ? -1 : bi;
        }
    }
}

// ---- exact distances of chosen pairs ---------------------------------------------------------------------------------------------
// one workgroup per pair (i, j), pair = i * k + j: thread t sums the coordinates t, t + 256, ... in double, then a tree in LDS;
// an index outside [0, nb) gives NaN and reads nothing
__global__ void __launch_bounds__(256)
pair_sqdist_kernel(const float* __restrict__ a, int64_t lda, const float* __restrict__ b, int64_t ldb, int nb, int d, int k,
                   const int32_t* __restrict__ idx, float* __restrict__ out) {
    __shared__ double part[256];
    const int64_t pair = blockIdx.x;
    const int64_t i = pair / k;
    const int j = idx[pair];
    const bool ok = j >= 0 && j < nb;
    double acc = 0.0;
    if (ok) {
        const float* pa = a + i * lda;
        const float* pb = b + (int64_t)j * ldb;
        for (int c = threadIdx.x; c < d; c += 256) {
            const double t = (double)pa[c] - (double)pb[c];
            acc += t * t;
        }
    }
    part[threadIdx.x] = acc;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[pair] = ok ? (float)part[0] : __builtin_nanf("");
}

template <int MODE, bool TRANS>
int launch_gram_as(const float* a, const float* b, const float* sa, const float* sb, float* out, int M, int N, int K, int64_t lda,
                   int64_t ldb, int64_t ldo, hipStream_t s) {
    // 16-byte loads: the base and every row start aligned, and the shift where one is read along the load
    auto vec = [](const float* p, int64_t ld, const float* shift) {
        return (reinterpret_cast<uintptr_t>(p) % 16 == 0 && ld % 4 == 0 && (TRANS || reinterpret_cast<uintptr_t>(shift) % 16 == 0)) ? 1 : 0;
    };
    hipLaunchKernelGGL((gram_kernel<MODE, TRANS>), dim3(cdiv(N, GT), cdiv(M, GT)), dim3(256), 0, s, a, b, sa, sb, out, M, N, K, lda,
                       ldb, ldo, (float)K, vec(a, lda, sa), vec(b, ldb, sb));
    SISIC_HIP(hipGetLastError());
    return SISIC_OK;
}

}  // namespace

// the arguments have been checked (api.cpp)
int launch_gram(sisic_ctx* ctx, const sisic_gram_args& g, hipStream_t s) {
    const float* b = g.b ? g.b : g.a;
    const int64_t ldb = g.b ? g.ldb : g.lda;
    if (g.contract_rows) {
        // out [d, d] = A'^T A': both operands are A read k-major, the contraction runs over the n rows
        ProfileScope prof(ctx, s, PK_OTHER, 4.0 * ((double)g.n * g.d + (double)g.d * g.d), 2.0 * g.d * (double)g.d * g.n);
        return launch_gram_as<SISIC_GRAM_DOT, true>(g.a, g.a, g.shift_a, g.shift_a, g.out, g.d, g.d, g.n, g.lda, g.lda, g.ldo, s);
    }
    ProfileScope prof(ctx, s, PK_OTHER, 4.0 * (((double)g.n + g.m) * g.d + (double)g.n * g.m), 2.0 * g.n * (double)g.m * g.d);
    switch (g.mode) {
    case SISIC_GRAM_DOT:
        return launch_gram_as<SISIC_GRAM_DOT, false>(g.a, b, g.shift_a, g.shift_b, g.out, g.n, g.m, g.d, g.lda, ldb, g.ldo, s);
    case SISIC_GRAM_SQDIST:
        return launch_gram_as<SISIC_GRAM_SQDIST, false>(g.a, b, g.shift_a, g.shift_b, g.out, g.n, g.m, g.d, g.lda, ldb, g.ldo, s);
    default:
        return launch_gram_as<SISIC_GRAM_POLY3, false>(g.a, b, g.shift_a, g.shift_b, g.out, g.n, g.m, g.d, g.lda, ldb, g.ldo, s);
    }
}

int launch_col_means(sisic_ctx* ctx, const float* x, int64_t ld, int n, int d, double* mean_out, hipStream_t s) {
    ProfileScope prof(ctx, s, PK_OTHER, 4.0 * n * (double)d, 0.0);
    hipLaunchKernelGGL(col_means_kernel, dim3(cdiv(d, 64)), dim3(64, 16), 0, s, x, ld, n, d, mean_out);
    SISIC_HIP(hipGetLastError());
    return SISIC_OK;
}

int launch_matrix_sum(sisic_ctx* ctx, const float* x, int64_t ld, int n, int m, int exclude_diagonal, double* out, hipStream_t s) {
    ProfileScope prof(ctx, s, PK_OTHER, 4.0 * n * (double)m, 0.0);
    hipLaunchKernelGGL(matrix_sum_kernel, dim3(1), dim3(1024), 0, s, x, ld, n, m, exclude_diagonal, out);
    SISIC_HIP(hipGetLastError());
    return SISIC_OK;
}

int launch_rows_topk(sisic_ctx* ctx, const float* dist, int64_t ld, const float* col_offset, int n, int m, int k, int skip_diagonal,
                     float* val_out, int32_t* idx_out, hipStream_t s) {
    ProfileScope prof(ctx, s, PK_OTHER, 4.0 * n * (double)m, 0.0);
    hipLaunchKernelGGL(rows_topk_kernel, dim3(cdiv(n, 4)), dim3(256), 0, s, dist, ld, col_offset, n, m, k, skip_diagonal, val_out,
                       idx_out);
    SISIC_HIP(hipGetLastError());
    return SISIC_OK;
}

int launch_pair_sqdist(sisic_ctx* ctx, const float* a, int64_t lda, const float* b, int64_t ldb, int n, int nb, int d, int k,
                       const int32_t* idx, float* out, hipStream_t s) {
    ProfileScope prof(ctx, s, PK_OTHER, 8.0 * n * (double)k * d, 0.0);
    hipLaunchKernelGGL(pair_sqdist_kernel, dim3((unsigned)((int64_t)n * k)), dim3(256), 0, s, a, lda, b, ldb, nb, d, k, idx, out);
    SISIC_HIP(hipGetLastError());
    return SISIC_OK;
}

}  // namespace sisic
