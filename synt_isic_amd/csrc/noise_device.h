// noise_device.h -- the device-noise contract: Philox4x32-10 + Box-Muller, one block per four
// consecutive elements of an image.  A pure function of (seed, step, tag, element): no state, nothing to synchronise.
// Included by elementwise.hip and xai_kernels.hip only, both compiled with -ffp-contract=off (csrc/Makefile), so that the step
// kernels, the stand-alone fill kernel and the noise interventions produce the same bits.  train_kernels.hip (built without that
// flag) takes the raw words only -- noise_bits4 for the dropout masks: integer arithmetic, which no floating-point flag changes.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace sisic {

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123 constants)
__device__ __forceinline__ uint4 philox4x32_10(uint4 c, uint32_t k0, uint32_t k1) {
    constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(M0, c.x), lo0 = M0 * c.x;
        const uint32_t hi1 = __umulhi(M1, c.z), lo1 = M1 * c.z;
        c = make_uint4(hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0);
        k0 += W0;
        k1 += W1;
    }
    return c;
}

// the block of elements 4q .. 4q+3 of the image with this seed
__device__ __forceinline__ uint4 noise_bits4(uint64_t seed, uint32_t q, uint32_t step, uint32_t tag) {
    return philox4x32_10(make_uint4(q, step, tag, 0u), (uint32_t)seed, (uint32_t)(seed >> 32));
}

// (r_a, r_b) -> two normals.  u1 = ((r_a >> 8) + 1) * 2^-24 in (0, 1], u2 = (r_b >> 8) * 2^-24 in [0, 1): both exact in fp32.
// The precise logf / sqrtf / sincospif, not the fast intrinsics (the accuracy is what tests pin; the rate does not matter here).
__device__ __forceinline__ void box_muller(uint32_t ra, uint32_t rb, float* zc, float* zs) {
#pragma clang fp contract(off)
    const float u1 = (float)((ra >> 8) + 1u) * 0x1p-24f;
    const float u2 = (float)(rb >> 8) * 0x1p-24f;
    const float rad = sqrtf(-2.0f * logf(u1));
    float s, c;
    sincospif(2.0f * u2, &s, &c);
    *zc = rad * c;
    *zs = rad * s;
}

__device__ __forceinline__ float4 noise_normal4(uint64_t seed, uint32_t q, uint32_t step, uint32_t tag) {
    const uint4 r = noise_bits4(seed, q, step, tag);
    float4 z;
    box_muller(r.x, r.y, &z.x, &z.y);
    box_muller(r.z, r.w, &z.z, &z.w);
    return z;
}

// one element (the scalar paths: an image size that is not a multiple of 4, or unaligned tensors)
__device__ __forceinline__ float noise_normal1(uint64_t seed, int64_t e, uint32_t step, uint32_t tag) {
    const float4 z = noise_normal4(seed, (uint32_t)(e >> 2), step, tag);
    const int k = (int)(e & 3);
    return k == 0 ? z.x : k == 1 ? z.y : k == 2 ? z.z : z.w;
}

}  // namespace sisic
