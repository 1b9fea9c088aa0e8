// The counter-based normal numbers of DESIGN.md 6m, shared by fg_obsnoise.hip (observation / action noise) and
// fg_mb_envrestore.hip (reset noise of the multi-block envs): Philox4x32-10 (Salmon et al., SC'11), the fp32 arithmetic that
// turns two of its words into two normal numbers, and dst = src + sigma z.  The arithmetic is defined at the top of fg_obsnoise.hip
// and restated operation for operation in tests/obs_noise_ref.py; a translation unit that includes this header is compiled with
// -ffp-contract=off, so that every operation is rounded on its own.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t w[4]) {
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}

// two normals of two words: the definition at the top of fg_obsnoise.hip, in its order
__device__ __forceinline__ void normal_pair(uint32_t w0, uint32_t w1, float& z0, float& z1) {
    const float u = ((float)(w0 >> 9) + 0.5f) * 0x1p-23f;
    const uint32_t ub = __float_as_uint(u);
    int e = (int)(ub >> 23) - 127;
    float m = __uint_as_float((ub & 0x007fffffu) | 0x3f800000u);
    if (m > 1.41421354f) { m = m * 0.5f; e = e + 1; }
    const float t = (m - 1.0f) / (m + 1.0f);
    const float t2 = t * t;
    float p = (float)(1.0 / 9.0) * t2 + (float)(1.0 / 7.0);
    p = p * t2 + (float)(1.0 / 5.0);
    p = p * t2 + (float)(1.0 / 3.0);
    p = p * t2 + 1.0f;
    const float ln_u = (float)e * 0.693147182f + (2.0f * t) * p;
    const float r = sqrtf(-2.0f * ln_u);

    const uint32_t q = w1 >> 30;
    float f = ((float)((w1 >> 9) & 0x1fffffu) + 0.5f) * 0x1p-21f;
    const bool swap = f > 0.5f;
    if (swap) f = 1.0f - f;
    const float a = f * 1.57079637f;
    const float a2 = a * a;
    float sn = (float)(1.0 / 362880.0) * a2 + (float)(-1.0 / 5040.0);
    sn = sn * a2 + (float)(1.0 / 120.0);
    sn = sn * a2 + (float)(-1.0 / 6.0);
    sn = sn * a2 + 1.0f;
    sn = sn * a;
    float cs = (float)(-1.0 / 3628800.0) * a2 + (float)(1.0 / 40320.0);
    cs = cs * a2 + (float)(-1.0 / 720.0);
    cs = cs * a2 + (float)(1.0 / 24.0);
    cs = cs * a2 + -0.5f;
    cs = cs * a2 + 1.0f;
    const float c = swap ? sn : cs, s = swap ? cs : sn;
    const float cr = (q == 0) ? c : (q == 1) ? -s : (q == 2) ? -c : s;
    const float sr = (q == 0) ? s : (q == 1) ? c : (q == 2) ? -s : -c;
    z0 = r * cr;
    z1 = r * sr;
}

__device__ __forceinline__ float add_noise(float v, double sigma, float z) { return v + (float)sigma * z; }
__device__ __forceinline__ double add_noise(double v, double sigma, float z) { return v + sigma * (double)z; }
