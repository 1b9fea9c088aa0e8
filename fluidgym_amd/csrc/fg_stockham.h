// The wave-level Stockham autosort FFT of the spectra kernels (fg_planespectra.hip: wavenumber spectra of planes; fg_signalspectra.hip:
// Welch spectra of per-env signals), in fg_real, for both libraries: one wave64 transforms sequences that lie in its own two LDS
// buffers; between stages only the lanes of that wave exchange data, so a wave-level barrier is enough.
#pragma once
#include "fg_internal.h"

#if FG_F64
typedef double2 ps_c;
#else
typedef float2 ps_c;
#endif

__device__ __forceinline__ void ps_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ ps_c ps_make(fg_real x, fg_real y) { ps_c r; r.x = x; r.y = y; return r; }
__device__ __forceinline__ ps_c ps_cmul(ps_c a, ps_c w) { return ps_make(a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x); }

// Forward Stockham autosort FFT of total / N sequences of N = 2^ln complex that lie one after the other in x (the arithmetic of
// fgfft::stockham, fg_fftrow.h, for fg_real and a run-time length): radix 4 while the remaining length allows it, then one radix-2
// stage; ping-pongs between x and y and returns the buffer that holds the result.  tw: W^k at tw[k * tws].
__device__ __forceinline__ ps_c* ps_stockham(ps_c* x, ps_c* y, const ps_c* __restrict__ tw, int ln, int tws, int total, int lane) {
    const int N = 1 << ln;
    auto twid = [&](int k) { ps_c w = tw[(k & (N - 1)) * tws]; w.y = -w.y; return w; };
    int sft = 0, lrem = ln;
    while (lrem >= 2) {
        const int sm = (1 << sft) - 1, nq = N >> 2;
        for (int i = lane; i < (total >> 2); i += 64) {
            const int s = i >> (ln - 2), t = i & (nq - 1);
            const int q = t & sm, ps = t - q;
            const ps_c* xs = x + (s << ln);
            const ps_c a0 = xs[t], a1 = xs[t + nq], a2 = xs[t + 2 * nq], a3 = xs[t + 3 * nq];
            const ps_c r1 = ps_make(a1.y, -a1.x), r3 = ps_make(a3.y, -a3.x);
            const ps_c b0 = ps_make(a0.x + a1.x + a2.x + a3.x, a0.y + a1.y + a2.y + a3.y);
            const ps_c c1 = ps_make(a0.x + r1.x - a2.x - r3.x, a0.y + r1.y - a2.y - r3.y);
            const ps_c c2 = ps_make(a0.x - a1.x + a2.x - a3.x, a0.y - a1.y + a2.y - a3.y);
            const ps_c c3 = ps_make(a0.x - r1.x - a2.x + r3.x, a0.y - r1.y - a2.y + r3.y);
            ps_c* o = y + (s << ln) + 4 * ps + q;
            o[0] = b0;
            o[1 << sft] = ps_cmul(c1, twid(ps));
            o[2 << sft] = ps_cmul(c2, twid(2 * ps));
            o[3 << sft] = ps_cmul(c3, twid(3 * ps));
        }
        ps_wave_sync();
        ps_c* tmp = x; x = y; y = tmp;
        sft += 2; lrem -= 2;
    }
    if (lrem == 1) {
        const int sm = (1 << sft) - 1, nh = N >> 1;
        for (int i = lane; i < (total >> 1); i += 64) {
            const int s = i >> (ln - 1), t = i & (nh - 1);
            const int q = t & sm, ps = t - q;
            const ps_c u = x[(s << ln) + t], v = x[(s << ln) + t + nh];
            ps_c* o = y + (s << ln) + 2 * ps + q;
            o[0] = ps_make(u.x + v.x, u.y + v.y);
            o[1 << sft] = ps_cmul(ps_make(u.x - v.x, u.y - v.y), twid(ps));
        }
        ps_wave_sync();
        ps_c* tmp = x; x = y; y = tmp;
    }
    return x;
}
