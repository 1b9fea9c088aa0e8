// Internal definitions shared by the HIP translation units of libfluidgym_hip.so.
// gfx950 / wave64 only.  Public C ABI: include/fluidgym_hip.h.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <math.h>
#include <stdint.h>
#include <cstring>
#include <string>
#include <type_traits>

#include "../../include/fluidgym_hip.h"
#include "fg_switches.h"

// fg_real (include/fluidgym_hip.h): float in libfluidgym_hip.so, double in libfluidgym_hip_f64.so (-DFG_REAL_DOUBLE).  The fp32 build is
// the product the benchmarks run; the fp64 build exists for FluidEnv(dtype=torch.float64) and compiles the core translation units only
// (fg_api / fg_piso / fg_poisson / fg_bicgstab / fg_profile + fg_f64_stubs), scalar lanes (VEC = 1) throughout.
#ifdef FG_REAL_DOUBLE
struct alignas(16) fg_real4 { double x, y, z, w; };   // four consecutive reals (two 16-byte accesses)
__host__ __device__ __forceinline__ fg_real4 make_fg_real4(double x, double y, double z, double w) { fg_real4 r; r.x = x; r.y = y; r.z = z; r.w = w; return r; }
#define FG_F64 1
#define FG_FMAX fmax
#define FG_FABS fabs
#define FG_SQRT sqrt
#else
typedef float4 fg_real4;
#define make_fg_real4 make_float4
#define FG_F64 0
#define FG_FMAX fmaxf
#define FG_FABS fabsf
#define FG_SQRT sqrtf
#endif

// The recurrence words of the multi-kernel Krylov solvers (accumulators, alpha / omega, flags) are read and zeroed through
// acc_ld / acc_st, sc_ld / sc_st, flag_ld / flag_st.  They are plain loads / stores: sums are accumulated with device-scope atomics
// in one kernel and read in the next, zeroed by a leader workgroup for a later one -- kernel boundaries order all of it.  While the
// "intermittent non-finite BiCGStab solve" of round 1 was hunted, the suspicion that plain accesses to these words are not
// coherent across the per-XCD L2s was tested and REJECTED: fg_coherence_litmus reads back 3.2e7 sums exactly under every
// combination of plain / agent-scope atomic loads and stores, and the captured failures reproduce identically under all of them
// (they are exact breakdowns of the fp32 recurrence, fg_mb_krylov.hip mbb_p_head).  Agent-scope loads by every wave
// cost 4-45 % of env-steps/s (same-address requests serialise at the memory side), so the build switches stay at 0:
// FG_ACC_ACCESS / FG_FLAG_ACCESS (profiles/bicg_stress.sh): bit 0 = agent-scope atomic loads, bit 1 = agent-scope atomic stores,
// for the accumulators and for the scalar / flag words.
#ifndef FG_ACC_ACCESS
#define FG_ACC_ACCESS 0
#endif
#ifndef FG_FLAG_ACCESS
#define FG_FLAG_ACCESS 0
#endif
template <typename T> __device__ __forceinline__ T fg_word_ld(const T* p, bool atomic) {
    return atomic ? __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : *p;
}
template <typename T> __device__ __forceinline__ void fg_word_st(T* p, T v, bool atomic) {
    if (atomic) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); else *p = v;
}
__device__ __forceinline__ double acc_ld(const double* p) { return fg_word_ld(p, (FG_ACC_ACCESS & 1) != 0); }
__device__ __forceinline__ void acc_st(double* p, double v) { fg_word_st(p, v, (FG_ACC_ACCESS & 2) != 0); }

// ------------------------------------------------------------------------------------------------
// Order-independent reduction accumulator.  The dot products of the Krylov recurrences end in one contribution per
// workgroup; added with fp64 atomics their order -- hence the rounded sum, hence every later iterate -- varied from run to
// run (a replayed airfoil episode differed by 4-6 % in the forces after 17 env steps).  The reference's dots are cuBLAS
// calls in a fixed order (cg_solver_kernel.cu:277,317), so its get_state -> set_state -> step replays exactly
// (envs/fluid_env.py:1320-1363).  Here a contribution is split EXACTLY into four fixed-point words of 42 bits (units 2^34,
// 2^-8, 2^-50, 2^-92) that are added with 64-bit INTEGER atomics: integer addition is associative, so the words -- and the
// double they are read back as -- do not depend on the order of arrival.  Range: |contribution| < 2^75 (3.8e22), up to 2^20
// contributions, resolution 2^-93; anything else (NaN, Inf, larger) sets the poison word and the accumulator reads as NaN,
// which the solvers already treat as a non-finite solve.  `plain` carries a value stored with acc_st (0 to reset the
// accumulator, or a scalar a leader parks between kernels); the value of an accumulator is plain + the sum of what was
// added since.  All-zero bytes are an accumulator holding 0 (hipMemset works).  Kernel boundaries order stores, adds and
// loads exactly as for the plain words above.
// ------------------------------------------------------------------------------------------------
struct alignas(64) FgDacc {
    unsigned long long w[4];
    unsigned long long poison;
    double plain;
    unsigned long long w4;     // fifth word: fp64 build only (FG_DACC_WORDS == 5)
    unsigned long long pad;
};
static_assert(sizeof(FgDacc) == 64, "one accumulator per 64-byte line segment");

// the split of one contribution and the value of the words: shared by the device accessors and the host self-test
// (fg_dacc_host_sum), so that what the CPU test checks is what the kernels run.
// fp32 build: four words, units 2^34 .. 2^-92, range 2^75.  fp64 build (FG_REAL_DOUBLE is defined before this header is read):
// FIVE words, the same range with a last unit of 2^-134, so that residuals of solves driven to 1e-13 .. 1e-15 stay resolved.  (Rounds
// 2-3 gave the fp64 build four words shifted down by 2^-30 -- range 2^45 = 3.5e13.  Round 4: the impulsive start of the fp64
// airfoil env exceeds that -- the tiny cells at the nose give residual components ~1e7 --, so its sums were poisoned until
// round 3 and saturated after the ADVICE-r3 change; with five words neither happens.)
#ifdef FG_REAL_DOUBLE
#define FG_DACC_WORDS 5
#else
#define FG_DACC_WORDS 4
#endif
#define FG_DACC_U0 0x1p34
#define FG_DACC_U1 0x1p-8
#define FG_DACC_U2 0x1p-50
#define FG_DACC_U3 0x1p-92
#define FG_DACC_U4 0x1p-134
#define FG_DACC_LIMIT 0x1p75
__host__ __device__ __forceinline__ bool fg_dacc_split(double v, long long k[5]) {
    if (!(fabs(v) <= 1.79769313486231570815e308)) return false;  // NaN, Inf: poison
    // a finite contribution beyond the window SATURATES (each contribution on its own, so the sum stays order-independent):
    // a diverging but finite solve keeps reading as a large finite residual -- return-best / the retry ladder then see
    // "not converged", not "not finite" (the poison word is for NaN / Inf only)
    if (!(fabs(v) < FG_DACC_LIMIT)) v = v < 0 ? -FG_DACC_LIMIT * (1.0 - 0x1p-30) : FG_DACC_LIMIT * (1.0 - 0x1p-30);
    double r = v;
    const double k0 = rint(r * (1.0 / FG_DACC_U0)); r -= k0 * FG_DACC_U0;      // exact: r keeps the bits of v below the word
    const double k1 = rint(r * (1.0 / FG_DACC_U1)); r -= k1 * FG_DACC_U1;
    const double k2 = rint(r * (1.0 / FG_DACC_U2)); r -= k2 * FG_DACC_U2;
    const double k3 = rint(r * (1.0 / FG_DACC_U3));                            // (4 words: bits below half the last unit are dropped, the same ones in any order)
    k[0] = (long long)k0; k[1] = (long long)k1; k[2] = (long long)k2; k[3] = (long long)k3;
    k[4] = 0;
#if FG_DACC_WORDS == 5
    r -= k3 * FG_DACC_U3;
    k[4] = (long long)rint(r * (1.0 / FG_DACC_U4));
#endif
    return true;
}
__host__ __device__ __forceinline__ double fg_dacc_value(unsigned long long w0, unsigned long long w1, unsigned long long w2,
                                                         unsigned long long w3, unsigned long long poison, double plain,
                                                         unsigned long long w4 = 0ull) {
    // smallest unit first; every conversion and addition is a fixed sequence on the same integer words
    double t = 0.0;
#if FG_DACC_WORDS == 5
    t = (double)(long long)w4 * FG_DACC_U4;
#endif
    t += (double)(long long)w3 * FG_DACC_U3;
    t += (double)(long long)w2 * FG_DACC_U2;
    t += (double)(long long)w1 * FG_DACC_U1;
    t += (double)(long long)w0 * FG_DACC_U0;
    t += plain;
    return poison ? (double)NAN : t;
}
inline double fg_dacc_host_value(const FgDacc& a) { return fg_dacc_value(a.w[0], a.w[1], a.w[2], a.w[3], a.poison, a.plain, a.w4); }
__device__ __forceinline__ void acc_st(FgDacc* p, double v) {
    ulonglong2* q = reinterpret_cast<ulonglong2*>(p);
    q[0] = make_ulonglong2(0ull, 0ull);
    q[1] = make_ulonglong2(0ull, 0ull);
    q[2] = make_ulonglong2(0ull, (unsigned long long)__double_as_longlong(v));
#if FG_DACC_WORDS == 5
    q[3] = make_ulonglong2(0ull, 0ull);
#endif
}
__device__ __forceinline__ double acc_ld(const FgDacc* p) {
    const ulonglong2* q = reinterpret_cast<const ulonglong2*>(p);
    const ulonglong2 a = q[0], b = q[1], c = q[2];
#if FG_DACC_WORDS == 5
    const ulonglong2 d = q[3];
    return fg_dacc_value(a.x, a.y, b.x, b.y, c.x, __longlong_as_double((long long)c.y), d.x);
#else
    return fg_dacc_value(a.x, a.y, b.x, b.y, c.x, __longlong_as_double((long long)c.y));
#endif
}
__device__ __forceinline__ void acc_add(FgDacc* p, double v) {
    long long k[5];
    if (!fg_dacc_split(v, k)) { atomicAdd(&p->poison, 1ull); return; }
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (k[i] != 0) atomicAdd(&p->w[i], (unsigned long long)k[i]);
#if FG_DACC_WORDS == 5
    if (k[4] != 0) atomicAdd(&p->w4, (unsigned long long)k[4]);
#endif
}

__device__ __forceinline__ fg_real sc_ld(const fg_real* p) { return fg_word_ld(p, (FG_FLAG_ACCESS & 1) != 0); }
__device__ __forceinline__ void sc_st(fg_real* p, fg_real v) { fg_word_st(p, v, (FG_FLAG_ACCESS & 2) != 0); }
__device__ __forceinline__ int32_t flag_ld(const int32_t* p) { return fg_word_ld(p, (FG_FLAG_ACCESS & 1) != 0); }
__device__ __forceinline__ void flag_st(int32_t* p, int32_t v) { fg_word_st(p, v, (FG_FLAG_ACCESS & 2) != 0); }

#define FG_BLOCK 256  // threads per workgroup = 4 waves of 64

// ------------------------------------------------------------------------------------------------
// Grid description handed to every kernel by value (lives in SGPRs / kernarg, no LDS struct copy as
// in the reference's KERNEL_PER_CELL_LOOP, PISO_multiblock_cuda_kernel.cu:3590-3610).
// ------------------------------------------------------------------------------------------------
struct FgGrid {
    int dims;
    int nx, ny, nz;
    int n;        // cells per env
    int B;        // env batch
    int b0;       // first env of the launch (0 except in a launch over a sub-batch of envs: fg_bicgstab_solve)
    int fixed[6]; // 1 = FIXED (prescribed) face, 0 = periodic
    const fg_real* h[3];  // cell widths per axis (device), length nx / ny / nz
    const fg_real* rh[3]; // reciprocals
};

struct FgBounds {
    const fg_real* vel[6];    // [B,d,slab] or nullptr (periodic)
    const fg_real* scal[6];   // [B,C,slab] or nullptr
    int scalar_bc[6];       // FG_DIRICHLET / FG_NEUMANN for the channel being processed
};

// Tile geometry: a workgroup covers 64 cells in x (16 lanes x float4, or 64 scalar lanes) and the
// remaining 256/BX threads are spread over y (and z in 3-D), so x accesses are 256-B coalesced rows.
template <int DIMS, int VEC>
struct FgTile {
    static constexpr int BX = 64 / VEC;
    static constexpr int BZ = (DIMS == 3) ? ((VEC == 4) ? 4 : 2) : 1;
    static constexpr int BY = FG_BLOCK / (BX * BZ);
    static constexpr int TX = 64;
};

struct FgLaunch {
    dim3 grid;
    int tiles_x, tiles_y, tiles_z, tiles; // per env
};

template <int DIMS, int VEC>
inline FgLaunch fg_launch_geometry(const FgGrid& g) {
    using T = FgTile<DIMS, VEC>;
    FgLaunch L;
    L.tiles_x = (g.nx + T::TX - 1) / T::TX;
    L.tiles_y = (g.ny + T::BY - 1) / T::BY;
    L.tiles_z = (g.nz + T::BZ - 1) / T::BZ;
    L.tiles = L.tiles_x * L.tiles_y * L.tiles_z;
    L.grid = dim3((unsigned)(L.tiles * g.B), 1, 1);
    return L;
}

#ifdef __HIPCC__
// ------------------------------------------------------------------------------------------------
// device helpers
// ------------------------------------------------------------------------------------------------
template <int VEC>
struct FgVec {
    fg_real v[VEC];
};

template <int VEC>
__device__ __forceinline__ FgVec<VEC> fg_load(const fg_real* __restrict__ p) {
    FgVec<VEC> r;
    if constexpr (VEC == 4) {
        const float4 t = *reinterpret_cast<const float4*>(p);
        r.v[0] = t.x; r.v[1] = t.y; r.v[2] = t.z; r.v[3] = t.w;
    } else {
        r.v[0] = *p;
    }
    return r;
}
template <int VEC>
__device__ __forceinline__ void fg_store(fg_real* __restrict__ p, const FgVec<VEC>& r) {
    if constexpr (VEC == 4) {
        *reinterpret_cast<float4*>(p) = make_float4(r.v[0], r.v[1], r.v[2], r.v[3]);
    } else {
        *p = r.v[0];
    }
}

// XCD-aware block remap (cdna_hip_programming.md T1, bijective form): hardware places block b on
// XCD b % 8; give every XCD a contiguous chunk of the logical grid so that one env's tiles (and its
// y/z halo re-reads) stay in one XCD's 4 MiB L2 across the kernels of a solver iteration.
__device__ __forceinline__ unsigned fg_xcd_remap(unsigned bid, unsigned nwg) {
    const unsigned nxcd = 8;
    if (nwg < nxcd * 2) return bid;
    const unsigned q = nwg / nxcd, r = nwg % nxcd;
    const unsigned xcd = bid % nxcd, k = bid / nxcd;
    const unsigned base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return base + k;
}

// Per-thread stencil context: where the thread's VEC cells and their 2*DIMS neighbours live.
template <int DIMS, int VEC>
struct FgCtx {
    int b;          // env
    int i0, j, k;   // first cell of the vector
    bool valid;
    int idx;        // linear index of cell i0 inside the env
    int ixm, ixp;   // linear index of the -x neighbour of element 0 / +x neighbour of element VEC-1
    int iym, iyp, izm, izp; // linear index of the vector start in the neighbouring rows
    // face masks (1 = face has a neighbour: interior or periodic; 0 = prescribed face)
    fg_real mxm, mxp, mym, myp, mzm, mzp;
};

template <int DIMS, int VEC>
__device__ __forceinline__ FgCtx<DIMS, VEC> fg_make_ctx(const FgGrid& g, int tiles_x, int tiles_y, int tiles) {
    using T = FgTile<DIMS, VEC>;
    FgCtx<DIMS, VEC> c;
    const unsigned bid = fg_xcd_remap(blockIdx.x, gridDim.x);
    c.b = bid / tiles;
    int t = bid - c.b * tiles;
    c.b += g.b0;
    int tix, tiy, tiz;
    if (DIMS == 3 && (tiles_y & 7) == 0 && gridDim.x == (unsigned)tiles) {
        // One big env (e.g. 256^3): the XCD remap hands each XCD a contiguous eighth of the tile ids.  Order the
        // ids [y-slab][z][y in slab][x] so that an XCD sweeps z inside a thin y-slab: the z-halo planes it
        // re-reads one layer later are still in its 4 MiB L2 (PMC: 27 % over-fetch with the plain x,y,z order).
        const int ys = tiles_y >> 3;
        const int per_slab = tiles / 8, per_layer = tiles_x * ys;
        const int slab = t / per_slab;
        int r = t - slab * per_slab;
        tiz = r / per_layer;
        r -= tiz * per_layer;
        tiy = slab * ys + r / tiles_x;
        tix = r % tiles_x;
    } else {
        tix = t % tiles_x;
        t /= tiles_x;
        tiy = t % tiles_y;
        tiz = t / tiles_y;
    }
    const int tid = threadIdx.x;
    const int lx = tid % T::BX;
    const int ly = (tid / T::BX) % T::BY;
    const int lz = tid / (T::BX * T::BY);
    c.i0 = (tix * T::BX + lx) * VEC;
    c.j = tiy * T::BY + ly;
    c.k = tiz * T::BZ + lz;
    c.valid = (c.i0 < g.nx) && (c.j < g.ny) && (c.k < g.nz);
    if (!c.valid) { c.i0 = 0; c.j = 0; c.k = 0; }
    const int row = (c.k * g.ny + c.j) * g.nx;
    c.idx = row + c.i0;
    // x neighbours
    const bool at_xm = (c.i0 == 0), at_xp = (c.i0 + VEC == g.nx);
    c.mxm = (at_xm && g.fixed[0]) ? 0.f : 1.f;
    c.mxp = (at_xp && g.fixed[1]) ? 0.f : 1.f;
    c.ixm = at_xm ? (g.fixed[0] ? c.idx : row + g.nx - 1) : c.idx - 1;
    c.ixp = at_xp ? (g.fixed[1] ? c.idx + VEC - 1 : row) : c.idx + VEC;
    // y neighbours
    const bool at_ym = (c.j == 0), at_yp = (c.j == g.ny - 1);
    c.mym = (at_ym && g.fixed[2]) ? 0.f : 1.f;
    c.myp = (at_yp && g.fixed[3]) ? 0.f : 1.f;
    c.iym = at_ym ? (g.fixed[2] ? c.idx : c.idx + (g.ny - 1) * g.nx) : c.idx - g.nx;
    c.iyp = at_yp ? (g.fixed[3] ? c.idx : c.idx - (g.ny - 1) * g.nx) : c.idx + g.nx;
    if constexpr (DIMS == 3) {
        const int sz = g.nx * g.ny;
        const bool at_zm = (c.k == 0), at_zp = (c.k == g.nz - 1);
        c.mzm = (at_zm && g.fixed[4]) ? 0.f : 1.f;
        c.mzp = (at_zp && g.fixed[5]) ? 0.f : 1.f;
        c.izm = at_zm ? (g.fixed[4] ? c.idx : c.idx + (g.nz - 1) * sz) : c.idx - sz;
        c.izp = at_zp ? (g.fixed[5] ? c.idx : c.idx - (g.nz - 1) * sz) : c.idx + sz;
    } else {
        c.mzm = c.mzp = 0.f;
        c.izm = c.izp = c.idx;
    }
    return c;
}

// A field value at the thread's cells and at their face neighbours.  At a prescribed face the
// "neighbour" is the cell itself (so one-sided differences fall out) and the mask is 0.
template <int DIMS, int VEC>
struct FgNbr {
    FgVec<VEC> c, xm, xp, ym, yp, zm, zp;
};

// x neighbours of a thread's vector: the cell left of element 0 is element VEC-1 of the lane before, the cell right of element VEC-1
// is element 0 of the lane after -- inside a tile row (16 consecutive lanes = one DPP row with VEC = 4) they come from a DPP row
// shift, and only the lanes at a tile or grid edge load them.  Until round 4 EVERY lane loaded both scalars: two wave-wide 4-byte
// gathers per field that pull the same sixteen cache lines through the L1 as the 16-byte centre load (PMC round 4: the stencil
// kernels of the headline sit 57-59 % of their wave cycles in s_waitcnt with ~3.5x their algorithmic bytes going through the L1).
#if !FG_F64
__device__ __forceinline__ float fg_dpp_from_lane_before(float v) {   // row_shr:1 -- lane i receives lane i-1 (of its row of 16)
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x111, 0xf, 0xf, true));
}
__device__ __forceinline__ float fg_dpp_from_lane_after(float v) {    // row_shl:1 -- lane i receives lane i+1
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x101, 0xf, 0xf, true));
}
#endif
template <int DIMS, int VEC>
__device__ __forceinline__ void fg_x_neighbours(const fg_real* __restrict__ q, const FgCtx<DIMS, VEC>& c, const FgVec<VEC>& ctr,
                                                fg_real& left, fg_real& right) {
#if !FG_F64
    if constexpr (VEC == 4) {
        // (callers run this under `c.valid`: the lanes before / after a valid interior lane of the same row are valid too)
        const int lx = threadIdx.x & 15;
        left = fg_dpp_from_lane_before(ctr.v[3]);
        right = fg_dpp_from_lane_after(ctr.v[0]);
        if (lx == 0 || c.ixm != c.idx - 1) left = q[c.ixm];
        if (lx == 15 || c.ixp != c.idx + VEC) right = q[c.ixp];
        return;
    }
#endif
    left = q[c.ixm];
    right = q[c.ixp];
}

template <int DIMS, int VEC>
__device__ __forceinline__ FgNbr<DIMS, VEC> fg_gather(const fg_real* __restrict__ q, const FgCtx<DIMS, VEC>& c) {
    FgNbr<DIMS, VEC> n;
    n.c = fg_load<VEC>(q + c.idx);
    fg_real left, right;
    fg_x_neighbours<DIMS, VEC>(q, c, n.c, left, right);
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        n.xm.v[e] = (e == 0) ? left : n.c.v[e - 1];
        n.xp.v[e] = (e == VEC - 1) ? right : n.c.v[e + 1];
    }
    n.ym = fg_load<VEC>(q + c.iym);
    n.yp = fg_load<VEC>(q + c.iyp);
    if constexpr (DIMS == 3) {
        n.zm = fg_load<VEC>(q + c.izm);
        n.zp = fg_load<VEC>(q + c.izp);
    }
    return n;
}

// only the neighbours along one axis (used for fluxes of one velocity component)
template <int DIMS, int VEC>
__device__ __forceinline__ void fg_gather_axis(const fg_real* __restrict__ q, const FgCtx<DIMS, VEC>& c, int axis,
                                               FgVec<VEC>& ctr, FgVec<VEC>& lo, FgVec<VEC>& hi) {
    ctr = fg_load<VEC>(q + c.idx);
    if (axis == 0) {
        fg_real left, right;
        fg_x_neighbours<DIMS, VEC>(q, c, ctr, left, right);
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            lo.v[e] = (e == 0) ? left : ctr.v[e - 1];
            hi.v[e] = (e == VEC - 1) ? right : ctr.v[e + 1];
        }
    } else if (axis == 1) {
        lo = fg_load<VEC>(q + c.iym);
        hi = fg_load<VEC>(q + c.iyp);
    } else {
        lo = fg_load<VEC>(q + c.izm);
        hi = fg_load<VEC>(q + c.izp);
    }
}

// Rectilinear metrics of the thread's cells: alpha_a = det*Minv_aa^2 = J/h_a^2
// (getLaplaceCoefficientOrthogonal, PISO_multiblock_cuda_kernel.cu:1224-1239) and of the neighbours
// across each face.
template <int DIMS, int VEC>
struct FgMetric {
    fg_real hx[VEC], rhx[VEC];
    fg_real rhx_m, rhx_p;   // 1/hx of the -x neighbour of element 0 / +x neighbour of element VEC-1
    fg_real hy, rhy, rhy_m, rhy_p;
    fg_real hz, rhz, rhz_m, rhz_p;
};

template <int DIMS, int VEC>
__device__ __forceinline__ FgMetric<DIMS, VEC> fg_metrics(const FgGrid& g, const FgCtx<DIMS, VEC>& c) {
    FgMetric<DIMS, VEC> m;
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        m.hx[e] = g.h[0][c.i0 + e];
        m.rhx[e] = g.rh[0][c.i0 + e];
    }
    m.rhx_m = g.rh[0][(c.i0 == 0) ? g.nx - 1 : c.i0 - 1];
    m.rhx_p = g.rh[0][(c.i0 + VEC == g.nx) ? 0 : c.i0 + VEC];
    m.hy = g.h[1][c.j];
    m.rhy = g.rh[1][c.j];
    m.rhy_m = g.rh[1][(c.j == 0) ? g.ny - 1 : c.j - 1];
    m.rhy_p = g.rh[1][(c.j == g.ny - 1) ? 0 : c.j + 1];
    if constexpr (DIMS == 3) {
        m.hz = g.h[2][c.k];
        m.rhz = g.rh[2][c.k];
        m.rhz_m = g.rh[2][(c.k == 0) ? g.nz - 1 : c.k - 1];
        m.rhz_p = g.rh[2][(c.k == g.nz - 1) ? 0 : c.k + 1];
    } else {
        m.hz = m.rhz = m.rhz_m = m.rhz_p = 1.f;
    }
    return m;
}

// wave64 sum / max; result valid in EVERY lane.  fp32: on the VALU alone -- DPP quad permutes, row rotations and row broadcasts (the
// rocPRIM sequence) and one v_readlane; until round 4 these were six dependent __shfl_down = ds_bpermute trips through the LDS
// crossbar per value.  Every lane of the wave must be active (all call sites sit next to a __syncthreads()).
#if !FG_F64
template <typename OP>
__device__ __forceinline__ float fg_wave_reduce_dpp(float v, OP op) {
    // (masked rows keep `old`, which is the neutral element handed in through the first operand of update_dpp)
#define FG_DPP(x, ctrl, rmask) __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(x), __float_as_int(x), ctrl, rmask, 0xf, false))
    v = op(v, FG_DPP(v, 0xb1, 0xf));     // quad_perm [1,0,3,2]
    v = op(v, FG_DPP(v, 0x4e, 0xf));     // quad_perm [2,3,0,1]
    v = op(v, FG_DPP(v, 0x124, 0xf));    // row_ror:4
    v = op(v, FG_DPP(v, 0x128, 0xf));    // row_ror:8  -> every lane holds its row's result
    float t = __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), 0x142, 0xa, 0xf, false));   // row_bcast:15 into rows 1, 3
    v = ((threadIdx.x >> 4) & 1) ? op(v, t) : v;
    t = __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), 0x143, 0xc, 0xf, false));         // row_bcast:31 into rows 2, 3
    v = ((threadIdx.x >> 5) & 1) ? op(v, t) : v;
#undef FG_DPP
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}
#ifdef FG_WAVE_SHFL   // (-DFG_WAVE_SHFL: the shuffle form of rounds 1-3, for A/B runs)
__device__ __forceinline__ float fg_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return __shfl(v, 0, 64);
}
__device__ __forceinline__ float fg_wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_down(v, o, 64));
    return __shfl(v, 0, 64);
}
#else
__device__ __forceinline__ float fg_wave_sum(float v) { return fg_wave_reduce_dpp(v, [](float a, float b) { return a + b; }); }
__device__ __forceinline__ float fg_wave_max(float v) { return fg_wave_reduce_dpp(v, [](float a, float b) { return fmaxf(a, b); }); }
#endif
#endif
__device__ __forceinline__ double fg_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return __shfl(v, 0, 64);
}
__device__ __forceinline__ double fg_wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_down(v, o, 64));
    return __shfl(v, 0, 64);
}
// Round 4, k_bicgf_b at the headline size: 15 values per thread through fg_block_sum (shuffle form) + ONE thread splitting and adding
// them all cost 11.7 of the kernel's 36.9 us (knock-out builds, profiles/micro_bicg2d.py) -- every workgroup of these launches is
// resident at once, so a serial per-workgroup tail is exposed.
// Workgroup sum of NV values with the result of value q returned to THREAD q (q < NV): the per-value tails (accumulator split +
// atomics) then run in NV lanes side by side instead of one after the other in thread 0.
template <int NV>
__device__ __forceinline__ fg_real fg_block_sum_lanes(fg_real (&v)[NV], fg_real* lds /* >= NV*4 */) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < NV; ++q) {
        const fg_real s = fg_wave_sum(v[q]);
        if (lane == 0) lds[q * 4 + wave] = s;
    }
    __syncthreads();
    fg_real r = 0;
    if (threadIdx.x < NV) { const int t = threadIdx.x; r = lds[t * 4] + lds[t * 4 + 1] + lds[t * 4 + 2] + lds[t * 4 + 3]; }
    return r;
}
template <int NV>
__device__ __forceinline__ void fg_block_sum(fg_real (&v)[NV], fg_real* lds /* >= NV*4 floats */) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < NV; ++q) {
        const fg_real s = fg_wave_sum(v[q]);
        if (lane == 0) lds[q * 4 + wave] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q < NV; ++q) v[q] = lds[q * 4] + lds[q * 4 + 1] + lds[q * 4 + 2] + lds[q * 4 + 3];
    }
}
#endif  // __HIPCC__

// ------------------------------------------------------------------------------------------------
// host-side state
// ------------------------------------------------------------------------------------------------
// ---- live per-kernel timing (bench.py roofline) ---------------------------------------------------
// Sampled launches go through hipExtLaunchKernelGGL with a start/stop event pair, which timestamps the
// kernel's own dispatch packet (no inter-kernel gap, agrees with rocprofv3 --kernel-trace); a one-wave helper
// kernel snapshots how many systems were still iterating so the algorithmic bytes count only work done.
enum FgProfKind {
    FG_PK_CG_AP = 0, FG_PK_CG_UPDATE, FG_PK_BICG_P, FG_PK_BICG_V, FG_PK_BICG_S, FG_PK_BICG_T, FG_PK_BICG_X,
    FG_PK_GEMM, FG_PK_GEMM_SK, FG_PK_TRIDIAG, FG_PK_DCT, FG_PK_LINE, FG_PK_BICGF_A, FG_PK_BICGF_B, FG_PK_FCG_UPD, FG_PK_FCG_INV,
    FG_PK_FBICG_FWD, FG_PK_FBICG_INV, FG_PK_JAC_PASS, FG_PK_JAC_STREAM, FG_PK_TRIDIAG_FAC,
    // round 6: the streaming kernels of the PISO step around the solves (all envs of the batch counted as live)
    FG_PK_ADV_BUILD, FG_PK_H, FG_PK_DIV, FG_PK_CORRECT, FG_PK_MAXVEL, FG_PK_COUNT
};
#define FG_PROF_POOL 256
struct FgProfMeta { int kind; int nsys; double bytes_per_sys; double flops_per_sys; };
struct FgProf {
    int on, used;
    int prefetched;           // slots whose counts a poll already copied to the host (fg_prof_prefetch)
    hipEvent_t ev[2 * FG_PROF_POOL];
    FgProfMeta meta[FG_PROF_POOL];
    int32_t* active_dev;      // [FG_PROF_POOL] active systems of each sampled launch
    int32_t* active_pinned;   // host-pinned: the count kernel writes it directly; only self-counted slots (active_dev) are copied
    unsigned char self_counted[FG_PROF_POOL];
    double ms[FG_PK_COUNT], bytes[FG_PK_COUNT], flops[FG_PK_COUNT], full_ms[FG_PK_COUNT], full_bytes[FG_PK_COUNT];
    long long n[FG_PK_COUNT], full_n[FG_PK_COUNT], launches[FG_PK_COUNT];
    double all_ms[FG_PK_COUNT];   // every sampled launch, including those that found all systems converged
    long long all_n[FG_PK_COUNT];
};
#define FG_ACC_DOUBLES 16  // reduction accumulators per linear system (see solver kernels)

// Best-iterate tracking (the reference's returnBestResult, cg_solver_kernel.cu:345-361): whenever the RMS residual of
// iterate x_it is less than half that of the last kept iterate (it >= 1), the kernel that is about to overwrite x
// (k_cg_update of iteration it) writes the old x to best_x -- no extra read, one extra store per cell for the envs concerned.  A solve that ends
// unconverged (max iterations, or fp32 stagnation followed by divergence) gets the kept iterate back (within 2x of the lowest residual reached).
// Host polls without hipStreamSynchronize (fg_poll.hip).  A kernel whose results the host waits for -- the convergence checks, the
// flux balance and CFL maximum of fg_single_step -- stores them into host-pinned memory and then, with a system-scope release, the
// poll's sequence number into a pinned word per entry; the host spins on those words.  Measured on MI355X (profiles/scratch/
// poll_latency.hip): kernel -> host -> next kernel costs 6 us this way against 11.5 us through hipStreamSynchronize, 4-5 times per
// PISO step.  Streams are in order, so "the polled kernel has finished" still means everything launched before it has.
struct FgJacHist { int sweeps, skip, fails; };
// the history of a solve kind's sweeps, shared by their drivers (fg_jacobi.hip, fg_linepre.hip).  enter: false while the kind sits out
// the solves its last give-up cost it | gave_up: back off (8, 16, ... 256, then 512 solves) | solved: `sweeps` is what the next solve
// of the kind enqueues ahead of its first poll
inline bool fg_sweeps_enter(FgJacHist& H) { if (H.skip > 0) { --H.skip; return false; } return true; }
inline void fg_sweeps_gave_up(FgJacHist& H) { H.fails += 1; H.skip = H.fails > 6 ? 512 : (4 << H.fails); H.sweeps = 0; }
inline void fg_sweeps_solved(FgJacHist& H, int sweeps) { H.fails = 0; H.sweeps = sweeps; }
// Round 6: result WORDS.  A kernel that publishes through the release above pays a write-back of its XCD's L2 (the 4-5 us the one-wave
// verdict kernels took were that write-back, and the host saw the verdict that much later).  A result that fits 32 bits can instead
// travel IN the word the host spins on: one 8-byte system-scope store {payload, sequence number} per result -- a single store is
// its own ordering, so nothing has to be fenced against anything (the "granule" form of fg_mb_cluster.hip's exchanges).  `gran` is
// the pinned array of such words (nullptr: the fp64 build, or FG_POLL_SPIN=0 -- the kernels then use the mirror + release form).
struct FgPollOut { int32_t* seq; int32_t value; unsigned long long* gran = nullptr; };     // seq == nullptr: no word is written (the caller synchronises the stream)
#ifdef __HIPCC__
__device__ __forceinline__ void fg_poll_publish_word(const FgPollOut& p, int i, uint32_t payload) {
    __hip_atomic_store(p.gran + i, ((unsigned long long)(uint32_t)p.value << 32) | (unsigned long long)payload, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_SYSTEM);
}
// a solve info as two result words: the residual's bits | (used_iterations + 1) << 2 | converged << 1 | is_finite
__device__ __forceinline__ uint32_t fg_info_word(const fg_solve_info& v) {
    return ((uint32_t)(v.used_iterations + 1) << 2) | (v.converged ? 2u : 0u) | (v.is_finite ? 1u : 0u);
}
// Records of W words per entry, written by a whole workgroup (EVERY thread calls): the writers (`valid`) put the record of entry
// first + slot into LDS, then the n entries of the workgroup are stored as one run of consecutive words, 64 per wave instruction -- the
// words cross PCIe as full lines.  (One 8-byte store per workgroup or thread, uncoalesced, made the verdict kernels SLOWER than the
// release form: 128-640 partial-line writes into host memory per poll.)  `stage`: n * W words of LDS.
template <int W>
__device__ __forceinline__ void fg_poll_publish_records(const FgPollOut& p, int first, int n, int slot, const uint32_t (&w)[W], bool valid,
                                                        uint32_t* stage) {
    if (valid)
#pragma unroll
        for (int k = 0; k < W; ++k) stage[slot * W + k] = w[k];
    __syncthreads();
    for (int i = threadIdx.x; i < n * W; i += blockDim.x) fg_poll_publish_word(p, first * W + i, stage[i]);
}
__device__ __forceinline__ void fg_poll_publish(const FgPollOut& p, int i);
// the end of a verdict kernel with one THREAD per system (every thread of the workgroup calls, `valid` = the thread has a system):
// the infos of systems first .. first + n - 1 leave as result words (two per system, fg_poll_wait_infos unpacks them) or, without
// result words, through the mirror + release form.  `stage`: 2 * blockDim.x words of LDS.
__device__ __forceinline__ void fg_poll_publish_infos(const FgPollOut& p, fg_solve_info* mirror, const fg_solve_info* info, int sys, bool valid,
                                                      int first, int n, uint32_t* stage) {
    if (p.gran) {
        uint32_t w[2] = {0u, 0u};
        if (valid) { const fg_solve_info v = info[sys]; w[0] = __float_as_uint((float)v.final_residual); w[1] = fg_info_word(v); }
        fg_poll_publish_records<2>(p, first, n, sys - first, w, valid, stage);
    } else if (valid) {
        mirror[sys] = info[sys];      // host-pinned copy: the poll that follows needs no device-to-host copy
        fg_poll_publish(p, sys);      // (after the entry: the host spins on this word instead of synchronising the stream)
    }
}
// the same end for a verdict kernel with one WAVE per system (fg_acc_total is a wave's shuffle tree): lane 0 is the system's thread;
// mirror == nullptr: nothing is published.  `stage`: 2 words of LDS per wave.
__device__ __forceinline__ void fg_poll_publish_infos_waves(const FgPollOut& p, fg_solve_info* mirror, const fg_solve_info* info, int sys, bool valid,
                                                            int first, int n, uint32_t* stage) {
    if (mirror) fg_poll_publish_infos(p, mirror, info, sys, valid && (threadIdx.x & 63) == 0, first, n, stage);
}
__device__ __forceinline__ void fg_poll_publish(const FgPollOut& p, int i) {
    // system-scope release: the results stored before it (by this thread, or by threads it synchronised with) are visible to the
    // host once the word is.  It writes the L2 back, so a kernel calls it from as few threads as possible, and after all its
    // other work (64 concurrent calls while other workgroups still streamed: k_max_velocity_rows 7.9 -> 18.3 us; fg_publish_max).
    // (A relaxed store behind a workgroup-scope fence was tried: the host then read result words that had not landed yet.)
    if (p.seq) __hip_atomic_store(p.seq + i, p.value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
#endif
struct FgPoll {
    int32_t* seq;      // pinned [n]
    int n; int32_t epoch; int spin, words;    // switches (fg_switches.h, set before fg_poll_create): spin == 0: hipStreamSynchronize; words == 0: no result words
    unsigned long long* gran; int n_gran;      // pinned result words {payload, sequence number} (FgPollOut::gran): 8 per sequence word
};
int fg_poll_create(FgPoll* P, int n);
void fg_poll_destroy(FgPoll* P);
FgPollOut fg_poll_next(FgPoll* P);     // the words and sequence number of the next poll ({nullptr, 0} when spinning is off)
// waits until words [first, first + count) carry out.value (or, without words / after 50 ms of spinning, for the stream)
int fg_poll_wait(FgPoll* P, const FgPollOut& out, int first, int count, hipStream_t st);
// the same for result words [first, first + count) of out.gran; fg_poll_word / fg_poll_info read them afterwards
int fg_poll_wait_words(FgPoll* P, const FgPollOut& out, int first, int count, hipStream_t st);
// infos of systems [first, first + count) into `pinned` (where the mirror form leaves them): result words when the poll has them
int fg_poll_wait_infos(FgPoll* P, const FgPollOut& out, int first, int count, fg_solve_info* pinned, hipStream_t st);
// the wait of a solver's poll round (the caller has launched its verdict kernel with `out`, and whatever it wants to run during the
// round trip): fg_poll_wait_infos, then how many of the systems still iterate (neither converged nor non-finite); < 0: an error code
int fg_poll_wait_active(FgPoll* P, const FgPollOut& out, int first, int count, fg_solve_info* pinned, hipStream_t st);
// the end of a Krylov solve over systems [0, count) (fg_poll.hip).  fg_solve_infos_settle: the infos into s->info_pinned unless a poll
// left them there (`fresh`), and the profiler's samples folded in (the stream is idle afterwards).  fg_solve_infos_report: the infos
// to the caller, the solve's status, *used_max = the largest used_iterations (what the iteration predictors remember)
struct fg_state;
int fg_solve_infos_settle(fg_state* s, int count, bool fresh, hipStream_t st);
int fg_solve_infos_report(const fg_state* s, int count, fg_solve_info* info_host, int* used_max);
inline uint32_t fg_poll_word(const FgPoll* P, int i) { return (uint32_t)(__atomic_load_n(P->gran + i, __ATOMIC_RELAXED) & 0xffffffffull); }
inline float fg_poll_word_float(const FgPoll* P, int i) { const uint32_t u = fg_poll_word(P, i); float f; memcpy(&f, &u, 4); return f; }
inline void fg_poll_info(const FgPoll* P, int sys, fg_solve_info* out) {
    const uint32_t w = fg_poll_word(P, 2 * sys + 1);
    out->final_residual = fg_poll_word_float(P, 2 * sys);
    out->used_iterations = (int32_t)(w >> 2) - 1; out->converged = (w >> 1) & 1; out->is_finite = w & 1;
}
void fg_htrace(const char* tag);      // FG_HTRACE=1: host time stamps (fg_poll.hip); a no-op otherwise
// FG_ROCTX=1: named ranges around the phases of a step for rocprofv3 --marker-trace (fg_poll.hip; a no-op otherwise)
void fg_range_push(const char* name);
void fg_range_pop();
struct FgRange { explicit FgRange(const char* name) { fg_range_push(name); } ~FgRange() { fg_range_pop(); } FgRange(const FgRange&) = delete; FgRange& operator=(const FgRange&) = delete; };

struct FgBest {
    fg_real* best_crit;   // [B] residual of the last kept iterate (leader-only state)
    fg_real* saved_crit;  // [B] residual of the iterate held in best_x (+inf: none)
    int32_t* save_at;   // [B] iteration whose k_cg_update stores x before updating it
    fg_real* best_x;      // [B, N]
};
#ifdef __HIPCC__
// Called by the ONE leader thread of the stencil kernel of iteration `it`, which has just derived crit = RMS residual of
// x_it: keep x_it when it beats the last kept iterate by a factor of two (a healthy solve then pays one extra store pass
// every few iterations, not every iteration -- at 256^3 the every-improvement rule cost 11 % of the CG iteration -- and a
// failed solve gets back an iterate within 2x of the lowest residual it reached).
__device__ __forceinline__ void fg_best_decide(const FgBest& best, int b, fg_real crit, int it) {
    if (it >= 1 && crit < 0.5f * best.best_crit[b]) {
        best.best_crit[b] = crit;
        best.saved_crit[b] = crit;
        best.save_at[b] = it;
    }
}
#endif

// Iteration statistics of the linear solves since the last reset: kind 0 scalar, 1 velocity, 2 / 3 pressure corrector 0 / 1.
// sum / n = mean iterations per SYSTEM (env x component) that took part in a solve; piso_steps counts fg_piso_step calls.
struct FgCounters {
    long long sum[4] = {0, 0, 0, 0}, n[4] = {0, 0, 0, 0}, piso_steps = 0;
    long long unconv[4] = {0, 0, 0, 0};   // systems whose solve ended without meeting its tolerance (iteration cap / best iterate kept)
    int max[4] = {0, 0, 0, 0};
    void add(int kind, const fg_solve_info* info, int count) {
        for (int i = 0; i < count; ++i) {
            const int it = info[i].used_iterations;
            if (it < 0 && info[i].final_residual == 0.f) continue;   // masked-out env (dt <= 0)
            const int v = it + 1;   // used_iterations is the 0-based index of the last iteration (-1: none was needed): a COUNT here
            sum[kind] += v; n[kind] += 1; max[kind] = v > max[kind] ? v : max[kind];
            if (!info[i].converged) unconv[kind] += 1;
        }
    }
    void reset() { *this = FgCounters(); }
    void write(int64_t* out) const {   // [13]: sum[4] | n[4] | max[4] | piso_steps
        for (int k = 0; k < 4; ++k) { out[k] = sum[k]; out[4 + k] = n[k]; out[8 + k] = max[k]; }
        out[12] = piso_steps;
    }
};

// Solver state already prepared by the kernel launched just before a solve (k_adv_build: FgBicgBegin; k_h: FgCgBegin; the divergence
// kernel: FgCgStart) -- the solve then skips its own begin launch.  One record: a producer replaces it, the next solve of either kind
// takes it and leaves none.
struct FgPrepared {
    int bicg_nc; const fg_real* bicg_dt;          // BiCGStab: systems per env, activity mask
    int cg_ns, cg_best; const fg_real* cg_dt;     // CG: accumulator slots, best-iterate tracking, activity mask
    int cg_start;   // 1: the CG was also started from zero (r = b in w[0], x = 0 in p_result, r.r in ring entry 0); 2: and w[3] holds Qx^T r_0 (k_fcg_div_fwd)
    void clear() { *this = FgPrepared{}; }
    void set_bicg(int nc, const fg_real* dt) { clear(); bicg_nc = nc; bicg_dt = dt; }
    void set_cg(int ns, int best, const fg_real* dt) { clear(); cg_ns = ns; cg_best = best; cg_dt = dt; }
    bool cg_for(const fg_real* dt) const { return cg_ns > 0 && cg_dt == dt; }      // the divergence kernel may start this CG ...
    void set_cg_start(int form) { cg_start = form; }                                 // ... and says so (0: it did not)
    bool take_bicg(int nc, const fg_real* dt) { const bool ready = bicg_nc == nc && bicg_dt == dt; clear(); return ready; }
    int take_cg(int ns, int best, const fg_real* dt) {      // -1: not prepared, else cg_start
        const int got = (cg_ns == ns && cg_best == best && cg_dt == dt) ? cg_start : -1; clear(); return got;
    }
};

// A diffusivity as the kernels take it: one value for the batch, or a device array [B] read as per_env[b] where it is installed
// (fg_set_viscosity_batch / fg_set_scalar_viscosity_batch) -- a wave-uniform load per workgroup, the arithmetic behind it unchanged.
struct FgNu {
    fg_real v = 0; const fg_real* per_env = nullptr;
#ifdef __HIPCC__
    __device__ __forceinline__ fg_real at(int b) const { return per_env ? per_env[b] : v; }
#endif
    bool same(const FgNu& o) const { return v == o.v && per_env == o.per_env; }
};

struct fg_state {
    fg_config cfg;
    FgGrid grid;
    int vec;  // 4 if nx % 4 == 0 else 1
    // read through fg_nu() below, nowhere else: per-env arrays (borrowed device [B], nullptr = the scalar) sit next to the scalars
    fg_real viscosity;
    fg_real scalar_viscosity[FG_MAX_SCALARS];
    bool scalar_viscosity_set;
    const fg_real* viscosity_B;
    const fg_real* scalar_viscosity_B[FG_MAX_SCALARS];
    // metrics (owned)
    fg_real* d_h[3];
    fg_real* d_rh[3];
    // bound (borrowed) fields
    fg_real* velocity;
    fg_real* pressure;
    fg_real* scalar;
    fg_real* velocity_source;
    fg_real* visc_field;          // [B,N] per-cell viscosity of the velocity system (FG_VISCOSITY_FIELD) or nullptr
    fg_real* bvel[6];
    fg_real* bscal[6];
    // owned solver workspace
    fg_real* A;          // [B,N]
    fg_real* rA;         // [B,N]
    fg_real* Coff;       // [B,2d,N]
    fg_real* adv_rhs;    // [B,d,N]
    fg_real* vel_result; // [B,d,N]
    fg_real* hvec;       // [B,d,N]   pressureRHS
    fg_real* div;        // [B,N]     pressureRHSdiv
    fg_real* p_result;   // [B,N]
    fg_real* scal_result;// [B,N]
    fg_real* w[8];       // Krylov work vectors, each [B,d,N]
    FgDacc* acc;       // [B*d][FG_ACC_DOUBLES] reduction accumulators (order-independent, FgDacc)
    int32_t* flags;    // [B*d] convergence flags (device)
    fg_solve_info* info_dev;   // [B*d]
    fg_solve_info* info_pinned;// [B*d] host-pinned mirror
    int32_t* flags_pinned;
    fg_real* scratch_B;  // [B*(4+2d)] small per-env floats
    FgProf prof;
    FgDacc* cg_acc;               // [B][FG_CG_NAMES=8][FG_CG_SLOTS=64] slotted CG accumulators
    FgBest cg_best;               // best-iterate tracking of the CG (returnBestResult, cg_solver_kernel.cu:345-361)
    int cg_return_best;           // 1 (default): track; 0: never keep an iterate (fg_set_return_best)
    int cg_reset_steps;           // residual restart period of the pressure CG inside the PISO step (100; fg_set_cg_reset_steps)
    int adv_from_result;          // 1 (default): velocity solve starts from velocityResult; 0: from zero (fg_set_advection_start)
    // y-line right preconditioner of the advection BiCGStab (fg_linepre.hip; fg_set_advection_preconditioner): 0 never (the
    // reference's first rung), 1 every solve (its preconditionBiCG), 2 only to repeat a solve that failed (its
    // BiCG_precondition_fallback); line_retries counts the repeats.  Factors [B][N], allocated on first use
    int adv_precond; long long line_retries;
    int wall_forcing_axis; fg_real wall_forcing_coef[2]; fg_real* force_uniform;   // fg_set_wall_stress_forcing: [B, dims] uniform body force (device)
    FG_SB_SWITCHES(FG_SW_MEMBER)      // every switch member of this handle family: declared, defaulted and described in fg_switches.h
    // fused row kernels (fg_fftcg.hip / fg_fftbicg.hip): alpha_k per env and parity; sum(x_k) per env and parity
    double* fcg_alpha; FgDacc* fcg_xsum;
    // First iterate of the fused CG left unmaterialised (fg_fftcg.hip, k_fcg_check0): fcg_lazy[b] = 1 for an env whose FIRST iterate
    // from zero met the tolerance -- its result is x = alpha_0 z_0 (FgCgOutcome says whether the marks belong to a solve and whether
    // any x was stored).  fcg_first: 0 switches the whole scheme off.
    int32_t* fcg_lazy;
    long jac_spec_missed;      // solves that went round again without the kernels launched behind the sweeps' check kernel (jac_spec, FgSpecHook)
    long jac_floor_released = 0;   // systems the streaming sweeps ended on the fp32-floor rule (measured residual above the tolerance): fg_config_dump
    long fcg_unstored, fcg_first_polls;      // solves that stored no x | solves whose first iterate was polled (fg_config_dump)
    fg_real* line_inv; fg_real* line_cp;
    fg_real* ilu_d;               // [B,N] modified diagonal of the ILU(0) preconditioner (fg_ilu0.hip), built per solve
    // the reference's retry ladder on this path (fg_set_double_fallback, fg_ladder; fg_rung64.h): double_fallback = repeat a failed
    // solve in fp64 before the preconditioned rung; rung_count: velocity / scalar fp64, preconditioned, pressure fp64 repeats;
    // ladder_force (tests): first attempts count as failed (1 advection, 2 pressure, 4 also the advection fp64 rung)
    int double_fallback; int ladder_force; long long rung_count[4];
    double* r64_buf; FgDacc* r64_acc;
    // opt-in mixed-precision refinement of the pressure solve (fg_set_pressure_refinement, fg_poisson.hip): outer corrections allowed (0 = off),
    // target RMS of the fp64 residual, relative tolerance of the fp32 correction solves; fp64 iterate [B][n]; corrections run so far
    int ref64_outer; float ref64_tol, ref64_inner; double* ref64_x; long ref64_corrections;
    // fast-diagonalisation preconditioner factors (device copies; null = not configured)
    float* fd_Qx; float* fd_QxT; float* fd_Qz; float* fd_QzT; float* fd_lower; float* fd_inv; float* fd_cp;   // (fp32 kernels only)
    // separable Helmholtz preconditioner of the advection-diffusion solves (fg_set_fd_helmholtz): eigenvalue sums lam [nz][nx] of the
    // transform axes, per-solve coefficient arrays [B][N] and a [B][d][N] temporary of the basis changes
    float* fd_lam; float* helm_diag; float* helm_lower; float* helm_upper; float* helm_tmp;
    // row form of the 2-D Helmholtz factors (fg_linepre.hip k_helm_factor_y / k_helm_apply_y): lower_j per env and row, 1 / (hx hz),
    // columns per workgroup the last fg_helm_factor chose (0 = the array form)
    float* helm_lower_row; float helm_rs; int helm_cb;
    // second factor set + the record of a factorisation made ahead of the solves (fg_helm_factor_pair): which sets are valid, for which
    // dt array / diffusivity / wall conditions; helm_set = the set the last fg_helm_factor selected for fg_helm_apply
    float* line_inv2; float* line_cp2; float* helm_lower_row2; int helm_pre_mask; const fg_real* helm_pre_dt; FgNu helm_pre_nu[2]; int helm_pre_walls[2][2]; int helm_set;
    // x axis marked as a cosine-transform axis (uniform width, FIXED ends): fg_fdfft.hip replaces the two x GEMMs
    int fd_dct_x; float2* fd_dct_tw; float2* fd_dct_rot; float fd_dct_fwd[2]; float fd_dct_inv[2];
    // row-mean preconditioner of the fused pressure CG (fg_fdprecond.hip k_fd_rowmean_factor): eigenvalues of the x basis [nx], per-env
    // factors [B][N] / [B][ny], epoch of the 1/A field the factors were made from (rA_epoch: bumped by everything that rewrites s->rA)
    float* fd_lam_x; float* fd_row_inv; float* fd_row_cp; float* fd_row_lower; long fd_row_epoch; mutable long rA_epoch;
    float* fd_row_part; long fd_row_part_epoch;   // per-tile row sums of 1/A written by k_adv_build, and the rA epoch they belong to
    // test entries only (fg_debug_apply_*): host array of FG_FORM_SLOTS the preconditioner dispatchers fill with the forms they launch
    // (FG_FORM_* codes of include/fluidgym_hip.h); nullptr on every step path
    int32_t* forms_rec;
    const fg_real* adv_last_dt;   // dt of the last velocity fg_setup_advection (the Helmholtz operator of fg_debug_apply_preconditioner mode 3)
    fg_real** d_bvel_ptrs;   // device copy of bvel[6] (writable pointers for the flux balancing kernel)
    fg_real* diag_pinned;    // [2B] host-pinned: flux balance | max velocity
    fg_real* dt_pinned;      // [B] host-pinned per-env substep sizes of fg_single_step
    fg_real* dt_dev;         // [B]
    double* t_rem_dev;       // [B] FgDtRule::t_rem (fp32 build)
    // iterations the last solve of each KIND needed (the first convergence poll of the next one is scheduled there): advection kinds
    // 0 scalar, 1 velocity; pressure kinds 0 first corrector, 1 later correctors, 2 stand-alone calls.  Until round 5 one predictor per
    // solver served all kinds: the RBC env's second corrector (0-1 iterations) then launched the first corrector's three iterations
    // before its first poll, and the first corrector polled twice
    int pred_bicg[4], pred_cg[4];
    // Jacobi sweeps for the velocity systems of the uniform 2-D grids (fg_jacobi.hip): switch (fg_switches.h / fg_set_advection_jacobi)
    // and whether the environment set it, per-kind history (sweeps the last solve needed; solves still to skip after a failure), pinned residuals of the pass before the last
    int adv_jacobi, adv_jacobi_env; FgJacHist jac_hist[4]; float* jac_prev;
    long long jac_solves, jac_fallbacks;
    long jac_rA_epoch;      // rA_epoch at which rA = 1 / A was written for the velocity system in s->A (the streaming sweeps read it)
    FgCounters ctr;         // iterations per solve kind since the last reset (fg_solver_counters)
    const fg_real* cur_dt;  // dt_B of the last fg_setup_advection: activity mask of the stepwise entry points
    FgPoll poll;                  // host polls of this handle (fg_poll.hip)
    mutable int maxvel_clean;     // scratch_B rows 1-2 (CFL maximum + arrival counters) are zero: left so by the mirrored k_max_velocity
    FgPrepared prepared;          // kept on the handle: the stepwise entry points (fg_setup_pressure_rhs, then fg_solve_pressure) hand it across calls
    fg_env_sel* env_sel_dev;      // [B] selection records of the last fg_env_restore_field / fg_env_reset_solver_state (fg_envrestore.hip)
    size_t n_cells() const { return (size_t)grid.n; }
};
// THE reader of the handle's viscosity and scalar diffusivities (getViscosity(domain, forPassiveScalar, ch),
// PISO_multiblock_cuda_kernel.cu:1803-1815): a channel's own array, else its scalar once any channel was set, else the velocity's
inline FgNu fg_nu(const fg_state* s, int for_scalar = 0, int channel = 0) {
    FgNu n;
    if (for_scalar && s->scalar_viscosity_B[channel]) { n.v = s->scalar_viscosity[channel]; n.per_env = s->scalar_viscosity_B[channel]; }
    else if (for_scalar && s->scalar_viscosity_set) n.v = s->scalar_viscosity[channel];
    else { n.v = s->viscosity; n.per_env = s->viscosity_B; }
    return n;
}

void fg_set_error(const std::string& msg);
// argument / state check of an extern "C" entry point: record the message for fg_last_error() and return the status
#define FG_REQUIRE(cond, code, msg)  \
    do {                             \
        if (!(cond)) {               \
            fg_set_error(msg);       \
            return code;             \
        }                            \
    } while (0)
#define FG_HIP_CHECK(expr)                                                                        \
    do {                                                                                          \
        hipError_t _e = (expr);                                                                   \
        if (_e != hipSuccess) {                                                                   \
            fg_set_error(std::string(#expr) + ": " + hipGetErrorString(_e));                      \
            return FG_ERR_HIP;                                                                    \
        }                                                                                         \
    } while (0)

// dims / vector-width dispatch for templated launches; the body sees constexpr DIMS and VEC
#if FG_F64
// fp64 build: scalar lanes only (the float4 paths of fg_load / fg_store are fp32 idioms)
#define FG_DISPATCH(s, ...)                                                       \
    do {                                                                          \
        if ((s)->grid.dims == 2) { constexpr int DIMS = 2, VEC = 1; __VA_ARGS__; } \
        else { constexpr int DIMS = 3, VEC = 1; __VA_ARGS__; }                    \
    } while (0)
#else
#define FG_DISPATCH(s, ...)                                                       \
    do {                                                                          \
        if ((s)->grid.dims == 2) {                                                \
            if ((s)->vec == 4) { constexpr int DIMS = 2, VEC = 4; __VA_ARGS__; }  \
            else { constexpr int DIMS = 2, VEC = 1; __VA_ARGS__; }                \
        } else {                                                                  \
            if ((s)->vec == 4) { constexpr int DIMS = 3, VEC = 4; __VA_ARGS__; }  \
            else { constexpr int DIMS = 3, VEC = 1; __VA_ARGS__; }                \
        }                                                                         \
    } while (0)
#endif

// launchers implemented in the kernel translation units -----------------------------------------
// State of the BiCGStab solve that follows an assembly, prepared by the assembly kernel itself (what a k_bicg_begin launch does:
// accumulators and scalars reset, flags from the activity mask, info cleared); acc == nullptr: not folded.
struct FgBicgBegin { FgDacc* acc; fg_real* sc; int32_t* flags; fg_solve_info* info; int nc; };
#ifdef __HIPCC__
__device__ __forceinline__ void fg_bicg_begin_sys(const FgBicgBegin& q, const fg_real* __restrict__ dt, int sys) {
    for (int k = 0; k < FG_ACC_DOUBLES; ++k) acc_st(q.acc + ((size_t)sys * FG_ACC_DOUBLES + k), 0.0);
    sc_st(q.sc + (sys * 2), 1.f); sc_st(q.sc + (sys * 2 + 1), 1.f);
    const bool active = (dt == nullptr) || (dt[sys / q.nc] > 0.f);
    flag_st(q.flags + (sys), active ? 0 : 3);
    q.info[sys].final_residual = 0.f;
    q.info[sys].used_iterations = -1;
    q.info[sys].converged = active ? 0 : 1;
    q.info[sys].is_finite = 1;
}
#endif
struct FgAdvArgs {
    const fg_real* vel;      // u^n [B,d,N]
    const fg_real* scal;     // T channel [B,?] base of the channel being advected (stride given)
    long scal_env_stride;  // elements between envs in `scal`
    const fg_real* source;   // velocity source [B,d,N] or nullptr
    const fg_real* force;    // uniform body force per env [B,d] or nullptr (fg_set_wall_stress_forcing): added like a source of that value
    const fg_real* dt;       // [B]
    FgNu nu;                 // viscosity (or scalar diffusivity): the batch's value or a per-env array
    const fg_real* visc;     // optional per-cell viscosity [B,N] of the velocity system (Block.setViscosity: SGS models); nullptr = nu
    int for_scalar;
    int channel, n_scalars;
    fg_real* A; fg_real* Coff; fg_real* rhs;
    fg_real* rA;             // optional: 1/A written alongside A (velocity system only)
    FgBicgBegin begin;       // optional (begin.acc != nullptr): the leader workgroup of every env prepares the solve that follows
    // optional (buoy_T != nullptr, velocity system): the RBC envs' PRE_VELOCITY_SETUP hook folded in -- the source is
    // S[axis] = factor * T, S[other] = 0 (rbc_env_base.py:285-297), used here AND written to `source_w` (the block's velocitySource
    // keeps the value the hook would have left) instead of being materialised by a k_buoyancy launch and read back
    const fg_real* buoy_T; long buoy_stride; int buoy_axis; fg_real buoy_factor; fg_real* source_w;
    fg_real* row_part;       // optional (2-D, float4 lanes): per-tile row sums of 1/A, [B][ny][tiles_x] (row-mean preconditioner, fg_fdprecond.hip)
};
int fg_launch_adv_build(fg_state* s, const FgBounds& bnd, const FgAdvArgs& a, hipStream_t st);      // (fg_state*: these three launches record what they prepared, FgPrepared)
int fg_launch_wall_forcing(const fg_state* s, hipStream_t st);   // force_uniform from the wall-adjacent layers of s->velocity
int fg_launch_sgs(const fg_state* s, const FgBounds& bnd, fg_real coefficient, fg_real* out, hipStream_t st);
int fg_launch_pressure_setup(const fg_state* s, const fg_real* dt, hipStream_t st);  // rA = 1/A
int fg_launch_h(fg_state* s, const fg_real* dt, const fg_real* vel_result, hipStream_t st);
int fg_launch_div(fg_state* s, const FgBounds& bnd, const fg_real* dt, const fg_real* hvec, fg_real* div, hipStream_t st,
                  bool cg_from_zero = false,    // true: the kernel also starts the pressure CG that follows from zero (FgCgStart, fg_cg.h)
                  bool fused_fwd = false);      // true (with cg_from_zero): the solve is the FD-preconditioned CG -- where the fused row kernels cover the grid, right-hand side, start and first forward transform are ONE launch (k_fcg_div_fwd)
// mean (optional): the corrector also writes p - mean(p) of active envs to p_copy (the block pressure: setPressureResult +
// CopyPressureResultToBlocks, PISOtorch_simulation.py:1922-1925, 1953, without the two passes of fg_launch_mean_sub), the sum of
// env b's pressure being sums[2 b + (info[b].used_iterations & 1)] (0 for a solve that took no iteration: x = 0)
// lazy / alpha (optional, FgLazyRef below): an env marked lazy took ONE iteration from zero, x = alpha z, and its sum is alpha * sums[2 b + 1]
struct FgMeanRef { const FgDacc* sums; const fg_solve_info* info; fg_real* p_copy; const int32_t* lazy; const double* alpha; };
// The pressure the corrector reads is not stored: `p` is z_0 of the fused CG and env b's pressure is alpha[2 b] * z (lazy[b] == 1) or
// zero (lazy[b] == 0: the env stopped at its start vector).  p_res (optional): the corrector also stores it (pressureResult).
struct FgLazyRef { const int32_t* lazy; const double* alpha; fg_real* p_res; };
int fg_launch_correct(const fg_state* s, const fg_real* dt, const fg_real* rA, const fg_real* hvec, const fg_real* p,
                      fg_real* vel_out, hipStream_t st, fg_real* vel_copy = nullptr, const FgMeanRef* mean = nullptr, const FgLazyRef* lazy = nullptr);
// mirror_B: optional host-pinned [B] the last workgroup of each env publishes the result to (out_B must then be
// scratch_B + B, whose next row holds the arrival counters)
// poll (optional): sequence words published per env after the host-pinned result (FgPollOut above)
// FgDtRule (round 6): the adaptive sub-step of fg_single_step taken ON THE DEVICE by the workgroup that finishes the CFL maxima (the
// reference's rule, PISOtorch_simulation.py:2013-2031, in the same doubles the host uses -- which repeats it from the published maxima
// for its own bookkeeping): t_rem [B] the time an env still has to cover in this sim step (reset to time_step when `reset`), dt_out [B]
// the sub-step the kernels of the PISO step read.  The host then needs the maxima only AFTER the PISO step (loop control), not
// before it: no round trip between the CFL kernel and the step's first kernels.  t_rem == nullptr: off.
struct FgDtRule { double* t_rem; fg_real* dt_out; float cfl; double time_step; int reset; };
int fg_launch_max_velocity(const fg_state* s, const FgBounds& bnd, fg_real* out_B, hipStream_t st, fg_real* mirror_B = nullptr,
                           FgPollOut poll = FgPollOut{nullptr, 0}, fg_real* flux_B = nullptr, fg_real* flux_mirror = nullptr,   // flux_B: device [B] scratch, the flux-balance guard computed in the same launch and mirrored to flux_mirror (host-pinned)
                           FgDtRule rule = FgDtRule{nullptr, nullptr, 0.f, 0.0, 0});
int fg_launch_flux_balance(const fg_state* s, const FgBounds& bnd, fg_real* out_B, hipStream_t st, FgPollOut poll = FgPollOut{nullptr, 0});
int fg_launch_copy_active(const fg_state* s, const fg_real* dt, const fg_real* src, fg_real* dst, int comps, hipStream_t st);
int fg_launch_buoyancy(const fg_state* s, const fg_real* dt, const fg_real* T, long t_env_stride, fg_real* source, int axis,
                       fg_real factor, hipStream_t st);
int fg_launch_outflow(const fg_state* s, int face, fg_real velm_axis, const fg_real* dt, hipStream_t st);
int fg_launch_balance(const fg_state* s, const FgBounds& bnd, int free_mask, fg_real atol, const fg_real* dt, hipStream_t st,
                      int outflow_mask = 0, const fg_real* outflow_velm = nullptr,    // outflow_mask: faces whose convective update rides in this launch
                      const fg_real* dt_host_values = nullptr);                       // B <= 64 time steps by value: the kernel fills s->dt_dev (no copy in front of it)
bool fg_outflow_folds(const fg_state* s, int outflow_mask);
int fg_launch_mean_sub(const fg_state* s, const fg_real* active_dt, fg_real* p, fg_real* p_copy, hipStream_t st);

// Poisson / CG (fg_poisson.hip)
int fg_poisson_apply_launch(const fg_state* s, const fg_real* rA, const fg_real* x, fg_real* y, hipStream_t st);
int fg_poisson_jacobi_launch(const fg_state* s, const fg_real* rA, const fg_real* b, const fg_real* x, fg_real* xnew,
                             fg_real omega, hipStream_t st);
int fg_poisson_rbgs_launch(const fg_state* s, const fg_real* rA, const fg_real* b, fg_real* x, fg_real omega, int color,
                           hipStream_t st);
// What a pressure solve left behind.  The default is the plain case: the result is stored in x and nothing else holds.
struct FgCgOutcome {
    const fg_real* lazy_z = nullptr;   // != nullptr: every env ended on its first iterate from zero (or at its start vector) and NO x was stored -- env b's result is fcg_alpha[2 b] * lazy_z where fcg_lazy[b] == 1, zero elsewhere (FgLazyRef)
    bool mean_ready = false;           // sum(x) of the result is in fcg_xsum[b][used_iterations & 1] (FgMeanRef)
    bool marks_valid = false;          // fcg_lazy[] belongs to this solve (k_fcg_check0 ran)
    bool spec_done = false;            // the corrector of FgCgSpec ran on this very result
};
// The corrector launched BEHIND k_fcg_check0, before the host knows the verdict: `fn` gets the outcome the solve will have if every
// env ends on its first iterate -- the common case: the corrector has then already run while the host turned the poll around
// (FgCgOutcome::spec_done); otherwise its output is overwritten by the corrector that follows the finished solve (same inputs: it reads
// h, 1/A and z / x, writes the velocity result and, in the last corrector, the block fields nothing reads in between).
struct FgCgSpec { int (*fn)(void* ctx, const FgCgOutcome& o) = nullptr; void* ctx = nullptr; };
struct FgCgArgs {
    const fg_real* rA; const fg_real* b; fg_real* x;
    fg_real* r; fg_real* p; fg_real* Ap;
    const fg_real* dt;   // [B] activity mask (nullptr = all active)
    fg_real tol; int max_iterations; int use_x0; int reset_steps;
    int check_every;
    int precond;   // 1: fast-diagonalisation preconditioned CG (needs fg_set_fd_preconditioner)
    int kind = 2;  // which poll predictor the solve reads and updates (fg_state::pred_cg)
    int lazy_ok = 0;   // the caller can read an unstored result through FgLazyRef (FgCgOutcome::lazy_z; the fused PISO step)
    FgCgSpec spec;     // optional
};
int fg_cg_solve(fg_state* s, const FgCgArgs& a, fg_solve_info* info_host, hipStream_t st, FgCgOutcome* out = nullptr);

// BiCGStab on the stencil-form advection matrix (fg_bicgstab.hip)
// The first kernels of the corrector -- k_h, the divergence kernel -- launched BEHIND the sweeps' check kernel, before the host knows
// the verdict (on-chip form, one planned pass writing the result vector): they read what the sweeps left and write h, the right-hand
// side and the CG's start, so the velocity solve's own device state (flags, sums) is gone once they ran -- a verdict that does not
// end the solve there (0.6 % of the soak's solves: profiles/r05_soak_first_iterate.jsonl) is FG_SWEEP_SPEC_MISSED.
struct FgSpecHook { int (*fn)(void* ctx) = nullptr; void* ctx = nullptr; };
struct FgBicgArgs {
    const fg_real* diag; const fg_real* off;  // [B,N], [B,2d,N]
    const fg_real* rhs; fg_real* x;           // [B,nc,N]
    int nc;
    const fg_real* dt;
    fg_real tol; int max_iterations; int use_x0;
    int precond = 0;   // 3: by ILU(0) of the matrix (fg_ilu0.hip, the reference's preconditioner);
                       // 1: right-preconditioned by the y-line solve of fg_linepre.hip (v = C M^-1 p, t = C M^-1 s); 2: by the
                       // separable Helmholtz operator I/dt - nu Laplacian (fast diagonalisation, fg_fd_helmholtz_apply)
    FgNu nu; int wall_lo = 1, wall_hi = 1;          // precond == 2: diffusivity of this solve; the variable is prescribed at the -y / +y wall
    int kind = 1;      // which poll predictor the solve reads and updates (fg_state::pred_bicg): 0 scalar, 1 velocity
    FgSpecHook spec;   // optional
};
// *spec_ran (optional): the kernels of a.spec ran on the result of this solve
int fg_bicgstab_solve(fg_state* s, const FgBicgArgs& a, fg_solve_info* info_host, hipStream_t st, bool* spec_ran = nullptr);
#if !FG_F64
// stationary sweeps instead of the Krylov iteration where the rows are diagonally dominant (fg_jacobi.hip)
enum FgSweepOutcome {
    FG_SWEEP_NOT_TRIED,     // the kind is backing off: the prepared solve state is untouched
    FG_SWEEP_SOLVED,
    FG_SWEEP_SOLVED_SPEC,   // solved, and the kernels of FgSpecHook ran on the result
    FG_SWEEP_GAVE_UP,       // the caller runs its Krylov solver from a cleared start vector behind a fresh k_bicg_begin
    FG_SWEEP_SPEC_MISSED,   // the kernels of FgSpecHook overwrote the state of a solve that was not over: the whole solve again, without them
};
bool fg_jacobi_ok(const fg_state* s, const FgBicgArgs& a);
// line sweeps x <- (D + O_y)^-1 (b - O_x x) for the Helmholtz-preconditioned family (wall-refined 2-D grids: RBC); fg_linepre.hip, round 6
bool fg_linesweep_ok(const fg_state* s, const FgBicgArgs& a);
int fg_linesweep_solve(fg_state* s, const FgBicgArgs& a, fg_solve_info* info_host, hipStream_t st, FgSweepOutcome* outcome);
int fg_jacobi_solve(fg_state* s, const FgBicgArgs& a, fg_solve_info* info_host, hipStream_t st, FgSweepOutcome* outcome);
#endif
// fp64 repeats of failed solves (fg_rung64.h; fp32 library only): every system of an env that has a failed one (BiCGStab: not
// converged; CG: non-finite), info_host updated in place; returns the status of the repeated solves (*out: the result is stored in a.x)
int fg_rung64_bicgstab(fg_state* s, const FgBicgArgs& a, fg_solve_info* info_host, bool all_systems, hipStream_t st);
int fg_rung64_cg(fg_state* s, const FgCgArgs& a, fg_solve_info* info_host, bool all_envs, hipStream_t st, FgCgOutcome* out);

// z-marching 3-D variants (fg_poisson3d.hip)
bool fg_zmarch_ok(const fg_state* s, int* zc_out);
int fg_zmarch_apply(const fg_state* s, const fg_real* rA, const fg_real* x, fg_real* y, int zc, hipStream_t st);
int fg_zmarch_relax(const fg_state* s, const fg_real* rA, const fg_real* b, const fg_real* x, fg_real* xnew, fg_real omega,
                    int color, int zc, hipStream_t st);
int fg_zmarch_cg_ap(const fg_state* s, const fg_real* rA, const fg_real* z, const fg_real* p_in, fg_real* p_out, fg_real* Ap,
                    FgDacc* acc, int32_t* flags, fg_solve_info* info, int prof_slot, fg_real tol, int it, int first,
                    int ns, int num_base, int zc, hipStream_t st);
// profiler (fg_profile.hip).  fg_prof_slot returns an event-pair slot when this launch is to be sampled (-1 otherwise);
// flags == nullptr means all nsys systems are active; flags == FG_PROF_SELF means the sampled kernel itself adds
// its active systems to prof.active_dev[slot] (kernels that retire systems in the same launch).  fg_prof_collect folds finished samples into the sums and
// must be called with the stream idle.
#define FG_PROF_SELF ((const int32_t*)(uintptr_t)1)
int fg_prof_slot(const fg_state* s, int kind, const int32_t* flags, int nsys, double bytes_per_sys,
                 double flops_per_sys, hipStream_t st);
int fg_prof_collect(fg_state* s, hipStream_t st);
// Called right before a solver poll waits for the stream: the counts of the samples taken so far ride along with that wait, so
// the collect that follows a poll which ends the solve needs neither a copy nor a second stream synchronisation (that second
// round trip per solve was most of what live profiling cost the timed region: 2 700 -> 2 900 env-steps/s on the headline)
void fg_prof_prefetch(fg_state* s, hipStream_t st);
void fg_prof_destroy(fg_state* s);
bool fg_fd_dct_supported(int n);
struct FgCgJudge;   // fg_cg.h: residual verdict folded into the first kernel of a preconditioner application (nullptr: none)
int fg_fd_dct_forward(fg_state* s, const fg_real* r, fg_real* out, hipStream_t st, int batch = 0, const FgCgJudge* judge = nullptr);   // batch 0: the env batch
int fg_fd_dct_inverse(fg_state* s, const fg_real* u, fg_real* z, const fg_real* dot_with, FgDacc* dot_acc, int dot_stride,
                      int dot_ns, hipStream_t st, int batch = 0);
#define FG_LAUNCH_P(s, slot, kernel, grid, block, shmem, st, ...)                                              \
    do {                                                                                                       \
        const int slot__ = (slot);                                                                             \
        if (slot__ >= 0)                                                                                       \
            hipExtLaunchKernelGGL(kernel, grid, block, shmem, st, (s)->prof.ev[2 * slot__],                    \
                                  (s)->prof.ev[2 * slot__ + 1], 0, __VA_ARGS__);                               \
        else                                                                                                   \
            hipLaunchKernelGGL(kernel, grid, block, shmem, st, __VA_ARGS__);                                   \
    } while (0)
// expect_active: the caller's estimate of envs still iterating (<= 0: all) -- only picks the GEMM tile shape
int fg_fd_apply(fg_state* s, const fg_real* r, fg_real* z, FgDacc* rz_acc, int rz_stride, int rz_ns, int expect_active,
                hipStream_t st, const FgCgJudge* judge = nullptr);
struct FgCgLead;    // fg_cg.h
int fg_fd_tridiag(fg_state* s, float* cur, hipStream_t st, const FgCgLead* lead, bool use_rowmean = false, const float* factor_from = nullptr, const float* factor_dt = nullptr);
bool fg_fd_tridiag_can_factor(const fg_state* s);      // the tridiagonal launch can make the row-mean factors itself (round 6)   // the per-mode Thomas solve of fg_fd_apply alone (in place); use_rowmean: the per-env factors of fg_fd_rowmean_factor
bool fg_fd_rowmean_ok(const fg_state* s);
int fg_refine64_pressure(fg_state* s, const FgCgArgs& a0, fg_solve_info* info_host, hipStream_t st, FgCgOutcome* out);   // fg_poisson.hip (fp32 library only)
int fg_fd_rowmean_factor(fg_state* s, const float* rA, const float* dt, hipStream_t st, const float* row_part = nullptr, int tiles_x = 0);
// the factors for the CURRENT 1/A field ahead of the pressure solves that will want them (fg_cg_solve then finds them made): launched
// behind a polled kernel, the factorisation -- 14 us, latency-sized, independent of the velocity solve -- runs while the host turns the
// poll around instead of in front of the first tridiagonal solve.  A no-op where the fused CG / the row-mean operator do not apply.
int fg_fd_rowmean_prefactor(fg_state* s, const fg_real* dt, hipStream_t st);
// y-line preconditioner (fg_linepre.hip): buffers, Thomas factorisation of the tridiagonal part of (diag, off) along y for every env
// with a live system, z = M^-1 r for every live system
int fg_line_alloc(fg_state* s);
// ILU(0) of the stencil-form matrix (fg_ilu0.hip): the reference's own preconditioner of the BiCGStab rungs
int fg_ilu_alloc(fg_state* s);
int fg_ilu_factor(fg_state* s, const fg_real* diag, const fg_real* off, hipStream_t st);
int fg_ilu_apply(fg_state* s, const fg_real* diag, const fg_real* off, int nc, const fg_real* r, fg_real* z, hipStream_t st);
int fg_helm_alloc(fg_state* s);
int fg_helm_factor(fg_state* s, const fg_real* dt, FgNu nu, int wall_lo, int wall_hi, int nc, hipStream_t st, int kind = -1);
int fg_helm_factor_pair(fg_state* s, const float* dt, const FgNu nu[2], const int wall_lo[2], const int wall_hi[2], hipStream_t st);
int fg_helm_apply(fg_state* s, int nc, const float* r, float* z, hipStream_t st);   // z = M^-1 r with the factors of the last fg_helm_factor (r == z allowed)
// z = M^-1 r with M the separable Helmholtz operator factorised by fg_helm_factor: basis change along x (and z), tridiagonal solve
// along y per mode and env, basis change back (fg_fdprecond.hip)
int fg_fd_helmholtz_apply(fg_state* s, int nc, const fg_real* r, fg_real* z, hipStream_t st);
int fg_line_factor(fg_state* s, const fg_real* diag, const fg_real* off, int nc, hipStream_t st);
int fg_line_apply(fg_state* s, const fg_real* diag, const fg_real* off, int nc, const fg_real* r, fg_real* z, hipStream_t st);
int fg_metrics_launch(const float* coords, float* transforms, int dims, int nx, int ny, int nz, hipStream_t st);
