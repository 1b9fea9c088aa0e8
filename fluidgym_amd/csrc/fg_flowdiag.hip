// Velocity-gradient diagnostics of the bound velocity (fg_flow_diagnostic, fg_mb_flow_diagnostic): the gradient tensor, vorticity,
// its magnitude, the Q criterion and the strain-rate norm, per cell, for the whole env batch in ONE launch per call.
//
// The reference builds all of these on ComputeSpatialVelocityGradients = getBlockDataGradient per velocity component
// (PISO_multiblock_cuda_kernel.cu:2997-3040, 6460-6553).  For component i and computational axis a:
//   lo / hi   the value across face 2a / 2a + 1 of the cell: the neighbour cell's u_i across an interior, periodic or connected face
//             (the VALUE only: no axis mapping, also across a rotated connection), the face's Dirichlet velocity across a prescribed one
//   c[i][a] = (hi - lo) / dist,  dist = 2 - 0.5 (prescribed faces among the two): a boundary value sits half a cell away
//   g[i][j] = d u_i / d x_j = sum_a c[i][a] Minv[a][j]     (single-block: Minv is diagonal, g[i][a] = c[i][a] rh_a)
// The derived kinds form their invariant from g in registers; the d x d tensor is never written and read back.
//
// Both kernels are gathers without reuse across envs, i.e. memory-bound:
//   single-block  lanes run along x (a wave's loads and stores of a row are contiguous); a thread marches FD_ROWS rows in y and keeps
//                 the three-row window of every component in registers, the x and z neighbours come from the cache lines the
//                 neighbouring lanes / planes load anyway.  The spacing comes from FgGrid.
//   multi-block   one thread per (cell, env); nbr[f][i] and T[i] are read once per thread, are shared by all envs and stay in L2.
// No atomics, no cross-lane operation, nothing returns to the host.
//
// This file is compiled with -ffp-contract=off (its own rule in the Makefile): every product and sum is rounded on its own, so
// FG_DIAG_GRADIENT and the derived kinds see the same gradient bits in every template instance.
#include "fg_mb.h"

namespace {

constexpr int FD_ROWS = 4;   // rows a thread of the single-block kernel marches in y

__host__ __device__ constexpr int fd_channels(int dims, int kind) {
    return kind == FG_DIAG_GRADIENT ? dims * dims : (kind == FG_DIAG_VORTICITY ? (dims == 2 ? 1 : 3) : 1);
}

template <typename R> __device__ __forceinline__ R fd_sqrt(R x) {
    if constexpr (std::is_same<R, double>::value) return sqrt(x); else return sqrtf(x);
}
template <typename R> __device__ __forceinline__ R fd_abs(R x) {
    if constexpr (std::is_same<R, double>::value) return fabs(x); else return fabsf(x);
}

// the channels of `KIND` from the gradient g[component][direction] of one cell; channel k goes to out[k * cs]
template <typename R, int DIMS, int KIND>
__device__ __forceinline__ void fd_emit(const R (&g)[DIMS][DIMS], R* __restrict__ out, size_t cs) {
    if constexpr (KIND == FG_DIAG_GRADIENT) {
#pragma unroll
        for (int i = 0; i < DIMS; ++i)
#pragma unroll
            for (int j = 0; j < DIMS; ++j) out[(size_t)(i * DIMS + j) * cs] = g[i][j];
    } else if constexpr (KIND == FG_DIAG_VORTICITY || KIND == FG_DIAG_VORTICITY_MAGNITUDE) {
        if constexpr (DIMS == 2) {
            const R w = g[1][0] - g[0][1];
            out[0] = KIND == FG_DIAG_VORTICITY ? w : fd_abs(w);
        } else {
            const R w0 = g[2][1] - g[1][2], w1 = g[0][2] - g[2][0], w2 = g[1][0] - g[0][1];
            if constexpr (KIND == FG_DIAG_VORTICITY) { out[0] = w0; out[cs] = w1; out[2 * cs] = w2; }
            else out[0] = fd_sqrt((w0 * w0 + w1 * w1) + w2 * w2);
        }
    } else if constexpr (KIND == FG_DIAG_Q) {
        R ss = 0, oo = 0;    // Frobenius norms of S = sym(g) and Omega = skew(g)
#pragma unroll
        for (int i = 0; i < DIMS; ++i)
#pragma unroll
            for (int j = 0; j < DIMS; ++j) {
                const R s = (R)0.5 * (g[i][j] + g[j][i]), o = (R)0.5 * (g[i][j] - g[j][i]);
                ss += s * s;
                oo += o * o;
            }
        out[0] = (R)0.5 * (oo - ss);
    } else {
        // |S| = sqrt(2 S:S), summed as k_sgs_smagorinsky sums it (fg_piso.hip)
        R d = 0;
#pragma unroll
        for (int i = 0; i < DIMS; ++i)
#pragma unroll
            for (int j = i; j < DIMS; ++j) {
                R sij = (R)0.5 * (g[i][j] + g[j][i]);
                sij *= sij;
                d += (i != j) ? (R)2 * sij : sij;
            }
        out[0] = fd_sqrt((R)2 * d);
    }
}

// (hi - lo) / (2 - 0.5 prescribed faces)
template <typename R> __device__ __forceinline__ R fd_diff(R lo, R hi, int prescribed) {
    return (hi - lo) / ((R)2 - (R)0.5 * (R)prescribed);
}

// Single-block.  A workgroup covers 64 cells in x and four chunks of FD_ROWS rows (one per wave); chunks run over y, then z.
template <typename R, int DIMS, int KIND>
__global__ __launch_bounds__(FG_BLOCK) void k_flow_diag(FgGrid g, FgBounds bnd, const R* __restrict__ vel, R* __restrict__ out, int tiles_x,
                                                         int chunks_y, int groups) {
    constexpr int K = fd_channels(DIMS, KIND);
    unsigned bid = blockIdx.x;
    const int tix = (int)(bid % (unsigned)tiles_x);
    bid /= (unsigned)tiles_x;
    const int grp = (int)(bid % (unsigned)groups), b = (int)(bid / (unsigned)groups);
    const int x = tix * 64 + (int)(threadIdx.x & 63), chunk = grp * 4 + (int)(threadIdx.x >> 6);
    const int nx = g.nx, ny = g.ny, nz = DIMS == 3 ? g.nz : 1;
    if (x >= nx || chunk >= chunks_y * nz) return;
    const int z = chunk / chunks_y, y0 = (chunk - z * chunks_y) * FD_ROWS, y1 = min(y0 + FD_ROWS, ny);
    const size_t n = (size_t)g.n, plane = (size_t)nx * ny;
    const R* __restrict__ u = vel + (size_t)b * DIMS * n;
    R* __restrict__ o = out + (size_t)b * K * n;

    // x: the neighbour columns (periodic wrap) or the prescribed faces of the first / last column
    const bool px_lo = x == 0 && g.fixed[0], px_hi = x + 1 == nx && g.fixed[1];
    const int xm = x == 0 ? nx - 1 : x - 1, xp = x + 1 == nx ? 0 : x + 1;
    const R rhx = g.rh[0][x];
    // boundary slabs [B][d][slab], slab index = the remaining axes, lowest fastest
    const size_t slab_x = (size_t)ny * nz, slab_y = (size_t)nx * nz, slab_z = plane;
    // z: the neighbour planes
    bool pz_lo = false, pz_hi = false;
    size_t zm = 0, zp = 0;
    R rhz = 0;
    if constexpr (DIMS == 3) {
        pz_lo = z == 0 && g.fixed[4]; pz_hi = z + 1 == nz && g.fixed[5];
        zm = (size_t)(z == 0 ? nz - 1 : z - 1) * plane; zp = (size_t)(z + 1 == nz ? 0 : z + 1) * plane;
        rhz = g.rh[2][z];
    }
    const size_t zbase = (size_t)z * plane;

    // the y window: below, centre, above -- `below` of the first row may be a boundary value
    R um[DIMS], uc[DIMS], up[DIMS];
#pragma unroll
    for (int q = 0; q < DIMS; ++q) {
        const R* uq = u + (size_t)q * n + zbase;
        uc[q] = uq[(size_t)y0 * nx + x];
        if (y0 > 0) um[q] = uq[(size_t)(y0 - 1) * nx + x];
        else if (g.fixed[2]) um[q] = bnd.vel[2][((size_t)b * DIMS + q) * slab_y + (size_t)z * nx + x];
        else um[q] = uq[(size_t)(ny - 1) * nx + x];
    }
    for (int j = y0; j < y1; ++j) {
        const bool py_lo = j == 0 && g.fixed[2], py_hi = j + 1 == ny && g.fixed[3];
        const R rhy = g.rh[1][j];
        const size_t row = zbase + (size_t)j * nx;
        R grad[DIMS][DIMS];
#pragma unroll
        for (int q = 0; q < DIMS; ++q) {
            const R* uq = u + (size_t)q * n;
            if (j + 1 < ny) up[q] = uq[row + nx + x];
            else if (g.fixed[3]) up[q] = bnd.vel[3][((size_t)b * DIMS + q) * slab_y + (size_t)z * nx + x];
            else up[q] = uq[zbase + x];
            const R xl = px_lo ? bnd.vel[0][((size_t)b * DIMS + q) * slab_x + (size_t)z * ny + j] : uq[row + xm];
            const R xh = px_hi ? bnd.vel[1][((size_t)b * DIMS + q) * slab_x + (size_t)z * ny + j] : uq[row + xp];
            grad[q][0] = fd_diff(xl, xh, (int)px_lo + (int)px_hi) * rhx;
            grad[q][1] = fd_diff(um[q], up[q], (int)py_lo + (int)py_hi) * rhy;
            if constexpr (DIMS == 3) {
                const R zl = pz_lo ? bnd.vel[4][((size_t)b * DIMS + q) * slab_z + (size_t)j * nx + x] : uq[zm + (size_t)j * nx + x];
                const R zh = pz_hi ? bnd.vel[5][((size_t)b * DIMS + q) * slab_z + (size_t)j * nx + x] : uq[zp + (size_t)j * nx + x];
                grad[q][2] = fd_diff(zl, zh, (int)pz_lo + (int)pz_hi) * rhz;
            }
            um[q] = uc[q];
            uc[q] = up[q];      // (a boundary value only behind the last row: never read as a centre)
        }
        fd_emit<R, DIMS, KIND>(grad, o + row + x, n);
    }
}

// Multi-block: one thread per (cell, env).
template <typename R, int DIMS, int KIND>
__global__ __launch_bounds__(FG_BLOCK) void k_mb_flow_diag(int N, int NB, const int32_t* __restrict__ nbr, const R* __restrict__ T,
                                                            const R* __restrict__ vel, const R* __restrict__ bvel, R* __restrict__ out) {
    constexpr int K = fd_channels(DIMS, KIND);
    const int i = blockIdx.x * FG_BLOCK + threadIdx.x, b = blockIdx.y;
    if (i >= N) return;
    R mi[DIMS * DIMS];      // Minv, row major
#pragma unroll
    for (int k = 0; k < DIMS * DIMS; ++k) mi[k] = T[(size_t)i * (DIMS * DIMS + 1) + k];
    const R* __restrict__ u = vel + (size_t)b * DIMS * N;
    const R* __restrict__ ub = bvel + (size_t)b * DIMS * NB;
    R c[DIMS][DIMS];        // [component][computational axis]
#pragma unroll
    for (int a = 0; a < DIMS; ++a) {
        const int nl = nbr[(size_t)(2 * a) * N + i], nh = nbr[(size_t)(2 * a + 1) * N + i];
        const int prescribed = (int)(nl < 0) + (int)(nh < 0);
#pragma unroll
        for (int q = 0; q < DIMS; ++q) {
            const R lo = nl >= 0 ? u[(size_t)q * N + nl] : ub[(size_t)q * NB + (-1 - nl)];
            const R hi = nh >= 0 ? u[(size_t)q * N + nh] : ub[(size_t)q * NB + (-1 - nh)];
            c[q][a] = fd_diff(lo, hi, prescribed);
        }
    }
    R grad[DIMS][DIMS];
#pragma unroll
    for (int q = 0; q < DIMS; ++q)
#pragma unroll
        for (int j = 0; j < DIMS; ++j) {
            R s = c[q][0] * mi[j];
#pragma unroll
            for (int a = 1; a < DIMS; ++a) s += c[q][a] * mi[a * DIMS + j];
            grad[q][j] = s;
        }
    fd_emit<R, DIMS, KIND>(grad, out + (size_t)b * K * N + i, (size_t)N);
}

// kind -> template instance; the body sees constexpr KIND
#define FD_DISPATCH_KIND(kind, ...)                                                               \
    switch (kind) {                                                                               \
        case FG_DIAG_GRADIENT: { constexpr int KIND = FG_DIAG_GRADIENT; __VA_ARGS__; } break;     \
        case FG_DIAG_VORTICITY: { constexpr int KIND = FG_DIAG_VORTICITY; __VA_ARGS__; } break;   \
        case FG_DIAG_VORTICITY_MAGNITUDE: { constexpr int KIND = FG_DIAG_VORTICITY_MAGNITUDE; __VA_ARGS__; } break; \
        case FG_DIAG_Q: { constexpr int KIND = FG_DIAG_Q; __VA_ARGS__; } break;                   \
        default: { constexpr int KIND = FG_DIAG_STRAIN_NORM; __VA_ARGS__; } break;                \
    }

inline bool fd_kind_ok(int kind) { return kind >= FG_DIAG_GRADIENT && kind <= FG_DIAG_STRAIN_NORM; }

}  // namespace

extern "C" int fg_flow_diagnostic(fg_handle s, int kind, fg_real* out, void* stream) {
    FG_REQUIRE(s && out, FG_ERR_INVALID_ARG, "fg_flow_diagnostic: null handle or out");
    FG_REQUIRE(fd_kind_ok(kind), FG_ERR_INVALID_ARG, "fg_flow_diagnostic: unknown kind (FG_DIAG_*)");
    FG_REQUIRE(s->velocity, FG_ERR_NOT_BOUND, "fg_flow_diagnostic: velocity not bound (fg_bind)");
    const FgGrid& g = s->grid;
    FgBounds bnd = {};
    for (int f = 0; f < 2 * g.dims; ++f) {
        FG_REQUIRE(!g.fixed[f] || s->bvel[f], FG_ERR_NOT_BOUND, "fg_flow_diagnostic: boundary velocity of a FIXED face not bound");
        bnd.vel[f] = s->bvel[f];
    }
    const int tiles_x = (g.nx + 63) / 64, chunks_y = (g.ny + FD_ROWS - 1) / FD_ROWS;
    const int groups = (chunks_y * (g.dims == 3 ? g.nz : 1) + 3) / 4;
    const long long blocks = (long long)tiles_x * groups * g.B;
    FG_REQUIRE(blocks <= 0x7fffffffLL, FG_ERR_UNSUPPORTED, "fg_flow_diagnostic: the launch exceeds 2^31 - 1 workgroups");
    const dim3 grid((unsigned)blocks);
    hipStream_t st = (hipStream_t)stream;
    FD_DISPATCH_KIND(kind, {
        if (g.dims == 2) hipLaunchKernelGGL((k_flow_diag<fg_real, 2, KIND>), grid, dim3(FG_BLOCK), 0, st, g, bnd, (const fg_real*)s->velocity, out, tiles_x, chunks_y, groups);
        else hipLaunchKernelGGL((k_flow_diag<fg_real, 3, KIND>), grid, dim3(FG_BLOCK), 0, st, g, bnd, (const fg_real*)s->velocity, out, tiles_x, chunks_y, groups);
    });
    FG_HIP_CHECK(hipGetLastError());
    return FG_OK;
}

extern "C" int fg_mb_flow_diagnostic(fg_mb_handle s, int kind, fg_real* out, void* stream) {
    FG_REQUIRE(s && out, FG_ERR_INVALID_ARG, "fg_mb_flow_diagnostic: null handle or out");
    FG_REQUIRE(fd_kind_ok(kind), FG_ERR_INVALID_ARG, "fg_mb_flow_diagnostic: unknown kind (FG_DIAG_*)");
    FG_REQUIRE(!s->host_only, FG_ERR_UNSUPPORTED, "fg_mb_flow_diagnostic: host-only handle");
    FG_REQUIRE(s->finalized && s->velocity && s->bvel, FG_ERR_NOT_BOUND, "fg_mb_flow_diagnostic: fields not bound");
    FG_REQUIRE(s->B <= 65535, FG_ERR_UNSUPPORTED, "fg_mb_flow_diagnostic: more than 65535 envs");
    const dim3 grid((unsigned)((s->N + FG_BLOCK - 1) / FG_BLOCK), (unsigned)s->B);
    hipStream_t st = (hipStream_t)stream;
    const MbDev& D = s->dev;
    FD_DISPATCH_KIND(kind, {
        if (s->d == 2) hipLaunchKernelGGL((k_mb_flow_diag<mb_real, 2, KIND>), grid, dim3(FG_BLOCK), 0, st, D.N, D.NB, D.nbr, D.T, (const mb_real*)s->velocity, (const mb_real*)s->bvel, (mb_real*)out);
        else hipLaunchKernelGGL((k_mb_flow_diag<mb_real, 3, KIND>), grid, dim3(FG_BLOCK), 0, st, D.N, D.NB, D.nbr, D.T, (const mb_real*)s->velocity, (const mb_real*)s->bvel, (mb_real*)out);
    });
    FG_HIP_CHECK(hipGetLastError());
    return FG_OK;
}
