// Wall distributions of the multi-block domains (WallRing.distribution / WallMoments, envs/forces.py, simulation/wall_stats.py): per
// face of a closed wall the integrand of fg_mb_wall_forces -- the wall-adjacent pressure, the traction (2 nu S - p I) n and its
// viscous part along the ring tangent t = (ny, -nx), the wall shear stress -- and the online mean and central sums of those four
// channels, merged over the samples of a run on the device.
//
// The reference has the sum only (compute_forces_2d / _3d, envs/util/forces.py:193-377); the curves Cp(s), Cf(s) and their time
// statistics are what its users build from tensor indexing afterwards.  Here one sample of a batch of B envs is ONE launch over the
// flat fields velocity [B, d, N], boundary_velocity [B, d, NB], pressure [B, N] as MultiBlockDomain holds them, gathered through the
// ring's index tables:
//   ws_face      the arithmetic of k_mb_wall_forces (fg_mb_step.hip) for face (b, layer, j) without the face length: the one-sided
//                normal derivative (cell - wall) / distance, the central tangential derivative over the ring's neighbours
//                cl = ci[j + 1 mod n], cr = ci[j - 1 mod n], the four composed gradients, sxy, two_nu -> p, tau_w, fx, fy in fg_real
//   distribution one thread per face, consecutive lanes consecutive j: the stores of every channel plane coalesce
//   moments      one thread per record -- face j over all layers (span_average, n_B = layers) or one face (n_B = 1): pass 1 the
//                sums of the four channels in ascending layer order, fp64 -> the sample's mean; pass 2 the same faces again, the
//                sums of d_i d_j (i <= j), fp64; merge with mean [B][4][R], central [B][10][R] by the order-2 rule of fg_rowstat.h,
//                n_A = samples * n_B; the first sample (samples = 0) is stored.  `samples` is a kernel argument: the host counts.
//
// No floating-point atomic, no cross-lane operation, no device counter: a face's and a record's result depend on their own cells and
// `samples` only.  This file is compiled with -ffp-contract=off (its own rule in the Makefile): every product, sum and division is
// rounded on its own, so any batch, any launch and both kernels give the same bits, and they are the bits of the NumPy twin
// (sample_wall_faces).  A ring has 30-400 faces: these are gather kernels whose cost is the launch; nothing is staged in LDS.
// An index outside its field is never dereferenced: the face's four channels are NaN.
#include <math.h>

#include "fg_rowstat.h"

namespace {

namespace rs = fg_rowstat;

constexpr int WS_K = 4;                          // p, tau_w, fx, fy
constexpr int WS_P = WS_K * (WS_K + 1) / 2;

struct WsArgs {
    const fg_real* u;                            // [B][d][N]
    const fg_real* ub;                           // [B][d][NB]
    const fg_real* p;                            // [B][N]
    const int32_t* ci;                           // [layers][n]
    const int32_t* si;                           // [layers][n]
    const fg_real* geom;                         // [5][n]
    const fg_real* nu_B;                         // [B] or nullptr
    fg_real nu;
    long long N, NB;
    int d, n, layers;
};

// the four channels of wall face (b, layer, j)
__device__ __forceinline__ void ws_face(const WsArgs& a, int b, int layer, int j, fg_real (&ch)[WS_K]) {
    const int n = a.n;
    const int32_t* ci = a.ci + (size_t)layer * n;
    const int c0 = ci[j], cl0 = ci[j + 1 == n ? 0 : j + 1], cr0 = ci[j == 0 ? n - 1 : j - 1], sl0 = a.si[(size_t)layer * n + j];
    const bool inside = (unsigned long long)c0 < (unsigned long long)a.N && (unsigned long long)cl0 < (unsigned long long)a.N &&
                        (unsigned long long)cr0 < (unsigned long long)a.N && (unsigned long long)sl0 < (unsigned long long)a.NB;
    // an index outside its field: the face reads element 0 instead (n_cells, n_slots > 0) and is NaN in the end; no branch
    const int c = inside ? c0 : 0, cl = inside ? cl0 : 0, cr = inside ? cr0 : 0, sl = inside ? sl0 : 0;
    const fg_real* ue = a.u + (size_t)b * a.d * a.N;
    const fg_real* ube = a.ub + (size_t)b * a.d * a.NB;
    const fg_real nu = a.nu_B ? a.nu_B[b] : a.nu;
    const fg_real nx = a.geom[j], ny = a.geom[(size_t)n + j], tl = a.geom[2 * (size_t)n + j], wd = a.geom[3 * (size_t)n + j];
    const fg_real tx = ny, ty = -nx;
    const fg_real* ve = ue + a.N;
    const fg_real dn0 = (ue[c] - ube[sl]) / wd, dn1 = (ve[c] - ube[(size_t)a.NB + sl]) / wd;
    const fg_real dt0 = (ue[cr] - ue[cl]) / ((fg_real)2 * tl), dt1 = (ve[cr] - ve[cl]) / ((fg_real)2 * tl);
    const fg_real du_dx = dn0 * nx + dt0 * tx, du_dy = dn0 * ny + dt0 * ty;
    const fg_real dv_dx = dn1 * nx + dt1 * tx, dv_dy = dn1 * ny + dt1 * ty;
    const fg_real sxy = (fg_real)0.5 * (du_dy + dv_dx), two_nu = (fg_real)2 * nu, pc = a.p[(size_t)b * a.N + c];
    const fg_real fx = (two_nu * du_dx - pc) * nx + two_nu * sxy * ny;
    const fg_real fy = two_nu * sxy * nx + (two_nu * dv_dy - pc) * ny;
    const fg_real tau = (two_nu * du_dx * nx + two_nu * sxy * ny) * ny - (two_nu * sxy * nx + two_nu * dv_dy * ny) * nx;
    const fg_real nan = (fg_real)NAN;
    ch[0] = inside ? pc : nan; ch[1] = inside ? tau : nan; ch[2] = inside ? fx : nan; ch[3] = inside ? fy : nan;
}

__global__ __launch_bounds__(FG_BLOCK) void k_mb_wall_distribution(WsArgs a, fg_real* __restrict__ out) {
    const long long faces = (long long)a.layers * a.n;
    const long long i = (long long)blockIdx.x * FG_BLOCK + threadIdx.x;
    if (i >= faces) return;
    const int b = blockIdx.y, layer = (int)(i / a.n), j = (int)(i - (long long)layer * a.n);
    fg_real ch[WS_K];
    ws_face(a, b, layer, j, ch);
    fg_real* o = out + (size_t)b * WS_K * faces + i;
#pragma unroll
    for (int k = 0; k < WS_K; ++k) o[(size_t)k * faces] = ch[k];
}

// SPAN: a record is face j over all layers; otherwise one face
template <bool SPAN>
__global__ __launch_bounds__(FG_BLOCK) void k_mb_wall_moments(WsArgs a, long long samples, double* __restrict__ mean,
                                                               double* __restrict__ central) {
    const long long R = SPAN ? (long long)a.n : (long long)a.layers * a.n;
    const long long r = (long long)blockIdx.x * FG_BLOCK + threadIdx.x;
    if (r >= R) return;
    const int b = blockIdx.y;
    const int layer0 = SPAN ? 0 : (int)(r / a.n), j = (int)(r - (long long)layer0 * a.n), nl = SPAN ? a.layers : 1;

    double mu[WS_K];
#pragma unroll
    for (int k = 0; k < WS_K; ++k) mu[k] = 0.0;
    for (int l = 0; l < nl; ++l) {
        fg_real ch[WS_K];
        ws_face(a, b, layer0 + l, j, ch);
#pragma unroll
        for (int k = 0; k < WS_K; ++k) mu[k] += (double)ch[k];
    }
    const double nB = (double)nl;
#pragma unroll
    for (int k = 0; k < WS_K; ++k) mu[k] = mu[k] / nB;

    double c[WS_P];
#pragma unroll
    for (int q = 0; q < WS_P; ++q) c[q] = 0.0;
    for (int l = 0; l < nl; ++l) {
        fg_real ch[WS_K];
        ws_face(a, b, layer0 + l, j, ch);
        double d[WS_K];
#pragma unroll
        for (int k = 0; k < WS_K; ++k) d[k] = (double)ch[k] - mu[k];
        int q = 0;
#pragma unroll
        for (int i1 = 0; i1 < WS_K; ++i1) {
#pragma unroll
            for (int i2 = i1; i2 < WS_K; ++i2) {
                c[q] += d[i1] * d[i2];
                ++q;
            }
        }
    }

    // ---- merge: A = the running record, B = this sample, delta = mean_B - mean_A
    double* gm = mean + (size_t)b * WS_K * R + r;
    double* gc = central + (size_t)b * WS_P * R + r;
    if (samples == 0) {
#pragma unroll
        for (int k = 0; k < WS_K; ++k) gm[(size_t)k * R] = mu[k];
#pragma unroll
        for (int q = 0; q < WS_P; ++q) gc[(size_t)q * R] = c[q];
        return;
    }
    const double nA = (double)samples * nB, nn = nA + nB, w2 = nA * nB / nn;
    double dl[WS_K];
#pragma unroll
    for (int k = 0; k < WS_K; ++k) {
        const double mA = gm[(size_t)k * R];
        dl[k] = mu[k] - mA;
        gm[(size_t)k * R] = (nA * mA + nB * mu[k]) / nn;
    }
    int q = 0;
#pragma unroll
    for (int i1 = 0; i1 < WS_K; ++i1) {
#pragma unroll
        for (int i2 = i1; i2 < WS_K; ++i2) {
            gc[(size_t)q * R] = rs::merge2(gc[(size_t)q * R], c[q], dl[i1], dl[i2], w2);
            ++q;
        }
    }
}

// the checks both entries share, and the arguments both kernels take
int ws_plan(WsArgs& a, const std::string& e, const fg_real* velocity, const fg_real* boundary_velocity, const fg_real* pressure, int dims,
            int batch, long long n_cells, long long n_slots, const int32_t* cell_index, const int32_t* slot_index, const fg_real* geom, int n,
            int layers, fg_real viscosity, const fg_real* viscosity_B) {
    FG_REQUIRE(velocity && boundary_velocity && pressure, FG_ERR_INVALID_ARG, e + ": null velocity, boundary velocity or pressure");
    FG_REQUIRE(cell_index && slot_index && geom, FG_ERR_INVALID_ARG, e + ": null index table or geometry");
    FG_REQUIRE(dims == 2 || dims == 3, FG_ERR_INVALID_ARG, e + ": dims must be 2 or 3");
    FG_REQUIRE(batch > 0 && batch <= 65535, FG_ERR_INVALID_ARG, e + ": batch must be 1..65535");
    FG_REQUIRE(n > 0 && layers > 0, FG_ERR_INVALID_ARG, e + ": n and layers must be positive");
    FG_REQUIRE(n_cells > 0 && n_cells <= 0x7fffffffLL && n_slots > 0 && n_slots <= 0x7fffffffLL, FG_ERR_INVALID_ARG,
               e + ": n_cells and n_slots must be 1..2^31 - 1");
    FG_REQUIRE((long long)n * layers <= 0x7fffffffLL, FG_ERR_INVALID_ARG, e + ": more than 2^31 - 1 faces");
    a.u = velocity; a.ub = boundary_velocity; a.p = pressure; a.ci = cell_index; a.si = slot_index; a.geom = geom;
    a.nu_B = viscosity_B; a.nu = viscosity; a.N = n_cells; a.NB = n_slots; a.d = dims; a.n = n; a.layers = layers;
    return FG_OK;
}

}  // namespace

extern "C" int fg_mb_wall_distribution(const fg_real* velocity, const fg_real* boundary_velocity, const fg_real* pressure, int32_t dims,
                                       int32_t batch, int64_t n_cells, int64_t n_slots, const int32_t* cell_index,
                                       const int32_t* slot_index, const fg_real* geom, int32_t n, int32_t layers, fg_real viscosity,
                                       const fg_real* viscosity_B, fg_real* out, void* stream) {
    WsArgs a;
    const int rc = ws_plan(a, "fg_mb_wall_distribution", velocity, boundary_velocity, pressure, dims, batch, n_cells, n_slots, cell_index,
                           slot_index, geom, n, layers, viscosity, viscosity_B);
    if (rc != FG_OK) return rc;
    FG_REQUIRE(out, FG_ERR_INVALID_ARG, "fg_mb_wall_distribution: null out");
    const long long faces = (long long)n * layers;
    const dim3 grid((unsigned)((faces + FG_BLOCK - 1) / FG_BLOCK), (unsigned)batch);
    hipLaunchKernelGGL(k_mb_wall_distribution, grid, dim3(FG_BLOCK), 0, (hipStream_t)stream, a, out);
    FG_HIP_CHECK(hipGetLastError());
    return FG_OK;
}

extern "C" int fg_mb_wall_moments(const fg_real* velocity, const fg_real* boundary_velocity, const fg_real* pressure, int32_t dims,
                                  int32_t batch, int64_t n_cells, int64_t n_slots, const int32_t* cell_index, const int32_t* slot_index,
                                  const fg_real* geom, int32_t n, int32_t layers, fg_real viscosity, const fg_real* viscosity_B,
                                  int32_t span_average, int64_t samples, double* mean, double* central, void* stream) {
    WsArgs a;
    const int rc = ws_plan(a, "fg_mb_wall_moments", velocity, boundary_velocity, pressure, dims, batch, n_cells, n_slots, cell_index,
                           slot_index, geom, n, layers, viscosity, viscosity_B);
    if (rc != FG_OK) return rc;
    FG_REQUIRE(mean && central, FG_ERR_INVALID_ARG, "fg_mb_wall_moments: null accumulator (mean, central)");
    FG_REQUIRE(samples >= 0 && samples < (1LL << 40), FG_ERR_INVALID_ARG, "fg_mb_wall_moments: samples must be 0..2^40 - 1");
    const long long R = span_average ? (long long)n : (long long)n * layers;
    const dim3 grid((unsigned)((R + FG_BLOCK - 1) / FG_BLOCK), (unsigned)batch);
    hipStream_t st = (hipStream_t)stream;
    if (span_average) hipLaunchKernelGGL((k_mb_wall_moments<true>), grid, dim3(FG_BLOCK), 0, st, a, (long long)samples, mean, central);
    else hipLaunchKernelGGL((k_mb_wall_moments<false>), grid, dim3(FG_BLOCK), 0, st, a, (long long)samples, mean, central);
    FG_HIP_CHECK(hipGetLastError());
    return FG_OK;
}
